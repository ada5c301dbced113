"""SegNet's training-input pipeline on the CPU (ppnet_amd/augment.py): the definition restated in tests/_augment_ref.py gives the hand
values of DESIGN.md §18; augment.apply on the CPU equals it bit for bit under all 64 flag combinations, on a palette image and on the
17-level colour lattice; draw_params equals the oracle's Philox draws slot by slot; the drawn flags and values have the reference's
distributions; and train.segnet_train_step takes augment=."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _augment_ref as R  # noqa: E402


def test_hand_values_of_the_definition():
    # the palette in HSV: white, red, black (as BGR)
    assert R.bgr2hsv_px(255, 255, 255) == (0, 0, 255)
    assert R.bgr2hsv_px(0, 0, 255) == (0, 255, 255)
    assert R.bgr2hsv_px(0, 0, 0) == (0, 0, 0)
    red = np.array([[[0, 0, 255]]], dtype=np.uint8)
    assert R.photometric(red.copy(), R.HUE, 0, 1, 1, -18).tolist() == [[[153, 0, 255]]]
    assert R.photometric(red.copy(), R.SATURATION, 0, 1, 0.5, 0).tolist() == [[[128, 128, 255]]]
    for v in range(256):                                                      # greys are fixed points of the round trip
        assert R.hsv2bgr_px(*R.bgr2hsv_px(v, v, v)) == (v, v, v)
    lat = R.lattice_colours()
    assert lat.shape == (4913, 3)
    back = np.array([R.hsv2bgr_px(*R.bgr2hsv_px(*(int(c) for c in col))) for col in lat])
    diff = np.abs(back - lat.astype(int))
    assert int((diff.max(axis=1) > 0).sum()) == 2262 and int(diff.max()) == 4
    # "on with alpha = 1" is not "off": the round trip itself is lossy
    img = lat.reshape(17, 289, 3)
    assert not np.array_equal(R.photometric(img.copy(), R.SATURATION, 0, 1, 1.0, 0), img)
    assert np.array_equal(R.photometric(img.copy(), 0, 5, 0.7, 0.7, 9), img)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_cpu_apply_equals_the_definition_under_all_flag_combinations(dtype):
    from ppnet_amd import augment
    rows = R.param_rows()
    params = torch.from_numpy(R.words(rows))
    aug = augment.SegAugment(out_size=(16, 24))
    codes = R.palette_codes(64, 8, 16)
    labels = np.random.RandomState(1).randint(0, 2, (64, 8, 16)).astype(np.uint8)
    want_img, want_lab = R.batch(codes, labels, rows, (16, 24))
    img, lab = augment.apply(aug, params, torch.from_numpy(codes), torch.from_numpy(labels), R.MEAN, R.STD, dtype)
    assert img.shape == (64, 3, 16, 24) and img.dtype == dtype and lab.dtype == torch.uint8
    assert torch.equal(img.permute(0, 2, 3, 1), torch.from_numpy(want_img).to(dtype))
    assert np.array_equal(lab.numpy(), want_lab)
    # the lattice as RGB images, one flag combination each: 4913 colours in 17 x 296 (23 spare pixels black)
    lat = np.zeros((17 * 296, 3), dtype=np.uint8)
    lat[:4913] = R.lattice_colours()
    rgb = np.broadcast_to(lat.reshape(1, 17, 296, 3), (64, 17, 296, 3)).copy()
    want_img, _ = R.batch(rgb, None, rows)
    img, lab = augment.apply(augment.SegAugment(), params, torch.from_numpy(rgb), None, R.MEAN, R.STD, dtype)
    assert lab is None and torch.equal(img.permute(0, 2, 3, 1), torch.from_numpy(want_img).to(dtype))
    # codes mode = RGB mode on the rendered palette image
    rendered = np.stack([R.render(c)[:, :, ::-1] for c in codes])
    a, _ = augment.apply(aug, params, torch.from_numpy(codes), None, R.MEAN, R.STD, dtype)
    b, _ = augment.apply(aug, params, torch.from_numpy(rendered.copy()), None, R.MEAN, R.STD, dtype)
    assert torch.equal(a, b)


def test_draw_params_equals_the_oracle_draws():
    from ppnet_amd import augment, philox
    from oracle import philox_np
    aug = augment.SegAugment(seed=R.SEED)
    for first in (0, 5, 2 ** 32 + 3, 2 ** 40 + 12345):
        got = augment.draw_params(aug, first, 6, "cpu")
        assert got.dtype == torch.int32 and got.shape == (6, 8)
        assert np.array_equal(got.numpy(), R.words([R.drawn(R.SEED, first + b) for b in range(6)])), first
        assert np.array_equal(philox.doubles_host(R.SEED, 5, first, 0, 10), philox_np.doubles(R.SEED, 5, first, 0, 10))
    # other settings scale the same draws
    aug2 = augment.SegAugment(seed=R.SEED, flip_ratio=0.25, brightness_delta=10.0, contrast_range=(0.8, 1.2), saturation_range=(0.25, 2.0), hue_delta=9)
    want = R.words([R.drawn(R.SEED, 7 + b, 0.25, 10.0, (0.8, 1.2), (0.25, 2.0), 9) for b in range(4)])
    assert np.array_equal(augment.draw_params(aug2, 7, 4, "cpu").numpy(), want)


def test_draw_statistics():
    rows = [R.drawn(R.SEED, i) for i in range(4096)]
    flags = np.array([r[0] for r in rows])
    for bit in (R.FLIP, R.BRIGHTNESS, R.CONTRAST, R.CONTRAST_LAST, R.SATURATION, R.HUE):
        freq = float(((flags & bit) != 0).mean())
        assert 0.45 <= freq <= 0.55, (bit, freq)                              # six standard deviations of a fair coin over 4096
    beta, alpha, alpha_s, delta = (np.array([r[k] for r in rows]) for k in (1, 2, 3, 4))
    assert set(delta.tolist()) == set(range(-18, 18))
    assert beta.min() >= -32 and beta.max() < 32 and beta.dtype == np.float32
    for a in (alpha, alpha_s):
        assert a.min() >= 0.5 and a.max() < 1.5 and a.dtype == np.float32
    # and the product's CPU draws are these
    from ppnet_amd import augment
    assert np.array_equal(augment.draw_params(augment.SegAugment(seed=R.SEED), 0, 64, "cpu").numpy(), R.words(rows[:64]))


TINY = dict(backbone=dict(embed_dim=16, mlp_ratio=2.0, depths=[1, 1, 1, 1], num_heads=[1, 1, 2, 4], kernel_size=7, layer_scale=1e-5,
                          drop_path_rate=0.0),
            decode_head=dict(in_channels=128, channels=16, num_convs=2, up_scale=2, num_classes=2, dropout_ratio=0.0))


def _cpu_step(monkeypatch, **kw):
    """One SGD step of a tiny SegNet on the CPU: (loss, first parameter afterwards).  The neighbourhood attention and the palette
    image, GPU-only in the product, are the float64 / NumPy definitions here."""
    from oracle import segnet_ref as SR
    from ppnet_amd import fused, na, train
    from ppnet_amd.segnet import SegNet

    def na_forward(self, x, real_hw=None):
        return SR.na_fp64(x.double(), self.qkv.weight.double(), self.qkv.bias.double(), self.rpb.double(), self.proj.weight.double(),
                          self.proj.bias.double(), self.num_heads, 7, self.dilation).to(x.dtype)

    def grid_to_image(grid, mean, std, dtype):
        img, _ = R.batch(grid.numpy(), None, [(0, 0, 1, 1, 0)] * grid.shape[0])
        return torch.from_numpy(img).to(dtype).permute(0, 3, 1, 2)
    monkeypatch.setattr(na.NeighborhoodAttention2D, "forward", na_forward)
    monkeypatch.setattr(fused, "grid_to_image", grid_to_image)
    torch.manual_seed(0)
    net = SegNet(**TINY)
    trainer = train.segnet_trainer(net)
    opt = train.segnet_optimizer(trainer, lr=0.01)
    codes = torch.from_numpy(R.palette_codes(2, 32, 32, seed=3))
    labels = torch.from_numpy(np.random.RandomState(4).randint(0, 2, (2, 32, 32)).astype(np.uint8))
    loss = train.segnet_train_step(trainer, opt, 3, 10, codes, labels, schedule=dict(warmup_iters=0), **kw)
    return float(loss), next(net.parameters()).detach().clone()


def test_cpu_training_step_with_augment(monkeypatch):
    from ppnet_amd import augment
    plain, p_plain = _cpu_step(monkeypatch)
    none, p_none = _cpu_step(monkeypatch, augment=None)
    assert plain == none and torch.equal(p_plain, p_none)
    aug = augment.SegAugment(seed=R.SEED, out_size=(40, 48))
    a, p_a = _cpu_step(monkeypatch, augment=aug)
    b, p_b = _cpu_step(monkeypatch, augment=aug)
    assert np.isfinite(a) and a == b and torch.equal(p_a, p_b)
    assert a != plain
