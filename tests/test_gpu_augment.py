"""ppn_augment_params / ppn_augment_codes / ppn_augment_rgb (csrc/augment.hip) on the GPU, float32 and bfloat16 outputs.

Reference: the definition restated in tests/_augment_ref.py (the reference's PhotoMetricDistortion control flow, the project's integer
HSV), computed once per module on the CPU.  Every comparison is bit for bit: the definition is integer and single float32 operations,
so there is no tolerance to choose; a bfloat16 output is the float32 one rounded to nearest even."""
import copy
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _augment_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.bfloat16]
IDS = {torch.float32: "f32", torch.bfloat16: "bf16"}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nhwc(img):
    return img.permute(0, 2, 3, 1).cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_flags_zero_is_grid_to_image(dtype):
    from ppnet_amd import fused
    codes = torch.from_numpy(np.random.RandomState(5).randint(0, 256, (6, 8, 16)).astype(np.uint8))
    codes[0, 0, :4] = torch.tensor([0, 128, 255, 127], dtype=torch.uint8)
    params = torch.zeros(6, 8, dtype=torch.int32, device=DEV)
    want = fused.grid_to_image(codes.to(DEV), R.MEAN, R.STD, dtype)
    got, lab = fused.augment_codes(codes.to(DEV), None, params, R.MEAN, R.STD, dtype)
    assert lab is None and got.shape == want.shape == (6, 3, 8, 16) and got.stride() == want.stride()
    assert torch.equal(got, want)


@functools.lru_cache(maxsize=None)
def _flag_case():
    rows = R.param_rows()
    codes = R.palette_codes(64, 8, 16)
    labels = np.random.RandomState(1).randint(0, 2, (64, 8, 16)).astype(np.uint8)
    return rows, codes, labels, R.batch(codes, labels, rows)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_all_flag_combinations_on_codes(dtype):
    from ppnet_amd import fused
    rows, codes, labels, (want_img, want_lab) = _flag_case()
    assert sorted(r[0] for r in rows) == list(range(64))
    params = _dev(R.words(rows))
    img, lab = fused.augment_codes(_dev(codes), _dev(labels), params, R.MEAN, R.STD, dtype)
    assert torch.equal(_nhwc(img), torch.from_numpy(want_img).to(dtype))
    assert np.array_equal(lab.cpu().numpy(), want_lab)
    # the codes mode is the RGB mode on the rendered palette image
    rendered = np.stack([R.render(c)[:, :, ::-1] for c in codes])
    img2, lab2 = fused.augment_rgb(_dev(rendered), _dev(labels), params, R.MEAN, R.STD, dtype)
    assert torch.equal(img, img2) and torch.equal(lab, lab2)


LATTICE_ROWS = [(0, 0.0, 1.0, 1.0, 0),
                (R.BRIGHTNESS | R.CONTRAST, 32.0, 1.5, 1.0, 0),
                (R.SATURATION, 0.0, 1.0, 0.5, 0),
                (R.SATURATION, 0.0, 1.0, 1.5, 0),
                (R.HUE | R.FLIP, 0.0, 1.0, 1.0, -18),
                (R.HUE, 0.0, 1.0, 1.0, 17),
                (R.BRIGHTNESS | R.CONTRAST | R.CONTRAST_LAST | R.SATURATION | R.HUE, -32.0, 0.5, 0.77, 5),
                (R.FLIP | R.BRIGHTNESS | R.CONTRAST | R.SATURATION | R.HUE, 11.25, 0.77, 1.23, -7)]


@functools.lru_cache(maxsize=None)
def _lattice_case():
    """RGB images [4, 64, 80, 3], each holding the 4913 lattice colours and 207 random pixels; two batches of four parameter sets."""
    g = np.random.RandomState(9)
    rgb = g.randint(0, 256, (4, 64, 80, 3)).astype(np.uint8)
    rgb.reshape(4, -1, 3)[:, :4913] = R.lattice_colours()
    labels = g.randint(0, 3, (4, 64, 80)).astype(np.uint8)
    want = [R.batch(rgb, labels, LATTICE_ROWS[k:k + 4]) for k in (0, 4)]
    return rgb, labels, want


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_rgb_mode_on_the_colour_lattice(dtype):
    from ppnet_amd import fused
    rgb, labels, want = _lattice_case()
    for k, (want_img, want_lab) in zip((0, 4), want):
        img, lab = fused.augment_rgb(_dev(rgb), _dev(labels), _dev(R.words(LATTICE_ROWS[k:k + 4])), R.MEAN, R.STD, dtype)
        assert torch.equal(_nhwc(img), torch.from_numpy(want_img).to(dtype)), k
        assert np.array_equal(lab.cpu().numpy(), want_lab), k


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("mode", ["codes", "rgb"])
def test_flip_and_pad_overwrite_every_output(mode, dtype):
    """[3, 8, 16] -> 16 x 24 through the raw entry points on outputs pre-filled with NaN and 7, with and without labels."""
    import ctypes as C
    from ppnet_amd import _lib
    B, H, W, Ho, Wo = 3, 8, 16, 16, 24
    rows = [(R.FLIP, 0.0, 1.0, 1.0, 0), (0, 0.0, 1.0, 1.0, 0), (R.FLIP | R.BRIGHTNESS | R.HUE, -20.0, 1.0, 1.0, 9)]
    codes = R.palette_codes(B, H, W, seed=2)
    src = codes if mode == "codes" else np.stack([R.render(c)[:, :, ::-1] for c in codes])
    labels = np.random.RandomState(3).randint(0, 200, (B, H, W)).astype(np.uint8)
    want_img, want_lab = R.batch(src, labels, rows, (Ho, Wo))
    entry = _lib.lib.ppn_augment_codes if mode == "codes" else _lib.lib.ppn_augment_rgb
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    m3, s3 = (C.c_float * 3)(*R.MEAN), (C.c_float * 3)(*R.STD)
    srcd, labd, params = _dev(src), _dev(labels), _dev(R.words(rows))
    for with_labels in (True, False):
        img = torch.full((B, Ho, Wo, 3), float("nan"), dtype=dtype, device=DEV)
        lab = torch.full((B, Ho, Wo), 7, dtype=torch.uint8, device=DEV)
        rc = entry(p(srcd), p(labd) if with_labels else None, p(params), p(img), p(lab) if with_labels else None, B, H, W, Ho, Wo, m3, s3, 255,
                   {torch.float32: 0, torch.bfloat16: 1}[dtype], C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
        assert rc == 0, rc
        torch.cuda.synchronize()
        got = img.cpu()
        assert not bool(torch.isnan(got.float()).any())
        assert torch.equal(got, torch.from_numpy(want_img).to(dtype))
        assert bool((got[:, H:] == 0).all()) and bool((got[:, :, W:] == 0).all())
        l = lab.cpu().numpy()
        if not with_labels:
            assert (l == 7).all()                                          # label_in = NULL: no label is touched
            continue
        assert np.array_equal(l, want_lab)
        assert (l[:, H:] == 255).all() and (l[:, :, W:] == 255).all()
        for b, row in enumerate(rows):
            inside = l[b, :H, :W]
            assert np.array_equal(inside, labels[b][:, ::-1] if row[0] & R.FLIP else labels[b])


def test_device_draws_equal_the_cpu_draws():
    from ppnet_amd import augment
    for aug in (augment.SegAugment(seed=R.SEED),
                augment.SegAugment(seed=2 ** 63 + 11, flip_ratio=0.25, brightness_delta=10.0, contrast_range=(0.8, 1.2), saturation_range=(0.25, 2.0),
                                   hue_delta=9)):
        for first, B in ((0, 300), (2 ** 32 - 2, 5), (2 ** 40 + 12345, 3)):
            got = augment.draw_params(aug, first, B, DEV)
            assert got.dtype == torch.int32 and got.shape == (B, 8)
            assert torch.equal(got.cpu(), augment.draw_params(aug, first, B, "cpu")), (first, B)
    assert np.array_equal(augment.draw_params(augment.SegAugment(seed=R.SEED), 0, 16, DEV).cpu().numpy(), R.words([R.drawn(R.SEED, i) for i in range(16)]))


def test_tiny_dinat_training_step_with_augment():
    """tests/test_gpu_resize_ce.py's tiny DiNAT + SETR-UP + auxiliary head: a step on augmented input is finite; the same (seed, it)
    feeds the network bit-identical images and labels — those of augment.apply at first_instance = it * B — and gives a bit-identical
    loss from the same weights; another `it` gives other inputs and another loss; out_size larger than the map trains through the
    ignore-255 path.

    The loss comparison depends on the network as well as on its input.  Measured on an MI355X with identical input tensors and
    weights: the tiny network's backbone features differed in some bits in 4 of 6 repeats and the decode head's logits on identical
    features in 9 of 11 (library convolutions and GEMMs in training mode; ppn_resize_ce_fwd on identical logits repeated exactly, and
    so do the kernels tested above), which moved the float32 loss by one ulp in 3 of 22 repeated steps.  The input assertions come
    first, so a failure of the loss assertion alone is that library effect."""
    from ppnet_amd import augment, train
    from ppnet_amd.segnet import IMG_MEAN, IMG_STD, SegNet, randomize_neutral_parameters
    torch.manual_seed(2)
    net0 = randomize_neutral_parameters(SegNet(**R.TINY_SEG, auxiliary_head=R.TINY_AUX), seed=3).to(DEV)
    codes = _dev(R.palette_codes(2, 64, 64, seed=6))
    labels = _dev(np.random.RandomState(7).randint(0, 2, (2, 64, 64)).astype(np.uint8))

    def step(it, aug):
        """(loss, first parameter afterwards, the image and labels the network was given)."""
        net = copy.deepcopy(net0)
        trainer = train.segnet_trainer(net, DEV)
        opt = train.segnet_optimizer(trainer, lr=0.01)
        fed = []
        hook = trainer.register_forward_pre_hook(lambda mod, args: fed.append((args[0].clone(), args[1].clone())))
        loss = train.segnet_train_step(trainer, opt, it, 40, codes, labels, schedule=dict(warmup_iters=0), augment=aug)
        hook.remove()
        return float(loss), next(net.parameters()).detach().clone(), fed[0]

    aug = augment.SegAugment(seed=R.SEED)
    a, pa, (xa, la) = step(3, aug)
    b, pb, (xb, lb) = step(3, aug)
    c, _, (xc, lc) = step(4, aug)
    plain, _, (xp, lp) = step(3, None)
    # the inputs: bit-identical for the same (seed, it), those of augment.apply for images it * B .., different for another it
    assert torch.equal(xa, xb) and torch.equal(la, lb)
    want_x, want_l = augment.apply(aug, augment.draw_params(aug, 3 * 2, 2, DEV), codes, labels, IMG_MEAN, IMG_STD, torch.float32)
    assert torch.equal(xa, want_x) and torch.equal(la, want_l) and xa.shape == (2, 3, 64, 64)
    assert not torch.equal(xa, xc) and not torch.equal(xa, xp) and torch.equal(lp, labels)
    assert np.isfinite(a) and np.isfinite(c) and bool(torch.isfinite(pa).all()) and bool(torch.isfinite(pb).all())
    assert c != a and plain != a
    assert a == b                                                          # the same (seed, it) from the same weights: bit for bit
    padded = augment.SegAugment(seed=R.SEED, out_size=(96, 96))
    d, pd, (xd, ld) = step(3, padded)
    assert np.isfinite(d) and d != a and bool(torch.isfinite(pd).all())
    assert xd.shape == (2, 3, 96, 96) and ld.shape == (2, 96, 96) and int((ld == 255).sum()) == 2 * (96 * 96 - 64 * 64)
    assert torch.equal(xd[:, :, :64, :64], xa) and torch.equal(ld[:, :64, :64], la) and bool((xd[:, :, 64:] == 0).all())
