"""UPerPUPHead (ppnet_amd/segnet.py) pinned to the REFERENCE's own head, and the dense NAT / Swin configs.

tests/golden/g19_uperpup.npz was written by tests/golden/make_uperpup_fixture.py, which loads SegNet/mmseg/decode_heads/uper_pup_head.py,
decode_head.py, psp_head.py and mmseg/ops/wrappers.py unmodified (mmcv names stubbed, see its docstring) and records, in float64 and
eval mode, the logits of a NAT-style head (num_convs 1-2-3-4, square levels) and a Swin-style one (2-3-4-5, non-square, batch 2), and
the state-dict layout of the two real config heads.  CPU only: the build's torch path in float64, to 1e-10."""
import ctypes
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests._swin_golden import assert_matches, checksum  # noqa: E402
from tests._uperpup_golden import CASES, REAL, features, head_kwargs, head_weights  # noqa: E402


@pytest.fixture(scope="module")
def g19(golden_dir):
    return np.load(os.path.join(golden_dir, "g19_uperpup.npz"))


def load_head(g, case, dtype=torch.float64):
    """The build's UPerPUPHead of `case` with g19's weights, loaded strictly by the reference's key names."""
    from ppnet_amd.segnet import UPerPUPHead
    keys = [str(k) for k in g[f"{case}/keys"]]
    shapes = [tuple(json.loads(str(s))) for s in g[f"{case}/shapes"]]
    w = head_weights(keys, shapes, CASES[case][5])
    assert np.allclose(np.array([[w[k].sum(), (w[k] ** 2).sum()] for k in keys]), g[f"{case}/checksum"], rtol=1e-13, atol=1e-13)
    m = UPerPUPHead(**head_kwargs(case)).to(dtype)
    sd = {k: torch.from_numpy(v) for k, v in w.items()}
    for k, v in m.state_dict().items():
        if k.endswith("num_batches_tracked"):
            sd[k] = v
    m.load_state_dict(sd, strict=True)
    return m.eval()


@pytest.mark.parametrize("case", ["a", "b"])
def test_torch_path_matches_reference_head(g19, case):
    m = load_head(g19, case)
    xs = features(case)
    assert np.array_equal(np.stack([checksum(x) for x in xs]), g19[f"{case}/x_checksum"])   # the regenerated inputs are the recorded ones
    with torch.no_grad():
        y = m([torch.from_numpy(x).double() for x in xs])
    B, (h, w) = CASES[case][3], CASES[case][4][0]
    n0 = CASES[case][0][0]
    assert tuple(y.shape) == (B, 2, h << n0, w << n0)
    assert_matches(y.numpy(), g19[f"{case}/y"], g19[f"{case}/y_checksum"], 1e-10, case)


@pytest.mark.parametrize("name", sorted(REAL))
def test_real_config_heads_have_the_reference_state_dict(g19, name):
    from ppnet_amd.segnet import NAT_BASE_UPERPUP, SWIN_BASE_UPERPUP, SegNet
    cfg = {"nat": NAT_BASE_UPERPUP, "swin": SWIN_BASE_UPERPUP}[name]
    sd = SegNet.from_config(cfg).decode_head.state_dict()
    keys = [str(k) for k in g19[f"real_{name}/keys"]]
    assert list(sd) == keys
    assert [list(v.shape) for v in sd.values()] == [json.loads(str(s)) for s in g19[f"real_{name}/shapes"]]
    assert "lateral_convs.2.conv.weight" in keys and "lateral_convs.3.conv.weight" not in keys
    assert f"fpn_convs.3.{REAL[name][3] - 1}.0.bn.running_var" in keys


@pytest.mark.parametrize("name,num_convs", [("NAT_BASE_UPERPUP", (1, 2, 3, 4)), ("SWIN_BASE_UPERPUP", (2, 3, 4, 5))])
def test_from_config_builds_dense_configs(name, num_convs):
    from ppnet_amd import segnet
    from ppnet_amd.swin import SwinTransformer
    m = segnet.SegNet.from_config(getattr(segnet, name))
    h = m.decode_head
    assert type(h) is segnet.UPerPUPHead and h.num_convs == num_convs
    assert [len(c) for c in h.fpn_convs] == list(num_convs) and len(h.lateral_convs) == 3
    assert h.fpn_bottleneck.conv.in_channels == 1024 and h.fpn_bottleneck.conv.out_channels == 256 and h.conv_seg.out_channels == 2
    assert isinstance(h.dropout, torch.nn.Dropout2d) and h.dropout.p == 0.1
    a = m.auxiliary_head
    assert type(a) is segnet.FCNHead and a.convs[0].conv.in_channels == 512 and a.conv_seg.out_channels == 2 and a.in_index == 2
    assert a.loss_weight == 0.4
    assert isinstance(m.backbone, SwinTransformer if name.startswith("SWIN") else segnet.NAT)
    if name.startswith("NAT"):
        assert m.backbone.num_features == [128, 256, 512, 1024] and len(m.backbone.levels[2].blocks) == 18


def test_chains_ending_at_different_sizes_raise():
    """num_convs[i] - i not constant: the reference's torch.cat raises, and so does this head (no silent resize)."""
    from ppnet_amd.segnet import UPerPUPHead
    torch.manual_seed(0)
    m = UPerPUPHead(in_channels=[8, 8, 8, 8], channels=8, num_convs=(1, 1, 3, 4), num_classes=2).eval()
    xs = [torch.randn(1, 8, 16 >> i, 16 >> i) for i in range(4)]
    with torch.no_grad(), pytest.raises(RuntimeError):
        m(xs)


def tiny_segnet_cfg(backbone):
    """A small SegNet with an UPerPUPHead (num_convs 1-2-3-4, as dense NAT) and an FCN auxiliary head on level 2."""
    bb = (dict(type="NAT", embed_dim=32, mlp_ratio=2.0, depths=[1, 1, 1, 1], num_heads=[1, 2, 4, 8], kernel_size=7, drop_path_rate=0.1,
               layer_scale=1e-5) if backbone == "NAT" else
          dict(type="SwinTransformer", embed_dims=32, depths=(2, 2, 2, 2), num_heads=(1, 2, 4, 8), drop_path_rate=0.1))
    return dict(backbone=bb,
                decode_head=dict(type="UPerPUPHead", in_channels=[32, 64, 128, 256], channels=16, num_convs=(1, 2, 3, 4), num_classes=2),
                auxiliary_head=dict(type="FCNHead", in_channels=128, in_index=2, channels=16, num_convs=1, concat_input=False, num_classes=2,
                                    loss_decode=dict(loss_weight=0.4)))


def check_forward_train(cfg, device="cpu"):
    """forward_train's decode.* / aux.* losses are finite and every head parameter gets a finite, non-zero gradient."""
    from ppnet_amd.segnet import SegNet
    torch.manual_seed(0)
    m = SegNet.from_config(cfg).to(device).train()
    img = torch.randn(2, 3, 64, 64, device=device)
    gt = torch.randint(0, 2, (2, 1, 64, 64), device=device)
    losses = m(img=img, img_metas=[{}, {}], gt_semantic_seg=gt)
    assert set(losses) == {"decode.loss_ce", "decode.acc_seg", "aux.loss_ce", "aux.acc_seg"}
    total = losses["decode.loss_ce"] + losses["aux.loss_ce"]
    assert torch.isfinite(total)
    total.backward()
    for k, p in m.decode_head.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0, k
    assert all(p.grad is None or torch.isfinite(p.grad).all() for p in m.parameters())


def test_forward_train_uperpup_losses_and_grads_cpu():
    """On the CPU with the Swin backbone (pure torch); the NAT form needs the GPU attention kernel (tests/test_gpu_uperpup.py)."""
    check_forward_train(tiny_segnet_cfg("SwinTransformer"))


def test_capi_upsample2x_concat_rejects_bad_arguments():
    """ppn_upsample2x_concat_nhwc validates before any HIP call: every bad argument returns PPN_E_INVALID (the pointers are never
    dereferenced, so host addresses stand in for device buffers)."""
    from ppnet_amd import _lib as L
    f = L.lib.ppn_upsample2x_concat_nhwc
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    E_INVALID = -1

    def call(n=2, ptrs=(p, p), ch=(16, 8), out=p, B=1, H=4, W=4, dtype=1):
        xs = (ctypes.c_void_p * max(1, len(ptrs)))(*ptrs) if ptrs is not None else None
        cs = (ctypes.c_int32 * max(1, len(ch)))(*ch) if ch is not None else None
        return f(xs, cs, n, out, B, H, W, dtype, None)
    assert call(n=0) == E_INVALID and call(n=9, ptrs=(p,) * 9, ch=(8,) * 9) == E_INVALID and call(n=-1) == E_INVALID
    assert call(ptrs=None) == E_INVALID and call(ch=None) == E_INVALID and call(out=None) == E_INVALID
    assert call(ptrs=(p, None)) == E_INVALID
    assert call(ch=(16, 12)) == E_INVALID and call(ch=(0, 8)) == E_INVALID and call(ch=(-8, 8)) == E_INVALID
    assert call(dtype=2) == E_INVALID and call(dtype=-1) == E_INVALID
    assert call(B=0) == E_INVALID and call(H=0) == E_INVALID and call(W=-3) == E_INVALID
    assert call(B=1 << 20, H=1 << 11) == E_INVALID                          # B (H + 1) block rows >= 2^31
    assert call(W=1 << 20, ch=(256, 8)) == E_INVALID                        # more than 65535 pieces of 256 threads per block row
    assert call(H=1 << 30) == E_INVALID
    assert call(ch=(1 << 30, 1 << 30)) == E_INVALID                         # the channel offsets pass 2^31
