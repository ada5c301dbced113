"""DiNAT at DiNAT-L's width ratios pinned to the REFERENCE's own code, and the two configs that complete SegNet/configs.

tests/golden/g24_dinat_l_tiny.npz (+ g24_dinat_l_tiny_y0.npz, level 0's output: no committed file above 1 MiB) was written by
tests/golden/make_dinat_l_fixture.py, which imports SegNet/nat.py and SegNet/dinat.py unmodified with the stand-ins g16 uses
(tests/test_segnet_wiring_golden.py): DiNAT(embed_dim=96, heads [3, 6, 12, 24], no LayerScale) — every level's width is 3 * 2^k * 8, the
rows the LayerNorm kernels take in three passes.

CPU: oracle/segnet_ref.py reproduces the four outputs in float64 to 1e-10; ppnet_amd.segnet.DiNAT keeps the key order; DINAT_LARGE and
NAT_MINI_UPER build by name.  GPU: the float32 backbone through the HIP kernels to 2e-3 (the bound of
test_gpu_nat_float32_vs_reference_outputs), and one training step at these widths on the library composition."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests._oracle_util import wiring_weights  # noqa: E402

NAME = "dinat_l_tiny"


@pytest.fixture(scope="module")
def g24(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "g24_dinat_l_tiny.npz")))
    g.update(np.load(os.path.join(golden_dir, "g24_dinat_l_tiny_y0.npz")))
    return g


def _case(g):
    cfg = json.loads(str(g[f"{NAME}/cfg"]))
    keys = [str(k) for k in g[f"{NAME}/keys"]]
    shapes = [tuple(json.loads(str(s))) for s in g[f"{NAME}/shapes"]]
    w = wiring_weights(keys, shapes, int(g[f"{NAME}/seed"][0]))
    chk = np.array([[w[k].sum(), (w[k] ** 2).sum()] for k in keys])
    assert np.allclose(chk, g[f"{NAME}/checksum"], rtol=1e-13, atol=1e-13)       # the regenerated weights ARE the reference module's
    return cfg, keys, w, g[f"{NAME}/x"], {i: g[f"{NAME}/y{i}"] for i in cfg["out_indices"]}


def test_fixture_holds_the_case_and_its_shapes(g24):
    assert [str(c) for c in g24["cases"]] == [NAME]
    cfg, keys, w, x, ys = _case(g24)
    assert cfg == dict(embed_dim=96, mlp_ratio=2.0, depths=[1, 2, 1, 1], num_heads=[3, 6, 12, 24], kernel_size=7,
                       dilations=[[1], [1, 2], [1], [1]], out_indices=[0, 1, 2, 3], layer_scale=None, drop_path_rate=0.3)
    assert x.shape == (2, 3, 64, 96) and x.dtype == np.float32
    assert [ys[i].shape for i in range(4)] == [(2, 96, 16, 24), (2, 192, 8, 12), (2, 384, 4, 6), (2, 768, 2, 3)]
    assert all(ys[i].dtype == np.float64 for i in range(4))
    assert not any(k.endswith(("gamma1", "gamma2")) for k in keys)               # no layer_scale: no LayerScale parameters
    assert w["levels.3.blocks.0.attn.rpb"].shape == (24, 13, 13) and w["levels.1.blocks.1.mlp.fc1.weight"].shape == (384, 192)
    assert "levels.2.downsample.reduction.weight" in keys and "levels.3.downsample.reduction.weight" not in keys


def test_oracle_backbone_is_the_references_wiring(g24):
    """oracle/segnet_ref.py backbone_fp64 == the reference's DiNAT.forward on the same weights and input (float64)."""
    from oracle import segnet_ref as SR
    cfg, keys, w, x, ys = _case(g24)
    sd = {k: torch.from_numpy(v) for k, v in w.items()}
    outs = SR.backbone_fp64(sd, torch.from_numpy(x).double(), cfg["depths"], cfg["num_heads"], cfg["dilations"],
                            layer_scale=cfg["layer_scale"] is not None, prefix="")
    for i, want in ys.items():
        got = outs[i].numpy()
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-10 * max(1.0, np.abs(want).max()), i


def test_cpu_product_module_keeps_the_references_keys(g24):
    from ppnet_amd.segnet import DiNAT
    cfg, keys, w, _, _ = _case(g24)
    m = DiNAT(**cfg)
    assert list(m.state_dict().keys()) == keys
    m.load_state_dict({k: torch.from_numpy(v).float() for k, v in w.items()}, strict=True)


def test_dinat_large_and_nat_mini_build_by_name():
    """Every config under SegNet/configs has a constant: the last two.  DiNAT-L (some 200 M parameters) is built on the meta device."""
    from ppnet_amd import configs, segnet
    from ppnet_amd.segnet import DINAT_LARGE, NAT_MINI_UPER, SegNet
    assert DINAT_LARGE is configs.DINAT_LARGE and NAT_MINI_UPER is configs.NAT_MINI_UPER
    for cfg in (DINAT_LARGE, NAT_MINI_UPER):
        assert "pretrained" not in cfg["backbone"] and cfg["pretrained"] is None
    assert "layer_scale" not in DINAT_LARGE["backbone"] and "auxiliary_head" not in DINAT_LARGE

    with torch.device("meta"):
        m = SegNet.from_config(DINAT_LARGE)
    bb, h = m.backbone, m.decode_head
    assert type(bb) is segnet.DiNAT and bb.num_features == [192, 384, 768, 1536] and [len(lv.blocks) for lv in bb.levels] == [3, 4, 18, 5]
    assert [lv.blocks[0].attn.num_heads for lv in bb.levels] == [6, 12, 24, 48]
    assert [[b.attn.dilation for b in lv.blocks] for lv in bb.levels] == DINAT_LARGE["backbone"]["dilations"]
    assert max(max(d) for d in DINAT_LARGE["backbone"]["dilations"]) == 20
    assert not any(b.layer_scale for lv in bb.levels for b in lv.blocks)
    assert [b.drop_path_rate for b in bb.levels[0].blocks][0] == 0.0 and abs(bb.levels[3].blocks[4].drop_path_rate - 0.3) < 1e-6
    assert type(h) is segnet.SETRUPHead and len(h.up_convs) == 4 and h.norm.normalized_shape == (1536,) and h.norm.eps == 1e-6
    assert bb.compute_indices == (3,) and m.auxiliary_head is None
    sd = m.state_dict()
    assert tuple(sd["backbone.levels.2.blocks.17.attn.rpb"].shape) == (24, 13, 13)
    assert tuple(sd["decode_head.up_convs.0.0.conv.weight"].shape) == (512, 1536, 3, 3)
    assert tuple(sd["backbone.levels.3.blocks.4.mlp.fc1.weight"].shape) == (3072, 1536)
    assert tuple(sd["decode_head.conv_seg.weight"].shape) == (2, 512, 1, 1)
    assert not any(k.endswith(("gamma1", "gamma2")) for k in sd)

    n = SegNet.from_config(NAT_MINI_UPER)
    bb, h, a = n.backbone, n.decode_head, n.auxiliary_head
    assert type(bb) is segnet.NAT and bb.num_features == [64, 128, 256, 512] and [len(lv.blocks) for lv in bb.levels] == [3, 4, 6, 5]
    assert [lv.blocks[0].attn.num_heads for lv in bb.levels] == [2, 4, 8, 16] and all(b.layer_scale for lv in bb.levels for b in lv.blocks)
    assert type(h) is segnet.UPerHead and [c.conv.in_channels for c in h.lateral_convs] == [64, 128, 256]
    assert h.bottleneck.conv.in_channels == 512 + 4 * 64 and h.fpn_bottleneck.conv.out_channels == 64 and h.conv_seg.out_channels == 2
    sd = n.state_dict()
    assert tuple(sd["backbone.levels.0.blocks.0.mlp.fc1.weight"].shape) == (192, 64)
    assert tuple(sd["backbone.levels.3.blocks.0.mlp.fc2.weight"].shape) == (512, 1536)
    # the auxiliary head as the reference merges it: 512 input channels on level 2, which has 256
    assert type(a) is segnet.FCNHead and a.in_index == 2 and a.convs[0].conv.in_channels == 512 and a.loss_weight == 0.4
    assert a.conv_seg.out_channels == 2 and bb.num_features[a.in_index] == 256


@pytest.mark.gpu
def test_gpu_dinat_float32_vs_reference_outputs(g24):
    """The product backbone on the HIP kernels in float32 (ppn_na2d_fwd at 3 / 6 / 12 / 24 heads, the three-pass residual / LayerNorm
    kernels at 96 / 192 / 384 / 768, library convolutions) against the reference module's float64 outputs."""
    from ppnet_amd.segnet import DiNAT
    cfg, keys, w, x, ys = _case(g24)
    m = DiNAT(**cfg)
    m.load_state_dict({k: torch.from_numpy(v).float() for k, v in w.items()}, strict=True)
    m = m.eval().cuda()
    with torch.no_grad():
        outs = m(torch.from_numpy(x).cuda())
    assert len(outs) == 4
    for i, o in zip(cfg["out_indices"], outs):
        got = o.float().cpu().double().numpy()
        want = ys[i]
        assert got.shape == want.shape
        err = np.abs(got - want).max()
        print(f"level {i}: max error {err:.3e} (max |want| {np.abs(want).max():.3f})")
        assert err < 2e-3 * max(1.0, np.abs(want).max()), (i, err)


@pytest.mark.gpu
def test_gpu_training_step_at_these_widths_keeps_the_library_composition(g24):
    """One train.segnet_train_step on the tiny config, 2 images of 64 x 96: every parameter gets a finite gradient.  The recorded
    LayerNorm pair keeps fused.NORM_WIDTHS (none of 96 / 192 / 384 / 768), so this runs the torch composition and launches no kernel of
    the pair."""
    from ppnet_amd import fused, train
    from ppnet_amd.segnet import SegNet
    cfg, keys, w, x, _ = _case(g24)
    assert not {96, 192, 384, 768, 1536} & set(fused.NORM_WIDTHS)
    torch.manual_seed(0)
    # an UPerHead reads all four levels, so every output norm is trained too
    net = SegNet(backbone=dict(cfg, type="DiNAT"),
                 decode_head=dict(type="UPerHead", in_channels=[96, 192, 384, 768], in_index=[0, 1, 2, 3], channels=32, num_classes=2))
    net.backbone.load_state_dict({k: torch.from_numpy(v).float() for k, v in w.items()}, strict=True)
    net = net.cuda()
    trainer = train.segnet_trainer(net)
    opt = train.segnet_optimizer(trainer, lr=0.01)
    img = torch.from_numpy(x).cuda()
    labels = (torch.arange(64 * 96, device="cuda").view(1, 64, 96) // 7 % 2).to(torch.uint8).expand(2, -1, -1).contiguous()
    before = dict(fused.NORM_CALLS)
    loss = train.segnet_train_step(trainer, opt, 0, 10, img, labels, schedule=dict(warmup_iters=0))
    assert bool(torch.isfinite(loss)) and fused.NORM_CALLS == before
    for n_, p in net.named_parameters():
        assert p.requires_grad and p.grad is not None and bool(torch.isfinite(p.grad).all()), n_
