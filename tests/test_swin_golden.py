"""The Swin backbone (ppnet_amd/swin.py) pinned to the REFERENCE's own code.

tests/golden/g18_swin.npz was written by tests/golden/make_swin_fixture.py, which loads SegNet/mmseg/backbones/swin.py and
SegNet/mmseg/models/utils/embed.py unmodified (mmcv / mmseg names stubbed, see its docstring) and records, in float64: a small Swin
(embed 64, depths 2-2-2-2, heads 2-4-8-16) on a 112 x 112 and a 60 x 92 input, and one shifted-window attention with logits of
+-60..90 under the reference's -100 mask and under -inf (outputs as float32 values plus float64 checksums, tests/_swin_golden.py).
CPU only: the build's torch path in float64, to 1e-10."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests._oracle_util import wiring_weights  # noqa: E402
from tests._swin_golden import assert_matches, checksum, image  # noqa: E402


@pytest.fixture(scope="module")
def g18(golden_dir):
    return np.load(os.path.join(golden_dir, "g18_swin.npz"))


def _net(g):
    from ppnet_amd.swin import SwinTransformer
    cfg = json.loads(str(g["net/cfg"]))
    keys = [str(k) for k in g["net/keys"]]
    fkeys = [k for k in keys if not k.endswith("relative_position_index")]
    shapes = dict(zip(keys, [tuple(json.loads(str(s))) for s in g["net/shapes"]]))
    w = wiring_weights(fkeys, [shapes[k] for k in fkeys], int(g["net/seed"][0]))
    chk = np.array([[w[k].sum(), (w[k] ** 2).sum()] for k in fkeys])
    assert np.allclose(chk, g["net/checksum"], rtol=1e-13, atol=1e-13)
    m = SwinTransformer(**cfg)
    return m, cfg, keys, shapes, w


def load_net(g, dtype=torch.float64):
    """The build's SwinTransformer with g18's weights, loaded strictly by mmseg's key names."""
    m, cfg, keys, shapes, w = _net(g)
    sd = {k: torch.from_numpy(v) for k, v in w.items()}
    for k in keys:
        if k.endswith("relative_position_index"):
            sd[k] = torch.from_numpy(g["net/relative_position_index"].astype(np.int64))
    m = m.to(dtype)
    m.load_state_dict(sd, strict=True)
    return m.eval(), cfg


def test_state_dict_layout_is_mmsegs(g18):
    m, cfg, keys, shapes, _ = _net(g18)
    sd = m.state_dict()
    assert list(sd.keys()) == keys
    assert {k: tuple(v.shape) for k, v in sd.items()} == shapes
    for k in ("patch_embed.projection.weight", "patch_embed.norm.bias", "stages.0.blocks.1.attn.w_msa.relative_position_bias_table",
              "stages.2.blocks.0.ffn.layers.0.0.weight", "stages.2.blocks.0.ffn.layers.1.bias", "stages.1.downsample.reduction.weight",
              "stages.1.downsample.norm.weight", "norm3.weight"):
        assert k in keys, k
    assert "stages.1.downsample.reduction.bias" not in keys and "stages.3.downsample.norm.weight" not in keys
    assert np.array_equal(sd["stages.0.blocks.0.attn.w_msa.relative_position_index"].numpy(), g18["net/relative_position_index"].astype(np.int64))


@pytest.mark.parametrize("case,shapes", [("a", [(64, 28, 28), (128, 14, 14), (256, 7, 7), (512, 4, 4)]),
                                         ("b", [(64, 15, 23), (128, 8, 12), (256, 4, 6), (512, 2, 3)])])
def test_torch_path_matches_reference_backbone(g18, case, shapes):
    m, cfg = load_net(g18)
    x = image(case)
    assert np.array_equal(checksum(x), g18[f"{case}/x_checksum"])            # the regenerated input is the recorded one
    with torch.no_grad():
        outs = m(torch.from_numpy(x).double())
    assert len(outs) == 4
    for i, (o, shp) in enumerate(zip(outs, shapes)):
        want = g18[f"{case}/y{i}"]
        assert want.shape == (1,) + shp
        assert_matches(o.numpy(), want, g18[f"{case}/y{i}_checksum"], 1e-10, (case, i))


def test_torch_window_attention_matches_reference_shifted_msa(g18):
    """The torch composition (ppnet_amd.swin.window_attention) against the reference's ShiftWindowMSA on logits of +-60..90:
    -100 as the reference masks, and -inf recorded beside it to show that the choice is visible here."""
    from ppnet_amd.swin import ShiftWindowMSA, window_attention
    c = json.loads(str(g18["c/cfg"]))
    C, heads, H, W, shift = c["embed_dims"], c["num_heads"], c["H"], c["W"], c["shift"]
    keys = [str(k) for k in g18["c/keys"]]
    a = ShiftWindowMSA(C, heads, 7, shift).double().eval()
    shapes = {k: tuple(v.shape) for k, v in a.state_dict().items()}
    w = wiring_weights(keys, [shapes[k] for k in keys], c["seed"])
    w["w_msa.qkv.weight"][: 2 * C] *= c["qk_gain"]
    assert np.allclose(np.array([[w[k].sum(), (w[k] ** 2).sum()] for k in keys]), g18["c/checksum"], rtol=1e-13, atol=1e-13)
    a.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    assert 60.0 <= float(g18["c/max_abs_logit"][0]) <= 90.0
    y100, yinf = g18["c/y_m100"], g18["c/y_minf"]
    assert np.abs(y100 - yinf).max() > 1.0 and float(g18["c/max_abs_diff"][0]) > 1.0   # the mask value matters on this input
    x = torch.from_numpy(g18["c/x"]).double().view(1, H, W, C)
    with torch.no_grad():
        assert_matches(a(x).numpy(), y100, g18["c/y_m100_checksum"], 1e-10, "-100")
        m = a.w_msa
        qkv = m.qkv(x)
        o = window_attention(qkv, m.qkv.bias, m.relative_position_bias_table, heads, shift, m.scale, mask_value=float("-inf"))
        assert_matches(m.proj(o).numpy(), yinf, g18["c/y_minf_checksum"], 1e-10, "-inf")


def _seg_keys(cfg):
    from ppnet_amd.segnet import SegNet
    return SegNet.from_config(cfg).state_dict()


def test_segnet_swin_base_configs_build_with_mmseg_keys():
    from ppnet_amd.segnet import SWIN_BASE_SETRUP, SWIN_BASE_UPER
    for cfg, head_keys in ((SWIN_BASE_UPER, ("decode_head.psp_modules.3.1.conv.weight", "decode_head.fpn_bottleneck.conv.weight",
                                             "auxiliary_head.convs.0.conv.weight")),
                           (SWIN_BASE_SETRUP, ("decode_head.up_convs.3.0.conv.weight", "decode_head.norm.weight"))):
        sd = _seg_keys(cfg)
        bb = [k for k in sd if k.startswith("backbone.")]
        blocks = {k.split(".")[2] + "." + k.split(".")[4] for k in bb if k.startswith("backbone.stages.") and ".blocks." in k}
        assert len(blocks) == 2 + 2 + 18 + 2
        assert sd["backbone.stages.2.blocks.17.attn.w_msa.relative_position_bias_table"].shape == (169, 16)
        assert sd["backbone.stages.3.blocks.1.ffn.layers.0.0.weight"].shape == (4096, 1024)
        assert sd["backbone.stages.2.downsample.reduction.weight"].shape == (1024, 2048)
        assert sd["backbone.patch_embed.projection.weight"].shape == (128, 3, 4, 4)
        assert all(f"backbone.norm{i}.weight" in sd for i in range(4))
        for k in head_keys:
            assert k in sd, k


def test_segnet_swin_forward_train_finite_losses_and_grads():
    from ppnet_amd.segnet import SegNet
    torch.manual_seed(0)
    cfg = dict(backbone=dict(type="SwinTransformer", embed_dims=32, depths=(2, 2, 2, 2), num_heads=(1, 2, 4, 8), drop_path_rate=0.1),
               decode_head=dict(type="UPerHead", in_channels=[32, 64, 128, 256], channels=16, num_classes=2),
               auxiliary_head=dict(type="FCNHead", in_channels=128, in_index=2, channels=16, num_convs=1, concat_input=False, num_classes=2,
                                   loss_decode=dict(loss_weight=0.4)))
    m = SegNet.from_config(cfg).train()
    img = torch.randn(2, 3, 64, 64)
    gt = torch.randint(0, 2, (2, 1, 64, 64))
    losses = m(img=img, img_metas=[{}, {}], gt_semantic_seg=gt)
    assert set(losses) == {"decode.loss_ce", "decode.acc_seg", "aux.loss_ce", "aux.acc_seg"}
    total = losses["decode.loss_ce"] + losses["aux.loss_ce"]
    assert torch.isfinite(total)
    total.backward()
    g = m.backbone.stages[0].blocks[1].attn.w_msa.relative_position_bias_table.grad
    assert g is not None and torch.isfinite(g).all() and g.abs().sum() > 0
    assert all(p.grad is None or torch.isfinite(p.grad).all() for p in m.parameters())
