"""The ViT backbone (ppnet_amd/vit.py) pinned to the REFERENCE's own code, and the ViT-B + SETR-UP SegNet config.

tests/golden/g20_vit.npz was written by tests/golden/make_vit_fixture.py, which loads SegNet/mmseg/backbones/vit.py,
SegNet/mmseg/models/utils/embed.py and SegNet/mmseg/ops/wrappers.py unmodified (mmcv names stubbed, see its docstring) and records,
in float64: a small ViT (embed 128, 2 heads of 64, 3 layers, out_indices (1, 2)) without and with the cls token / final norm / patch
norm on a 64 x 64 (stored pos grid), a 96 x 128 (bicubic pos resize) and a 70 x 50 ('corner' padding) input, one encoder layer
with logits of +-60..90, and the key list of the real ViT-B.  CPU only: the build's torch path in float64, to 1e-10."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests._oracle_util import wiring_weights  # noqa: E402
from tests._vit_golden import assert_matches, attn_tokens, checksum, image  # noqa: E402


@pytest.fixture(scope="module")
def g20(golden_dir):
    return np.load(os.path.join(golden_dir, "g20_vit.npz"))


def _net(g, net):
    from ppnet_amd.vit import VisionTransformer
    cfg = json.loads(str(g[f"{net}/cfg"]))
    keys = [str(k) for k in g[f"{net}/keys"]]
    shapes = dict(zip(keys, [tuple(json.loads(str(s))) for s in g[f"{net}/shapes"]]))
    w = wiring_weights(keys, [shapes[k] for k in keys], int(g[f"{net}/seed"][0]))
    assert np.allclose(np.array([[w[k].sum(), (w[k] ** 2).sum()] for k in keys]), g[f"{net}/checksum"], rtol=1e-13, atol=1e-13)
    return VisionTransformer(**cfg), keys, shapes, w


def load_net(g, net, dtype=torch.float64):
    """The build's VisionTransformer with g20's weights of network a / b, loaded strictly by mmseg's key names."""
    m, keys, shapes, w = _net(g, net)
    m = m.to(dtype)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    return m.eval()


@pytest.mark.parametrize("net", ["a", "b"])
def test_state_dict_layout_is_mmsegs(g20, net):
    m, keys, shapes, _ = _net(g20, net)
    sd = m.state_dict()
    assert list(sd.keys()) == keys
    assert {k: tuple(v.shape) for k, v in sd.items()} == shapes
    for k in ("patch_embed.projection.weight", "cls_token", "pos_embed", "layers.2.ln1.weight", "layers.0.attn.attn.in_proj_weight",
              "layers.0.attn.attn.in_proj_bias", "layers.1.attn.attn.out_proj.weight", "layers.1.ln2.bias", "layers.2.ffn.layers.0.0.weight",
              "layers.2.ffn.layers.1.bias"):
        assert k in keys, k
    assert ("ln1.weight" in keys) == (net == "b") and ("patch_embed.norm.weight" in keys) == (net == "b")


def test_vit_base_keys_and_shapes_are_the_references(g20):
    from ppnet_amd.segnet import VIT_BASE_SETRUP
    from ppnet_amd.vit import VisionTransformer
    cfg = {k: v for k, v in VIT_BASE_SETRUP["backbone"].items() if k != "type"}
    sd = VisionTransformer(**cfg).state_dict()
    assert list(sd.keys()) == [str(k) for k in g20["d/keys"]]
    assert [tuple(v.shape) for v in sd.values()] == [tuple(json.loads(str(s))) for s in g20["d/shapes"]]
    assert VisionTransformer(**cfg).layers[0].ln1.eps == float(g20["d/ln_eps"][0]) == 1e-6


@pytest.mark.parametrize("net", ["a", "b"])
@pytest.mark.parametrize("case,hw", [("a64", (4, 4)), ("a96", (6, 8)), ("a70", (5, 4))])
def test_torch_path_matches_reference_backbone(g20, net, case, hw):
    m = load_net(g20, net)
    x = image(case)
    assert np.array_equal(checksum(x), g20[f"{net}/{case}/x_checksum"])     # the regenerated input is the recorded one
    with torch.no_grad():
        outs = m(torch.from_numpy(x).double())
    assert len(outs) == 2
    for i, o in enumerate(outs):
        want = g20[f"{net}/{case}/y{i}"]
        assert want.shape == (1, 128) + hw
        assert o.is_contiguous(memory_format=torch.channels_last)
        assert_matches(o.numpy(), want, g20[f"{net}/{case}/y{i}_checksum"], 1e-10, (net, case, i))


def test_torch_layer_matches_reference_on_large_logits(g20):
    from ppnet_amd.vit import TransformerEncoderLayer
    c = json.loads(str(g20["c/cfg"]))
    C, heads = c["embed_dims"], c["num_heads"]
    layer = TransformerEncoderLayer(C, heads, 4 * C).double().eval()
    keys = [str(k) for k in g20["c/keys"]]
    sd = layer.state_dict()
    assert list(sd.keys()) == keys
    w = wiring_weights(keys, [tuple(sd[k].shape) for k in keys], c["seed"])
    w["attn.attn.in_proj_weight"][: 2 * C] *= c["qk_gain"]
    w["attn.attn.in_proj_bias"][: 2 * C] *= c["qk_gain"]
    assert np.allclose(np.array([[w[k].sum(), (w[k] ** 2).sum()] for k in keys]), g20["c/checksum"], rtol=1e-13, atol=1e-13)
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    assert 60.0 <= float(g20["c/max_abs_logit"][0]) <= 90.0
    x = torch.from_numpy(attn_tokens(c["tokens"], C)).double()
    with torch.no_grad():
        y, _ = layer(x)
    assert_matches(y.numpy(), g20["c/y"], g20["c/y_checksum"], 1e-10, "c")


def test_out_indices_int_and_compute_indices():
    from ppnet_amd.vit import VisionTransformer
    torch.manual_seed(0)
    m = VisionTransformer(img_size=32, embed_dims=64, num_layers=3, num_heads=1, out_indices=-1).eval()
    assert m.out_indices == [2]
    m.init_weights()
    with torch.no_grad():
        full = m(torch.randn(2, 3, 32, 32))
        m.out_indices, m.compute_indices = [0, 2], (0,)
        part = m(torch.randn(2, 3, 32, 32))
    assert len(full) == 1 and full[0].shape == (2, 64, 2, 2)
    assert part[0].shape == (2, 64, 2, 2) and part[1] is None              # stopped after layer 0
    for kw in (dict(output_cls_token=True), dict(with_cp=True), dict(num_fcs=3), dict(norm_cfg=dict(type="BN")),
               dict(act_cfg=dict(type="ReLU"))):
        with pytest.raises(NotImplementedError):
            VisionTransformer(img_size=32, embed_dims=64, num_layers=1, num_heads=1, **kw)


def test_segnet_vit_base_setrup_builds():
    from ppnet_amd.segnet import VIT_BASE_SETRUP, SegNet
    m = SegNet.from_config(VIT_BASE_SETRUP)
    sd = m.state_dict()
    assert sd["backbone.layers.11.attn.attn.in_proj_weight"].shape == (2304, 768)
    assert sd["backbone.layers.11.attn.attn.out_proj.weight"].shape == (768, 768)
    assert sd["backbone.layers.0.ffn.layers.0.0.weight"].shape == (3072, 768)
    assert sd["backbone.pos_embed"].shape == (1, 197, 768) and sd["backbone.cls_token"].shape == (1, 1, 768)
    assert sd["backbone.patch_embed.projection.weight"].shape == (768, 3, 16, 16)
    assert sd["decode_head.up_convs.0.0.conv.weight"].shape == (512, 768, 3, 3)
    assert sd["decode_head.up_convs.3.0.conv.weight"].shape == (512, 512, 3, 3)
    assert "backbone.ln1.weight" not in sd and "backbone.patch_embed.norm.weight" not in sd
    assert len({k.split(".")[2] for k in sd if k.startswith("backbone.layers.")}) == 12
    assert m.backbone.compute_indices == (11,) and m.backbone.layers[0].ln1.eps == 1e-6
    assert m.backbone.patch_embed.takes_codes(None) is False
    assert all(level.fold() is level for level in m.backbone.levels)


def test_mmcv_checkpoint_round_trip_and_pos_embed_resize(tmp_path):
    from ppnet_amd.vit import VisionTransformer, resize_pos_embed
    torch.manual_seed(1)
    kw = dict(img_size=64, embed_dims=64, num_layers=2, num_heads=1, with_cls_token=False)
    src = VisionTransformer(**kw)
    src.init_weights()
    assert src.pos_embed.abs().sum() > 0 and src.cls_token.abs().sum() > 0
    path = str(tmp_path / "vit.pth")
    torch.save({"state_dict": src.state_dict(), "meta": {"epoch": 1}}, path)
    dst = VisionTransformer(**kw)
    dst.init_weights(path)
    for k, v in src.state_dict().items():
        assert torch.equal(v, dst.state_dict()[k]), k
    big = VisionTransformer(**dict(kw, img_size=96), pretrained=path)            # 4 x 4 grid -> 6 x 6 (vit.py:277-288)
    assert big.pos_embed.shape == (1, 37, 64)
    assert torch.equal(big.pos_embed, resize_pos_embed(src.pos_embed.detach(), (6, 6), (4, 4), "bicubic"))
    assert torch.equal(big.layers[1].ffn.layers[1].weight, src.layers[1].ffn.layers[1].weight)


def test_segnet_vit_forward_train_finite_losses_and_grads():
    from ppnet_amd.segnet import SegNet
    torch.manual_seed(0)
    cfg = dict(backbone=dict(type="VisionTransformer", img_size=64, patch_size=16, embed_dims=64, num_layers=2, num_heads=1, drop_rate=0.1,
                             attn_drop_rate=0.1, drop_path_rate=0.1, with_cls_token=False),
               decode_head=dict(type="SETRUPHead", in_channels=64, channels=16, num_convs=4, up_scale=2, num_classes=2))
    m = SegNet.from_config(cfg)
    m.backbone.init_weights()
    m.train()
    img = torch.randn(2, 3, 64, 64)
    gt = torch.randint(0, 2, (2, 1, 64, 64))
    losses = m(img=img, img_metas=[{}, {}], gt_semantic_seg=gt)
    assert set(losses) == {"decode.loss_ce", "decode.acc_seg"}
    assert torch.isfinite(losses["decode.loss_ce"])
    losses["decode.loss_ce"].backward()
    for p in (m.backbone.layers[0].attn.attn.in_proj_weight, m.backbone.pos_embed, m.backbone.patch_embed.projection.weight):
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0
    assert all(p.grad is None or torch.isfinite(p.grad).all() for p in m.parameters())
