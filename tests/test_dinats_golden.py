"""DiNAT_s pinned to the REFERENCE's own code on the CPU, in float64.

tests/golden/g23_dinats.npz was written by tests/golden/make_dinats_fixture.py, which loads SegNet/dinats.py (and SegNet/nat.py for its
Mlp) unmodified with stand-ins for timm, mmcv, mmseg and natten — the attention op is the build's own statement of NATTEN's semantics
(oracle/segnet_ref.py na_fp64) and stays "parity unpinned", as in g16; everything around it is the reference's: PatchEmbed
dinats.py:172-202, NATransformerLayer :21-71, PatchMerging :74-104, BasicLayer :107-169, DiNAT_s.forward :319-336.

merge/*: the torch composition of fused.patch_merge_ln and dinats.PatchMerging reproduce the reference's PatchMerging — output and all
four gradients — within 1e-12 relative (test_dice_golden.py's bound for float64 against float64).  net: ppnet_amd.dinats.DiNAT_s has
the reference's keys, shapes and key order, loads its weights strictly and reproduces every level within 1e-10 * max(1, max|want|)
(the bound tests/test_segnet_wiring_golden.py applies to g16), with na_fp64 standing in for the attention kernel on the CPU."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests._oracle_util import wiring_weights  # noqa: E402


@pytest.fixture(scope="module")
def g23(golden_dir):
    return np.load(os.path.join(golden_dir, "g23_dinats.npz"))


def _close(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (what, np.abs(got - want).max(), np.abs(want).max())


def test_fixture_holds_the_cases_of_the_issue(g23):
    assert sorted(str(c) for c in g23["merge/cases"]) == ["even", "odd", "one"]
    assert g23["merge/odd/x"].shape == (2, 7, 5, 16) and g23["merge/even/x"].shape == (1, 4, 6, 8) and g23["merge/one/x"].shape == (1, 1, 1, 8)
    assert g23["merge/odd/y"].shape == (2, 12, 32) and g23["merge/one/y"].shape == (1, 1, 16)       # [B, L, 2C] as the reference returns it
    cfg = json.loads(str(g23["net/cfg"]))
    assert cfg["embed_dim"] == 32 and cfg["depths"] == [2, 2, 2, 1] and cfg["dilations"] == [[1, 3], [1, 2], [1, 2], [1]]
    assert g23["net/x"].shape == (1, 3, 50, 66) and g23["net/x"].dtype == np.float32
    assert [g23[f"net/y{i}"].shape for i in range(4)] == [(1, 32, 13, 17), (1, 64, 7, 9), (1, 128, 4, 5), (1, 256, 2, 3)]
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "g23_dinats.npz")) < 1_200_000


@pytest.mark.parametrize("case", ["odd", "even", "one"])
def test_patch_merging_is_the_references(g23, case):
    from ppnet_amd import dinats, fused
    z = {k: torch.from_numpy(g23[f"merge/{case}/{k}"]) for k in ("x", "norm.weight", "norm.bias", "reduction.weight", "y", "cot", "dx",
                                                                "dnorm.weight", "dnorm.bias", "dreduction.weight")}
    C = z["x"].shape[-1]
    m = dinats.PatchMerging(C).double()
    assert list(m.state_dict().keys()) == ["reduction.weight", "norm.weight", "norm.bias"]
    m.load_state_dict({k: z[k] for k in ("reduction.weight", "norm.weight", "norm.bias")}, strict=True)
    calls = dict(fused.MERGE_CALLS)
    x = z["x"].clone().requires_grad_(True)
    y = m(x)
    B, H, W, _ = x.shape
    assert y.shape == (B, -(-H // 2), -(-W // 2), 2 * C)
    gx, gw, gb, gr = torch.autograd.grad(y, [x, m.norm.weight, m.norm.bias, m.reduction.weight], z["cot"].view(y.shape))
    _close(y.detach().reshape(z["y"].shape), z["y"], "y")
    for got, key in ((gx, "dx"), (gw, "dnorm.weight"), (gb, "dnorm.bias"), (gr, "dreduction.weight")):
        _close(got, z[key], key)
    # the wrapper's torch composition alone, in front of the same reduction
    x2 = z["x"].clone().requires_grad_(True)
    y2 = torch.nn.functional.linear(fused.patch_merge_ln(x2, m.norm), m.reduction.weight)
    g2 = torch.autograd.grad(y2, [x2, m.norm.weight, m.norm.bias, m.reduction.weight], z["cot"].view(y2.shape))
    _close(y2.detach().reshape(z["y"].shape), z["y"], "y (wrapper)")
    for got, key in zip(g2, ("dx", "dnorm.weight", "dnorm.bias", "dreduction.weight")):
        _close(got, z[key], key + " (wrapper)")
    with torch.no_grad():
        _close(m(z["x"]).reshape(z["y"].shape), z["y"], "y (no autograd)")
    assert fused.MERGE_CALLS == calls                                        # CPU tensors never reach the kernels


def _cpu_attention(monkeypatch):
    """The float64 definition where the kernel cannot run: test_gpu_dice.py's route for its CPU reference."""
    from oracle import segnet_ref as SR
    from ppnet_amd import na
    own = na.NeighborhoodAttention2D.forward

    def forward(self, x, real_hw=None):
        if x.is_cuda:
            return own(self, x, real_hw)
        return SR.na_fp64(x, self.qkv.weight, self.qkv.bias, self.rpb, self.proj.weight, self.proj.bias, self.num_heads, 7, self.dilation)
    monkeypatch.setattr(na.NeighborhoodAttention2D, "forward", forward)


def test_dinats_is_the_references_wiring(g23, monkeypatch):
    from ppnet_amd.segnet import DiNAT_s
    cfg = json.loads(str(g23["net/cfg"]))
    keys = [str(k) for k in g23["net/keys"]]
    shapes = [tuple(json.loads(str(s))) for s in g23["net/shapes"]]
    w = wiring_weights(keys, shapes, int(g23["net/seed"][0]))
    chk = np.array([[w[k].sum(), (w[k] ** 2).sum()] for k in keys])
    assert np.allclose(chk, g23["net/checksum"], rtol=1e-13, atol=1e-13)     # the regenerated weights ARE the reference module's
    m = DiNAT_s(**cfg).double()
    sd = m.state_dict()
    assert list(sd.keys()) == keys and [tuple(v.shape) for v in sd.values()] == shapes
    for k in ("patch_embed.proj.weight", "patch_embed.norm.bias", "layers.0.blocks.1.attn.rpb", "layers.2.blocks.0.mlp.fc2.bias",
              "layers.0.downsample.reduction.weight", "layers.2.downsample.norm.weight", "norm3.bias"):
        assert k in keys, k
    assert not any("gamma" in k or k.startswith("levels") for k in keys) and "layers.3.downsample.reduction.weight" not in keys
    assert "layers.0.downsample.reduction.bias" not in keys
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    m.eval()
    _cpu_attention(monkeypatch)
    outs = m(torch.from_numpy(g23["net/x"]).double())                         # (grad mode on: the torch compositions, as in training)
    assert len(outs) == 4
    for i, o in enumerate(outs):
        got, want = o.detach().numpy(), g23[f"net/y{i}"]
        assert got.shape == want.shape
        assert np.abs(got - want).max() < 1e-10 * max(1.0, np.abs(want).max()), (i, np.abs(got - want).max())


def test_base_config_builds_and_narrows():
    from ppnet_amd import configs, dinats
    from ppnet_amd.segnet import DINATS_BASE_SETRUP, DiNAT_s, SegNet
    assert DINATS_BASE_SETRUP is configs.DINATS_BASE_SETRUP and DiNAT_s is dinats.DiNAT_s
    assert "pretrained" not in configs.DINATS_BASE_SETRUP["backbone"]
    net = SegNet.from_config(configs.DINATS_BASE_SETRUP)
    bb = net.backbone
    assert isinstance(bb, dinats.DiNAT_s) and bb.levels is bb.layers and len(bb.layers) == 4
    assert [len(layer.blocks) for layer in bb.layers] == [2, 2, 18, 2] and bb.num_features == [128, 256, 512, 1024]
    want = configs.DINATS_BASE_SETRUP["backbone"]["dilations"]
    assert want == [[1, 16], [1, 8], [1, 2, 1, 3, 1, 4] * 3, [1, 2]]
    assert [[blk.attn.dilation for blk in layer.blocks] for layer in bb.layers] == want
    assert [layer.blocks[0].attn.num_heads for layer in bb.layers] == [4, 8, 16, 32]
    assert all(blk.attn.head_dim == 32 and not blk.layer_scale and blk.mlp.fc1.out_features == 4 * blk.mlp.fc1.in_features
               for layer in bb.layers for blk in layer.blocks)
    assert [type(layer.downsample) for layer in bb.layers] == [dinats.PatchMerging] * 3 + [type(None)]
    assert [layer.downsample.norm.normalized_shape[0] for layer in bb.layers[:3]] == [512, 1024, 2048]
    assert all(layer.downsample.reduction.bias is None for layer in bb.layers[:3])
    assert bb.layers[2].blocks[17].drop_path_rate == pytest.approx(0.3 * 21 / 23) and bb.layers[0].blocks[0].drop_path_rate == 0.0
    assert bb.out_indices == (0, 1, 2, 3) and bb.compute_indices == (3,)                   # SETR-UP reads the last level only
    assert net.decode_head.conv_seg.out_channels == 2 and len(net.decode_head.up_convs) == 4
    assert not bb.patch_embed.takes_codes(torch.zeros(1, 8, 8, dtype=torch.uint8))


def test_segnet_narrows_compute_indices_as_for_nat():
    from ppnet_amd.segnet import SegNet
    bb = dict(type="DiNAT_s", embed_dim=32, depths=[1, 1, 1, 1], num_heads=[1, 2, 4, 8], mlp_ratio=2.0)
    head = dict(in_channels=256, channels=32, num_convs=2, up_scale=2, num_classes=2, kernel_size=3)
    aux = dict(type="FCNHead", in_channels=128, in_index=2, channels=16, num_convs=1, concat_input=False, num_classes=2)
    net = SegNet(backbone=bb, decode_head=head, auxiliary_head=aux)
    assert net.backbone.compute_indices == (2, 3)
    assert SegNet(backbone=bb, decode_head=head).backbone.compute_indices == (3,)
    net.prepare_inference()
    assert net.backbone.compute_indices == (3,) and all(blk.folded for layer in net.backbone.layers for blk in layer.blocks)
    two = SegNet(backbone=dict(bb, out_indices=(1, 3)), decode_head=head)
    assert two.backbone.compute_indices == (3,) and not hasattr(two.backbone, "norm0") and hasattr(two.backbone, "norm1")


def test_frozen_stages_raise():
    from ppnet_amd.dinats import DiNAT_s
    from ppnet_amd.segnet import SegNet
    with pytest.raises(NotImplementedError):
        DiNAT_s(embed_dim=32, depths=[1], num_heads=[1], frozen_stages=0)
    with pytest.raises(NotImplementedError):
        SegNet(backbone=dict(type="DiNAT_s", embed_dim=32, depths=[1, 1], num_heads=[1, 2], frozen_stages=0),
               decode_head=dict(in_channels=64, channels=32, num_convs=2, up_scale=2, num_classes=2, kernel_size=3))
    DiNAT_s(embed_dim=32, depths=[1], num_heads=[1], out_indices=(0,), frozen_stages=-1)
