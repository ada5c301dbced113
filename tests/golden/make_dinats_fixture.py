"""Writes tests/golden/g23_dinats.npz: the reference's DiNAT_s (SegNet/dinats.py) in float64, eval mode.

SegNet/dinats.py and SegNet/nat.py (for its Mlp) are loaded by path, UNMODIFIED, with the stand-ins of make_fixtures.py's
_install_segnet_stubs: timm.models.layers (DropPath = identity, trunc_normal_ = no-op, to_2tuple), mmcv.runner.load_checkpoint,
mmseg.utils.get_root_logger, mmseg.models.builder.BACKBONES, and natten.NeighborhoodAttention2D = oracle.segnet_ref.na_fp64 (the
attention op itself stays "parity unpinned", as in g16).  Numbers only.

  merge/<k>/*   PatchMerging alone at (2,7,5,16) (both sizes odd), (1,4,6,8) and (1,1,1,8): the input, the three parameters, the output
                ([B, Ho Wo, 2C], as the reference returns it), a stored cotangent and the autograd gradients of the input and of the three
                parameters.
  net/*         DiNAT_s(embed_dim=32, depths=[2,2,2,1], num_heads=[1,2,4,8], dilations=[[1,3],[1,2],[1,2],[1]], mlp_ratio=2.0,
                drop_path_rate=0.2, out_indices=(0,1,2,3)) on a (1,3,50,66) input: the patch embed pads it to 52 x 68, a 13 x 17 grid that
                becomes 7 x 9, 4 x 5 and 2 x 3 — every merge pads, every dilated layer is smaller than its window.  Weights from
                tests/_oracle_util.wiring_weights; stored: state-dict keys, shapes, checksums, the input rounded to float32, every level.

One thing the reference's file cannot do by itself: PatchMerging.forward ends in `x.view(B, -1, 4 * C)` (dinats.py:100), so the next
BasicLayer hands a [B, L, C] tensor to an attention module that takes [B, H, W, C].  The `net` case therefore registers a forward hook on
every `downsample` module that views its output back as the [B, ceil(H/2), ceil(W/2), 2C] grid it is — the same numbers, no arithmetic;
the module's own code is untouched, and the `merge/*` cases record its output as it returns it.

Run from the repository root:  python tests/golden/make_dinats_fixture.py <path to the reference's SegNet directory>"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))


def install_stubs():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    from oracle import segnet_ref as SR

    class DropPath(nn.Module):
        def __init__(self, drop_prob=0.0):
            super().__init__()

        def forward(self, x):
            assert not self.training
            return x

    class NeighborhoodAttention2D(nn.Module):
        def __init__(self, dim, kernel_size, dilation=None, num_heads=1, qkv_bias=True, qk_scale=None, attn_drop=0.0, proj_drop=0.0):
            super().__init__()
            assert qk_scale is None and attn_drop == 0.0 and proj_drop == 0.0
            self.num_heads, self.kernel_size, self.dilation = num_heads, kernel_size, dilation or 1
            self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
            self.rpb = nn.Parameter(torch.zeros(num_heads, 2 * kernel_size - 1, 2 * kernel_size - 1))
            self.proj = nn.Linear(dim, dim)

        def forward(self, x):
            return SR.na_fp64(x, self.qkv.weight, self.qkv.bias, self.rpb, self.proj.weight, self.proj.bias, self.num_heads,
                              self.kernel_size, self.dilation)

    class _Registry:
        def register_module(self, *a, **k):
            return lambda cls: cls

    def mod(name, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m

    mod("timm"); mod("timm.models")
    mod("timm.models.layers", DropPath=DropPath, trunc_normal_=lambda t, *a, **k: t, to_2tuple=lambda v: v if isinstance(v, tuple) else (v, v))
    mod("mmcv"); mod("mmcv.runner", load_checkpoint=lambda *a, **k: None)
    mod("mmseg"); mod("mmseg.utils", get_root_logger=lambda *a, **k: None)
    mod("mmseg.models"); mod("mmseg.models.builder", BACKBONES=_Registry())
    mod("natten", NeighborhoodAttention2D=NeighborhoodAttention2D)


def load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


MERGE_CASES = {"odd": (2, 7, 5, 16), "even": (1, 4, 6, 8), "one": (1, 1, 1, 8)}
NET_CFG = dict(embed_dim=32, depths=[2, 2, 2, 1], num_heads=[1, 2, 4, 8], dilations=[[1, 3], [1, 2], [1, 2], [1]], mlp_ratio=2.0,
               drop_path_rate=0.2, out_indices=(0, 1, 2, 3))
NET_X, NET_SEED = (1, 3, 50, 66), 3


def main(seg):
    install_stubs()
    from _oracle_util import wiring_weights
    load_by_path("nat", os.path.join(seg, "nat.py"))                         # dinats.py:18: `from nat import Mlp`
    D = load_by_path("dinats", os.path.join(seg, "dinats.py"))
    out = {"merge/cases": np.array(sorted(MERGE_CASES))}
    for n, (name, shape) in enumerate(sorted(MERGE_CASES.items())):
        rs = np.random.RandomState(2300 + n)
        C = shape[-1]
        m = D.PatchMerging(C).double()
        with torch.no_grad():
            m.norm.weight.copy_(torch.from_numpy(rs.uniform(0.7, 1.3, 4 * C)))
            m.norm.bias.copy_(torch.from_numpy(rs.uniform(-0.2, 0.2, 4 * C)))
            m.reduction.weight.copy_(torch.from_numpy(rs.normal(0.0, (4 * C) ** -0.5, (2 * C, 4 * C))))
        x = torch.from_numpy(rs.normal(0.3, 1.0, shape)).requires_grad_(True)
        y = m(x)
        cot = torch.from_numpy(rs.normal(0.0, 1.0, tuple(y.shape)))
        gx, gw, gb, gr = torch.autograd.grad(y, [x, m.norm.weight, m.norm.bias, m.reduction.weight], cot)
        for k, v in (("x", x), ("norm.weight", m.norm.weight), ("norm.bias", m.norm.bias), ("reduction.weight", m.reduction.weight),
                     ("y", y), ("cot", cot), ("dx", gx), ("dnorm.weight", gw), ("dnorm.bias", gb), ("dreduction.weight", gr)):
            out[f"merge/{name}/{k}"] = v.detach().numpy()
    m = D.DiNAT_s(**NET_CFG).double()
    m.eval()
    assert not m.training
    sd = m.state_dict()
    keys = list(sd.keys())
    shapes = [tuple(v.shape) for v in sd.values()]
    w = wiring_weights(keys, shapes, NET_SEED)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)

    def regrid(module, args, result):                                        # see the module docstring: a view, no arithmetic
        B, H, W, _ = args[0].shape
        return result.view(B, (H + 1) // 2, (W + 1) // 2, result.shape[-1])
    for layer in m.layers:
        if layer.downsample is not None:
            layer.downsample.register_forward_hook(regrid)
    x32 = np.random.RandomState(1000 + NET_SEED).normal(0.0, 1.0, NET_X).astype(np.float32)
    with torch.no_grad():
        ys = m(torch.from_numpy(x32).double())
    out["net/cfg"] = np.array(json.dumps(NET_CFG))
    out["net/seed"] = np.array([NET_SEED])
    out["net/keys"] = np.array(keys)
    out["net/shapes"] = np.array([json.dumps(s) for s in shapes])
    out["net/checksum"] = np.array([[w[k].sum(), (w[k] ** 2).sum()] for k in keys])
    out["net/x"] = x32
    for i, y in zip(NET_CFG["out_indices"], ys):
        out[f"net/y{i}"] = y.numpy()
    path = os.path.join(OUT, "g23_dinats.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), [tuple(y.shape) for y in ys])


if __name__ == "__main__":
    main(sys.argv[1])
