"""Writes tests/golden/g24_dinat_l_tiny.npz and g24_dinat_l_tiny_y0.npz: the reference's DiNAT (SegNet/dinat.py over SegNet/nat.py) at
DiNAT-L's width ratios (embed a multiple of 3 * 32: every level's width is 3 * 2^k * 8), in float64, eval mode.

SegNet/nat.py and SegNet/dinat.py are loaded by path, UNMODIFIED, with the stand-ins of make_fixtures.py's _install_segnet_stubs (the
same ones fixture_nat_wiring uses): timm.models.layers.DropPath = identity, mmcv.runner.load_checkpoint, mmseg.utils.get_root_logger,
mmseg.models.builder.BACKBONES, and natten.NeighborhoodAttention2D = oracle.segnet_ref.na_fp64 (the attention op itself stays "parity
unpinned", as in g16).  Numbers only.

One case, "dinat_l_tiny": DiNAT(embed_dim=96, mlp_ratio=2.0, depths=[1, 2, 1, 1], num_heads=[3, 6, 12, 24], kernel_size=7,
dilations=[[1], [1, 2], [1], [1]], out_indices=(0, 1, 2, 3), layer_scale=None, drop_path_rate=0.3) — no LayerScale, as
configs/dinat/dinat_large.py sets none — on a (2, 3, 64, 96) float32-representable input: levels of width 96 / 192 / 384 / 768 on grids
16 x 24, 8 x 12 (its d = 2 layer is padded to 14), 4 x 6 and 2 x 3 (both padded to 7).  Weights from tests/_oracle_util.wiring_weights;
stored, as g16 does: the constructor arguments, state-dict key order / shapes / checksums, the input and the four float64 outputs.  The
outputs are 1.1 MB of float64 that does not compress, so level 0's lies in a file of its own (no committed file above 1 MiB).

Run from the repository root:  python tests/golden/make_dinat_l_fixture.py <path to the reference's SegNet directory>"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))

NAME = "dinat_l_tiny"
CFG = dict(embed_dim=96, mlp_ratio=2.0, depths=[1, 2, 1, 1], num_heads=[3, 6, 12, 24], kernel_size=7, dilations=[[1], [1, 2], [1], [1]],
           out_indices=(0, 1, 2, 3), layer_scale=None, drop_path_rate=0.3)
X_SHAPE, SEED = (2, 3, 64, 96), 24


def load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def main(seg):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), OUT]
    from make_fixtures import _install_segnet_stubs
    from _oracle_util import wiring_weights
    _install_segnet_stubs()
    load_by_path("nat", os.path.join(seg, "nat.py"))                         # dinat.py imports NAT from it
    D = load_by_path("dinat", os.path.join(seg, "dinat.py"))
    m = D.DiNAT(**CFG).double()
    m.eval()                                                                 # (NAT.train returns None: no chaining)
    assert not m.training
    sd = m.state_dict()
    keys = list(sd.keys())
    shapes = [tuple(v.shape) for v in sd.values()]
    w = wiring_weights(keys, shapes, SEED)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    x32 = np.random.RandomState(1000 + SEED).normal(0.0, 1.0, X_SHAPE).astype(np.float32)
    with torch.no_grad():
        ys = m(torch.from_numpy(x32).double())
    out = {"cases": np.array([NAME]), f"{NAME}/cfg": np.array(json.dumps(CFG)), f"{NAME}/seed": np.array([SEED]),
           f"{NAME}/keys": np.array(keys), f"{NAME}/shapes": np.array([json.dumps(s) for s in shapes]),
           f"{NAME}/checksum": np.array([[w[k].sum(), (w[k] ** 2).sum()] for k in keys]), f"{NAME}/x": x32}
    big = {}
    for i, y in zip(CFG["out_indices"], ys):
        (big if i == 0 else out)[f"{NAME}/y{i}"] = y.numpy()
    for fname, d in (("g24_dinat_l_tiny.npz", out), ("g24_dinat_l_tiny_y0.npz", big)):
        path = os.path.join(OUT, fname)
        np.savez_compressed(path, **d)
        print(path, os.path.getsize(path))
    print([tuple(y.shape) for y in ys])


if __name__ == "__main__":
    main(sys.argv[1])
