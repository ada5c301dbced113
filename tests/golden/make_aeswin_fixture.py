"""Writes tests/golden/g25_aeswin.npz from the REFERENCE's own AESwin: GenNet/networks/ae_swin.py on vanilla_swin.py and base.py,
imported unmodified from a checkout of the reference; the only stand-in is an empty `cv2` module (utils/ imports it, nothing on the
recorded path calls it).  The fixture holds numbers only.

The model: AESwin(1, 1, 128, 24) under torch.manual_seed(0), every relative_position_bias_table redrawn at std 0.5 (so that the
bias matters), non-trivial BatchNorm statistics (so that eval-mode folding is exercised), and every floating-point state-dict
entry rounded to the nearest bfloat16 value BEFORE anything is computed: the stored float32 weights are exactly what the
reference ran, and the archive stays below the repository's 1 MiB limit per file (259 705 float32 parameters alone are 1.04 MB).
Recorded:
  keys                 the 247 state-dict keys in the reference's order
  w/<key>              the state dict, float32 (relative_position_index as int16)
  x128, x112           two binary {0, 255} inputs [2,1,R,R], uint8: R = 128 (token grids 64 / 32 / 16: every stage padded) and
                       R = 112 (56 / 28 / 14: none padded; the same weights, down_time is 1 for both)
  y128, y112           the reference's eval-mode float64 outputs, stored as float32
  blk_in, blk_out      input and output [1024,24] of swin.1.blocks.1 (window 14, shift 7, 32 x 32 grid padded to 42 x 42) for
                       sample 0 of x128, float64 stored as float32

Run from the repository root: PPNET_REFERENCE=<checkout of the reference> python tests/golden/make_aeswin_fixture.py"""
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    ref = os.environ.get("PPNET_REFERENCE")
    if not ref or not os.path.isdir(os.path.join(ref, "GenNet", "networks")):
        sys.exit("set PPNET_REFERENCE to a checkout of the reference (the directory that holds GenNet/)")
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.path.insert(0, os.path.join(ref, "GenNet"))
    from networks.ae_swin import AESwin
    torch.manual_seed(0)
    m = AESwin(1, 1, 128, 24).eval()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("relative_position_bias_table"):
                p.normal_(0.0, 0.5)
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.uniform_(-0.2, 0.2)
                mod.running_var.uniform_(0.5, 1.5)
                mod.weight.uniform_(0.8, 1.2)
                mod.bias.uniform_(-0.1, 0.1)
        for v in m.state_dict().values():
            if v.is_floating_point():
                v.copy_(v.to(torch.bfloat16).float())
    sd = m.state_dict()
    out = {"keys": np.array(list(sd.keys()))}
    for k, v in sd.items():
        out["w/" + k] = v.numpy().astype(np.int16) if k.endswith("relative_position_index") else v.numpy().astype(np.float32)
    m64 = AESwin(1, 1, 128, 24).double().eval()
    m64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, strict=True)
    kept = {}
    hook = m64.swin[1].blocks[1].register_forward_hook(lambda mod, a, o: kept.update(blk_in=a[0].detach(), blk_out=o.detach()))
    for R in (128, 112):
        x = ((torch.rand(2, 1, R, R) > 0.5) * 255).to(torch.uint8)
        with torch.no_grad():
            y = m64(x.double())
        out[f"x{R}"] = x.numpy()
        out[f"y{R}"] = y.numpy().astype(np.float32)
        if R == 128:
            out["blk_in"] = kept["blk_in"][0].numpy().astype(np.float32)
            out["blk_out"] = kept["blk_out"][0].numpy().astype(np.float32)
    hook.remove()
    path = os.path.join(OUT, "g25_aeswin.npz")
    np.savez_compressed(path, **out)
    n = sum(p.numel() for p in m.parameters())
    print(path, os.path.getsize(path), "bytes;", len(sd), "state-dict entries,", n, "parameters; max |y128|", float(np.abs(out["y128"]).max()),
          "max |y112|", float(np.abs(out["y112"]).max()))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
