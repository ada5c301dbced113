"""Writes tests/golden/g22_dice.npz from the REFERENCE's own loss: SegNet/mmseg/models/losses/dice_loss.py and
models/losses/utils.py, loaded by path, unmodified, as modules of a synthetic `mmseg` package, with make_ohem_fixture.py's stand-ins
(they pin nothing about mmcv itself):
  mmseg.models.builder.LOSSES -> a registry whose register_module() returns the class unchanged
  mmcv                        -> an empty module (utils.py imports it for weight FILES only)
The loss is called as BaseDecodeHead.losses calls it (decode_head.py:246-262): DiceLoss(...)(logit, label, weight=seg_weight,
ignore_index=255) — both keyword arguments fall into **kwards and are unused, which the writer asserts by passing a weight of zeros.
Everything in float64; the file stores numbers only.

Per case: full-resolution logits [2, C, 12, 20] (make_ohem_fixture.py's: randn * 1.5, + 2 on the label's channel), labels with about
20 % ignored, the loss's arguments, and what the reference returns: the loss and its autograd gradient w.r.t. the logits.
  plain_cC      C in {2, 3, 5}: smooth 1, no class weights
  cw_cC         C in {2, 3, 5}: class weights 0.5 + 0.75 i
  smooth_cC     C in {2, 3, 5}: smooth 0.5
  lw3_c3        loss_weight 3, class weights
  allign_c2/5   every label ignored
  ign1_c3       ignore_index = 1, the skipped class: the ignored labels ARE 1 (no 255: the reference would clamp it to a valid class 2,
                this build ignores every out-of-range label — the one case where the two rules part)
  exp1_c3       exponent 1 (the torch form only; the kernels are exponent 2)

Run from the repository root: python tests/golden/make_dice_fixture.py <path of the reference's SegNet directory>"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
B, H, W = 2, 12, 20


def _install_stubs():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__path__ = []
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    class _Registry:
        def register_module(self, *a, **k):
            return lambda cls: cls

    mod("mmcv")
    for name in ("mmseg", "mmseg.models", "mmseg.models.losses"):
        mod(name)
    mod("mmseg.models.builder", LOSSES=_Registry())


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def _inputs(C, seed, ignore=255, all_ignored=False):
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, C, (B, H, W), generator=g)
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * 1.5
    x.scatter_add_(1, lab.unsqueeze(1), torch.full((B, 1, H, W), 2.0, dtype=torch.float64))
    lab[torch.rand(B, H, W, generator=g) < 0.2] = ignore
    if all_ignored:
        lab[:] = ignore
    return x, lab


def main():
    seg = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PPNET_REFERENCE_SEGNET")
    if not seg or not os.path.isdir(os.path.join(seg, "mmseg")):
        sys.exit(__doc__.strip().splitlines()[-1])
    torch.set_default_dtype(torch.float64)
    _install_stubs()
    _load("mmseg.models.losses.utils", os.path.join(seg, "mmseg", "models", "losses", "utils.py"))
    D = _load("mmseg.models.losses.dice_loss", os.path.join(seg, "mmseg", "models", "losses", "dice_loss.py"))
    #        name: (C, class weights, smooth, exponent, loss_weight, ignore_index, all ignored)
    cases = {}
    for C in (2, 3, 5):
        cases[f"plain_c{C}"] = (C, False, 1, 2, 1.0, 255, False)
        cases[f"cw_c{C}"] = (C, True, 1, 2, 1.0, 255, False)
        cases[f"smooth_c{C}"] = (C, False, 0.5, 2, 1.0, 255, False)
    cases["lw3_c3"] = (3, True, 1, 2, 3.0, 255, False)
    cases["allign_c2"] = (2, False, 1, 2, 1.0, 255, True)
    cases["allign_c5"] = (5, True, 1, 2, 1.0, 255, True)
    cases["ign1_c3"] = (3, True, 1, 2, 1.0, 1, False)
    cases["exp1_c3"] = (3, True, 1, 1, 1.0, 255, False)
    out, names = {}, []
    for i, (name, (C, weighted, smooth, exponent, lw, ignore, all_ignored)) in enumerate(cases.items()):
        x, lab = _inputs(C, 2200 + 10 * C + i, ignore, all_ignored)
        cw = [0.5 + 0.75 * c for c in range(C)] if weighted else None
        mod = D.DiceLoss(smooth=smooth, exponent=exponent, class_weight=cw, loss_weight=lw, ignore_index=ignore)
        xr = x.clone().requires_grad_(True)
        loss = mod(xr, lab, weight=torch.zeros(B, H, W), ignore_index=255)       # as the head calls it: both land in **kwards
        grad, = torch.autograd.grad(loss, xr)
        assert float(loss.detach()) == float(mod(x, lab)) and float(loss.detach()) > 0.0 and mod.loss_name == "loss_dice"
        assert all_ignored == bool((lab == ignore).all()) and (all_ignored or 0.1 < float((lab == ignore).double().mean()) < 0.6)
        names.append(name)
        out[f"{name}/logit"] = x.numpy()
        out[f"{name}/label"] = lab.numpy().astype(np.float64)
        out[f"{name}/class_weight"] = np.array(cw if cw else [], dtype=np.float64)
        out[f"{name}/args"] = np.array([smooth, exponent, lw, ignore], dtype=np.float64)      # smooth, exponent, loss_weight, ignore_index
        out[f"{name}/loss"] = np.float64(float(loss.detach()))
        out[f"{name}/grad"] = grad.numpy()
        print(name, "ignored", int((lab == ignore).sum()), "loss", float(loss.detach()), "max |grad|", float(grad.abs().max()))
    out["cases"] = np.array([[ord(ch) for ch in n.ljust(16)] for n in names], dtype=np.float64)     # names as character codes: numbers only
    path = os.path.join(OUT, "g22_dice.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
