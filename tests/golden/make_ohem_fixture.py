"""Writes tests/golden/g21_ohem.npz from the REFERENCE's own sampler and loss: SegNet/mmseg/core/seg/sampler/ohem_pixel_sampler.py,
core/seg/sampler/base_pixel_sampler.py, models/losses/cross_entropy_loss.py and models/losses/utils.py, loaded by path, unmodified, as
modules of a synthetic `mmseg` package.  Stand-ins (they pin nothing about mmcv itself):
  mmseg.core.seg.builder.PIXEL_SAMPLERS, mmseg.models.builder.LOSSES -> registries whose register_module() returns the class unchanged
  mmcv                                                               -> an empty module (utils.py imports it for weight FILES only)
The sampler's `context` is an object with ignore_index = 255 and loss_decode = the reference's CrossEntropyLoss(class_weight,
loss_weight=1.0).  Everything in float64; the file stores numbers only.

Per case: full-resolution logits [2, C, 12, 20] (randn * 1.5, + 2 on the label's channel: a head that is mostly right), labels with
about 20 % at 255, the sampler's arguments, the class weights, and what the reference returns — seg_weight = sampler.sample(logit,
label[:, None]) and loss = CrossEntropyLoss(...)(logit, label, weight=seg_weight, ignore_index=255).  For C in {2, 5}:
  a  thresh 0.7, min_kept 20     the 40th smallest probability is below 0.7: the threshold is 0.7
  b  thresh 0.7, min_kept 150    the 300th smallest probability is above 0.7: the threshold is that probability
  c  thresh 0.7, min_kept 1000   batch_kept >= n_valid: the largest probability is the candidate
  d  thresh 0.7 / None           every label ignored: all weights 0
  e  thresh None, min_kept 30    the 60 largest losses
  f  a and e again with class weights
The writer asserts each case's condition, and that no other score lies within 1e-9 of the cut: ties play no part, so the reference's
unstable sort and this build's keep-all-ties rule select the same pixels.

Run from the repository root: python tests/golden/make_ohem_fixture.py <path of the reference's SegNet directory>"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
B, H, W, IGNORE = 2, 12, 20, 255


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
    for name in ("mmseg", "mmseg.core", "mmseg.core.seg", "mmseg.core.seg.sampler", "mmseg.models", "mmseg.models.losses"):
        mod(name)
    mod("mmseg.core.seg.builder", PIXEL_SAMPLERS=_Registry())
    mod("mmseg.models.builder", LOSSES=_Registry())


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def _inputs(C, seed, all_ignored=False):
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, C, (B, H, W), generator=g)
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * 1.5
    x.scatter_add_(1, lab.unsqueeze(1), torch.full((B, 1, H, W), 2.0, dtype=torch.float64))
    lab[torch.rand(B, H, W, generator=g) < 0.2] = IGNORE
    if all_ignored:
        lab[:] = IGNORE
    return x, lab


def main():
    seg = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PPNET_REFERENCE_SEGNET")
    if not seg or not os.path.isdir(os.path.join(seg, "mmseg")):
        sys.exit(__doc__.strip().splitlines()[-1])
    torch.set_default_dtype(torch.float64)
    _install_stubs()
    _load("mmseg.core.seg.sampler.base_pixel_sampler", os.path.join(seg, "mmseg", "core", "seg", "sampler", "base_pixel_sampler.py"))
    S = _load("mmseg.core.seg.sampler.ohem_pixel_sampler", os.path.join(seg, "mmseg", "core", "seg", "sampler", "ohem_pixel_sampler.py"))
    _load("mmseg.models.losses.utils", os.path.join(seg, "mmseg", "models", "losses", "utils.py"))
    L = _load("mmseg.models.losses.cross_entropy_loss", os.path.join(seg, "mmseg", "models", "losses", "cross_entropy_loss.py"))
    #        thresh min_kept class weights  all ignored
    kinds = {"a": (0.7, 20, False, False), "b": (0.7, 150, False, False), "c": (0.7, 1000, False, False), "d1": (0.7, 20, False, True),
             "d2": (None, 20, False, True), "e": (None, 30, False, False), "fa": (0.7, 20, True, False), "fe": (None, 30, True, False)}
    out, names = {}, []
    for C in (2, 5):
        for i, (kind, (thresh, min_kept, weighted, all_ignored)) in enumerate(kinds.items()):
            name = f"{kind}_c{C}"
            x, lab = _inputs(C, 1000 * C + i, all_ignored)
            cw = [0.5 + 0.75 * c for c in range(C)] if weighted else None
            loss_mod = L.CrossEntropyLoss(use_sigmoid=False, class_weight=cw, loss_weight=1.0)
            ctx = types.SimpleNamespace(ignore_index=IGNORE, loss_decode=loss_mod)
            sampler = S.OHEMPixelSampler(ctx, thresh=thresh, min_kept=min_kept)
            weight = sampler.sample(x, lab.unsqueeze(1))
            loss = loss_mod(x, lab, weight=weight, ignore_index=IGNORE)
            # the case's condition, and no score within 1e-9 of the cut but the cut itself
            valid = lab != IGNORE
            n_valid, kept = int(valid.sum()), min_kept * B
            assert (n_valid == 0) == all_ignored and int(weight.sum()) == int(weight[valid].sum())
            if n_valid:
                if thresh is not None:
                    p = torch.softmax(x, 1).gather(1, lab.clamp(max=C - 1).unsqueeze(1)).squeeze(1)[valid].sort().values
                    kth = float(p[min(kept, n_valid - 1)])
                    cut = max(kth, thresh)
                    assert {"a": kth < thresh, "fa": kth < thresh, "b": kth > thresh and kept < n_valid - 1, "c": kept >= n_valid}[kind], (name, kth)
                    near = int(((p - cut).abs() < 1e-9).sum())
                    assert near == (1 if cut == kth else 0), (name, near)
                    assert int(weight.sum()) == int((p < cut).sum()) and (kind != "c" or int(weight.sum()) == n_valid - 1)
                else:
                    s = loss_mod(x, lab, ignore_index=IGNORE, reduction_override="none")[valid].sort(descending=True).values
                    assert kept < n_valid and int(((s - s[kept - 1]).abs() < 1e-9).sum()) == 1, name
                    assert int(weight.sum()) == kept
            else:
                assert float(weight.sum()) == 0.0 and float(loss) == 0.0
            names.append(name)
            out[f"{name}/logit"] = x.numpy()
            out[f"{name}/label"] = lab.numpy().astype(np.int64)
            out[f"{name}/thresh"] = np.float64(np.nan if thresh is None else thresh)
            out[f"{name}/min_kept"] = np.int64(min_kept)
            out[f"{name}/class_weight"] = np.array(cw if cw else [], dtype=np.float64)
            out[f"{name}/seg_weight"] = weight.numpy().astype(np.float64)
            out[f"{name}/loss"] = np.float64(float(loss))
            print(name, "n_valid", n_valid, "kept", int(weight.sum()), "loss", float(loss))
    out["cases"] = np.array(names)
    path = os.path.join(OUT, "g21_ohem.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
