"""Writes tests/golden/g19_uperpup.npz from the REFERENCE's own head: SegNet/mmseg/decode_heads/uper_pup_head.py (the file
decode_heads/__init__.py registers), decode_heads/decode_head.py, decode_heads/psp_head.py and mmseg/ops/wrappers.py, loaded by path,
unmodified, as modules of a synthetic `mmseg` package.  Stand-ins for mmcv (they pin nothing about mmcv itself):
  mmcv.cnn.ConvModule                  -> conv (bias iff no norm), then BatchNorm2d (eval), then ReLU; attribute names conv / bn
  mmcv.runner.BaseModule               -> torch.nn.Module (taking and ignoring init_cfg)
  mmcv.runner.auto_fp16 / force_fp32   -> identity decorator factories
  mmseg.builder.HEADS                  -> a registry whose register_module() returns the class unchanged
  build_loss, accuracy, build_pixel_sampler -> unused stubs (the recorded forward never reaches them)
Everything in float64, eval mode, weights from tests/_uperpup_golden.py head_weights (tests/_oracle_util.py wiring_weights per
state-dict key, BatchNorm running variances mapped to 0.5 .. 1.5; the fixture stores the key list, shapes and checksums, not the
weights).  Logits are stored in the form of tests/_swin_golden.py: float32 values plus float64 checksums; the level features are
regenerated, not stored.

Cases (tests/_uperpup_golden.py CASES): a) NAT-style, num_convs (1, 2, 3, 4), in_channels 16-32-64-128, channels 16, levels 64^2 .. 8^2,
batch 1 (logits 128^2); b) Swin-style and non-square, num_convs (2, 3, 4, 5), levels 16 x 24 .. 2 x 3, batch 2 (logits 64 x 96).
Also the state-dict keys and shapes of the two real config heads (dense NAT / dense Swin: in_channels 128-256-512-1024, channels 256),
built but not run.

Run from the repository root: python tests/golden/make_uperpup_fixture.py"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

OUT = os.path.dirname(os.path.abspath(__file__))
SEG = "/root/reference/SegNet"


def _install_stubs():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__path__ = []
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    class BaseModule(nn.Module):
        def __init__(self, init_cfg=None):
            super().__init__()
            self.init_cfg = init_cfg

    class ConvModule(nn.Module):
        def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias="auto", conv_cfg=None,
                     norm_cfg=None, act_cfg=dict(type="ReLU"), inplace=True, **kwargs):
            super().__init__()
            assert conv_cfg is None and act_cfg == dict(type="ReLU") and not kwargs
            with_norm = norm_cfg is not None
            self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride, padding, dilation, groups,
                                  bias=(not with_norm) if bias == "auto" else bias)
            if with_norm:
                assert norm_cfg["type"] in ("BN", "SyncBN")
                self.bn = nn.BatchNorm2d(out_channels)
            self.activate = nn.ReLU(inplace=inplace)
            self.with_norm = with_norm

        def forward(self, x):
            x = self.conv(x)
            if self.with_norm:
                assert not self.bn.training
                x = self.bn(x)
            return self.activate(x)

    def identity_factory(*a, **k):
        return lambda f: f

    class _Registry:
        def register_module(self, *a, **k):
            return lambda cls: cls

    def unused(*a, **k):
        return None

    mod("mmcv")
    mod("mmcv.cnn", ConvModule=ConvModule)
    mod("mmcv.runner", BaseModule=BaseModule, auto_fp16=identity_factory, force_fp32=identity_factory)
    mod("mmseg")
    mod("mmseg.core", build_pixel_sampler=unused)
    mod("mmseg.builder", HEADS=_Registry(), build_loss=unused)
    mod("mmseg.losses", accuracy=unused)
    mod("mmseg.ops")
    mod("mmseg.decode_heads")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def _head(P, num_convs, in_channels, channels):
    return P.UPerPUPHead(num_convs=num_convs, up_scale=2, pool_scales=(1, 2, 3, 6), in_channels=list(in_channels), in_index=[0, 1, 2, 3],
                         channels=channels, dropout_ratio=0.1, num_classes=2, norm_cfg=dict(type="SyncBN", requires_grad=True),
                         align_corners=False, loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0))


def main():
    torch.set_default_dtype(torch.float64)
    _install_stubs()
    W = _load("mmseg.ops.wrappers", os.path.join(SEG, "mmseg", "ops", "wrappers.py"))
    sys.modules["mmseg.ops"].resize, sys.modules["mmseg.ops"].Upsample = W.resize, W.Upsample
    _load("mmseg.decode_heads.decode_head", os.path.join(SEG, "mmseg", "decode_heads", "decode_head.py"))
    _load("mmseg.decode_heads.psp_head", os.path.join(SEG, "mmseg", "decode_heads", "psp_head.py"))
    P = _load("mmseg.decode_heads.uper_pup_head", os.path.join(SEG, "mmseg", "decode_heads", "uper_pup_head.py"))
    sys.path[:0] = [os.path.dirname(os.path.dirname(OUT))]                # the repository root (tests._oracle_util, tests._swin_golden)
    from tests._swin_golden import checksum
    from tests._uperpup_golden import CASES, REAL, features, head_weights
    out = {}
    for case, (num_convs, in_channels, channels, B, sizes, seed) in CASES.items():
        m = _head(P, num_convs, in_channels, channels).double().eval()
        sd = m.state_dict()
        keys = [k for k in sd if not k.endswith("num_batches_tracked")]
        w = head_weights(keys, [tuple(sd[k].shape) for k in keys], seed)
        m.load_state_dict({**{k: torch.from_numpy(v) for k, v in w.items()}, **{k: sd[k] for k in sd if k not in w}}, strict=True)
        xs = features(case)
        with torch.no_grad():
            y = m([torch.from_numpy(x).double() for x in xs])
        out[f"{case}/keys"] = np.array(keys)
        out[f"{case}/shapes"] = np.array([json.dumps(list(sd[k].shape)) for k in keys])
        out[f"{case}/checksum"] = np.array([[w[k].sum(), (w[k] ** 2).sum()] for k in keys])
        out[f"{case}/x_checksum"] = np.stack([checksum(x) for x in xs])
        out[f"{case}/y"] = y.numpy().astype(np.float32)
        out[f"{case}/y_checksum"] = checksum(y.numpy())
        print(case, tuple(y.shape), "max |y|", float(y.abs().max()))
    for name, num_convs in REAL.items():
        sd = _head(P, num_convs, (128, 256, 512, 1024), 256).state_dict()
        out[f"real_{name}/keys"] = np.array(list(sd))
        out[f"real_{name}/shapes"] = np.array([json.dumps(list(v.shape)) for v in sd.values()])
    path = os.path.join(OUT, "g19_uperpup.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
