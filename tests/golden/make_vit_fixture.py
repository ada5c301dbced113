"""Writes tests/golden/g20_vit.npz from the REFERENCE's own ViT code: SegNet/mmseg/backbones/vit.py, SegNet/mmseg/models/utils/embed.py
and SegNet/mmseg/ops/wrappers.py, loaded by path, unmodified, as modules of a synthetic package whose mmcv / mmseg imports are
stand-ins:
  mmcv.cnn.build_norm_layer                      -> ("ln" + postfix, nn.LayerNorm(num_features, eps=cfg.get("eps", 1e-5)))
  mmcv.cnn.build_conv_layer                      -> nn.Conv2d(*args, **kwargs)           (PatchEmbed's conv_type 'Conv2d')
  mmcv.cnn.bricks.transformer.MultiheadAttention -> mmcv 1.4.8's wrapper: attn = nn.MultiheadAttention(embed_dims, num_heads, attn_drop,
                                                    bias=...), batch-first inputs transposed to sequence-first and back, forward
                                                    `identity + dropout_layer(proj_drop(out))`
  mmcv.cnn.bricks.transformer.FFN                -> mmcv 1.4.8's FFN: layers = Sequential(Sequential(Linear, GELU, Dropout), Linear,
                                                    Dropout), forward `identity + dropout_layer(layers(x))`
  mmcv.cnn.bricks.transformer.build_dropout      -> identity (eval mode: DropPath / Dropout do nothing)
  mmcv.runner.BaseModule / ModuleList            -> torch.nn.Module / nn.ModuleList (init_cfg accepted and ignored)
  mmcv.utils.to_2tuple, weight_init functions, _load_checkpoint, get_root_logger, BACKBONES (a registry whose register_module()
  returns the class unchanged)                  -> trivial stand-ins, never on the recorded arithmetic
  mmseg.ops.resize                               -> the reference's own ops/wrappers.py (F.interpolate), loaded by path
These stand-ins pin nothing about mmcv itself: they are what the recorded arithmetic assumes mmcv does.
Everything in float64, eval mode, weights from tests/_oracle_util.py wiring_weights (one deterministic stream per state-dict key;
the fixture stores the key list, shapes and checksums, not the weights).  Outputs are stored in the form of tests/_vit_golden.py:
float32 values plus float64 checksums; the input images are regenerated, not stored.

Cases: a) img_size 64, patch 16, embed 128, 2 heads of 64, 3 layers, no cls token, out_indices (1, 2) on 1 x 3 x 64 x 64 (the
stored grid), 1 x 3 x 96 x 128 (bicubic pos_embed resize, non-square) and 1 x 3 x 70 x 50 ('corner' padding to 80 x 64);
b) the same network with with_cls_token, final_norm and patch_norm, on the same three inputs;
c) one TransformerEncoderLayer (embed 128, 2 heads) on 40 tokens with the q / k rows of in_proj_weight scaled so that the
   logits reach +-60..90;
d) the key list and shapes of the real ViT-B VisionTransformer (configs/vit/vit_base.py over _base_/models/vit.py), no weights.

Run from the repository root: python tests/golden/make_vit_fixture.py"""
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
PKG = "_refvit"


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

    class ModuleList(nn.ModuleList):
        def __init__(self, modules=None, init_cfg=None):
            super().__init__(modules)

    class _Identity(nn.Module):
        def forward(self, x):
            assert not self.training
            return x

    def build_dropout(cfg):
        return _Identity()

    class FFN(BaseModule):                                              # mmcv 1.4.8 cnn/bricks/transformer.py FFN
        def __init__(self, embed_dims=256, feedforward_channels=1024, num_fcs=2, act_cfg=dict(type="ReLU", inplace=True), ffn_drop=0.0,
                     dropout_layer=None, add_identity=True, init_cfg=None, **kwargs):
            super().__init__(init_cfg)
            assert num_fcs >= 2 and act_cfg["type"] == "GELU"
            layers, cin = [], embed_dims
            for _ in range(num_fcs - 1):
                layers.append(nn.Sequential(nn.Linear(cin, feedforward_channels), nn.GELU(), nn.Dropout(ffn_drop)))
                cin = feedforward_channels
            layers.append(nn.Linear(feedforward_channels, embed_dims))
            layers.append(nn.Dropout(ffn_drop))
            self.layers = nn.Sequential(*layers)
            self.dropout_layer = build_dropout(dropout_layer) if dropout_layer else nn.Identity()
            self.add_identity = add_identity

        def forward(self, x, identity=None):
            out = self.layers(x)
            if not self.add_identity:
                return self.dropout_layer(out)
            if identity is None:
                identity = x
            return identity + self.dropout_layer(out)

    class MultiheadAttention(BaseModule):                               # mmcv 1.4.8 cnn/bricks/transformer.py MultiheadAttention
        def __init__(self, embed_dims, num_heads, attn_drop=0.0, proj_drop=0.0, dropout_layer=dict(type="Dropout", drop_prob=0.0),
                     init_cfg=None, batch_first=False, **kwargs):
            super().__init__(init_cfg)
            self.embed_dims, self.num_heads, self.batch_first = embed_dims, num_heads, batch_first
            self.attn = nn.MultiheadAttention(embed_dims, num_heads, attn_drop, **kwargs)
            self.proj_drop = nn.Dropout(proj_drop)
            self.dropout_layer = build_dropout(dropout_layer) if dropout_layer else nn.Identity()

        def forward(self, query, key=None, value=None, identity=None, query_pos=None, key_pos=None, attn_mask=None, key_padding_mask=None,
                    **kwargs):
            if key is None:
                key = query
            if value is None:
                value = key
            if identity is None:
                identity = query
            assert query_pos is None and key_pos is None
            if self.batch_first:
                query, key, value = query.transpose(0, 1), key.transpose(0, 1), value.transpose(0, 1)
            out = self.attn(query=query, key=key, value=value, attn_mask=attn_mask, key_padding_mask=key_padding_mask)[0]
            if self.batch_first:
                out = out.transpose(0, 1)
            return identity + self.dropout_layer(self.proj_drop(out))

    def build_norm_layer(cfg, num_features, postfix=""):
        assert cfg["type"] == "LN"
        return "ln" + str(postfix), nn.LayerNorm(num_features, eps=cfg.get("eps", 1e-5))

    def build_conv_layer(cfg, *args, **kwargs):
        assert cfg is None or cfg.get("type", "Conv2d") == "Conv2d"
        return nn.Conv2d(*args, **kwargs)

    def to_2tuple(x):
        return tuple(x) if isinstance(x, (tuple, list)) else (x, x)

    class _Registry:
        def register_module(self, *a, **k):
            return lambda cls: cls

    noop = lambda *a, **k: None
    mod("mmcv")
    mod("mmcv.cnn", build_norm_layer=build_norm_layer, build_conv_layer=build_conv_layer)
    mod("mmcv.cnn.bricks")
    mod("mmcv.cnn.bricks.transformer", FFN=FFN, MultiheadAttention=MultiheadAttention, build_dropout=build_dropout)
    mod("mmcv.cnn.utils")
    mod("mmcv.cnn.utils.weight_init", constant_init=noop, kaiming_init=noop, trunc_normal_=noop)
    mod("mmcv.runner", BaseModule=BaseModule, ModuleList=ModuleList, _load_checkpoint=noop)
    mod("mmcv.runner.base_module", BaseModule=BaseModule)
    mod("mmcv.utils", to_2tuple=to_2tuple)
    mod("mmseg")
    mod("mmseg.utils", get_root_logger=lambda *a, **k: None)
    mod(PKG)
    mod(PKG + ".builder", BACKBONES=_Registry())
    mod(PKG + ".backbones")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def _seeded(m, seed, tweak=None):
    sd = m.state_dict()
    keys = list(sd.keys())
    w = wiring_weights(keys, [tuple(v.shape) for v in sd.values()], seed)
    if tweak is not None:
        tweak(w)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    return keys, w


def main():
    global wiring_weights
    torch.set_default_dtype(torch.float64)
    _install_stubs()
    wr = _load("mmseg.ops", os.path.join(SEG, "mmseg", "ops", "wrappers.py"))
    assert wr.resize is not None
    embed = _load(PKG + ".utils", os.path.join(SEG, "mmseg", "models", "utils", "embed.py"))
    assert embed.PatchEmbed is not None
    V = _load(PKG + ".backbones.vit", os.path.join(SEG, "mmseg", "backbones", "vit.py"))
    sys.path[:0] = [os.path.dirname(OUT), os.path.dirname(os.path.dirname(OUT))]   # tests/ (_oracle_util) and the root
    from _oracle_util import wiring_weights
    from tests._vit_golden import SMALL, SMALL_CLS, attn_tokens, checksum, image
    out = {}
    for net, cfg, seed in (("a", SMALL, 20), ("b", SMALL_CLS, 21)):
        m = V.VisionTransformer(**cfg).double()
        m.eval()                                                         # (VisionTransformer.train returns None, vit.py:407-412)
        keys, w = _seeded(m, seed)
        out[f"{net}/cfg"] = np.array(json.dumps(cfg))
        out[f"{net}/seed"] = np.array([seed])
        out[f"{net}/keys"] = np.array(keys)
        out[f"{net}/shapes"] = np.array([json.dumps(tuple(w[k].shape)) for k in keys])
        out[f"{net}/checksum"] = np.array([[w[k].sum(), (w[k] ** 2).sum()] for k in keys])
        for case in ("a64", "a96", "a70"):
            x = image(case)
            with torch.no_grad():
                ys = m(torch.from_numpy(x).double())
            out[f"{net}/{case}/x_checksum"] = checksum(x)
            assert len(ys) == 2
            for i, y in enumerate(ys):
                out[f"{net}/{case}/y{i}"] = y.numpy().astype(np.float32)
                out[f"{net}/{case}/y{i}_checksum"] = checksum(y.numpy())

    # c) one encoder layer, logits of +-60..90
    C, heads, n = 128, 2, 40
    layer = V.TransformerEncoderLayer(C, heads, 4 * C, batch_first=True).double().eval()
    x = torch.from_numpy(attn_tokens(n, C)).double()
    keys, w = _seeded(layer, 22)
    with torch.no_grad():
        def logits(ww):
            y = layer.ln1(x)[0]
            q = y @ torch.from_numpy(ww["attn.attn.in_proj_weight"][:C]).T + torch.from_numpy(ww["attn.attn.in_proj_bias"][:C])
            k = y @ torch.from_numpy(ww["attn.attn.in_proj_weight"][C:2 * C]).T + torch.from_numpy(ww["attn.attn.in_proj_bias"][C:2 * C])
            return torch.stack([(q[:, 64 * h:64 * h + 64] @ k[:, 64 * h:64 * h + 64].T) * 64 ** -0.5 for h in range(heads)])
        gain = float((75.0 / float(logits(w).abs().max())) ** 0.5)

        def tweak(ww):
            ww["attn.attn.in_proj_weight"][: 2 * C] *= gain
            ww["attn.attn.in_proj_bias"][: 2 * C] *= gain
        keys, w = _seeded(layer, 22, tweak)
        lg = logits(w)
        y = layer(x)
    assert 60.0 <= float(lg.abs().max()) <= 90.0, float(lg.abs().max())
    out["c/cfg"] = np.array(json.dumps(dict(embed_dims=C, num_heads=heads, tokens=n, seed=22, qk_gain=gain)))
    out["c/keys"] = np.array(keys)
    out["c/checksum"] = np.array([[w[k].sum(), (w[k] ** 2).sum()] for k in keys])
    out["c/y"] = y.numpy().astype(np.float32)
    out["c/y_checksum"] = checksum(y.numpy())
    out["c/max_abs_logit"] = np.array([float(lg.abs().max())])

    # d) ViT-B / 16 as VIT_BASE_SETRUP builds it: keys and shapes only
    torch.set_default_dtype(torch.float32)
    vb = V.VisionTransformer(img_size=224, patch_size=16, in_channels=3, embed_dims=768, num_layers=12, num_heads=12, drop_rate=0.0,
                             norm_cfg=dict(type="LN", eps=1e-6, requires_grad=True), with_cls_token=False)
    sd = vb.state_dict()
    out["d/keys"] = np.array(list(sd.keys()))
    out["d/shapes"] = np.array([json.dumps(tuple(v.shape)) for v in sd.values()])
    out["d/ln_eps"] = np.array([vb.layers[0].ln1.eps])
    path = os.path.join(OUT, "g20_vit.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; c: max |logit|", float(lg.abs().max()), "gain", gain)


if __name__ == "__main__":
    main()
