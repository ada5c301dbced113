"""Writes tests/golden/g18_swin.npz from the REFERENCE's own Swin code: SegNet/mmseg/backbones/swin.py and
SegNet/mmseg/models/utils/embed.py, loaded by path, unmodified, as modules of a synthetic package whose mmcv / mmseg imports are
stand-ins:
  mmcv.cnn.build_norm_layer                      -> ("ln", nn.LayerNorm(num_features))  (every config: norm_cfg LN)
  mmcv.cnn.build_conv_layer                      -> nn.Conv2d(*args, **kwargs)           (PatchEmbed's conv_type 'Conv2d')
  mmcv.cnn.bricks.transformer.FFN                -> mmcv 1.4.8's FFN: layers = Sequential(Sequential(Linear, GELU, Dropout), Linear,
                                                    Dropout), forward `identity + dropout_layer(layers(x))`
  mmcv.cnn.bricks.transformer.build_dropout      -> identity (eval mode: DropPath / Dropout do nothing)
  mmcv.runner.BaseModule / ModuleList            -> torch.nn.Module / nn.ModuleList (init_cfg accepted and ignored)
  mmcv.utils.to_2tuple, weight_init functions, _load_checkpoint, get_root_logger, BACKBONES (a registry whose register_module()
  returns the class unchanged)                  -> trivial stand-ins, never on the recorded arithmetic
Everything in float64, eval mode, weights from tests/_oracle_util.py wiring_weights (one deterministic stream per state-dict key;
the fixture stores the key list, shapes and checksums, not the weights).  Outputs are stored in the form of
tests/_swin_golden.py: float32 values plus float64 checksums; the two input images are regenerated, not stored.

Cases: a) embed 64, depths (2,2,2,2), heads (2,4,8,16) on 1 x 3 x 112 x 112 (levels 28, 14, 7, 4: the last padded to 7, shifted);
b) the same network on 1 x 3 x 60 x 92 (every level padded, odd sizes merged with 'corner' padding, non-square);
c) one ShiftWindowMSA (embed 32, 1 head, shift 3) on a 14 x 17 grid with the q / k rows of qkv scaled so that logits reach
   +-60..90: recorded with the reference's -100 mask and with -inf in its place (swin.py:179-253 with the mask value swapped,
   through the module's own window_partition / w_msa / window_reverse); the two differ.

Run from the repository root: python tests/golden/make_swin_fixture.py"""
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
PKG = "_refswin"


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

    def build_norm_layer(cfg, num_features, postfix=""):
        assert cfg["type"] == "LN"
        return "ln" + str(postfix), nn.LayerNorm(num_features)

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
    mod("mmcv.cnn.bricks.transformer", FFN=FFN, build_dropout=build_dropout)
    mod("mmcv.cnn.utils")
    mod("mmcv.cnn.utils.weight_init", constant_init=noop, trunc_normal_=noop, trunc_normal_init=noop)
    mod("mmcv.runner", BaseModule=BaseModule, ModuleList=ModuleList, _load_checkpoint=noop)
    mod("mmcv.runner.base_module", BaseModule=BaseModule)
    mod("mmcv.utils", to_2tuple=to_2tuple)
    mod(PKG)
    mod(PKG + ".utils", get_root_logger=lambda *a, **k: None)
    mod(PKG + ".models")
    mod(PKG + ".models.builder", BACKBONES=_Registry())
    mod(PKG + ".models.utils")
    mod(PKG + ".models.backbones")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def main():
    torch.set_default_dtype(torch.float64)
    _install_stubs()
    _load(PKG + ".models.utils.embed", os.path.join(SEG, "mmseg", "models", "utils", "embed.py"))
    S = _load(PKG + ".models.backbones.swin", os.path.join(SEG, "mmseg", "backbones", "swin.py"))
    sys.path[:0] = [os.path.dirname(OUT), os.path.dirname(os.path.dirname(OUT))]   # tests/ (_oracle_util) and the root (oracle/)
    from _oracle_util import wiring_weights
    from _swin_golden import checksum, image
    out = {}
    cfg = dict(embed_dims=64, depths=(2, 2, 2, 2), num_heads=(2, 4, 8, 16), window_size=7, mlp_ratio=4, drop_path_rate=0.1,
               out_indices=(0, 1, 2, 3))
    seed = 18
    m = S.SwinTransformer(**cfg).double()
    m.eval()                                                             # (SwinTransformer.train returns None, swin.py:621-624)
    sd = m.state_dict()
    keys = list(sd.keys())
    shapes = [tuple(v.shape) for v in sd.values()]
    fkeys = [k for k in keys if not k.endswith("relative_position_index")]
    w = wiring_weights(fkeys, [tuple(sd[k].shape) for k in fkeys], seed)
    m.load_state_dict({**{k: torch.from_numpy(v) for k, v in w.items()}, **{k: sd[k] for k in keys if k not in w}}, strict=True)
    out["net/cfg"] = np.array(json.dumps(cfg))
    out["net/seed"] = np.array([seed])
    out["net/keys"] = np.array(keys)
    out["net/shapes"] = np.array([json.dumps(s) for s in shapes])
    out["net/checksum"] = np.array([[w[k].sum(), (w[k] ** 2).sum()] for k in fkeys])
    out["net/relative_position_index"] = sd["stages.0.blocks.0.attn.w_msa.relative_position_index"].numpy().astype(np.uint8)
    for case in ("a", "b"):
        x = image(case)                                                  # regenerated by the tests (tests/_swin_golden.py)
        with torch.no_grad():
            ys = m(torch.from_numpy(x).double())
        out[f"{case}/x_checksum"] = checksum(x)
        for i, y in enumerate(ys):
            out[f"{case}/y{i}"] = y.numpy().astype(np.float32)
            out[f"{case}/y{i}_checksum"] = checksum(y.numpy())

    # c) one ShiftWindowMSA, large logits
    C, heads, H, W, shift = 32, 1, 14, 17, 3
    a = S.ShiftWindowMSA(C, heads, 7, shift_size=shift).double().eval()
    asd = a.state_dict()
    akeys = [k for k in asd if not k.endswith("relative_position_index")]
    aw = wiring_weights(akeys, [tuple(asd[k].shape) for k in akeys], seed + 1)
    qk_gain = 1.0
    aw["w_msa.qkv.weight"][: 2 * C] *= qk_gain                            # q and k rows: logits of +-60..90
    a.load_state_dict({**{k: torch.from_numpy(v) for k, v in aw.items()}, "w_msa.relative_position_index": asd["w_msa.relative_position_index"]},
                      strict=True)
    # the input: noise plus alpha * v * (-1)^(region row + region column) with v the direction of the most negative q.k form,
    # so that pairs of DIFFERENT regions have the large positive logits (+60..90) and the -100 of the mask decides the output
    Wq, Wk = torch.from_numpy(aw["w_msa.qkv.weight"][:C]), torch.from_numpy(aw["w_msa.qkv.weight"][C:2 * C])
    Mqk = a.w_msa.scale * Wq.T @ Wk
    ev, evec = torch.linalg.eigh(0.5 * (Mqk + Mqk.T))
    alpha = (80.0 / -float(ev[0])) ** 0.5
    Hp0, Wp0 = -(-H // 7) * 7, -(-W // 7) * 7
    lab = lambda y, n: 0 if (y - shift) % n < n - 7 else (1 if (y - shift) % n < n - shift else 2)
    sign = torch.tensor([[(-1.0) ** (lab(i, Hp0) + lab(j, Wp0)) for j in range(W)] for i in range(H)])
    noise = torch.from_numpy(np.random.RandomState(1814).normal(0.0, 0.2, (H, W, C)))
    x = (noise + alpha * sign[..., None] * evec[:, 0]).view(1, H * W, C).float().double()
    with torch.no_grad():
        y100 = a(x, (H, W))
        # swin.py:179-253 with -inf where the reference adds -100, on the module's own pieces
        q = x.view(1, H, W, C)
        Hp, Wp = -(-H // 7) * 7, -(-W // 7) * 7
        q = torch.nn.functional.pad(q, (0, 0, 0, Wp - W, 0, Hp - H))
        sq = torch.roll(q, shifts=(-shift, -shift), dims=(1, 2))
        img = torch.zeros((1, Hp, Wp, 1))
        cnt = 0
        for hs in (slice(0, -7), slice(-7, -shift), slice(-shift, None)):
            for ws in (slice(0, -7), slice(-7, -shift), slice(-shift, None)):
                img[:, hs, ws, :] = cnt
                cnt += 1
        mw = a.window_partition(img).view(-1, 49)
        mask = mw.unsqueeze(1) - mw.unsqueeze(2)
        mask = mask.masked_fill(mask != 0, float("-inf")).masked_fill(mask == 0, 0.0)
        aw_ = a.w_msa(a.window_partition(sq).view(-1, 49, C), mask=mask).view(-1, 7, 7, C)
        yinf = torch.roll(a.window_reverse(aw_, Hp, Wp), shifts=(shift, shift), dims=(1, 2))[:, :H, :W, :].reshape(1, H * W, C)
        qkv = a.w_msa.qkv(a.window_partition(sq).view(-1, 49, C)).view(-1, 49, 3, C)      # the logits inside the windows
        logits = (qkv[:, :, 0] * a.w_msa.scale) @ qkv[:, :, 1].transpose(1, 2)
    assert 60.0 <= float(logits.abs().max()) <= 90.0, float(logits.abs().max())
    d = float((y100 - yinf).abs().max())
    assert d > 1e-3, d
    out["c/cfg"] = np.array(json.dumps(dict(embed_dims=C, num_heads=heads, H=H, W=W, shift=shift, seed=seed + 1, qk_gain=qk_gain)))
    out["c/keys"] = np.array(akeys)
    out["c/checksum"] = np.array([[aw[k].sum(), (aw[k] ** 2).sum()] for k in akeys])
    out["c/x"] = x.numpy().astype(np.float32)
    for key, y in (("c/y_m100", y100), ("c/y_minf", yinf)):
        out[key] = y.view(1, H, W, C).numpy().astype(np.float32)
        out[key + "_checksum"] = checksum(y.numpy())
    out["c/max_abs_diff"] = np.array([d])
    out["c/max_abs_logit"] = np.array([float(logits.abs().max())])
    path = os.path.join(OUT, "g18_swin.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; c: max |logit|", float(logits.abs().max()), "max |y(-100) - y(-inf)|", d)


if __name__ == "__main__":
    main()
