"""Vision Transformer backbone (reference SegNet/mmseg/backbones/vit.py:21-412, mmseg/models/utils/embed.py:12-204) with mmseg's
constructor arguments and state-dict layout (`patch_embed.{projection,norm}`, `cls_token`, `pos_embed`, `layers.i.{ln1,ln2}`,
`layers.i.attn.attn.{in_proj_weight,in_proj_bias,out_proj}` — mmcv's MultiheadAttention around nn.MultiheadAttention —,
`layers.i.ffn.layers.{0.0,1}`, `ln1` with final_norm), so an mmseg ViT checkpoint loads unchanged.

Two forms of the same arithmetic:
* GPU inference (CUDA tensors, no autograd): the qkv / out / MLP projections on the build's GEMMs where their gates pass
  (dense.linear, bias and GELU in the float32 epilogue; each branch joins the residual stream in one add), the global attention
  kernel ppn_mhsa_fwd between in_proj and out_proj.  The LayerNorm kernels take widths up to 512 and 1024, not ViT-B's 768: those
  rows take the framework's LayerNorm (fused.layer_norm_any_width); the patch embedding stays on the framework's convolution.
* GPU training (autograd recording, float32 / bfloat16 tokens, head dim 64, attention dropout inactive): in_proj and out_proj
  on the library's GEMMs (differentiable, as every dense op of the training step), between them mhsa_autograd — ppn_mhsa_fwd
  forward and ppn_mhsa_bwd (csrc/mhsa_bwd.hip) backward: P is recomputed from qkv and per-query statistics, so a layer saves qkv
  and out and nothing of size N x N, and the gradients are bitwise reproducible (no atomics).  Dropout and drop path as the
  reference applies them.
* everything else (CPU, other head dims, active attention dropout): nn.MultiheadAttention itself.
"""
import ctypes
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from . import fused
from .dense import drop_path, gpu_inference, linear
from .swin import FFN, PatchEmbed

HEAD_DIM = 64
# head dims ppn_mhsa_fwd / ppn_mhsa_bwd take: 64 (mmseg's ViT: matrix cores) and 8 (GenNet's AE-ViT: csrc/mhsa_d8.hip)
KERNEL_HEAD_DIMS = (8, 64)

# Launch counters (tests / tools): how many attentions ran on the HIP forward kernel, how many backwards on ppn_mhsa_bwd.
CALLS = {"kernel": 0, "bwd_kernel": 0}
# Measurement hook like swin.TIMING: a list here makes every kernel launch record (start event, end event, B, N, heads, element size).
TIMING = None


def mhsa_forward(qkv, heads, scale):
    """ppn_mhsa_fwd: qkv [B,N,3*heads*D] CUDA (float32 / bfloat16; each row q | k | v, each [heads][D]) -> [B,N,heads*D]; the head
    dim D = C // heads is read off the shape and must be 8 or 64."""
    if not qkv.is_cuda:
        raise RuntimeError("ppnet_amd.vit: the attention kernel runs on the GPU only (no CPU fallback)")
    B, N, C3 = qkv.shape
    C = C3 // 3
    hd = C // max(heads, 1)
    if C3 != 3 * C or heads < 1 or C != heads * hd or hd not in KERNEL_HEAD_DIMS:
        raise NotImplementedError(f"head dim {hd}: the kernel takes head dims {KERNEL_HEAD_DIMS}")
    dtype = {torch.float32: 0, torch.bfloat16: 1}.get(qkv.dtype)
    if dtype is None:
        raise NotImplementedError(f"dtype {qkv.dtype}")
    qkv = qkv.contiguous()
    out = torch.empty(B, N, C, dtype=qkv.dtype, device=qkv.device)
    stream = torch.cuda.current_stream(qkv.device)
    ev = None
    if TIMING is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    with torch.cuda.device(qkv.device):
        rc = L.lib.ppn_mhsa_fwd(ctypes.c_void_p(qkv.data_ptr()), ctypes.c_void_p(out.data_ptr()), B, N, heads, hd, float(scale), dtype,
                                ctypes.c_void_p(stream.cuda_stream))
    L.check(rc, "ppn_mhsa_fwd")
    CALLS["kernel"] += 1
    if ev is not None:
        ev[1].record()
        TIMING.append((ev[0], ev[1], B, N, heads, qkv.element_size()))
    return out


class _MHSAFunction(torch.autograd.Function):
    """qkv [B,N,3*heads*D] -> [B,N,heads*D] (D = 8 or 64) on ppn_mhsa_fwd; backward on ppn_mhsa_bwd.  Saves qkv and out, nothing else."""

    @staticmethod
    def forward(ctx, qkv, heads, scale):
        qkv = qkv.detach().contiguous()
        out = mhsa_forward(qkv, heads, scale)
        ctx.save_for_backward(qkv, out)
        ctx.meta = (heads, scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out = ctx.saved_tensors
        heads, scale = ctx.meta
        B, N, C3 = qkv.shape
        dout = dout.to(qkv.dtype).contiguous()
        dqkv = torch.empty_like(qkv)
        need = L.lib.ppn_mhsa_bwd_workspace(B, N, heads)                  # per-query softmax statistic and rowsum(dO o O); P is recomputed
        if need < 0:
            raise ValueError(f"ppn_mhsa_bwd: shape {(B, N, heads)} is outside the kernel")
        ws = torch.empty(need, dtype=torch.float32, device=qkv.device)
        dtype = {torch.float32: 0, torch.bfloat16: 1}[qkv.dtype]
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        with torch.cuda.device(qkv.device):
            rc = L.lib.ppn_mhsa_bwd(p(qkv), p(out), p(dout), p(dqkv), p(ws), need, B, N, heads, C3 // (3 * heads), float(scale), dtype,
                                    ctypes.c_void_p(torch.cuda.current_stream(qkv.device).cuda_stream))
        L.check(rc, "ppn_mhsa_bwd")
        CALLS["bwd_kernel"] += 1
        return dqkv, None, None


def mhsa_autograd(qkv, heads, scale):
    """Differentiable global attention on qkv [B,N,3*heads*D] CUDA (float32 / bfloat16; head dim D = 8 or 64, read off the shape):
    ppn_mhsa_fwd, and ppn_mhsa_bwd in backward."""
    return _MHSAFunction.apply(qkv, heads, scale)


class _Proj:
    """in_proj_weight / in_proj_bias of an nn.MultiheadAttention seen as a Linear (what dense.linear takes)."""

    def __init__(self, mha):
        self.m = mha

    in_features = property(lambda s: s.m.embed_dim)
    out_features = property(lambda s: 3 * s.m.embed_dim)
    weight = property(lambda s: s.m.in_proj_weight)
    bias = property(lambda s: s.m.in_proj_bias)


class MultiheadAttention(nn.Module):
    """mmcv 1.4.8's MultiheadAttention as vit.py:63-70 builds it: `attn` = nn.MultiheadAttention(embed_dims, num_heads, attn_drop,
    bias=qkv_bias) on batch-first tokens; forward returns identity + drop_path(proj_drop(attn(x)))."""

    def __init__(self, embed_dims, num_heads, attn_drop=0.0, proj_drop=0.0, drop_path_rate=0.0, bias=True):
        super().__init__()
        self.embed_dims, self.num_heads = embed_dims, num_heads
        self.attn = nn.MultiheadAttention(embed_dims, num_heads, attn_drop, bias=bias)
        self.proj_drop = nn.Dropout(proj_drop)
        self.drop_path_rate = float(drop_path_rate)
        self.__dict__["_in_proj"] = _Proj(self.attn)

    def forward(self, x, identity):
        """x [B,N,C] (after ln1) -> identity + the attention branch.  Training on the GPU: library GEMMs around mhsa_autograd;
        every other case the torch composition."""
        a = self.attn
        if (x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and self.embed_dims == self.num_heads * HEAD_DIM
                and (a.dropout == 0.0 or not self.training)
                and fused.recording(x, a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias)):
            qkv = F.linear(x, a.in_proj_weight, a.in_proj_bias)
            out = F.linear(mhsa_autograd(qkv, self.num_heads, HEAD_DIM ** -0.5), a.out_proj.weight, a.out_proj.bias)
        else:
            out = a(x.transpose(0, 1), x.transpose(0, 1), x.transpose(0, 1), need_weights=False)[0].transpose(0, 1)
        return identity + drop_path(self.proj_drop(out), self.drop_path_rate, self.training)

    def attend_gpu(self, y):
        """GPU inference: attention(in_proj(y)) for y [B,N,C] (before out_proj), on the build's GEMM and ppn_mhsa_fwd."""
        B, N, C = y.shape
        qkv = linear(y.reshape(-1, C).contiguous(), self._in_proj).view(B, N, 3 * C)
        return mhsa_forward(qkv, self.num_heads, (C // self.num_heads) ** -0.5)


class TransformerEncoderLayer(nn.Module):
    """vit.py:21-95: x + attn(ln1(x)), then x + ffn(ln2(x)) (pre-LN, GELU MLP)."""

    def __init__(self, embed_dims, num_heads, feedforward_channels, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0, qkv_bias=True,
                 eps=1e-5):
        super().__init__()
        self.ln1 = nn.LayerNorm(embed_dims, eps=eps)
        self.attn = MultiheadAttention(embed_dims, num_heads, attn_drop_rate, drop_rate, drop_path_rate, qkv_bias)
        self.ln2 = nn.LayerNorm(embed_dims, eps=eps)
        self.ffn = FFN(embed_dims, feedforward_channels, drop_rate, drop_path_rate)

    def fold(self):
        """SegNet.prepare_inference calls fold() on every level; a ViT layer has no LayerScale or offsets to fold."""
        return self

    def forward(self, x, y=None, next_norm=None):
        """x: residual stream [B,N,C]; y = ln1(x) if the caller has it.  Returns (x', next_norm(x') or None)."""
        if gpu_inference(x):
            # x is updated in place (the caller hands over a fresh tensor).  out_proj and fc2 run with their bias in the GEMM's
            # float32 epilogue, and each branch joins the stream in one add: the stream is rounded once per sub-layer
            B, N, C = x.shape
            x2 = x.view(-1, C)
            if y is None:
                y = fused.layer_norm_any_width(x, self.ln1)
            x2.add_(linear(self.attn.attend_gpu(y).view(-1, C), self.attn.attn.out_proj))
            h = linear(fused.layer_norm_any_width(x, self.ln2).view(-1, C), self.ffn.layers[0][0], gelu=True)
            x2.add_(linear(h, self.ffn.layers[1]))
            return x, (fused.layer_norm_any_width(x, next_norm) if next_norm is not None else None)
        x = self.attn(self.ln1(x), identity=x)
        x = x + self.ffn(self.ln2(x))
        return x, (next_norm(x) if next_norm is not None else None)


def resize_pos_embed(pos_embed, input_shape, pos_shape, mode):
    """vit.py:342-370: the grid part of pos_embed [1, 1 + h w, C] resized to input_shape (align_corners=False); the cls entry kept."""
    pos_h, pos_w = pos_shape
    cls_w = pos_embed[:, 0]
    w = pos_embed[:, (-1 * pos_h * pos_w):].reshape(1, pos_h, pos_w, pos_embed.shape[2]).permute(0, 3, 1, 2)
    w = F.interpolate(w, size=input_shape, mode=mode, align_corners=False)
    return torch.cat((cls_w.unsqueeze(1), torch.flatten(w, 2).transpose(1, 2)), dim=1)


class VisionTransformer(nn.Module):
    """vit.py:98-412 with mmseg's constructor arguments.  forward(x [B,3,H,W] or u8 occupancy codes [B,H,W]) -> one [B,C,h,w] tensor
    per out_index (channels_last memory); layers outside compute_indices stay None (SegNet narrows them to what its heads read)."""

    def __init__(self, img_size=224, patch_size=16, in_channels=3, embed_dims=768, num_layers=12, num_heads=12, mlp_ratio=4, out_indices=-1,
                 qkv_bias=True, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0, with_cls_token=True, output_cls_token=False,
                 norm_cfg=None, act_cfg=None, patch_norm=False, final_norm=False, interpolate_mode="bicubic", num_fcs=2, norm_eval=False,
                 with_cp=False, pretrained=None, init_cfg=None):
        super().__init__()
        if isinstance(img_size, int):
            img_size = (img_size, img_size)
        elif isinstance(img_size, tuple):
            if len(img_size) == 1:
                img_size = (img_size[0], img_size[0])
            assert len(img_size) == 2, f"The size of image should have length 1 or 2, but got {len(img_size)}"
        if output_cls_token:
            assert with_cls_token is True, f"with_cls_token must be True if set output_cls_token to True, but got {with_cls_token}"
            raise NotImplementedError("output_cls_token=True: the SegNet heads read feature maps only")
        if with_cp:
            raise NotImplementedError("with_cp=True (activation checkpointing) is not supported")
        if num_fcs != 2:
            raise NotImplementedError("num_fcs=2 only (every SegNet ViT configuration)")
        norm_cfg = dict(norm_cfg or {"type": "LN"})
        if (act_cfg or {"type": "GELU"}).get("type") != "GELU" or norm_cfg.get("type") != "LN":
            raise NotImplementedError("act_cfg GELU and norm_cfg LN only")
        if pretrained is not None and not isinstance(pretrained, str):
            raise TypeError("pretrained must be a str or None")
        eps = float(norm_cfg.get("eps", 1e-5))
        self.img_size, self.patch_size, self.interpolate_mode = img_size, patch_size, interpolate_mode
        self.norm_eval, self.pretrained = norm_eval, pretrained
        self.patch_embed = PatchEmbed(in_channels, embed_dims, patch_size, patch_norm, norm_eps=eps)
        num_patches = (img_size[0] // patch_size) * (img_size[1] // patch_size)
        self.with_cls_token = with_cls_token
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dims))
        self.pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1, embed_dims))
        self.drop_after_pos = nn.Dropout(p=drop_rate)
        if isinstance(out_indices, int):
            out_indices = [num_layers - 1 if out_indices == -1 else out_indices]
        elif not isinstance(out_indices, (list, tuple)):
            raise TypeError("out_indices must be type of int, list or tuple")
        # the reference appends one output per layer whose index is listed, in layer order (vit.py:386-404): kept in that order, so
        # output slot k is out_indices[k] here (what SegNet's heads index) and an index listed twice or out of range adds nothing
        self.out_indices = [i for i in range(num_layers) if i in out_indices]
        self.compute_indices = tuple(self.out_indices)
        dpr = [float(v) for v in torch.linspace(0, drop_path_rate, num_layers)]
        self.layers = nn.ModuleList(
            TransformerEncoderLayer(embed_dims, num_heads, mlp_ratio * embed_dims, drop_rate, attn_drop_rate, dpr[i], qkv_bias, eps)
            for i in range(num_layers))
        self.final_norm = final_norm
        if final_norm:
            self.ln1 = nn.LayerNorm(embed_dims, eps=eps)
        if isinstance(pretrained, str):
            self.init_weights(pretrained)

    @property
    def levels(self):
        return self.layers

    def init_weights(self, pretrained=None):
        """vit.py:265-310.  A checkpoint path (or self.pretrained): an mmcv checkpoint ({'state_dict', ...} or plain, optional
        'backbone.' prefix), pos_embed resized to img_size / patch_size when its grid differs, loaded non-strictly.  Without one: the
        reference's initialisation (truncated normal 0.02 for pos_embed, cls_token and Linear weights, zero biases — N(0, 1e-6) in
        the MLP —, Kaiming fan-in for the convolution, ones / zeros for LayerNorm)."""
        pretrained = pretrained if pretrained is not None else self.pretrained
        if isinstance(pretrained, str):
            ckpt = torch.load(pretrained, map_location="cpu", weights_only=True)
            sd = ckpt["state_dict"] if "state_dict" in ckpt else ckpt
            sd = {(k[9:] if k.startswith("backbone.") else k): v for k, v in sd.items()}
            if "pos_embed" in sd and self.pos_embed.shape != sd["pos_embed"].shape:
                h, w = self.img_size
                pos_size = int(math.sqrt(sd["pos_embed"].shape[1] - 1))
                sd["pos_embed"] = resize_pos_embed(sd["pos_embed"], (h // self.patch_size, w // self.patch_size), (pos_size, pos_size),
                                                   self.interpolate_mode)
            self.load_state_dict(sd, strict=False)
            return
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        nn.init.trunc_normal_(self.cls_token, std=0.02)
        for n, m in self.named_modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    if "ffn" in n:
                        nn.init.normal_(m.bias, mean=0.0, std=1e-6)
                    else:
                        nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.MultiheadAttention):
                # the in-projection is a bare parameter of nn.MultiheadAttention, not an nn.Linear: mmcv's loop never reaches
                # it and it keeps nn.MultiheadAttention's own (xavier-uniform weight, zero bias) initialisation
                pass
            elif isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, a=0, mode="fan_in", nonlinearity="relu")
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.LayerNorm):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0.0)

    def _grid_pos(self, hw, x):
        """pos_embed for a token grid hw (vit.py:311-340): as stored when the lengths agree, else resized."""
        pos = self.pos_embed
        resize = hw[0] * hw[1] + 1 != pos.shape[1]
        ph, pw = self.img_size[0] // self.patch_size, self.img_size[1] // self.patch_size
        if resize and pos.shape[1] != ph * pw + 1:
            raise ValueError(f"Unexpected shape of pos_embed, got {tuple(pos.shape)}.")
        if gpu_inference(x):
            # computed once per (parameter, grid, dtype) and kept: resized in float32, then rounded to x's dtype
            cache = self.__dict__.get("_pos")
            if cache is None:
                cache = self.__dict__["_pos"] = fused.WeightCache()
            build = lambda: (resize_pos_embed(pos.detach().float(), hw, (ph, pw), self.interpolate_mode) if resize else pos.detach()).to(x.dtype)
            return cache.get((pos,), build, tuple(hw), x.dtype)
        return (resize_pos_embed(pos, hw, (ph, pw), self.interpolate_mode) if resize else pos).to(x.dtype)

    def forward(self, x):
        B = x.shape[0]
        pe = self.patch_embed                          # swin.PatchEmbed's projection; the [B,N,C] tokens and their LayerNorm here
        x = pe.project(x)
        hw = (x.shape[2], x.shape[3])
        x = x.flatten(2).transpose(1, 2)
        if pe.norm is not None:
            x = fused.layer_norm_any_width(x, pe.norm) if gpu_inference(x) else pe.norm(x)
        pos = self._grid_pos(hw, x)
        gpu = gpu_inference(x)
        if self.with_cls_token:
            x = torch.cat((self.cls_token.to(x.dtype).expand(B, -1, -1), x), dim=1) + pos
        else:
            x = x + pos[:, 1:]                         # the cls entry is added, then dropped with the token (vit.py:377-384)
        x = self.drop_after_pos(x)
        if gpu:
            x = x.contiguous()                         # a fresh tensor: the fused kernels update the stream in place
        outs = [None] * len(self.out_indices)
        last = max(self.compute_indices)
        n = len(self.layers)
        y = None
        for i, layer in enumerate(self.layers):
            if i + 1 == n:
                nxt = self.ln1 if self.final_norm else None
            else:                                      # the GPU form hands the next layer its ln1(x); not needed after `last`
                nxt = self.layers[i + 1].ln1 if gpu and i < last else None
            x, y = layer(x, y, nxt)
            if i == n - 1 and self.final_norm:
                x = y                                  # the layer returned ln1(x) (vit.py:389-391)
            if i in self.compute_indices:
                tok = x[:, 1:] if self.with_cls_token else x
                out = tok.reshape(B, hw[0], hw[1], -1)
                if gpu and i < n - 1:
                    out = out.clone()                  # later layers update x in place
                outs[self.out_indices.index(i)] = out.contiguous().permute(0, 3, 1, 2)
            if i >= last:
                break                                  # no layer past this one is read
        return outs

    def train(self, mode=True):
        super().train(mode)
        if mode and self.norm_eval:
            for m in self.modules():
                if isinstance(m, nn.LayerNorm):
                    m.eval()
        return self
