"""Swin Transformer backbone (reference SegNet/mmseg/backbones/swin.py:22-757, mmseg/models/utils/embed.py:12-330) with mmseg's
constructor arguments and state-dict layout (`patch_embed.{projection,norm}`, `stages.i.blocks.j.{norm1,attn.w_msa.{qkv,proj,
relative_position_bias_table,relative_position_index},norm2,ffn.layers.{0.0,1}}`, `stages.i.downsample.{norm,reduction}`,
`norm{i}`), so an mmseg Swin checkpoint loads unchanged.

Two forms of the same arithmetic:
* GPU inference (CUDA tensors, no autograd): LayerNorm kernels, the build's GEMMs where their gates pass (dense.linear) and the
  fused (shifted-)window attention kernel ppn_swin_wmsa_fwd between the qkv and proj projections.
* GPU training (CUDA tensors, autograd recording, head dim 32, window 7): library GEMMs for the qkv / proj Linears around
  `wmsa_autograd`: ppn_swin_wmsa_fwd forward and ppn_swin_wmsa_bwd (csrc/swin_wmsa_bwd.hip) backward.  P is recomputed from qkv,
  so a block saves qkv, the qkv bias and the bias table and nothing of size 49 x 49; the gradients of qkv, of the qkv bias (the
  padded positions' k / v) and of the bias table are bitwise reproducible.
* everything else (CPU, other head dims or windows): a pure-torch composition of mmseg's ops (`window_attention`).

`wmsa_forward` also serves GenNet's AESwin (gennet.py): window 14 with head dims 8 / 16 / 32 and window 7 with head dims 8 / 16 run on
ppn_wmsa_fwd (csrc/wmsa_gen.hip), forward only; the backbone above asks for window 7 / head dim 32 only and is unchanged.
"""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from . import fused
from .dense import IMG_MEAN, IMG_STD, drop_path, gpu_inference, linear

WINDOW = 7
HEAD_DIM = 32

# Launch counter (tests / tools): how many window attentions ran on the HIP kernel and how many on the torch composition.
CALLS = {"kernel": 0, "torch": 0}
# The training path's launches (wmsa_autograd): forwards on ppn_swin_wmsa_fwd (not counted in CALLS), backwards on ppn_swin_wmsa_bwd.
TRAIN_CALLS = {"fwd_kernel": 0, "bwd_kernel": 0}
# Measurement hook like na.TIMING: a list here makes every kernel launch record (start event, end event, real tokens, channels,
# element size).
TIMING = None


def padded_hw(H, W, window=WINDOW):
    """mmseg pads every grid to multiples of the window, also when it is smaller (swin.py:186-189)."""
    return -(-H // window) * window, -(-W // window) * window


def region_mask(Hp, Wp, window, shift, device=None, dtype=torch.float64, value=-100.0):
    """The SW-MSA mask of swin.py:199-219: [nW, N, N] with `value` between slots of different regions, 0 elsewhere."""
    img = torch.zeros(Hp, Wp, device=device)
    cnt = 0
    for hs in (slice(0, -window), slice(-window, -shift), slice(-shift, None)):
        for ws in (slice(0, -window), slice(-window, -shift), slice(-shift, None)):
            img[hs, ws] = cnt
            cnt += 1
    mw = img.view(Hp // window, window, Wp // window, window).permute(0, 2, 1, 3).reshape(-1, window * window)
    d = mw.unsqueeze(1) - mw.unsqueeze(2)
    return torch.where(d != 0, torch.full_like(d, value), torch.zeros_like(d)).to(dtype)


def bias_table_hw(table, heads, window=WINDOW):
    """mmseg's relative_position_bias_table [(2w-1)^2, heads] as the kernel's [heads][2w-1][2w-1] (indexed [h][dy+w-1][dx+w-1],
    (dy, dx) = query minus key)."""
    return table.t().reshape(heads, 2 * window - 1, 2 * window - 1)


def window_attention(qkv, pad_kv, table, heads, shift, scale, window=WINDOW, mask_value=-100.0):
    """The pure-torch composition (mmseg's op chain, swin.py:80-118,179-253, on the qkv projection instead of the normed tokens):
    qkv [B,H,W,3C] of the real tokens, pad_kv [3C] (what a zero-padded token projects to: the qkv bias), table [(2w-1)^2, heads].
    Returns [B,H,W,C] — the attention output before the proj Linear (which is per token, so it commutes with the window reverse,
    the roll back and the crop)."""
    CALLS["torch"] += 1
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    Hp, Wp = padded_hw(H, W, window)
    if Hp != H or Wp != W:
        full = pad_kv.to(qkv.dtype).view(1, 1, 1, C3).expand(B, Hp, Wp, C3).clone()
        full[:, :H, :W] = qkv
        qkv = full
    if shift > 0:
        qkv = torch.roll(qkv, shifts=(-shift, -shift), dims=(1, 2))
    N = window * window
    win = qkv.view(B, Hp // window, window, Wp // window, window, C3).permute(0, 1, 3, 2, 4, 5).reshape(-1, N, 3, heads, C // heads)
    q, k, v = win.permute(2, 0, 3, 1, 4).unbind(0)                       # [B nW, heads, N, d]
    attn = (q * scale) @ k.transpose(-2, -1)
    idx = _relative_index(window, qkv.device)
    attn = attn + table[idx.view(-1)].view(N, N, -1).permute(2, 0, 1).to(attn.dtype).unsqueeze(0)
    if shift > 0:
        m = region_mask(Hp, Wp, window, shift, qkv.device, attn.dtype, mask_value)
        nW = m.shape[0]
        attn = (attn.view(B, nW, heads, N, N) + m.unsqueeze(1).unsqueeze(0)).view(-1, heads, N, N)
    attn = attn.softmax(dim=-1)
    o = (attn @ v).transpose(1, 2).reshape(B, Hp // window, Wp // window, window, window, C)
    o = o.permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)
    if shift > 0:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    return o[:, :H, :W]


def _relative_index(window, device=None):
    """swin.py:64-68 (double_step_seq + flip(1))."""
    seq1 = torch.arange(0, (2 * window - 1) * window, 2 * window - 1)
    seq2 = torch.arange(0, window)
    c = (seq1[:, None] + seq2[None, :]).reshape(1, -1)
    return (c + c.T).flip(1).contiguous().to(device)


# (window, head dim) of ppn_wmsa_fwd (csrc/wmsa_gen.hip): GenNet's AESwin.  (7, 32), Swin-B's shape, stays on ppn_swin_wmsa_fwd.
GEN_SHAPES = ((14, 8), (14, 16), (14, 32), (7, 8), (7, 16))


def kernel_takes(window, head_dim):
    """Whether a HIP forward kernel exists for this (window, head dim)."""
    return (window, head_dim) == (WINDOW, HEAD_DIM) or (window, head_dim) in GEN_SHAPES


def wmsa_forward(qkv, pad_kv, rpb_hw, heads, shift, scale, window=WINDOW):
    """qkv [B,H,W,3C] CUDA (float32 / bfloat16), pad_kv [3C], rpb_hw [heads,2w-1,2w-1] float32 -> [B,H,W,C]; the head dim is
    C / heads.  ppn_swin_wmsa_fwd for window 7 / head dim 32, ppn_wmsa_fwd for GEN_SHAPES."""
    out = _wmsa_launch(qkv, pad_kv, rpb_hw, heads, shift, scale, window)
    CALLS["kernel"] += 1
    return out


def _wmsa_launch(qkv, pad_kv, rpb_hw, heads, shift, scale, window=WINDOW):
    if not qkv.is_cuda:
        raise RuntimeError("ppnet_amd.swin: the window-attention kernel runs on the GPU only (no CPU fallback)")
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    head_dim = C // max(heads, 1)
    gen = C == heads * head_dim and (window, head_dim) in GEN_SHAPES
    if C != heads * HEAD_DIM and not gen:
        raise NotImplementedError(f"head dim {C // max(heads, 1)}: the kernel takes head dim {HEAD_DIM}")
    dtype = {torch.float32: 0, torch.bfloat16: 1}.get(qkv.dtype)
    if dtype is None:
        raise NotImplementedError(f"dtype {qkv.dtype}")
    qkv = qkv.contiguous()
    pad_kv = pad_kv.detach().to(qkv.dtype).contiguous()
    rpb_hw = rpb_hw.detach().to(torch.float32).contiguous()
    out = torch.empty(B, H, W, C, dtype=qkv.dtype, device=qkv.device)
    stream = torch.cuda.current_stream(qkv.device)
    ev = None
    if TIMING is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    ptrs = (ctypes.c_void_p(qkv.data_ptr()), ctypes.c_void_p(pad_kv.data_ptr()), ctypes.c_void_p(rpb_hw.data_ptr()),
            ctypes.c_void_p(out.data_ptr()))
    with torch.cuda.device(qkv.device):
        if gen:
            rc = L.lib.ppn_wmsa_fwd(*ptrs, B, H, W, heads, head_dim, window, shift, float(scale), dtype, ctypes.c_void_p(stream.cuda_stream))
        else:
            rc = L.lib.ppn_swin_wmsa_fwd(*ptrs, B, H, W, heads, window, shift, float(scale), dtype, ctypes.c_void_p(stream.cuda_stream))
    L.check(rc, "ppn_wmsa_fwd" if gen else "ppn_swin_wmsa_fwd")
    if ev is not None:
        ev[1].record()
        TIMING.append((ev[0], ev[1], B * H * W, C, qkv.element_size()))
    return out


class _WMSAFunction(torch.autograd.Function):
    """(qkv [B,H,W,3C], pad_kv [3C], table [(2w-1)^2, heads]) -> [B,H,W,C] on ppn_swin_wmsa_fwd; backward on ppn_swin_wmsa_bwd.
    Saves qkv, pad_kv and the [heads,13,13] float32 table, nothing else."""

    @staticmethod
    def forward(ctx, qkv, pad_kv, table, heads, shift, scale):
        qkv = qkv.detach().contiguous()
        pad = pad_kv.detach().to(qkv.dtype).contiguous()
        rpb_hw = bias_table_hw(table.detach().float(), heads).contiguous()
        out = _wmsa_launch(qkv, pad, rpb_hw, heads, shift, scale)
        TRAIN_CALLS["fwd_kernel"] += 1
        ctx.save_for_backward(qkv, pad, rpb_hw)
        ctx.meta = (heads, shift, scale, pad_kv.dtype, table.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, pad, rpb_hw = ctx.saved_tensors
        heads, shift, scale, pad_dtype, table_dtype = ctx.meta
        B, H, W, _ = qkv.shape
        dout = dout.to(qkv.dtype).contiguous()
        dqkv = torch.empty_like(qkv)
        dpad = torch.empty(3 * heads * HEAD_DIM, dtype=torch.float32, device=qkv.device)
        drpb = torch.empty(heads, 2 * WINDOW - 1, 2 * WINDOW - 1, dtype=torch.float32, device=qkv.device)
        with torch.cuda.device(qkv.device):
            need = L.lib.ppn_swin_wmsa_bwd_workspace(B, H, W, heads)      # the workgroups' partial sums of drpb and dpad_kv
            if need < 0:
                raise ValueError(f"ppn_swin_wmsa_bwd: shape {(B, H, W, heads)} is outside the kernel")
            ws = torch.empty(need, dtype=torch.float32, device=qkv.device)
            p = lambda t: ctypes.c_void_p(t.data_ptr())
            rc = L.lib.ppn_swin_wmsa_bwd(p(qkv), p(pad), p(rpb_hw), p(dout), p(dqkv), p(dpad), p(drpb), p(ws), need, B, H, W, heads, WINDOW,
                                         shift, float(scale), {torch.float32: 0, torch.bfloat16: 1}[qkv.dtype],
                                         ctypes.c_void_p(torch.cuda.current_stream(qkv.device).cuda_stream))
        L.check(rc, "ppn_swin_wmsa_bwd")
        TRAIN_CALLS["bwd_kernel"] += 1
        dtable = drpb.reshape(heads, -1).t().to(table_dtype) if ctx.needs_input_grad[2] else None     # the inverse of bias_table_hw
        return dqkv, (dpad.to(pad_dtype) if ctx.needs_input_grad[1] else None), dtable, None, None, None


def wmsa_autograd(qkv, pad_kv, table, heads, shift, scale):
    """Differentiable window attention on qkv [B,H,W,3*heads*32] CUDA (float32 / bfloat16), pad_kv [3C] (the qkv bias), table
    [(2w-1)^2, heads] (the parameter's layout): ppn_swin_wmsa_fwd, and ppn_swin_wmsa_bwd in backward (window 7, shift 0 or 3)."""
    if not qkv.is_cuda:
        raise RuntimeError("ppnet_amd.swin: the window-attention kernel runs on the GPU only (no CPU fallback)")
    return _WMSAFunction.apply(qkv, pad_kv, table, heads, shift, scale)


class WindowMSA(nn.Module):
    """swin.py:22-124: parameters qkv, proj, relative_position_bias_table [(2w-1)^2, heads], buffer relative_position_index."""

    def __init__(self, embed_dims, num_heads, window_size, qkv_bias=True, qk_scale=None, attn_drop_rate=0.0, proj_drop_rate=0.0):
        super().__init__()
        self.embed_dims, self.num_heads = embed_dims, num_heads
        self.window_size = (window_size, window_size)
        self.scale = qk_scale or (embed_dims // num_heads) ** -0.5
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * window_size - 1) ** 2, num_heads))
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)
        self.register_buffer("relative_position_index", _relative_index(window_size))
        self.qkv = nn.Linear(embed_dims, embed_dims * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop_rate)
        self.proj = nn.Linear(embed_dims, embed_dims)
        self.proj_drop = nn.Dropout(proj_drop_rate)
        self._rpb32 = None

    def pad_kv(self, ref):
        b = self.qkv.bias
        return b if b is not None else torch.zeros(3 * self.embed_dims, dtype=ref.dtype, device=ref.device)

    def rpb_hw(self):
        """The table as the kernel's float32 [heads,13,13], cached while the parameter is unchanged."""
        r = self.relative_position_bias_table
        key = (r.device, r._version, r.data_ptr(), r.dtype)
        if self._rpb32 is None or self._rpb32[0] != key:
            self._rpb32 = (key, bias_table_hw(r.detach().float(), self.num_heads, self.window_size[0]).contiguous())
        return self._rpb32[1]


class ShiftWindowMSA(nn.Module):
    """swin.py:127-284: the attention sub-layer of a block, mmseg's parameter nesting (`w_msa.*`)."""

    def __init__(self, embed_dims, num_heads, window_size, shift_size=0, qkv_bias=True, qk_scale=None, attn_drop_rate=0.0,
                 proj_drop_rate=0.0, drop_path_rate=0.0):
        super().__init__()
        assert 0 <= shift_size < window_size
        self.window_size, self.shift_size = window_size, shift_size
        self.w_msa = WindowMSA(embed_dims, num_heads, window_size, qkv_bias, qk_scale, attn_drop_rate, proj_drop_rate)
        self.drop_path_rate = float(drop_path_rate)

    def attend(self, qkv):
        """Attention of qkv [B,H,W,3C] (before proj): the HIP forward kernel for GPU inference, the forward and backward kernels
        (wmsa_autograd) when autograd records on the GPU, the torch composition otherwise."""
        m = self.w_msa
        if gpu_inference(qkv):
            return wmsa_forward(qkv, m.pad_kv(qkv), m.rpb_hw(), m.num_heads, self.shift_size, m.scale, self.window_size)
        if m.attn_drop.p > 0 and self.training:
            raise NotImplementedError("attn_drop_rate > 0 in training")
        if self.trains_on_kernel(qkv):
            return wmsa_autograd(qkv, m.pad_kv(qkv), m.relative_position_bias_table, m.num_heads, self.shift_size, m.scale)
        return window_attention(qkv, m.pad_kv(qkv), m.relative_position_bias_table, m.num_heads, self.shift_size, m.scale,
                                self.window_size)

    def trains_on_kernel(self, qkv):
        """Autograd records, on CUDA float32 / bfloat16 tensors, with the kernels' head dim, window and shifts."""
        m = self.w_msa
        return (qkv.is_cuda and qkv.dtype in (torch.float32, torch.bfloat16) and m.embed_dims == m.num_heads * HEAD_DIM
                and self.window_size == WINDOW and self.shift_size in (0, WINDOW // 2)
                and fused.recording(qkv, m.qkv.bias, m.relative_position_bias_table))

    def forward(self, x):
        """x [B,H,W,C] (after norm1) -> [B,H,W,C] (DropPath in training)."""
        m = self.w_msa
        B, H, W, C = x.shape
        x2 = x.reshape(-1, C)
        qkv = (linear(x2.contiguous(), m.qkv) if gpu_inference(x) else m.qkv(x2)).view(B, H, W, 3 * C)
        o = self.attend(qkv).reshape(-1, C)
        o = linear(o.contiguous(), m.proj) if gpu_inference(x) else m.proj(o)
        return drop_path(m.proj_drop(o.view(B, H, W, C)), self.drop_path_rate, self.training)


class FFN(nn.Module):
    """mmcv 1.4.8 FFN (num_fcs=2): layers = Sequential(Sequential(Linear, GELU, Dropout), Linear, Dropout); identity + out."""

    def __init__(self, embed_dims, feedforward_channels, ffn_drop=0.0, drop_path_rate=0.0):
        super().__init__()
        self.layers = nn.Sequential(nn.Sequential(nn.Linear(embed_dims, feedforward_channels), nn.GELU(), nn.Dropout(ffn_drop)),
                                    nn.Linear(feedforward_channels, embed_dims), nn.Dropout(ffn_drop))
        self.drop_path_rate = float(drop_path_rate)

    def forward(self, x):
        """The branch only (the caller adds the identity): [B,H,W,C] -> [B,H,W,C]."""
        fc1, fc2 = self.layers[0][0], self.layers[1]
        if gpu_inference(x):
            x2 = x.reshape(-1, x.shape[-1]).contiguous()
            return linear(linear(x2, fc1, gelu=True), fc2).view(x.shape)
        return drop_path(self.layers(x), self.drop_path_rate, self.training)


class SwinBlock(nn.Module):
    """swin.py:287-376: x + attn(norm1(x)), then x + ffn(norm2(x))."""

    def __init__(self, embed_dims, num_heads, feedforward_channels, window_size=7, shift=False, qkv_bias=True, qk_scale=None,
                 drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0):
        super().__init__()
        self.norm1 = nn.LayerNorm(embed_dims)
        self.attn = ShiftWindowMSA(embed_dims, num_heads, window_size, window_size // 2 if shift else 0, qkv_bias, qk_scale,
                                   attn_drop_rate, drop_rate, drop_path_rate)
        self.norm2 = nn.LayerNorm(embed_dims)
        self.ffn = FFN(embed_dims, feedforward_channels, drop_rate, drop_path_rate)

    def forward(self, x, y=None, next_norm=None):
        """x: residual stream [B,H,W,C]; y = norm1(x) if the caller has it.  Returns (x', next_norm(x') or None)."""
        if gpu_inference(x):
            # LayerNorm and residual adds on the fused kernels (x is updated in place: the caller hands over a fresh tensor)
            if y is None:
                y = fused.layer_norm(x, self.norm1)
            x, y2 = fused.residual_layer_norm(x, self.attn(y), None, self.norm2)
            return fused.residual_layer_norm(x, self.ffn(y2), None, next_norm)
        x = x + self.attn(self.norm1(x))
        x = x + self.ffn(self.norm2(x))
        return x, (next_norm(x) if next_norm is not None else None)


class PatchMerging(nn.Module):
    """embed.py:207-330: 'corner' padding to even sizes, nn.Unfold(2, 2) channel order c * 4 + kh * 2 + kw, LN(4C), Linear(4C, 2C,
    bias=False)."""

    def __init__(self, in_channels, out_channels, stride=2, norm=True):
        super().__init__()
        assert stride == 2, "kernel = stride = 2 (every Swin configuration)"
        self.in_channels, self.out_channels = in_channels, out_channels
        self.norm = nn.LayerNorm(4 * in_channels) if norm else None
        self.reduction = nn.Linear(4 * in_channels, out_channels, bias=False)

    def forward(self, x):
        """x [B,H,W,C] -> [B,ceil(H/2),ceil(W/2),2C]."""
        B, H, W, C = x.shape
        if H % 2 or W % 2:
            x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
        Ho, Wo = x.shape[1] // 2, x.shape[2] // 2
        x = x.reshape(B, Ho, 2, Wo, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, Ho, Wo, 4 * C)
        if gpu_inference(x):
            if self.norm is not None:
                # the LayerNorm kernel takes rows of up to 1024 channels; the 2048-wide rows of Swin-B's last merge take the
                # framework's LayerNorm (one launch per forward)
                x = fused.layer_norm(x, self.norm) if 4 * C <= 1024 else F.layer_norm(x, (4 * C,), self.norm.weight, self.norm.bias, self.norm.eps)
            return linear(x.reshape(-1, 4 * C), self.reduction).view(B, Ho, Wo, -1)
        if self.norm is not None:
            x = self.norm(x)
        return self.reduction(x)


class PatchEmbed(nn.Module):
    """embed.py:83-204 with kernel = stride = patch_size: 'corner' adaptive padding (bottom / right), the framework's convolution,
    optional LayerNorm.  Swin calls the module; vit.py (same parameters and keys) calls project() and normalises its own [B,N,C] layout."""

    def __init__(self, in_channels, embed_dims, patch_size, norm=True, norm_eps=1e-5):
        super().__init__()
        self.patch_size = patch_size
        self.projection = nn.Conv2d(in_channels, embed_dims, patch_size, patch_size)
        self.norm = nn.LayerNorm(embed_dims, eps=norm_eps) if norm else None

    def takes_codes(self, grid_u8):
        return False                                   # SegNet.labels_u8 renders occupancy codes to an image first

    def project(self, x):
        """x [B,3,H,W], or the u8 occupancy codes [B,H,W] it would be rendered from -> the projection [B,C,h,w], before the norm."""
        if x.dtype == torch.uint8:
            x = fused.grid_to_image(x, IMG_MEAN, IMG_STD, self.projection.weight.dtype)
        p = self.patch_size
        H, W = x.shape[-2:]
        ph, pw = (-H) % p, (-W) % p
        if ph or pw:
            x = F.pad(x, [0, pw, 0, ph])
        return self.projection(x)

    def forward(self, x):
        """-> tokens [B,H/4,W/4,C] (NHWC)."""
        x = self.project(x).permute(0, 2, 3, 1)
        if self.norm is None:
            return x
        return fused.layer_norm(x, self.norm) if gpu_inference(x) else self.norm(x)


class SwinBlockSequence(nn.Module):
    """swin.py:379-460: depth blocks, odd ones shifted, then the optional PatchMerging."""

    def __init__(self, embed_dims, num_heads, feedforward_channels, depth, window_size=7, qkv_bias=True, qk_scale=None, drop_rate=0.0,
                 attn_drop_rate=0.0, drop_path_rate=0.0, downsample=None):
        super().__init__()
        dpr = drop_path_rate if isinstance(drop_path_rate, list) else [drop_path_rate] * depth
        assert len(dpr) == depth
        self.blocks = nn.ModuleList(
            SwinBlock(embed_dims, num_heads, feedforward_channels, window_size, i % 2 == 1, qkv_bias, qk_scale, drop_rate, attn_drop_rate,
                      dpr[i]) for i in range(depth))
        self.downsample = downsample

    def fold(self):
        """SegNet.prepare_inference calls fold() on every level; a Swin stage has no LayerScale or offsets to fold."""
        return self

    def forward(self, x, out_norm=None):
        """Returns (next level's input, out_norm(x) or None)."""
        if gpu_inference(x):
            x = x.contiguous().clone()                 # the fused kernels update the stream in place
        y = None
        n = len(self.blocks)
        for i, blk in enumerate(self.blocks):
            x, y = blk(x, y, self.blocks[i + 1].norm1 if i + 1 < n else out_norm)
        xo = y
        return (x if self.downsample is None else self.downsample(x)), xo


class SwinTransformer(nn.Module):
    """swin.py:463-757 with mmseg's constructor arguments.  forward(x [B,3,H,W] or u8 occupancy codes [B,H,W]) -> one [B,C,H,W]
    tensor per out_index (channels_last memory); levels outside compute_indices stay None (SegNet narrows them to what its
    heads read)."""

    def __init__(self, pretrain_img_size=224, in_channels=3, embed_dims=96, patch_size=4, window_size=7, mlp_ratio=4, depths=(2, 2, 6, 2),
                 num_heads=(3, 6, 12, 24), strides=(4, 2, 2, 2), out_indices=(0, 1, 2, 3), qkv_bias=True, qk_scale=None, patch_norm=True,
                 drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.1, use_abs_pos_embed=False, act_cfg=None, norm_cfg=None,
                 with_cp=False, pretrained=None, frozen_stages=-1, init_cfg=None):
        super().__init__()
        if use_abs_pos_embed:
            raise NotImplementedError("use_abs_pos_embed=True: every SegNet Swin configuration sets False")
        if with_cp:
            raise NotImplementedError("with_cp=True (activation checkpointing) is not supported")
        if frozen_stages is not None and frozen_stages >= 0:
            raise NotImplementedError("frozen_stages >= 0 is not supported")
        if (act_cfg or {"type": "GELU"}).get("type") != "GELU" or (norm_cfg or {"type": "LN"}).get("type") != "LN":
            raise NotImplementedError("act_cfg GELU and norm_cfg LN only")
        if strides[0] != patch_size:
            raise ValueError("Use non-overlapping patch embed.")
        self.window_size = window_size
        self.out_indices = tuple(out_indices)
        self.compute_indices = tuple(out_indices)
        self.patch_embed = PatchEmbed(in_channels, embed_dims, patch_size, patch_norm)
        self.drop_after_pos = nn.Dropout(p=drop_rate)
        total = sum(depths)
        dpr = [float(v) for v in torch.linspace(0, drop_path_rate, total)]
        self.stages = nn.ModuleList()
        c = embed_dims
        for i in range(len(depths)):
            down = PatchMerging(c, 2 * c, strides[i + 1], patch_norm) if i < len(depths) - 1 else None
            self.stages.append(SwinBlockSequence(c, num_heads[i], int(mlp_ratio * c), depths[i], window_size, qkv_bias, qk_scale, drop_rate,
                                                 attn_drop_rate, dpr[sum(depths[:i]):sum(depths[:i + 1])], down))
            if down is not None:
                c = down.out_channels
        self.num_features = [int(embed_dims * 2 ** i) for i in range(len(depths))]
        for i in self.out_indices:
            self.add_module(f"norm{i}", nn.LayerNorm(self.num_features[i]))
        if isinstance(pretrained, str):
            self.init_weights(pretrained)

    @property
    def levels(self):
        return self.stages

    def init_weights(self, pretrained=None):
        """An mmseg / mmcv checkpoint ({'state_dict' | 'model' | plain}, optional 'backbone.' prefix); not strict (swin.py:686)."""
        if isinstance(pretrained, str):
            sd = torch.load(pretrained, map_location="cpu", weights_only=True)
            sd = sd.get("state_dict", sd.get("model", sd))
            sd = {(k[9:] if k.startswith("backbone.") else k): v for k, v in sd.items()}
            self.load_state_dict(sd, strict=False)

    def forward(self, x):
        x = self.drop_after_pos(self.patch_embed(x))
        outs = [None] * len(self.out_indices)
        for i, stage in enumerate(self.stages):
            want = i in self.compute_indices
            x, xo = stage(x, getattr(self, f"norm{i}") if want else None)
            if want:
                outs[self.out_indices.index(i)] = xo.permute(0, 3, 1, 2)
            if all(j <= i for j in self.compute_indices) and i + 1 < len(self.stages):
                break                                    # no level past this one is read
        return outs
