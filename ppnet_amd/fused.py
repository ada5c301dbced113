"""Host side of the fused residual / LayerScale / LayerNorm kernel (ppn_residual_layernorm). GPU only.

Inference runs the HIP kernels below.  When autograd is recording (a training step, ppnet_amd/train.py) layer_norm and
residual_layer_norm record the training pair of the same kernel (ppn_residual_layernorm_train_fwd / ppn_residual_layernorm_bwd,
_ResidualLayerNormFunction: stochastic depth, LayerScale, the residual add, the next LayerNorm and the backward of all of it), and
the functions without a backward kernel compose differentiable torch ops instead.  The other hand-written backwards are the
attentions': neighbourhood (ppn_na2d_bwd, na.na2d_autograd), ViT's global one (ppn_mhsa_bwd, vit.mhsa_autograd) and Swin's window one
(ppn_swin_wmsa_bwd, swin.wmsa_autograd) — the heads' loss: bilinear resize + cross-entropy (ppn_resize_ce_bwd,
resize_cross_entropy below) — and the heads' bilinear up-sampling (ppn_upsample2x_nhwc_bwd, ppn_upsample2x_concat_nhwc_bwd,
ppn_resize_concat_nhwc_bwd: upsample2x_nhwc, upsample2x_add, upsample2x_concat and resize_concat record their own kernels) — and
GenNet's stem, convolution + BatchNorm on batch statistics + LeakyReLU (ppn_gennet_stem_train_fwd / ppn_gennet_stem_train_bwd,
stem_bn_act near the end of this file) and its tail, BatchNorm on batch statistics + LeakyReLU + the 24 -> 1 convolution
(ppn_gennet_tail_train_fwd / ppn_gennet_tail_train_bwd, tail_bn_act_conv near the end of this file) and its six 24 -> 24 stride-2
stages' convolutions (ppn_gennet_s2_down / ppn_gennet_s2_up / ppn_gennet_s2_wgrad, conv_s2 at the end of this file)."""
import ctypes
import os

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib as L

_DT = {torch.float32: 0, torch.bfloat16: 1}


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(None)


class WeightCache:
    """A value derived from module parameters (a packed / folded / converted copy for a kernel), rebuilt whenever a source changes:
    the key holds each source tensor's device, `_version` (bumped by every in-place update: optimizer.step, load_state_dict's
    copy_) and `data_ptr` (a new storage after .to(dtype) / .to(device) or re-assignment).  An eval -> step -> eval flow therefore
    never runs a kernel on stale weights.  NOT covered: writes through `param.data` (EMA / weight-tying code, legacy checkpoint
    loaders) — `.data` is a separate tensor object with its own version counter, so neither the version nor the pointer of the
    parameter moves.  After such a write call `invalidate_caches()` (or `WeightCache.clear()` on the one cache)."""
    __slots__ = ("key", "value", "__weakref__")
    _all = None            # weak set of every live cache (invalidate_caches)

    def __init__(self):
        self.key = self.value = None
        if WeightCache._all is None:
            import weakref
            WeightCache._all = weakref.WeakSet()
        WeightCache._all.add(self)

    def clear(self):
        """Forget the derived value: the next get() rebuilds it."""
        self.key = self.value = None

    def get(self, sources, build, *extra):
        key = tuple((t.device, t._version, t.data_ptr()) if t is not None else None for t in sources) + extra
        if key != self.key:
            self.value, self.key = build(), key
        return self.value


def invalidate_caches():
    """Drop every packed / folded / converted weight copy in the process (all WeightCache instances).  Needed only after
    in-place writes through `param.data`, which no key can see; ordinary updates (optimizer.step, load_state_dict, .to()) are
    tracked by themselves."""
    for c in list(WeightCache._all or ()):
        c.clear()


_PADDED = {}


def _padded_buffer(B, Hp, Wp, C, dtype, device):
    """Persistent zero-initialised [B,Hp,Wp,C] buffer: the kernels only ever write the real tokens, so the pad
    region stays zero; consumers (the qkv projection) read it before the next same-shaped producer runs."""
    key = (B, Hp, Wp, C, dtype, device, torch.cuda.current_stream(device).cuda_stream)     # batches in flight on two streams must not share it
    buf = _PADDED.get(key)
    if buf is None:
        buf = _PADDED[key] = torch.zeros(B, Hp, Wp, C, dtype=dtype, device=device)
    return buf


def _call(x, a, gamma, ln, x_out, y_out, pad=None):
    if not x.is_cuda:
        raise RuntimeError("ppnet_amd.fused: GPU tensors only (no CPU fallback)")
    C = x.shape[-1]
    rows = x.numel() // C
    dt = _DT[x.dtype]
    # parameters follow the activation dtype (a no-op when the module holds weights in that dtype already)
    w = ln.weight.detach().to(x.dtype) if ln is not None else None
    b = ln.bias.detach().to(x.dtype) if ln is not None else None
    gamma = gamma.to(x.dtype) if gamma is not None else None
    for t in (a, gamma, w, b):
        assert t is None or (t.dtype == x.dtype and t.is_contiguous())
    hr, wr, hp, wp = pad if pad is not None else (0, 0, 0, 0)
    with torch.cuda.device(x.device):
        rc = L.lib.ppn_residual_layernorm_padded(_p(x), _p(a), _p(gamma), _p(w), _p(b), _p(x_out), _p(y_out), rows, C,
                                                 float(ln.eps) if ln is not None else 0.0, dt, hr, wr, hp, wp,
                                                 ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
    L.check(rc, "ppn_residual_layernorm")


def _y_for(x, pad_to):
    if pad_to is None:
        return torch.empty_like(x), None
    B, Hr, Wr, C = x.shape
    return _padded_buffer(B, pad_to[0], pad_to[1], C, x.dtype, x.device), (Hr, Wr, pad_to[0], pad_to[1])


def recording(*tensors):
    """True when autograd must see the op: grad mode on and an input / parameter requires grad."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _layer_norm_autograd(x, ln, pad_to, offset):
    y = F.layer_norm(x if offset is None else x + offset.to(x.dtype), ln.normalized_shape, ln.weight, ln.bias, ln.eps)
    if pad_to is not None:
        y = F.pad(y, (0, 0, 0, pad_to[1] - x.shape[2], 0, pad_to[0] - x.shape[1]))
    return y


NORM_CALLS = {"fwd": 0, "bwd": 0}        # launches of ppn_residual_layernorm_train_fwd / ppn_residual_layernorm_bwd (like LOSS_CALLS)
NORM_WIDTHS = frozenset(range(8, 65, 8)) | {128, 256, 512, 1024}          # csrc/residual_ln_bwd.hip: rln_geometry


# Elements from which a PLAIN layer_norm records the kernel pair.  Below, the library's LayerNorm is two framework ops each way whose
# dispatch costs less host time than one Python autograd node, three launches and a workspace, and the tensor is too small for the
# kernels' bandwidth to pay that back (tools/residual_ln_timing.py, DESIGN.md section 22: 3.4x faster at 16.8 M elements, level to
# 0.65x at 8.4 M, 0.62-0.66x at 4.2 M and 2.1 M in both dtypes).  residual_layer_norm replaces four to six framework ops each way and
# was faster on every level shape: no gate.
NORM_RECORD_MIN = 1 << 24


def library_norm():
    """PPNET_LIBRARY_NORM=1 (read at call time, like PPNET_LIBRARY_UPSAMPLE): while autograd records, layer_norm and residual_layer_norm
    take the library composition (the DropPath multiply, gamma *, +, F.layer_norm and the framework's backwards) instead of the HIP
    pair.  Inference is untouched."""
    return bool(os.environ.get("PPNET_LIBRARY_NORM"))


def _norm_kernels_record(x, a, gamma, ln, scale):
    """Whether _ResidualLayerNormFunction takes these tensors while autograd records: CUDA, float32 / bfloat16, the branch and the
    parameters of the activation's dtype, a width the kernels take (NORM_WIDTHS: not ViT-B's 768), a float32 scale per image, and the
    knob off.  Everything else keeps the library composition."""
    if library_norm() or not x.is_cuda or x.dtype not in _DT or x.dim() < 2 or x.numel() == 0 or x.shape[-1] not in NORM_WIDTHS:
        return False
    if ln is not None and (tuple(ln.normalized_shape) != (x.shape[-1],) or ln.weight is None or ln.bias is None):
        return False
    params = (gamma,) + ((ln.weight, ln.bias) if ln is not None else ())
    if any(t is not None and (t.dtype != x.dtype or t.device != x.device or t.numel() != x.shape[-1]) for t in params):
        return False
    if a is not None and (a.dtype != x.dtype or a.device != x.device or a.shape != x.shape):
        return False
    return scale is None or (a is not None and scale.dtype == torch.float32 and scale.device == x.device and scale.dim() == 1
                             and scale.numel() == x.shape[0] and not scale.requires_grad)


def _rln_fwd(x, a, gamma, scale, w, b, eps):
    """ppn_residual_layernorm_train_fwd on contiguous tensors: (x' — x itself for a plain LayerNorm —, y or None, stats or None)."""
    C = x.shape[-1]
    rows = x.numel() // C
    x_out = torch.empty_like(x) if a is not None else None
    y = torch.empty_like(x) if w is not None else None
    stats = torch.empty(rows, 2, dtype=torch.float32, device=x.device) if w is not None else None
    with torch.cuda.device(x.device):
        rc = L.lib.ppn_residual_layernorm_train_fwd(_p(x), _p(a), _p(gamma), _p(scale), _p(w), _p(b), _p(x_out), _p(y), _p(stats), rows,
                                                    rows // x.shape[0], C, float(eps), _DT[x.dtype], _stream(x))
    L.check(rc, "ppn_residual_layernorm_train_fwd")
    NORM_CALLS["fwd"] += 1
    return (x_out if a is not None else x), y, stats


def _rln_bwd(gy, gx, xn, stats, a, gamma, scale, w, want_dx, want_da, want_dgamma, want_dwb):
    """ppn_residual_layernorm_bwd on contiguous tensors: (dx, da, dgamma, dw, dbeta), None where not wanted."""
    ref = gy if gy is not None else gx
    C = ref.shape[-1]
    rows = ref.numel() // C
    dx = torch.empty_like(ref) if want_dx else None
    da = torch.empty_like(ref) if want_da else None
    dgamma = torch.empty_like(gamma) if want_dgamma else None
    dw, dbeta = (torch.empty_like(w), torch.empty_like(w)) if want_dwb else (None, None)
    need = L.lib.ppn_residual_layernorm_bwd_workspace(rows, C)
    ws = torch.empty(max(need, 1), dtype=torch.float32, device=ref.device)
    with torch.cuda.device(ref.device):
        rc = L.lib.ppn_residual_layernorm_bwd(_p(gy), _p(gx), _p(xn), _p(a), _p(gamma), _p(scale), _p(w), _p(stats), _p(dx), _p(da), _p(dgamma),
                                              _p(dw), _p(dbeta), _p(ws), need, rows, rows // ref.shape[0], C, _DT[ref.dtype], _stream(ref))
    L.check(rc, "ppn_residual_layernorm_bwd")
    NORM_CALLS["bwd"] += 1
    return dx, da, dgamma, dw, dbeta


class _ResidualLayerNormFunction(torch.autograd.Function):
    """x' = x + scale[b] * gamma * a, y = LayerNorm(x') on ppn_residual_layernorm_train_fwd / ppn_residual_layernorm_bwd: two outputs
    (x', y), y None without a LayerNorm; a None = a plain LayerNorm, whose single output is y.  Saved: x' and the row statistics
    (with a LayerNorm), the LayerNorm weight, gamma and scale when given, and a when gamma is given (dgamma is its only reader).  y is
    not saved.  A gradient that does not arrive stays None and reaches the kernel as NULL."""

    @staticmethod
    def forward(ctx, x, a, gamma, scale, w, b, eps):
        ctx.set_materialize_grads(False)
        x = x.contiguous()
        a = a.contiguous() if a is not None else None
        gamma, w, b = (t.detach().contiguous() if t is not None else None for t in (gamma, w, b))
        xn, y, stats = _rln_fwd(x, a, gamma, scale, w, b, eps)
        ctx.plain, ctx.has_ln, ctx.has_gamma, ctx.has_scale = a is None, w is not None, gamma is not None, scale is not None
        ctx.save_for_backward(*([xn, stats, w] if ctx.has_ln else []), *([gamma, a] if ctx.has_gamma else []), *([scale] if ctx.has_scale else []))
        return y if ctx.plain else (xn, y)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        gx, gy = (None, grads[0]) if ctx.plain else grads
        saved = list(ctx.saved_tensors)
        xn, stats, w = (saved.pop(0), saved.pop(0), saved.pop(0)) if ctx.has_ln else (None, None, None)
        gamma, a = (saved.pop(0), saved.pop(0)) if ctx.has_gamma else (None, None)
        scale = saved.pop(0) if ctx.has_scale else None
        need_x, need_a, need_gamma, _, need_w, need_b, _ = ctx.needs_input_grad
        if gx is None and gy is None:
            return (None,) * 7
        gx, gy = (t.contiguous() if t is not None else None for t in (gx, gy))
        # da is dx unless LayerScale or stochastic depth scales the branch; without a LayerNorm term dx is gx itself
        own_da = need_a and (ctx.has_gamma or ctx.has_scale)
        own_dx = gy is not None and (need_x or (need_a and not own_da))
        want_dgamma, want_dwb = need_gamma and ctx.has_gamma, gy is not None and (need_w or need_b)
        if own_dx or own_da or want_dgamma or want_dwb:
            dx, da, dgamma, dw, dbeta = _rln_bwd(gy, gx, xn, stats, a, gamma, scale, w, gy is not None, own_da, want_dgamma, want_dwb)
        else:
            dx = da = dgamma = dw = dbeta = None
        if gy is None:
            dx = gx
        return (dx if need_x else None, (da if own_da else dx) if need_a else None, dgamma, None, dw if need_w else None,
                dbeta if need_b else None, None)


def layer_norm(x, ln, pad_to=None, offset=None):
    """y = ln(x) for a torch.nn.LayerNorm over the last dimension. pad_to=(Hp,Wp): x is [B,H,W,C] and y is the
    zero-padded (bottom/right) [B,Hp,Wp,C] grid the next neighbourhood attention wants.  offset [C]: y = ln(x + offset)
    (a residual stream whose constant part is carried outside the tensor, ppn_layernorm_offset).
    Widths of the inference kernels (outside autograd; csrc/fused_norm.hip launch_norm): multiples of 8 up to 64 (without pad_to), then
    C / 8 = 2^k up to 64 lanes (128, 256, 512), 1024, and C / 8 = 3 * 2^k (96, 192, 384, 768, 1536: DiNAT-L's levels, and 24 / 48 with
    pad_to); any other width raises PpnError(PPN_E_UNSUPPORTED).  The recorded pair keeps NORM_WIDTHS."""
    if recording(x, ln.weight, ln.bias):
        if pad_to is None and offset is None and x.numel() >= NORM_RECORD_MIN and _norm_kernels_record(x, None, None, ln, None):
            return _ResidualLayerNormFunction.apply(x, None, None, None, ln.weight, ln.bias, ln.eps)
        return _layer_norm_autograd(x, ln, pad_to, offset)
    x = x.contiguous()
    if offset is not None:
        assert pad_to is None
        C = x.shape[-1]
        y = torch.empty_like(x)
        w, b = ln.weight.detach().to(x.dtype), ln.bias.detach().to(x.dtype)
        off = offset
        assert off.dtype == torch.float32 and off.is_contiguous() and off.device == x.device
        with torch.cuda.device(x.device):
            rc = L.lib.ppn_layernorm_offset(_p(x), _p(off), _p(w), _p(b), _p(y), x.numel() // C, C, float(ln.eps), _DT[x.dtype],
                                            ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
        L.check(rc, "ppn_layernorm_offset")
        return y
    y, pad = _y_for(x, pad_to)
    _call(x, None, None, ln, None, y, pad)
    return y


_LN_REFUSED = set()        # (width, dtype) pairs the LayerNorm kernels answered with PPN_E_UNSUPPORTED

# Widths layer_norm_any_width keeps on the framework's LayerNorm although the kernel takes them: 768 is ViT-B's token width (every
# LayerNorm of vit.py) and the SETR-UP head's norm on its 768-channel features, which ran there while the kernel refused the width.
# Moving ViT-B onto the kernel is a follow-up of its own: it needs an A/B at ViT-B's shapes and a re-measurement of the label
# agreement tests/test_gpu_vit.py pins.  Nothing else reads this set: fused.layer_norm at 768 (DiNAT-L's level 2) runs the kernel.
LN_FRAMEWORK_WIDTHS = frozenset({768})


def layer_norm_any_width(x, ln):
    """ln(x) over the last dimension on the LayerNorm kernel; a row width the kernel does not take (it answers PPN_E_UNSUPPORTED
    before any launch: csrc/fused_norm.hip launch_norm takes C / 8 = 2^k up to 64, 128, and 3 * 2^k up to 1536) runs on the
    framework's LayerNorm instead, and the refusal is remembered.  So does a width of LN_FRAMEWORK_WIDTHS (ViT-B's 768), without asking
    the kernel."""
    key = (x.shape[-1], x.dtype)
    if key[0] not in LN_FRAMEWORK_WIDTHS and key not in _LN_REFUSED:
        try:
            return layer_norm(x, ln)
        except L.PpnError as e:
            if e.code != L.PPN_E_UNSUPPORTED:
                raise
            _LN_REFUSED.add(key)
    return F.layer_norm(x, ln.normalized_shape, ln.weight, ln.bias, ln.eps)


def residual_layer_norm(x, a, gamma, ln_next, pad_to=None, scale=None):
    """x' = x + scale[b] * gamma * a (gamma None = 1; scale None = 1) in place of x; returns (x', ln_next(x')) — y is None when ln_next
    is None.  scale: float32 [B], the per-image stochastic-depth factor (0 = dropped, 1 / keep otherwise) of a training step.
    Under autograd x' is a new tensor and the HIP training pair is recorded (_ResidualLayerNormFunction); CPU tensors, mixed dtypes,
    widths outside NORM_WIDTHS (DiNAT-L's 192 / 384 / 768 / 1536 among them), pad_to and PPNET_LIBRARY_NORM=1 compose the torch ops
    then.  Outside autograd the widths are layer_norm's: one to three passes of the inference kernel, 8 .. 1536."""
    if recording(x, a, gamma, *((ln_next.weight, ln_next.bias) if ln_next is not None else ())):
        if pad_to is None and _norm_kernels_record(x, a, gamma, ln_next, scale):
            w, b = (ln_next.weight, ln_next.bias) if ln_next is not None else (None, None)
            return _ResidualLayerNormFunction.apply(x, a, gamma, scale, w, b, ln_next.eps if ln_next is not None else 0.0)
        if scale is not None:                                               # the DropPath multiply (dense.drop_path) in the branch's dtype
            a = a * scale.view((-1,) + (1,) * (a.dim() - 1)).to(a.dtype)
        x2 = x + (a if gamma is None else gamma * a)
        return x2, (_layer_norm_autograd(x2, ln_next, pad_to, None) if ln_next is not None else None)
    if scale is not None:
        a = a * scale.view((-1,) + (1,) * (a.dim() - 1)).to(a.dtype)
    x = x.contiguous()
    a = a.to(x.dtype).contiguous()
    y, pad = _y_for(x, pad_to) if ln_next is not None else (None, None)
    _call(x, a, gamma.detach() if gamma is not None else None, ln_next, x, y, pad)
    return x, y


def library_upsample():
    """PPNET_LIBRARY_UPSAMPLE=1 (read at call time, like PPNET_LIBRARY_LOSS): while autograd records, the decode heads' up-sampling
    takes the library composition (F.relu, F.interpolate, +, torch.cat and the library's scatter backward) instead of the HIP
    kernels and their backward entries.  Inference is untouched."""
    return bool(os.environ.get("PPNET_LIBRARY_UPSAMPLE"))


def _upsample_kernels_record(*tensors):
    """Whether the up-sampling Functions below take these [B,C,H,W] tensors while autograd records: CUDA, float32 / bfloat16 of one
    dtype, channels a multiple of 8, and the knob off.  Everything else keeps the library composition."""
    t0 = tensors[0]
    return (not library_upsample() and all(t.is_cuda and t.dim() == 4 and t.dtype == t0.dtype and t.device == t0.device and t.shape[1] % 8 == 0
                                           and t.numel() > 0 for t in tensors) and t0.dtype in _DT)


# Output elements from which the SINGLE-operator forms (upsample2x_nhwc, upsample2x_add) record their kernels.  Below, the library
# composition is two framework ops each way, whose dispatch costs less host time than one Python autograd node and two ctypes
# launches, and the tensors are too small for the kernels' bandwidth to pay that back (tools/upsample_bwd_timing.py, DESIGN.md
# section 21: float32 slower up to 4.2 M output elements and faster from 12.8 M; bfloat16 — where the library's atomics round after
# every add — slower at 1.05 M and faster from 1.6 M).  upsample2x_concat and resize_concat replace 4 to 10 framework ops each way
# and were level or faster on every shape: no gate.
UPSAMPLE_RECORD_MIN = {torch.float32: 1 << 23, torch.bfloat16: (1 << 20) + 1}


def _nhwc(t):
    """The contiguous [B,H,W,C] view of a [B,C,H,W] tensor (a copy only when it is not channels_last)."""
    x = t.permute(0, 2, 3, 1)
    return x if x.is_contiguous() else x.contiguous()


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _upsample2x_fwd(x, bias, relu):
    """ppn_upsample2x_nhwc_bias on a contiguous [B,H,W,C] tensor -> [B,2H,2W,C]."""
    B, H, W, C = x.shape
    y = torch.empty(B, 2 * H, 2 * W, C, dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        bias = bias.detach().to(x.dtype).contiguous() if bias is not None else None
        rc = L.lib.ppn_upsample2x_nhwc_bias(_p(x), _p(bias), _p(y), B, H, W, C, 1 if relu else 0, _DT[x.dtype], _stream(x))
    L.check(rc, "ppn_upsample2x_nhwc_bias")
    return y


def _upsample2x_bwd(dy, x):
    """ppn_upsample2x_nhwc_bwd: contiguous dy [B,2H,2W,C] -> dx [B,H,W,C]; x (or None) the forward's input before its folded ReLU."""
    B, H2, W2, C = dy.shape
    H, W = H2 // 2, W2 // 2
    assert x is None or (tuple(x.shape) == (B, H, W, C) and x.dtype == dy.dtype and x.is_contiguous())
    dx = torch.empty(B, H, W, C, dtype=dy.dtype, device=dy.device)
    with torch.cuda.device(dy.device):
        rc = L.lib.ppn_upsample2x_nhwc_bwd(_p(dy), _p(x), _p(dx), B, H, W, C, _DT[dy.dtype], _stream(dy))
    L.check(rc, "ppn_upsample2x_nhwc_bwd")
    return dx


class _Upsample2xFunction(torch.autograd.Function):
    """ppn_upsample2x_nhwc / ppn_upsample2x_nhwc_bwd.  Saves the input only when the ReLU is folded in (its sign is the mask)."""

    @staticmethod
    def forward(ctx, x_nchw, relu):
        x = _nhwc(x_nchw)
        ctx.relu = bool(relu)
        if ctx.relu:
            ctx.save_for_backward(x)
        return _upsample2x_fwd(x, None, ctx.relu).permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        x = ctx.saved_tensors[0] if ctx.relu else None
        return _upsample2x_bwd(_nhwc(grad), x).permute(0, 3, 1, 2), None


def upsample2x_nhwc(x_nchw_cl, relu=False, bias=None):
    """Bilinear x2 (align_corners=False) of a channels_last [B,C,H,W] tensor, optionally with a per-channel bias and a
    ReLU folded into the loads (conv -> folded BN -> ReLU -> Upsample with a bias-free library convolution).  Returns a
    channels_last [B,C,2H,2W] tensor (zero-copy views on both sides).  While autograd records, the same kernel runs behind
    _Upsample2xFunction (backward: ppn_upsample2x_nhwc_bwd); a bias (prepared modules only, which do not train), a channel count
    that is no multiple of 8, an output below UPSAMPLE_RECORD_MIN elements and PPNET_LIBRARY_UPSAMPLE=1 take the library
    composition then."""
    if recording(x_nchw_cl, bias):
        if bias is None and _upsample_kernels_record(x_nchw_cl) and 4 * x_nchw_cl.numel() >= UPSAMPLE_RECORD_MIN[x_nchw_cl.dtype]:
            return _Upsample2xFunction.apply(x_nchw_cl, relu)
        t = x_nchw_cl if bias is None else x_nchw_cl + bias.view(1, -1, 1, 1)
        return F.interpolate(F.relu(t) if relu else t, scale_factor=2.0, mode="bilinear", align_corners=False)
    if not x_nchw_cl.is_cuda:
        raise RuntimeError("ppnet_amd.fused: GPU tensors only (no CPU fallback)")
    return _upsample2x_fwd(_nhwc(x_nchw_cl), bias, relu).permute(0, 3, 1, 2)


def upsample2x_add_(fine, coarse):
    """fine += bilinear x2 (align_corners=False) of coarse, in place: the FPN's top-down step (uper_head.py:103-108) on channels_last
    [B,C,2H,2W] / [B,C,H,W] tensors, one kernel (ppn_upsample2x_add_nhwc) instead of interpolate + add."""
    f, c = fine.permute(0, 2, 3, 1), coarse.permute(0, 2, 3, 1)
    if not c.is_contiguous():
        c = c.contiguous()
    B, H, W, C = c.shape
    assert f.is_contiguous() and f.is_cuda and f.dtype == c.dtype and f.dtype in _DT and tuple(f.shape) == (B, 2 * H, 2 * W, C)
    with torch.cuda.device(f.device):
        rc = L.lib.ppn_upsample2x_add_nhwc(_p(c), _p(f), _p(f), B, H, W, C, _DT[f.dtype], ctypes.c_void_p(torch.cuda.current_stream(f.device).cuda_stream))
    L.check(rc, "ppn_upsample2x_add_nhwc")
    return fine


def _upsample2x_add_fwd(f, c):
    """ppn_upsample2x_add_nhwc out of place on contiguous NHWC tensors: a new [B,2H,2W,C] tensor = f + (c resized x2)."""
    B, H, W, C = c.shape
    if tuple(f.shape) != (B, 2 * H, 2 * W, C):
        raise RuntimeError(f"upsample2x_add: fine {tuple(f.shape)} is not twice coarse {tuple(c.shape)} (NHWC)")
    y = torch.empty_like(f)
    with torch.cuda.device(f.device):
        rc = L.lib.ppn_upsample2x_add_nhwc(_p(c), _p(f), _p(y), B, H, W, C, _DT[f.dtype], _stream(f))
    L.check(rc, "ppn_upsample2x_add_nhwc")
    return y


class _Upsample2xAddFunction(torch.autograd.Function):
    """ppn_upsample2x_add_nhwc out of place.  Saves nothing: the gradient passes through to `fine` and goes through
    ppn_upsample2x_nhwc_bwd to `coarse`."""

    @staticmethod
    def forward(ctx, fine, coarse):
        return _upsample2x_add_fwd(_nhwc(fine), _nhwc(coarse)).permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        d_coarse = _upsample2x_bwd(_nhwc(grad), None).permute(0, 3, 1, 2) if ctx.needs_input_grad[1] else None
        return (grad if ctx.needs_input_grad[0] else None), d_coarse


def upsample2x_add(fine, coarse):
    """fine + bilinear x2 (align_corners=False) of coarse as a NEW channels_last tensor: the differentiable form of upsample2x_add_
    (one ppn_upsample2x_add_nhwc; backward: the identity to `fine`, ppn_upsample2x_nhwc_bwd to `coarse`).  CPU tensors, other dtypes,
    channels that are no multiple of 8 and, while autograd records, an output below UPSAMPLE_RECORD_MIN elements and
    PPNET_LIBRARY_UPSAMPLE=1 take interpolate + add."""
    kernel_types = fine.is_cuda and coarse.is_cuda and fine.dtype == coarse.dtype and fine.dtype in _DT and coarse.shape[1] % 8 == 0
    if recording(fine, coarse):
        if _upsample_kernels_record(fine, coarse) and fine.numel() >= UPSAMPLE_RECORD_MIN[fine.dtype]:
            return _Upsample2xAddFunction.apply(fine, coarse)
    elif kernel_types:
        return _upsample2x_add_fwd(_nhwc(fine), _nhwc(coarse)).permute(0, 3, 1, 2)
    return fine + F.interpolate(coarse, scale_factor=2.0, mode="bilinear", align_corners=False)


def _upsample2x_concat_fwd(xs):
    B, H, W, _ = xs[0].shape
    n = len(xs)
    out = torch.empty(B, 2 * H, 2 * W, sum(x.shape[3] for x in xs), dtype=xs[0].dtype, device=xs[0].device)
    ptrs = (ctypes.c_void_p * n)(*[x.data_ptr() for x in xs])
    ch = (ctypes.c_int32 * n)(*[x.shape[3] for x in xs])
    with torch.cuda.device(out.device):
        rc = L.lib.ppn_upsample2x_concat_nhwc(ptrs, ch, n, _p(out), B, H, W, _DT[xs[0].dtype], _stream(out))
    L.check(rc, "ppn_upsample2x_concat_nhwc")
    return out


class _Upsample2xConcatFunction(torch.autograd.Function):
    """ppn_upsample2x_concat_nhwc / ppn_upsample2x_concat_nhwc_bwd.  Saves nothing but the channel counts."""

    @staticmethod
    def forward(ctx, *levels):
        xs = [_nhwc(t) for t in levels]
        ctx.channels = [x.shape[3] for x in xs]
        return _upsample2x_concat_fwd(xs).permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        dout = _nhwc(grad)
        B, H2, W2, _ = dout.shape
        n = len(ctx.channels)
        dxs = [torch.empty(B, H2 // 2, W2 // 2, c, dtype=dout.dtype, device=dout.device) for c in ctx.channels]
        ptrs = (ctypes.c_void_p * n)(*[d.data_ptr() for d in dxs])
        ch = (ctypes.c_int32 * n)(*ctx.channels)
        with torch.cuda.device(dout.device):
            rc = L.lib.ppn_upsample2x_concat_nhwc_bwd(_p(dout), ptrs, ch, n, B, H2 // 2, W2 // 2, _DT[dout.dtype], _stream(dout))
        L.check(rc, "ppn_upsample2x_concat_nhwc_bwd")
        return tuple(d.permute(0, 3, 1, 2) for d in dxs)


def upsample2x_concat(levels):
    """Up to eight channels_last [B,C_l,H,W] tensors of ONE size, each bilinearly up-sampled x2 (align_corners=False) into its channel
    range of one output, in ONE kernel (ppn_upsample2x_concat_nhwc): UPerPUPHead's last Upsample of every FPN chain and the
    concatenation behind them (uper_pup_head.py:121-128).  Returns a channels_last [B, sum C_l, 2H, 2W] tensor.  Differentiable
    (ppn_upsample2x_concat_nhwc_bwd); PPNET_LIBRARY_UPSAMPLE=1 composes interpolate + torch.cat while autograd records."""
    assert 1 <= len(levels) <= 8
    if any(tuple(t.shape[2:]) != tuple(levels[0].shape[2:]) or t.shape[0] != levels[0].shape[0] for t in levels):
        raise RuntimeError(f"upsample2x_concat: levels of different sizes {[tuple(t.shape[2:]) for t in levels]}")
    if recording(*levels):
        if _upsample_kernels_record(*levels):
            return _Upsample2xConcatFunction.apply(*levels)
        return torch.cat([F.interpolate(t, scale_factor=2.0, mode="bilinear", align_corners=False) for t in levels], dim=1)
    xs = [_nhwc(t) for t in levels]
    assert all(x.is_cuda and x.dtype == xs[0].dtype and x.shape[3] % 8 == 0 for x in xs) and xs[0].dtype in _DT
    return _upsample2x_concat_fwd(xs).permute(0, 3, 1, 2)


def _resize_concat_fwd(xs):
    B, H0, W0, _ = xs[0].shape
    n = len(xs)
    out = torch.empty(B, H0, W0, sum(x.shape[3] for x in xs), dtype=xs[0].dtype, device=xs[0].device)
    ptrs = (ctypes.c_void_p * n)(*[x.data_ptr() for x in xs])
    hw = (ctypes.c_int32 * (2 * n))(*[v for x in xs for v in (x.shape[1], x.shape[2])])
    ch = (ctypes.c_int32 * n)(*[x.shape[3] for x in xs])
    with torch.cuda.device(out.device):
        rc = L.lib.ppn_resize_concat_nhwc(ptrs, hw, ch, n, _p(out), B, _DT[xs[0].dtype], _stream(out))
    L.check(rc, "ppn_resize_concat_nhwc")
    return out


class _ResizeConcatFunction(torch.autograd.Function):
    """ppn_resize_concat_nhwc / ppn_resize_concat_nhwc_bwd.  Saves nothing but the levels' sizes and channel counts."""

    @staticmethod
    def forward(ctx, *levels):
        xs = [_nhwc(t) for t in levels]
        ctx.sizes = [tuple(x.shape[1:]) for x in xs]
        return _resize_concat_fwd(xs).permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        dout = _nhwc(grad)
        B, n = dout.shape[0], len(ctx.sizes)
        dxs = [torch.empty(B, h, w, c, dtype=dout.dtype, device=dout.device) for h, w, c in ctx.sizes]
        ptrs = (ctypes.c_void_p * n)(*[d.data_ptr() for d in dxs])
        hw = (ctypes.c_int32 * (2 * n))(*[v for h, w, _ in ctx.sizes for v in (h, w)])
        ch = (ctypes.c_int32 * n)(*[c for _, _, c in ctx.sizes])
        with torch.cuda.device(dout.device):
            rc = L.lib.ppn_resize_concat_nhwc_bwd(_p(dout), ptrs, hw, ch, n, B, _DT[dout.dtype], _stream(dout))
        L.check(rc, "ppn_resize_concat_nhwc_bwd")
        return tuple(d.permute(0, 3, 1, 2) for d in dxs)


def resize_concat(levels):
    """Up to eight channels_last [B,C_l,H_l,W_l] tensors, each bilinearly resized (align_corners=False) to the FIRST one's size and
    concatenated over channels in ONE kernel (ppn_resize_concat_nhwc): UPerHead's FPN output assembly (uper_head.py:117-127) and
    its pyramid pooling module's output (psp_head.py:48-60).  Returns a channels_last [B, sum C_l, H_0, W_0] tensor.  Differentiable
    (ppn_resize_concat_nhwc_bwd) when no level is larger than the first; otherwise, and with PPNET_LIBRARY_UPSAMPLE=1, interpolate +
    torch.cat are composed while autograd records."""
    assert 1 <= len(levels) <= 8
    if recording(*levels):
        H0, W0 = levels[0].shape[2:]
        if _upsample_kernels_record(*levels) and all(t.shape[0] == levels[0].shape[0] and t.shape[2] <= H0 and t.shape[3] <= W0 for t in levels):
            return _ResizeConcatFunction.apply(*levels)
        return torch.cat([levels[0]] + [F.interpolate(t, size=(H0, W0), mode="bilinear", align_corners=False) for t in levels[1:]], dim=1)
    xs = [_nhwc(t) for t in levels]
    B = xs[0].shape[0]
    assert all(x.is_cuda and x.dtype == xs[0].dtype and x.shape[0] == B and x.shape[3] % 8 == 0 for x in xs) and xs[0].dtype in _DT
    return _resize_concat_fwd(xs).permute(0, 3, 1, 2)


def resize_concat4(levels):
    """The four-level form (UPerHead's FPN output assembly)."""
    assert len(levels) == 4
    return resize_concat(levels)


def adaptive_pools(x_nchw_cl, scales):
    """nn.AdaptiveAvgPool2d(s) for every s in `scales` (<= 4) of one channels_last [B,C,H,W] tensor in ONE kernel
    (ppn_adaptive_pools_nhwc; psp_head.py:33-38).  Returns channels_last [B,C,s,s] tensors."""
    x = x_nchw_cl.permute(0, 2, 3, 1)
    if not x.is_contiguous():
        x = x.contiguous()
    B, H, W, C = x.shape
    n = len(scales)
    assert x.is_cuda and x.dtype in _DT and 1 <= n <= 4 and C % 8 == 0
    ys = [torch.empty(B, s, s, C, dtype=x.dtype, device=x.device) for s in scales]
    ptrs = (ctypes.c_void_p * n)(*[y.data_ptr() for y in ys])
    sc = (ctypes.c_int32 * n)(*[int(s) for s in scales])
    with torch.cuda.device(x.device):
        rc = L.lib.ppn_adaptive_pools_nhwc(_p(x), ptrs, sc, n, B, H, W, C, _DT[x.dtype], ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
    L.check(rc, "ppn_adaptive_pools_nhwc")
    return [y.permute(0, 3, 1, 2) for y in ys]


def bias_act_(x_nchw_cl, bias, negative_slope):
    """In place leaky_relu(x + bias[c], negative_slope) on a channels_last [B,C,H,W] tensor (slope 0 = ReLU, 1 = bias
    only).  Returns x."""
    if not x_nchw_cl.is_cuda:
        raise RuntimeError("ppnet_amd.fused: GPU tensors only (no CPU fallback)")
    assert x_nchw_cl.is_contiguous(memory_format=torch.channels_last)
    C = x_nchw_cl.shape[1]
    with torch.cuda.device(x_nchw_cl.device):
        rc = L.lib.ppn_bias_act_nhwc(_p(x_nchw_cl), _p(bias.detach().to(x_nchw_cl.dtype).contiguous()), x_nchw_cl.numel(), C,
                                     float(negative_slope), _DT[x_nchw_cl.dtype],
                                     ctypes.c_void_p(torch.cuda.current_stream(x_nchw_cl.device).cuda_stream))
    L.check(rc, "ppn_bias_act_nhwc")
    return x_nchw_cl


def conv3x3_c1(x, w32, b32, negative_slope):
    """leaky_relu(conv2d(x [B,1,H,W], weight [Cout,1,3,3], bias, stride 1, padding 1), slope) -> channels_last [B,Cout,H,W].
    w32 / b32: the weight and bias as contiguous float32 device tensors."""
    if not x.is_cuda:
        raise RuntimeError("ppnet_amd.fused: GPU tensors only (no CPU fallback)")
    B, _, H, W = x.shape
    Cout = w32.shape[0]
    x = x.contiguous()
    y = torch.empty(B, H, W, Cout, dtype=x.dtype, device=x.device)
    assert w32.dtype == torch.float32 and b32.dtype == torch.float32 and w32.is_contiguous() and b32.is_contiguous()
    with torch.cuda.device(x.device):
        rc = L.lib.ppn_conv3x3_c1_nhwc(_p(x), _p(w32), _p(b32), _p(y), B, H, W, Cout, float(negative_slope), _DT[x.dtype],
                                       ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
    L.check(rc, "ppn_conv3x3_c1_nhwc")
    return y.permute(0, 3, 1, 2)


def conv3x3_to1(x_nchw_cl, w32, bias):
    """conv2d(x channels_last [B,Cin,H,W], weight [1,Cin,3,3], bias, stride 1, padding 1) -> [B,1,H,W].
    w32: the weight as a contiguous float32 device tensor; bias: a Python float."""
    if not x_nchw_cl.is_cuda:
        raise RuntimeError("ppnet_amd.fused: GPU tensors only (no CPU fallback)")
    x = x_nchw_cl.permute(0, 2, 3, 1)
    if not x.is_contiguous():
        x = x.contiguous()
    B, H, W, Cin = x.shape
    y = torch.empty(B, 1, H, W, dtype=x.dtype, device=x.device)
    assert w32.dtype == torch.float32 and w32.is_contiguous()
    with torch.cuda.device(x.device):
        rc = L.lib.ppn_conv3x3_to1_nhwc(_p(x), _p(w32), float(bias), _p(y), B, H, W, Cin,
                                        _DT[x.dtype], ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
    L.check(rc, "ppn_conv3x3_to1_nhwc")
    return y


def seg_labels_2class(logits_lo, out_hw):
    """u8 labels [B,Ho,Wo] of a two-class segmentor from its low-resolution logits [B,2,h,w]: x2 bilinear, bilinear to out_hw,
    float32 softmax, argmax — the three library kernels of the reference tail in one (ppn_seg_labels_2class)."""
    if not logits_lo.is_cuda:
        raise RuntimeError("ppnet_amd.fused: GPU tensors only (no CPU fallback)")
    x = logits_lo.contiguous()
    B, C2, h, w = x.shape
    assert C2 == 2
    labels = torch.empty(B, out_hw[0], out_hw[1], dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        rc = L.lib.ppn_seg_labels_2class(_p(x), _p(labels), B, h, w, out_hw[0], out_hw[1], _DT[x.dtype],
                                         ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
    L.check(rc, "ppn_seg_labels_2class")
    return labels


AUG_FLIP, AUG_BRIGHTNESS, AUG_CONTRAST, AUG_CONTRAST_LAST, AUG_SATURATION, AUG_HUE = 1, 2, 4, 8, 16, 32   # include/ppnet_hip.h: PPN_AUG_*
AUG_PARAM_WORDS = 8                      # flags, beta f32, alpha f32, alpha_s f32, delta i32, three reserved zeros


def augment_params(seed, first_instance, B, device, flip_ratio=0.5, brightness_delta=32.0, contrast_range=(0.5, 1.5),
                   saturation_range=(0.5, 1.5), hue_delta=18):
    """int32 [B, 8] per-image parameters of augment_codes / augment_rgb, drawn on the device from Philox stream 5 with instance
    first_instance + b (ppn_augment_params; the draw slots are in include/ppnet_hip.h).  The float32 words are held as their bits."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("ppnet_amd.fused: GPU tensors only (no CPU fallback)")
    params = torch.empty(B, AUG_PARAM_WORDS, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        rc = L.lib.ppn_augment_params(int(seed) & (2 ** 64 - 1), int(first_instance) & (2 ** 64 - 1), B, flip_ratio, brightness_delta,
                                      contrast_range[0], contrast_range[1], saturation_range[0], saturation_range[1], int(hue_delta),
                                      _p(params), ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream))
    L.check(rc, "ppn_augment_params")
    return params


def _augment(entry, name, src, labels, params, mean, std, dtype, out_size, seg_pad_val):
    if not src.is_cuda or not params.is_cuda or (labels is not None and not labels.is_cuda):
        raise RuntimeError("ppnet_amd.fused: GPU tensors only (no CPU fallback)")
    if src.dtype != torch.uint8 or (labels is not None and labels.dtype != torch.uint8) or params.dtype != torch.int32:
        raise ValueError(f"{name}: uint8 input and labels, int32 parameters")
    src, params = src.contiguous(), params.contiguous()
    B, H, W = src.shape[:3]
    Ho, Wo = (H, W) if out_size is None else out_size
    if tuple(params.shape) != (B, AUG_PARAM_WORDS) or (labels is not None and tuple(labels.shape) != (B, H, W)):
        raise ValueError(f"{name}: parameters {tuple(params.shape)} / labels {None if labels is None else tuple(labels.shape)} do not "
                         f"belong to a batch of {B} images of {H} x {W}")
    img = torch.empty(B, Ho, Wo, 3, dtype=dtype, device=src.device)
    lab_in = labels.contiguous() if labels is not None else None
    lab_out = torch.empty(B, Ho, Wo, dtype=torch.uint8, device=src.device) if labels is not None else None
    m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    with torch.cuda.device(src.device):
        rc = entry(_p(src), _p(lab_in), _p(params), _p(img), _p(lab_out), B, H, W, Ho, Wo, m3, s3, int(seg_pad_val), _DT[dtype],
                   ctypes.c_void_p(torch.cuda.current_stream(src.device).cuda_stream))
    L.check(rc, name)
    return img.permute(0, 3, 1, 2), lab_out


def augment_codes(grid_u8, labels, params, mean, std, dtype, out_size=None, seg_pad_val=255):
    """SegNet's TRAINING input from stage B's u8 codes [B,H,W]: the reference's flip + photometric distortion + normalise + pad
    with the per-image parameters `params` (augment_params), one kernel (ppn_augment_codes).  Returns (image: channels_last
    [B,3,Ho,Wo] of `dtype`, labels u8 [B,Ho,Wo] flipped and padded with the image, or None when `labels` is None)."""
    if grid_u8.dim() != 3:
        raise ValueError(f"augment_codes: [B,H,W] codes, got {tuple(grid_u8.shape)}")
    return _augment(L.lib.ppn_augment_codes, "ppn_augment_codes", grid_u8, labels, params, mean, std, dtype, out_size, seg_pad_val)


def augment_rgb(rgb_u8, labels, params, mean, std, dtype, out_size=None, seg_pad_val=255):
    """augment_codes for u8 RGB images [B,H,W,3] (ppn_augment_rgb): the same colour function on every pixel."""
    if rgb_u8.dim() != 4 or rgb_u8.shape[-1] != 3:
        raise ValueError(f"augment_rgb: [B,H,W,3] images, got {tuple(rgb_u8.shape)}")
    return _augment(L.lib.ppn_augment_rgb, "ppn_augment_rgb", rgb_u8, labels, params, mean, std, dtype, out_size, seg_pad_val)


def grid_to_image(grid_u8, mean, std, dtype):
    """Normalised SegNet input, channels_last [B,3,R,R] of `dtype`, from stage B's u8 codes [B,R,R] (ppn_grid_to_image)."""
    if not grid_u8.is_cuda:
        raise RuntimeError("ppnet_amd.fused: GPU tensors only (no CPU fallback)")
    g = grid_u8.contiguous()
    B, H, W = g.shape
    img = torch.empty(B, H, W, 3, dtype=dtype, device=g.device)
    m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    with torch.cuda.device(g.device):
        rc = L.lib.ppn_grid_to_image(_p(g), _p(img), g.numel(), m3, s3, _DT[dtype], ctypes.c_void_p(torch.cuda.current_stream(g.device).cuda_stream))
    L.check(rc, "ppn_grid_to_image")
    return img.permute(0, 3, 1, 2)


def heatmap_u8(y):
    """[B,R,R] u8 = per-sample min-max normalised y [B,1,R,R] or [B,R,R] (float32 / bfloat16) times 255, truncated
    (ppn_heatmap_u8; GenNet/predict.py:95-102)."""
    if not y.is_cuda or y.dtype not in _DT:
        raise RuntimeError("ppnet_amd.fused.heatmap_u8: float32 / bfloat16 GPU tensors only")
    y = y.contiguous()
    B, H, W = y.shape[0], y.shape[-2], y.shape[-1]
    assert y.numel() == B * H * W
    out = torch.empty(B, H, W, dtype=torch.uint8, device=y.device)
    with torch.cuda.device(y.device):
        rc = L.lib.ppn_heatmap_u8(_p(y), _p(out), B, H * W, _DT[y.dtype], ctypes.c_void_p(torch.cuda.current_stream(y.device).cuda_stream))
    L.check(rc, "ppn_heatmap_u8")
    return out


def tokenizer_lut(conv, mean, std):
    """The [2][64][32] bfloat16 table ppn_tokenizer_conv1_codes_bf16 reads, from the tokenizer's first convolution
    (Conv2d(3, 64, 3, 2, 1), bfloat16 parameters) and the image normalisation: column 3 * (ky * 3 + kx) + colour holds
    sum_ci w[co][ci][ky][kx] * image_ci(colour) with the image values rounded to bfloat16 as ppn_grid_to_image stores them
    (colour 0 = free (255,255,255), 1 = marker (255,0,0), 2 = other (0,0,0)); column 27 the bias; hi + lo split."""
    w = conv.weight.detach().double()                                                    # [64,3,3,3]
    assert w.shape == (64, 3, 3, 3)
    lo = torch.tensor([(0.0 - m) / s for m, s in zip(mean, std)], dtype=torch.float32).to(torch.bfloat16).double()
    hi = torch.tensor([(255.0 - m) / s for m, s in zip(mean, std)], dtype=torch.float32).to(torch.bfloat16).double()
    pal = torch.stack([hi, torch.stack([hi[0], lo[1], lo[2]]), lo]).to(w.device)         # [colour][ci]
    table = torch.zeros(64, 32, dtype=torch.float64, device=w.device)
    table[:, :27] = torch.einsum("oikl,ci->oklc", w, pal).reshape(64, 27)               # k = (ky * 3 + kx) * 3 + colour
    if conv.bias is not None:
        table[:, 27] = conv.bias.detach().double()
    t_hi = table.to(torch.float32).to(torch.bfloat16)
    t_lo = (table - t_hi.double()).to(torch.float32).to(torch.bfloat16)
    t_lo[:, 27:] = 0
    return torch.stack([t_hi, t_lo]).contiguous()        # rows = channels; each kernel applies its own row order when it loads


def tokenizer_pack(conv2, ln):
    """(w2p, vec) of ppn_tokenizer_codes_bf16 from the tokenizer's second convolution (Conv2d(64, 128, 3, 2, 1), bfloat16) and its
    LayerNorm: the weight as MFMA A fragments [8][9][2][16][32] and [3][128] float32 = (conv bias, LN weight, LN bias)."""
    w = conv2.weight.detach().float()                                      # [co 128][ci 64][ky][kx]
    assert w.shape == (128, 64, 3, 3)
    dev = w.device
    co = torch.tensor([[(nt >> 2) * 64 + 16 * (i >> 2) + 4 * (nt & 3) + (i & 3) for i in range(16)] for nt in range(8)], device=dev)         # [8][16]
    ci = torch.tensor([[(2 * s + (e >> 2)) * 16 + 4 * g + (e & 3) for g in range(4) for e in range(8)] for s in range(2)], device=dev)      # [2][32]
    taps = w.reshape(128, 64, 9)
    w2p = taps[co][:, :, ci]                                               # [8][16][2][32][9]
    w2p = w2p.permute(0, 4, 2, 1, 3).contiguous()                          # [8][9][2][16][32]
    bias = conv2.bias.detach().float() if conv2.bias is not None else torch.zeros(128, device=dev)
    vec = torch.stack([bias, ln.weight.detach().float(), ln.bias.detach().float()]).contiguous()
    return w2p.to(torch.bfloat16).contiguous(), vec


def tokenizer_codes(grid_u8, lut, w2p, vec, eps):
    """Tokens [B,R/4,R/4,128] bfloat16 of the palette image of u8 occupancy codes [B,R,R]: both tokenizer convolutions and the
    LayerNorm in one kernel (ppn_tokenizer_codes_bf16)."""
    if not grid_u8.is_cuda or grid_u8.dtype != torch.uint8:
        raise RuntimeError("ppnet_amd.fused.tokenizer_codes: u8 GPU code grids only")
    g = grid_u8.contiguous()
    B, H, W = g.shape
    assert lut.shape == (2, 64, 32) and w2p.shape == (8, 9, 2, 16, 32) and vec.shape == (3, 128)
    assert lut.dtype == w2p.dtype == torch.bfloat16 and vec.dtype == torch.float32 and lut.is_contiguous() and w2p.is_contiguous() and vec.is_contiguous()
    out = torch.empty(B, H // 4, W // 4, 128, dtype=torch.bfloat16, device=g.device)
    with torch.cuda.device(g.device):
        rc = L.lib.ppn_tokenizer_codes_bf16(_p(g), _p(lut), _p(w2p), _p(vec), _p(out), B, H, W, float(eps),
                                            ctypes.c_void_p(torch.cuda.current_stream(g.device).cuda_stream))
    L.check(rc, "ppn_tokenizer_codes_bf16")
    return out


def tokenizer_conv1_codes(grid_u8, lut):
    """[B,R/2,R/2,64] bfloat16 = the tokenizer's first convolution applied to the palette image of the u8 occupancy codes
    [B,R,R] (ppn_tokenizer_conv1_codes_bf16); lut from tokenizer_lut."""
    if not grid_u8.is_cuda or grid_u8.dtype != torch.uint8:
        raise RuntimeError("ppnet_amd.fused.tokenizer_conv1_codes: u8 GPU code grids only")
    g = grid_u8.contiguous()
    B, H, W = g.shape
    assert lut.shape == (2, 64, 32) and lut.dtype == torch.bfloat16 and lut.is_contiguous() and lut.device == g.device
    out = torch.empty(B, H // 2, W // 2, 64, dtype=torch.bfloat16, device=g.device)
    with torch.cuda.device(g.device):
        rc = L.lib.ppn_tokenizer_conv1_codes_bf16(_p(g), _p(lut), _p(out), B, H, W, ctypes.c_void_p(torch.cuda.current_stream(g.device).cuda_stream))
    L.check(rc, "ppn_tokenizer_conv1_codes_bf16")
    return out


def conv3x3_mfma(x_nchw_cl, w_k, bias32, stride=1, relu=False):
    """3x3 convolution (padding 1) of a channels_last bfloat16 [B,Cin,H,W] tensor on the MFMA implicit-GEMM kernel
    (ppn_conv3x3_mfma_bf16).  w_k: the weight as [Cout,3,3,Cin] bfloat16 (weight.permute(0,2,3,1).contiguous()); bias32:
    float32 [Cout].  Returns channels_last [B,Cout,Ho,Wo]."""
    if not x_nchw_cl.is_cuda or x_nchw_cl.dtype != torch.bfloat16:
        raise RuntimeError("ppnet_amd.fused.conv3x3_mfma: bfloat16 GPU tensors only")
    x = x_nchw_cl.permute(0, 2, 3, 1)
    if not x.is_contiguous():
        x = x.contiguous()
    B, H, W, Cin = x.shape
    Cout = w_k.shape[0]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    assert w_k.dtype == torch.bfloat16 and w_k.is_contiguous() and w_k.shape == (Cout, 3, 3, Cin)
    assert bias32.dtype == torch.float32 and bias32.is_contiguous() and bias32.numel() == Cout
    y = torch.empty(B, Ho, Wo, Cout, dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        rc = L.lib.ppn_conv3x3_mfma_bf16(_p(x), _p(w_k), _p(bias32), _p(y), B, H, W, Cin, Cout, stride, 1 if relu else 0,
                                         ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
    L.check(rc, "ppn_conv3x3_mfma_bf16")
    return y.permute(0, 3, 1, 2)


def conv3x3_relu_classify2(x_nchw_cl, w_k, bias32, w2_32, b2_32):
    """relu(conv3x3(x) + bias) followed by a 2-class 1x1 classifier, without writing the Cout-channel activation
    (ppn_conv3x3_relu_classify2_bf16).  w2_32 [2,Cout], b2_32 [2] float32.  Returns float32 logits [B,2,H,W]."""
    if not x_nchw_cl.is_cuda or x_nchw_cl.dtype != torch.bfloat16:
        raise RuntimeError("ppnet_amd.fused.conv3x3_relu_classify2: bfloat16 GPU tensors only")
    x = x_nchw_cl.permute(0, 2, 3, 1)
    if not x.is_contiguous():
        x = x.contiguous()
    B, H, W, Cin = x.shape
    Cout = w_k.shape[0]
    logits = b2_32.to(torch.float32).repeat(B * H * W).view(B, H, W, 2).contiguous()
    slots = L.lib.ppn_conv3x3_relu_classify2_slots(Cout)            # 0 for Cout <= 256: the kernel adds straight onto the logits
    partial = torch.empty(slots, B * H * W, 2, dtype=torch.float32, device=x.device) if slots > 0 else None
    with torch.cuda.device(x.device):
        rc = L.lib.ppn_conv3x3_relu_classify2_bf16(_p(x), _p(w_k), _p(bias32), _p(w2_32), _p(logits), _p(partial), B, H, W, Cin, Cout,
                                                   ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
    L.check(rc, "ppn_conv3x3_relu_classify2_bf16")
    return logits.permute(0, 3, 1, 2)


def gemm_bf16(a, w, bias32, epilogue="bias", out=None, persistent_blocks=0):
    """out[M,N] = epilogue(a[M,K] @ w[N,K]^T) on the MFMA kernel (ppn_gemm_bf16).  epilogue: "bias", "bias_gelu", or "accum"
    (out += a @ w^T, bias unused)."""
    epi = {"bias": 0, "bias_gelu": 1, "accum": 2, "bias_relu": 3}[epilogue]
    M, K = a.shape
    N = w.shape[0]
    assert a.is_cuda and a.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and a.is_contiguous() and w.is_contiguous()
    if out is None:
        assert epi != 2
        out = torch.empty(M, N, dtype=a.dtype, device=a.device)
    assert out.is_contiguous() and out.shape == (M, N)
    with torch.cuda.device(a.device):
        rc = L.lib.ppn_gemm_bf16(_p(a), _p(w), _p(bias32), _p(out), M, N, K, epi, persistent_blocks,
                                 ctypes.c_void_p(torch.cuda.current_stream(a.device).cuda_stream))
    L.check(rc, "ppn_gemm_bf16")
    return out


def nat_gemm(a, w, bias32, mode, out, colsum=None, stats_in=None, stats_out=None, eps=1e-5):
    """The NAT projections with the LayerNorm / residual / statistics in the epilogue (ppn_nat_gemm_bf16, csrc/mfma_gemm.h).
    mode "ln": out = LN(a) W0^T + b0 from the raw rows of a (w = W0 diag(gamma), bias32 = b0 + W0 beta, colsum, stats_in
    [P, M, 2]); "ln_gelu": gelu of that; "acc": out += a w^T + bias32 in place, row partials of the new out -> stats_out
    [nat_partials(N), M, 2]."""
    md = {"ln": 0, "ln_gelu": 1, "acc": 2}[mode]
    M, K = a.shape
    N = w.shape[0]
    assert a.is_cuda and a.dtype == w.dtype == out.dtype == torch.bfloat16 and a.is_contiguous() and w.is_contiguous() and out.is_contiguous()
    assert w.shape == (N, K) and out.shape == (M, N) and bias32.dtype == torch.float32 and bias32.numel() == N and bias32.is_contiguous()
    P = 0
    if md != 2:
        assert colsum.dtype == torch.float32 and colsum.numel() == N and colsum.is_contiguous()
        assert stats_in.dtype == torch.float32 and stats_in.is_contiguous() and stats_in.dim() == 3 and stats_in.shape[1:] == (M, 2)
        P = stats_in.shape[0]
    else:
        assert stats_out.dtype == torch.float32 and stats_out.is_contiguous() and stats_out.shape == (nat_partials(N), M, 2)
    with torch.cuda.device(a.device):
        rc = L.lib.ppn_nat_gemm_bf16(_p(a), _p(w), _p(bias32), _p(colsum), _p(stats_in), P, _p(stats_out), _p(out), M, N, K, md, float(eps),
                                     ctypes.c_void_p(torch.cuda.current_stream(a.device).cuda_stream))
    L.check(rc, "ppn_nat_gemm_bf16")
    return out


def nat_mlp_ok(M, C, hidden):
    """Shapes the fused MLP kernel serves (ppn_nat_mlp_supported): C = 256 streams, whole 128-token blocks."""
    return bool(L.lib.ppn_nat_mlp_supported(int(M), int(C), int(hidden)))


def nat_mlp_pack(w1_folded, w2):
    """The two MLP weights in the fused kernel's streaming order (ppn_nat_mlp_pack_bf16): w1_folded [hidden, C] = W1 diag(gamma)
    (LayerNorm folded in), w2 [C, hidden] (LayerScale folded in), both bfloat16 -> one bfloat16 tensor of 2 * C * hidden."""
    hid, Cc = w1_folded.shape
    assert w1_folded.is_cuda and w1_folded.dtype == w2.dtype == torch.bfloat16 and tuple(w2.shape) == (Cc, hid)
    w1_folded, w2 = w1_folded.contiguous(), w2.contiguous()
    out = torch.empty(2 * Cc * hid, dtype=torch.bfloat16, device=w1_folded.device)
    with torch.cuda.device(out.device):
        rc = L.lib.ppn_nat_mlp_pack_bf16(_p(w1_folded), _p(w2), _p(out), Cc, hid, ctypes.c_void_p(torch.cuda.current_stream(out.device).cuda_stream))
    L.check(rc, "ppn_nat_mlp_pack_bf16")
    return out


def nat_mlp_(s2d, wpk, hb, b2, hidden, stats_out=None, eps=1e-5):
    """s += gelu(LN(s) W1^T + b1) W2^T + b2 in place on the residual stream s2d [M, C] (bfloat16) in ONE kernel — the hidden
    activation never reaches HBM (ppn_nat_mlp_bf16, csrc/nat_mlp.hip).  wpk from nat_mlp_pack; hb [hidden, 2] float32 =
    (colsum of the folded w1 rows, b1 + W1 beta); b2 [C] float32; stats_out [C / 128, M, 2] receives the row partials of the new s."""
    M, Cc = s2d.shape
    assert s2d.is_cuda and s2d.dtype == torch.bfloat16 and s2d.is_contiguous() and wpk.dtype == torch.bfloat16 and wpk.numel() == 2 * Cc * hidden
    assert hb.dtype == torch.float32 and hb.is_contiguous() and tuple(hb.shape) == (hidden, 2) and b2.dtype == torch.float32 and b2.numel() == Cc
    assert stats_out is None or (stats_out.dtype == torch.float32 and stats_out.is_contiguous() and tuple(stats_out.shape) == (Cc // 128, M, 2))
    with torch.cuda.device(s2d.device):
        rc = L.lib.ppn_nat_mlp_bf16(_p(s2d), _p(wpk), _p(hb), _p(b2), _p(stats_out), M, Cc, hidden, float(eps),
                                    ctypes.c_void_p(torch.cuda.current_stream(s2d.device).cuda_stream))
    L.check(rc, "ppn_nat_mlp_bf16")
    return s2d


def nat_partials(C):
    """Row-statistics partials per row of a residual stream of width C (ppn_nat_gemm_partials, csrc/mfma_gemm.hip: one per 128
    columns up to C = 256, one per 256 columns above — what the accumulating GEMM's epilogue emits and the LayerNorm-folding GEMM
    reads)."""
    n = L.lib.ppn_nat_gemm_partials(C)
    if n < 0:
        raise ValueError(f"ppn_nat_gemm_partials({C})")
    return n


def row_stats(x2d):
    """[1, rows, 2] float32 = (sum, sum of squares) of every row of a bfloat16 [rows, C] tensor (ppn_row_stats_bf16)."""
    rows, Cc = x2d.shape
    assert x2d.is_cuda and x2d.dtype == torch.bfloat16 and x2d.is_contiguous()
    st = torch.empty(1, rows, 2, dtype=torch.float32, device=x2d.device)
    with torch.cuda.device(x2d.device):
        rc = L.lib.ppn_row_stats_bf16(_p(x2d), rows, Cc, _p(st), ctypes.c_void_p(torch.cuda.current_stream(x2d.device).cuda_stream))
    L.check(rc, "ppn_row_stats_bf16")
    return st


def gennet_conv_s2(x_nchw_cl, w_packed, bias32, negative_slope, transposed):
    """GenNet's 24-channel stride-2 conv (transposed=False) / transposed conv (True) + bias + LeakyReLU on MFMA
    (ppn_gennet_conv_s2_bf16).  x: channels_last bfloat16 [B,24,H,W]; w_packed / bias32 from gennet.pack_s2_weights."""
    if not x_nchw_cl.is_cuda or x_nchw_cl.dtype != torch.bfloat16:
        raise RuntimeError("ppnet_amd.fused.gennet_conv_s2: bfloat16 GPU tensors only")
    x = x_nchw_cl.permute(0, 2, 3, 1)
    if not x.is_contiguous():
        x = x.contiguous()
    B, H, W, C = x.shape
    assert C == 24
    Ho, Wo = (2 * H, 2 * W) if transposed else (H // 2, W // 2)
    y = torch.empty(B, Ho, Wo, C, dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        rc = L.lib.ppn_gennet_conv_s2_bf16(_p(x), _p(w_packed), _p(bias32), _p(y), B, H, W, float(negative_slope), 1 if transposed else 0,
                                           ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
    L.check(rc, "ppn_gennet_conv_s2_bf16")
    return y.permute(0, 3, 1, 2)


def _nat128_args(s, offset, ln):
    if not s.is_cuda or s.dtype != torch.bfloat16 or not s.is_contiguous() or s.shape[-1] != 128:
        raise RuntimeError("ppnet_amd.fused.nat128: contiguous bfloat16 GPU token rows of 128 channels only")
    assert offset is None or (offset.dtype == torch.float32 and offset.is_contiguous() and offset.device == s.device and offset.numel() == 128)
    return ln.weight.detach().to(torch.bfloat16), ln.bias.detach().to(torch.bfloat16)


def nat128_ln_qkv(s, offset, ln, qkv_linear):
    """qkv = qkv_linear(ln(s + offset)) for 128-channel token rows s [...,128] in ONE kernel (ppn_nat128_ln_qkv_bf16): the
    normalised tokens go from registers straight into the matrix pipe.  Returns [...,384] bfloat16."""
    lw, lb = _nat128_args(s, offset, ln)
    w = qkv_linear.weight.detach()
    assert w.shape == (384, 128) and w.dtype == torch.bfloat16 and w.is_contiguous()
    bias = qkv_linear.bias.detach() if qkv_linear.bias is not None else None
    out = torch.empty(*s.shape[:-1], 384, dtype=s.dtype, device=s.device)
    with torch.cuda.device(s.device):
        rc = L.lib.ppn_nat128_ln_qkv_bf16(_p(s), _p(offset) if offset is not None else None, _p(lw), _p(lb), _p(w),
                                          _p(bias) if bias is not None else None, _p(out), s.numel() // 128, float(ln.eps),
                                          ctypes.c_void_p(torch.cuda.current_stream(s.device).cuda_stream))
    L.check(rc, "ppn_nat128_ln_qkv_bf16")
    return out


def nat128_ln_mlp_(s, offset, ln, fc1, fc2, final_add=None):
    """s += fc2.weight @ gelu(fc1(ln(s + offset))) (+ final_add) in place, ONE kernel (ppn_nat128_ln_mlp_add_bf16): the hidden
    activations never reach HBM.  fc2's bias is NOT added (the folded layer carries it in the next offset); final_add [128]
    float32: a per-channel constant added to the result (the level's accumulated biases, on its last layer)."""
    lw, lb = _nat128_args(s, offset, ln)
    w1, w2 = fc1.weight.detach(), fc2.weight.detach()
    assert w1.shape == (256, 128) and w2.shape == (128, 256) and w1.dtype == w2.dtype == torch.bfloat16
    assert w1.is_contiguous() and w2.is_contiguous()
    with torch.cuda.device(s.device):
        if final_add is not None:
            assert final_add.dtype == torch.float32 and final_add.is_contiguous() and final_add.numel() == 128 and final_add.device == s.device
        rc = L.lib.ppn_nat128_ln_mlp_add_bf16(_p(s), _p(offset) if offset is not None else None, _p(lw), _p(lb), _p(w1), _p(fc1.bias.detach()),
                                              _p(w2), _p(final_add), s.numel() // 128, float(ln.eps),
                                              ctypes.c_void_p(torch.cuda.current_stream(s.device).cuda_stream))
    L.check(rc, "ppn_nat128_ln_mlp_add_bf16")
    return s


def nat128_proj_add_(s, a, proj):
    """s += a @ proj.weight^T in place for 128-channel token rows (ppn_nat128_proj_add_bf16; no bias: the folded layer carries it in
    the next offset)."""
    w = proj.weight.detach()
    assert s.is_cuda and s.dtype == a.dtype == w.dtype == torch.bfloat16 and s.is_contiguous() and a.is_contiguous() and w.is_contiguous()
    assert s.shape[-1] == 128 and a.shape == s.shape and w.shape == (128, 128)
    with torch.cuda.device(s.device):
        rc = L.lib.ppn_nat128_proj_add_bf16(_p(s), _p(a), _p(w), s.numel() // 128, ctypes.c_void_p(torch.cuda.current_stream(s.device).cuda_stream))
    L.check(rc, "ppn_nat128_proj_add_bf16")
    return s


def gennet_dec_final(x_nchw_cl, w_packed, bias32, negative_slope, w_final32, bias_final):
    """GenNet's last decoder stage + final convolution as one kernel (ppn_gennet_dec_final_bf16): x channels_last bfloat16
    [B,24,H,W] -> [B,1,2H,2W]; w_packed / bias32 from gennet.pack_s2_weights (transposed), w_final32 the final convolution's
    float32 weight [1,24,3,3], bias_final a Python float."""
    if not (x_nchw_cl.is_cuda and x_nchw_cl.dtype == torch.bfloat16):
        raise RuntimeError("ppnet_amd.fused.gennet_dec_final: bfloat16 GPU tensors only")
    x = x_nchw_cl.permute(0, 2, 3, 1)
    if not x.is_contiguous():
        x = x.contiguous()
    B, H, W, C = x.shape
    assert C == 24 and w_final32.dtype == torch.float32 and w_final32.is_contiguous() and w_final32.numel() == 24 * 9
    y = torch.empty(B, 1, 2 * H, 2 * W, dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        rc = L.lib.ppn_gennet_dec_final_bf16(_p(x), _p(w_packed), _p(bias32), float(negative_slope), _p(w_final32), float(bias_final), _p(y), B, H, W,
                                             ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
    L.check(rc, "ppn_gennet_dec_final_bf16")
    return y


def gennet_first_enc(x, w1, b1, wk2, b2, slope1, slope2):
    """GenNet's first convolution + first encoder stage as one kernel (ppn_gennet_first_enc_bf16): x [B,1,H,W] bfloat16 ->
    channels_last [B,24,H/2,W/2]; parameters from gennet.pack_first_enc_weights."""
    if not x.is_cuda or x.dtype != torch.bfloat16:
        raise RuntimeError("ppnet_amd.fused.gennet_first_enc: bfloat16 GPU tensors only")
    B, _, H, W = x.shape
    x = x.contiguous()
    assert w1.shape == (2, 16, 32) and wk2.shape == (2, 9, 16, 32) and w1.dtype == wk2.dtype == torch.bfloat16
    assert b1.dtype == b2.dtype == torch.float32 and b1.numel() == b2.numel() == 32
    y = torch.empty(B, H // 2, W // 2, 24, dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        rc = L.lib.ppn_gennet_first_enc_bf16(_p(x), _p(w1), _p(b1), _p(wk2), _p(b2), _p(y), B, H, W, float(slope1), float(slope2),
                                             ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
    L.check(rc, "ppn_gennet_first_enc_bf16")
    return y.permute(0, 3, 1, 2)


def gennet_trunk(x_nchw_cl, params32, n_blocks):
    """GenNet's ViT blocks as one kernel (ppn_gennet_trunk_bf16): channels_last bfloat16 [B,24,H,W] in and out; params32 from
    gennet.pack_trunk_params."""
    if not x_nchw_cl.is_cuda or x_nchw_cl.dtype != torch.bfloat16:
        raise RuntimeError("ppnet_amd.fused.gennet_trunk: bfloat16 GPU tensors only")
    x = x_nchw_cl.permute(0, 2, 3, 1)
    if not x.is_contiguous():
        x = x.contiguous()
    B, H, W, C = x.shape
    assert C == 24 and params32.dtype == torch.float32 and params32.is_contiguous() and params32.numel() == n_blocks * 7224
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        rc = L.lib.ppn_gennet_trunk_bf16(_p(x), _p(y), _p(params32), B, H * W, n_blocks,
                                         ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
    L.check(rc, "ppn_gennet_trunk_bf16")
    return y.permute(0, 3, 1, 2)


# ---------------------------------------------------------------- the heads' training loss: bilinear resize + cross-entropy
LOSS_CALLS = {"fwd": 0, "bwd": 0}        # launches of ppn_resize_ce_fwd / ppn_resize_ce_bwd (like vit.CALLS)
_LABEL_DT = {torch.uint8: 0, torch.int64: 1}
_INT32_END = 1 << 31
RESIZE_CE_THREADS = 256                  # work-items per workgroup of every kernel of csrc/resize_ce.hip
RESIZE_CE_FWD_PIXELS = 1024              # pixels per workgroup of its forward (the unit of ppn_resize_ce_workspace)


def resize_ce_bwd_lanes(h, w, H, W):
    """Lanes that share one dlogit element in ppn_resize_ce_bwd (csrc/resize_ce.hip: resize_ce_bwd_lanes, the same rule): by the
    pixels whose taps touch a low-resolution element, about (2 H/h)(2 W/w).  A workgroup writes RESIZE_CE_THREADS / lanes elements."""
    f = 2.0 * max(H / h, 1.0) * 2.0 * max(W / w, 1.0)
    return 1 if f <= 16.0 else (8 if f <= 128.0 else 64)


def resize_ce_ok(logit, labels):
    """Whether ppn_resize_ce_fwd / _bwd take these tensors: CUDA float32 / bfloat16 logits [B,C,h,w], CUDA uint8 / int64 labels
    [B,H,W] of the same batch on the same device, sizes inside the entry points' limits (include/ppnet_hip.h)."""
    if not (logit.is_cuda and labels.is_cuda and logit.device == labels.device and logit.dtype in _DT and labels.dtype in _LABEL_DT):
        return False
    if logit.dim() != 4 or labels.dim() != 3 or labels.shape[0] != logit.shape[0] or min(*logit.shape, *labels.shape) < 1:
        return False
    B, C, h, w = logit.shape
    H, W = labels.shape[-2:]
    per = RESIZE_CE_THREADS // resize_ce_bwd_lanes(h, w, H, W)              # the backward launch below 2^31 work-items
    return labels.numel() < _INT32_END and logit.numel() < _INT32_END and -(-logit.numel() // per) * RESIZE_CE_THREADS < _INT32_END - 1


def _resize_ce_fwd(logit, labels, ignore_index, want_lse):
    """One ppn_resize_ce_fwd on contiguous tensors: (loss 0-d float32, correct 0-d int64, lse [B,H,W] float32 or None)."""
    B, C, h, w = logit.shape
    H, W = labels.shape[-2:]
    dev = logit.device
    need = L.lib.ppn_resize_ce_workspace(B, H, W)
    if need < 0:
        raise L.PpnError(f"ppn_resize_ce_workspace: invalid sizes B={B} H={H} W={W}", -1)
    ws = torch.empty(need, dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    correct = torch.empty((), dtype=torch.int64, device=dev)
    lse = torch.empty(B, H, W, dtype=torch.float32, device=dev) if want_lse else None
    with torch.cuda.device(dev):
        rc = L.lib.ppn_resize_ce_fwd(_p(logit), _p(labels), _p(lse), _p(loss), _p(correct), _p(ws), need, B, C, h, w, H, W, ignore_index,
                                     _DT[logit.dtype], _LABEL_DT[labels.dtype], ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    L.check(rc, "ppn_resize_ce_fwd")
    LOSS_CALLS["fwd"] += 1
    return loss, correct, lse


def _resize_ce_bwd(logit, labels, lse, grad_out, ignore_index):
    """One ppn_resize_ce_bwd: dlogit in logit's layout and dtype; grad_out a float32 scalar on the device."""
    B, C, h, w = logit.shape
    H, W = labels.shape[-2:]
    dlogit = torch.empty_like(logit)
    with torch.cuda.device(logit.device):
        rc = L.lib.ppn_resize_ce_bwd(_p(logit), _p(labels), _p(lse), _p(grad_out), _p(dlogit), B, C, h, w, H, W, ignore_index, _DT[logit.dtype],
                                     _LABEL_DT[labels.dtype], ctypes.c_void_p(torch.cuda.current_stream(logit.device).cuda_stream))
    L.check(rc, "ppn_resize_ce_bwd")
    LOSS_CALLS["bwd"] += 1
    return dlogit


class _ResizeCEFunction(torch.autograd.Function):
    """Saves logit, labels and the per-pixel log-sum-exp, nothing else."""

    @staticmethod
    def forward(ctx, logit, labels, ignore_index):
        loss, correct, lse = _resize_ce_fwd(logit, labels, ignore_index, True)
        ctx.save_for_backward(logit, labels, lse)
        ctx.ignore_index = ignore_index
        ctx.mark_non_differentiable(correct)
        return loss, correct

    @staticmethod
    def backward(ctx, grad_loss, _grad_correct):
        logit, labels, lse = ctx.saved_tensors
        g = grad_loss.to(dtype=torch.float32, device=logit.device).contiguous()          # stays on the device: no synchronisation
        return _resize_ce_bwd(logit, labels, lse, g, ctx.ignore_index), None, None


def resize_cross_entropy(logit, labels, ignore_index=255):
    """(loss, correct) of a head's low-resolution logits [B,C,h,w] (float32 / bfloat16) against labels [B,H,W] (uint8 / int64):
    the mean over ALL B*H*W pixels of the cross-entropy of the logits resized bilinearly (align_corners=False) to H x W — ignored
    pixels add 0 and count in the divisor — as a 0-d float32 tensor differentiable w.r.t. `logit`, and the number of pixels whose
    argmax equals the label as a 0-d int64 tensor.  The resized logits are never built (ppn_resize_ce_fwd / ppn_resize_ce_bwd); a
    label outside [0, C) counts as ignored.  Without autograd recording the per-pixel buffer and the backward are skipped."""
    if not (logit.is_cuda and labels.is_cuda):
        raise RuntimeError("ppnet_amd.fused: GPU tensors only (no CPU fallback)")
    if not resize_ce_ok(logit, labels):
        raise ValueError(f"resize_cross_entropy: logits {tuple(logit.shape)} {logit.dtype} / labels {tuple(labels.shape)} {labels.dtype} "
                         "are outside ppn_resize_ce_fwd's types and limits")
    logit, labels = logit.contiguous(), labels.contiguous()
    if torch.is_grad_enabled() and logit.requires_grad:
        return _ResizeCEFunction.apply(logit, labels, int(ignore_index))
    loss, correct, _ = _resize_ce_fwd(logit.detach(), labels, int(ignore_index), False)
    return loss, correct


# ---------------------------------------------------------------- the heads' evaluation: bilinear resize + argmax + area histograms
EVAL_CALLS = {"fwd": 0}                  # launches of ppn_seg_eval (like LOSS_CALLS)
SEG_EVAL_THREADS = 256                   # work-items per workgroup of csrc/seg_eval.hip
SEG_EVAL_PIXELS = 1024                   # pixels per tile: four consecutive ones per work-item
SEG_EVAL_MAX_GROUPS = 1024               # workgroups at most: beyond SEG_EVAL_MAX_GROUPS tiles a workgroup strides over several
SEG_EVAL_BALLOT_CLASSES = 8              # C up to here counts with wave ballots; above, with LDS integer atomics
SEG_EVAL_MAX_CLASSES = 256               # pred is uint8 and the LDS histogram is fixed


def seg_eval_ok(logit, labels):
    """Whether ppn_seg_eval takes these tensors: CUDA float32 / bfloat16 logits [B,C,h,w] with C <= 256, CUDA uint8 / int64 labels
    [B,H,W] of the same batch on the same device, sizes inside the entry point's limits (include/ppnet_hip.h)."""
    if not (logit.is_cuda and labels.is_cuda and logit.device == labels.device and logit.dtype in _DT and labels.dtype in _LABEL_DT):
        return False
    if logit.dim() != 4 or labels.dim() != 3 or labels.shape[0] != logit.shape[0] or min(*logit.shape, *labels.shape) < 1:
        return False
    return logit.shape[1] <= SEG_EVAL_MAX_CLASSES and labels.numel() < _INT32_END and logit.numel() < _INT32_END


def seg_eval(logit, labels, ignore_index=255, want_pred=False):
    """(areas, pred) of a head's low-resolution logits [B,C,h,w] (float32 / bfloat16) against labels [B,H,W] (uint8 / int64): areas
    int64 [3,C] on the device — per class the valid pixels with pred == label (intersect), with pred == class, with label == class,
    where pred is the argmax (ties to the lowest class, a NaN never wins) of the logits resized bilinearly (align_corners=False) to
    H x W — and pred uint8 [B,H,W] (every pixel, ignored or not) or None.  The resized logits are never built (ppn_seg_eval); a label
    equal to ignore_index or outside [0, C) is ignored.  Nothing is read back: no host synchronisation."""
    if not (logit.is_cuda and labels.is_cuda):
        raise RuntimeError("ppnet_amd.fused: GPU tensors only (no CPU fallback)")
    if not seg_eval_ok(logit, labels):
        raise ValueError(f"seg_eval: logits {tuple(logit.shape)} {logit.dtype} / labels {tuple(labels.shape)} {labels.dtype} "
                         "are outside ppn_seg_eval's types and limits")
    logit, labels = logit.detach().contiguous(), labels.contiguous()
    B, C, h, w = logit.shape
    H, W = labels.shape[-2:]
    dev = logit.device
    areas = torch.empty(3, C, dtype=torch.int64, device=dev)
    pred = torch.empty(B, H, W, dtype=torch.uint8, device=dev) if want_pred else None
    with torch.cuda.device(dev):
        rc = L.lib.ppn_seg_eval(_p(logit), _p(labels), _p(pred), _p(areas), B, C, h, w, H, W, int(ignore_index), _DT[logit.dtype],
                                _LABEL_DT[labels.dtype], ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    L.check(rc, "ppn_seg_eval")
    EVAL_CALLS["fwd"] += 1
    return areas, pred


# ---------------------------------------------------------------- test-time augmentation: resizes + softmax + un-flip + mean + argmax
TTA_CALLS = {"fwd": 0}                   # launches of ppn_seg_tta (like EVAL_CALLS)
SEG_TTA_MAX_AUGS = 16                    # augmentations of one launch (include/ppnet_hip.h: PPN_SEG_TTA_MAX_AUGS)
SEG_TTA_REG_CLASSES = 8                  # C up to here sums in registers; above, prob is the accumulator (PPN_SEG_TTA_REG_CLASSES)
SEG_TTA_LDS_CLASSES = 64                 # C up to here the accumulating kernel keeps a pixel's logits in LDS; above, it interpolates thrice
SEG_TTA_THREADS = 256                    # work-items per workgroup of csrc/seg_tta.hip
SEG_TTA_PIXELS = 1024                    # pixels per tile: four consecutive ones per work-item
SEG_TTA_MAX_CLASSES = 256                # pred is uint8
_TTA_FLIP = {None: 0, "horizontal": 1, "vertical": 2}


def seg_tta_ok(logits, mids, flips, out_hw):
    """Whether ppn_seg_tta takes these: 1 to 16 CUDA float32 / bfloat16 logits [B,C,h_a,w_a] of one dtype, device, B and C <= 256, as
    many (hm, wm) >= 1 and flips of None / 'horizontal' / 'vertical', sizes inside the entry point's limits (include/ppnet_hip.h)."""
    if not 1 <= len(logits) <= SEG_TTA_MAX_AUGS or len(mids) != len(logits) or len(flips) != len(logits):
        return False
    x0 = logits[0]
    if not (x0.is_cuda and x0.dtype in _DT and x0.dim() == 4):
        return False
    for x, mid, fl in zip(logits, mids, flips):
        if not (x.is_cuda and x.device == x0.device and x.dtype == x0.dtype and x.dim() == 4 and x.shape[:2] == x0.shape[:2]):
            return False
        if min(x.shape) < 1 or x.numel() >= _INT32_END or len(mid) != 2 or min(mid) < 1 or max(mid) >= _INT32_END or fl not in _TTA_FLIP:
            return False
    B, C = x0.shape[:2]
    return len(out_hw) == 2 and min(out_hw) >= 1 and C <= SEG_TTA_MAX_CLASSES and B * C * out_hw[0] * out_hw[1] < _INT32_END


def seg_tta(logits, mids, flips, out_hw, want_prob=False):
    """(pred, prob) of a test-time augmentation's merge (mmseg's aug_test): per augmentation a the head's low-resolution logits
    logits[a] [B,C,h_a,w_a] (float32 / bfloat16) resized bilinearly (align_corners=False) to mids[a] = (hm, wm), the augmentation's
    image size, and from there to out_hw = (H, W); softmax; flipped back where flips[a] is 'horizontal' / 'vertical' (None: not);
    the mean over the augmentations; pred uint8 [B,H,W] its argmax (ties to the lowest class, a NaN never wins) and prob float32
    [B,C,H,W] the mean itself, or None (want_prob False and C <= 8: above, the kernel accumulates in prob and it is returned).  One
    ppn_seg_tta launch, float32 throughout, no full-resolution logits; nothing is read back: no host synchronisation."""
    if not all(x.is_cuda for x in logits):
        raise RuntimeError("ppnet_amd.fused: GPU tensors only (no CPU fallback)")
    if not seg_tta_ok(logits, mids, flips, out_hw):
        raise ValueError(f"seg_tta: {len(logits)} logits {[tuple(x.shape) for x in logits]} {sorted({str(x.dtype) for x in logits})} / "
                         f"sizes {list(mids)} -> {tuple(out_hw)} / flips {list(flips)} are outside ppn_seg_tta's types and limits")
    logits = [x.detach().contiguous() for x in logits]
    B, C = logits[0].shape[:2]
    H, W = int(out_hw[0]), int(out_hw[1])
    dev = logits[0].device
    augs = (L.TtaAug * len(logits))()
    for g, x, mid, fl in zip(augs, logits, mids, flips):
        g.logit, g.h, g.w, g.hm, g.wm, g.flip = x.data_ptr(), x.shape[2], x.shape[3], int(mid[0]), int(mid[1]), _TTA_FLIP[fl]
    pred = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
    prob = torch.empty(B, C, H, W, dtype=torch.float32, device=dev) if want_prob or C > SEG_TTA_REG_CLASSES else None
    with torch.cuda.device(dev):
        rc = L.lib.ppn_seg_tta(augs, len(logits), _p(pred), _p(prob), B, C, H, W, _DT[logits[0].dtype],
                               ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    L.check(rc, "ppn_seg_tta")
    TTA_CALLS["fwd"] += 1
    return pred, prob


# ---------------------------------------------------------------- the heads' training loss with a pixel sampler and class weights
OHEM_CALLS = {"fwd": 0, "bwd": 0}        # launches of ppn_ohem_ce_fwd / ppn_ohem_ce_bwd (like LOSS_CALLS, which they leave alone)
OHEM_THREADS = 256                       # work-items per workgroup of every kernel of csrc/ohem_ce.hip
OHEM_PIXELS = 1024                       # pixels per tile
OHEM_MAX_GROUPS = 1024                   # workgroups at most: beyond OHEM_MAX_GROUPS tiles a workgroup strides over several
OHEM_DIGIT_BITS = (11, 11, 10)           # the radix select's three digits of the 32-bit score key
OHEM_MODE_NONE, OHEM_MODE_THRESH, OHEM_MODE_TOPK = 0, 1, 2


def ohem_ce_ok(logit, labels):
    """Whether ppn_ohem_ce_fwd / _bwd take these tensors: ppn_resize_ce_fwd's types and limits (the backward launches the same grid)."""
    return resize_ce_ok(logit, labels)


def _ohem_mode(thresh, min_kept):
    """(mode, thresh, min_kept) of the entry points: no sampler without min_kept, else the threshold or the top-k form."""
    if min_kept is None:
        if thresh is not None:
            raise ValueError("ohem_cross_entropy: thresh without min_kept (a sampler has both; min_kept=None means no sampler)")
        return OHEM_MODE_NONE, 1.0, 1
    return (OHEM_MODE_TOPK, 1.0, int(min_kept)) if thresh is None else (OHEM_MODE_THRESH, float(thresh), int(min_kept))


def _ohem_ce_fwd(logit, labels, cw, ignore_index, mode, thresh, min_kept, want_mask):
    """One ppn_ohem_ce_fwd on contiguous tensors: (loss 0-d float32, counts int64 [3], threshold 0-d float32, lse, score [B,H,W]
    float32, mask uint8 [B,H,W] or None), all on the device."""
    B, C, h, w = logit.shape
    H, W = labels.shape[-2:]
    dev = logit.device
    need = L.lib.ppn_ohem_ce_workspace(B, H, W)
    if need < 0:
        raise L.PpnError(f"ppn_ohem_ce_workspace: invalid sizes B={B} H={H} W={W}", -1)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    threshold = torch.empty((), dtype=torch.float32, device=dev)
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    lse = torch.empty(B, H, W, dtype=torch.float32, device=dev)
    score = torch.empty(B, H, W, dtype=torch.float32, device=dev)
    mask = torch.empty(B, H, W, dtype=torch.uint8, device=dev) if want_mask else None
    with torch.cuda.device(dev):
        rc = L.lib.ppn_ohem_ce_fwd(_p(logit), _p(labels), _p(cw), _p(lse), _p(score), _p(loss), _p(counts), _p(threshold), _p(mask), _p(ws), need,
                                   B, C, h, w, H, W, ignore_index, mode, thresh, min_kept, _DT[logit.dtype], _LABEL_DT[labels.dtype],
                                   ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    L.check(rc, "ppn_ohem_ce_fwd")
    OHEM_CALLS["fwd"] += 1
    return loss, counts, threshold, lse, score, mask


def _ohem_ce_bwd(logit, labels, cw, lse, score, threshold, grad_out, ignore_index, mode):
    """One ppn_ohem_ce_bwd: dlogit in logit's layout and dtype; threshold and grad_out float32 scalars on the device."""
    B, C, h, w = logit.shape
    H, W = labels.shape[-2:]
    dlogit = torch.empty_like(logit)
    with torch.cuda.device(logit.device):
        rc = L.lib.ppn_ohem_ce_bwd(_p(logit), _p(labels), _p(cw), _p(lse), _p(score), _p(threshold), _p(grad_out), _p(dlogit), B, C, h, w, H, W,
                                   ignore_index, mode, _DT[logit.dtype], _LABEL_DT[labels.dtype],
                                   ctypes.c_void_p(torch.cuda.current_stream(logit.device).cuda_stream))
    L.check(rc, "ppn_ohem_ce_bwd")
    OHEM_CALLS["bwd"] += 1
    return dlogit


class _OhemCEFunction(torch.autograd.Function):
    """Saves logit, labels, the class weights, the per-pixel log-sum-exp and score, and the device threshold; no weight tensor."""

    @staticmethod
    def forward(ctx, logit, labels, cw, ignore_index, mode, thresh, min_kept, want_mask):
        loss, counts, threshold, lse, score, mask = _ohem_ce_fwd(logit, labels, cw, ignore_index, mode, thresh, min_kept, want_mask)
        ctx.save_for_backward(logit, labels, lse, score, threshold, *(() if cw is None else (cw,)))
        ctx.ignore_index, ctx.mode = ignore_index, mode
        out = (loss, counts) if mask is None else (loss, counts, mask)
        ctx.mark_non_differentiable(*out[1:])
        return out

    @staticmethod
    def backward(ctx, grad_loss, *_unused):
        logit, labels, lse, score, threshold, *cw = ctx.saved_tensors
        g = grad_loss.to(dtype=torch.float32, device=logit.device).contiguous()          # stays on the device: no synchronisation
        d = _ohem_ce_bwd(logit, labels, cw[0] if cw else None, lse, score, threshold, g, ctx.ignore_index, ctx.mode)
        return d, None, None, None, None, None, None, None


def ohem_cross_entropy(logit, labels, ignore_index=255, class_weight=None, thresh=None, min_kept=None, want_mask=False):
    """(loss, correct, n_kept[, mask]) of a head's low-resolution logits [B,C,h,w] (float32 / bfloat16) against labels [B,H,W] (uint8 /
    int64) under mmseg's OHEMPixelSampler(thresh, min_kept) and CrossEntropyLoss(class_weight): loss = the sum over the SELECTED
    pixels of class_weight[label] * cross-entropy of the logits resized bilinearly (align_corners=False) to H x W, divided by ALL B*H*W
    pixels — a 0-d float32 tensor differentiable w.r.t. `logit`; correct = valid pixels whose argmax equals the label (sampling does not
    change it) and n_kept = selected pixels, 0-d int64; mask uint8 [B,H,W] (1 selected) with want_mask.  min_kept=None: no sampler,
    every valid pixel (class weights only); thresh given: pixels whose label probability is below max(thresh, the
    min(min_kept * B, n_valid - 1)-th smallest one); thresh=None: the min_kept * B largest losses, ties at the cut all kept.  class_weight:
    a float32 tensor [C] on the logits' device, or None.  Neither the resized logits nor a weight tensor is built and nothing is read
    back (ppn_ohem_ce_fwd / ppn_ohem_ce_bwd); a label outside [0, C) counts as ignored."""
    if not (logit.is_cuda and labels.is_cuda):
        raise RuntimeError("ppnet_amd.fused: GPU tensors only (no CPU fallback)")
    if not ohem_ce_ok(logit, labels):
        raise ValueError(f"ohem_cross_entropy: logits {tuple(logit.shape)} {logit.dtype} / labels {tuple(labels.shape)} {labels.dtype} "
                         "are outside ppn_ohem_ce_fwd's types and limits")
    mode, thresh, min_kept = _ohem_mode(thresh, min_kept)
    if min_kept < 1 or (mode == OHEM_MODE_THRESH and not 0.0 < thresh <= 1.0):
        raise ValueError(f"ohem_cross_entropy: min_kept {min_kept} / thresh {thresh} outside min_kept >= 1, 0 < thresh <= 1")
    cw = None
    if class_weight is not None:
        cw = torch.as_tensor(class_weight, dtype=torch.float32, device=logit.device).contiguous()
        if cw.shape != (logit.shape[1],):
            raise ValueError(f"ohem_cross_entropy: class_weight {tuple(cw.shape)} for {logit.shape[1]} classes")
    logit, labels = logit.contiguous(), labels.contiguous()
    if torch.is_grad_enabled() and logit.requires_grad:
        loss, counts, *mask = _OhemCEFunction.apply(logit, labels, cw, int(ignore_index), mode, thresh, min_kept, bool(want_mask))
    else:
        loss, counts, _, _, _, m = _ohem_ce_fwd(logit.detach(), labels, cw, int(ignore_index), mode, thresh, min_kept, bool(want_mask))
        mask = [] if m is None else [m]
    return (loss, counts[0], counts[2], *mask)


# ---------------------------------------------------------------- the heads' training loss: bilinear resize + Dice (mmseg's DiceLoss)
DICE_CALLS = {"fwd": 0, "bwd": 0}        # launches of ppn_resize_dice_fwd / ppn_resize_dice_bwd (like LOSS_CALLS, which they leave alone)
RESIZE_DICE_THREADS = 256                # work-items per workgroup of every kernel of csrc/resize_dice.hip
RESIZE_DICE_PIXELS = 1024                # pixels per tile; a tile lies inside ONE image (the unit of ppn_resize_dice_workspace)
RESIZE_DICE_MAX_CLASSES = 256            # the LDS partial sums and coefficients are fixed arrays


def resize_dice_workspace_bytes(B, C, H, W):
    """include/ppnet_hip.h's formula for ppn_resize_dice_workspace: the forward's per-tile partials or the backward's per-pixel buffer
    and coefficients, whichever is larger, in bytes."""
    tiles = B * -(-(H * W) // RESIZE_DICE_PIXELS)
    return 4 * max(tiles * (3 * C + 1), B * H * W + 4 * B * C)


def resize_dice_ok(logit, labels):
    """Whether ppn_resize_dice_fwd / _bwd take these tensors: ppn_resize_ce_fwd's types and limits (the gather launches the same
    grid), C <= RESIZE_DICE_MAX_CLASSES and a per-pixel launch (a workgroup per tile of an image) below 2^31 work-items."""
    if not resize_ce_ok(logit, labels) or logit.shape[1] > RESIZE_DICE_MAX_CLASSES:
        return False
    B, (H, W) = labels.shape[0], labels.shape[-2:]
    return B * -(-(H * W) // RESIZE_DICE_PIXELS) * RESIZE_DICE_THREADS < _INT32_END - 1


def _dice_workspace(B, C, H, W, dev):
    need = L.lib.ppn_resize_dice_workspace(B, C, H, W)
    if need < 0:
        raise L.PpnError(f"ppn_resize_dice_workspace: invalid sizes B={B} C={C} H={H} W={W}", -1)
    return torch.empty(need, dtype=torch.uint8, device=dev)


def _resize_dice_fwd(logit, labels, cw, ignore_index, smooth, want_lse):
    """One ppn_resize_dice_fwd on contiguous tensors: (loss 0-d float32, correct 0-d int64, sums float64 [B,C,3], lse [B,H,W] float32
    or None), all on the device."""
    B, C, h, w = logit.shape
    H, W = labels.shape[-2:]
    dev = logit.device
    ws = _dice_workspace(B, C, H, W, dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    correct = torch.empty((), dtype=torch.int64, device=dev)
    sums = torch.empty(B, C, 3, dtype=torch.float64, device=dev)
    lse = torch.empty(B, H, W, dtype=torch.float32, device=dev) if want_lse else None
    with torch.cuda.device(dev):
        rc = L.lib.ppn_resize_dice_fwd(_p(logit), _p(labels), _p(cw), _p(ws), _p(lse), _p(sums), _p(loss), _p(correct), B, C, h, w, H, W,
                                       ignore_index, smooth, _DT[logit.dtype], _LABEL_DT[labels.dtype],
                                       ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    L.check(rc, "ppn_resize_dice_fwd")
    DICE_CALLS["fwd"] += 1
    return loss, correct, sums, lse


def _resize_dice_bwd(logit, labels, cw, lse, sums, grad_out, ignore_index, smooth):
    """One ppn_resize_dice_bwd: dlogit in logit's layout and dtype; grad_out a float32 scalar on the device."""
    B, C, h, w = logit.shape
    H, W = labels.shape[-2:]
    ws = _dice_workspace(B, C, H, W, logit.device)
    dlogit = torch.empty_like(logit)
    with torch.cuda.device(logit.device):
        rc = L.lib.ppn_resize_dice_bwd(_p(logit), _p(labels), _p(lse), _p(sums), _p(cw), _p(grad_out), _p(ws), _p(dlogit), B, C, h, w, H, W,
                                       ignore_index, smooth, _DT[logit.dtype], _LABEL_DT[labels.dtype],
                                       ctypes.c_void_p(torch.cuda.current_stream(logit.device).cuda_stream))
    L.check(rc, "ppn_resize_dice_bwd")
    DICE_CALLS["bwd"] += 1
    return dlogit


class _ResizeDiceFunction(torch.autograd.Function):
    """Saves logit, labels, the per-pixel log-sum-exp, the [B,C,3] sums and the class weights, nothing else."""

    @staticmethod
    def forward(ctx, logit, labels, cw, ignore_index, smooth):
        loss, correct, sums, lse = _resize_dice_fwd(logit, labels, cw, ignore_index, smooth, True)
        ctx.save_for_backward(logit, labels, lse, sums, *(() if cw is None else (cw,)))
        ctx.ignore_index, ctx.smooth = ignore_index, smooth
        ctx.mark_non_differentiable(correct)
        return loss, correct

    @staticmethod
    def backward(ctx, grad_loss, _grad_correct):
        logit, labels, lse, sums, *cw = ctx.saved_tensors
        g = grad_loss.to(dtype=torch.float32, device=logit.device).contiguous()          # stays on the device: no synchronisation
        return _resize_dice_bwd(logit, labels, cw[0] if cw else None, lse, sums, g, ctx.ignore_index, ctx.smooth), None, None, None, None


def resize_dice(logit, labels, ignore_index=255, smooth=1.0, class_weight=None):
    """(loss, correct) of a head's low-resolution logits [B,C,h,w] (float32 / bfloat16) against labels [B,H,W] (uint8 / int64): mmseg's
    DiceLoss(smooth, exponent=2, class_weight, loss_weight=1, ignore_index) of the logits resized bilinearly (align_corners=False) to
    H x W — 1 / (C B) * the sum over images and classes i != ignore_index of class_weight_i (1 - (2 I + smooth) / (P2 + T + smooth)),
    the sums of heads.dice_loss — as a 0-d float32 tensor differentiable w.r.t. `logit`, and the number of valid pixels whose argmax
    equals the label as a 0-d int64 tensor (resize_cross_entropy's count).  Neither the resized logits, their softmax nor a one-hot
    tensor is built and nothing is read back (ppn_resize_dice_fwd / ppn_resize_dice_bwd); a label outside [0, C) counts as ignored in
    the numerator and, clamped, in the denominator.  class_weight: a float32 tensor [C] on the logits' device, or C floats, or None.
    Without autograd recording the per-pixel buffer and the backward are skipped."""
    if not (logit.is_cuda and labels.is_cuda):
        raise RuntimeError("ppnet_amd.fused: GPU tensors only (no CPU fallback)")
    if not resize_dice_ok(logit, labels):
        raise ValueError(f"resize_dice: logits {tuple(logit.shape)} {logit.dtype} / labels {tuple(labels.shape)} {labels.dtype} "
                         "are outside ppn_resize_dice_fwd's types and limits")
    smooth = float(smooth)
    if not 0.0 <= smooth < float("inf"):
        raise ValueError(f"resize_dice: smooth {smooth} is negative or not finite")
    cw = None
    if class_weight is not None:
        cw = torch.as_tensor(class_weight, dtype=torch.float32, device=logit.device).contiguous()
        if cw.shape != (logit.shape[1],):
            raise ValueError(f"resize_dice: class_weight {tuple(cw.shape)} for {logit.shape[1]} classes")
    logit, labels = logit.contiguous(), labels.contiguous()
    if torch.is_grad_enabled() and logit.requires_grad:
        return _ResizeDiceFunction.apply(logit, labels, cw, int(ignore_index), smooth)
    loss, correct, _, _ = _resize_dice_fwd(logit.detach(), labels, cw, int(ignore_index), smooth, False)
    return loss, correct


# ---------------------------------------------------------------------------------------------------------------- DiNAT_s patch merge
MERGE_CALLS = {"fwd": 0, "bwd": 0}       # launches of ppn_patch_merge_ln_fwd / ppn_patch_merge_ln_bwd (like NORM_CALLS)
MERGE_WIDTHS = frozenset(8 << i for i in range(7))                         # csrc/patch_merge_ln.hip: C / 8 lanes per row, a power of two up to 64
MERGE_MAX_BLOCKS = 1024                  # workgroups at most (ppn_patch_merge_ln_max_blocks): beyond that many tiles a workgroup strides


def patch_merge_rows(C):
    """Rows of one workgroup tile of csrc/patch_merge_ln.hip (ppn_patch_merge_ln_rows): 256 / (C / 8); 0 for a width it does not take."""
    return 256 // (C // 8) if C in MERGE_WIDTHS else 0


def patch_merge_workspace_bytes(B, H, W, C):
    """ppn_patch_merge_ln_bwd_workspace's formula (include/ppnet_hip.h): one [2][4C] float32 partial per workgroup."""
    rows = B * -(-H // 2) * -(-W // 2)
    return 4 * min(-(-rows // patch_merge_rows(C)), MERGE_MAX_BLOCKS) * 2 * 4 * C


def library_merge():
    """PPNET_LIBRARY_MERGE=1 (read at call time, like PPNET_LIBRARY_NORM): patch_merge_ln takes the torch composition (pad, four strided
    slices, cat, F.layer_norm and the framework's backwards) instead of the HIP pair, with and without autograd."""
    return bool(os.environ.get("PPNET_LIBRARY_MERGE"))


def patch_merge_ln_ok(x, ln):
    """Whether patch_merge_ln runs x [B,H,W,C] on the HIP pair: a CUDA tensor of float32 / bfloat16, a width of MERGE_WIDTHS, an affine
    LayerNorm over 4C whose parameters live on x's device in float32 or bfloat16 (a bfloat16 autocast step keeps float32 parameters:
    patch_merge_ln runs the wider dtype), fewer than 2^31 elements, and the knob off.  Everything else is the torch composition."""
    if library_merge() or not x.is_cuda or x.dtype not in _DT or x.dim() != 4 or x.numel() == 0 or x.shape[-1] not in MERGE_WIDTHS:
        return False
    B, H, W, C = x.shape
    if tuple(ln.normalized_shape) != (4 * C,) or ln.weight is None or ln.bias is None:
        return False
    if any(t.dtype not in _DT or t.device != x.device for t in (ln.weight, ln.bias)):
        return False
    return B * -(-H // 2) * -(-W // 2) * 4 * C < 2 ** 31 - 1


def patch_merge_gather(x):
    """The reference's gather (SegNet/dinats.py:88-99): zero-pad to even sizes, x0 (even row, even col) | x1 (odd row, even col) |
    x2 (even row, odd col) | x3 (odd row, odd col) -> [B,ceil(H/2),ceil(W/2),4C]."""
    H, W = x.shape[1], x.shape[2]
    if H % 2 or W % 2:
        x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
    return torch.cat([x[:, 0::2, 0::2, :], x[:, 1::2, 0::2, :], x[:, 0::2, 1::2, :], x[:, 1::2, 1::2, :]], -1)


def _patch_merge_ln_torch(x, ln):
    return F.layer_norm(patch_merge_gather(x), ln.normalized_shape, ln.weight, ln.bias, ln.eps)


def _pm_fwd(x, w, b, eps, want_stats):
    """ppn_patch_merge_ln_fwd on contiguous tensors of one dtype: (y [B,Ho,Wo,4C], stats [rows,2] float32 or None)."""
    B, H, W, C = x.shape
    Ho, Wo = -(-H // 2), -(-W // 2)
    y = torch.empty(B, Ho, Wo, 4 * C, dtype=x.dtype, device=x.device)
    stats = torch.empty(B * Ho * Wo, 2, dtype=torch.float32, device=x.device) if want_stats else None
    with torch.cuda.device(x.device):
        rc = L.lib.ppn_patch_merge_ln_fwd(_p(x), _p(w), _p(b), _p(y), _p(stats), B, H, W, C, float(eps), _DT[x.dtype], _stream(x))
    L.check(rc, "ppn_patch_merge_ln_fwd")
    MERGE_CALLS["fwd"] += 1
    return y, stats


def _pm_bwd(gy, x, stats, w, want_params):
    """ppn_patch_merge_ln_bwd on contiguous tensors: (dx, dgamma, dbeta), the last two None where not wanted."""
    B, H, W, C = x.shape
    dx = torch.empty_like(x)
    dgamma, dbeta = (torch.empty_like(w), torch.empty_like(w)) if want_params else (None, None)
    need = L.lib.ppn_patch_merge_ln_bwd_workspace(B, H, W, C)
    ws = torch.empty(max(need, 16) // 4, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = L.lib.ppn_patch_merge_ln_bwd(_p(gy), _p(x), _p(stats), _p(w), _p(ws), _p(dx), _p(dgamma), _p(dbeta), B, H, W, C, _DT[x.dtype],
                                          _stream(x))
    L.check(rc, "ppn_patch_merge_ln_bwd")
    MERGE_CALLS["bwd"] += 1
    return dx, dgamma, dbeta


class _PatchMergeLNFunction(torch.autograd.Function):
    """y = LayerNorm_{4C}(2 x 2 gather of x) on ppn_patch_merge_ln_fwd / ppn_patch_merge_ln_bwd; x, gamma and beta of one dtype.  Saved: x,
    the row statistics [rows,2] and gamma — no [.., 4C] tensor."""

    @staticmethod
    def forward(ctx, x, w, b, eps):
        x, w, b = x.contiguous(), w.detach().contiguous(), b.detach().contiguous()
        y, stats = _pm_fwd(x, w, b, eps, True)
        ctx.save_for_backward(x, stats, w)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, stats, w = ctx.saved_tensors
        need_x, need_w, need_b, _ = ctx.needs_input_grad
        dx, dgamma, dbeta = _pm_bwd(gy.to(x.dtype).contiguous(), x, stats, w, need_w or need_b)
        return dx if need_x else None, dgamma if need_w else None, dbeta if need_b else None, None


def patch_merge_ln(x, ln):
    """ln(2 x 2 gather of x) for x [B,H,W,C] and a LayerNorm over 4C -> [B,ceil(H/2),ceil(W/2),4C]: DiNAT_s's PatchMerging in front of its
    reduction (SegNet/dinats.py:88-102).  On the GPU one kernel reads x once and writes y once (ppn_patch_merge_ln_fwd with stats = NULL);
    while autograd records, the training pair (_PatchMergeLNFunction).  No size gate: the pair replaces about six framework ops each way
    (tools/patch_merge_timing.py).  Tokens and parameters of two dtypes — bfloat16 tokens in front of float32
    parameters, the later levels of a bfloat16 autocast step — run in the wider one and y has it, as autocast runs a LayerNorm in
    float32.  CPU tensors, other dtypes, widths outside MERGE_WIDTHS and PPNET_LIBRARY_MERGE=1 take the torch composition."""
    if not patch_merge_ln_ok(x, ln):
        return _patch_merge_ln_torch(x, ln)
    dt = torch.promote_types(x.dtype, torch.promote_types(ln.weight.dtype, ln.bias.dtype))
    if recording(x, ln.weight, ln.bias):
        return _PatchMergeLNFunction.apply(x.to(dt), ln.weight.to(dt), ln.bias.to(dt), ln.eps)
    return _pm_fwd(x.to(dt).contiguous(), ln.weight.detach().to(dt).contiguous(), ln.bias.detach().to(dt).contiguous(), ln.eps, False)[0]


# ---------------------------------------------------------------------------------------------------------------- GenNet stem training
STEM_CALLS = {"fwd": 0, "bwd": 0}        # launches of ppn_gennet_stem_train_fwd / ppn_gennet_stem_train_bwd (like MERGE_CALLS)
STEM_CHANNELS = frozenset({8, 16, 24, 32})                                  # csrc/gennet_stem_train.hip: the set ppn_conv3x3_c1_nhwc takes
STEM_THREADS = 256                       # work-items per workgroup of every kernel of csrc/gennet_stem_train.hip
STEM_LINE = 4                            # consecutive pixels per work-item: the unit of its vector loads and stores
STEM_TILE = 1024                         # pixels per workgroup tile (ppn_gennet_stem_train_tile)
STEM_MAX_BLOCKS = 512                    # workgroups at most in x of the summing kernels (ppn_gennet_stem_train_max_blocks)
STEM_MOMENTS = 54                        # float64 moments of the 3 x 3 patches: S1 (9), the lower triangle of S2 (45)
STEM_SUMS = 11                           # float32 sums per channel of the backward: g, g xhat, g p_0 .. g p_8


def stem_train_workspace_bytes(B, H, W, C):
    """ppn_gennet_stem_train_workspace's formula (include/ppnet_hip.h): per workgroup one [54] float64 partial forward, one [C][11] float32
    partial backward, in the same buffer."""
    return max(STEM_MOMENTS * 8, C * STEM_SUMS * 4) * min(-(-(B * H * W) // STEM_TILE), STEM_MAX_BLOCKS)


def library_stem():
    """PPNET_LIBRARY_STEM=1 (read at call time, like PPNET_LIBRARY_MERGE): stem_bn_act takes Conv2d + BatchNorm2d + LeakyReLU and the
    framework's backwards instead of the HIP pair."""
    return bool(os.environ.get("PPNET_LIBRARY_STEM"))


def stem_train_ok(x, conv, bn):
    """Whether stem_bn_act runs conv -> bn -> LeakyReLU on the HIP pair: x a contiguous CUDA float32 [B,1,H,W] that does not require grad
    (the kernels have no input gradient) with B H W >= 2 (one value per channel is torch's own ValueError) and fewer than 2^31 outputs;
    conv exactly a Conv2d(1, C, 3, 1, 1), dilation 1, groups 1, zero padding, C in STEM_CHANNELS; bn exactly a BatchNorm2d (a SyncBatchNorm
    reduces over ranks) in training mode, affine, tracking running statistics with a float momentum; float32 parameters and buffers on
    x's device, autograd recording a parameter; no autocast or bfloat16 autocast; and the knob off.  Everything else keeps the library."""
    if library_stem() or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 1 or x.requires_grad:
        return False
    if type(conv) is not torch.nn.Conv2d or type(bn) is not torch.nn.BatchNorm2d:
        return False
    if (conv.in_channels != 1 or conv.out_channels not in STEM_CHANNELS or conv.kernel_size != (3, 3) or conv.stride != (1, 1)
            or conv.padding != (1, 1) or conv.dilation != (1, 1) or conv.groups != 1 or conv.padding_mode != "zeros"):
        return False
    if not (bn.training and bn.affine and bn.track_running_stats and isinstance(bn.momentum, float) and bn.num_features == conv.out_channels):
        return False
    B, _, H, W = x.shape
    if B * H * W < 2 or B * H * W * conv.out_channels >= 2 ** 31 or not x.is_contiguous():
        return False
    tensors = (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)
    if any(t is not None and (t.dtype != torch.float32 or t.device != x.device) for t in tensors) or bn.running_mean is None:
        return False
    if torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") != torch.bfloat16:
        return False
    return recording(conv.weight, conv.bias, bn.weight, bn.bias)


def _stem_workspace(B, H, W, C, dev):
    need = L.lib.ppn_gennet_stem_train_workspace(B, H, W, C)
    if need < 0:
        raise L.PpnError(f"ppn_gennet_stem_train_workspace refuses B {B} H {H} W {W} C {C}", -1)
    return torch.empty(max(need, 16) // 4, dtype=torch.float32, device=dev)


def _stem_fwd(x, w, b, gamma, beta, eps, slope, dtype):
    """ppn_gennet_stem_train_fwd on contiguous float32 tensors (x [B,1,H,W] or [B,H,W], w [C,1,3,3] or [C,9], b None = no bias):
    (z [B,C,H,W] of dtype, stats [3,C] float32, moments [54] float64)."""
    B, H, W, C = x.shape[0], x.shape[-2], x.shape[-1], w.shape[0]
    z = torch.empty(B, C, H, W, dtype=dtype, device=x.device)
    stats = torch.empty(3, C, dtype=torch.float32, device=x.device)
    moments = torch.empty(STEM_MOMENTS, dtype=torch.float64, device=x.device)
    ws = _stem_workspace(B, H, W, C, x.device)
    with torch.cuda.device(x.device):
        rc = L.lib.ppn_gennet_stem_train_fwd(_p(x), _p(w), _p(b), _p(gamma), _p(beta), _p(z), _p(stats), _p(moments), _p(ws), B, H, W, C,
                                             float(eps), float(slope), _DT[dtype], _stream(x))
    L.check(rc, "ppn_gennet_stem_train_fwd")
    STEM_CALLS["fwd"] += 1
    return z, stats, moments


def _stem_bwd(dz, x, w, b, gamma, beta, stats, moments, slope):
    """ppn_gennet_stem_train_bwd on contiguous tensors: (dw shaped like w, dgamma [C], dbeta [C]), float32."""
    B, H, W, C = x.shape[0], x.shape[-2], x.shape[-1], w.shape[0]
    dw, dgamma, dbeta = torch.empty_like(w), torch.empty_like(gamma), torch.empty_like(beta)
    ws = _stem_workspace(B, H, W, C, x.device)
    with torch.cuda.device(x.device):
        rc = L.lib.ppn_gennet_stem_train_bwd(_p(dz), _p(x), _p(w), _p(b), _p(gamma), _p(beta), _p(stats), _p(moments), _p(ws), _p(dw), _p(dgamma),
                                             _p(dbeta), B, H, W, C, float(slope), _DT[dz.dtype], _stream(x))
    L.check(rc, "ppn_gennet_stem_train_bwd")
    STEM_CALLS["bwd"] += 1
    return dw, dgamma, dbeta


class _StemTrainFunction(torch.autograd.Function):
    """(z, stats) = LeakyReLU(BatchNorm_train(conv3x3(x))) on ppn_gennet_stem_train_fwd / ppn_gennet_stem_train_bwd.  Saved: x, the
    parameters, the statistics [3,C] and the moments [54] — nothing of z's size.  x gets no gradient; the convolution bias gets zeros
    (its gradient is the sum of a BatchNorm input gradient: exactly 0), not None — DistributedDataParallel waits for every parameter."""

    @staticmethod
    def forward(ctx, x, w, b, gamma, beta, eps, slope, dtype):
        w, gamma, beta = w.detach().contiguous(), gamma.detach().contiguous(), beta.detach().contiguous()
        b = b.detach().contiguous() if b is not None else None
        z, stats, moments = _stem_fwd(x, w, b, gamma, beta, eps, slope, dtype)
        ctx.save_for_backward(x, w, b, gamma, beta, stats, moments)
        ctx.slope = slope
        ctx.mark_non_differentiable(stats)
        return z, stats

    @staticmethod
    @once_differentiable
    def backward(ctx, dz, _dstats):
        x, w, b, gamma, beta, stats, moments = ctx.saved_tensors
        dw, dgamma, dbeta = _stem_bwd(dz.contiguous(), x, w, b, gamma, beta, stats, moments, ctx.slope)
        return None, dw, torch.zeros_like(b) if b is not None else None, dgamma, dbeta, None, None, None


def stem_bn_act(x, conv, bn, negative_slope):
    """leaky_relu(bn(conv(x))) for GenNet's stem.  Where stem_train_ok holds, the HIP pair: z is written once in the CUDA autocast dtype
    (float32 without autocast) and the backward is one pass over dz; bn's running statistics are updated as
    F.batch_norm does in training (momentum, the unbiased variance N / (N - 1)) and num_batches_tracked counts the call.  Otherwise the
    library composition, untouched."""
    if not stem_train_ok(x, conv, bn):
        return F.leaky_relu(bn(conv(x)), negative_slope)
    dtype = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else torch.float32
    z, stats = _StemTrainFunction.apply(x, conv.weight, conv.bias, bn.weight, bn.bias, bn.eps, float(negative_slope), dtype)
    with torch.no_grad():
        n, m = x.shape[0] * x.shape[2] * x.shape[3], bn.momentum
        bn.num_batches_tracked.add_(1)
        bn.running_mean.mul_(1.0 - m).add_(stats[0], alpha=m)
        bn.running_var.mul_(1.0 - m).add_(stats[1], alpha=m * n / (n - 1))
    return z


# ---------------------------------------------------------------------------------------------------------------- GenNet tail training
TAIL_CALLS = {"fwd": 0, "bwd": 0}        # launches of ppn_gennet_tail_train_fwd / ppn_gennet_tail_train_bwd (like STEM_CALLS)
TAIL_CHANNELS = frozenset({8, 16, 24, 32})                                  # csrc/gennet_tail_train.hip: the stem's set
TAIL_THREADS = 256                       # work-items per workgroup of every kernel of csrc/gennet_tail_train.hip
TAIL_LINE = 4                            # consecutive pixels per work-item: the unit of its vector loads and stores
TAIL_TILE = 1024                         # pixels per workgroup tile (ppn_gennet_tail_train_tile)
TAIL_MAX_BLOCKS = 512                    # workgroups at most in x of the summing kernels (ppn_gennet_tail_train_max_blocks)
TAIL_SUMS = 11                           # float32 sums per channel of the backward: g, g xhat, z d(. - tap) for 9 taps
TAIL_RECORD_MIN = 0                      # the smallest y.numel() that takes the kernels (no crossover was measured)


def tail_train_workspace_bytes(B, H, W, C):
    """ppn_gennet_tail_train_workspace's formula (include/ppnet_hip.h): per workgroup one [C][2] float64 partial forward, one [C][11] + 1
    float32 partial backward, in the same buffer."""
    return max(C * 2 * 8, (C * TAIL_SUMS + 1) * 4) * min(-(-(B * H * W) // TAIL_TILE), TAIL_MAX_BLOCKS)


def library_tail():
    """PPNET_LIBRARY_TAIL=1 (read at call time, like PPNET_LIBRARY_STEM): tail_bn_act_conv takes BatchNorm2d + LeakyReLU + Conv2d and the
    framework's backwards instead of the HIP pair."""
    return bool(os.environ.get("PPNET_LIBRARY_TAIL"))


def tail_train_ok(y, bn, conv):
    """Whether tail_bn_act_conv runs bn -> LeakyReLU -> conv on the HIP pair: y a contiguous CUDA [B,C,H,W], float32 or (under bfloat16
    autocast, where the library composition takes it too) bfloat16, with B H W >= 2 (one value per channel is torch's own ValueError),
    fewer than 2^31 elements and at least TAIL_RECORD_MIN; bn exactly a BatchNorm2d (a SyncBatchNorm reduces over ranks) in training mode,
    affine, tracking running statistics with a float momentum, C features, C in TAIL_CHANNELS; conv exactly a Conv2d(C, 1, 3, 1, 1),
    dilation 1, groups 1, zero padding; float32 parameters and buffers on y's device; autograd recording y or a parameter; no autocast or
    bfloat16 autocast; and the knob off.  Everything else keeps the library."""
    if library_tail() or not y.is_cuda or y.dtype not in (torch.float32, torch.bfloat16) or y.dim() != 4:
        return False
    if type(bn) is not torch.nn.BatchNorm2d or type(conv) is not torch.nn.Conv2d:
        return False
    B, C, H, W = y.shape
    if (conv.in_channels != C or conv.out_channels != 1 or C not in TAIL_CHANNELS or conv.kernel_size != (3, 3) or conv.stride != (1, 1)
            or conv.padding != (1, 1) or conv.dilation != (1, 1) or conv.groups != 1 or conv.padding_mode != "zeros"):
        return False
    if not (bn.training and bn.affine and bn.track_running_stats and isinstance(bn.momentum, float) and bn.num_features == C):
        return False
    if B * H * W < 2 or B * C * H * W >= 2 ** 31 or B * C * H * W < TAIL_RECORD_MIN or not y.is_contiguous():
        return False
    tensors = (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)
    if any(t is not None and (t.dtype != torch.float32 or t.device != y.device) for t in tensors) or bn.running_mean is None:
        return False
    autocast = torch.is_autocast_enabled("cuda")
    if autocast and torch.get_autocast_dtype("cuda") != torch.bfloat16:
        return False
    if y.dtype == torch.bfloat16 and not autocast:                           # the library's convolution refuses bfloat16 z x float32 weight
        return False
    return recording(y, conv.weight, conv.bias, bn.weight, bn.bias)


def _tail_workspace(B, H, W, C, dev):
    need = L.lib.ppn_gennet_tail_train_workspace(B, H, W, C)
    if need < 0:
        raise L.PpnError(f"ppn_gennet_tail_train_workspace refuses B {B} H {H} W {W} C {C}", -1)
    return torch.empty(max(need, 16) // 4, dtype=torch.float32, device=dev)


def _tail_fwd(y, gamma, beta, wf, bf, eps, slope):
    """ppn_gennet_tail_train_fwd on contiguous tensors (y [B,C,H,W] float32 or bfloat16; gamma, beta [C], wf [1,C,3,3] or [C,9], bf [1] or
    None = no bias, float32): (out [B,1,H,W] of y's dtype, stats [3,C] float32)."""
    B, C, H, W = y.shape
    out = torch.empty(B, 1, H, W, dtype=y.dtype, device=y.device)
    stats = torch.empty(3, C, dtype=torch.float32, device=y.device)
    ws = _tail_workspace(B, H, W, C, y.device)
    with torch.cuda.device(y.device):
        rc = L.lib.ppn_gennet_tail_train_fwd(_p(y), _p(gamma), _p(beta), _p(wf), _p(bf), _p(out), _p(stats), _p(ws), B, H, W, C, float(eps),
                                             float(slope), _DT[y.dtype], _stream(y))
    L.check(rc, "ppn_gennet_tail_train_fwd")
    TAIL_CALLS["fwd"] += 1
    return out, stats


def _tail_bwd(dout, y, gamma, beta, wf, stats, slope, need_dy=True, need_dbf=True):
    """ppn_gennet_tail_train_bwd on contiguous tensors: (dy like y or None, dgamma [C], dbeta [C], dwf shaped like wf, dbf [1] or None)."""
    B, C, H, W = y.shape
    dy = torch.empty_like(y) if need_dy else None
    dgamma, dbeta, dwf = torch.empty_like(gamma), torch.empty_like(beta), torch.empty_like(wf)
    dbf = torch.empty(1, dtype=torch.float32, device=y.device) if need_dbf else None
    ws = _tail_workspace(B, H, W, C, y.device)
    with torch.cuda.device(y.device):
        rc = L.lib.ppn_gennet_tail_train_bwd(_p(dout), _p(y), _p(gamma), _p(beta), _p(wf), _p(stats), _p(ws), _p(dy), _p(dgamma), _p(dbeta), _p(dwf),
                                             _p(dbf), B, H, W, C, float(slope), _DT[y.dtype], _stream(y))
    L.check(rc, "ppn_gennet_tail_train_bwd")
    TAIL_CALLS["bwd"] += 1
    return dy, dgamma, dbeta, dwf, dbf


class _TailTrainFunction(torch.autograd.Function):
    """(out, stats) = conv3x3_to_1(LeakyReLU(BatchNorm_train(y))) on ppn_gennet_tail_train_fwd / ppn_gennet_tail_train_bwd.  Saved: y, the
    parameters and the statistics [3,C] — nothing else of y's size.  y gets dy, or None (and no second pass) when it needs no gradient."""

    @staticmethod
    def forward(ctx, y, gamma, beta, wf, bf, eps, slope):
        gamma, beta, wf = gamma.detach().contiguous(), beta.detach().contiguous(), wf.detach().contiguous()
        bf = bf.detach().contiguous() if bf is not None else None
        out, stats = _tail_fwd(y, gamma, beta, wf, bf, eps, slope)
        ctx.save_for_backward(y, gamma, beta, wf, stats)
        ctx.slope, ctx.bias = slope, bf is not None
        ctx.mark_non_differentiable(stats)
        return out, stats

    @staticmethod
    @once_differentiable
    def backward(ctx, dout, _dstats):
        y, gamma, beta, wf, stats = ctx.saved_tensors
        dy, dgamma, dbeta, dwf, dbf = _tail_bwd(dout.to(y.dtype).contiguous(), y, gamma, beta, wf, stats, ctx.slope, ctx.needs_input_grad[0], ctx.bias)
        return dy, dgamma, dbeta, dwf, dbf, None, None


def tail_bn_act_conv(y, bn, negative_slope, conv):
    """conv(leaky_relu(bn(y))) for GenNet's tail: the last decoder stage's BatchNorm2d and LeakyReLU and conv_final (C -> 1).  Where
    tail_train_ok holds, the HIP pair: two reads of y forward, two reads of y and one write of dy backward, only y kept alive (DESIGN.md
    section 28); out has the dtype the library composition gives (the autocast dtype under bfloat16 autocast, else y's); bn's running
    statistics are updated as F.batch_norm does in training (momentum, the unbiased variance N / (N - 1)) and num_batches_tracked counts
    the call.  Otherwise the library composition, untouched."""
    if not tail_train_ok(y, bn, conv):
        return conv(F.leaky_relu(bn(y), negative_slope))
    out, stats = _TailTrainFunction.apply(y, bn.weight, bn.bias, conv.weight, conv.bias, bn.eps, float(negative_slope))
    with torch.no_grad():
        n, m = y.shape[0] * y.shape[2] * y.shape[3], bn.momentum
        bn.num_batches_tracked.add_(1)
        bn.running_mean.mul_(1.0 - m).add_(stats[0], alpha=m)
        bn.running_var.mul_(1.0 - m).add_(stats[1], alpha=m * n / (n - 1))
    if torch.is_autocast_enabled("cuda") and out.dtype != torch.get_autocast_dtype("cuda"):
        out = out.to(torch.get_autocast_dtype("cuda"))                        # float32 y under autocast: the library's convolution rounds
    return out


# ---------------------------------------------------------------------------------------------------------------- GenNet stride-2 stage training
S2_CALLS = {"down": 0, "up": 0, "wgrad": 0}    # launches of ppn_gennet_s2_down / ppn_gennet_s2_up / ppn_gennet_s2_wgrad (like TAIL_CALLS)
S2_CHANNELS = 24                         # csrc/gennet_s2_train.hip: the one width
S2_TILE = 512                            # small pixels per workgroup tile (ppn_gennet_s2_tile)
S2_MAX_BLOCKS = 768                      # workgroups at most of the weight-gradient kernel (ppn_gennet_s2_max_blocks)
S2_RECORD_MIN = 8 * 24 * 224 * 224       # the smallest big-side numel() that takes the kernels: the smallest measured size at which a
#                                          stage still wins; below it the launches cost more than the library's
S2_DTYPES = frozenset({torch.float32})   # the kernels' data types that take them: the bfloat16 step did not beat the parent's by more
#                                          than the spread when it was measured, so bfloat16 autocast keeps the library


def s2_wgrad_workspace_bytes(B, Hs, Ws):
    """ppn_gennet_s2_wgrad_workspace's formula (include/ppnet_hip.h), of the SMALL grid: per workgroup one float32 partial of the
    24 * 24 * 9 weight-gradient sums and the 2 * 24 channel sums."""
    return (S2_CHANNELS * S2_CHANNELS * 9 + 2 * S2_CHANNELS) * 4 * min(-(-(B * Hs * Ws) // S2_TILE), S2_MAX_BLOCKS)


def library_s2():
    """PPNET_LIBRARY_S2=1 (read at call time, like PPNET_LIBRARY_TAIL): conv_s2 takes the library's Conv2d / ConvTranspose2d and the
    framework's backwards instead of the HIP kernels."""
    return bool(os.environ.get("PPNET_LIBRARY_S2"))


def module_hooked(mod):
    """Whether a forward or backward hook is registered on `mod` (or on every module): such a module is run through its own __call__."""
    from torch.nn.modules import module as M
    return bool(mod._forward_hooks or mod._forward_pre_hooks or mod._backward_hooks or mod._backward_pre_hooks or M._global_forward_hooks
                or M._global_forward_pre_hooks or M._global_backward_hooks or M._global_backward_pre_hooks)


def conv_s2_ok(x, conv):
    """Whether conv_s2 runs conv on the HIP kernels: x a contiguous CUDA [B,24,H,W], float32 or (under bfloat16 autocast only, where the
    library takes it too) bfloat16; conv exactly a Conv2d(24, 24, 3, 2, 1) or a ConvTranspose2d(24, 24, 3, 2, 1, output_padding=1),
    dilation 1, groups 1, zero padding; float32 parameters on x's device; fewer than 2^31 elements on both sides and at least
    S2_RECORD_MIN on the big one; the kernels' data type (bfloat16 under autocast) in S2_DTYPES; autograd recording x or a parameter;
    no autocast or bfloat16 autocast; no hook on conv; and the knob off.  Everything else keeps the library."""
    if library_s2() or not x.is_cuda or x.dtype not in (torch.float32, torch.bfloat16) or x.dim() != 4:
        return False
    if module_hooked(conv):                                                  # a hook watches conv's own call: it keeps it
        return False
    up = type(conv) is torch.nn.ConvTranspose2d
    if not up and type(conv) is not torch.nn.Conv2d:
        return False
    B, C, H, W = x.shape
    if (C != S2_CHANNELS or conv.in_channels != C or conv.out_channels != C or conv.kernel_size != (3, 3) or conv.stride != (2, 2)
            or conv.padding != (1, 1) or conv.dilation != (1, 1) or conv.groups != 1 or conv.padding_mode != "zeros"
            or (up and conv.output_padding != (1, 1))):
        return False
    big = B * C * H * W * (4 if up else 1)
    if B * H * W < 1 or big >= 2 ** 31 or big < S2_RECORD_MIN or not x.is_contiguous():
        return False
    if any(t is not None and (t.dtype != torch.float32 or t.device != x.device) for t in (conv.weight, conv.bias)):
        return False
    autocast = torch.is_autocast_enabled("cuda")
    if autocast and torch.get_autocast_dtype("cuda") != torch.bfloat16:
        return False
    if x.dtype == torch.bfloat16 and not autocast:                           # the library's convolution refuses bfloat16 x x float32 weight
        return False
    if (torch.bfloat16 if autocast else x.dtype) not in S2_DTYPES:            # the data type the kernels would run in
        return False
    return recording(x, conv.weight, conv.bias)


def _s2_down(big, w, bias):
    """ppn_gennet_s2_down on contiguous tensors (big [B,24,H,W] float32 or bfloat16; w [24,24,3,3] read as [out][in], bias [24] or None,
    float32): small [B,24,ceil(H/2),ceil(W/2)] of big's dtype."""
    B, C, H, W = big.shape
    small = torch.empty(B, C, (H + 1) // 2, (W + 1) // 2, dtype=big.dtype, device=big.device)
    with torch.cuda.device(big.device):
        rc = L.lib.ppn_gennet_s2_down(_p(big), _p(w), _p(bias), _p(small), B, H, W, C, _DT[big.dtype], _stream(big))
    L.check(rc, "ppn_gennet_s2_down")
    S2_CALLS["down"] += 1
    return small


def _s2_up(small, w, bias, H, W):
    """ppn_gennet_s2_up on contiguous tensors (small [B,24,ceil(H/2),ceil(W/2)]; w [24,24,3,3] read as [in][out]): big [B,24,H,W]."""
    B, C, Hs, Ws = small.shape
    if (H + 1) // 2 != Hs or (W + 1) // 2 != Ws:
        raise ValueError(f"_s2_up: the extent {H} x {W} does not halve to {Hs} x {Ws}")
    big = torch.empty(B, C, H, W, dtype=small.dtype, device=small.device)
    with torch.cuda.device(small.device):
        rc = L.lib.ppn_gennet_s2_up(_p(small), _p(w), _p(bias), _p(big), B, H, W, C, _DT[small.dtype], _stream(small))
    L.check(rc, "ppn_gennet_s2_up")
    S2_CALLS["up"] += 1
    return big


def _s2_wgrad(small, big, want_small=True, want_big=True):
    """ppn_gennet_s2_wgrad on contiguous tensors of one dtype: (dw [24,24,3,3] as [small channel][big channel], sum_small [24] or None,
    sum_big [24] or None), float32."""
    B, C, H, W = big.shape
    Hs, Ws = small.shape[2], small.shape[3]
    if small.shape[:2] != big.shape[:2] or (H + 1) // 2 != Hs or (W + 1) // 2 != Ws or small.dtype != big.dtype:
        raise ValueError(f"_s2_wgrad: small {tuple(small.shape)} {small.dtype} does not belong to big {tuple(big.shape)} {big.dtype}")
    need = L.lib.ppn_gennet_s2_wgrad_workspace(B, Hs, Ws)
    if need < 0:
        raise L.PpnError(f"ppn_gennet_s2_wgrad_workspace refuses B {B} Hs {Hs} Ws {Ws}", -1)
    ws = torch.empty(max(need, 16) // 4, dtype=torch.float32, device=big.device)
    dw = torch.empty(C, C, 3, 3, dtype=torch.float32, device=big.device)
    ssum = torch.empty(C, dtype=torch.float32, device=big.device) if want_small else None
    bsum = torch.empty(C, dtype=torch.float32, device=big.device) if want_big else None
    with torch.cuda.device(big.device):
        rc = L.lib.ppn_gennet_s2_wgrad(_p(small), _p(big), _p(ws), _p(dw), _p(ssum), _p(bsum), B, H, W, C, _DT[big.dtype], _stream(big))
    L.check(rc, "ppn_gennet_s2_wgrad")
    S2_CALLS["wgrad"] += 1
    return dw, ssum, bsum


class _ConvS2Function(torch.autograd.Function):
    """conv(x) for the two 24 -> 24 stride-2 layer types on ppn_gennet_s2_down / ppn_gennet_s2_up / ppn_gennet_s2_wgrad (the table in
    include/ppnet_hip.h).  `dtype` is the one the kernels run in: x's, or bfloat16 for a float32 x under bfloat16 autocast.  Saved: x in
    that dtype and the weight.  dx comes back in x's own dtype, or None (and no kernel) when x needs no gradient; the bias always gets
    its gradient — a plain channel sum of dy from the weight-gradient pass — because DistributedDataParallel waits for every parameter."""

    @staticmethod
    def forward(ctx, x, w, b, up, dtype):
        w = w.detach().contiguous()
        b = b.detach().contiguous() if b is not None else None
        xk = x.to(dtype).contiguous()
        y = _s2_up(xk, w, b, 2 * x.shape[2], 2 * x.shape[3]) if up else _s2_down(xk, w, b)
        ctx.save_for_backward(xk, w)
        ctx.up, ctx.bias, ctx.x_dtype = up, b is not None, x.dtype
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        xk, w = ctx.saved_tensors
        dy = dy.to(xk.dtype).contiguous()
        dx = None
        if ctx.up:                                                           # ConvTranspose2d: x is the small side
            if ctx.needs_input_grad[0]:
                dx = _s2_down(dy, w, None)
            dw, _, db = _s2_wgrad(xk, dy, False, ctx.bias)
        else:                                                                # Conv2d: x is the big side
            if ctx.needs_input_grad[0]:
                dx = _s2_up(dy, w, None, xk.shape[2], xk.shape[3])
            dw, db, _ = _s2_wgrad(dy, xk, ctx.bias, False)
        if dx is not None and dx.dtype != ctx.x_dtype:
            dx = dx.to(ctx.x_dtype)
        return dx, dw, db, None, None


def conv_s2(x, conv):
    """conv(x) for GenNet's six 24 -> 24 stride-2 stages.  Where conv_s2_ok holds, the HIP kernels, forward and backward (DESIGN.md section
    29); under bfloat16 autocast a float32 x (the first decoder stage's input, from the trunk's residual stream) is cast to bfloat16
    first and the output is bfloat16, as the library gives.  Otherwise the library's conv(x), untouched."""
    if not conv_s2_ok(x, conv):
        return conv(x)
    dtype = torch.bfloat16 if torch.is_autocast_enabled("cuda") else x.dtype
    return _ConvS2Function.apply(x, conv.weight, conv.bias, type(conv) is torch.nn.ConvTranspose2d, dtype)
