"""Which dense op a layer takes: the one place that decides whether a Linear or a 3x3 convolution runs on the build's own MFMA
kernels (ppn_gemm_bf16, ppn_conv3x3_mfma_bf16, through fused.py) or on the ROCm libraries through PyTorch, with the `PPNET_LIBRARY_*`
A/B knobs (read at call time: tests and tools set them after import; PPNET_LIBRARY_ATTENTION likewise sends the training attention of
GenNet's AE-ViT, gennet._Attention, to the library's scaled_dot_product_attention instead of ppn_mhsa_fwd / ppn_mhsa_bwd at head
dim 8, PPNET_LIBRARY_LOSS sends the heads' training loss, heads.resized_decode_losses, to F.interpolate + F.cross_entropy instead of
ppn_resize_ce_fwd / ppn_resize_ce_bwd, and PPNET_LIBRARY_EVAL sends the evaluation's area histograms, heads.resized_eval_areas, to
F.interpolate + argmax + torch.bincount instead of ppn_seg_eval, and PPNET_LIBRARY_STEM sends the training stem of GenNet's AE-ViT,
fused.stem_bn_act, to Conv2d + BatchNorm2d + LeakyReLU instead of ppn_gennet_stem_train_fwd / ppn_gennet_stem_train_bwd, and PPNET_LIBRARY_TAIL its training tail, fused.tail_bn_act_conv, to
BatchNorm2d + LeakyReLU + Conv2d instead of ppn_gennet_tail_train_fwd / ppn_gennet_tail_train_bwd) — plus what every network file shares: stochastic depth, the "GPU inference" predicate, the image normalisation.  nat.py, swin.py, vit.py, heads.py and gennet.py import from here; none imports
segnet.py, which re-exports these names under their earlier underscore spellings."""
import os

import torch
import torch.nn.functional as F

from . import fused


def drop_path(x, rate, training):
    """Stochastic depth per sample (timm's DropPath as SegNet/nat.py:122,145-152 and GenNet/networks/vit.py:150-161 use it):
    identity unless training with rate > 0."""
    if not training or rate <= 0.0:
        return x
    keep = 1.0 - rate
    mask = x.new_empty((x.shape[0],) + (1,) * (x.dim() - 1)).bernoulli_(keep)
    return x * (mask / keep)


def gpu_inference(x):
    """The form Swin and ViT run on the HIP kernels: CUDA tensors and no autograd (everything else is the torch composition)."""
    return x.is_cuda and not torch.is_grad_enabled()


def use_mfma_conv(x, conv, narrow=False):
    """The hand-written MFMA implicit-GEMM convolution (ppn_conv3x3_mfma_bf16) serves bfloat16 inference on the GPU for 3x3,
    padding 1, Cin % 64 == 0, Cout % 256 == 0 (whole 256-wide output tiles); everything else stays on the library.
    narrow=True also takes Cout % 8 == 0 (UPerNet's 64-channel convolutions: a quarter of the 256-wide tile computes — they are
    3 % of the backbone's arithmetic, and a library call per convolution costs more than the idle columns)."""
    if fused.recording(x, conv.weight):
        return False                                   # training: the library convolution (differentiable)
    return (x.is_cuda and x.dtype == torch.bfloat16 and not conv.training and conv.kernel_size == (3, 3) and conv.padding == (1, 1)
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.in_channels % 64 == 0
            and conv.out_channels % (8 if narrow else 256) == 0
            and conv.weight.dtype == torch.bfloat16 and not os.environ.get("PPNET_LIBRARY_CONV"))


# Per-shape gate between the build's GEMMs and the vendor library behind LayerNorm kernels: stream widths C with
# C >= LIBRARY_GEMM_FROM_C or C < LIBRARY_GEMM_BELOW_C take the library.  Defaults from the alternating A/B of tools/ppnet_ab.py
# (DESIGN.md section 4); PPNET_LIBRARY_GEMM_FROM_C / PPNET_LIBRARY_GEMM_BELOW_C override, PPNET_LIBRARY_GEMM=1 = the library everywhere.
# Round 5: NO width takes the library by default.  With the LayerNorm-folded and accumulating epilogues on the 256 x 256 core
# (csrc/mfma_gemm.h EPI_LN_BIAS[_GELU] / EPI_ACCUM_STATS: the old stream read in the epilogue, both wave groups' epilogues side by side)
# the build's kernels on every level take 22.02 ms per SegNet batch against 22.55 with the round-4 gate at 512 and 22.93 with the
# vendor's GEMMs everywhere (alternating on one box, profiles/r05_ppnet_ab.txt): no `Cijk_*` kernel is left in a bf16 batch.
LIBRARY_GEMM_FROM_C = 1 << 30
LIBRARY_GEMM_BELOW_C = 0


def library_width(C):
    if os.environ.get("PPNET_LIBRARY_GEMM"):
        return True
    return (C >= int(os.environ.get("PPNET_LIBRARY_GEMM_FROM_C", LIBRARY_GEMM_FROM_C))
            or C < int(os.environ.get("PPNET_LIBRARY_GEMM_BELOW_C", LIBRARY_GEMM_BELOW_C)))


def own_gemm_ok(x2, lin):
    """The build's own MFMA GEMM (ppn_gemm_bf16) serves bfloat16 inference with K % 64 == 0, K >= 128, N % 8 == 0."""
    K, N = lin.in_features, lin.out_features
    return (x2.is_cuda and x2.dtype == torch.bfloat16 and lin.weight.dtype == torch.bfloat16 and K % 64 == 0 and K >= 128 and N % 8 == 0
            and x2.is_contiguous() and not fused.recording(x2, lin.weight) and not library_width(min(K, N)))


def bias32(lin):
    """A Linear's bias as float32 (zeros if none), cached on the module against its parameter's version."""
    c = lin.__dict__.get("_ppn_b32")
    if c is None:
        c = lin.__dict__["_ppn_b32"] = fused.WeightCache()
    return c.get((lin.bias, lin.weight), lambda: (lin.bias.detach().float().contiguous() if lin.bias is not None
                                                  else torch.zeros(lin.out_features, dtype=torch.float32, device=lin.weight.device)))


def linear(x2, lin, gelu=False):
    """lin(x2) (+ erf GELU) for 2-D x2 on the build's own GEMM where it applies; the framework's call otherwise (float32, odd sizes)."""
    if own_gemm_ok(x2, lin):
        return fused.gemm_bf16(x2, lin.weight.detach(), bias32(lin), "bias_gelu" if gelu else "bias")
    if gelu and x2.is_cuda and x2.dtype == torch.bfloat16:
        return torch._addmm_activation(lin.bias, x2, lin.weight.t(), use_gelu=True)
    y = F.linear(x2, lin.weight, lin.bias)
    return F.gelu(y) if gelu else y


def accumulate(s2, x2, lin):
    """s2 += x2 @ lin.weight^T in place (no bias: the folded layer carries it outside), own GEMM where it applies."""
    if own_gemm_ok(x2, lin) and s2.is_contiguous():
        return fused.gemm_bf16(x2, lin.weight.detach(), None, "accum", out=s2)
    return s2.addmm_(x2, lin.weight.t())


def mfma_weights(conv):
    """(weight as [Cout,3,3,Cin] bfloat16 — the k order of the implicit GEMM — and the bias as float32, zeros if none)."""
    w = conv.weight.detach().permute(0, 2, 3, 1).contiguous()
    b = conv.bias.detach().float().contiguous() if conv.bias is not None else torch.zeros(conv.out_channels, dtype=torch.float32, device=w.device)
    return w, b


IMG_MEAN = (123.675, 116.28, 103.53)       # _base_/datasets/planning_seg.py:12-13
IMG_STD = (58.395, 57.12, 57.375)


def normalize_images(rgb_u8):
    """u8 [B,R,R,3] or float [B,3,R,R] in [0,255] -> (x - mean) / std, [B,3,R,R] (planning_seg.py:12-41)."""
    x = rgb_u8.permute(0, 3, 1, 2).float() if rgb_u8.dtype == torch.uint8 else rgb_u8.float()
    mean = torch.tensor(IMG_MEAN, device=x.device).view(1, 3, 1, 1)
    std = torch.tensor(IMG_STD, device=x.device).view(1, 3, 1, 1)
    return (x - mean) / std
