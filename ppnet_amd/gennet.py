"""GenNet's AE-ViT (reference GenNet/networks/ae_vit.py:12-76 + vit.py:71-161) as an inference module with the
reference's constructor `AEViT(img_channels, out_channels, img_resolution, dim)` and state-dict key names
(`conv_first.{0,1}`, `enc_conv.i.{0,1}`, `vit_blocks.i.{norm1,attn.qkv,attn.proj,norm2,mlp.fc1,mlp.fc2}`,
`dec_conv.i.{0,1}`, `conv_final`), so `model.load_state_dict(torch.load(w)['model'])` (predict.py:51-52) works.

Structure: conv3x3+BN+LeakyReLU stem, int(log2(R//28)) stride-2 conv stages, 3 pre-LN ViT blocks (3 heads,
MLP x4, GELU, LN eps 1e-6) on the (R/2^n)^2 tokens, mirrored transposed-conv stages, conv3x3 to out_channels.
Dense work runs on the ROCm libraries through PyTorch (bf16 autocast optional); pinned against the reference's
own module by tests/golden/g13_aevit.npz.

AESwin (reference GenNet/networks/ae_swin.py on vanilla_swin.py and base.py), the reference's second model, is below AEViT: five
Swin stages with 7 x 7 and 14 x 14 windows between the same kind of conv encoder and decoder, GPU inference on the window-attention
kernels (swin.wmsa_forward); pinned against the reference's own module by tests/golden/g25_aeswin.npz.
"""
import math
from functools import partial

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import fused
from . import swin
from .dense import drop_path, gpu_inference, linear
from .vit import mhsa_autograd


class _Attention(nn.Module):
    def __init__(self, dim, num_heads, qkv_bias=True):
        super().__init__()
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x):
        B, N, C = x.shape
        # GPU training (autograd recording, float32 / bfloat16 tokens, head dim 8): ppn_mhsa_fwd forward, ppn_mhsa_bwd backward
        # (csrc/mhsa_d8.hip) - nothing of size N x N is saved, the gradients are bitwise reproducible.  PPNET_LIBRARY_ATTENTION
        # (read here, at call time) keeps the library's attention below.
        # The kernel sees the projection's output: under autocast that has the autocast dtype, not x's.
        qkv_dtype = torch.get_autocast_dtype("cuda") if x.is_cuda and torch.is_autocast_enabled("cuda") else x.dtype
        if (x.is_cuda and qkv_dtype in (torch.float32, torch.bfloat16) and C == 8 * self.num_heads
                and fused.recording(x, self.qkv.weight, self.qkv.bias, self.proj.weight, self.proj.bias)
                and not os.environ.get("PPNET_LIBRARY_ATTENTION")):
            return self.proj(mhsa_autograd(self.qkv(x), self.num_heads, self.scale))
        q, k, v = self.qkv(x).view(B, N, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4)
        o = F.scaled_dot_product_attention(q, k, v, scale=self.scale)        # softmax(q k^T * scale) v, vit.py:103-109
        return self.proj(o.transpose(1, 2).reshape(B, N, C))


class _Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x):
        return self.fc2(F.gelu(self.fc1(x)))


class _Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio=4, drop_path=0.0):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = _Attention(dim, num_heads)
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = _Mlp(dim, int(dim * mlp_ratio))
        self.drop_path_rate = float(drop_path)    # stochastic depth, training only (vit.py:150,158-161)

    def forward(self, x):
        x = x + drop_path(self.attn(_ln(x, self.norm1)), self.drop_path_rate, self.training)
        return x + drop_path(self.mlp(_ln(x, self.norm2)), self.drop_path_rate, self.training)


def _stage(conv):
    return nn.Sequential(conv, nn.BatchNorm2d(conv.out_channels), nn.LeakyReLU())


def pack_trunk_params(blocks):
    """The float32 parameter blocks ppn_gennet_trunk_bf16 reads (include/ppnet_hip.h), from the ViT blocks' modules."""
    out = []
    for b in blocks:
        f = lambda t: t.detach().float().reshape(-1)
        out += [f(b.norm1.weight), f(b.norm1.bias), f(b.attn.qkv.weight), f(b.attn.qkv.bias), f(b.attn.proj.weight), f(b.attn.proj.bias),
                f(b.norm2.weight), f(b.norm2.bias), f(b.mlp.fc1.weight), f(b.mlp.fc1.bias), f(b.mlp.fc2.weight.detach().float().t().contiguous()),
                f(b.mlp.fc2.bias)]
    return torch.cat(out).contiguous()


def pack_s2_weights(conv):
    """(weights, bias) in the layout ppn_gennet_conv_s2_bf16 reads, from a 24 -> 24 3x3 stride-2 Conv2d / ConvTranspose2d
    (padding 1, output_padding 1) whose BatchNorm is already folded."""
    C = 24
    w = conv.weight.detach().float()
    dev = w.device
    bias = torch.zeros(32, dtype=torch.float32, device=dev)
    if conv.bias is not None:
        bias[:C] = conv.bias.detach().float()
    if isinstance(conv, nn.ConvTranspose2d):                   # weight [ci][co][ky][kx]; out(2iy+a) <- in(iy+dy) through tap ky
        tap = lambda a, d: (1 if d == 0 else None) if a == 0 else (2 if d == 0 else 0)
        wt = torch.zeros(4, 32, 96, dtype=torch.float32, device=dev)
        for a in range(2):
            for b in range(2):
                for dy in range(2):
                    for dx in range(2):
                        ky, kx = tap(a, dy), tap(b, dx)
                        if ky is None or kx is None:
                            continue
                        p = dy * 2 + dx
                        wt[a * 2 + b, :C, p * C:(p + 1) * C] = w[:, :, ky, kx].t()
        return wt.to(torch.bfloat16).contiguous(), bias
    wk = torch.zeros(32, 224, dtype=torch.float32, device=dev)  # weight [co][ci][ky][kx] -> [co][(ky*3+kx)*24 + ci]
    wk[:C, :216] = w.permute(0, 2, 3, 1).reshape(C, 216)
    return wk.to(torch.bfloat16).contiguous(), bias


def pack_first_enc_weights(conv1, conv2):
    """The four parameter blocks of ppn_gennet_first_enc_bf16 (include/ppnet_hip.h) from the BatchNorm-folded first convolution
    (1 -> 24, 3x3, stride 1) and first encoder convolution (24 -> 24, 3x3, stride 2)."""
    C = 24
    dev = conv1.weight.device
    w = conv1.weight.detach().float().reshape(C, 9)
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    w1 = torch.zeros(32, 32, dtype=torch.bfloat16, device=dev)
    w1[:C, 0:9] = hi
    w1[:C, 16:25] = lo
    b1 = torch.zeros(32, dtype=torch.float32, device=dev)
    b1[:C] = conv1.bias.detach().float()
    bh = b1[:C].to(torch.bfloat16)                                         # the bias rides in the product: columns 9 (hi) and 25 (lo)
    w1[:C, 9] = bh                                                         # against the kernel's constant-1 input slots
    w1[:C, 25] = (b1[:C] - bh.float()).to(torch.bfloat16)
    w2 = conv2.weight.detach().float()                                     # [co][ci][ky][kx]
    slot_ci = [(4 * g + e) if e < 4 else ((16 + 4 * g + e - 4) if g < 2 else -1) for g in range(4) for e in range(8)]
    wk2 = torch.zeros(2, 9, 16, 32, dtype=torch.float32, device=dev)
    for k, ci in enumerate(slot_ci):
        if ci < 0:
            continue
        taps = w2[:, ci].reshape(C, 9)                                     # [co][tap]
        for nt in range(2):
            rows = min(16, C - nt * 16)
            wk2[nt, :, :rows, k] = taps[nt * 16:nt * 16 + rows].t()
    b2 = torch.zeros(32, dtype=torch.float32, device=dev)
    if conv2.bias is not None:
        b2[:C] = conv2.bias.detach().float()
    return w1.reshape(2, 16, 32).contiguous(), b1, wk2.to(torch.bfloat16).contiguous(), b2


def _is_s2_stage(c):
    return (c.in_channels == 24 and c.out_channels == 24 and c.kernel_size == (3, 3) and c.stride == (2, 2) and c.padding == (1, 1)
            and c.dilation == (1, 1) and c.groups == 1 and (not isinstance(c, nn.ConvTranspose2d) or c.output_padding == (1, 1)))


class _FusedStage(nn.Module):
    """A conv stage after prepare_inference(): the (transposed) convolution with the BatchNorm folded in runs WITHOUT its
    bias on the library, and bias + LeakyReLU are one in-place pass of the HIP kernel (ppn_bias_act_nhwc) instead of the
    library's separate add and activation kernels.  C % 8 != 0 or a CPU tensor: plain torch ops."""

    def __init__(self, conv, slope):
        super().__init__()
        self.conv, self.slope = conv, slope
        self._f32 = fused.WeightCache()                   # (weight, bias) as float32 for the direct 1-channel kernel
        self._s2 = fused.WeightCache()                    # (packed weight, bias) for the MFMA stride-2 kernels

    def s2_pack(self):
        return self._s2.get((self.conv.weight, self.conv.bias), lambda: pack_s2_weights(self.conv))

    def forward(self, x):
        c = self.conv
        if not (x.is_cuda and c.out_channels % 8 == 0):
            return F.leaky_relu(c(x), self.slope)
        if (isinstance(c, nn.Conv2d) and c.in_channels == 1 and c.out_channels <= 32 and c.kernel_size == (3, 3) and c.stride == (1, 1)
                and c.padding == (1, 1) and c.dilation == (1, 1)):
            # 1 -> dim at full resolution: the direct HIP kernel (ppn_conv3x3_c1_nhwc), bias + LeakyReLU inside
            w32, b32 = self._f32.get((c.weight, c.bias), lambda: (c.weight.detach().float().contiguous(), c.bias.detach().float().contiguous()))
            return fused.conv3x3_c1(x, w32, b32, self.slope)
        if x.dtype == torch.bfloat16 and _is_s2_stage(c) and x.shape[-1] % 2 == 0 and x.shape[-2] % 2 == 0 and not os.environ.get("PPNET_LIBRARY_CONV"):
            # the 24-channel stride-2 stages: MFMA kernel with the weights in registers, bias + LeakyReLU in its epilogue
            wp, bp = self.s2_pack()
            return fused.gennet_conv_s2(x, wp, bp, self.slope, isinstance(c, nn.ConvTranspose2d))
        if isinstance(c, nn.ConvTranspose2d):
            y = F.conv_transpose2d(x, c.weight, None, c.stride, c.padding, c.output_padding, c.groups, c.dilation)
        else:
            y = F.conv2d(x, c.weight, None, c.stride, c.padding, c.dilation, c.groups)
        return fused.bias_act_(y.contiguous(memory_format=torch.channels_last), c.bias, self.slope)


def _run_stage(blk, x):
    """One enc_conv / dec_conv stage.  An unprepared stage (conv, BatchNorm2d, LeakyReLU) runs its convolution through fused.conv_s2: GPU
    training of the 24 -> 24 stride-2 stages takes the HIP kernels forward and backward (ppn_gennet_s2_down / ppn_gennet_s2_up /
    ppn_gennet_s2_wgrad; s2_from_adjoint below is the algebra), everything else the library's conv(x), untouched.  PPNET_LIBRARY_S2
    (read at call time) keeps the library.  BatchNorm and LeakyReLU stay library ops."""
    if type(blk) is nn.Sequential and len(blk) == 3 and not fused.module_hooked(blk):     # a hooked stage keeps its own call
        return blk[2](blk[1](fused.conv_s2(x, blk[0])))
    return blk(x)


def _ln(x, ln):
    # The CPU branches of this module (here and in _FusedStage) are not a product fallback: they let the CPU golden test
    # (tests/test_gennet_golden.py) check the module's wiring against the reference's own outputs without a GPU.  PPNet, the
    # drop-in classes and bench.py run on the GPU only, where every op below is a HIP kernel or a ROCm library call.
    if x.is_cuda:
        return fused.layer_norm(x, ln)                                       # thread-per-row HIP kernel (C = 24)
    return ln(x)


class AEViT(nn.Module):
    def __init__(self, img_channels, out_channels, img_resolution=256, dim=192):
        super().__init__()
        n_down = int(math.log2(img_resolution // 28))                       # ae_vit.py:23
        self.conv_first = _stage(nn.Conv2d(img_channels, dim, 3, 1, 1))
        self.enc_conv = nn.ModuleList(_stage(nn.Conv2d(dim, dim, 3, 2, 1)) for _ in range(n_down))
        dpr = [float(v) for v in torch.linspace(0, 0.1, 3)]                   # ae_vit.py:35-36: drop_path_rate 0.1 over the depth
        self.vit_blocks = nn.Sequential(*[_Block(dim, 3, 4, dpr[i]) for i in range(3)])
        self.dec_conv = nn.ModuleList(_stage(nn.ConvTranspose2d(dim, dim, 3, 2, 1, output_padding=1)) for _ in range(n_down))
        self.conv_final = nn.Conv2d(dim, out_channels, 3, 1, 1)
        self._final_f32 = None                            # set by prepare_inference(): WeightCache of (float32 weight, float bias)
        self._trunk = fused.WeightCache()                 # float32 parameter blocks of the fused ViT-trunk kernel
        self._first_enc = fused.WeightCache()             # packed parameters of the fused first convolution + first encoder stage

    def prepare_inference(self):
        """After the checkpoint is loaded: fold every eval-mode BatchNorm into the (transposed) convolution in front of
        it (exact algebra in float32) and switch the convolution weights to channels_last. Load the state dict first."""
        for stage in [self.conv_first, *self.enc_conv, *self.dec_conv]:
            _fold_bn(stage)
        self.to(memory_format=torch.channels_last)
        self.conv_first = _FusedStage(self.conv_first[0], self.conv_first[2].negative_slope)
        self.enc_conv = nn.ModuleList(_FusedStage(st[0], st[2].negative_slope) for st in self.enc_conv)
        self.dec_conv = nn.ModuleList(_FusedStage(st[0], st[2].negative_slope) for st in self.dec_conv)
        self._final_f32 = fused.WeightCache()
        return self

    def _final_pack(self):
        cf = self.conv_final
        return self._final_f32.get((cf.weight, cf.bias), lambda: (
            cf.weight.detach().float().contiguous(), float(cf.bias.detach().float()[0]) if cf.bias is not None and cf.out_channels == 1 else 0.0))

    def _fused_first_stage(self, x):
        """Prepared bfloat16 inference: conv_first and enc_conv[0] as one kernel (ppn_gennet_first_enc_bf16), or None."""
        cf = self.conv_first
        if not (isinstance(cf, _FusedStage) and len(self.enc_conv) > 0 and isinstance(self.enc_conv[0], _FusedStage) and x.is_cuda
                and x.dtype == torch.bfloat16 and not os.environ.get("PPNET_GENNET_UNFUSED")):
            return None
        c1, c2 = cf.conv, self.enc_conv[0].conv
        if not (isinstance(c1, nn.Conv2d) and c1.in_channels == 1 and c1.out_channels == 24 and c1.kernel_size == (3, 3) and c1.stride == (1, 1)
                and c1.padding == (1, 1) and c1.bias is not None and isinstance(c2, nn.Conv2d) and _is_s2_stage(c2)
                and x.shape[-1] % 2 == 0 and x.shape[-2] % 2 == 0):
            return None
        packs = self._first_enc.get((c1.weight, c1.bias, c2.weight, c2.bias), lambda: pack_first_enc_weights(c1, c2))
        return fused.gennet_first_enc(x, *packs, cf.slope, self.enc_conv[0].slope)

    def forward(self, x):
        y = self._fused_first_stage(x)
        if y is not None:
            x = y
            for blk in self.enc_conv[1:]:
                x = blk(x)
        else:
            cf = self.conv_first
            if (isinstance(cf, nn.Sequential) and len(cf) == 3 and type(cf[2]) is nn.LeakyReLU and fused.stem_train_ok(x, cf[0], cf[1])):
                # GPU training of the unprepared stem: conv + BatchNorm (batch statistics) + LeakyReLU as one write of z and one read
                # of dz (ppn_gennet_stem_train_fwd / ppn_gennet_stem_train_bwd; stem_from_moments below is the algebra).
                # PPNET_LIBRARY_STEM (read at call time) keeps the three library ops.
                x = fused.stem_bn_act(x, cf[0], cf[1], cf[2].negative_slope)
            else:
                x = cf(x)
            for blk in self.enc_conv:
                x = _run_stage(blk, x)
        B, C, H, W = x.shape
        if (x.is_cuda and x.dtype == torch.bfloat16 and self._final_f32 is not None and C == 24 and H * W <= 1024 and (H * W) % 8 == 0
                and self.vit_blocks[0].attn.num_heads == 3 and not os.environ.get("PPNET_LIBRARY_TRUNK")):
            # prepared bfloat16 inference: the three ViT blocks are one kernel (residual stream in registers, K / V in LDS)
            trunk = self._trunk.get(list(self.vit_blocks.parameters()), lambda: pack_trunk_params(self.vit_blocks).to(x.device))
            x = fused.gennet_trunk(x.contiguous(memory_format=torch.channels_last), trunk, len(self.vit_blocks))
        else:
            t = self.vit_blocks(x.flatten(2).transpose(1, 2))                # feature2token / token2feature, base.py:43-52
            x = t.transpose(1, 2).reshape(B, C, H, W)
        c = self.conv_final
        last = self.dec_conv[-1] if len(self.dec_conv) else None
        if (isinstance(last, _FusedStage) and x.is_cuda and x.dtype == torch.bfloat16 and self._final_f32 is not None and c.out_channels == 1
                and c.in_channels == 24 and isinstance(last.conv, nn.ConvTranspose2d) and _is_s2_stage(last.conv)
                and not os.environ.get("PPNET_GENNET_UNFUSED_TAIL") and not os.environ.get("PPNET_LIBRARY_CONV")):
            # prepared bfloat16 inference: the last decoder stage and the final convolution are one kernel — the 24-channel tensor
            # at the output resolution never reaches memory (ppn_gennet_dec_final_bf16; bit-identical to the two kernels)
            for blk in self.dec_conv[:-1]:
                x = blk(x)
            wp, bp = last.s2_pack()
            wf, bf = self._final_pack()
            return fused.gennet_dec_final(x, wp, bp, last.slope, wf, bf)
        if isinstance(last, nn.Sequential) and len(last) == 3 and type(last[2]) is nn.LeakyReLU and self._final_f32 is None:
            # the unprepared last stage, step by step: GPU training runs its BatchNorm (batch statistics) + LeakyReLU and conv_final as
            # two reads of y and, backward, two reads of y and one write of dy (ppn_gennet_tail_train_fwd / ppn_gennet_tail_train_bwd;
            # tail_from_sums below is the algebra).  PPNET_LIBRARY_TAIL (read at call time) keeps the three library ops.
            for blk in self.dec_conv[:-1]:
                x = _run_stage(blk, x)
            y = fused.conv_s2(x, last[0])
            if fused.tail_train_ok(y, last[1], c):
                return fused.tail_bn_act_conv(y, last[1], last[2].negative_slope, c)
            x = last[2](last[1](y))
        else:
            for blk in self.dec_conv:
                x = blk(x)
        if x.is_cuda and self._final_f32 is not None and c.out_channels == 1 and c.in_channels % 8 == 0 and c.in_channels <= 32:
            wf, bf = self._final_pack()                                      # dim -> 1 at full resolution: direct HIP kernel
            return fused.conv3x3_to1(x, wf, bf)
        return c(x)


class _WindowAttention(nn.Module):
    """vanilla_swin.py:191-284: parameters relative_position_bias_table [(2w-1)^2, heads], qkv, proj; buffer relative_position_index.
    forward takes the qkv projection's input on the token GRID [B,H,W,C] (after norm1) — padding, shift, window partition, mask,
    window reverse, reverse shift and crop (vanilla_swin.py:334-368) are index arithmetic of the kernel / of swin.window_attention."""

    def __init__(self, dim, window, num_heads, shift):
        super().__init__()
        self.dim, self.window, self.num_heads, self.shift = dim, window, num_heads, shift
        self.scale = (dim // num_heads) ** -0.5
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * window - 1) ** 2, num_heads))
        self.register_buffer("relative_position_index", swin._relative_index(window))
        self.qkv = nn.Linear(dim, dim * 3)
        self.proj = nn.Linear(dim, dim)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)
        self._rpb32 = fused.WeightCache()                 # the table as the kernel's float32 [heads, 2w-1, 2w-1]

    def on_kernel(self, qkv):
        """GPU inference (CUDA, no autograd) in float32 / bfloat16 with a (window, head dim) of the HIP kernels; PPNET_LIBRARY_WMSA=1
        (read here, at call time) keeps the torch composition."""
        return (gpu_inference(qkv) and qkv.dtype in (torch.float32, torch.bfloat16) and self.dim % self.num_heads == 0
                and swin.kernel_takes(self.window, self.dim // self.num_heads) and not os.environ.get("PPNET_LIBRARY_WMSA"))

    def attend(self, qkv):
        """qkv [B,H,W,3C] -> the attention output [B,H,W,C] before proj: ppn_wmsa_fwd / ppn_swin_wmsa_fwd (swin.wmsa_forward) where
        on_kernel holds, the differentiable torch composition everywhere else (CPU, autograd, head dims 4 / 2 / 1 of dim = 24)."""
        t = self.relative_position_bias_table
        if self.on_kernel(qkv):
            rpb = self._rpb32.get((t,), lambda: swin.bias_table_hw(t.detach().float(), self.num_heads, self.window).contiguous())
            return swin.wmsa_forward(qkv, self.qkv.bias, rpb, self.num_heads, self.shift, self.scale, self.window)
        return swin.window_attention(qkv, self.qkv.bias, t, self.num_heads, self.shift, self.scale, self.window)

    def forward(self, x):
        B, H, W, C = x.shape
        x2 = x.reshape(-1, C)
        fast = gpu_inference(x)
        qkv = (linear(x2.contiguous(), self.qkv) if fast else self.qkv(x2)).view(B, H, W, 3 * C)
        o = self.attend(qkv).reshape(-1, C)
        return (linear(o.contiguous(), self.proj) if fast else self.proj(o)).view(B, H, W, C)


class _SwinMlp(nn.Module):
    """vanilla_swin.py:168-188 with the reference's activation for this model: LeakyReLU, not GELU (vanilla_swin.py:171,306)."""

    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x):
        if gpu_inference(x):
            x2 = x.reshape(-1, x.shape[-1]).contiguous()
            return linear(F.leaky_relu_(linear(x2, self.fc1)), self.fc2).view(x.shape)
        return self.fc2(F.leaky_relu(self.fc1(x)))


class _SwinBlock(nn.Module):
    """vanilla_swin.py:287-376 on the token grid [B,H,W,C]: x + drop_path(attn(norm1(x))), then x + drop_path(mlp(norm2(x)))."""

    def __init__(self, dim, num_heads, window, shift, drop_path=0.0):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.attn = _WindowAttention(dim, window, num_heads, shift)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = _SwinMlp(dim, int(dim * 4))
        self.drop_path_rate = float(drop_path)

    def forward(self, x, y=None, next_norm=None):
        """x: the residual stream; y = norm1(x) if the caller has it.  Returns (x', next_norm(x') or None)."""
        if gpu_inference(x):
            # LayerNorm and the residual adds on the fused kernels (x is updated in place: the stage hands over a fresh tensor)
            if y is None:
                y = fused.layer_norm(x, self.norm1)
            x, y2 = fused.residual_layer_norm(x, self.attn(y), None, self.norm2)
            return fused.residual_layer_norm(x, self.mlp(y2), None, next_norm)
        x = x + drop_path(self.attn(self.norm1(x)), self.drop_path_rate, self.training)
        x = x + drop_path(self.mlp(self.norm2(x)), self.drop_path_rate, self.training)
        return x, None


class _Resample(nn.Module):
    """base.py:4-40, PatchMerging / PatchUpsampling: a stride-2 (transposed) convolution + BatchNorm2d + LeakyReLU on the token grid
    (key `conv.{0,1}`).  [B,H,W,C] -> [B,H',W',C]."""

    def __init__(self, conv):
        super().__init__()
        self.conv = _stage(conv)

    def forward(self, x):
        return _run_stage(self.conv, x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)


class _SwinStage(nn.Module):
    """vanilla_swin.py:379-467, BasicLayer: `depth` blocks, the odd ones shifted by window // 2 — always, also when one window covers
    the whole grid (vanilla_swin.py:406,414) — then the optional resampling."""

    def __init__(self, dim, depth, num_heads, window, drop_path, downsample):
        super().__init__()
        self.blocks = nn.ModuleList(_SwinBlock(dim, num_heads, window, 0 if i % 2 == 0 else window // 2, drop_path[i]) for i in range(depth))
        self.downsample = downsample

    def forward(self, x):
        if gpu_inference(x):
            x = x.contiguous().clone()                     # the fused kernels update the stream in place
        y = None
        for i, blk in enumerate(self.blocks):
            x, y = blk(x, y, self.blocks[i + 1].norm1 if i + 1 < len(self.blocks) else None)
        return x if self.downsample is None else self.downsample(x)


class AESwin(nn.Module):
    """GenNet's second model (reference GenNet/networks/ae_swin.py:10-85 on vanilla_swin.py and base.py) with the reference's constructor
    and its state-dict keys (`conv_first.{0,1}`, `enc_conv.i.{0,1}`, `swin.s.blocks.j.{norm1,attn.{relative_position_bias_table,
    relative_position_index,qkv,proj},norm2,mlp.{fc1,fc2}}`, `swin.s.downsample.conv.{0,1}` on stages 0, 1, 3, 4, `dec_conv.i.{0,1}`,
    `conv_final`), so a reference checkpoint loads with strict=True.

    Structure: conv3x3 + BN + LeakyReLU stem, int(log2(R // 56)) stride-2 conv stages, five Swin stages (depths 2, 3, 4, 3, 2; heads 6,
    12, 24, 12, 6; windows 7, 14, 14, 14, 7; LeakyReLU MLP x4; LN eps 1e-5; drop path 0.1 spread over the 14 blocks) on token grids
    g, g/2, g/4, g/4, g/2 with stride-2 (transposed) convolutions between them, mirrored transposed-conv stages, conv3x3 to
    out_channels.  GPU inference runs the window attention on ppn_wmsa_fwd / ppn_swin_wmsa_fwd, LayerNorm and the residual adds on the
    fused kernels and the Linears through dense.linear; the LeakyReLU, the dim-channel convolutions and everything under autograd or
    on the CPU are library ops."""

    DEPTHS, RATIOS, HEADS, WINDOWS = (2, 3, 4, 3, 2), (0.5, 0.5, 1, 2, 2), (6, 12, 24, 12, 6), (7, 14, 14, 14, 7)

    def __init__(self, img_channels, out_channels, img_resolution=256, dim=192):
        super().__init__()
        n_down = int(math.log2(img_resolution // 56))                        # ae_swin.py:21
        self.conv_first = _stage(nn.Conv2d(img_channels, dim, 3, 1, 1))
        self.enc_conv = nn.ModuleList(_stage(nn.Conv2d(dim, dim, 3, 2, 1)) for _ in range(n_down))
        dpr = [float(v) for v in torch.linspace(0, 0.1, sum(self.DEPTHS))]   # ae_swin.py:35-36
        self.swin = nn.ModuleList()
        for i, depth in enumerate(self.DEPTHS):
            r = self.RATIOS[i]
            merge = (_Resample(nn.Conv2d(dim, dim, 3, 2, 1)) if r < 1 else
                     _Resample(nn.ConvTranspose2d(dim, dim, 3, 2, 1, output_padding=1)) if r > 1 else None)
            lo = sum(self.DEPTHS[:i])
            self.swin.append(_SwinStage(dim, depth, self.HEADS[i], self.WINDOWS[i], dpr[lo:lo + depth], merge))
        self.dec_conv = nn.ModuleList(_stage(nn.ConvTranspose2d(dim, dim, 3, 2, 1, output_padding=1)) for _ in range(n_down))
        self.conv_final = nn.Conv2d(dim, out_channels, 3, 1, 1)
        self._final_f32 = None                            # set by prepare_inference(): WeightCache of (float32 weight, float bias)

    def _conv_stages(self):
        """(owner, attribute or index) of every conv + BatchNorm + LeakyReLU stage, the four inside the Swin stages included."""
        out = [(self, "conv_first")]
        out += [(self.enc_conv, i) for i in range(len(self.enc_conv))]
        out += [(st.downsample, "conv") for st in self.swin if st.downsample is not None]
        return out + [(self.dec_conv, i) for i in range(len(self.dec_conv))]

    def prepare_inference(self):
        """As AEViT.prepare_inference: fold every eval-mode BatchNorm into the (transposed) convolution in front of it (float32
        algebra), switch the convolution weights to channels_last and wrap each stage in _FusedStage.  Load the state dict first."""
        stages = self._conv_stages()
        for owner, key in stages:
            stage = getattr(owner, key) if isinstance(key, str) else owner[key]
            _fold_bn(stage)
        self.to(memory_format=torch.channels_last)
        for owner, key in stages:
            stage = getattr(owner, key) if isinstance(key, str) else owner[key]
            f = _FusedStage(stage[0], stage[2].negative_slope)
            if isinstance(key, str):
                setattr(owner, key, f)
            else:
                owner[key] = f
        self._final_f32 = fused.WeightCache()
        return self

    def forward(self, x):
        x = self.conv_first(x)
        for blk in self.enc_conv:
            x = _run_stage(blk, x)
        x = x.permute(0, 2, 3, 1)                                            # feature2token, kept as a grid: [B,H,W,C]
        for stage in self.swin:
            x = stage(x)
        x = x.permute(0, 3, 1, 2)                                            # token2feature
        for blk in self.dec_conv:
            x = _run_stage(blk, x)
        c = self.conv_final
        if x.is_cuda and self._final_f32 is not None and c.out_channels == 1 and c.in_channels % 8 == 0 and c.in_channels <= 32:
            wf, bf = self._final_f32.get((c.weight, c.bias), lambda: (
                c.weight.detach().float().contiguous(), float(c.bias.detach().float()[0]) if c.bias is not None else 0.0))
            return fused.conv3x3_to1(x, wf, bf)                              # dim -> 1 at full resolution: direct HIP kernel
        return c(x)


def _fold_bn(stage):
    """Fold the eval-mode BatchNorm2d of a (conv, BatchNorm2d, LeakyReLU) stage into its (transposed) convolution, exactly, in the
    parameters' dtype; the BatchNorm becomes an Identity."""
    conv, bn = stage[0], stage[1]
    if not isinstance(bn, nn.BatchNorm2d):
        return
    scale = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).detach()
    shape = (1, -1, 1, 1) if isinstance(conv, nn.ConvTranspose2d) else (-1, 1, 1, 1)             # out-channel axis
    conv.weight = nn.Parameter(conv.weight.detach() * scale.view(shape))
    conv.bias = nn.Parameter(((conv.bias.detach() if conv.bias is not None else 0) - bn.running_mean) * scale + bn.bias.detach())
    stage[1] = nn.Identity()


def stem_from_moments(x, dz, w, b, gamma, beta, eps, slope):
    """The algebra of the stem's training kernels (csrc/gennet_stem_train.hip) in torch ops, in the inputs' dtype,
    on any device: z = leaky_relu(BatchNorm_train(conv3x3(x) + b)) and the parameter gradients for an upstream dz, with the batch
    statistics from the 54 moments of the input's 3 x 3 patches and the backward from per-channel sums — neither pass forms a
    gradient of y's size.  x [B,H,W] or [B,1,H,W]; dz [B,C,H,W]; w [C,1,3,3] or [C,9]; b [C] or None; gamma, beta [C].
    Returns (z, mean, biased var, dW shaped like w, dgamma, dbeta); the gradient of b is exactly 0."""
    B, H, W = x.shape[0], x.shape[-2], x.shape[-1]
    C, N = w.shape[0], x.shape[0] * x.shape[-2] * x.shape[-1]
    w9 = w.reshape(C, 9)
    b = torch.zeros(C, dtype=x.dtype, device=x.device) if b is None else b
    p = F.unfold(x.reshape(B, 1, H, W), 3, padding=1).transpose(1, 2).reshape(N, 9)      # zero-padded patches, tap 3 dy + dx
    S1, S2 = p.sum(0), p.t() @ p                                                      # one pass over the 1-channel input
    m = S1 / N
    cov = S2 / N - torch.outer(m, m)
    mean, var = w9 @ m + b, ((w9 @ cov) * w9).sum(1)
    rstd = torch.rsqrt(var + eps)
    xh = (p @ w9.t() + (b - mean)) * rstd                                             # [N, C], recomputed by the backward
    u = gamma * xh + beta
    z = torch.where(u > 0, u, u * slope).reshape(B, H, W, C).permute(0, 3, 1, 2)
    g = dz.permute(0, 2, 3, 1).reshape(N, C)
    g = torch.where(u > 0, g, g * slope)
    dbeta, dgamma, G = g.sum(0), (g * xh).sum(0), g.t() @ p                           # 11 sums per channel
    X = rstd[:, None] * (w9 @ S2 + (b - mean)[:, None] * S1)                          # sum xhat p, from the moments
    dW = (gamma * rstd)[:, None] * (G - (dbeta / N)[:, None] * S1 - (dgamma / N)[:, None] * X)
    return z, mean, var, dW.reshape(w.shape), dgamma, dbeta


def tail_from_sums(y, dout, gamma, beta, wf, bf, eps, slope):
    """The algebra of the tail's training kernels (csrc/gennet_tail_train.hip) in torch ops, in the inputs' dtype, on
    any device: out = conv3x3(leaky_relu(BatchNorm_train(y))) + bf with C -> 1 channels, and every gradient for an upstream dout.  The
    batch statistics come from sum y and sum y^2; z is zero outside the image; everything that flows back through the one-channel
    convolution is a 3 x 3 stencil of dout, so neither z nor its gradient is kept: 11 sums per channel (and sum dout), then dy.
    y [B,C,H,W]; dout [B,1,H,W]; gamma, beta [C]; wf [1,C,3,3] or [C,9]; bf [1] or None.
    Returns (out, mean, biased var, dy, dgamma, dbeta, dWf shaped like wf, dbf [1] or None)."""
    B, C, H, W = y.shape
    N = B * H * W
    v = lambda t: t.reshape(1, C, 1, 1)
    mean = y.sum((0, 2, 3)) / N
    var = ((y * y).sum((0, 2, 3)) / N - mean * mean).clamp_min(0)
    rstd = torch.rsqrt(var + eps)
    xh = (y - v(mean)) * v(rstd)
    u = v(gamma) * xh + v(beta)
    z = torch.where(u > 0, u, u * slope)
    w9 = wf.reshape(C, 9)
    zp, dp = F.pad(z, (1, 1, 1, 1)), F.pad(dout, (1, 1, 1, 1))                            # zero outside the image, both
    out = torch.zeros_like(dout) if bf is None else bf.reshape(1, 1, 1, 1).expand_as(dout).clone()
    dz, dW = torch.zeros_like(y), torch.zeros_like(w9)
    for t in range(9):
        r, j = divmod(t, 3)
        out += (zp[:, :, r:r + H, j:j + W] * v(w9[:, t])).sum(1, keepdim=True)          # z(p + tap)
        ds = dp[:, :, 2 - r:2 - r + H, 2 - j:2 - j + W]                                   # d(q - tap), shared by all channels
        dz += v(w9[:, t]) * ds
        dW[:, t] = (z * ds).sum((0, 2, 3))
    g = torch.where(u > 0, dz, dz * slope)
    dbeta, dgamma = g.sum((0, 2, 3)), (g * xh).sum((0, 2, 3))                             # with dW: 11 sums per channel
    dy = v(gamma * rstd) * (g - v(dbeta) / N - xh * v(dgamma) / N)
    return out, mean, var, dy, dgamma, dbeta, dW.reshape(wf.shape), None if bf is None else dout.sum().reshape(1)


def s2_from_adjoint(x, dy, weight, transposed):
    """The algebra of the stride-2 stages' training kernels (csrc/gennet_s2_train.hip) in torch ops, in the inputs'
    dtype, on any device: one adjoint pair D (big -> small) / U (small -> big) and one reduction W serve Conv2d(C, C, 3, 2, 1) and
    ConvTranspose2d(C, C, 3, 2, 1, output_padding=1) with the weight as stored, built from strided slices and einsum.
    x [B,C,H,W]; dy shaped like the layer's output; weight [C,C,3,3] ([out][in] for Conv2d, [in][out] transposed).
    Returns (forward without bias, dx, dw in the stored layout, dbias)."""
    def taps(big, Hs, Ws):                                                   # tap (ky, kx) -> big(2i + ky - 1, 2j + kx - 1), zero outside
        H, W = big.shape[2], big.shape[3]
        bp = F.pad(big, (1, 2 * Ws - W, 1, 2 * Hs - H))
        return [[bp[:, :, ky:ky + 2 * Hs:2, kx:kx + 2 * Ws:2] for kx in range(3)] for ky in range(3)]

    def down(big, w):                                                        # D: w [out][in]
        Hs, Ws = (big.shape[2] + 1) // 2, (big.shape[3] + 1) // 2
        t = taps(big, Hs, Ws)
        return sum(torch.einsum("oc,bcij->boij", w[:, :, ky, kx], t[ky][kx]) for ky in range(3) for kx in range(3))

    def up(small, w, H, W):                                                  # U: w [in][out], scattered through D's own index map
        B, _, Hs, Ws = small.shape
        op = torch.zeros(B, w.shape[1], 2 * Hs + 1, 2 * Ws + 1, dtype=small.dtype, device=small.device)
        for ky in range(3):
            for kx in range(3):
                op[:, :, ky:ky + 2 * Hs:2, kx:kx + 2 * Ws:2] += torch.einsum("ac,baij->bcij", w[:, :, ky, kx], small)
        return op[:, :, 1:1 + H, 1:1 + W]

    def wgrad(small, big):                                                   # W: [small channel][big channel][3][3]
        t = taps(big, small.shape[2], small.shape[3])
        return torch.stack([torch.stack([torch.einsum("baij,bcij->ac", small, t[ky][kx]) for kx in range(3)], -1) for ky in range(3)], -2)

    if transposed:
        return up(x, weight, 2 * x.shape[2], 2 * x.shape[3]), down(dy, weight), wgrad(x, dy), dy.sum((0, 2, 3))
    return down(x, weight), up(dy, weight, x.shape[2], x.shape[3]), wgrad(dy, x), dy.sum((0, 2, 3))


AE = AEViT      # predict.py:12 `from networks import AEViT as AE`


def normalize_heatmap_u8(y):
    """predict.py:95-102 per sample: (y - min) / (max - min) -> 8-bit 'L' image. y [B,1,R,R] -> u8 [B,R,R]."""
    B = y.shape[0]
    f = y.float().reshape(B, -1)
    lo = f.min(dim=1, keepdim=True).values
    hi = f.max(dim=1, keepdim=True).values
    n = (f - lo) / (hi - lo)
    return (n * 255).to(torch.uint8).reshape(B, y.shape[-2], y.shape[-1])    # ToPILImage: mul(255).byte()


WEIGHTS_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "weights")


def trained_checkpoint(resolution):
    """Path of the GenNet checkpoint this build trained itself at `resolution` (tools/train_gennet.py: the build's own training step
    on pairs from the build's own generator; the reference ships no weights), or None.  The file has the reference's layout —
    {'model': state_dict}, float32 (GenNet/train.py:133-141; predict.py:51-52 reads that key)."""
    path = os.path.join(WEIGHTS_DIR, f"gennet_r{int(resolution)}.pth")
    return path if os.path.exists(path) else None


def load_trained(model, resolution):
    """Load trained_checkpoint(resolution) into an (unprepared) AEViT the way predict.py:51-52 does; returns True if there was one."""
    path = trained_checkpoint(resolution)
    if path is None:
        return False
    model.load_state_dict(torch.load(path, map_location="cpu", weights_only=True)["model"], strict=True)
    return True
