"""NAT / DiNAT backbone (reference SegNet/nat.py:17-332, dinat.py:15-22) as plain nn.Modules with the reference's constructor
arguments and checkpoint key names (`patch_embed.proj.{0,1}`, `levels.i.blocks.j.{norm1,attn.{qkv,rpb,proj},norm2,mlp.{fc1,fc2},
gamma1,gamma2}`, `levels.i.downsample.{reduction,norm}`, `norm{i}`).  The neighbourhood attention is the hand-written HIP kernel
(ppnet_amd/na.py); the tokenizer, the downsampler and the linear projections take the build's own kernels or the ROCm libraries
through PyTorch as ppnet_amd/dense.py decides."""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import fused
from .dense import IMG_MEAN, IMG_STD, accumulate, library_width, linear, mfma_weights, use_mfma_conv
from .na import NeighborhoodAttention2D


class ConvTokenizer(nn.Module):
    def __init__(self, in_chans=3, embed_dim=96, norm_layer=None):
        super().__init__()
        self.proj = nn.Sequential(nn.Conv2d(in_chans, embed_dim // 2, 3, 2, 1), nn.Conv2d(embed_dim // 2, embed_dim, 3, 2, 1))
        self.norm = norm_layer(embed_dim) if norm_layer is not None else None

    def forward(self, x):
        # channels_last in, channels_last out: the NHWC token tensor is a zero-copy view of the conv output
        x = self.proj(x.contiguous(memory_format=torch.channels_last)).permute(0, 2, 3, 1)
        return fused.layer_norm(x, self.norm) if self.norm is not None else x

    _codes = None         # WeightCache of (lut, second convolution's bias as float32, packed second conv, vectors) for forward_codes

    def takes_codes(self, grid_u8):
        c0, c1 = self.proj[0], self.proj[1]
        return (grid_u8.is_cuda and grid_u8.dtype == torch.uint8 and grid_u8.dim() == 3 and grid_u8.shape[1] % 2 == 0
                and grid_u8.shape[2] % 32 == 0 and c0.weight.shape == (64, 3, 3, 3) and c0.weight.dtype == torch.bfloat16
                and self.norm is not None and c1.bias is not None and not os.environ.get("PPNET_LIBRARY_TOKENIZER"))

    def forward_codes(self, grid_u8):
        """The tokens of the palette image of u8 occupancy codes [B,R,R] (what ppn_grid_to_image would render): the first
        convolution is a table product on the matrix cores (ppn_tokenizer_conv1_codes_bf16), the second convolution runs
        without its bias, which the LayerNorm kernel adds in registers — the normalised image and two bias passes are
        never written."""
        c0, c1 = self.proj[0], self.proj[1]
        if self._codes is None:
            self._codes = fused.WeightCache()
        lut, b2, w2p, vec = self._codes.get(
            (c0.weight, c0.bias, c1.weight, c1.bias, self.norm.weight, self.norm.bias),
            lambda: (fused.tokenizer_lut(c0, IMG_MEAN, IMG_STD).to(grid_u8.device), c1.bias.detach().float().contiguous())
            + fused.tokenizer_pack(c1, self.norm))
        if (c1.weight.shape == (128, 64, 3, 3) and grid_u8.shape[1] % 4 == 0 and grid_u8.shape[2] % 64 == 0
                and not os.environ.get("PPNET_TOKENIZER_TWO_KERNELS")):
            # both convolutions and the LayerNorm in one kernel (ppn_tokenizer_codes_bf16): no library convolution, no intermediate
            return fused.tokenizer_codes(grid_u8, lut, w2p, vec, self.norm.eps)
        x = fused.tokenizer_conv1_codes(grid_u8, lut).permute(0, 3, 1, 2)
        x = F.conv2d(x, c1.weight, None, c1.stride, c1.padding).permute(0, 2, 3, 1)
        return fused.layer_norm(x, self.norm, offset=b2)


class ConvDownsampler(nn.Module):
    def __init__(self, dim, norm_layer=nn.LayerNorm):
        super().__init__()
        self.reduction = nn.Conv2d(dim, 2 * dim, 3, 2, 1, bias=False)
        self.norm = norm_layer(2 * dim)

    _mfma = None          # WeightCache of (weight [2C,3,3,C] bf16, zero bias float32) for the MFMA implicit-GEMM kernel

    def forward(self, x):                      # x [B,H,W,C] contiguous == a channels_last [B,C,H,W] view: no layout copies
        if use_mfma_conv(x, self.reduction):
            if self._mfma is None:
                self._mfma = fused.WeightCache()
            w, b = self._mfma.get((self.reduction.weight,), lambda: mfma_weights(self.reduction))
            y = fused.conv3x3_mfma(x.permute(0, 3, 1, 2), w, b, stride=2, relu=False)
            return fused.layer_norm(y.permute(0, 2, 3, 1), self.norm)
        return fused.layer_norm(self.reduction(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1), self.norm)


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.0):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features or in_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features or in_features, out_features or in_features)

    def _erf_gelu(self):
        return isinstance(self.act, nn.GELU) and self.act.approximate == "none"

    def _gelu_epilogue(self, x):
        return x.is_cuda and x.dtype == torch.bfloat16 and self._erf_gelu() and not fused.recording(x, self.fc1.weight)

    def hidden(self, x):
        """act(fc1(x)) as a 2-D [tokens, hidden] tensor: bias + GELU in the projection's epilogue (one pass over the hidden
        activations less; in bf16 at least as close to float32 erf-GELU as the two-kernel form, tools/gelu_epilogue_check.py)."""
        x2 = x.reshape(-1, x.shape[-1])
        if self._gelu_epilogue(x):
            return linear(x2.contiguous(), self.fc1, gelu=True)
        return self.act(self.fc1(x2))

    def forward(self, x):
        if self._gelu_epilogue(x):
            return linear(self.hidden(x), self.fc2).view(*x.shape[:-1], -1)
        return self.fc2(self.act(self.fc1(x)))


class NATLayer(nn.Module):
    def __init__(self, dim, num_heads, kernel_size=7, dilation=None, mlp_ratio=4.0, qkv_bias=True, qk_scale=None,
                 drop=0.0, attn_drop=0.0, drop_path=0.0, act_layer=nn.GELU, norm_layer=nn.LayerNorm, layer_scale=None):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = NeighborhoodAttention2D(dim, kernel_size=kernel_size, dilation=dilation, num_heads=num_heads,
                                            qkv_bias=qkv_bias, qk_scale=qk_scale)
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(dim, int(dim * mlp_ratio), act_layer=act_layer)
        self.drop_path_rate = float(drop_path)                              # stochastic depth, training only (nat.py:122)
        self.layer_scale = layer_scale is not None and type(layer_scale) in (int, float)
        if self.layer_scale:
            self.gamma1 = nn.Parameter(layer_scale * torch.ones(dim))
            self.gamma2 = nn.Parameter(layer_scale * torch.ones(dim))

    folded = False        # set by NATBlock.fold(): LayerScale in the projection weights, biases carried as offsets
    _c = _c_dev = None

    def _forward_folded(self, s, y, next_norm, restore=False):
        """s: the residual stream minus the level's accumulated projection biases (see _fold_doc); y = norm1(s + c_in).
        restore (the level's last layer): the returned stream is the TRUE one, s + c_out — where the layer's own kernel can add the
        constant in its epilogue (the 128-channel streaming form) it does, and reports so by the third return value."""
        C = s.shape[-1]
        c_in, c_mid, c_out = self.offsets(s.device)
        if self._streams_c128(s):
            # 128-channel level: LN -> qkv and LN -> MLP -> residual are one token-streaming kernel each (weights in LDS)
            qkv = fused.nat128_ln_qkv(s, c_in, self.norm1, self.attn.qkv)
            fused.nat128_proj_add_(s, self.attn.attend(s, qkv=qkv), self.attn.proj)      # s += o W'^T (bias in c_mid)
            fused.nat128_ln_mlp_(s, c_mid, self.norm2, self.mlp.fc1, self.mlp.fc2, final_add=c_out if restore else None)
            off = None if restore else c_out
            return s, (fused.layer_norm(s, next_norm, offset=off) if next_norm is not None else None), restore
        if y is None:
            y = fused.layer_norm(s, self.norm1, offset=c_in)
        s2 = s.view(-1, C)
        accumulate(s2, self.attn.attend(y).view(-1, C), self.attn.proj)                # s += o W'^T  (bias in c_mid)
        y2 = fused.layer_norm(s, self.norm2, offset=c_mid)
        accumulate(s2, self.mlp.hidden(y2), self.mlp.fc2)                              # s += h W2'^T (bias in c_out)
        return s, (fused.layer_norm(s, next_norm, offset=c_out) if next_norm is not None else None), False

    _ln_packs = None

    def ln_packs(self):
        """What ppn_nat_gemm_bf16 reads for this (folded) layer, rebuilt when a parameter changes: the LayerNorms folded into the
        projections behind them — W' = W diag(gamma) (bfloat16), b' = b + W beta, colsum(W') of the bfloat16 values, float32 —
        for qkv and fc1, and proj / fc2 (LayerScale already folded by NATBlock.fold) with float32 biases:
        (wq, bq, csq, w1, b1, cs1, wp, bp, w2, b2)."""
        if self._ln_packs is None:
            self._ln_packs = fused.WeightCache()
        q, f1, pj, f2, n1, n2 = self.attn.qkv, self.mlp.fc1, self.attn.proj, self.mlp.fc2, self.norm1, self.norm2

        def build():
            out = []
            for lin, ln in ((q, n1), (f1, n2)):
                w32 = lin.weight.detach().float()
                wf = (w32 * ln.weight.detach().float()[None, :]).to(torch.bfloat16).contiguous()
                b = (lin.bias.detach().float() if lin.bias is not None else 0.0) + w32 @ ln.bias.detach().float()
                out += [wf, b.contiguous(), wf.float().sum(1).contiguous()]
            for lin in (pj, f2):
                out += [lin.weight.detach().contiguous(), lin.bias.detach().float().contiguous() if lin.bias is not None
                        else torch.zeros(lin.out_features, dtype=torch.float32, device=lin.weight.device)]
            return tuple(out)
        return self._ln_packs.get((q.weight, q.bias, f1.weight, f1.bias, pj.weight, pj.bias, f2.weight, f2.bias, n1.weight, n1.bias,
                                   n2.weight, n2.bias), build)

    _mlp_packs = None

    def mlp_packs(self):
        """What ppn_nat_mlp_bf16 reads for this (folded) layer's MLP: (packed weights, hb [hidden, 2] = (colsum, folded bias),
        b2) — built from ln_packs() on the device, rebuilt when a parameter changes."""
        if self._mlp_packs is None:
            self._mlp_packs = fused.WeightCache()
        f1, f2, n2 = self.mlp.fc1, self.mlp.fc2, self.norm2

        def build():
            _, _, _, w1, b1, cs1, _, _, w2, b2 = self.ln_packs()
            return fused.nat_mlp_pack(w1, w2), torch.stack([cs1, b1], dim=1).contiguous(), b2
        return self._mlp_packs.get((f1.weight, f1.bias, f2.weight, f2.bias, n2.weight, n2.bias), build)

    def _streams_c128(self, s):
        return (s.shape[-1] == 128 and s.is_cuda and s.dtype == torch.bfloat16 and (s.numel() // 128) % 16 == 0
                and self.mlp.fc1.out_features == 256 and isinstance(self.mlp.act, nn.GELU) and self.mlp.act.approximate == "none"
                and self.attn.qkv.weight.dtype == torch.bfloat16 and not os.environ.get("PPNET_LIBRARY_NAT128"))

    def offsets(self, device):
        """(c_in, c_mid, c_out) as float32 tensors on `device`: plain attributes, not buffers, so that module.to(bfloat16)
        does not round the accumulated biases."""
        if self._c_dev is None or self._c_dev[0].device != device:
            self._c_dev = tuple(t.to(device) for t in self._c)
        return self._c_dev

    def forward(self, x, y=None, next_norm=None, next_pad=None):
        """x: residual stream [B,H,W,C]; y = norm1(x) if the caller already has it. Returns (x', next_norm(x')).
        The attention's zero-padding to kernel*dilation is virtual (na.NeighborhoodAttention2D.forward), so next_pad
        stays None; the argument is kept for a caller that wants the materialised padded grid.
        Residual add, LayerScale and the following LayerNorm are one fused kernel each (DropPath is the identity
        at inference, nat.py:140-153)."""
        if self.folded:
            return self._forward_folded(x, y, next_norm)[:2]
        hw = (x.shape[1], x.shape[2])
        if y is None:
            y = fused.layer_norm(x, self.norm1)
        real = hw if (y.shape[1], y.shape[2]) != hw else None               # a materialised padded y still works
        # x + drop_path(gamma * f(.)): the mask commutes with gamma and rides into the residual kernel as a per-image scale
        a = self.attn(y, real)
        x, y2 = fused.residual_layer_norm(x, a, self.gamma1 if self.layer_scale else None, self.norm2, scale=self._drop_scale(a))
        a = self.mlp(y2)
        return fused.residual_layer_norm(x, a, self.gamma2 if self.layer_scale else None, next_norm, next_pad, scale=self._drop_scale(a))

    def _drop_scale(self, a):
        """Stochastic depth per sample (dense.drop_path's draw: the same call, shape, dtype and order, so a seeded run draws the same
        masks) as the float32 [B] factor mask / keep of fused.residual_layer_norm; None in eval mode or at rate 0."""
        if not self.training or self.drop_path_rate <= 0.0:
            return None
        keep = 1.0 - self.drop_path_rate
        mask = a.new_empty((a.shape[0],) + (1,) * (a.dim() - 1)).bernoulli_(keep)
        return (mask / keep).float().view(-1)


def _fold_doc():
    """Folded inference form of a NAT level (SegNet.prepare_inference on the GPU path).  LayerScale is folded into the two
    output projections (W' = diag(gamma) W, b' = gamma * b), so a sub-layer is x' = x + o W'^T + b'.  The residual stream
    is kept WITHOUT the constant part: s = x - c, where c is the sum of the b' seen so far in the level (known when the
    weights are).  Then s' = s + o W'^T is ONE library GEMM accumulating into s (beta = 1: `addmm_`), every LayerNorm is
    LN(s + c) with c added in registers (ppn_layernorm_offset), and the level's end adds c once for the downsampler.
    Per sub-layer the activations cross HBM 4 times (GEMM reads s, writes s'; LN reads s', writes y) instead of 5
    (GEMM writes a; the fused residual+LN kernel reads x and a, writes x' and y)."""


class NATBlock(nn.Module):
    def __init__(self, dim, depth, num_heads, kernel_size, dilations=None, downsample=True, mlp_ratio=4.0, qkv_bias=True,
                 qk_scale=None, drop=0.0, attn_drop=0.0, drop_path=0.0, norm_layer=nn.LayerNorm, layer_scale=None):
        super().__init__()
        self.blocks = nn.ModuleList(
            NATLayer(dim, num_heads, kernel_size, None if dilations is None else dilations[i], mlp_ratio, qkv_bias,
                     qk_scale, drop_path=drop_path[i] if isinstance(drop_path, (list, tuple)) else drop_path,
                     norm_layer=norm_layer, layer_scale=layer_scale) for i in range(depth))
        self.downsample = ConvDownsampler(dim, norm_layer) if downsample else None

    def forward(self, x, out_norm=None, inplace=False):
        """Returns (next level's input, out_norm(x) or x): the level's output norm rides on the last fused kernel.
        The fused kernels update the residual stream in place: inplace=True lets them use the caller's tensor (NAT hands
        over the tokenizer's / downsampler's fresh output), otherwise it is copied first."""
        if not inplace:
            x = x.clone()
        if self._ln_folded_ok(x):
            return self._forward_ln_folded(x, out_norm)
        y = None
        n = len(self.blocks)
        hw = (x.shape[1], x.shape[2])
        for i, blk in enumerate(self.blocks):
            if i + 1 < n:
                nxt = self.blocks[i + 1]
                x, y = blk(x, y, None if (nxt.folded and nxt._streams_c128(x)) else nxt.norm1, None)
            elif blk.folded:
                # x is s = x_true - c: the true stream is read itself by the downsampler (or returned when there is no output norm)
                want = self.downsample is not None or out_norm is None
                x, y, restored = blk._forward_folded(x, y, out_norm, restore=want)
                if want and not restored:
                    x = fused.bias_act_(x.permute(0, 3, 1, 2), blk.offsets(x.device)[2], 1.0).permute(0, 2, 3, 1)
            else:
                x, y = blk(x, y, out_norm, None)
        xo = y if out_norm is not None else x
        return (x, xo) if self.downsample is None else (self.downsample(x), xo)

    def _ln_folded_ok(self, x):
        """The level runs on ppn_nat_gemm_bf16 (csrc/mfma_gemm.h): folded bfloat16 inference, C and the MLP width multiples of
        256, whole 256-token tiles — and at least 64 of them in the narrowest projection (tokens x C): the persistent kernels walk
        256 x 256 tiles one per CU, and a batch of 1-16 problems has a handful (a level-2 projection at batch 1 is TWO tiles, each
        walking K alone: 34 us where the wave-per-block kernel of gemm_small.hip behind a LayerNorm launch takes 12).  The stream is
        at most 1024 wide (ppn_row_stats_bf16) with at most 4 row-statistic partials (ppn_nat_gemm_bf16): DiNAT-L's level 3
        (C = 1536, 6 partials) takes the per-layer folded path, LayerNorm kernel + accumulating library GEMM."""
        b0 = self.blocks[0]
        C = x.shape[-1]
        return (b0.folded and x.is_cuda and x.dtype == torch.bfloat16 and b0.attn.qkv.weight.dtype == torch.bfloat16 and C % 256 == 0
                and C <= 1024 and fused.nat_partials(C) <= 4
                and (x.numel() // C) % 256 == 0 and (x.numel() // C // 256) * (C // 256) >= int(os.environ.get("PPNET_SMALL_GEMM_TILES", "64")) and b0.mlp.fc1.out_features % 256 == 0 and b0.mlp._erf_gelu() and x.is_contiguous()
                and not torch.is_grad_enabled() and not library_width(C) and not os.environ.get("PPNET_NO_LN_FOLD"))

    def _forward_ln_folded(self, x, out_norm):
        """The level with the dense half of every layer on the build's own persistent GEMMs (reference SegNet/nat.py:140-153): per
        layer four launches and the attention —
            qkv = GEMM_ln(s)            LayerNorm folded into the projection: the GEMM reads the raw residual stream and the row
                                        sums the previous accumulating GEMM left behind
            a   = NA(qkv)
            s  += a Wp'^T + bp'         in place, residual add in the matrix pipe, row sums of the new s out
            h   = GEMM_ln_gelu(s)       LayerNorm folded in, erf-GELU in the epilogue
            s  += h W2'^T + b2'
        — no LayerNorm kernel, no separate residual / bias / activation pass, no vendor GEMM.  s is the TRUE residual stream (the
        biases are added in the epilogues), so the downsampler and the output norm read it as it is."""
        B, H, W, C = x.shape
        M = B * H * W
        s2 = x.view(M, C)
        st = fused.row_stats(s2)                                            # the level's first stream came from a LayerNorm kernel
        P = fused.nat_partials(C)
        st_mid = torch.empty(P, M, 2, dtype=torch.float32, device=x.device)
        st_out = torch.empty(P, M, 2, dtype=torch.float32, device=x.device)
        fused_mlp = (P == C // 128 and fused.nat_mlp_ok(M, C, self.blocks[0].mlp.fc1.out_features) and not os.environ.get("PPNET_NO_FUSED_MLP"))
        for blk in self.blocks:
            wq, bq, csq, w1, b1, cs1, wp, bp, w2, b2 = blk.ln_packs()
            qkv = torch.empty(B, H, W, 3 * C, dtype=x.dtype, device=x.device)
            fused.nat_gemm(s2, wq, bq, "ln", qkv.view(M, 3 * C), colsum=csq, stats_in=st, eps=blk.norm1.eps)
            a = blk.attn.attend(x, qkv=qkv)
            fused.nat_gemm(a.view(M, C), wp, bp, "acc", s2, stats_out=st_mid)
            if fused_mlp:
                # LN -> fc1 -> GELU -> fc2 -> residual as ONE kernel: the hidden activation never reaches HBM (csrc/nat_mlp.hip)
                wpk, hb, b2v = blk.mlp_packs()
                fused.nat_mlp_(s2, wpk, hb, b2v, w1.shape[0], stats_out=st_out, eps=blk.norm2.eps)
            else:
                h = torch.empty(M, w1.shape[0], dtype=x.dtype, device=x.device)
                fused.nat_gemm(s2, w1, b1, "ln_gelu", h, colsum=cs1, stats_in=st_mid, eps=blk.norm2.eps)
                fused.nat_gemm(h, w2, b2, "acc", s2, stats_out=st_out)
            st = st_out
        xo = fused.layer_norm(x, out_norm) if out_norm is not None else x
        return (x, xo) if self.downsample is None else (self.downsample(x), xo)

    def fold(self):
        """See _fold_doc.  After the checkpoint is loaded; float32 algebra, then back to the parameters' dtype."""
        c = None
        for blk in self.blocks:
            g1 = blk.gamma1.detach().float() if blk.layer_scale else None
            g2 = blk.gamma2.detach().float() if blk.layer_scale else None
            for lin, g in ((blk.attn.proj, g1), (blk.mlp.fc2, g2)):
                if g is not None:
                    lin.weight = nn.Parameter((lin.weight.detach().float() * g[:, None]).to(lin.weight.dtype))
                    lin.bias = nn.Parameter((lin.bias.detach().float() * g).to(lin.bias.dtype))
            dim = blk.attn.proj.bias.shape[0]
            zero = torch.zeros(dim, dtype=torch.float32, device=blk.attn.proj.bias.device)
            c_in = c if c is not None else zero
            c_mid = c_in + blk.attn.proj.bias.detach().float()
            c_out = c_mid + blk.mlp.fc2.bias.detach().float()
            blk._c, blk._c_dev = (c_in.clone().contiguous(), c_mid.clone().contiguous(), c_out.clone().contiguous()), None
            if blk.layer_scale:
                blk.gamma1 = nn.Parameter(torch.ones_like(blk.gamma1)); blk.gamma2 = nn.Parameter(torch.ones_like(blk.gamma2))
            blk.folded = True
            c = c_out
        return self


class NAT(nn.Module):
    def __init__(self, embed_dim, mlp_ratio, depths, num_heads, drop_path_rate=0.2, in_chans=3, kernel_size=7,
                 dilations=None, out_indices=(0, 1, 2, 3), qkv_bias=True, qk_scale=None, drop_rate=0.0,
                 attn_drop_rate=0.0, norm_layer=nn.LayerNorm, frozen_stages=-1, pretrained=None, layer_scale=None,
                 **kwargs):
        super().__init__()
        self.num_levels = len(depths)
        self.embed_dim = embed_dim
        self.num_features = [int(embed_dim * 2 ** i) for i in range(self.num_levels)]
        self.patch_embed = ConvTokenizer(in_chans, embed_dim, norm_layer)
        dpr = [float(v) for v in torch.linspace(0, drop_path_rate, sum(depths), device="cpu")]      # nat.py:247 (values: never on meta)
        self.levels = nn.ModuleList(
            NATBlock(int(embed_dim * 2 ** i), depths[i], num_heads[i], kernel_size,
                     None if dilations is None else dilations[i], downsample=(i < self.num_levels - 1),
                     mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale,
                     drop_path=dpr[sum(depths[:i]):sum(depths[:i + 1])], norm_layer=norm_layer,
                     layer_scale=layer_scale) for i in range(self.num_levels))
        self.out_indices = tuple(out_indices)
        self.compute_indices = tuple(out_indices)      # inference may narrow this to the levels the head reads
        for i in out_indices:
            self.add_module(f"norm{i}", norm_layer(self.num_features[i]))
        if isinstance(pretrained, str):
            self.init_weights(pretrained)

    def init_weights(self, pretrained=None):
        if isinstance(pretrained, str):
            sd = torch.load(pretrained, map_location="cpu", weights_only=True)
            sd = sd.get("state_dict", sd.get("model", sd))
            self.load_state_dict(sd, strict=False)

    def forward(self, x):
        """x: the image [B,3,H,W], or (GPU inference) the u8 occupancy codes [B,H,W] it would be rendered from."""
        x = self.patch_embed.forward_codes(x) if x.dtype == torch.uint8 else self.patch_embed(x)
        outs = [None] * len(self.out_indices)          # one slot per out_index (nat.py:326-332); levels nobody reads stay None
        for idx, level in enumerate(self.levels):
            want = idx in self.compute_indices
            x, xo = level(x, getattr(self, f"norm{idx}") if want else None, inplace=True)   # x: fresh LayerNorm output
            if want:
                outs[self.out_indices.index(idx)] = xo.permute(0, 3, 1, 2)    # [B,C,H,W] in channels_last memory format (zero-copy view)
        return outs


class DiNAT(NAT):
    """DiNAT is NAT with per-layer dilations (dinat.py:15-22)."""
