"""DiNAT_s backbone (reference SegNet/dinats.py:21-341: "our alternative model" of the DiNAT paper — Swin's layout, a 4x4 / stride-4
patch embed and 2x2 patch merging, around dilated neighbourhood-attention layers) as plain nn.Modules with the reference's constructor
arguments and checkpoint key names (`patch_embed.{proj,norm}`, `layers.i.blocks.j.{norm1,attn.{qkv,rpb,proj},norm2,mlp.{fc1,fc2}}`,
`layers.i.downsample.{reduction.weight,norm}`, `norm{i}`).

NATransformerLayer (dinats.py:21-71) is nat.NATLayer without LayerScale: the neighbourhood-attention kernels, the residual + LayerNorm
pair, the folded inference forms and the GEMM core are nat.py's.  The patch embed is swin.PatchEmbed's arithmetic under the reference's
key names.  PatchMerging's gather + LayerNorm is one HIP kernel pair (fused.patch_merge_ln: ppn_patch_merge_ln_fwd /
ppn_patch_merge_ln_bwd) in front of the reduction GEMM."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import dense, fused, na, nat, swin  # noqa: F401  (na, swin: what nat's layers and the patch embed stand on)


class PatchEmbed(nn.Module):
    """dinats.py:172-202: pad right / bottom to a multiple of the patch, Conv2d(kernel = stride = patch), optional LayerNorm — what
    swin.PatchEmbed computes, with the reference's keys `proj.*`, `norm.*`."""

    def __init__(self, patch_size=4, in_chans=3, embed_dim=96, norm_layer=None):
        super().__init__()
        self.patch_size = (patch_size, patch_size) if isinstance(patch_size, int) else tuple(patch_size)
        self.in_chans, self.embed_dim = in_chans, embed_dim
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=self.patch_size, stride=self.patch_size)
        self.norm = None if norm_layer is None else norm_layer(embed_dim)

    def takes_codes(self, grid_u8):
        return False                                   # SegNet.labels_u8 renders occupancy codes to an image first

    def forward(self, x):
        """x [B,3,H,W], or the u8 occupancy codes [B,H,W] it would be rendered from -> tokens [B,ceil(H/p),ceil(W/p),C] (NHWC)."""
        if x.dtype == torch.uint8:
            x = fused.grid_to_image(x, dense.IMG_MEAN, dense.IMG_STD, self.proj.weight.dtype)
        H, W = x.shape[-2:]
        ph, pw = (-H) % self.patch_size[0], (-W) % self.patch_size[1]
        if ph or pw:
            x = F.pad(x, [0, pw, 0, ph])
        x = self.proj(x).permute(0, 2, 3, 1)
        if self.norm is None:
            return x
        return fused.layer_norm(x, self.norm) if dense.gpu_inference(x) else self.norm(x)


class PatchMerging(nn.Module):
    """dinats.py:74-104: zero-pad to even sizes, gather the 2x2 block as x0 (even row, even col) | x1 (odd, even) | x2 (even, odd) |
    x3 (odd, odd), LayerNorm(4C), Linear(4C, 2C, bias=False).  Swin's PatchMerging orders the 4C channels differently
    (c * 4 + kh * 2 + kw) and is a different module.  Returns the token GRID [B,ceil(H/2),ceil(W/2),2C] (the next level's attention
    needs it; the reference flattens it to [B,L,2C])."""

    def __init__(self, dim, norm_layer=nn.LayerNorm):
        super().__init__()
        self.dim = dim
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = norm_layer(4 * dim)

    def forward(self, x):
        y = fused.patch_merge_ln(x, self.norm)
        return dense.linear(y.reshape(-1, y.shape[-1]), self.reduction).view(*y.shape[:-1], -1)


class BasicLayer(nat.NATBlock):
    """dinats.py:107-169: `depth` NATransformerLayers (nat.NATLayer with layer_scale=None), then the PatchMerging.  Children `blocks`
    and `downsample`, as in the reference.  forward is NATBlock's: (next level's input, out_norm(x) or x)."""

    def __init__(self, dim, depth, num_heads, kernel_size, dilations=None, mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop=0.0,
                 attn_drop=0.0, drop_path=0.0, norm_layer=nn.LayerNorm, downsample=None):
        super().__init__(dim, depth, num_heads, kernel_size, dilations, downsample=False, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias,
                         qk_scale=qk_scale, drop=drop, attn_drop=attn_drop, drop_path=drop_path, norm_layer=norm_layer, layer_scale=None)
        self.dim, self.depth = dim, depth
        self.downsample = downsample(dim=dim, norm_layer=norm_layer) if downsample is not None else None


class DiNAT_s(nn.Module):
    """dinats.py:205-341 with the reference's constructor arguments and defaults.  forward(x [B,3,H,W] or u8 occupancy codes [B,H,W])
    -> one [B,C,H,W] view (channels_last memory) per out_index; levels outside compute_indices stay None (SegNet narrows them to what
    its heads read)."""

    def __init__(self, pretrain_img_size=224, patch_size=4, in_chans=3, embed_dim=96, depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24),
                 kernel_size=7, dilations=None, mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0,
                 drop_path_rate=0.2, norm_layer=nn.LayerNorm, patch_norm=True, out_indices=(0, 1, 2, 3), pretrained=None, frozen_stages=-1):
        super().__init__()
        if frozen_stages is not None and frozen_stages >= 0:
            raise NotImplementedError("frozen_stages >= 0 is not supported")
        if drop_rate or attn_drop_rate:
            raise NotImplementedError("drop_rate / attn_drop_rate: every SegNet configuration sets 0")
        self.pretrain_img_size = pretrain_img_size
        self.num_layers = len(depths)
        self.embed_dim = embed_dim
        self.patch_norm = patch_norm
        self.frozen_stages = frozen_stages
        self.patch_embed = PatchEmbed(patch_size, in_chans, embed_dim, norm_layer if patch_norm else None)
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = [float(v) for v in torch.linspace(0, drop_path_rate, sum(depths))]      # dinats.py:249-251
        self.layers = nn.ModuleList(
            BasicLayer(int(embed_dim * 2 ** i), depths[i], num_heads[i], kernel_size, None if dilations is None else dilations[i],
                       mlp_ratio, qkv_bias, qk_scale, drop_rate, attn_drop_rate, dpr[sum(depths[:i]):sum(depths[:i + 1])], norm_layer,
                       PatchMerging if i < self.num_layers - 1 else None) for i in range(self.num_layers))
        self.num_features = [int(embed_dim * 2 ** i) for i in range(self.num_layers)]
        self.out_indices = tuple(out_indices)
        self.compute_indices = tuple(out_indices)      # inference may narrow this to the levels the head reads
        for i in self.out_indices:
            self.add_module(f"norm{i}", norm_layer(self.num_features[i]))
        if pretrained is not None:
            self.init_weights(pretrained)

    @property
    def levels(self):
        return self.layers                             # SegNet.prepare_inference folds every level

    def init_weights(self, pretrained=None):
        """dinats.py:303-317: a checkpoint path ({'state_dict' | 'model' | plain}, optional 'backbone.' prefix), not strict; or None."""
        if isinstance(pretrained, str):
            sd = torch.load(pretrained, map_location="cpu", weights_only=True)
            sd = sd.get("state_dict", sd.get("model", sd))
            sd = {(k[9:] if k.startswith("backbone.") else k): v for k, v in sd.items()}
            self.load_state_dict(sd, strict=False)
        elif pretrained is not None:
            raise TypeError("pretrained must be a str or None")

    def forward(self, x):
        x = self.pos_drop(self.patch_embed(x))
        outs = [None] * len(self.out_indices)          # one slot per out_index (dinats.py:324-336); levels nobody reads stay None
        for idx, layer in enumerate(self.layers):
            want = idx in self.compute_indices
            # x is this level's own tensor (the patch embed's or the reduction's fresh output) unless autograd holds it
            x, xo = layer(x, getattr(self, f"norm{idx}") if want else None, inplace=not x.requires_grad)
            if want:
                outs[self.out_indices.index(idx)] = xo.permute(0, 3, 1, 2)    # [B,C,H,W] in channels_last memory format (zero-copy view)
            if all(j <= idx for j in self.compute_indices) and idx + 1 < len(self.layers):
                break                                  # no level past this one is read
        return outs
