"""SegNet's decode heads (reference SegNet/mmseg/decode_heads: setr_up_head.py:28-81, uper_head.py:12-127 + psp_head.py:10-60,
uper_pup_head.py:12-131, fcn_head.py:11-81 over decode_head.py) as plain nn.Modules with mmseg's constructor arguments and
checkpoint key names (`norm`, `up_convs.i.0.{conv,bn}`, `psp_modules.i.1.{conv,bn}`, `bottleneck`, `lateral_convs.i`, `fpn_convs.i`,
`fpn_bottleneck`, `convs.i`, `conv_cat`, `conv_seg`), and BaseDecodeHead's losses.  Unprepared they are the reference's op chains
through PyTorch; prepared bfloat16 inference on the GPU takes the build's own kernels (`_forward_mfma`) where dense.py lets it."""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import fused
from .dense import mfma_weights, use_mfma_conv


class _BatchNorm2d(nn.BatchNorm2d):
    """nn.BatchNorm2d that takes its input in the dtype of its own parameters.  Under autocast the convolution in front hands it
    bfloat16 activations while weight and running statistics stay float32; the statistics are float32 either way, and the cast
    keeps the layer on the float32 channels_last path that float32 training takes (the mixed bfloat16 / float32 channels_last
    form had never been run in this project: SETR-UP's training step under bfloat16 autocast ended in a segmentation fault inside
    torch.batch_norm).  Same parameters, buffers and state-dict keys."""

    def forward(self, x):
        if self.weight is not None and x.dtype != self.weight.dtype:
            x = x.to(self.weight.dtype)
        return super().forward(x)


class _ConvModule(nn.Sequential):
    """mmcv ConvModule(conv -> bn -> ReLU) with its parameter names `conv.*`, `bn.*` (conv has no bias under a norm)."""

    def __init__(self, cin, cout, k, dilation=1):
        super().__init__()
        self.add_module("conv", nn.Conv2d(cin, cout, k, 1, ((k - 1) // 2) * dilation, dilation, bias=False))
        self.add_module("bn", _BatchNorm2d(cout))            # SyncBN reverts to BN outside distributed runs (SegNet/train.py:179-185)
        self.add_module("activate", nn.ReLU(inplace=True))


class _Upsample(nn.Module):
    def __init__(self, scale_factor, align_corners=False):
        super().__init__()
        self.scale_factor, self.align_corners = float(scale_factor), align_corners

    def forward(self, x, relu=False, bias=None):
        if self.scale_factor == 2.0 and not self.align_corners and x.shape[1] % 8 == 0 and x.is_cuda:
            return fused.upsample2x_nhwc(x, relu, bias)                      # HIP kernel, bias + ReLU folded into the loads
        if bias is not None:
            x = x + bias.view(1, -1, 1, 1)
        if relu:
            x = F.relu(x)
        size = [int(t * self.scale_factor) for t in x.shape[-2:]]            # mmseg/ops/wrappers.py:43-51
        return F.interpolate(x, size, None, "bilinear", self.align_corners)


def _seg_pack(conv_seg):
    """The 1x1 classifier as the classify kernels read it: (weight [classes, channels], bias), both float32."""
    return conv_seg.weight.detach().float().reshape(conv_seg.out_channels, -1).contiguous(), conv_seg.bias.detach().float().contiguous()


def _in_equal_slices(feats, bmax, run):
    """run(feats) for a list of batched tensors (None entries stay None) with at most bmax images per call: a batch within bmax
    goes through as it is, a larger one in equal slices whose results are concatenated (torch.cat is reached only then)."""
    B = next(t for t in feats if t is not None).shape[0]
    if B <= bmax:
        return run(feats)
    step = -(-B // (-(-B // bmax)))                                       # equal slices
    return torch.cat([run([t[i:i + step] if t is not None else None for t in feats]) for i in range(0, B, step)], dim=0)


class OHEMPixelSampler:
    """mmseg's online hard example mining sampler (core/seg/sampler/ohem_pixel_sampler.py:11-30): `thresh` — pixels whose label
    probability is below it are hard; None: the min_kept largest losses — and `min_kept`, the pixels kept at least, PER IMAGE (the
    sampler multiplies by the batch size).  It only holds the two numbers: ohem_weight is its sample(), and on the GPU
    resized_decode_losses hands them to the fused kernels (fused.ohem_cross_entropy)."""

    def __init__(self, context=None, thresh=None, min_kept=100000):
        assert min_kept > 1
        self.context, self.thresh, self.min_kept = context, thresh, min_kept

    def __repr__(self):
        return f"OHEMPixelSampler(thresh={self.thresh}, min_kept={self.min_kept})"


def _loss_options(sampler, loss_decode, num_classes):
    """(sampler, class_weight) of a head from the reference's config entries `sampler=dict(type='OHEMPixelSampler', thresh=...,
    min_kept=...)` (decode_head.py:96-99) and `loss_decode=dict(type='CrossEntropyLoss', class_weight=[...])`
    (losses/cross_entropy_loss.py:158-171): an OHEMPixelSampler or None, and a tuple of num_classes floats or None.  Both are kept as
    plain attributes of the head — no buffer, so no checkpoint key.  Another sampler type, or class weights given as a file path
    (losses/utils.py:9-24), raise NotImplementedError."""
    if isinstance(sampler, dict):
        cfg = dict(sampler)
        typ = cfg.pop("type", None)
        if typ != "OHEMPixelSampler":
            raise NotImplementedError(f"pixel sampler type {typ!r}: OHEMPixelSampler only")
        sampler = OHEMPixelSampler(**cfg)
    elif sampler is not None and not isinstance(sampler, OHEMPixelSampler):
        raise NotImplementedError(f"pixel sampler {sampler!r}: a dict(type='OHEMPixelSampler', ...) or an OHEMPixelSampler")
    if isinstance(loss_decode, (list, tuple)):                               # a list: the first cross-entropy entry's
        loss_decode = next((d for d in loss_decode if isinstance(d, dict) and d.get("type", _CE) == _CE), None)
    elif isinstance(loss_decode, dict) and loss_decode.get("type", _CE) != _CE:
        loss_decode = None                                                   # a single loss of another type: its weights are its own
    return sampler, _class_weight_entry(loss_decode.get("class_weight") if isinstance(loss_decode, dict) else None, num_classes)


_CE, _DICE = "CrossEntropyLoss", "DiceLoss"


def _class_weight_entry(cw, num_classes):
    """A loss's `class_weight` entry as a tuple of num_classes floats, or None; a file path (losses/utils.py:9-24) raises."""
    if cw is None:
        return None
    if isinstance(cw, str):
        raise NotImplementedError(f"class_weight {cw!r}: a list of {num_classes} floats (files are not read)")
    cw = tuple(float(v) for v in cw)
    if len(cw) != num_classes:
        raise ValueError(f"class_weight has {len(cw)} entries for {num_classes} classes")
    return cw


def _single_ce(loss_decode):
    """Whether loss_decode is the form every config had before loss lists: None, or ONE dict of type CrossEntropyLoss (or none)."""
    return loss_decode is None or (isinstance(loss_decode, dict) and loss_decode.get("type", _CE) == _CE)


def _loss_specs(loss_decode, num_classes):
    """A head's `loss_decode` (decode_head.py:36-43,87-95: a dict or a sequence of dicts; None is the default CrossEntropyLoss) as a
    tuple of specs, one dict per loss: `type` ('CrossEntropyLoss' | 'DiceLoss'), `loss_name` (default 'loss_ce' / 'loss_dice'; equal
    names are summed, decode_head.py:246-262), `loss_weight`, `class_weight` (a tuple of num_classes floats or None) and, for DiceLoss
    (losses/dice_loss.py:74-90), `smooth`, `exponent` and its own `ignore_index` (default 255).  Raised, never dropped silently
    (NotImplementedError): another type (LovaszLoss needs a per-class device sort, FocalLoss the sigmoid form of an mmcv op),
    class_weight as a file path, a reduction other than 'mean', and use_sigmoid=True (sigmoid / binary cross-entropy) inside a list or
    on a DiceLoss.  A SINGLE CrossEntropyLoss dict is read as it always was: class_weight, and loss_weight by the auxiliary head
    (FCNHead.loss_weight) — its other keys stay unread (resized_head_losses takes the head's weight for it, not the spec's)."""
    if loss_decode is None:
        entries = [{}]
    elif isinstance(loss_decode, dict):
        entries = [loss_decode]
    elif isinstance(loss_decode, (list, tuple)) and len(loss_decode) > 0 and all(isinstance(d, dict) for d in loss_decode):
        entries = list(loss_decode)
    else:
        raise TypeError(f"loss_decode must be a dict or a non-empty sequence of dicts, got {loss_decode!r}")
    single = _single_ce(loss_decode)
    specs = []
    for d in entries:
        typ = d.get("type", _CE)
        if typ not in (_CE, _DICE):
            raise NotImplementedError(f"loss type {typ!r}: CrossEntropyLoss and DiceLoss only (LovaszLoss, FocalLoss and the rest are not built)")
        if not single:
            if d.get("use_sigmoid", False):
                raise NotImplementedError(f"{typ}(use_sigmoid=True): sigmoid / binary cross-entropy is not built")
            if d.get("reduction", "mean") != "mean":
                raise NotImplementedError(f"{typ}(reduction={d['reduction']!r}): 'mean' only")
        spec = dict(type=typ, loss_name=str(d.get("loss_name", "loss_ce" if typ == _CE else "loss_dice")),
                    loss_weight=float(d.get("loss_weight", 1.0)), class_weight=_class_weight_entry(d.get("class_weight"), num_classes))
        if typ == _DICE:
            ignore = d.get("ignore_index", 255)
            spec.update(smooth=float(d.get("smooth", 1)), exponent=d.get("exponent", 2), ignore_index=-1 if ignore is None else int(ignore))
            if not spec["smooth"] >= 0.0:
                raise ValueError(f"DiceLoss(smooth={d.get('smooth')!r}): not negative")
        specs.append(spec)
    return tuple(specs)


class SETRUPHead(nn.Module):
    def __init__(self, in_channels=1024, channels=512, num_classes=2, num_convs=1, up_scale=4, kernel_size=3,
                 in_index=-1, dropout_ratio=0.1, align_corners=False, norm_layer=None, norm_cfg=None, sampler=None, loss_decode=None,
                 **kwargs):
        super().__init__()
        assert kernel_size in (1, 3)
        self.in_index, self.align_corners = in_index, align_corners
        self.sampler, self.class_weight = _loss_options(sampler, loss_decode, num_classes)
        self.loss_specs, self.loss_single_ce = _loss_specs(loss_decode, num_classes), _single_ce(loss_decode)
        self.norm = nn.LayerNorm(in_channels, eps=1e-6)
        self.up_convs = nn.ModuleList()
        cin = in_channels
        for _ in range(num_convs):
            self.up_convs.append(nn.Sequential(_ConvModule(cin, channels, kernel_size), _Upsample(up_scale, align_corners)))
            cin = channels
        self.conv_seg = nn.Conv2d(channels, num_classes, 1)
        self.dropout = nn.Dropout2d(dropout_ratio) if dropout_ratio > 0 else nn.Identity()   # decode_head.py cls_seg; identity in eval

    def forward(self, inputs, lowres=False):
        """lowres=True: the classifier's logits BEFORE the last x2 up-sampling (the caller fuses the rest of the tail)."""
        x = inputs[self.in_index]
        # LayerNorm over channels (setr_up_head.py:73-76) on the NHWC view; stays channels_last for the convolutions
        # (768-wide rows, ViT-B's, take the framework's LayerNorm: fused.layer_norm_any_width)
        x = fused.layer_norm_any_width(x.permute(0, 2, 3, 1), self.norm).permute(0, 3, 1, 2)
        prepared = all(isinstance(up[0].bn, nn.Identity) and up[0].conv.bias is not None for up in self.up_convs)
        if prepared and all(use_mfma_conv(x, up[0].conv) for up in self.up_convs) and self.conv_seg.out_channels == 2:
            return self._forward_mfma(x, lowres)
        for up in self.up_convs[:-1]:
            cm = up[0]
            if isinstance(cm.bn, nn.Identity) and cm.conv.bias is not None:  # prepared: the folded-BN bias rides in the upsample kernel
                c = cm.conv
                x = up[1](F.conv2d(x, c.weight, None, c.stride, c.padding), relu=True, bias=c.bias)
            else:
                x = up[1](cm.bn(cm.conv(x)), relu=True)                      # conv -> BN -> ReLU + x2 bilinear in one kernel
        # last stage: conv_seg is a 1x1 convolution and bilinear interpolation is linear with weights summing to 1,
        # so conv_seg(upsample(y)) == upsample(conv_seg(y)): classify at the low resolution and upsample 2 channels
        # instead of `channels` (the reference materialises a [B,512,R/2,R/2] tensor here, setr_up_head.py:78-80)
        conv, up = self.up_convs[-1][0], self.up_convs[-1][1]
        if isinstance(conv.bn, nn.Identity) and conv.conv.bias is not None and x.is_cuda:
            c = conv.conv                                                     # prepared: bias + ReLU in one in-place HIP pass
            y = fused.bias_act_(F.conv2d(x, c.weight, None, c.stride, c.padding).contiguous(memory_format=torch.channels_last), c.bias, 0.0)
        else:
            y = conv(x)
        if self.training:
            # the reference's order (setr_up_head.py:78-80, decode_head.py:232-237): up-sample, channel dropout, classify —
            # the dropout mask does not commute with the interpolation
            return self.conv_seg(self.dropout(up(y)))
        lo = self.conv_seg(y).contiguous()
        return lo if lowres else up(lo)                                      # 2 channels: the library bilinear kernel

    _mfma = None

    def _forward_mfma(self, x, lowres):
        """Prepared bfloat16 inference on the hand-written MFMA kernels: every ConvModule is one implicit-GEMM launch with the
        folded-BatchNorm bias and the ReLU in its epilogue, and the last one also applies the 1x1 classifier (commuted in front
        of the last up-sampling, as in forward()) so the 512-channel activation at the highest resolution is never written."""
        if self._mfma is None:
            self._mfma = fused.WeightCache()
        cs = self.conv_seg
        src = [t for up in self.up_convs for t in (up[0].conv.weight, up[0].conv.bias)] + [cs.weight, cs.bias]
        packs = self._mfma.get(src, lambda: [mfma_weights(up[0].conv) for up in self.up_convs] + [_seg_pack(cs)])
        n = len(self.up_convs) - 1

        def run(feats):
            x, = feats
            for i, up in enumerate(self.up_convs[:-1]):
                x = up[1](fused.conv3x3_mfma(x, packs[i][0], packs[i][1], stride=1, relu=True))
            lo = fused.conv3x3_relu_classify2(x, *packs[n], *packs[-1]).to(x.dtype).contiguous()
            return lo if lowres else self.up_convs[-1][1](lo)
        # The convolution kernels address their input with 32-bit byte offsets: the last stage reads [B, channels, H 2^n, W 2^n]
        # bfloat16, which passes 4 GiB at batch 256 of 512 x 512 maps.  Larger batches go through the head in slices.
        last_in = self.up_convs[-1][0].conv.in_channels * x.shape[-2] * x.shape[-1] * 4 ** n * 2
        return _in_equal_slices([x], max(1, (2 ** 32 - 1) // last_in), run)


class UPerHead(nn.Module):
    """UPerNet head (SegNet/mmseg/decode_heads/uper_head.py:12-127 + psp_head.py:10-60): pyramid pooling on the last level,
    lateral 1x1 convs, top-down bilinear fusion, 3x3 FPN convs, concatenation, 3x3 bottleneck, 1x1 classifier.  Checkpoint
    keys follow mmseg: `psp_modules.i.1.{conv,bn}`, `bottleneck.{conv,bn}`, `lateral_convs.i.{conv,bn}`,
    `fpn_convs.i.{conv,bn}`, `fpn_bottleneck.{conv,bn}`, `conv_seg`.  The head of the reference's default SegNet config
    (SegNet/test.py:29-32 -> configs/nat/upernet_nat_base.py)."""

    def __init__(self, in_channels=(128, 256, 512, 1024), channels=64, num_classes=2, pool_scales=(1, 2, 3, 6),
                 in_index=(0, 1, 2, 3), dropout_ratio=0.1, align_corners=False, norm_cfg=None, sampler=None, loss_decode=None, **kwargs):
        super().__init__()
        self.in_index, self.align_corners = tuple(in_index), align_corners
        self.sampler, self.class_weight = _loss_options(sampler, loss_decode, num_classes)
        self.loss_specs, self.loss_single_ce = _loss_specs(loss_decode, num_classes), _single_ce(loss_decode)
        self.psp_modules = nn.ModuleList(
            nn.Sequential(nn.AdaptiveAvgPool2d(ps), _ConvModule(in_channels[-1], channels, 1)) for ps in pool_scales)
        self.bottleneck = _ConvModule(in_channels[-1] + len(pool_scales) * channels, channels, 3)
        self.lateral_convs = nn.ModuleList(_ConvModule(c, channels, 1) for c in in_channels[:-1])
        self.fpn_convs = nn.ModuleList(_ConvModule(channels, channels, 3) for _ in in_channels[:-1])
        self.fpn_bottleneck = _ConvModule(len(in_channels) * channels, channels, 3)
        self.conv_seg = nn.Conv2d(channels, num_classes, 1)                  # Dropout2d is the identity at inference

    def _resize(self, x, size):
        if (x.is_cuda and not self.align_corners and tuple(size) == (2 * x.shape[2], 2 * x.shape[3]) and x.shape[1] % 8 == 0
                and x.dtype in (torch.float32, torch.bfloat16) and not (fused.library_upsample() and fused.recording(x))):
            return fused.upsample2x_nhwc(x)                                  # the FPN's x2 steps: the build's NHWC kernel (it records its own backward)
        return F.interpolate(x, size=size, mode="bilinear", align_corners=self.align_corners)

    _packs = None

    def _prepared_mfma(self, x):
        """Prepared bfloat16 inference on the build's own kernels: BatchNorm folded into every ConvModule (a bias on its conv)."""
        cms = [m for m in self.modules() if isinstance(m, _ConvModule)]
        return (x.is_cuda and x.dtype == torch.bfloat16 and not self.training and all(isinstance(c.bn, nn.Identity) and c.conv.bias is not None for c in cms)
                and self.conv_seg.out_channels == 2 and not fused.recording(x, self.conv_seg.weight) and not os.environ.get("PPNET_LIBRARY_CONV"))

    def _conv_modules(self):
        return [m[1] for m in self.psp_modules] + [self.bottleneck] + list(self.lateral_convs) + list(self.fpn_convs) + [self.fpn_bottleneck]

    def _mfma_packs(self):
        """Every ConvModule's folded weight and bias in the layout its kernel reads (1x1: [Cout, Cin]; 3x3: mfma_weights) and the
        classifier's as float32 (key "seg"), keyed by module; rebuilt when a parameter changes."""
        if self._packs is None:
            self._packs = fused.WeightCache()
        cms = self._conv_modules()
        src = [t for c in cms for t in (c.conv.weight, c.conv.bias)] + [self.conv_seg.weight, self.conv_seg.bias]

        def build():
            pk = {}
            for c in cms:
                cv = c.conv
                if cv.kernel_size == (1, 1):
                    pk[c] = (cv.weight.detach().reshape(cv.out_channels, cv.in_channels).contiguous(), cv.bias.detach().float().contiguous())
                else:
                    pk[c] = mfma_weights(cv)
            pk["seg"] = _seg_pack(self.conv_seg)
            return pk
        return self._packs.get(src, build)

    @staticmethod
    def _mfma_conv1(pk, cm, t):
        """1x1 ConvModule on a channels_last [B,C,H,W] tensor."""
        Bn, Cc, Hh, Ww = t.shape
        tok = t.permute(0, 2, 3, 1).reshape(-1, Cc)
        w, b = pk[cm]
        if tok.shape[0] >= 256 and Cc % 64 == 0 and Cc >= 128 and tok.is_contiguous():
            y = fused.gemm_bf16(tok, w, b, "bias_relu")
        else:                                                                # the pyramid's 1 .. 36 pooled positions per image: too few rows for a tile
            y = F.relu(F.linear(tok, w, b.to(tok.dtype)))
        return y.view(Bn, Hh, Ww, -1).permute(0, 3, 1, 2)

    @staticmethod
    def _mfma_conv3(pk, cm, t, relu=True):
        w, b = pk[cm]
        if use_mfma_conv(t, cm.conv, narrow=True):
            return fused.conv3x3_mfma(t, w, b, stride=1, relu=relu)
        y = F.conv2d(t, cm.conv.weight, cm.conv.bias, 1, 1)
        return F.relu(y) if relu else y

    def _own_resize(self):
        return not self.align_corners and self.conv_seg.in_channels % 8 == 0 and not os.environ.get("PPNET_UPER_UNFUSED_RESIZE")

    def _mfma_top_down(self, inputs, pk, own_resize):
        """uper_head.py:76-108 on the build's kernels: the pyramid pooling module + bottleneck, the laterals and the top-down sums.
        Returns the laterals, finest first, the last one the bottleneck's output."""
        conv1, conv3 = self._mfma_conv1, self._mfma_conv3
        inputs = [inputs[i] for i in self.in_index]
        x = inputs[-1]
        scales = [m[0].output_size if isinstance(m[0].output_size, int) else m[0].output_size[0] for m in self.psp_modules]
        if own_resize and len(scales) <= 4 and x.shape[1] % 8 == 0:
            # the pyramid pooling module (psp_head.py:48-60) as 6 launches: every pool in one kernel, a 1x1 ConvModule each on the
            # GEMM kernel (B s^2 rows), the resizes back + the concatenation with x in one kernel
            pooled = fused.adaptive_pools(x, scales)
            psp = fused.resize_concat([x] + [conv1(pk, m[1], t) for m, t in zip(self.psp_modules, pooled)])
        else:
            psp = torch.cat([x] + [self._resize(conv1(pk, m[1], m[0](x)), x.shape[2:]) for m in self.psp_modules], dim=1).contiguous(memory_format=torch.channels_last)
        laterals = [conv1(pk, cm, inputs[i]) for i, cm in enumerate(self.lateral_convs)] + [conv3(pk, self.bottleneck, psp)]
        for i in range(len(laterals) - 1, 0, -1):
            fine, coarse = laterals[i - 1], laterals[i]
            if (own_resize and fine.shape[2] == 2 * coarse.shape[2] and fine.shape[3] == 2 * coarse.shape[3]
                    and fine.permute(0, 2, 3, 1).is_contiguous()):
                fused.upsample2x_add_(fine, coarse)                         # the resize and the sum: one kernel, in place
            else:
                laterals[i - 1] = fine + self._resize(coarse, fine.shape[2:])
        return laterals

    def _forward_mfma(self, inputs):
        """uper_head.py:76-127 with every convolution on the hand-written kernels: 1x1 ConvModules (laterals, pyramid pooling) are
        ppn_gemm_bf16 over the NHWC tokens with bias + ReLU in the epilogue, 3x3 ConvModules the implicit-GEMM kernel
        (ppn_conv3x3_mfma_bf16), the last one fused with the 1x1 classifier (ppn_conv3x3_relu_classify2_bf16: the 64-channel
        activation at the highest resolution is never written); the FPN's top-down step, the resize + concatenation of its outputs
        and the pyramid pooling module's pools and output assembly on NHWC kernels (ppn_upsample2x_add_nhwc, ppn_resize_concat_nhwc,
        ppn_adaptive_pools_nhwc).  Nothing of the head runs on framework kernels but the 1x1 ConvModule of a pool scale with fewer
        than 256 pooled positions in the batch."""
        pk = self._mfma_packs()
        own_resize = self._own_resize()
        laterals = self._mfma_top_down(inputs, pk, own_resize)
        outs = [self._mfma_conv3(pk, self.fpn_convs[i], laterals[i].contiguous(memory_format=torch.channels_last)) for i in range(len(laterals) - 1)] + [laterals[-1]]
        if len(outs) == 4 and own_resize:
            cat = fused.resize_concat(outs)                                 # the three resizes + the concatenation: one kernel
        else:
            outs = [outs[0]] + [self._resize(o, outs[0].shape[2:]) for o in outs[1:]]
            cat = torch.cat(outs, dim=1).contiguous(memory_format=torch.channels_last)
        fb = self.fpn_bottleneck
        if use_mfma_conv(cat, fb.conv, narrow=True):
            return fused.conv3x3_relu_classify2(cat, *pk[fb], *pk["seg"]).to(cat.dtype)
        return self.conv_seg(self._mfma_conv3(pk, fb, cat))

    def _top_down(self, inputs):
        """uper_head.py:76-108 (= uper_pup_head.py:88-118) as the reference composes it: the pyramid pooling module + bottleneck, the
        laterals and the top-down sums.  Returns the laterals, finest first, the last one the bottleneck's output."""
        inputs = [inputs[i] for i in self.in_index]
        x = inputs[-1]
        pooled = [m(x) for m in self.psp_modules]
        if self._records_own([x] + pooled):                                 # training: the resizes back + the concatenation, one kernel each way
            psp = fused.resize_concat([x] + pooled)
        else:
            psp = torch.cat([x] + [self._resize(t, x.shape[2:]) for t in pooled], dim=1)
        laterals = [conv(inputs[i]) for i, conv in enumerate(self.lateral_convs)] + [self.bottleneck(psp)]
        for i in range(len(laterals) - 1, 0, -1):
            fine, coarse = laterals[i - 1], laterals[i]
            if fine.shape[2] == 2 * coarse.shape[2] and fine.shape[3] == 2 * coarse.shape[3] and self._records_own([fine, coarse]):
                laterals[i - 1] = fused.upsample2x_add(fine, coarse)        # training: the resize and the sum in one kernel
            else:
                laterals[i - 1] = fine + self._resize(coarse, fine.shape[2:])
        return laterals

    def _records_own(self, levels):
        """Whether a resize + sum / resize + concatenation of these tensors is recorded on the build's NHWC kernels (fused.upsample2x_add,
        fused.resize_concat and their backward entries): only while autograd records — inference keeps its path — on the GPU, under
        the conditions _mfma_top_down / _forward_mfma apply (_own_resize, at most 8 levels, channels a multiple of 8, no level larger than
        the first) and with PPNET_LIBRARY_UPSAMPLE unset.  The kernels read NHWC: a level that is not channels_last is copied once, as
        _forward_mfma's .contiguous(memory_format=channels_last) does."""
        t0 = levels[0]
        return (fused.recording(*levels) and not fused.library_upsample() and self._own_resize() and len(levels) <= 8
                and t0.dtype in (torch.float32, torch.bfloat16)
                and all(t.is_cuda and t.dtype == t0.dtype and t.shape[1] % 8 == 0 and t.shape[2] <= t0.shape[2] and t.shape[3] <= t0.shape[3]
                        for t in levels))

    def forward(self, inputs):
        if self._prepared_mfma(inputs[self.in_index[-1]]):
            return self._forward_mfma(inputs)
        laterals = self._top_down(inputs)
        outs = [self.fpn_convs[i](laterals[i]) for i in range(len(laterals) - 1)] + [laterals[-1]]
        if self._records_own(outs):                                         # training: the three resizes + the concatenation, one kernel each way
            return self.conv_seg(self.fpn_bottleneck(fused.resize_concat(outs)))
        outs = [outs[0]] + [self._resize(o, outs[0].shape[2:]) for o in outs[1:]]
        return self.conv_seg(self.fpn_bottleneck(torch.cat(outs, dim=1)))


class UPerPUPHead(UPerHead):
    """The authors' UPerNet head with progressive up-sampling chains (SegNet/mmseg/decode_heads/uper_pup_head.py:12-131, the file
    decode_heads/__init__.py:29 registers; over decode_head.py and psp_head.py): UPerHead's pyramid pooling, bottleneck, three lateral
    1x1 convs and top-down sums, then on EVERY level, the pooling output included, a chain of num_convs[i] steps of 3x3 ConvModule +
    bilinear x2 (`fpn_convs.i.j.0.{conv,bn}`), the four chain outputs concatenated, the 3x3 `fpn_bottleneck` and Dropout2d + the 1x1
    `conv_seg`.  The chains must end at one size (num_convs[i] - i constant); otherwise the concatenation raises, as the reference's
    torch.cat does.  The head of configs/nat/dense_nat_base.py and configs/swin/dense_swin_base.py."""

    def __init__(self, in_channels=(128, 256, 512, 1024), channels=256, num_classes=2, num_convs=(2, 3, 4, 5), up_scale=2,
                 pool_scales=(1, 2, 3, 6), in_index=(0, 1, 2, 3), dropout_ratio=0.1, align_corners=False, norm_cfg=None, sampler=None,
                 loss_decode=None, **kwargs):
        nn.Module.__init__(self)
        assert len(num_convs) == len(in_channels) == len(in_index)
        self.in_index, self.align_corners, self.num_convs = tuple(in_index), align_corners, tuple(num_convs)
        self.sampler, self.class_weight = _loss_options(sampler, loss_decode, num_classes)
        self.loss_specs, self.loss_single_ce = _loss_specs(loss_decode, num_classes), _single_ce(loss_decode)
        # registration order = mmseg's state-dict order (BaseDecodeHead.__init__ makes conv_seg and dropout first, decode_head.py:102-106)
        self.conv_seg = nn.Conv2d(channels, num_classes, 1)
        self.dropout = nn.Dropout2d(dropout_ratio) if dropout_ratio > 0 else nn.Identity()
        self.psp_modules = nn.ModuleList(
            nn.Sequential(nn.AdaptiveAvgPool2d(ps), _ConvModule(in_channels[-1], channels, 1)) for ps in pool_scales)
        self.bottleneck = _ConvModule(in_channels[-1] + len(pool_scales) * channels, channels, 3)
        # uper_pup_head.py:48-77: four laterals are built and the last is dropped; a chain per level
        self.lateral_convs = nn.ModuleList(_ConvModule(c, channels, 1) for c in in_channels[:-1])
        self.fpn_convs = nn.ModuleList(
            nn.ModuleList(nn.Sequential(_ConvModule(channels, channels, 3), _Upsample(up_scale, align_corners)) for _ in range(n))
            for n in num_convs)
        self.fpn_bottleneck = _ConvModule(len(in_channels) * channels, channels, 3)

    def _conv_modules(self):
        return ([m[1] for m in self.psp_modules] + [self.bottleneck] + list(self.lateral_convs)
                + [step[0] for chain in self.fpn_convs for step in chain] + [self.fpn_bottleneck])

    def _chains_x2(self, channels):
        """Every chain non-empty and every step a bilinear x2 without align_corners: the NHWC up-sampling kernels apply."""
        return (channels % 8 == 0 and all(len(chain) > 0 for chain in self.fpn_convs)
                and all(step[1].scale_factor == 2.0 and not step[1].align_corners for chain in self.fpn_convs for step in chain))

    def forward(self, inputs):
        x = inputs[self.in_index[-1]]
        if self._prepared_mfma(x) and self._chains_x2(self.conv_seg.in_channels):
            return self._forward_mfma(inputs)
        laterals = self._top_down(inputs)                                   # uper_pup_head.py:88-118
        ends = []
        for i, chain in enumerate(self.fpn_convs):                          # uper_pup_head.py:121-126, all but each chain's last Upsample
            t = laterals[i]
            for j, step in enumerate(chain):
                t = step[0](t)
                if j + 1 < len(chain):
                    t = step[1](t)
            ends.append(t)
        if (t.is_cuda and t.dtype in (torch.float32, torch.bfloat16) and self._chains_x2(t.shape[1])
                and len({tuple(e.shape) for e in ends}) == 1):
            cat = fused.upsample2x_concat(ends)                             # the last Upsample of every chain + torch.cat: one kernel (it records its own backward)
        else:
            cat = torch.cat([chain[-1][1](e) if len(chain) else e for chain, e in zip(self.fpn_convs, ends)], dim=1)
        return self.conv_seg(self.dropout(self.fpn_bottleneck(cat)))        # cls_seg, decode_head.py:224-229

    @staticmethod
    def _mfma_conv1(pk, cm, t):
        """UPerHead._mfma_conv1 with its few-row case (a pool scale with fewer than 256 pooled positions in the batch) in float32 with
        the float32 bias, as ppn_gemm_bf16's epilogue adds it: which of the two a pool scale takes depends on the batch, and this way
        the two differ only in the order of the float32 sums (the bfloat16 library call rounds the bias first)."""
        Cc = t.shape[1]
        if t.shape[0] * t.shape[2] * t.shape[3] >= 256 and Cc % 64 == 0 and Cc >= 128 and t.permute(0, 2, 3, 1).is_contiguous():
            return UPerHead._mfma_conv1(pk, cm, t)
        Bn, _, Hh, Ww = t.shape
        w, b = pk[cm]
        y = F.relu(F.linear(t.permute(0, 2, 3, 1).reshape(-1, Cc).float(), w.float(), b)).to(t.dtype)
        return y.view(Bn, Hh, Ww, -1).permute(0, 3, 1, 2)

    def _slice_images(self, inputs):
        """Images per launch such that no operand of the 3x3 convolution kernel reaches 2^32 bytes (it addresses them with 32-bit byte
        offsets, ppn_conv3x3_mfma_bf16 refuses larger ones): from the shapes of the bottleneck's input, every chain convolution's input
        and the concatenation — the largest (33.5 MB per image for dense NAT at R = 256: batches of at most 127)."""
        feats = [inputs[i] for i in self.in_index]
        ch = self.conv_seg.in_channels
        h, w = feats[-1].shape[2:]
        per = [(feats[-1].shape[1] + len(self.psp_modules) * ch) * h * w]
        for f, chain in zip(feats, self.fpn_convs):
            h, w = f.shape[2:]
            per += [ch * (h << j) * (w << j) for j in range(len(chain))]
        h, w = feats[0].shape[2:]
        per.append(len(self.fpn_convs) * ch * (h << self.num_convs[0]) * (w << self.num_convs[0]))
        return max(1, (2 ** 32 - 1) // (max(per) * feats[0].element_size()))

    def _forward_mfma(self, inputs):
        """Prepared bfloat16 inference on the build's own kernels: the pyramid pooling, bottleneck, laterals and top-down sums as in
        UPerHead._forward_mfma; every chain step one ppn_conv3x3_mfma_bf16 with the folded bias and the ReLU in its epilogue, then
        ppn_upsample2x_nhwc — except the last step of every chain, whose up-sampling and the concatenation of the four chains are ONE
        ppn_upsample2x_concat_nhwc; fpn_bottleneck + conv_seg one ppn_conv3x3_relu_classify2_bf16 (its 256-channel activation is
        never written; its float32 logits are returned as they are).  Batches past _slice_images go through in equal slices."""
        return _in_equal_slices(inputs, self._slice_images(inputs), self._mfma_slice)

    def _mfma_slice(self, inputs):
        pk = self._mfma_packs()
        laterals = self._mfma_top_down(inputs, pk, self._own_resize())
        ends = []
        for lat, chain in zip(laterals, self.fpn_convs):
            t = lat
            for step in chain[:-1]:
                t = fused.upsample2x_nhwc(self._mfma_conv3(pk, step[0], t))
            ends.append(self._mfma_conv3(pk, chain[-1][0], t))
        cat = fused.upsample2x_concat(ends)                                 # raises on chains of different lengths, as torch.cat does
        fb = self.fpn_bottleneck
        if use_mfma_conv(cat, fb.conv, narrow=True):
            return fused.conv3x3_relu_classify2(cat, *pk[fb], *pk["seg"])
        return self.conv_seg(self._mfma_conv3(pk, fb, cat))


class FCNHead(nn.Module):
    """mmseg's FCNHead (SegNet/mmseg/decode_heads/fcn_head.py:11-81 over decode_head.py:54-107,224-229) — the auxiliary head of
    the reference's NAT training configs (configs/_base_/models/nat.py:22-35, configs/nat/setr_up_nat_base.py:39-42: level 2,
    512 -> 256 channels, one 3x3 conv-BN-ReLU, Dropout2d(0.1), 1x1 classifier, loss weight 0.4).  Checkpoint keys follow mmseg:
    `convs.i.{conv,bn}`, `conv_cat.{conv,bn}`, `conv_seg`.  Training only: inference never evaluates it (encoder_decoder.py:63-80)."""

    def __init__(self, in_channels=256, channels=256, num_classes=19, num_convs=2, kernel_size=3, concat_input=True, dilation=1,
                 in_index=-1, dropout_ratio=0.1, align_corners=False, norm_cfg=None, loss_decode=None, sampler=None, **kwargs):
        super().__init__()
        assert num_convs >= 0 and dilation > 0
        self.in_index, self.align_corners, self.concat_input = in_index, align_corners, concat_input
        # the single cross-entropy form carries the head's weight here; every entry of another form carries its own (loss_specs)
        self.loss_weight = float((loss_decode or {}).get("loss_weight", 1.0)) if _single_ce(loss_decode) else 1.0
        self.sampler, self.class_weight = _loss_options(sampler, loss_decode, num_classes)
        self.loss_specs, self.loss_single_ce = _loss_specs(loss_decode, num_classes), _single_ce(loss_decode)
        if num_convs == 0:
            assert in_channels == channels
            self.convs = nn.Identity()
        else:
            self.convs = nn.Sequential(*[_ConvModule(in_channels if i == 0 else channels, channels, kernel_size, dilation)
                                         for i in range(num_convs)])
        if concat_input:
            self.conv_cat = _ConvModule(in_channels + channels, channels, kernel_size)
        self.conv_seg = nn.Conv2d(channels, num_classes, 1)
        self.dropout = nn.Dropout2d(dropout_ratio) if dropout_ratio > 0 else nn.Identity()

    def forward(self, inputs):
        x = inputs[self.in_index]
        y = self.convs(x)
        if self.concat_input:
            y = self.conv_cat(torch.cat([x, y], dim=1))
        return self.conv_seg(self.dropout(y))


def _valid_labels(gt, num_classes, ignore_index):
    return (gt != ignore_index) & (gt >= 0) & (gt < num_classes)


_CLASS_WEIGHTS = {}        # (weights, device, dtype) -> tensor: a head's list goes to the device once, not every step


def _class_weight_tensor(class_weight, device, dtype):
    if class_weight is None or torch.is_tensor(class_weight):
        return class_weight if class_weight is None else class_weight.to(device=device, dtype=dtype)
    key = (tuple(float(v) for v in class_weight), device, dtype)
    if key not in _CLASS_WEIGHTS:
        _CLASS_WEIGHTS[key] = torch.tensor(key[0], dtype=dtype, device=device)
    return _CLASS_WEIGHTS[key]


def _weighted_ce(logit, gt, class_weight, ignore_index):
    """class_weight[label] * cross-entropy per pixel [B,H,W], 0 on ignored pixels (label == ignore_index or outside [0, C))."""
    valid = _valid_labels(gt, logit.shape[1], ignore_index)
    safe = torch.where(valid, gt, torch.zeros_like(gt))
    ce = F.cross_entropy(logit, safe, weight=_class_weight_tensor(class_weight, logit.device, logit.dtype), reduction="none")
    return ce * valid.to(ce.dtype), valid


def ohem_weight(logit_fullres, gt, sampler, class_weight=None, ignore_index=255):
    """OHEMPixelSampler.sample (core/seg/sampler/ohem_pixel_sampler.py:32-85) as a torch composition: the 0 / 1 weight [B,H,W], in the
    logits' dtype, of full-resolution logits [B,C,H,W] against labels [B,H,W]; any dtype, CPU or GPU.  With n_valid valid pixels and
    batch_kept = min_kept * B: `thresh` given — 1 where the label's softmax probability is below max(thresh, the min(batch_kept,
    n_valid - 1)-th smallest one); thresh None — 1 on the batch_kept largest class_weight[label] * cross-entropy, and on every
    pixel that TIES with the smallest of them (the reference's unstable sort picks among ties; keeping all is the deterministic
    reading and the one deliberate difference); sampler None — 1 on every valid pixel.  A label outside [0, C) is ignored, the
    build's rule."""
    with torch.no_grad():
        gt = gt.long()
        valid = _valid_labels(gt, logit_fullres.shape[1], ignore_index)
        weight = torch.zeros(gt.shape, dtype=logit_fullres.dtype, device=logit_fullres.device)
        n_valid = int(valid.sum())
        if sampler is None or n_valid == 0:
            if sampler is None:
                weight[valid] = 1.0
            return weight
        batch_kept = sampler.min_kept * gt.shape[0]
        if sampler.thresh is not None:
            safe = torch.where(valid, gt, torch.zeros_like(gt))
            prob = F.softmax(logit_fullres, dim=1).gather(1, safe.unsqueeze(1)).squeeze(1)
            sort_prob = prob[valid].sort().values
            threshold = max(float(sort_prob[min(batch_kept, n_valid - 1)]), sampler.thresh)
            weight[valid & (prob < threshold)] = 1.0
        else:
            score, _ = _weighted_ce(logit_fullres, gt, class_weight, ignore_index)
            cut = score[valid].sort(descending=True).values[min(batch_kept, n_valid) - 1]
            weight[valid & (score >= cut)] = 1.0
        return weight


def decode_losses(logit, gt, loss_weight=1.0, ignore_index=255, class_weight=None, sampler=None):
    """(loss_ce, acc_seg) of BaseDecodeHead.losses (decode_head.py:231-265) for resized logits [B,C,H,W] and labels [B,H,W].
    mmseg's CrossEntropyLoss is F.cross_entropy(reduction='none', ignore_index) followed by a mean over ALL pixels — ignored
    ones contribute 0 to the sum and still count in the divisor (losses/cross_entropy_loss.py:20-31, losses/utils.py:66-68);
    accuracy() is called without an ignore index and divides by target.numel() (decode_head.py:264, losses/accuracy.py:39-49).
    class_weight (C floats or a tensor) scales every pixel's term by its label's weight and sampler (an OHEMPixelSampler) by
    ohem_weight's 0 / 1, still under the mean over all pixels (decode_head.py:245-256); acc_seg is not changed by either.  With
    both None this is the two library calls it always was."""
    if class_weight is None and sampler is None:
        loss = loss_weight * F.cross_entropy(logit, gt, ignore_index=ignore_index, reduction="none").mean()
    else:
        ce, _ = _weighted_ce(logit, gt, class_weight, ignore_index)
        loss = loss_weight * (ce * ohem_weight(logit, gt, sampler, class_weight, ignore_index).to(ce.dtype)).mean()
    with torch.no_grad():
        acc = (logit.argmax(1) == gt).float().sum() * (100.0 / gt.numel())
    return loss, acc


def resized_decode_losses(logit_lowres, gt, loss_weight=1.0, ignore_index=255, align_corners=False, class_weight=None, sampler=None):
    """decode_losses of a head's LOW-resolution logits [B,C,h,w] resized bilinearly to the labels' size [B,H,W]: the same
    (loss_ce, acc_seg).  CUDA float32 / bfloat16 logits with CUDA uint8 / int64 labels, align_corners False and sizes inside
    ppn_resize_ce_fwd's limits run on the fused kernel pair (fused.resize_cross_entropy: the resized logits are never built, the
    gradient reaches the low-resolution logits directly) — with class_weight or sampler on fused.ohem_cross_entropy's kernels
    (ppn_ohem_ce_fwd / _bwd: the sampler is a radix select on the device, no sort, no weight tensor; a thresh outside (0, 1] is
    outside them); PPNET_LIBRARY_LOSS=1 (read at call time), CPU tensors and everything else take the library composition,
    F.interpolate of the float32 logits followed by decode_losses on int64 labels."""
    own = not align_corners and not os.environ.get("PPNET_LIBRARY_LOSS")
    if class_weight is None and sampler is None:
        if own and fused.resize_ce_ok(logit_lowres, gt):
            mean, correct = fused.resize_cross_entropy(logit_lowres, gt, ignore_index)
            return loss_weight * mean, correct.float() * (100.0 / gt.numel())        # (a count below 2^24 is exact in float32)
    elif (own and fused.ohem_ce_ok(logit_lowres, gt)
          and (sampler is None or sampler.thresh is None or 0.0 < sampler.thresh <= 1.0)):
        cw = _class_weight_tensor(class_weight, logit_lowres.device, torch.float32)
        mean, correct, _ = fused.ohem_cross_entropy(logit_lowres, gt, ignore_index, cw, None if sampler is None else sampler.thresh,
                                                    None if sampler is None else sampler.min_kept)
        return loss_weight * mean, correct.float() * (100.0 / gt.numel())
    logit = F.interpolate(logit_lowres.float(), gt.shape[-2:], mode="bilinear", align_corners=align_corners)
    return decode_losses(logit, gt.long(), loss_weight, ignore_index, class_weight, sampler)


def eval_areas(pred, gt, num_classes, ignore_index=255):
    """The three area histograms of an evaluation, int64 [3, num_classes] (intersect | prediction | label; union = prediction + label -
    intersect), from argmax labels `pred` and ground truth `gt` of one shape — mmseg's intersect_and_union (core/evaluation/
    metrics.py:26-86) with exact integer counts (torch.bincount; the reference's histc works on floats).  A label equal to
    ignore_index OR outside [0, num_classes) is ignored: it adds to none of the three.  mmseg masks by label != ignore_index only, so
    an out-of-range label would still count in its prediction histogram — the deliberate difference, ppn_seg_eval's rule."""
    pred, gt = pred.reshape(-1).long(), gt.reshape(-1).long()
    valid = (gt != ignore_index) & (gt >= 0) & (gt < num_classes)
    pred, gt = pred[valid], gt[valid]
    return torch.stack([torch.bincount(pred[pred == gt], minlength=num_classes), torch.bincount(pred, minlength=num_classes),
                        torch.bincount(gt, minlength=num_classes)])


def resized_eval_areas(logit_lowres, gt, ignore_index=255, align_corners=False):
    """eval_areas of a head's LOW-resolution logits [B,C,h,w] resized bilinearly to the labels' size [B,H,W] and their argmax: int64
    [3,C].  CUDA float32 / bfloat16 logits with CUDA uint8 / int64 labels, align_corners False, C <= 256 and sizes inside
    ppn_seg_eval's limits run on the fused kernel (fused.seg_eval: neither the resized logits nor the labels' masks are built);
    PPNET_LIBRARY_EVAL=1 (read at call time), CPU tensors and everything else take the library composition, F.interpolate of the
    float32 logits, argmax and three bincounts."""
    if not align_corners and not os.environ.get("PPNET_LIBRARY_EVAL") and fused.seg_eval_ok(logit_lowres, gt):
        return fused.seg_eval(logit_lowres, gt, ignore_index)[0]
    with torch.no_grad():
        logit = F.interpolate(logit_lowres.float(), gt.shape[-2:], mode="bilinear", align_corners=align_corners)
        return eval_areas(logit.argmax(1), gt, logit.shape[1], ignore_index)


def tta_mean_prob(logits, mids, flips, out_hw):
    """The mean class probabilities [B,C,H,W] of a test-time augmentation (mmseg's aug_test, encoder_decoder.py:200-285) from the
    heads' low-resolution logits, in torch ops: per augmentation logits[a] [B,C,h_a,w_a] resized bilinearly (align_corners=False) to
    mids[a] = (hm, wm), the augmentation's image size, and from there to out_hw = (H, W); softmax over the classes; flipped back along
    W for flips[a] == 'horizontal', along H for 'vertical' (None: not); summed in index order and divided by the number of
    augmentations.  Everything in the logits' dtype promoted to at least float32, nothing rounded in between — ppn_seg_tta's
    definition (fused.seg_tta), on any device."""
    if not len(logits) == len(mids) == len(flips) or not logits:
        raise ValueError(f"tta_mean_prob: {len(logits)} logits, {len(mids)} sizes, {len(flips)} flips")
    total = None
    for x, mid, fl in zip(logits, mids, flips):
        if fl not in (None, "horizontal", "vertical"):
            raise ValueError(f"tta_mean_prob: flip {fl!r}")
        x = x.to(torch.promote_types(x.dtype, torch.float32))
        x = F.interpolate(x, tuple(mid), mode="bilinear", align_corners=False)
        p = F.softmax(F.interpolate(x, tuple(out_hw), mode="bilinear", align_corners=False), dim=1)
        if fl is not None:
            p = p.flip(dims=(3,) if fl == "horizontal" else (2,))
        total = p if total is None else total + p
    return total / len(logits)


def dice_loss(logit_fullres, gt, smooth=1.0, exponent=2, class_weight=None, loss_weight=1.0, ignore_index=255):
    """mmseg's DiceLoss.forward (losses/dice_loss.py:12-47,92-123) for full-resolution logits [B,C,H,W] and labels [B,H,W], in torch
    ops: any dtype, any exponent, CPU or GPU.  p = softmax(logit, 1), tc = the labels clamped into [0, C - 1], v = the label is valid;
    per image and class  num = 2 sum_px p_i [tc == i] v + smooth,  den = sum_px (p_i^exponent + [tc == i]) + smooth  — the
    denominator is NOT masked: an ignored label counts as the class its clamp lands on (255 as class C - 1), the reference's own quirk —
    and  loss = loss_weight / C * sum_{i != ignore_index} class_weight_i * mean_b (1 - num / den)  (binary_dice_loss is itself
    @weighted_loss: the batch mean; the class that equals ignore_index is skipped).  The head calls the reference's loss with
    weight=seg_weight and ignore_index=255 as keyword arguments that fall into **kwards unused: a pixel sampler's weights do not reach
    Dice, and the ignore_index is the loss's own.  v: a label equal to ignore_index OR outside [0, C) is not valid — this build's
    rule; the reference masks by label != ignore_index only (the two agree on every in-range label and on ignore_index itself)."""
    C = logit_fullres.shape[1]
    gt = gt.long()
    p = F.softmax(logit_fullres, dim=1).flatten(2)                                              # [B, C, HW]
    onehot = F.one_hot(gt.clamp(0, C - 1), C).permute(0, 3, 1, 2).flatten(2).to(p.dtype)
    valid = _valid_labels(gt, C, ignore_index).flatten(1).unsqueeze(1).to(p.dtype)
    num = (p * onehot * valid).sum(2) * 2 + smooth
    den = (p.pow(exponent) + onehot).sum(2) + smooth                                            # (0 / 1 to any positive power is itself)
    per_class = (1 - num / den).mean(0)                                                         # [C]
    if class_weight is not None:
        per_class = per_class * _class_weight_tensor(class_weight, p.device, p.dtype)
    keep = [i for i in range(C) if i != ignore_index]
    return loss_weight * per_class[keep].sum() / C


def resized_dice_losses(logit_lowres, gt, loss_weight=1.0, smooth=1.0, exponent=2, class_weight=None, ignore_index=255, align_corners=False):
    """(loss_dice, acc_seg) of a head's LOW-resolution logits [B,C,h,w] resized bilinearly to the labels' size [B,H,W]: dice_loss and
    decode_losses' accuracy.  CUDA float32 / bfloat16 logits with CUDA uint8 / int64 labels, align_corners False, exponent 2 and sizes
    inside ppn_resize_dice_fwd's limits (C <= 256) run on the fused kernel pair (fused.resize_dice: neither the resized logits, their
    softmax nor a one-hot tensor is built); PPNET_LIBRARY_LOSS=1 (read at call time), CPU tensors and everything else take the library
    composition, F.interpolate of the float32 logits followed by dice_loss on int64 labels."""
    if not align_corners and not os.environ.get("PPNET_LIBRARY_LOSS") and exponent == 2 and fused.resize_dice_ok(logit_lowres, gt):
        cw = _class_weight_tensor(class_weight, logit_lowres.device, torch.float32)
        dice, correct = fused.resize_dice(logit_lowres, gt, ignore_index, smooth, cw)
        return loss_weight * dice, correct.float() * (100.0 / gt.numel())
    logit = F.interpolate(logit_lowres.float(), gt.shape[-2:], mode="bilinear", align_corners=align_corners)
    loss = dice_loss(logit, gt, smooth, exponent, class_weight, loss_weight, ignore_index)
    with torch.no_grad():
        acc = (logit.argmax(1) == gt).float().sum() * (100.0 / gt.numel())
    return loss, acc


def resized_head_losses(logit_lowres, gt, head, head_weight=1.0):
    """BaseDecodeHead.losses (decode_head.py:231-265) for a head's low-resolution logits and its loss_specs: {loss_name: value, ...,
    'acc_seg': value}.  CrossEntropyLoss entries go through resized_decode_losses — the head's pixel sampler and the entry's class
    weights apply to them only — and DiceLoss entries through resized_dice_losses; entries with equal names add.  acc_seg is computed
    once: by the cross-entropy kernel when there is such an entry, else from Dice's count.  The single cross-entropy form is the call
    it always was: weight head_weight (1.0 for the decode head, FCNHead.loss_weight for the auxiliary one), ignore_index 255; every
    entry of another form carries its own loss_weight, times head_weight."""
    out, acc = {}, None
    for spec in head.loss_specs:
        w = head_weight if head.loss_single_ce else head_weight * spec["loss_weight"]
        if spec["type"] == _CE:
            loss, a = resized_decode_losses(logit_lowres, gt, w, align_corners=head.align_corners, class_weight=spec["class_weight"],
                                            sampler=head.sampler)
            if acc is None or acc[0] != _CE:
                acc = (_CE, a)
        else:
            loss, a = resized_dice_losses(logit_lowres, gt, w, spec["smooth"], spec["exponent"], spec["class_weight"], spec["ignore_index"],
                                          head.align_corners)
            if acc is None:
                acc = (_DICE, a)
        name = spec["loss_name"]
        out[name] = out[name] + loss if name in out else loss
    out["acc_seg"] = acc[1]
    return out
