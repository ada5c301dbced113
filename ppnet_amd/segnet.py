"""SegNet = a backbone (NAT / DiNAT, DiNAT_s, Swin, ViT) + a decode head (SETR-UP, UPerNet, UPerPUP; FCN auxiliary) wired as the reference's
EncoderDecoder (mmseg/models/segmentors/encoder_decoder.py:63-80,200-265) — plain nn.Modules with the reference's constructor
arguments and checkpoint key names (`backbone.*`, `decode_head.*`, `auxiliary_head.*`), so mmcv `{'state_dict', 'meta'}`
checkpoints load.  The parts live in dense.py (dispatch policy), nat.py / dinats.py / swin.py / vit.py, heads.py and configs.py, none of which
imports this module; every name it defined while it held them all is re-exported below under its earlier spelling (same objects)."""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import fused
from .configs import (DINAT_BASE, DINAT_LARGE, DINATS_BASE_SETRUP, NAT_BASE_UPER, NAT_BASE_UPERPUP, NAT_MINI_UPER, SWIN_BASE_SETRUP,  # noqa: F401
                      SWIN_BASE_UPER, SWIN_BASE_UPERPUP, VIT_BASE_SETRUP, _SWIN_BASE_BACKBONE, _SWIN_NORM_CFG, _UPERPUP_AUX)
from .dense import (IMG_MEAN, IMG_STD, LIBRARY_GEMM_BELOW_C, LIBRARY_GEMM_FROM_C, drop_path, normalize_images)  # noqa: F401
from .dense import accumulate as _accumulate, bias32 as _bias32, library_width as _library_width, linear as _linear  # noqa: F401
from .dense import mfma_weights as _mfma_weights, own_gemm_ok as _own_gemm_ok, use_mfma_conv as _use_mfma_conv  # noqa: F401
from .heads import (FCNHead, SETRUPHead, UPerHead, UPerPUPHead, _ConvModule, _Upsample, decode_losses, dice_loss,  # noqa: F401
                    resized_decode_losses, resized_head_losses)
from .heads import OHEMPixelSampler, eval_areas, ohem_weight, resized_eval_areas  # noqa: F401
from .dinats import DiNAT_s
from .na import NeighborhoodAttention2D  # noqa: F401
from .nat import NAT, ConvDownsampler, ConvTokenizer, DiNAT, Mlp, NATBlock, NATLayer, _fold_doc  # noqa: F401
from .swin import SwinTransformer
from .vit import VisionTransformer


# Class counts from which aug_test merges with the library composition by default: ppn_seg_tta is the faster side where a pixel's logits
# stay in registers or LDS (12 augmentations to 16 x 512^2: 1.7-2.3 x at C = 2, 1.6 x at C = 19) and the slower one above (0.6 x float32,
# 0.4 x bfloat16 at C = 150; tools/seg_tta_timing.py).  PPNET_LIBRARY_TTA_FROM_C overrides, read at call time.
LIBRARY_TTA_FROM_C = fused.SEG_TTA_LDS_CLASSES + 1


class SegNet(nn.Module):
    """EncoderDecoder(test_cfg=mode 'whole') (SegNet/mmseg/models/segmentors/encoder_decoder.py:16-265, base.py:62-112): the
    constructor takes the reference's config sub-dicts (`from_config` the whole `model=dict(...)`), `forward` the reference
    harness's call — `model(return_loss=False, img=[x], img_metas=[[...]]) -> list[np.ndarray int64 [H,W]]`
    (mmseg/apis/test.py:93) — and `model(img=x, img_metas=[...], gt_semantic_seg=y)` returns the loss dict of forward_train."""

    def __init__(self, backbone=None, decode_head=None, auxiliary_head=None, train_cfg=None, test_cfg=None, pretrained=None):
        super().__init__()
        bb_cfg = dict(backbone or DINAT_BASE["backbone"])
        bb_type = bb_cfg.pop("type", "DiNAT")
        if pretrained is not None and bb_cfg.get("pretrained") is None:
            bb_cfg["pretrained"] = pretrained                                  # encoder_decoder.py:32-36
        self.backbone = {"NAT": NAT, "DiNAT": DiNAT, "DiNAT_s": DiNAT_s, "SwinTransformer": SwinTransformer,
                         "VisionTransformer": VisionTransformer}[bb_type](**bb_cfg)
        head_cfg = dict(decode_head or DINAT_BASE["decode_head"])
        head_type = head_cfg.pop("type", "SETRUPHead")
        self.decode_head = {"SETRUPHead": SETRUPHead, "UPerHead": UPerHead, "UPerPUPHead": UPerPUPHead, "FCNHead": FCNHead}[head_type](**head_cfg)
        self.auxiliary_head = None
        if auxiliary_head is not None:                                         # encoder_decoder.py:52-61 (a dict, or a list of them)
            mk = lambda c: FCNHead(**{k: v for k, v in dict(c).items() if k != "type"})
            self.auxiliary_head = nn.ModuleList(mk(c) for c in auxiliary_head) if isinstance(auxiliary_head, (list, tuple)) else mk(auxiliary_head)
        self.align_corners = self.decode_head.align_corners
        self.train_cfg, self.test_cfg = train_cfg, dict(test_cfg or {"mode": "whole"})
        if self.test_cfg.get("mode", "whole") != "whole":
            raise NotImplementedError("test_cfg.mode 'whole' only (every configuration under SegNet/configs)")
        self._narrow_levels()

    def _aux_heads(self):
        a = self.auxiliary_head
        return [] if a is None else (list(a) if isinstance(a, nn.ModuleList) else [a])

    def _narrow_levels(self, inference=False):
        """The backbone evaluates only the levels a head reads (their output norm + the NHWC -> NCHW view): SETR-UP reads the last
        one; the auxiliary head's level joins while it can be trained (not after prepare_inference)."""
        outs = tuple(self.backbone.out_indices)        # a head's in_index selects a SLOT of the backbone's output list

        def levels(ii):
            ii = ii if isinstance(ii, (tuple, list)) else (ii,)
            for i in ii:
                if not -len(outs) <= i < len(outs):
                    raise ValueError(f"head in_index {i} outside the backbone's {len(outs)} outputs (out_indices {outs})")
            return {outs[i] for i in ii}

        need = levels(self.decode_head.in_index)
        if not inference:
            for h in self._aux_heads():
                need |= levels(h.in_index)
        self.backbone.compute_indices = tuple(sorted(need))

    @classmethod
    def from_config(cls, cfg):
        """cfg: the reference's `model = dict(type='EncoderDecoder', pretrained=..., backbone=dict(type='DiNAT', ...),
        decode_head=dict(type='SETRUPHead', ...), auxiliary_head=..., train_cfg=..., test_cfg=dict(mode='whole'))`
        (configs/_base_/models/dinat.py:3-46 merged with configs/dinat/dinat_base.py:5-24), or a whole config holding it under
        'model'.  A head's `sampler=dict(type='OHEMPixelSampler', thresh=..., min_kept=...)` and `loss_decode['class_weight']` (a list
        of floats) are read and applied by forward_train (heads._loss_options; another sampler type or a weight file raises);
        `loss_decode['loss_weight']` is read by the auxiliary head.  `loss_decode` may also be a DiceLoss dict or a list of
        CrossEntropyLoss / DiceLoss dicts (heads._loss_specs): then every entry's type, loss_name, loss_weight and class_weight are
        honoured, and DiceLoss's smooth, exponent and ignore_index; another loss type (LovaszLoss, FocalLoss, ...), use_sigmoid=True, a
        reduction other than 'mean' and a weight file raise NotImplementedError.  A single CrossEntropyLoss dict is read as before: its
        keys other than class_weight and loss_weight stay unread.  mmcv-only keys (init_cfg, norm_cfg, conv_cfg, act_cfg,
        in_patch_size, frozen_stages) are accepted and ignored where this build has one fixed choice."""
        cfg = dict(cfg.get("model", cfg))
        typ = cfg.pop("type", "EncoderDecoder")
        if typ != "EncoderDecoder":
            raise NotImplementedError(f"segmentor type {typ!r}: EncoderDecoder only")
        known = ("backbone", "decode_head", "auxiliary_head", "train_cfg", "test_cfg", "pretrained")
        extra = set(cfg) - set(known) - {"neck", "init_cfg"}
        if extra or cfg.get("neck") is not None:
            raise NotImplementedError(f"unsupported model keys: {sorted(extra | ({'neck'} if cfg.get('neck') is not None else set()))}")
        return cls(**{k: cfg[k] for k in known if k in cfg})

    def prepare_inference(self):
        """After the checkpoint is loaded: fold each head BatchNorm into its convolution (exact algebra in float32,
        W' = W * g/sqrt(v+eps), b' = beta - mu * g/sqrt(v+eps)) and put every convolution weight in channels_last, so
        the whole network runs on NHWC tensors with no layout copies.  Changes the state-dict layout: load first."""
        cms = [up[0] for up in self.decode_head.up_convs] if isinstance(self.decode_head, SETRUPHead) else \
              [m for m in self.decode_head.modules() if isinstance(m, _ConvModule)]
        for cm in cms:
            if isinstance(cm.bn, nn.BatchNorm2d):
                bn, conv = cm.bn, cm.conv
                scale = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).detach()
                conv.weight = nn.Parameter((conv.weight.detach() * scale.view(-1, 1, 1, 1)))
                conv.bias = nn.Parameter((bn.bias - bn.running_mean * scale).detach())
                cm.bn = nn.Identity()
        if not os.environ.get("PPNET_NO_FOLD"):          # A/B knob: keep the fused residual+LayerNorm form
            for level in self.backbone.levels:
                level.fold()
        self._narrow_levels(inference=True)              # the auxiliary head is a training-time branch
        self.prepared = True
        self.to(memory_format=torch.channels_last)
        return self

    prepared = False

    def encode_decode(self, img):
        out = self.decode_head(self.backbone(img))
        return F.interpolate(out, img.shape[-2:], mode="bilinear", align_corners=self.align_corners)   # (img may be u8 codes [B,R,R])

    def labels_u8(self, img):
        """argmax labels as u8 [B,R,R].  SETR-UP head with two classes on the GPU: the x2 up-sampling of the logits, the
        resize to the input size, softmax and argmax are one HIP kernel (ppn_seg_labels_2class); otherwise forward()."""
        head = self.decode_head
        if img.dtype == torch.uint8 and isinstance(self.backbone, NAT) and not self.backbone.patch_embed.takes_codes(img):
            # a NAT tokenizer the palette kernels do not serve (float32 weights, an embed width other than 128 — DiNAT-L, NAT-Mini): render
            img = fused.grid_to_image(img, IMG_MEAN, IMG_STD, next(self.parameters()).dtype)
        if (img.is_cuda and isinstance(head, SETRUPHead) and head.conv_seg.out_channels == 2 and not self.align_corners
                and not head.align_corners and head.up_convs[-1][1].scale_factor == 2.0):
            return fused.seg_labels_2class(head(self.backbone(img), lowres=True), img.shape[-2:])
        if img.dtype == torch.uint8 and not self.backbone.patch_embed.takes_codes(img):
            img = fused.grid_to_image(img, IMG_MEAN, IMG_STD, next(self.parameters()).dtype)   # occupancy codes the tokenizer kernel cannot take: render
        return self.forward(img).to(torch.uint8)                  # (codes go straight to the palette tokenizer: NAT.forward)

    # ------------------------------------------------------------------ the reference's calling convention
    def forward(self, img=None, img_metas=None, return_loss=True, return_logits=False, **kwargs):
        """base.py:99-112.  Three forms:
        * `model(return_loss=False, img=[x], img_metas=[[meta, ...]])` — what single_gpu_test / multi_gpu_test call
          (mmseg/apis/test.py:93,196): one entry per test-time augmentation; returns list[np.ndarray int64 [H,W]], one per image.
        * `model(img=x, img_metas=[meta, ...], gt_semantic_seg=y)` (return_loss=True) — forward_train: the dict of losses.
        * `model(x)` with a tensor and no img_metas (this build's batched form): the argmax labels as a tensor [B,H,W]
          (+ the logits with return_logits=True)."""
        if isinstance(img, (list, tuple)):
            if return_loss:
                raise TypeError("return_loss=True takes img as a Tensor and img_metas as list[dict] (base.py:103-107)")
            return self.forward_test(list(img), img_metas, **kwargs)
        if img_metas is None and "gt_semantic_seg" not in kwargs:
            logits = self.encode_decode(img)
            pred = F.softmax(logits.float(), dim=1).argmax(dim=1)           # encoder_decoder.py:242,257
            return (pred, logits) if return_logits else pred
        if return_loss:
            return self.forward_train(img, img_metas, **kwargs)
        raise TypeError("return_loss=False takes img as list[Tensor] and img_metas as list[list[dict]] (base.py:103-107)")

    def forward_test(self, imgs, img_metas, rescale=True, **kwargs):
        """base.py:64-96 + encoder_decoder.py:254-292: per augmentation softmax of the logits resized to ori_shape, flipped back
        where the augmentation flipped, averaged over the augmentations; argmax -> one int64 array per image."""
        for var, name in ((imgs, "imgs"), (img_metas, "img_metas")):
            if not isinstance(var, list):
                raise TypeError(f"{name} must be a list, but got {type(var)}")
        if len(imgs) != len(img_metas):
            raise ValueError(f"num of augmentations ({len(imgs)}) != num of image meta ({len(img_metas)})")
        if len(imgs) == 1:
            return self.simple_test(imgs[0], img_metas[0], rescale)
        return self.aug_test(imgs, img_metas, rescale)

    def aug_test(self, imgs, img_metas, rescale=True):
        """encoder_decoder.py:267-285: the labels of the mean, over the augmentations, of `inference`'s probabilities; one int64 array
        per image.  CUDA inputs without autograd, at most fused.SEG_TTA_MAX_AUGS augmentations of one ori_shape, C <= 256 and
        align_corners False on model and head: the head runs once per augmentation and its LOW-resolution logits go to one
        ppn_seg_tta launch (fused.seg_tta: both resizes, softmax, un-flip, mean and argmax in float32; no full-resolution tensor but
        the uint8 labels).  PPNET_LIBRARY_TTA=1 (read at call time), CPU tensors and everything else take the composition of
        `inference` calls as it always ran — and so does C >= LIBRARY_TTA_FROM_C by default: above fused.SEG_TTA_LDS_CLASSES the kernel
        interpolates every logit three times and is the slower side; PPNET_LIBRARY_TTA_FROM_C=257 opts in."""
        return list(self.aug_labels(imgs, img_metas, rescale).to(torch.int64).cpu().numpy())

    def aug_labels(self, imgs, img_metas, rescale=True):
        """aug_test's labels as a tensor [B,H,W] on the inputs' device: uint8 from the kernel, int64 from the composition."""
        assert rescale                                                       # encoder_decoder.py:274-276
        merged = self._aug_test_fused(imgs, img_metas)
        if merged is not None:
            return merged
        prob = self.inference(imgs[0], img_metas[0], rescale)
        for x, m in zip(imgs[1:], img_metas[1:]):
            prob = prob + self.inference(x, m, rescale)
        return (prob / len(imgs)).argmax(dim=1)

    def _aug_test_fused(self, imgs, img_metas):
        """aug_test's labels as uint8 [B,H,W] from one ppn_seg_tta launch, or None where that path does not apply."""
        classes = self.decode_head.conv_seg.out_channels
        if (torch.is_grad_enabled() or os.environ.get("PPNET_LIBRARY_TTA") or not all(x.is_cuda for x in imgs)
                or len(imgs) > fused.SEG_TTA_MAX_AUGS or self.align_corners or self.decode_head.align_corners
                or classes > fused.SEG_TTA_MAX_CLASSES or classes >= int(os.environ.get("PPNET_LIBRARY_TTA_FROM_C", LIBRARY_TTA_FROM_C))):
            return None
        mids, flips, sizes = [], [], set()
        for x, m in zip(imgs, img_metas):
            metas = _meta(m) if m else [{}]
            ori = metas[0].get("ori_shape")
            assert all(mm.get("ori_shape") == ori for mm in metas)
            mids.append(tuple(x.shape[-2:]))                                 # encode_decode's resize target
            sizes.add(tuple(ori[:2]) if ori is not None else mids[-1])
            d = metas[0].get("flip_direction", "horizontal") if metas[0].get("flip", False) else None
            assert d in (None, "horizontal", "vertical")
            flips.append(d)
        if len(sizes) != 1:
            return None                                                      # (the composition's own add raises)
        logits = [self.decode_head(self.backbone(x)) for x in imgs]
        out_hw = sizes.pop()
        if not fused.seg_tta_ok(logits, mids, flips, out_hw):
            return None                                                      # a dtype or size outside the kernel's
        return fused.seg_tta(logits, mids, flips, out_hw)[0]

    def simple_test(self, img, img_meta, rescale=True):
        """encoder_decoder.py:254-265.  Unflipped whole-image inference at the input size on the GPU takes the fused tail
        (labels_u8: up-sampling, resize, softmax and argmax in one kernel) — the same labels, as int64 arrays."""
        meta0 = _meta(img_meta)[0] if img_meta else {}
        size = tuple(meta0.get("ori_shape", img.shape[-2:])[:2]) if rescale else tuple(img.shape[-2:])
        if img.is_cuda and not meta0.get("flip", False) and size == tuple(img.shape[-2:]) and not torch.is_grad_enabled():
            return list(self.labels_u8(img).to(torch.int64).cpu().numpy())
        return list(self.inference(img, img_meta, rescale).argmax(dim=1).cpu().numpy())

    def inference(self, img, img_meta, rescale=True):
        """encoder_decoder.py:200-252: whole_inference + softmax + un-flip.  Returns the class probabilities [B,C,H,W]."""
        metas = _meta(img_meta) if img_meta else [{}]
        ori = metas[0].get("ori_shape")
        assert all(m.get("ori_shape") == ori for m in metas)
        logits = self.encode_decode(img)
        if rescale and ori is not None and tuple(ori[:2]) != tuple(logits.shape[-2:]):
            logits = F.interpolate(logits, tuple(ori[:2]), mode="bilinear", align_corners=self.align_corners)
        out = F.softmax(logits.float(), dim=1)
        if metas[0].get("flip", False):
            d = metas[0].get("flip_direction", "horizontal")
            assert d in ("horizontal", "vertical")
            out = out.flip(dims=(3,) if d == "horizontal" else (2,))
        return out

    def forward_train(self, img, img_metas, gt_semantic_seg, **kwargs):
        """encoder_decoder.py:122-152 with decode_head.py:209-265 (losses): {'decode.loss_ce', 'decode.acc_seg'} and, with an
        auxiliary head, {'aux.loss_ce', 'aux.acc_seg'} (loss weights 1.0 / 0.4, ignore_index 255).  Each head's own pixel sampler and
        class weights (decode_head.py:245-256) go with its logits.  A head whose loss_decode is a list, or a DiceLoss, emits
        '{prefix}.{loss_name}' for every name of its loss_specs (equal names summed) — '{prefix}.loss_dice' for DiceLoss — and one
        '{prefix}.acc_seg'."""
        if self.prepared:
            raise RuntimeError("SegNet.prepare_inference() folded BatchNorm / LayerScale into the weights: build a fresh SegNet to train")
        feats = self.backbone(img)
        gt = gt_semantic_seg.squeeze(1) if gt_semantic_seg.dim() == 4 else gt_semantic_seg
        if gt.dtype != torch.uint8:                    # uint8 labels go to the loss kernel as they are
            gt = gt.long()
        losses = {}
        heads = [("decode", self.decode_head, 1.0)] + [(f"aux_{i}" if isinstance(self.auxiliary_head, nn.ModuleList) else "aux", h, h.loss_weight)
                                                       for i, h in enumerate(self._aux_heads())]
        for name, head, w in heads:
            # the head's output in its own dtype: the resize and each loss are one kernel pair on the GPU (heads.resized_head_losses)
            if head.loss_single_ce:                    # one CrossEntropyLoss, or none: the call it always was
                losses[f"{name}.loss_ce"], losses[f"{name}.acc_seg"] = resized_decode_losses(
                    head(feats), gt, w, align_corners=head.align_corners, class_weight=head.class_weight, sampler=head.sampler)
                continue
            for key, value in resized_head_losses(head(feats), gt, head, w).items():
                losses[f"{name}.{key}"] = value
        return losses

    @torch.no_grad()
    def eval_areas(self, img, gt_semantic_seg, ignore_index=255, aug=None):
        """The area histograms that mmseg's evaluation sums over a dataset (intersect_and_union of the whole-image prediction,
        core/evaluation/metrics.py:26-86): int64 [3, C] on img's device — intersect | prediction | label per class, for
        evaluate.total_area_to_metrics.  Labels as in forward_train ([B,1,H,W] or [B,H,W]; uint8 as they are).  With labels of the
        input's size the head's output goes to heads.resized_eval_areas in its own resolution and dtype — one kernel on the GPU
        (ppn_seg_eval: no [B,C,H,W] logits, no softmax, no int64 argmax, no masks); labels of another size get encode_decode's
        resize to the input size, then the resize to the labels (encoder_decoder.py:247-252) and the library composition.
        aug, an augment.MultiScaleFlipAug: the prediction is aug_labels' merge over aug(img) (on the GPU one ppn_seg_tta launch) at the
        input's size, which the labels must have; the areas are heads.eval_areas of it."""
        gt = gt_semantic_seg.squeeze(1) if gt_semantic_seg.dim() == 4 else gt_semantic_seg
        if gt.dtype != torch.uint8:
            gt = gt.long()
        if aug is not None:
            imgs, metas = aug(img)
            pred = self.aug_labels(imgs, metas) if len(imgs) > 1 else self.inference(imgs[0], metas[0]).argmax(dim=1)
            if tuple(pred.shape) != tuple(gt.shape):
                raise ValueError(f"eval_areas with test-time augmentation: labels {tuple(gt.shape)} for predictions {tuple(pred.shape)}")
            return eval_areas(pred, gt, self.decode_head.conv_seg.out_channels, ignore_index)
        if tuple(gt.shape[-2:]) == tuple(img.shape[-2:]):
            return resized_eval_areas(self.decode_head(self.backbone(img)), gt, ignore_index, align_corners=self.align_corners)
        logit = F.interpolate(self.encode_decode(img).float(), gt.shape[-2:], mode="bilinear", align_corners=self.align_corners)
        return eval_areas(logit.argmax(1), gt, logit.shape[1], ignore_index)


def randomize_neutral_parameters(model, seed=0, gamma=(0.05, 0.3)):
    """Give every parameter that a fresh initialisation leaves NEUTRAL a non-trivial seeded value, in place: LayerScale
    (`layer_scale=1e-5`, dinat_base.py:14, makes every residual branch invisible), biases (0), LayerNorm / BatchNorm affine
    parameters (1 / 0), the relative position bias and the BatchNorm running statistics (0 / 1).  No trained weights ship with
    the reference; a model initialised this way exercises the arithmetic the way a trained checkpoint does, which is what a
    precision comparison (bench.py's `ppnet.parity`, tests/test_ppnet_config3.py) needs.  Returns the model."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("gamma1") or name.endswith("gamma2"):
                p.copy_(torch.empty(p.shape).uniform_(gamma[0], gamma[1], generator=g))
            elif p.dim() == 1 and name.endswith("bias"):
                p.copy_(torch.empty(p.shape).uniform_(-0.2, 0.2, generator=g))
            elif p.dim() == 1 and name.endswith("weight"):
                p.copy_(torch.empty(p.shape).uniform_(0.7, 1.3, generator=g))
            elif name.endswith("rpb"):
                p.copy_(torch.empty(p.shape).normal_(0.0, 0.5, generator=g))
        for mod in model.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.running_mean.copy_(torch.empty(mod.running_mean.shape).uniform_(-0.2, 0.2, generator=g))
                mod.running_var.copy_(torch.empty(mod.running_var.shape).uniform_(0.5, 1.5, generator=g))
    return model


@torch.no_grad()
def balance_classifier_bias(segnet, images):
    """Shift the decode head's class-1 bias so that the two classes split the pixels of `images` ([n,3,R,R], normalised)
    evenly: an UNTRAINED network labels every pixel alike, which makes any label-agreement figure trivially 1.  Run on the
    unprepared module (before SegNet.prepare_inference folds anything); returns the shift applied (the median class margin)."""
    lg = segnet.encode_decode(images).float()
    d = (lg[:, 1] - lg[:, 0]).flatten().median()
    segnet.decode_head.conv_seg.bias[1] -= d.to(segnet.decode_head.conv_seg.bias.dtype)
    return float(d)


def _meta(img_meta):
    """img_metas as the data loader hands them: list[dict], or a DataContainer-like object whose `.data[0]` is that list
    (mmseg/apis/test.py:97)."""
    if hasattr(img_meta, "data") and not isinstance(img_meta, (list, tuple)):
        img_meta = img_meta.data[0]
    return list(img_meta)
