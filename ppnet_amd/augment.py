"""SegNet's training input: the reference's train_pipeline (SegNet/configs/_base_/datasets/planning_seg.py:18-27) RandomFlip(0.5) ->
PhotoMetricDistortion -> Normalize -> Pad(size, pad_val 0, seg_pad_val 255) for a batch of generated maps (u8 occupancy codes
[B,H,W]) or of u8 RGB images [B,H,W,3], image and labels together.

On the GPU: ppn_augment_params draws the per-image parameters, ppn_augment_codes / ppn_augment_rgb apply them (csrc/augment.hip,
through fused).  On the CPU the same definition in NumPy, bit for bit (convert = float32(x) * alpha + beta in two
rounded float32 operations, clipped, truncated; 8-bit HSV in exact integers with round-half-up; draws from Philox stream 5 with the
global image index as the instance), so that CPU training and the CPU tests run.
"""
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import fused, philox

FLIP, BRIGHTNESS, CONTRAST, CONTRAST_LAST, SATURATION, HUE = (fused.AUG_FLIP, fused.AUG_BRIGHTNESS, fused.AUG_CONTRAST,
                                                             fused.AUG_CONTRAST_LAST, fused.AUG_SATURATION, fused.AUG_HUE)
DRAWS = 10                                # draw slots per image (include/ppnet_hip.h: ppn_augment_params)


@dataclass
class SegAugment:
    """Settings of the pipeline, the reference's defaults (transforms.py:855-859; RandomFlip prob 0.5).  out_size (Ho, Wo) >= the
    map's size pads to the reference's crop_size (None: no padding); seed keys the Philox draws."""
    flip_ratio: float = 0.5
    brightness_delta: float = 32.0
    contrast_range: Tuple[float, float] = (0.5, 1.5)
    saturation_range: Tuple[float, float] = (0.5, 1.5)
    hue_delta: int = 18
    out_size: Optional[Tuple[int, int]] = None
    seg_pad_val: int = 255
    seed: int = 0


def pack_params(flags, beta, alpha, alpha_s, delta):
    """int32 [B, 8] parameter words from per-image sequences (the float32 values are stored as their bits)."""
    B = len(flags)
    words = np.zeros((B, fused.AUG_PARAM_WORDS), dtype=np.int32)
    words[:, 0] = np.asarray(flags, dtype=np.int32)
    for col, v in ((1, beta), (2, alpha), (3, alpha_s)):
        words[:, col] = np.asarray(v, dtype=np.float32).view(np.int32)
    words[:, 4] = np.asarray(delta, dtype=np.int32)
    return torch.from_numpy(words)


def draw_params(aug, first_instance, B, device):
    """int32 [B, 8] on `device`: the parameters of images first_instance .. first_instance + B - 1."""
    device = torch.device(device)
    if device.type == "cuda":
        return fused.augment_params(aug.seed, first_instance, B, device, aug.flip_ratio, aug.brightness_delta, aug.contrast_range,
                                    aug.saturation_range, aug.hue_delta)
    flags, beta, alpha, alpha_s, delta = [], [], [], [], []
    (clo, chi), (slo, shi), db, dh = aug.contrast_range, aug.saturation_range, float(aug.brightness_delta), int(aug.hue_delta)
    for b in range(B):
        d = [float(v) for v in philox.doubles_host(aug.seed, philox.STREAM_AUG, first_instance + b, 0, DRAWS)]
        flags.append((FLIP if d[0] < aug.flip_ratio else 0) | (BRIGHTNESS if d[1] < 0.5 else 0) | (0 if d[3] < 0.5 else CONTRAST_LAST) |
                     (CONTRAST if d[4] < 0.5 else 0) | (SATURATION if d[6] < 0.5 else 0) | (HUE if d[8] < 0.5 else 0))
        beta.append(-db + (2.0 * db) * d[2])
        alpha.append(clo + (chi - clo) * d[5])
        alpha_s.append(slo + (shi - slo) * d[7])
        delta.append(-dh + math.floor((2 * dh) * d[9]))
    return pack_params(flags, beta, alpha, alpha_s, delta)


# ------------------------------------------------------------------------------------------------ the definition in NumPy
def _convert(x, alpha, beta):
    f = x.astype(np.float32) * np.float32(alpha) + np.float32(beta)
    return np.clip(f, 0, 255).astype(np.uint8).astype(np.int64)


def _bgr2hsv(b, g, r):
    v = np.maximum(r, np.maximum(g, b))
    d = v - np.minimum(r, np.minimum(g, b))
    s = np.where(v > 0, (2 * 255 * d + v) // np.maximum(2 * v, 1), 0)
    n = np.where(v == r, g - b, np.where(v == g, b - r + 2 * d, r - g + 4 * d))
    n = np.where(n < 0, n + 6 * d, n)
    h = np.where(d > 0, ((60 * n + d) // np.maximum(2 * d, 1)) % 180, 0)
    return h, s, v


def _hsv2bgr(h, s, v):
    sec, f = h // 30, h % 30
    p = (2 * v * (255 - s) + 255) // 510
    q = (2 * v * (7650 - s * f) + 7650) // 15300
    t = (2 * v * (7650 - s * (30 - f)) + 7650) // 15300
    r = np.choose(sec, [v, q, p, p, t, v])
    g = np.choose(sec, [t, v, v, q, p, p])
    b = np.choose(sec, [p, p, t, v, v, q])
    return b, g, r


def _distort(b, g, r, flags, beta, alpha, alpha_s, delta):
    """PhotoMetricDistortion.__call__ (transforms.py:909-940) on int64 BGR arrays of one image."""
    if flags & BRIGHTNESS:
        b, g, r = (_convert(c, 1.0, beta) for c in (b, g, r))
    if flags & CONTRAST and not flags & CONTRAST_LAST:
        b, g, r = (_convert(c, alpha, 0.0) for c in (b, g, r))
    if flags & SATURATION:
        h, s, v = _bgr2hsv(b, g, r)
        b, g, r = _hsv2bgr(h, _convert(s, alpha_s, 0.0), v)
    if flags & HUE:
        h, s, v = _bgr2hsv(b, g, r)
        b, g, r = _hsv2bgr((h + delta) % 180, s, v)
    if flags & CONTRAST and flags & CONTRAST_LAST:
        b, g, r = (_convert(c, alpha, 0.0) for c in (b, g, r))
    return b, g, r


def _apply_cpu(params, src, labels, mean, std, dtype, out_size, seg_pad_val):
    if params.dtype != torch.int32 or (labels is not None and labels.dtype != torch.uint8):
        raise ValueError("augment: uint8 input and labels, int32 parameters")
    B, H, W = src.shape[:3]
    if tuple(params.shape) != (B, fused.AUG_PARAM_WORDS) or (labels is not None and tuple(labels.shape) != (B, H, W)):
        raise ValueError(f"augment: parameters {tuple(params.shape)} / labels {None if labels is None else tuple(labels.shape)} do not "
                         f"belong to a batch of {B} images of {H} x {W}")
    words = params.contiguous().numpy()
    x = src.contiguous().numpy()
    codes = x.ndim == 3
    Ho, Wo = (H, W) if out_size is None else out_size
    if W % 8 or Wo % 8 or Ho < H or Wo < W:
        raise ValueError(f"augment: widths are multiples of 8 and out_size {Ho, Wo} covers the map {H, W}")
    mean32, std32 = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
    img = np.zeros((B, Ho, Wo, 3), dtype=np.float32)
    lab = None if labels is None else np.full((B, Ho, Wo), seg_pad_val & 0xff, dtype=np.uint8)
    for i in range(B):
        flags = int(words[i, 0])
        beta, alpha, alpha_s = (float(v) for v in words[i, 1:4].view(np.float32))
        if codes:                                           # ppn_grid_to_image's palette as BGR planes
            free, mark = x[i] == 255, x[i] == 128
            r = np.where(free | mark, 255, 0).astype(np.int64)
            g = b = np.where(free, 255, 0).astype(np.int64)
        else:
            r, g, b = (x[i, :, :, c].astype(np.int64) for c in range(3))
        b, g, r = _distort(b, g, r, flags, beta, alpha, alpha_s, int(words[i, 4]))
        rgb = (np.stack([r, g, b], axis=-1).astype(np.float32) - mean32) / std32
        if flags & FLIP:
            rgb = rgb[:, ::-1]
        img[i, :H, :W] = rgb
        if lab is not None:
            li = labels[i].numpy()
            lab[i, :H, :W] = li[:, ::-1] if flags & FLIP else li
    return torch.from_numpy(img).to(dtype).permute(0, 3, 1, 2), None if lab is None else torch.from_numpy(lab)


def apply(aug, params, grid_or_rgb, labels, mean, std, dtype):
    """(image: channels_last [B,3,Ho,Wo] of `dtype`, labels u8 [B,Ho,Wo] or None) of u8 occupancy codes [B,H,W] or u8 RGB images
    [B,H,W,3] under the per-image parameters `params` (draw_params).  One kernel on the GPU; the NumPy definition on the CPU."""
    if grid_or_rgb.dtype != torch.uint8 or grid_or_rgb.dim() not in (3, 4):
        raise ValueError(f"augment.apply: uint8 codes [B,H,W] or RGB images [B,H,W,3], got {grid_or_rgb.dtype} {tuple(grid_or_rgb.shape)}")
    if grid_or_rgb.is_cuda:
        run = fused.augment_codes if grid_or_rgb.dim() == 3 else fused.augment_rgb
        return run(grid_or_rgb, labels, params, mean, std, dtype, aug.out_size, aug.seg_pad_val)
    if grid_or_rgb.dim() == 4 and grid_or_rgb.shape[-1] != 3:
        raise ValueError(f"augment.apply: [B,H,W,3] images, got {tuple(grid_or_rgb.shape)}")
    return _apply_cpu(params, grid_or_rgb, labels, mean, std, dtype, aug.out_size, aug.seg_pad_val)


# ------------------------------------------------------------------------------------------------ test-time augmentation
class MultiScaleFlipAug:
    """mmseg's MultiScaleFlipAug (datasets/pipelines/test_time_aug.py) with the transforms of the reference's `--aug-test`
    (SegNet/test.py:142-147: img_ratios [0.5, 0.75, 1.0, 1.25, 1.5, 1.75], flip True) for a batch on its device: calling it on a
    normalised batch [B,3,H,W] — or on u8 occupancy codes [B,H,W], rendered with fused.grid_to_image (GPU) in `dtype` — returns
    (imgs, img_metas), the two lists SegNet.forward(return_loss=False, img=imgs, img_metas=img_metas) takes.  Order as the
    reference's loops (:112-115): scale-major, unflipped before flipped, one entry per direction.  Sizes are (int(H * ratio),
    int(W * ratio)) (:73-75); an entry is F.interpolate(bilinear, align_corners=False) of the batch, then its flip.  Each entry's
    metas (one dict per image) carry ori_shape, img_shape, pad_shape (H, W, 3 triples), scale_factor (float32 [4]: w, h, w, h),
    flip and flip_direction.  Library ops only: a cold path of a dozen small resizes.

    resize=False reproduces the test pipeline of configs/_base_/datasets/planning_seg.py as written: it has no Resize step, so under
    `--aug-test` the ratios do not change the image — six ratios give six equal copies, each unflipped and flipped, and the merged
    result is plain flip averaging."""

    def __init__(self, img_ratios=(0.5, 0.75, 1.0, 1.25, 1.5, 1.75), flip=True, flip_direction="horizontal", resize=True):
        self.img_ratios = [float(r) for r in (img_ratios if isinstance(img_ratios, (list, tuple)) else [img_ratios])]
        self.flip = bool(flip)
        self.flip_direction = list(flip_direction) if isinstance(flip_direction, (list, tuple)) else [flip_direction]
        self.resize = bool(resize)
        if not self.img_ratios or min(self.img_ratios) <= 0:
            raise ValueError(f"MultiScaleFlipAug: img_ratios {self.img_ratios}")
        if any(d not in ("horizontal", "vertical") for d in self.flip_direction):
            raise ValueError(f"MultiScaleFlipAug: flip_direction {self.flip_direction}")

    def __len__(self):
        return len(self.img_ratios) * (2 if self.flip else 1) * len(self.flip_direction)

    def __call__(self, img, dtype=torch.float32):
        if img.dtype == torch.uint8 and img.dim() == 3:
            from .dense import IMG_MEAN, IMG_STD
            img = fused.grid_to_image(img, IMG_MEAN, IMG_STD, dtype)
        if img.dim() != 4 or not img.is_floating_point():
            raise ValueError(f"MultiScaleFlipAug: a normalised batch [B,3,H,W] or u8 codes [B,H,W], got {img.dtype} {tuple(img.shape)}")
        B, ch, H, W = img.shape
        imgs, img_metas = [], []
        for ratio in self.img_ratios:
            h, w = (int(H * ratio), int(W * ratio)) if self.resize else (H, W)
            if h < 1 or w < 1:
                raise ValueError(f"MultiScaleFlipAug: ratio {ratio} of {H} x {W} is empty")
            scaled = img if (h, w) == (H, W) else torch.nn.functional.interpolate(img, (h, w), mode="bilinear", align_corners=False)
            for flip in ([False, True] if self.flip else [False]):
                for direction in self.flip_direction:
                    imgs.append(scaled.flip(3 if direction == "horizontal" else 2) if flip else scaled)
                    meta = {"ori_shape": (H, W, ch), "img_shape": (h, w, ch), "pad_shape": (h, w, ch),
                            "scale_factor": np.array([w / W, h / H, w / W, h / H], dtype=np.float32), "flip": flip,
                            "flip_direction": direction}
                    img_metas.append([dict(meta) for _ in range(B)])
        return imgs, img_metas
