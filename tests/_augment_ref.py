"""TEST INFRASTRUCTURE — the definition of SegNet's training-input pipeline restated for the tests, independent of
ppnet_amd/augment.py: the control flow of the reference's PhotoMetricDistortion / RandomFlip / Normalize / Pad
(SegNet/mmseg/datasets/pipelines/transforms.py:835-940, configs/_base_/datasets/planning_seg.py:18-27) on BGR u8 images with the
random decisions passed in, and the project's 8-bit HSV as plain Python integers, one colour at a time."""
import numpy as np

FLIP, BRIGHTNESS, CONTRAST, CONTRAST_LAST, SATURATION, HUE = 1, 2, 4, 8, 16, 32
MEAN = (123.675, 116.28, 103.53)
STD = (58.395, 57.12, 57.375)
LATTICE = [0, 16, 32, 48, 64, 80, 96, 112, 128, 144, 160, 176, 192, 208, 224, 240, 255]


def bgr2hsv_px(b, g, r):
    v, m = max(b, g, r), min(b, g, r)
    d = v - m
    s = (2 * 255 * d + v) // (2 * v) if v else 0
    if v == r:
        n = g - b
    elif v == g:
        n = b - r + 2 * d
    else:
        n = r - g + 4 * d
    if n < 0:
        n += 6 * d
    h = ((60 * n + d) // (2 * d)) % 180 if d else 0
    return h, s, v


def hsv2bgr_px(h, s, v):
    rd = lambda a, b: (2 * a + b) // (2 * b)
    sec, f = divmod(h, 30)
    p, q, t = rd(v * (255 - s), 255), rd(v * (7650 - s * f), 7650), rd(v * (7650 - s * (30 - f)), 7650)
    r, g, b = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)][sec]
    return b, g, r


def _per_colour(img, fn):
    """fn (b, g, r) -> (x, y, z) applied to an [..., 3] u8 image through its distinct colours."""
    flat = img.reshape(-1, 3)
    colours, inverse = np.unique(flat, axis=0, return_inverse=True)
    mapped = np.array([fn(*(int(c) for c in col)) for col in colours], dtype=np.uint8).reshape(-1, 3)
    return mapped[inverse.reshape(-1)].reshape(img.shape)


def bgr2hsv(img):
    return _per_colour(img, bgr2hsv_px)


def hsv2bgr(img):
    return _per_colour(img, hsv2bgr_px)


def convert(img, alpha=1, beta=0):
    img = img.astype(np.float32) * np.float32(alpha) + np.float32(beta)
    img = np.clip(img, 0, 255)
    return img.astype(np.uint8)


def photometric(img, flags, beta, alpha, alpha_s, delta):
    """PhotoMetricDistortion.__call__ on a BGR u8 image; each `random.randint(2)` is a flag bit, each drawn value an argument."""
    if flags & BRIGHTNESS:
        img = convert(img, beta=beta)
    mode = 0 if flags & CONTRAST_LAST else 1
    if mode == 1 and flags & CONTRAST:
        img = convert(img, alpha=alpha)
    if flags & SATURATION:
        img = bgr2hsv(img)
        img[:, :, 1] = convert(img[:, :, 1], alpha=alpha_s)
        img = hsv2bgr(img)
    if flags & HUE:
        img = bgr2hsv(img)
        img[:, :, 0] = (img[:, :, 0].astype(int) + int(delta)) % 180
        img = hsv2bgr(img)
    if mode == 0 and flags & CONTRAST:
        img = convert(img, alpha=alpha)
    return img


def render(codes):
    """BGR u8 palette image of occupancy codes: free (255) white, marker (128) red, anything else black."""
    img = np.zeros(codes.shape + (3,), dtype=np.uint8)
    img[codes == 255] = 255
    img[codes == 128] = (0, 0, 255)
    return img


def pipeline(bgr, label, flags, beta, alpha, alpha_s, delta, out_hw=None, seg_pad_val=255):
    """One image through flip -> distortion -> normalise (to RGB) -> pad: (float32 [Ho, Wo, 3], u8 [Ho, Wo] or None)."""
    if flags & FLIP:
        bgr = np.flip(bgr, axis=1)
        label = None if label is None else np.flip(label, axis=1)
    img = photometric(np.ascontiguousarray(bgr), flags, np.float32(beta), np.float32(alpha), np.float32(alpha_s), delta)
    rgb = (img[:, :, ::-1].astype(np.float32) - np.asarray(MEAN, np.float32)) / np.asarray(STD, np.float32)
    H, W = rgb.shape[:2]
    Ho, Wo = out_hw or (H, W)
    out = np.zeros((Ho, Wo, 3), dtype=np.float32)
    out[:H, :W] = rgb
    lab = None
    if label is not None:
        lab = np.full((Ho, Wo), seg_pad_val, dtype=np.uint8)
        lab[:H, :W] = label
    return out, lab


def batch(src, labels, params, out_hw=None):
    """`pipeline` over a batch: src u8 codes [B,H,W] or RGB images [B,H,W,3]; params rows (flags, beta, alpha, alpha_s, delta)."""
    imgs, labs = [], []
    for i, (flags, beta, alpha, alpha_s, delta) in enumerate(params):
        bgr = render(src[i]) if src.ndim == 3 else src[i][:, :, ::-1]
        o, l = pipeline(bgr, None if labels is None else labels[i], int(flags), beta, alpha, alpha_s, int(delta), out_hw)
        imgs.append(o)
        labs.append(l)
    return np.stack(imgs), None if labels is None else np.stack(labs)


def lattice_colours():
    """[4913, 3] u8: the 17-level lattice."""
    g = np.array(LATTICE, dtype=np.uint8)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def words(params):
    """int32 [B, 8] parameter words (ppn_augment_params' layout) of rows (flags, beta, alpha, alpha_s, delta)."""
    w = np.zeros((len(params), 8), dtype=np.int32)
    for i, (flags, beta, alpha, alpha_s, delta) in enumerate(params):
        w[i, 0] = flags
        w[i, 1:4] = np.array([beta, alpha, alpha_s], dtype=np.float32).view(np.int32)
        w[i, 4] = delta
    return w


def drawn(seed, instance, flip_ratio=0.5, db=32.0, contrast=(0.5, 1.5), saturation=(0.5, 1.5), dh=18):
    """(flags, beta, alpha, alpha_s, delta) of one image from the oracle's Philox draws, slot by slot."""
    import math
    from oracle import philox_np
    u = [float(x) for x in philox_np.doubles(seed, 5, instance, 0, 10)]
    flags = (FLIP * (u[0] < flip_ratio) | BRIGHTNESS * (u[1] < 0.5) | CONTRAST_LAST * (not u[3] < 0.5) | CONTRAST * (u[4] < 0.5) |
             SATURATION * (u[6] < 0.5) | HUE * (u[8] < 0.5))
    return (int(flags), np.float32(-db + 2 * db * u[2]), np.float32(contrast[0] + (contrast[1] - contrast[0]) * u[5]),
            np.float32(saturation[0] + (saturation[1] - saturation[0]) * u[7]), -dh + math.floor(2 * dh * u[9]))


# ------------------------------------------------------------------------------------------------ shared fixtures
SEED = 2024                     # tests/test_augment.py::test_draw_statistics checks the bounds for this seed from the oracle alone


def param_rows():
    """64 images, one per flag combination, with extreme and interior values."""
    betas, alphas, deltas = (32.0, -32.0, 7.3), (0.5, 1.5, 0.77), (-18, 17, 5)
    return [(f, betas[f % 3], alphas[(f // 3) % 3], alphas[(f // 9) % 3], deltas[(f // 2) % 3]) for f in range(64)]


def palette_codes(B, H, W, seed=0):
    g = np.random.RandomState(seed)
    return np.array([0, 128, 255, 7], dtype=np.uint8)[g.randint(0, 4, (B, H, W))]


# the tiny DiNAT + SETR-UP + FCN auxiliary head of tests/test_gpu_resize_ce.py (stochastic depth and dropout at 0)
TINY_SEG = dict(
    backbone=dict(embed_dim=32, mlp_ratio=2.0, depths=[1, 1, 2, 1], num_heads=[1, 2, 4, 8], kernel_size=7, layer_scale=1e-1,
                  dilations=[[1], [2], [1, 2], [1]], drop_path_rate=0.0),
    decode_head=dict(in_channels=256, channels=32, num_convs=4, up_scale=2, num_classes=2, kernel_size=3, dropout_ratio=0.0))
TINY_AUX = dict(type="FCNHead", in_channels=128, in_index=2, channels=32, num_convs=1, concat_input=False, dropout_ratio=0.0,
                num_classes=2, align_corners=False, loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=0.4))
