"""TEST INFRASTRUCTURE — plain float64 references, in NHWC, of the convolutions that do NOT run on the GEMM core: GenNet's 24-channel
stride-2 stages and their fused forms (csrc/gennet_conv.hip), the two single-channel 3x3 convolutions (csrc/small_conv.hip) and
SegNet's tokenizer from occupancy codes (csrc/tokenizer_codes.hip).  tests/test_gpu_gennet_conv.py compares every one of those
kernels with these.

Every convolution is an explicit gather: a loop over the nine taps, each a strided slice of the zero-padded input times that tap's
[Cin, Cout] matrix.  No torch.nn.functional.conv* is called, so the reference is independent of the library; tests/test_conv_ref.py
holds it against the library's float64 convolutions on the CPU (1e-12) on any machine.

Besides the value each convolution returns the ROUNDING SCALE of every output element,

    A = sum_taps,ci |w| |x| + |b|,

which is what a float32 accumulation's error is proportional to (tests/_na_ref.py does the same for attention).

Weights are in torch's layouts: Conv2d [Cout, Cin, 3, 3], ConvTranspose2d [Cin, Cout, 3, 3].  A parameter pair is (weight, bias) with
bias None for "no bias", or a module with .weight / .bias.
"""
import types

import torch

BF = torch.bfloat16


def _wb(c):
    w, b = (c.weight, c.bias) if hasattr(c, "weight") else c
    return w.detach().cpu().double(), (None if b is None else b.detach().cpu().double())


def bf16_round(x):
    """x (float64) rounded to the nearest bfloat16 (ties to even), as float64.  The rounding goes through float32, as a kernel's does
    that holds the value in a float32 register; where x is not a float32 number the two roundings can differ from a direct one only
    for an x within a float32 ulp of a bfloat16 tie."""
    return x.to(torch.float32).to(BF).double()


def leaky(x, slope):
    return torch.where(x > 0, x, x * slope)


def conv3x3(x, w, b, stride=1):
    """x [B, H, W, Cin], w [Cout, Cin, 3, 3], b [Cout] or None; zero padding 1 -> (y, A), both [B, Ho, Wo, Cout] float64 with
    Ho = (H - 1) // stride + 1."""
    x, w = x.detach().cpu().double(), w.detach().cpu().double()
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    assert w.shape == (Cout, Cin, 3, 3)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    xp = torch.zeros(B, H + 2, W + 2, Cin, dtype=torch.float64)
    xp[:, 1:H + 1, 1:W + 1] = x
    y = torch.zeros(B, Ho, Wo, Cout, dtype=torch.float64)
    A = torch.zeros_like(y)
    for ky in range(3):
        for kx in range(3):
            # output (oy, ox) reads input (stride * oy + ky - 1, stride * ox + kx - 1): index + 1 on the padded grid
            xs = xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            wt = w[:, :, ky, kx].t()                                       # [Cin, Cout]
            y += xs @ wt
            A += xs.abs() @ wt.abs()
    if b is not None:
        b = b.detach().cpu().double()
        y += b
        A += b.abs()
    return y, A


def conv_transpose3x3_s2(x, w, b):
    """ConvTranspose2d(3, stride 2, padding 1, output_padding 1): x [B, H, W, Cin], w [Cin, Cout, 3, 3] -> (y, A) [B, 2H, 2W, Cout].
    Input (iy, ix) reaches output (2 iy + ky - 1, 2 ix + kx - 1) through tap (ky, kx)."""
    x, w = x.detach().cpu().double(), w.detach().cpu().double()
    B, H, W, Cin = x.shape
    Cout = w.shape[1]
    assert w.shape == (Cin, Cout, 3, 3)
    # row r of the buffer is output row r - 1: rows 0 .. 2H, of which 1 .. 2H are the result (row 0 is cut by the padding)
    y = torch.zeros(B, 2 * H + 2, 2 * W + 2, Cout, dtype=torch.float64)
    A = torch.zeros_like(y)
    for ky in range(3):
        for kx in range(3):
            wt = w[:, :, ky, kx]                                           # [Cin, Cout]
            y[:, ky:ky + 2 * H:2, kx:kx + 2 * W:2] += x @ wt
            A[:, ky:ky + 2 * H:2, kx:kx + 2 * W:2] += x.abs() @ wt.abs()
    y, A = y[:, 1:2 * H + 1, 1:2 * W + 1].contiguous(), A[:, 1:2 * H + 1, 1:2 * W + 1].contiguous()
    if b is not None:
        b = b.detach().cpu().double()
        y += b
        A += b.abs()
    return y, A


def first_enc(x, c1, c2, slope1, slope2):
    """GenNet's first convolution (1 -> C, stride 1) + LeakyReLU, rounded to bfloat16 where the two-kernel path stores it, then the
    first encoder stage (C -> C, stride 2) + LeakyReLU.  x [B, H, W, 1].  Returns a namespace: out, A (of the second convolution, on
    the rounded intermediate), mid (the rounded intermediate) and mid_exact (before its rounding)."""
    (w1, b1), (w2, b2) = _wb(c1), _wb(c2)
    y1, _ = conv3x3(x, w1, b1, 1)
    mid_exact = leaky(y1, slope1)
    mid = bf16_round(mid_exact)
    y2, A = conv3x3(mid, w2, b2, 2)
    return types.SimpleNamespace(out=leaky(y2, slope2), A=A, mid=mid, mid_exact=mid_exact)


def dec_final(x, dec, slope, fin):
    """GenNet's last decoder stage (ConvTranspose2d C -> C) + LeakyReLU, rounded to bfloat16 where the two-kernel path stores it, then
    the final convolution (C -> 1, stride 1).  x [B, H, W, C].  Returns a namespace: out [B, 2H, 2W, 1], A, mid, mid_exact."""
    (wd, bd), (wf, bfin) = _wb(dec), _wb(fin)
    y1, _ = conv_transpose3x3_s2(x, wd, bd)
    mid_exact = leaky(y1, slope)
    mid = bf16_round(mid_exact)
    y2, A = conv3x3(mid, wf, bfin, 1)
    return types.SimpleNamespace(out=y2, A=A, mid=mid, mid_exact=mid_exact)


GRID_FREE, GRID_MARK = 255, 128                                            # include/ppnet_hip.h: PPN_GRID_FREE / PPN_GRID_MARK


def palette_image(codes, mean, std):
    """[B, H, W, 3] float64: the normalised three-colour image of u8 occupancy codes [B, H, W] with its values rounded to bfloat16, as
    the network's input tensor holds them: free = (255, 255, 255), marker = (255, 0, 0), anything else = (0, 0, 0)."""
    codes = codes.detach().cpu()
    norm = lambda v: torch.tensor([(v - m) / s for m, s in zip(mean, std)], dtype=torch.float32).to(BF).double()
    lo, hi = norm(0.0), norm(255.0)
    img = lo.expand(*codes.shape, 3).clone()
    free, mark = codes == GRID_FREE, codes == GRID_MARK
    img[free] = hi
    img[mark] = torch.stack([hi[0], lo[1], lo[2]])
    return img


def layer_norm(x, w, b, eps):
    """Over the last axis, biased variance."""
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w.detach().cpu().double() + b.detach().cpu().double()


def tokenizer(codes, c1, c2, ln_w, ln_b, eps, mean, std):
    """SegNet's tokenizer on the palette image of u8 codes [B, H, W]: convolution (3 -> 64, stride 2), rounded to bfloat16 where the
    two-kernel path stores it, convolution (64 -> 128, stride 2), LayerNorm over the channels.  Returns a namespace: image, conv1 and
    A1 (first convolution and its scale, [B, H/2, W/2, 64]), mid (conv1 rounded), conv2 [B, H/4, W/4, 128], out (after the LayerNorm)."""
    (w1, b1), (w2, b2) = _wb(c1), _wb(c2)
    image = palette_image(codes, mean, std)
    conv1, A1 = conv3x3(image, w1, b1, 2)
    mid = bf16_round(conv1)
    conv2, _ = conv3x3(mid, w2, b2, 2)
    return types.SimpleNamespace(image=image, conv1=conv1, A1=A1, mid=mid, conv2=conv2, out=layer_norm(conv2, ln_w, ln_b, eps))
