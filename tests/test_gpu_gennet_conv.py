"""The convolutions that do NOT run on the GEMM core, every kernel against the float64 gather references of tests/_conv_ref.py
(themselves held against the library's float64 convolutions by tests/test_conv_ref.py) at the smallest shapes where their index code
can go wrong:

    enc       gennet_enc_conv_kernel      csrc/gennet_conv.hip     fused.gennet_conv_s2(transposed=False)   gennet.pack_s2_weights
    dec       gennet_dec_conv_kernel                               fused.gennet_conv_s2(transposed=True)    gennet.pack_s2_weights
    first     gennet_first_enc_kernel                              fused.gennet_first_enc                   gennet.pack_first_enc_weights
    decfinal  gennet_dec_final_kernel                              fused.gennet_dec_final                   gennet.pack_s2_weights
    c1        conv3x3_c1_kernel<T, CG>    csrc/small_conv.hip      fused.conv3x3_c1
    to1       conv3x3_to1_mfma_kernel / conv3x3_to1_kernel<T, CG>  fused.conv3x3_to1
    tok1      tokenizer_codes_kernel      csrc/tokenizer_codes.hip fused.tokenizer_conv1_codes              fused.tokenizer_lut
    tokf      tokenizer_fused_kernel                               fused.tokenizer_codes                    fused.tokenizer_lut, tokenizer_pack

Every kernel is reached through its wrapper with parameters packed by the project's packers, which are therefore under test too.

(a) EXACT.  Inputs in {-1, 0, 1} (variant pm1, slopes 1) or {0, 1} (GenNet's mask, slopes 0.5), weights in {-1, 0, 1}, small integer
    biases: every partial sum is exact in float32 and the float64 result is a bfloat16 number, which the test asserts on the REFERENCE
    (want.to(bfloat16) == want, and the same for the intermediate of the two fused kernels) before it asserts equality of every output
    element.  For the two fused kernels the weights of the stage in front are thinned until that holds (_DENSITIES);
    test_exact_first_stage_draws_cover_every_weight_slot asserts that the thinned draws still reach every slot of the packed weights.
    One wrong tap, lane, image base or weight slot changes an integer.  In these variants every lo fragment of a hi + lo weight split
    is zero; variant "split" (SPLIT_LSB below) makes them count.  The tokenizer ends in a LayerNorm and has no exact form.
(b) FLOAT64, unit-normal data, a bound per ELEMENT.  A kernel that accumulates exact bfloat16 products in float32 and rounds once:

        |got - want| <= 2^-8 |want| + 2 n 2^-24 A,      A = sum |w| |x| + |b| from the reference,

    n the reduction length with the bias (enc 217, dec 97, c1 10, to1 9 Cin + 1); float32 output has no 2^-8 term.  2^-8 is
    bfloat16's unit roundoff; n 2^-24 A bounds n float32 roundings of partial sums of magnitude <= A; the factor 2 covers the matrix
    core's own summation order and the LeakyReLU product.  The matrix-core to1 kernel with float32 weights that are not bfloat16
    numbers multiplies by hi + lo fragments (16 significand bits): + 2^-17 A.  The two-stage kernels (first, decfinal, tok1, tokf)
    keep the measured bounds of their tests in tests/test_gpu_mfma.py, unchanged, on the same kind of parameters (the modules'
    default initialisation in bfloat16): a float32-vs-float64 difference can flip the bfloat16 rounding of the intermediate, which no
    A-proportional bound of the second stage covers.
(c) LOOP WRAPS.  Every output pixel is one MFMA column of its own, so a batch's result is bit-equal to the concatenation of its
    chunks' results.  B is sized from the launcher's cap (CAPS below restates them; cus = the device's CU count) so that the
    grid-stride / persistent loop makes a second trip that ends in the middle of a group; the chunks do not wrap.  The first image,
    the last one and the one holding the wrap point are also held to float64 with the bound of (b).
(d) GUARDS, through the C ABI: every input sits inside a larger allocation filled with 3.0e4 (code grids: the marker code), the output
    inside a sentinel-filled one.  The sentinels survive and the result still meets (a) ((b) for the tokenizer) — which pins the
    clamped addresses of dead lanes (pix = total - 1, cx = min(max(ix, 0), W - 2), the zero line).  The guards are part of the
    allocations: no test reads or writes outside one.

WHICH to1 KERNEL RUNS is decided by conv3x3_to1_launch from dtype, Cin and PPNET_TO1_VALU, which it reads ONCE per process: the
bfloat16 Cin = 24 direct form runs in a child process of its own; this process must not have the knob set.

MEASURED on MI355X, worst err / bound over the shapes of a kernel — see DESIGN.md, "Convolution kernels off the GEMM core".
"""
import ctypes
import functools
import os
import subprocess
import sys
import tempfile
import types
import zlib

import pytest

torch = pytest.importorskip("torch")

from tests import _conv_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG_MEAN, IMG_STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)       # ppnet_amd.dense; test_palette_constants holds them equal
SLOPE_B = float(torch.tensor(0.01, dtype=F32))                              # the float32 the kernel multiplies by, for the reference

CONTROL = (2, 16, 16)
_EVEN = [(1, 2, 2), (5, 2, 2), (3, 6, 6), (7, 10, 6), (2, 2, 34), (2, 34, 2), CONTROL]
SHAPES = {
    "enc": _EVEN,                                    # input H x W, even: 1 output pixel; one group over 5 images; 9 and 15 pixels per
    "first": _EVEN,                                  # image (groups and the double group straddle); a tail; one output row / column
    "dec": [(1, 1, 1), (17, 1, 1), (3, 3, 5), (2, 1, 7), (2, 7, 1), (3, 9, 21), CONTROL],       # group + tail over 17 images; row; column
    "decfinal": [(1, 1, 1), (3, 1, 1), (1, 8, 16), (2, 9, 17), (2, 3, 5), CONTROL],             # one 32 x 16 tile exactly; one past it
    "to1_mfma": [(1, 1, 1), (1, 16, 32), (2, 17, 33), (2, 1, 40), (2, 40, 1), CONTROL],         # one tile; one past; row; column
    "to1_valu": [(2, 1, 1), CONTROL, (3, 17, 5)],
    "c1": [(1, 1, 1), (1, 1, 257), (100, 3, 3), CONTROL],                    # a row crossing a 256-thread block; blocks spanning images
    "tok1": [(1, 2, 32), (3, 6, 32), (2, 2, 64), (2, 8, 96), (2, 16, 64)],   # W % 32 == 0: the aligned control is 16 x 64
    "tokf": [(1, 4, 64), (3, 4, 64), (2, 8, 128), (2, 12, 64), (2, 16, 64)],  # W % 64 == 0
}
TO1_VALU_CONFIGS = [("float32", 8), ("float32", 16), ("float32", 24), ("float32", 32), ("bfloat16", 8), ("bfloat16", 16), ("bfloat16", 32)]
TO1_CHILD_SHAPES = SHAPES["to1_mfma"] + [(3, 17, 5)]                        # bfloat16 Cin = 24 on the direct kernel (16 x 16 tiles)
VARIANTS = {"pm1": ("pm1", 1.0), "mask": ("mask", 0.5)}                     # input alphabet, slope(s)
_DENSITIES = (1.0, 0.5, 0.25, 0.125, 0.0625)
# Variant "split" of (a), for the kernels that take float32 weights as hi + lo bfloat16 fragments (first: the first convolution and
# its bias; decfinal and the matrix-core to1: the 24 -> 1 convolution): those weights are k + j 2^-9 with independent small integers
# k and j in {-1, 0, 1}, so hi is (about) k and lo = +-2^-9 is NOT zero as it is in the integer variants.  Every product and float32
# partial sum is still exact (asserted on the reference), so the kernel's output is the exact sum rounded ONCE to bfloat16 — the
# reference rounded the same way.
SPLIT_LSB = 2.0 ** -9

# The launchers' loop caps, in units of work per sweep of the grid, and a shape that wraps them: (H, W, units per image, cap, the
# granularity a sweep must not end on).  gennet_conv.hip: encoder 4096 blocks x 4 waves x 32 pixels; first stage 3072 blocks x 4 waves
# x 16 pixels; decoder 2048 blocks x 4 waves x 16 positions; dec_final 2 cus tiles of 32 x 16 outputs.  tokenizer_codes.hip:
# tokenizer_codes 4096 blocks x 4 groups of 16 pixels; tokenizer_fused cus blocks x 8 groups of 16 tokens.
CAPS = {
    "enc": lambda cus: (126, 126, 63 * 63, 4096 * 128, 32),
    "first": lambda cus: (126, 126, 63 * 63, 3072 * 64, 16),
    "dec": lambda cus: (63, 63, 63 * 63, 2048 * 64, 16),
    "decfinal": lambda cus: (36, 40, 5 * 3, 2 * cus, 1),                     # 72 x 80 outputs: 4.5 x 2.5 tiles, ragged both ways
    "tok1": lambda cus: (62, 96, 31 * 3, 4096 * 4, 4),
    "tokf": lambda cus: (36, 128, 9 * 2, cus * 8, 8),
}


def _sid(s):
    return "x".join(str(v) for v in s)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _alphabet(g, alpha, *shape):
    return _ints(g, -1, 1, *shape) if alpha == "pm1" else _ints(g, 0, 1, *shape)


def _thin(g, w, density):
    return w if density >= 1.0 else w * (torch.rand(w.shape, generator=g) < density)


def _is(dtype, t):
    """t (float64) holds numbers of dtype only."""
    return bool((t.to(F32).to(dtype).double() == t).all())


def _conv(w, b, stride=1, transposed=False, dtype=F32):
    import torch.nn as nn
    m = nn.ConvTranspose2d(w.shape[0], w.shape[1], 3, 2, 1, output_padding=1) if transposed else nn.Conv2d(w.shape[1], w.shape[0], 3, stride, 1)
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(b)
    return m.to(dtype)


# ------------------------------------------------------------------------------------------------ cases: parameters, packed and raw
def _pack(kernel, raw):
    """The kernel's packed parameter tensors, by the project's packers, from the raw (weight, bias) pairs of the case."""
    from ppnet_amd import fused, gennet
    if kernel in ("enc", "dec"):
        wp, bp = gennet.pack_s2_weights(_conv(*raw["conv"], stride=2, transposed=kernel == "dec"))
        return dict(wp=wp, bp=bp)
    if kernel == "first":
        w1, b1, wk2, b2 = gennet.pack_first_enc_weights(_conv(*raw["c1"]), _conv(*raw["c2"], stride=2))
        return dict(w1=w1, b1=b1, wk2=wk2, b2=b2)
    if kernel == "decfinal":
        wp, bp = gennet.pack_s2_weights(_conv(*raw["dec"], transposed=True))
        return dict(wp=wp, bp=bp, wf=raw["fin"][0].to(F32).contiguous(), bias_f=float(raw["fin"][1][0]))
    if kernel == "c1":
        return dict(w=raw["conv"][0].to(F32).contiguous(), b=raw["conv"][1].to(F32).contiguous())
    if kernel == "to1":
        return dict(w=raw["conv"][0].to(F32).contiguous(), bias_f=float(raw["conv"][1][0]))
    lut = fused.tokenizer_lut(_conv(*raw["c1"], stride=2, dtype=BF), IMG_MEAN, IMG_STD)
    if kernel == "tok1":
        return dict(lut=lut)
    import torch.nn as nn
    ln = nn.LayerNorm(128)
    with torch.no_grad():
        ln.weight.copy_(raw["ln"][0])
        ln.bias.copy_(raw["ln"][1])
    w2p, vec = fused.tokenizer_pack(_conv(*raw["c2"], stride=2, dtype=BF), ln.to(BF))
    return dict(lut=lut, w2p=w2p, vec=vec, eps=ln.eps)


def _reference(kernel, c, x=None):
    """The float64 reference of case c on input x (default: the case's own): a namespace with out (NHWC) and what the bounds need."""
    raw = c.raw
    x = (c.inp["grid"] if kernel in ("tok1", "tokf") else c.inp["x"]) if x is None else x
    x = x.detach().cpu()
    if kernel in ("enc", "dec"):
        y, A = R.conv_transpose3x3_s2(x, *raw["conv"]) if kernel == "dec" else R.conv3x3(x, *raw["conv"], 2)
        return types.SimpleNamespace(out=R.leaky(y, c.inp["slope"]), A=A)
    if kernel == "first":
        return R.first_enc(x.unsqueeze(-1), raw["c1"], raw["c2"], c.inp["slope1"], c.inp["slope2"])
    if kernel == "decfinal":
        return R.dec_final(x, raw["dec"], c.inp["slope"], raw["fin"])
    if kernel == "c1":
        y, A = R.conv3x3(x.unsqueeze(-1), *raw["conv"], 1)
        return types.SimpleNamespace(out=R.leaky(y, c.inp["slope"]), A=A)
    if kernel == "to1":
        y, A = R.conv3x3(x, *raw["conv"], 1)
        return types.SimpleNamespace(out=y, A=A)
    r = R.tokenizer(x, raw["c1"], raw["c2"], *raw["ln"], 1e-5, IMG_MEAN, IMG_STD)
    if kernel == "tok1":
        return types.SimpleNamespace(out=r.conv1, A=r.A1, image=r.image)
    return r


def _case(kernel, raw, inp, out_dtype=BF):
    c = types.SimpleNamespace(kernel=kernel, raw=raw, inp=dict(inp, **_pack(kernel, raw)), out_dtype=out_dtype)
    c.ref = _reference(kernel, c)
    return c


@functools.lru_cache(maxsize=None)
def _exact_case(kernel, variant, shape, dtype_name="bfloat16", C=24):
    """(a).  Returns the case of the densest draw whose reference is exact in the output dtype, with .density and .exact set.
    variant "split" (first, decfinal, to1): see SPLIT_LSB; its reference is rounded once to bfloat16, as the kernel's exact sum is."""
    B, H, W = shape
    split = variant == "split"
    alpha, slope = ("mask", 0.5) if split else VARIANTS[variant]
    sw = (lambda lo, hi, *sh: _ints(g, lo, hi, *sh) + SPLIT_LSB * _ints(g, -1, 1, *sh)) if split else (lambda lo, hi, *sh: _ints(g, lo, hi, *sh))
    dtype = getattr(torch, dtype_name)
    for density in (_DENSITIES[2:] if split and kernel != "to1" else _DENSITIES):
        g = _gen("exact", kernel, variant, shape, dtype_name, C, density)
        if kernel in ("enc", "dec"):
            raw = dict(conv=(_ints(g, -1, 1, 24, 24, 3, 3), _ints(g, -3, 3, 24)))
            c = _case(kernel, raw, dict(x=_alphabet(g, alpha, B, H, W, 24).to(BF), slope=slope))
        elif kernel == "first":
            raw = dict(c1=(sw(-1, 1, 24, 1, 3, 3), sw(-2, 2, 24)), c2=(_thin(g, _ints(g, -1, 1, 24, 24, 3, 3), density), _ints(g, -3, 3, 24)))
            c = _case(kernel, raw, dict(x=_alphabet(g, alpha, B, H, W).to(BF), slope1=slope, slope2=slope))
        elif kernel == "decfinal":
            raw = dict(dec=(_thin(g, _ints(g, -1, 1, 24, 24, 3, 3), density), _ints(g, -1, 1, 24)), fin=(sw(-1, 1, 1, 24, 3, 3), sw(-3, 3, 1)))
            c = _case(kernel, raw, dict(x=_alphabet(g, alpha, B, H, W, 24).to(BF), slope=slope))
        elif kernel == "c1":
            raw = dict(conv=(_ints(g, -3, 3, C, 1, 3, 3), _ints(g, -3, 3, C)))
            c = _case(kernel, raw, dict(x=(2 * _alphabet(g, alpha, B, H, W)).to(dtype), slope=slope), dtype)
        else:
            assert kernel == "to1"
            raw = dict(conv=(sw(-1, 1, 1, C, 3, 3), sw(-3, 3, 1)))
            c = _case(kernel, raw, dict(x=_alphabet(g, alpha, B, H, W, C).to(dtype)), dtype)
        c.density = density
        r = c.ref
        if split:
            # every float32 partial sum is exact in any order: multiples of 2^-11 below 2^12; the first stage's intermediate is the
            # rounding of an exact float32 (multiples of 2^-10 below 2^5), the decoder's is a bfloat16 number as in the other variants
            fine = lambda t, lsb: bool((t * 2.0 ** lsb == (t * 2.0 ** lsb).round()).all())
            c.exact = fine(r.out, 11) and float(r.A.max()) < 2.0 ** 12 and (
                kernel == "to1" or (fine(r.mid_exact, 10) if kernel == "first" else torch.equal(r.mid, r.mid_exact)))
            c.lo_matters = int((R.bf16_round(r.out) != R.bf16_round(_reference(kernel, _hi_only(c)).out)).sum())
            r.out = R.bf16_round(r.out)
        else:
            c.exact = _is(c.out_dtype, r.out) and (not hasattr(r, "mid") or torch.equal(r.mid, r.mid_exact))
        if c.exact or kernel not in ("first", "decfinal"):
            break
    return c


def _hi_only(c):
    """Case c with the hi + lo split weights of its "split" variant rounded to bfloat16 (the lo fragments dropped), reference input only."""
    key = {"first": "c1", "decfinal": "fin", "to1": "conv"}[c.kernel]
    return types.SimpleNamespace(kernel=c.kernel, raw=dict(c.raw, **{key: _bf(c.raw[key])}), inp=c.inp, out_dtype=c.out_dtype)


def _code_grid(g, B, H, W):
    grid = torch.full((B, H, W), 255, dtype=torch.uint8)
    grid[torch.rand(B, H, W, generator=g) < 0.3] = 0                       # obstacles
    grid[torch.rand(B, H, W, generator=g) < 0.05] = 128                    # marker pixels
    grid[torch.rand(B, H, W, generator=g) < 0.02] = 77                     # any other code renders black
    grid[:, 0, :] = 0
    grid[:, :, -1] = 128                                                   # borders exercise the zero padding
    return grid


def _default_init(g, cout, cin, transposed=False):
    """nn.Conv2d's default initialisation (uniform +- 1 / sqrt(fan_in)) from the case's own generator."""
    k = (9 * (cout if transposed else cin)) ** -0.5
    shape = (cin, cout, 3, 3) if transposed else (cout, cin, 3, 3)
    return ((torch.rand(shape, generator=g) * 2 - 1) * k).double(), ((torch.rand(cout, generator=g) * 2 - 1) * k).double()


def _bf(pair):
    return tuple(R.bf16_round(t) for t in pair)


@functools.lru_cache(maxsize=None)
def _params_b(kernel, key, dtype_name="bfloat16", C=24, representable=True):
    """(b) / (c): the raw parameters.  Single-stage kernels: unit-normal weights over sqrt(n), rounded to bfloat16 where the kernel
    takes bfloat16 weights; two-stage kernels: the modules' default initialisation in bfloat16, as their tests in test_gpu_mfma.py
    (the first stage's first convolution stays float32: the packer splits it hi + lo)."""
    g = _gen("params", kernel, key, dtype_name, C, representable)
    rn = lambda *s: torch.randn(*s, generator=g).to(F32).double()
    f32 = lambda t: t.to(F32).double()                                     # the reference multiplies by the float32 the kernel gets
    if kernel in ("enc", "dec"):
        n = 216 if kernel == "enc" else 96
        return dict(conv=(R.bf16_round(rn(24, 24, 3, 3) / n ** 0.5), rn(24)))
    if kernel == "first":
        return dict(c1=_default_init(g, 24, 1), c2=_bf(_default_init(g, 24, 24)))   # c1: float32, split hi + lo by the packer
    if kernel == "decfinal":
        (wd, bd), fin = _default_init(g, 24, 24, transposed=True), _default_init(g, 1, 24)
        return dict(dec=(R.bf16_round(wd), bd.to(F32).double()), fin=tuple(t.to(F32).double() for t in fin))
    if kernel == "c1":
        return dict(conv=(f32(rn(C, 1, 3, 3) / 3), rn(C)))
    if kernel == "to1":
        w = rn(1, C, 3, 3) / (9 * C) ** 0.5
        return dict(conv=(R.bf16_round(w) if representable else f32(w), rn(1)))
    raw = dict(c1=_bf(_default_init(g, 64, 3)), c2=_bf(_default_init(g, 128, 64)))
    raw["ln"] = _bf(((torch.rand(128, generator=g) + 0.5).double(), (torch.randn(128, generator=g) * 0.2).double()))
    return raw


@functools.lru_cache(maxsize=None)
def _normal_case(kernel, shape, dtype_name="bfloat16", C=24, representable=True, mask=False):
    """(b): unit-normal input (mask: GenNet's {0, 1} mask, first stage only)."""
    B, H, W = shape
    dtype = getattr(torch, dtype_name)
    raw = _params_b(kernel, shape, dtype_name, C, representable)
    g = _gen("normal", kernel, shape, dtype_name, C, mask)
    if kernel in ("tok1", "tokf"):
        return _case(kernel, raw, dict(grid=_code_grid(g, B, H, W)))
    if kernel in ("first", "c1"):
        x = (torch.rand(B, H, W, generator=g) < 0.4).float() if mask else torch.randn(B, H, W, generator=g)
    else:
        x = torch.randn(B, H, W, C, generator=g)
    inp = dict(x=x.to(dtype))
    if kernel == "first":
        inp.update(slope1=SLOPE_B, slope2=float(torch.tensor(0.2, dtype=F32)))
    elif kernel != "to1":
        inp.update(slope=SLOPE_B)
    return _case(kernel, raw, inp, dtype)


# ------------------------------------------------------------------------------------------------ launches
def _wrapper_kernel(kernel):
    return "to1" if kernel.startswith("to1") else kernel


def _run(kernel, inp, dev):
    """Through the ppnet_amd.fused wrapper; returns the output as NHWC on the device."""
    from ppnet_amd import fused
    d = lambda k: inp[k].to(dev)
    if kernel in ("enc", "dec"):
        return fused.gennet_conv_s2(d("x").permute(0, 3, 1, 2), d("wp"), d("bp"), inp["slope"], kernel == "dec").permute(0, 2, 3, 1)
    if kernel == "first":
        return fused.gennet_first_enc(d("x").unsqueeze(1), d("w1"), d("b1"), d("wk2"), d("b2"), inp["slope1"], inp["slope2"]).permute(0, 2, 3, 1)
    if kernel == "decfinal":
        return fused.gennet_dec_final(d("x").permute(0, 3, 1, 2), d("wp"), d("bp"), inp["slope"], d("wf"), inp["bias_f"]).permute(0, 2, 3, 1)
    if kernel == "c1":
        return fused.conv3x3_c1(d("x").unsqueeze(1), d("w"), d("b"), inp["slope"]).permute(0, 2, 3, 1)
    if kernel == "to1":
        return fused.conv3x3_to1(d("x").permute(0, 3, 1, 2), d("w"), inp["bias_f"]).permute(0, 2, 3, 1)
    if kernel == "tok1":
        return fused.tokenizer_conv1_codes(d("grid"), d("lut"))
    assert kernel == "tokf"
    return fused.tokenizer_codes(d("grid"), d("lut"), d("w2p"), d("vec"), inp["eps"])


_OUT = object()
_DT = {F32: 0, BF: 1}


def _abi(kernel, inp):
    """(exported function, its arguments without the stream): a string names an input tensor of inp, _OUT stands for the output."""
    x = inp["grid"] if kernel in ("tok1", "tokf") else inp["x"]
    B, H, W = x.shape[:3]
    if kernel in ("enc", "dec"):
        return "ppn_gennet_conv_s2_bf16", ["x", "wp", "bp", _OUT, B, H, W, inp["slope"], int(kernel == "dec")]
    if kernel == "first":
        return "ppn_gennet_first_enc_bf16", ["x", "w1", "b1", "wk2", "b2", _OUT, B, H, W, inp["slope1"], inp["slope2"]]
    if kernel == "decfinal":
        return "ppn_gennet_dec_final_bf16", ["x", "wp", "bp", inp["slope"], "wf", inp["bias_f"], _OUT, B, H, W]
    if kernel == "c1":
        return "ppn_conv3x3_c1_nhwc", ["x", "w", "b", _OUT, B, H, W, inp["w"].shape[0], inp["slope"], _DT[x.dtype]]
    if kernel == "to1":
        return "ppn_conv3x3_to1_nhwc", ["x", "w", inp["bias_f"], _OUT, B, H, W, x.shape[3], _DT[x.dtype]]
    if kernel == "tok1":
        return "ppn_tokenizer_conv1_codes_bf16", ["grid", "lut", _OUT, B, H, W]
    return "ppn_tokenizer_codes_bf16", ["grid", "lut", "w2p", "vec", _OUT, B, H, W, inp["eps"]]


SENTINEL = 12345.0


def _guard_elems(t):
    """Elements on either side of a tensor inside its allocation: one image (its first axis) rounded up to 64 elements, plus 256 —
    every element size keeps the 16-byte alignment of the vector loads and stores."""
    per = t.numel() // max(1, t.shape[0])
    return (per + 63) // 64 * 64 + 256


def _run_guarded(kernel, c, dev):
    """The launch through the C ABI with every operand inside a larger allocation.  Returns (rc, front, result, tail) of the output
    buffer on the host; front and tail were filled with SENTINEL."""
    from ppnet_amd import _lib as L
    fn, spec = _abi(kernel, c.inp)
    out_shape = tuple(c.ref.out.shape)
    keep, args, ob = [], [], None
    for a in spec:
        if isinstance(a, str):
            t = c.inp[a].contiguous()
            g = _guard_elems(t)
            buf = torch.full((g + t.numel() + g,), 128 if t.dtype == torch.uint8 else 3.0e4, dtype=t.dtype)
            buf[g:g + t.numel()] = t.reshape(-1)
            buf = buf.to(dev)
            keep.append(buf)
            args.append(ctypes.c_void_p(buf.data_ptr() + g * t.element_size()))
        elif a is _OUT:
            n = 1
            for v in out_shape:
                n *= v
            og = (n // out_shape[0] + 63) // 64 * 64 + 256
            ob = torch.full((og + n + og,), SENTINEL, dtype=c.out_dtype, device=dev)
            args.append(ctypes.c_void_p(ob.data_ptr() + og * ob.element_size()))
        else:
            args.append(a)
    with torch.cuda.device(dev):
        rc = getattr(L.lib, fn)(*args, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize()
    ob = ob.cpu()
    return rc, ob[:og], ob[og:og + n].reshape(out_shape), ob[og + n:]


# ------------------------------------------------------------------------------------------------ checks
def _assert_exact(c, got, label):
    """(a): the precondition on the reference, then equality at every element."""
    assert c.exact, f"{label}: the float64 result of this draw is not exact in {c.out_dtype} at any density: the test's own data is wrong"
    got = got.detach().cpu()
    assert got.shape == c.ref.out.shape and got.dtype == c.out_dtype, label
    bad = got.double() != c.ref.out
    assert not bool(bad.any()), (f"{label}: {int(bad.sum())} of {bad.numel()} elements differ, first at {tuple(int(v) for v in bad.nonzero()[0])}: "
                                 f"got {float(got.double()[bad][0])}, want {float(c.ref.out[bad][0])}")


def _reduction(kernel, c):
    return {"enc": 217, "dec": 97, "c1": 10}.get(kernel) or 9 * c.inp["x"].shape[3] + 1


def _ratio_b(kernel, c, got, ref, label, hi_lo=False):
    """(b): asserts the kernel's bound on got against ref; returns the worst err / bound.  hi_lo: the matrix-core to1 kernel on float32
    weights that are not bfloat16 numbers."""
    got = got.detach().cpu()
    want = ref.out
    assert got.shape == want.shape and got.dtype == c.out_dtype, label
    assert bool(torch.isfinite(got.float()).all()), label
    err = (got.double() - want).abs()
    if kernel in ("enc", "dec", "c1", "to1"):
        bound = 2 * _reduction(kernel, c) * 2.0 ** -24 * ref.A
        if hi_lo:
            bound = bound + 2.0 ** -17 * ref.A                             # the products of the hi + lo weight fragments
        if c.out_dtype == BF:
            bound = bound + 2.0 ** -8 * want.abs()
        mean_ratio = 0.0
    elif kernel == "first":                                                # test_gennet_fused_first_stage_vs_float64
        bound, mean_ratio = want.abs() * 2.0 ** -7 + 6e-3, float(err.mean()) / 1e-3
    elif kernel == "decfinal":                                             # test_gennet_fused_decoder_tail_is_bit_identical_to_the_two_kernels
        bound, mean_ratio = torch.full_like(want, 1.5e-2 * max(1.0, float(want.abs().max()))), 0.0
    elif kernel == "tok1":                                                 # test_tokenizer_palette_conv_vs_float64
        bound, mean_ratio = want.abs() * 2.0 ** -8 + 1e-4, 0.0
    else:                                                                  # test_tokenizer_one_kernel_vs_float64 (strict there)
        bound, mean_ratio = torch.full_like(want, 0.03), float(err.mean()) / 3e-3
    ratio = float((err / bound.clamp_min(1e-300)).max())
    bad = err > bound
    assert not bool(bad.any()), f"{label}: {int(bad.sum())} of {bad.numel()} elements over the bound, worst err / bound = {ratio:.3f}"
    assert mean_ratio < 1.0, f"{label}: mean error at {mean_ratio:.3f} of its bound"
    return max(ratio, mean_ratio)


def _report(capsys, label, ratio):
    with capsys.disabled():
        print(f"\nCONV_RATIO {label} {ratio:.3f}", end="")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert not os.environ.get("PPNET_TO1_VALU"), "PPNET_TO1_VALU is set: the to1 tests of this process would not reach the matrix-core kernel"
    return torch.device("cuda:0")


def test_palette_constants():
    from ppnet_amd import dense
    assert tuple(dense.IMG_MEAN) == IMG_MEAN and tuple(dense.IMG_STD) == IMG_STD


# ------------------------------------------------------------------------------------------------ (a) exact
_A_CASES = ([(k, v, s) for k in ("enc", "dec", "first", "decfinal") for v in VARIANTS for s in SHAPES[k]]
            + [(k, "split", s) for k in ("first", "decfinal") for s in SHAPES[k]])


@pytest.mark.parametrize("kernel,variant,shape", _A_CASES, ids=[f"{k}-{v}-{_sid(s)}" for k, v, s in _A_CASES])
def test_exact_stride2_stages(dev, kernel, variant, shape):
    c = _exact_case(kernel, variant, shape)
    _assert_exact(c, _run(kernel, c.inp, dev), f"{kernel} {variant} {_sid(shape)} density {c.density}")


def test_exact_first_stage_draws_cover_every_weight_slot():
    """The thinned draws of (a) still put a non-zero weight into every (tap, input channel) slot of the packed second-stage weights
    and every tap of the first stage at least once — and into no padding slot ever."""
    wk2 = torch.zeros(9, 32, dtype=torch.bool)
    w1 = torch.zeros(32, dtype=torch.bool)
    pairs = torch.zeros(24, 9, dtype=torch.bool)
    for variant in VARIANTS:
        for shape in SHAPES["first"]:
            c = _exact_case("first", variant, shape)
            wk2 |= (c.inp["wk2"].float() != 0).any(dim=2).any(dim=0)       # [2][9][16][32] -> [tap][k slot]
            w1 |= (c.inp["w1"].float() != 0).reshape(32, 32).any(dim=0)    # [2][16][32] -> [k column]
            pairs |= (c.raw["c2"][0] != 0).any(dim=0).reshape(24, 9)        # [co][ci][3][3] -> [ci][tap]
    real = torch.tensor([(e < 4) or (g < 2) for g in range(4) for e in range(8)])      # the kernel's slot (g, e) holds a channel
    assert bool(pairs.all())
    assert bool(wk2[:, real].all()) and not bool(wk2[:, ~real].any())
    assert bool(w1[:10].all()) and not bool(w1[10:].any())                 # taps 0 .. 8 and the bias column; integers: the lo half is zero


def test_split_variant_depends_on_the_lo_fragments():
    """On the reference: dropping the lo halves of the split weights changes outputs of every "split" draw but the one-pixel ones."""
    for kernel, shapes in (("first", SHAPES["first"]), ("decfinal", SHAPES["decfinal"]), ("to1", SHAPES["to1_mfma"])):
        counts = {s: _exact_case(kernel, "split", s).lo_matters for s in shapes}
        assert all(n > 0 for s, n in counts.items() if s[0] * s[1] * s[2] > 8), (kernel, counts)


@pytest.mark.parametrize("variant", list(VARIANTS) + ["split"])
@pytest.mark.parametrize("shape", SHAPES["to1_mfma"], ids=_sid)
def test_exact_to1_matrix_core(dev, variant, shape):
    c = _exact_case("to1", variant, shape)
    _assert_exact(c, _run("to1", c.inp, dev), f"to1 mfma {variant} {_sid(shape)}")


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("shape", SHAPES["to1_valu"], ids=_sid)
@pytest.mark.parametrize("dtype_name,C", TO1_VALU_CONFIGS)
def test_exact_to1_direct(dev, dtype_name, C, shape, variant):
    c = _exact_case("to1", variant, shape, dtype_name, C)
    _assert_exact(c, _run("to1", c.inp, dev), f"to1 valu {dtype_name} Cin {C} {variant} {_sid(shape)}")


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("shape", SHAPES["c1"], ids=_sid)
@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
@pytest.mark.parametrize("C", [8, 16, 24, 32])
def test_exact_c1(dev, C, dtype_name, shape, variant):
    c = _exact_case("c1", variant, shape, dtype_name, C)
    _assert_exact(c, _run("c1", c.inp, dev), f"c1 {dtype_name} Cout {C} {variant} {_sid(shape)}")


# ------------------------------------------------------------------------------------------------ (b) float64
_B_CASES = [(k, s) for k in ("enc", "dec", "decfinal", "tok1", "tokf") for s in SHAPES[k]]


@pytest.mark.parametrize("kernel,shape", _B_CASES, ids=[f"{k}-{_sid(s)}" for k, s in _B_CASES])
def test_float64_bound(dev, capsys, kernel, shape):
    c = _normal_case(kernel, shape)
    label = f"{kernel} {_sid(shape)}"
    if kernel == "tok1":                                                   # the reference's palette is the one the network's input tensor holds
        from ppnet_amd import fused
        img = fused.grid_to_image(c.inp["grid"].to(dev), IMG_MEAN, IMG_STD, BF).permute(0, 2, 3, 1)
        assert torch.equal(img.cpu().double(), c.ref.image), label
    _report(capsys, label, _ratio_b(kernel, c, _run(kernel, c.inp, dev), c.ref, label))


@pytest.mark.parametrize("mask", [False, True], ids=["normal", "mask"])
@pytest.mark.parametrize("shape", SHAPES["first"], ids=_sid)
def test_float64_bound_first_stage(dev, capsys, shape, mask):
    c = _normal_case("first", shape, mask=mask)
    label = f"first {'mask' if mask else 'normal'} {_sid(shape)}"
    _report(capsys, label, _ratio_b("first", c, _run("first", c.inp, dev), c.ref, label))


@pytest.mark.parametrize("representable", [True, False], ids=["bf16_weights", "f32_weights"])
@pytest.mark.parametrize("shape", SHAPES["to1_mfma"], ids=_sid)
def test_float64_bound_to1_matrix_core(dev, capsys, shape, representable):
    c = _normal_case("to1", shape, representable=representable)
    label = f"to1_mfma {'bf16w' if representable else 'f32w'} {_sid(shape)}"
    assert _is(BF, c.raw["conv"][0]) == representable
    _report(capsys, label, _ratio_b("to1", c, _run("to1", c.inp, dev), c.ref, label, hi_lo=not representable))


@pytest.mark.parametrize("shape", SHAPES["to1_valu"], ids=_sid)
@pytest.mark.parametrize("dtype_name,C", TO1_VALU_CONFIGS)
def test_float64_bound_to1_direct(dev, capsys, dtype_name, C, shape):
    c = _normal_case("to1", shape, dtype_name, C, representable=False)
    label = f"to1_valu {dtype_name} Cin {C} {_sid(shape)}"
    _report(capsys, label, _ratio_b("to1", c, _run("to1", c.inp, dev), c.ref, label))


@pytest.mark.parametrize("shape", SHAPES["c1"], ids=_sid)
@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
@pytest.mark.parametrize("C", [8, 16, 24, 32])
def test_float64_bound_c1(dev, capsys, C, dtype_name, shape):
    c = _normal_case("c1", shape, dtype_name, C)
    label = f"c1 {dtype_name} Cout {C} {_sid(shape)}"
    _report(capsys, label, _ratio_b("c1", c, _run("c1", c.inp, dev), c.ref, label))


# ------------------------------------------------------------------------------------------------ (c) the loops' second trip
@pytest.mark.parametrize("kernel", list(CAPS))
def test_batch_split_identity_across_the_loop_wrap(dev, capsys, kernel):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    H, W, per, cap, unit = CAPS[kernel](cus)
    B = cap // per + 2
    while unit > 1 and (B * per) % unit == 0:
        B += 1
    chunk = max(1, cap // per // 2)
    wrap = cap // per                                                      # the image that holds the first unit of the second trip
    assert B * per > cap and chunk * per <= cap and 0 < wrap < B - 1 and (unit == 1 or (B * per) % unit)
    raw = _params_b(kernel, "wrap")
    g = torch.Generator(device=dev).manual_seed(zlib.crc32(kernel.encode()))
    if kernel in ("tok1", "tokf"):
        codes = torch.tensor([255, 255, 255, 0, 0, 128, 77], dtype=torch.uint8, device=dev)
        inp = dict(grid=codes[torch.randint(0, 7, (B, H, W), generator=g, device=dev)])
        key = "grid"
    else:
        shape = (B, H, W) if kernel == "first" else (B, H, W, 24)
        inp = dict(x=torch.randn(*shape, generator=g, device=dev).to(BF))
        inp.update(dict(slope1=SLOPE_B, slope2=float(torch.tensor(0.2, dtype=F32))) if kernel == "first" else dict(slope=SLOPE_B))
        key = "x"
    c = types.SimpleNamespace(kernel=kernel, raw=raw, inp=dict(inp, **{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in _pack(kernel, raw).items()}),
                              out_dtype=BF)
    full = _run(kernel, c.inp, dev)
    for i in range(0, B, chunk):
        part = _run(kernel, dict(c.inp, **{key: c.inp[key][i:i + chunk]}), dev)
        assert torch.equal(full[i:i + chunk], part), f"{kernel}: images {i} .. {min(B, i + chunk) - 1} of the batch of {B} differ from the same images alone"
    worst = 0.0
    for i in (0, wrap, B - 1):
        worst = max(worst, _ratio_b(kernel, c, full[i:i + 1], _reference(kernel, c, c.inp[key][i:i + 1]), f"{kernel} wrap image {i} of {B}"))
    _report(capsys, f"{kernel} wrap B={B} {H}x{W}", worst)


# ------------------------------------------------------------------------------------------------ (d) guards
_D_CASES = ([(k, s) for k in ("enc", "dec", "first", "decfinal") for s in SHAPES[k]] + [("to1_mfma", s) for s in SHAPES["to1_mfma"]]
            + [("to1_valu", s) for s in SHAPES["to1_valu"]] + [("c1", s) for s in SHAPES["c1"]])


@pytest.mark.parametrize("kernel,shape", _D_CASES, ids=[f"{k}-{_sid(s)}" for k, s in _D_CASES])
def test_kernel_reads_and_writes_only_its_tensors(dev, kernel, shape):
    cases = {"to1_mfma": [("bfloat16", 24)], "to1_valu": [("float32", 8), ("bfloat16", 32)], "c1": [("float32", 8), ("bfloat16", 24)]}.get(kernel, [("bfloat16", 24)])
    for dtype_name, C in cases:
        c = _exact_case(_wrapper_kernel(kernel), "pm1", shape, dtype_name, C)
        rc, front, got, tail = _run_guarded(_wrapper_kernel(kernel), c, dev)
        label = f"guard {kernel} {dtype_name} {C} {_sid(shape)}"
        assert rc == 0, label
        fill = torch.full((), SENTINEL, dtype=c.out_dtype)
        assert bool((front == fill).all()), f"{label}: written in front of the output"
        assert bool((tail == fill).all()), f"{label}: written behind the output"
        _assert_exact(c, got, label)


@pytest.mark.parametrize("kernel,shape", [(k, s) for k in ("tok1", "tokf") for s in SHAPES[k]], ids=lambda v: v if isinstance(v, str) else _sid(v))
def test_tokenizer_reads_and_writes_only_its_tensors(dev, kernel, shape):
    c = _normal_case(kernel, shape)
    rc, front, got, tail = _run_guarded(kernel, c, dev)
    label = f"guard {kernel} {_sid(shape)}"
    assert rc == 0, label
    fill = torch.full((), SENTINEL, dtype=BF)
    assert bool((front == fill).all()) and bool((tail == fill).all()), f"{label}: written outside the output"
    _ratio_b(kernel, c, got, c.ref, label)


# ------------------------------------------------------------------------------------------------ the direct to1 kernel at bfloat16 Cin = 24
def _to1_valu_child(outdir):
    """Runs in a fresh process with PPNET_TO1_VALU=1 (read once per process): every case in sequence, outputs to outdir."""
    assert os.environ.get("PPNET_TO1_VALU") == "1"
    dev = torch.device("cuda", 0)
    res = {}
    for shape in TO1_CHILD_SHAPES:
        for variant in VARIANTS:
            res[("a", variant, shape)] = _run("to1", _exact_case("to1", variant, shape).inp, dev).cpu()
        res[("b", shape)] = _run("to1", _normal_case("to1", shape, representable=False).inp, dev).cpu()
    torch.save(res, os.path.join(outdir, "out.pt"))


@pytest.fixture(scope="module")
def to1_valu_outputs(dev):
    env = dict(os.environ, PPNET_TO1_VALU="1", PYTHONPATH=ROOT)
    with tempfile.TemporaryDirectory() as td:
        code = "import sys; from tests.test_gpu_gennet_conv import _to1_valu_child; _to1_valu_child(sys.argv[1])"
        done = subprocess.run([sys.executable, "-c", code, td], env=env, cwd=ROOT, timeout=300)
        assert done.returncode == 0, f"the PPNET_TO1_VALU child exited with {done.returncode}"
        return torch.load(os.path.join(td, "out.pt"))


@pytest.mark.parametrize("shape", TO1_CHILD_SHAPES, ids=_sid)
def test_to1_direct_bf16_cin24_in_a_child_process(to1_valu_outputs, capsys, shape):
    for variant in VARIANTS:
        _assert_exact(_exact_case("to1", variant, shape), to1_valu_outputs[("a", variant, shape)], f"to1 valu child {variant} {_sid(shape)}")
    c = _normal_case("to1", shape, representable=False)
    label = f"to1_valu bfloat16 Cin 24 {_sid(shape)}"
    _report(capsys, label, _ratio_b("to1", c, to1_valu_outputs[("b", shape)], c.ref, label))
