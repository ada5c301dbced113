"""Every kernel behind ppn_na2d_fwd / _padded / _vpad, one at a time, against the float64 reference (tests/_na_ref.py, itself held
against oracle/na_np.py by tests/test_na_ref.py) at the smallest shapes where each kernel's border, mask, ragged-group, re-ordering
and persistent-loop code runs.  tests/test_gpu_na.py reaches the same kernels through the default routing only.

WHICH KERNEL RUNS is chosen by na2d_launch (csrc/na2d.hip) and na2d_mfma_launch (csrc/na2d_mfma.hip) from shape, dtype and the
A/B environment knobs.  These tests CANNOT OBSERVE the kernel that ran: they rely on the knobs as those two files document them
(VARIANTS below).  A change that removes or renames a knob must update that table, or its rows silently test the default kernel.

Inputs per (variant, shape):
  (a) unit-normal qkv and rpb, every element against the reference:
        float32    |got - want| <= 2e-5 (the project's bound);
        bfloat16   |got - want| <= k * 2^-9 * A + 1e-6,   A = sum_j p_j |v_j| from the reference.
      Rounding points, from the kernels' code; u = 2^-8 is bfloat16's unit roundoff (half a step of an 8-bit significand), i.e. TWO of
      the bound's units of 2^-9.  Matrix-core kernels (na2d_mfma.hip, na2d_halo16.hip, na2d_dense7.hip): the probabilities are
      rounded to bfloat16 for the PV product AND for the normaliser (an all-ones MFMA over the same rounded values), so the result
      is a weighted mean with weights p (1 + e_j), |e_j| <= u: its error is sum p e_j (v_j - o), at most u (A + |o|) <= 2 u A; the
      output rounding adds u |o| <= u A.  The v_dot2 kernel (na2d.hip, bfloat16) rounds the probabilities for the numerator only
      (<= u A) and the output (<= u A).  Everything else is float32 (logits from exact bf16 products, exp2 and rcp at 1 ulp).
      Worst case 3 u A resp. 2 u A = 6 resp. 4 units; independent signs keep the worst element seen near 2 - 3 units.
  (b) known answer: q = 0, 13 heads, rpb[h] = -60 except 0 at (a, h), launches a = 0 .. 12 — all 169 bias entries.  A query whose
      window holds that offset puts probability 1 (float32: 1 / (1 + 48 e^-60)) on that member, so its output IS that member's v:
      within one bfloat16 step 2^-8 |v| (float32: 1e-6); the v of a padded member is pad_kv's.  The other queries see 49 equal
      logits and are held to the bound of (a).  Pins the rpb indexing, the window clamp and the V gather of every lane.
  (c) q and k times 6 (logits near +-80), rpb unit normal: finite, and the bound of (a).
  guards  through the raw C ABI: qkv, pad_kv and rpb sit inside larger buffers whose neighbouring rows hold 3e4, out inside a
      sentinel-filled buffer; the sentinels survive and the result meets the bound of (a).  The guards are part of the allocations.

MEASURED on MI355X (gfx950): the largest (|got - want| - 1e-6) / (2^-9 A) over all shapes of the variant and, for reference, of an
IDEAL kernel (the float64 result rounded once to bfloat16, computed on the CPU):

    variant       (a) + guards   (b) rest   (c)       k
    ideal         1.90           -          1.99
    halo16_2x8    2.08           1.77       2.74      4
    halo16_4x4    2.08           1.77       2.74      4
    mfma16        2.08           1.77       2.74      4
    mfma8         2.08           1.77       2.74      4
    mfma4         2.08           1.77       2.74      4
    default       2.08           1.77       2.74      4
    dense7        2.19           0.72       -         4
    valu_bf16     2.34           1.77       2.97      4

(The matrix-core variants agree to the digit: they do the same arithmetic block for block, and the worst element is the same.)
The rule "k = twice the measured value, at most 4" ends at its cap for every variant, because one bfloat16 rounding is worth two
of the bound's units (above): the output rounding alone reaches 2.0 (the ideal row).  k = 4 is both the cap and "three counted
rounding points + 1".  It is NOT twice the measured value: the margin over the worst element seen is 1.35 (c) to 1.9 (a), not 2.
Inputs are seeded and the kernels deterministic, so the tests do not move from run to run; a new seed or shape that exceeds 4 needs
the derivation above (worst case 6 resp. 4), not a larger common k.

A kernel trace (rocprofv3 --kernel-trace over one launch per variant and shape, once, by hand) showed the kernel names of the
VARIANTS table and of F32_SHAPES below: na2d_halo16_kernel<2,8> / <4,4>, na2d_mfma_kernel<16> / <8> / <4>, na2d_dense7_kernel<7>
(<8> for 16x16_d2), na2d_fwd_kernel<float, 4 | 8 | 16, ...> as F32_SHAPES says, na2d_fwd_kernel<__hip_bfloat16, 4 | 8, ...>
on SHAPES under PPNET_NA_VALU (its tile of 16 on the float32 shapes follows from launch_typed and was not traced); "default" went to halo16<2,8> at 17x23_d1 and 40x40_d2, to mfma<4> on the two 28x35 shapes, to mfma<8> elsewhere.
"""
import ctypes
import functools
import os
import subprocess
import sys
import tempfile
import zlib

import pytest

torch = pytest.importorskip("torch")

from tests import _na_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SCALE = 32 ** -0.5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Read on every launch (na2d_mfma_launch, na2d_halo16_launch): monkeypatch selects them inside one process.
KNOBS = ("PPNET_NA_RT", "PPNET_NA_HALO16", "PPNET_NA_HALO_BLOCK")
# Read once per process (na2d_launch): must be unset here; the valu_bf16 variant runs in a child of its own.
PROCESS_KNOBS = ("PPNET_NA_VALU", "PPNET_NA_NO_DENSE7")
VARIANTS = {                                                               # kernel, by the launchers' documentation
    "halo16_2x8": {"PPNET_NA_RT": "16"},                                   # na2d_halo16_kernel<2,8>
    "halo16_4x4": {"PPNET_NA_RT": "16", "PPNET_NA_HALO_BLOCK": "4x4"},     # na2d_halo16_kernel<4,4>
    "mfma16": {"PPNET_NA_RT": "16", "PPNET_NA_HALO16": "0"},               # na2d_mfma_kernel<16>
    "mfma8": {"PPNET_NA_RT": "8"},                                         # na2d_mfma_kernel<8>
    "mfma4": {"PPNET_NA_RT": "4"},                                         # na2d_mfma_kernel<4>
    "default": {},                                                         # whatever na_region_size picks
}
# k of the bound of (a), per variant, for inputs (a) / (b) and for (c); see MEASURED above
K_A = {"halo16_2x8": 4.0, "halo16_4x4": 4.0, "mfma16": 4.0, "mfma8": 4.0, "mfma4": 4.0, "default": 4.0, "dense7": 4.0, "valu_bf16": 4.0}
K_C = dict(K_A)


def _shape(B, H, W, heads, d, real=None, form="plain"):
    """H x W: the (padded) grid.  form: "plain" (every token real), "mat" (the stored grid is the padded one, real = the queries),
    "vpad" (the stored grid is the real part of the same tensor, pad_kv stands for the rest)."""
    return dict(B=B, H=H, W=W, heads=heads, d=d, real=real, form=form)


SHAPES = {
    "7x9_d1": _shape(3, 7, 9, 1, 1),                # every window clamped on the 7-long axis; RT = 4: 18 tiles, surplus waves
    "17x23_d1": _shape(1, 17, 23, 2, 1),            # remainders 1 and 7 at RT = 16, 1 and 3 at RT = 4
    "15x22_d2": _shape(3, 15, 22, 3, 2),            # groups of 8 / 7 rows; grid not a multiple of 8: the XCD order's remainder branch
    "23x29_d3": _shape(1, 23, 29, 2, 3),            # groups of 8 / 8 / 7 by 10 / 10 / 9
    "14x21_d2": _shape(2, 14, 21, 1, 2),            # 7-row groups, all clamped, not dense7-eligible
    "40x40_d2": _shape(10, 40, 40, 4, 2),           # 640 halo16 items on 256 CUs: 2 - 3 items per persistent workgroup
    "mat_21x28_r16x13_d3": _shape(2, 21, 28, 2, 3, (16, 13), "mat"),
    "mat_28x35_r3x5_d4": _shape(2, 28, 35, 1, 4, (3, 5), "mat"),           # Hr < d: dilation groups without a query
    "vpad_21x28_r16x13_d3": _shape(2, 21, 28, 2, 3, (16, 13), "vpad"),
    "vpad_28x35_r3x5_d4": _shape(2, 28, 35, 1, 4, (3, 5), "vpad"),
}
DENSE7_SHAPES = {
    "7x7_d1": _shape(3, 7, 7, 1, 1),
    "21x21_d3": _shape(1, 21, 21, 3, 3),
    "16x16_d2": _shape(2, 16, 16, 2, 2),                                   # 8 x 8 groups
    "vpad_28x28_r16x16_d4": _shape(2, 28, 28, 2, 4, (16, 16), "vpad"),
    "vpad_28x28_r3x3_d4": _shape(2, 28, 28, 1, 4, (3, 3), "vpad"),         # groups without a query
}
# float32 (na2d_fwd_kernel<float, TILE>): launch_typed takes the tile with the best lane utilisation of the largest query sub-image
# (hq x wq), so the sub-image side selects the kernel.  Sides 4, 8, 16 fill tiles of 4, 8, 16; 5 is a partial tile of 8; 9 and 17
# are 3 and 5 tiles of 4 with a remainder of 1; 31 is two tiles of 16 per axis with a remainder of 15.
F32_SHAPES = {
    "q4_mat_28x28_r16x16_d4": (4, _shape(1, 28, 28, 2, 4, (16, 16), "mat")),
    "q4_vpad_28x28_r16x16_d4": (4, _shape(1, 28, 28, 2, 4, (16, 16), "vpad")),
    "q8_8x8_d1": (8, _shape(2, 8, 8, 1, 1)),
    "q16_16x16_d1": (16, _shape(1, 16, 16, 2, 1)),
    "q5_mat_21x21_r14x13_d3": (8, _shape(1, 21, 21, 1, 3, (14, 13), "mat")),
    "q9_18x17_d2": (4, _shape(1, 18, 17, 1, 2)),
    "q17_17x17_d1": (4, _shape(2, 17, 17, 2, 1)),
    "q31_31x31_d1": (16, _shape(1, 31, 31, 1, 1)),
    "15x22_d2": (4, SHAPES["15x22_d2"]),
}
ALL_SHAPES = dict(SHAPES, **{"dense7_" + k: v for k, v in DENSE7_SHAPES.items()}, **{"f32_" + k: v[1] for k, v in F32_SHAPES.items()})
B_SHAPES = ("15x22_d2", "mat_21x28_r16x13_d3", "vpad_21x28_r16x13_d3")     # (b); dense7: 21x21_d3
C_SHAPES = ("17x23_d1", "15x22_d2")                                        # (c)
GUARD_SHAPES = ("15x22_d2", "vpad_21x28_r16x13_d3")


def _dense7_eligible(s):
    """na2d_dense7_launch's condition: it is looked at before any knob."""
    H, W, d = s["H"], s["W"], s["d"]
    all_real = s["real"] is None
    return (H == W == 7 * d and (s["form"] == "vpad" or all_real)) or (H == W == 8 * d and all_real)


def _f32_tile(s):
    """launch_typed's choice (csrc/na2d.hip)."""
    Hr, Wr = s["real"] or (s["H"], s["W"])
    hq, wq = -(-Hr // s["d"]), -(-Wr // s["d"])
    util = lambda t: hq * wq / ((-(-hq // t) * t) * (-(-wq // t) * t))
    best = 16
    if util(8) > util(best) + 0.05:
        best = 8
    if util(4) > util(best) + 0.05:
        best = 4
    return best


assert not any(_dense7_eligible(s) for s in SHAPES.values()) and all(_dense7_eligible(s) for s in DENSE7_SHAPES.values())
assert all(_f32_tile(s) == t for t, s in F32_SHAPES.values())


# ------------------------------------------------------------------------------------------------ inputs and references
def _seed(s, kind):
    return zlib.crc32(repr((s["B"], s["H"], s["W"], s["heads"], s["d"], s["real"], kind)).encode())     # the same for "mat" and "vpad"


@functools.lru_cache(maxsize=None)
def _inputs(kind, name, dtype_name):
    """The launches of one (input kind, shape): a list of dicts in na2d_forward's terms; 13 launches for (b), one otherwise."""
    s = ALL_SHAPES[name]
    dtype = getattr(torch, dtype_name)
    heads = 13 if kind == "b" else s["heads"]
    B = min(s["B"], 2) if kind == "b" else s["B"]
    C = heads * 32
    g = torch.Generator().manual_seed(_seed(s, kind))
    full = torch.randn(B, s["H"], s["W"], 3 * C, generator=g)
    pad = torch.randn(3 * C, generator=g)
    if kind == "b":
        full[..., :C] = 0.0
    if kind == "c":
        full[..., :2 * C] *= 6.0
        pad[:2 * C] *= 6.0
    base = dict(heads=heads, d=s["d"], real_hw=None, pad_kv=None, padded_hw=None)
    if s["form"] == "vpad":
        Hr, Wr = s["real"]
        base.update(qkv=full[:, :Hr, :Wr].contiguous().to(dtype), pad_kv=pad.to(dtype), padded_hw=(s["H"], s["W"]))
    else:
        base.update(qkv=full.to(dtype), real_hw=s["real"])
    if kind != "b":
        return [dict(base, rpb=torch.randn(heads, 13, 13, generator=g))]
    launches = []
    for a in range(13):
        rpb = torch.full((13, 13, 13), -60.0)
        rpb[torch.arange(13), a, torch.arange(13)] = 0.0                   # head h: bias entry (a, h)
        launches.append(dict(base, rpb=rpb))
    return launches


@functools.lru_cache(maxsize=None)
def _refs(kind, name, dtype_name):
    """The float64 reference of every launch of _inputs, on the values as the kernel gets them (rounded to dtype)."""
    return [R.na2d_ref(i["qkv"], i["rpb"], i["heads"], i["d"], SCALE, real_hw=i["real_hw"], pad_kv=i["pad_kv"], padded_hw=i["padded_hw"])
            for i in _inputs(kind, name, dtype_name)]


def _run(inp, dev):
    from ppnet_amd import na
    kw = {}
    if inp["pad_kv"] is not None:
        kw = dict(pad_kv=inp["pad_kv"].to(dev), padded_hw=inp["padded_hw"])
    elif inp["real_hw"] is not None:
        kw = dict(real_hw=inp["real_hw"])
    return na.na2d_forward(inp["qkv"].to(dev), inp["rpb"].to(dev), inp["heads"], inp["d"], SCALE, **kw).cpu()


SENTINEL = 12345.0


def _run_guarded(inp, dev):
    """The launch through the C ABI with every operand inside a larger allocation: one image of 3e4 in front of and behind qkv, one
    row of 3e4 around pad_kv, one head of 3e4 around rpb, one image of SENTINEL around out.  Returns (rc, the whole out buffer)."""
    from ppnet_amd import _lib as L
    qkv, rpb = inp["qkv"], inp["rpb"]
    B, Hs, Ws, C3 = qkv.shape
    heads, C = inp["heads"], C3 // 3
    qb = torch.full((B + 2, Hs, Ws, C3), 3.0e4, dtype=qkv.dtype)
    qb[1:B + 1] = qkv
    rb = torch.full((heads + 2, 13, 13), 3.0e4)
    rb[1:heads + 1] = rpb
    qb, rb = qb.to(dev), rb.to(dev)
    Hr, Wr = (Hs, Ws) if inp["pad_kv"] is not None else (inp["real_hw"] or (Hs, Ws))
    ob = torch.full((B + 2, Hr, Wr, C), SENTINEL, dtype=qkv.dtype, device=dev)
    es = qkv.element_size()
    P = ctypes.c_void_p
    qp, rp, op = P(qb.data_ptr() + Hs * Ws * C3 * es), P(rb.data_ptr() + 169 * 4), P(ob.data_ptr() + Hr * Wr * C * es)
    stream = P(torch.cuda.current_stream(dev).cuda_stream)
    dt = {torch.float32: 0, torch.bfloat16: 1}[qkv.dtype]
    with torch.cuda.device(dev):
        if inp["pad_kv"] is not None:
            pb = torch.full((3, C3), 3.0e4, dtype=qkv.dtype)
            pb[1] = inp["pad_kv"]
            pb = pb.to(dev)
            H, W = inp["padded_hw"]
            rc = L.lib.ppn_na2d_fwd_vpad(qp, P(pb.data_ptr() + C3 * es), rp, op, B, H, W, Hr, Wr, heads, inp["d"], SCALE, dt, stream)
        else:
            rc = L.lib.ppn_na2d_fwd_padded(qp, rp, op, B, Hs, Ws, Hr, Wr, heads, inp["d"], SCALE, dt, stream)
        torch.cuda.synchronize()
    return rc, ob.cpu()


# ------------------------------------------------------------------------------------------------ checks
def _check_bound(got, ref, k, label, where=None):
    """Bound of (a).  k = None: float32, 2e-5 absolute.  where: [B, Hr, Wr, heads] bool, the (query, head) pairs to hold to it."""
    assert got.shape == ref.out.shape, label
    assert bool(torch.isfinite(got.float()).all()), label
    err = (got.double() - ref.out).abs()
    if where is not None:
        err = err * where.repeat_interleave(32, dim=-1)
    if k is None:
        print(f"NA_ERR {label} {float(err.max()):.3e}")
        assert float(err.max()) <= 2e-5, label
        return
    ratio = float(((err - 1e-6).clamp_min(0) / (2.0 ** -9 * ref.A).clamp_min(1e-30)).max())
    print(f"NA_RATIO {label} {ratio:.3f}")
    bad = err > k * 2.0 ** -9 * ref.A + 1e-6
    assert not bool(bad.any()), f"{label}: {int(bad.sum())} elements, worst err / (2^-9 A) = {ratio:.3f} > k = {k}"


def _check_unit(run, kind, name, k, label, dtype_name="bfloat16"):
    (inp,), (ref,) = _inputs(kind, name, dtype_name), _refs(kind, name, dtype_name)
    _check_bound(run(inp), ref, k, f"{label} {kind} {name}")


def _check_selection(outs, name, k, label, dtype_name="bfloat16"):
    """(b): outs = the 13 launches' outputs."""
    refs = _refs("b", name, dtype_name)
    selected = 0
    for a, (got, ref) in enumerate(zip(outs, refs)):
        B, Hr, Wr, _ = ref.out.shape
        H, W = ref.v_full.shape[1:3]
        g5, v5 = got.double().view(B, Hr, Wr, 13, 32), ref.v_full.view(B, H, W, 13, 32)
        assert bool(torch.isfinite(g5).all())
        sel = torch.zeros(B, Hr, Wr, 13, dtype=torch.bool)
        for h in range(13):
            mask, row, col = ref.select(a, h)
            want = v5[:, row, col, h]                                      # [B, Hr, Wr, 32]: the selected member's v
            err = (g5[:, :, :, h] - want).abs()
            lim = 2.0 ** -8 * want.abs() if k is not None else torch.full_like(want, 1e-6)
            bad = (err > lim) & mask[None, :, :, None]
            assert not bool(bad.any()), (f"{label} b {name}: bias entry ({a}, {h}): {int(bad.any(-1).sum())} of {int(mask.sum()) * B} selecting "
                                         f"queries do not return the selected member's v; worst |err| {float((err * mask[None, :, :, None]).max()):.3e}")
            sel[:, :, :, h] = mask
            selected += int(mask.sum())
        _check_bound(got, ref, k, f"{label} b{a} {name}", where=~sel)      # 49 equal logits: the plain mean of the window
    assert selected == 49 * Hr * Wr                                        # every member of every window was selected once


def _check_guarded(res, name, k, label, dtype_name="bfloat16"):
    rc, ob = res
    (ref,) = _refs("a", name, dtype_name)
    B = ref.out.shape[0]
    assert rc == 0
    fill = torch.full((), SENTINEL, dtype=ob.dtype)
    assert bool((ob[0] == fill).all()) and bool((ob[B + 1] == fill).all()), f"{label} guard {name}: out written outside its rows"
    _check_bound(ob[1:B + 1], ref, k, f"{label} guard {name}")


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture
def select_variant(monkeypatch):
    def select(variant):
        assert not any(v in os.environ for v in PROCESS_KNOBS), "a per-process NA knob is set: the variant table does not hold"
        for kname in KNOBS:
            monkeypatch.delenv(kname, raising=False)
        for kname, val in VARIANTS.get(variant, {}).items():
            monkeypatch.setenv(kname, val)
    return select


# ------------------------------------------------------------------------------------------------ the per-launch knob variants
@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_unit_normal_inputs_against_float64(dev, select_variant, variant, name):
    select_variant(variant)
    _check_unit(lambda i: _run(i, dev), "a", name, K_A[variant], variant)


@pytest.mark.parametrize("name", B_SHAPES)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_bias_entry_selects_one_window_member(dev, select_variant, variant, name):
    select_variant(variant)
    _check_selection([_run(i, dev) for i in _inputs("b", name, "bfloat16")], name, K_A[variant], variant)


@pytest.mark.parametrize("name", C_SHAPES)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_large_logits(dev, select_variant, variant, name):
    select_variant(variant)
    _check_unit(lambda i: _run(i, dev), "c", name, K_C[variant], variant)


@pytest.mark.parametrize("name", GUARD_SHAPES)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_kernel_reads_and_writes_only_its_rows(dev, select_variant, variant, name):
    select_variant(variant)
    _check_guarded(_run_guarded(_inputs("a", name, "bfloat16")[0], dev), name, K_A[variant], variant)


# ------------------------------------------------------------------------------------------------ dense7: its own shapes, nothing set
@pytest.mark.parametrize("name", list(DENSE7_SHAPES))
def test_dense7_unit_normal_inputs_against_float64(dev, select_variant, name):
    select_variant("dense7")
    _check_unit(lambda i: _run(i, dev), "a", "dense7_" + name, K_A["dense7"], "dense7")


def test_dense7_bias_entry_selects_one_window_member(dev, select_variant):
    select_variant("dense7")
    name = "dense7_21x21_d3"
    _check_selection([_run(i, dev) for i in _inputs("b", name, "bfloat16")], name, K_A["dense7"], "dense7")


def test_dense7_reads_and_writes_only_its_rows(dev, select_variant):
    select_variant("dense7")
    name = "dense7_vpad_28x28_r16x16_d4"
    _check_guarded(_run_guarded(_inputs("a", name, "bfloat16")[0], dev), name, K_A["dense7"], "dense7")


# ------------------------------------------------------------------------------------------------ the bfloat16 v_dot2 kernel: one child
# (a) also on the float32 shapes: launch_typed picks this kernel's tile (4 / 8 / 16) from the shape for both dtypes
VALU_A_SHAPES = list(SHAPES) + ["f32_" + n for n in F32_SHAPES if n not in SHAPES]
VALU_CASES = ([("a", n) for n in VALU_A_SHAPES] + [("b", n) for n in B_SHAPES] + [("c", n) for n in C_SHAPES] + [("guard", n) for n in GUARD_SHAPES])


def _valu_child(outdir):
    """Runs in a fresh process with PPNET_NA_VALU=1 (read once per process): every case in sequence, outputs to outdir."""
    assert os.environ.get("PPNET_NA_VALU") == "1"
    dev = torch.device("cuda", 0)
    res = {}
    for kind, name in VALU_CASES:
        if kind == "guard":
            res[f"guard/{name}"] = _run_guarded(_inputs("a", name, "bfloat16")[0], dev)
        else:
            res[f"{kind}/{name}"] = [_run(i, dev) for i in _inputs(kind, name, "bfloat16")]
    torch.save(res, os.path.join(outdir, "out.pt"))


@pytest.fixture(scope="module")
def valu_outputs(dev):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS + PROCESS_KNOBS}
    env.update(PPNET_NA_VALU="1", PYTHONPATH=ROOT)
    with tempfile.TemporaryDirectory() as td:
        code = "import sys; from tests.test_gpu_na_variants import _valu_child; _valu_child(sys.argv[1])"
        subprocess.run([sys.executable, "-c", code, td], check=True, env=env, cwd=ROOT, timeout=300)
        return torch.load(os.path.join(td, "out.pt"))


@pytest.mark.parametrize("name", VALU_A_SHAPES)
def test_valu_bf16_unit_normal_inputs_against_float64(valu_outputs, name):
    _check_unit(lambda i: valu_outputs[f"a/{name}"][0], "a", name, K_A["valu_bf16"], "valu_bf16")


@pytest.mark.parametrize("name", B_SHAPES)
def test_valu_bf16_bias_entry_selects_one_window_member(valu_outputs, name):
    _check_selection(valu_outputs[f"b/{name}"], name, K_A["valu_bf16"], "valu_bf16")


@pytest.mark.parametrize("name", C_SHAPES)
def test_valu_bf16_large_logits(valu_outputs, name):
    _check_unit(lambda i: valu_outputs[f"c/{name}"][0], "c", name, K_C["valu_bf16"], "valu_bf16")


@pytest.mark.parametrize("name", GUARD_SHAPES)
def test_valu_bf16_reads_and_writes_only_its_rows(valu_outputs, name):
    _check_guarded(valu_outputs[f"guard/{name}"], name, K_A["valu_bf16"], "valu_bf16")


# ------------------------------------------------------------------------------------------------ float32: the tile follows the shape
@pytest.mark.parametrize("name", list(F32_SHAPES))
def test_f32_unit_normal_inputs_against_float64(dev, select_variant, name):
    select_variant("float32")
    _check_unit(lambda i: _run(i, dev), "a", "f32_" + name, None, "float32", "float32")


@pytest.mark.parametrize("name", B_SHAPES)
def test_f32_bias_entry_selects_one_window_member(dev, select_variant, name):
    select_variant("float32")
    _check_selection([_run(i, dev) for i in _inputs("b", name, "float32")], name, None, "float32", "float32")


@pytest.mark.parametrize("name", GUARD_SHAPES)
def test_f32_reads_and_writes_only_its_rows(dev, select_variant, name):
    select_variant("float32")
    _check_guarded(_run_guarded(_inputs("a", name, "float32")[0], dev), name, None, "float32", "float32")
