"""ppn_patch_merge_ln_fwd / ppn_patch_merge_ln_bwd (csrc/patch_merge_ln.hip) on the device: DiNAT_s's 2 x 2 patch gather fused with the
LayerNorm over 4C, forward and backward, float32 and bfloat16.

Reference: float64 CPU autograd of the composition (pad, four strided slices, cat, F.layer_norm) on the kernel's own input values.
Bound, for every output (y, dx, dgamma, dbeta) — tests/test_gpu_residual_ln_bwd.py's rule for the same kind of sums:

    max|kernel - ref|  <=  2 * max|library - ref|  +  eps(dtype) * max|ref|

where `library` is the PPNET_LIBRARY_MERGE=1 composition on the GPU in the same dtype on the same inputs in the same test, and eps(dtype)
is one unit in the last place at the output's magnitude (2^-23 float32, 2^-7 bfloat16).  Raw calls go through ctypes on NaN-filled,
canary-guarded buffers (test_gpu_dice.py's _guarded): no NaN survives in dx — every element is written, odd sizes included — and the
canaries are intact.  Constant rows use values whose row sums are exact in float32 (halves up to 4: 2048 of them stay below 2^24
halves), so the mean is the value itself, the centred row is exactly zero and y is beta's bits.

Every case prints its figures.  Measured on the device, worst over all cases, kernel error / library error: float32 y 1.21, dx 2.42
(6.5e-8 against 2.7e-8 of the magnitude at one row of 32 values: inside the one-ulp term), dgamma 1.45, dbeta 1.82, at most 0.65 of the
bound (dgamma at randn + 100: 2.5e-6 against 1.9e-6); bfloat16 1.00 on every output of every case, at most 0.23 of the bound (DESIGN.md
section 24).  With the reciprocal-square-root instruction for rstd and one 32-long chain per lane for the row sums the float32 y missed
the bound at 2x3x5x16 and 1x13x17x32 (3.7e-7 against 1.1e-7): the kernel computes 1 / sqrt and sums piece by piece."""
import ctypes as C

import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

from tests.test_gpu_dice import PAD, _guarded  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.bfloat16]
IDS = {torch.float32: "f32", torch.bfloat16: "bf16"}
DT = {torch.float32: 0, torch.bfloat16: 1}
EPS = 1e-5
NAN = float("nan")

#          B  H  W  C
SHAPES = [(1, 2, 2, 8),            # one row
          (1, 1, 1, 64),           # a lone token with three zero quadrants
          (2, 7, 5, 32),           # both sizes odd
          (3, 6, 9, 128),          # W odd
          (1, 9, 6, 256),          # H odd
          (1, 4, 4, 512),          # the widest row
          (1, 13, 17, 32), (1, 16, 16, 32), (1, 9, 25, 32),      # R - 1, R and R + 1 rows at C = 32 (R = 64 rows per workgroup)
          (2, 3, 5, 16)]           # two images, a narrow row: 128 rows per tile, 12 live
STRIDE_SHAPE = (1, 33, 481, 512)   # 17 * 241 = 4097 rows = cap * R + 1 at C = 512 (R = 4): the stride loop runs twice


def _rows(shape):
    B, H, W, _ = shape
    return B * -(-H // 2) * -(-W // 2)


def test_shapes_sit_where_they_claim_to():
    from ppnet_amd import _lib
    rows_of, cap = _lib.lib.ppn_patch_merge_ln_rows, _lib.lib.ppn_patch_merge_ln_max_blocks()
    assert {s[3] for s in SHAPES} >= {8, 32, 64, 128, 256, 512} and all(rows_of(s[3]) > 0 for s in SHAPES)
    R = rows_of(32)
    assert R == 64 and {R - 1, R, R + 1} <= {_rows(s) for s in SHAPES if s[3] == 32}
    assert _rows((1, 2, 2, 8)) == 1 and _rows((1, 1, 1, 64)) == 1
    assert any(s[1] % 2 and s[2] % 2 for s in SHAPES) and any(s[1] % 2 and not s[2] % 2 for s in SHAPES)
    assert any(s[2] % 2 and not s[1] % 2 for s in SHAPES) and any(s[0] > 1 for s in SHAPES)
    assert STRIDE_SHAPE[3] == 512 and _rows(STRIDE_SHAPE) == cap * rows_of(512) + 1
    assert -(-_rows(STRIDE_SHAPE) // rows_of(512)) == cap + 1            # one tile more than there are workgroups
    assert all(_rows(s) <= cap * rows_of(s[3]) for s in SHAPES)          # the others: a tile per workgroup at the most


# ------------------------------------------------------------------------------------------------ inputs, references
def _inputs(shape, dtype, kind="randn", seed=0):
    """(x, gamma, beta, gy) on the device in `dtype`."""
    B, H, W, Cc = shape
    g = torch.Generator().manual_seed(1000 * seed + 7 * H + W + Cc)
    Ho, Wo = -(-H // 2), -(-W // 2)
    if kind == "randn":
        x = torch.randn(shape, generator=g)
    elif kind == "offset":                                                  # cancellation in a one-pass variance
        x = torch.randn(shape, generator=g) + 100.0
    elif kind == "constant":                                                # every gathered row constant (even sizes): exact sums
        assert H % 2 == 0 and W % 2 == 0
        c = torch.randint(-8, 9, (B, Ho, 1, Wo, 1, 1), generator=g).float() * 0.5
        x = c.expand(B, Ho, 2, Wo, 2, Cc).reshape(shape).clone()
    else:
        x = torch.zeros(shape)
    gamma = torch.empty(4 * Cc).uniform_(0.7, 1.3, generator=g)
    beta = torch.empty(4 * Cc).uniform_(-0.2, 0.2, generator=g)
    gy = torch.randn(B, Ho, Wo, 4 * Cc, generator=g)
    return tuple(t.to(dtype).to(DEV).contiguous() for t in (x, gamma, beta, gy))


def _composition(x, gamma, beta, gy):
    from ppnet_amd import fused
    x, gamma, beta = (t.detach().clone().requires_grad_(True) for t in (x, gamma, beta))
    y = F.layer_norm(fused.patch_merge_gather(x), (gamma.numel(),), gamma, beta, EPS)
    dx, dgamma, dbeta = torch.autograd.grad(y, [x, gamma, beta], gy)
    return {"y": y.detach(), "dx": dx, "dgamma": dgamma, "dbeta": dbeta}


def _reference(x, gamma, beta, gy):
    """float64 on the CPU, from the values the kernel reads."""
    return _composition(*(t.double().cpu() for t in (x, gamma, beta, gy)))


def _ln(gamma, beta):
    ln = torch.nn.LayerNorm(gamma.numel(), eps=EPS).to(device=DEV, dtype=gamma.dtype)
    with torch.no_grad():
        ln.weight.copy_(gamma); ln.bias.copy_(beta)
    return ln


def _library(x, gamma, beta, gy, monkeypatch):
    """The PPNET_LIBRARY_MERGE=1 composition through the wrapper on the GPU, in the inputs' dtype."""
    from ppnet_amd import fused
    monkeypatch.setenv("PPNET_LIBRARY_MERGE", "1")
    calls = dict(fused.MERGE_CALLS)
    ln = _ln(gamma, beta)
    xr = x.clone().requires_grad_(True)
    y = fused.patch_merge_ln(xr, ln)
    dx, dgamma, dbeta = torch.autograd.grad(y, [xr, ln.weight, ln.bias], gy)
    monkeypatch.delenv("PPNET_LIBRARY_MERGE")
    assert fused.MERGE_CALLS == calls
    return {"y": y.detach(), "dx": dx, "dgamma": dgamma, "dbeta": dbeta}


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _raw(x, gamma, beta, gy, stats=True, dgamma=True, dbeta=True, backward=True):
    """The entry points straight through ctypes on NaN-filled, canary-guarded buffers: dict of y, stats, dx, dgamma, dbeta, ws (None where
    not asked for).  Asserts the return codes, the canaries and that nothing but the outputs changed."""
    from ppnet_amd import _lib
    B, H, W, Cc = x.shape
    rows, dt = _rows(x.shape), x.dtype
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    keep = [t.clone() for t in (x, gamma, beta, gy)]
    y, y_ok = _guarded(rows * 4 * Cc, dt, NAN)
    st, st_ok = _guarded(rows * 2, torch.float32, NAN) if stats else (None, lambda: True)
    assert _lib.lib.ppn_patch_merge_ln_fwd(_p(x), _p(gamma), _p(beta), _p(y), _p(st), B, H, W, Cc, EPS, DT[dt], stream) == 0
    torch.cuda.synchronize()
    assert y_ok() and st_ok()
    out = {"y": y.view(B, -(-H // 2), -(-W // 2), 4 * Cc), "stats": st.view(rows, 2) if stats else None, "dx": None, "dgamma": None,
           "dbeta": None, "ws": None}
    if backward:
        assert stats
        need = _lib.lib.ppn_patch_merge_ln_bwd_workspace(B, H, W, Cc)
        assert need > 0 and need % 16 == 0
        ws, ws_ok = _guarded(need // 4, torch.float32, NAN)
        dx, dx_ok = _guarded(x.numel(), dt, NAN)
        dg, dg_ok = _guarded(4 * Cc, dt, NAN) if dgamma else (None, lambda: True)
        db, db_ok = _guarded(4 * Cc, dt, NAN) if dbeta else (None, lambda: True)
        st_keep = st.clone()
        assert _lib.lib.ppn_patch_merge_ln_bwd(_p(gy), _p(x), _p(st), _p(gamma), _p(ws), _p(dx), _p(dg), _p(db), B, H, W, Cc, DT[dt], stream) == 0
        torch.cuda.synchronize()
        assert ws_ok() and dx_ok() and dg_ok() and db_ok() and st_ok() and y_ok() and torch.equal(st, st_keep)
        out.update(dx=dx.view(x.shape), dgamma=dg, dbeta=db, ws=ws)
    for t, k in zip((x, gamma, beta, gy), keep):
        assert torch.equal(t, k)                                            # the inputs are read only
    return out


def _check(what, got, ref, lib, dtype, capsys):
    eps = torch.finfo(dtype).eps
    line = []
    for name in ("y", "dx", "dgamma", "dbeta"):
        g, r, l = got[name].double().cpu(), ref[name], lib[name].double().cpu()
        assert g.shape == r.shape == l.shape, (what, name)
        assert bool(torch.isfinite(g).all()), (what, name)                  # no NaN of the fill survives: every element is written
        m = float(r.abs().max())
        ek, el = float((g - r).abs().max()), float((l - r).abs().max())
        tol = 2.0 * el + eps * m
        line.append(f"{name} {ek / m if m else ek:.2e} / {el / m if m else el:.2e} ({ek / tol if tol else 0.0:.2f} of the bound)")
        with capsys.disabled():
            if name == "dbeta":
                print(f"\npatch_merge_ln {IDS[dtype]} {what}: kernel / library error over max|ref|: " + ", ".join(line), end="")
        assert ek <= tol, (what, name, ek, el, m)


def _stats_check(got, x):
    """(mean, rstd) of every row against float64."""
    from ppnet_amd import fused
    rows = fused.patch_merge_gather(x.double().cpu()).flatten(0, 2)
    mean, var = rows.mean(1), rows.var(1, unbiased=False)
    st = got["stats"].double().cpu()
    assert float((st[:, 0] - mean).abs().max()) <= 4e-6 * max(1.0, float(mean.abs().max()))
    rstd = (var + EPS).rsqrt()
    assert float(((st[:, 1] - rstd) / rstd).abs().max()) <= 1e-3          # bfloat16 rows at +-100: var of O(1) from float32 squares


# ------------------------------------------------------------------------------------------------ shapes and values
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("shape", SHAPES + [STRIDE_SHAPE], ids=lambda s: "x".join(map(str, s)))
def test_kernels_vs_float64(shape, dtype, monkeypatch, capsys):
    args = _inputs(shape, dtype)
    got = _raw(*args)
    _check("x".join(map(str, shape)), got, _reference(*args), _library(*args, monkeypatch), dtype, capsys)
    _stats_check(got, args[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("shape", [(2, 7, 5, 32), (1, 9, 6, 256), (1, 4, 4, 512)], ids=lambda s: "x".join(map(str, s)))
def test_rows_with_a_large_mean(shape, dtype, monkeypatch, capsys):
    """randn + 100: mean first, then the centred squares — a one-pass variance loses these rows."""
    args = _inputs(shape, dtype, "offset", seed=1)
    got = _raw(*args)
    _check("x".join(map(str, shape)) + " +100", got, _reference(*args), _library(*args, monkeypatch), dtype, capsys)
    _stats_check(got, args[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("kind", ["constant", "zeros"])
@pytest.mark.parametrize("shape", [(2, 6, 4, 32), (1, 4, 4, 512), (1, 2, 2, 8)], ids=lambda s: "x".join(map(str, s)))
def test_constant_rows_give_beta_exactly(shape, kind, dtype, monkeypatch, capsys):
    x, gamma, beta, gy = args = _inputs(shape, dtype, kind, seed=2)
    got = _raw(*args)
    assert torch.equal(got["y"], beta.expand_as(got["y"]))                  # the centred row is exactly zero
    assert bool(torch.isfinite(got["dx"]).all()) and bool(torch.isfinite(got["dgamma"]).all()) and bool(torch.isfinite(got["dbeta"]).all())
    st = got["stats"]
    rows = x.view(x.shape[0], shape[1] // 2, 2, shape[2] // 2, 2, shape[3])[:, :, 0, :, 0, 0].reshape(-1)
    assert torch.equal(st[:, 0], rows.float()) and torch.equal(st[:, 1], torch.full_like(st[:, 1], float(st[0, 1])))
    assert float(st[0, 1]) == pytest.approx(EPS ** -0.5, rel=1e-6)
    assert torch.equal(got["dgamma"], torch.zeros_like(got["dgamma"]))      # xhat is exactly zero
    _check("x".join(map(str, shape)) + " " + kind, got, _reference(*args), _library(*args, monkeypatch), dtype, capsys)


def test_odd_sizes_pad_with_zeros_and_drop_the_pads_gradient():
    """(1,1,1,64): three quadrants of the only row are padding.  They enter the statistics as zeros, y there is the LayerNorm of a zero,
    and dx has the lone token's C values only."""
    x, gamma, beta, gy = args = _inputs((1, 1, 1, 64), torch.float32)
    got = _raw(*args)
    row = torch.cat([x.view(-1), torch.zeros(192, device=DEV)]).double()
    mean, var = row.mean(), row.var(unbiased=False)
    assert float(got["stats"][0, 0]) == pytest.approx(float(mean), rel=1e-6) and float(got["stats"][0, 1]) == pytest.approx(float((var + EPS).rsqrt()), rel=1e-6)
    pad_y = (0.0 - mean) * (var + EPS).rsqrt() * gamma[64:].double() + beta[64:].double()
    assert float((got["y"].view(-1)[64:].double() - pad_y).abs().max()) < 1e-6
    assert got["dx"].shape == (1, 1, 1, 64) and bool(torch.isfinite(got["dx"]).all())


# ------------------------------------------------------------------------------------------------ determinism, optional pointers
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("shape", [(2, 7, 5, 32), STRIDE_SHAPE], ids=lambda s: "x".join(map(str, s)))
def test_three_runs_are_bit_equal(shape, dtype):
    args = _inputs(shape, dtype, seed=3)
    first = _raw(*args)
    for _ in range(2):
        again = _raw(*args)
        for k in ("y", "stats", "dx", "dgamma", "dbeta"):
            assert torch.equal(first[k], again[k]), k


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_null_stats_dgamma_and_dbeta_are_honoured(dtype):
    args = _inputs((3, 6, 9, 128), dtype, seed=4)
    full = _raw(*args)
    inference = _raw(*args, stats=False, backward=False)
    assert inference["stats"] is None and torch.equal(inference["y"], full["y"])
    only_gamma, only_beta, neither = _raw(*args, dbeta=False), _raw(*args, dgamma=False), _raw(*args, dgamma=False, dbeta=False)
    for run in (only_gamma, only_beta, neither):
        assert torch.equal(run["dx"], full["dx"]) and torch.equal(run["y"], full["y"])
    assert only_gamma["dbeta"] is None and torch.equal(only_gamma["dgamma"], full["dgamma"])
    assert only_beta["dgamma"] is None and torch.equal(only_beta["dbeta"], full["dbeta"])
    assert bool(torch.isnan(neither["ws"]).all())                           # no sums wanted: the workspace is not touched
    assert not bool(torch.isnan(full["ws"]).any())                          # one [2][4C] partial per workgroup, all of it written


# ------------------------------------------------------------------------------------------------ the wrapper
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_wrapper_returns_the_raw_bits_and_saves_x_stats_gamma(dtype, monkeypatch):
    from ppnet_amd import fused
    monkeypatch.delenv("PPNET_LIBRARY_MERGE", raising=False)
    shape = (2, 7, 5, 32)
    x, gamma, beta, gy = args = _inputs(shape, dtype, seed=5)
    raw = _raw(*args)
    ln = _ln(gamma, beta)
    assert fused.patch_merge_ln_ok(x, ln)
    calls = dict(fused.MERGE_CALLS)
    with torch.no_grad():
        y = fused.patch_merge_ln(x, ln)
    assert torch.equal(y, raw["y"]) and fused.MERGE_CALLS == {"fwd": calls["fwd"] + 1, "bwd": calls["bwd"]}
    xr = x.clone().requires_grad_(True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append((tuple(t.shape), t.dtype)), t)[1], lambda t: t):
        y = fused.patch_merge_ln(xr, ln)
    assert saved == [(shape, dtype), ((_rows(shape), 2), torch.float32), ((4 * shape[3],), dtype)], saved
    dx, dgamma, dbeta = torch.autograd.grad(y, [xr, ln.weight, ln.bias], gy)
    assert fused.MERGE_CALLS == {"fwd": calls["fwd"] + 2, "bwd": calls["bwd"] + 1}
    assert torch.equal(y, raw["y"]) and torch.equal(dx, raw["dx"]) and torch.equal(dgamma, raw["dgamma"]) and torch.equal(dbeta, raw["dbeta"])
    # a float32 LayerNorm in front of bfloat16 tokens (the later levels of an autocast step): the float32 kernels on the same values, as
    # autocast runs a LayerNorm; dx comes back in the tokens' dtype, the parameters' gradients in float32
    if dtype == torch.bfloat16:
        raw32 = _raw(x.float(), gamma.float(), beta.float(), gy.float())
        ln32 = _ln(gamma.float(), beta.float())
        xr = x.clone().requires_grad_(True)
        y = fused.patch_merge_ln(xr, ln32)
        g = torch.autograd.grad(y, [xr, ln32.weight, ln32.bias], gy.float())
        assert y.dtype == torch.float32 and torch.equal(y, raw32["y"]) and g[0].dtype == dtype and torch.equal(g[0], raw32["dx"].to(dtype))
        assert g[1].dtype == torch.float32 and torch.equal(g[1], raw32["dgamma"]) and torch.equal(g[2], raw32["dbeta"])
        with torch.no_grad():
            assert torch.equal(fused.patch_merge_ln(x, ln32), raw32["y"])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_knob_and_unsupported_widths_make_no_launch(dtype, monkeypatch):
    from ppnet_amd import fused
    monkeypatch.delenv("PPNET_LIBRARY_MERGE", raising=False)
    calls = dict(fused.MERGE_CALLS)
    for Cc in (12, 96, 1024):                                               # outside the kernel's set: the torch composition, no error
        x, gamma, beta, gy = _inputs((1, 3, 5, Cc), dtype, seed=6)
        ln = _ln(gamma, beta)
        assert not fused.patch_merge_ln_ok(x, ln)
        with torch.no_grad():
            y = fused.patch_merge_ln(x, ln)
        assert torch.equal(y, F.layer_norm(fused.patch_merge_gather(x), (4 * Cc,), gamma, beta, EPS))
        xr = x.clone().requires_grad_(True)
        torch.autograd.grad(fused.patch_merge_ln(xr, ln), [xr, ln.weight, ln.bias], gy)
    x, gamma, beta, gy = _inputs((2, 7, 5, 32), dtype, seed=6)
    ln = _ln(gamma, beta)
    monkeypatch.setenv("PPNET_LIBRARY_MERGE", "1")                          # read at call time, in both modes
    assert not fused.patch_merge_ln_ok(x, ln)
    with torch.no_grad():
        y = fused.patch_merge_ln(x, ln)
    assert torch.equal(y, F.layer_norm(fused.patch_merge_gather(x), (128,), gamma, beta, EPS))
    xr = x.clone().requires_grad_(True)
    torch.autograd.grad(fused.patch_merge_ln(xr, ln), [xr, ln.weight, ln.bias], gy)
    assert fused.MERGE_CALLS == calls
    monkeypatch.delenv("PPNET_LIBRARY_MERGE")
    assert fused.patch_merge_ln_ok(x, ln)
    assert not fused.patch_merge_ln_ok(x.double(), ln) and not fused.patch_merge_ln_ok(x.half(), ln)
    assert not fused.patch_merge_ln_ok(x.cpu(), ln) and not fused.patch_merge_ln_ok(x[0], ln)
    assert PAD >= 16                                                        # (the canaries of every raw call above)
