"""The LayerNorm inference kernels (csrc/fused_norm.hip norm_kernel) at the three-pass widths C / 8 = 3 * 2^k — 96, 192, 384, 768, 1536,
DiNAT-L's residual streams, and 24 / 48 on the padded form — through the three C entry points (ppn_residual_layernorm,
ppn_residual_layernorm_padded, ppn_layernorm_offset), float32 and bfloat16, every form: plain LN, residual + LN with and without gamma,
residual only, the float32 offset, the padded scatter.  The one- and two-pass widths 128, 256, 512, 1024 run through the same harness as
a guard (their bit-equality with the parent rests on their code not having changed, not on this test).

Reference: float64 on the same, already dtype-rounded, inputs.  With a residual the LayerNorm is taken of the stream the kernel stored
(x' rounded to the dtype: under bfloat16 the kernel normalises the rounded stream, as its header says), and that stream is itself
checked against the float64 x + gamma * a to 1 ulp of its dtype.
Bounds: float32 y: max |y - y64| <= 4 * max |F.layer_norm(float32 input) - y64| + 1 float32 ulp of max |y64| — the library's own error
on the same tensor, measured here; the factor 4 covers another summation order and is nothing against an indexing error, which is O(1).
bfloat16 y: |y - y64| <= 1 bfloat16 ulp of |y64| per element, plus that float32 allowance.
Row counts sit at the launch's edges: 1, a wave's rows - 1, a wave's rows + 1, a workgroup's rows + 3 (a workgroup holds
4 waves * (64 / lpr) rows * NORM_ROW_ITERS = 8 row groups)."""
import ctypes

import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

pytestmark = pytest.mark.gpu

NEW_WIDTHS = (96, 192, 384, 768, 1536)
OLD_WIDTHS = (128, 256, 512, 1024)
DTYPES = (torch.float32, torch.bfloat16)
FORMS = ("ln", "res_ln_gamma", "res_ln", "res_only", "offset")
NORM_ROW_ITERS = 8
EPS = 1e-5
MANT = {torch.float32: 23, torch.bfloat16: 7}


def geometry(C):
    """(passes, lanes per row) as launch_norm chooses them."""
    g = C // 8
    if g & (g - 1) == 0 and g <= 64:
        return 1, g
    if g == 128:
        return 2, 64
    assert g % 3 == 0 and (g // 3) & (g // 3 - 1) == 0 and g // 3 <= 64
    return 3, g // 3


def row_counts(C):
    rpw = 64 // geometry(C)[1]
    return sorted({1, max(rpw - 1, 1), rpw + 1, 4 * rpw * NORM_ROW_ITERS + 3})


def ulp(ref, dtype):
    """One unit in the last place of `dtype` at |ref| (float64 tensor)."""
    tiny = 2.0 ** -126
    return torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(tiny))) - MANT[dtype])


def operands(rows, C, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    chan = torch.rand(C, device="cuda", generator=g) * 4.0 - 2.0                       # a per-channel offset in [-2, 2]
    x = (torch.randn(rows, C, device="cuda", generator=g) + chan).to(dtype)
    a = torch.randn(rows, C, device="cuda", generator=g).to(dtype)
    gamma = (0.5 + torch.rand(C, device="cuda", generator=g)).to(dtype)
    w = (1.0 + 0.3 * torch.randn(C, device="cuda", generator=g)).to(dtype)
    b = (0.2 * torch.randn(C, device="cuda", generator=g)).to(dtype)
    off = (torch.rand(C, device="cuda", generator=g) * 2.0 - 1.0).contiguous()           # float32 whatever the dtype
    return x, a, gamma, w, b, off


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def launch(form, x, a, gamma, w, b, off, pad=None):
    """One call of the C entry point of `form`; returns (rc, x_out or None, y_out or None).  pad = (B, Hr, Wr, Hp, Wp)."""
    from ppnet_amd import _lib
    L = _lib.lib
    rows, C = x.shape
    dt = 0 if x.dtype == torch.float32 else 1
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    resid = form.startswith("res")
    x_out = torch.full_like(x, float("nan")) if resid else None
    want_y = form != "res_only"
    if pad is not None:
        B, Hr, Wr, Hp, Wp = pad
        y = torch.zeros(B * Hp * Wp, C, dtype=x.dtype, device="cuda")
        rc = L.ppn_residual_layernorm_padded(_ptr(x), _ptr(a if resid else None), _ptr(gamma if form == "res_ln_gamma" else None), _ptr(w), _ptr(b),
                                             _ptr(x_out), _ptr(y), rows, C, EPS, dt, Hr, Wr, Hp, Wp, stream)
    elif form == "offset":
        y = torch.full_like(x, float("nan"))
        rc = L.ppn_layernorm_offset(_ptr(x), _ptr(off), _ptr(w), _ptr(b), _ptr(y), rows, C, EPS, dt, stream)
    else:
        y = torch.full_like(x, float("nan")) if want_y else None
        g = gamma if form in ("res_ln_gamma", "res_only") else None
        rc = L.ppn_residual_layernorm(_ptr(x), _ptr(a if resid else None), _ptr(g), _ptr(w if want_y else None), _ptr(b if want_y else None),
                                      _ptr(x_out), _ptr(y), rows, C, EPS, dt, stream)
    torch.cuda.synchronize()
    return rc, x_out, y


def check_stream(x_out, x, a, gamma, tag):
    """x_out against the float64 x + gamma * a: within 1 ulp of its dtype."""
    ref = x.double() + (a.double() if gamma is None else gamma.double() * a.double())
    err = (x_out.double() - ref).abs()
    bad = err - ulp(ref, x.dtype)
    assert bool((bad <= 0).all()), (tag, "x_out", float(bad.max()))


def check_norm(y, z, w, b, dtype, tag, eps=EPS):
    """y against the float64 LayerNorm of z (a float64 tensor the dtype's values of which the kernel normalised)."""
    mean = z.mean(1, keepdim=True)
    var = z.var(1, unbiased=False, keepdim=True)
    y64 = (z - mean) / torch.sqrt(var + eps) * w.double() + b.double()
    lib = F.layer_norm(z.float(), (z.shape[1],), w.float(), b.float(), eps)                # the library's float32 error on the same tensor
    lib_err = float((lib.double() - y64).abs().max())
    allow = 4.0 * lib_err + float(ulp(y64.abs().max(), torch.float32))
    err = (y.double() - y64).abs()
    if dtype == torch.float32:
        assert float(err.max()) <= allow, (tag, float(err.max()), allow, lib_err)
    else:
        bad = err - (ulp(y64, torch.bfloat16) + allow)
        assert bool((bad <= 0).all()), (tag, float(bad.max()), allow)
    return float(err.max()), lib_err


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
@pytest.mark.parametrize("C", NEW_WIDTHS + OLD_WIDTHS)
def test_every_form_vs_float64(C, dtype):
    """The five unpadded forms at the four edge row counts.  On the parent the new widths return PPN_E_UNSUPPORTED (-3) here."""
    worst = 0.0
    for rows in row_counts(C):
        x, a, gamma, w, b, off = operands(rows, C, dtype, seed=C + rows)
        for form in FORMS:
            tag = (C, str(dtype), form, rows)
            rc, x_out, y = launch(form, x, a, gamma, w, b, off)
            assert rc == 0, (tag, rc)
            z = x.double()
            if form == "offset":
                z = z + off.double()
            if form.startswith("res"):
                g = gamma if form in ("res_ln_gamma", "res_only") else None
                check_stream(x_out, x, a, g, tag)
                z = x_out.double()                                                       # the LN sees the stored (dtype-rounded) stream
            if form == "res_only":
                assert y is None
                continue
            assert bool(torch.isfinite(y).all()), tag
            e, _ = check_norm(y, z, w, b, dtype, tag)
            worst = max(worst, e)
    print(f"C {C} {str(dtype)[6:]}: passes x lanes {geometry(C)}, rows {row_counts(C)}, worst |y - y64| {worst:.3e}")


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
@pytest.mark.parametrize("C", (24, 48) + NEW_WIDTHS + OLD_WIDTHS)
def test_padded_scatter(C, dtype):
    """3 images of 5 x 6 tokens scattered into 7 x 7 grids: the pad positions of a zeroed y_out stay zero, the tokens land at
    [b][i][j], x_out keeps the unpadded layout.  24 and 48 reach norm_kernel only on this form (one lane, two lanes x three passes)."""
    B, Hr, Wr, Hp, Wp = 3, 5, 6, 7, 7
    rows = B * Hr * Wr
    x, a, gamma, w, b, off = operands(rows, C, dtype, seed=7 * C)
    for form in ("ln", "res_ln_gamma"):
        tag = (C, str(dtype), form, "padded")
        rc, x_out, y = launch(form, x, a, gamma, w, b, off, pad=(B, Hr, Wr, Hp, Wp))
        assert rc == 0, (tag, rc)
        grid = y.view(B, Hp, Wp, C)
        assert bool((grid[:, Hr:] == 0).all()) and bool((grid[:, :, Wr:] == 0).all()), tag
        z = x.double()
        if form == "res_ln_gamma":
            check_stream(x_out, x, a, gamma, tag)
            z = x_out.double()
        check_norm(grid[:, :Hr, :Wr].reshape(rows, C), z, w, b, dtype, tag)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
@pytest.mark.parametrize("C", (520, 2048, 40 * 8, 1536 * 2))
def test_other_widths_stay_unsupported(C, dtype):
    from ppnet_amd import _lib, fused
    ln = torch.nn.LayerNorm(C).to("cuda", dtype)
    x = torch.randn(4, 2, 3, C, device="cuda").to(dtype)
    with torch.no_grad():
        for call in (lambda: fused.layer_norm(x, ln), lambda: fused.layer_norm(x, ln, offset=torch.zeros(C, device="cuda")),
                     lambda: fused.layer_norm(x, ln, pad_to=(7, 7)), lambda: fused.residual_layer_norm(x.clone(), x, None, ln),
                     lambda: fused.residual_layer_norm(x.clone(), x, ln.weight, None)):
            with pytest.raises(_lib.PpnError) as e:
                call()
            assert e.value.code == _lib.PPN_E_UNSUPPORTED


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
def test_768_kernel_by_layer_norm_framework_by_any_width(dtype, monkeypatch):
    """fused.layer_norm at 768 (DiNAT-L's level 2) runs the kernel; fused.layer_norm_any_width (ViT-B's and the SETR-UP head's call)
    keeps the framework's LayerNorm at 768 — LN_FRAMEWORK_WIDTHS — and takes the kernel at 1536 (DiNAT-L's head)."""
    from ppnet_amd import fused
    assert fused.LN_FRAMEWORK_WIDTHS == frozenset({768})
    for C in (768, 1536):
        ln = torch.nn.LayerNorm(C, eps=1e-6).to("cuda", dtype)
        with torch.no_grad():
            ln.weight.uniform_(0.5, 1.5); ln.bias.uniform_(-0.5, 0.5)
            x = (torch.randn(2, 5, 7, C, device="cuda") + 0.5).to(dtype)
            lib = F.layer_norm(x, (C,), ln.weight, ln.bias, ln.eps)
            calls = []
            own = fused.layer_norm
            monkeypatch.setattr(fused, "layer_norm", lambda *a, **k: (calls.append(1), own(*a, **k))[1])
            y_any = fused.layer_norm_any_width(x, ln)
            monkeypatch.setattr(fused, "layer_norm", own)
            y_k = fused.layer_norm(x, ln)
        if C == 768:
            assert not calls and torch.equal(y_any, lib)
        else:
            assert calls and torch.equal(y_any, y_k)
        check_norm(y_k.view(-1, C), x.double().view(-1, C), ln.weight.detach(), ln.bias.detach(), dtype, (C, str(dtype), "fused.layer_norm"), eps=ln.eps)
