"""ppn_mhsa_fwd / ppn_mhsa_bwd at head dim 8 (csrc/mhsa_d8.hip) on the GPU: the kernels against float64 autograd of the definition,
known answers, bitwise reproducibility, the memory they may touch, GenNet's AE-ViT through the kernel path (the reference's golden
numbers, parameter gradients, peak memory) and training steps.

The precision rule, forward and backward (DESIGN section 12's): err = max|got - ref| / max|ref| over EVERY element, for out, dq, dk
and dv apart; ref = float64 autograd of softmax(scale q k^T) v on the CPU (bfloat16: on the rounded inputs); err <= max(2 x the
error of the explicit matmul / softmax chain in the same data type on the same inputs, measured in the same run; 2e-6 float32,
1e-2 bfloat16).  The chain is neither SDPA nor the code under test.  A reference that is exactly 0 asks for exactly 0.

The kernels' own sizes (csrc/mhsa_d8.hip): a workgroup owns 256 rows (128 lanes x 2 rows: the query block of the forward, the
statistics and dQ, the key block of dK / dV), the other side comes in LDS tiles of 128 rows, whose sums are formed 16 rows at a time.
The shapes below sit one below, at and one above each of 16, 128 and 256.

Each test prints what it measured (run with -s); the worst figures per data type are in profiles/r12_gennet_attention_precision.txt."""
import copy
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda"
HD = 8
SCALE = HD ** -0.5
FLOOR = {torch.float32: 2e-6, torch.bfloat16: 1e-2}
ROW_BLOCK, TILE, CHUNK = 256, 128, 16                          # mhsa_d8.hip: D8_RB, D8_KT, D8_CH
SHAPES = ([(1, 1, 1), (2, 7, 3)]
          + [(1, n, 2) for s in (CHUNK, TILE, ROW_BLOCK) for n in (s - 1, s, s + 1)]
          + [(2, 784, 3), (2, 1024, 3), (1, 1025, 5)])
DTYPES = [torch.float32, torch.bfloat16]
NAMES = ("out", "dq", "dk", "dv")


def _definition(qkv, dout, heads, scale):
    """(out, dqkv) of softmax(scale q k^T) v by matmul / softmax under autograd, in qkv's dtype on qkv's device."""
    B, N, _ = qkv.shape
    t = qkv.detach().clone().requires_grad_(True)
    u = t.view(B, N, 3, heads, HD).permute(2, 0, 3, 1, 4)                  # [3, B, heads, N, 8]
    p = torch.softmax((u[0] @ u[1].transpose(-1, -2)) * scale, dim=-1)
    out = (p @ u[2]).permute(0, 2, 1, 3).reshape(B, N, heads * HD)
    g, = torch.autograd.grad(out, t, dout)
    return out.detach(), g


def _kernel(qkv, dout, heads, scale):
    """(out, dqkv) through vit.mhsa_autograd (ppn_mhsa_fwd forward, ppn_mhsa_bwd backward)."""
    from ppnet_amd import vit
    t = qkv.detach().clone().requires_grad_(True)
    out = vit.mhsa_autograd(t, heads, scale)
    g, = torch.autograd.grad(out, t, dout)
    torch.cuda.synchronize()
    return out.detach(), g


def _rel(got, ref):
    d, r = (got.double().cpu() - ref).abs().max().item(), ref.abs().max().item()
    return d / r if r > 0 else (0.0 if d == 0 else float("inf"))


def _errors(out, g, ref_out, ref_g, heads):
    """max|got - ref| / max|ref| of out, dq, dk, dv (every element); a reference that is exactly 0 asks for exactly 0."""
    B, N, _ = ref_g.shape
    g = g.view(B, N, 3, heads * HD)
    ref_g = ref_g.view(B, N, 3, heads * HD)
    return [_rel(out, ref_out)] + [_rel(g[:, :, i], ref_g[:, :, i]) for i in range(3)]


def _measure(qkv, dout, heads, scale, dtype):
    """(kernel errors, chain errors, bounds) for out, dq, dk, dv on inputs already rounded to dtype."""
    ref_out, ref_g = _definition(qkv.double(), dout.double(), heads, scale)             # float64, CPU
    ch_out, ch_g = _definition(qkv.to(DEV), dout.to(DEV), heads, scale)
    out, g = _kernel(qkv.to(DEV), dout.to(DEV), heads, scale)
    assert out.dtype == g.dtype == dtype and g.shape == qkv.shape and out.shape == dout.shape
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(g).all())
    ek, ec = _errors(out, g, ref_out, ref_g, heads), _errors(ch_out, ch_g, ref_out, ref_g, heads)
    return ek, ec, [max(2.0 * c, FLOOR[dtype]) for c in ec]


def _fmt(v):
    return " ".join(f"{x:.2e}" for x in v)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,N,heads", SHAPES)
def test_kernel_vs_float64(dtype, B, N, heads, capsys):
    g = torch.Generator().manual_seed(1000 * N + 10 * heads + B)
    qkv = torch.randn(B, N, 3 * heads * HD, generator=g).to(dtype)
    dout = torch.randn(B, N, heads * HD, generator=g).to(dtype)
    ek, ec, bound = _measure(qkv, dout, heads, SCALE, dtype)
    with capsys.disabled():
        print(f"\nmhsa_d8 {str(dtype)[6:]} B {B} N {N} heads {heads}: out dq dk dv kernel {_fmt(ek)} | chain {_fmt(ec)} | bound {_fmt(bound)}")
    for name, e, b in zip(NAMES, ek, bound):
        assert e <= b, (name, B, N, heads, e, b)


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _raw_fwd(qkv, heads, scale, out=None, B=None, N=None):
    from ppnet_amd import _lib as L
    B = qkv.shape[0] if B is None else B
    N = qkv.shape[1] if N is None else N
    if out is None:
        out = torch.empty(B, N, heads * HD, dtype=qkv.dtype, device=DEV)
    rc = L.lib.ppn_mhsa_fwd(_P(qkv), _P(out), B, N, heads, HD, float(scale), 0 if qkv.dtype == torch.float32 else 1, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    return out


def _raw_bwd(qkv, out, dout, heads, scale, dqkv=None, ws=None, B=None, N=None):
    """ppn_mhsa_bwd itself on device tensors; the workspace is NaN before the call unless the caller brings one."""
    from ppnet_amd import _lib as L
    B = qkv.shape[0] if B is None else B
    N = qkv.shape[1] if N is None else N
    need = L.lib.ppn_mhsa_bwd_workspace(B, N, heads)
    assert need >= 2 * B * heads * N
    if dqkv is None:
        dqkv = torch.empty(B, N, 3 * heads * HD, dtype=qkv.dtype, device=DEV)
    if ws is None:
        ws = torch.full((need,), float("nan"), dtype=torch.float32, device=DEV)
    rc = L.lib.ppn_mhsa_bwd(_P(qkv), _P(out), _P(dout), _P(dqkv), _P(ws), need, B, N, heads, HD, float(scale),
                            0 if qkv.dtype == torch.float32 else 1, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    return dqkv


@pytest.mark.parametrize("dtype", DTYPES)
def test_known_answers(dtype, capsys):
    heads = 3
    name = str(dtype)[6:]
    g = torch.Generator().manual_seed(21)
    # N = 1: P = 1 whatever q and k are -> out = v, dq = dk = 0 and dv = dout, all exactly
    qkv = torch.randn(3, 1, 3 * heads * HD, generator=g).to(dtype).to(DEV)
    dout = torch.randn(3, 1, heads * HD, generator=g).to(dtype).to(DEV)
    out, got = _kernel(qkv, dout, heads, SCALE)
    got = got.view(3, 1, 3, heads * HD)
    assert torch.equal(out, qkv.view(3, 1, 3, heads * HD)[:, :, 2])
    assert bool((got[:, :, 0] == 0).all()) and bool((got[:, :, 1] == 0).all())
    assert torch.equal(got[:, :, 2], dout)

    # all keys equal: P is uniform and every row of dS sums to 0 -> dq = scale (sum_j dS_ij) k = 0 to rounding.  Measured against
    # the same sum without cancellation, scale sum_j |dS_ij| |k|, with the forward bound of the data type (section 12).
    B, N = 2, 300
    q = torch.randn(B, N, heads, HD, generator=g)
    k = torch.randn(B, 1, heads, HD, generator=g).expand(B, N, heads, HD)
    v = torch.randn(B, N, heads, HD, generator=g)
    qkv = torch.stack([q, k, v], 2).reshape(B, N, 3 * heads * HD).to(dtype)
    dout = torch.randn(B, N, heads * HD, generator=g).to(dtype)
    out, got = _kernel(qkv.to(DEV), dout.to(DEV), heads, SCALE)
    got = got.double().cpu().view(B, N, 3, heads, HD)
    t = qkv.double().view(B, N, 3, heads, HD).permute(2, 0, 3, 1, 4)
    do = dout.double().view(B, N, heads, HD).permute(0, 2, 1, 3)
    dp = do @ t[2].transpose(-1, -2)                                                   # P = 1 / N
    ds = (dp - dp.mean(-1, keepdim=True)) / N
    nocancel = (SCALE * ds.abs().sum(-1, keepdim=True) * t[1].abs()).max().item()
    dq = got[:, :, 0].abs().max().item()
    mean_v = t[2].mean(2, keepdim=True).expand(B, heads, N, HD).permute(0, 2, 1, 3).reshape(B, N, heads * HD)
    eo = _rel(out, mean_v)
    with capsys.disabled():
        print(f"\nmhsa_d8 {name} equal keys: max|dq| {dq:.2e} = {dq / nocancel:.2e} x the uncancelled sum; out vs mean(v) {eo:.2e}")
    assert dq <= FLOOR[dtype] * nocancel
    assert eo <= FLOOR[dtype]

    # one-hot rows: for query i the key at 37 (i mod 8) has a logit of 50, every other key 0 -> out = that key's v row to one
    # rounding step (the other 299 keys weigh 299 e^-50 = 6e-20 together)
    N = 300
    a = (50.0 / SCALE) ** 0.5
    a = float(torch.tensor(a).to(dtype))                                               # the bfloat16 a: the logit is a^2 scale >= 49.7
    eye = torch.eye(HD)
    q = a * eye[torch.arange(N) % HD].view(1, N, 1, HD).expand(2, N, heads, HD)
    k = torch.zeros(2, N, heads, HD)
    k[:, 37 * torch.arange(HD)] = a * eye.view(1, HD, 1, HD)
    v = torch.randn(2, N, heads, HD, generator=g)
    qkv = torch.stack([q, k, v], 2).reshape(2, N, 3 * heads * HD).to(dtype)
    assert a * a * SCALE >= 49.5
    out = _raw_fwd(qkv.to(DEV), heads, SCALE).double().cpu().view(2, N, heads, HD)
    want = qkv.double().view(2, N, 3, heads, HD)[:, 37 * (torch.arange(N) % HD), 2]
    ulp = 2.0 ** -23 if dtype == torch.float32 else 2.0 ** -8
    worst = ((out - want).abs() / want.abs().clamp_min(1e-30)).max().item()
    with capsys.disabled():
        print(f"mhsa_d8 {name} one-hot rows: max |out - v| / |v| {worst:.2e} (one step {ulp:.2e})")
    assert bool(((out - want).abs() <= ulp * want.abs()).all())

    # logits of +-60..90: finite, within 5 x the rule (section 12's bound for this case).  At |logit| 90 the float32 rounding of
    # the scaled logit alone is 90 x 2^-24 = 5e-6 relative in p, in the chain and in the kernel alike, so the case is measured
    # against the chain; the kernel's exponent additionally carries its statistic (|L2| up to 130 in the exp2 domain, rounded once).
    B, N = 2, 300
    g = torch.Generator().manual_seed(5)
    u = torch.randn(B, N, heads, HD, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    s = torch.sign(torch.randn(B, N, heads, 1, generator=g))
    a = (75.0 / SCALE) ** 0.5
    q = a * u + 0.05 * torch.randn(B, N, heads, HD, generator=g)
    k = a * s * u[:, torch.randperm(N, generator=g)] + 0.05 * torch.randn(B, N, heads, HD, generator=g)
    v = torch.randn(B, N, heads, HD, generator=g)
    qkv = torch.stack([q, k, v], 2).reshape(B, N, 3 * heads * HD).to(dtype)
    dout = torch.randn(B, N, heads * HD, generator=g).to(dtype)
    t = qkv.double().view(B, N, 3, heads, HD)
    lg = torch.einsum("bnhd,bmhd->bhnm", t[:, :, 0], t[:, :, 1]) * SCALE
    assert 60.0 <= lg.max().item() <= 90.0 and 60.0 <= -lg.min().item() <= 90.0, (lg.min().item(), lg.max().item())
    ek, ec, bound = _measure(qkv, dout, heads, SCALE, dtype)
    with capsys.disabled():
        print(f"mhsa_d8 {name} logits +-60..90: out dq dk dv kernel {_fmt(ek)} | chain {_fmt(ec)} | bound 5 x {_fmt(bound)}")
    for nm, e, b in zip(NAMES, ek, bound):
        assert e <= 5.0 * b, (nm, e, b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,N,heads", [(2, 784, 3), (1, 1025, 5)])
def test_bitwise_reproducible_and_autograd_is_the_raw_call(dtype, B, N, heads):
    from ppnet_amd import vit
    g = torch.Generator().manual_seed(77 + N)
    qkv = torch.randn(B, N, 3 * heads * HD, generator=g).to(dtype).to(DEV)
    dout = torch.randn(B, N, heads * HD, generator=g).to(dtype).to(DEV)
    out = _raw_fwd(qkv, heads, SCALE)
    assert torch.equal(out, _raw_fwd(qkv, heads, SCALE))
    a = _raw_bwd(qkv, out, dout, heads, SCALE)
    b = _raw_bwd(qkv, out, dout, heads, SCALE)
    # unrelated work in between: other kernels, another shape of this one, fresh allocations
    x = torch.randn(1024, 1024, device=DEV)
    y = (x @ x).relu().sum()
    q2 = torch.randn(1, 333, 3 * HD, device=DEV).to(dtype)
    _raw_bwd(q2, _raw_fwd(q2, 1, SCALE), torch.randn(1, 333, HD, device=DEV).to(dtype), 1, SCALE)
    assert bool(torch.isfinite(y))
    c = _raw_bwd(qkv, out, dout, heads, SCALE)
    assert bool(torch.isfinite(a).all())
    assert torch.equal(a, b) and torch.equal(a, c)                                     # three calls, NaN workspaces
    calls = dict(vit.CALLS)
    ko, kg = _kernel(qkv, dout, heads, SCALE)
    assert vit.CALLS["kernel"] == calls["kernel"] + 1 and vit.CALLS["bwd_kernel"] == calls["bwd_kernel"] + 1
    assert torch.equal(ko, out) and torch.equal(kg, a)
    zero = _raw_bwd(qkv, out, torch.zeros_like(dout), heads, SCALE, dqkv=torch.full_like(qkv, 7.0))
    assert bool((zero == 0).all())                                                     # dout = 0 -> dqkv = 0 exactly, all of it written


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernels_read_and_write_only_their_rows(dtype):
    """Large finite garbage in the rows just past row N of qkv, out and dout must reach nothing; out, dqkv and the workspace sit
    inside canary-filled buffers whose canaries survive; the workspace holds NaN before the call; the results equal the plain
    calls' bit for bit."""
    from ppnet_amd import _lib as L
    B, N, heads = 1, 333, 3
    C = heads * HD
    g = torch.Generator().manual_seed(13)
    qkv = torch.randn(B, N, 3 * C, generator=g).to(dtype).to(DEV)
    dout = torch.randn(B, N, C, generator=g).to(dtype).to(DEV)
    out = _raw_fwd(qkv, heads, SCALE)
    plain = _raw_bwd(qkv, out, dout, heads, SCALE)

    def padded(t):
        buf = torch.full((N + 300, t.shape[-1]), 3.0e4, dtype=dtype, device=DEV)       # rows N .. N + 299: exp(huge) if read
        buf[:N] = t[0]
        return buf
    qp, op, dp = padded(qkv), padded(out), padded(dout)
    pad = 4096                                                                         # elements: a multiple of 16 bytes
    obuf = torch.full((pad + B * N * C + pad,), 777.0, dtype=dtype, device=DEV)
    got_out = _raw_fwd(qp, heads, SCALE, out=obuf[pad:pad + B * N * C], B=B, N=N)
    assert bool((obuf[:pad] == 777.0).all()) and bool((obuf[pad + B * N * C:] == 777.0).all())
    assert torch.equal(got_out.view(B, N, C), out)
    n = B * N * 3 * C
    dbuf = torch.full((pad + n + pad,), 12345.0, dtype=dtype, device=DEV)
    need = L.lib.ppn_mhsa_bwd_workspace(B, N, heads)
    wbuf = torch.full((pad + need + pad,), 54321.0, dtype=torch.float32, device=DEV)
    wbuf[pad:pad + need] = float("nan")
    got = _raw_bwd(qp, op, dp, heads, SCALE, dqkv=dbuf[pad:pad + n], ws=wbuf[pad:pad + need], B=B, N=N)
    assert bool((dbuf[:pad] == 12345.0).all()) and bool((dbuf[pad + n:] == 12345.0).all())
    assert bool((wbuf[:pad] == 54321.0).all()) and bool((wbuf[pad + need:] == 54321.0).all())
    assert bool(torch.isfinite(wbuf[pad:pad + 2 * B * heads * N]).all())               # the statistics of every query were written
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got.view(B, N, 3 * C), plain)
    for buf in (qp, op, dp):
        assert bool((buf[N:] == 3.0e4).all())


def test_kernel_rejects_bad_arguments_on_gpu_buffers():
    from ppnet_amd import _lib as L
    q = torch.zeros(1, 8, 3 * HD, device=DEV)
    o = torch.zeros(1, 8, HD, device=DEV)
    d = torch.ones(1, 8, 3 * HD, device=DEV)
    w = torch.zeros(64, device=DEV)
    f = L.lib.ppn_mhsa_bwd
    assert L.lib.ppn_mhsa_bwd_workspace(1, 8, 1) == 16
    assert f(_P(q), _P(o), _P(o), _P(d), _P(w), 16, 1, 8, 1, 16, SCALE, 0, _stream()) == -3
    assert f(_P(q), _P(o), _P(o), _P(d), _P(w), 15, 1, 8, 1, HD, SCALE, 0, _stream()) == -1
    assert f(_P(q), _P(o), _P(o), ctypes.c_void_p(d.data_ptr() + 4), _P(w), 16, 1, 8, 1, HD, SCALE, 0, _stream()) == -1
    assert L.lib.ppn_mhsa_fwd(_P(q), ctypes.c_void_p(o.data_ptr() + 8), 1, 8, 1, HD, SCALE, 0, _stream()) == -1
    torch.cuda.synchronize()
    assert bool((d == 1).all())
    assert f(_P(q), _P(o), _P(o), _P(d), _P(w), 16, 1, 8, 1, HD, SCALE, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert bool((d == 0).all())
    from ppnet_amd import vit
    with pytest.raises(NotImplementedError):
        vit.mhsa_autograd(torch.zeros(1, 8, 3 * 32, device=DEV, requires_grad=True), 2, 0.25)       # head dim 16


# ------------------------------------------------------------------------------------------------ the module and the model
def _golden_model(golden_dir, R):
    from ppnet_amd.gennet import AEViT
    g = np.load(os.path.join(golden_dir, "g13_aevit.npz"))
    m = AEViT(1, 1, R, 24).eval()
    m.load_state_dict({k[len(f"R{R}/w/"):]: torch.tensor(g[k]) for k in g.files if k.startswith(f"R{R}/w/")}, strict=True)
    return m, torch.tensor(g[f"R{R}/x"]).float(), g[f"R{R}/y"]


@pytest.mark.parametrize("R", [64, 224])
def test_aevit_reference_numbers_through_the_kernel_path(golden_dir, R, capsys):
    """The reference module's own output (tests/golden/g13_aevit.npz) with grad enabled: the three ViT blocks run ppn_mhsa_fwd at
    head dim 8 (1024 tokens at R 64, 784 at R 224) and the output stays within the existing GPU golden test's bound."""
    from ppnet_amd import vit
    m, x, y = _golden_model(golden_dir, R)
    m = m.to(DEV)
    calls = dict(vit.CALLS)
    got = m(x.to(DEV))                                                                 # eval mode, autograd recording
    assert got.requires_grad
    assert vit.CALLS["kernel"] == calls["kernel"] + 3 and vit.CALLS["bwd_kernel"] == calls["bwd_kernel"]
    got = got.detach().float().cpu().numpy()
    err = np.abs(got - y).max()
    with capsys.disabled():
        print(f"\nAEViT R {R} float32 through ppn_mhsa_fwd: max|y - reference| {err:.2e} (max|y| {np.abs(y).max():.2e})")
    assert err < 1e-3 * max(1.0, np.abs(y).max())
    with torch.no_grad():                                                              # inference keeps the library's attention
        m(x.to(DEV))
    assert vit.CALLS["kernel"] == calls["kernel"] + 3


def _aevit_grads(m, x0, w):
    x = x0.clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    (m(x) * w).sum().backward()
    return {"input": x.grad.detach().double().cpu(), **{n: p.grad.detach().double().cpu() for n, p in m.named_parameters()}}


def test_aevit_parameter_gradients_through_the_kernel(monkeypatch, capsys):
    """AEViT(1, 1, 64, 24) in train mode without drop path, float32: the gradient of every parameter (and of the input) through the
    kernel path and through the library's attention (PPNET_LIBRARY_ATTENTION=1: same weights, same GPU), each against the float64
    CPU model: the rule above with the library path as the chain, relative to each gradient's max."""
    from ppnet_amd import vit
    from ppnet_amd.gennet import AEViT
    torch.manual_seed(4)
    m = AEViT(1, 1, 64, 24).train()
    for blk in m.vit_blocks:
        blk.drop_path_rate = 0.0
    with torch.no_grad():                                                              # biases and norms off their neutral values
        for n, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    g = torch.Generator().manual_seed(8)
    x0 = (torch.rand(4, 1, 64, 64, generator=g) > 0.5).float()
    w = torch.randn(4, 1, 64, 64, generator=g)
    ref = _aevit_grads(copy.deepcopy(m).double(), x0.double(), w.double())              # CPU, float64
    mg = copy.deepcopy(m).to(DEV)
    sd = {k: v.clone() for k, v in mg.state_dict().items()}
    vit.CALLS.update(kernel=0, bwd_kernel=0)
    got = _aevit_grads(mg, x0.to(DEV), w.to(DEV))
    torch.cuda.synchronize()
    assert vit.CALLS == {"kernel": 3, "bwd_kernel": 3}
    mg.load_state_dict(sd)                                                             # BatchNorm's running statistics
    monkeypatch.setenv("PPNET_LIBRARY_ATTENTION", "1")
    lib = _aevit_grads(mg, x0.to(DEV), w.to(DEV))
    monkeypatch.delenv("PPNET_LIBRARY_ATTENTION")
    assert vit.CALLS == {"kernel": 3, "bwd_kernel": 3}                                  # the knob is read at call time
    assert set(got) == set(ref) == set(lib) and len(got) == 1 + len(list(m.parameters()))
    # A convolution bias ahead of a train-mode BatchNorm has a gradient of exactly 0 in exact arithmetic; float64 leaves rounding
    # there (sums of 16384 terms that cancel: about 1e-16 x the terms).  A reference below 1e-12 x the model's largest gradient is
    # such a zero: a ratio to it would compare noise with noise, so the kernel path's value is bounded in absolute terms instead,
    # by the float32 floor of the rule against that largest gradient.
    gmax = max(ref[n].abs().max().item() for n in ref)
    zero = sorted(n for n in ref if ref[n].abs().max().item() < 1e-12 * gmax)
    worst, worst_zero = (0.0, 0.0, None), (0.0, 0.0, None)
    for n in ref:
        r = ref[n].abs().max().item()
        if n in zero:
            ak, al = got[n].abs().max().item() / gmax, lib[n].abs().max().item() / gmax
            if ak >= worst_zero[0]:
                worst_zero = (ak, al, n)
            assert ak <= FLOOR[torch.float32], (n, ak, al)
            continue
        ek, el = (got[n] - ref[n]).abs().max().item() / r, (lib[n] - ref[n]).abs().max().item() / r
        if ek > worst[0]:
            worst = (ek, el, n)
        assert ek <= max(2.0 * el, FLOOR[torch.float32]), (n, ek, el)
    assert len(zero) < len(ref) // 4 and all(n.endswith(".0.bias") for n in zero), zero        # only biases ahead of a BatchNorm
    with capsys.disabled():
        print(f"\nAEViT R 64 float32: worst kernel-path gradient error {worst[0]:.2e} x max (library path {worst[1]:.2e}) at {worst[2]}; "
              f"{len(zero)} gradients that are 0 in exact arithmetic: at most {worst_zero[0]:.2e} x the largest gradient "
              f"(library path {worst_zero[1]:.2e}) at {worst_zero[2]}")


def test_attention_saves_nothing_of_size_n_squared(capsys):
    """One gennet attention at B 8, N 1024, 3 heads, float32: forward + backward raise the peak of allocated memory by less than a
    quarter of ONE [B, heads, N, N] float32 tensor (100.7 MB); the path's own tensors (qkv, out, dout, dqkv, the workspace) come
    to under 8 MB."""
    from ppnet_amd import _lib as L
    from ppnet_amd import gennet, vit
    B, N, heads = 8, 1024, 3
    C = heads * HD
    torch.manual_seed(0)
    m = gennet._Attention(C, heads).to(DEV).train()

    def peak():
        x = torch.randn(B, N, C, device=DEV, requires_grad=True)
        dy = torch.randn(B, N, C, device=DEV)
        m.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        held = torch.cuda.memory_allocated()
        m(x).backward(dy)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - held
    peak()                                                                             # library workspaces allocated once
    vit.CALLS.update(kernel=0, bwd_kernel=0)
    rise = peak()
    assert vit.CALLS == {"kernel": 1, "bwd_kernel": 1}
    one_p = B * heads * N * N * 4
    own = 4 * (2 * B * N * 3 * C + 2 * B * N * C + L.lib.ppn_mhsa_bwd_workspace(B, N, heads))
    with capsys.disabled():
        print(f"\ngennet attention B {B} N {N} heads {heads} float32: peak rise {rise / 1e6:.1f} MB on the kernel path; the path's own "
              f"tensors {own / 1e6:.1f} MB; one probabilities tensor {one_p / 1e6:.1f} MB")
    assert own < 8e6
    assert rise < one_p / 4, (rise, one_p)


@pytest.mark.parametrize("amp", [None, torch.bfloat16])
def test_gennet_training_steps_use_the_head_dim_8_kernels(amp):
    """12 gennet_train_steps at R 64, batch 8, on (mask_space, mask_path) pairs from the generator: each step launches the forward
    and the backward kernel once per ViT block, every parameter gets a finite gradient, the loss falls."""
    from ppnet_amd import edage, train, vit
    from ppnet_amd.gennet import AEViT
    dev = torch.device("cuda:0")
    pb = edage.generate_paths(2, 64, 50, 3, seed=2, device=dev)
    mb = edage.generate_maps(pb, 4, 5, 20, seed=2)
    grid, space, path = train.generator_pairs(pb, mb, 4)
    assert space.shape[0] == 8
    torch.manual_seed(0)
    net = AEViT(1, 1, img_resolution=64, dim=24).cuda()
    opt = train.gennet_optimizer(net)
    vit.CALLS.update(kernel=0, bwd_kernel=0)
    losses = []
    for it in range(12):
        losses.append(float(train.gennet_train_step(net, opt, None, space, path, amp_dtype=amp)))
        assert vit.CALLS == {"kernel": 3 * (it + 1), "bwd_kernel": 3 * (it + 1)}
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    assert all(float(p.grad.abs().sum()) > 0 for n, p in net.named_parameters() if "attn.qkv.weight" in n)
    assert all(l == l for l in losses) and losses[-1] < losses[0], losses


def test_float16_autocast_keeps_the_library_attention():
    """Under float16 autocast the projection's output is float16, which the kernels do not take: the SDPA line runs, as before."""
    from ppnet_amd import gennet, vit
    torch.manual_seed(0)
    m = gennet._Attention(3 * HD, 3).to(DEV).train()
    x = torch.randn(2, 50, 3 * HD, device=DEV, requires_grad=True)
    calls = dict(vit.CALLS)
    with torch.autocast("cuda", dtype=torch.float16):
        y = m(x)
    y.float().sum().backward()
    assert y.dtype == torch.float16 and bool(torch.isfinite(x.grad).all()) and vit.CALLS == calls
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = m(x)
    y.float().sum().backward()
    assert y.dtype == torch.bfloat16 and vit.CALLS == {"kernel": calls["kernel"] + 1, "bwd_kernel": calls["bwd_kernel"] + 1}
