"""ppn_gennet_tail_train_fwd / ppn_gennet_tail_train_bwd (csrc/gennet_tail_train.hip) on the GPU: the kernels against float64 autograd of
BatchNorm(train) -> LeakyReLU -> Conv2d(C, 1, 3, 1, 1), known answers, bitwise reproducibility, the memory they may touch, GenNet's AE-ViT
through the kernel path (parameter gradients, running statistics, training steps) and the bytes the tail keeps alive.

The precision rule (tests/test_gpu_stem_train.py's): err = max|got - ref| / max|ref| over EVERY element, for out, mean, var, dy, dgamma,
dbeta, dW_f and db_f apart; ref = float64 autograd on the CPU of the same y, parameters and upstream gradient; err <= max(2 x the error of
the library composition F.batch_norm(training) -> F.leaky_relu -> F.conv2d and autograd in the same data type (bfloat16: bfloat16 y under
bfloat16 autocast) on the same inputs in the same run; FLOOR), FLOOR 2e-6 float32, 1e-2 bfloat16.  The bfloat16 floor applies to out and
dy only: mean, var and the parameter gradients are float32 in both data types and use the float32 floor.

The mask condition: a pre-activation within rounding of 0 flips the LeakyReLU mask against float64, which is no error of the kernel, so
every case asserts min|u| >= 1e-4 on its float64 reference.  y = clamp(round(4 (0.5 + 1.5 randn)) / 4, -8, 8): quarter steps, exact in
bfloat16 too, so both data types read the same values; parameters default-initialised under torch.manual_seed(seed) plus 0.1 randn on
gamma, beta and b_f; y, then d (randn rounded to bfloat16) from Generator(seed + 100).  Seed 0 meets the condition on every shape.

The kernels' own sizes: a work-item owns 4 consecutive pixels of the batch-wide pixel index (one vector of y and dy when H W is a
multiple of 4; a 3 x 6 window when the four lie in one row), a workgroup 1024, one-dimensional; the summing kernels launch at most 512
workgroups.  The shapes sit one below, at and one above 1024 pixels with rows of 3, 4 and 5, put image seams and row ends inside a
work-item's four pixels and inside a tile, put the whole halo row / column outside the image, and 725 x 725 has 514 tiles.

Each test prints what it measured (run with -s); the figures are in profiles/gennet_tail_precision.txt."""
import copy
import ctypes
import functools

import pytest

torch = pytest.importorskip("torch")
import torch.nn as nn                                                          # noqa: E402
import torch.nn.functional as F                                               # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-5
F32, BF16 = torch.float32, torch.bfloat16
FLOOR = {F32: 2e-6, BF16: 1e-2}
DTYPES = [F32, BF16]
SLOPES = [0.01, 0.0, 1.0]
LINE, TILE, MAX_BLOCKS = 4, 1024, 512                              # gennet_tail_train.hip: TL_PPT, TL_TILE, TL_MAX_BLOCKS
NAMES = ("out", "mean", "var", "dy", "dgamma", "dbeta", "dWf", "dbf")
WIDE = (0, 3)                                                      # out and dy have the data type; the others are float32
MIN_U = 1e-4
SEED = 0
# (B, H, W, C)
CASES = [(1, 1, 2, 8), (2, 1, 1, 24), (1, 3, 5, 16), (2, 9, 7, 24), (3, 1, 300, 32), (1, 300, 1, 8), (1, 341, LINE - 1, 8), (1, 256, LINE, 16),
         (1, 205, LINE + 1, 8), (2, 17, 31, 24), (1, 32, 32, 24), (4, 64, 64, 24), (2, 224, 224, 24), (1, 725, 725, 8)]


def build_case(shape, seed, kind="steps"):
    """Float32 CPU tensors of one case: (y, d, [gamma, beta, wf, bf])."""
    B, H, W, C = shape
    torch.manual_seed(seed)
    bn, conv = nn.BatchNorm2d(C), nn.Conv2d(C, 1, 3, 1, 1)
    with torch.no_grad():
        for p in (bn.weight, bn.bias, conv.bias):
            p.add_(0.1 * torch.randn_like(p))
    g = torch.Generator().manual_seed(seed + 100)
    if kind == "constant":
        y = (torch.arange(C, dtype=F32) / 4).view(1, C, 1, 1).expand(B, C, H, W).contiguous()
    else:
        y = (torch.round(4 * (0.5 + 1.5 * torch.randn(B, C, H, W, generator=g))) / 4).clamp(-8, 8)
    d = torch.randn(B, 1, H, W, generator=g).to(BF16).float()
    return y, d, [p.detach().clone() for p in (bn.weight, bn.bias, conv.weight, conv.bias)]


def composition(y, d, params, slope, autocast=False):
    """(out, mean, var, dy, dgamma, dbeta, dWf, dbf, min|u|, u) of the library composition under autograd, in y's dtype on y's device."""
    y = y.detach().clone().requires_grad_(True)
    ps = [p.detach().clone().requires_grad_(True) for p in params]
    C, n = y.shape[1], y.numel() // y.shape[1]
    rm, rv = torch.zeros(C, dtype=ps[0].dtype, device=y.device), torch.zeros(C, dtype=ps[0].dtype, device=y.device)
    with torch.autocast("cuda", dtype=BF16, enabled=autocast):
        u = F.batch_norm(y, rm, rv, ps[0], ps[1], training=True, momentum=1.0, eps=EPS)     # momentum 1: the running buffers ARE the batch's
        out = F.conv2d(F.leaky_relu(u, slope), ps[2], ps[3], padding=1)
    grads = torch.autograd.grad(out, [y] + ps, d.to(out.dtype))
    return (out.detach(), rm, rv * ((n - 1) / n), grads[0], grads[1], grads[2], grads[3], grads[4], u.detach().abs().min().item(), u.detach())


@functools.lru_cache(maxsize=None)
def reference(shape, seed, slope, kind="steps"):
    """The case and its float64 CPU reference, computed once and shared by the tests that need it (never modified)."""
    y, d, params = build_case(shape, seed, kind)
    ref = composition(y.double(), d.double(), [p.double() for p in params], slope)
    return y, d, params, ref[:8], ref[8], (ref[9] > 0).sum((0, 2, 3))


def kernel(y, d, params, slope, dtype, need_dy=True):
    """The eight outputs through the raw launches (fused._tail_fwd / fused._tail_bwd) on DEV."""
    from ppnet_amd import fused
    yg, ps = y.to(DEV).to(dtype), [p.to(DEV) for p in params]
    out, stats = fused._tail_fwd(yg, *ps, EPS, slope)
    dy, dgamma, dbeta, dwf, dbf = fused._tail_bwd(d.to(DEV).to(dtype), yg, ps[0], ps[1], ps[2], stats, slope, need_dy)
    torch.cuda.synchronize()
    assert out.dtype == dtype and out.shape == d.shape and dwf.shape == params[2].shape and dbf.shape == (1,)
    assert stats.dtype == dgamma.dtype == dbeta.dtype == dwf.dtype == dbf.dtype == F32
    assert (dy is None) == (not need_dy) and (dy is None or (dy.dtype == dtype and dy.shape == y.shape))
    return out, stats[0], stats[1], dy, dgamma, dbeta, dwf, dbf


def _rel(got, ref):
    d, r = (got.double().cpu() - ref).abs().max().item(), ref.abs().max().item()
    return d / r if r > 0 else (0.0 if d == 0 else float("inf"))


def _fmt(v):
    return " ".join(f"{x:.2e}" for x in v)


def _bounds(lib_err, dtype):
    return [max(2.0 * e, FLOOR[dtype if i in WIDE else F32]) for i, e in enumerate(lib_err)]


def measure(shape, seed, slope, dtype, tag, capsys, kind="steps"):
    y, d, params, ref, min_u, _ = reference(shape, seed, slope, kind)
    got = kernel(y, d, params, slope, dtype)
    lib = composition(y.to(DEV).to(dtype), d.to(DEV), [p.to(DEV) for p in params], slope, autocast=dtype == BF16)[:8]
    assert all(bool(torch.isfinite(t).all()) for t in got)
    ek, el = [_rel(a, r) for a, r in zip(got, ref)], [_rel(a, r) for a, r in zip(lib, ref)]
    bound = _bounds(el, dtype)
    with capsys.disabled():
        print(f"\ntail {tag} {str(dtype)[6:]} B H W C {shape} slope {slope} seed {seed} min|u| {min_u:.1e}: {' '.join(NAMES)} "
              f"kernel {_fmt(ek)} | library {_fmt(el)} | bound {_fmt(bound)}")
    return ek, bound, min_u


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("shape", CASES)
def test_kernel_vs_float64(shape, slope, dtype, capsys):
    ek, bound, min_u = measure(shape, SEED, slope, dtype, "steps", capsys)
    assert min_u >= MIN_U, (shape, SEED, min_u)                               # the mask condition: the case must meet it, it does not skip
    for name, e, b in zip(NAMES, ek, bound):
        assert e <= b, (name, shape, slope, e, b)


# ------------------------------------------------------------------------------------------------------------------------ known answers
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 9, 7, 24), (1, 32, 32, 8), (2, 1, 5, 16)])
def test_constant_planes_and_the_zero_padding_of_z(shape, dtype):
    """y = c / 4 in channel c: mean is it and var is 0, exactly; xhat = 0, so z = leaky(beta_c) inside the image and 0 in the halo:
    out(p) = b_f + sum_c leaky(beta_c) (the sum of w_f[c]'s taps that fall inside the image at p), within the floor at every pixel —
    corners, edges, interior, both images of the batch."""
    B, H, W, C = shape
    y, d, params = build_case(shape, 1, "constant")
    gamma, beta, wf, bf = [p.double() for p in params]
    slope = 0.01
    out, mean, var = kernel(y, d, params, slope, dtype)[:3]
    assert torch.equal(mean.cpu(), torch.arange(C, dtype=F32) / 4) and bool((var == 0).all())
    s = float(torch.tensor(slope, dtype=F32))
    lb = torch.where(beta > 0, beta, beta * s)
    want = torch.empty(H, W, dtype=torch.float64)
    for h in range(H):
        for w in range(W):
            m = torch.tensor([[0 <= h + r - 1 < H and 0 <= w + j - 1 < W for j in range(3)] for r in range(3)], dtype=torch.float64)
            want[h, w] = bf[0] + (lb * (wf[0] * m).sum((1, 2))).sum()
    assert out.shape == (B, 1, H, W)
    for b in range(B):
        err = (out[b, 0].double().cpu() - want).abs().max().item() / want.abs().max().item()
        assert err <= FLOOR[dtype], (shape, b, err)
    if H > 2 and W > 2:                                                        # the seam shows: a corner differs from the interior
        assert abs(want[0, 0].item() - want[1, 1].item()) > 1e-3 * want.abs().max().item()


@pytest.mark.parametrize("shape", [(2, 9, 7, 24), (1, 205, 5, 8), (4, 64, 64, 24), (2, 224, 224, 24)])
def test_slope_zero_counts_the_forward_mask_exactly(shape):
    """slope 0, d = 1 and a centre-tap-only w_f = 1, so dz = 1 at every pixel, float32: dbeta_c = the number of positive pre-activations
    in channel c of the float64 reference, exactly (min|u| >= 1e-4 keeps the float32 mask the float64 one).  At most 2^24 pixels, so
    every count is a float32 integer.  dgamma_c is then the sum of xhat over those pixels."""
    assert shape[0] * shape[1] * shape[2] <= 2 ** 24
    y, _, params, _, min_u, count = reference(shape, SEED, 0.0)
    assert min_u >= MIN_U
    wf = torch.zeros_like(params[2])
    wf[0, :, 1, 1] = 1.0
    d = torch.ones(shape[0], 1, shape[1], shape[2])
    _, _, _, dy, _, dbeta, _, dbf = kernel(y, d, [params[0], params[1], wf, params[3]], 0.0, F32)
    n = shape[0] * shape[1] * shape[2]
    assert bool((count > 0).any()) and bool((count < n).any())
    assert torch.equal(dbeta.cpu(), count.float())
    assert float(dbf) == float(n)


@pytest.mark.parametrize("dtype", DTYPES)
def test_slope_one_has_no_mask(dtype, capsys):
    """slope 1: z is the BatchNorm output, whatever the sign — the rule holds with no mask condition (seed 1 is not picked for it)."""
    ek, bound, _ = measure((2, 9, 7, 24), 1, 1.0, dtype, "slope-1", capsys)
    for name, e, b in zip(NAMES, ek, bound):
        assert e <= b, (name, e, b)


# ------------------------------------------------------------------------------------------------------------------------------ hygiene
def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


GUARD = 64                                                                     # elements on each side of every output


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _raw_pair(y, d, params, slope, dtype, fill, want_dy=True):
    """Both raw entry points on outputs and a workspace filled with `fill` and surrounded by it: (outputs, their buffers)."""
    from ppnet_amd import _lib as L
    B, C, H, W = y.shape
    need = L.lib.ppn_gennet_tail_train_workspace(B, H, W, C)
    assert need > 0 and need % 4 == 0
    bufs = {"out": _guarded(B * H * W, dtype, fill), "stats": _guarded(3 * C, F32, fill), "ws": _guarded(need // 4, F32, fill),
            "dy": _guarded(B * C * H * W, dtype, fill), "dgamma": _guarded(C, F32, fill), "dbeta": _guarded(C, F32, fill),
            "dwf": _guarded(C * 9, F32, fill), "dbf": _guarded(4, F32, fill)}
    v = {k: b[1] for k, b in bufs.items()}
    yg, dg, ps = y.to(DEV).to(dtype), d.to(DEV).to(dtype), [p.to(DEV) for p in params]
    dt = 0 if dtype == F32 else 1
    rc = L.lib.ppn_gennet_tail_train_fwd(_P(yg), *[_P(p) for p in ps], _P(v["out"]), _P(v["stats"]), _P(v["ws"]), B, H, W, C, EPS, slope, dt, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    v["ws"].fill_(fill)
    rc = L.lib.ppn_gennet_tail_train_bwd(_P(dg), _P(yg), _P(ps[0]), _P(ps[1]), _P(ps[2]), _P(v["stats"]), _P(v["ws"]), _P(v["dy"]) if want_dy else None,
                                         _P(v["dgamma"]), _P(v["dbeta"]), _P(v["dwf"]), _P(v["dbf"]), B, H, W, C, slope, dt, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return v, bufs


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 9, 7, 24), (1, 205, 5, 8), (2, 17, 31, 24), (1, 1100, 1024, 8)])
def test_three_calls_agree_bitwise_and_stay_inside_their_buffers(shape, dtype):
    """Three calls on NaN-filled outputs and workspaces give the same bits (one writer per element, fixed-order sums: 1100 x 1024 has
    more tiles than workgroups), every output element is written (db_f: its one), and the 64 elements on either side of out, stats, the
    workspace, dy and the gradients keep their fill.  dy = NULL: the same parameter gradients bit for bit, and dy's buffer untouched."""
    y, d, params = build_case(shape, 5)
    nan = float("nan")
    first = None
    for _ in range(3):
        v, bufs = _raw_pair(y, d, params, 0.01, dtype, nan)
        for k, (buf, view) in bufs.items():
            assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + view.numel():]).all()), k
            if k == "dbf":
                assert bool(torch.isfinite(view[0])) and bool(torch.isnan(view[1:]).all())
            elif k != "ws":
                assert bool(torch.isfinite(view).all()), k
        out = {k: t.clone() for k, t in v.items() if k != "ws"}
        out["dbf"] = out["dbf"][:1]
        if first is None:
            first = out
        assert all(torch.equal(out[k], first[k]) for k in first)
    v7, bufs7 = _raw_pair(y, d, params, 0.01, dtype, 7.0)                      # another fill: nothing read before it was written
    assert all(torch.equal(v7[k][:first[k].numel()], first[k]) for k in first)
    assert all(bool((b[:GUARD] == 7).all()) and bool((b[GUARD + view.numel():] == 7).all()) for b, view in bufs7.values())
    vn, bufsn = _raw_pair(y, d, params, 0.01, dtype, 7.0, want_dy=False)
    assert bool((bufsn["dy"][0] == 7).all())
    assert all(torch.equal(vn[k][:first[k].numel()], first[k]) for k in first if k != "dy")


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_upstream_gradient_and_the_autograd_function(dtype):
    """d = 0 gives every gradient exactly 0; the autograd function returns the raw calls' bits, and no dy (and no second pass's output)
    for a y that needs none; a convolution without bias gets no db_f."""
    from ppnet_amd import fused
    shape = (2, 9, 7, 24)
    y, d, params = build_case(shape, 2)
    zero = kernel(y, torch.zeros_like(d), params, 0.01, dtype)
    assert all(bool((t == 0).all()) for t in zero[3:])
    raw = kernel(y, d, params, 0.01, dtype)
    ps = [p.to(DEV).requires_grad_(True) for p in params]
    yg = y.to(DEV).to(dtype).requires_grad_(True)
    calls = dict(fused.TAIL_CALLS)
    out, stats = fused._TailTrainFunction.apply(yg, *ps, EPS, 0.01)
    assert not stats.requires_grad and out.requires_grad
    grads = torch.autograd.grad(out, [yg] + ps, d.to(DEV).to(dtype))
    assert fused.TAIL_CALLS == {"fwd": calls["fwd"] + 1, "bwd": calls["bwd"] + 1}
    assert torch.equal(out, raw[0]) and torch.equal(stats[0], raw[1]) and torch.equal(stats[1], raw[2])
    assert all(torch.equal(g, r) for g, r in zip(grads, raw[3:]))
    out2, _ = fused._TailTrainFunction.apply(yg.detach(), *ps, EPS, 0.01)      # y needs no gradient: dy is skipped
    grads2 = torch.autograd.grad(out2, ps, d.to(DEV).to(dtype))
    assert all(torch.equal(g, r) for g, r in zip(grads2, raw[4:]))
    out3, _ = fused._TailTrainFunction.apply(yg, ps[0], ps[1], ps[2], None, EPS, 0.01)
    want = kernel(y, d, [params[0], params[1], params[2], torch.zeros_like(params[3])], 0.01, dtype)
    assert torch.equal(out3, want[0])
    assert all(torch.equal(g, r) for g, r in zip(torch.autograd.grad(out3, [yg] + ps[:3], d.to(DEV).to(dtype)), want[3:7]))


# ---------------------------------------------------------------------------------------------------------------------- the module
def _model(seed):
    from ppnet_amd.gennet import AEViT
    torch.manual_seed(seed)
    m = AEViT(1, 1, 64, 24).train()
    for blk in m.vit_blocks:
        blk.drop_path_rate = 0.0
    with torch.no_grad():                                                      # biases and norms off their neutral values
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    return m


def _grads_and_stats(m, x, w):
    m.zero_grad(set_to_none=True)
    (m(x) * w).sum().backward()
    bn = m.dec_conv[-1][1]
    out = {n: (p.grad.detach().double().cpu() if p.grad is not None else None) for n, p in m.named_parameters()}
    return out, (bn.running_mean.detach().double().cpu(), bn.running_var.detach().double().cpu(), int(bn.num_batches_tracked))


def test_aevit_parameter_gradients_and_running_statistics(monkeypatch, capsys):
    """AEViT(1, 1, 64, 24) in train mode without drop path, float32, one forward + backward of (m(x) * w).sum(): one launch pair; every
    parameter gradient through the kernel tail and through the library tail (PPNET_LIBRARY_TAIL=1: same weights, same GPU) against the
    float64 CPU model by the rule; the last stage's running statistics are the float64 model's within the rule."""
    from ppnet_amd import fused
    monkeypatch.delenv("PPNET_LIBRARY_TAIL", raising=False)
    monkeypatch.setattr(fused, "TAIL_RECORD_MIN", 0)
    m = _model(4)
    g = torch.Generator().manual_seed(8)
    x0 = (torch.rand(4, 1, 64, 64, generator=g) > 0.5).float()
    w = torch.randn(4, 1, 64, 64, generator=g)
    ref, ref_stats = _grads_and_stats(copy.deepcopy(m).double(), x0.double(), w.double())
    mg = copy.deepcopy(m).to(DEV)
    sd = {k: v.clone() for k, v in mg.state_dict().items()}
    fused.TAIL_CALLS.update(fwd=0, bwd=0)
    got, got_stats = _grads_and_stats(mg, x0.to(DEV), w.to(DEV))
    torch.cuda.synchronize()
    assert fused.TAIL_CALLS == {"fwd": 1, "bwd": 1}
    mg.load_state_dict(sd)
    monkeypatch.setenv("PPNET_LIBRARY_TAIL", "1")
    lib, lib_stats = _grads_and_stats(mg, x0.to(DEV), w.to(DEV))
    monkeypatch.delenv("PPNET_LIBRARY_TAIL")
    assert fused.TAIL_CALLS == {"fwd": 1, "bwd": 1}                            # the knob is read at call time
    assert all(v is not None for v in got.values()) and set(got) == set(ref) == set(lib)
    # a convolution bias ahead of a train-mode BatchNorm has gradient 0 in exact arithmetic (float64 leaves rounding): bounded in
    # absolute terms by the float32 floor against the model's largest gradient, as tests/test_gpu_stem_train.py does
    gmax = max(r.abs().max().item() for r in ref.values())
    worst = (0.0, 0.0, None)
    for n, r in ref.items():
        top = r.abs().max().item()
        if top < 1e-12 * gmax:
            assert n.endswith(".0.bias") and got[n].abs().max().item() / gmax <= FLOOR[F32], n
            continue
        ek, el = (got[n] - r).abs().max().item() / top, (lib[n] - r).abs().max().item() / top
        worst = max(worst, (ek, el, n))
        assert ek <= max(2.0 * el, FLOOR[F32]), (n, ek, el)
    es = [_rel(a, r) for a, r in zip(got_stats[:2], ref_stats[:2])]
    ls = [_rel(a, r) for a, r in zip(lib_stats[:2], ref_stats[:2])]
    with capsys.disabled():
        print(f"\nAEViT R 64 float32 kernel tail: worst gradient error {worst[0]:.2e} x max (library tail {worst[1]:.2e}) at {worst[2]}; "
              f"running mean / var error {_fmt(es)} (library {_fmt(ls)})")
    assert got_stats[2] == lib_stats[2] == ref_stats[2] == 1
    for e, l in zip(es, ls):
        assert e <= max(2.0 * l, FLOOR[F32]), (es, ls)


def test_running_statistics_where_the_unbiased_factor_matters(monkeypatch):
    """B H W = 2: the running variance takes the batch's unbiased variance, twice the biased one."""
    from ppnet_amd import fused
    monkeypatch.setattr(fused, "TAIL_RECORD_MIN", 0)
    torch.manual_seed(1)
    bn, conv = nn.BatchNorm2d(24, momentum=0.3), nn.Conv2d(24, 1, 3, 1, 1)
    y = (torch.round(4 * torch.randn(1, 24, 1, 2)) / 4)
    b64, c64 = copy.deepcopy(bn).double(), copy.deepcopy(conv).double()
    o64 = c64(F.leaky_relu(b64(y.double()), 0.01))
    bn, conv = bn.to(DEV), conv.to(DEV)
    calls = dict(fused.TAIL_CALLS)
    yg = y.to(DEV).requires_grad_(True)
    assert fused.tail_train_ok(yg, bn, conv)
    o = fused.tail_bn_act_conv(yg, bn, 0.01, conv)
    assert fused.TAIL_CALLS["fwd"] == calls["fwd"] + 1
    assert int(bn.num_batches_tracked) == int(b64.num_batches_tracked) == 1
    assert _rel(bn.running_mean, b64.running_mean) <= FLOOR[F32] and _rel(bn.running_var, b64.running_var) <= FLOOR[F32]
    assert _rel(o.detach(), o64.detach()) <= 1e-4                               # two pixels: y - mean is half a float32 difference
    with pytest.raises(ValueError):                                            # one value per channel: torch's own error, from torch
        fused.tail_bn_act_conv(yg[..., :1], bn, 0.01, conv)


def test_everything_else_keeps_the_library_tail(monkeypatch):
    """Eval mode with grad, no_grad, SyncBatchNorm and float16 autocast leave TAIL_CALLS alone; bfloat16 autocast takes the kernels and
    gives a bfloat16 output, from a bfloat16 y (the model) and from a float32 y alike."""
    from ppnet_amd import fused
    monkeypatch.delenv("PPNET_LIBRARY_TAIL", raising=False)
    monkeypatch.setattr(fused, "TAIL_RECORD_MIN", 0)
    m = _model(2).to(DEV)
    x = (torch.rand(2, 1, 64, 64, device=DEV) > 0.5).float()
    last = m.dec_conv[-1]
    y = torch.randn(2, 24, 64, 64, device=DEV, requires_grad=True)
    calls = dict(fused.TAIL_CALLS)
    m.eval()
    m(x).sum().backward()
    m.train()
    with torch.no_grad():
        m(x)
    with torch.autocast("cuda", dtype=torch.float16):
        o = fused.tail_bn_act_conv(y, last[1], 0.01, m.conv_final)
    assert o.dtype == torch.float16 and fused.TAIL_CALLS == calls
    keep = last[1]
    last[1] = nn.SyncBatchNorm(24).to(DEV)
    assert not fused.tail_train_ok(y, last[1], m.conv_final)
    last[1] = keep
    assert fused.TAIL_CALLS == calls
    with torch.autocast("cuda", dtype=BF16):
        o = m(x)
    assert o.dtype == BF16
    o.float().sum().backward()
    assert fused.TAIL_CALLS == {"fwd": calls["fwd"] + 1, "bwd": calls["bwd"] + 1}
    with torch.autocast("cuda", dtype=BF16):
        o = fused.tail_bn_act_conv(y, last[1], 0.01, m.conv_final)
    assert o.dtype == BF16
    o.float().sum().backward()
    assert y.grad is not None and y.grad.dtype == F32 and fused.TAIL_CALLS == {"fwd": calls["fwd"] + 2, "bwd": calls["bwd"] + 2}


def _pairs(R, n_paths, placements, seed):
    from ppnet_amd import edage, train
    dev = torch.device("cuda:0")
    pb = edage.generate_paths(n_paths, R, 50, 3, seed=seed, device=dev)
    mb = edage.generate_maps(pb, placements, 5, 20, seed=seed)
    return train.generator_pairs(pb, mb, placements)


@pytest.mark.parametrize("amp", [None, BF16])
def test_gennet_training_steps_use_the_tail_kernels(amp, monkeypatch):
    """12 gennet_train_steps at R 64, batch 8, on (mask_space, mask_path) pairs from the generator: one launch pair per step, every
    parameter gets a finite gradient, the loss falls, and under autocast the tail reads a bfloat16 y."""
    from ppnet_amd import fused, train
    from ppnet_amd.gennet import AEViT
    monkeypatch.delenv("PPNET_LIBRARY_TAIL", raising=False)
    monkeypatch.setattr(fused, "TAIL_RECORD_MIN", 0)
    grid, space, path = _pairs(64, 2, 4, seed=2)
    assert space.shape[0] == 8
    torch.manual_seed(0)
    net = AEViT(1, 1, img_resolution=64, dim=24).cuda()
    opt = train.gennet_optimizer(net)
    seen = []
    hook = net.dec_conv[-1][0].register_forward_hook(lambda mod, args, out: seen.append(out.dtype))
    fused.TAIL_CALLS.update(fwd=0, bwd=0)
    losses = []
    for it in range(12):
        losses.append(float(train.gennet_train_step(net, opt, None, space, path, amp_dtype=amp)))
        assert fused.TAIL_CALLS == {"fwd": it + 1, "bwd": it + 1}
    hook.remove()
    assert seen == [amp or F32] * 12
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    assert float(net.conv_final.weight.grad.abs().sum()) > 0 and int(net.dec_conv[-1][1].num_batches_tracked) == 12
    assert all(l == l for l in losses) and losses[-1] < losses[0], losses


# --------------------------------------------------------------------------------------------------------------------------- memory
def test_the_tail_keeps_only_y_alive(monkeypatch, capsys):
    """(8, 224, 224, 24) float32, T = 38.5 MB, y created outside the measured region: the bytes still allocated after the tail's forward,
    above those before it.  The kernel path holds at most 0.25 T (out, the statistics); the library composition holds at least 1.5 T more
    (it keeps BN(y) and z for its backward: the expected gap is 2 T)."""
    from ppnet_amd import fused
    monkeypatch.delenv("PPNET_LIBRARY_TAIL", raising=False)
    monkeypatch.setattr(fused, "TAIL_RECORD_MIN", 0)
    B, H, W, C = 8, 224, 224, 24
    T = B * C * H * W * 4
    torch.manual_seed(0)
    bn, conv = nn.BatchNorm2d(C).to(DEV), nn.Conv2d(C, 1, 3, 1, 1).to(DEV)
    y = torch.randn(B, C, H, W, device=DEV, requires_grad=True)

    def held():
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        out = fused.tail_bn_act_conv(y, bn, 0.01, conv)
        torch.cuda.synchronize()
        after = torch.cuda.memory_allocated()
        out.sum().backward()                                                   # the graph is released with out
        del out
        y.grad = None
        return after - before
    held()
    calls = dict(fused.TAIL_CALLS)
    ours = held()
    assert fused.TAIL_CALLS == {"fwd": calls["fwd"] + 1, "bwd": calls["bwd"] + 1}
    monkeypatch.setenv("PPNET_LIBRARY_TAIL", "1")
    held()
    theirs = held()
    monkeypatch.delenv("PPNET_LIBRARY_TAIL")
    with capsys.disabled():
        print(f"\ntail (8, 224, 224, 24) float32, T = {T / 1e6:.1f} MB: held after the forward {ours / 1e6:.1f} MB = {ours / T:.2f} T on the kernel "
              f"path, {theirs / 1e6:.1f} MB = {theirs / T:.2f} T on the library composition")
    assert ours <= 0.25 * T, (ours, T)
    assert theirs - ours >= 1.5 * T, (theirs, ours, T)
