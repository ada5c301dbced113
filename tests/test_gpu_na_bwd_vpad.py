"""ppn_na2d_bwd_vpad (csrc/na2d_bwd.hip) on the GPU: the kernel against float64 autograd of the definition on the materialised grid,
the hazards of the virtual form (a padded query in a key's range, garbage in the workspace), bitwise reproducibility, the memory it
may touch, the NeighborhoodAttention2D training branch, its peak memory, and training steps of a reduced DiNAT-B + SETR-UP.

The definition: full = pad_kv.expand(B, H, W, 3C).clone(); full[:, :Hr, :Wr] = real; the neighbourhood attention over `full` as
the float64 gather of oracle/segnet_ref.py (tests/test_gpu_na.py::test_na2d_backward_vs_fp64_autograd), the output cropped to the
real tokens before backward; the gradient of pad_kv through expand().clone() is dpad_kv.  bfloat16: on the rounded inputs.

The precision rule: for each of dq, dk, dv, dpad_k, dpad_v and drpb, err = max|got - ref| / max|ref| over EVERY
element; err <= max(2 x the error of the materialised path, FLOOR) — the materialised path is na.na2d_autograd on `full` and a
crop, in the same dtype on the same inputs in the same run.  FLOOR is this op's own (tests/test_gpu_na.py:219-220, :242-243):
2e-4 in float32; in bfloat16 2e-2 for dq / dk / dv (and for dpad_k / dpad_v), 1e-3 for drpb.  A reference that is exactly 0 (the q
third of dpad_kv; all of it without padding) asks for exactly 0.

Each test prints what it measured (run with -s)."""
import copy
import ctypes

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda"
SCALE = 32 ** -0.5
NAMES = ("dq", "dk", "dv", "dpad_k", "dpad_v", "drpb")
FLOOR = {torch.float32: (2e-4,) * 6, torch.bfloat16: (2e-2, 2e-2, 2e-2, 2e-2, 2e-2, 1e-3)}
# B, H, W, Hr, Wr, heads, dilation: each the smallest that reaches one hazard
CASES = [(2, 14, 14, 9, 10, 2, 2),       # the module test's shape, two heads
         (1, 14, 14, 7, 7, 3, 2),        # level 3 at R = 224: groups of 4 and 3 real rows
         (1, 28, 28, 16, 16, 2, 4),
         (1, 21, 21, 16, 13, 2, 3),      # groups of unequal real extent on both axes
         (1, 40, 14, 40, 9, 1, 2),       # padded on one axis only; three regions along y, a query halo of 15
         (1, 21, 21, 2, 20, 1, 3),       # a dilation group with no real token
         (2, 112, 112, 56, 56, 1, 16),   # DiNAT-B level 0 at R = 224: 256 groups per image, dpad_kv over 9 408 positions per image
         (1, 16, 16, 16, 16, 2, 2)]      # no padding: dpad_kv exactly 0
HAZARD = CASES[1]


def _inputs(case, dtype, seed):
    """real [B,Hr,Wr,3C], pad [3C], dout [B,Hr,Wr,C] in dtype; rpb [heads,13,13] float32 (CPU)."""
    B, H, W, Hr, Wr, heads, d = case
    g = torch.Generator().manual_seed(seed)
    C = heads * 32
    real = torch.randn(B, Hr, Wr, 3 * C, generator=g).to(dtype)
    pad = (torch.randn(3 * C, generator=g) * 0.5).to(dtype)
    rpb = torch.randn(heads, 13, 13, generator=g) * 0.5
    dout = torch.randn(B, Hr, Wr, C, generator=g).to(dtype)
    return real, pad, rpb, dout


def _full(real, pad, H, W):
    B, Hr, Wr, C3 = real.shape
    full = pad.expand(B, H, W, C3).clone()
    full[:, :Hr, :Wr] = real
    return full


def _definition(real, pad, rpb, dout, case):
    """float64 autograd of the definition -> (out [B,Hr,Wr,C], dreal, dpad [3C], drpb), all float64."""
    from oracle import segnet_ref as SR
    B, H, W, Hr, Wr, heads, d = case
    C = heads * 32
    real, pad, rpb = (t.detach().to(DEV).double().requires_grad_(True) for t in (real, pad, rpb))
    full = _full(real, pad, H, W)
    ri, bi = SR._axis_tables(H, 7, d, full.device)
    cj, bj = SR._axis_tables(W, 7, d, full.device)
    bias = rpb[:, bi[:, None, :, None], bj[None, :, None, :]]
    outs = []
    for b in range(B):
        t = full[b].view(H, W, 3, heads, 32).permute(2, 3, 0, 1, 4)
        q, kk, v = t[0] * SCALE, t[1], t[2]
        kg, vg = kk[:, ri][:, :, :, cj], v[:, ri][:, :, :, cj]
        p = torch.softmax((torch.einsum("hijc,hiajbc->hijab", q, kg) + bias).reshape(heads, H, W, 49), dim=-1).view(heads, H, W, 7, 7)
        outs.append(torch.einsum("hijab,hiajbc->hijc", p, vg).permute(1, 2, 0, 3).reshape(H, W, C)[:Hr, :Wr])
    out = torch.stack(outs)
    g = torch.autograd.grad(out, (real, pad, rpb), dout.to(DEV).double())
    return (out.detach(),) + g


def _materialised(real, pad, rpb, dout, case):
    """The path the module trained through before: na2d_autograd on the materialised grid, crop; in real's dtype."""
    from ppnet_amd.na import na2d_autograd
    B, H, W, Hr, Wr, heads, d = case
    real, pad, rpb = (t.detach().to(DEV).requires_grad_(True) for t in (real, pad, rpb))
    out = na2d_autograd(_full(real, pad, H, W), rpb, heads, d, SCALE)[:, :Hr, :Wr]
    return torch.autograd.grad(out, (real, pad, rpb), dout.to(DEV))


def _raw(real, pad, rpb, dout, case, outs=None, ws_floats=None, want_rc=0):
    """ppn_na2d_bwd_vpad itself on device tensors -> (dqkv, dpad_kv [3C] float32, drpb [heads,13,13] float32); `outs` = (dqkv, dpad,
    drpb, ws) may be views into larger buffers."""
    from ppnet_amd import _lib as L
    B, H, W, Hr, Wr, heads, d = case
    C = heads * 32
    need = L.lib.ppn_na2d_bwd_vpad_workspace(B, H, W, Hr, Wr, heads, d)
    assert need > 0
    if outs is None:
        outs = (torch.empty(B, Hr, Wr, 3 * C, dtype=real.dtype, device=DEV), torch.empty(3 * C, dtype=torch.float32, device=DEV),
                torch.empty(heads, 13, 13, dtype=torch.float32, device=DEV), torch.empty(need, dtype=torch.float32, device=DEV))
    dqkv, dpad, drpb, ws = outs
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = L.lib.ppn_na2d_bwd_vpad(P(real), P(pad), P(rpb), P(dout), P(dqkv), P(dpad), P(drpb), P(ws), need if ws_floats is None else ws_floats,
                                 B, H, W, Hr, Wr, heads, d, float(SCALE), 0 if real.dtype == torch.float32 else 1,
                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == want_rc
    return dqkv, dpad, drpb


def _dev(*ts):
    return [t.to(DEV).contiguous() for t in ts]


def _parts(dqkv, dpad, drpb, heads):
    """The six gradients of the rule and the q third of dpad_kv, float64 on the CPU."""
    C = heads * 32
    q = dqkv.double().cpu().reshape(*dqkv.shape[:3], 3, C)
    p = dpad.double().cpu().reshape(3, C)
    return [q[..., 0, :], q[..., 1, :], q[..., 2, :], p[1], p[2], drpb.double().cpu()], p[0]


def _errors(got, ref, heads):
    """max|got - ref| / max|ref| per gradient; a reference that is exactly 0 asks for exactly 0."""
    (gs, gq0), (rs, rq0) = _parts(*got, heads), _parts(*ref, heads)
    assert float(rq0.abs().max()) == 0.0 and float(gq0.abs().max()) == 0.0              # the q third of dpad_kv
    errs = []
    for a, b in zip(gs, rs):
        d, r = (a - b).abs().max().item(), b.abs().max().item()
        errs.append(d / r if r > 0 else (0.0 if d == 0 else float("inf")))
    return errs


def _measure(real, pad, rpb, dout, case, dtype):
    """(kernel errors, materialised-path errors, bounds) for NAMES on inputs already rounded to dtype; the forward on the way."""
    from ppnet_amd import na
    heads = case[5]
    ref = _definition(real, pad, rpb, dout, case)
    out = na.na2d_forward(*_dev(real, rpb), heads, case[6], SCALE, pad_kv=pad.to(DEV), padded_hw=case[1:3])
    assert out.shape == ref[0].shape
    if dtype == torch.float32:
        assert (out.double() - ref[0]).abs().max().item() < 1e-4
    chain = _materialised(real, pad, rpb, dout, case)
    got = _raw(*_dev(real, pad, rpb, dout), case)
    assert got[0].dtype == dtype and got[0].shape == real.shape and all(bool(torch.isfinite(t).all()) for t in got)
    ek, ec = _errors(got, ref[1:], heads), _errors(chain, ref[1:], heads)
    return ek, ec, [max(2.0 * c, f) for c, f in zip(ec, FLOOR[dtype])]


def _report(capsys, what, ek, ec, bound, factor=1.0):
    with capsys.disabled():
        f = lambda v: " ".join(f"{x:.2e}" for x in v)
        print(f"\nna_bwd_vpad {what}: {' '.join(NAMES)} kernel {f(ek)} | materialised {f(ec)} | bound {factor:g} x {f(bound)}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_kernel_vs_float64(dtype, case, capsys):
    B, H, W, Hr, Wr, heads, d = case
    real, pad, rpb, dout = _inputs(case, dtype, 100 * H + 10 * Hr + Wr + d)
    ek, ec, bound = _measure(real, pad, rpb, dout, case, dtype)
    _report(capsys, f"{str(dtype)[6:]} {case}", ek, ec, bound)
    for name, e, b in zip(NAMES, ek, bound):
        assert e <= b, (name, case, e, b)
    if (Hr, Wr) == (H, W):                                                               # no padded position: exactly 0, all of it
        assert bool((_raw(*_dev(real, pad, rpb, dout), case)[1] == 0).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_large_logits_and_a_workspace_of_nan(dtype, capsys):
    """Logits of +-60..90 between real tokens and towards the padded keys (qkv and pad_kv scaled): a padded query that stayed in a
    key's range would meet statistics that were never written — exp(s - garbage) * 0.  Finite outputs, float32 within 5 x the
    rule; the same outputs bit for bit from a workspace that held NaN before the call."""
    from ppnet_amd import _lib as L
    case = HAZARD
    B, H, W, Hr, Wr, heads, d = case
    C = heads * 32
    g = torch.Generator().manual_seed(7)
    u = torch.randn(32, generator=g)
    u = u / u.norm()
    # inside a dilation group neighbours alternate in sign, so one window holds logits near +80 and near -80
    sgn = torch.tensor([[(-1.0) ** (i // d + j // d) for j in range(Wr)] for i in range(Hr)])
    a = (80.0 / SCALE) ** 0.5
    real = torch.randn(B, Hr, Wr, 3, heads, 32, generator=g) * 0.05
    real[..., 0, :, :] += a * sgn[None, :, :, None, None] * u
    real[..., 1, :, :] -= a * sgn[None, :, :, None, None] * u
    real[..., 2, :, :] = torch.randn(B, Hr, Wr, heads, 32, generator=g)
    real = real.reshape(B, Hr, Wr, 3 * C).to(dtype)
    pad = torch.randn(3, heads, 32, generator=g) * 0.05
    pad[1] -= a * u                                                                       # a padded key: logit -+80 with every query
    pad = pad.reshape(3 * C).to(dtype)
    rpb = torch.randn(heads, 13, 13, generator=g) * 0.5
    dout = torch.randn(B, Hr, Wr, C, generator=g).to(dtype)
    q = real.double().view(B * Hr * Wr, 3, heads, 32)
    keys = torch.cat([q[:, 1], pad.double().view(1, 3, heads, 32)[:, 1]])
    lg = torch.einsum("nhc,mhc->hnm", q[:, 0], keys) * SCALE
    assert 60 <= lg.abs().max() <= 90 and 60 <= lg[..., -1].abs().max()
    ek, ec, bound = _measure(real, pad, rpb, dout, case, dtype)
    _report(capsys, f"{str(dtype)[6:]} logits +-60..90", ek, ec, bound, 5.0)
    if dtype == torch.float32:
        for name, e, b in zip(NAMES, ek, bound):
            assert e <= 5.0 * b, (name, e, b)
    args = _dev(real, pad, rpb, dout)
    clean = [t.clone() for t in _raw(*args, case)]
    need = L.lib.ppn_na2d_bwd_vpad_workspace(*case)
    outs = (torch.empty_like(clean[0]), torch.empty_like(clean[1]), torch.empty_like(clean[2]), torch.full((need,), float("nan"), device=DEV))
    again = _raw(*args, case, outs=outs)
    for x, y in zip(clean, again):
        assert bool(torch.isfinite(y).all()) and torch.equal(x, y)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bitwise_reproducible(dtype):
    case = (4, 56, 56, 30, 45, 2, 8)
    args = _dev(*_inputs(case, dtype, 77))
    runs = []
    for i in range(3):
        runs.append([t.clone() for t in _raw(*args, case)])
        a = torch.randn(1024, 1024, device=DEV)                                          # unrelated work in between
        (a @ a).sum().item()
        if i == 1:
            _raw(*_dev(*_inputs(CASES[3], dtype, 5)), CASES[3])
    for r in runs[1:]:
        for x, y in zip(runs[0], r):
            assert torch.equal(x, y)
    assert float(runs[0][1].abs().max()) > 0 and float(runs[0][2].abs().max()) > 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_memory_it_may_touch_and_known_answers(dtype):
    from ppnet_amd import _lib as L
    case = CASES[3]
    B, H, W, Hr, Wr, heads, d = case
    C = heads * 32
    CANARY = 12345.0
    real, pad, rpb, dout = _dev(*_inputs(case, dtype, 11))
    plain = [t.clone() for t in _raw(real, pad, rpb, dout, case)]
    need = L.lib.ppn_na2d_bwd_vpad_workspace(*case)
    sizes = (B * Hr * Wr * 3 * C, 3 * C, heads * 169, need)

    def canaries():                                  # outputs and workspace as views inside canary-filled buffers (16-byte aligned)
        bufs = [torch.full((n + 2 * 1024,), CANARY, dtype=(dtype if i == 0 else torch.float32), device=DEV) for i, n in enumerate(sizes)]
        views = [b[1024:1024 + n] for b, n in zip(bufs, sizes)]
        return bufs, (views[0].view(B, Hr, Wr, 3 * C), views[1], views[2].view(heads, 13, 13), views[3])
    bufs, outs = canaries()
    got = _raw(real, pad, rpb, dout, case, outs=outs)
    for b, n in zip(bufs, sizes):
        assert bool((b[:1024] == CANARY).all()) and bool((b[1024 + n:] == CANARY).all())
    for x, y in zip(plain, got):
        assert torch.equal(x, y) and not bool((y == CANARY).any())
    assert bool((got[1][:C] == 0).all()) and float(got[1][C:2 * C].abs().max()) > 0 and float(got[1][2 * C:].abs().max()) > 0
    # dout = 0: every output exactly 0, every element written
    bufs, outs = canaries()
    for t in _raw(real, pad, rpb, torch.zeros_like(dout), case, outs=outs):
        assert bool((t == 0).all())
    # a workspace one float short is refused and nothing runs
    bufs, outs = canaries()
    _raw(real, pad, rpb, dout, case, outs=outs, ws_floats=need - 1, want_rc=-1)
    assert all(bool((b == CANARY).all()) for b in bufs)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_autograd_function_is_the_raw_call(dtype):
    """na.na2d_autograd with pad_kv returns ppn_na2d_fwd_vpad's output and ppn_na2d_bwd_vpad's gradients: dqkv as is, dpad_kv cast
    to pad_kv's dtype and shaped [3C], drpb; without pad_kv it is the materialised function, uncounted."""
    from ppnet_amd import na
    case = CASES[0]
    B, H, W, Hr, Wr, heads, d = case
    real, pad, rpb, dout = _dev(*_inputs(case, dtype, 13))
    raw = _raw(real, pad, rpb, dout, case)
    q, p, r = (t.clone().requires_grad_(True) for t in (real, pad, rpb))
    calls = dict(na.TRAIN_CALLS)
    assert set(calls) == {"fwd_vpad_kernel", "bwd_vpad_kernel"}
    out = na.na2d_autograd(q, r, heads, d, SCALE, pad_kv=p, padded_hw=(H, W))
    assert torch.equal(out, na.na2d_forward(real, rpb, heads, d, SCALE, pad_kv=pad, padded_hw=(H, W)))
    gq, gp, gr = torch.autograd.grad(out, (q, p, r), dout)
    assert torch.equal(gq, raw[0]) and torch.equal(gp, raw[1].to(dtype)) and torch.equal(gr, raw[2])
    assert gp.shape == (3 * heads * 32,) and gp.dtype == dtype
    assert na.TRAIN_CALLS == {"fwd_vpad_kernel": calls["fwd_vpad_kernel"] + 1, "bwd_vpad_kernel": calls["bwd_vpad_kernel"] + 1}
    out = na.na2d_autograd(q, r, heads, d, SCALE, pad_kv=pad, padded_hw=(H, W))          # a Linear without bias: pad_kv needs no grad
    assert torch.autograd.grad(out, (q, r), dout)[0].shape == q.shape
    full = _full(real, pad, H, W).requires_grad_(True)
    na.na2d_autograd(full, r, heads, d, SCALE).backward(torch.ones(B, H, W, heads * 32, dtype=dtype, device=DEV))
    assert na.TRAIN_CALLS == {"fwd_vpad_kernel": calls["fwd_vpad_kernel"] + 2, "bwd_vpad_kernel": calls["bwd_vpad_kernel"] + 2}


# ------------------------------------------------------------------------------------------------ module
def _materialised_module(m, x):
    """NeighborhoodAttention2D's training branch as it was: zero-pad, qkv, NA over the padded grid, crop, proj."""
    import torch.nn.functional as F
    from ppnet_amd.na import na2d_autograd
    B, H, W, _ = x.shape
    Hp, Wp = m.padded_hw(H, W)
    o = na2d_autograd(m.qkv(F.pad(x, (0, 0, 0, Wp - W, 0, Hp - H))), m.rpb, m.num_heads, m.dilation, m.scale)
    return m.proj(o[:, :H, :W])


def _module_grads(m, x0, dy, forward):
    x = x0.clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    forward(m, x).backward(dy)
    return {"input": x.grad.detach().double().cpu(), **{n: p.grad.detach().double().cpu() for n, p in m.named_parameters() if p.grad is not None}}


@pytest.mark.parametrize("qkv_bias", [True, False])
def test_module_gradients_through_the_kernel(qkv_bias, capsys):
    """NeighborhoodAttention2D(64, 7, dilation=2, num_heads=2) on x [2, 9, 10, 64] in float32 (padded to 14 x 14): the gradient of
    the input and of every parameter — qkv.bias among them, which receives the padded positions' share through dpad_kv — against
    the float64 CPU definition (oracle.segnet_ref.na_fp64 under autograd), under the rule with the pad / crop composition as the
    materialised path.  One vpad launch each way, and the saved qkv holds the real tokens only: F.pad is not reached."""
    from oracle import segnet_ref as SR
    from ppnet_amd import na
    torch.manual_seed(5)
    m = na.NeighborhoodAttention2D(64, 7, dilation=2, num_heads=2, qkv_bias=qkv_bias).train()
    with torch.no_grad():
        m.rpb.add_(0.3 * torch.randn_like(m.rpb))
    g = torch.Generator().manual_seed(9)
    x0, dy = torch.randn(2, 9, 10, 64, generator=g), torch.randn(2, 9, 10, 64, generator=g)

    def fp64(mm, x):
        return SR.na_fp64(x, mm.qkv.weight, mm.qkv.bias, mm.rpb, mm.proj.weight, mm.proj.bias, mm.num_heads, 7, mm.dilation)
    ref = _module_grads(copy.deepcopy(m).double(), x0.double(), dy.double(), fp64)
    mg = copy.deepcopy(m).to(DEV)
    calls = dict(na.TRAIN_CALLS)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(tuple(t.shape)), t)[1], lambda t: t):
        got = _module_grads(mg, x0.to(DEV), dy.to(DEV), lambda mm, x: mm(x))
    assert na.TRAIN_CALLS == {"fwd_vpad_kernel": calls["fwd_vpad_kernel"] + 1, "bwd_vpad_kernel": calls["bwd_vpad_kernel"] + 1}
    assert (2, 9, 10, 192) in saved and not any(s[1:3] == (14, 14) for s in saved if len(s) == 4), saved
    lib = _module_grads(mg, x0.to(DEV), dy.to(DEV), _materialised_module)
    assert na.TRAIN_CALLS["bwd_vpad_kernel"] == calls["bwd_vpad_kernel"] + 1
    want = {"input", "qkv.weight", "rpb", "proj.weight", "proj.bias"} | ({"qkv.bias"} if qkv_bias else set())
    assert set(got) == set(ref) == set(lib) == want
    for n in sorted(ref):
        r = ref[n].abs().max().item()
        assert r > 0 and bool(torch.isfinite(got[n]).all()), n
        ek, el = (got[n] - ref[n]).abs().max().item() / r, (lib[n] - ref[n]).abs().max().item() / r
        with capsys.disabled():
            print(f"\nna module float32 qkv_bias={qkv_bias} {n}: vpad path {ek:.2e} x max, pad / crop composition {el:.2e}", end="")
        assert ek <= max(2.0 * el, 2e-4), (n, ek, el)
    # inference and the materialised real_hw= form are not counted
    with torch.no_grad():
        mg(x0.to(DEV))
    assert na.TRAIN_CALLS["fwd_vpad_kernel"] == calls["fwd_vpad_kernel"] + 1


def test_module_peak_memory_below_the_materialised_composition(capsys):
    """One NeighborhoodAttention2D at B 8, 56 x 56, C 128, 4 heads, dilation 16 (DiNAT-B level 0 at R = 224: padded to 112 x 112),
    float32: forward + backward raise the peak of allocated memory by strictly less than the pad / crop composition, which holds a
    4 x larger qkv."""
    from ppnet_amd import na
    B, R, C = 8, 56, 128
    torch.manual_seed(0)
    m = na.NeighborhoodAttention2D(C, 7, dilation=16, num_heads=4).to(DEV).train()

    def peak(forward):
        x = torch.randn(B, R, R, C, device=DEV, requires_grad=True)
        dy = torch.randn(B, R, R, C, device=DEV)
        m.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        held = torch.cuda.memory_allocated()
        forward(m, x).backward(dy)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - held
    peak(lambda mm, x: mm(x))                                                          # library workspaces allocated once
    calls = dict(na.TRAIN_CALLS)
    rise = peak(lambda mm, x: mm(x))
    assert na.TRAIN_CALLS == {"fwd_vpad_kernel": calls["fwd_vpad_kernel"] + 1, "bwd_vpad_kernel": calls["bwd_vpad_kernel"] + 1}
    peak(_materialised_module)
    comp = peak(_materialised_module)
    with capsys.disabled():
        print(f"\nNeighborhoodAttention2D B {B} {R}x{R} C {C} dilation 16 float32: peak rise {rise / 2 ** 20:.1f} MiB on the vpad path, "
              f"{comp / 2 ** 20:.1f} MiB on the pad / crop composition; one padded qkv {B * 112 * 112 * 3 * C * 4 / 2 ** 20:.1f} MiB")
    assert rise < comp, (rise, comp)


# ------------------------------------------------------------------------------------------------ training
def _codes(B, R, seed):
    g = torch.Generator().manual_seed(seed)
    lo = (torch.rand(B, 1, R // 16, R // 16, generator=g) > 0.4).float()
    return (torch.nn.functional.interpolate(lo, size=(R, R), mode="nearest")[:, 0] * 255).to(torch.uint8)


@pytest.mark.parametrize("amp", [None, torch.bfloat16], ids=["float32", "bf16-autocast"])
def test_reduced_dinat_training_steps_use_the_vpad_kernels(amp):
    """DINAT_BASE with depths [1, 1, 2, 1], one padded dilated layer of every kind per level (dilation 16 / 8 / 3, 4 / 2 on the
    56 / 28 / 14 / 7 token grids of R = 224), batch 2, 12 SGD steps: the loss falls, every gradient is finite, every level's rpb and
    qkv.bias gradient is non-zero, and each step launches the vpad forward and backward once per padded layer.  The learning rate
    is the reference's 0.02 for 16 images (SegNet/configs/dinat/dinat_base.py:27-32) scaled linearly to the 2 of this test."""
    from ppnet_amd import na, segnet, train
    cfg = copy.deepcopy(segnet.DINAT_BASE)
    cfg["backbone"].update(depths=[1, 1, 2, 1], dilations=[[16], [8], [3, 4], [2]], drop_path_rate=0.0)
    torch.manual_seed(1)
    net = segnet.SegNet(**cfg).to(DEV)
    layers = [m for m in net.modules() if isinstance(m, na.NeighborhoodAttention2D)]
    sides = (56, 28, 14, 14, 7)
    assert [m.dilation for m in layers] == [16, 8, 3, 4, 2] and all(m.padded_hw(s, s) is not None for m, s in zip(layers, sides))
    trainer = train.segnet_trainer(net)
    opt = train.segnet_optimizer(trainer, lr=0.02 * 2 / 16)
    codes = _codes(2, 224, 5).to(DEV)
    labels = (codes > 0).to(torch.uint8)
    na.TRAIN_CALLS.update(fwd_vpad_kernel=0, bwd_vpad_kernel=0)
    losses = []
    for it in range(12):
        with torch.autocast("cuda", dtype=amp, enabled=amp is not None):
            losses.append(float(train.segnet_train_step(trainer, opt, it, 40, codes, labels, schedule=dict(warmup_iters=3, warmup_ratio=0.1))))
        assert na.TRAIN_CALLS == {"fwd_vpad_kernel": 5 * (it + 1), "bwd_vpad_kernel": 5 * (it + 1)}
        if it == 0:
            missing = [n for n, p in net.named_parameters() if p.requires_grad and p.grad is None]
            assert not missing, missing
            for n, p in net.named_parameters():
                if n.endswith("attn.rpb") or n.endswith("attn.qkv.bias"):
                    assert float(p.grad.abs().sum()) > 0, n
        assert all(bool(torch.isfinite(p.grad).all()) for p in net.parameters() if p.grad is not None)
    assert len([n for n, _ in net.named_parameters() if n.endswith("attn.rpb")]) == 5
    assert all(l == l for l in losses) and losses[-1] < losses[0], losses
