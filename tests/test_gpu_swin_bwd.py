"""ppn_swin_wmsa_bwd (csrc/swin_wmsa_bwd.hip) on the GPU: the kernel against float64 autograd of the torch composition
(swin.window_attention, pinned to the reference's forward by tests/test_swin_golden.py), known answers, bitwise reproducibility,
the memory it may touch, argument checks, the Swin module's training branch, its peak memory, and training steps of Swin + UPerHead.

The precision rule (tests/test_gpu_mhsa_bwd.py's): for each of dq, dk, dv, dpad_k, dpad_v and drpb, err = max|got - ref| / max|ref|
over EVERY element, ref = float64 autograd of window_attention on the CPU (bfloat16: on the rounded inputs; the bias table holds
bfloat16-representable values there, so kernel, chain and reference see the same numbers): err <= max(2 x the error of
window_attention under autograd on the GPU in the same data type on the same inputs, measured in the same run; FLOOR: 2e-6 float32,
1e-2 bfloat16).  Factor 2: the kernel keeps S, dP and all sums in float32 and rounds P and dS once where the bfloat16 chain rounds
every intermediate (1 x), and it sums in another order (1 x).  A reference that is exactly 0 (the q third of dpad_kv; all of it on
unpadded grids) asks for exactly 0.

Each test prints what it measured (run with -s): kernel error, chain error and bound per gradient, the module's worst gradient, both
peak-memory rises."""
import copy
import ctypes

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda"
SCALE = 32 ** -0.5
FLOOR = {torch.float32: 2e-6, torch.bfloat16: 1e-2}            # tests/test_gpu_mhsa_bwd.py: the attention kernels' bound
NAMES = ("dq", "dk", "dv", "dpad_k", "dpad_v", "drpb")
# the forward suite's 12 cases (tests/test_gpu_swin.py CASES) and one where every wave walks several windows and the reduction of
# drpb / dpad_kv has many partials: 32 x 100 windows x 4 heads = 12800 items (test_large_case_walks_several_windows_per_wave)
CASES = [(1, 7, 7, 1, 0), (1, 7, 7, 2, 3), (2, 14, 21, 2, 3), (1, 2, 3, 4, 3), (3, 4, 6, 3, 0), (1, 4, 6, 2, 3), (1, 8, 8, 32, 3),
         (2, 15, 23, 5, 3), (1, 28, 28, 4, 0), (2, 9, 16, 8, 3), (1, 64, 64, 4, 3), (3, 8, 8, 16, 0)]
LARGE = (32, 64, 64, 4, 3)


def _inputs(B, H, W, heads, seed, dtype, pad_scale=0.3):
    """qkv [B,H,W,3C], pad [3C], dout [B,H,W,C] in dtype; rpb [heads,13,13] float32 holding values dtype represents."""
    g = torch.Generator().manual_seed(seed)
    C = heads * 32
    qkv = torch.randn(B, H, W, 3 * C, generator=g).to(dtype)
    pad = (torch.randn(3 * C, generator=g) * pad_scale).to(dtype)
    rpb = (torch.randn(heads, 13, 13, generator=g) * 0.5).to(dtype).float()
    dout = torch.randn(B, H, W, C, generator=g).to(dtype)
    return qkv, pad, rpb, dout


def _composition(qkv, pad, rpb, dout, heads, shift, scale, mask_value=-100.0):
    """(dqkv, dpad [3C], drpb [heads,13,13]) of swin.window_attention under autograd, in qkv's dtype on qkv's device."""
    from ppnet_amd.swin import bias_table_hw, window_attention
    q = qkv.detach().clone().requires_grad_(True)
    p = pad.detach().clone().requires_grad_(True)
    t = rpb.to(qkv.dtype).reshape(heads, 169).t().contiguous().requires_grad_(True)     # the parameter's [(2w-1)^2, heads]
    out = window_attention(q, p, t, heads, shift, scale, mask_value=mask_value)
    gq, gp, gt = torch.autograd.grad(out, (q, p, t), dout, allow_unused=True)
    if gp is None:                                                                       # a grid without padding never reads pad
        gp = torch.zeros_like(p)
    return gq, gp, bias_table_hw(gt, heads)


def _raw(qkv, pad, rpb, dout, heads, shift, scale, outs=None, B=None, window=7, want_rc=0):
    """ppn_swin_wmsa_bwd itself on device tensors -> (dqkv, dpad_kv [3C] float32, drpb [heads,13,13] float32); `outs` = (dqkv, dpad,
    drpb, ws) may be views into larger buffers."""
    from ppnet_amd import _lib as L
    B = qkv.shape[0] if B is None else B
    H, W = qkv.shape[1:3]
    C = heads * 32
    need = L.lib.ppn_swin_wmsa_bwd_workspace(B, H, W, heads)
    assert need > 0
    if outs is None:
        outs = (torch.empty(B, H, W, 3 * C, dtype=qkv.dtype, device=DEV), torch.empty(3 * C, dtype=torch.float32, device=DEV),
                torch.empty(heads, 13, 13, dtype=torch.float32, device=DEV), torch.empty(need, dtype=torch.float32, device=DEV))
    dqkv, dpad, drpb, ws = outs
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = L.lib.ppn_swin_wmsa_bwd(P(qkv), P(pad), P(rpb), P(dout), P(dqkv), P(dpad), P(drpb), P(ws), need, B, H, W, heads, window, shift,
                                 float(scale), 0 if qkv.dtype == torch.float32 else 1, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
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


def _measure(qkv, pad, rpb, dout, heads, shift, scale, dtype):
    """(kernel errors, chain errors, bounds) for NAMES on inputs already rounded to dtype."""
    ref = _composition(qkv.double(), pad.double(), rpb.double(), dout.double(), heads, shift, scale)      # float64, CPU
    chain = _composition(*_dev(qkv, pad, rpb, dout), heads, shift, scale)
    got = _raw(*_dev(qkv, pad, rpb, dout), heads, shift, scale)
    assert got[0].dtype == dtype and got[0].shape == qkv.shape and all(bool(torch.isfinite(t).all()) for t in got)
    ek, ec = _errors(got, ref, heads), _errors(chain, ref, heads)
    return ek, ec, [max(2.0 * c, FLOOR[dtype]) for c in ec]


def _report(capsys, what, ek, ec, bound, factor=1.0):
    with capsys.disabled():
        f = lambda v: " ".join(f"{x:.2e}" for x in v)
        print(f"\nswin_bwd {what}: {' '.join(NAMES)} kernel {f(ek)} | chain {f(ec)} | bound {factor:g} x {f(bound)}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,H,W,heads,shift", CASES + [LARGE])
def test_kernel_vs_float64(dtype, B, H, W, heads, shift, capsys):
    qkv, pad, rpb, dout = _inputs(B, H, W, heads, 100 * H + W + heads + shift, dtype)
    ek, ec, bound = _measure(qkv, pad, rpb, dout, heads, shift, SCALE, dtype)
    _report(capsys, f"{str(dtype)[6:]} B {B} {H}x{W} heads {heads} shift {shift}", ek, ec, bound)
    for name, e, b in zip(NAMES, ek, bound):
        assert e <= b, (name, B, H, W, heads, shift, e, b)


def test_large_case_walks_several_windows_per_wave():
    """The geometry behind LARGE: the workspace holds 256 floats per workgroup of the largest grid the launcher may choose, a
    workgroup has at most 4 waves, and LARGE has at least 4 items (window, head) per launched wave."""
    from ppnet_amd import _lib as L
    B, H, W, heads, _ = LARGE
    need = L.lib.ppn_swin_wmsa_bwd_workspace(B, H, W, heads)
    assert need > 0 and need % 256 == 0
    waves = need // 256 * 4
    items = B * ((H + 6) // 7) * ((W + 6) // 7) * heads
    assert items >= 4 * waves, (items, waves)
    assert need // 256 >= 8 * heads * 2                                                  # several partials per head for the reduction


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_large_logits_mask_is_minus_100(dtype, capsys):
    """The forward suite's logits of +-60..90 with the shift's region mask: finite, within 5 x the rule (the precedent's margin for
    this input), and the gradient of the -100 mask, measurably not the -inf one's."""
    B, H, W, heads, shift = 1, 14, 17, 2, 3
    g = torch.Generator().manual_seed(7)
    C = heads * 32
    u = torch.randn(32, generator=g)
    u = u / u.norm()
    Hp, Wp = 14, 21
    lab = lambda y, n: 0 if (y - shift) % n < n - 7 else (1 if (y - shift) % n < n - shift else 2)
    sgn = torch.tensor([[(-1.0) ** (lab(i, Hp) + lab(j, Wp)) for j in range(W)] for i in range(H)])
    a = (80.0 / SCALE) ** 0.5
    qkv = torch.randn(B, H, W, 3, heads, 32, generator=g) * 0.05
    qkv[..., 0, :, :] += a * sgn[None, :, :, None, None] * u
    qkv[..., 1, :, :] -= a * sgn[None, :, :, None, None] * u
    qkv[..., 2, :, :] = torch.randn(B, H, W, heads, 32, generator=g)
    qkv = qkv.reshape(B, H, W, 3 * C).to(dtype)
    pad = torch.zeros(3 * C).to(dtype)
    rpb = (torch.randn(heads, 13, 13, generator=g) * 0.5).to(dtype).float()
    dout = torch.randn(B, H, W, C, generator=g).to(dtype)
    lg = (qkv.double()[..., :32] * SCALE * qkv.double()[..., C:C + 32]).sum(-1)
    assert 60 <= lg.abs().max() <= 90
    ek, ec, bound = _measure(qkv, pad, rpb, dout, heads, shift, SCALE, dtype)
    _report(capsys, f"{str(dtype)[6:]} logits +-60..90", ek, ec, bound, 5.0)
    for name, e, b in zip(NAMES, ek, bound):
        assert e <= 5.0 * b, (name, e, b)
    ref = _composition(qkv.double(), pad.double(), rpb.double(), dout.double(), heads, shift, SCALE)
    rinf = _composition(qkv.double(), pad.double(), rpb.double(), dout.double(), heads, shift, SCALE, mask_value=float("-inf"))
    got = _raw(*_dev(qkv, pad, rpb, dout), heads, shift, SCALE)
    dv_ref, dv_inf, dv_got = (_parts(*t, heads)[0][2] for t in (ref, rinf, got))
    apart = (dv_ref - dv_inf).abs().max().item() / dv_ref.abs().max().item()
    mine = (dv_got - dv_inf).abs().max().item() / dv_ref.abs().max().item()
    with capsys.disabled():
        print(f"swin_bwd {str(dtype)[6:]} logits +-60..90: dv of the -100 mask and of the -inf mask differ by {apart:.2e} x max; the kernel's "
              f"from the -inf one's by {mine:.2e}")
    assert apart > 0.05 and mine > 0.5 * apart


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_known_answers(dtype, capsys):
    from ppnet_amd import _lib as L
    CANARY = 777.0
    for (B, H, W, heads, shift) in ((2, 9, 11, 3, 3), (2, 14, 7, 2, 3), (1, 14, 14, 2, 0)):
        qkv, pad, rpb, dout = _dev(*_inputs(B, H, W, heads, 31 + H, dtype))
        C = heads * 32
        need = L.lib.ppn_swin_wmsa_bwd_workspace(B, H, W, heads)

        def canaries():
            return (torch.full((B, H, W, 3 * C), CANARY, dtype=dtype, device=DEV), torch.full((3 * C,), CANARY, device=DEV),
                    torch.full((heads, 13, 13), CANARY, device=DEV), torch.full((need,), CANARY, device=DEV))
        # dout = 0: every output exactly 0, every element written
        z = _raw(qkv, pad, rpb, torch.zeros_like(dout), heads, shift, SCALE, outs=canaries())
        for t in z:
            assert bool((t == 0).all())
        got = _raw(qkv, pad, rpb, dout, heads, shift, SCALE, outs=canaries())
        for t in got:
            assert bool(torch.isfinite(t).all()) and not bool((t == CANARY).any())
        dqkv, dpad, drpb = got
        assert bool((dpad[:C] == 0).all())                                               # the q third
        if H % 7 == 0 and W % 7 == 0:
            assert bool((dpad == 0).all())                                               # no padded position: exactly 0
        else:
            assert float(dpad[C:2 * C].abs().max()) > 0 and float(dpad[2 * C:].abs().max()) > 0
        # rows of dS sum to 0, so the 169 bins of a head sum to 0 to rounding.  Measured against sum|drpb bins| of the float64
        # reference, which is at most sum|dS| (a bin is a sum of dS values): the smaller yardstick, the stricter check
        ref = _composition(qkv.double().cpu(), pad.double().cpu(), rpb.double().cpu(), dout.double().cpu(), heads, shift, SCALE)[2]
        tot = drpb.double().cpu().sum(dim=(1, 2)).abs()
        yard = ref.abs().sum(dim=(1, 2))
        with capsys.disabled():
            print(f"\nswin_bwd {str(dtype)[6:]} {H}x{W}: max over heads |sum of drpb bins| / sum|bins| = {(tot / yard).max().item():.2e}")
        assert bool((tot <= FLOOR[dtype] * yard).all()), (tot, yard)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bitwise_reproducible(dtype):
    B, H, W, heads, shift = 8, 30, 45, 4, 3
    qkv, pad, rpb, dout = _dev(*_inputs(B, H, W, heads, 77, dtype))
    runs = []
    for i in range(3):
        runs.append([t.clone() for t in _raw(qkv, pad, rpb, dout, heads, shift, SCALE)])
        a = torch.randn(1024, 1024, device=DEV)                                          # unrelated work in between
        (a @ a).sum().item()
        if i == 1:
            _raw(*_dev(*_inputs(3, 8, 8, 16, 5, dtype)), 16, 0, SCALE)
    for r in runs[1:]:
        for u, v in zip(runs[0], r):
            assert torch.equal(u, v)
    assert float(runs[0][1].abs().max()) > 0 and float(runs[0][2].abs().max()) > 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_memory_it_may_touch(dtype):
    from ppnet_amd import _lib as L
    B, H, W, heads, shift = 2, 9, 11, 3, 3
    C = heads * 32
    CANARY = 12345.0
    qkv, pad, rpb, dout = _dev(*_inputs(B, H, W, heads, 11, dtype))
    plain = [t.clone() for t in _raw(qkv, pad, rpb, dout, heads, shift, SCALE)]
    need = L.lib.ppn_swin_wmsa_bwd_workspace(B, H, W, heads)
    # outputs and workspace as views inside canary-filled buffers (offsets keep the 16-byte alignment)
    sizes = (B * H * W * 3 * C, 3 * C, heads * 169, need)
    bufs = [torch.full((n + 2 * 1024,), CANARY, dtype=(dtype if i == 0 else torch.float32), device=DEV) for i, n in enumerate(sizes)]
    views = [b[1024:1024 + n] for b, n in zip(bufs, sizes)]
    got = _raw(qkv, pad, rpb, dout, heads, shift, SCALE,
               outs=(views[0].view(B, H, W, 3 * C), views[1], views[2].view(heads, 13, 13), views[3]))
    for b, n in zip(bufs, sizes):
        assert bool((b[:1024] == CANARY).all()) and bool((b[1024 + n:] == CANARY).all())
    for u, v in zip(plain, got):
        assert torch.equal(u, v)
    # large finite garbage in the token rows just past B * H * W of qkv and dout is never read
    rows = B * H * W
    qbig = torch.full((rows + 64, 3 * C), 1.0e30, dtype=dtype, device=DEV)
    dbig = torch.full((rows + 64, C), -1.0e30, dtype=dtype, device=DEV)
    qbig[:rows] = qkv.view(rows, 3 * C)
    dbig[:rows] = dout.view(rows, C)
    again = _raw(qbig[:rows].view(B, H, W, 3 * C), pad, rpb, dbig[:rows].view(B, H, W, C), heads, shift, SCALE)
    for u, v in zip(plain, again):
        assert torch.equal(u, v)


def test_bad_arguments_on_gpu_buffers():
    from ppnet_amd import _lib as L
    B, H, W, heads = 1, 7, 9, 1
    qkv, pad, rpb, dout = _dev(*_inputs(B, H, W, heads, 3, torch.float32))
    need = L.lib.ppn_swin_wmsa_bwd_workspace(B, H, W, heads)
    outs = [torch.zeros(B, H, W, 96, device=DEV), torch.zeros(96, device=DEV), torch.zeros(1, 13, 13, device=DEV), torch.zeros(need, device=DEV)]
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = [P(qkv), P(pad), P(rpb), P(dout), P(outs[0]), P(outs[1]), P(outs[2]), P(outs[3]), need, B, H, W, heads, 7, 3, SCALE, 0, s]

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return L.lib.ppn_swin_wmsa_bwd(*a)
    E_INVALID, E_UNSUPPORTED = -1, -3
    assert call(a3=None) == E_INVALID and call(a6=None) == E_INVALID
    assert call(a4=ctypes.c_void_p(outs[0].data_ptr() + 4)) == E_INVALID                  # 16-byte alignment
    assert call(a8=need - 1) == E_INVALID and call(a15=float("nan")) == E_INVALID and call(a16=3) == E_INVALID
    assert call(a13=8) == E_UNSUPPORTED and call(a14=2) == E_UNSUPPORTED
    assert all(bool((t == 0).all()) for t in outs)                                        # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    assert float(outs[0].abs().max()) > 0 and float(outs[2].abs().max()) > 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_autograd_function_is_the_raw_call(dtype):
    """swin.wmsa_autograd returns ppn_swin_wmsa_fwd's output and ppn_swin_wmsa_bwd's gradients: dqkv as is, dpad_kv cast to pad_kv's
    dtype, drpb in the parameter's [(2w-1)^2, heads] layout; None for a pad_kv that does not require grad."""
    from ppnet_amd import swin
    B, H, W, heads, shift = 2, 9, 11, 3, 3
    qkv, pad, rpb, dout = _dev(*_inputs(B, H, W, heads, 13, dtype))
    raw = _raw(qkv, pad, rpb, dout, heads, shift, SCALE)
    q, p = qkv.clone().requires_grad_(True), pad.clone().requires_grad_(True)
    t = rpb.reshape(heads, 169).t().contiguous().requires_grad_(True)
    calls, train = dict(swin.CALLS), dict(swin.TRAIN_CALLS)
    out = swin.wmsa_autograd(q, p, t, heads, shift, SCALE)
    with torch.no_grad():
        assert torch.equal(out, swin.wmsa_forward(qkv, pad, rpb, heads, shift, SCALE))
    gq, gp, gt = torch.autograd.grad(out, (q, p, t), dout)
    assert torch.equal(gq, raw[0]) and torch.equal(gp, raw[1].to(dtype)) and torch.equal(swin.bias_table_hw(gt, heads), raw[2])
    assert gt.shape == (169, heads)
    assert swin.TRAIN_CALLS == {"fwd_kernel": train["fwd_kernel"] + 1, "bwd_kernel": train["bwd_kernel"] + 1}
    assert swin.CALLS == {"kernel": calls["kernel"] + 1, "torch": calls["torch"]}        # the wmsa_forward above only
    out = swin.wmsa_autograd(q, pad, t, heads, shift, SCALE)                             # no qkv bias
    assert torch.autograd.grad(out, (q, t), dout)[0].shape == q.shape


# ------------------------------------------------------------------------------------------------ module
def _small_swin():
    from ppnet_amd import swin
    torch.manual_seed(4)
    m = swin.SwinTransformer(embed_dims=64, depths=(2, 2), num_heads=(2, 4), strides=(4, 2), out_indices=(0, 1), drop_path_rate=0.0)
    with torch.no_grad():                                                              # biases, norms and tables off their neutral values
        for n, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
            if n.endswith("relative_position_bias_table"):
                p.add_(0.3 * torch.randn_like(p))
    return m


def _grads(m, x0, ws):
    x = x0.clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    sum((o * w).sum() for o, w in zip(m(x), ws)).backward()
    return {"input": x.grad.detach().double().cpu(), **{n: p.grad.detach().double().cpu() for n, p in m.named_parameters() if p.grad is not None}}


def test_module_gradients_through_the_kernel(monkeypatch, capsys):
    """A small SwinTransformer in float32 (two stages, shift 0 and 3 in each, a 60 x 92 input so both levels pad): gradients of the
    input and of every parameter through the kernel path and through the torch composition (same weights, same GPU), each against
    the float64 CPU model: the rule above with the composition as the chain, relative to each gradient's max."""
    from ppnet_amd import swin
    m = _small_swin().train()
    g = torch.Generator().manual_seed(8)
    x0 = torch.randn(2, 3, 60, 92, generator=g)
    ws = [torch.randn(2, 64, 15, 23, generator=g), torch.randn(2, 128, 8, 12, generator=g)]
    ref = _grads(copy.deepcopy(m).double(), x0.double(), [w.double() for w in ws])     # CPU: window_attention in float64
    mg = copy.deepcopy(m).to(DEV)
    xg, wg = x0.to(DEV), [w.to(DEV) for w in ws]
    swin.CALLS.update(kernel=0, torch=0)
    swin.TRAIN_CALLS.update(fwd_kernel=0, bwd_kernel=0)
    got = _grads(mg, xg, wg)
    torch.cuda.synchronize()
    assert swin.TRAIN_CALLS == {"fwd_kernel": 4, "bwd_kernel": 4} and swin.CALLS == {"kernel": 0, "torch": 0}   # one per block
    with monkeypatch.context() as mp:
        mp.setattr(swin.ShiftWindowMSA, "trains_on_kernel", lambda self, qkv: False)
        lib = _grads(mg, xg, wg)
    assert swin.TRAIN_CALLS == {"fwd_kernel": 4, "bwd_kernel": 4} and swin.CALLS == {"kernel": 0, "torch": 4}
    assert set(got) == set(ref) == set(lib) and len(got) > 40
    named = [n for n in ref if n.endswith("qkv.bias") or n.endswith("relative_position_bias_table")]
    assert len(named) == 8
    worst = (0.0, 0.0, None)
    for n in ref:
        r = ref[n].abs().max().item()
        assert r > 0, n
        ek, el = (got[n] - ref[n]).abs().max().item() / r, (lib[n] - ref[n]).abs().max().item() / r
        if ek > worst[0]:
            worst = (ek, el, n)
        if n in named:
            with capsys.disabled():
                print(f"swin module float32 {n}: kernel path {ek:.2e} x max, composition {el:.2e}")
        assert ek <= max(2.0 * el, FLOOR[torch.float32]), (n, ek, el)
    with capsys.disabled():
        print(f"\nswin module float32: worst kernel-path gradient error {worst[0]:.2e} x max (composition {worst[1]:.2e}) at {worst[2]}")
    # inference keeps ppn_swin_wmsa_fwd and its counter; eval() with grad enabled takes the kernel path
    swin.CALLS.update(kernel=0, torch=0)
    swin.TRAIN_CALLS.update(fwd_kernel=0, bwd_kernel=0)
    with torch.no_grad():
        mg(xg)
    assert swin.CALLS == {"kernel": 4, "torch": 0} and swin.TRAIN_CALLS == {"fwd_kernel": 0, "bwd_kernel": 0}
    mg.eval()
    _grads(mg, xg, wg)
    assert swin.CALLS == {"kernel": 4, "torch": 0} and swin.TRAIN_CALLS == {"fwd_kernel": 4, "bwd_kernel": 4}
    # an active attention dropout in training keeps raising
    md = swin.ShiftWindowMSA(64, 2, 7, attn_drop_rate=0.1).to(DEV).train()
    with pytest.raises(NotImplementedError):
        md(torch.randn(1, 7, 7, 64, device=DEV, requires_grad=True))


def test_module_peak_memory_below_the_composition(monkeypatch, capsys):
    """One ShiftWindowMSA at B 64, 64 x 64, C 128, shift 3, float32: forward + backward raise the peak of allocated memory by
    strictly less on the kernel path than on the torch composition (which keeps [B nW, heads, 49, 49] tensors), same test."""
    from ppnet_amd import swin
    B, R, C = 64, 64, 128
    torch.manual_seed(0)
    m = swin.ShiftWindowMSA(C, 4, 7, shift_size=3).to(DEV).train()

    def peak():
        x = torch.randn(B, R, R, C, device=DEV, requires_grad=True)
        dy = torch.randn(B, R, R, C, device=DEV)
        m.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        held = torch.cuda.memory_allocated()
        m(x).backward(dy)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - held
    peak()                                                                             # library workspaces allocated once
    swin.TRAIN_CALLS.update(fwd_kernel=0, bwd_kernel=0)
    rise = peak()
    assert swin.TRAIN_CALLS == {"fwd_kernel": 1, "bwd_kernel": 1}
    with monkeypatch.context() as mp:
        mp.setattr(swin.ShiftWindowMSA, "trains_on_kernel", lambda self, qkv: False)
        peak()
        comp = peak()
    one_p = B * 100 * 4 * 49 * 49 * 4
    with capsys.disabled():
        print(f"\nShiftWindowMSA B {B} {R}x{R} C {C} shift 3 float32: peak rise {rise / 1e6:.1f} MB on the kernel path, {comp / 1e6:.1f} MB on "
              f"the torch composition; one [B nW, heads, 49, 49] tensor {one_p / 1e6:.1f} MB")
    assert rise < comp, (rise, comp)


# ------------------------------------------------------------------------------------------------ training
def _codes(B, R, seed):
    g = torch.Generator().manual_seed(seed)
    lo = (torch.rand(B, 1, R // 16, R // 16, generator=g) > 0.4).float()
    return (torch.nn.functional.interpolate(lo, size=(R, R), mode="nearest")[:, 0] * 255).to(torch.uint8)


def _reduced_swin_uper():
    from ppnet_amd import segnet
    cfg = copy.deepcopy(segnet.SWIN_BASE_UPER)
    cfg["backbone"].update(embed_dims=32, depths=(2, 2, 2, 2), num_heads=(1, 2, 4, 8), drop_path_rate=0.0)
    cfg["decode_head"].update(in_channels=[32, 64, 128, 256], channels=64)
    cfg["auxiliary_head"].update(in_channels=128, channels=32)
    return cfg


def test_segnet_swin_training_steps_use_the_backward_kernel():
    """SGD + cross-entropy on (rendered map, mask_space) pairs from the generator for a small Swin + UPerHead at R = 128 (every
    level pads): every trainable parameter receives a finite gradient, every bias table a non-zero one, each block's attention runs
    on the forward and backward kernels, 12 steps lower the loss."""
    from ppnet_amd import edage, swin, train
    from ppnet_amd.segnet import SegNet
    dev = torch.device("cuda:0")
    pb = edage.generate_paths(2, 128, 50, 3, seed=4, device=dev)
    mb = edage.generate_maps(pb, 3, 5, 20, seed=4)
    grid, space, path = train.generator_pairs(pb, mb, 3)
    torch.manual_seed(1)
    net = SegNet.from_config(_reduced_swin_uper()).cuda()
    trainer = train.segnet_trainer(net)
    opt = train.segnet_optimizer(trainer, lr=0.02)
    sched = dict(warmup_iters=3, warmup_ratio=0.1)
    losses = []
    swin.CALLS.update(kernel=0, torch=0)
    swin.TRAIN_CALLS.update(fwd_kernel=0, bwd_kernel=0)
    for it in range(12):
        losses.append(float(train.segnet_train_step(trainer, opt, it, 40, grid, space, schedule=sched)))
        if it == 0:
            assert swin.TRAIN_CALLS == {"fwd_kernel": 8, "bwd_kernel": 8}
            missing = [n for n, p in net.named_parameters() if p.requires_grad and p.grad is None]
            assert not missing, missing
            assert all(torch.isfinite(p.grad).all() for p in net.parameters() if p.grad is not None)
            tables = [p for n, p in net.named_parameters() if n.endswith("relative_position_bias_table")]
            assert len(tables) == 8 and all(float(p.grad.abs().sum()) > 0 for p in tables)
            assert all(float(p.grad.abs().sum()) > 0 for n, p in net.named_parameters() if n.endswith("w_msa.qkv.bias"))
    assert swin.TRAIN_CALLS == {"fwd_kernel": 8 * 12, "bwd_kernel": 8 * 12} and swin.CALLS["torch"] == 0
    assert all(l == l for l in losses) and losses[-1] < losses[0], losses


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_full_swin_base_uper_training_step(dtype):
    """One step of the full SWIN_BASE_UPER at R = 224 on 2 images: finite loss, gradients and parameters, 24 forward and 24
    backward launches."""
    from ppnet_amd import segnet, swin, train
    torch.manual_seed(0)
    net = segnet.SegNet.from_config(segnet.SWIN_BASE_UPER).to(DEV).to(dtype)
    trainer = train.segnet_trainer(net)
    opt = train.segnet_optimizer(trainer, lr=0.01)
    codes = _codes(2, 224, 5).to(DEV)
    labels = (codes > 0).to(torch.uint8)
    swin.CALLS.update(kernel=0, torch=0)
    swin.TRAIN_CALLS.update(fwd_kernel=0, bwd_kernel=0)
    loss = train.segnet_train_step(trainer, opt, 0, 10, codes, labels, schedule=dict(warmup_iters=0))
    torch.cuda.synchronize()
    assert swin.TRAIN_CALLS == {"fwd_kernel": 24, "bwd_kernel": 24} and swin.CALLS == {"kernel": 0, "torch": 0}
    assert bool(torch.isfinite(loss))
    grads = [(n, p.grad) for n, p in net.named_parameters() if p.requires_grad]
    assert all(g is not None for _, g in grads), [n for n, g in grads if g is None]
    assert all(bool(torch.isfinite(g).all()) for _, g in grads)
    assert all(bool(torch.isfinite(p).all()) for p in net.parameters())
