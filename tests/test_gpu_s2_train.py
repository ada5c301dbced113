"""ppn_gennet_s2_down / ppn_gennet_s2_up / ppn_gennet_s2_wgrad (csrc/gennet_s2_train.hip) on the GPU: the kernels against float64 autograd
of Conv2d(24, 24, 3, 2, 1) and ConvTranspose2d(24, 24, 3, 2, 1, output_padding=1), exact integer answers, adjointness, bitwise
reproducibility, the memory they may touch, and GenNet's AE-ViT through the kernel path.

The precision rule (tests/test_gpu_tail_train.py's): err = max|got - ref| / max|ref| over EVERY element, for the forward, dx, dw and dbias
apart; ref = float64 autograd on the CPU of the same x, parameters and upstream gradient; err <= max(2 x the error of the library's
layer and autograd in the same data type (bfloat16: bfloat16 tensors under bfloat16 autocast) on the same inputs in the same run; FLOOR),
FLOOR 2e-6 float32, 1e-2 bfloat16.  The bfloat16 floor applies to the forward and dx only: dw and dbias are float32 in both data types
and use the float32 floor.  x and dy are randn rounded to bfloat16, so both data types read the same values; the parameters are the
layer's default initialisation under torch.manual_seed(seed) plus 0.1 randn on the bias.

A shape (B, H, W) is the BIG extent: a Conv2d case has x [B,24,H,W] (an odd H or W runs U, its input gradient, at extent 2 Hs - 1); a
ConvTranspose2d case has x [B,24,ceil(H/2),ceil(W/2)] and the big side is its output, 2 Hs x 2 Ws.

The kernels' own sizes: small pixels are numbered over the batch, a workgroup owns 512 consecutive ones, and a work-item of D and U owns
two of them 256 apart — its span is ONE pixel, so no row can be shorter than it: the seam shapes put 511, 512 and 513 small pixels in
rows of one pixel (equal to the span) and of 16 .. 513 pixels (longer), with row and image ends anywhere in a tile; W walks a tile in
chunks of 32 pixels and launches at most 768 workgroups, and 1255 x 1256 has 771 tiles.

Each test prints what it measured (run with -s)."""
import copy
import ctypes
import functools

import pytest

torch = pytest.importorskip("torch")
import torch.nn as nn                                                          # noqa: E402
import torch.nn.functional as F                                               # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
C = 24
F32, BF16 = torch.float32, torch.bfloat16
FLOOR = {F32: 2e-6, BF16: 1e-2}
DTYPES = [F32, BF16]
TILE, MAX_BLOCKS = 512, 768                                        # gennet_s2_train.hip: S2_TILE, S2_MAX_BLOCKS
NAMES = ("fwd", "dx", "dw", "dbias")
WIDE = (0, 1)                                                      # the forward and dx have the data type; dw and dbias are float32
SEED = 0
SEAMS = [(1, 13, 145), (1, 1023, 1), (1, 31, 64), (1, 1, 1025), (1, 53, 38)]   # 511, 512 (rows of 1), 512, 513 (one row), 513 small pixels
LARGE = (1, 1255, 1256)                                            # 628 x 628 small pixels: 771 tiles; the big operand is 151 MB
CASES = [(1, 1, 1), (1, 1, 2), (1, 2, 2), (2, 3, 5), (1, 1, 9), (1, 9, 1), (2, 7, 8), (1, 16, 16), (2, 33, 31), (2, 64, 64)] + SEAMS + [LARGE]
EXACT = [(2, 7, 8), (1, 16, 16), (1, 13, 145)]
UP = [False, True]


def _small(n):
    return (n + 1) // 2


def x_shape(shape, up):
    B, H, W = shape
    return (B, C, _small(H), _small(W)) if up else (B, C, H, W)


def layer(up):
    return nn.ConvTranspose2d(C, C, 3, 2, 1, output_padding=1) if up else nn.Conv2d(C, C, 3, 2, 1)


def build_case(shape, up, seed, exact=False):
    """Float32 CPU tensors of one case: (x, dy, weight, bias)."""
    torch.manual_seed(seed)
    conv = layer(up)
    g = torch.Generator().manual_seed(seed + 100)
    xs = x_shape(shape, up)
    ys = (xs[0], C, 2 * xs[2], 2 * xs[3]) if up else (xs[0], C, _small(xs[2]), _small(xs[3]))
    if exact:                                                       # {-1, 0, 1} data and weights, bias in {-2 .. 2}
        draw = lambda s, lo, hi: torch.randint(lo, hi + 1, s, generator=g).float()
        return draw(xs, -1, 1), draw(ys, -1, 1), draw((C, C, 3, 3), -1, 1), draw((C,), -2, 2)
    with torch.no_grad():
        conv.bias.add_(0.1 * torch.randn_like(conv.bias))
    x = torch.randn(xs, generator=g).to(BF16).float()
    dy = torch.randn(ys, generator=g).to(BF16).float()
    return x, dy, conv.weight.detach().clone(), conv.bias.detach().clone()


def composition(x, dy, w, b, up, autocast=False):
    """(fwd, dx, dw, dbias) of the library's layer under autograd, in x's dtype on x's device."""
    x, w, b = (t.detach().clone().requires_grad_(True) for t in (x, w, b))
    with torch.autocast("cuda", dtype=BF16, enabled=autocast):
        y = F.conv_transpose2d(x, w, b, 2, 1, 1) if up else F.conv2d(x, w, b, 2, 1)
    return (y.detach(),) + tuple(torch.autograd.grad(y, [x, w, b], dy.to(y.dtype)))


@functools.lru_cache(maxsize=None)
def reference(shape, up, seed, exact=False):
    """The case and its float64 CPU reference, computed once and shared by the tests that need it (never modified)."""
    case = build_case(shape, up, seed, exact)
    return case, composition(*[t.double() for t in case], up)


def kernel(x, dy, w, b, up, dtype):
    """The four outputs through the raw launches (fused._s2_down / _s2_up / _s2_wgrad) on DEV, by the table of include/ppnet_hip.h."""
    from ppnet_amd import fused
    xg, dg, wg, bg = x.to(DEV).to(dtype), dy.to(DEV).to(dtype), w.to(DEV), (b.to(DEV) if b is not None else None)
    if up:
        y = fused._s2_up(xg, wg, bg, 2 * x.shape[2], 2 * x.shape[3])
        dx = fused._s2_down(dg, wg, None)
        dw, none, db = fused._s2_wgrad(xg, dg, False, True)
    else:
        y = fused._s2_down(xg, wg, bg)
        dx = fused._s2_up(dg, wg, None, x.shape[2], x.shape[3])
        dw, db, none = fused._s2_wgrad(dg, xg, True, False)
    torch.cuda.synchronize()
    assert none is None and y.dtype == dx.dtype == dtype and y.shape == dy.shape and dx.shape == x.shape
    assert dw.dtype == db.dtype == F32 and dw.shape == (C, C, 3, 3) and db.shape == (C,)
    return y, dx, dw, db


def _rel(got, ref):
    d, r = (got.double().cpu() - ref).abs().max().item(), ref.abs().max().item()
    return d / r if r > 0 else (0.0 if d == 0 else float("inf"))


def _fmt(v):
    return " ".join(f"{x:.2e}" for x in v)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("up", UP)
@pytest.mark.parametrize("shape", CASES)
def test_kernel_vs_float64(shape, up, dtype, capsys):
    (x, dy, w, b), ref = reference(shape, up, SEED)
    got = kernel(x, dy, w, b, up, dtype)
    lib = composition(x.to(DEV).to(dtype), dy.to(DEV), w.to(DEV), b.to(DEV), up, autocast=dtype == BF16)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    ek, el = [_rel(a, r) for a, r in zip(got, ref)], [_rel(a, r) for a, r in zip(lib, ref)]
    bound = [max(2.0 * e, FLOOR[dtype if i in WIDE else F32]) for i, e in enumerate(el)]
    with capsys.disabled():
        print(f"\ns2 {'convT' if up else 'conv'} {str(dtype)[6:]} B H W {shape}: {' '.join(NAMES)} kernel {_fmt(ek)} | library {_fmt(el)} | "
              f"bound {_fmt(bound)}")
    for name, e, bd in zip(NAMES, ek, bound):
        assert e <= bd, (name, shape, up, e, bd)


# ------------------------------------------------------------------------------------------------------------------------ exact values
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("up", UP)
@pytest.mark.parametrize("shape", EXACT)
def test_integer_inputs_give_the_float64_answer_bit_for_bit(shape, up, dtype):
    """x, dy and w from {-1, 0, 1}, bias from {-2 .. 2}: every D and U output is an integer of magnitude <= 218 (exact in bfloat16 too) and
    every W sum is far below 2^24, so whatever the summation order the kernels equal the float64 reference exactly."""
    (x, dy, w, b), ref = reference(shape, up, 3, True)
    assert ref[0].abs().max() <= 218 and ref[1].abs().max() <= 216 and ref[2].abs().max() < 2 ** 20 and ref[0].abs().max() > 8
    got = kernel(x, dy, w, b, up, dtype)
    for name, a, r in zip(NAMES, got, ref):
        assert torch.equal(a.double().cpu(), r), (name, shape, up, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", EXACT + [(2, 3, 5), (1, 9, 1)])
def test_down_and_up_are_adjoint(shape, dtype):
    """sum D(x, w) g == sum x U(g, w) with the SAME stored weight, exactly on the integer inputs (the products are summed in float64)."""
    from ppnet_amd import fused
    (x, g, w, _), _ = reference(shape, False, 3, True)
    xg, gg, wg = x.to(DEV).to(dtype), g.to(DEV).to(dtype), w.to(DEV)
    d = fused._s2_down(xg, wg, None)
    u = fused._s2_up(gg, wg, None, x.shape[2], x.shape[3])
    lhs, rhs = (d.double() * gg.double()).sum().item(), (xg.double() * u.double()).sum().item()
    assert lhs == rhs and bool((d != 0).any())


# ------------------------------------------------------------------------------------------------------------------------------ hygiene
def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


GUARD = 64                                                                     # elements on each side of every output


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _raw(big, small, w, b, dtype, fill, sums=(True, True)):
    """The three raw entry points on outputs and a workspace filled with `fill` and surrounded by it: (outputs, their buffers)."""
    from ppnet_amd import _lib as L
    B, _, H, W = big.shape
    Hs, Ws = small.shape[2], small.shape[3]
    need = L.lib.ppn_gennet_s2_wgrad_workspace(B, Hs, Ws)
    assert need > 0 and need % 4 == 0
    bufs = {"down": _guarded(small.numel(), dtype, fill), "up": _guarded(big.numel(), dtype, fill), "ws": _guarded(need // 4, F32, fill),
            "dw": _guarded(C * C * 9, F32, fill), "sum_small": _guarded(C, F32, fill), "sum_big": _guarded(C, F32, fill)}
    v = {k: t[1] for k, t in bufs.items()}
    bg, sg, wg, biasg = big.to(DEV).to(dtype), small.to(DEV).to(dtype), w.to(DEV), b.to(DEV)
    dt = 0 if dtype == F32 else 1
    assert L.lib.ppn_gennet_s2_down(_P(bg), _P(wg), _P(biasg), _P(v["down"]), B, H, W, C, dt, _stream()) == 0
    assert L.lib.ppn_gennet_s2_up(_P(sg), _P(wg), _P(biasg), _P(v["up"]), B, H, W, C, dt, _stream()) == 0
    assert L.lib.ppn_gennet_s2_wgrad(_P(sg), _P(bg), _P(v["ws"]), _P(v["dw"]), _P(v["sum_small"]) if sums[0] else None,
                                     _P(v["sum_big"]) if sums[1] else None, B, H, W, C, dt, _stream()) == 0
    torch.cuda.synchronize()
    return v, bufs


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 7, 8), (2, 33, 31), (1, 53, 38), LARGE])
def test_three_calls_agree_bitwise_and_stay_inside_their_buffers(shape, dtype):
    """Three calls on NaN-filled outputs and workspaces give the same bits (one writer per element, fixed-order sums: 1255 x 1256 has more
    tiles than workgroups), every output element is written, and the 64 elements on either side of the outputs, the workspace and the
    sums keep their fill.  sum_small / sum_big = NULL: the same dw bit for bit, the other sum too, and the unwanted buffer untouched."""
    B, H, W = shape
    g = torch.Generator().manual_seed(5)
    big = torch.randn(B, C, H, W, generator=g).to(BF16).float()
    small = torch.randn(B, C, _small(H), _small(W), generator=g).to(BF16).float()
    w, b = torch.randn(C, C, 3, 3, generator=g), torch.randn(C, generator=g)
    nan = float("nan")
    first = None
    for _ in range(3):
        v, bufs = _raw(big, small, w, b, dtype, nan)
        for k, (buf, view) in bufs.items():
            assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + view.numel():]).all()), k
            if k != "ws":
                assert bool(torch.isfinite(view).all()), k
        out = {k: t.clone() for k, t in v.items() if k != "ws"}
        if first is None:
            first = out
        assert all(torch.equal(out[k], first[k]) for k in first)
    v7, bufs7 = _raw(big, small, w, b, dtype, 7.0)                               # another fill: nothing read before it was written
    assert all(torch.equal(v7[k], first[k]) for k in first)
    assert all(bool((t[:GUARD] == 7).all()) and bool((t[GUARD + view.numel():] == 7).all()) for t, view in bufs7.values())
    for sums, idle in (((False, True), "sum_small"), ((True, False), "sum_big"), ((False, False), None)):
        vn, bufsn = _raw(big, small, w, b, dtype, 7.0, sums)
        for k, on in zip(("sum_small", "sum_big"), sums):
            assert bool((bufsn[k][0] == 7).all()) if not on else torch.equal(vn[k], first[k]), (k, idle)
        assert torch.equal(vn["dw"], first["dw"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("up", UP)
def test_the_autograd_function_returns_the_raw_calls_bits(up, dtype, monkeypatch):
    """conv_s2 under autograd gives the raw launches' bits; an x that needs no gradient gets none (and one launch fewer); a layer without
    bias gets no bias gradient; a float32 x under bfloat16 autocast runs in bfloat16 and gets a float32 dx."""
    from ppnet_amd import fused
    monkeypatch.delenv("PPNET_LIBRARY_S2", raising=False)
    monkeypatch.setattr(fused, "S2_RECORD_MIN", 0)                             # the shipped gates are measured ones: the test opens them
    monkeypatch.setattr(fused, "S2_DTYPES", frozenset(DTYPES))
    shape = (2, 7, 8)
    (x, dy, w, b), _ = reference(shape, up, SEED)
    raw = kernel(x, dy, w, b, up, dtype)
    conv = layer(up).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(w); conv.bias.copy_(b)
    xg = x.to(DEV).to(dtype).requires_grad_(True)
    calls = dict(fused.S2_CALLS)
    with torch.autocast("cuda", dtype=BF16, enabled=dtype == BF16):
        assert fused.conv_s2_ok(xg, conv)
        y = fused.conv_s2(xg, conv)
    grads = torch.autograd.grad(y, [xg, conv.weight, conv.bias], dy.to(DEV).to(dtype))
    assert fused.S2_CALLS == {k: calls[k] + 1 for k in calls}                  # forward, its adjoint for dx, and W
    assert torch.equal(y, raw[0]) and all(torch.equal(g, r) for g, r in zip(grads, raw[1:]))
    calls = dict(fused.S2_CALLS)
    with torch.autocast("cuda", dtype=BF16, enabled=dtype == BF16):
        y2 = fused.conv_s2(xg.detach(), conv)
    grads2 = torch.autograd.grad(y2, [conv.weight, conv.bias], dy.to(DEV).to(dtype))
    fwd = "up" if up else "down"
    assert fused.S2_CALLS == {k: calls[k] + (1 if k in (fwd, "wgrad") else 0) for k in calls}
    assert all(torch.equal(g, r) for g, r in zip(grads2, raw[2:]))
    nb = layer(up).to(DEV)
    nb.bias = None
    with torch.no_grad():
        nb.weight.copy_(w)
    with torch.autocast("cuda", dtype=BF16, enabled=dtype == BF16):
        y3 = fused.conv_s2(xg, nb)
    g3 = torch.autograd.grad(y3, [xg, nb.weight], dy.to(DEV).to(dtype))
    assert torch.equal(g3[0], raw[1]) and torch.equal(g3[1], raw[2])
    if dtype == BF16:
        xf = x.to(DEV).requires_grad_(True)                                    # bfloat16-exact float32 values: the cast loses nothing
        with torch.autocast("cuda", dtype=BF16):
            y4 = fused.conv_s2(xf, conv)
        g4 = torch.autograd.grad(y4, [xf], dy.to(DEV).to(BF16))[0]
        assert y4.dtype == BF16 and g4.dtype == F32 and torch.equal(y4, raw[0]) and torch.equal(g4, raw[1].float())
        assert not fused.conv_s2_ok(xg, conv)                                   # a bfloat16 x outside autocast keeps the library
        monkeypatch.setattr(fused, "S2_DTYPES", frozenset({F32}))
        with torch.autocast("cuda", dtype=BF16):
            assert not fused.conv_s2_ok(xf, conv) and not fused.conv_s2_ok(xg, conv)     # the data type gate reads the kernels' dtype
        assert fused.conv_s2_ok(xf, conv)
        monkeypatch.setattr(fused, "S2_RECORD_MIN", 4 * xf.numel() + 1)             # past the big side of either layer type
        assert not fused.conv_s2_ok(xf, conv)
        with torch.autocast("cuda", dtype=torch.float16):
            assert not fused.conv_s2_ok(xf, conv)


# ---------------------------------------------------------------------------------------------------------------------- the module
def _model(seed):
    from ppnet_amd.gennet import AEViT
    torch.manual_seed(seed)
    m = AEViT(1, 1, 112, 24).train()
    assert len(m.enc_conv) == 2 and len(m.dec_conv) == 2
    for blk in m.vit_blocks:
        blk.drop_path_rate = 0.0
    with torch.no_grad():                                                      # biases and norms off their neutral values
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    return m


def _grads(m, x, w, amp=None):
    m.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=BF16, enabled=amp is not None):
        out = m(x)
    (out.float() * w).sum().backward() if amp is not None else (out * w).sum().backward()
    return {n: (p.grad.detach().double().cpu() if p.grad is not None else None) for n, p in m.named_parameters()}


@pytest.mark.parametrize("amp", [None, BF16])
def test_aevit_parameter_gradients(amp, monkeypatch, capsys):
    """AEViT(1, 1, 112, 24) — two encoder and two decoder stages — in train mode without drop path, batch 2, one forward + backward: four
    launches of each kernel; every parameter gradient through the kernel stages and through the library stages (PPNET_LIBRARY_S2=1: same
    weights, same GPU) against the float64 CPU model by the rule; the knob leaves the counters alone and gives the gradients of a model
    with the three functions patched out (bit for bit, but for the library's own atomically summed weight gradients of the four stages);
    the stem's and the tail's kernels run as before."""
    from ppnet_amd import fused
    monkeypatch.delenv("PPNET_LIBRARY_S2", raising=False)
    monkeypatch.setattr(fused, "S2_RECORD_MIN", 0)
    monkeypatch.setattr(fused, "S2_DTYPES", frozenset(DTYPES))
    m = _model(4)
    g = torch.Generator().manual_seed(8)
    x0 = (torch.rand(2, 1, 112, 112, generator=g) > 0.5).float()
    w = torch.randn(2, 1, 112, 112, generator=g)
    m64 = copy.deepcopy(m).double()
    m64.zero_grad(set_to_none=True)
    (m64(x0.double()) * w.double()).sum().backward()
    ref = {n: p.grad.detach() for n, p in m64.named_parameters()}
    mg = copy.deepcopy(m).to(DEV)
    sd = {k: v.clone() for k, v in mg.state_dict().items()}
    fused.S2_CALLS.update(down=0, up=0, wgrad=0)
    stem, tail = dict(fused.STEM_CALLS), dict(fused.TAIL_CALLS)
    got = _grads(mg, x0.to(DEV), w.to(DEV), amp)
    torch.cuda.synchronize()
    assert fused.S2_CALLS == {"down": 4, "up": 4, "wgrad": 4}
    assert fused.STEM_CALLS == {k: v + 1 for k, v in stem.items()} and fused.TAIL_CALLS == {k: v + 1 for k, v in tail.items()}
    mg.load_state_dict(sd)
    monkeypatch.setenv("PPNET_LIBRARY_S2", "1")
    lib = _grads(mg, x0.to(DEV), w.to(DEV), amp)
    assert fused.S2_CALLS == {"down": 4, "up": 4, "wgrad": 4}                  # the knob is read at call time
    assert fused.STEM_CALLS == {k: v + 2 for k, v in stem.items()} and fused.TAIL_CALLS == {k: v + 2 for k, v in tail.items()}
    monkeypatch.delenv("PPNET_LIBRARY_S2")
    mg.load_state_dict(sd)

    def refuse(*a, **k):
        raise AssertionError("a stride-2 launcher ran")
    with monkeypatch.context() as mp:                                          # the parent's forward: conv(x), whatever the gate says
        for name in ("_s2_down", "_s2_up", "_s2_wgrad"):
            mp.setattr(fused, name, refuse)
        mp.setattr(fused, "conv_s2", lambda x, conv: conv(x))
        parent = _grads(mg, x0.to(DEV), w.to(DEV), amp)
    # The library's own weight gradient of these convolutions adds with atomics: two identical library runs differ in exactly those four
    # tensors (measured 2.5e-7 .. 4.2e-7 x max in float32, up to 2.1e-5 under bfloat16 autocast) and in nothing else.  So: bit equality
    # everywhere else, and the data type's floor — the reordering of a float32 / bfloat16 sum — on the four.
    assert set(parent) == set(lib)
    stage_w = {f"{part}.{i}.0.weight" for part in ("enc_conv", "dec_conv") for i in range(2)}
    for n in lib:
        if n in stage_w:
            diff = (parent[n] - lib[n]).abs().max().item() / lib[n].abs().max().item()
            with capsys.disabled():
                print(f"\nknob vs patched-out {n}: {diff:.2e} x max")
            assert diff <= FLOOR[amp or F32], (n, diff)
        else:
            assert torch.equal(parent[n], lib[n]), n
    assert all(v is not None for v in got.values()) and set(got) == set(ref) == set(lib)
    for n, p in mg.named_parameters():
        if n.endswith(".0.bias"):
            assert p.grad is not None and p.grad.shape == p.shape, n           # every convolution bias has a gradient tensor
    # a convolution bias ahead of a train-mode BatchNorm has gradient 0 in exact arithmetic (float64 leaves rounding): bounded in
    # absolute terms by the floor against the model's largest gradient, as tests/test_gpu_tail_train.py does
    floor = FLOOR[amp or F32]
    gmax = max(r.abs().max().item() for r in ref.values())
    worst = (0.0, 0.0, None)
    for n, r in ref.items():
        top = r.abs().max().item()
        if top < 1e-12 * gmax:
            assert n.endswith(".0.bias") and got[n].abs().max().item() / gmax <= max(2.0 * lib[n].abs().max().item() / gmax, floor), n
            continue
        ek, el = (got[n] - r).abs().max().item() / top, (lib[n] - r).abs().max().item() / top
        worst = max(worst, (ek, el, n))
        assert ek <= max(2.0 * el, floor), (n, ek, el)
    with capsys.disabled():
        print(f"\nAEViT R 112 {'bfloat16 autocast' if amp else 'float32'} kernel stages: worst gradient error {worst[0]:.2e} x max "
              f"(library stages {worst[1]:.2e}) at {worst[2]}")


@pytest.mark.parametrize("amp", [None, BF16])
def test_gennet_training_steps_use_the_stage_kernels(amp, monkeypatch):
    """Three gennet_train_steps at R 112, batch 2, on a fixed batch: four launches of each kernel per step, every parameter gets a finite
    gradient, and the loss falls."""
    from ppnet_amd import fused, train
    from ppnet_amd.gennet import AEViT
    monkeypatch.delenv("PPNET_LIBRARY_S2", raising=False)
    monkeypatch.setattr(fused, "S2_RECORD_MIN", 0)
    monkeypatch.setattr(fused, "S2_DTYPES", frozenset(DTYPES))
    torch.manual_seed(0)
    net = AEViT(1, 1, img_resolution=112, dim=24).cuda()
    opt = train.gennet_optimizer(net)
    g = torch.Generator().manual_seed(3)
    space = (torch.rand(2, 112, 112, generator=g) > 0.5).to(torch.uint8).to(DEV)          # {0, 1} and {0, 255}, as the generator's pairs
    path = ((torch.rand(2, 112, 112, generator=g) > 0.9).to(torch.uint8) * 255).to(DEV)
    fused.S2_CALLS.update(down=0, up=0, wgrad=0)
    losses = []
    for it in range(3):
        losses.append(float(train.gennet_train_step(net, opt, None, space, path, amp_dtype=amp)))
        assert fused.S2_CALLS == {"down": 4 * (it + 1), "up": 4 * (it + 1), "wgrad": 4 * (it + 1)}
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    assert all(l == l for l in losses) and losses[-1] < losses[0], losses
