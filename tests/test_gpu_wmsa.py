"""ppn_wmsa_fwd (csrc/wmsa_gen.hip) on the GPU: the window-attention kernel for window 14 with head dims 8 / 16 / 32 and window 7
with head dims 8 / 16 against the float64 torch composition (ppnet_amd.swin.window_attention on the CPU, itself equal to the
reference's SwinTransformerBlock attention branch).  Bounds are the Swin suite's (tests/test_gpu_swin.py): float32 within 2e-5,
bfloat16 within 3e-2, times max(1, max|want|) where values are large.  Grids that are and are not multiples of the window (also
smaller than it, and one window with four mask regions), both shifts, logits of 60..90 where the -100 mask (not -inf) decides,
one-hot and constant rows, a large pad_kv, no writes outside the real tokens, (7, 32) bit-equal to ppn_swin_wmsa_fwd, and the
dispatch counters."""
import ctypes

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [(torch.float32, 2e-5), (torch.bfloat16, 3e-2)]


def _ref(qkv, pad_kv, rpb_hw, heads, shift, scale, window, mask_value=-100.0):
    from ppnet_amd.swin import window_attention
    table = rpb_hw.double().reshape(heads, (2 * window - 1) ** 2).t()
    return window_attention(qkv.double().cpu(), pad_kv.double().cpu(), table.cpu(), heads, shift, scale, window=window, mask_value=mask_value)


def _run(qkv, pad_kv, rpb_hw, heads, shift, scale, window):
    from ppnet_amd.swin import wmsa_forward
    with torch.no_grad():
        out = wmsa_forward(qkv.to(DEV), pad_kv.to(DEV), rpb_hw.to(DEV), heads, shift, scale, window)
    torch.cuda.synchronize()
    return out


def _inputs(B, H, W, heads, d, window, seed, dtype, pad_scale=0.3):
    g = torch.Generator().manual_seed(seed)
    C = heads * d
    qkv = torch.randn(B, H, W, 3, C, generator=g)
    pad = torch.randn(3, C, generator=g) * pad_scale
    rpb = torch.randn(heads, 2 * window - 1, 2 * window - 1, generator=g) * 0.5
    return qkv.reshape(B, H, W, 3 * C).to(dtype), pad.reshape(-1).to(dtype), rpb


# (B, H, W, heads, shift).  Window 14: one unshifted window; one window with four mask regions; a grid smaller than the window;
# Hp = 28, Wp = 42: six windows with every region combination; four whole windows, both shifts; AESwin's middle stage at R = 256
# (head dim 8 only); a padded unshifted grid.
CASES14 = [(1, 14, 14, 1, 0), (1, 14, 14, 2, 7), (1, 2, 3, 3, 7), (2, 15, 29, 3, 7), (1, 28, 28, 2, 0), (1, 28, 28, 2, 7), (3, 16, 16, 24, 7),
           (2, 16, 20, 4, 0)]
CASES7 = [(1, 7, 7, 1, 0), (2, 9, 16, 2, 3), (1, 2, 3, 4, 3), (2, 15, 23, 5, 3)]
SWEEP = ([(14, d) + c for d in (8, 16, 32) for c in CASES14 if c[3] != 24 or d == 8] + [(7, d) + c for d in (8, 16) for c in CASES7])


@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("window,d,B,H,W,heads,shift", SWEEP)
def test_kernel_vs_float64(dtype, tol, window, d, B, H, W, heads, shift):
    qkv, pad, rpb = _inputs(B, H, W, heads, d, window, 1000 * window + 100 * H + W + heads + shift + d, dtype)
    scale = d ** -0.5
    got = _run(qkv, pad, rpb, heads, shift, scale, window).double().cpu()
    want = _ref(qkv, pad, rpb, heads, shift, scale, window)
    assert got.shape == want.shape
    err = (got - want).abs().max().item()
    assert err < tol, (window, d, B, H, W, heads, shift, err)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_window7_head32_is_the_swin_kernel_bit_for_bit(dtype):
    from ppnet_amd import _lib as L
    B, H, W, heads, shift = 2, 9, 16, 2, 3
    qkv, pad, rpb = _inputs(B, H, W, heads, 32, 7, 5, dtype)
    q, p, r = qkv.to(DEV).contiguous(), pad.to(DEV).contiguous(), rpb.to(DEV).float().contiguous()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dt = 0 if dtype == torch.float32 else 1
    a = torch.full((B, H, W, heads * 32), 7.0, dtype=dtype, device=DEV)
    b = torch.full((B, H, W, heads * 32), 9.0, dtype=dtype, device=DEV)
    assert L.lib.ppn_wmsa_fwd(P(q), P(p), P(r), P(a), B, H, W, heads, 32, 7, shift, float(32 ** -0.5), dt, s) == 0
    assert L.lib.ppn_swin_wmsa_fwd(P(q), P(p), P(r), P(b), B, H, W, heads, 7, shift, float(32 ** -0.5), dt, s) == 0
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def large_logit_inputs(dtype, d=16):
    """(1, 14, 17), 2 heads, window 14, shift 7: q = -k = a * s(token) * u + noise with s = +-1 by region parity, so that pairs of
    DIFFERENT regions get the large positive logits (60..90) and the -100 of the mask decides the output."""
    B, H, W, heads, shift, window = 1, 14, 17, 2, 7, 14
    g = torch.Generator().manual_seed(7)
    C = heads * d
    u = torch.randn(d, generator=g)
    u = u / u.norm()
    Hp, Wp = 14, 28
    lab = lambda y, n: 0 if (y - shift) % n < n - window else (1 if (y - shift) % n < n - shift else 2)
    sgn = torch.tensor([[(-1.0) ** (lab(i, Hp) + lab(j, Wp)) for j in range(W)] for i in range(H)])
    scale = d ** -0.5
    a = (80.0 / scale) ** 0.5
    qkv = torch.randn(B, H, W, 3, heads, d, generator=g) * 0.05
    qkv[..., 0, :, :] += a * sgn[None, :, :, None, None] * u
    qkv[..., 1, :, :] -= a * sgn[None, :, :, None, None] * u
    qkv[..., 2, :, :] = torch.randn(B, H, W, heads, d, generator=g)
    qkv = qkv.reshape(B, H, W, 3 * C).to(dtype)
    pad = torch.zeros(3 * C).to(dtype)
    rpb = torch.randn(heads, 27, 27, generator=g) * 0.5
    return qkv, pad, rpb, heads, shift, scale, window, d, C


@pytest.mark.parametrize("dtype,tol", DTYPES)
def test_kernel_large_logits_mask_is_minus_100(dtype, tol):
    """Logits of 60..90 with the shift's region mask: the result is the -100 one and measurably not the -inf one."""
    qkv, pad, rpb, heads, shift, scale, window, d, C = large_logit_inputs(dtype)
    lg = torch.einsum("bhwd,bxyd->bhwxy", qkv.double()[..., :d] * scale, qkv.double()[..., C:C + d])     # every pair of tokens, head 0
    assert 60 <= lg.max() <= 90
    want = _ref(qkv, pad, rpb, heads, shift, scale, window)
    winf = _ref(qkv, pad, rpb, heads, shift, scale, window, mask_value=float("-inf"))
    assert (want - winf).abs().max() > 0.5
    got = _run(qkv, pad, rpb, heads, shift, scale, window).double().cpu()
    assert (got - want).abs().max() < tol


@pytest.mark.parametrize("dtype,tol", DTYPES)
def test_kernel_one_hot_and_constant_rows(dtype, tol):
    B, H, W, heads, d, window = 2, 15, 18, 2, 8, 14
    C = heads * d
    g = torch.Generator().manual_seed(3)
    for shift in (0, 7):
        qkv = torch.zeros(B, H, W, 3, C)
        qkv[..., 0, :] = 0.7                                             # constant q and k: every key alike but for the bias
        qkv[..., 1, :] = -0.3
        idx = torch.randint(0, C, (B, H, W), generator=g)
        qkv[..., 2, :] = torch.nn.functional.one_hot(idx, C).float() * 2.0   # one-hot values
        qkv = qkv.reshape(B, H, W, 3 * C).to(dtype)
        pad = torch.randn(3 * C, generator=g).to(dtype)
        rpb = torch.randn(heads, 27, 27, generator=g)
        for r in (rpb, torch.zeros_like(rpb)):                            # zero bias: uniform attention over each window
            got = _run(qkv, pad, r, heads, shift, 0.2, window).double().cpu()
            assert (got - _ref(qkv, pad, r, heads, shift, 0.2, window)).abs().max() < tol


@pytest.mark.parametrize("dtype,tol", DTYPES)
def test_kernel_large_pad_kv_and_no_writes_outside(dtype, tol):
    """Padded keys carry pad_kv (large here, so a wrong one shows); out is written on the real tokens only: a sentinel-filled buffer
    longer than the output keeps its tail."""
    from ppnet_amd import _lib as L
    B, H, W, heads, shift, d, window = 2, 9, 11, 3, 7, 16, 14
    C = heads * d
    qkv, pad, rpb = _inputs(B, H, W, heads, d, window, 11, dtype, pad_scale=3.0)
    n = B * H * W * C
    buf = torch.full((n + 4096,), 12345.0, dtype=dtype, device=DEV)
    q, p, r = qkv.to(DEV).contiguous(), pad.to(DEV).contiguous(), rpb.to(DEV).float().contiguous()
    rc = L.lib.ppn_wmsa_fwd(ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(p.data_ptr()), ctypes.c_void_p(r.data_ptr()),
                            ctypes.c_void_p(buf.data_ptr()), B, H, W, heads, d, window, shift, float(d ** -0.5), 0 if dtype == torch.float32 else 1,
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((buf[n:] == 12345.0).all())
    got = buf[:n].view(B, H, W, C).double().cpu()
    want = _ref(qkv, pad, rpb, heads, shift, d ** -0.5, window)
    assert (got - want).abs().max() < tol * max(1.0, want.abs().max().item())     # bf16's rounding scales with the outputs
    wrong = _ref(qkv, torch.zeros_like(pad), rpb, heads, shift, d ** -0.5, window)
    assert (want - wrong).abs().max() > tol * max(1.0, want.abs().max().item())   # the case sees pad_kv


def test_dispatch_counting(monkeypatch):
    """swin.CALLS counts the launches; with PPNET_LIBRARY_WMSA=1 (read at call time) the same call through AESwin's attention module
    takes the torch composition."""
    from ppnet_amd import swin
    from ppnet_amd.gennet import _WindowAttention
    torch.manual_seed(0)
    attn = _WindowAttention(48, 14, 3, 7).to(DEV).eval()                  # head dim 16
    x = torch.randn(2, 15, 18, 48, device=DEV)
    monkeypatch.delenv("PPNET_LIBRARY_WMSA", raising=False)
    with torch.no_grad():
        swin.CALLS.update(kernel=0, torch=0)
        a = attn(x)
        assert swin.CALLS == {"kernel": 1, "torch": 0}
        monkeypatch.setenv("PPNET_LIBRARY_WMSA", "1")
        b = attn(x)
        assert swin.CALLS == {"kernel": 1, "torch": 1}
    torch.cuda.synchronize()
    assert (a - b).abs().max().item() < 2e-5 * max(1.0, b.abs().max().item())
    monkeypatch.delenv("PPNET_LIBRARY_WMSA")
    y = attn(x.requires_grad_())                                          # autograd records: the composition, differentiable
    assert swin.CALLS == {"kernel": 1, "torch": 2} and y.requires_grad
