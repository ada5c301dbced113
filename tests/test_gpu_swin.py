"""ppn_swin_wmsa_fwd (csrc/swin_wmsa.hip) and the Swin backbone / SegNet on the GPU.

Kernel against the float64 torch composition of mmseg's op chain (ppnet_amd.swin.window_attention, itself pinned to the reference
by tests/test_swin_golden.py): float32 within 2e-5, bfloat16 within 3e-2 (the neighbourhood-attention suite's bounds), on grids that
are and are not multiples of the window (also smaller than it), shift 0 / 3, 1-32 heads, batch 1-3, logits of +-60..90 where the
-100 mask (not -inf) decides, one-hot and constant rows, a large pad_kv, no writes outside the real tokens, and argument checks."""
import copy
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ref(qkv, pad_kv, rpb_hw, heads, shift, scale, mask_value=-100.0):
    from ppnet_amd.swin import window_attention
    table = rpb_hw.double().reshape(heads, 169).t()
    return window_attention(qkv.double().cpu(), pad_kv.double().cpu(), table.cpu(), heads, shift, scale, mask_value=mask_value)


def _run(qkv, pad_kv, rpb_hw, heads, shift, scale):
    from ppnet_amd.swin import wmsa_forward
    with torch.no_grad():
        out = wmsa_forward(qkv.to(DEV), pad_kv.to(DEV), rpb_hw.to(DEV), heads, shift, scale)
    torch.cuda.synchronize()
    return out


def _inputs(B, H, W, heads, seed, dtype, qk=1.0, pad_scale=0.3):
    g = torch.Generator().manual_seed(seed)
    C = heads * 32
    qkv = torch.randn(B, H, W, 3, C, generator=g)
    qkv[..., :2, :] *= qk
    pad = torch.randn(3, C, generator=g) * pad_scale
    rpb = torch.randn(heads, 13, 13, generator=g) * 0.5
    return qkv.reshape(B, H, W, 3 * C).to(dtype), pad.reshape(-1).to(dtype), rpb


CASES = [(1, 7, 7, 1, 0), (1, 7, 7, 2, 3), (2, 14, 21, 2, 3), (1, 2, 3, 4, 3), (3, 4, 6, 3, 0), (1, 4, 6, 2, 3), (1, 8, 8, 32, 3),
         (2, 15, 23, 5, 3), (1, 28, 28, 4, 0), (2, 9, 16, 8, 3), (1, 64, 64, 4, 3), (3, 8, 8, 16, 0)]


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.bfloat16, 3e-2)])
@pytest.mark.parametrize("B,H,W,heads,shift", CASES)
def test_kernel_vs_float64(dtype, tol, B, H, W, heads, shift):
    qkv, pad, rpb = _inputs(B, H, W, heads, 100 * H + W + heads + shift, dtype)
    scale = 32 ** -0.5
    got = _run(qkv, pad, rpb, heads, shift, scale).double().cpu()
    want = _ref(qkv, pad, rpb, heads, shift, scale)
    assert got.shape == want.shape
    err = (got - want).abs().max().item()
    assert err < tol, (B, H, W, heads, shift, err)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.bfloat16, 3e-2)])
def test_kernel_large_logits_mask_is_minus_100(dtype, tol):
    """Logits of +-60..90 with the shift's region mask: the result is the -100 one and measurably not the -inf one."""
    B, H, W, heads, shift = 1, 14, 17, 2, 3
    g = torch.Generator().manual_seed(7)
    C = heads * 32
    # q = k = a * s(token) * u + noise, s = +-1 by region parity: pairs of different regions get the LARGE logits
    u = torch.randn(32, generator=g)
    u = u / u.norm()
    Hp, Wp = 14, 21
    lab = lambda y, n: 0 if (y - shift) % n < n - 7 else (1 if (y - shift) % n < n - shift else 2)
    sgn = torch.tensor([[(-1.0) ** (lab(i, Hp) + lab(j, Wp)) for j in range(W)] for i in range(H)])
    a = (80.0 / 32 ** -0.5) ** 0.5
    qkv = torch.randn(B, H, W, 3, heads, 32, generator=g) * 0.05
    qkv[..., 0, :, :] += a * sgn[None, :, :, None, None] * u
    qkv[..., 1, :, :] -= a * sgn[None, :, :, None, None] * u
    qkv[..., 2, :, :] = torch.randn(B, H, W, heads, 32, generator=g)
    qkv = qkv.reshape(B, H, W, 3 * C).to(dtype)
    pad = torch.zeros(3 * C).to(dtype)
    rpb = torch.randn(heads, 13, 13, generator=g) * 0.5
    scale = 32 ** -0.5
    lg = (qkv.double()[..., :32] * scale * qkv.double()[..., C:C + 32]).sum(-1)
    assert 60 <= lg.abs().max() <= 90
    want = _ref(qkv, pad, rpb, heads, shift, scale)
    winf = _ref(qkv, pad, rpb, heads, shift, scale, mask_value=float("-inf"))
    assert (want - winf).abs().max() > 0.5
    got = _run(qkv, pad, rpb, heads, shift, scale).double().cpu()
    assert (got - want).abs().max() < tol


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.bfloat16, 3e-2)])
def test_kernel_one_hot_and_constant_rows(dtype, tol):
    B, H, W, heads = 2, 10, 12, 2
    C = heads * 32
    g = torch.Generator().manual_seed(3)
    for shift in (0, 3):
        qkv = torch.zeros(B, H, W, 3, C)
        qkv[..., 0, :] = 0.7                                             # constant q and k: every key alike but for the bias
        qkv[..., 1, :] = -0.3
        idx = torch.randint(0, C, (B, H, W), generator=g)
        qkv[..., 2, :] = torch.nn.functional.one_hot(idx, C).float() * 2.0   # one-hot values
        qkv = qkv.reshape(B, H, W, 3 * C).to(dtype)
        pad = torch.randn(3 * C, generator=g).to(dtype)
        rpb = torch.randn(heads, 13, 13, generator=g)
        for r in (rpb, torch.zeros_like(rpb)):                            # zero bias: uniform attention over each window
            got = _run(qkv, pad, r, heads, shift, 0.2).double().cpu()
            assert (got - _ref(qkv, pad, r, heads, shift, 0.2)).abs().max() < tol


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.bfloat16, 3e-2)])
def test_kernel_large_pad_kv_and_no_writes_outside(dtype, tol):
    """Padded keys carry pad_kv (large here, so a wrong one shows); out is written on the real tokens only: a sentinel-filled
    buffer longer than the output keeps its tail."""
    from ppnet_amd import _lib as L
    B, H, W, heads, shift = 2, 9, 11, 3, 3
    C = heads * 32
    qkv, pad, rpb = _inputs(B, H, W, heads, 11, dtype, pad_scale=3.0)
    n = B * H * W * C
    buf = torch.full((n + 4096,), 12345.0, dtype=dtype, device=DEV)
    q, p, r = qkv.to(DEV).contiguous(), pad.to(DEV).contiguous(), rpb.to(DEV).float().contiguous()
    rc = L.lib.ppn_swin_wmsa_fwd(ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(p.data_ptr()), ctypes.c_void_p(r.data_ptr()),
                                 ctypes.c_void_p(buf.data_ptr()), B, H, W, heads, 7, shift, float(32 ** -0.5), 0 if dtype == torch.float32 else 1,
                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((buf[n:] == 12345.0).all())
    got = buf[:n].view(B, H, W, C).double().cpu()
    want = _ref(qkv, pad, rpb, heads, shift, 32 ** -0.5)
    assert (got - want).abs().max() < tol * max(1.0, want.abs().max().item())     # outputs up to ~8 here: bf16's rounding scales
    wrong = _ref(qkv, torch.zeros_like(pad), rpb, heads, shift, 32 ** -0.5)
    assert (want - wrong).abs().max() > 0.1                               # the case sees pad_kv


def test_kernel_argument_validation():
    from ppnet_amd import _lib as L
    q = torch.zeros(1, 7, 7, 96, device=DEV)
    p = torch.zeros(96, device=DEV)
    r = torch.zeros(1, 13, 13, device=DEV)
    o = torch.zeros(1, 7, 7, 32, device=DEV)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    f = L.lib.ppn_swin_wmsa_fwd
    ok = (P(q), P(p), P(r), P(o), 1, 7, 7, 1, 7, 0, 0.1, 0, s)

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    E_INVALID, E_UNSUPPORTED = -1, -3
    assert call(a0=None) == E_INVALID and call(a1=None) == E_INVALID and call(a2=None) == E_INVALID and call(a3=None) == E_INVALID
    assert call(a4=0) == E_INVALID and call(a5=0) == E_INVALID and call(a6=-1) == E_INVALID and call(a7=0) == E_INVALID
    assert call(a11=2) == E_INVALID and call(a10=0.0) == E_INVALID and call(a9=-1) == E_INVALID and call(a9=7) == E_INVALID
    assert call(a8=8, a9=0) == E_UNSUPPORTED and call(a9=2) == E_UNSUPPORTED
    assert call(a0=ctypes.c_void_p(q.data_ptr() + 4)) == E_INVALID        # 16-byte alignment
    assert call(a4=1 << 30, a5=1 << 10, a6=1 << 10) == E_INVALID          # B * windows >= 2^31: refused before any launch
    assert call() == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ backbone vs the reference
@pytest.fixture(scope="module")
def g18(golden_dir):
    return np.load(os.path.join(golden_dir, "g18_swin.npz"))


@pytest.mark.parametrize("case", ["a", "b"])
def test_backbone_gpu_vs_reference(g18, case, capsys):
    from ppnet_amd import swin
    from tests.test_swin_golden import load_net
    m, _ = load_net(g18, torch.float32)
    m = m.to(DEV)
    from tests._swin_golden import image
    x = torch.from_numpy(image(case)).to(DEV)
    swin.CALLS.update(kernel=0, torch=0)
    with torch.no_grad():
        outs = m(x)
        mb = copy.deepcopy(m).to(torch.bfloat16)
        outs16 = mb(x.to(torch.bfloat16))
    assert swin.CALLS["torch"] == 0 and swin.CALLS["kernel"] == 16
    for i, (o, o16) in enumerate(zip(outs, outs16)):
        want = g18[f"{case}/y{i}"]
        ref = np.abs(want).max()
        err = np.abs(o.double().cpu().numpy() - want).max()
        err16 = np.abs(o16.double().cpu().numpy() - want).max()
        with capsys.disabled():
            print(f"\nswin backbone case {case} level {i}: fp32 max err {err / ref:.2e} x max|ref|, bf16 {err16 / ref:.2e} x max|ref|")
        assert err < 5e-6 * ref, (case, i, err)                          # measured <= 8.2e-7 x max|ref|
        assert err16 < 4e-2 * ref, (case, i, err16)                      # measured <= 1.4e-2 x max|ref|


# ------------------------------------------------------------------------------------------------ SegNet with Swin-B
def _codes(B, R, seed):
    g = torch.Generator().manual_seed(seed)
    lo = (torch.rand(B, 1, R // 16, R // 16, generator=g) > 0.4).float()
    return (torch.nn.functional.interpolate(lo, size=(R, R), mode="nearest")[:, 0] * 255).to(torch.uint8)


@pytest.mark.parametrize("name", ["SWIN_BASE_UPER", "SWIN_BASE_SETRUP"])
def test_segnet_swin_base_bf16_vs_fp32(name, capsys):
    from ppnet_amd import fused, segnet, swin
    cfg = getattr(segnet, name)
    torch.manual_seed(0)
    m32 = segnet.randomize_neutral_parameters(segnet.SegNet.from_config(cfg), seed=1).eval().to(DEV)
    codes = _codes(4, 256, 5).to(DEV)
    with torch.no_grad():
        segnet.balance_classifier_bias(m32, fused.grid_to_image(codes, segnet.IMG_MEAN, segnet.IMG_STD, torch.float32))
    m16 = copy.deepcopy(m32).to(torch.bfloat16)
    m32.prepare_inference()
    m16.prepare_inference()
    with torch.no_grad():
        l32 = m32.labels_u8(codes)
        swin.CALLS.update(kernel=0, torch=0)
        l16 = m16.labels_u8(codes)
        calls = dict(swin.CALLS)
        res = m16.simple_test(codes, [{"ori_shape": (256, 256, 3)}] * 4)
    torch.cuda.synchronize()
    assert calls == {"kernel": 24, "torch": 0}                          # every block's attention on ppn_swin_wmsa_fwd
    assert len(res) == 4 and res[0].shape == (256, 256)
    assert np.array_equal(np.stack(res), l16.cpu().numpy().astype(np.int64))
    agree = (l32 == l16).float().mean().item()
    frac1 = l32.float().mean().item()
    with capsys.disabled():
        print(f"\n{name}: bf16 vs fp32 label agreement {agree:.5f} (class-1 fraction {frac1:.3f})")
    assert 0.05 < frac1 < 0.95
    assert agree > 0.98, agree                                          # measured 0.9937 (UPerHead), 0.9896 (SETR-UP)
