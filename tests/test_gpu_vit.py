"""ppn_mhsa_fwd (csrc/mhsa.hip) and the ViT backbone / SegNet on the GPU.

Kernel against a float64 torch reference of softmax(scale q k^T) v per (batch, head): float32 within 2e-6 x max|ref|, bfloat16 (on
bfloat16-rounded inputs) within 1e-2 x max|ref|, for N from 1 to 4096 (tails of the 64-key tiles and 128-query blocks included);
logits of +-60..90, one-hot and constant rows, N = 1, large finite garbage just past row N and no writes outside `out`.  The fp32
backbone against the reference golden g20, and ViT-B + SETR-UP prepared bfloat16 against float32."""
import copy
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ref(qkv, heads, scale):
    """float64 [B,N,heads*64] from qkv [B,N,3*heads*64]."""
    B, N, _ = qkv.shape
    t = qkv.double().cpu().view(B, N, 3, heads, 64).permute(2, 0, 3, 1, 4)        # [3, B, heads, N, 64]
    p = torch.softmax((t[0] @ t[1].transpose(-1, -2)) * scale, dim=-1)
    return (p @ t[2]).permute(0, 2, 1, 3).reshape(B, N, heads * 64)


def _run(qkv, heads, scale):
    from ppnet_amd.vit import mhsa_forward
    with torch.no_grad():
        out = mhsa_forward(qkv.to(DEV), heads, scale)
    torch.cuda.synchronize()
    return out


SHAPES = [(1, 1, 1), (2, 7, 2), (3, 64, 12), (2, 196, 12), (2, 197, 12), (1, 256, 12), (2, 257, 3), (1, 1024, 12), (1, 1025, 2),
          (1, 4096, 1)]


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-6), (torch.bfloat16, 1e-2)])
@pytest.mark.parametrize("B,N,heads", SHAPES)
def test_kernel_vs_float64(dtype, tol, B, N, heads, capsys):
    g = torch.Generator().manual_seed(1000 * N + 10 * heads + B)
    qkv = torch.randn(B, N, 3 * heads * 64, generator=g).to(dtype)          # bf16: the reference sees the rounded inputs
    scale = 64 ** -0.5
    got = _run(qkv, heads, scale).double().cpu()
    want = _ref(qkv, heads, scale)
    assert got.shape == want.shape
    err = (got - want).abs().max().item() / want.abs().max().item()
    with capsys.disabled():
        print(f"\nmhsa {str(dtype)[6:]} B {B} N {N} heads {heads}: max err {err:.2e} x max|ref|")
    assert err <= tol, (B, N, heads, err)                                 # measured: see DESIGN.md section 11


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.bfloat16, 1e-2)])
def test_kernel_large_logits(dtype, tol):
    """Logits of +-60..90: a wrong running maximum or rescale overflows or loses the winners.  (float32: a logit of 80 carries
    float32 rounding of ~80 * 2^-24 * 8 from its 64-term dot product alone, so the bound is 1e-5 here; measured 2.6e-6.)"""
    B, N, heads = 2, 300, 3
    g = torch.Generator().manual_seed(5)
    u = torch.randn(B, N, heads, 64, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    s = torch.sign(torch.randn(B, N, heads, 1, generator=g))
    a = (70.0 / 64 ** -0.5) ** 0.5
    q = a * u + 0.05 * torch.randn(B, N, heads, 64, generator=g)
    k = a * s * u[:, torch.randperm(N, generator=g)] + 0.05 * torch.randn(B, N, heads, 64, generator=g)
    k[:, :, :, :] = k + a * s * 0.3 * u                                       # every query has a few strongly matching keys
    v = torch.randn(B, N, heads, 64, generator=g)
    qkv = torch.stack([q, k, v], 2).reshape(B, N, 3 * heads * 64).to(dtype)
    scale = 64 ** -0.5
    lg = _logits(qkv, heads, scale)
    assert 60.0 <= lg.abs().max().item() <= 90.0, lg.abs().max().item()
    got = _run(qkv, heads, scale).double().cpu()
    assert torch.isfinite(got).all()
    want = _ref(qkv, heads, scale)
    assert (got - want).abs().max().item() <= tol * want.abs().max().item()


def _logits(qkv, heads, scale):
    B, N, _ = qkv.shape
    t = qkv.double().view(B, N, 3, heads, 64)
    return torch.einsum("bnhd,bmhd->bhnm", t[:, :, 0], t[:, :, 1]) * scale


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_kernel_one_hot_constant_and_single_key(dtype):
    B, heads = 2, 2
    g = torch.Generator().manual_seed(9)
    scale = 64 ** -0.5
    # one-hot rows: N = 60 keys, query n's logit is +50 with key perm[n] and 0 with every other one -> v[perm[n]]
    N = 60
    perm = torch.randperm(N, generator=g)
    q = torch.zeros(B, N, heads, 64)
    k = torch.zeros(B, N, heads, 64)
    q[:, torch.arange(N), :, torch.arange(N)] = 50.0 / scale
    k[:, perm, :, torch.arange(N)] = 1.0
    v = torch.randn(B, N, heads, 64, generator=g)
    qkv = torch.stack([q, k, v], 2).reshape(B, N, 3 * heads * 64).to(dtype)
    got = _run(qkv, heads, scale).double().cpu().view(B, N, heads, 64)
    vr = qkv.double().view(B, N, 3, heads, 64)[:, :, 2]
    want = vr[:, perm]
    step = 2.0 ** -7 if dtype == torch.bfloat16 else 1e-6                  # one bfloat16 step of the largest |v|
    assert (got - want).abs().max().item() <= step * vr.abs().max().item()
    # constant rows: every logit equal -> the mean of v over all N keys (N past one key tile and one query block)
    N = 300
    v = torch.randn(B, N, heads, 64, generator=g)
    qc = torch.full((B, N, heads, 64), 0.3)
    qkv = torch.stack([qc, qc, v], 2).reshape(B, N, 3 * heads * 64).to(dtype)
    got = _run(qkv, heads, scale).double().cpu().view(B, N, heads, 64)
    mean = qkv.double().view(B, N, 3, heads, 64)[:, :, 2].mean(dim=1, keepdim=True).expand(B, N, heads, 64)
    assert (got - mean).abs().max().item() <= (1e-2 if dtype == torch.bfloat16 else 2e-6) * mean.abs().max().item()
    # N = 1: the one value row
    qkv1 = torch.randn(3, 1, 3 * heads * 64, generator=g).to(dtype)
    got = _run(qkv1, heads, scale).double().cpu()
    want = qkv1.double()[:, :, 2 * heads * 64:]
    assert (got - want).abs().max().item() <= (2.0 ** -8 if dtype == torch.bfloat16 else 1e-7) * want.abs().max().item()


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-6), (torch.bfloat16, 1e-2)])
def test_kernel_reads_and_writes_only_its_rows(dtype, tol):
    """Large finite garbage in the rows just past row N of a padded qkv buffer must not reach the softmax (tail keys), and a
    sentinel-filled out buffer longer than [B,N,C] keeps its tail (tail queries are not stored)."""
    from ppnet_amd import _lib as L
    B, N, heads = 1, 197, 2
    C = heads * 64
    g = torch.Generator().manual_seed(13)
    qkv = torch.randn(B, N, 3 * C, generator=g).to(dtype)
    buf = torch.full((N + 130, 3 * C), 3.0e4, dtype=dtype)                  # rows N .. N + 129: garbage (exp(huge) if read)
    buf[:N] = qkv[0]
    q = buf.to(DEV).contiguous()
    n = B * N * C
    out = torch.full((n + 8192,), 12345.0, dtype=dtype, device=DEV)
    rc = L.lib.ppn_mhsa_fwd(ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(out.data_ptr()), B, N, heads, 64, float(64 ** -0.5),
                            0 if dtype == torch.float32 else 1, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((out[n:] == 12345.0).all())
    got = out[:n].view(B, N, C).double().cpu()
    want = _ref(qkv, heads, 64 ** -0.5)
    assert torch.isfinite(got).all()
    assert (got - want).abs().max().item() <= tol * want.abs().max().item()


def test_kernel_rejects_bad_arguments_on_gpu_buffers():
    from ppnet_amd import _lib as L
    q = torch.zeros(1, 8, 3 * 64, device=DEV)
    o = torch.zeros(1, 8, 64, device=DEV)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    f = L.lib.ppn_mhsa_fwd
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    assert f(P(q), P(o), 1, 8, 1, 32, 0.125, 0, s) == -3
    assert f(ctypes.c_void_p(q.data_ptr() + 4), P(o), 1, 8, 1, 64, 0.125, 0, s) == -1
    assert f(P(q), P(o), 1, 8, 1, 64, 0.125, 0, s) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ backbone vs the reference
@pytest.fixture(scope="module")
def g20(golden_dir):
    return np.load(os.path.join(golden_dir, "g20_vit.npz"))


@pytest.mark.parametrize("net", ["a", "b"])
@pytest.mark.parametrize("case", ["a64", "a96", "a70"])
def test_backbone_gpu_vs_reference(g20, net, case, capsys):
    from ppnet_amd import vit
    from tests._vit_golden import image
    from tests.test_vit_golden import load_net
    m = load_net(g20, net, torch.float32).to(DEV)
    x = torch.from_numpy(image(case)).to(DEV)
    vit.CALLS.update(kernel=0)
    with torch.no_grad():
        outs = m(x)
    torch.cuda.synchronize()
    assert vit.CALLS["kernel"] == 3
    for i, o in enumerate(outs):
        want = g20[f"{net}/{case}/y{i}"]
        ref = np.abs(want).max()
        err = np.abs(o.double().cpu().numpy() - want).max() / ref
        with capsys.disabled():
            print(f"\nvit backbone net {net} case {case} out {i}: fp32 max err {err:.2e} x max|ref|")
        assert err <= 1e-6, (net, case, i, err)


# ------------------------------------------------------------------------------------------------ SegNet with ViT-B
def _codes(B, R, seed):
    g = torch.Generator().manual_seed(seed)
    lo = (torch.rand(B, 1, R // 16, R // 16, generator=g) > 0.4).float()
    return (torch.nn.functional.interpolate(lo, size=(R, R), mode="nearest")[:, 0] * 255).to(torch.uint8)


def test_segnet_vit_base_setrup_bf16_vs_fp32(capsys):
    from ppnet_amd import fused, segnet, vit
    torch.manual_seed(0)
    m32 = segnet.randomize_neutral_parameters(segnet.SegNet.from_config(segnet.VIT_BASE_SETRUP), seed=1)
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():                                                   # the helper leaves these two alone: the reference's std
        m32.backbone.pos_embed.copy_(torch.randn(m32.backbone.pos_embed.shape, generator=g) * 0.02)
        m32.backbone.cls_token.copy_(torch.randn(m32.backbone.cls_token.shape, generator=g) * 0.02)
    m32 = m32.eval().to(DEV)
    codes = _codes(4, 256, 5).to(DEV)
    with torch.no_grad():
        segnet.balance_classifier_bias(m32, fused.grid_to_image(codes, segnet.IMG_MEAN, segnet.IMG_STD, torch.float32))
    m16 = copy.deepcopy(m32).to(torch.bfloat16)
    m32.prepare_inference()
    m16.prepare_inference()
    with torch.no_grad():
        l32 = m32.labels_u8(codes)
        vit.CALLS.update(kernel=0)
        l16 = m16.labels_u8(codes)
        calls = vit.CALLS["kernel"]
        res = m16.simple_test(codes, [{"ori_shape": (256, 256, 3)}] * 4)
    torch.cuda.synchronize()
    assert calls == 12                                                      # every layer's attention on ppn_mhsa_fwd
    assert l16.dtype == torch.uint8 and l16.shape == (4, 256, 256)
    assert len(res) == 4 and res[0].shape == (256, 256) and res[0].dtype == np.int64
    assert np.array_equal(np.stack(res), l16.cpu().numpy().astype(np.int64))
    agree = (l32 == l16).float().mean().item()
    frac1 = l32.float().mean().item()
    with capsys.disabled():
        print(f"\nVIT_BASE_SETRUP: bf16 vs fp32 label agreement {agree:.5f} (class-1 fraction {frac1:.3f})")
    assert 0.05 < frac1 < 0.95
    # The backbone's share: its bf16 features through the float32 head agree on > 0.98 (measured 0.993).  The whole bf16 network
    # measured 0.966, and float32 features rounded to bf16 through the bf16 SETR-UP head alone 0.970: the head on these 768-channel
    # features sets the whole network's bound, and the framework's bf16 backbone gives the same 0.966 (tools/vit_precision.py,
    # profiles/r08_vit_precision.txt).
    with torch.no_grad():
        lb = fused.seg_labels_2class(m32.decode_head([f.float() for f in m16.backbone(codes)], lowres=True), (256, 256))
    agree_bb = (l32 == lb).float().mean().item()
    with capsys.disabled():
        print(f"VIT_BASE_SETRUP: bf16 backbone + fp32 head vs fp32 label agreement {agree_bb:.5f}")
    assert agree_bb > 0.98, agree_bb
    assert agree > 0.95, agree
