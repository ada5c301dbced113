"""GPU parity of the fused neighbourhood-attention kernel (C ABI ppn_na2d_fwd) and its nn.Module against the
definition oracle (oracle/na_np.py; parity unpinned — NATTEN is not in the reference).  float32: 2e-5 absolute
on O(1) outputs (fp32 accumulation order); bfloat16 I/O: 3e-2.
Every kernel variant on its own (A/B knobs, known answers, large logits, guards): tests/test_gpu_na_variants.py."""
import numpy as np
import pytest

from oracle import na_np as NA

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


CASES = [  # B, H, W, heads, dilation
    (2, 14, 15, 2, 1), (1, 7, 7, 1, 1), (1, 33, 18, 3, 1), (2, 20, 17, 2, 2), (1, 30, 28, 2, 4), (1, 21, 23, 1, 3),
    (1, 40, 36, 2, 1), (1, 64, 64, 4, 1), (1, 56, 56, 1, 8),
]


@pytest.mark.parametrize("B,H,W,heads,d", CASES)
def test_kernel_vs_oracle_f32(dev, B, H, W, heads, d):
    import torch
    from ppnet_amd import na
    rng = np.random.RandomState(H * 100 + W + d)
    C = heads * 32
    qkv = rng.standard_normal((B, H, W, 3 * C)).astype(np.float32)
    rpb = rng.standard_normal((heads, 13, 13)).astype(np.float32)
    scale = 32 ** -0.5
    got = na.na2d_forward(torch.tensor(qkv, device=dev), torch.tensor(rpb, device=dev), heads, d, scale).cpu().numpy()
    want = NA.na2d_from_qkv(qkv, rpb, heads, 7, d, scale)
    assert np.abs(got - want).max() < 2e-5


@pytest.mark.parametrize("B,H,W,heads,d", [(2, 20, 17, 2, 2), (1, 64, 64, 4, 1), (2, 56, 56, 2, 8), (3, 7, 7, 1, 1), (1, 21, 21, 3, 3),
                                           (2, 16, 16, 2, 2), (3, 8, 8, 3, 1), (1, 32, 32, 1, 4),    # 7 x 7 and 8 x 8 dilation groups: na2d_dense7.hip
                                           # groups that fill a 16 x 16 region poorly and still take it (na_region_size: the cheapest
                                           # cover, round 4): 11 x 11 / 10 x 11 groups of dilation 3 at 32 x 32 (DiNAT-B level 2 at 512 x 512),
                                           # the 56 x 56 level of a 224 x 224 input, a 9 x 12 remainder; and one the 8 x 8 regions keep
                                           (2, 32, 32, 2, 3), (1, 56, 56, 2, 1), (1, 25, 28, 1, 1), (2, 9, 9, 1, 1), (1, 18, 20, 2, 2)])
def test_kernel_vs_oracle_bf16(dev, B, H, W, heads, d):
    import torch
    from ppnet_amd import na
    rng = np.random.RandomState(3)
    C = heads * 32
    qkv = torch.tensor(rng.standard_normal((B, H, W, 3 * C)).astype(np.float32)).to(torch.bfloat16)
    rpb = rng.standard_normal((heads, 13, 13)).astype(np.float32)
    got = na.na2d_forward(qkv.to(dev), torch.tensor(rpb, device=dev), heads, d, 32 ** -0.5).float().cpu().numpy()
    want = NA.na2d_from_qkv(qkv.float().numpy(), rpb, heads, 7, d, 32 ** -0.5)
    assert np.abs(got - want).max() < 3e-2


@pytest.mark.parametrize("H,W,d", [(10, 12, 2), (16, 16, 4), (8, 8, 16), (20, 20, 1)])
def test_module_with_padding_vs_oracle(dev, H, W, d):
    """DiNAT-B's dilations exceed L//7 on every level at 224/256 inputs, so the pad-to-k*d path is the common case."""
    import torch
    from ppnet_amd import na
    torch.manual_seed(0)
    dim, heads = 64, 2
    m = na.NeighborhoodAttention2D(dim, kernel_size=7, dilation=d, num_heads=heads).to(dev).eval()
    assert set(m.state_dict().keys()) == {"qkv.weight", "qkv.bias", "rpb", "proj.weight", "proj.bias"}
    x = torch.randn(2, H, W, dim, device=dev)
    with torch.no_grad():
        got = m(x).cpu().numpy()
    sd = {k: v.detach().cpu().double().numpy() for k, v in m.state_dict().items()}
    want = NA.neighborhood_attention_2d(x.cpu().double().numpy(), sd["qkv.weight"], sd["qkv.bias"], sd["rpb"],
                                        sd["proj.weight"], sd["proj.bias"], heads, 7, d)
    assert got.shape == (2, H, W, dim)
    assert np.abs(got - want).max() < 5e-5


@pytest.mark.parametrize("H,W,Hr,Wr,d,heads", [(28, 28, 16, 16, 4, 2), (112, 112, 64, 64, 16, 1), (14, 14, 8, 8, 2, 3), (21, 21, 16, 13, 3, 2)])
def test_padded_grid_queries_only_real_tokens(dev, H, W, Hr, Wr, d, heads):
    """ppn_na2d_fwd_padded: keys/values over the padded grid, queries and output over the real tokens only."""
    import torch
    from ppnet_amd import na
    rng = np.random.RandomState(7)
    C = heads * 32
    qkv = rng.standard_normal((1, H, W, 3 * C)).astype(np.float32)
    rpb = rng.standard_normal((heads, 13, 13)).astype(np.float32)
    got = na.na2d_forward(torch.tensor(qkv, device=dev), torch.tensor(rpb, device=dev), heads, d, 32 ** -0.5, (Hr, Wr)).cpu().numpy()
    want = NA.na2d_from_qkv(qkv, rpb, heads, 7, d, 32 ** -0.5)[:, :Hr, :Wr]
    assert got.shape == (1, Hr, Wr, C)
    assert np.abs(got - want).max() < 2e-5


@pytest.mark.parametrize("B,side,C,heads,d,pad", [(256, 64, 128, 4, 1, 0), (64, 56, 128, 4, 1, 0), (8, 32, 256, 8, 1, 0), (4, 40, 64, 2, 2, 0),
                                                  (3, 33, 64, 2, 1, 0), (2, 30, 64, 2, 2, 34)])
def test_persistent_halo_kernel_against_the_per_tile_kernel(dev, B, side, C, heads, d, pad, monkeypatch):
    """na2d_halo16_kernel (persistent, LDS-DMA staging, tile descriptors) against na2d_mfma_kernel<16> at the bench's full size
    (256 x 64 x 64 x 4 heads), on partial tiles, dilation groups of unequal size and virtual padding — a size-independent property
    the oracle is too slow to give.  With 4 x 4 query blocks (PPNET_NA_HALO_BLOCK=4x4) it computes block for block what the per-tile
    kernel does and the outputs are EQUAL; with 2 x 8 blocks (the default) logits, maxima and probabilities are the same numbers
    and only the float32 order of the 8 instead of 10 key tiles' sums differs: at most one bfloat16 step, on a few elements."""
    import os
    import torch
    from ppnet_amd.na import na2d_forward
    torch.manual_seed(side + d)
    qkv = torch.randn(B, side, side, 3 * C, device=dev, dtype=torch.bfloat16)
    rpb = torch.randn(heads, 13, 13, device=dev)
    kw = dict(pad_kv=torch.randn(3 * C, device=dev, dtype=torch.bfloat16), padded_hw=(pad, pad)) if pad else {}
    monkeypatch.setenv("PPNET_NA_RT", "16")                      # both runs on 16 x 16 regions
    monkeypatch.delenv("PPNET_NA_HALO16", raising=False)
    a = na2d_forward(qkv, rpb, heads, d, 32 ** -0.5, **kw)
    monkeypatch.setenv("PPNET_NA_HALO16", "0")
    b = na2d_forward(qkv, rpb, heads, d, 32 ** -0.5, **kw)
    assert torch.isfinite(a.float()).all()
    if os.environ.get("PPNET_NA_HALO_BLOCK", "").startswith("4"):
        assert torch.equal(a, b)
    else:
        af, bf = a.float(), b.float()
        assert bool(((af - bf).abs() <= 2.0 ** -7 * bf.abs().clamp_min(2.0 ** -6)).all())          # one step of an 8-bit significand
        assert float((a != b).float().mean()) < 1e-4


@pytest.mark.parametrize("B,side,heads,d,pad", [(64, 56, 2, 8, 0), (48, 16, 2, 3, 21), (96, 32, 2, 4, 0), (40, 16, 4, 4, 28)])
def test_dense_group_kernel_over_many_items_per_wave(dev, B, side, heads, d, pad, monkeypatch):
    """na2d_dense7_kernel walks its (image, group) items with a constant stride and advances (image, group row, group column) by
    carries instead of dividing them out per item (round 5), and rewrites a wave's padding pieces only when a group's extent changes:
    sizes at which a wave takes several items (more groups than resident waves) with equal and with unequal extents (16 / 3: groups of
    6 and 5 rows), against the halo / per-tile kernels on the same input (PPNET_NA_NO_DENSE7 is read per process: a child runs them)."""
    import subprocess, sys, os, tempfile
    import torch
    from ppnet_amd.na import na2d_forward
    C = heads * 32
    torch.manual_seed(B + side + d)
    qkv = torch.randn(B, side, side, 3 * C, device=dev, dtype=torch.bfloat16)
    rpb = torch.randn(heads, 13, 13, device=dev)
    pkv = torch.randn(3 * C, device=dev, dtype=torch.bfloat16)
    kw = dict(pad_kv=pkv, padded_hw=(pad, pad)) if pad else {}
    a = na2d_forward(qkv, rpb, heads, d, 32 ** -0.5, **kw).float().cpu()
    with tempfile.TemporaryDirectory() as td:
        torch.save({"qkv": qkv.cpu(), "rpb": rpb.cpu(), "pkv": pkv.cpu()}, os.path.join(td, "in.pt"))
        code = ("import torch, sys; from ppnet_amd.na import na2d_forward; d = torch.load(sys.argv[1] + '/in.pt'); dev = torch.device('cuda', 0);"
                f"kw = dict(pad_kv=d['pkv'].to(dev), padded_hw=({pad}, {pad})) if {pad} else dict();"
                f"o = na2d_forward(d['qkv'].to(dev), d['rpb'].to(dev), {heads}, {d}, 32 ** -0.5, **kw); torch.save(o.float().cpu(), sys.argv[1] + '/out.pt')")
        env = dict(os.environ, PPNET_NA_NO_DENSE7="1", PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        subprocess.run([sys.executable, "-c", code, td], check=True, env=env, timeout=300)
        b = torch.load(os.path.join(td, "out.pt"))
    assert torch.isfinite(a).all() and a.shape == b.shape
    assert float((a - b).abs().max()) < 3e-2 and float((a - b).pow(2).mean().sqrt()) < 2e-3


def test_no_cpu_fallback():
    import torch
    from ppnet_amd import na
    with pytest.raises(RuntimeError):
        na.na2d_forward(torch.zeros(1, 7, 7, 96), torch.zeros(1, 13, 13), 1, 1, 1.0)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("H,W,Hr,Wr,d,heads", [(28, 28, 16, 16, 4, 2), (112, 112, 64, 64, 16, 1), (14, 14, 8, 8, 2, 3), (21, 21, 16, 13, 3, 2)])
def test_virtual_padding_equals_materialised_padding(dev, H, W, Hr, Wr, d, heads, dtype):
    """ppn_na2d_fwd_vpad (real tokens + one k/v for every padded position) gives the bits of ppn_na2d_fwd_padded on the
    grid that holds that k/v at every padded position — what projecting a zero-padded input produces."""
    import torch
    from ppnet_amd import na
    rng = np.random.RandomState(11)
    C = heads * 32
    dt = getattr(torch, dtype)
    real = torch.tensor(rng.standard_normal((2, Hr, Wr, 3 * C)).astype(np.float32), device=dev).to(dt)
    bias = torch.tensor(rng.standard_normal(3 * C).astype(np.float32), device=dev).to(dt)
    rpb = torch.tensor(rng.standard_normal((heads, 13, 13)).astype(np.float32), device=dev)
    full = bias.expand(2, H, W, 3 * C).clone()
    full[:, :Hr, :Wr] = real
    want = na.na2d_forward(full, rpb, heads, d, 32 ** -0.5, real_hw=(Hr, Wr))
    got = na.na2d_forward(real, rpb, heads, d, 32 ** -0.5, pad_kv=bias, padded_hw=(H, W))
    assert got.shape == want.shape == (2, Hr, Wr, C)
    if dt == torch.float32:
        assert torch.equal(got, want)
    else:
        # bf16: the padded neighbours' probabilities are pooled into one p_pad * v_pad term (float32) instead of being
        # rounded to bf16 one by one — same logits and softmax, a different (finer) accumulation of the AV product
        assert (got.float() - want.float()).abs().max() < 2e-2
        ref = NA.na2d_from_qkv(full.float().cpu().numpy(), rpb.cpu().numpy(), heads, 7, d, 32 ** -0.5)[:, :Hr, :Wr]
        assert np.abs(got.float().cpu().numpy() - ref).max() < 3e-2


@pytest.mark.parametrize("B,H,W,heads,d", [(2, 9, 11, 2, 1), (1, 16, 14, 2, 2), (2, 7, 7, 1, 1), (1, 21, 24, 1, 3), (1, 20, 27, 2, 1),
                                           (1, 37, 40, 1, 2), (1, 33, 17, 1, 1)])
def test_na2d_backward_vs_fp64_autograd(dev, B, H, W, heads, d):
    """ppn_na2d_bwd (dQ, dK, dV, dRPB) against autograd through the float64 gather definition of the op (oracle/segnet_ref.py
    na_fp64, itself checked against the brute-force oracle) — borders, dilation groups of unequal size, several heads, maps of
    several 8 x 8 regions per axis (a border key is seen by up to 10 queries per axis; 20 rows: a region whose query halo is 15)."""
    import torch
    from oracle import segnet_ref as SR
    from ppnet_amd.na import na2d_autograd
    torch.manual_seed(H * W + d)
    C = heads * 32
    qkv = torch.randn(B, H, W, 3 * C, device=dev, dtype=torch.float32, requires_grad=True)
    rpb = (torch.randn(heads, 13, 13, device=dev) * 0.5).requires_grad_(True)
    gout = torch.randn(B, H, W, C, device=dev)
    out = na2d_autograd(qkv, rpb, heads, d, 32 ** -0.5)
    out.backward(gout)
    # float64 definition: identity projections around the gather (x -> qkv is the identity on a 3C-wide "token")
    q64 = qkv.detach().double().requires_grad_(True)
    r64 = rpb.detach().double().requires_grad_(True)

    def ref(qkv_, rpb_):
        Hp, Wp = qkv_.shape[1], qkv_.shape[2]
        ri, bi = SR._axis_tables(Hp, 7, d, qkv_.device)
        cj, bj = SR._axis_tables(Wp, 7, d, qkv_.device)
        bias = rpb_[:, bi[:, None, :, None], bj[None, :, None, :]]
        outs = []
        for b in range(qkv_.shape[0]):
            t = qkv_[b].view(Hp, Wp, 3, heads, 32).permute(2, 3, 0, 1, 4)
            q, kk, v = t[0] * 32 ** -0.5, t[1], t[2]
            kg, vg = kk[:, ri][:, :, :, cj], v[:, ri][:, :, :, cj]
            p = torch.softmax((torch.einsum("hijc,hiajbc->hijab", q, kg) + bias).reshape(heads, Hp, Wp, 49), dim=-1).view(heads, Hp, Wp, 7, 7)
            outs.append(torch.einsum("hijab,hiajbc->hijc", p, vg).permute(1, 2, 0, 3).reshape(Hp, Wp, C))
        return torch.stack(outs)
    want = ref(q64, r64)
    assert (out.detach().double() - want.detach()).abs().max() < 1e-4
    want.backward(gout.double())
    assert (qkv.grad.double() - q64.grad).abs().max() < 2e-4 * max(1.0, float(q64.grad.abs().max()))
    assert (rpb.grad.double() - r64.grad).abs().max() < 2e-4 * max(1.0, float(r64.grad.abs().max()))


def test_na2d_backward_bf16_workspace_and_reproducibility(dev):
    """bfloat16 tensors (float32 arithmetic) against the float32 run on the same values; the rpb gradient is bit-identical from
    run to run (fixed summation order, no atomics); a workspace smaller than ppn_na2d_bwd_workspace says is refused."""
    import ctypes
    import torch
    from ppnet_amd import _lib as L
    from ppnet_amd.na import na2d_autograd
    torch.manual_seed(3)
    B, H, W, heads, d = 2, 19, 23, 2, 1
    C = heads * 32
    q16 = torch.randn(B, H, W, 3 * C, device=dev).to(torch.bfloat16)
    rpb = torch.randn(heads, 13, 13, device=dev) * 0.5
    gout = torch.randn(B, H, W, C, device=dev).to(torch.bfloat16)
    grads = []
    for dt in (torch.float32, torch.bfloat16, torch.float32):
        q = q16.detach().to(dt).clone().requires_grad_(True)
        r = rpb.clone().requires_grad_(True)
        na2d_autograd(q, r, heads, d, 32 ** -0.5).backward(gout.to(dt))
        grads.append((q.grad.float(), r.grad.clone()))
    assert (grads[1][0] - grads[0][0]).abs().max() < 2e-2 * float(grads[0][0].abs().max())      # bf16-rounded outputs
    assert (grads[1][1] - grads[0][1]).abs().max() < 1e-3 * max(1.0, float(grads[0][1].abs().max()))
    assert torch.equal(grads[2][0], grads[0][0]) and torch.equal(grads[2][1], grads[0][1])
    need = L.lib.ppn_na2d_bwd_workspace(B, H, W, heads, d)
    assert need == B * heads * H * W * 4 + 3 * 3 * B * heads * 169
    assert L.lib.ppn_na2d_bwd_workspace(B, 6, W, heads, d) < 0
    q = q16.float()
    dq, dr, ws = torch.empty_like(q), torch.empty_like(rpb), torch.empty(need, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert L.lib.ppn_na2d_bwd(p(q), p(rpb), p(gout.float()), p(dq), p(dr), p(ws), need - 1, B, H, W, heads, d, 32 ** -0.5, 0, None) == -1      # PPN_E_INVALID


def test_na_module_trains_through_padding(dev):
    """The module's training path (pad -> qkv -> NA -> crop -> proj) is differentiable end to end on a padded dilated layer and
    its forward equals the inference path (virtual padding)."""
    import torch
    from ppnet_amd.na import NeighborhoodAttention2D
    torch.manual_seed(5)
    m = NeighborhoodAttention2D(64, 7, dilation=2, num_heads=2).to(dev)
    x = torch.randn(2, 9, 10, 64, device=dev, requires_grad=True)              # 9 x 10 < 14: padded to 14 x 14
    y = m(x)
    with torch.no_grad():
        y_inf = m(x.detach())
    assert (y.detach() - y_inf).abs().max() < 1e-4
    y.square().mean().backward()
    for t in (x.grad, m.rpb.grad, m.qkv.weight.grad, m.proj.weight.grad):
        assert t is not None and torch.isfinite(t).all() and float(t.abs().max()) > 0
