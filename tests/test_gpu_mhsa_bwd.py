"""ppn_mhsa_bwd (csrc/mhsa_bwd.hip) on the GPU: the kernel against float64 autograd of the definition, known answers, bitwise
reproducibility, memory it may touch, the ViT module's training branch, its peak memory, and training steps of ViT + SETR-UP.

The precision rule (every gradient dq, dk, dv apart, err = max|got - ref| / max|ref| over EVERY element, ref = float64 autograd on
the CPU, bfloat16: on the rounded inputs): err <= max(2 x the error of the framework's explicit op chain in the same data type on
the same inputs, measured in the same run; the forward kernel's bound: 2e-6 float32, 1e-2 bfloat16).  The chain is
softmax(scale q k^T) v written with matmul and softmax under autograd on the GPU — not the code under test and not SDPA.  Factor 2:
the kernel keeps S, dP and all sums in float32 and rounds P and dS once where the bfloat16 chain rounds every intermediate (1 x),
and it sums in another order (1 x).

Each test prints what it measured (run with -s); the worst figures per data type are in profiles/r09_mhsa_bwd_precision.txt."""
import copy
import ctypes

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda"
SCALE = 64 ** -0.5
FLOOR = {torch.float32: 2e-6, torch.bfloat16: 1e-2}            # tests/test_gpu_vit.py: the forward kernel's bounds
SHAPES = [(1, 1, 1), (2, 7, 2), (3, 64, 12), (2, 196, 12), (2, 197, 12), (1, 256, 12), (2, 257, 3), (1, 1024, 12), (1, 1025, 2),
          (1, 4096, 1)]


def _definition(qkv, dout, heads, scale):
    """(out, dqkv) of softmax(scale q k^T) v by matmul / softmax under autograd, in qkv's dtype on qkv's device."""
    B, N, _ = qkv.shape
    t = qkv.detach().clone().requires_grad_(True)
    u = t.view(B, N, 3, heads, 64).permute(2, 0, 3, 1, 4)                  # [3, B, heads, N, 64]
    p = torch.softmax((u[0] @ u[1].transpose(-1, -2)) * scale, dim=-1)
    out = (p @ u[2]).permute(0, 2, 1, 3).reshape(B, N, heads * 64)
    g, = torch.autograd.grad(out, t, dout)
    return out.detach(), g


def _kernel(qkv, dout, heads, scale):
    """dqkv through vit.mhsa_autograd (ppn_mhsa_fwd forward, ppn_mhsa_bwd backward)."""
    from ppnet_amd import vit
    t = qkv.detach().clone().requires_grad_(True)
    out = vit.mhsa_autograd(t, heads, scale)
    g, = torch.autograd.grad(out, t, dout)
    torch.cuda.synchronize()
    return g


def _errors(got, ref, heads):
    """max|got - ref| / max|ref| of dq, dk, dv (every element); a reference that is exactly 0 asks for exactly 0."""
    B, N, _ = ref.shape
    got = got.double().cpu().view(B, N, 3, heads * 64)
    ref = ref.view(B, N, 3, heads * 64)
    errs = []
    for i in range(3):
        d, r = (got[:, :, i] - ref[:, :, i]).abs().max().item(), ref[:, :, i].abs().max().item()
        errs.append(d / r if r > 0 else (0.0 if d == 0 else float("inf")))
    return errs


def _measure(qkv, dout, heads, scale, dtype):
    """(kernel errors, chain errors, bounds) for dq, dk, dv on inputs already rounded to dtype."""
    _, ref = _definition(qkv.double(), dout.double(), heads, scale)                    # float64, CPU
    _, chain = _definition(qkv.to(DEV), dout.to(DEV), heads, scale)
    got = _kernel(qkv.to(DEV), dout.to(DEV), heads, scale)
    assert got.dtype == dtype and got.shape == qkv.shape and bool(torch.isfinite(got).all())
    ek, ec = _errors(got, ref, heads), _errors(chain, ref, heads)
    return ek, ec, [max(2.0 * c, FLOOR[dtype]) for c in ec]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,N,heads", SHAPES)
def test_kernel_vs_float64(dtype, B, N, heads, capsys):
    g = torch.Generator().manual_seed(1000 * N + 10 * heads + B)
    qkv = torch.randn(B, N, 3 * heads * 64, generator=g).to(dtype)
    dout = torch.randn(B, N, heads * 64, generator=g).to(dtype)
    ek, ec, bound = _measure(qkv, dout, heads, SCALE, dtype)
    with capsys.disabled():
        f = lambda v: " ".join(f"{x:.2e}" for x in v)
        print(f"\nmhsa_bwd {str(dtype)[6:]} B {B} N {N} heads {heads}: dq dk dv kernel {f(ek)} | chain {f(ec)} | bound {f(bound)}")
    for name, e, b in zip(("dq", "dk", "dv"), ek, bound):
        assert e <= b, (name, B, N, heads, e, b)


def _raw(qkv, out, dout, heads, scale, dqkv=None, ws=None, B=None, N=None):
    """ppn_mhsa_bwd itself on device tensors; dqkv / ws may be views into larger buffers."""
    from ppnet_amd import _lib as L
    B = qkv.shape[0] if B is None else B
    N = qkv.shape[1] if N is None else N
    need = L.lib.ppn_mhsa_bwd_workspace(B, N, heads)
    assert need >= 2 * B * heads * N
    if dqkv is None:
        dqkv = torch.empty(B, N, 3 * heads * 64, dtype=qkv.dtype, device=DEV)
    if ws is None:
        ws = torch.empty(need, dtype=torch.float32, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = L.lib.ppn_mhsa_bwd(P(qkv), P(out), P(dout), P(dqkv), P(ws), need, B, N, heads, 64, float(scale), 0 if qkv.dtype == torch.float32 else 1,
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    return dqkv


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_known_answers(dtype, capsys):
    from ppnet_amd import vit
    heads = 2
    g = torch.Generator().manual_seed(21)
    # N = 1: P = 1 whatever q and k are -> dq = dk = 0 exactly, dv = dout exactly
    qkv = torch.randn(3, 1, 3 * heads * 64, generator=g).to(dtype).to(DEV)
    dout = torch.randn(3, 1, heads * 64, generator=g).to(dtype).to(DEV)
    got = _kernel(qkv, dout, heads, SCALE).view(3, 1, 3, heads * 64)
    assert bool((got[:, :, 0] == 0).all()) and bool((got[:, :, 1] == 0).all())
    assert torch.equal(got[:, :, 2], dout)
    # all keys equal: P is uniform and every row of dS sums to 0 -> dq = scale (sum_j dS_ij) k = 0 to rounding.  Measured against
    # the same sum without cancellation, scale sum_j |dS_ij| |k|, with the forward bound of the data type.
    B, N = 2, 300
    q = torch.randn(B, N, heads, 64, generator=g)
    k = torch.randn(B, 1, heads, 64, generator=g).expand(B, N, heads, 64)
    v = torch.randn(B, N, heads, 64, generator=g)
    qkv = torch.stack([q, k, v], 2).reshape(B, N, 3 * heads * 64).to(dtype)
    dout = torch.randn(B, N, heads * 64, generator=g).to(dtype)
    got = _kernel(qkv.to(DEV), dout.to(DEV), heads, SCALE).double().cpu().view(B, N, 3, heads, 64)
    t = qkv.double().view(B, N, 3, heads, 64).permute(2, 0, 3, 1, 4)
    do = dout.double().view(B, N, heads, 64).permute(0, 2, 1, 3)
    dp = do @ t[2].transpose(-1, -2)                                                   # P = 1 / N
    ds = (dp - dp.mean(-1, keepdim=True)) / N
    nocancel = (SCALE * ds.abs().sum(-1, keepdim=True) * t[1].abs()).max().item()
    dq = got[:, :, 0].abs().max().item()
    with capsys.disabled():
        print(f"\nmhsa_bwd {str(dtype)[6:]} equal keys: max|dq| {dq:.2e} = {dq / nocancel:.2e} x the uncancelled sum")
    assert dq <= FLOOR[dtype] * nocancel
    # logits of +-60..90 (the forward test's construction): finite, within 5 x the rule
    B, N, heads = 2, 300, 3
    g = torch.Generator().manual_seed(5)
    u = torch.randn(B, N, heads, 64, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    s = torch.sign(torch.randn(B, N, heads, 1, generator=g))
    a = (70.0 / SCALE) ** 0.5
    q = a * u + 0.05 * torch.randn(B, N, heads, 64, generator=g)
    k = a * s * u[:, torch.randperm(N, generator=g)] + 0.05 * torch.randn(B, N, heads, 64, generator=g)
    k[:, :, :, :] = k + a * s * 0.3 * u
    v = torch.randn(B, N, heads, 64, generator=g)
    qkv = torch.stack([q, k, v], 2).reshape(B, N, 3 * heads * 64).to(dtype)
    dout = torch.randn(B, N, heads * 64, generator=g).to(dtype)
    t = qkv.double().view(B, N, 3, heads, 64)
    lg = torch.einsum("bnhd,bmhd->bhnm", t[:, :, 0], t[:, :, 1]) * SCALE
    assert 60.0 <= lg.abs().max().item() <= 90.0, lg.abs().max().item()
    ek, ec, bound = _measure(qkv, dout, heads, SCALE, dtype)
    with capsys.disabled():
        f = lambda v: " ".join(f"{x:.2e}" for x in v)
        print(f"mhsa_bwd {str(dtype)[6:]} logits +-60..90: dq dk dv kernel {f(ek)} | chain {f(ec)} | bound 5 x {f(bound)}")
    for name, e, b in zip(("dq", "dk", "dv"), ek, bound):
        assert e <= 5.0 * b, (name, e, b)
    assert vit.CALLS["bwd_kernel"] > 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,N,heads", [(2, 197, 12), (1, 1024, 12)])
def test_bitwise_reproducible(dtype, B, N, heads):
    from ppnet_amd import vit
    g = torch.Generator().manual_seed(77 + N)
    qkv = torch.randn(B, N, 3 * heads * 64, generator=g).to(dtype).to(DEV)
    dout = torch.randn(B, N, heads * 64, generator=g).to(dtype).to(DEV)
    with torch.no_grad():
        out = vit.mhsa_forward(qkv, heads, SCALE)
    a = _raw(qkv, out, dout, heads, SCALE)
    b = _raw(qkv, out, dout, heads, SCALE)
    # unrelated work in between: other kernels, another shape of this one, fresh allocations
    x = torch.randn(2048, 2048, device=DEV)
    y = (x @ x).relu().sum()
    q2 = torch.randn(1, 333, 3 * 64, device=DEV).to(dtype)
    with torch.no_grad():
        o2 = vit.mhsa_forward(q2, 1, SCALE)
    _raw(q2, o2, torch.randn(1, 333, 64, device=DEV).to(dtype), 1, SCALE)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y))
    c = _raw(qkv, out, dout, heads, SCALE)
    assert bool(torch.isfinite(a).all())
    assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_kernel_reads_and_writes_only_its_rows(dtype):
    """Large finite garbage in the rows just past row N of qkv, out and dout must reach nothing; dqkv and the workspace sit inside
    canary-filled buffers whose canaries survive; the result equals the plain call's bit for bit."""
    from ppnet_amd import _lib as L
    from ppnet_amd import vit
    B, N, heads = 1, 197, 2
    C = heads * 64
    g = torch.Generator().manual_seed(13)
    qkv = torch.randn(B, N, 3 * C, generator=g).to(dtype).to(DEV)
    dout = torch.randn(B, N, C, generator=g).to(dtype).to(DEV)
    with torch.no_grad():
        out = vit.mhsa_forward(qkv, heads, SCALE)
    plain = _raw(qkv, out, dout, heads, SCALE)

    def padded(t):
        buf = torch.full((N + 130, t.shape[-1]), 3.0e4, dtype=dtype, device=DEV)       # rows N .. N + 129: exp(huge) if read
        buf[:N] = t[0]
        return buf
    qp, op, dp = padded(qkv), padded(out), padded(dout)
    pad = 4096                                                                         # elements: a multiple of 16 bytes
    n = B * N * 3 * C
    dbuf = torch.full((pad + n + pad,), 12345.0, dtype=dtype, device=DEV)
    need = L.lib.ppn_mhsa_bwd_workspace(B, N, heads)
    wbuf = torch.full((pad + need + pad,), 54321.0, dtype=torch.float32, device=DEV)
    got = _raw(qp, op, dp, heads, SCALE, dqkv=dbuf[pad:pad + n], ws=wbuf[pad:pad + need], B=B, N=N)
    assert bool((dbuf[:pad] == 12345.0).all()) and bool((dbuf[pad + n:] == 12345.0).all())
    assert bool((wbuf[:pad] == 54321.0).all()) and bool((wbuf[pad + need:] == 54321.0).all())
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got.view(B, N, 3 * C), plain)
    for buf in (qp, op, dp):
        assert bool((buf[N:] == 3.0e4).all())


def test_kernel_rejects_bad_arguments_on_gpu_buffers():
    from ppnet_amd import _lib as L
    q = torch.zeros(1, 8, 3 * 64, device=DEV)
    o = torch.zeros(1, 8, 64, device=DEV)
    d = torch.zeros(1, 8, 3 * 64, device=DEV)
    w = torch.zeros(64, device=DEV)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    f = L.lib.ppn_mhsa_bwd
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    assert L.lib.ppn_mhsa_bwd_workspace(1, 8, 1) == 16
    assert f(P(q), P(o), P(o), P(d), P(w), 16, 1, 8, 1, 32, 0.125, 0, s) == -3
    assert f(P(q), P(o), P(o), P(d), P(w), 15, 1, 8, 1, 64, 0.125, 0, s) == -1
    assert f(P(q), P(o), P(o), ctypes.c_void_p(d.data_ptr() + 4), P(w), 16, 1, 8, 1, 64, 0.125, 0, s) == -1
    assert f(P(q), P(o), P(o), P(d), P(w), 16, 1, 8, 1, 64, 0.125, 0, s) == 0
    torch.cuda.synchronize()
    assert bool((d == 0).all())                                                        # dout = 0 -> every gradient 0, all of dqkv written


# ------------------------------------------------------------------------------------------------ the module
def _library_forward(self, x, identity):
    """vit.MultiheadAttention.forward through the wrapped nn.MultiheadAttention (what every non-kernel case runs)."""
    from ppnet_amd.dense import drop_path
    out = self.attn(x.transpose(0, 1), x.transpose(0, 1), x.transpose(0, 1), need_weights=False)[0].transpose(0, 1)
    return identity + drop_path(self.proj_drop(out), self.drop_path_rate, self.training)


def _small_vit(**kw):
    from ppnet_amd import vit
    torch.manual_seed(4)
    m = vit.VisionTransformer(img_size=64, patch_size=16, embed_dims=128, num_layers=2, num_heads=2, **kw)
    m.init_weights()
    with torch.no_grad():                                                              # biases and norms off their neutral values
        for n, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    return m


def _grads(m, x0, w):
    x = x0.clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    (m(x)[0] * w).sum().backward()
    return {"input": x.grad.detach().double().cpu(), **{n: p.grad.detach().double().cpu() for n, p in m.named_parameters() if p.grad is not None}}


def test_module_gradients_through_the_kernel(monkeypatch, capsys):
    """A small ViT in float32: gradients of every parameter and of the input through the kernel path and through
    nn.MultiheadAttention (same weights, same GPU), each against the float64 CPU model: the item-4 rule with the library path as
    the chain, relative to each gradient's max."""
    from ppnet_amd import vit
    m = _small_vit().train()
    g = torch.Generator().manual_seed(8)
    x0 = torch.randn(2, 3, 64, 64, generator=g)
    w = torch.randn(2, 128, 4, 4, generator=g)
    ref = _grads(copy.deepcopy(m).double(), x0.double(), w.double())                   # CPU: nn.MultiheadAttention in float64
    mg = copy.deepcopy(m).to(DEV)
    vit.CALLS.update(kernel=0, bwd_kernel=0)
    got = _grads(mg, x0.to(DEV), w.to(DEV))
    torch.cuda.synchronize()
    assert vit.CALLS["kernel"] == 2 and vit.CALLS["bwd_kernel"] == 2                   # one per layer and backward
    with monkeypatch.context() as mp:
        mp.setattr(vit.MultiheadAttention, "forward", _library_forward)
        lib = _grads(mg, x0.to(DEV), w.to(DEV))
    assert vit.CALLS["bwd_kernel"] == 2
    assert set(got) == set(ref) == set(lib) and len(got) > 20
    worst = (0.0, 0.0, None)
    for n in ref:
        r = ref[n].abs().max().item()
        assert r > 0, n
        ek, el = (got[n] - ref[n]).abs().max().item() / r, (lib[n] - ref[n]).abs().max().item() / r
        if ek > worst[0]:
            worst = (ek, el, n)
        assert ek <= max(2.0 * el, FLOOR[torch.float32]), (n, ek, el)
    with capsys.disabled():
        print(f"\nvit module float32: worst kernel-path gradient error {worst[0]:.2e} x max (library path {worst[1]:.2e}) at {worst[2]}")
    # active attention dropout: the library path, no kernel; the same module in eval mode with grad enabled: the kernel
    md = _small_vit(attn_drop_rate=0.1).to(DEV).train()
    vit.CALLS.update(kernel=0, bwd_kernel=0)
    _grads(md, x0.to(DEV), w.to(DEV))
    assert vit.CALLS == {"kernel": 0, "bwd_kernel": 0}
    md.eval()
    _grads(md, x0.to(DEV), w.to(DEV))
    assert vit.CALLS == {"kernel": 2, "bwd_kernel": 2}
    with torch.no_grad():                                                              # inference keeps attend_gpu
        vit.CALLS.update(kernel=0, bwd_kernel=0)
        md(x0.to(DEV))
    assert vit.CALLS == {"kernel": 2, "bwd_kernel": 0}


def test_module_saves_nothing_of_size_n_squared(monkeypatch, capsys):
    """One attention module at B 2, N 2048, 12 heads, float32: forward + backward raise the peak of allocated memory by less than
    ONE [B, heads, N, N] float32 tensor (403 MB).  The path's own tensors come to about 160 MB were they all alive at once."""
    from ppnet_amd import vit
    B, N, heads = 2, 2048, 12
    torch.manual_seed(0)
    m = vit.MultiheadAttention(heads * 64, heads).to(DEV).train()

    def peak():
        x = torch.randn(B, N, heads * 64, device=DEV, requires_grad=True)
        dy = torch.randn(B, N, heads * 64, device=DEV)
        m.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        held = torch.cuda.memory_allocated()
        m(x, x.detach()).backward(dy)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - held
    peak()                                                                             # library workspaces allocated once
    vit.CALLS.update(kernel=0, bwd_kernel=0)
    rise = peak()
    assert vit.CALLS == {"kernel": 1, "bwd_kernel": 1}
    with monkeypatch.context() as mp:
        mp.setattr(vit.MultiheadAttention, "forward", _library_forward)
        peak()
        lib = peak()
    one_p = B * heads * N * N * 4
    with capsys.disabled():
        print(f"\nattention module B {B} N {N} heads {heads} float32: peak rise {rise / 1e6:.1f} MB on the kernel path, "
              f"{lib / 1e6:.1f} MB on nn.MultiheadAttention; one probabilities tensor {one_p / 1e6:.1f} MB")
    assert rise < one_p, (rise, one_p)


# ------------------------------------------------------------------------------------------------ training
def _codes(B, R, seed):
    g = torch.Generator().manual_seed(seed)
    lo = (torch.rand(B, 1, R // 16, R // 16, generator=g) > 0.4).float()
    return (torch.nn.functional.interpolate(lo, size=(R, R), mode="nearest")[:, 0] * 255).to(torch.uint8)


def _reduced_vit_setrup():
    from ppnet_amd import segnet
    cfg = copy.deepcopy(segnet.VIT_BASE_SETRUP)
    cfg["backbone"].update(img_size=128, embed_dims=128, num_layers=2, num_heads=2)
    cfg["decode_head"].update(in_channels=128, channels=32)
    return cfg


def test_segnet_vit_training_steps_use_the_mhsa_backward_kernel():
    """SGD + cross-entropy on (rendered map, mask_space) pairs from the generator for a small ViT + SETR-UP: every trainable
    parameter receives a finite gradient, each layer's attention backward runs on ppn_mhsa_bwd, 12 steps lower the loss."""
    from ppnet_amd import edage, train, vit
    from ppnet_amd.segnet import SegNet
    dev = torch.device("cuda:0")
    pb = edage.generate_paths(2, 128, 50, 3, seed=4, device=dev)
    mb = edage.generate_maps(pb, 3, 5, 20, seed=4)
    grid, space, path = train.generator_pairs(pb, mb, 3)
    torch.manual_seed(1)
    net = SegNet.from_config(_reduced_vit_setrup()).cuda()
    trainer = train.segnet_trainer(net)
    opt = train.segnet_optimizer(trainer, lr=0.02)
    sched = dict(warmup_iters=3, warmup_ratio=0.1)
    losses = []
    vit.CALLS.update(kernel=0, bwd_kernel=0)
    for it in range(12):
        losses.append(float(train.segnet_train_step(trainer, opt, it, 40, grid, space, schedule=sched)))
        if it == 0:
            assert vit.CALLS == {"kernel": 2, "bwd_kernel": 2}
            missing = [n for n, p in net.named_parameters() if p.requires_grad and p.grad is None]
            assert not missing, missing
            frozen = sorted(n for n, p in net.named_parameters() if not p.requires_grad)
            assert frozen == ["backbone.cls_token"], frozen                            # with_cls_token=False: never read
            assert all(torch.isfinite(p.grad).all() for p in net.parameters() if p.grad is not None)
            assert all(float(p.grad.abs().sum()) > 0 for n, p in net.named_parameters() if "in_proj_weight" in n)
    assert vit.CALLS == {"kernel": 24, "bwd_kernel": 24}
    assert all(l == l for l in losses) and losses[-1] < losses[0], losses


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_full_vit_base_setrup_training_step(dtype):
    """One step of the full VIT_BASE_SETRUP at R = 224 on 2 images: finite loss and gradients, 12 backward launches."""
    from ppnet_amd import segnet, train, vit
    torch.manual_seed(0)
    net = segnet.SegNet.from_config(segnet.VIT_BASE_SETRUP).to(DEV).to(dtype)
    trainer = train.segnet_trainer(net)
    opt = train.segnet_optimizer(trainer, lr=0.01)
    codes = _codes(2, 224, 5).to(DEV)
    labels = (codes > 0).to(torch.uint8)
    vit.CALLS.update(kernel=0, bwd_kernel=0)
    loss = train.segnet_train_step(trainer, opt, 0, 10, codes, labels, schedule=dict(warmup_iters=0))
    torch.cuda.synchronize()
    assert vit.CALLS == {"kernel": 12, "bwd_kernel": 12}
    assert bool(torch.isfinite(loss))
    grads = [(n, p.grad) for n, p in net.named_parameters() if p.requires_grad]
    assert all(g is not None for _, g in grads), [n for n, g in grads if g is None]
    assert all(bool(torch.isfinite(g).all()) for _, g in grads)
    assert all(bool(torch.isfinite(p).all()) for p in net.parameters())
