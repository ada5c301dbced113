"""Times GenNet's attention at head dim 8 and the AE-ViT training step (output kept under profiles/).

default      per launch, 3 heads of 8, float32 and bfloat16, at N = 784 and N = 1024 with batch 64 (one ViT block of a batch-64
             step at R 224 and at R 256 / 512): ppn_mhsa_fwd and ppn_mhsa_bwd (all three passes, one call) beside the forward and
             backward of F.scaled_dot_product_attention and of the explicit op chain (matmul, softmax, matmul under autograd) on
             the same tensors (the library forwards with autograd recording on a tensor that requires grad, as in a training step;
             ppn_mhsa_fwd is the same call in both modes); device events, every side warmed up, the sides alternated for three
             rounds in one process, the minimum of the rounds reported.  For information: which backend SDPA picked (the grad_fn of its output), whether two
             of its backward runs are bitwise equal, and the peak of allocated memory one forward + backward adds on each side.
--passes N B DTYPE
             30 calls of ppn_mhsa_fwd + ppn_mhsa_bwd at one shape and nothing else on the GPU: run under
             `rocprofv3 --kernel-trace --stats` for the per-pass split.
--step R DTYPE [--tree DIR]
             the whole training step (train.gennet_train_step, AEViT(1, 1, R, 24), batch 64; DTYPE float32, or bfloat16 =
             autocast) with the package imported from DIR (another checkout with its own built library, e.g. the parent commit's;
             default: this tree): ms per step over 6 steps after 3, and the peak of allocated memory.  PPNET_LIBRARY_ATTENTION=1
             in the environment selects the library's attention in this tree.  One process per run; alternate from the shell.
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else ROOT
sys.path.insert(0, os.path.abspath(TREE))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from ppnet_amd import _lib as L  # noqa: E402
from ppnet_amd import train, vit  # noqa: E402
from ppnet_amd.gennet import AEViT  # noqa: E402

dev = torch.device("cuda", 0)
HEADS, HD, BATCH = 3, 8, 64
C, SCALE = HEADS * HD, HD ** -0.5
DT = {"bfloat16": torch.bfloat16, "float32": torch.float32}
P = lambda t: ctypes.c_void_p(t.data_ptr())


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernel_calls(qkv, dout):
    B, N, _ = qkv.shape
    need = L.lib.ppn_mhsa_bwd_workspace(B, N, HEADS)
    out, dqkv = torch.empty(B, N, C, dtype=qkv.dtype, device=dev), torch.empty_like(qkv)
    ws = torch.empty(need, dtype=torch.float32, device=dev)
    dt = 0 if qkv.dtype == torch.float32 else 1
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fwd():
        L.check(L.lib.ppn_mhsa_fwd(P(qkv), P(out), B, N, HEADS, HD, SCALE, dt, stream()), "ppn_mhsa_fwd")

    def bwd():
        L.check(L.lib.ppn_mhsa_bwd(P(qkv), P(out), P(dout), P(dqkv), P(ws), need, B, N, HEADS, HD, SCALE, dt, stream()), "ppn_mhsa_bwd")
    return fwd, bwd


def heads_of(t):
    B, N, _ = t.shape
    return t.view(B, N, 3, HEADS, HD).permute(2, 0, 3, 1, 4).unbind(0)


def chain_of(t):
    q, k, v = heads_of(t)
    return (torch.softmax((q @ k.transpose(-2, -1)) * SCALE, dim=-1) @ v).transpose(1, 2).reshape(t.shape[0], t.shape[1], C)


def sdpa_of(t):
    q, k, v = heads_of(t)
    return F.scaled_dot_product_attention(q, k, v, scale=SCALE).transpose(1, 2).reshape(t.shape[0], t.shape[1], C)


def sdpa_backend(y):
    """The attention node of y's autograd graph: its name tells which SDPA backend ran (none: the decomposed math backend)."""
    seen, todo = [], [y.grad_fn]
    while todo:
        f = todo.pop()
        if f is None:
            continue
        name = type(f).__name__
        if "Attention" in name or "ScaledDot" in name:
            return name
        seen.append(name)
        todo.extend(g for g, _ in f.next_functions)
    return "math (decomposed: " + ", ".join(n for n in seen if "Softmax" in n or "Bmm" in n or "Mm" in n) + ")"


def peak_rise(fn):
    """Peak of allocated memory that one forward + backward adds to what is held before it."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - held) / 1e6


def launch_table():
    for dtype in (torch.float32, torch.bfloat16):
        for N in (784, 1024):
            B = BATCH
            qkv = torch.randn(B, N, 3 * C, device=dev).to(dtype)
            dout = torch.randn(B, N, C, device=dev).to(dtype)
            kf, kb = kernel_calls(qkv, dout)
            t = qkv.detach().clone().requires_grad_(True)
            oc, os_ = chain_of(t), sdpa_of(t)
            backend = sdpa_backend(os_)
            rec = lambda f: (lambda: f(t))                    # the library forwards record the graph, as a training step's do
            sides = (("ppn fwd", kf, 20), ("sdpa fwd", rec(sdpa_of), 10), ("chain fwd", rec(chain_of), 5),
                     ("ppn bwd", kb, 20), ("sdpa bwd", lambda: torch.autograd.grad(os_, t, dout, retain_graph=True), 10),
                     ("chain bwd", lambda: torch.autograd.grad(oc, t, dout, retain_graph=True), 5))
            for _, fn, _ in sides:
                for _ in range(2):
                    fn()
            best = {}
            for _ in range(3):
                for name, fn, reps in sides:
                    best[name] = min(best.get(name, 1e9), timed(fn, reps))
            sb = sides[4][1]
            same = torch.equal(sb()[0], sb()[0])
            del oc, os_, sides, sb
            mem = {}
            for name, f in (("ppn", lambda u: vit.mhsa_autograd(u, HEADS, SCALE)), ("sdpa", sdpa_of), ("chain", chain_of)):
                def run(f=f):
                    u = qkv.detach().clone().requires_grad_(True)
                    f(u).backward(dout)
                run()
                mem[name] = peak_rise(run)
            exps = 1.0 * B * HEADS * N * N
            print(f"{str(dtype)[6:]:8s} N {N:4d} batch {B}: forward ppn_mhsa_fwd {best['ppn fwd']:7.4f} ms ({exps / best['ppn fwd'] / 1e9:6.1f} T exp/s) | "
                  f"sdpa {best['sdpa fwd']:7.4f} ms ({best['sdpa fwd'] / best['ppn fwd']:5.2f}x) | chain {best['chain fwd']:7.4f} ms "
                  f"({best['chain fwd'] / best['ppn fwd']:5.2f}x)", flush=True)
            print(f"{'':8s} {'':6s} {'':8s}  backward ppn_mhsa_bwd {best['ppn bwd']:7.4f} ms ({3 * exps / best['ppn bwd'] / 1e9:6.1f} T exp/s) | "
                  f"sdpa {best['sdpa bwd']:7.4f} ms ({best['sdpa bwd'] / best['ppn bwd']:5.2f}x) | chain {best['chain bwd']:7.4f} ms "
                  f"({best['chain bwd'] / best['ppn bwd']:5.2f}x)", flush=True)
            print(f"{'':8s} {'':6s} {'':8s}  sdpa backend (grad_fn) {backend}, two sdpa backward runs bitwise equal: {same}; forward + backward "
                  f"peak rise: ppn {mem['ppn']:.1f} MB, sdpa {mem['sdpa']:.1f} MB, chain {mem['chain']:.1f} MB "
                  f"(one probabilities tensor {exps * qkv.element_size() / 1e6:.1f} MB)", flush=True)
            del qkv, dout, t, kf, kb
            torch.cuda.empty_cache()


if "--passes" in sys.argv:
    i = sys.argv.index("--passes")
    N, B, dtype = int(sys.argv[i + 1]), int(sys.argv[i + 2]), DT[sys.argv[i + 3]]
    qkv = torch.randn(B, N, 3 * C, device=dev).to(dtype)
    dout = torch.randn(B, N, C, device=dev).to(dtype)
    kf, kb = kernel_calls(qkv, dout)
    for _ in range(30):
        kf()
        kb()
    torch.cuda.synchronize()
    print(f"30 x ppn_mhsa_fwd + ppn_mhsa_bwd head dim 8 {sys.argv[i + 3]} N {N} batch {B} done", flush=True)
elif "--step" in sys.argv:
    i = sys.argv.index("--step")
    R, amp = int(sys.argv[i + 1]), {"float32": None, "bfloat16": torch.bfloat16}[sys.argv[i + 2]]
    torch.manual_seed(0)
    net = AEViT(1, 1, img_resolution=R, dim=24).to(dev)
    opt = train.gennet_optimizer(net)
    space = (torch.rand(BATCH, R, R, device=dev) > 0.4).to(torch.uint8)
    path = ((torch.rand(BATCH, R, R, device=dev) > 0.9).to(torch.uint8) * 255)
    step = lambda: train.gennet_train_step(net, opt, None, space, path, amp_dtype=amp)
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ms = timed(step, 6)
    calls = getattr(vit, "CALLS", {})
    which = "library attention" if os.environ.get("PPNET_LIBRARY_ATTENTION") else "default"
    print(f"tree {os.path.relpath(os.path.abspath(TREE), ROOT):18s} {which:17s} AEViT train step R {R} batch {BATCH} {sys.argv[i + 2]:8s}: {ms:8.2f} ms per step, "
          f"peak allocated {torch.cuda.max_memory_allocated() / 2 ** 20:8.0f} MiB, ppn_mhsa_fwd / bwd launches {calls.get('kernel')} / {calls.get('bwd_kernel')}",
          flush=True)
else:
    launch_table()
