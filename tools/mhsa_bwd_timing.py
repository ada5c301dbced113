"""Times ViT's attention backward and the ViT-B + SETR-UP training step (output kept under profiles/).

default      per layer, 12 heads of 64, bfloat16 and float32, at N = 256 batch 256, N = 1024 batch 64 (section 11's shapes) and
             N = 196 batch 64: ppn_mhsa_bwd (all three passes, one call) beside the backward of the explicit op chain (matmul,
             softmax, matmul under autograd) and of F.scaled_dot_product_attention on the same tensors; device events, every
             shape warmed up, the three sides alternated for three rounds in one process, the minimum of the rounds reported.
             The FLOP rate is given twice: on the 16 B heads N^2 64 the three passes EXECUTE (S and dP are formed in both the
             dK / dV and the dQ pass, S once more in the statistics pass: 2 + 8 + 6) and on the 10 the algorithm NEEDS.
             Whether two SDPA backward runs are bitwise equal is printed for information.
--passes N B DTYPE
             30 calls of ppn_mhsa_bwd at one shape and nothing else on the GPU: run under `rocprofv3 --kernel-trace --stats` for
             the per-pass split.
--step R DTYPE [--tree DIR]
             the whole training step (train.segnet_train_step, VIT_BASE_SETRUP, 8 images at R x R) with the package imported
             from DIR (another checkout with its own built library, e.g. the parent commit's; default: this tree): ms per step
             over 6 steps after 3, and the peak of allocated memory.  One process per side; alternate the sides from the shell.
--trace-step three bfloat16 training steps at R = 224, 8 images (for `rocprofv3 --kernel-trace --stats`).
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
from ppnet_amd import segnet, train, vit  # noqa: E402

dev = torch.device("cuda", 0)
HEADS, C, SCALE = 12, 768, 64 ** -0.5
DT = {"bfloat16": torch.bfloat16, "float32": torch.float32}


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def bwd_call(qkv, out, dout):
    B, N, _ = qkv.shape
    need = L.lib.ppn_mhsa_bwd_workspace(B, N, HEADS)
    dqkv, ws = torch.empty_like(qkv), torch.empty(need, dtype=torch.float32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    dt = 0 if qkv.dtype == torch.float32 else 1

    def call():
        L.check(L.lib.ppn_mhsa_bwd(p(qkv), p(out), p(dout), p(dqkv), p(ws), need, B, N, HEADS, 64, SCALE, dt,
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "ppn_mhsa_bwd")
    return call, dqkv


def codes(B, R):
    c = (torch.rand(B, R // 16, R // 16, device=dev) > 0.4).float()
    return (F.interpolate(c[:, None], size=(R, R), mode="nearest")[:, 0] * 255).to(torch.uint8)


def trainer_for(dtype):
    torch.manual_seed(0)
    net = segnet.SegNet.from_config(segnet.VIT_BASE_SETRUP).to(dev).to(dtype)
    tr = train.segnet_trainer(net)
    return tr, train.segnet_optimizer(tr, lr=0.01)


def layer_table():
    for dtype in (torch.bfloat16, torch.float32):
        for N, B in ((256, 256), (1024, 64), (196, 64)):
            qkv = torch.randn(B, N, 3 * C, device=dev).to(dtype)
            dout = torch.randn(B, N, C, device=dev).to(dtype)
            with torch.no_grad():
                out = vit.mhsa_forward(qkv, HEADS, SCALE)
            kern, _ = bwd_call(qkv, out, dout)
            t = qkv.detach().clone().requires_grad_(True)
            q, k, v = t.view(B, N, 3, HEADS, 64).permute(2, 0, 3, 1, 4).unbind(0)
            oc = (torch.softmax((q @ k.transpose(-2, -1)) * SCALE, dim=-1) @ v).transpose(1, 2).reshape(B, N, C)
            os_ = F.scaled_dot_product_attention(q, k, v, scale=SCALE).transpose(1, 2).reshape(B, N, C)
            chain = lambda: torch.autograd.grad(oc, t, dout, retain_graph=True)
            sdpa = lambda: torch.autograd.grad(os_, t, dout, retain_graph=True)
            sides = (("ppn_mhsa_bwd", kern, 20), ("chain backward", chain, 5), ("sdpa backward", sdpa, 10))
            for _, fn, _ in sides:
                for _ in range(2):
                    fn()
            best = {}
            for _ in range(3):
                for name, fn, reps in sides:
                    best[name] = min(best.get(name, 1e9), timed(fn, reps))
            same = torch.equal(sdpa()[0], sdpa()[0])
            f16, f10 = 16.0 * B * HEADS * N * N * 64, 10.0 * B * HEADS * N * N * 64
            mk = best["ppn_mhsa_bwd"]
            print(f"{str(dtype)[6:]:8s} N {N:4d} batch {B:3d}: ppn_mhsa_bwd {mk:8.4f} ms per layer "
                  f"({f16 / mk / 1e9:7.1f} TFLOP/s executed, {f10 / mk / 1e9:7.1f} TFLOP/s needed) | chain backward {best['chain backward']:8.4f} ms "
                  f"({best['chain backward'] / mk:5.2f}x) | sdpa backward {best['sdpa backward']:8.4f} ms ({best['sdpa backward'] / mk:5.2f}x), "
                  f"two runs bitwise equal: {same}", flush=True)
            del qkv, dout, out, t, q, k, v, oc, os_, kern, chain, sdpa, sides
            torch.cuda.empty_cache()


if "--passes" in sys.argv:
    i = sys.argv.index("--passes")
    N, B, dtype = int(sys.argv[i + 1]), int(sys.argv[i + 2]), DT[sys.argv[i + 3]]
    qkv = torch.randn(B, N, 3 * C, device=dev).to(dtype)
    dout = torch.randn(B, N, C, device=dev).to(dtype)
    with torch.no_grad():
        out = vit.mhsa_forward(qkv, HEADS, SCALE)
    kern, _ = bwd_call(qkv, out, dout)
    for _ in range(30):
        kern()
    torch.cuda.synchronize()
    print(f"30 x ppn_mhsa_bwd {sys.argv[i + 3]} N {N} batch {B} done", flush=True)
elif "--step" in sys.argv:
    i = sys.argv.index("--step")
    R, dtype = int(sys.argv[i + 1]), DT[sys.argv[i + 2]]
    tr, opt = trainer_for(dtype)
    grid = codes(8, R)
    labels = (grid > 0).to(torch.uint8)
    step = lambda it=0: train.segnet_train_step(tr, opt, it, 100, grid, labels, schedule=dict(warmup_iters=0))
    for it in range(3):
        step(it)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ms = timed(step, 6)
    bwd = getattr(vit, "CALLS", {}).get("bwd_kernel")
    print(f"tree {os.path.relpath(os.path.abspath(TREE), ROOT):12s} VIT_BASE_SETRUP train step R {R} 8 images {sys.argv[i + 2]:8s}: {ms:8.2f} ms per step, "
          f"peak allocated {torch.cuda.max_memory_allocated() / 2 ** 20:8.0f} MiB, ppn_mhsa_bwd launches {bwd}", flush=True)
elif "--trace-step" in sys.argv:
    tr, opt = trainer_for(torch.bfloat16)
    grid = codes(8, 224)
    labels = (grid > 0).to(torch.uint8)
    for it in range(3):
        train.segnet_train_step(tr, opt, it, 100, grid, labels, schedule=dict(warmup_iters=0))
    torch.cuda.synchronize()
    print("3 bfloat16 training steps at R 224, 8 images done", flush=True)
else:
    layer_table()
