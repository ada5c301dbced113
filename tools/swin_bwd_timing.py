"""Times Swin's window-attention backward and the Swin-B + UPerHead training step (output kept under profiles/).

default      per launch on the four Swin-B levels at R = 256, shift 0 and 3, bfloat16 at batch 256 and float32 at batch
             SWIN_BWD_F32_BATCH (default 64): ppn_swin_wmsa_bwd beside the backward of the torch composition
             (swin.window_attention under autograd) on the same tensors, and forward + backward of swin.wmsa_autograd beside forward
             + backward of the composition; device events, every shape warmed up, the sides alternated for three rounds in one
             process, the minimum of the rounds reported.  The HBM fraction is on the compulsory 7 C elements per real token (qkv
             and dout read, dqkv written: 14 C bytes in bfloat16) at 8 TB/s.
--passes SIDE B DTYPE SHIFT
             30 calls of ppn_swin_wmsa_bwd at one level (SIDE = 64 / 32 / 16 / 8) and nothing else on the GPU: run under
             `rocprofv3 --kernel-trace --stats` for the split between the main and the reduction kernel.
--step R DTYPE [--tree DIR]
             the whole training step (train.segnet_train_step, SWIN_BASE_UPER, 8 images at R x R) with the package imported from DIR
             (another checkout with its own built library, e.g. the parent commit's; default: this tree): ms per step over 6 steps
             after 3, and the peak of allocated memory.  One process per side; alternate the sides from the shell.
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
from ppnet_amd import segnet, swin, train  # noqa: E402

dev = torch.device("cuda", 0)
SCALE = 32 ** -0.5
DT = {"bfloat16": torch.bfloat16, "float32": torch.float32}
LEVELS = {64: (128, 4), 32: (256, 8), 16: (512, 16), 8: (1024, 32)}      # grid side at R = 256 -> (channels, heads)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def level_inputs(side, B, dtype):
    C, heads = LEVELS[side]
    qkv = torch.randn(B, side, side, 3 * C, device=dev).to(dtype)
    pad = (torch.randn(3 * C, device=dev) * 0.2).to(dtype)
    rpb = torch.randn(heads, 13, 13, device=dev)
    dout = torch.randn(B, side, side, C, device=dev).to(dtype)
    return qkv, pad, rpb, dout, heads


def bwd_call(qkv, pad, rpb, dout, heads, shift):
    B, H, W, _ = qkv.shape
    need = L.lib.ppn_swin_wmsa_bwd_workspace(B, H, W, heads)
    dqkv = torch.empty_like(qkv)
    dpad = torch.empty(pad.numel(), dtype=torch.float32, device=dev)
    drpb, ws = torch.empty_like(rpb), torch.empty(need, dtype=torch.float32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    dt = 0 if qkv.dtype == torch.float32 else 1

    def call():
        L.check(L.lib.ppn_swin_wmsa_bwd(p(qkv), p(pad), p(rpb), p(dout), p(dqkv), p(dpad), p(drpb), p(ws), need, B, H, W, heads, 7, shift, SCALE, dt,
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "ppn_swin_wmsa_bwd")
    return call, (dqkv, dpad, drpb, ws)


def codes(B, R):
    c = (torch.rand(B, R // 16, R // 16, device=dev) > 0.4).float()
    return (F.interpolate(c[:, None], size=(R, R), mode="nearest")[:, 0] * 255).to(torch.uint8)


def trainer_for(dtype):
    torch.manual_seed(0)
    net = segnet.SegNet.from_config(segnet.SWIN_BASE_UPER).to(dev).to(dtype)
    tr = train.segnet_trainer(net)
    return tr, train.segnet_optimizer(tr, lr=0.01)


def launch_table():
    for dtype, B in ((torch.bfloat16, 256), (torch.float32, int(os.environ.get("SWIN_BWD_F32_BATCH", "64")))):
        for side in (64, 32, 16, 8):
            qkv, pad, rpb, dout, heads = level_inputs(side, B, dtype)
            C = LEVELS[side][0]
            byts = B * side * side * 7 * C * qkv.element_size()
            for shift in (0, 3):
                kern, keep = bwd_call(qkv, pad, rpb, dout, heads, shift)
                q = qkv.detach().clone().requires_grad_(True)
                pp = pad.detach().clone().requires_grad_(True)
                t = rpb.to(dtype).reshape(heads, 169).t().contiguous().requires_grad_(True)
                oc = swin.window_attention(q, pp, t, heads, shift, SCALE)
                chain = lambda: torch.autograd.grad(oc, (q, pp, t), dout, retain_graph=True)
                both_k = lambda: torch.autograd.grad(swin.wmsa_autograd(q, pp, t, heads, shift, SCALE), (q, pp, t), dout)
                both_c = lambda: torch.autograd.grad(swin.window_attention(q, pp, t, heads, shift, SCALE), (q, pp, t), dout)
                sides = (("bwd", kern, 20), ("chain bwd", chain, 3), ("fwd+bwd", both_k, 10), ("chain fwd+bwd", both_c, 3))
                for _, fn, _ in sides:
                    for _ in range(2):
                        fn()
                best = {}
                for _ in range(3):
                    for name, fn, reps in sides:
                        best[name] = min(best.get(name, 1e9), timed(fn, reps))
                mk = best["bwd"]
                print(f"{str(dtype)[6:]:8s} level {side:3d}x{side:<3d} C {C:4d} heads {heads:2d} batch {B:3d} shift {shift}: ppn_swin_wmsa_bwd {mk:8.4f} ms "
                      f"hbm-time frac {byts / 8e12 * 1e3 / mk:5.2f} | chain backward {best['chain bwd']:8.3f} ms ({best['chain bwd'] / mk:6.1f}x) | "
                      f"wmsa_autograd fwd+bwd {best['fwd+bwd']:8.4f} ms, chain fwd+bwd {best['chain fwd+bwd']:8.3f} ms "
                      f"({best['chain fwd+bwd'] / best['fwd+bwd']:6.1f}x)", flush=True)
                del kern, keep, q, pp, t, oc, chain, both_k, both_c, sides
                torch.cuda.empty_cache()
            del qkv, dout


if "--passes" in sys.argv:
    i = sys.argv.index("--passes")
    side, B, dtype, shift = int(sys.argv[i + 1]), int(sys.argv[i + 2]), DT[sys.argv[i + 3]], int(sys.argv[i + 4])
    qkv, pad, rpb, dout, heads = level_inputs(side, B, dtype)
    kern, keep = bwd_call(qkv, pad, rpb, dout, heads, shift)
    for _ in range(30):
        kern()
    torch.cuda.synchronize()
    print(f"30 x ppn_swin_wmsa_bwd {sys.argv[i + 3]} level {side} batch {B} shift {shift} done", flush=True)
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
    bwd = getattr(swin, "TRAIN_CALLS", {}).get("bwd_kernel")
    print(f"tree {os.path.relpath(os.path.abspath(TREE), ROOT):12s} SWIN_BASE_UPER train step R {R} 8 images {sys.argv[i + 2]:8s}: {ms:8.2f} ms per step, "
          f"peak allocated {torch.cuda.max_memory_allocated() / 2 ** 20:8.0f} MiB, ppn_swin_wmsa_bwd launches {bwd}", flush=True)
elif "--trace-step" in sys.argv:
    tr, opt = trainer_for(torch.bfloat16)
    grid = codes(8, 224)
    labels = (grid > 0).to(torch.uint8)
    for it in range(3):
        train.segnet_train_step(tr, opt, it, 100, grid, labels, schedule=dict(warmup_iters=0))
    torch.cuda.synchronize()
    print("3 bfloat16 training steps at R 224, 8 images done", flush=True)
else:
    launch_table()
