"""Times the training pair of GenNet's tail and the AE-ViT training step (output kept in
profiles/gennet_tail_timing.txt).

default      the tail alone, forward + backward through autograd (fused.tail_bn_act_conv on BatchNorm2d(24) + LeakyReLU + Conv2d(24, 1, 3, 1,
             1), out.backward(d) with a fixed d and a y that requires grad): batch 64 at R 224 / 256 / 512 and batch 8 at R 224, float32 and
             bfloat16 autocast (a bfloat16 y, what the last transposed convolution gives there); the kernel path beside the library
             composition (PPNET_LIBRARY_TAIL=1, read at call time) on the same tensors; device events, both sides warmed up, the sides
             alternated for three rounds in one process, the minimum of the rounds reported, and the kernel side measured a second time
             in every round: the difference of its two minima is the spread.  Bytes per step from the shapes (5 T: y read twice forward,
             twice backward, dy written once; out and d are T / 24 each and left out); achieved bytes/s and the share of the 6.29 TB/s copy
             rate are the kernel path's.  Peak of allocated memory one forward + backward adds, per side.
--passes B R DTYPE
             30 calls of ppn_gennet_tail_train_fwd + ppn_gennet_tail_train_bwd at one shape and nothing else on the GPU: run under
             `rocprofv3 --kernel-trace --stats` for the per-kernel split.
--step R DTYPE [--tree DIR]
             the whole training step (train.gennet_train_step, AEViT(1, 1, R, 24), batch 64; DTYPE float32, or bfloat16 = autocast) with
             the package imported from DIR (another checkout with its own built library, e.g. the parent commit's; default: this tree):
             ms per step over 6 steps after 3, and the peak of allocated memory.  PPNET_LIBRARY_TAIL=1 in the environment selects the
             library tail in this tree.  One process per run; alternate from the shell.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else ROOT
sys.path.insert(0, os.path.abspath(TREE))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from ppnet_amd import fused, train  # noqa: E402
from ppnet_amd.gennet import AEViT  # noqa: E402

dev = torch.device("cuda", 0)
C, BATCH, COPY_RATE = 24, 64, 6.29e12
KNOB = "PPNET_LIBRARY_TAIL"


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def peak_rise(fn):
    """Peak of allocated memory that one forward + backward adds to what is held before it."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - held) / 2 ** 20


def tail_table():
    for amp in (None, torch.bfloat16):
        for B, R in ((64, 224), (64, 256), (64, 512), (8, 224)):
            torch.manual_seed(0)
            bn, conv = nn.BatchNorm2d(C).to(dev), nn.Conv2d(C, 1, 3, 1, 1).to(dev)
            y = (0.5 + 1.5 * torch.randn(B, C, R, R, device=dev)).to(amp or torch.float32).requires_grad_(True)
            d = torch.randn(B, 1, R, R, device=dev).to(amp or torch.float32)

            def step(library):
                if library:
                    os.environ[KNOB] = "1"
                else:
                    os.environ.pop(KNOB, None)
                with torch.autocast("cuda", dtype=amp, enabled=amp is not None):
                    out = fused.tail_bn_act_conv(y, bn, 0.01, conv)
                out.backward(d)
                y.grad = None
            sides = (("kernel", lambda: step(False)), ("library", lambda: step(True)), ("kernel again", lambda: step(False)))
            calls = dict(fused.TAIL_CALLS)
            for _, fn in sides:
                for _ in range(3):
                    fn()
            took = fused.TAIL_CALLS["fwd"] == calls["fwd"] + 6 and fused.TAIL_CALLS["bwd"] == calls["bwd"] + 6      # the gate held
            assert took or y.numel() < fused.TAIL_RECORD_MIN, "the kernel side did not take the kernels"
            reps = 20 if B * R * R <= 64 * 256 * 256 else 8
            best = {}
            for _ in range(3):
                for name, fn in sides:
                    best[name] = min(best.get(name, 1e9), timed(fn, reps))
            mem = {name: peak_rise(fn) for name, fn in sides[:2]}
            os.environ.pop(KNOB, None)
            T = B * C * R * R * y.element_size()
            nbytes = 5 * T
            k = min(best["kernel"], best["kernel again"])
            print(f"{'bf16 autocast' if amp else 'float32':13s} batch {B:2d} R {R:3d}: kernel {best['kernel']:7.3f} / {best['kernel again']:7.3f} ms "
                  f"(spread {abs(best['kernel'] - best['kernel again']):.3f}) | library {best['library']:7.3f} ms ({best['library'] / k:5.2f}x) | "
                  f"{nbytes / 1e6:7.1f} MB per step from the shapes: {nbytes / k / 1e9:6.2f} TB/s = {100 * nbytes / k * 1e3 / COPY_RATE:4.1f} % of the copy "
                  f"rate | forward + backward peak rise: kernel {mem['kernel']:.0f} MiB, library {mem['library']:.0f} MiB (T = {T / 2 ** 20:.0f} MiB)"
                  f"{'' if took else ' | below TAIL_RECORD_MIN: both sides are the library'}", flush=True)
            del bn, conv, y, d, sides
            torch.cuda.empty_cache()


if "--passes" in sys.argv:
    i = sys.argv.index("--passes")
    B, R, dtype = int(sys.argv[i + 1]), int(sys.argv[i + 2]), {"float32": torch.float32, "bfloat16": torch.bfloat16}[sys.argv[i + 3]]
    torch.manual_seed(0)
    bn, conv = nn.BatchNorm2d(C).to(dev), nn.Conv2d(C, 1, 3, 1, 1).to(dev)
    ps = [p.detach() for p in (bn.weight, bn.bias, conv.weight, conv.bias)]
    y = (0.5 + 1.5 * torch.randn(B, C, R, R, device=dev)).to(dtype)
    d = torch.randn(B, 1, R, R, device=dev).to(dtype)
    for _ in range(30):
        out, stats = fused._tail_fwd(y, *ps, 1e-5, 0.01)
        fused._tail_bwd(d, y, ps[0], ps[1], ps[2], stats, 0.01)
    torch.cuda.synchronize()
    print(f"30 x ppn_gennet_tail_train_fwd + ppn_gennet_tail_train_bwd {sys.argv[i + 3]} batch {B} R {R} done", flush=True)
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
    calls = getattr(fused, "TAIL_CALLS", {})
    which = "library tail" if os.environ.get(KNOB) else "default"
    print(f"tree {os.path.relpath(os.path.abspath(TREE), ROOT):18s} {which:12s} AEViT train step R {R} batch {BATCH} {sys.argv[i + 2]:8s}: {ms:8.2f} ms per step, "
          f"peak allocated {torch.cuda.max_memory_allocated() / 2 ** 20:8.0f} MiB, tail launches fwd / bwd {calls.get('fwd')} / {calls.get('bwd')}",
          flush=True)
else:
    tail_table()
