"""Times the training kernels of GenNet's 24 -> 24 stride-2 stages and the AE-ViT training step (output kept in
profiles/gennet_s2_timing.txt).

default      each stage's convolution alone, forward + backward through autograd (fused.conv_s2 on the stage's Conv2d(24, 24, 3, 2, 1) or
             ConvTranspose2d(24, 24, 3, 2, 1, output_padding=1), out.backward(d) with a fixed d and an x that requires grad): the
             int(log2(R // 28)) encoder and as many decoder stages of AEViT(1, 1, R, 24) at batch 64, R 224 / 256 / 512 and batch 8, R 224,
             float32 and bfloat16 autocast (bfloat16 x), with the measured gates open; the kernel path beside the library (PPNET_LIBRARY_S2=1, read at call time) on the
             same tensors; device events, both sides warmed up, the sides alternated for three rounds in one process, the minimum of the
             rounds reported, and the kernel side measured a second time in every round: the difference of its two minima is the spread.
             Bytes per stage from the shapes (3.75 T: the big tensor T and the small one T / 4, each touched once forward, once for the
             data gradient and once for the weight gradient); achieved bytes/s and the share of the 6.29 TB/s copy rate are the kernel
             path's.
--passes B R DTYPE
             30 calls of ppn_gennet_s2_down + ppn_gennet_s2_up + ppn_gennet_s2_wgrad at one big extent R x R and nothing else on the GPU:
             run under `rocprofv3 --kernel-trace --stats` for the per-kernel split.
--step R DTYPE [--tree DIR] [--open]
             the whole training step (train.gennet_train_step, AEViT(1, 1, R, 24), batch 64; DTYPE float32, or bfloat16 = autocast) with
             the package imported from DIR (another checkout with its own built library, e.g. the parent commit's; default: this tree):
             ms per step over 6 steps after 3, and the peak of allocated memory.  PPNET_LIBRARY_S2=1 in the environment selects the
             library stages in this tree; --open opens the measured gates (fused.S2_RECORD_MIN, fused.S2_DTYPES), so that a gated data type
             or size runs on the kernels.  One process per run; alternate from the shell.  Under `rocprofv3 --kernel-trace --stats` the
             same run gives the per-kernel split of a step.
"""
import math
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
KNOB = "PPNET_LIBRARY_S2"


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def open_gates():
    """The measured gates of fused.conv_s2_ok opened: every size and both data types take the kernels (what sets the gates is measured so)."""
    fused.S2_RECORD_MIN = 0
    fused.S2_DTYPES = frozenset({torch.float32, torch.bfloat16})


def stage_table():
    open_gates()
    for amp in (None, torch.bfloat16):
        for B, R in ((64, 224), (64, 256), (64, 512), (8, 224)):
            n_down = int(math.log2(R // 28))
            stages = [("enc", i, R >> i) for i in range(n_down)] + [("dec", i, R >> (n_down - 1 - i)) for i in range(n_down)]
            total = {"kernel": 0.0, "library": 0.0}
            for kind, idx, big in stages:                                      # big: the extent of the stage's big side
                up = kind == "dec"
                torch.manual_seed(0)
                conv = (nn.ConvTranspose2d(C, C, 3, 2, 1, output_padding=1) if up else nn.Conv2d(C, C, 3, 2, 1)).to(dev)
                xe, ye = (big // 2, big) if up else (big, big // 2)
                x = torch.randn(B, C, xe, xe, device=dev).to(amp or torch.float32).requires_grad_(True)
                d = torch.randn(B, C, ye, ye, device=dev).to(amp or torch.float32)

                def step(library):
                    if library:
                        os.environ[KNOB] = "1"
                    else:
                        os.environ.pop(KNOB, None)
                    with torch.autocast("cuda", dtype=amp, enabled=amp is not None):
                        out = fused.conv_s2(x, conv)
                    out.backward(d)
                    x.grad = None
                sides = (("kernel", lambda: step(False)), ("library", lambda: step(True)), ("kernel again", lambda: step(False)))
                calls = dict(fused.S2_CALLS)
                for _, fn in sides:
                    for _ in range(3):
                        fn()
                took = fused.S2_CALLS["wgrad"] == calls["wgrad"] + 6
                assert took or B * C * big * big < fused.S2_RECORD_MIN, "the kernel side did not take the kernels"
                reps = 10 if B * big * big <= 64 * 256 * 256 else 4
                best = {}
                for _ in range(3):
                    for name, fn in sides:
                        best[name] = min(best.get(name, 1e9), timed(fn, reps))
                os.environ.pop(KNOB, None)
                T = B * C * big * big * x.element_size()
                nbytes = 3.75 * T
                k = min(best["kernel"], best["kernel again"])
                total["kernel"] += k
                total["library"] += best["library"]
                print(f"{'bf16 autocast' if amp else 'float32':13s} batch {B:2d} R {R:3d} {kind}_conv[{idx}] big {big:3d}: kernel {best['kernel']:7.3f} / "
                      f"{best['kernel again']:7.3f} ms (spread {abs(best['kernel'] - best['kernel again']):.3f}) | library {best['library']:7.3f} ms "
                      f"({best['library'] / k:5.2f}x) | {nbytes / 1e6:7.1f} MB from the shapes: {nbytes / k / 1e9:6.2f} TB/s = "
                      f"{100 * nbytes / k * 1e3 / COPY_RATE:4.1f} % of the copy rate"
                      f"{'' if took else ' | below S2_RECORD_MIN: both sides are the library'}", flush=True)
                del conv, x, d, sides
                torch.cuda.empty_cache()
            print(f"{'bf16 autocast' if amp else 'float32':13s} batch {B:2d} R {R:3d} all {len(stages)} stages: kernel {total['kernel']:7.3f} ms | library "
                  f"{total['library']:7.3f} ms ({total['library'] / total['kernel']:5.2f}x)", flush=True)


if "--passes" in sys.argv:
    i = sys.argv.index("--passes")
    B, R, dtype = int(sys.argv[i + 1]), int(sys.argv[i + 2]), {"float32": torch.float32, "bfloat16": torch.bfloat16}[sys.argv[i + 3]]
    torch.manual_seed(0)
    w, b = torch.randn(C, C, 3, 3, device=dev) / 15, torch.randn(C, device=dev)
    big = torch.randn(B, C, R, R, device=dev).to(dtype)
    small = torch.randn(B, C, (R + 1) // 2, (R + 1) // 2, device=dev).to(dtype)
    for _ in range(30):
        fused._s2_down(big, w, b)
        fused._s2_up(small, w, b, R, R)
        fused._s2_wgrad(small, big)
    torch.cuda.synchronize()
    print(f"30 x ppn_gennet_s2_down + ppn_gennet_s2_up + ppn_gennet_s2_wgrad {sys.argv[i + 3]} batch {B} big {R} x {R} done", flush=True)
elif "--step" in sys.argv:
    i = sys.argv.index("--step")
    R, amp = int(sys.argv[i + 1]), {"float32": None, "bfloat16": torch.bfloat16}[sys.argv[i + 2]]
    if "--open" in sys.argv:
        open_gates()
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
    loss = float(step())
    calls = getattr(fused, "S2_CALLS", {})
    which = "library stages" if os.environ.get(KNOB) else ("gates open" if "--open" in sys.argv else "default")
    print(f"tree {os.path.relpath(os.path.abspath(TREE), ROOT):18s} {which:14s} AEViT train step R {R} batch {BATCH} {sys.argv[i + 2]:8s}: {ms:8.2f} ms per step, "
          f"peak allocated {torch.cuda.max_memory_allocated() / 2 ** 20:8.0f} MiB, loss after 10 steps {loss:.6f}, stage launches down / up / wgrad "
          f"{calls.get('down')} / {calls.get('up')} / {calls.get('wgrad')}", flush=True)
else:
    stage_table()
