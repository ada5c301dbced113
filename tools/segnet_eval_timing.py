"""Times the SegNet evaluation — bilinear resize + argmax + the three per-class area histograms — beside the library composition in the
same process (output kept under profiles/).

bare   ppn_seg_eval (fused.seg_eval, areas only) on 8 images with 512 x 512 uint8 labels, about 10 % ignored, from logits 256 x 256
       (SETR-UP), 128 x 128 (UPerHead / UPerPUP) and 32 x 32 (the auxiliary head's resolution), float32 and bfloat16, C = 2 (the
       project's own workload: wave ballots) and C = 19 (Cityscapes: LDS atomics), beside heads.resized_eval_areas with
       PPNET_LIBRARY_EVAL=1 — F.interpolate of the float32 logits, argmax, the validity mask and three bincounts.  Device events
       around batches of calls, every side warmed up, the sides alternated for three rounds, the minimum of the rounds reported; then
       the peak of allocated memory that one call adds on each side.  The two sides' areas are compared first (they may differ by
       near-tie pixels only; the count is printed).
model  SegNet.eval_areas of DiNAT-B + SETR-UP (prepared, bfloat16, and unprepared float32) at 8 x 512 x 512, the same two sides, the
       same protocol: ms per batch and peak rise.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ppnet_amd import fused, heads  # noqa: E402
from ppnet_amd.segnet import IMG_MEAN, IMG_STD, SegNet, randomize_neutral_parameters  # noqa: E402

dev = torch.device("cuda", 0)
BATCH, FULL = 8, 512


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def peak_rise(fn):
    """Peak of allocated memory that one call adds to what is held before it."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - held) / 2 ** 20


def library(fn):
    def run():
        os.environ["PPNET_LIBRARY_EVAL"] = "1"
        try:
            return fn()
        finally:
            del os.environ["PPNET_LIBRARY_EVAL"]
    return run


def alternate(sides, rounds=3):
    for _, fn, _ in sides:
        for _ in range(2):
            fn()
    best = {}
    for _ in range(rounds):
        for name, fn, reps in sides:
            best[name] = min(best.get(name, 1e9), timed(fn, reps))
    return best


def bare_table():
    for classes in (2, 19):
        labels = torch.randint(0, classes, (BATCH, FULL, FULL), device=dev).to(torch.uint8)
        labels[torch.rand(BATCH, FULL, FULL, device=dev) < 0.1] = 255
        for dtype in (torch.float32, torch.bfloat16):
            for low in (256, 128, 32):
                logit = (torch.randn(BATCH, classes, low, low, device=dev) * 2).to(dtype)
                ppn = lambda: heads.resized_eval_areas(logit, labels)
                lib = library(ppn)
                calls = fused.EVAL_CALLS["fwd"]
                a, b = ppn(), lib()
                assert fused.EVAL_CALLS["fwd"] == calls + 1
                differ = int((a - b).abs().sum())
                best = alternate((("ppn", ppn, 50), ("lib", lib, 20)))
                mem = {"ppn": peak_rise(ppn), "lib": peak_rise(lib)}
                print(f"{str(dtype)[6:]:8s} C {classes:2d} {low:3d}^2 -> {FULL}^2 batch {BATCH}: ppn_seg_eval {best['ppn']:7.4f} ms | library "
                      f"{best['lib']:7.4f} ms ({best['lib'] / best['ppn']:6.2f}x) | peak rise ppn {mem['ppn']:.2f} MiB, library {mem['lib']:.1f} MiB "
                      f"(one float32 [B, C, H, W] {BATCH * classes * FULL * FULL * 4 / 2 ** 20:.1f} MiB) | sum |areas difference| {differ} "
                      f"of {int(a[2].sum())} valid pixels", flush=True)
                del logit
                torch.cuda.empty_cache()


def model_table():
    g = torch.Generator().manual_seed(0)
    grid = ((torch.rand(BATCH, FULL, FULL, generator=g) > 0.3).to(torch.uint8) * 255).to(dev)
    gt = (grid > 0).to(torch.uint8)
    for name, dtype, prepare in (("prepared bfloat16", torch.bfloat16, True), ("unprepared float32", torch.float32, False)):
        torch.manual_seed(0)
        net = randomize_neutral_parameters(SegNet(), seed=1).to(dev).eval()
        if prepare:
            net.prepare_inference()
        net = net.to(dtype)
        img = fused.grid_to_image(grid, IMG_MEAN, IMG_STD, dtype)
        ppn = lambda: net.eval_areas(img, gt)
        lib = library(ppn)
        a, b = ppn(), lib()
        differ = int((a - b).abs().sum())
        best = alternate((("ppn", ppn, 5), ("lib", lib, 5)))
        mem = {"ppn": peak_rise(ppn), "lib": peak_rise(lib)}
        print(f"DiNAT-B + SETR-UP {name:18s} eval_areas {BATCH} x {FULL}^2: ppn_seg_eval path {best['ppn']:8.3f} ms | library composition "
              f"{best['lib']:8.3f} ms ({best['lib'] / best['ppn']:5.3f}x) | peak rise ppn {mem['ppn']:.1f} MiB, library {mem['lib']:.1f} MiB | "
              f"sum |areas difference| {differ} of {int(a[2].sum())} valid pixels", flush=True)
        del net, img
        torch.cuda.empty_cache()


if __name__ == "__main__":
    print(f"{torch.cuda.get_device_name(0)}; device events, minimum of 3 alternated rounds", flush=True)
    bare_table()
    model_table()
