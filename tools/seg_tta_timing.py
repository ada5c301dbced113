"""Times the merge of a test-time augmentation (output kept as profiles/seg_tta_timing.txt): fused.seg_tta — one
ppn_seg_tta launch from the heads' low-resolution logits to uint8 labels — beside the library composition that SegNet.aug_test runs
under PPNET_LIBRARY_TTA=1 from the same logits (per augmentation F.interpolate to the augmentation's image size, F.interpolate to the
output size, softmax in float32, flip, add; then / n and argmax), in one process.  The reference's `--aug-test` list: ratios 0.5 .. 1.75
x {none, horizontal} = 12 augmentations, 16 images, 512 x 512 output, the head's logits at 1 / 2 (SETR-UP) or 1 / 4 (UPerNet) of each
augmentation's image size, C = 2 and C = 19 (and C = 150, the form without LDS), float32 and bfloat16.  The networks' own time is on neither side.

Device events around REPS repetitions, every side warmed up, the sides alternated for ROUNDS rounds, the median and the spread
(min .. max) of the rounds reported; the library side's launches are counted as its framework ops, and the labels of the two sides
are compared.
Usage: python tools/seg_tta_timing.py [output file]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from ppnet_amd import fused  # noqa: E402

dev = torch.device("cuda", 0)
ROUNDS, REPS = 5, 10
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "seg_tta_timing.txt")
BATCH, FULL = 16, 512
RATIOS = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)
CONFIGS = ((2, 2), (2, 4), (19, 4), (150, 4))        # (classes, the head's down-sampling); 150 > fused.SEG_TTA_LDS_CLASSES: three sweeps of loads
_lines = []


def say(s):
    print(s, flush=True)
    _lines.append(s)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(sides):
    for _, fn in sides:
        for _ in range(3):
            fn()
    rounds = {n: [] for n, _ in sides}
    for _ in range(ROUNDS):
        for n, fn in sides:
            rounds[n].append(timed(fn, REPS))
    return {n: (statistics.median(v), min(v), max(v)) for n, v in rounds.items()}


def fmt(t):
    return f"{t[0]:8.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"


def library(logits, mids, flips, out_hw, ops):
    """SegNet.inference per augmentation from the head's logits, and aug_test's mean and argmax; ops[0] counts the framework ops"""
    total = None
    for x, mid, fl in zip(logits, mids, flips):
        z = F.interpolate(x, mid, mode="bilinear", align_corners=False)
        ops[0] += 1
        if tuple(mid) != tuple(out_hw):
            z = F.interpolate(z, out_hw, mode="bilinear", align_corners=False)
            ops[0] += 1
        if z.dtype != torch.float32:
            z = z.float()
            ops[0] += 1
        p = F.softmax(z, dim=1)
        ops[0] += 1
        if fl is not None:
            p = p.flip(dims=(3,))
            ops[0] += 1
        if total is not None:
            total = total + p
            ops[0] += 1
        else:
            total = p
    ops[0] += 2
    return (total / len(logits)).argmax(dim=1)


@torch.no_grad()
def main():
    say(f"{torch.cuda.get_device_name(0)}; {len(RATIOS) * 2} augmentations, {BATCH} x {FULL}^2 output; medians of {ROUNDS} alternated rounds of "
        f"{REPS} repetitions (min .. max of the rounds)")
    for dtype in (torch.float32, torch.bfloat16):
        for classes, down in CONFIGS:
            g = torch.Generator(device=dev).manual_seed(classes * 10 + down)
            logits, mids, flips = [], [], []
            for r in RATIOS:
                m = int(FULL * r)
                for fl in (None, "horizontal"):
                    logits.append((torch.randn(BATCH, classes, m // down, m // down, device=dev, generator=g) * 3).to(dtype))
                    mids.append((m, m))
                    flips.append(fl)
            ops = [0]
            want = library(logits, mids, flips, (FULL, FULL), ops)
            n_ops = ops[0]
            before = fused.TTA_CALLS["fwd"]
            got = fused.seg_tta(logits, mids, flips, (FULL, FULL))[0]
            launches = fused.TTA_CALLS["fwd"] - before
            differ = int((got.long() != want).sum())
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fused.seg_tta(logits, mids, flips, (FULL, FULL))
            peak_ppn = torch.cuda.max_memory_allocated() - base
            torch.cuda.reset_peak_memory_stats()
            library(logits, mids, flips, (FULL, FULL), ops)
            peak_lib = torch.cuda.max_memory_allocated() - base
            t = alternate((("ppn", lambda: fused.seg_tta(logits, mids, flips, (FULL, FULL))),
                           ("lib", lambda: library(logits, mids, flips, (FULL, FULL), ops))))
            say(f"  {str(dtype)[6:]:8s} C {classes:3d} head 1/{down}: ppn_seg_tta {fmt(t['ppn'])}, {launches} launch, peak {peak_ppn / 2**20:7.1f} MiB | "
                f"library {fmt(t['lib'])}, {n_ops} ops, peak {peak_lib / 2**20:7.1f} MiB  ({t['lib'][0] / t['ppn'][0]:5.2f}x);  "
                f"{differ} of {got.numel()} labels differ")
            del logits, want, got
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    main()
