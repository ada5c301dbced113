"""Times the heads' training loss under OHEMPixelSampler (output kept under profiles/): forward + backward of the
fused path (fused.ohem_cross_entropy: ppn_ohem_ce_fwd / ppn_ohem_ce_bwd, the sampler a radix select on the device) beside the library
composition it replaces (F.interpolate of the float32 logits, then heads.decode_losses with the sampler: softmax, gather, boolean
index, a full sort of the valid pixels, the weighted mean — and one host read-back of n_valid), in the same process.

Shapes as tools/segnet_loss_timing.py: 8 images, 2 classes, 512 x 512 uint8 labels with about 10 % ignored, logits
256 x 256 (SETR-UP), 128 x 128 (UPerHead / UPerPUP) and 32 x 32 (the auxiliary FCN head), float32 and bfloat16; the reference's
sampler settings thresh 0.7 / min_kept 100000, the top-k form (thresh None) and class weights alone.  Each side is a whole forward +
backward through its public entry on a tensor that requires grad, as in a training step (allocations included); device events around
10 repetitions, every side warmed up, the sides alternated for 5 rounds, the median of the rounds reported, the forward alone beside
it.  Then the peak of allocated memory one forward + backward adds on each side."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from ppnet_amd import fused  # noqa: E402
from ppnet_amd.heads import OHEMPixelSampler, decode_losses  # noqa: E402

dev = torch.device("cuda", 0)
BATCH, CLASSES, FULL = 8, 2, 512
ROUNDS, REPS = 5, 10
#          name                        thresh min_kept class weights
CONFIGS = [("thresh 0.7 min_kept 100000", 0.7, 100000, None),
           ("top-k      min_kept 100000", None, 100000, None),
           ("class weights, no sampler ", None, None, [1.0, 2.0])]


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def peak_rise(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - held) / 2 ** 20


def main():
    labels = torch.randint(0, CLASSES, (BATCH, FULL, FULL), device=dev).to(torch.uint8)
    labels[torch.rand(BATCH, FULL, FULL, device=dev) < 0.1] = 255
    for dtype in (torch.float32, torch.bfloat16):
        for low in (256, 128, 32):
            logit = (torch.randn(BATCH, CLASSES, low, low, device=dev) * 2).to(dtype)
            for name, thresh, min_kept, cw in CONFIGS:
                sampler = None if min_kept is None else OHEMPixelSampler(thresh=thresh, min_kept=min_kept)
                cwt = None if cw is None else torch.tensor(cw, dtype=torch.float32, device=dev)

                def own(u):
                    return fused.ohem_cross_entropy(u, labels, 255, cwt, thresh, min_kept)[0]

                def lib(u):
                    z = F.interpolate(u.float(), labels.shape[-2:], mode="bilinear", align_corners=False)
                    return decode_losses(z, labels.long(), 1.0, 255, cw, sampler)[0]

                def both(f):
                    def run():
                        u = logit.detach().requires_grad_(True)
                        f(u).backward()
                    return run

                def fwd(f):
                    def run():
                        with torch.no_grad():
                            f(logit)
                    return run
                sides = (("ppn fwd+bwd", both(own)), ("lib fwd+bwd", both(lib)), ("ppn fwd", fwd(own)), ("lib fwd", fwd(lib)))
                for _, fn in sides:
                    for _ in range(2):
                        fn()
                rounds = {n: [] for n, _ in sides}
                for _ in range(ROUNDS):
                    for n, fn in sides:
                        rounds[n].append(timed(fn, REPS))
                t = {n: statistics.median(v) for n, v in rounds.items()}
                mem = {n: peak_rise(both(f)) for n, f in (("ppn", own), ("lib", lib))}
                print(f"{str(dtype)[6:]:8s} {low:3d}^2 -> {FULL}^2 batch {BATCH} C {CLASSES} {name}: forward + backward ppn {t['ppn fwd+bwd']:7.4f} ms | "
                      f"library {t['lib fwd+bwd']:7.4f} ms ({t['lib fwd+bwd'] / t['ppn fwd+bwd']:5.2f}x);  forward ppn {t['ppn fwd']:7.4f} ms | library "
                      f"{t['lib fwd']:7.4f} ms;  peak rise ppn {mem['ppn']:.1f} MiB | library {mem['lib']:.1f} MiB", flush=True)
            del logit
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
