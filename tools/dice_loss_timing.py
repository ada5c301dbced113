"""Times the heads' Dice loss (output kept under profiles/): forward + backward of the fused path
(fused.resize_dice: ppn_resize_dice_fwd / ppn_resize_dice_bwd) beside the library composition it replaces (F.interpolate of the logits,
then heads.dice_loss: softmax, one-hot, the per-class sums, autograd backward), in the same process and the same dtype.

Shapes (B, C, h, w -> H, W): (8, 2, 224, 224 -> 224, 224), SETR-UP's training case (identity); (8, 2, 56, 56 -> 224, 224), UPerHead;
(8, 19, 56, 56 -> 224, 224); uint8 labels with about 10 % ignored; float32 and bfloat16 logits.  Each side is a whole forward + backward
through its public entry on a tensor that requires grad, as in a training step (allocations included); device events around 10
repetitions, every side warmed up, the sides alternated for 5 rounds, the median of the rounds reported, the forward alone beside it.
Then the peak of allocated memory one forward + backward adds on each side (torch.cuda.max_memory_allocated), and the two results
side by side."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from ppnet_amd import fused  # noqa: E402
from ppnet_amd.heads import dice_loss  # noqa: E402

dev = torch.device("cuda", 0)
ROUNDS, REPS = 5, 10
SHAPES = [(8, 2, 224, 224, 224, 224), (8, 2, 56, 56, 224, 224), (8, 19, 56, 56, 224, 224)]


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
    for dtype in (torch.float32, torch.bfloat16):
        for B, C, h, w, H, W in SHAPES:
            g = torch.Generator(device=dev).manual_seed(B * C + h)
            labels = torch.randint(0, C, (B, H, W), device=dev, generator=g).to(torch.uint8)
            labels[torch.rand(B, H, W, device=dev, generator=g) < 0.1] = 255
            logit = (torch.randn(B, C, h, w, device=dev, generator=g) * 2).to(dtype)

            def own(u):
                return fused.resize_dice(u, labels)[0]

            def lib(u):
                return dice_loss(F.interpolate(u, (H, W), mode="bilinear", align_corners=False), labels)

            def both(f):
                def run():
                    u = logit.detach().requires_grad_(True)
                    f(u).backward()
                    return u.grad
                return run

            def fwd(f):
                def run():
                    with torch.no_grad():
                        return f(logit)
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
            lo, ll = float(fwd(own)()), float(fwd(lib)())
            go, gl = both(own)().float(), both(lib)().float()
            gd = float((go - gl).abs().max() / gl.abs().max())
            print(f"{str(dtype)[6:]:8s} B {B} C {C:2d} {h:3d}x{w:3d} -> {H}x{W}: forward + backward ppn {t['ppn fwd+bwd']:7.4f} ms | library "
                  f"{t['lib fwd+bwd']:7.4f} ms ({t['lib fwd+bwd'] / t['ppn fwd+bwd']:5.2f}x);  forward ppn {t['ppn fwd']:7.4f} ms | library "
                  f"{t['lib fwd']:7.4f} ms;  peak rise ppn {mem['ppn']:.1f} MiB | library {mem['lib']:.1f} MiB;  loss ppn {lo:.6f} | library {ll:.6f}, "
                  f"gradients differ by {gd:.1e} of the largest", flush=True)
            del logit, labels
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
