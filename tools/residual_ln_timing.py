"""Times the NAT / DiNAT residual stream under autograd (output kept as profiles/residual_ln_timing.txt):
fused.residual_layer_norm(x, a, gamma, ln, scale=s) and fused.layer_norm(x, ln), forward + backward, on the HIP training pair
(ppn_residual_layernorm_train_fwd / ppn_residual_layernorm_bwd) beside the library composition PPNET_LIBRARY_NORM=1 selects (the
DropPath multiply, gamma *, +, F.layer_norm and the framework's backwards), in one process, at the four level shapes of DiNAT-B with
8 images at 512 x 512: 131072 x 128, 32768 x 256, 8192 x 512, 2048 x 1024 rows x channels, float32 and bfloat16.

Every side is a whole forward + backward through the public entry on tensors that require grad (allocations included); device events
around REPS repetitions, every side warmed up, the sides alternated for ROUNDS rounds, the median and the spread (min .. max) of the
rounds reported, and the bytes the fused pair has to move (4 + 6 passes over the stream) over its time.
Usage: python tools/residual_ln_timing.py [output file]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ppnet_amd import fused  # noqa: E402

dev = torch.device("cuda", 0)
ROUNDS, REPS = 5, 50
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "residual_ln_timing.txt")
SHAPES = ((8, 128, 128, 128), (8, 64, 64, 256), (8, 32, 32, 512), (8, 16, 16, 1024))
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


def with_knob(fn):
    def run():
        os.environ["PPNET_LIBRARY_NORM"] = "1"
        try:
            return fn()
        finally:
            os.environ.pop("PPNET_LIBRARY_NORM", None)
    return run


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
    return f"{t[0]:7.4f} ms ({t[1]:.4f} .. {t[2]:.4f})"


def main():
    say(f"{torch.cuda.get_device_name(0)}; forward + backward, medians of {ROUNDS} alternated rounds of {REPS} repetitions (min .. max of the rounds)")
    for dtype in (torch.float32, torch.bfloat16):
        for B, H, W, C in SHAPES:
            g = torch.Generator(device=dev).manual_seed(C)
            x, a, gx, gy = (torch.randn(B, H, W, C, device=dev, generator=g).to(dtype) for _ in range(4))
            gamma = torch.full((C,), 1e-5, device=dev, dtype=dtype, requires_grad=True)
            ln = torch.nn.LayerNorm(C).to(dev, dtype)
            s = torch.tensor([1 / 0.7, 0.0] * (B // 2), device=dev)

            def residual():
                xs, as_ = x.detach().requires_grad_(True), a.detach().requires_grad_(True)
                xn, y = fused.residual_layer_norm(xs, as_, gamma, ln, scale=s)
                torch.autograd.backward([xn, y], [gx, gy])

            def plain():                                                     # (the kernel side with the size gate open, so that every shape is measured)
                xs = x.detach().requires_grad_(True)
                gate, fused.NORM_RECORD_MIN = fused.NORM_RECORD_MIN, 0
                try:
                    fused.layer_norm(xs, ln).backward(gy)
                finally:
                    fused.NORM_RECORD_MIN = gate
            nbytes = x.numel() * x.element_size()
            for name, fn, passes in (("residual + DropPath + LayerScale + LN", residual, 10), ("plain LayerNorm", plain, 5)):
                t = alternate((("ppn", fn), ("lib", with_knob(fn))))
                say(f"  {str(dtype)[6:]:8s} {B * H * W:6d} x {C:4d} {name:38s}: ppn {fmt(t['ppn'])} | library {fmt(t['lib'])}  ({t['lib'][0] / t['ppn'][0]:5.2f}x);  "
                    f"{passes} passes = {passes * nbytes / 1e6:.0f} MB = {passes * nbytes / t['ppn'][0] / 1e6:.0f} GB/s on the kernels")
            del x, a, gx, gy
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    main()
