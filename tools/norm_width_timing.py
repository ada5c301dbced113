"""Times the LayerNorm inference kernels at the three-pass widths (output kept as profiles/norm_width_timing.txt).

Per launch, outside autograd, through the public entries: fused.layer_norm(x, ln) (2 passes over the tensor: read x, write y) and
fused.residual_layer_norm(x, a, None, ln) (4 passes: read x and a, write x' and y) at DiNAT-L's four level shapes for 8 images of
512 x 512 — 131072 x 192, 32768 x 384, 8192 x 768, 2048 x 1536 rows x channels — beside the one- and two-pass instances at
128 / 256 / 512 / 1024 channels on the same row counts (DiNAT-B's shapes: code this width change did not touch) and beside
F.layer_norm on the same tensor, float32 and bfloat16.  Reported: time, the bytes the launch has to move over it, and that rate as a
fraction of the one- / two-pass instance's on the same rows.

Whole model: the prepared bfloat16 DiNAT-L + SETR-UP (configs.DINAT_LARGE) on 16 occupancy-code images of 512 x 512 and NAT-Mini +
UPerHead (configs.NAT_MINI_UPER) on 64, SegNet.labels_u8, in ms per batch, with PPNET_LIBRARY_GEMM=1 (the vendor's GEMMs behind the
LayerNorm kernels) as the other side.

Device events around REPS launches, every side warmed up, the sides alternated for ROUNDS rounds; the median and the spread
(min .. max) of the rounds.
Usage: python tools/norm_width_timing.py [output file] [--no-models]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from ppnet_amd import fused, segnet  # noqa: E402

dev = torch.device("cuda", 0)
ROUNDS, REPS = 5, 50
ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = ARGS[0] if ARGS else os.path.join(ROOT, "profiles", "norm_width_timing.txt")
MODELS = "--no-models" not in sys.argv
LEVELS = ((8 * 128 * 128, 192, 128), (8 * 64 * 64, 384, 256), (8 * 32 * 32, 768, 512), (8 * 16 * 16, 1536, 1024))   # rows, new C, old C


def say(s):
    print(s, flush=True)
    with open(OUT, "a") as fh:                                               # line by line: a run that is cut short keeps what it measured
        fh.write(s + "\n")


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(sides, reps=REPS):
    for _, fn in sides:
        for _ in range(3):
            fn()
    rounds = {n: [] for n, _ in sides}
    for _ in range(ROUNDS):
        for n, fn in sides:
            rounds[n].append(timed(fn, reps))
    return {n: (statistics.median(v), min(v), max(v)) for n, v in rounds.items()}


def fmt(t):
    return f"{t[0]:7.4f} ms ({t[1]:.4f} .. {t[2]:.4f})"


def kernel_sides(rows, C, dtype):
    g = torch.Generator(device=dev).manual_seed(C)
    x = torch.randn(rows, C, device=dev, generator=g).to(dtype)
    a = torch.randn(rows, C, device=dev, generator=g).to(dtype)
    ln = torch.nn.LayerNorm(C).to(dev, dtype)
    return {"plain": lambda: fused.layer_norm(x, ln), "resid": lambda: fused.residual_layer_norm(x, a, None, ln),
            "lib": lambda: F.layer_norm(x, (C,), ln.weight, ln.bias, ln.eps)}, x.numel() * x.element_size()


@torch.no_grad()
def kernels():
    say(f"{torch.cuda.get_device_name(0)}; per launch, medians of {ROUNDS} alternated rounds of {REPS} launches (min .. max of the rounds)")
    for dtype in (torch.float32, torch.bfloat16):
        for rows, c_new, c_old in LEVELS:
            new, nb_new = kernel_sides(rows, c_new, dtype)
            old, nb_old = kernel_sides(rows, c_old, dtype)
            t = alternate([("new " + k, f) for k, f in new.items()] + [("old " + k, f) for k, f in old.items()])
            for form, passes in (("plain", 2), ("resid", 4)):
                r_new = passes * nb_new / t["new " + form][0] / 1e6
                r_old = passes * nb_old / t["old " + form][0] / 1e6
                lib = f"; F.layer_norm {fmt(t['new lib'])} ({t['new lib'][0] / t['new plain'][0]:5.2f}x the kernel's time)" if form == "plain" else ""
                say(f"  {str(dtype)[6:]:8s} {rows:6d} rows {'LayerNorm' if form == 'plain' else 'residual + LayerNorm':20s}: "
                    f"C {c_new:4d} {fmt(t['new ' + form])} = {r_new:5.0f} GB/s | C {c_old:4d} {fmt(t['old ' + form])} = {r_old:5.0f} GB/s | "
                    f"rate {r_new / r_old:4.2f} of the {'two' if c_old == 1024 else 'one'}-pass instance{lib}")
            del new, old
            torch.cuda.empty_cache()


def codes(B, R, seed):
    g = torch.Generator().manual_seed(seed)
    lo = (torch.rand(B, 1, R // 16, R // 16, generator=g) > 0.4).float()
    return (F.interpolate(lo, size=(R, R), mode="nearest")[:, 0] * 255).to(torch.uint8).to(dev)


def with_library_gemm(fn):
    def run():
        os.environ["PPNET_LIBRARY_GEMM"] = "1"
        try:
            return fn()
        finally:
            os.environ.pop("PPNET_LIBRARY_GEMM", None)
    return run


@torch.no_grad()
def models():
    say(f"whole model, prepared bfloat16, SegNet.labels_u8 on occupancy codes of 512 x 512: ms per batch, medians of {ROUNDS} alternated rounds of 5 batches")
    for name, cfg, B in (("DINAT_LARGE", segnet.DINAT_LARGE, 16), ("NAT_MINI_UPER", segnet.NAT_MINI_UPER, 64)):
        torch.manual_seed(0)
        m = segnet.randomize_neutral_parameters(segnet.SegNet.from_config(cfg), seed=1).eval().to(dev).to(torch.bfloat16).prepare_inference()
        x = codes(B, 512, 5)
        run = lambda: m.labels_u8(x)
        t = alternate((("ppn", run), ("lib", with_library_gemm(run))), reps=5)
        say(f"  {name:14s} batch {B:3d}: own GEMMs {fmt(t['ppn'])} | PPNET_LIBRARY_GEMM=1 {fmt(t['lib'])}  ({t['lib'][0] / t['ppn'][0]:5.2f}x)")
        del m, x
        torch.cuda.empty_cache()


def main():
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, "w").close()
    kernels()
    if MODELS:
        models()


if __name__ == "__main__":
    main()
