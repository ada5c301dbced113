"""A/B of ppn_upsample2x_nhwc_bias between two builds of libppnet_hip.so on the SETR-UP head's three up-sampling launches at batch 256,
R = 256 (DiNAT-B: 512 channels, 8^2 -> 16^2, 16^2 -> 32^2, 32^2 -> 64^2, bias + ReLU, bfloat16): both libraries loaded side by side
through ctypes, the same inputs, the outputs compared bit for bit, and rounds of the three launches timed with device events,
alternating A and B.

    python tools/upsample_ab.py LIB_A LIB_B [--rounds 10] [--reps 20]"""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib_a")
    ap.add_argument("lib_b")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    libs = []
    for path in (a.lib_a, a.lib_b):
        lib = ctypes.CDLL(os.path.abspath(path))
        f = lib.ppn_upsample2x_nhwc_bias
        f.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int32] * 6 + [ctypes.c_void_p]
        f.restype = ctypes.c_int
        libs.append(f)
    dev = torch.device("cuda", 0)
    B, C = 256, 512
    g = torch.Generator(device=dev).manual_seed(0)
    xs = [torch.randn(B, s, s, C, generator=g, device=dev).to(torch.bfloat16) for s in (8, 16, 32)]
    bias = (torch.randn(C, generator=g, device=dev) * 0.2).to(torch.bfloat16)
    ys = [[torch.empty(B, 2 * s, 2 * s, C, device=dev, dtype=torch.bfloat16) for s in (8, 16, 32)] for _ in libs]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(k):
        for x, y in zip(xs, ys[k]):
            s = x.shape[1]
            assert libs[k](ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(bias.data_ptr()), ctypes.c_void_p(y.data_ptr()), B, s, s, C, 1, 1,
                           stream) == 0
    byts = sum(x.numel() * 2 + 4 * x.numel() * 2 for x in xs)
    for k in (0, 1):
        run(k)
    torch.cuda.synchronize()
    same = all(torch.equal(p, q) for p, q in zip(ys[0], ys[1]))
    print(f"outputs bit-equal: {same}; {byts / 1e9:.2f} GB per round of three launches")
    times = {0: [], 1: []}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(a.rounds):
        for k in ((0, 1) if r % 2 == 0 else (1, 0)):
            run(k)
            e0.record()
            for _ in range(a.reps):
                run(k)
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.reps)
    for k, name in ((0, "A " + a.lib_a), (1, "B " + a.lib_b)):
        t = sorted(times[k])
        print(f"{name}: three launches {t[len(t) // 2]:.4f} ms median (min {t[0]:.4f}, max {t[-1]:.4f}) over {a.rounds} rounds; "
              f"{byts / (t[len(t) // 2] * 1e-3) / 8e12:.3f} of 8 TB/s")
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
