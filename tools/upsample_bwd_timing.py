"""Times the decode heads' up-sampling under autograd (output kept as profiles/upsample_bwd_timing.txt): the HIP
kernels and their backward entries (fused.upsample2x_nhwc / upsample2x_add / upsample2x_concat / resize_concat) beside the library
composition PPNET_LIBRARY_UPSAMPLE=1 selects (F.relu, F.interpolate, +, torch.cat and the library's scatter backward), in one process.

(a) the stages of DiNAT-B + SETR-UP's head at 8 images, R = 224 and 256 (512 channels; ReLU folded in front of all but the last, which
    only training runs): forward + backward, and the backward kernel alone with its achieved GB/s against the compulsory bytes
    (read dy, read x when the ReLU is folded, write dx);
(b) UPerHead's assembly steps (NAT-B + UPerHead, 64 channels: the pyramid pooling output, the three top-down sums, the FPN output)
    and UPerPUPHead's last up-sampling + concatenation (256 channels), likewise;
(c) the whole train.segnet_train_step (DiNAT-B + SETR-UP, tools/train_timing.py's SegNet leg), float32 and bfloat16 autocast, the
    knob off and on.  With the knob on the heads run the op sequence they ran before the backward kernels existed.

In (a) and (b) the kernel side runs with the size gate of the single-operator forms (fused.UPSAMPLE_RECORD_MIN) open, so that every
shape is measured on both sides, and the line says where the shipped gate routes the shape; (c) runs the shipped routing.

Every side is a whole forward + backward through the public entry on tensors that require grad (allocations included); device events
around REPS repetitions, every side warmed up, the sides alternated for ROUNDS rounds, the median and the spread (min .. max) of the
rounds reported.  Usage: python tools/upsample_bwd_timing.py [output file] [abc]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ppnet_amd import fused  # noqa: E402

dev = torch.device("cuda", 0)
ROUNDS, REPS = 5, 100               # a timed window is REPS calls: 6 ms at the smallest shape, so that the clock's and the scheduler's grain stay below 1 %
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "upsample_bwd_timing.txt")
PARTS = sys.argv[2] if len(sys.argv) > 2 else "abc"
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


def with_knob(fn, on):
    def run():
        if on:
            os.environ["PPNET_LIBRARY_UPSAMPLE"] = "1"
        try:
            return fn()
        finally:
            os.environ.pop("PPNET_LIBRARY_UPSAMPLE", None)
    return run


def alternate(sides, reps=REPS):
    """{name: (median, min, max)} in ms of the sides, warmed up and alternated."""
    for _, fn in sides:
        for _ in range(2):
            fn()
    rounds = {n: [] for n, _ in sides}
    for _ in range(ROUNDS):
        for n, fn in sides:
            rounds[n].append(timed(fn, reps))
    return {n: (statistics.median(v), min(v), max(v)) for n, v in rounds.items()}


def fmt(t):
    return f"{t[0]:7.4f} ms ({t[1]:.4f} .. {t[2]:.4f})"


def rand_cl(B, C, H, W, dtype, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(B, H, W, C, device=dev, generator=g).to(dtype).permute(0, 3, 1, 2)


def fwd_bwd(call, tensors, grad):
    def run():
        xs = [t.detach().requires_grad_(True) for t in tensors]
        call(xs).backward(grad)
        return [x.grad for x in xs]
    return run


GATE = dict(fused.UPSAMPLE_RECORD_MIN)


def gate_open(fn):
    """fn with the size gate of the single-operator forms open: the kernels whatever the size."""
    def run():
        fused.UPSAMPLE_RECORD_MIN = dict.fromkeys(GATE, 0)
        try:
            return fn()
        finally:
            fused.UPSAMPLE_RECORD_MIN = GATE
    return run


def compare(name, call, tensors, extra=""):
    with torch.no_grad():
        grad = torch.randn_like(call(tensors))
    own, lib = gate_open(fwd_bwd(call, tensors, grad)), with_knob(fwd_bwd(call, tensors, grad), True)
    t = alternate((("ppn", own), ("lib", lib)))
    go, gl = own(), lib()
    gd = max(float((a.float() - b.float()).abs().max() / b.float().abs().max().clamp(min=1e-30)) for a, b in zip(go, gl))
    routed = "kernels" if "Function" in type(call([x.detach().requires_grad_(True) for x in tensors]).grad_fn).__name__ else "library"
    say(f"  {name}: forward + backward ppn {fmt(t['ppn'])} | library {fmt(t['lib'])}  ({t['lib'][0] / t['ppn'][0]:5.2f}x), routed to the {routed};  "
        f"gradients differ by {gd:.1e} of the largest{extra}")


def part_a():
    say("(a) SETR-UP stages, 8 images, 512 channels: ReLU + x2 up-sampling (the last stage: no ReLU, training only)")
    for dtype in (torch.float32, torch.bfloat16):
        for R in (224, 256):
            for k in range(4):
                H = (R // 32) << k
                relu = k < 3
                x = rand_cl(8, 512, H, H, dtype, 100 + H)
                dy = torch.randn(8, 2 * H, 2 * H, 512, device=dev).to(dtype)
                xn = x.permute(0, 2, 3, 1).contiguous() if relu else None
                tb = alternate((("bwd", lambda: fused._upsample2x_bwd(dy, xn)),))["bwd"]
                nbytes = (dy.numel() + (x.numel() if relu else 0) + x.numel()) * dy.element_size()
                compare(f"{str(dtype)[6:]:8s} R {R} {H:3d} -> {2 * H:3d}{' relu' if relu else '     '}", lambda t: fused.upsample2x_nhwc(t[0], relu), [x],
                        f";  ppn_upsample2x_nhwc_bwd alone {fmt(tb)}, {nbytes / 1e6:.1f} MB compulsory = {nbytes / tb[0] / 1e6:.0f} GB/s")
                del x, dy, xn
                torch.cuda.empty_cache()


def part_b():
    say("(b) UPerHead (64 channels) and UPerPUPHead (256 channels) assembly steps, 8 images")
    for dtype in (torch.float32, torch.bfloat16):
        for R in (224, 256):
            s = [R // 4, R // 8, R // 16, R // 32]
            tag = f"{str(dtype)[6:]:8s} R {R}"
            psp = [rand_cl(8, 1024, s[3], s[3], dtype, 1)] + [rand_cl(8, 64, p, p, dtype, 2 + p) for p in (1, 2, 3, 6)]
            compare(f"{tag} pyramid pooling output, {s[3]}x{s[3]} <- 1, 2, 3, 6", fused.resize_concat, psp)
            for k in (3, 2, 1):
                fine, coarse = rand_cl(8, 64, s[k - 1], s[k - 1], dtype, 10 + k), rand_cl(8, 64, s[k], s[k], dtype, 20 + k)
                compare(f"{tag} top-down sum {s[k]:3d} -> {s[k - 1]:3d}", lambda t: fused.upsample2x_add(t[0], t[1]), [fine, coarse])
            compare(f"{tag} FPN output, {s[0]} <- {s[1]}, {s[2]}, {s[3]}", fused.resize_concat, [rand_cl(8, 64, h, h, dtype, 30 + h) for h in s])
            compare(f"{tag} UPerPUP x2 + concat, 4 x 256 channels {s[0]} -> {2 * s[0]}", fused.upsample2x_concat,
                    [rand_cl(8, 256, s[0], s[0], dtype, 40 + l) for l in range(4)])
            torch.cuda.empty_cache()


def part_c():
    from ppnet_amd import edage, train
    from ppnet_amd.segnet import SegNet
    say("(c) train.segnet_train_step, DiNAT-B + SETR-UP, 8 images: PPNET_LIBRARY_UPSAMPLE unset | set | unset with the size gate open")
    for R in (224, 256):
        pb = edage.generate_paths(1, R, 50, 3, seed=2, device=dev)
        mb = edage.generate_maps(pb, 8, 5, 20, seed=2)
        grid, space, _ = train.generator_pairs(pb, mb, 8)
        for mode, amp in (("fp32", None), ("bf16 autocast", torch.bfloat16)):
            torch.manual_seed(0)
            seg = SegNet().to(dev)
            trainer = train.segnet_trainer(seg)
            opt = train.segnet_optimizer(trainer)
            it = [0]

            def step():
                it[0] += 1
                with torch.autocast("cuda", dtype=amp, enabled=amp is not None):
                    return train.segnet_train_step(trainer, opt, it[0], 160000, grid, space)
            t = alternate((("ppn", step), ("lib", with_knob(step, True)), ("open", gate_open(step))), reps=8)
            say(f"  R {R} {mode:13s}: shipped routing {fmt(t['ppn'])} | library {fmt(t['lib'])} | every stage on the kernels (gate open) "
                f"{fmt(t['open'])}  (library - shipped = {t['lib'][0] - t['ppn'][0]:+.3f} ms)")
            del seg, trainer, opt
            torch.cuda.empty_cache()


def main():
    say(f"{torch.cuda.get_device_name(0)}; medians of {ROUNDS} alternated rounds of {REPS} repetitions (min .. max of the rounds)")
    for p, f in (("a", part_a), ("b", part_b), ("c", part_c)):
        if p in PARTS:
            f()
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    main()
