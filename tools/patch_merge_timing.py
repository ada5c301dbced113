"""Times DiNAT_s's patch merge (output kept as profiles/patch_merge_timing.txt): fused.patch_merge_ln on the HIP
pair (ppn_patch_merge_ln_fwd / ppn_patch_merge_ln_bwd) beside the torch composition PPNET_LIBRARY_MERGE=1 selects (pad, four strided
slices, cat, F.layer_norm and the framework's backwards), in one process, at DiNAT_s-B's three merge shapes for 8 images of 224 x 224
(56 x 56 x 128, 28 x 28 x 256, 14 x 14 x 512) and of 512 x 512 (128 x 128 x 128, 64 x 64 x 256, 32 x 32 x 512), float32 and bfloat16,
forward alone (no autograd) and forward + backward (through the public entry on tensors that require grad, allocations included).

Device events around REPS repetitions, every side warmed up, the sides alternated for ROUNDS rounds, the median and the spread
(min .. max) of the rounds reported, and the bytes the pair has to move (forward: x in, y out = 2 passes over the tokens; backward:
gy and x in, dx out = 3 more) over its time.

With `--model` also one DiNAT_s-B + SETR-UP training step (2 images of 512 x 512, float32 and bfloat16 autocast, AdamW) and one
prepared bfloat16 inference batch (8 images of 512 x 512), each with and without the knob.
Usage: python tools/patch_merge_timing.py [--model] [output file]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ppnet_amd import fused  # noqa: E402

dev = torch.device("cuda", 0)
ROUNDS, REPS = 5, 400
ARGS = [a for a in sys.argv[1:] if a != "--model"]
MODEL = "--model" in sys.argv[1:]
OUT = ARGS[0] if ARGS else os.path.join(ROOT, "profiles", "patch_merge_timing.txt")
SHAPES = ((8, 56, 56, 128), (8, 28, 28, 256), (8, 14, 14, 512), (8, 128, 128, 128), (8, 64, 64, 256), (8, 32, 32, 512))
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
        os.environ["PPNET_LIBRARY_MERGE"] = "1"
        try:
            return fn()
        finally:
            os.environ.pop("PPNET_LIBRARY_MERGE", None)
    return run


def alternate(sides, reps=REPS, warm=3):
    for _, fn in sides:
        for _ in range(warm):
            fn()
    rounds = {n: [] for n, _ in sides}
    for _ in range(ROUNDS):
        for n, fn in sides:
            rounds[n].append(timed(fn, reps))
    return {n: (statistics.median(v), min(v), max(v)) for n, v in rounds.items()}


def fmt(t):
    return f"{t[0]:8.4f} ms ({t[1]:.4f} .. {t[2]:.4f})"


def kernels():
    say(f"{torch.cuda.get_device_name(0)}; medians of {ROUNDS} alternated rounds of {REPS} repetitions (min .. max of the rounds)")
    for dtype in (torch.float32, torch.bfloat16):
        for B, H, W, C in SHAPES:
            g = torch.Generator(device=dev).manual_seed(C + H)
            x = torch.randn(B, H, W, C, device=dev, generator=g).to(dtype)
            gy = torch.randn(B, H // 2, W // 2, 4 * C, device=dev, generator=g).to(dtype)
            ln = torch.nn.LayerNorm(4 * C).to(dev, dtype)

            def forward():
                with torch.no_grad():
                    fused.patch_merge_ln(x, ln)

            def both():
                fused.patch_merge_ln(x.detach().requires_grad_(True), ln).backward(gy)
            nbytes = x.numel() * x.element_size()
            for name, fn, passes in (("forward", forward, 2), ("forward + backward", both, 5)):
                t = alternate((("ppn", fn), ("lib", with_knob(fn))))
                say(f"  {str(dtype)[6:]:8s} {B} x {H:3d} x {W:3d} x {C:3d} {name:18s}: ppn {fmt(t['ppn'])} | library {fmt(t['lib'])}  "
                    f"({t['lib'][0] / t['ppn'][0]:5.2f}x);  {passes} passes = {passes * nbytes / 1e6:6.1f} MB = "
                    f"{passes * nbytes / t['ppn'][0] / 1e6:5.0f} GB/s on the kernels")
            del x, gy
            torch.cuda.empty_cache()


def model():
    from ppnet_amd import configs, train
    from ppnet_amd.segnet import SegNet, randomize_neutral_parameters
    torch.manual_seed(0)
    g = torch.Generator(device=dev).manual_seed(1)
    img = torch.randn(2, 3, 512, 512, device=dev, generator=g)
    gt = torch.randint(0, 2, (2, 512, 512), device=dev, generator=g).to(torch.uint8)
    for autocast in (False, True):
        net = randomize_neutral_parameters(SegNet.from_config(configs.DINATS_BASE_SETRUP)).to(dev).train()
        trainer = train.segnet_trainer(net, dev)
        opt = train.segnet_adamw(net)

        def step():
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                loss = trainer(img, gt)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        t = alternate((("ppn", step), ("lib", with_knob(step))), reps=3, warm=2)
        say(f"  DiNAT_s-B + SETR-UP training step, 2 x 512 x 512, {'bfloat16 autocast' if autocast else 'float32'}, AdamW: "
            f"ppn {fmt(t['ppn'])} | library merge {fmt(t['lib'])}  ({t['lib'][0] / t['ppn'][0]:5.3f}x)")
        del net, trainer, opt
        torch.cuda.empty_cache()
    net = randomize_neutral_parameters(SegNet.from_config(configs.DINATS_BASE_SETRUP)).to(dev, torch.bfloat16).eval().prepare_inference()
    batch = torch.randn(8, 3, 512, 512, device=dev, generator=g).to(torch.bfloat16)

    def infer():
        with torch.no_grad():
            net.labels_u8(batch)
    t = alternate((("ppn", infer), ("lib", with_knob(infer))), reps=5, warm=2)
    say(f"  DiNAT_s-B + SETR-UP prepared bfloat16 inference, 8 x 512 x 512 (labels_u8): ppn {fmt(t['ppn'])} | library merge {fmt(t['lib'])}  "
        f"({t['lib'][0] / t['ppn'][0]:5.3f}x)")


def main():
    kernels()
    if MODEL:
        model()
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    main()
