"""Times SegNet's training-input kernels (output kept under profiles/augment_timing.txt).

default      ppn_augment_codes (with labels, parameters drawn by ppn_augment_params) beside ppn_grid_to_image — the parent's kernel, the
             baseline — on the same occupancy codes, and ppn_augment_rgb on the rendered RGB image, at 224 x 224 and 512 x 512, 8 and
             256 images, float32 and bfloat16 outputs: device events, every side warmed up, the sides alternated for three rounds in
             one process, the minimum of the rounds reported; beside each time the bytes the call moves over that time (no padding:
             Ho = H, Wo = W; per pixel the input — 1 code byte or 3 RGB bytes —, the image written and, for the two new kernels, one
             label byte read and one written; each call includes its output allocation, the same on every side).  Then
             ppn_augment_params alone at 256 images, the raw entry point on a preallocated buffer.
--step R DTYPE
             the whole training step (train.segnet_train_step, SegNet() = DiNAT-B + SETR-UP as tools/train_timing.py and DESIGN.md
             section 6b time it, 8 images at R x R; DTYPE float32, or bfloat16 = autocast) without and with augment=, alternated for
             three rounds in one process: ms per step over 6 steps, the minimum of the rounds.
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ppnet_amd import _lib as L  # noqa: E402
from ppnet_amd import augment, fused, train  # noqa: E402
from ppnet_amd.segnet import IMG_MEAN, IMG_STD, SegNet  # noqa: E402

dev = torch.device("cuda", 0)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def codes_of(B, R):
    """Occupancy-like codes: free space with obstacle blobs and a few marker pixels."""
    g = torch.Generator(device=dev).manual_seed(B * 1000 + R)
    lo = torch.rand(B, 1, R // 8, R // 8, device=dev, generator=g)
    grid = (torch.nn.functional.interpolate(lo, size=(R, R), mode="nearest")[:, 0] > 0.3).to(torch.uint8) * 255
    grid[:, :8, :8] = 128
    return grid.contiguous()


def kernel_table():
    aug = augment.SegAugment(seed=1)
    for R in (224, 512):
        for B in (8, 256):
            grid = codes_of(B, R)
            labels = (grid > 0).to(torch.uint8)
            rgb = torch.stack([(grid >= 128), grid == 255, grid == 255], dim=-1).to(torch.uint8) * 255
            params = augment.draw_params(aug, 0, B, dev)
            for dtype in (torch.float32, torch.bfloat16):
                sides = (("grid_to_image", lambda: fused.grid_to_image(grid, IMG_MEAN, IMG_STD, dtype)),
                         ("augment_codes", lambda: fused.augment_codes(grid, labels, params, IMG_MEAN, IMG_STD, dtype)),
                         ("augment_rgb", lambda: fused.augment_rgb(rgb, labels, params, IMG_MEAN, IMG_STD, dtype)))
                a, _ = sides[1][1]()
                b, _ = sides[2][1]()
                assert torch.equal(a, b)                                   # the two modes agree on the palette image
                reps = 200 if B == 8 else 20
                for _, fn in sides:
                    for _ in range(3):
                        fn()
                best = {}
                for _ in range(3):
                    for name, fn in sides:
                        best[name] = min(best.get(name, 1e9), timed(fn, reps))
                px, esz = B * R * R, (4 if dtype == torch.float32 else 2)
                moved = {"grid_to_image": px * (1 + 3 * esz), "augment_codes": px * (3 + 3 * esz), "augment_rgb": px * (5 + 3 * esz)}
                row = ", ".join(f"{n} {best[n] * 1e3:8.1f} us ({moved[n] / best[n] / 1e9:5.2f} TB/s)" for n, _ in sides)
                print(f"{R:3d}^2 x {B:3d} {str(dtype)[6:]:8s}: {row}; codes / grid_to_image {best['augment_codes'] / best['grid_to_image']:.2f}x",
                      flush=True)
            del grid, labels, rgb
            torch.cuda.empty_cache()
    words = torch.empty(256, fused.AUG_PARAM_WORDS, dtype=torch.int32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def draw():
        L.check(L.lib.ppn_augment_params(1, 0, 256, 0.5, 32.0, 0.5, 1.5, 0.5, 1.5, 18, ctypes.c_void_p(words.data_ptr()), stream), "ppn_augment_params")
    for _ in range(3):
        draw()
    print(f"ppn_augment_params, 256 images: {min(timed(draw, 200) for _ in range(3)) * 1e3:.1f} us per call (raw entry point, preallocated output)",
          flush=True)


def step_rows(R, name):
    amp = {"float32": None, "bfloat16": torch.bfloat16}[name]
    B = 8
    torch.manual_seed(0)
    net = SegNet().to(dev)
    tr = train.segnet_trainer(net)
    opt = train.segnet_optimizer(tr)
    grid = codes_of(B, R)
    labels = (grid > 0).to(torch.uint8)
    aug = augment.SegAugment(seed=1)
    it = [0]

    def step(a):
        it[0] += 1
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp is not None):
            return train.segnet_train_step(tr, opt, it[0], 100000, grid, labels, schedule=dict(warmup_iters=0), augment=a)
    for a in (None, aug, None, aug, None, aug):
        step(a)
    best = {}
    for _ in range(3):
        for key, a in (("plain", None), ("augment", aug)):
            best[key] = min(best.get(key, 1e9), timed(lambda: step(a), 6))
    print(f"DiNAT-B + SETR-UP train step R {R} {B} images {name:8s}: {best['plain']:8.2f} ms per step on the palette image, "
          f"{best['augment']:8.2f} ms with augment= ({best['augment'] - best['plain']:+.2f} ms)", flush=True)


if "--step" in sys.argv:
    i = sys.argv.index("--step")
    step_rows(int(sys.argv[i + 1]), sys.argv[i + 2])
else:
    kernel_table()
