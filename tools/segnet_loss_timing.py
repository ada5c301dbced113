"""Times the heads' training loss — bilinear resize + cross-entropy — and the DiNAT-B training step (output
kept under profiles/).

default      forward and backward of the loss alone at the three training ratios, 8 images, 2 classes, 512 x 512 uint8 labels with
             about 10 % ignored: logits 256 x 256 (SETR-UP), 128 x 128 (UPerHead / UPerPUP) and 32 x 32 (the auxiliary FCN head), in
             float32 and bfloat16: ppn_resize_ce_fwd (with the lse buffer) and ppn_resize_ce_bwd beside the library composition
             forward_train ran before (F.interpolate of the float32 logits, decode_losses on int64 labels: cross-entropy, mean and
             the argmax accuracy, the .float() and .long() copies included) with autograd recording on a tensor that requires grad,
             as in a training step; device events, every side warmed up, the sides alternated for three rounds in one process, the
             minimum of the rounds reported.  Then the peak of allocated memory one forward + backward adds on each side.
--step R DTYPE [--tree DIR]
             the whole training step (train.segnet_train_step, DiNAT-B + SETR-UP with the FCN auxiliary head on level 2, 8 images
             at R x R; DTYPE float32, or bfloat16 = autocast) with the package imported from DIR (another checkout with its own
             built library, e.g. the parent commit's; default: this tree): ms per step over 6 steps after 3, and the peak of
             allocated memory.  PPNET_LIBRARY_LOSS=1 in the environment selects the library composition in this tree.  One process
             per run; alternate from the shell.
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else ROOT
sys.path.insert(0, os.path.abspath(TREE))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from ppnet_amd import _lib as L  # noqa: E402
from ppnet_amd import fused, train  # noqa: E402
from ppnet_amd.heads import decode_losses  # noqa: E402
from ppnet_amd.segnet import DINAT_BASE, SegNet, _UPERPUP_AUX  # noqa: E402

dev = torch.device("cuda", 0)
BATCH, CLASSES, FULL = 8, 2, 512
DT = {"bfloat16": torch.bfloat16, "float32": torch.float32}
P = lambda t: ctypes.c_void_p(t.data_ptr())


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernel_calls(logit, labels):
    B, C, h, w = logit.shape
    H, W = labels.shape[-2:]
    need = L.lib.ppn_resize_ce_workspace(B, H, W)
    ws = torch.empty(need, dtype=torch.float32, device=dev)
    lse = torch.empty(B, H, W, dtype=torch.float32, device=dev)
    loss, correct = torch.empty((), dtype=torch.float32, device=dev), torch.empty((), dtype=torch.int64, device=dev)
    g, dlogit = torch.ones((), dtype=torch.float32, device=dev), torch.empty_like(logit)
    dt = 0 if logit.dtype == torch.float32 else 1
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fwd():
        L.check(L.lib.ppn_resize_ce_fwd(P(logit), P(labels), P(lse), P(loss), P(correct), P(ws), need, B, C, h, w, H, W, 255, dt, 0, stream()),
                "ppn_resize_ce_fwd")

    def bwd():
        L.check(L.lib.ppn_resize_ce_bwd(P(logit), P(labels), P(lse), P(g), P(dlogit), B, C, h, w, H, W, 255, dt, 0, stream()), "ppn_resize_ce_bwd")
    return fwd, bwd


def library_of(t, labels):
    """forward_train's lines before the kernel pair: the float32 copy, the resize, the int64 labels, decode_losses."""
    return decode_losses(F.interpolate(t.float(), labels.shape[-2:], mode="bilinear", align_corners=False), labels.long(), 1.0)


def peak_rise(fn):
    """Peak of allocated memory that one forward + backward adds to what is held before it."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - held) / 2 ** 20


def launch_table():
    labels = torch.randint(0, CLASSES, (BATCH, FULL, FULL), device=dev).to(torch.uint8)
    labels[torch.rand(BATCH, FULL, FULL, device=dev) < 0.1] = 255
    for dtype in (torch.float32, torch.bfloat16):
        for low in (256, 128, 32):
            logit = (torch.randn(BATCH, CLASSES, low, low, device=dev) * 2).to(dtype)
            kf, kb = kernel_calls(logit, labels)
            t = logit.detach().clone().requires_grad_(True)
            lib_loss = library_of(t, labels)[0]
            sides = (("ppn fwd", kf, 20), ("lib fwd", lambda: library_of(t, labels), 10),
                     ("ppn bwd", kb, 20), ("lib bwd", lambda: torch.autograd.grad(lib_loss, t, retain_graph=True), 10))
            for _, fn, _ in sides:
                for _ in range(2):
                    fn()
            best = {}
            for _ in range(3):
                for name, fn, reps in sides:
                    best[name] = min(best.get(name, 1e9), timed(fn, reps))
            del lib_loss, sides
            mem = {}
            for name, f in (("ppn", lambda u: fused.resize_cross_entropy(u, labels)[0]), ("lib", lambda u: library_of(u, labels)[0])):
                def run(f=f):
                    u = logit.detach().clone().requires_grad_(True)
                    f(u).backward()
                run()
                mem[name] = peak_rise(run)
            lanes = fused.resize_ce_bwd_lanes(low, low, FULL, FULL)
            print(f"{str(dtype)[6:]:8s} {low:3d}^2 -> {FULL}^2 batch {BATCH} C {CLASSES}: forward ppn_resize_ce_fwd {best['ppn fwd']:7.4f} ms | library "
                  f"{best['lib fwd']:7.4f} ms ({best['lib fwd'] / best['ppn fwd']:5.2f}x)", flush=True)
            print(f"{'':8s} {'':29s} backward ppn_resize_ce_bwd {best['ppn bwd']:7.4f} ms ({lanes} lanes per output) | library "
                  f"{best['lib bwd']:7.4f} ms ({best['lib bwd'] / best['ppn bwd']:5.2f}x)", flush=True)
            print(f"{'':8s} {'':29s} forward + backward peak rise: ppn {mem['ppn']:.1f} MiB, library {mem['lib']:.1f} MiB (one float32 "
                  f"[B, C, H, W] {BATCH * CLASSES * FULL * FULL * 4 / 2 ** 20:.1f} MiB, one lse {BATCH * FULL * FULL * 4 / 2 ** 20:.1f} MiB)", flush=True)
            del logit, t, kf, kb
            torch.cuda.empty_cache()


if "--step" in sys.argv:
    i = sys.argv.index("--step")
    R, amp = int(sys.argv[i + 1]), {"float32": None, "bfloat16": torch.bfloat16}[sys.argv[i + 2]]
    torch.manual_seed(0)
    net = SegNet(**DINAT_BASE, auxiliary_head=dict(_UPERPUP_AUX)).to(dev)
    tr = train.segnet_trainer(net)
    opt = train.segnet_optimizer(tr)
    grid = (torch.rand(BATCH, R, R, device=dev) > 0.3).to(torch.uint8) * 255
    labels = (grid > 0).to(torch.uint8)

    def step(it=0):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp is not None):
            return train.segnet_train_step(tr, opt, it, 100, grid, labels, schedule=dict(warmup_iters=0))
    for it in range(3):
        step(it)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ms = timed(step, 6)
    calls = getattr(fused, "LOSS_CALLS", {})
    which = "library loss" if os.environ.get("PPNET_LIBRARY_LOSS") else "default"
    print(f"tree {os.path.relpath(os.path.abspath(TREE), ROOT):16s} {which:12s} DiNAT-B + SETR-UP + aux train step R {R} {BATCH} images {sys.argv[i + 2]:8s}: "
          f"{ms:8.2f} ms per step, peak allocated {torch.cuda.max_memory_allocated() / 2 ** 20:8.0f} MiB, ppn_resize_ce_fwd / bwd launches "
          f"{calls.get('fwd')} / {calls.get('bwd')}", flush=True)
else:
    launch_table()
