"""Training-step timings on one GPU (config sizes of the reference: GenNet batch 8 at 224 -> here 256, SegNet 8 images per GPU).
Data: generator kernels (stage A/B + label masks), built once outside the timed loop.

Environment: TRAIN_TIMING_ONLY = segnet / gennet (one model only); for the SegNet leg TRAIN_TIMING_R (comma list of sides, default
256), TRAIN_TIMING_AMP (comma list of fp32 / bf16, bf16 = autocast; default fp32), TRAIN_TIMING_STEPS (timed steps after 3 warm-up
steps, default 5), TRAIN_TIMING_MATERIALISED=1 (the neighbourhood attention's padded layers train through the pad / qkv / NA / crop
composition instead of the virtual-padding kernels: the A/B of DESIGN section 14).  The SegNet line also reports the peak of
allocated memory over the timed steps and the vpad launches per step."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from ppnet_amd import edage, na, train
from ppnet_amd.gennet import AEViT
from ppnet_amd.segnet import SegNet

dev = torch.device("cuda:0")
R = 256


def pairs(n_paths, placements, seed, R=R):
    pb = edage.generate_paths(n_paths, R, 50, 3, seed=seed, device=dev)
    mb = edage.generate_maps(pb, placements, 5, 20, seed=seed)
    return train.generator_pairs(pb, mb, placements)


def timeit(step, n):
    for _ in range(3):
        step()
    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats(); t = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n


def _materialised_forward(self, x, real_hw=None):
    """NeighborhoodAttention2D's training branch as the pad / crop composition (what it was before ppn_na2d_bwd_vpad)."""
    if real_hw is not None or not (torch.is_grad_enabled() and (x.requires_grad or self.rpb.requires_grad)):
        return _module_forward(self, x, real_hw)
    B, H, W, _ = x.shape
    pad = self.padded_hw(H, W)
    xp = x if pad is None else F.pad(x, (0, 0, 0, pad[1] - W, 0, pad[0] - H))
    o = na.na2d_autograd(self.qkv(xp), self.rpb, self.num_heads, self.dilation, self.scale)
    return self.proj_drop(self.proj(o[:, :H, :W]))


_module_forward = na.NeighborhoodAttention2D.forward
MATERIALISED = bool(os.environ.get("TRAIN_TIMING_MATERIALISED"))
if MATERIALISED:
    na.NeighborhoodAttention2D.forward = _materialised_forward

ONLY = os.environ.get("TRAIN_TIMING_ONLY", "")                      # "segnet" / "gennet": one model only (profiler passes)
for batch, amp in (() if ONLY == "segnet" else ((8, None), (64, None), (64, torch.bfloat16))):
    grid, space, path = pairs(batch // 8, 8, 1)
    net = AEViT(1, 1, img_resolution=R, dim=24).to(dev)
    opt = train.gennet_optimizer(net); sch = train.PolyLR(opt, 1000)
    dt = timeit(lambda: train.gennet_train_step(net, opt, sch, space, path, amp_dtype=amp), 10)
    print("GenNet train step: batch %3d %s  %.1f ms  %.0f maps/s" % (batch, "bf16 autocast" if amp else "fp32", dt * 1e3, batch / dt))

STEPS = int(os.environ.get("TRAIN_TIMING_STEPS", "5"))
for batch in (() if ONLY == "gennet" else (8,)):
    for side in (int(s) for s in os.environ.get("TRAIN_TIMING_R", str(R)).split(",")):
        for mode in os.environ.get("TRAIN_TIMING_AMP", "fp32").split(","):
            amp = {"fp32": None, "bf16": torch.bfloat16}[mode]
            grid, space, path = pairs(1, batch, 2, side)
            torch.manual_seed(0)
            seg = SegNet().to(dev)
            trainer = train.segnet_trainer(seg)
            opt = train.segnet_optimizer(trainer)
            it = [0]
            def step():
                it[0] += 1
                with torch.autocast("cuda", dtype=amp, enabled=amp is not None):
                    return train.segnet_train_step(trainer, opt, it[0], 160000, grid, space)
            calls = getattr(na, "TRAIN_CALLS", None)
            before = dict(calls) if calls else None
            dt = timeit(step, STEPS)
            vpad = "" if not calls else "  vpad launches per step fwd %g bwd %g" % tuple((calls[k] - before[k]) / (STEPS + 3) for k in ("fwd_vpad_kernel", "bwd_vpad_kernel"))
            print("SegNet (DiNAT-B + SETR-UP) train step: R %d batch %d %s%s  %.1f ms  %.1f images/s  peak allocated %.0f MiB%s"
                  % (side, batch, "bf16 autocast" if amp else "fp32", " (materialised padding)" if MATERIALISED else "", dt * 1e3, batch / dt,
                     torch.cuda.max_memory_allocated() / 2 ** 20, vpad), flush=True)
            del seg, trainer, opt
            torch.cuda.empty_cache()
