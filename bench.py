#!/usr/bin/env python3
"""bench.py — EDaGe-PP map+path instances/s on MI355X (BASELINE.json metric, config 2).

A "step" is one pass of the hot path over one batch of synthetic input: stage A for 100 target
paths (Philox seed) + stage B for 100 x 100 = 10 000 maps at R=256, K=20, clearance 3 — per GPU.
Problem instances shard embarrassingly (rank r owns path ids [r*100, (r+1)*100) and their maps, no
data-path collective); the only collective is the end-of-batch all-gather of the fixed-size
per-instance records over RCCL.  One JSON line is printed by rank 0.

    python bench.py --gpus 1 --steps 20 --warmup 3
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

R, K, PATHS, PLACEMENTS = 256, 20, 100, 100
MAP_SIZE, CLEARANCE, OBST_SIZE, SEED = 50, 3, 5, 0
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy)


def algorithmic_bytes_per_map(k_tot, k_pocket):
    """Compulsory HBM bytes per map for this build's data layout: every output written once,
    every per-path input read once per PLACEMENTS maps.  (SURVEY.md §8(d) priced a byte-per-pixel corridor mask
    and float32 labels: 2*R^2 + 16384 + 12*K_tot = 147.7 KB; the build reads an R^2/8 bit mask shared by all
    placements of a path and writes float64 labels, so its true figure is smaller — the smaller one is used.)"""
    out = R * R + 16000 + 176 + 24.0 * k_tot + K + 8 + 8 + 4 + 8 + 4      # grid, pathpoint, segpoint, obstacles, accept, scalars
    inp = (R * R / 8 + 16000 + 64 * 16 + 176 + 24.0 * k_pocket + 32) / PLACEMENTS
    return out + inp


def measured_traffic():
    """HBM bytes per edage_maps_kernel launch from rocprofv3 PMC passes (FETCH_SIZE doubled per the gfx950
    correction, WRITE_SIZE as read), committed under profiles/ by tools/collect_traffic.py."""
    try:
        with open(os.path.join(ROOT, "profiles", "traffic_maps_kernel.json")) as f:
            return json.load(f)["hbm_bytes_per_launch"]
    except (OSError, KeyError, ValueError):
        return None


def _cpu_sample(args):
    """One worker's share of the CPU baseline: `n_paths` target paths from `first_path` and their placements (oracle)."""
    first_path, n_paths, placements = args
    from oracle import edage_np as E
    src = E.PhiloxSource(SEED)
    t0 = time.perf_counter()
    precs = E.generate_paths(src, n_paths, R, MAP_SIZE, CLEARANCE, first_path_id=first_path)
    t1 = time.perf_counter()
    maps = E.generate_maps(src, precs, R, MAP_SIZE, OBST_SIZE, K, CLEARANCE, placements, first_map_id=first_path * placements)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, n_paths, len(maps)


def usable_cores():
    """Host cores this process may actually run on: the scheduler affinity mask, cut to the cgroup CPU quota when one is set
    (a one-GPU box is a 16-core share of a 256-core host: os.cpu_count() alone overstates it)."""
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        n = os.cpu_count() or 1
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            with open(path) as f:
                parts = f.read().split()
            if path.endswith("cpu.max"):
                if parts[0] != "max":
                    n = min(n, max(1, int(int(parts[0]) / int(parts[1]) + 0.5)))
            else:
                q = int(parts[0])
                if q > 0:
                    with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                        n = min(n, max(1, int(q / int(f.read().split()[0]) + 0.5)))
            break
        except (OSError, ValueError, IndexError):
            continue
    return max(1, n)


def cpu_baseline():
    """The CPU oracle (a NumPy port of the reference's algorithm) on a bounded sample of the same workload:
    (a) one host core: 20 target paths x 100 placements at R=256, K=20 (~15 s); (b) all usable host cores (usable_cores():
    affinity mask and cgroup quota; BENCH_CPU_WORKERS overrides): one worker process per core, 2 target paths x 100 placements
    each, wall-clock over the pool, also stated per core.  Reported, not a target."""
    import multiprocessing as mp
    n_paths, placements = 20, 100
    ta, tb, _, n_maps = _cpu_sample((0, n_paths, placements))
    # same amortisation as the GPU step: stage A once per PLACEMENTS maps
    per_inst = ta / n_paths / PLACEMENTS + tb / n_maps
    out = {"value": round(1.0 / per_inst, 3), "unit": "instances/s", "cores": 1, "kind": "port",
           "sample": f"oracle/edage_np.py: {n_paths} paths ({ta / n_paths * 1e3:.0f} ms each) + {n_maps} maps "
                     f"({tb / n_maps * 1e3:.1f} ms each) at R={R}, K={K}; stage A amortised over {PLACEMENTS} placements",
           "host_cores": os.cpu_count(), "usable_cores": usable_cores()}
    try:
        from concurrent.futures import ProcessPoolExecutor
        workers = max(1, int(os.environ.get("BENCH_CPU_WORKERS", "0")) or usable_cores())
        # spawn: the parent holds a HIP context and must never be forked; an executor (not mp.Pool) so that a worker that
        # dies raises instead of being respawned for ever; 2 paths per 200 maps = the GPU step's 1 path per PLACEMENTS maps
        with ProcessPoolExecutor(workers, mp_context=mp.get_context("spawn")) as ex:
            list(ex.map(_cpu_sample, [(1000 + w, 0, 1) for w in range(workers)], timeout=120))   # start-up outside the clock
            t0 = time.perf_counter()
            parts = list(ex.map(_cpu_sample, [(100 + 2 * w, 2, placements) for w in range(workers)], timeout=240))
            wall = time.perf_counter() - t0
        inst = sum(p[3] for p in parts)
        out["all_cores"] = {"value": round(inst / wall, 2), "unit": "instances/s", "cores": workers,
                            "per_core": round(inst / wall / workers, 2),
                            "sample": f"{workers} worker processes x (2 paths + {2 * placements} maps), {wall:.1f} s wall"}
    except Exception as e:                               # a reported extra: never fail the bench line over it
        out["all_cores"] = {"value": None, "error": repr(e)[:200]}
    return out


MFMA_PEAK_BF16_TFLOPS = 2500.0   # MI355X_MICROARCH.md: ~2.5 PF dense bf16


def ppnet_flops_per_plan(R):
    """FLOPs (2 per multiply-add) of one PPNet problem AS EXECUTED at resolution R — SURVEY.md 8(d)'s count for DiNAT-B +
    SETR-UP (x4 stages) + AE-ViT, with the two places where the build does less work than the reference's graph:
    dilated layers are virtually padded (the qkv projection, LayerNorm and the attention's queries cover the real tokens
    only, so the unpadded figure is the executed one), and the 1x1 classifier runs before the last x2 up-sampling (2 output
    channels at R/4 instead of 512 channels at R/2)."""
    from ppnet_amd.segnet import DINAT_BASE
    b, h = DINAT_BASE["backbone"], DINAT_BASE["decode_head"]
    C0 = b["embed_dim"]
    fl = 2 * (3 * 9 * (C0 // 2)) * (R // 2) ** 2 + 2 * ((C0 // 2) * 9 * C0) * (R // 4) ** 2         # tokenizer
    side = R // 4
    for li, depth in enumerate(b["depths"]):
        C, T = C0 * 2 ** li, side * side
        hidden = int(C * b["mlp_ratio"])
        fl += depth * T * (2 * C * 3 * C + 2 * C * C + 2 * 2 * C * hidden + 2 * 2 * 49 * C)          # qkv, proj, fc1+fc2, QK+AV
        if li + 1 < len(b["depths"]):
            side //= 2
            fl += 2 * (C * 9 * 2 * C) * side * side                                                  # downsampler
    cin, hw = h["in_channels"], side
    for _ in range(h["num_convs"]):
        fl += 2 * cin * 9 * h["channels"] * hw * hw
        cin, hw = h["channels"], hw * 2
    fl += 2 * h["channels"] * h["num_classes"] * (hw // 2) ** 2                                      # classifier at the low resolution
    seg = fl
    n_down = 0
    while (R // 28) >> (n_down + 1):
        n_down += 1                                                                                   # int(log2(R // 28)), ae_vit.py:23
    dim, N = 24, (R >> n_down) ** 2
    gen = 2 * 9 * dim * R * R * 2                                                                     # conv_first + conv_final
    for k in range(n_down):
        gen += 2 * 2 * 9 * dim * dim * (R >> (k + 1)) ** 2                                            # stride-2 conv + its mirrored deconv
    gen += 3 * (N * (2 * dim * 3 * dim + 2 * dim * dim + 2 * 2 * dim * 4 * dim) + 2 * 2 * N * N * dim)
    return seg, gen


def ppnet_cpu_baseline(torch, grids_u8, heat_ridge, init, end, obs, n_obs, R_):
    """Loop B's CPU leg on the host cores (seeded random weights of the same architectures), a bounded sample: the reference's SegNet
    as the float32 PyTorch-CPU composition of its sources (oracle/segnet_ref.py; its NATTEN op has no CPU build here, so
    the attention is the definition oracle's gather) on 2 problems, the reference-architecture AE-ViT (PyTorch-CPU float32)
    on a batch of 8, and the NumPy port of extract_path + collision_check_circle_edge on 8 problems."""
    import numpy as np
    from oracle import plan_np as PN
    from oracle import segnet_ref as SR
    from ppnet_amd import edage
    from ppnet_amd.gennet import AEViT
    from ppnet_amd.segnet import DINAT_BASE, SegNet, normalize_images
    torch.manual_seed(0)
    seg = SegNet().eval()
    img = normalize_images(edage.grid_to_rgb(grids_u8[:2]) * 255.0).cpu()
    with torch.no_grad():
        t0 = time.perf_counter()
        SR.segnet_logits_fp64(seg, DINAT_BASE, img, dtype=torch.float32)
        t_seg = (time.perf_counter() - t0) / 2
        gen = AEViT(1, 1, R_, 24).eval()
        x = torch.rand(8, 1, R_, R_).round()
        gen(x)
        t0 = time.perf_counter()
        gen(x)
        t_gen = (time.perf_counter() - t0) / 8
    hh, ih, eh = heat_ridge[:8].cpu().numpy(), init[:8].cpu().numpy(), end[:8].cpu().numpy()
    oh, nh = obs[:8].cpu().numpy().astype(np.float32), n_obs[:8].cpu().numpy()
    t0 = time.perf_counter()
    for i in range(8):
        ok, path = PN.extract_path(hh[i], ih[i], eh[i], down_sample_rate=2)
        if ok:
            p32 = path.astype(np.float32)
            for j in range(len(path) - 1):
                if PN.collision_check_circle_edge(p32[j], p32[j + 1], oh[i, :nh[i]], R_ / 50, bound=R_):
                    break
    t_tail = (time.perf_counter() - t0) / 8
    per = t_seg + t_gen + t_tail
    return {"value": round(1.0 / per, 3), "unit": "plans/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"SegNet (oracle/segnet_ref.py, float32 PyTorch-CPU composition, 2 problems): {t_seg:.2f} s each; AE-ViT "
                      f"(PyTorch-CPU float32, batch 8): {t_gen * 1e3:.0f} ms each; extract_path + collision (oracle/plan_np.py, "
                      f"1 core, 8 problems on ridge heat maps): {t_tail * 1e3:.0f} ms each",
            "host_cores": os.cpu_count()}


CALIBRATION_PROBLEMS = 4        # grids of the batch the classifier bias is balanced on (bench_ppnet)
PARITY_PROBLEMS = 16            # problems of the batch on which the bf16 leg is compared with the float32 leg
MFMA_PEAK_FP32_TFLOPS = 157.3   # MI355X_MICROARCH.md: float32-input MFMA = the float32 vector rate


def bench_ppnet(torch, dev, resolution, weights_dtype="bf16", calibrate=None):
    """The PPNet object every leg times: the reference architectures (DiNAT-B + SETR-UP, AE-ViT dim 24) with seeded random
    weights — no trained weights ship with the reference — whose NEUTRAL parameters (LayerScale 1e-5, zero biases, unit norms,
    BatchNorm statistics) are given non-trivial seeded values too (segnet.randomize_neutral_parameters), so the residual
    branches carry signal as in a trained checkpoint and the bf16-vs-float32 comparison (`ppnet.parity`) means something.
    The same seeds in every leg: the bf16 and the float32 objects hold the same weights.  calibrate: u8 grids [n,R,R] on which
    the classifier's bias is balanced (segnet.balance_classifier_bias, float32, before anything is folded) — an untrained
    network otherwise puts every pixel in one class and label agreement would be trivially 1; same grids, same shift, in
    every leg."""
    from ppnet_amd import edage
    from ppnet_amd.gennet import AEViT
    from ppnet_amd.ppnet import PPNet
    from ppnet_amd.segnet import SegNet, balance_classifier_bias, normalize_images, randomize_neutral_parameters
    torch.manual_seed(0)
    seg = randomize_neutral_parameters(SegNet().eval(), seed=1)
    if calibrate is not None:
        seg.to(dev)
        balance_classifier_bias(seg, normalize_images(edage.grid_to_rgb(calibrate) * 255.0))
    # GenNet: the checkpoint this build trained itself (tools/train_gennet.py -> ppnet_amd/weights/gennet_r{R}.pth, the reference's
    # {'model': state_dict} layout), loaded as predict.py:51-52 loads one; seeded random weights where there is none
    from ppnet_amd.gennet import load_trained
    gen = AEViT(1, 1, resolution, 24).eval()
    trained = load_trained(gen, resolution) and not os.environ.get("BENCH_UNTRAINED_GENNET")
    if not trained:
        gen = randomize_neutral_parameters(AEViT(1, 1, resolution, 24).eval(), seed=2)
    kw = {} if weights_dtype == "bf16" else {"weights_dtype": None}
    model = PPNet(resolution=resolution, segnet=seg, gennet=gen, **kw).to(dev).eval()
    model.gennet_trained = bool(trained)
    return model


PARITY_TOLERANCE = {      # what tests/test_ppnet_config3.py asserts for the same objects (bf16 prepared vs float32)
    # <= 4 x what is measured (rms logit error 0.0021-0.0025 of the logit rms, heat map 2 codes / rms 0.56 codes; VERDICT r04 item 6:
    # the round-4 bounds 0.08 / 16 / 7.65 would have survived a 30 x regression).  The dominant terms: one bf16 rounding per stored
    # activation (2^-9 relative) and the fused MLP's polynomial GELU (|error| <= 9.2e-5 absolute, include/ppnet_hip.h)
    "rms_logit_rel_max": 0.01, "labels_agree_where_margin_exceeds_rms_x": 6.0,      # x the rms error of the class margin l1 - l0
    "heat_u8_max_code_diff_max": 6, "heat_u8_rms_code_diff_max": 2.0,
    "label_agreement_min_unbalanced_classifier": 0.97,
    "label_agreement_note": "overall agreement is reported, not a criterion here: the bench balances the untrained classifier's bias, so the "
                            "class margin is a small difference of two near-equal logits and a pixel inside 6 x the rms margin error of a tie "
                            "may flip; outside that band every pixel must agree (test_bf16_parity_criteria_with_balanced_classifier). The "
                            "tests' >= 0.97 overall holds for the same weights with the classifier as initialised.",
}


def ppnet_parity(torch, model16, model32, grids):
    """The bf16 leg's outputs against the float32 (reference-precision) leg's on the same grids, outside any clock: SegNet
    logits (rms and maximum error relative to the logit rms), labels (agreement overall and wherever the float32 class margin
    exceeds 6 x the rms error of that margin), and GenNet's 8-bit heat map on the SAME mask (the float32 labels), so each network's own precision is isolated;
    `heat_u8_end_to_end` chains the bf16 labels into the bf16 GenNet.  The tolerance is the one the GPU tests assert."""
    from ppnet_amd import fused
    from ppnet_amd.segnet import IMG_MEAN, IMG_STD
    with torch.no_grad():
        l32 = model32.segnet.encode_decode(fused.grid_to_image(grids, IMG_MEAN, IMG_STD, torch.float32)).float()
        l16 = model16.segnet.encode_decode(fused.grid_to_image(grids, IMG_MEAN, IMG_STD, torch.bfloat16)).float()
        lab32, lab16 = model32.segment_u8(grids).long(), model16.segment_u8(grids).long()
        h32, h16 = model32.heatmap(lab32).int(), model16.heatmap(lab32).int()
        h16e = model16.heatmap(lab16).int()
    rms = float((l16 - l32).pow(2).mean().sqrt())
    lrms = max(float(l32.pow(2).mean().sqrt()), 1e-30)
    rel = rms / lrms
    agree = lab16 == lab32
    # the label is the sign of the class margin l1 - l0: the band a flip may fall in is measured in the MARGIN's error (the
    # difference of two logit errors: ~sqrt(2) x the logit error's rms, and its tail decides)
    m32, m16 = l32[:, 1] - l32[:, 0], l16[:, 1] - l16[:, 0]
    if tuple(m32.shape[-2:]) != tuple(agree.shape[-2:]):              # logits at the head's resolution: compare labels at the input's
        up = lambda t: torch.nn.functional.interpolate(t[:, None], agree.shape[-2:], mode="bilinear", align_corners=False)[:, 0]
        m32, m16 = up(m32), up(m16)
    rms_margin = float((m16 - m32).pow(2).mean().sqrt())
    sure = m32.abs() > PARITY_TOLERANCE["labels_agree_where_margin_exceeds_rms_x"] * rms_margin
    d, de = (h16 - h32).abs().float(), (h16e - h32).abs().float()
    out = {"problems": int(grids.shape[0]), "rms_logit_rel": round(rel, 5), "logit_rms_fp32": round(lrms, 4),
           "label_agreement_vs_fp32": round(float(agree.float().mean()), 5),
           "rms_margin_error_rel": round(rms_margin / max(float(m32.std()), 1e-30), 5),
           "labels_agree_where_margin_exceeds_6rms": bool(agree[sure].all()), "pixels_with_such_margin": round(float(sure.float().mean()), 4),
           "max_logit_err_rel": round(float((l16 - l32).abs().max()) / lrms, 5),
           "free_fraction_fp32": round(float(lab32.float().mean()), 4),
           "heat_u8_max_code_diff": int(d.max()), "heat_u8_rms_code_diff": round(float(d.pow(2).mean().sqrt()), 3),
           "heat_u8_end_to_end": {"max_code_diff": int(de.max()), "rms_code_diff": round(float(de.pow(2).mean().sqrt()), 3)},
           "tolerance_stated": PARITY_TOLERANCE}
    out["within_tolerance"] = bool(rel < PARITY_TOLERANCE["rms_logit_rel_max"]
                                   and out["labels_agree_where_margin_exceeds_6rms"]
                                   and out["heat_u8_max_code_diff"] <= PARITY_TOLERANCE["heat_u8_max_code_diff_max"]
                                   and out["heat_u8_rms_code_diff"] <= PARITY_TOLERANCE["heat_u8_rms_code_diff_max"])
    return out


def ppnet_fp32_leg(torch, dev, grids_u8, batch, steps=3, parity_with=None):
    """The same two networks at the REFERENCE's precision (GenNet/predict.py:46-52,88 and SegNet/test.py:181-191 run float32):
    PPNet(weights_dtype=None) on the same batch — a reported leg, not a tuning target.  It makes the bfloat16 figure a stated
    speed-up over a same-precision run.  On this path the convolutions and projections are ROCm library calls (MIOpen,
    hipBLASLt / rocBLAS through PyTorch) in float32; the neighbourhood attention (ppn_na2d_fwd, float32 form), the fused residual /
    LayerNorm / up-sampling / label kernels are the build's own.  The kernel names of one batch are listed from the profiler."""
    model = bench_ppnet(torch, dev, R, weights_dtype="f32", calibrate=grids_u8[:CALIBRATION_PROBLEMS])
    # PPNet(weights_dtype=None) asks MIOpen for its exhaustive algorithm search (140 s on a fresh box for a 6 % faster batch:
    # 147 -> ~138 ms): a reported leg of a bench that has to finish in minutes takes the heuristic pick
    torch.backends.cudnn.benchmark = bool(os.environ.get("BENCH_FP32_MIOPEN_SEARCH"))
    g = grids_u8[:batch]

    def one():
        return model.heatmap(model.segment_u8(g))
    t0 = time.perf_counter()
    one(); torch.cuda.synchronize()
    first_s = time.perf_counter() - t0                                  # includes the libraries' one-off algorithm search
    one(); torch.cuda.synchronize()
    t1 = time.perf_counter()
    for _ in range(steps):
        one()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t1) / steps * 1e3
    seg_fl, gen_fl = ppnet_flops_per_plan(R)
    tflops = (seg_fl + gen_fl) * batch / (ms * 1e-3) / 1e12
    lib_kernels, own_kernels = None, None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            one(); torch.cuda.synchronize()
        agg = {}
        for ev in prof.key_averages():
            if getattr(ev, "device_time_total", 0) or getattr(ev, "cuda_time_total", 0):
                agg[ev.key] = agg.get(ev.key, 0.0) + float(getattr(ev, "device_time_total", 0) or getattr(ev, "cuda_time_total", 0))
        own = {k: v for k, v in agg.items() if "ppn::" in k}
        lib = {k: v for k, v in agg.items() if "ppn::" not in k and "Memcpy" not in k and "Memset" not in k}
        top = lambda d: [f"{k[:70]} ({v / 1e3:.2f} ms)" for k, v in sorted(d.items(), key=lambda kv: -kv[1])[:12]]
        lib_kernels, own_kernels = top(lib), top(own)
        lib_ms, own_ms = sum(lib.values()) / 1e3, sum(own.values()) / 1e3
    except Exception as e:                                               # the list is an extra: never fail the bench line over it
        lib_kernels, lib_ms, own_ms = [f"profiler unavailable: {e!r}"[:160]], None, None
    parity = None
    if parity_with is not None and parity_with.get("model") is not None:
        try:
            parity = ppnet_parity(torch, parity_with["model"], model, grids_u8[:PARITY_PROBLEMS])
        except Exception as e:
            parity = {"error": repr(e)[:300]}
    del model
    torch.cuda.empty_cache()
    return {"metric": "ppnet_plans_per_sec_fp32", "parity": parity, "value": round(batch / (ms * 1e-3), 1), "unit": "plans/s", "ms_per_batch": round(ms, 2),
            "steps": steps, "dtype": "f32", "first_batch_s": round(first_s, 1),
            "what": "SegNet + GenNet forward only (the planner tail is identical to the bf16 leg's), PPNet(weights_dtype=None)",
            "roofline": {"bound": "mfma", "achieved": round(tflops, 1), "peak": MFMA_PEAK_FP32_TFLOPS, "unit": "TFLOP/s",
                         "frac": round(tflops / MFMA_PEAK_FP32_TFLOPS, 4)},
            "library_kernels_ms": round(lib_ms, 2) if lib_ms is not None else None, "own_kernels_ms": round(own_ms, 2) if own_ms is not None else None,
            "library_kernels": lib_kernels, "own_kernels": own_kernels}


def _kernel_split(torch, fn, top=14):
    """(own kernels, other kernels) of one call of fn as ["name (ms)", ...] lists + their totals in ms, from the profiler."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn(); torch.cuda.synchronize()
    agg = {}
    for ev in prof.key_averages():
        t = float(getattr(ev, "device_time_total", 0) or getattr(ev, "cuda_time_total", 0))
        if t:
            agg[ev.key] = agg.get(ev.key, 0.0) + t
    own = {k: v for k, v in agg.items() if "ppn::" in k}
    lib = {k: v for k, v in agg.items() if "ppn::" not in k and "Memcpy" not in k and "Memset" not in k}
    fmt = lambda d: [f"{k[:70]} ({v / 1e3:.2f} ms)" for k, v in sorted(d.items(), key=lambda kv: -kv[1])[:top]]
    return fmt(own), fmt(lib), sum(own.values()) / 1e3, sum(lib.values()) / 1e3


def segnet_nat_uper_leg(torch, dev, grids_u8, batch, steps=5):
    """The reference's DEFAULT SegNet configuration (SegNet/test.py:29-32 -> configs/nat/upernet_nat_base.py:6-34): NAT-Base (dilation
    1 everywhere) + UPerHead(channels 64), prepared bfloat16 inference on the build's own kernels (UPerHead._forward_mfma), batch of
    256 maps at 256 x 256: segmentations per second and the per-kernel split of one batch."""
    from ppnet_amd import fused
    from ppnet_amd.segnet import IMG_MEAN, IMG_STD, NAT_BASE_UPER, SegNet
    torch.manual_seed(0)
    net = SegNet(**NAT_BASE_UPER).to(dev).eval().prepare_inference().to(torch.bfloat16)
    g = grids_u8[:batch]

    def one():
        with torch.no_grad():
            return net.labels_u8(g)                                            # u8 occupancy codes -> palette tokenizer -> ... -> u8 labels
    one(); one(); torch.cuda.synchronize()
    t1 = time.perf_counter()
    for _ in range(steps):
        one()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t1) / steps * 1e3
    out = {"metric": "segnet_nat_upernet_maps_per_sec", "value": round(batch / (ms * 1e-3), 1), "unit": "maps/s", "ms_per_batch": round(ms, 2),
           "batch": batch, "steps": steps, "dtype": "bf16 (fp32 accumulate)",
           "config": "NAT-Base (depths 3/4/18/5, kernel 7, dilation 1) + UPerHead(channels 64, pool scales 1/2/3/6), 2 classes"}
    try:
        own, lib, own_ms, lib_ms = _kernel_split(torch, one)
        out.update(own_kernels=own, own_kernels_ms=round(own_ms, 2), other_kernels=lib, other_kernels_ms=round(lib_ms, 2))
    except Exception as e:
        out["kernel_split_error"] = repr(e)[:200]
    del net
    torch.cuda.empty_cache()
    return out


R5, PATHS5, PLACEMENTS5 = 512, 16, 16      # BASELINE config 5 per GPU: 512 x 512 maps, 16 target paths x 16 placements = 256 problems per step


def end_to_end_cpu_baseline(torch, model_cfg_R, grids_u8, ridge, init, end, obs, n_obs):
    """Config 5's CPU leg on the host cores, a bounded sample (~30 s): the NumPy port of the generator on 1 target path + 4
    placements at R = 512, the float32 PyTorch-CPU composition of the reference's SegNet (oracle/segnet_ref.py) on 1 problem,
    the reference-architecture AE-ViT (PyTorch-CPU float32, R = 512) on 2, the NumPy planner tail on 4 ridge heat maps."""
    import numpy as np
    from oracle import edage_np as E
    from oracle import plan_np as PN
    from oracle import segnet_ref as SR
    from ppnet_amd import edage
    from ppnet_amd.gennet import AEViT
    from ppnet_amd.segnet import DINAT_BASE, SegNet, normalize_images
    Rr = model_cfg_R
    src = E.PhiloxSource(SEED)
    t0 = time.perf_counter()
    precs = E.generate_paths(src, 1, Rr, MAP_SIZE, CLEARANCE, first_path_id=7)
    t1 = time.perf_counter()
    maps = E.generate_maps(src, precs, Rr, MAP_SIZE, OBST_SIZE, K, CLEARANCE, 4, first_map_id=7 * PLACEMENTS5)
    t2 = time.perf_counter()
    t_gen = (t1 - t0) / PLACEMENTS5 + (t2 - t1) / len(maps)              # stage A amortised over the placements of a path
    torch.manual_seed(0)
    seg = SegNet().eval()
    img = normalize_images(edage.grid_to_rgb(grids_u8[:1]) * 255.0).cpu()
    with torch.no_grad():
        t0 = time.perf_counter()
        SR.segnet_logits_fp64(seg, DINAT_BASE, img, dtype=torch.float32)
        t_seg = time.perf_counter() - t0
        gen = AEViT(1, 1, Rr, 24).eval()
        x = torch.rand(2, 1, Rr, Rr).round()
        gen(x)
        t0 = time.perf_counter()
        gen(x)
        t_gn = (time.perf_counter() - t0) / 2
    hh, ih, eh = ridge[:4].cpu().numpy(), init[:4].cpu().numpy(), end[:4].cpu().numpy()
    oh, nh = obs[:4].cpu().numpy().astype(np.float32), n_obs[:4].cpu().numpy()
    t0 = time.perf_counter()
    for i in range(4):
        ok, path = PN.extract_path(hh[i], ih[i], eh[i], down_sample_rate=2)
        if ok:
            p32 = path.astype(np.float32)
            for j in range(len(path) - 1):
                if PN.collision_check_circle_edge(p32[j], p32[j + 1], oh[i, :nh[i]], Rr / 50, bound=Rr):
                    break
    t_tail = (time.perf_counter() - t0) / 4
    per = t_gen + t_seg + t_gn + t_tail
    return {"value": round(1.0 / per, 4), "unit": "instances/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"R={Rr}: generator (oracle/edage_np.py, 1 core, 1 path + 4 maps) {t_gen * 1e3:.0f} ms per instance; SegNet "
                      f"(oracle/segnet_ref.py, float32 PyTorch-CPU composition, 1 problem) {t_seg:.1f} s; AE-ViT (PyTorch-CPU float32, 2 "
                      f"problems) {t_gn * 1e3:.0f} ms each; extract_path + collision (oracle/plan_np.py, 1 core, 4 ridge maps) {t_tail * 1e3:.0f} ms each",
            "host_cores": os.cpu_count()}


def end_to_end_leg(torch, dev, steps, world, rank, cpu_leg):
    """BASELINE config 5, one GPU's share: EDaGe-PP generation -> PPNet inference -> success rate / path length, at 512 x 512,
    CHAINED in one timed loop: every step runs stage A (16 target paths) + stage B (16 placements each: 256 maps), SegNet on
    those grids (segment_u8), GenNet on SegNet's labels (heatmap) and the planner tail (extract_path + collision check) on
    GenNet's own heat map.  Instances shard by id over the ranks as in config 2; consecutive steps alternate over two HIP
    streams, each with its own buffers.  instances/s == plans/s here: every generated instance is planned.
    No trained weights ship with the reference: GenNet runs the checkpoint this build trained itself at 512 x 512
    (tools/train_gennet.py), SegNet a seeded random initialisation whose labels are noise — so inside the chain GenNet reads the
    generator's own mask_space of the same maps (PPNet.generate_and_plan(gennet_input="labels"): what SegNet is trained to emit; SegNet
    still segments every grid inside the clock, its mask goes nowhere).  `tail_network_output` is the success / length criterion of
    the OMPL harness (reach (1 + eps) x the target length, experiments/ompl_experiments/updated_geometric_planner.py:260-277,349-354)
    on the last timed batch, i.e. on what the trained GenNet predicted; `tail_ridge` the same on ridge heat maps along the label
    paths (untimed).  OMPL itself is absent: problems are emitted in the harness's JSON
    schema (dataset.problem_records / solution_records) for an external run."""
    import torch.distributed as dist
    from ppnet_amd import dataset, edage, evaluate, shard
    model = bench_ppnet(torch, dev, R5)
    n_streams = max(1, int(os.environ.get("PPNET_STREAMS", "2")))
    streams = [torch.cuda.Stream(dev) for _ in range(n_streams)]
    n_local = PATHS5 * PLACEMENTS5
    bufs = [(edage.PathsBatch(PATHS5, R5, MAP_SIZE, CLEARANCE, dev), edage.MapsBatch(n_local, R5, K, dev)) for _ in range(n_streams)]
    s_comm = torch.cuda.Stream(dev) if world > 1 else None
    gathered = torch.empty(world * n_local, shard.PLAN_RECORD_WIDTH, dtype=torch.float64, device=dev) if world > 1 else None

    def one(it, timers=None, gather=True):
        pb, mb = bufs[it % n_streams]
        first_path, _, first_map = shard.local_ids(PATHS5 * world, PLACEMENTS5, rank, world, batch_index=it)
        marks = iter(timers) if timers else None
        r = model.generate_and_plan(pb, mb, PLACEMENTS5, first_path, first_map, seed=SEED + 5, obstacles_size=OBST_SIZE, obstacles_num=K,
                                    mark=(lambda name: next(marks).record()) if timers else None,
                                    gennet_input="labels" if model.gennet_trained else "segnet")
        if world > 1 and gather:                                              # end-of-batch gather of the plan records (RCCL, own stream)
            res = r["result"]
            rec = shard.pack_plan_records(res, evaluate.plan_lengths(res["waypoints"], res["counts"]))
            ev = torch.cuda.Event(); ev.record()
            with torch.cuda.stream(s_comm):
                s_comm.wait_event(ev)
                shard.gather_records(rec, world, out=gathered)
                rec.record_stream(s_comm)
        return pb, mb, r["heat"], r["result"]
    for i in range(2 * n_streams):                                   # allocator pools, tile descriptors, library workspaces: outside the clock
        with torch.cuda.stream(streams[i % n_streams]):
            one(i)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    one(0, ev)
    torch.cuda.synchronize()
    split = [ev[i].elapsed_time(ev[i + 1]) for i in range(4)]
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for i in range(steps):
        with torch.cuda.stream(streams[i % n_streams]):
            pb, mb, heat, res = one(100 + i)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    el = time.perf_counter() - t1
    if world > 1:
        el = shard.max_over_ranks(el, dev)
    if rank != 0:
        return None
    ms = el / steps * 1e3
    seg_fl, gen_fl = ppnet_flops_per_plan(R5)
    tflops = (seg_fl + gen_fl) * n_local / (ms * 1e-3) / 1e12
    target_px = pb.length.repeat_interleave(PLACEMENTS5) * R5 / MAP_SIZE
    init, end = mb.segpoint[:, 0].contiguous(), mb.segpoint[:, 10].contiguous()
    obs, n_obs = mb.obstacles, mb.n_obstacles[:, 0].contiguous()
    ev_net = evaluate.evaluate_plans(res, target_px)
    ridge = evaluate.label_heatmaps(pb, mb, PLACEMENTS5)
    res_r = model.plan_tail(ridge, init, end, obs, n_obs)
    ev_ridge = evaluate.evaluate_plans(res_r, target_px)
    # the harness's input / output schema for the last batch (updated_geometric_planner.py:500-569): problems as MapGenerate
    # writes them, PPNet's solution appended the way the harness appends a planner's
    problems = dataset.problem_records(mb, pb.length, PLACEMENTS5, first_index=0)
    solved = dataset.solution_records(problems, res_r["success"], res_r["waypoints"], res_r["counts"], ms * 1e-3 / n_local)
    rnd = lambda d: {k: (round(v, 4) if isinstance(v, float) else v) for k, v in d.items()}
    out = {"metric": "edage_pp_plus_ppnet_end_to_end_instances_per_sec", "value": round(world * n_local * steps / el, 1), "unit": "instances/s",
           "plans_per_s": round(world * n_local * steps / el, 1), "ms_per_step": round(ms, 2), "steps": steps, "problems_per_step_per_gpu": n_local,
           "dtype": "f64 generator, bf16 networks (fp32 accumulate)", "streams": n_streams,
           "config": {"workload": f"BASELINE config 5, one GPU's share: {PATHS5} target paths x {PLACEMENTS5} placements at {R5}x{R5} -> DiNAT-B + SETR-UP "
                                  "-> AE-ViT (down_time 4) -> extract_path -> collision check, chained", "resolution": R5, "obstacles_num": K,
                      "clearance": CLEARANCE, "map_size": MAP_SIZE},
           "ms_generate": round(split[0], 3), "ms_segnet": round(split[1], 2), "ms_gennet": round(split[2], 2), "ms_tail": round(split[3], 3),
           "tail_network_output": dict(rnd(ev_net), note=("the timed chain's last batch: the TRAINED GenNet's heat map of the generator's label masks "
                                                          "(SegNet untrained: its labels are computed and not used)") if model.gennet_trained
                                       else "the timed chain: GenNet's own heat map (seeded random weights: noise, few plans)"),
           "weights": {"gennet": f"trained by this build (ppnet_amd/weights/gennet_r{R5}.pth)" if model.gennet_trained else "seeded random init",
                       "segnet": "seeded random init"},
           "tail_ridge": dict(rnd(ev_ridge), note="untimed, last batch: ridge heat maps along the label paths (GenNet's training target, blurred)"),
           "ompl": "unavailable (no OMPL python bindings in this image): PPNet column only",
           "harness_records": {"problems": len(problems), "with_solution": sum(1 for q in solved if q["Solution"][-1]["Waypoint"] is not None),
                               "problem_keys": sorted(problems[0].keys()), "solution_keys": sorted(solved[0]["Solution"][-1].keys())},
           "roofline": {"bound": "mfma", "achieved": round(tflops, 1), "peak": MFMA_PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                        "frac": round(tflops / MFMA_PEAK_BF16_TFLOPS, 4), "traffic": None,
                        "gflop_per_plan": round((seg_fl + gen_fl) / 1e9, 2), "counting": "as executed (ppnet_flops_per_plan)"}}
    try:
        # rank 0 alone is here: the profiled step must not enter a collective the other ranks have left (with RCCL it would never return)
        own, lib, own_ms, lib_ms = _kernel_split(torch, lambda: one(999, gather=False), top=6)
        out["roofline"]["dominant_kernels"] = own
        out["own_kernels_ms"], out["other_kernels_ms"] = round(own_ms, 2), round(lib_ms, 2)
    except Exception as e:
        out["kernel_split_error"] = repr(e)[:200]
    if cpu_leg:
        try:
            out["cpu_baseline"] = end_to_end_cpu_baseline(torch, R5, mb.grid, ridge, init, end, obs, n_obs)
        except Exception as e:
            out["cpu_baseline"] = {"error": repr(e)[:300]}
    del model
    torch.cuda.empty_cache()
    return out


def ppnet_leg(torch, dev, pb, mb, batch, steps, world, rank, cpu_leg, hold=None):
    """BASELINE config 3: PPNet inference (SegNet DiNAT-B + SETR-UP -> GenNet AE-ViT -> waypoint extraction ->
    collision check), batch of 256 problems over the 256x256 maps stage B just produced, per GPU.  Weights are
    No trained weights ship with the reference.  GenNet holds the weights this build trained itself (tools/train_gennet.py, the
    build's own training step on its own generator's pairs; ppnet_amd/weights/); SegNet (90 M parameters: no checkpoint fits a
    repo) is a seeded random initialisation, so the labels it emits are noise.  The timed batch runs both networks on the grids —
    every kernel of the chain, SegNet's labels into GenNet — and the planner tail on the heat maps the TRAINED GenNet predicts
    from the generator's label masks of the same problems (mask_space, process_map.py:165-191: SegNet's training target), built
    once outside the timed region: `tail_network_output` is the harness's success / length criterion (config 5's) on that
    PREDICTION.  `tail_ridge` is the same on ridge maps along the label paths (GenNet's training target, blurred; untimed).
    Ends with the end-of-batch gather of the fixed-size plan records (RCCL, own stream) when N > 1."""
    import torch.distributed as dist
    from ppnet_amd import evaluate, na, shard
    model = bench_ppnet(torch, dev, R, calibrate=mb.grid[:CALIBRATION_PROBLEMS])
    if hold is not None:
        hold["model"] = model                  # the float32 leg compares its outputs with this object's (ppnet.parity)
    # the batch: every (n_maps / batch)-th map of the step — 256 problems spread over all 100 target paths (rounds 1-4 took the first
    # 256 maps = 2.56 paths: three paths decide a success rate)
    sel = torch.arange(batch, device=dev) * (mb.grid.shape[0] // batch)
    g = mb.grid[sel].contiguous()
    init, end = mb.segpoint[sel, 0].contiguous(), mb.segpoint[sel, 10].contiguous()
    obs, n_obs = mb.obstacles[sel].contiguous(), mb.n_obstacles[sel, 0].contiguous()
    from ppnet_amd import edage
    ridge = evaluate.label_heatmaps(pb, mb, PLACEMENTS)[sel].contiguous()
    _, space = edage.label_masks(pb, mb, PLACEMENTS, want_path=False, want_space=True)
    tail_heat = model.heatmap(space[sel].contiguous()) if model.gennet_trained else ridge     # the trained network's own prediction
    target_px = (pb.length.repeat_interleave(PLACEMENTS) * R / MAP_SIZE)[sel]
    s_comm = torch.cuda.Stream(dev) if world > 1 else None
    gathered = torch.empty(world * batch, shard.PLAN_RECORD_WIDTH, dtype=torch.float64, device=dev) if world > 1 else None

    def one(timers=None, tail_stream=None):
        """One batch on the current stream.  tail_stream: the planner tail on that stream (PPNet.plan_tail(side_stream=...)): with a
        trained GenNet the walk kernel is as long as its longest walk (2.5 ms at 1 / 16 of the chip), and behind it on the SAME stream
        the next batch's SegNet would wait for it."""
        if timers: timers[0].record()
        mask = model.segment_u8(g)
        if timers: timers[1].record()
        heat = model.heatmap(mask)
        if timers: timers[2].record()
        res = model.plan_tail(tail_heat, init, end, obs, n_obs, side_stream=tail_stream)
        if timers: timers[3].record()
        if world > 1:                                                         # end-of-batch gather of the plan records
            with torch.cuda.stream(tail_stream if tail_stream is not None else torch.cuda.current_stream(dev)):
                rec = shard.pack_plan_records(res, evaluate.plan_lengths(res["waypoints"], res["counts"]))
                ev = torch.cuda.Event(); ev.record()
            with torch.cuda.stream(s_comm):
                s_comm.wait_event(ev)
                shard.gather_records(rec, world, out=gathered)
                rec.record_stream(s_comm)
        return res, heat
    for _ in range(2):
        res, heat = one()
    torch.cuda.synchronize()
    # per-stage split and the attention kernel's own time: one extra, untimed batch with events
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    one(ev)
    na.TIMING = []
    model.segment_u8(g)
    torch.cuda.synchronize()
    na_ms = sum(a.elapsed_time(b) for a, b, _, _, _ in na.TIMING)
    na_bytes = sum(4 * tok * ch * esz for _, _, tok, ch, esz in na.TIMING)        # q, k, v read + out written, once each
    na_launches = len(na.TIMING)
    na.TIMING = None
    t_seg, t_gen, t_tail = ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), ev[2].elapsed_time(ev[3])
    # The same batch as ONE HIP graph (PPNet.capture: the ~290 launches recorded once, replayed by a single hipGraphLaunch), timed
    # beside the eager loop.  Measured at batch 256: the GPU is never waiting for the host (26.99 ms eager, 27.24 ms replayed), so
    # the timed region below stays eager; the graph is what pays at small batches, where the launches are the time.
    ms_graph = None
    if world == 1 and not os.environ.get("PPNET_NO_GRAPH"):
        cp = model.capture(g, init, end, obs, n_obs, tail_heat=tail_heat)
        cp.replay()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(steps):
            cp.replay()
        torch.cuda.synchronize()
        ms_graph = (time.perf_counter() - t1) / steps * 1e3
        del cp
    # Consecutive batches alternate over PPNET_STREAMS HIP streams (default 2): a batch is a chain of dependent kernels, some bound
    # by the matrix pipe (projections, convolutions), some by HBM (attention, LayerNorm, GenNet, tail); with two batches in flight
    # the dispatcher fills one kind's idle units with the other's waves.  Measured on one box: 27.0 -> 26.45 ms per batch (2 streams),
    # 26.40 (3).  Every batch is still the full chain on its own buffers; the timed region is `steps` whole batches.
    n_streams = max(1, int(os.environ.get("PPNET_STREAMS", "2")))
    pp_streams = [torch.cuda.Stream(dev) for _ in range(n_streams)] if n_streams > 1 else [torch.cuda.current_stream(dev)]
    # ... and each batch stream has a tail stream of its own (PPNET_TAIL_STREAM=0: the tail stays on the batch's stream, as in rounds 2-4)
    tail_streams = [torch.cuda.Stream(dev) for _ in pp_streams] if os.environ.get("PPNET_TAIL_STREAM", "1") != "0" else [None] * len(pp_streams)
    for st, ts in zip(pp_streams, tail_streams):            # each stream's allocator pool and library workspaces: outside the clock
        st.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(st):
            one(tail_stream=ts)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for i in range(steps):
        with torch.cuda.stream(pp_streams[i % n_streams]):
            res, heat = one(tail_stream=tail_streams[i % n_streams])
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    el = time.perf_counter() - t1
    if world > 1:
        el = shard.max_over_ranks(el, dev)
    if rank != 0:
        return None
    ms = el / steps * 1e3
    seg_fl, gen_fl = ppnet_flops_per_plan(R)
    tflops = (seg_fl + gen_fl) * batch / (ms * 1e-3) / 1e12
    ev_tail = evaluate.evaluate_plans(res, target_px)
    ev_ridge = evaluate.evaluate_plans(model.plan_tail(ridge, init, end, obs, n_obs), target_px)
    net_tail = model.plan_tail(heat, init, end, obs, n_obs)
    # the same batch CHAINED end to end — the planner tail walks GenNet's own heat map (PPNet.plan) — on the same two streams: with
    # untrained weights that map is noise and the walk ends early, so this is the lighter batch; reported beside the ridge-map one
    for st in pp_streams:
        with torch.cuda.stream(st):
            model.plan(g, init, end, obs, n_obs)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    for i in range(steps):
        with torch.cuda.stream(pp_streams[i % n_streams]):
            model.plan(g, init, end, obs, n_obs)
    torch.cuda.synchronize()
    ms_chained = (time.perf_counter() - t2) / steps * 1e3
    out = {"metric": "ppnet_plans_per_sec", "value": round(world * batch * steps / el, 1), "unit": "plans/s",
           "batch_per_gpu": batch, "steps": steps, "ms_per_batch": round(ms, 2), "dtype": "bf16 (fp32 accumulate)",
           "workload": "PPNet inference batch=256 over 256x256 maps: DiNAT-B + SETR-UP -> AE-ViT -> extract_path -> collision check"
                       + (" -> all-gather of plan records" if world > 1 else ""),
           "ms_segnet": round(t_seg, 2), "ms_gennet": round(t_gen, 2), "ms_tail": round(t_tail, 2),
           "ms_per_batch_hip_graph": round(ms_graph, 2) if ms_graph is not None else None, "streams": n_streams,
           "tail_streams": sum(t is not None for t in tail_streams),
           "ms_per_batch_chained_network_output": round(ms_chained, 2),
           "weights": {"gennet": ("trained by this build (tools/train_gennet.py; ppnet_amd/weights/gennet_r%d.pth, reference checkpoint layout)" % R)
                                 if model.gennet_trained else "seeded random init",
                       "segnet": "seeded random init, neutral parameters randomised too (no trained weights in the reference; 90 M parameters)"},
           "tail_input": ("the TRAINED GenNet's heat maps of the generator's label masks (mask_space) of the same problems" if model.gennet_trained
                          else "ridge heat maps along the label paths (GenNet's training target, blurred)"),
           "tail_network_output": dict({k: (round(v, 4) if isinstance(v, float) else v) for k, v in ev_tail.items()},
                                       note="timed tail: success / length criterion of the OMPL harness on what the trained GenNet PREDICTS from label masks"
                                       if model.gennet_trained else "no trained GenNet checkpoint found: ridge maps"),
           "tail_ridge": {k: (round(v, 4) if isinstance(v, float) else v) for k, v in ev_ridge.items()},
           "extract_ok_rate_untrained_segnet_chain": round(float(net_tail["ok"].float().mean().item()), 4),
           "roofline": {"bound": "mfma", "achieved": round(tflops, 1), "peak": MFMA_PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                        "frac": round(tflops / MFMA_PEAK_BF16_TFLOPS, 4), "traffic": None,
                        "gflop_per_plan": round((seg_fl + gen_fl) / 1e9, 2), "gflop_segnet": round(seg_fl / 1e9, 2),
                        "gflop_gennet": round(gen_fl / 1e9, 3), "counting": "as executed: virtual padding, classifier before the last upsample",
                        "na_kernel": {"bound": "hbm", "ms": round(na_ms, 3), "launches": na_launches,
                                      "algorithmic_bytes": na_bytes, "achieved": round(na_bytes / (na_ms * 1e-3) / 1e9, 1),
                                      "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(na_bytes / (na_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}}}
    if cpu_leg:
        out["cpu_baseline"] = ppnet_cpu_baseline(torch, g, tail_heat, init, end, obs, n_obs, R)
    return out


DUMP_SAMPLE_MAPS = 64           # maps whose full grid / path points --dump-outputs writes (the whole step's grids are 655 MB)
DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(torch, out_dir, pb, mb):
    """--dump-outputs: what the caller of the timed path receives from its last step, as DIR/<name>.npy (float64; the grids
    float32) — stage A's PathsBatch (paths_*) and stage B's MapsBatch (maps_*).  Rows past a count (obstacles, hull) are zeroed:
    the buffers are reused and keep earlier steps' values there.  grid and pathpoint are kept for DUMP_SAMPLE_MAPS maps, rows
    sorted(np.random.default_rng(0).choice(n, DUMP_SAMPLE_MAPS, replace=False)) of the step.  Returns the bytes written."""
    import numpy as np

    def upto(t, n):
        live = torch.arange(t.shape[1], device=t.device)[None, :] < n.reshape(-1, 1)
        return t * live.reshape(live.shape + (1,) * (t.dim() - 2)).to(t.dtype)

    rows = torch.from_numpy(np.sort(np.random.default_rng(0).choice(mb.n, DUMP_SAMPLE_MAPS, replace=False))).to(mb.device)
    arrays = {}
    for name, _ in type(pb.struct)._fields_:
        t = getattr(pb, name)
        if t is not None:
            arrays["paths_" + name] = t
    arrays["paths_obstacles"] = upto(pb.obstacles, pb.n_obstacles)
    arrays["paths_hull"] = upto(pb.hull, pb.hull_n)
    for name, _ in type(mb.struct)._fields_:
        t = getattr(mb, name)
        if t is not None and name not in ("grid", "pathpoint"):
            arrays["maps_" + name] = t
    arrays["maps_obstacles"] = upto(mb.obstacles, mb.n_obstacles[:, 0])
    arrays["maps_grid_sample"] = mb.grid.index_select(0, rows).float()
    if mb.pathpoint is not None:
        arrays["maps_pathpoint_sample"] = mb.pathpoint.index_select(0, rows)
    arrays = {k: v.cpu().numpy() for k, v in arrays.items()}
    arrays = {k: v if v.dtype in (np.float32, np.float64) else v.astype(np.float64) for k, v in arrays.items()}
    total = sum(v.nbytes for v in arrays.values())
    assert total <= DUMP_LIMIT_BYTES, f"--dump-outputs: {total} bytes, more than {DUMP_LIMIT_BYTES}"
    os.makedirs(out_dir, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(out_dir, k + ".npy"), v)
    return total


def pick_path_group(warmup, steps):
    """Steps served by one stage-A launch (BENCH_PATH_GROUP overrides).  Every cross-stream hand-off is a marker packet the
    compute queue drains before the next kernel starts (~5 us on this runtime): with one stage-A launch, one wait and one
    release per GROUP steps instead of per step the stage-B kernels run back to back.  The work per step is unchanged; the
    timed region must hold whole groups, so the group is the largest of 8..1 that divides both --warmup and --steps."""
    env = os.environ.get("BENCH_PATH_GROUP")
    if env:
        return max(1, int(env))
    import math
    g = math.gcd(warmup, steps) if warmup else steps
    for c in range(DEFAULT_PATH_GROUP_MAX, 1, -1):
        if g % c == 0:
            return c
    return 1


DEFAULT_PATH_GROUP_MAX = 8      # measured (gpurun_out/r04/group_*.json): 54.2 M instances/s at 1, 54.3 at 4, 54.85 at 8; see DESIGN.md section 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # Defaults: 0.1 s of untimed steps, then 0.35 s of timed ones.  A step is 0.17-0.2 ms, and the chip needs tens of milliseconds of
    # load to leave its idle clocks: measured back to back on one box (profiles/r02_steps_sweep.txt) 20 timed steps give 45 M
    # instances/s (maps kernel 0.211 ms), 100 steps 52 M, 400 to 16 000 steps a flat 54-55 M (0.175 ms); another box reached
    # 59-60 M at 4 000 steps and fell back to 53-55 M over 3 s.  --steps / --warmup given on the command line are used as they are.
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-ppnet", action="store_true", help="skip the PPNet plans/s leg (BASELINE config 3)")
    ap.add_argument("--ppnet-batch", type=int, default=256)
    ap.add_argument("--ppnet-steps", type=int, default=10)
    ap.add_argument("--no-ppnet-fp32", action="store_true", help="skip the float32 (reference-precision) PPNet leg")
    ap.add_argument("--no-end-to-end", action="store_true", help="skip the config-5 leg (generate -> PPNet -> success rate at 512 x 512)")
    ap.add_argument("--end-to-end-steps", type=int, default=5)
    ap.add_argument("--segnet", choices=["dinat_setr", "nat_uper", "both"], default="both",
                    help="SegNet legs: dinat_setr = BASELINE config 3 (DiNAT-B + SETR-UP, inside the ppnet object); nat_uper = the reference's "
                         "default config (NAT-Base + UPerHead) as a leg of its own; both (default)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (stage A's paths, stage B's maps; rank 0's) to DIR/<name>.npy")
    args = ap.parse_args()

    import torch
    import torch.distributed as dist
    from ppnet_amd import edage, shard

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} needs a torch.distributed.run launch with WORLD_SIZE={args.gpus}")
    # BENCH_REHEARSE_SHARED_GPU: every rank on GPU 0 with a gloo group — a one-GPU box runs the N > 1 control flow (sharding by rank,
    # the record ring and its events, barriers, the max over ranks) before an 8-GPU node sees it; the rows of the gathers travel
    # through the host (shard.all_gather_rows), so the VALUE of such a run is not a measurement and the line says so
    shared_gpu = bool(os.environ.get("BENCH_REHEARSE_SHARED_GPU"))
    if shared_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if shared_gpu:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    # buffers are allocated once and reused every step (resident in HBM).  Stage A is a latency chain (one workgroup
    # per path, ~0.19 ms for 100 paths) that leaves most of the chip idle, so it runs DEPTH batches ahead of stage B on
    # its own HIP streams: while stage B of batch i writes its maps, stage A of batches i+1 .. i+DEPTH is in flight.
    # DEPTH+1 path buffers, events for the hand-off.  Every step launches exactly one stage-A and one stage-B kernel.
    DEPTH = int(os.environ.get("BENCH_DEPTH", "2"))
    # GROUP > 1: one stage-A launch produces the target paths of GROUP consecutive steps (GROUP x PATHS workgroups instead of
    # PATHS: the latency chains fill the chip for a short while instead of trickling beside every stage-B launch); the steps
    # consume views of that batch.  Work per step is unchanged; a timed region of K steps contains K / GROUP stage-A launches.
    GROUP = pick_path_group(args.warmup, args.steps)
    if GROUP > 1 and (args.warmup % GROUP or args.steps % GROUP):
        raise SystemExit(f"BENCH_PATH_GROUP={GROUP}: --warmup and --steps must be multiples of it (the timed region must hold whole groups)")
    # The roofline's kernel duration is sampled over whole GROUPS of launches: a start marker in front of a group's first stage-B
    # launch, the group's closing event (the path-buffer release, there anyway) as the end, elapsed / GROUP per launch — a marker
    # around a single launch of a marker-free run would add its own ~5 us to that launch alone.  Every SAMPLE_EVERY-th group: at
    # least 10 launches from --steps 20 on, 500 at the default window.  (GROUP = 1: an event pair around every 2nd / 4th launch.)
    n_groups = max(1, args.steps // GROUP)
    SAMPLE_EVERY = max(1, (n_groups * GROUP) // 500) if GROUP > 1 else (2 if args.steps < 80 else 4)
    TIMED_EVERY = SAMPLE_EVERY                    # (stage A's sampled launches use the same stride, in groups)
    NPB = DEPTH + 1
    pbs = [edage.PathsBatch(PATHS * GROUP, R, MAP_SIZE, CLEARANCE, dev) for _ in range(NPB)]
    pviews = [[pb.view(k * PATHS, PATHS) for k in range(GROUP)] for pb in pbs]
    # N > 1: the end-of-batch all-gather of the fixed-size records.  Stage B writes each step's records straight into a slice of
    # a staging ring (shard.RecordRing) and ONE collective ships the records of GATHER steps — enough steps that a gather carries
    # >= 1 M instances over all ranks, as SURVEY 8e sizes the exchange — on its own stream beside the next group's steps.
    exchange = world > 1 or bool(os.environ.get("BENCH_FORCE_EXCHANGE"))      # the env knob rehearses the stream logic on one GPU
    n_local = PATHS * PLACEMENTS
    mb = edage.MapsBatch(n_local, R, K, dev)
    ring, mviews = None, None
    if exchange:
        GATHER = int(os.environ.get("BENCH_GATHER_STEPS", "0")) or shard.gather_steps(world, n_local)
        ring = shard.RecordRing(world, n_local, GATHER, dev, torch.cuda.Stream(dev))
        mviews = [[mb.with_records(ring.slot_view(sl, k)) for k in range(GATHER)] for sl in range(2)]
    prio = os.environ.get("BENCH_PRIO", "")
    lo_p, hi_p = torch.cuda.Stream.priority_range() if hasattr(torch.cuda.Stream, "priority_range") else (0, -1)
    s_paths = [torch.cuda.Stream(dev, priority=hi_p if prio == "paths" else (lo_p if prio == "maps" else 0)) for _ in range(DEPTH)]
    s_maps = torch.cuda.current_stream(dev)
    if prio == "maps":
        s_maps = torch.cuda.Stream(dev, priority=hi_p)
        s_maps.wait_stream(torch.cuda.current_stream(dev))
        torch.cuda.set_stream(s_maps)
    ready = [None] * NPB          # paths of buffer b are complete
    consumed = [None] * NPB       # the maps kernel reading buffer b has finished
    launched = [-1]               # newest batch whose stage A has been launched
    stage_a_evs = []              # (start, end) events around the sampled stage-A launches of the timed region, on their own streams
    stage_a_on = [False]
    id_shift = [0]                # steps subtracted from a step's index to give its batch id (set after the clock-warm phase)
    last_out = [None]             # (paths, maps) of the newest step

    def launch_paths(it):
        """Stage A of path group `it` (the paths of steps it*GROUP .. it*GROUP + GROUP - 1)."""
        b = it % NPB
        sp = s_paths[it % DEPTH]
        bid = it - id_shift[0] // GROUP
        with torch.cuda.stream(sp):
            if consumed[b] is not None:
                sp.wait_event(consumed[b])
            ea = None
            if stage_a_on[0] and it % TIMED_EVERY == 0:
                ea = torch.cuda.Event(enable_timing=True)
                ea.record(sp)
            if GROUP == 1:
                first_path, _, _ = shard.local_ids(PATHS * world, PLACEMENTS, rank, world, batch_index=bid)
                edage.generate_paths(PATHS, R, MAP_SIZE, CLEARANCE, seed=SEED, first_path_id=first_path, device=dev, out=pbs[b])
            else:
                # path ids of this rank for GROUP consecutive batches are not contiguous across ranks: one launch per batch id
                # range would defeat the grouping, so a group draws the ids [first(it*GROUP) .. ) of a world whose batch is
                # GROUP times as large — same streams for any N, every id used once
                first_path, _, _ = shard.local_ids(PATHS * GROUP * world, PLACEMENTS, rank, world, batch_index=bid)
                edage.generate_paths(PATHS * GROUP, R, MAP_SIZE, CLEARANCE, seed=SEED, first_path_id=first_path, device=dev, out=pbs[b])
            ready[b] = torch.cuda.Event(enable_timing=ea is not None)
            ready[b].record(sp)
            if ea is not None:
                stage_a_evs.append((ea, ready[b]))
        launched[0] = it

    def step(it):
        # a fresh batch every step: path / map ids advance so no two steps generate the same instances
        grp, sub = divmod(it, GROUP)
        b = grp % NPB
        if GROUP == 1:
            _, _, first_map = shard.local_ids(PATHS * world, PLACEMENTS, rank, world, batch_index=it - id_shift[0])
        else:
            fp, _, _ = shard.local_ids(PATHS * GROUP * world, PLACEMENTS, rank, world, batch_index=grp - id_shift[0] // GROUP)
            first_map = (fp + sub * PATHS) * PLACEMENTS
        if sub == 0:
            while launched[0] < grp + DEPTH - 1:
                launch_paths(launched[0] + 1)     # pipeline fill (first step only)
            launch_paths(grp + DEPTH)             # this group's stage A: the paths stage B will reach DEPTH groups from now
            s_maps.wait_event(ready[b])
            ready[b] = None
        # every event is a marker packet the queue has to drain before the next kernel starts (~5 us each on this
        # runtime), so the stream carries one per step (it doubles as the buffer hand-off) and a start marker only on
        # every TIMED_EVERY-th step: those launches are the sample the roofline's kernel duration is averaged over
        sampled = (grp % SAMPLE_EVERY == 0) or args.steps < SAMPLE_EVERY * GROUP
        ev0 = None
        if sampled and sub == 0:
            ev0 = torch.cuda.Event(enable_timing=True)
            ev0.record()
        target = mb
        if exchange:
            ring.begin_step()                 # before a group's first step: the slot's previous collective has read it
            target = mviews[ring.slot][ring.k]
        edage.generate_maps(pviews[b][sub], PLACEMENTS, OBST_SIZE, K, seed=SEED, first_map_id=first_map, out=target)
        last_out[0] = (pviews[b][sub], target)
        ev1 = None
        if sub == GROUP - 1:
            ev1 = torch.cuda.Event(enable_timing=sampled)      # a timestamp only on the sampled groups
            ev1.record()
        if sub == GROUP - 1:
            consumed[b] = ev1                     # the last step of the group releases the path buffer
        if exchange:
            ring.end_step()                   # after the group's last step: one all-gather on the communication stream
        return ev0, ev1

    for it in range(args.warmup):
        step(it)
    # Clock-warm phase (untimed, reported): the identical step loop for a fixed wall time, independent of --warmup.  A step is
    # 0.17-0.2 ms and the chip needs ~0.1 s of load to leave its idle clocks; without this a `--steps 20 --warmup 5` run (4 ms)
    # measures the idle-clock kernel (profiles/r02_steps_sweep.txt).  The timed region below is exactly --steps steps.
    warm_target_s = float(os.environ.get("BENCH_CLOCK_WARM_MS", "150")) * 1e-3
    warm_steps = 0
    torch.cuda.synchronize()
    tw = time.perf_counter()
    while True:
        # N > 1: every step carries a collective, so all ranks must run the SAME number of warm steps — the decision to go on is
        # taken on the slowest rank's clock (one all-reduce per chunk of 25 steps, outside the timed region)
        elapsed_w = shard.agreed_max(time.perf_counter() - tw, world, dev)
        if elapsed_w >= warm_target_s:
            break
        for _ in range(25 * GROUP):
            step(args.warmup + warm_steps)
            warm_steps += 1
        torch.cuda.synchronize()
    clock_warm_ms = (time.perf_counter() - tw) * 1e3
    first = args.warmup + warm_steps
    # The clock-warm phase runs for a wall time, so its step count differs from run to run.  The timed steps take the batch ids
    # that follow --warmup instead (same arguments, same instances in every run); the stage-A groups already launched ahead
    # for them are launched again under those ids, outside the clock.
    id_shift[0] = warm_steps
    for g in range(first // GROUP, launched[0] + 1):
        launch_paths(g)
    if exchange:
        ring.flush()                          # the warm steps' partial group leaves outside the clock
        gathers_before = ring.n_gathers
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    stage_a_on[0] = True
    t0 = time.perf_counter()
    evs = [step(first + it) for it in range(args.steps)]
    stage_a_on[0] = False
    if exchange:
        ring.flush()                          # every record of the timed steps is gathered inside the clock
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        elapsed = shard.max_over_ranks(elapsed, dev)

    starts = [a for a, _ in evs if a is not None]
    ends = [evs[i + GROUP - 1][1] for i, (a, _) in enumerate(evs) if a is not None]
    timed = list(zip(starts, ends))
    maps_kernel_ms = sum(a.elapsed_time(b) for a, b in timed) / (len(timed) * GROUP)
    stage_a_ms = sum(a.elapsed_time(b) for a, b in stage_a_evs) / len(stage_a_evs) if stage_a_evs else None
    k_tot = float(mb.n_obstacles[:, 0].double().mean().item())
    k_pocket = float(pbs[0].n_obstacles.double().mean().item())
    placed = float(((mb.flags & 2) == 0).double().mean().item())
    total_instances = world * n_local * args.steps
    value = total_instances / elapsed
    dumped = None
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(torch, args.dump_outputs, *last_out[0])

    ppnet = None
    if not args.no_ppnet:
        last = first + args.steps - 1
        hold = {}
        ppnet = ppnet_leg(torch, dev, pviews[(last // GROUP) % NPB][last % GROUP], mb, args.ppnet_batch, args.ppnet_steps, world, rank,
                          cpu_leg=(world == 1 and not args.no_cpu_baseline), hold=hold)
    if rank == 0:
        bytes_per_launch = algorithmic_bytes_per_map(k_tot, k_pocket) * n_local
        achieved = bytes_per_launch / (maps_kernel_ms * 1e-3) / 1e9
        out = {
            "metric": "edage_pp_map_path_instances_per_sec",
            "value": round(value, 1),
            "unit": "instances/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "clock_warm_ms": round(clock_warm_ms, 1), "clock_warm_steps": warm_steps,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": "EDaGe-PP config 2: 100 target paths x 100 placements = 10000 maps+paths per GPU per step",
                       "resolution": R, "obstacles_num": K, "clearance": CLEARANCE, "map_size": MAP_SIZE,
                       "rng": "philox4x32-10", "parallelism": f"instances sharded over {world} GPU(s), end-of-batch all-gather"},
            "roofline": {"bound": "hbm", "kernel": "edage_maps_kernel_t<3>", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": measured_traffic(),
                         "kernel_ms": round(maps_kernel_ms, 4), "timed_launches": len(timed) * GROUP, "units_per_launch": n_local,
                         "algorithmic_bytes_per_map": round(algorithmic_bytes_per_map(k_tot, k_pocket), 1),
                         "survey_bytes_per_map": round(2 * R * R + 16384 + 12.0 * k_tot, 1)},
            # stage A paths/s, stage B maps/s (each kernel's own launch time by events on its stream, while
            # the other stage runs beside it) and the end-to-end figure (`value`)
            "stage_a": {"kernel": "edage_paths_kernel", "kernel_ms": round(stage_a_ms, 4) if stage_a_ms else None,
                        "paths_per_launch": PATHS * GROUP, "timed_launches": len(stage_a_evs),
                        "paths_per_s": round(PATHS * GROUP / (stage_a_ms * 1e-3), 1) if stage_a_ms else None,
                        "note": "a latency chain, one workgroup per path, in flight beside stage B on its own streams"},
            "stage_b": {"kernel": "edage_maps_kernel_t<3>", "kernel_ms": round(maps_kernel_ms, 4),
                        "maps_per_s": round(n_local / (maps_kernel_ms * 1e-3), 1)},
            "exchange": ({"gather_every_steps": ring.G, "gathers_in_timed_region": ring.n_gathers - gathers_before,
                          "bytes_per_rank_per_gather": ring.G * n_local * shard.RECORD_WIDTH * 8,
                          "collective": ("all_gather_into_tensor (gloo, rows through the host: rehearsal)" if shared_gpu else "all_gather_into_tensor (RCCL)") if world > 1 else "copy (BENCH_FORCE_EXCHANGE rehearsal on one GPU)"}
                         if exchange else None),
            "path_group": GROUP,
            "placement_success": round(placed, 4),
            "mean_obstacles_per_map": round(k_tot, 2),
        }
        if dumped is not None:
            out["dump_outputs"] = {"dir": args.dump_outputs, "bytes": dumped}
        if shared_gpu:
            out["rehearsal"] = ("BENCH_REHEARSE_SHARED_GPU: every rank on one GPU, gloo group, gathered rows through the host - the N > 1 control "
                                "flow run for its own sake, not a measurement")
        if ppnet is not None:
            out["ppnet"] = ppnet
            if world == 1 and args.segnet in ("nat_uper", "both"):
                try:
                    out["segnet_nat_uper"] = segnet_nat_uper_leg(torch, dev, mb.grid, args.ppnet_batch)
                except Exception as e:
                    out["segnet_nat_uper"] = {"error": repr(e)[:300]}
            if world == 1 and not args.no_ppnet_fp32:
                try:
                    f32 = ppnet_fp32_leg(torch, dev, mb.grid, args.ppnet_batch, parity_with=hold)
                    # the bf16 figure's tolerance, measured in this run against the float32 leg on the same grids
                    ppnet["parity"] = f32.pop("parity")
                    f32["bf16_speedup"] = round(ppnet["ms_segnet"] + ppnet["ms_gennet"] and f32["ms_per_batch"] / (ppnet["ms_segnet"] + ppnet["ms_gennet"]), 2)
                    out["ppnet_fp32"] = f32
                except Exception as e:
                    out["ppnet_fp32"] = {"error": repr(e)[:300]}
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline()
    if not args.no_ppnet and not args.no_end_to_end:
        hold = None                            # (the config-3 object is no longer needed)
        try:
            e2e = end_to_end_leg(torch, dev, args.end_to_end_steps, world, rank, cpu_leg=(world == 1 and not args.no_cpu_baseline))
        except Exception as e:
            if world > 1:
                raise                          # a rank that skipped the leg's collectives would hang the others
            e2e = {"error": repr(e)[:300]}
        if rank == 0:
            out["end_to_end_r512"] = e2e
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
