"""UPerPUPHead (the dense NAT / Swin configs) at R = 256, batch 256, bfloat16, prepared inference: SegNet ms per batch (labels_u8 on
occupancy codes) and the head alone on the backbone's features (device events, warmed), and from shapes the head's matrix work and
the bytes of its FPN output assembly (ppn_upsample2x_concat_nhwc).

    python tools/uperpup_timing.py [--batch 256] [--res 256] [--configs nat,swin] [--reps 5]
        prints ms per batch, the head's GFLOP and the concatenation's bytes per batch
    python tools/uperpup_timing.py --head-only --configs nat --reps 3
        the head alone, untimed (the workload of a `rocprofv3 --kernel-trace --stats` run)
    python tools/uperpup_timing.py --stats kernel_stats.csv --configs nat --reps 3
        no GPU: the achieved FLOP/s of the head's 3x3 convolution kernels against 2.5 PF/s bf16 and the bytes/s of the
        concatenation kernel against 8 TB/s, from that run's kernel totals (over 2 + reps head calls, the warm-up included)"""
import argparse
import csv
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_FLOPS, PEAK_BYTES = 2.5e15, 8e12                                         # MI355X dense bf16, HBM
NUM_CONVS = {"nat": (1, 2, 3, 4), "swin": (2, 3, 4, 5)}
NAMES = {"nat": "NAT_BASE_UPERPUP", "swin": "SWIN_BASE_UPERPUP"}


def head_work(num_convs, R, B, in_channels=(128, 256, 512, 1024), ch=256, pool_scales=(1, 2, 3, 6)):
    """(FLOP of the 3x3 convolutions, FLOP of the 1x1 ones, bytes the concatenation kernel reads + writes) per batch, bf16."""
    sides = [R // 4 >> i for i in range(4)]
    conv3 = 2 * 9 * (in_channels[-1] + len(pool_scales) * ch) * ch * sides[-1] ** 2          # bottleneck
    for s, n in zip(sides, num_convs):
        conv3 += sum(2 * 9 * ch * ch * (s << j) ** 2 for j in range(n))                      # the chains
    out = sides[0] << num_convs[0]
    conv3 += 2 * 9 * len(in_channels) * ch * ch * out ** 2 + 2 * ch * 2 * out ** 2         # fpn_bottleneck + conv_seg (one kernel)
    conv1 = sum(2 * c * ch * s * s for c, s in zip(in_channels[:-1], sides[:-1])) + sum(2 * in_channels[-1] * ch * p * p for p in pool_scales)
    cat = 2 * (len(in_channels) * ch * (out // 2) ** 2 + len(in_channels) * ch * out ** 2)
    return conv3 * B, conv1 * B, cat * B


def stats(path, cfg, R, B, calls):
    tot = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            tot[row["Name"]] = tot.get(row["Name"], 0) + int(row["TotalDurationNs"])
    conv_ns = sum(v for k, v in tot.items() if "gemm_bf16_kernel<1," in k)   # AMode CONV3 (csrc/mfma_gemm.h): the 3x3 convolutions
    cat_ns = sum(v for k, v in tot.items() if "upsample2x_concat_kernel" in k)
    f3, _, cb = head_work(NUM_CONVS[cfg], R, B)
    print(f"{cfg}: 3x3 convolution kernels {conv_ns / calls / 1e6:8.3f} ms per batch, {f3 / (conv_ns / calls * 1e-9) / 1e12:7.1f} TFLOP/s"
          f" = {f3 / (conv_ns / calls * 1e-9) / PEAK_FLOPS:5.3f} of 2.5 PF/s")
    print(f"{cfg}: ppn_upsample2x_concat_nhwc {cat_ns / calls / 1e6:8.3f} ms per batch, {cb / 1e9:6.2f} GB, "
          f"{cb / (cat_ns / calls * 1e-9) / 1e12:5.2f} TB/s = {cb / (cat_ns / calls * 1e-9) / PEAK_BYTES:5.3f} of 8 TB/s")
    for k, v in sorted(tot.items(), key=lambda kv: -kv[1])[:12]:
        print(f"    {v / calls / 1e6:8.3f} ms  {k[:150]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--configs", default="nat,swin")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--head-only", action="store_true")
    ap.add_argument("--stats")
    a = ap.parse_args()
    B, R = a.batch, a.res
    cfgs = a.configs.split(",")
    if a.stats is not None:
        for c in cfgs:
            stats(a.stats, c, R, B, 2 + a.reps)
        return
    import torch
    from ppnet_amd import segnet
    dev = torch.device("cuda", 0)

    def timed(fn, reps):
        for _ in range(2):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    g = torch.Generator().manual_seed(0)
    codes = (torch.rand(B, 1, R // 16, R // 16, generator=g) > 0.4).float()
    codes = (torch.nn.functional.interpolate(codes, size=(R, R), mode="nearest")[:, 0] * 255).to(torch.uint8).to(dev)
    with torch.no_grad():
        for c in cfgs:
            torch.manual_seed(0)
            m = segnet.randomize_neutral_parameters(segnet.SegNet.from_config(getattr(segnet, NAMES[c]))).eval().to(dev).to(torch.bfloat16)
            m.prepare_inference()
            if a.head_only:                                                    # level features of the backbone's shapes: no backbone kernel in the trace
                feats = [torch.randn(B, C, R // s, R // s, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
                         for C, s in ((128, 4), (256, 8), (512, 16), (1024, 32))]
                for _ in range(2 + a.reps):
                    m.decode_head(feats)
                torch.cuda.synchronize()
                print(f"{c}: {2 + a.reps} head calls at batch {B}, R {R}", flush=True)
                continue
            feats = m.backbone(codes)
            ms_head = timed(lambda: m.decode_head(feats), a.reps)
            del feats
            ms_seg = timed(lambda: m.labels_u8(codes), a.reps)
            f3, f1, cb = head_work(NUM_CONVS[c], R, B)
            print(f"{NAMES[c]:18s} R {R} batch {B}: SegNet {ms_seg:8.2f} ms per batch, head alone {ms_head:8.2f} ms per batch "
                  f"({(f3 + f1) / 1e12:6.2f} TFLOP per batch: {(f3 + f1) / (ms_head * 1e-3) / 1e12:6.1f} TFLOP/s over the head's wall time; "
                  f"concatenation {cb / 1e9:5.2f} GB per batch)", flush=True)
            del m
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
