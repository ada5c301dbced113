"""Times Swin's window attention on every Swin-B level at 256 x 256, batch 256, bfloat16: ppn_swin_wmsa_fwd per launch (shift 0
and 3) with its HBM fraction (8 C bytes per real token — q, k, v read once, out written once — at 8 TB/s), the same launches as
the reference's torch op chain (pad, roll, window partition, two matmuls, bias, mask, softmax, reverse, roll, crop:
ppnet_amd.swin.window_attention) on the same GPU, and SegNet ms per batch for both Swin-B configurations next to DiNAT-B's
(prepared bfloat16 inference, labels_u8 on occupancy codes).  Prints one line per measurement; the output is kept under profiles/."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ppnet_amd import segnet, swin  # noqa: E402

dev = torch.device("cuda", 0)
B = int(os.environ.get("SWIN_TIMING_BATCH", "256"))


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


with torch.no_grad():
    for side, C, heads in ((64, 128, 4), (32, 256, 8), (16, 512, 16), (8, 1024, 32)):
        qkv = torch.randn(B, side, side, 3 * C, device=dev, dtype=torch.bfloat16)
        pad = torch.randn(3 * C, device=dev, dtype=torch.bfloat16) * 0.2
        rpb = torch.randn(heads, 13, 13, device=dev)
        table = rpb.reshape(heads, 169).t().contiguous()
        byts = B * side * side * 8 * C
        for shift in (0, 3):
            ms = timed(lambda: swin.wmsa_forward(qkv, pad, rpb, heads, shift, 32 ** -0.5), 20)
            mt = timed(lambda: swin.window_attention(qkv, pad, table, heads, shift, 32 ** -0.5), 5)
            print(f"level {side:3d}x{side:<3d} C {C:4d} heads {heads:2d} shift {shift}: kernel {ms:7.4f} ms  hbm-time frac {byts / 8e12 * 1e3 / ms:5.2f}"
                  f"   torch chain {mt:7.3f} ms  speed-up {mt / ms:6.1f}x", flush=True)
        del qkv

    SB = int(os.environ.get("SWIN_TIMING_SEG_BATCH", "64"))
    codes = (torch.rand(SB, 16, 16, device=dev) > 0.4).float()
    codes = (torch.nn.functional.interpolate(codes[:, None], size=(256, 256), mode="nearest")[:, 0] * 255).to(torch.uint8)
    for name in ("SWIN_BASE_UPER", "SWIN_BASE_SETRUP", "DINAT_BASE", "NAT_BASE_UPER"):
        m = segnet.randomize_neutral_parameters(segnet.SegNet.from_config(getattr(segnet, name))).eval().to(dev).to(torch.bfloat16)
        m.prepare_inference()
        ms = timed(lambda: m.labels_u8(codes), 5)
        print(f"SegNet {name:16s} R 256 batch {SB}: {ms:8.2f} ms per batch", flush=True)
        del m
        torch.cuda.empty_cache()
