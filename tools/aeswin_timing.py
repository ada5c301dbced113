"""Times AESwin's window attention on the GPU: for the five Swin stages' shapes at R = 224 (token grids 56 / 28 / 14 / 14 / 28) and
R = 256 (64 / 32 / 16 / 16 / 32, every stage padded), batch 64 (AESWIN_TIMING_BATCH), in float32 and bfloat16, both shifts — the
HIP kernel per launch (swin.wmsa_forward: ppn_wmsa_fwd, and ppn_swin_wmsa_fwd for the window-7 / head-dim-32 stages) beside the
torch composition of the reference's op chain (swin.window_attention) — and the whole prepared bfloat16 forward of
AESwin(1, 1, R, 192) with the kernels and with PPNET_LIBRARY_WMSA=1.  Every figure is the median over alternated rounds (kernel,
composition, kernel, ...), each round a device-event time over several calls.  One line per measurement; DESIGN.md section 30
holds the table."""
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ppnet_amd import swin  # noqa: E402
from ppnet_amd.gennet import AESwin  # noqa: E402

dev = torch.device("cuda", 0)
B = int(os.environ.get("AESWIN_TIMING_BATCH", "64"))
ROUNDS = int(os.environ.get("AESWIN_TIMING_ROUNDS", "5"))
DIM = 192


def once(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternated(fa, ra, fb, rb):
    """Medians (and min-max spreads) of ROUNDS alternated rounds of fa and fb."""
    fa(), fb()                                                           # warm-up: code objects, the library's algorithm choices
    ta, tb = [], []
    for _ in range(ROUNDS):
        ta.append(once(fa, ra))
        tb.append(once(fb, rb))
    return statistics.median(ta), statistics.median(tb), (min(ta), max(ta)), (min(tb), max(tb))


with torch.no_grad():
    for R in (224, 256):
        g = R >> int(math.log2(R // 56))                                 # the token grid behind the stride-2 conv stages (ae_swin.py:21)
        for stage, (side, heads, window) in enumerate(((g, 6, 7), (g // 2, 12, 14), (g // 4, 24, 14), (g // 4, 12, 14), (g // 2, 6, 7))):
            d = DIM // heads
            for dtype in (torch.float32, torch.bfloat16):
                qkv = torch.randn(B, side, side, 3 * DIM, device=dev, dtype=dtype)
                pad = torch.randn(3 * DIM, device=dev, dtype=dtype) * 0.2
                rpb = torch.randn(heads, 2 * window - 1, 2 * window - 1, device=dev) * 0.5
                table = rpb.reshape(heads, -1).t().contiguous().to(dtype)
                for shift in (0, window // 2):
                    mk, mt, sk, st = alternated(lambda: swin.wmsa_forward(qkv, pad, rpb, heads, shift, d ** -0.5, window), 10,
                                                lambda: swin.window_attention(qkv, pad, table, heads, shift, d ** -0.5, window), 3)
                    print(f"R {R} stage {stage} grid {side:2d}x{side:<2d} heads {heads:2d} d {d:2d} window {window:2d} shift {shift} {str(dtype)[6:]:8s}: "
                          f"kernel {mk:7.4f} ms ({sk[0]:.4f}-{sk[1]:.4f})  composition {mt:8.4f} ms ({st[0]:.4f}-{st[1]:.4f})  "
                          f"ratio {mt / mk:6.2f}x", flush=True)
                del qkv
        torch.manual_seed(0)
        m = AESwin(1, 1, R, DIM).eval().prepare_inference().to(dev).to(torch.bfloat16)
        x = (torch.rand(B, 1, R, R, device=dev) > 0.5).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)

        def forward(library):
            if library:
                os.environ["PPNET_LIBRARY_WMSA"] = "1"
            else:
                os.environ.pop("PPNET_LIBRARY_WMSA", None)
            m(x)
            os.environ.pop("PPNET_LIBRARY_WMSA", None)

        mk, mt, sk, st = alternated(lambda: forward(False), 3, lambda: forward(True), 3)
        print(f"AESwin(1, 1, {R}, {DIM}) prepared bfloat16 forward, batch {B}: kernels {mk:8.3f} ms ({sk[0]:.3f}-{sk[1]:.3f})  "
              f"PPNET_LIBRARY_WMSA=1 {mt:8.3f} ms ({st[0]:.3f}-{st[1]:.3f})  ratio {mt / mk:5.2f}x", flush=True)
        del m, x
        torch.cuda.empty_cache()
