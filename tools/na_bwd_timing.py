"""Times the NA backward (query pass + key pass + drpb sum) on the GPU (diagnostic).

  python tools/na_bwd_timing.py         the (level, dilation) shapes of DiNAT-B at 256x256, 8 images, float32 — the SegNet training
                                        step's unpadded shapes, through autograd.  NA_BWD_B overrides the batch.
  python tools/na_bwd_timing.py vpad    the five padded DiNAT-B layers at R = 224 and 256, batch 8 and 64 (NA_BWD_B: one batch), both
                                        dtypes: ppn_na2d_bwd_vpad on the real tokens beside ppn_na2d_bwd on the materialised grid, per
                                        launch through the C ABI, and the attention forward + backward pair the same way
                                        (ppn_na2d_fwd_vpad + ppn_na2d_bwd_vpad beside ppn_na2d_fwd + ppn_na2d_bwd).  Device events
                                        around 10 launches, the two sides alternated, the minimum of three rounds."""
import ctypes
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ppnet_amd import _lib as L
from ppnet_amd import na
from ppnet_amd.na import na2d_autograd

dev = torch.device("cuda", 0)
SCALE = 32 ** -0.5


def unpadded():
    B = int(os.environ.get("NA_BWD_B", "8"))
    tot = 0.0
    for side, C, heads, dils, layers in ((64, 128, 4, (1, 8), (2, 1)), (32, 256, 8, (1, 4), (2, 2)), (16, 512, 16, (1, 2), (9, 9)), (8, 1024, 32, (1,), (5,))):
        for d, n in zip(dils, layers):
            qkv = torch.randn(B, side, side, 3 * C, device=dev, requires_grad=True)
            rpb = torch.randn(heads, 13, 13, device=dev, requires_grad=True)
            out = na2d_autograd(qkv, rpb, heads, d, SCALE)
            g = torch.randn_like(out)
            for _ in range(3):
                out.backward(g, retain_graph=True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                out.backward(g, retain_graph=True)
            e1.record(); torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / 10
            tot += ms * n
            print(f"side {side:3d} C {C:4d} heads {heads:2d} d {d}: {ms * 1e3:7.1f} us per backward (incl. autograd glue)  x {n} layers")
    print(f"DiNAT-B, {B} images: {tot:.2f} ms of NA backward per step")


def _timed(fn, n=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def vpad():
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    batches = (int(os.environ["NA_BWD_B"]),) if os.environ.get("NA_BWD_B") else (8, 64)
    # level, C, heads, dilation, layers of DINAT_BASE with that dilation on that level
    layers = ((0, 128, 4, 16, 1), (1, 256, 8, 8, 1), (2, 512, 16, 3, 3), (2, 512, 16, 4, 3), (3, 1024, 32, 2, 2))
    for R in (224, 256):
        for dtype in (torch.float32, torch.bfloat16):
            dt = 0 if dtype == torch.float32 else 1
            for B in batches:
                tot = [0.0] * 4
                for level, C, heads, d, count in layers:
                    Hr = R // (4 << level)
                    H = max(Hr, 7 * d)
                    real = torch.randn(B, Hr, Hr, 3 * C, device=dev).to(dtype)
                    pad = (torch.randn(3 * C, device=dev) * 0.5).to(dtype)
                    rpb = torch.randn(heads, 13, 13, device=dev) * 0.5
                    full = pad.expand(B, H, H, 3 * C).clone()
                    full[:, :Hr, :Hr] = real
                    dout = torch.randn(B, Hr, Hr, C, device=dev).to(dtype)
                    dfull = torch.zeros(B, H, H, C, device=dev, dtype=dtype)
                    dfull[:, :Hr, :Hr] = dout
                    dq_v, dq_m = torch.empty_like(real), torch.empty_like(full)
                    dpad, drpb = torch.empty(3 * C, device=dev), torch.empty(heads, 13, 13, device=dev)
                    need_v = L.lib.ppn_na2d_bwd_vpad_workspace(B, H, H, Hr, Hr, heads, d)
                    need_m = L.lib.ppn_na2d_bwd_workspace(B, H, H, heads, d)
                    ws_v, ws_m = torch.empty(need_v, device=dev), torch.empty(need_m, device=dev)
                    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

                    def bwd_v():
                        L.check(L.lib.ppn_na2d_bwd_vpad(P(real), P(pad), P(rpb), P(dout), P(dq_v), P(dpad), P(drpb), P(ws_v), need_v, B, H, H, Hr, Hr,
                                                        heads, d, SCALE, dt, stream), "ppn_na2d_bwd_vpad")

                    def bwd_m():
                        L.check(L.lib.ppn_na2d_bwd(P(full), P(rpb), P(dfull), P(dq_m), P(drpb), P(ws_m), need_m, B, H, H, heads, d, SCALE, dt, stream),
                                "ppn_na2d_bwd")

                    def pair_v():
                        na.na2d_forward(real, rpb, heads, d, SCALE, pad_kv=pad, padded_hw=(H, H))
                        bwd_v()

                    def pair_m():
                        na.na2d_forward(full, rpb, heads, d, SCALE)
                        bwd_m()
                    fns = (bwd_v, bwd_m, pair_v, pair_m)
                    for f in fns:
                        f()
                    torch.cuda.synchronize()
                    best = [float("inf")] * 4
                    for _ in range(3):
                        for i, f in enumerate(fns):
                            best[i] = min(best[i], _timed(f))
                    for i in range(4):
                        tot[i] += best[i] * count
                    print(f"R {R} {str(dtype)[6:]:8s} batch {B:2d} level {level} {Hr:2d}x{Hr:<2d} -> {H:3d}x{H:<3d} C {C:4d} dilation {d:2d} x{count}: "
                          f"bwd vpad {best[0]:7.3f} ms, materialised {best[1]:7.3f} ms ({best[1] / best[0]:4.2f}x) | "
                          f"fwd + bwd vpad {best[2]:7.3f} ms, materialised {best[3]:7.3f} ms ({best[3] / best[2]:4.2f}x)", flush=True)
                print(f"R {R} {str(dtype)[6:]:8s} batch {B:2d} DiNAT-B's 10 padded layers: bwd vpad {tot[0]:7.2f} ms, materialised {tot[1]:7.2f} ms | "
                      f"fwd + bwd vpad {tot[2]:7.2f} ms, materialised {tot[3]:7.2f} ms", flush=True)


if __name__ == "__main__":
    vpad() if sys.argv[1:] == ["vpad"] else unpadded()
