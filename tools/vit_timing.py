"""Times ViT's global attention at the two ViT-B shapes of DESIGN.md section 11 — R = 256, batch 256 (N = 256) and R = 512, batch 64
(N = 1024), 12 heads of 64, bfloat16 — as ppn_mhsa_fwd per launch (= per layer), as the torch op chain (matmul, softmax, matmul) and
as F.scaled_dot_product_attention on the same inputs.  Each is reported as a fraction of 8 TB/s for its unavoidable bytes (qkv read
once, out written once: 8 C bytes per token) and of the 2.5 PF/s bf16 MFMA peak (4 B heads N^2 64 FLOP).  Then SegNet ms per batch
for VIT_BASE_SETRUP at R = 256, batch 64 (prepared bfloat16 inference, labels_u8 on occupancy codes) next to SWIN_BASE_SETRUP and
DINAT_BASE on the same GPU.  `--segnet-only`: just two ViT SegNet batches (for a kernel trace).  The output is kept under profiles/."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from ppnet_amd import segnet, vit  # noqa: E402

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


def codes(B, R):
    c = (torch.rand(B, R // 16, R // 16, device=dev) > 0.4).float()
    return (F.interpolate(c[:, None], size=(R, R), mode="nearest")[:, 0] * 255).to(torch.uint8)


def vit_segnet():
    m = segnet.randomize_neutral_parameters(segnet.SegNet.from_config(segnet.VIT_BASE_SETRUP))
    with torch.no_grad():
        m.backbone.pos_embed.normal_(0.0, 0.02)
        m.backbone.cls_token.normal_(0.0, 0.02)
    return m.eval().to(dev).to(torch.bfloat16).prepare_inference()


with torch.no_grad():
    if "--segnet-only" in sys.argv:
        m, c = vit_segnet(), codes(64, 256)
        for _ in range(2):
            m.labels_u8(c)
        torch.cuda.synchronize()
        print("ViT-B SegNet: 2 batches of 64 at R 256 done", flush=True)
        sys.exit(0)
    heads, C = 12, 768
    scale = 64 ** -0.5
    for R, B in ((256, 256), (512, 64)):
        N = (R // 16) ** 2
        qkv = torch.randn(B, N, 3 * C, device=dev, dtype=torch.bfloat16)
        q, k, v = qkv.view(B, N, 3, heads, 64).permute(2, 0, 3, 1, 4).unbind(0)      # [B, heads, N, 64] views

        def chain():
            p = torch.softmax((q @ k.transpose(-2, -1)) * scale, dim=-1)
            return (p @ v).transpose(1, 2).reshape(B, N, C)

        def sdpa():
            return F.scaled_dot_product_attention(q, k, v, scale=scale).transpose(1, 2).reshape(B, N, C)

        byts, flop = B * N * 8 * C, 4.0 * B * heads * N * N * 64
        for name, fn, reps in (("ppn_mhsa_fwd", lambda: vit.mhsa_forward(qkv, heads, scale), 20), ("torch chain", chain, 5),
                               ("F.sdpa", sdpa, 10)):
            ms = timed(fn, reps)
            if name == "ppn_mhsa_fwd":
                mk = ms
            print(f"R {R:3d} batch {B:3d} N {N:4d}: {name:12s} {ms:8.4f} ms per layer  hbm frac {byts / 8e12 * 1e3 / ms:5.2f}  "
                  f"mfma frac {flop / 2.5e15 * 1e3 / ms:5.3f}  kernel speed-up {ms / mk:5.2f}x", flush=True)
        del qkv, q, k, v
        torch.cuda.empty_cache()

    SB = int(os.environ.get("VIT_TIMING_SEG_BATCH", "64"))
    c = codes(SB, 256)
    for name in ("VIT_BASE_SETRUP", "SWIN_BASE_SETRUP", "DINAT_BASE"):
        if name == "VIT_BASE_SETRUP":
            m = vit_segnet()
        else:
            m = segnet.randomize_neutral_parameters(segnet.SegNet.from_config(getattr(segnet, name))).eval().to(dev).to(torch.bfloat16)
            m.prepare_inference()
        ms = timed(lambda: m.labels_u8(c), 5)
        print(f"SegNet {name:16s} R 256 batch {SB}: {ms:8.2f} ms per batch", flush=True)
        del m
        torch.cuda.empty_cache()
