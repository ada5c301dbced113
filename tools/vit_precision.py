"""Where ViT-B + SETR-UP's bfloat16 labels part from its float32 ones: the setting of tests/test_gpu_vit.py (R = 256, batch 4,
randomize_neutral_parameters, pos_embed / cls_token N(0, 0.02), balance_classifier_bias, prepare_inference), with the label
agreement against float32 for
  bf16 kernels      the shipped bf16 path (ppn_mhsa_fwd, the build's GEMMs),
  bf16 framework    the backbone as the framework's bf16 ops (nn.MultiheadAttention, nn.Linear, LayerNorm: the grad-enabled
                    composition), then the same bf16 head,
  fp32 bb, bf16 hd  the float32 backbone's features rounded to bf16, then the bf16 head (the head's own share),
  bf16 bb, fp32 hd  the bf16 kernel backbone's features in float32, then the float32 head (the backbone's own share),
and the backbone features' relative deviation from float32 (max and rms over max|ref|).  Prints one line per variant; the output
is kept under profiles/."""
import copy
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from ppnet_amd import fused, segnet  # noqa: E402

dev = torch.device("cuda", 0)
R, B = 256, 4


def codes(seed):
    g = torch.Generator().manual_seed(seed)
    lo = (torch.rand(B, 1, R // 16, R // 16, generator=g) > 0.4).float()
    return (F.interpolate(lo, size=(R, R), mode="nearest")[:, 0] * 255).to(torch.uint8)


torch.manual_seed(0)
m32 = segnet.randomize_neutral_parameters(segnet.SegNet.from_config(segnet.VIT_BASE_SETRUP), seed=1)
g = torch.Generator().manual_seed(2)
with torch.no_grad():
    m32.backbone.pos_embed.copy_(torch.randn(m32.backbone.pos_embed.shape, generator=g) * 0.02)
    m32.backbone.cls_token.copy_(torch.randn(m32.backbone.cls_token.shape, generator=g) * 0.02)
m32 = m32.eval().to(dev)
c = codes(5).to(dev)
with torch.no_grad():
    segnet.balance_classifier_bias(m32, fused.grid_to_image(c, segnet.IMG_MEAN, segnet.IMG_STD, torch.float32))
m16 = copy.deepcopy(m32).to(torch.bfloat16)
m32.prepare_inference()
m16.prepare_inference()
for p in list(m32.parameters()) + list(m16.parameters()):
    p.requires_grad_(False)


def head_labels(m, feats):
    with torch.no_grad():
        return fused.seg_labels_2class(m.decode_head(feats, lowres=True), (R, R))


with torch.no_grad():
    f32 = m32.backbone(c)
    l32 = head_labels(m32, f32)
    f16 = m16.backbone(c)
    l16 = head_labels(m16, f16)
with torch.enable_grad():                                   # the backbone's framework composition (no parameter needs grad)
    f16t = m16.backbone(c)
lt = head_labels(m16, [t.detach() for t in f16t])
lh = head_labels(m16, [t.to(torch.bfloat16) for t in f32])
lb = head_labels(m32, [t.float() for t in f16])
ref = f32[-1].double()
print(f"class-1 fraction of the float32 labels: {l32.float().mean().item():.3f}", flush=True)
for name, lab, feat in (("bf16 kernels", l16, f16), ("bf16 framework", lt, f16t), ("fp32 bb, bf16 hd", lh, None),
                        ("bf16 bb, fp32 hd", lb, f16)):
    agree = (lab == l32).float().mean().item()
    dev_s = ""
    if feat is not None:
        d = feat[-1].detach().double() - ref
        dev_s = f"  backbone max dev {d.abs().max().item() / ref.abs().max().item():.2e}  rms dev {d.pow(2).mean().sqrt().item() / ref.abs().max().item():.2e}"
    print(f"{name:17s}: label agreement with float32 {agree:.5f}{dev_s}", flush=True)
