"""DiNAT_s on the device: the backbone against the reference's own outputs (tests/golden/g23_dinats.npz `net`), a prepared SegNet in
bfloat16 against its float32 leg, and one training step against the float64 CPU definition — each time next to the same network with
PPNET_LIBRARY_MERGE=1 (the torch composition of the patch merge) in the same test:

  outputs    max|kernel path - ref| <= 2 * max|library path - ref| + eps(dtype) * max|ref|     (one ulp at the output's magnitude)
  gradients  test_gpu_dice.py's model rule, per parameter with m = max|ref|:  dk / m <= max(2 * dl / m, floor), floor 2e-6 in float32 and
             1e-2 under bfloat16 autocast

fused.MERGE_CALLS counts the launches of ppn_patch_merge_ln_fwd / ppn_patch_merge_ln_bwd: three merges each way, none with the knob.

Measured on the device, kernel merge | library merge: backbone float32 levels 3.4e-7 | 3.4e-7, 4.9e-7 | 5.8e-7, 4.7e-7 | 5.4e-7, 9.7e-7 |
9.7e-7 of the level's magnitude, bfloat16 1.01e-2 | 1.01e-2, 1.27e-2 | 1.27e-2, 1.12e-2 | 9.1e-3, 1.31e-2 | 1.31e-2; prepared bfloat16 logits
9.91e-3 | 9.91e-3; training step float32 worst parameter 4.3e-6 | 2.9e-6 (see the note above TRAIN_BB), autocast 2.1e-1 | 2.1e-1."""
import copy
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

from tests._oracle_util import wiring_weights  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
IDS = {torch.float32: "f32", torch.bfloat16: "bf16"}


@pytest.fixture(scope="module")
def g23(golden_dir):
    return np.load(os.path.join(golden_dir, "g23_dinats.npz"))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=IDS.get)
def test_backbone_vs_reference_outputs(g23, dtype, monkeypatch, capsys):
    """Every merge pads (13 x 17 -> 7 x 9 -> 4 x 5 -> 2 x 3) and every dilated layer is smaller than its window."""
    from ppnet_amd import fused
    from ppnet_amd.segnet import DiNAT_s
    monkeypatch.delenv("PPNET_LIBRARY_MERGE", raising=False)
    cfg = json.loads(str(g23["net/cfg"]))
    keys = [str(k) for k in g23["net/keys"]]
    w = wiring_weights(keys, [tuple(json.loads(str(s))) for s in g23["net/shapes"]], int(g23["net/seed"][0]))
    m = DiNAT_s(**cfg)
    m.load_state_dict({k: torch.from_numpy(v).float() for k, v in w.items()}, strict=True)
    m = m.eval().to(DEV, dtype)
    x = torch.from_numpy(g23["net/x"]).to(DEV, dtype)
    calls = dict(fused.MERGE_CALLS)
    with torch.no_grad():
        outs = m(x)
        assert fused.MERGE_CALLS == {"fwd": calls["fwd"] + 3, "bwd": calls["bwd"]}
        monkeypatch.setenv("PPNET_LIBRARY_MERGE", "1")
        lib = m(x)
        monkeypatch.delenv("PPNET_LIBRARY_MERGE")
    assert fused.MERGE_CALLS == {"fwd": calls["fwd"] + 3, "bwd": calls["bwd"]}
    assert len(outs) == len(lib) == 4
    eps, line = torch.finfo(dtype).eps, []
    for i, (o, l) in enumerate(zip(outs, lib)):
        want = g23[f"net/y{i}"]
        got, gl = o.float().cpu().double().numpy(), l.float().cpu().double().numpy()
        assert got.shape == want.shape == gl.shape
        mx, ek, el = np.abs(want).max(), np.abs(got - want).max(), np.abs(gl - want).max()
        line.append(f"level {i} {ek / mx:.2e} / {el / mx:.2e}")
        with capsys.disabled():
            if i == 3:
                print(f"\nDiNAT_s {IDS[dtype]} vs g23, kernel / library merge error over max|ref|: " + ", ".join(line), end="")
        assert ek <= 2.0 * el + eps * mx, (i, ek, el, mx)
        if dtype == torch.float32:
            assert ek < 2e-3 * max(1.0, mx), (i, ek)                         # test_segnet_wiring_golden.py's bound for the float32 backbone


TINY_BB = dict(type="DiNAT_s", embed_dim=32, depths=[2, 1, 2, 1], num_heads=[1, 2, 4, 8], mlp_ratio=2.0, dilations=[[1, 2], [1], [1, 2], [1]],
               drop_path_rate=0.0)
TINY_HEAD = dict(in_channels=256, channels=32, num_convs=4, up_scale=2, num_classes=2, kernel_size=3, dropout_ratio=0.0)
TINY_AUX = dict(type="FCNHead", in_channels=128, in_index=2, channels=32, num_convs=1, concat_input=False, dropout_ratio=0.0, num_classes=2,
                align_corners=False)


def test_prepared_inference_bf16_against_its_float32_leg(monkeypatch, capsys):
    """72 x 56 input: an 18 x 14 grid that becomes 9 x 7, 5 x 4 and 3 x 2 — two of the three merges pad."""
    from ppnet_amd import fused
    from ppnet_amd.segnet import SegNet, randomize_neutral_parameters
    monkeypatch.delenv("PPNET_LIBRARY_MERGE", raising=False)
    torch.manual_seed(5)
    base = randomize_neutral_parameters(SegNet(backbone=TINY_BB, decode_head=TINY_HEAD, auxiliary_head=TINY_AUX), seed=6).eval()
    img = torch.randn(2, 3, 72, 56, generator=torch.Generator().manual_seed(7)).to(DEV)
    leg32 = copy.deepcopy(base).to(DEV).prepare_inference()
    net = copy.deepcopy(base).to(DEV, torch.bfloat16).prepare_inference()
    assert net.backbone.compute_indices == (3,) and all(blk.folded for layer in net.backbone.layers for blk in layer.blocks)
    with torch.no_grad():
        ref = leg32(img, return_logits=True)[1].double()
        calls = dict(fused.MERGE_CALLS)
        pred, logits = net(img.to(torch.bfloat16), return_logits=True)
        assert fused.MERGE_CALLS == {"fwd": calls["fwd"] + 3, "bwd": calls["bwd"]}
        labels = net.labels_u8(img.to(torch.bfloat16))
        simple = net.simple_test(img.to(torch.bfloat16), [dict(ori_shape=(72, 56, 3), flip=False)])
        monkeypatch.setenv("PPNET_LIBRARY_MERGE", "1")
        lib = net(img.to(torch.bfloat16), return_logits=True)[1]
        monkeypatch.delenv("PPNET_LIBRARY_MERGE")
    assert fused.MERGE_CALLS == {"fwd": calls["fwd"] + 9, "bwd": calls["bwd"]}              # three forwards of three merges; none with the knob
    assert logits.shape == ref.shape == (2, 2, 72, 56) and labels.dtype == torch.uint8 and labels.shape == (2, 72, 56)
    assert len(simple) == 2 and all(np.array_equal(s, l) for s, l in zip(simple, labels.cpu().numpy().astype(np.int64)))
    m = float(ref.abs().max())
    ek, el = float((logits.double() - ref).abs().max()), float((lib.double() - ref).abs().max())
    with capsys.disabled():
        print(f"\nprepared tiny DiNAT_s + SETR-UP bf16 vs float32 logits: kernel merge {ek / m:.2e}, library merge {el / m:.2e} of max|ref|", end="")
    assert ek <= 2.0 * el + torch.finfo(torch.bfloat16).eps * m, (ek, el, m)


# ------------------------------------------------------------------------------------------------ one training step
# The smallest network with all three merges: one layer per level (one of them dilated: smaller than its window), two head stages of 16
# channels.  Everything in front of and behind the merges is the same code in both legs, and its float32 rounding is noise in the
# comparison below — per parameter 1-3e-6 of the gradient's magnitude in EITHER leg, around the rule's floor, and a step is not
# bit-reproducible from run to run (library convolutions and GEMMs).  Measured on the device, worst parameter's dk / max(2 dl, floor) over
# 5 seeds x 3 repeats: this network 0.62-1.03 (one of 15 above 1); with depths 2-1-2-1 and four head stages of 32 channels 0.73-1.19 (6 of
# 15 above 1) — the kind of miss DESIGN.md section 22 records for the float32 model tests of sections 16 and 20.
TRAIN_BB = dict(TINY_BB, depths=[1, 1, 1, 1], dilations=[[1], [2], [1], [1]])
TRAIN_HEAD = dict(TINY_HEAD, num_convs=2, channels=16)


def _definition(net, img, gt):
    """forward_train's loss dict from the definition in the network's own dtype (no float32 stage: the float64 reference)."""
    feats = net.backbone(img)
    losses = {}
    for name, head, w in (("decode", net.decode_head, 1.0), ("aux", net.auxiliary_head, net.auxiliary_head.loss_weight)):
        z = F.interpolate(head(feats), gt.shape[-2:], mode="bilinear", align_corners=False)
        losses[f"{name}.loss_ce"] = w * F.cross_entropy(z, gt.long(), ignore_index=255, reduction="none").mean()
        losses[f"{name}.acc_seg"] = (z.argmax(1) == gt).double().sum() * (100.0 / gt.numel())
    return losses


def _model_run(net, img, gt, autocast=False, forward=None):
    net.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        losses = net.forward_train(img, None, gt) if forward is None else forward(net, img, gt)
    sum(v for k, v in losses.items() if "loss" in k).backward()
    grads = {n: p.grad.detach().double().cpu() for n, p in net.named_parameters() if p.grad is not None}
    return {k: v.detach().double().cpu() for k, v in losses.items()}, grads


@pytest.fixture(scope="module")
def tiny_model():
    """(the float32 network on the CPU, image, uint8 labels, the float64 CPU losses and gradients)."""
    from oracle import segnet_ref as SR
    from ppnet_amd import na
    from ppnet_amd.segnet import SegNet, randomize_neutral_parameters
    torch.manual_seed(2)
    net = randomize_neutral_parameters(SegNet(backbone=TRAIN_BB, decode_head=TRAIN_HEAD, auxiliary_head=TINY_AUX), seed=3).train()
    g = torch.Generator().manual_seed(4)
    img = torch.randn(2, 3, 64, 64, generator=g)
    gt = torch.randint(0, 2, (2, 64, 64), generator=g).to(torch.uint8)
    gt[torch.rand(2, 64, 64, generator=g) < 0.1] = 255
    own = na.NeighborhoodAttention2D.forward

    def forward(self, x, real_hw=None):                          # the float64 definition where the kernel cannot run
        if x.is_cuda:
            return own(self, x, real_hw)
        return SR.na_fp64(x, self.qkv.weight, self.qkv.bias, self.rpb, self.proj.weight, self.proj.bias, self.num_heads, 7, self.dilation)
    na.NeighborhoodAttention2D.forward = forward
    try:
        ref = _model_run(copy.deepcopy(net).double(), img.double(), gt, forward=_definition)
    finally:
        na.NeighborhoodAttention2D.forward = own
    return net, img, gt, ref


@pytest.mark.parametrize("autocast", [False, True], ids=["f32", "bf16_autocast"])
def test_tiny_dinats_training_step(tiny_model, autocast, monkeypatch, capsys):
    from ppnet_amd import fused
    monkeypatch.delenv("PPNET_LIBRARY_MERGE", raising=False)
    cpu_net, img, gt, (ref_losses, ref_grads) = tiny_model
    net = copy.deepcopy(cpu_net).to(DEV)
    imgd, gtd = img.to(DEV), gt.to(DEV)
    calls = dict(fused.MERGE_CALLS)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(tuple(t.shape)), t)[1], lambda t: t):
        losses, grads = _model_run(net, imgd, gtd, autocast)
    assert fused.MERGE_CALLS == {"fwd": calls["fwd"] + 3, "bwd": calls["bwd"] + 3}
    for rows in (2 * 8 * 8, 2 * 4 * 4, 2 * 2 * 2):
        assert (rows, 2) in saved, (rows, saved)                              # the merges' row statistics
    monkeypatch.setenv("PPNET_LIBRARY_MERGE", "1")
    lib_losses, lib_grads = _model_run(net, imgd, gtd, autocast)
    monkeypatch.delenv("PPNET_LIBRARY_MERGE")
    assert fused.MERGE_CALLS == {"fwd": calls["fwd"] + 3, "bwd": calls["bwd"] + 3}          # with the knob nothing is launched
    assert list(losses) == list(lib_losses) == ["decode.loss_ce", "decode.acc_seg", "aux.loss_ce", "aux.acc_seg"]
    for k in ("decode", "aux"):
        assert float(losses[f"{k}.loss_ce"]) == pytest.approx(float(lib_losses[f"{k}.loss_ce"]), rel=1e-5)
        if not autocast:
            assert float(losses[f"{k}.loss_ce"]) == pytest.approx(float(ref_losses[f"{k}.loss_ce"]), rel=1e-4)
    names = {n for n, p in net.named_parameters() if p.requires_grad}
    unread = {f"backbone.norm{i}.{s}" for i in (0, 1) for s in ("weight", "bias")}          # output norms of levels no head reads
    assert set(grads) == set(lib_grads) == set(ref_grads) == names - unread               # every parameter gets a gradient
    for i in range(3):
        for s in ("norm.weight", "norm.bias", "reduction.weight"):
            assert f"backbone.layers.{i}.downsample.{s}" in grads
    floor = 1e-2 if autocast else 2e-6
    largest = max(float(r.abs().max()) for r in ref_grads.values())
    worst = (0.0, 0.0, "")
    for n in sorted(ref_grads):
        r = ref_grads[n]
        m = float(r.abs().max())
        dk, dl = float((grads[n] - r).abs().max()), float((lib_grads[n] - r).abs().max())
        if m < 1e-12 * largest:                # a gradient that is 0 in exact arithmetic: bounded against the largest one instead
            assert dk <= max(2.0 * dl, floor * largest), (n, dk, dl)
            continue
        worst = max(worst, (dk / m, dl / m, n))
        assert dk / m <= max(2.0 * dl / m, floor), (n, dk / m, dl / m)
    with capsys.disabled():
        print(f"\ntiny DiNAT_s + SETR-UP + aux, {'bf16 autocast' if autocast else 'float32'}: worst parameter {worst[2]} kernel path "
              f"{worst[0]:.2e} x its max, library path {worst[1]:.2e}; loss {float(losses['decode.loss_ce']):.6f} "
              f"(library {float(lib_losses['decode.loss_ce']):.6f}, float64 {float(ref_losses['decode.loss_ce']):.6f})", end="")
