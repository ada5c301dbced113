"""ppn_resize_ce_fwd / ppn_resize_ce_bwd (csrc/resize_ce.hip) on the GPU: the heads' training loss — bilinear resize +
cross-entropy — without the resized logits.

Reference: float64 autograd on the CPU of the definition, F.interpolate(bilinear, align_corners=False) ->
F.cross_entropy(ignore_index, reduction='none').mean(), on the exact input values (for bfloat16 the rounded ones, widened).
Bound, per output (loss, dlogit): err = max|got - ref| / max|ref| <= max(2 x the error of the library chain — the same two torch
calls on the GPU in the same dtype on the same inputs in the same run —, floor), floor 2e-6 for float32 results (the loss is float32
in both dtypes) and 1e-2 for a bfloat16 dlogit.  `correct` equals the reference's count exactly: the logits are generated so that no
two classes come within 1e-3 of each other at any pixel (checked on the CPU in float64).  Every raw call runs on NaN-filled
workspace / lse / dlogit buffers with canaries around every output."""
import copy
import ctypes as C
import functools
import math

import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FWD_PX, THREADS = 1024, 256                      # pixels per forward workgroup; work-items per workgroup (csrc/resize_ce.hip)
FLOOR = {torch.float32: 2e-6, torch.bfloat16: 1e-2}
PAD = 64                                         # canary elements on either side of every output buffer
DTYPES = [torch.float32, torch.bfloat16]
IDS = {torch.float32: "f32", torch.bfloat16: "bf16"}

#          B  C   h   w   H    W
SHAPES = [(1, 2, 1, 1, 1, 1),
          (1, 2, 1, 1, 5, 3),                    # one source pixel, every tap clamped
          (2, 2, 3, 5, 6, 10),                   # x2
          (1, 2, 4, 4, 16, 16),                  # x4
          (1, 3, 2, 3, 32, 48),                  # x16, footprint about 880
          (1, 2, 5, 7, 13, 9), (1, 3, 3, 3, 10, 11),        # non-integer ratios
          (1, 4, 6, 4, 3, 4),                    # down-sampling and identity
          (2, 2, 4, 4, 4, 4),                    # identity
          (1, 19, 3, 2, 12, 8),
          (1, 1, 2, 2, 4, 4),                    # C = 1: loss and gradient exactly 0
          (1, 2, 1, 4, 7, 16),
          # B H W one below, at and one above the forward's pixels per workgroup
          (1, 2, 8, 8, 31, 33), (1, 2, 8, 8, 32, 32), (1, 2, 8, 8, 25, 41),
          # B C h w one below, at and one above the backward's outputs per workgroup: 256 (a lane per output, ratio <= 2) ...
          (1, 3, 5, 17, 10, 34), (1, 2, 8, 16, 16, 32), (1, 257, 1, 1, 2, 2),
          # ... 32 (8 lanes per output, x4) and 4 (a wave per output, x16)
          (1, 31, 1, 1, 4, 4), (1, 2, 4, 4, 16, 16), (1, 3, 1, 11, 4, 44),
          (1, 3, 1, 1, 16, 16), (1, 2, 1, 2, 16, 32), (1, 5, 1, 1, 16, 16),
          (2, 2, 64, 64, 128, 128)]              # the reduction: 32 forward workgroups
SHAPES = list(dict.fromkeys(SHAPES))


def test_shapes_sit_on_the_workgroup_boundaries():
    from ppnet_amd import fused
    assert fused.RESIZE_CE_FWD_PIXELS == FWD_PX and fused.RESIZE_CE_THREADS == THREADS
    px = {B * H * W for B, C, h, w, H, W in SHAPES}
    assert {FWD_PX - 1, FWD_PX, FWD_PX + 1} <= px
    for lanes in (1, 8, 64):
        per = THREADS // lanes
        outs = {B * C * h * w for B, C, h, w, H, W in SHAPES if fused.resize_ce_bwd_lanes(h, w, H, W) == lanes}
        assert {per - 1, per, per + 1} <= outs, (lanes, sorted(outs))


# ------------------------------------------------------------------------------------------------ inputs and references
def _resized64(x, H, W):
    return F.interpolate(x.double(), (H, W), mode="bilinear", align_corners=False)


def _min_gap(x, H, W):
    z = _resized64(x, H, W)
    if z.shape[1] == 1:
        return math.inf
    top = z.topk(2, dim=1).values
    return float((top[:, 0] - top[:, 1]).min())


@functools.lru_cache(maxsize=None)
def _logits(shape, dtype, peak=None):
    """CPU float32 logits (for bfloat16: already rounded) with no two classes within 1e-3 at any full-resolution pixel; peak: scaled
    so that the largest magnitude is `peak`.  Plain normal values (x 3) where a seed gives that; otherwise (many pixels, or
    bfloat16's coarse steps at a large peak) a random class order per image with gaps that no convex combination can close, plus
    noise."""
    B, Cc, h, w, H, W = shape

    def finish(x):
        if peak is not None:
            x = x * (peak / float(x.abs().max()))
        return x.to(dtype).float()
    for seed in range(40):
        g = torch.Generator().manual_seed(1000 * seed + 7)
        x = finish(torch.randn(B, Cc, h, w, generator=g) * 3.0)
        if _min_gap(x, H, W) > 1e-3:
            return x
    g = torch.Generator().manual_seed(5)
    order = torch.stack([torch.randperm(Cc, generator=g) for _ in range(B)]).float()
    x = finish((order.view(B, Cc, 1, 1) - (Cc - 1) / 2 + (torch.rand(B, Cc, h, w, generator=g) - 0.5) * 0.6) * 1.5)
    assert _min_gap(x, H, W) > 1e-3
    return x


@functools.lru_cache(maxsize=None)
def _labels(shape, mode, ignore=255):
    """CPU int64 labels [B,H,W]: 'mixed' about 20 % ignored, 'none', 'all'."""
    B, Cc, h, w, H, W = shape
    g = torch.Generator().manual_seed(B * 131 + Cc * 17 + H * 5 + W)
    lab = torch.randint(0, min(Cc, 255), (B, H, W), generator=g)              # (uint8 holds every one of them)
    if mode == "mixed":
        lab[torch.rand(B, H, W, generator=g) < 0.2] = ignore
    elif mode == "all":
        lab[:] = ignore
    return lab


def _reference(x, lab, ignore, grad=1.0):
    """float64 CPU: (loss, correct, dlogit) of the definition."""
    H, W = lab.shape[-2:]
    xd = x.detach().double().requires_grad_(True)
    z = F.interpolate(xd, (H, W), mode="bilinear", align_corners=False)
    loss = F.cross_entropy(z, lab, ignore_index=ignore, reduction="none").mean()
    (loss * grad).backward()
    return loss.detach(), int((z.argmax(1) == lab).sum()), xd.grad


def _library(x, lab, ignore, dtype, grad=1.0):
    """The same two torch calls on the GPU in `dtype`: (loss, dlogit) as float64 CPU tensors."""
    H, W = lab.shape[-2:]
    xg = x.detach().to(DEV, dtype).clone().requires_grad_(True)
    z = F.interpolate(xg, (H, W), mode="bilinear", align_corners=False)
    loss = F.cross_entropy(z, lab.to(DEV), ignore_index=ignore, reduction="none").mean()
    (loss * grad).backward()
    return loss.detach().double().cpu(), xg.grad.double().cpu()


def _guarded(n, dtype, fill):
    canary = 0x5A5A5A5A if dtype == torch.int64 else 1024.0                   # (exact in bfloat16 too)
    buf = torch.full((n + 2 * PAD,), canary, dtype=dtype, device=DEV)
    view = buf[PAD:PAD + n]
    view.fill_(fill)
    assert view.data_ptr() % 16 == 0

    def intact():
        return bool((buf[:PAD] == canary).all()) and bool((buf[PAD + n:] == canary).all())
    return view, intact


def _raw(x, lab, ignore=255, grad=1.0, label_dtype=torch.uint8, dtype=torch.float32, backward=True, lse=True):
    """ppn_resize_ce_fwd (+ _bwd) straight through ctypes on NaN-filled, canary-guarded buffers:
    (loss 0-d float32, correct int, lse [B,H,W] or None, dlogit or None), on the GPU."""
    from ppnet_amd import _lib
    B, Cc, h, w = x.shape
    H, W = lab.shape[-2:]
    xg, lg = x.to(DEV, dtype).contiguous(), lab.to(DEV, label_dtype).contiguous()
    need = _lib.lib.ppn_resize_ce_workspace(B, H, W)
    assert need == 2 * -(-(B * H * W) // FWD_PX)
    nan = float("nan")
    ws, ws_ok = _guarded(need, torch.float32, nan)
    loss, loss_ok = _guarded(1, torch.float32, nan)
    cor, cor_ok = _guarded(2, torch.int64, -7)                  # two, so that the view stays 16-byte aligned; the second is a canary too
    lse_b, lse_ok = _guarded(B * H * W, torch.float32, nan) if (lse or backward) else (None, lambda: True)
    dl, dl_ok = _guarded(x.numel(), dtype, nan)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    ld, bd = {torch.float32: 0, torch.bfloat16: 1}[dtype], {torch.uint8: 0, torch.int64: 1}[label_dtype]
    rc = _lib.lib.ppn_resize_ce_fwd(p(xg), p(lg), p(lse_b), p(loss), p(cor), p(ws), need, B, Cc, h, w, H, W, ignore, ld, bd, stream)
    assert rc == 0, rc
    if backward:
        g = torch.tensor(grad, dtype=torch.float32, device=DEV)
        rc = _lib.lib.ppn_resize_ce_bwd(p(xg), p(lg), p(lse_b), p(g), p(dl), B, Cc, h, w, H, W, ignore, ld, bd, stream)
        assert rc == 0, rc
    torch.cuda.synchronize()
    assert ws_ok() and loss_ok() and cor_ok() and lse_ok() and dl_ok(), "a canary was overwritten"
    assert int(cor[1]) == -7
    assert not backward or bool(torch.isfinite(dl.float()).all())
    return (loss[0].clone(), int(cor[0]), lse_b.clone().view(B, H, W) if lse_b is not None else None,
            dl.clone().view_as(xg) if backward else None)


def _check(x, lab, ignore, dtype, what, capsys, grad=1.0, label_dtypes=(torch.uint8, torch.int64)):
    """The rule for one (logits, labels): every label dtype against the float64 reference; the label dtypes bit-equal."""
    ref_loss, ref_correct, ref_d = _reference(x, lab, ignore, grad)
    lib_loss, lib_d = _library(x, lab, ignore, dtype, grad)
    got = [_raw(x, lab, ignore, grad, ld, dtype) for ld in label_dtypes]
    for other in got[1:]:
        assert torch.equal(got[0][0], other[0]) and got[0][1] == other[1] and torch.equal(got[0][2], other[2]) and torch.equal(got[0][3], other[3])
    loss, correct, _, d = got[0]
    assert d.dtype == dtype and loss.dtype == torch.float32
    assert correct == ref_correct, (what, correct, ref_correct)
    out = []
    for name, g, r, l, floor in (("loss", loss.double().cpu(), ref_loss, lib_loss, 2e-6), ("dlogit", d.double().cpu(), ref_d, lib_d, FLOOR[dtype])):
        m = float(r.abs().max())
        if m == 0.0:                                                        # C = 1, or every pixel ignored
            assert float(g.abs().max()) == 0.0, (what, name)
            out.append(f"{name} exactly 0")
            continue
        ek, el = float((g - r).abs().max()) / m, float((l - r).abs().max()) / m
        out.append(f"{name} kernel {ek:.2e} library {el:.2e}")
        assert ek <= max(2.0 * el, floor), (what, name, ek, el)
    with capsys.disabled():
        print(f"\nresize_ce {IDS[dtype]} {what}: " + ", ".join(out), end="")
    return got[0]


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_vs_float64(shape, dtype, capsys):
    """Every shape, both logit dtypes, uint8 and int64 labels, about 20 % / none / all of the pixels ignored."""
    x = _logits(shape, dtype)
    for mode in ("mixed", "none", "all"):
        lab = _labels(shape, mode)
        loss, correct, _, d = _check(x, lab, 255, dtype, f"{shape} {mode}", capsys)
        if mode == "all" or shape[1] == 1:
            assert float(loss) == 0.0 and bool((d == 0).all())
        if mode == "all":
            assert correct == 0


# ------------------------------------------------------------------------------------------------ labels
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_ignore_index_minus_100_and_out_of_range_labels(dtype, capsys):
    shape = (2, 2, 3, 5, 6, 10)
    x = _logits(shape, dtype)
    lab = _labels(shape, "mixed", ignore=-100)
    assert int((lab == -100).sum()) > 0
    _check(x, lab, -100, dtype, f"{shape} ignore_index -100", capsys, label_dtypes=(torch.int64,))
    # 255 is an ordinary out-of-range label now: ignored like -100
    lab255 = lab.clone()
    lab255[lab == -100] = 255
    a, b = _raw(x, lab255, -100, label_dtype=torch.int64, dtype=dtype), _raw(x, lab, -100, label_dtype=torch.int64, dtype=dtype)
    assert torch.equal(a[0], b[0]) and a[1] == b[1] and torch.equal(a[3], b[3])
    # out-of-range labels (7 at C = 2; negative ones with int64) give the bits of the same call with those pixels ignored
    g = torch.Generator().manual_seed(3)
    base = _labels(shape, "mixed")
    bad = torch.rand(base.shape, generator=g) < 0.25
    assert int(bad.sum()) > 0 and int((~bad & (base != 255)).sum()) > 0
    ignored = base.clone()
    ignored[bad] = 255
    for ld, values in ((torch.uint8, (7, 2, 254)), (torch.int64, (7, 2, -1, 1 << 40, -(1 << 40) + 1))):
        want = _raw(x, ignored, 255, label_dtype=ld, dtype=dtype)
        for v in values:
            oor = base.clone()
            oor[bad] = v
            got = _raw(x, oor, 255, label_dtype=ld, dtype=dtype)
            assert torch.equal(got[0], want[0]) and got[1] == want[1] and torch.equal(got[2], want[2]) and torch.equal(got[3], want[3]), (ld, v)


# ------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_logits_of_80(dtype, capsys):
    """Logits scaled to +-80: a wrong maximum overflows exp."""
    for shape in ((2, 2, 3, 5, 6, 10), (1, 19, 3, 2, 12, 8), (1, 3, 2, 3, 32, 48)):
        x = _logits(shape, dtype, 80.0)
        assert _min_gap(x, *shape[-2:]) > 1e-3 and 79.0 <= float(x.abs().max()) <= 80.5
        loss, _, lse, d = _check(x, _labels(shape, "mixed"), 255, dtype, f"{shape} +-80", capsys)
        assert bool(torch.isfinite(lse).all()) and bool(torch.isfinite(loss))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_one_class_50_above_the_rest(dtype, capsys):
    shape = (1, 4, 3, 3, 10, 11)
    B, Cc, h, w, H, W = shape
    g = torch.Generator().manual_seed(11)
    x = (torch.rand(B, Cc, h, w, generator=g) * 2 - 1)
    x[:, 2] += 50.0
    x = x.to(dtype).float()
    only = torch.full((B, H, W), 2, dtype=torch.int64)
    loss, correct, _, d = _raw(x, only, dtype=dtype)
    assert abs(float(loss)) <= 1e-6 and correct == B * H * W
    assert float(d.float().abs().max()) <= 1e-6
    _check(x, _labels(shape, "mixed"), 255, dtype, f"{shape} class 2 at +50", capsys)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_equal_logits_across_classes(dtype, capsys):
    """Every class the same value at every source pixel: loss = log C, ties go to class 0, gradient = the gathered 1/C - onehot."""
    for shape in ((1, 3, 3, 3, 10, 11), (1, 19, 3, 2, 12, 8), (1, 2, 4, 4, 16, 16)):
        B, Cc, h, w, H, W = shape
        g = torch.Generator().manual_seed(13)
        x = (torch.randn(B, 1, h, w, generator=g).expand(B, Cc, h, w).contiguous() * 3).to(dtype).float()
        lab = _labels(shape, "mixed")
        ref_loss, _, ref_d = _reference(x, lab, 255)
        lib_loss, lib_d = _library(x, lab, 255, dtype)
        loss, correct, _, d = _raw(x, lab, dtype=dtype)
        assert correct == int((lab == 0).sum())
        valid = float((lab != 255).double().mean())
        m = float(ref_loss)
        assert m == pytest.approx(math.log(Cc) * valid, rel=1e-12)
        ek, el = abs(float(loss) - m) / m, abs(float(lib_loss) - m) / m
        assert ek <= max(2 * el, 2e-6), (shape, ek, el)
        md = float(ref_d.abs().max())
        dk, dl = float((d.double().cpu() - ref_d).abs().max()) / md, float((lib_d - ref_d).abs().max()) / md
        with capsys.disabled():
            print(f"\nresize_ce {IDS[dtype]} {shape} equal logits: loss kernel {ek:.2e} library {el:.2e}, dlogit kernel {dk:.2e} library {dl:.2e}", end="")
        assert dk <= max(2 * dl, FLOOR[dtype]), (shape, dk, dl)


# ------------------------------------------------------------------------------------------------ mechanics
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_upstream_gradient_and_repeatability(dtype, capsys):
    shape = (1, 3, 2, 3, 32, 48)
    x, lab = _logits(shape, dtype), _labels(shape, "mixed")
    _check(x, lab, 255, dtype, f"{shape} grad_out 0.4", capsys, grad=0.4)
    zero = _raw(x, lab, grad=0.0, dtype=dtype)
    assert bool((zero[3] == 0).all())
    for shape in ((2, 2, 64, 64, 128, 128), (1, 3, 2, 3, 32, 48), (1, 2, 5, 7, 13, 9)):
        x, lab = _logits(shape, dtype), _labels(shape, "mixed")
        a, b, c = (_raw(x, lab, dtype=dtype) for _ in range(3))
        for u in (b, c):
            assert torch.equal(a[0], u[0]) and a[1] == u[1] and torch.equal(a[2], u[2]) and torch.equal(a[3], u[3])
    # lse = NULL: the same loss and count, nothing else written (the canaries in _raw)
    d = _raw(x, lab, dtype=dtype, backward=False, lse=False)
    assert torch.equal(a[0], d[0]) and a[1] == d[1] and d[2] is None


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("label_dtype", [torch.uint8, torch.int64], ids=["u8", "i64"])
def test_autograd_function_returns_the_raw_bits(dtype, label_dtype, monkeypatch):
    from ppnet_amd import fused
    shape = (2, 2, 64, 64, 128, 128)
    x, lab = _logits(shape, dtype), _labels(shape, "mixed")
    raw = _raw(x, lab, grad=0.4, label_dtype=label_dtype, dtype=dtype)
    xg, lg = x.to(DEV, dtype).requires_grad_(True), lab.to(DEV, label_dtype)
    calls = dict(fused.LOSS_CALLS)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append((tuple(t.shape), t.dtype)), t)[1], lambda t: t):
        loss, correct = fused.resize_cross_entropy(xg, lg)
    assert sorted(saved, key=str) == sorted([((2, 2, 64, 64), dtype), ((2, 128, 128), label_dtype), ((2, 128, 128), torch.float32)], key=str)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.requires_grad
    assert correct.shape == () and correct.dtype == torch.int64 and not correct.requires_grad
    (loss * 0.4).backward()
    assert torch.equal(loss.detach(), raw[0]) and int(correct) == raw[1]
    assert xg.grad.dtype == dtype and torch.equal(xg.grad, raw[3])
    assert fused.LOSS_CALLS == {"fwd": calls["fwd"] + 1, "bwd": calls["bwd"] + 1}
    # no_grad, or nothing that requires grad: no lse, no backward, the same loss
    seen = []
    inner = fused._resize_ce_fwd
    monkeypatch.setattr(fused, "_resize_ce_fwd", lambda *a: (seen.append(a[3]), inner(*a))[1])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()
    with torch.no_grad():
        l2, c2 = fused.resize_cross_entropy(xg, lg)
    l3, c3 = fused.resize_cross_entropy(xg.detach(), lg)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - held
    assert seen == [False, False] and rise < 2 * 128 * 128 * 4, (seen, rise)          # less than one lse buffer
    assert not l2.requires_grad and not l3.requires_grad
    assert torch.equal(l2, raw[0]) and torch.equal(l3, raw[0]) and int(c2) == int(c3) == raw[1]
    assert fused.LOSS_CALLS == {"fwd": calls["fwd"] + 3, "bwd": calls["bwd"] + 1}
    # heads.resized_decode_losses: the weight, the percentage, and the knob
    from ppnet_amd.heads import decode_losses, resized_decode_losses
    lw, acc = resized_decode_losses(xg.detach(), lg, 0.4)
    assert torch.equal(lw, 0.4 * raw[0]) and float(acc) == pytest.approx(raw[1] * 100.0 / lab.numel(), rel=1e-6)
    monkeypatch.setenv("PPNET_LIBRARY_LOSS", "1")
    lk, acck = resized_decode_losses(xg.detach(), lg, 0.4)
    want = decode_losses(F.interpolate(xg.detach().float(), (128, 128), mode="bilinear", align_corners=False), lg.long(), 0.4)
    assert torch.equal(lk, want[0]) and torch.equal(acck, want[1]) and torch.equal(acck, acc)
    assert fused.LOSS_CALLS["fwd"] == calls["fwd"] + 4
    monkeypatch.delenv("PPNET_LIBRARY_LOSS")
    # align_corners=True is the library's
    resized_decode_losses(xg.detach(), lg, 1.0, align_corners=True)
    assert fused.LOSS_CALLS["fwd"] == calls["fwd"] + 4


# ------------------------------------------------------------------------------------------------ model
# tests/test_gpu_train.py's tiny DiNAT + SETR-UP + FCN auxiliary head, with stochastic depth and dropout at 0 so that the CPU copy
# and the two GPU paths see the same network
TINY_SEG = dict(
    backbone=dict(embed_dim=32, mlp_ratio=2.0, depths=[1, 1, 2, 1], num_heads=[1, 2, 4, 8], kernel_size=7, layer_scale=1e-1,
                  dilations=[[1], [2], [1, 2], [1]], drop_path_rate=0.0),
    decode_head=dict(in_channels=256, channels=32, num_convs=4, up_scale=2, num_classes=2, kernel_size=3, dropout_ratio=0.0))
TINY_AUX = dict(type="FCNHead", in_channels=128, in_index=2, channels=32, num_convs=1, concat_input=False, dropout_ratio=0.0,
                num_classes=2, align_corners=False, loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=0.4))


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
    (losses["decode.loss_ce"] + losses["aux.loss_ce"]).backward()
    grads = {n: p.grad.detach().double().cpu() for n, p in net.named_parameters() if p.grad is not None}
    return {k: v.detach().double().cpu() for k, v in losses.items()}, grads


@pytest.fixture(scope="module")
def tiny_model():
    """(the float32 network on the CPU, image, uint8 labels, the float64 CPU losses and gradients)."""
    from oracle import segnet_ref as SR
    from ppnet_amd import na
    from ppnet_amd.segnet import SegNet, randomize_neutral_parameters
    torch.manual_seed(2)
    net = randomize_neutral_parameters(SegNet(**TINY_SEG, auxiliary_head=TINY_AUX), seed=3).train()
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
def test_tiny_dinat_training_step_through_the_loss_kernels(tiny_model, autocast, monkeypatch, capsys):
    from ppnet_amd import fused
    cpu_net, img, gt, (ref_losses, ref_grads) = tiny_model
    net = copy.deepcopy(cpu_net).to(DEV)
    imgd, gtd = img.to(DEV), gt.to(DEV)
    calls = dict(fused.LOSS_CALLS)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(tuple(t.shape)), t)[1], lambda t: t):
        losses, grads = _model_run(net, imgd, gtd, autocast)
    assert fused.LOSS_CALLS == {"fwd": calls["fwd"] + 2, "bwd": calls["bwd"] + 2}
    assert (2, 2, 64, 64) not in saved and saved.count((2, 64, 64)) >= 4, saved         # labels and lse per head; no resized logits
    monkeypatch.setenv("PPNET_LIBRARY_LOSS", "1")
    lib_losses, lib_grads = _model_run(net, imgd, gtd, autocast)
    monkeypatch.delenv("PPNET_LIBRARY_LOSS")
    assert fused.LOSS_CALLS == {"fwd": calls["fwd"] + 2, "bwd": calls["bwd"] + 2}
    assert list(losses) == list(lib_losses) == ["decode.loss_ce", "decode.acc_seg", "aux.loss_ce", "aux.acc_seg"]
    for k in ("decode", "aux"):
        assert float(losses[f"{k}.loss_ce"]) == pytest.approx(float(lib_losses[f"{k}.loss_ce"]), rel=1e-5)
        assert float(losses[f"{k}.acc_seg"]) == float(lib_losses[f"{k}.acc_seg"])
        if not autocast:
            assert float(losses[f"{k}.loss_ce"]) == pytest.approx(float(ref_losses[f"{k}.loss_ce"]), rel=1e-4)
    assert set(grads) == set(lib_grads) == set(ref_grads)
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
        print(f"\ntiny DiNAT + SETR-UP + aux, {'bf16 autocast' if autocast else 'float32'}: worst parameter {worst[2]} kernel path "
              f"{worst[0]:.2e} x its max, library path {worst[1]:.2e}; losses {float(losses['decode.loss_ce']):.6f} / "
              f"{float(losses['aux.loss_ce']):.6f} (library {float(lib_losses['decode.loss_ce']):.6f} / {float(lib_losses['aux.loss_ce']):.6f})", end="")
