"""ppn_resize_dice_fwd / ppn_resize_dice_bwd (csrc/resize_dice.hip) on the GPU: mmseg's DiceLoss of a head's logits — bilinear resize
+ softmax + per-class overlap sums — without the resized logits.

Reference: float64 autograd on the CPU of the definition, F.interpolate(bilinear, align_corners=False) -> heads.dice_loss (pinned to
the reference's own dice_loss.py by tests/test_dice_golden.py), on the exact input values (for bfloat16 the rounded ones, widened).
Bound, per output (loss, dlogit): err = max|got - ref| / max|ref| <= max(2 x the error of the library chain — the same torch
composition on the GPU in the same dtype on the same inputs in the same run —, floor), floor 2e-6 for float32 results (the loss is
float32 in both dtypes) and 1e-2 for a bfloat16 dlogit.  The counts sums[..., 2] are exact; `correct` equals ppn_resize_ce_fwd's on
the same inputs (the logits are generated so that no two classes come within 1e-3 of each other at any pixel, checked on the CPU in
float64).  I and P2 (sums[..., 0:2]) against the largest reference sum: 2e-6 + 5e-7 max|logit| — z and lse each carry a few float32
roundings of their magnitude (4 x 6e-8 |z| in z - lse, which is the relative error of p = exp(z - lse)), expf one or two more, and a
tile's float32 sum of at most 1024 terms in [0, 1] about 1e-6; the tiles are then summed in double.  Every raw call runs on NaN-filled
workspace / lse / sums / dlogit buffers with canaries around every output.

Figures on the device while the kernels were written (float32, dlogit, kernel / library): per-pixel combination in float32,
(1,2,1,1,1,1) 5.14e-6 / 5.4e-7; the backward's per-pixel term as a plain sum, (1,256,2,2,4,4) mixed 3.30e-6 / 3.6e-7 and
(2,2,3,5,6,10) at +-80 3.07e-6 / 4.1e-7; the forward's p from the rounded lse, (1,19,3,2,12,8) at +-80 2.95e-6 / 1.24e-6 (bound
2.47e-6).  Each was a property of the arithmetic and is fixed in csrc/resize_dice.hip (its header comment says how).  As the file stands: 6.9e-7,
6.9e-7 / 5.9e-7 and 1.28e-6 on those cases."""
import copy
import ctypes as C

import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

from tests.test_gpu_resize_ce import SHAPES as CE_SHAPES, _labels, _logits, _min_gap, _raw as _ce_raw  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
PX, THREADS, MAX_C = 1024, 256, 256              # pixels per tile; work-items per workgroup; largest C (csrc/resize_dice.hip)
FLOOR = {torch.float32: 2e-6, torch.bfloat16: 1e-2}
PAD = 64                                         # canary elements on either side of every output buffer
DTYPES = [torch.float32, torch.bfloat16]
IDS = {torch.float32: "f32", torch.bfloat16: "bf16"}

#          B  C   h   w   H    W
SHAPES = [s for s in CE_SHAPES if s[1] <= MAX_C] + [
    (1, 1, 1, 257, 2, 514), (1, 2, 1, 129, 2, 258),        # one above the backward's 256 outputs per workgroup (a lane per output)
    (3, 2, 5, 7, 33, 37),                        # H W = 1221: two tiles per image, the second partial; a flat tile would straddle images
    (1, MAX_C, 2, 2, 4, 4)]                      # C = DICE_MAX_C
SHAPES = list(dict.fromkeys(SHAPES))


def test_shapes_sit_on_the_workgroup_boundaries():
    from ppnet_amd import fused
    assert (fused.RESIZE_DICE_PIXELS, fused.RESIZE_DICE_THREADS, fused.RESIZE_DICE_MAX_CLASSES) == (PX, THREADS, MAX_C)
    assert all(s in SHAPES for s in CE_SHAPES if s[1] <= MAX_C) and all(s[1] <= MAX_C for s in SHAPES)
    px = {B * H * W for B, C_, h, w, H, W in SHAPES}
    assert {PX - 1, PX, PX + 1} <= px
    for lanes in (1, 8, 64):
        per = THREADS // lanes
        outs = {B * C_ * h * w for B, C_, h, w, H, W in SHAPES if fused.resize_ce_bwd_lanes(h, w, H, W) == lanes}
        assert {per - 1, per, per + 1} <= outs, (lanes, sorted(outs))
    assert any(B >= 3 and (H * W) % PX != 0 and H * W > PX for B, C_, h, w, H, W in SHAPES)            # a flat tile would straddle images
    assert any(C_ == MAX_C for B, C_, h, w, H, W in SHAPES) and any(C_ == 1 for B, C_, h, w, H, W in SHAPES)
    assert (2, 2, 64, 64, 128, 128) in SHAPES and any((h, w) == (H, W) for B, C_, h, w, H, W in SHAPES)
    assert {fused.resize_ce_bwd_lanes(h, w, H, W) for B, C_, h, w, H, W in SHAPES} == {1, 8, 64}


# ------------------------------------------------------------------------------------------------ references
def _rule_sums(z, lab, ignore):
    """float64 [B,C,3] of the definition: I, P2, T from resized logits z and int64 labels."""
    Cc = z.shape[1]
    p = F.softmax(z, 1).flatten(2)
    onehot = F.one_hot(lab.clamp(0, Cc - 1), Cc).permute(0, 3, 1, 2).flatten(2).double()
    valid = ((lab != ignore) & (lab >= 0) & (lab < Cc)).flatten(1).unsqueeze(1).double()
    return torch.stack([(p * onehot * valid).sum(2), (p * p).sum(2), onehot.sum(2)], dim=2)


def _reference(x, lab, ignore=255, smooth=1.0, cw=None, grad=1.0):
    """float64 CPU: (loss, dlogit, sums [B,C,3]) of the definition."""
    from ppnet_amd import heads
    H, W = lab.shape[-2:]
    xd = x.detach().double().requires_grad_(True)
    z = F.interpolate(xd, (H, W), mode="bilinear", align_corners=False)
    loss = heads.dice_loss(z, lab, smooth, 2, cw, 1.0, ignore)
    (loss * grad).backward()
    return loss.detach(), xd.grad, _rule_sums(z.detach(), lab.long(), ignore)


def _library(x, lab, dtype, ignore=255, smooth=1.0, cw=None, grad=1.0):
    """The same torch composition on the GPU in `dtype`: (loss, dlogit) as float64 CPU tensors."""
    from ppnet_amd import heads
    H, W = lab.shape[-2:]
    xg = x.detach().to(DEV, dtype).clone().requires_grad_(True)
    z = F.interpolate(xg, (H, W), mode="bilinear", align_corners=False)
    loss = heads.dice_loss(z, lab.to(DEV), smooth, 2, cw, 1.0, ignore)
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


def _raw(x, lab, ignore=255, smooth=1.0, cw=None, grad=1.0, label_dtype=torch.uint8, dtype=torch.float32, backward=True, lse=True):
    """ppn_resize_dice_fwd (+ _bwd) straight through ctypes on NaN-filled, canary-guarded buffers: (loss 0-d float32, correct int,
    sums [B,C,3] float64, lse [B,H,W] or None, dlogit or None), on the GPU."""
    from ppnet_amd import _lib, fused
    B, Cc, h, w = x.shape
    H, W = lab.shape[-2:]
    xg, lg = x.to(DEV, dtype).contiguous(), lab.to(DEV, label_dtype).contiguous()
    cwg = None if cw is None else torch.tensor(cw, dtype=torch.float32, device=DEV)
    need = _lib.lib.ppn_resize_dice_workspace(B, Cc, H, W)
    assert need == fused.resize_dice_workspace_bytes(B, Cc, H, W) and need % 4 == 0
    nan = float("nan")
    ws, ws_ok = _guarded(need // 4, torch.float32, nan)
    loss, loss_ok = _guarded(1, torch.float32, nan)
    cor, cor_ok = _guarded(2, torch.int64, -7)                  # two, so that the view stays 16-byte aligned; the second is a canary too
    sums, sums_ok = _guarded(B * Cc * 3, torch.float64, nan)
    lse_b, lse_ok = _guarded(B * H * W, torch.float32, nan) if (lse or backward) else (None, lambda: True)
    dl, dl_ok = _guarded(x.numel(), dtype, nan)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    ld, bd = {torch.float32: 0, torch.bfloat16: 1}[dtype], {torch.uint8: 0, torch.int64: 1}[label_dtype]
    rc = _lib.lib.ppn_resize_dice_fwd(p(xg), p(lg), p(cwg), p(ws), p(lse_b), p(sums), p(loss), p(cor), B, Cc, h, w, H, W, ignore, smooth, ld, bd,
                                      stream)
    assert rc == 0, rc
    if backward:
        ws.fill_(nan)                                           # the backward needs nothing of what the forward left there
        g = torch.tensor(grad, dtype=torch.float32, device=DEV)
        rc = _lib.lib.ppn_resize_dice_bwd(p(xg), p(lg), p(lse_b), p(sums), p(cwg), p(g), p(ws), p(dl), B, Cc, h, w, H, W, ignore, smooth, ld, bd,
                                          stream)
        assert rc == 0, rc
    torch.cuda.synchronize()
    assert ws_ok() and loss_ok() and cor_ok() and sums_ok() and lse_ok() and dl_ok(), "a canary was overwritten"
    assert int(cor[1]) == -7 and bool(torch.isfinite(sums).all())
    assert not backward or bool(torch.isfinite(dl.float()).all())
    return (loss[0].clone(), int(cor[0]), sums.clone().view(B, Cc, 3), lse_b.clone().view(B, H, W) if lse_b is not None else None,
            dl.clone().view_as(xg) if backward else None)


def _same(a, b):
    return (torch.equal(a[0], b[0]) and a[1] == b[1] and torch.equal(a[2], b[2]) and (a[3] is None or b[3] is None or torch.equal(a[3], b[3]))
            and (a[4] is None or b[4] is None or torch.equal(a[4], b[4])))


def _check(x, lab, dtype, what, capsys, ignore=255, smooth=1.0, cw=None, grad=1.0, label_dtypes=(torch.uint8, torch.int64)):
    """The rule for one (logits, labels): every label dtype against the float64 reference; the label dtypes bit-equal."""
    ref_loss, ref_d, ref_sums = _reference(x, lab, ignore, smooth, cw, grad)
    lib_loss, lib_d = _library(x, lab, dtype, ignore, smooth, cw, grad)
    got = [_raw(x, lab, ignore, smooth, cw, grad, ld, dtype) for ld in label_dtypes]
    for other in got[1:]:
        assert _same(got[0], other)
    loss, correct, sums, _, d = got[0]
    assert d.dtype == dtype and loss.dtype == torch.float32 and bool(torch.isfinite(loss))
    sums = sums.cpu()
    assert torch.equal(sums[..., 2], ref_sums[..., 2]), what                                  # the counts: exact
    sums_tol = 2e-6 + 5e-7 * float(x.abs().max())
    assert float((sums[..., :2] - ref_sums[..., :2]).abs().max()) <= sums_tol * float(ref_sums[..., :2].abs().max()), what
    out = []
    for name, g, r, l, floor in (("loss", loss.double().cpu(), ref_loss, lib_loss, 2e-6), ("dlogit", d.double().cpu(), ref_d, lib_d, FLOOR[dtype])):
        m = float(r.abs().max())
        if m == 0.0:                                                        # C = 1: the gradient is exactly 0
            assert float(g.abs().max()) == 0.0, (what, name)
            out.append(f"{name} exactly 0")
            continue
        ek, el = float((g - r).abs().max()) / m, float((l - r).abs().max()) / m
        out.append(f"{name} kernel {ek:.2e} library {el:.2e}")
        assert ek <= max(2.0 * el, floor), (what, name, ek, el)
    with capsys.disabled():
        print(f"\nresize_dice {IDS[dtype]} {what}: " + ", ".join(out), end="")
    return got[0]


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_vs_float64(shape, dtype, capsys):
    """Every shape, both logit dtypes, uint8 and int64 labels, about 20 % / none / all of the pixels ignored; `correct` is
    ppn_resize_ce_fwd's."""
    B, Cc, h, w, H, W = shape
    x = _logits(shape, dtype)
    for mode in ("mixed", "none", "all"):
        lab = _labels(shape, mode)
        loss, correct, sums, _, d = _check(x, lab, dtype, f"{shape} {mode}", capsys)
        assert correct == _ce_raw(x, lab, dtype=dtype, backward=False, lse=False)[1], (shape, mode)
        if mode == "all":
            assert correct == 0 and bool((sums[..., 0] == 0).all()) and bool((sums[:, :Cc - 1, 2] == 0).all())
            assert bool((sums[:, Cc - 1, 2] == H * W).all())                # an ignored 255 counts as class C - 1 in the denominator
        if Cc == 1:                                                           # p = 1: the closed form, and a gradient of exactly 0
            n_valid = (lab != 255).flatten(1).sum(1).double()
            want = float((1 - (2 * n_valid + 1) / (2 * H * W + 1)).mean())
            assert float(loss) == pytest.approx(want, rel=2e-6, abs=1e-7) and bool((d == 0).all())
            assert bool((sums[:, 0, 1] == H * W).all()) and torch.equal(sums[:, 0, 0].cpu(), n_valid)


# ------------------------------------------------------------------------------------------------ labels
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_out_of_range_labels(dtype, capsys):
    """A label outside [0, C) is not valid (the numerator, `correct`) and counts, clamped, in T of class 0 or C - 1.  Values that
    clamp to C - 1 — where 255 lands too — give the bits of the same call with those pixels set to ignore_index; negative ones move
    their counts from T[C - 1] to T[0], which is checked against the rule (the float64 reference applies it) like any other case."""
    shape = (2, 3, 3, 5, 6, 10)
    x = _logits(shape, dtype)
    g = torch.Generator().manual_seed(3)
    base = _labels(shape, "mixed")
    bad = torch.rand(base.shape, generator=g) < 0.25
    assert int(bad.sum()) > 0 and int((~bad & (base != 255)).sum()) > 0
    ignored = base.clone()
    ignored[bad] = 255
    for ld, values in ((torch.uint8, (7, 254)), (torch.int64, (7, 1 << 40, -1, -(1 << 40)))):
        want = _raw(x, ignored, label_dtype=ld, dtype=dtype)
        for v in values:
            oor = base.clone()
            oor[bad] = v
            got = _check(x, oor, dtype, f"{shape} label {v}", capsys, label_dtypes=(ld,))
            assert got[1] == want[1] and torch.equal(got[3], want[3]) and torch.equal(got[2][..., 0], want[2][..., 0])
            if v > 0:
                assert _same(got, want), (ld, v)
            else:
                moved = bad.flatten(1).sum(1).double().to(DEV)
                assert torch.equal(got[2][:, 0, 2], want[2][:, 0, 2] + moved) and torch.equal(got[2][:, 2, 2], want[2][:, 2, 2] - moved)
                assert torch.equal(got[2][:, 1], want[2][:, 1])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_ignore_index_1_class_weights_and_smooth(dtype, capsys):
    shape = (2, 3, 3, 5, 6, 10)
    x, lab = _logits(shape, dtype), _labels(shape, "none")
    assert int((lab == 1).sum()) > 0
    a = _check(x, lab, dtype, f"{shape} ignore_index 1", capsys, ignore=1)                 # class 1 is skipped, its pixels ignored
    b = _check(x, lab, dtype, f"{shape} ignore_index 1, weights", capsys, ignore=1, cw=(0.5, 7.0, 2.0))
    assert bool((a[2][:, 1, 0] == 0).all()) and float(a[0]) != float(b[0])
    assert bool((b[4][:, 1].float().abs().sum() > 0))                                       # class 1 still has a gradient through the softmax
    for shape in ((2, 2, 3, 5, 6, 10), (1, 19, 3, 2, 12, 8), (1, 3, 2, 3, 32, 48)):
        x, lab = _logits(shape, dtype), _labels(shape, "mixed")
        cw = tuple(0.5 + 0.75 * (c % 5) for c in range(shape[1]))
        _check(x, lab, dtype, f"{shape} class weights", capsys, cw=cw)
        _check(x, lab, dtype, f"{shape} smooth 0.5", capsys, smooth=0.5)
        _check(x, lab, dtype, f"{shape} smooth 0.5, weights, grad_out 0.4", capsys, smooth=0.5, cw=cw, grad=0.4)


# ------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_logits_of_80(dtype, capsys):
    """Logits scaled to +-80: a wrong maximum overflows exp."""
    for shape in ((2, 2, 3, 5, 6, 10), (1, 19, 3, 2, 12, 8), (1, 3, 2, 3, 32, 48)):
        x = _logits(shape, dtype, 80.0)
        assert _min_gap(x, *shape[-2:]) > 1e-3 and 79.0 <= float(x.abs().max()) <= 80.5
        loss, _, sums, lse, d = _check(x, _labels(shape, "mixed"), dtype, f"{shape} +-80", capsys)
        assert bool(torch.isfinite(lse).all()) and bool(torch.isfinite(loss)) and bool(torch.isfinite(d.float()).all())


# ------------------------------------------------------------------------------------------------ mechanics
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_repeatability_zero_gradient_and_no_lse(dtype):
    for shape in ((2, 2, 64, 64, 128, 128), (1, 3, 2, 3, 32, 48), (3, 2, 5, 7, 33, 37), (1, 2, 5, 7, 13, 9)):
        x, lab = _logits(shape, dtype), _labels(shape, "mixed")
        a, b, c = (_raw(x, lab, dtype=dtype, cw=tuple(1.0 + i for i in range(shape[1]))) for _ in range(3))
        assert _same(a, b) and _same(a, c) and a[4] is not None
    zero = _raw(x, lab, grad=0.0, dtype=dtype)
    assert bool((zero[4] == 0).all())
    # lse = NULL: the same loss, sums and count, nothing else written (the canaries in _raw)
    full = _raw(x, lab, dtype=dtype)
    d = _raw(x, lab, dtype=dtype, backward=False, lse=False)
    assert _same(full, d) and d[3] is None and d[4] is None


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("label_dtype", [torch.uint8, torch.int64], ids=["u8", "i64"])
def test_wrapper_returns_the_raw_bits(dtype, label_dtype, monkeypatch):
    from ppnet_amd import fused, heads
    shape = (2, 2, 64, 64, 128, 128)
    x, lab = _logits(shape, dtype), _labels(shape, "mixed")
    cw = (0.5, 2.0)
    raw = _raw(x, lab, smooth=0.5, cw=cw, grad=0.4, label_dtype=label_dtype, dtype=dtype)
    xg, lg = x.to(DEV, dtype).requires_grad_(True), lab.to(DEV, label_dtype)
    calls, ce_calls = dict(fused.DICE_CALLS), dict(fused.LOSS_CALLS)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append((tuple(t.shape), t.dtype)), t)[1], lambda t: t):
        loss, correct = fused.resize_dice(xg, lg, 255, 0.5, cw)
    assert sorted(saved, key=str) == sorted([((2, 2, 64, 64), dtype), ((2, 128, 128), label_dtype), ((2, 128, 128), torch.float32),
                                             ((2, 2, 3), torch.float64), ((2,), torch.float32)], key=str)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.requires_grad
    assert correct.shape == () and correct.dtype == torch.int64 and not correct.requires_grad
    (loss * 0.4).backward()
    assert torch.equal(loss.detach(), raw[0]) and int(correct) == raw[1]
    assert xg.grad.dtype == dtype and torch.equal(xg.grad, raw[4])
    assert fused.DICE_CALLS == {"fwd": calls["fwd"] + 1, "bwd": calls["bwd"] + 1} and fused.LOSS_CALLS == ce_calls
    # no_grad, or nothing that requires grad: no lse, no backward, the same loss
    seen = []
    inner = fused._resize_dice_fwd
    monkeypatch.setattr(fused, "_resize_dice_fwd", lambda *a: (seen.append(a[5]), inner(*a))[1])
    with torch.no_grad():
        l2, c2 = fused.resize_dice(xg, lg, 255, 0.5, cw)
    l3, c3 = fused.resize_dice(xg.detach(), lg, 255, 0.5, torch.tensor(cw, device=DEV))
    assert seen == [False, False] and not l2.requires_grad and not l3.requires_grad
    assert torch.equal(l2, raw[0]) and torch.equal(l3, raw[0]) and int(c2) == int(c3) == raw[1]
    assert fused.DICE_CALLS == {"fwd": calls["fwd"] + 3, "bwd": calls["bwd"] + 1}
    # heads.resized_dice_losses: the weight, the percentage, and what makes no launch
    lw, acc = heads.resized_dice_losses(xg.detach(), lg, 3.0, 0.5, 2, cw)
    assert torch.equal(lw, 3.0 * raw[0]) and float(acc) == pytest.approx(raw[1] * 100.0 / lab.numel(), rel=1e-6)
    n = fused.DICE_CALLS["fwd"]
    assert n == calls["fwd"] + 4
    full = F.interpolate(xg.detach().float(), (128, 128), mode="bilinear", align_corners=False)
    monkeypatch.setenv("PPNET_LIBRARY_LOSS", "1")
    lk, acck = heads.resized_dice_losses(xg.detach(), lg, 3.0, 0.5, 2, cw)
    monkeypatch.delenv("PPNET_LIBRARY_LOSS")
    assert torch.equal(lk, heads.dice_loss(full, lg, 0.5, 2, cw, 3.0)) and torch.equal(acck, acc)
    assert float(lk) == pytest.approx(float(lw), rel=1e-5)
    heads.resized_dice_losses(xg.detach(), lg, 3.0, 0.5, 2, cw, align_corners=True)
    l1, _ = heads.resized_dice_losses(xg.detach(), lg, 3.0, 0.5, 1, cw)                    # exponent 1: the torch form only
    assert torch.equal(l1, heads.dice_loss(full, lg, 0.5, 1, cw, 3.0))
    wide = torch.randn(1, MAX_C + 1, 2, 2, device=DEV, dtype=dtype)
    wl = torch.zeros(1, 4, 4, dtype=label_dtype, device=DEV)
    assert not fused.resize_dice_ok(wide, wl) and fused.resize_dice_ok(wide[:, :MAX_C].contiguous(), wl)
    heads.resized_dice_losses(wide, wl)
    with pytest.raises(ValueError):
        fused.resize_dice(wide, wl)
    with pytest.raises(ValueError):
        fused.resize_dice(xg.detach(), lg, smooth=-1.0)
    assert fused.DICE_CALLS["fwd"] == n


# ------------------------------------------------------------------------------------------------ model
# tests/test_gpu_seg_eval.py's tiny DiNAT + SETR-UP plus tests/test_gpu_resize_ce.py's FCN auxiliary head, [CE, Dice(loss_weight=3)] on both
LOSSES = [dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0), dict(type="DiceLoss", loss_weight=3.0)]
TINY_SEG = dict(
    backbone=dict(embed_dim=32, mlp_ratio=2.0, depths=[1, 1, 2, 1], num_heads=[1, 2, 4, 8], kernel_size=7, layer_scale=1e-1,
                  dilations=[[1], [2], [1, 2], [1]], drop_path_rate=0.0),
    decode_head=dict(in_channels=256, channels=32, num_convs=4, up_scale=2, num_classes=2, kernel_size=3, dropout_ratio=0.0,
                     loss_decode=LOSSES))
TINY_AUX = dict(type="FCNHead", in_channels=128, in_index=2, channels=32, num_convs=1, concat_input=False, dropout_ratio=0.0,
                num_classes=2, align_corners=False, loss_decode=LOSSES)
KEYS = ["decode.loss_ce", "decode.loss_dice", "decode.acc_seg", "aux.loss_ce", "aux.loss_dice", "aux.acc_seg"]


def _definition(net, img, gt):
    """forward_train's loss dict from the definition in the network's own dtype (no float32 stage: the float64 reference)."""
    from ppnet_amd import heads
    feats = net.backbone(img)
    losses = {}
    for name, head in (("decode", net.decode_head), ("aux", net.auxiliary_head)):
        z = F.interpolate(head(feats), gt.shape[-2:], mode="bilinear", align_corners=False)
        losses[f"{name}.loss_ce"] = F.cross_entropy(z, gt.long(), ignore_index=255, reduction="none").mean()
        losses[f"{name}.loss_dice"] = heads.dice_loss(z, gt, loss_weight=3.0)
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
def test_tiny_dinat_training_step_through_the_dice_kernels(tiny_model, autocast, monkeypatch, capsys):
    from ppnet_amd import fused
    cpu_net, img, gt, (ref_losses, ref_grads) = tiny_model
    net = copy.deepcopy(cpu_net).to(DEV)
    imgd, gtd = img.to(DEV), gt.to(DEV)
    calls, dice = dict(fused.LOSS_CALLS), dict(fused.DICE_CALLS)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(tuple(t.shape)), t)[1], lambda t: t):
        losses, grads = _model_run(net, imgd, gtd, autocast)
    assert fused.LOSS_CALLS == {"fwd": calls["fwd"] + 2, "bwd": calls["bwd"] + 2}
    assert fused.DICE_CALLS == {"fwd": dice["fwd"] + 2, "bwd": dice["bwd"] + 2}
    assert (2, 2, 64, 64) not in saved and saved.count((2, 2, 3)) == 2, saved            # the sums per head; no resized logits
    monkeypatch.setenv("PPNET_LIBRARY_LOSS", "1")
    lib_losses, lib_grads = _model_run(net, imgd, gtd, autocast)
    monkeypatch.delenv("PPNET_LIBRARY_LOSS")
    assert fused.LOSS_CALLS == {"fwd": calls["fwd"] + 2, "bwd": calls["bwd"] + 2}
    assert fused.DICE_CALLS == {"fwd": dice["fwd"] + 2, "bwd": dice["bwd"] + 2}
    assert list(losses) == list(lib_losses) == KEYS
    for k in ("decode", "aux"):
        for name in ("loss_ce", "loss_dice"):
            assert float(losses[f"{k}.{name}"]) == pytest.approx(float(lib_losses[f"{k}.{name}"]), rel=1e-5)
            if not autocast:
                assert float(losses[f"{k}.{name}"]) == pytest.approx(float(ref_losses[f"{k}.{name}"]), rel=1e-4)
        assert float(losses[f"{k}.acc_seg"]) == float(lib_losses[f"{k}.acc_seg"])
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
        print(f"\ntiny DiNAT + SETR-UP + aux, [CE, 3 Dice], {'bf16 autocast' if autocast else 'float32'}: worst parameter {worst[2]} kernel "
              f"path {worst[0]:.2e} x its max, library path {worst[1]:.2e}; dice {float(losses['decode.loss_dice']):.6f} / "
              f"{float(losses['aux.loss_dice']):.6f} (library {float(lib_losses['decode.loss_dice']):.6f} / {float(lib_losses['aux.loss_dice']):.6f})", end="")
