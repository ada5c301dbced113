"""ppn_seg_eval (csrc/seg_eval.hip) on the GPU: bilinear resize + argmax + the three per-class area histograms of a segmentation
evaluation, without the resized logits.

Reference: float64 on the CPU, F.interpolate(x.double(), bilinear, align_corners=False).argmax(1) followed by the masked bincounts, on
the exact input values (for bfloat16 the rounded ones, widened).  Logits are randn x 3; a pixel whose two largest float64 logits lie
within 1e-3 of each other (float32 interpolation error at these magnitudes is about 1e-5) gets its label set to ignore_index before
both sides run, so it drops out of every count and everything left must match EXACTLY (torch.equal on int64).  At most max(2 pixels,
1 %) of a case's pixels may be removed this way (asserted).  pred must equal the reference off that band and be < C on it.  Every raw
call runs on garbage-filled areas / pred buffers with canaries around both."""
import ctypes as C
import functools

import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
PX, THREADS, BALLOT_C, MAX_GROUPS = 1024, 256, 8, 1024      # csrc/seg_eval.hip: pixels per tile, work-items, ballot threshold, largest grid
PAD = 64                                                    # canary elements on either side of every output buffer
BAND = 1e-3
DTYPES = [torch.float32, torch.bfloat16]
IDS = {torch.float32: "f32", torch.bfloat16: "bf16"}

#          B  C   h   w   H    W
SHAPES = [(1, 2, 1, 1, 1, 1),
          (1, 2, 1, 1, 5, 3),
          (2, 2, 3, 5, 6, 10),
          (1, 2, 4, 4, 16, 16),
          (1, 3, 2, 3, 32, 48),
          (1, 2, 5, 7, 13, 9), (1, 3, 3, 3, 10, 11),
          (1, 4, 6, 4, 3, 4),                    # down-sampling
          (2, 2, 4, 4, 4, 4),                    # identity
          (1, 19, 3, 2, 12, 8),
          (1, 1, 2, 2, 4, 4),                    # C = 1: intersect = pred = label = the number of valid pixels
          # B H W one below, at and one above the pixels per tile
          (1, 2, 8, 8, 31, 33), (1, 2, 8, 8, 32, 32), (1, 2, 8, 8, 25, 41),
          # C one below, at and one above the threshold between wave ballots and LDS atomics
          (1, BALLOT_C - 1, 4, 4, 16, 16), (1, BALLOT_C, 4, 4, 16, 16), (1, BALLOT_C + 1, 4, 4, 16, 16),
          (1, 150, 4, 4, 16, 16),
          (2, 19, 8, 8, 32, 32),
          (3, 5, 7, 9, 40, 36),                  # W not a multiple of 4
          (2, 2, 64, 64, 128, 128),              # many workgroups into the same bins
          # one tile more than the largest grid: a workgroup strides over two tiles (ballots and LDS atomics)
          (1, 2, 8, 8, 1025, 1024), (1, 9, 8, 8, 1025, 1024)]
BIG_C = (1, 256, 2, 2, 8, 8)                     # int64 labels and ignore_index -100 (255 is a class)


def test_shapes_sit_on_the_boundaries():
    from ppnet_amd import fused
    assert fused.SEG_EVAL_PIXELS == PX and fused.SEG_EVAL_THREADS == THREADS
    assert fused.SEG_EVAL_BALLOT_CLASSES == BALLOT_C and fused.SEG_EVAL_MAX_GROUPS == MAX_GROUPS and fused.SEG_EVAL_MAX_CLASSES == 256
    px = {B * H * W for B, Cc, h, w, H, W in SHAPES}
    assert {PX - 1, PX, PX + 1} <= px
    assert {BALLOT_C - 1, BALLOT_C, BALLOT_C + 1} <= {s[1] for s in SHAPES}
    for ballot in (True, False):
        assert any(-(-(B * H * W) // PX) == MAX_GROUPS + 1 for B, Cc, h, w, H, W in SHAPES if (Cc <= BALLOT_C) == ballot)


# ------------------------------------------------------------------------------------------------ inputs and references
@functools.lru_cache(maxsize=None)
def _case(shape, dtype):
    """(CPU float32 logits already rounded to dtype, float64 argmax [B,H,W], near-tie band [B,H,W] bool) — computed once per case."""
    B, Cc, h, w, H, W = shape
    g = torch.Generator().manual_seed(B * 131 + Cc * 17 + H * 5 + W + 3)
    x = (torch.randn(B, Cc, h, w, generator=g) * 3.0).to(dtype).float()
    pred, band = _argmax64(x, H, W)
    n = int(band.sum())
    assert n <= max(2, 0.01 * B * H * W), (shape, n)                       # the condition of the exact comparison
    return x, pred, band


def _argmax64(x, H, W):
    z = F.interpolate(x.double(), (H, W), mode="bilinear", align_corners=False)
    if z.shape[1] == 1:
        return torch.zeros(z.shape[0], H, W, dtype=torch.int64), torch.zeros(z.shape[0], H, W, dtype=torch.bool)
    top = z.topk(2, dim=1).values
    return z.argmax(1), (top[:, 0] - top[:, 1]) < BAND


@functools.lru_cache(maxsize=None)
def _labels(shape, mode, ignore=255):
    """CPU int64 labels [B,H,W]: 'mixed' about 20 % ignored, 'none', 'all'."""
    B, Cc, h, w, H, W = shape
    g = torch.Generator().manual_seed(B * 131 + Cc * 17 + H * 5 + W)
    lab = torch.randint(0, min(Cc, 255) if ignore == 255 else Cc, (B, H, W), generator=g)
    if mode == "mixed":
        lab[torch.rand(B, H, W, generator=g) < 0.2] = ignore
    elif mode == "all":
        lab[:] = ignore
    return lab


def _ref_areas(pred, lab, Cc, ignore):
    valid = (lab != ignore) & (lab >= 0) & (lab < Cc)
    p, t = pred[valid], lab[valid]
    return torch.stack([torch.bincount(p[p == t], minlength=Cc), torch.bincount(p, minlength=Cc), torch.bincount(t, minlength=Cc)])


def _guarded(n, dtype, fill, canary, shift=0):
    buf = torch.full((n + 2 * PAD + shift,), canary, dtype=dtype, device=DEV)
    view = buf[PAD + shift:PAD + shift + n]
    view.fill_(fill)

    def intact():
        return bool((buf[:PAD + shift] == canary).all()) and bool((buf[PAD + shift + n:] == canary).all())
    return view, intact


def _raw(x, lab, ignore=255, label_dtype=torch.uint8, dtype=torch.float32, want_pred=True, pred_shift=0):
    """ppn_seg_eval straight through ctypes on garbage-filled, canary-guarded buffers: (areas [3,C] int64, pred [B,H,W] uint8 or
    None), on the GPU."""
    from ppnet_amd import _lib
    B, Cc, h, w = x.shape
    H, W = lab.shape[-2:]
    xg, lg = x.to(DEV, dtype).contiguous(), lab.to(DEV, label_dtype).contiguous()
    areas, areas_ok = _guarded(3 * Cc, torch.int64, -7, 0x5A5A5A5A)
    pred, pred_ok = _guarded(B * H * W, torch.uint8, 0xEE, 0xA5, pred_shift) if want_pred else (None, lambda: True)
    assert areas.data_ptr() % 8 == 0 and (pred is None or pred.data_ptr() % 4 == pred_shift % 4)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    ld, bd = {torch.float32: 0, torch.bfloat16: 1}[dtype], {torch.uint8: 0, torch.int64: 1}[label_dtype]
    rc = _lib.lib.ppn_seg_eval(p(xg), p(lg), p(pred), p(areas), B, Cc, h, w, H, W, ignore, ld, bd,
                               C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert areas_ok() and pred_ok(), "a canary was overwritten"
    return areas.clone().view(3, Cc).cpu(), (pred.clone().view(B, H, W).cpu() if want_pred else None)


def _check(shape, dtype, ignore, label_dtypes):
    """The rule for one case: about 20 % / none / all of the pixels ignored, every label dtype (bit-equal to each other), pred NULL
    and non-NULL (the same areas), all exactly the float64 reference outside the near-tie band."""
    B, Cc, h, w, H, W = shape
    x, ref_pred, band = _case(shape, dtype)
    for mode in ("mixed", "none", "all"):
        lab = _labels(shape, mode, ignore).clone()
        lab[band] = ignore
        want = _ref_areas(ref_pred, lab, Cc, ignore)
        for ld in label_dtypes:
            areas, pred = _raw(x, lab, ignore, ld, dtype, True)
            areas_only, none = _raw(x, lab, ignore, ld, dtype, False)
            assert none is None and torch.equal(areas, areas_only), (shape, mode, ld)
            assert areas.dtype == torch.int64 and torch.equal(areas, want), (shape, mode, ld, areas, want)
            assert pred.dtype == torch.uint8 and torch.equal(pred.long()[~band], ref_pred[~band]) and bool((pred.long()[band] < Cc).all())
            if mode == "all":
                assert int(areas.abs().sum()) == 0                          # exactly 0, and pred still written (compared above)
            if mode == "none":
                assert int(areas[1].sum()) == int(areas[2].sum()) == B * H * W - int(band.sum())
            if Cc == 1:
                n = int((lab == 0).sum())
                assert areas.flatten().tolist() == [n, n, n]


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_vs_float64(shape, dtype):
    _check(shape, dtype, 255, (torch.uint8, torch.int64))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_256_classes_int64_labels_ignore_minus_100(dtype):
    _check(BIG_C, dtype, -100, (torch.int64,))
    # and a smaller C with ignore_index -100, where 255 is one more out-of-range label
    shape = (2, 2, 3, 5, 6, 10)
    x, ref_pred, band = _case(shape, dtype)
    lab = _labels(shape, "mixed", -100).clone()
    lab[band] = -100
    a = _raw(x, lab, -100, torch.int64, dtype)[0]
    lab255 = lab.clone()
    lab255[lab == -100] = 255
    assert torch.equal(_raw(x, lab255, -100, torch.int64, dtype)[0], a) and torch.equal(a, _ref_areas(ref_pred, lab, 2, -100))


# ------------------------------------------------------------------------------------------------ labels
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_out_of_range_labels_count_as_ignored(dtype):
    shape = (2, 2, 3, 5, 6, 10)
    x, _, _ = _case(shape, dtype)
    g = torch.Generator().manual_seed(3)
    base = _labels(shape, "mixed")
    bad = torch.rand(base.shape, generator=g) < 0.25
    assert int(bad.sum()) > 0 and int((~bad & (base != 255)).sum()) > 0
    ignored = base.clone()
    ignored[bad] = 255
    for ld, values in ((torch.uint8, (7, 2, 254)), (torch.int64, (7, 2, 254, -1, 1 << 40, -(1 << 40) + 1))):
        want = _raw(x, ignored, 255, ld, dtype)
        for v in values:
            oor = base.clone()
            oor[bad] = v
            got = _raw(x, oor, 255, ld, dtype)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (ld, v)


# ------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_equal_logits_predict_class_0(dtype):
    for shape in ((1, 3, 3, 3, 10, 11), (1, 19, 3, 2, 12, 8), (1, 2, 4, 4, 16, 16)):
        B, Cc, h, w, H, W = shape
        g = torch.Generator().manual_seed(13)
        x = (torch.randn(B, 1, h, w, generator=g).expand(B, Cc, h, w).contiguous() * 3).to(dtype).float()
        lab = _labels(shape, "mixed")
        areas, pred = _raw(x, lab, dtype=dtype)
        assert int(pred.sum()) == 0
        valid = lab != 255
        assert int(areas[1, 0]) == int(valid.sum()) and int(areas[1, 1:].sum()) == 0
        assert int(areas[0, 0]) == int((lab == 0).sum()) and int(areas[0, 1:].sum()) == 0
        assert torch.equal(areas[2], torch.bincount(lab[valid], minlength=Cc))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_a_nan_logit_never_wins(dtype):
    """The one difference from torch.argmax: a pixel's NaN logits are skipped; with nothing but NaN the prediction is class 0."""
    shape = (1, 3, 4, 4, 16, 16)
    B, Cc, h, w, H, W = shape
    x = _case(shape, dtype)[0].clone()
    x[0, 0, 1, 1] = float("nan")                                            # class 0 at one source pixel
    x[0, 2, 0, 3] = float("nan")                                            # the last class at another
    x[0, :, 3, 0] = float("nan")                                            # every class at a third
    z = F.interpolate(x.double(), (H, W), mode="bilinear", align_corners=False)
    nan = torch.isnan(z)
    assert bool(nan[:, 0].any()) and bool(nan.all(1).any()) and not bool(nan.all())
    zz = z.clone()
    zz[nan] = -float("inf")
    ref = zz.argmax(1)
    ref[nan.all(1)] = 0
    top = torch.nan_to_num(zz, neginf=-1e30).topk(2, dim=1).values
    band = ((top[:, 0] - top[:, 1]) < BAND) & ~nan.all(1)
    lab = _labels(shape, "none").clone()
    lab[band] = 255
    areas, pred = _raw(x, lab, dtype=dtype)
    assert torch.equal(pred.long()[~band], ref[~band])
    assert torch.equal(areas, _ref_areas(ref, lab, Cc, 255))
    assert not bool((pred.long()[nan[:, 0] & ~nan.all(1)] == 0).any())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("label_dtype", [torch.uint8, torch.int64], ids=["u8", "i64"])
def test_intersect_sums_to_the_loss_kernels_correct_count(dtype, label_dtype):
    """The shared-tap claim: the evaluation's argmax is the one ppn_resize_ce_fwd counts, bit for bit — no band is masked here."""
    from ppnet_amd import fused
    for shape in ((2, 2, 64, 64, 128, 128), (2, 19, 8, 8, 32, 32), (3, 5, 7, 9, 40, 36), (1, 2, 5, 7, 13, 9), (1, 4, 6, 4, 3, 4)):
        x = _case(shape, dtype)[0]
        lab = _labels(shape, "mixed")
        areas, _ = _raw(x, lab, 255, label_dtype, dtype)
        _, correct, _ = fused._resize_ce_fwd(x.to(DEV, dtype).contiguous(), lab.to(DEV, label_dtype).contiguous(), 255, False)
        assert int(areas[0].sum()) == int(correct), shape
    # ties included: equal logits everywhere
    x = torch.ones(1, 3, 3, 3)
    lab = _labels((1, 3, 3, 3, 10, 11), "mixed")
    areas, _ = _raw(x, lab, 255, label_dtype, dtype)
    _, correct, _ = fused._resize_ce_fwd(x.to(DEV, dtype), lab.to(DEV, label_dtype), 255, False)
    assert int(areas[0].sum()) == int(correct) == int((lab == 0).sum())


# ------------------------------------------------------------------------------------------------ mechanics
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_repeatable_on_garbage_and_any_pred_alignment(dtype):
    for shape in ((2, 2, 64, 64, 128, 128), (2, 19, 8, 8, 32, 32), (1, 2, 5, 7, 13, 9)):
        x, lab = _case(shape, dtype)[0], _labels(shape, "mixed")
        a, b, c = (_raw(x, lab, dtype=dtype) for _ in range(3))              # each on areas / pred filled with garbage
        for u in (b, c):
            assert torch.equal(a[0], u[0]) and torch.equal(a[1], u[1])
        for shift in (1, 2, 3):                                             # pred at an odd address: byte stores, the same labels
            u = _raw(x, lab, dtype=dtype, pred_shift=shift)
            assert torch.equal(a[0], u[0]) and torch.equal(a[1], u[1]), (shape, shift)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_host_wrapper_counts_launches_and_returns_the_raw_bits(dtype, monkeypatch):
    from ppnet_amd import fused, heads
    shape = (3, 5, 7, 9, 40, 36)
    x, lab = _case(shape, dtype)[0], _labels(shape, "mixed")
    raw = _raw(x, lab, dtype=dtype)
    xg = x.to(DEV, dtype)
    calls = fused.EVAL_CALLS["fwd"]
    for ld in (torch.uint8, torch.int64):
        lg = lab.to(DEV, ld)
        assert fused.seg_eval_ok(xg, lg)
        areas, pred = fused.seg_eval(xg, lg, want_pred=True)
        assert areas.is_cuda and areas.dtype == torch.int64 and areas.shape == (3, 5) and torch.equal(areas.cpu(), raw[0])
        assert pred.dtype == torch.uint8 and torch.equal(pred.cpu(), raw[1])
        a2, none = fused.seg_eval(xg, lg)
        assert none is None and torch.equal(a2, areas)
        assert torch.equal(heads.resized_eval_areas(xg, lg), areas)
    assert fused.EVAL_CALLS["fwd"] == calls + 6
    # the knob, align_corners=True and C > 256 take the library composition: no launch
    lg = lab.to(DEV)
    monkeypatch.setenv("PPNET_LIBRARY_EVAL", "1")
    lib = heads.resized_eval_areas(xg, lg)
    monkeypatch.delenv("PPNET_LIBRARY_EVAL")
    assert lib.is_cuda and lib.dtype == torch.int64 and lib.shape == (3, 5)
    heads.resized_eval_areas(xg, lg, align_corners=True)
    wide = torch.randn(1, 257, 2, 2, device=DEV)
    assert not fused.seg_eval_ok(wide, lg[:1]) and heads.resized_eval_areas(wide, lg[:1]).shape == (3, 257)
    assert fused.EVAL_CALLS["fwd"] == calls + 6
    with pytest.raises(ValueError):
        fused.seg_eval(wide, lg[:1])


# ------------------------------------------------------------------------------------------------ model
# tests/test_gpu_resize_ce.py's tiny DiNAT + SETR-UP (stochastic depth and dropout at 0), in eval mode
TINY_SEG = dict(
    backbone=dict(embed_dim=32, mlp_ratio=2.0, depths=[1, 1, 2, 1], num_heads=[1, 2, 4, 8], kernel_size=7, layer_scale=1e-1,
                  dilations=[[1], [2], [1, 2], [1]], drop_path_rate=0.0),
    decode_head=dict(in_channels=256, channels=32, num_convs=4, up_scale=2, num_classes=2, kernel_size=3, dropout_ratio=0.0))


def test_tiny_dinat_eval_areas_is_one_launch(monkeypatch):
    from ppnet_amd import evaluate, fused, heads, train
    from ppnet_amd.segnet import SegNet, randomize_neutral_parameters
    torch.manual_seed(2)
    net = randomize_neutral_parameters(SegNet(**TINY_SEG), seed=3).eval().to(DEV)
    g = torch.Generator().manual_seed(4)
    img = torch.randn(2, 3, 64, 64, generator=g).to(DEV)
    gt = torch.randint(0, 2, (2, 64, 64), generator=g).to(torch.uint8)
    gt[torch.rand(2, 64, 64, generator=g) < 0.1] = 255
    with torch.no_grad():
        low = net.decode_head(net.backbone(img))
    assert low.shape[:2] == (2, 2) and low.dtype == torch.float32
    # near-tie pixels of these logits are masked by the rule of this file
    _, band = _argmax64(low.cpu(), 64, 64)
    assert int(band.sum()) <= max(2, 0.01 * gt.numel()), int(band.sum())
    gt[band] = 255
    gtd = gt.to(DEV)
    calls = fused.EVAL_CALLS["fwd"]
    got = net.eval_areas(img, gtd.unsqueeze(1))
    assert fused.EVAL_CALLS["fwd"] == calls + 1                             # one launch
    assert got.is_cuda and got.dtype == torch.int64 and got.shape == (3, 2)
    assert torch.equal(got, heads.resized_eval_areas(low, gtd))
    assert 0 < int(got[0].sum()) and int(got[1].sum()) == int(got[2].sum()) == int((gt != 255).sum())
    monkeypatch.setenv("PPNET_LIBRARY_EVAL", "1")
    lib = net.eval_areas(img, gtd)
    monkeypatch.delenv("PPNET_LIBRARY_EVAL")
    assert fused.EVAL_CALLS["fwd"] == calls + 2 and torch.equal(lib, got)
    # evaluate_segnet: the metrics of those areas, two batches of one image
    m = train.evaluate_segnet(net, img, gtd, batch=1, metrics=("mIoU", "mDice"))
    want = evaluate.total_area_to_metrics(got, ("mIoU", "mDice"))
    assert fused.EVAL_CALLS["fwd"] == calls + 4 and list(m) == list(want) == ["aAcc", "IoU", "Acc", "Dice"]
    for k in m:
        assert (m[k] == want[k]).all(), k
    assert not net.training
