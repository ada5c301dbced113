"""ppn_ohem_ce_fwd / ppn_ohem_ce_bwd (csrc/ohem_ce.hip) on the GPU: the heads' loss under OHEMPixelSampler and class weights without the
resized logits, the sampler as a radix select on the device.  Every raw call runs through ctypes on garbage-filled, canary-guarded
buffers (the workspace included: it needs no initialisation).

1. THE SELECT IS EXACT against the kernel's own scores: `score` is read back and sorted with torch, the cut computed by the rules
   (mode 1: t = max(asc[min(batch_kept, n_valid - 1)], thresh), selected = score < t, n_valid == 0: t = thresh; mode 2: t =
   asc[n_valid - min(batch_kept, n_valid)], selected = score >= t — ties all kept —, n_valid == 0: t = +inf) and mask, threshold,
   n_kept and n_valid must equal it bit for bit, on every input of this file.
2. SCORES, LOSS AND GRADIENT against float64 (F.interpolate(x.double()) + log_softmax on the CPU, the composition tests/
   test_ohem_golden.py pins to the reference): score, lse, and — with the kernel's own mask as a fixed weight — loss and dlogit.  The
   kernel's error may be at most max(2 x the error of the float32 library composition on the GPU, floor), both measured here against the
   same reference; floors as tests/test_gpu_resize_ce.py: 2e-6 of the largest reference value for float32 results, 1e-2 for a bfloat16 dlogit.
3. THE MASK against the float64 reference's own selection: equal outside the band |s64 - cut64| < 2 eps, where eps bounds the kernel's
   score error (the k-th order statistic moves by at most the largest score error, and so may a score: 2 eps).  Derivation of eps,
   with u = 2^-24, M = max |logit|, S = max(h, w), cwmax = max(1, max class weight):
     taps    the source index scale * (X + 0.5) - 0.5 <= S carries 4 roundings: the interpolation weight is off by <= 4 u S, and it
             multiplies a difference of neighbouring logits <= 2 M, per axis: 16 u S M; the 6 roundings of the products and sums of
             values <= M add 6 u M:                                              eps_z   = u M (16 S + 6)
     lse     a maximum (exact), C expf of arguments <= 0 (2 ulp each of values <= 1, averaged by the sum), C - 1 roundings of a sum, one
             logf (2 ulp) and one sum with the maximum:                           eps_lse = eps_z + 8 u (1 + M)
     ce      = lse - z_label, one more rounding of a value <= 2 M + log C:        eps_ce  = eps_lse + eps_z + 4 u (1 + M)
     p       = expf(-ce): an error d of the argument is a RELATIVE error d of p:   eps_p   = p (eps_ce + 2 u)
     score   mode 2: cw ce, one more rounding:  eps = cwmax E;   mode 1: p:  eps = E max(p, cut)   with E = 2 eps_z + 16 u (1 + M)
   (mode 1's bound is relative because the probabilities of a many-class head crowd near 0, where an absolute band of E would hold
   dozens of pixels whose float32 scores are in fact right to 1e-9.)  The band may hold at most max(2, 1 %) of the pixels: asserted
   from the float64 reference alone.
4. Two runs give bit-equal loss, mask and dlogit.
5. The public path: heads.resized_decode_losses(sampler=...) makes one forward and one backward entry call, none under
   PPNET_LIBRARY_LOSS=1; with neither sampler nor class weights OHEM_CALLS stays and LOSS_CALLS advances; a tiny SegNet with an OHEM
   sampler takes a training step."""
import ctypes as C
import functools
import math

import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
PAD = 64                                                    # canary elements on either side of every buffer
U = 2.0 ** -24
FLOOR = {torch.float32: 2e-6, torch.bfloat16: 1e-2}         # tests/test_gpu_resize_ce.py's
DTYPES = [torch.float32, torch.bfloat16]
IDS = {torch.float32: "f32", torch.bfloat16: "bf16"}
INF = float("inf")

#          B  C   h   w   H   W
SHAPES = [(2, 2, 7, 9, 28, 36),
          (1, 5, 8, 8, 13, 21),
          (3, 19, 6, 10, 24, 40),
          (2, 2, 16, 16, 64, 64),               # several workgroups
          (1, 3, 20, 20, 10, 10)]               # a downscale


def _modes(shape):
    """(name, thresh, min_kept): batch_kept = min_kept B stays below n_valid (about 80 % of the pixels).  'thresh': the 20 B-th smallest
    probability lies below 0.7, which is the cut; 'kth': thresh 1e-4 lies below the probability at the first quarter, which is the cut;
    'topk': the 20 B largest losses."""
    B, Cc, h, w, H, W = shape
    return [("thresh", 0.7, 20), ("kth", 1e-4, H * W // 4), ("topk", None, 20)]


def _cw(Cc):
    return [0.5 + 0.75 * (c % 4) for c in range(Cc)]


# ------------------------------------------------------------------------------------------------ inputs and references
@functools.lru_cache(maxsize=None)
def _logits(shape, dtype, scale=2.0):
    B, Cc, h, w, H, W = shape
    g = torch.Generator().manual_seed(B * 131 + Cc * 17 + H * 5 + W + 11)
    return (torch.randn(B, Cc, h, w, generator=g) * scale).to(dtype).float()         # CPU float32, already rounded to dtype


@functools.lru_cache(maxsize=None)
def _labels(shape, mode="mixed", ignore=255):
    """CPU int64 labels [B,H,W]: 'mixed' about 20 % ignored, 'none', 'all'."""
    B, Cc, h, w, H, W = shape
    g = torch.Generator().manual_seed(B * 131 + Cc * 17 + H * 5 + W)
    lab = torch.randint(0, Cc, (B, H, W), generator=g)
    if mode == "mixed":
        lab[torch.rand(B, H, W, generator=g) < 0.2] = ignore
    elif mode == "all":
        lab[:] = ignore
    return lab


def _valid(lab, Cc, ignore=255):
    return (lab != ignore) & (lab >= 0) & (lab < Cc)


def _composition(x, lab, cw, thresh, ignore, device, dtype):
    """The torch composition in `dtype` on `device`: (z leaf [B,C,h,w], lse, weighted ce, score), scores NaN on ignored pixels."""
    H, W = lab.shape[-2:]
    Cc = x.shape[1]
    xd = x.detach().to(device, dtype).requires_grad_(True)
    z = F.interpolate(xd, (H, W), mode="bilinear", align_corners=False)
    lab = lab.to(device)
    valid = _valid(lab, Cc, ignore)
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    logp = F.log_softmax(z, 1).gather(1, safe.unsqueeze(1)).squeeze(1)
    w = torch.ones(Cc, dtype=dtype, device=device) if cw is None else torch.tensor(cw, dtype=dtype, device=device)
    wce = -logp * w[safe]
    score = torch.where(valid, logp.exp() if thresh is not None else wce, torch.full_like(wce, float("nan")))
    return xd, torch.logsumexp(z, 1).detach(), wce, score.detach()


def _loss_and_grad(xd, wce, mask, grad):
    """loss = sum(mask * cw ce) / (B H W) and d(grad * loss)/dx for a FIXED 0 / 1 mask."""
    loss = (wce * mask.to(wce.dtype)).sum() / mask.numel()
    g, = torch.autograd.grad(loss * grad, xd)
    return loss.detach().double().cpu(), g.double().cpu()


def _rule(score, thresh, batch_kept):
    """The selection rule on a score tensor whose ignored pixels are NaN: (cut as a 0-d tensor of score's dtype, bool mask)."""
    valid = ~torch.isnan(score)
    asc = score[valid].sort().values
    n = asc.numel()
    if thresh is not None:
        t = torch.tensor(thresh, dtype=score.dtype)
        cut = t if n == 0 else torch.maximum(asc[min(batch_kept, n - 1)], t)
        return cut, valid & (score < cut)
    cut = torch.tensor(INF, dtype=score.dtype) if n == 0 else asc[n - min(batch_kept, n)]
    return cut, valid & (score >= cut)


def _eps(x, shape, cw, thresh, s64, cut64):
    """The bound on the kernel's score error per pixel (a tensor like s64): the module docstring's derivation."""
    B, Cc, h, w, H, W = shape
    M = float(x.abs().max())
    eps_z = U * M * (16 * max(h, w) + 6)
    E = 2 * eps_z + 16 * U * (1 + M)
    if thresh is None:
        return torch.full_like(s64, max(1.0, max(cw) if cw else 1.0) * E)
    return E * torch.maximum(torch.nan_to_num(s64, nan=0.0), cut64)


# ------------------------------------------------------------------------------------------------ the raw call
def _guarded(n, dtype, fill, canary):
    buf = torch.full((n + 2 * PAD,), canary, dtype=dtype, device=DEV)
    view = buf[PAD:PAD + n]
    view.fill_(fill)
    assert view.data_ptr() % 16 == 0

    def intact():
        return bool((buf[:PAD] == canary).all()) and bool((buf[PAD + n:] == canary).all())
    return view, intact


def _raw(x, lab, cw=None, thresh=None, min_kept=None, ignore=255, grad=1.0, label_dtype=torch.uint8, dtype=torch.float32, want_mask=True,
         backward=True):
    """ppn_ohem_ce_fwd (+ _bwd) straight through ctypes: a dict of CPU tensors — loss, counts [3], threshold, lse, score, mask, dlogit."""
    from ppnet_amd import _lib
    B, Cc, h, w = x.shape
    H, W = lab.shape[-2:]
    n = B * H * W
    mode = 0 if min_kept is None else (2 if thresh is None else 1)
    xg, lg = x.to(DEV, dtype).contiguous(), lab.to(DEV, label_dtype).contiguous()
    cwg = None if cw is None else torch.tensor(cw, dtype=torch.float32, device=DEV)
    need = _lib.lib.ppn_ohem_ce_workspace(B, H, W)
    assert need > 0 and need % 16 == 0
    nan = float("nan")
    ws, ws_ok = _guarded(need, torch.uint8, 0xEE, 0xA5)                        # garbage: the call initialises what it reads
    assert ws.data_ptr() % 16 == 0
    small, small_ok = _guarded(8, torch.float32, nan, 1024.0)                  # loss at [0], threshold at [4]
    cnt, cnt_ok = _guarded(4, torch.int64, -7, 0x5A5A5A5A)                     # counts [3]; the fourth stays -7
    lse, lse_ok = _guarded(n, torch.float32, nan, 1024.0)
    sc, sc_ok = _guarded(n, torch.float32, nan, 1024.0)
    mk, mk_ok = _guarded(n, torch.uint8, 0xEE, 0xA5) if want_mask else (None, lambda: True)
    dl, dl_ok = _guarded(x.numel(), dtype, nan, 1024.0)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    ld, bd = {torch.float32: 0, torch.bfloat16: 1}[dtype], {torch.uint8: 0, torch.int64: 1}[label_dtype]
    rc = _lib.lib.ppn_ohem_ce_fwd(p(xg), p(lg), p(cwg), p(lse), p(sc), p(small), p(cnt), p(small[4:]), p(mk), p(ws), need, B, Cc, h, w, H, W,
                                  ignore, mode, 1.0 if thresh is None else thresh, 1 if min_kept is None else min_kept, ld, bd, stream)
    assert rc == 0, rc
    if backward:
        g = torch.tensor(grad, dtype=torch.float32, device=DEV)
        rc = _lib.lib.ppn_ohem_ce_bwd(p(xg), p(lg), p(cwg), p(lse), p(sc), p(small[4:]), p(g), p(dl), B, Cc, h, w, H, W, ignore, mode, ld, bd, stream)
        assert rc == 0, rc
    torch.cuda.synchronize()
    assert ws_ok() and small_ok() and cnt_ok() and lse_ok() and sc_ok() and mk_ok() and dl_ok(), "a canary was overwritten"
    assert int(cnt[3]) == -7 and bool(torch.isnan(small[1:4]).all()) and bool(torch.isnan(small[5:]).all())
    assert not backward or bool(torch.isfinite(dl.float()).all())
    return dict(loss=small[0].cpu(), threshold=small[4].cpu(), counts=cnt[:3].cpu(), lse=lse.view(B, H, W).cpu(), score=sc.view(B, H, W).cpu(),
                mask=mk.view(B, H, W).cpu() if want_mask else None, dlogit=dl.view_as(xg).cpu() if backward else None)


def _check_select(out, lab, Cc, thresh, min_kept, ignore=255):
    """Rule 1: mask, threshold, n_kept and n_valid against torch's sort of the kernel's own scores.  Returns the bool mask."""
    B = lab.shape[0]
    score, valid = out["score"], _valid(lab, Cc, ignore)
    assert torch.equal(torch.isnan(score), ~valid)                            # the sentinel on the ignored pixels and nowhere else
    cut, mask = _rule(score, thresh, min_kept * B)
    assert torch.equal(out["mask"], mask.to(torch.uint8))
    assert out["threshold"].dtype == torch.float32 and torch.equal(out["threshold"], cut), (float(out["threshold"]), float(cut))
    assert int(out["counts"][1]) == int(valid.sum()) and int(out["counts"][2]) == int(mask.sum())
    return mask


def _equal_runs(a, b):
    return all(torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k], b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k])
               for k in a if a[k] is not None)


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_vs_float64(shape, dtype, capsys):
    """Every shape, both logit dtypes, uint8 and int64 labels, both modes, with and without class weights: rules 1 - 4."""
    B, Cc, h, w, H, W = shape
    x, lab = _logits(shape, dtype), _labels(shape)
    n_px, grad = B * H * W, 0.4
    lines = []
    for mode_name, thresh, min_kept in _modes(shape):
        for cw in (None, _cw(Cc)):
            what = f"{mode_name}{' cw' if cw else ''}"
            out = _raw(x, lab, cw, thresh, min_kept, grad=grad, label_dtype=torch.uint8, dtype=dtype)
            other = _raw(x, lab, cw, thresh, min_kept, grad=grad, label_dtype=torch.int64, dtype=dtype)
            assert _equal_runs(out, other), what                            # the label dtypes bit-equal; and rule 4, a second run
            assert out["dlogit"].dtype == dtype
            mask = _check_select(out, lab, Cc, thresh, min_kept)
            assert 0 < int(mask.sum()) <= int(_valid(lab, Cc).sum()) - (thresh is None or thresh < 0.5)       # the sampler selects
            # rule 2
            x64, lse64, wce64, s64 = _composition(x, lab, cw, thresh, 255, "cpu", torch.float64)
            x32, lse32, wce32, s32 = _composition(x, lab, cw, thresh, 255, DEV, torch.float32)
            ref_loss, ref_d = _loss_and_grad(x64, wce64, mask, grad)
            lib_loss, lib_d = _loss_and_grad(x32, wce32, mask.to(DEV), grad)
            correct = int(((F.interpolate(x.double(), (H, W), mode="bilinear", align_corners=False).argmax(1) == lab)).sum())
            assert abs(int(out["counts"][0]) - correct) <= max(2, 0.01 * n_px)                # near-ties of two classes aside
            v = _valid(lab, Cc)
            for name, got, ref, lib, floor in (("lse", out["lse"].double(), lse64, lse32.double().cpu(), 2e-6),
                                               ("score", out["score"].double()[v], s64[v], s32.double().cpu()[v], 2e-6),
                                               ("loss", out["loss"].double(), ref_loss, lib_loss, 2e-6),
                                               ("dlogit", out["dlogit"].double(), ref_d, lib_d, FLOOR[dtype])):
                m = float(ref.abs().max())
                assert m > 0.0
                ek, el = float((got - ref).abs().max()) / m, float((lib - ref).abs().max()) / m
                lines.append(f"{what} {name} kernel {ek:.2e} library {el:.2e}")
                with capsys.disabled():
                    print(f"\nohem {IDS[dtype]} {'x'.join(map(str, shape))} {lines[-1]}", end="")
                assert ek <= max(2.0 * el, floor), (what, name, ek, el)
            # rule 3
            cut64, mask64 = _rule(s64, thresh, min_kept * B)
            eps = _eps(x, shape, cw, thresh, s64, cut64)
            band = (s64 - cut64).abs() < 2 * eps
            assert int(band.sum()) <= max(2, 0.01 * n_px), (what, int(band.sum()))             # from the float64 reference alone
            assert torch.equal(mask[~band], mask64[~band]), (what, int((mask != mask64).sum()))
            assert bool(((out["score"].double()[v] - s64[v]).abs() <= eps[v]).all()), what    # the bound the band rests on


# ------------------------------------------------------------------------------------------------ the select's hard inputs
def _select_only(x, lab, thresh, min_kept, dtype=torch.float32, label_dtype=torch.uint8, cw=None, ignore=255):
    out = _raw(x, lab, cw, thresh, min_kept, ignore=ignore, dtype=dtype, label_dtype=label_dtype)
    again = _raw(x, lab, cw, thresh, min_kept, ignore=ignore, dtype=dtype, label_dtype=label_dtype)
    assert _equal_runs(out, again)
    return out, _check_select(out, lab, x.shape[1], thresh, min_kept, ignore)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=lambda s: "x".join(map(str, s)))
def test_select_when_every_key_shares_its_leading_digits(shape):
    """Logits 1 + 1e-3 randn: C = 2 probabilities within 3e-3 of 0.5 and losses within 3e-3 of log 2 — the first two digits of the key
    (22 bits) are nearly the same for every pixel, the third decides.  thresh 0.3 lies below every probability, so the k-th one is the
    cut.  Expected from the rules, with k = min_kept B: mode 1 keeps the scores strictly below asc[k] — k of them, less those that tie
    with asc[k] from below; mode 2 keeps k plus the pixels further down that tie with the cut."""
    B, Cc, h, w, H, W = shape
    g = torch.Generator().manual_seed(5)
    x = 1.0 + 1e-3 * torch.randn(B, Cc, h, w, generator=g)
    lab = _labels(shape)
    n_valid, k = int(_valid(lab, Cc).sum()), 20 * B
    assert k < n_valid - 1
    out, mask = _select_only(x, lab, 0.3, 20)
    asc = out["score"][~torch.isnan(out["score"])].sort().values
    assert 0.49 < float(asc[0]) and float(asc[-1]) < 0.51 and float(out["threshold"]) == float(asc[k])
    assert int(out["counts"][2]) == int((asc < asc[k]).sum()) <= k
    out, mask = _select_only(x, lab, None, 20)
    asc = out["score"][~torch.isnan(out["score"])].sort().values
    assert abs(float(asc[0]) - math.log(2)) < 5e-3 and abs(float(asc[-1]) - math.log(2)) < 5e-3
    assert int(out["counts"][2]) == k + int((asc[:n_valid - k] == asc[n_valid - k]).sum())


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=lambda s: "x".join(map(str, s)))
def test_select_when_every_score_ties(shape):
    """All-zero logits: every pixel has p = 1 / C and loss log C, exactly.  Expected from the rules: mode 2 — the cut ties with every
    pixel, all n_valid are kept whatever batch_kept is; mode 1 with thresh 0.7 > 1 / C — every p is below it, n_valid; mode 1 with
    thresh 0.1 < 1 / C — t = p itself and p < t is strict: 0."""
    B, Cc, h, w, H, W = shape
    x, lab = torch.zeros(B, Cc, h, w), _labels(shape)
    n_valid = int(_valid(lab, Cc).sum())
    for thresh, want in ((None, n_valid), (0.7, n_valid), (0.1, 0)):
        out, mask = _select_only(x, lab, thresh, 2)
        assert int(out["counts"][2]) == want == int(mask.sum()), (thresh, want)
        s = out["score"][~torch.isnan(out["score"])]
        assert bool((s == s[0]).all())
        if thresh is None or thresh == 0.1:
            assert float(out["threshold"]) == float(s[0])
        assert float(out["loss"]) == pytest.approx(want * math.log(Cc) / (B * H * W), rel=1e-6)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_batch_kept_beyond_the_valid_pixels(dtype):
    """min_kept B >= n_valid.  Expected from the rules: mode 2 keeps all n_valid; mode 1 takes the LARGEST probability as the candidate
    (thresh 0.05 lies below it) and keeps what is strictly below it: n_valid less the pixels that tie with the largest."""
    shape = SHAPES[0]
    B, Cc = shape[:2]
    x, lab = _logits(shape, dtype), _labels(shape)
    n_valid = int(_valid(lab, Cc).sum())
    for min_kept in (-(-n_valid // B), 100000, 2 ** 31 - 1):                  # at n_valid, the reference's default, and min_kept B past 2^31
        out, mask = _select_only(x, lab, None, min_kept, dtype)
        assert int(out["counts"][2]) == n_valid and torch.equal(mask, _valid(lab, Cc))
        out, mask = _select_only(x, lab, 0.05, min_kept, dtype)
        s = out["score"][~torch.isnan(out["score"])]
        assert float(out["threshold"]) == float(s.max()) and int(out["counts"][2]) == n_valid - int((s == s.max()).sum())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_every_label_ignored(dtype):
    """Expected from the rules: nothing is valid, nothing is kept, the loss and every gradient are exactly 0; t = thresh / +inf."""
    shape = SHAPES[2]
    x, lab = _logits(shape, dtype), _labels(shape, "all")
    for thresh, cw in ((0.7, None), (None, _cw(shape[1])), (0.7, _cw(shape[1]))):
        out, mask = _select_only(x, lab, thresh, 20, dtype, cw=cw)
        assert out["counts"].tolist() == [0, 0, 0] and int(mask.sum()) == 0
        assert float(out["loss"]) == 0.0 and float(out["dlogit"].float().abs().max()) == 0.0
        assert float(out["threshold"]) == (float(torch.tensor(0.7, dtype=torch.float32)) if thresh else INF)


def test_labels_outside_the_classes_are_ignored():
    """int64 labels C, C + 100, -1 and -100 beside 255: never indexed, never counted, never selected — bit for bit the run with 255
    in their place (ignore_index -100 as well: then 255 is out of range for C = 5 and ignored by that rule)."""
    shape = SHAPES[1]
    B, Cc, h, w, H, W = shape
    x, lab = _logits(shape, torch.float32), _labels(shape).clone()
    g = torch.Generator().manual_seed(9)
    r = torch.rand(B, H, W, generator=g)
    wild = lab.clone()
    for lo, v in ((0.0, Cc), (0.05, Cc + 100), (0.1, -1), (0.15, -100)):
        wild[(r >= lo) & (r < lo + 0.05)] = v
    clean = torch.where(_valid(wild, Cc), wild, torch.full_like(wild, 255))
    assert int((wild != clean).sum()) > 10
    for thresh, cw in ((0.7, None), (None, _cw(Cc))):
        want = _raw(x, clean, cw, thresh, 10, label_dtype=torch.int64)
        for ignore in (255, -100):
            out, mask = _select_only(x, wild, thresh, 10, label_dtype=torch.int64, cw=cw, ignore=ignore)
            assert _equal_runs(out, want)
            assert int(out["counts"][1]) == int(_valid(wild, Cc).sum())


def test_no_sampler_is_the_weighted_mean_and_mask_may_be_null():
    """mode 0 (class weights only): every valid pixel selected, t = -inf; mask NULL gives the same loss and gradient."""
    shape = SHAPES[2]
    B, Cc, h, w, H, W = shape
    x, lab, cw = _logits(shape, torch.float32), _labels(shape), _cw(shape[1])
    out = _raw(x, lab, cw, None, None, grad=1.0)
    bare = _raw(x, lab, cw, None, None, grad=1.0, want_mask=False)
    assert torch.equal(out["mask"].bool(), _valid(lab, Cc)) and float(out["threshold"]) == -INF
    assert int(out["counts"][2]) == int(out["counts"][1]) == int(_valid(lab, Cc).sum())
    assert torch.equal(out["loss"], bare["loss"]) and torch.equal(out["dlogit"], bare["dlogit"])
    x64, _, wce64, _ = _composition(x, lab, cw, None, 255, "cpu", torch.float64)
    ref_loss, ref_d = _loss_and_grad(x64, wce64, _valid(lab, Cc), 1.0)
    x32, _, wce32, _ = _composition(x, lab, cw, None, 255, DEV, torch.float32)
    lib_loss, lib_d = _loss_and_grad(x32, wce32, _valid(lab, Cc).to(DEV), 1.0)
    for got, ref, lib in ((out["loss"].double(), ref_loss, lib_loss), (out["dlogit"].double(), ref_d, lib_d)):
        m = float(ref.abs().max())
        assert float((got - ref).abs().max()) / m <= max(2.0 * float((lib - ref).abs().max()) / m, 2e-6)
    # all ones as class weights is no class weights, bit for bit
    ones = _raw(x, lab, [1.0] * Cc, 0.7, 20)
    none = _raw(x, lab, None, 0.7, 20)
    assert _equal_runs(ones, none)


# ------------------------------------------------------------------------------------------------ the public path
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_resized_decode_losses_takes_the_fused_path(dtype, monkeypatch):
    from ppnet_amd import fused
    from ppnet_amd.heads import OHEMPixelSampler, resized_decode_losses
    shape = SHAPES[0]
    B, Cc, h, w, H, W = shape
    x, lab, cw = _logits(shape, dtype), _labels(shape), [1.0, 2.0]
    # thresh = the middle of the widest gap between the float64 probabilities in [0.5, 0.8] (as a float32): it is the cut (the 100th
    # smallest probability lies below it) and no probability comes within the band of it, so the kernels, the library composition
    # and the float64 reference select the same pixels
    x64, _, wce64, s64 = _composition(x, lab, cw, 0.7, 255, "cpu", torch.float64)
    ps = s64[~torch.isnan(s64)].sort().values
    ps = ps[(ps >= 0.5) & (ps <= 0.8)]
    i = int((ps[1:] - ps[:-1]).argmax())
    thresh = float(((ps[i] + ps[i + 1]) / 2).float())
    sampler = OHEMPixelSampler(thresh=thresh, min_kept=50)
    cut64, mask64 = _rule(s64, thresh, sampler.min_kept * B)
    assert float(cut64) == thresh and int(((s64 - cut64).abs() < 2 * _eps(x, shape, cw, thresh, s64, cut64)).sum()) == 0
    ref_loss, ref_d = _loss_and_grad(x64, wce64, mask64, 0.4)
    raw = _raw(x, lab, cw, thresh, 50, grad=0.4, dtype=dtype)
    assert torch.equal(raw["mask"].bool(), mask64)

    def run():
        xg = x.to(DEV, dtype).requires_grad_(True)
        loss, acc = resized_decode_losses(xg, lab.to(DEV, torch.uint8), 0.4, class_weight=cw, sampler=sampler)
        loss.backward()
        return loss.detach(), acc, xg.grad
    ohem, plain = dict(fused.OHEM_CALLS), dict(fused.LOSS_CALLS)
    loss, acc, d = run()
    assert fused.OHEM_CALLS == {"fwd": ohem["fwd"] + 1, "bwd": ohem["bwd"] + 1} and fused.LOSS_CALLS == plain
    assert loss.dtype == torch.float32 and d.dtype == dtype
    assert torch.equal(loss, 0.4 * raw["loss"].to(DEV)) and torch.equal(d.cpu(), raw["dlogit"])
    assert float(acc) == pytest.approx(int(raw["counts"][0]) * 100.0 / lab.numel(), rel=1e-6)
    monkeypatch.setenv("PPNET_LIBRARY_LOSS", "1")
    lib_loss, lib_acc, lib_d = run()
    monkeypatch.delenv("PPNET_LIBRARY_LOSS")
    assert fused.OHEM_CALLS == {"fwd": ohem["fwd"] + 1, "bwd": ohem["bwd"] + 1} and fused.LOSS_CALLS == plain
    assert float(lib_acc) == float(acc)
    for got, lib, ref, floor in ((loss, lib_loss, 0.4 * ref_loss, 2e-6), (d, lib_d, ref_d, FLOOR[dtype])):
        m = float(ref.abs().max())
        ek, el = float((got.double().cpu() - ref).abs().max()) / m, float((lib.double().cpu() - ref).abs().max()) / m
        assert ek <= max(2.0 * el, floor), (ek, el)
    # the top-k form and want_mask through fused.ohem_cross_entropy
    xg, lg = x.to(DEV, dtype), lab.to(DEV)
    l2, correct, n_kept, mask = fused.ohem_cross_entropy(xg, lg, 255, None, None, 50, want_mask=True)
    r2 = _raw(x, lab, None, None, 50, label_dtype=torch.int64, dtype=dtype, backward=False)
    assert torch.equal(l2.cpu(), r2["loss"]) and int(correct) == int(r2["counts"][0]) and int(n_kept) == int(r2["counts"][2]) == int(mask.sum())
    assert torch.equal(mask.cpu(), r2["mask"]) and not l2.requires_grad
    # neither sampler nor class weights: today's kernels
    ohem = dict(fused.OHEM_CALLS)
    xg = x.to(DEV, dtype).requires_grad_(True)
    resized_decode_losses(xg, lab.to(DEV, torch.uint8), 0.4)[0].backward()
    assert fused.OHEM_CALLS == ohem and fused.LOSS_CALLS == {"fwd": plain["fwd"] + 1, "bwd": plain["bwd"] + 1}
    # align_corners=True is the library's
    resized_decode_losses(xg.detach(), lab.to(DEV), 1.0, align_corners=True, sampler=sampler)
    assert fused.OHEM_CALLS == ohem


def test_the_autograd_function_saves_no_weight_tensor():
    from ppnet_amd import fused
    shape = SHAPES[3]
    x, lab = _logits(shape, torch.bfloat16), _labels(shape)
    xg, lg = x.to(DEV, torch.bfloat16).requires_grad_(True), lab.to(DEV, torch.uint8)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append((tuple(t.shape), t.dtype)), t)[1], lambda t: t):
        loss, correct, n_kept = fused.ohem_cross_entropy(xg, lg, thresh=0.7, min_kept=100)
    # logit, labels, lse, score, threshold — no [B,C,H,W] logits, no [B,H,W] weight
    assert sorted(saved, key=str) == sorted([((2, 2, 16, 16), torch.bfloat16), ((2, 64, 64), torch.uint8), ((2, 64, 64), torch.float32),
                                             ((2, 64, 64), torch.float32), ((), torch.float32)], key=str)
    assert loss.requires_grad and not correct.requires_grad and not n_kept.requires_grad


def test_tiny_segnet_takes_a_training_step_with_an_ohem_sampler():
    """tests/test_gpu_train.py's DiNAT widths at 64 x 64 with sampler=dict(type='OHEMPixelSampler', thresh=0.7, min_kept=500) on the
    SETR-UP head and class weights on an FCN auxiliary head: one segnet_train_step, a finite loss, finite non-zero gradients, two OHEM
    forward and backward calls and none of the plain loss kernels."""
    from ppnet_amd import fused, train
    from ppnet_amd.segnet import SegNet
    torch.manual_seed(1)
    net = SegNet(
        backbone=dict(embed_dim=32, mlp_ratio=2.0, depths=[1, 1, 2, 1], num_heads=[1, 2, 4, 8], kernel_size=7, layer_scale=1e-1,
                      dilations=[[1], [2], [1, 2], [1]], drop_path_rate=0.1),
        decode_head=dict(in_channels=256, channels=32, num_convs=4, up_scale=2, num_classes=2, kernel_size=3,
                         sampler=dict(type="OHEMPixelSampler", thresh=0.7, min_kept=500)),
        auxiliary_head=dict(type="FCNHead", in_channels=128, in_index=2, channels=32, num_convs=1, concat_input=False, num_classes=2,
                            loss_decode=dict(type="CrossEntropyLoss", loss_weight=0.4, class_weight=[1.0, 2.0]))).cuda()
    assert net.decode_head.sampler.min_kept == 500 and net.auxiliary_head.class_weight == (1.0, 2.0)
    g = torch.Generator().manual_seed(2)
    free = torch.rand(2, 64, 64, generator=g) > 0.4
    grid, space = (free.to(torch.uint8) * 255).cuda(), free.to(torch.uint8).cuda()
    trainer = train.segnet_trainer(net)
    opt = train.segnet_optimizer(trainer, lr=0.02)
    ohem, plain = dict(fused.OHEM_CALLS), dict(fused.LOSS_CALLS)
    loss = train.segnet_train_step(trainer, opt, 0, 40, grid, space, schedule=dict(warmup_iters=0))
    assert math.isfinite(float(loss)) and float(loss) > 0.0
    assert fused.OHEM_CALLS == {"fwd": ohem["fwd"] + 2, "bwd": ohem["bwd"] + 2} and fused.LOSS_CALLS == plain
    grads = {n: p.grad for n, p in net.named_parameters() if p.requires_grad}
    assert all(v is not None and bool(torch.isfinite(v).all()) for v in grads.values())
    assert all(float(v.abs().max()) > 0.0 for n, v in grads.items() if n.endswith("conv_seg.weight"))
    assert sum(float(v.abs().max()) > 0.0 for v in grads.values()) >= 0.9 * len(grads)
