"""ppn_seg_tta (csrc/seg_tta.hip) on the GPU against a float64 CPU reference: heads.tta_mean_prob's composition written out with
F.interpolate(x.double(), ...) on the exact input values (for bfloat16 the rounded ones, widened).  Logits are randn x 3, seeded per case.

Labels must equal the reference's argmax exactly outside a near-tie band — the pixels whose two largest float64 mean probabilities differ
by less than 1e-5 (the float32 library composition on the CPU stays within 7e-7 of float64 on these shapes) — the band may hold at most
max(2, 1 %) of a case's pixels, and on it pred < C.  Probabilities: absolute error against float64 at most max(1e-6, 4 x e32), e32 the
error of the CPU float32 library composition against the same reference on that case: the bound is measured against the reference, not
against the kernel.  Every raw call runs on garbage-filled outputs with canaries on both sides, at pred offsets 0 to 3 bytes, and the
four runs are bit-equal.

Largest kernel errors observed on an MI355X over the cases below: see DESIGN.md section 25."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BAND = 1e-5
H_, V_ = "horizontal", "vertical"


def A(h, w, hm, wm, flip=None):
    return (h, w, hm, wm, flip)


def ratios12(H, W, down=4):
    """the reference's --aug-test: six ratios x {none, horizontal}, the head at 1 / down of each image size"""
    out = []
    for r in (0.5, 0.75, 1.0, 1.25, 1.5, 1.75):
        hm, wm = int(H * r), int(W * r)
        out += [A(max(hm // down, 1), max(wm // down, 1), hm, wm), A(max(hm // down, 1), max(wm // down, 1), hm, wm, H_)]
    return out


def sixteen(H, W):
    """every piece in one call: identity / up- / down-sampling stage 2, stage-1 down-sampling (h > hm), h = w = 1, three flips"""
    return [A(4, 3, H, W), A(4, 3, H, W, H_), A(4, 3, H, W, V_), A(7, 5, H // 2, W // 2), A(7, 5, H // 2, W // 2, V_),
            A(3, 2, int(1.75 * H), int(1.75 * W), H_), A(1, 1, H, W), A(1, 1, 3, 2, V_), A(9, 11, 5, 4), A(9, 11, 5, 4, H_),
            A(H, W, H, W), A(H, W, 2 * H, 2 * W, V_), A(2, 7, 6, 5, H_), A(5, 1, 7, 3), A(1, 6, 2, 9, V_), A(6, 6, 12, 12, H_)]


#        name             B  C    H    W   augmentations
CASES = [("1x1",          1, 2,   1,   1, [A(1, 1, 1, 1)]),
         ("1x1_flips",    2, 3,   1,   1, [A(2, 2, 3, 3, H_), A(1, 1, 1, 1, V_)]),
         ("5x3_from_1x1", 2, 3,   5,   3, [A(1, 1, 2, 2), A(1, 1, 5, 3, H_)]),
         ("13x9",         2, 3,  13,   9, [A(4, 3, 13, 9), A(7, 5, 6, 4, V_), A(3, 2, 22, 15, H_)]),
         ("33x31",        1, 8,  33,  31, [A(9, 8, 33, 31), A(5, 4, 16, 15, H_)]),
         ("tile_12",      1, 2,  32,  32, ratios12(32, 32)),
         ("1023",         3, 2,  11,  31, [A(3, 8, 11, 31, V_), A(6, 16, 19, 54)]),
         ("1025",         5, 9,   5,  41, [A(2, 11, 5, 41, H_), A(4, 30, 2, 20, V_)]),
         ("groups",       2, 2, 128, 128, [A(32, 32, 128, 128), A(16, 16, 64, 64, H_)]),
         ("C1_2",         2, 1,  13,   9, [A(4, 3, 13, 9), A(7, 5, 6, 4, H_)]),
         ("C2_1",         2, 2,  13,   9, [A(7, 5, 22, 15, V_)]),
         ("C3_16",        1, 3,  13,   9, sixteen(13, 9)),
         ("C8_16",        2, 8,  13,   9, sixteen(13, 9)),
         ("C9_12",        1, 9,  32,  32, ratios12(32, 32)),
         ("C9_1",         2, 9,  13,   9, [A(4, 3, 13, 9)]),
         ("C19_16",       2, 19, 13,   9, sixteen(13, 9)),
         ("C64_3",        2, 64, 13,   9, [A(4, 3, 13, 9, V_), A(7, 5, 6, 4), A(3, 2, 22, 15, H_)]),     # the last C with its logits in LDS
         ("C65_3",        2, 65, 13,   9, [A(4, 3, 13, 9, V_), A(7, 5, 6, 4), A(3, 2, 22, 15, H_)]),     # the first without
         ("C150_12",      1, 150, 16, 16, ratios12(16, 16)),
         ("C256_16",      1, 256, 13,  9, sixteen(13, 9)),
         ("C256_2",       1, 256, 33, 31, [A(9, 8, 33, 31, H_), A(5, 4, 57, 54)])]
DTYPES = [torch.float32, torch.bfloat16]


def ref64(logits, mids, flips, out_hw):
    total = None
    for x, mid, fl in zip(logits, mids, flips):
        z = F.interpolate(x.double(), tuple(mid), mode="bilinear", align_corners=False)
        p = F.softmax(F.interpolate(z, tuple(out_hw), mode="bilinear", align_corners=False), dim=1)
        if fl is not None:
            p = p.flip(dims=(3,) if fl == H_ else (2,))
        total = p if total is None else total + p
    return total / len(logits)


@functools.lru_cache(maxsize=None)
def case(i, dtype):
    """(CPU logits in `dtype`, mids, flips, (H, W), float64 reference, e32) of CASES[i]; computed once, never modified"""
    from ppnet_amd import heads
    name, B, Cn, H, W, augs = CASES[i]
    g = torch.Generator().manual_seed(1000 + i)
    logits = [(torch.randn(B, Cn, h, w, generator=g) * 3).to(dtype) for h, w, _, _, _ in augs]
    mids, flips = [(a[2], a[3]) for a in augs], [a[4] for a in augs]
    ref = ref64(logits, mids, flips, (H, W))
    e32 = float((heads.tta_mean_prob([x.float() for x in logits], mids, flips, (H, W)).double() - ref).abs().max())
    return logits, mids, flips, (H, W), ref, e32


def raw(logits, mids, flips, out_hw, off=0, want_pred=True, want_prob=True):
    """ppn_seg_tta itself on garbage-filled outputs between canaries; pred starts `off` bytes past a 4-byte boundary"""
    from ppnet_amd import _lib
    dev = logits[0].device
    B, Cn = logits[0].shape[:2]
    H, W = out_hw
    n, N = B * H * W, B * Cn * H * W
    pbuf = torch.full((n + 16,), 0xA5, dtype=torch.uint8, device=dev)
    qbuf = torch.full((N + 8,), 12345.0, dtype=torch.float32, device=dev)
    augs = (_lib.TtaAug * len(logits))()
    for a, x, mid, fl in zip(augs, logits, mids, flips):
        assert x.is_contiguous()
        a.logit, a.h, a.w, a.hm, a.wm, a.flip = x.data_ptr(), x.shape[2], x.shape[3], mid[0], mid[1], {None: 0, H_: 1, V_: 2}[fl]
    rc = _lib.lib.ppn_seg_tta(augs, len(logits), C.c_void_p(pbuf.data_ptr() + 4 + off if want_pred else None),
                              C.c_void_p(qbuf.data_ptr() + 16 if want_prob else None), B, Cn, H, W,
                              0 if logits[0].dtype == torch.float32 else 1, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    pb, qb = pbuf.cpu(), qbuf.cpu()
    lo, hi = (4 + off, 4 + off + n) if want_pred else (0, 0)
    assert bool((pb[:lo] == 0xA5).all()) and bool((pb[hi:] == 0xA5).all()), "pred wrote outside [B][H][W]"
    lo, hi = (4, 4 + N) if want_prob else (0, 0)
    assert bool((qb[:lo] == 12345.0).all()) and bool((qb[hi:] == 12345.0).all()), "prob wrote outside [B][C][H][W]"
    pred = pb[4 + off:4 + off + n].reshape(B, H, W).clone() if want_pred else None
    prob = qb[4:4 + N].reshape(B, Cn, H, W).clone() if want_prob else None
    return pred, prob


def check_labels(pred, ref, what):
    """exact outside the near-tie band, which holds at most max(2, 1 %) of the pixels; inside it a valid class"""
    Cn = ref.shape[1]
    want = ref.argmax(1)
    if Cn == 1:
        band = torch.zeros_like(want, dtype=torch.bool)
    else:
        top = ref.topk(2, dim=1).values
        band = (top[:, 0] - top[:, 1]) < BAND
    n_band = int(band.sum())
    print(f"{what}: {n_band} of {band.numel()} pixels in the band")
    assert n_band <= max(2, band.numel() // 100), (what, n_band, band.numel())
    assert torch.equal(pred.long()[~band], want[~band]), (what, int((pred.long() != want)[~band].sum()))
    assert bool((pred[band] < Cn).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_kernel_against_float64(i, dtype):
    from ppnet_amd import fused
    logits, mids, flips, out_hw, ref, e32 = case(i, dtype)
    Cn = ref.shape[1]
    dev = [x.cuda() for x in logits]
    runs = [raw(dev, mids, flips, out_hw, off) for off in range(4)]
    pred, prob = runs[0]
    for p, q in runs[1:]:                                                      # any alignment of pred, and reproducible bit for bit
        assert torch.equal(p, pred) and torch.equal(q.view(torch.int32), prob.view(torch.int32))
    check_labels(pred, ref, CASES[i][0])
    err, bound = float((prob.double() - ref).abs().max()), max(1e-6, 4 * e32)
    print(f"{CASES[i][0]} {dtype}: prob error {err:.3e}, float32 composition {e32:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, e32)
    assert torch.equal(prob.argmax(1), pred.long())                            # pred is the argmax of what prob holds
    only_prob = raw(dev, mids, flips, out_hw, want_pred=False)                 # pred NULL with prob
    assert only_prob[0] is None and torch.equal(only_prob[1].view(torch.int32), prob.view(torch.int32))
    if Cn <= fused.SEG_TTA_REG_CLASSES:                                        # prob NULL: the same pred
        for off in range(4):
            p, q = raw(dev, mids, flips, out_hw, off, want_prob=False)
            assert q is None and torch.equal(p, pred)
    # the wrapper: one launch per call, the same bits
    before = fused.TTA_CALLS["fwd"]
    wp, wq = fused.seg_tta(dev, mids, flips, out_hw, want_prob=True)
    assert fused.TTA_CALLS["fwd"] == before + 1
    assert wp.dtype == torch.uint8 and torch.equal(wp.cpu(), pred) and torch.equal(wq.cpu().view(torch.int32), prob.view(torch.int32))
    wp2, wq2 = fused.seg_tta(dev, mids, flips, out_hw)
    assert torch.equal(wp2.cpu(), pred) and ((wq2 is None) == (Cn <= fused.SEG_TTA_REG_CLASSES))
    assert fused.TTA_CALLS["fwd"] == before + 2


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("Cn", [2, 3, 19])
def test_one_identity_augmentation_is_seg_eval_bit_for_bit(Cn, dtype):
    from ppnet_amd import fused
    g = torch.Generator().manual_seed(7 + Cn)
    for (B, h, w, H, W) in ((2, 7, 5, 13, 9), (1, 9, 8, 33, 31), (3, 40, 24, 11, 31)):
        x = (torch.randn(B, Cn, h, w, generator=g) * 3).to(dtype).cuda()
        want = fused.seg_eval(x, torch.zeros(B, H, W, dtype=torch.uint8, device="cuda"), want_pred=True)[1]
        got = fused.seg_tta([x], [(H, W)], [None], (H, W))[0]
        assert torch.equal(got, want)


def test_equal_logits_give_class_0_and_a_nan_gives_class_0_where_it_reaches():
    from ppnet_amd import fused
    for Cn in (2, 8, 9, 19):
        ones = [torch.ones(2, Cn, 4, 3, device="cuda"), torch.full((2, Cn, 7, 5), -2.5, device="cuda")]
        pred, prob = fused.seg_tta(ones, [(13, 9), (6, 4)], [None, H_], (13, 9), want_prob=True)
        assert int(pred.max()) == 0 and torch.equal(prob, torch.full_like(prob, 1.0 / Cn))
    # a NaN in one augmentation's logits (one whose two resizes both interpolate): registers (C = 3) and the prob accumulator (C = 19)
    for name, a in (("13x9", 1), ("C19_16", 3)):
        logits, mids, flips, out_hw, ref, _ = case([c[0] for c in CASES].index(name), torch.float32)
        bad = [x.clone() for x in logits]
        bad[a][0, 0, 2, 1] = float("nan")
        hit = torch.isnan(ref64(bad, mids, flips, out_hw)).any(1)               # the pixels the NaN reaches
        assert 0 < int(hit[0].sum()) < hit[0].numel() and not bool(hit[1:].any())
        got = fused.seg_tta([x.cuda() for x in bad], mids, flips, out_hw)[0].cpu()
        clean = fused.seg_tta([x.cuda() for x in logits], mids, flips, out_hw)[0].cpu()
        assert int(got[hit].max()) == 0 and torch.equal(got[~hit], clean[~hit])
        check_labels(clean, ref, name)


def test_wrapper_refuses_what_the_kernel_does_not_take():
    from ppnet_amd import fused
    x = torch.randn(1, 2, 4, 4, device="cuda")
    before = fused.TTA_CALLS["fwd"]
    with pytest.raises(ValueError):
        fused.seg_tta([x] * 17, [(8, 8)] * 17, [None] * 17, (8, 8))
    with pytest.raises(ValueError):
        fused.seg_tta([x, x.to(torch.bfloat16)], [(8, 8)] * 2, [None] * 2, (8, 8))
    with pytest.raises(ValueError):
        fused.seg_tta([x, x], [(8, 8)] * 2, [None, "diagonal"], (8, 8))
    with pytest.raises(ValueError):
        fused.seg_tta([x, x[:, :1]], [(8, 8)] * 2, [None] * 2, (8, 8))
    with pytest.raises(ValueError):
        fused.seg_tta([x.half()], [(8, 8)], [None], (8, 8))
    assert fused.TTA_CALLS["fwd"] == before
    pred, prob = fused.seg_tta([x] * 16, [(8, 8)] * 16, [None] * 16, (8, 8))
    assert prob is None and tuple(pred.shape) == (1, 8, 8) and fused.TTA_CALLS["fwd"] == before + 1


def test_model_aug_test_is_one_launch_and_the_composition_of_its_own_logits(monkeypatch):
    """DiNAT + SETR-UP under the harness call with a 3-ratio + flip list: the wiring of sizes, flips and order, not the network."""
    from ppnet_amd import evaluate, fused, heads, train
    from ppnet_amd.augment import MultiScaleFlipAug
    from ppnet_amd.segnet import SegNet
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    m = SegNet(backbone=dict(embed_dim=32, mlp_ratio=2.0, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], kernel_size=7,
                             dilations=[[1, 2], [1, 2], [1, 2], [1, 1]], layer_scale=1e-5),
               decode_head=dict(in_channels=256, channels=32, num_convs=4, up_scale=2, num_classes=2)).to(dev).eval()
    x = torch.randn(4, 3, 64, 64, device=dev)
    aug = MultiScaleFlipAug((0.5, 1.0, 1.5))
    imgs, metas = aug(x)
    assert [tuple(i.shape[-2:]) for i in imgs] == [(32, 32)] * 2 + [(64, 64)] * 2 + [(96, 96)] * 2
    low = []
    hook = m.decode_head.register_forward_hook(lambda mod, inp, out: low.append(out.detach().cpu()))
    try:
        with torch.no_grad():
            before = fused.TTA_CALLS["fwd"]
            res = m(return_loss=False, img=imgs, img_metas=metas)
            assert fused.TTA_CALLS["fwd"] == before + 1
    finally:
        hook.remove()
    assert isinstance(res, list) and len(res) == 4 and all(r.dtype == np.int64 and r.shape == (64, 64) for r in res)
    got = torch.from_numpy(np.stack(res))
    assert len(low) == 6 and all(tuple(l.shape[:2]) == (4, 2) for l in low)
    ref = ref64(low, [tuple(i.shape[-2:]) for i in imgs], [H_ if ms[0]["flip"] else None for ms in metas], (64, 64))
    check_labels(got, ref, "model")
    with torch.no_grad():
        monkeypatch.setenv("PPNET_LIBRARY_TTA", "1")
        lib = torch.from_numpy(np.stack(m(return_loss=False, img=imgs, img_metas=metas)))
        monkeypatch.delenv("PPNET_LIBRARY_TTA")
        assert fused.TTA_CALLS["fwd"] == before + 1
        assert float((lib == got).float().mean()) > 0.995
        # the class-count gate is read at call time: from C = 2 the library composition, its labels; back to the kernel
        monkeypatch.setenv("PPNET_LIBRARY_TTA_FROM_C", "2")
        assert np.array_equal(np.stack(m(return_loss=False, img=imgs, img_metas=metas)), lib.numpy()) and fused.TTA_CALLS["fwd"] == before + 1
        monkeypatch.setenv("PPNET_LIBRARY_TTA_FROM_C", "257")
        assert np.array_equal(np.stack(m(return_loss=False, img=imgs, img_metas=metas)), got.numpy()) and fused.TTA_CALLS["fwd"] == before + 2
        monkeypatch.delenv("PPNET_LIBRARY_TTA_FROM_C")
        gt = torch.randint(0, 2, (4, 64, 64), device=dev).to(torch.uint8)
        gt[:, :3] = 255
        want = evaluate.total_area_to_metrics(heads.eval_areas(got.to(dev), gt, 2, 255), ("mIoU",))
        met = train.evaluate_segnet(m, x, gt, batch=4, aug=aug)
        assert fused.TTA_CALLS["fwd"] == before + 3
    assert met.keys() == want.keys() and all(np.array_equal(met[k], want[k], equal_nan=True) for k in met)
