"""CPU-side checks of the test-time augmentation merge (ppn_seg_tta, csrc/seg_tta.hip) and the layers above it: header, library and
bindings carry the entry point at ABI 111; every bad argument is refused with PPN_E_INVALID before any HIP call (the pointers below are
never dereferenced); the source is built, uses resize_tap.h's functions and no scratch; the host constants are the kernel's;
augment.MultiScaleFlipAug gives mmseg's list; and on the CPU SegNet's aug_test, the evaluation with `aug` and heads.tta_mean_prob are
one definition."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ppnet_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
E_INVALID = -1
ONE = 0x1000                                                   # 16-byte aligned, never dereferenced on these paths
ARGS = ["augs", "n_augs", "pred", "prob", "B", "C", "H", "W", "logit_dtype", "stream"]
FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fno-slp-vectorize --cuda-device-only -S".split()


def _args(decl):
    code = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    return [a.split()[-1].lstrip("*") for a in code.split(",")]


def test_header_library_and_bindings_carry_the_entry_point_at_abi_111():
    from ppnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "ppnet_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert int(re.search(r"#define\s+PPN_ABI_VERSION\s+(\d+)", header).group(1)) == 111
    assert _lib.ABI_VERSION == 111 and _lib.lib.ppn_version() == 111
    assert "ppn_seg_tta" in _lib.EXPORTS and hasattr(_lib.lib, "ppn_seg_tta")
    assert "ppn_seg_tta" in re.search(r"/\* ABI version of this header.*?\*/", header, re.S).group(0)
    assert _args(re.search(r"int\s+ppn_seg_tta\s*\((.*?)\)\s*;", code, re.S).group(1)) == ARGS
    assert len(_lib.lib.ppn_seg_tta.argtypes) == len(ARGS) == 10 and _lib.lib.ppn_seg_tta.restype is C.c_int
    capi = open(os.path.join(CSRC, "capi.hip")).read()
    assert _args(re.search(r"\bppn_seg_tta\s*\((.*?)\)\s*\{", capi, re.S).group(1)) == ARGS
    assert re.search(r"\bint\s+seg_tta_launch\s*\(", open(os.path.join(CSRC, "ppn_kernels.h")).read())
    # the struct of the header is the struct of the bindings: pointer, five int32, padded to 32 bytes
    fields = re.search(r"typedef struct ppn_tta_aug \{(.*?)\} ppn_tta_aug;", code, re.S).group(1)
    names = [part.split()[-1].lstrip("*") for decl in fields.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f[0] for f in _lib.TtaAug._fields_] == ["logit", "h", "w", "hm", "wm", "flip"] and C.sizeof(_lib.TtaAug) == 32


def _augs(n=2, **kw):
    from ppnet_amd import _lib
    a = (_lib.TtaAug * max(n, 1))()
    for g in a:
        g.logit, g.h, g.w, g.hm, g.wm, g.flip = ONE, 8, 6, 16, 12, 0
    for k, v in kw.items():
        setattr(a[max(n, 1) - 1], k, v)                        # the LAST entry is the bad one: every entry is checked
    return a


@pytest.mark.parametrize("dtype", [0, 1])
def test_rejects_bad_arguments_without_gpu(dtype):
    from ppnet_amd import _lib
    f = _lib.lib.ppn_seg_tta
    p = C.c_void_p(ONE)

    def call(augs=None, n=2, pred=p, prob=p, B=2, Cc=3, H=32, W=24, dt=dtype):
        return f(_augs(n) if augs is None else augs, n, pred, prob, B, Cc, H, W, dt, None)
    assert f(None, 2, p, p, 2, 3, 32, 24, dtype, None) == E_INVALID                        # NULL augs
    for n in (0, -1, 17, 1 << 20):
        assert call(augs=_augs(16), n=n) == E_INVALID, n
    assert call(augs=_augs(2, logit=None)) == E_INVALID
    for off in (8, 4, 2, 1):
        assert call(augs=_augs(2, logit=ONE + off)) == E_INVALID, off
    assert call(augs=_augs(16, logit=ONE + 8), n=16) == E_INVALID                          # the sixteenth entry is read too
    for field in ("h", "w", "hm", "wm"):
        for v in (0, -1):
            assert call(augs=_augs(2, **{field: v})) == E_INVALID, (field, v)
    for v in (3, -1, 255):
        assert call(augs=_augs(2, flip=v)) == E_INVALID, v
    for name in ("B", "Cc", "H", "W"):
        for v in (0, -1):
            assert call(**{name: v}) == E_INVALID, (name, v)
    assert call(Cc=257) == E_INVALID and call(Cc=2 ** 31 - 1) == E_INVALID                # C > 256
    assert call(Cc=9, prob=None) == E_INVALID and call(Cc=256, prob=None) == E_INVALID    # C > 8 accumulates in prob
    assert call(pred=None, prob=None) == E_INVALID and call(Cc=8, pred=None, prob=None) == E_INVALID
    assert call(B=1, Cc=1, H=1 << 16, W=1 << 15) == E_INVALID                             # B H W = 2^31
    assert call(B=1 << 11, Cc=1, H=1 << 10, W=1 << 10) == E_INVALID
    assert call(B=2 ** 31 - 1, Cc=1, H=2 ** 31 - 1, W=2 ** 31 - 1) == E_INVALID
    assert call(B=1, Cc=256, H=1 << 12, W=1 << 11) == E_INVALID                           # B C H W = 2^31
    assert call(B=8, Cc=4, H=1 << 13, W=1 << 13) == E_INVALID
    assert call(B=1, Cc=256, augs=_augs(2, h=1 << 12, w=1 << 11)) == E_INVALID             # B C h w = 2^31
    assert call(B=1 << 11, Cc=4, H=8, W=8, augs=_augs(2, h=1 << 9, w=1 << 9)) == E_INVALID
    assert call(augs=_augs(2, h=2 ** 31 - 1, w=2 ** 31 - 1)) == E_INVALID
    for dt in (2, -1):
        assert call(dt=dt) == E_INVALID, dt


def test_host_constants():
    from ppnet_amd import fused
    header = open(os.path.join(ROOT, "include", "ppnet_hip.h")).read()
    assert int(re.search(r"#define\s+PPN_SEG_TTA_MAX_AUGS\s+(\d+)", header).group(1)) == fused.SEG_TTA_MAX_AUGS == 16
    assert int(re.search(r"#define\s+PPN_SEG_TTA_REG_CLASSES\s+(\d+)", header).group(1)) == fused.SEG_TTA_REG_CLASSES == 8
    src = open(os.path.join(CSRC, "seg_tta.hip")).read()
    const = {k: v for k, v in re.findall(r"constexpr int (ST_\w+) = ([^;]+);", src)}
    assert int(const["ST_THREADS"]) == fused.SEG_TTA_THREADS == 256
    assert const["ST_PX"] == "ST_THREADS * ST_PER_THREAD" and int(const["ST_PER_THREAD"]) * 256 == fused.SEG_TTA_PIXELS == 1024
    assert const["ST_MAX_AUGS"] == "PPN_SEG_TTA_MAX_AUGS" and const["ST_REG_C"] == "PPN_SEG_TTA_REG_CLASSES"
    assert int(const["ST_MAX_C"]) == fused.SEG_TTA_MAX_CLASSES == 256 and int(const["ST_LDS_C"]) == fused.SEG_TTA_LDS_CLASSES == 64
    assert 4 * fused.SEG_TTA_LDS_CLASSES * fused.SEG_TTA_THREADS <= 64 * 1024         # the LDS a launch may ask for without an attribute
    assert fused.TTA_CALLS.keys() == {"fwd"}
    from ppnet_amd import segnet
    assert segnet.LIBRARY_TTA_FROM_C == fused.SEG_TTA_LDS_CLASSES + 1     # aug_test's default: the kernel where a pixel's logits fit LDS


def test_seg_tta_source_is_built_shares_the_taps_and_uses_no_scratch(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not present")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "seg_tta.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    for fl in FLAGS[:-2]:
        assert fl.replace("gfx950", "$(ARCH)") in mk, fl                            # the Makefile's own flags
    out = tmp_path / "seg_tta.s"
    subprocess.run([HIPCC, *FLAGS, os.path.join(CSRC, "seg_tta.hip"), "-o", str(out)], check=True, cwd=CSRC, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    scratch = dict(re.findall(r"\.amdhsa_kernel (\S+).*?; ScratchSize: (\d+)", out.read_text(), re.S))
    # per logit type: one register kernel per class count 1 .. 8, and the kernel that accumulates in prob with and without LDS
    assert len(scratch) == 20 and sum("seg_tta_reg_kernel" in k for k in scratch) == 16 and sum("seg_tta_acc_kernel" in k for k in scratch) == 4
    assert all(int(v) == 0 for v in scratch.values()), scratch
    text = open(os.path.join(CSRC, "seg_tta.hip")).read()
    assert '#include "resize_tap.h"' in text and "bilinear_tap(int" not in text and not re.search(r"\bfloat\s+(interp|ldf)\s*\(", text)


def test_seg_tta_refuses_cpu_tensors():
    torch = pytest.importorskip("torch")
    from ppnet_amd import fused
    lg = [torch.randn(1, 2, 4, 4), torch.randn(1, 2, 6, 6)]
    assert not fused.seg_tta_ok(lg, [(8, 8), (12, 12)], [None, "horizontal"], (8, 8))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        fused.seg_tta(lg, [(8, 8), (12, 12)], [None, "horizontal"], (8, 8))


def test_multi_scale_flip_aug_on_cpu():
    torch = pytest.importorskip("torch")
    import torch.nn.functional as F
    from ppnet_amd.augment import MultiScaleFlipAug
    torch.manual_seed(0)
    x = torch.randn(2, 3, 64, 64)
    imgs, metas = MultiScaleFlipAug()(x)
    ratios = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)
    assert len(imgs) == len(metas) == 12 == len(MultiScaleFlipAug())
    for i, (im, ms) in enumerate(zip(imgs, metas)):
        s = int(64 * ratios[i // 2])                                               # scale-major, unflipped before flipped
        assert tuple(im.shape) == (2, 3, s, s) and len(ms) == 2
        for m in ms:
            assert m["ori_shape"] == (64, 64, 3) and m["img_shape"] == m["pad_shape"] == (s, s, 3)
            assert m["flip"] == bool(i % 2) and m["flip_direction"] == "horizontal"
            assert m["scale_factor"].dtype == np.float32 and np.array_equal(m["scale_factor"], np.full(4, s / 64, dtype=np.float32))
        if i % 2 == 0:
            want = x if s == 64 else F.interpolate(x, (s, s), mode="bilinear", align_corners=False)
            assert torch.equal(im, want)
        else:
            assert torch.equal(im, imgs[i - 1].flip(3))
    # odd sizes truncate (test_time_aug.py:73-75), both directions: unflipped, then flipped, per direction
    imgs, metas = MultiScaleFlipAug((0.75, 1.3), flip_direction=["horizontal", "vertical"])(torch.randn(1, 3, 13, 9))
    assert [tuple(i.shape[-2:]) for i in imgs] == [(9, 6)] * 4 + [(16, 11)] * 4
    assert [(m[0]["flip"], m[0]["flip_direction"]) for m in metas[:4]] == [(False, "horizontal"), (False, "vertical"), (True, "horizontal"),
                                                                            (True, "vertical")]
    assert torch.equal(imgs[2], imgs[0].flip(3)) and torch.equal(imgs[3], imgs[1].flip(2)) and torch.equal(imgs[0], imgs[1])
    assert len(MultiScaleFlipAug((1.0, 2.0), flip=False)(x)[0]) == 2
    # the planning_seg test pipeline has no Resize: equal sizes, plain flip averaging
    imgs, metas = MultiScaleFlipAug(resize=False)(x)
    assert len(imgs) == 12 and all(tuple(i.shape) == (2, 3, 64, 64) for i in imgs)
    assert all(torch.equal(imgs[i], x if i % 2 == 0 else x.flip(3)) for i in range(12))
    assert all(m[0]["img_shape"] == (64, 64, 3) and m[0]["flip"] == bool(i % 2) for i, m in enumerate(metas))


# The DiNAT + SETR-UP of tests/test_segnet.py does not run on the CPU without autograd (its tokenizer's LayerNorm is a kernel); the Swin +
# UPerPUP of tests/test_evaluate_metrics.py does, through the real encode_decode.
TINY = dict(backbone=dict(type="SwinTransformer", embed_dims=32, depths=(2, 2, 2, 2), num_heads=(1, 2, 4, 8), drop_path_rate=0.0),
            decode_head=dict(type="UPerPUPHead", in_channels=[32, 64, 128, 256], channels=16, num_convs=(1, 2, 3, 4), num_classes=3))
CLASSES = 3


def _tiny_segnet():
    import torch
    from ppnet_amd.segnet import SegNet, randomize_neutral_parameters
    torch.manual_seed(1)
    m = randomize_neutral_parameters(SegNet.from_config(TINY), seed=2).eval()
    with torch.no_grad():                                      # an untrained head labels every pixel alike: level the classes' means
        m.decode_head.conv_seg.bias -= m.encode_decode(torch.randn(2, 3, 64, 64)).mean((0, 2, 3))
    return m


def test_cpu_aug_test_is_the_reference_composition_and_tta_mean_prob():
    torch = pytest.importorskip("torch")
    import torch.nn.functional as F
    from ppnet_amd import fused, heads
    from ppnet_amd.augment import MultiScaleFlipAug
    m = _tiny_segnet()
    torch.manual_seed(3)
    x = torch.randn(2, 3, 64, 64)
    imgs, metas = MultiScaleFlipAug((0.5, 1.0, 1.5))(x)
    assert len(imgs) == 6
    before = dict(fused.TTA_CALLS)
    with torch.no_grad():
        got = np.stack(m(return_loss=False, img=imgs, img_metas=metas))
        assert got.dtype == np.int64 and got.shape == (2, 64, 64)
        # the hand-written composition of encoder_decoder.py:200-285
        total = 0
        for im, ms in zip(imgs, metas):
            lg = F.interpolate(m.decode_head(m.backbone(im)), im.shape[-2:], mode="bilinear", align_corners=False)
            if tuple(lg.shape[-2:]) != (64, 64):
                lg = F.interpolate(lg, (64, 64), mode="bilinear", align_corners=False)
            p = F.softmax(lg, dim=1)
            total = total + (p.flip(3) if ms[0]["flip"] else p)
        want = (total / len(imgs)).argmax(1).numpy()
        assert len(np.unique(want)) > 1, "a one-class prediction tests nothing"
        assert np.array_equal(got, want)
        low = [m.decode_head(m.backbone(im)) for im in imgs]
        mean = heads.tta_mean_prob(low, [tuple(im.shape[-2:]) for im in imgs], ["horizontal" if ms[0]["flip"] else None for ms in metas],
                                   (64, 64))
        assert mean.dtype == torch.float32 and tuple(mean.shape) == (2, CLASSES, 64, 64)
        assert np.array_equal(got, mean.argmax(1).numpy())
        assert torch.allclose(mean.sum(1), torch.ones(2, 64, 64), atol=1e-6)
    assert fused.TTA_CALLS == before
    # a vertical flip un-flips along H; float64 logits stay float64
    p = heads.tta_mean_prob([torch.randn(1, 3, 4, 5, dtype=torch.float64)], [(8, 10)], ["vertical"], (7, 9))
    assert p.dtype == torch.float64 and tuple(p.shape) == (1, 3, 7, 9)
    z = torch.randn(1, 3, 4, 5)
    a = heads.tta_mean_prob([z], [(8, 10)], ["vertical"], (7, 9))
    b = F.softmax(F.interpolate(F.interpolate(z, (8, 10), mode="bilinear"), (7, 9), mode="bilinear"), 1).flip(2)
    assert torch.equal(a, b)
    with pytest.raises(ValueError):
        heads.tta_mean_prob([z], [(8, 10)], ["diagonal"], (7, 9))


def test_cpu_evaluate_segnet_with_aug_scores_the_merged_labels():
    torch = pytest.importorskip("torch")
    from ppnet_amd import evaluate, heads, train
    from ppnet_amd.augment import MultiScaleFlipAug
    m = _tiny_segnet()
    torch.manual_seed(4)
    x = torch.randn(3, 3, 64, 64)
    gt = torch.randint(0, CLASSES, (3, 64, 64), dtype=torch.uint8)
    gt[:, :4] = 255
    aug = MultiScaleFlipAug((0.5, 1.0, 1.5))
    with torch.no_grad():
        labels = torch.cat([torch.from_numpy(np.stack(m(return_loss=False, img=list(i), img_metas=list(ms))))
                            for i, ms in (aug(x[:2]), aug(x[2:]))])
    want = evaluate.total_area_to_metrics(heads.eval_areas(labels, gt, CLASSES, 255), ("mIoU",))
    got = train.evaluate_segnet(m, x, gt, batch=2, aug=aug)
    assert got.keys() == want.keys() and all(np.array_equal(got[k], want[k], equal_nan=True) for k in got)
    assert not m.training
    plain = train.evaluate_segnet(m, x, gt, batch=2)
    assert plain.keys() == got.keys()                                              # aug=None is the path it always was
    areas = m.eval_areas(x, gt, aug=aug)
    assert torch.equal(areas, heads.eval_areas(labels, gt, CLASSES, 255))
    ev = evaluate.SegEvaluator(CLASSES)
    ev.update(m, x, gt, aug=aug)
    assert torch.equal(ev.areas, areas)
    with pytest.raises(ValueError):
        m.eval_areas(x, gt[:, :32], aug=aug)
