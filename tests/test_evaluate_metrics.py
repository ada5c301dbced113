"""Segmentation metrics on the CPU: evaluate.total_area_to_metrics / summarize against hand-computed values (mmseg's formulas,
core/evaluation/metrics.py:333-395, datasets/custom.py:411-448), the library composition of heads.resized_eval_areas against a plain
per-pixel loop, SegNet.eval_areas against that composition of the model's own encode_decode output, and SegEvaluator's accumulation
in one process and over two gloo ranks."""
import math
import os
import socket
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from ppnet_amd import evaluate, heads


# ------------------------------------------------------------------------------------------------ metric values
#                        class 0  1  2      class 1 is absent from predictions and labels
AREAS = torch.tensor([[6, 0, 2],          # intersect
                      [8, 0, 4],          # prediction
                      [9, 0, 3]])         # label


def test_metric_values_by_hand():
    m = evaluate.total_area_to_metrics(AREAS, metrics=("mIoU", "mDice", "mFscore"))
    assert isinstance(m, OrderedDict) and list(m) == ["aAcc", "IoU", "Acc", "Dice", "Fscore", "Precision", "Recall"]
    assert all(isinstance(v, (np.ndarray, np.floating)) and np.asarray(v).dtype == np.float64 for v in m.values())
    assert float(m["aAcc"]) == 8 / 12                                              # sum intersect / sum label
    # union = prediction + label - intersect = 11, 0, 5
    assert m["IoU"][0] == 6 / 11 and math.isnan(m["IoU"][1]) and m["IoU"][2] == 2 / 5
    assert m["Acc"][0] == 6 / 9 and math.isnan(m["Acc"][1]) and m["Acc"][2] == 2 / 3
    assert m["Dice"][0] == 12 / 17 and math.isnan(m["Dice"][1]) and m["Dice"][2] == 4 / 7
    assert m["Precision"][0] == 6 / 8 and math.isnan(m["Precision"][1]) and m["Precision"][2] == 2 / 4
    assert m["Recall"][0] == 6 / 9 and m["Recall"][2] == 2 / 3
    # beta = 1: the F-score is the Dice coefficient, 2 P R / (P + R) = 2 I / (pred + label)
    for c in (0, 2):
        assert m["Fscore"][c] == pytest.approx(m["Dice"][c], rel=1e-15)
    assert math.isnan(m["Fscore"][1])
    # beta = 2: (1 + 4) P R / (4 P + R) = 5 I / (4 label + pred)
    m2 = evaluate.total_area_to_metrics(AREAS, metrics="mFscore", beta=2)
    assert list(m2) == ["aAcc", "Fscore", "Precision", "Recall"]
    assert m2["Fscore"][0] == pytest.approx(5 * 6 / (4 * 9 + 8), rel=1e-15) and m2["Fscore"][2] == pytest.approx(5 * 2 / (4 * 3 + 4), rel=1e-15)
    # the default is mIoU alone; arrays and lists are taken too
    d = evaluate.total_area_to_metrics(AREAS.numpy())
    assert list(d) == ["aAcc", "IoU", "Acc"] and np.array_equal(d["IoU"], m["IoU"], equal_nan=True)


def test_nan_to_num_summarize_and_unknown_metric():
    m = evaluate.total_area_to_metrics(AREAS, metrics=("mIoU",))
    s = evaluate.summarize(m)
    assert list(s) == ["aAcc", "mIoU", "mAcc"] and all(isinstance(v, float) for v in s.values())
    assert s["aAcc"] == 8 / 12
    assert s["mIoU"] == pytest.approx((6 / 11 + 2 / 5) / 2, rel=1e-15)            # nanmean: the absent class does not count
    assert s["mAcc"] == pytest.approx((6 / 9 + 2 / 3) / 2, rel=1e-15)
    z = evaluate.total_area_to_metrics(AREAS, metrics=("mIoU",), nan_to_num=0)
    assert z["IoU"][1] == 0.0 and z["Acc"][1] == 0.0 and z["IoU"][0] == 6 / 11
    assert evaluate.summarize(z)["mIoU"] == pytest.approx((6 / 11 + 2 / 5) / 3, rel=1e-15)
    m9 = evaluate.total_area_to_metrics(AREAS, metrics=("mDice",), nan_to_num=-9)
    assert m9["Dice"][1] == -9.0
    with pytest.raises(KeyError):
        evaluate.total_area_to_metrics(AREAS, metrics=("mIoU", "mAP"))
    with pytest.raises(KeyError):
        evaluate.total_area_to_metrics(AREAS, metrics="IoU")
    # nothing valid at all: 0 / 0 everywhere, as in the reference
    e = evaluate.total_area_to_metrics(torch.zeros(3, 2, dtype=torch.int64))
    assert math.isnan(float(e["aAcc"])) and np.isnan(e["IoU"]).all() and math.isnan(evaluate.summarize(e)["mIoU"])


# ------------------------------------------------------------------------------------------------ the library composition
def _loop_areas(logit, gt, ignore_index):
    """A plain per-pixel loop over the float32 interpolation: the definition."""
    B, Cc = logit.shape[:2]
    H, W = gt.shape[-2:]
    z = F.interpolate(logit.float(), (H, W), mode="bilinear", align_corners=False)
    areas = [[0] * Cc for _ in range(3)]
    for b in range(B):
        for y in range(H):
            for x in range(W):
                lab = int(gt[b, y, x])
                if lab == ignore_index or lab < 0 or lab >= Cc:
                    continue
                best = max(range(Cc), key=lambda c: (float(z[b, c, y, x]), -c))    # ties to the lowest class
                areas[1][best] += 1
                areas[2][lab] += 1
                if best == lab:
                    areas[0][lab] += 1
    return torch.tensor(areas)


def _mixed_case():
    g = torch.Generator().manual_seed(7)
    logit = torch.randn(2, 3, 3, 5, generator=g) * 3
    gt = torch.randint(0, 3, (2, 6, 10), generator=g)
    gt[torch.rand(2, 6, 10, generator=g) < 0.2] = 255
    gt[0, 0, :3] = torch.tensor([7, 3, 254])                                       # out of range, not ignore_index
    gt[1, 5, 7:] = torch.tensor([-1, -100, 1 << 40])
    return logit, gt


def test_library_composition_equals_a_plain_loop():
    logit, gt = _mixed_case()
    got = heads.resized_eval_areas(logit, gt)
    want = _loop_areas(logit, gt, 255)
    assert got.dtype == torch.int64 and got.shape == (3, 3) and torch.equal(got, want)
    assert int(want[2].sum()) == int(((gt >= 0) & (gt < 3)).sum()) == int(want[1].sum()) and int(want[0].sum()) > 0
    # the out-of-range labels count like ignored ones
    ign = gt.clone()
    ign[(gt < 0) | (gt >= 3)] = 255
    assert torch.equal(heads.resized_eval_areas(logit, ign), got)
    # another ignore_index: 255 is then one more out-of-range label
    m100 = gt.clone()
    m100[gt == 255] = -100
    assert torch.equal(heads.resized_eval_areas(logit, m100, ignore_index=-100), got)
    assert torch.equal(heads.resized_eval_areas(logit, gt, ignore_index=-100), got)
    # uint8 labels (those that fit) and bfloat16 logits are taken as they are
    g8 = ign.to(torch.uint8)
    assert torch.equal(heads.resized_eval_areas(logit, g8), got)
    lb = logit.to(torch.bfloat16)
    assert torch.equal(heads.resized_eval_areas(lb, g8), _loop_areas(lb.float(), ign, 255))
    # align_corners=True is the library's own rule
    zt = F.interpolate(logit, (6, 10), mode="bilinear", align_corners=True).argmax(1)
    assert torch.equal(heads.resized_eval_areas(logit, gt, align_corners=True), heads.eval_areas(zt, gt, 3))
    # equal logits: every pixel predicts class 0
    flat = heads.resized_eval_areas(torch.ones(2, 3, 3, 5), gt)
    assert int(flat[1, 0]) == int(want[2].sum()) and int(flat[1, 1:].sum()) == 0 and torch.equal(flat[2], want[2])


# ------------------------------------------------------------------------------------------------ model level
TINY = dict(backbone=dict(type="SwinTransformer", embed_dims=32, depths=(2, 2, 2, 2), num_heads=(1, 2, 4, 8), drop_path_rate=0.0),
            decode_head=dict(type="UPerPUPHead", in_channels=[32, 64, 128, 256], channels=16, num_convs=(1, 2, 3, 4), num_classes=3))


@pytest.fixture(scope="module")
def tiny():
    from ppnet_amd.segnet import SegNet, randomize_neutral_parameters
    torch.manual_seed(0)
    net = randomize_neutral_parameters(SegNet.from_config(TINY), seed=1).eval()
    g = torch.Generator().manual_seed(2)
    img = torch.randn(4, 3, 64, 64, generator=g)
    gt = torch.randint(0, 3, (4, 1, 64, 64), generator=g).to(torch.uint8)
    gt[:, :, :5] = 255
    return net, img, gt


def test_model_eval_areas_is_the_composition_of_its_encode_decode(tiny, monkeypatch):
    net, img, gt = tiny
    with torch.no_grad():
        logits = net.encode_decode(img)
    want = heads.eval_areas(logits.float().argmax(1), gt.squeeze(1), 3)
    got = net.eval_areas(img, gt)
    assert got.dtype == torch.int64 and got.shape == (3, 3) and not got.requires_grad and torch.equal(got, want)
    assert int(want[2].sum()) == 4 * 59 * 64 and 0 < int(want[0].sum()) < int(want[2].sum())
    assert torch.equal(net.eval_areas(img, gt.squeeze(1).long()), want)            # [B,H,W] int64 labels
    monkeypatch.setenv("PPNET_LIBRARY_EVAL", "1")
    assert torch.equal(net.eval_areas(img, gt), want)
    monkeypatch.delenv("PPNET_LIBRARY_EVAL")
    assert net.training is False
    # labels of another size: encode_decode's resize to the input size, then the resize to the labels
    small = gt[:, :, ::2, ::2].contiguous()
    two_step = F.interpolate(logits.float(), (32, 32), mode="bilinear", align_corners=False).argmax(1)
    assert torch.equal(net.eval_areas(img, small), heads.eval_areas(two_step, small.squeeze(1), 3))


def test_evaluate_segnet_on_cpu_images(tiny):
    from ppnet_amd import train
    net, img, gt = tiny
    net.train()
    try:
        m = train.evaluate_segnet(net, img, gt.squeeze(1), batch=3, metrics=("mIoU", "mFscore"))
        assert net.training                                                        # the training flag comes back
    finally:
        net.eval()
    want = evaluate.total_area_to_metrics(net.eval_areas(img, gt), ("mIoU", "mFscore"))
    assert list(m) == list(want)
    for k in m:
        assert np.array_equal(m[k], want[k], equal_nan=True), k


# ------------------------------------------------------------------------------------------------ SegEvaluator
def test_evaluator_two_updates_equal_one_on_the_concatenated_batch(tiny):
    net, img, gt = tiny
    whole = evaluate.SegEvaluator(3)
    whole.update(net, img, gt)
    parts = evaluate.SegEvaluator(3)
    first = parts.update(net, img[:1], gt[:1])
    parts.update(net, img[1:], gt[1:])
    assert torch.equal(parts.areas, whole.areas) and not torch.equal(first, whole.areas)
    assert torch.equal(first, net.eval_areas(img[:1], gt[:1]))                     # update returns the batch's own areas, unaccumulated
    a, b = whole.compute(("mIoU", "mDice")), parts.compute(("mIoU", "mDice"))
    assert list(a) == list(b) == ["aAcc", "IoU", "Acc", "Dice"] and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
    # logits instead of a model, at any resolution
    logit, lab = _mixed_case()
    ev = evaluate.SegEvaluator(3)
    ev.update(logit[:1], None, lab[:1])
    ev.update(logit[1:], None, lab[1:].unsqueeze(1))
    assert torch.equal(ev.areas, heads.resized_eval_areas(logit, lab))
    assert ev.all_reduce() is ev and torch.equal(ev.areas, heads.resized_eval_areas(logit, lab))      # no process group: unchanged
    with pytest.raises(ValueError):
        evaluate.SegEvaluator(4).update(logit, None, lab)
    with pytest.raises(RuntimeError):
        evaluate.SegEvaluator(3).compute()


def _rank(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    logit, lab = _mixed_case()
    ev = evaluate.SegEvaluator(3)
    ev.update(logit[rank:rank + 1], None, lab[rank:rank + 1])
    own = ev.areas.clone()
    ev.all_reduce()
    torch.save({"own": own, "total": ev.areas, "mIoU": evaluate.summarize(ev.compute())["mIoU"]}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_report_the_single_process_totals(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_rank, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"rank{r}.pt") for r in (0, 1))
    logit, lab = _mixed_case()
    want = heads.resized_eval_areas(logit, lab)
    assert torch.equal(r0["total"], want) and torch.equal(r1["total"], want)
    assert torch.equal(r0["own"] + r1["own"], want) and not torch.equal(r0["own"], want)
    assert r0["mIoU"] == r1["mIoU"] == evaluate.summarize(evaluate.total_area_to_metrics(want))["mIoU"]
