"""Success-rate / path-length evaluation of batched plans (BASELINE config 5's PPNet column).

Reference: EDaGe-PP/process_map.py:452-506 (extract_path_image: a problem is solved when extract_path succeeds and no
consecutive-waypoint segment collides; the solution's cost is the polyline length) and the OMPL harness's stopping rule
experiments/ompl_experiments/updated_geometric_planner.py:260-277,349-354 (a planner is done once its best cost is within
(1 + epsilon) of the target path's length).  Everything here runs on the device batch `PPNet.plan` returned; nothing is
read back per problem.

Segmentation metrics: SegNet/mmseg/core/evaluation/metrics.py:333-395 (total_area_to_metrics: aAcc, IoU / Acc, Dice, Fscore /
Precision / Recall from the per-class intersect / prediction / label areas summed over a dataset) and mmseg/datasets/custom.py:411-448
(the mIoU / mAcc / ... summary: the nan-mean over the classes).  The areas come from SegNet.eval_areas / heads.resized_eval_areas — on
the GPU one kernel per batch (ppn_seg_eval) — and stay on the device until compute().
"""
from collections import OrderedDict

import numpy as np
import torch

from . import edage, heads


def plan_lengths(waypoints, counts):
    """Polyline length of each plan: waypoints [B,M,2] (row, col), counts [B] valid points (0 = no plan) -> [B] f64."""
    M = waypoints.shape[1]
    seg = (waypoints[:, 1:] - waypoints[:, :-1]).pow(2).sum(dim=2).sqrt()
    valid = torch.arange(M - 1, device=waypoints.device)[None, :] < (counts[:, None].to(torch.int64) - 1)
    return (seg * valid).sum(dim=1)


def evaluate_plans(result, target_length_px, epsilon=0.1):
    """result: the dict of PPNet.plan / plan_tail; target_length_px [B]: the target path's Length in pixels
    (Path.Length * R / map_size).  Returns a dict of Python floats:
      extract_ok     fraction with a waypoint chain reaching the goal            (process_map.py:486-490)
      collision_free fraction of those whose segments all pass the circle test   (:491-495)
      success        fraction solved = ok and no collision                       (:496-503)
      length_ratio   mean (plan length / target length) over solved problems
      within_eps     fraction of ALL problems solved with length <= (1+epsilon) * target  (the harness's criterion)"""
    ok, coll = result["ok"], result["collision"]
    succ = ok & ~coll
    length = plan_lengths(result["waypoints"], result["counts"])
    ratio = length / target_length_px.to(length.dtype)
    n_ok = int(ok.sum())
    n_s = int(succ.sum())
    B = ok.numel()
    return {"extract_ok": n_ok / B, "collision_free": (int((ok & ~coll).sum()) / n_ok) if n_ok else 0.0,
            "success": n_s / B, "length_ratio": float(ratio[succ].mean()) if n_s else None,
            "within_eps": int((succ & (ratio <= 1.0 + epsilon)).sum()) / B, "epsilon": epsilon, "problems": B}


def label_heatmaps(paths, maps, placements, sigma=2.0, bound=None):
    """8-bit heat maps [n,R,R] with a ridge along each map's label path: GenNet's training target (mask_path,
    process_map.py:148-163, every 5th label point) blurred with a Gaussian and min-max normalised per sample as
    predict.py:95-102 does — what a trained GenNet is fitted to produce (GenNet/train.py: MSE against mask_path).
    No trained weights ship with the reference; these maps let the planner tail be exercised on plans that exist."""
    mask_path, _ = edage.label_masks(paths, maps, placements, bound=bound, want_path=True, want_space=False)
    x = (mask_path > 0).to(torch.float32).unsqueeze(1)
    r = max(1, int(3 * sigma + 0.5))
    t = torch.arange(-r, r + 1, device=x.device, dtype=torch.float32)
    k = torch.exp(-t * t / (2 * sigma * sigma))
    k = k / k.sum()
    # separable blur as sums of shifted slices (no library convolution: PPNet switches MIOpen's exhaustive search on, and a
    # search over these one-off 1 x (2r+1) shapes can take minutes)
    H, W = x.shape[-2:]
    xp = torch.nn.functional.pad(x, (r, r, 0, 0))
    x = sum(k[i] * xp[..., :, i:i + W] for i in range(2 * r + 1))
    xp = torch.nn.functional.pad(x, (0, 0, r, r))
    x = sum(k[i] * xp[..., i:i + H, :] for i in range(2 * r + 1))
    from .gennet import normalize_heatmap_u8
    return normalize_heatmap_u8(x)


# ---------------------------------------------------------------- segmentation metrics from area histograms
SEG_METRICS = ("mIoU", "mDice", "mFscore")


def total_area_to_metrics(areas, metrics=("mIoU",), nan_to_num=None, beta=1):
    """mmseg's total_area_to_metrics (metrics.py:333-395) from areas [3, C] (intersect | prediction | label; a tensor on any device,
    or an array): an OrderedDict of numpy float64 values — 'aAcc' (a scalar: sum intersect / sum label) and per class [C], for
    'mIoU': 'IoU' = intersect / union with union = prediction + label - intersect, 'Acc' = intersect / label; for 'mDice': 'Dice' =
    2 intersect / (prediction + label), 'Acc'; for 'mFscore': 'Fscore' = (1 + beta^2) P R / (beta^2 P + R), 'Precision' = intersect /
    prediction, 'Recall' = intersect / label.  0 / 0 is NaN as in the reference (a class absent from predictions and labels);
    nan_to_num replaces NaN.  An unknown metric raises KeyError."""
    if isinstance(metrics, str):
        metrics = [metrics]
    if not set(metrics).issubset(SEG_METRICS):
        raise KeyError("metrics {} is not supported".format(list(metrics)))
    a = areas.detach().cpu().numpy() if isinstance(areas, torch.Tensor) else np.asarray(areas)
    if a.ndim != 2 or a.shape[0] != 3:
        raise ValueError(f"areas must be [3, C] (intersect | prediction | label), got {a.shape}")
    inter, pred, label = a.astype(np.float64)
    ret = OrderedDict()
    with np.errstate(divide="ignore", invalid="ignore"):
        ret["aAcc"] = np.float64(inter.sum()) / np.float64(label.sum())
        for metric in metrics:
            if metric == "mIoU":
                ret["IoU"] = inter / (pred + label - inter)
                ret["Acc"] = inter / label
            elif metric == "mDice":
                ret["Dice"] = 2 * inter / (pred + label)
                ret["Acc"] = inter / label
            else:
                precision, recall = inter / pred, inter / label
                ret["Fscore"] = (1 + beta ** 2) * (precision * recall) / ((beta ** 2 * precision) + recall)
                ret["Precision"] = precision
                ret["Recall"] = recall
    if nan_to_num is not None:
        ret = OrderedDict((k, np.nan_to_num(v, nan=nan_to_num)) for k, v in ret.items())
    return ret


def summarize(metrics):
    """The summary mmseg's CustomDataset.evaluate reports (custom.py:411-448) as fractions: 'aAcc' as it is, and for every per-class
    entry 'm' + key (mIoU, mAcc, mDice, mFscore, mPrecision, mRecall) = the nan-mean over the classes (a class without pixels does not
    count).  Python floats."""
    out = OrderedDict()
    for k, v in metrics.items():
        v = np.asarray(v, dtype=np.float64)
        out[k if k == "aAcc" else "m" + k] = float(v) if k == "aAcc" else (float(np.nanmean(v)) if not np.isnan(v).all() else float("nan"))
    return out


class SegEvaluator:
    """Sums the area histograms of an evaluation over batches (and ranks) on the device; nothing is read back before compute().

        ev = SegEvaluator(num_classes=2)
        for img, gt in loader: ev.update(segnet, img, gt)        # or ev.update(lowres_logits, None, gt)
        ev.all_reduce()                                          # under an initialised process group
        m = ev.compute(("mIoU", "mFscore")); summarize(m)["mIoU"]"""

    def __init__(self, num_classes, ignore_index=255):
        self.num_classes, self.ignore_index = int(num_classes), int(ignore_index)
        self.areas = None                                        # int64 [3, C] on the device of the first update

    def update(self, model_or_logits, img, gt, aug=None):
        """model_or_logits: a SegNet (img its input batch) or a head's logits [B,C,h,w] at any resolution (img None); gt the labels
        [B,H,W] / [B,1,H,W].  aug (a SegNet only): an augment.MultiScaleFlipAug — the prediction is the test-time augmentation's merge
        (SegNet.eval_areas).  Returns this batch's areas (on the device, not synchronised)."""
        if isinstance(model_or_logits, torch.Tensor):
            if aug is not None:
                raise ValueError("SegEvaluator.update: test-time augmentation needs the model, not its logits")
            g = gt.squeeze(1) if gt.dim() == 4 else gt
            a = heads.resized_eval_areas(model_or_logits, g if g.dtype == torch.uint8 else g.long(), self.ignore_index)
        elif aug is not None:
            a = model_or_logits.eval_areas(img, gt, self.ignore_index, aug=aug)
        else:
            a = model_or_logits.eval_areas(img, gt, self.ignore_index)
        if a.shape != (3, self.num_classes):
            raise ValueError(f"areas {tuple(a.shape)} from logits of {a.shape[1]} classes; this evaluator has {self.num_classes}")
        self.areas = a.clone() if self.areas is None else self.areas + a.to(self.areas.device)
        return a

    def all_reduce(self, group=None):
        """Sum the areas over the process group (the default one when group is None); a no-op without an initialised group."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            if self.areas is None:
                raise RuntimeError("SegEvaluator.all_reduce before the first update (no device to reduce on)")
            dist.all_reduce(self.areas, op=dist.ReduceOp.SUM, group=group)
        return self

    def compute(self, metrics=("mIoU",), nan_to_num=None, beta=1):
        if self.areas is None:
            raise RuntimeError("SegEvaluator.compute before the first update")
        return total_area_to_metrics(self.areas, metrics, nan_to_num, beta)
