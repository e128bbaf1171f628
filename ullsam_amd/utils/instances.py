"""Scoring a predicted instance label image against a ground-truth one (the reference has CalcIoU for ONE mask pair only,
train_joint_v2.py:683-694; instance segmentation of cells is scored by matching instances).  Everything follows from one integer
contingency table (`utils.amg.label_overlap`, csrc/labels.hip on the GPU), in float64.
"""
from __future__ import annotations

import math
from typing import Dict, Sequence

import numpy as np
import torch

from . import amg as A

DEFAULT_THRESHOLDS = tuple(round(0.5 + 0.05 * i, 2) for i in range(10))


def scores_from_table(table: np.ndarray, thresholds: Sequence[float] = DEFAULT_THRESHOLDS) -> Dict[str, np.ndarray]:
    """table int64 [na + 1, nb + 1] (row / column 0 = background) -> the dict `instance_scores` returns."""
    t = np.asarray(table, dtype=np.int64)
    thr = np.asarray(list(thresholds), dtype=np.float64).reshape(-1)
    if (thr < 0.5).any() or not np.isfinite(thr).all():
        raise ValueError(f"instance_scores: every threshold must be >= 0.5 (the match is unique only there), got {thr.tolist()}")
    area_a, area_b = t.sum(axis=1), t.sum(axis=0)
    n_pred, n_gt = int((area_a[1:] > 0).sum()), int((area_b[1:] > 0).sum())
    i, j = np.nonzero(t[1:, 1:])                              # only pairs that share a pixel have IoU > 0
    inter = t[1:, 1:][i, j]
    iou = inter.astype(np.float64) / (area_a[1:][i] + area_b[1:][j] - inter).astype(np.float64)
    out = {k: np.zeros(len(thr), np.int64) for k in ("tp", "fp", "fn")}
    out.update({k: np.zeros(len(thr), np.float64) for k in ("precision", "recall", "f1", "ap", "mean_matched_iou")})
    for n, th in enumerate(thr):
        m = iou > th
        tp = int(m.sum())
        fp, fn = n_pred - tp, n_gt - tp
        out["tp"][n], out["fp"][n], out["fn"][n] = tp, fp, fn
        out["precision"][n] = tp / (tp + fp) if tp + fp else 0.0
        out["recall"][n] = tp / (tp + fn) if tp + fn else 0.0
        out["f1"][n] = 2 * tp / (2 * tp + fp + fn) if tp + fp + fn else 0.0
        out["ap"][n] = tp / (tp + fp + fn) if tp + fp + fn else 0.0
        out["mean_matched_iou"][n] = math.fsum(iou[m].tolist()) / tp if tp else 0.0     # the exact sum, rounded once
    out["thresholds"] = thr
    out["n_pred"], out["n_gt"] = n_pred, n_gt
    return out


def instance_scores(pred, gt, thresholds: Sequence[float] = DEFAULT_THRESHOLDS) -> Dict[str, np.ndarray]:
    """Match the instances of two label images (0 = background, ids need not be consecutive) at IoU thresholds t >= 0.5.
    IoU[i, j] = T[i, j] / (area_pred[i] + area_gt[j] - T[i, j]) over the overlap table T; a pair matches when IoU > t, STRICTLY.  With
    t >= 0.5 a matched pair shares more than half of each of its two instances (T > union / 2 >= area_i / 2, and likewise for j), so no
    instance can match twice and the matching needs no assignment solver; at IoU == 0.5 exactly two candidates could tie, which is why the
    comparison is strict and thresholds below 0.5 are refused.
    Per threshold (arrays in the order of `thresholds`): tp, fp = n_pred - tp, fn = n_gt - tp (n_pred / n_gt count the ids that are present),
    precision = tp / (tp + fp), recall = tp / (tp + fn), f1 = 2 tp / (2 tp + fp + fn), ap = tp / (tp + fp + fn), mean_matched_iou = the mean IoU
    of the matched pairs; a ratio whose denominator is 0 is 0.  One `label_overlap` call; GPU tensors are tabulated on the GPU and only the
    table comes back."""
    table = A.label_overlap(pred, gt)
    return scores_from_table(table.cpu().numpy() if isinstance(table, torch.Tensor) else table, thresholds)
