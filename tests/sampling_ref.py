"""float64 numpy restatement of what ullsam_sample_topk_topp computes for one row (helper of test_sampling_cpu.py / test_sampling_gpu.py).

reference(row, T, k, p):
  candidates   the min(k, V) largest values, NaN counted as -inf, in descending value, equal values by ascending id (so ties at the k-th value go
               to the lower ids);
  p_j          exp((x_j - x_0) / T) / sum;  a row whose leading candidate is +inf or -inf (a +inf in the row; nothing above -inf) has all its mass
               on candidate 0 (the first +inf id; id 0);
  nucleus      with m_j the mass strictly before j, candidate j stays iff j == 0 or m_j < p (p None or >= 1: all stay); renormalised over those;
  draw(u)      the first remaining candidate whose inclusive cumulative probability exceeds u."""
import numpy as np


def eps_for(top_k):
    """Worst-case rounding of an fp32 running sum of top_k terms bounded by 1 (top_k * 2^-24), with a factor 4 for the exponentials' own error."""
    return 4 * top_k * 2.0 ** -24


def full_order(row):
    """ids by value descending (NaN as -inf, -0.0 == 0.0), equal values by ascending id."""
    x = np.asarray(row, dtype=np.float64).copy()
    x[np.isnan(x)] = -np.inf
    return np.lexsort((np.arange(x.shape[0]), -x))


def reference(row, T, k, p, order=None):
    """-> dict(ids int64 [kk], probs float64 [kk] (final: 0 for removed candidates), before float64 [kk] (mass strictly before j, pre-nucleus),
    raw float64 [kk] (probabilities before the nucleus cut), top_p).  order: full_order(row) computed earlier (it does not depend on T, k, p)."""
    x = np.asarray(row, dtype=np.float64).copy()
    x[np.isnan(x)] = -np.inf
    V = x.shape[0]
    kk = min(int(k), V)
    order = (full_order(x) if order is None else order)[:kk]
    xs = x[order]
    if np.isinf(xs[0]):
        raw = np.zeros(kk); raw[0] = 1.0
    else:
        with np.errstate(over="ignore"):
            e = np.exp((xs - xs[0]) / float(T))
        raw = e / e.sum()
    before = np.concatenate([[0.0], np.cumsum(raw)[:-1]])
    keep = np.ones(kk, bool) if (p is None or p >= 1.0) else (before < p)
    keep[0] = True
    probs = np.where(keep, raw, 0.0)
    probs = probs / probs.sum()
    return dict(ids=order.astype(np.int64), probs=probs, before=before, raw=raw, top_p=p)


def _intervals(raw, keep):
    pr = np.where(keep, raw, 0.0)
    pr = pr / pr.sum()
    c = np.cumsum(pr)
    return np.concatenate([[0.0], c[:-1]]), c, pr


def accepted(ref, u, eps):
    """The set of token ids whose cumulative interval [c_{j-1}, c_j), widened by eps on both sides, contains u.  A candidate whose mass-before is within
    eps of p may be kept or dropped: the union over both readings of every such candidate (they are consecutive; each cut point is tried)."""
    raw, before, ids, p = ref["raw"], ref["before"], ref["ids"], ref["top_p"]
    kk = len(ids)
    if p is None or p >= 1.0:
        cuts = [kk]
    else:
        sure = 1 + int(np.sum(before[1:] < p - eps))                 # kept under every reading (before is non-decreasing)
        maybe = 1 + int(np.sum(before[1:] < p + eps))
        cuts = list(range(sure, maybe + 1))
    acc = set()
    for K in cuts:
        keep = np.arange(kk) < K
        lo, hi, pr = _intervals(raw, keep)
        for j in range(K):
            if pr[j] > 0.0 and lo[j] - eps <= u < hi[j] + eps:
                acc.add(int(ids[j]))
    return acc
