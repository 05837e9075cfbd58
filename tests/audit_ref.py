"""numpy restatement of the three audit decoders (include/stair_hip.h "Audit decoders"), written from the rules and not from the
kernels: float64 arithmetic on the fp32 inputs.  Shared by tests/test_audit_host.py (hand-worked cases) and tests/test_gpu_audit.py."""
import math

import numpy as np


def span_mask(start, end, L):
    """span_to_attention (train_module.py:67-81) for L frames, in float64"""
    g = np.zeros(L, dtype=np.float64)
    start = min(L - 0.002, max(0.001, float(start)))
    end = min(L - 0.001, float(end))
    si, ei = math.ceil(start), math.floor(end)
    if si < ei:
        g[si:ei] += 1
    if si <= ei:
        g[si - 1] += si - start
        g[ei] += end - ei
    else:
        g[ei] += end - start
    return g


def decode_attention(row, L, threshold, gold=None):
    """row: fp32 values of an attention row (only row[:L] is looked at); threshold: the fp32 bound; gold: (start, end) or None.
    Returns dict(start, end, peak, on, peak_value, iou)."""
    a = np.asarray(row, dtype=np.float32)[:L]
    thr = np.float32(threshold)
    on = np.zeros(L, dtype=bool)
    peak, best = -1, None
    for t in range(L):
        v = a[t]
        if np.isnan(v):
            continue
        on[t] = bool(v >= thr)
        if best is None or v > best:           # strictly larger: the first of equal values stays
            peak, best = t, v
    if peak < 0:
        start = end = 0
        value = np.float32(np.nan)
    elif not on[peak]:
        start = end = peak
        value = best
    else:
        start, end = peak, peak + 1
        while start > 0 and on[start - 1]:
            start -= 1
        while end < L and on[end]:
            end += 1
        value = best
    iou = -1.0
    if gold is not None:
        g = span_mask(gold[0], gold[1], L)
        m = np.zeros(L, dtype=np.float64)
        m[start:end] = 1.0
        den = float(np.maximum(m, g).sum())
        iou = float((m * g).sum()) / den if den > 0 else 0.0
    return dict(start=start, end=end, peak=peak, on=int(on.sum()), peak_value=value, iou=iou)


def head_score(x, W, b):
    """float64 score of the pretrain head W [nout, H], b [nout] on x [H]: z1 - z0 (nout 2) or z (nout 1)"""
    z = np.asarray(W, dtype=np.float64) @ np.asarray(x, dtype=np.float64) + np.asarray(b, dtype=np.float64)
    return float(z[1] - z[0]) if z.size == 2 else float(z[0])


def head_pred(score, nout):
    """the decision rule on a score (any precision): nout 2: score > 0 (a tie is class 0); nout 1: score >= 0.5"""
    return int(score > 0) if nout == 2 else int(score >= 0.5)


def head_bound(x, W, b):
    """(H + 1) 2^-24 (sum_h |w_h x_h| + |b|), the rows and biases of both classes summed for nout 2"""
    W, x, b = (np.asarray(t, dtype=np.float64) for t in (W, x, b))
    return (x.size + 1) * 2.0 ** -24 * float((np.abs(W * x[None, :])).sum() + np.abs(b).sum())


def cosine_sims(q, reps):
    """float64 cos(q, reps[c]) with nn.CosineSimilarity's eps per operand (1e-8)"""
    q, reps = np.asarray(q, dtype=np.float64), np.asarray(reps, dtype=np.float64)
    dots = (reps * q[None, :]).sum(axis=1)             # row by row, so that bit-identical rows give bit-identical similarities
    return dots / (max(np.sqrt((q * q).sum()), 1e-8) * np.maximum(np.sqrt((reps * reps).sum(axis=1)), 1e-8))


def decode_rank(sims, k, gold):
    """sims: similarities of one item to every class; gold: class ids (may be empty).  Returns dict(top, top_sim, rank, best_gold_sim):
    the k best classes best first, equal similarities lower class first; rank = 1 + #{c: sim_c > best gold sim}, 0 without gold."""
    sims = np.asarray(sims)
    order = sorted(range(sims.size), key=lambda c: (-sims[c], c))[:k]
    if len(gold) == 0:
        return dict(top=order, top_sim=[sims[c] for c in order], rank=0, best_gold_sim=-np.inf)
    g = max(sims[c] for c in gold)
    return dict(top=order, top_sim=[sims[c] for c in order], rank=1 + int((sims > g).sum()), best_gold_sim=g)
