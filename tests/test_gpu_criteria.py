"""Direct tests of the intermediate-supervision loss kernels (csrc/losses.hip, and the decoder CE of csrc/rowops_bwd.hip)
against the reference's own values (tests/golden/criteria.npz, criteria_filterframe.npz) and against float64
restatements of CriterionByModule (train_module.py:33-194), at the shapes, interval edges and saturations where a
kernel goes wrong.  Every call goes straight through the C ABI with device tensors.  Gradients land in arenas larger
than the items need: the items sit at non-zero slots, and the rows no item owns must stay exactly zero."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import GOLDEN, load_golden
from stair_amd import losses as SL
from stair_amd._lib import StairError, check, lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LDS_FLOATS = 60 * 1024 // 4          # the loss kernels' LDS budget


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().double().numpy()


def assert_losses(got, ref, tol=2e-5, what=''):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bad = ~(np.abs(got - ref) <= tol * np.maximum(1.0, np.abs(ref)))
    assert not bad.any(), (what, np.flatnonzero(bad)[:8], got[bad][:8], ref[bad][:8])


def assert_grad(got, ref, tol=2e-5, what='', mag=None, elem_tol=1e-5):
    """|got - ref| <= tol * max|ref| over the tensor.  With `mag` (per element, the size of the terms that make it) also
    |got - ref| <= elem_tol * mag element by element, so that a wrong small element is not hidden behind a large one."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.isfinite(got).all(), what
    err = np.abs(got - ref)
    assert err.max(initial=0.0) <= tol * np.abs(ref).max(initial=0.0), (what, err.max(initial=0.0), np.abs(ref).max(initial=0.0))
    if mag is not None:
        bad = err > elem_tol * np.asarray(mag)
        assert not bad.any(), (what, np.argwhere(bad)[:8], got[bad][:8], ref[bad][:8])


def assert_rows(got, ref, rows, tol, what=''):
    """Per row r of `rows` (one item's gradient): max |got - ref| <= tol * max |ref| of that row, plus 1e-6 of the tensor's
    largest |ref| for rows whose fp64 value is below what fp32 resolves (an exp that underflows to an exact 0)."""
    floor = 1e-6 * np.abs(ref).max()
    for r in rows:
        err = np.abs(got[r] - ref[r]).max()
        assert err <= tol * np.abs(ref[r]).max() + floor, (what, r, err, np.abs(ref[r]).max())


def assert_unowned_zero(d, owned, what=''):
    d = np.asarray(d)
    assert (d[~owned] == 0.0).all(), (what, np.argwhere((d != 0.0) & ~owned)[:8])


def set_groups(slots, mode):
    """mode None: no grouping call; 'slot': the groups of losses.slot_groups; 'too_many': n_groups = n + 1 with a grp_off
    that would make a grouped launch evaluate nothing (the launch must fall back to one item per workgroup).  Returns the
    device arrays, which must outlive the launch."""
    if mode is None:
        return None
    if mode == 'slot':
        order, goff = SL.slot_groups(slots)
        ng = len(goff) - 1
    else:
        order, goff = np.arange(len(slots), dtype=np.int32), np.zeros(len(slots) + 2, dtype=np.int32)
        ng = len(slots) + 1
    keep = (i32(order), i32(goff))
    check(lib.stair_loss_groups(P(keep[0]), P(keep[1]), ng))
    return keep


# ---------------------------------------------------------------------------------------------------------------
# attention BCE (Localize / Temporal / ExistsFrame)

def span64(g0, g1, L):
    """train_module.py:67-81 in float64 with Python's index rule (a negative end counts from the clip's end), rounded to
    float32 like the reference's tensor (every frame receives at most one term)."""
    g = np.zeros(L)
    start, end = min(L - 0.002, max(0.001, g0)), min(L - 0.001, g1)
    si, ei = math.ceil(start), math.floor(end)
    if si < ei:
        g[si:ei] += 1
    if si <= ei:
        g[si - 1] += si - start
        g[ei] += end - ei
    else:
        g[ei] += end - start
    return g.astype(np.float32).astype(np.float64)


def interval_families(L, rng):
    """(family, (start, end)) at clip length L: integer endpoints, zero length, inside one frame, reversed, start < 0,
    end > L, start >= L, negative end with -L <= floor(end) < 0."""
    u = lambda a, b: float(rng.uniform(a, b))
    f = int(rng.integers(0, L))
    fam = [('integer', (0.0, float(L))), ('integer', (float(L // 4), float(max(L // 4 + 1, 3 * L // 4)))),
           ('zero', (u(0, L),) * 2), ('zero', (float(L // 2),) * 2),
           ('one_frame', (f + 0.2, f + 0.7)),
           ('reversed', (u(0.6 * L, L), u(0, 0.4 * L))),
           ('start<0', (-3.5, u(0.1, L))),
           ('end>L', (u(0, L), L + 5.2)),
           ('start>=L', (float(L), L + 1.0)), ('start>=L', (L + 0.5, L + 3.0)),
           ('neg_end', (-1.0, -0.5)), ('neg_end', (3.0, -2.0)), ('neg_end', (-3.0, -1.0)),
           ('neg_end', (u(0, L), -float(L))), ('neg_end', (u(-2, L), u(-L, 0)))]
    return [(n, iv) for n, iv in fam if math.floor(min(L - 0.001, iv[1])) >= -L]


def attention_ref(att, items, scale):
    """items [(slot, K, intervals, L)]; att [R, T] float32 numpy.  (loss [n], d_att, |terms| of d_att) in float64."""
    a = att.astype(np.float64)
    loss, d, mag = [], np.zeros_like(a), np.zeros_like(a)
    for slot, K, ivs, L in items:
        p = a[slot:slot + K, :L]
        g = np.stack([span64(s, e, L) for s, e in ivs])
        loss.append(np.mean(-(g * np.log(p) + (1 - g) * np.log(1 - p))))
        c = scale / (K * L)
        d[slot:slot + K, :L] += c * (-g / p + (1 - g) / (1 - p))
        mag[slot:slot + K, :L] += abs(c) * (np.abs(g) / p + np.abs(1 - g) / (1 - p))       # (a reversed interval's gold is < 0)
    return np.array(loss), d, mag


def run_attention(att, items, T, scale, use_len=True, grad=True, groups=None):
    slots = [it[0] for it in items]
    K = [it[1] for it in items]
    iv = np.array([v for it in items for v in it[2]], dtype=np.float64).reshape(-1, 2)
    att_d = f32(att)
    d = torch.zeros_like(att_d) if grad else None
    loss = torch.full((len(items),), float('nan'), device=DEV)
    args = (i32(slots), i32(K), i32(np.concatenate([[0], np.cumsum(K)[:-1]])), torch.from_numpy(iv).to(DEV))
    keep = set_groups(slots, groups)
    if use_len:
        check(lib.stair_loss_attention_len(P(att_d), P(d), *[P(a) for a in args], P(i32([it[3] for it in items])), len(items), T,
                                           C.c_float(scale), P(loss), S()))
    else:
        check(lib.stair_loss_attention(P(att_d), P(d), *[P(a) for a in args], len(items), T, C.c_float(scale), P(loss), S()))
    out = host(loss), (host(d) if d is not None else None)
    del keep
    return out


def attention_arena(items_spec, T, rng):
    """items_spec [(K, intervals, L)] -> (att [R, T] float32, items with slots, owned-row mask).  Items at slots 1, K+2, ...
    (a free row between them); probabilities from a sigmoid of random logits, some within 1e-6 of 0 and 1; 7.0 (a value
    whose log(1-p) is NaN) past each clip's own frames; 0.5 in rows no item owns."""
    rows = 1 + sum(k + 1 for k, _, _ in items_spec) + 1
    att = np.full((rows, T), 0.5, dtype=np.float32)
    owned = np.zeros((rows, T), dtype=bool)
    items, at = [], 1
    for K, ivs, L in items_spec:
        p = 1.0 / (1.0 + np.exp(-3.0 * rng.standard_normal((K, L))))
        flat = p.reshape(-1)
        flat[rng.random(flat.size) < 0.1] = 5e-7
        flat[rng.random(flat.size) < 0.1] = 1 - 5e-7
        att[at:at + K, :L] = np.clip(p, 5e-7, 1 - 5e-7)
        att[at:at + K, L:] = 7.0
        owned[at:at + K, :L] = True
        items.append((at, K, ivs, L))
        at += K + 1
    assert (att[owned] > 0).all() and (att[owned] < 1).all()
    return att, items, owned


def test_attention_kernel_matches_reference_fixture():
    """Every Temporal, ExistsFrame and Localize case of criteria.npz (the reference's CriterionByModule), interval edges
    [5,5], [7,9], [-1,0.4], [39.5,41], [0,40] included: loss and d_att within 2e-6."""
    z, meta = load_golden('criteria')
    T, n = meta['T'], 0
    for i, case in enumerate(meta['cases']):
        if case['module'] not in SL.ATTENTION_KINDS:
            continue
        pred = z['c%d/pred' % i].reshape(-1, T)
        K = pred.shape[0]
        ivs = [tuple(case['gold'])] if case['module'] != 'Localize' else [tuple(g) for g in case['gold']]
        att = np.full((K + 3, T), 0.5, dtype=np.float32)
        att[2:2 + K] = pred
        loss, d = run_attention(att, [(2, K, ivs, T)], T, 1.0, use_len=False)
        ref_loss, ref_d = float(z['c%d/loss' % i]), z['c%d/dpred' % i].reshape(K, T).astype(np.float64)
        assert abs(loss[0] - ref_loss) <= 2e-6 * max(1.0, abs(ref_loss)), (i, case, loss[0], ref_loss)
        assert np.abs(d[2:2 + K] - ref_d).max() <= 2e-6 * max(1.0, np.abs(ref_d).max()), (i, case)
        owned = np.zeros_like(att, dtype=bool)
        owned[2:2 + K] = True
        assert_unowned_zero(d, owned, i)
        n += 1
    assert n == 16


@pytest.mark.parametrize('T', [1, 2, 40, 63, 64, 65, 100])
def test_attention_kernel_interval_families_vs_fp64(T):
    """K in {1, 2}, clips of T and fewer frames (stride still T, garbage past the clip), every interval family including
    negative ends (the reference's gold_tensor[end_int] wraps to frame L + end_int), predictions near 0 and 1."""
    rng = np.random.default_rng(100 + T)
    spec, names = [], []
    for L in sorted({T, max(1, T - 1), max(1, (T + 1) // 2)}):
        fam = interval_families(L, rng)
        for name, iv in fam:
            spec.append((1, [iv], L)); names.append(name)
        for j in range(0, len(fam) - 1, 2):
            spec.append((2, [fam[j][1], fam[j + 1][1]], L)); names.append(fam[j][0] + '+' + fam[j + 1][0])
    att, items, owned = attention_arena(spec, T, rng)
    scale = 0.37 if T % 2 else 1.0
    loss, d = run_attention(att, items, T, scale)
    ref_loss, ref_d, mag = attention_ref(att, items, scale)
    for j, nm in enumerate(names):
        assert_losses(loss[j:j + 1], ref_loss[j:j + 1], what=(T, nm, items[j]))
    assert_grad(d, ref_d, what=T, mag=mag)
    assert_unowned_zero(d, owned, T)
    # values only (NULL gradient), as the validation loop calls it: the same losses
    loss2, _ = run_attention(att, items, T, 0.0, grad=False)
    assert np.array_equal(loss2, loss)
    # the entry point without `len` on the items that span the whole stride
    full = [j for j, it in enumerate(items) if it[3] == T]
    loss3, d3 = run_attention(att, [items[j] for j in full], T, scale, use_len=False)
    assert np.array_equal(loss3, loss[full])
    rows = np.zeros(att.shape[0], dtype=bool)
    for j in full:
        rows[items[j][0]:items[j][0] + items[j][1]] = True
    assert np.array_equal(d3[rows], d[rows]) and (d3[~rows] == 0).all()


# ---------------------------------------------------------------------------------------------------------------
# linear heads (Exists / Xor: 2-way CE, Equals: MSE)

def head_ref(vec, slots, labels, W, b, scale):
    x = vec[slots].astype(np.float64)
    W64, y = W.astype(np.float64), np.asarray(labels) != 0
    z = x @ W64.T + b.astype(np.float64)
    if W.shape[0] == 2:
        m = z.max(1, keepdims=True)
        lse = (m + np.log(np.exp(z - m).sum(1, keepdims=True)))[:, 0]
        loss = lse - z[np.arange(len(y)), y.astype(int)]
        dz = np.exp(z - lse[:, None])
        dz[np.arange(len(y)), y.astype(int)] -= 1.0
    else:
        diff = z[:, 0] - y
        loss, dz = diff * diff, 2.0 * diff[:, None]
    dz *= scale
    dvec = np.zeros(vec.shape)
    np.add.at(dvec, slots, dz @ W64)
    return loss, dvec, dz.T @ x, dz.sum(0)


def run_head(vec, slots, labels, W, b, scale, groups=None, grads=True):
    H, nout = vec.shape[1], W.shape[0]
    vd, Wd, bd = f32(vec), f32(W), f32(b)
    dv, dW, db = (torch.zeros_like(vd), torch.zeros_like(Wd), torch.zeros_like(bd)) if grads else (None, None, None)
    loss = torch.full((len(slots),), float('nan'), device=DEV)
    s_d, l_d = i32(slots), i32(labels)
    keep = set_groups(slots, groups)
    check(lib.stair_loss_head(nout, P(vd), P(dv), P(s_d), P(l_d), P(Wd), P(bd), P(dW), P(db), len(slots), H, C.c_float(scale),
                              P(loss), S()))
    out = (host(loss),) + ((host(dv), host(dW), host(db)) if grads else (None, None, None))
    del keep
    return out


def test_head_kernel_matches_reference_fixture():
    """Exists / Xor / Equals cases of criteria.npz: with H = nout, W = I, b = 0 the head is the identity, so loss and
    d vec are the reference's loss and d loss / d pred; dW = dz x^T, db = dz."""
    z, meta = load_golden('criteria')
    n = 0
    for i, case in enumerate(meta['cases']):
        if case['module'] not in ('Exists', 'Xor', 'Equals'):
            continue
        pred = z['c%d/pred' % i].astype(np.float32)
        nout = pred.size
        vec = np.zeros((4, nout), dtype=np.float32)
        vec[0] = 0.7
        vec[2] = pred
        loss, dv, dW, db = run_head(vec, [2], [int(case['gold'])], np.eye(nout, dtype=np.float32), np.zeros(nout, np.float32), 1.0)
        ref_loss, ref_d = float(z['c%d/loss' % i]), z['c%d/dpred' % i].astype(np.float64)
        assert abs(loss[0] - ref_loss) <= 2e-6 * max(1.0, abs(ref_loss)), (i, case)
        assert np.abs(dv[2] - ref_d).max() <= 2e-6 * max(1.0, np.abs(ref_d).max()), (i, case)
        assert np.abs(db - ref_d).max() <= 2e-6 and np.abs(dW - np.outer(ref_d, pred)).max() <= 2e-6, (i, case)
        assert (dv[[0, 1, 3]] == 0).all()
        n += 1
    assert n == 6


@pytest.mark.parametrize('nout', [2, 1])
@pytest.mark.parametrize('H', [1, 63, 64, 65, 300, 512, 1000])
def test_head_kernel_vs_fp64(H, nout):
    """Logits up to ~60 in magnitude, ~2000 items (dW / db accumulate over many waves), scale != 1."""
    rng = np.random.default_rng(7 * H + nout)
    n = 2000
    slots = 1 + 2 * np.arange(n)                                  # a free row after every item
    vec = np.zeros((2 * n + 2, H), dtype=np.float32)
    vec[0::2] = 3.0                                               # rows no item owns (never read)
    u = np.exp(rng.uniform(np.log(0.01), np.log(20.0), n))        # per-item logit size (|z| up to ~60)
    vec[slots] = (rng.standard_normal((n, H)) * u[:, None]).astype(np.float32)
    W = (rng.standard_normal((nout, H)) / math.sqrt(H)).astype(np.float32)
    b = (rng.standard_normal(nout) * 0.5).astype(np.float32)
    labels = rng.integers(0, 2, n)
    labels[::5] *= 7                                              # any non-zero label is True
    scale = 0.25
    loss, dv, dW, db = run_head(vec, slots, labels, W, b, scale)
    ref_loss, ref_dv, ref_dW, ref_db = head_ref(vec, slots, labels, W, b, scale)
    assert_losses(loss, ref_loss, what=H)
    assert_grad(dv, ref_dv, what='d_vec')
    assert_rows(dv, ref_dv, slots, 1e-4, 'd_vec per item')
    assert_grad(dW, ref_dW, what='dW')
    assert_grad(db, ref_db, what='db')
    owned = np.zeros(vec.shape, dtype=bool)
    owned[slots] = True
    assert_unowned_zero(dv, owned)


# ---------------------------------------------------------------------------------------------------------------
# contrastive CE through L2Normalize (Filter / ToAction / Superlative)

def contrastive_ref(x, Gwin, pos, scale):
    """cross_entropy(Gwin @ normalize(x)) at class `pos`, float64 autograd: (loss, scale * d loss / d x)."""
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    logits = torch.tensor(Gwin, dtype=torch.float64) @ F.normalize(xt, dim=0)
    loss = F.cross_entropy(logits[None], torch.tensor([pos]))
    (loss * scale).backward()
    return float(loss.detach()), xt.grad.numpy()


def run_contrastive(vec, slots, pos, ws, wc, G, scale, max_classes=None, groups=None, grads=True):
    H = vec.shape[1]
    vd, Gd = f32(vec), f32(G)
    dv = torch.zeros_like(vd) if grads else None
    loss = torch.full((len(slots),), float('nan'), device=DEV)
    a = [i32(slots), i32(pos), i32(ws), i32(wc)]
    keep = set_groups(slots, groups)
    check(lib.stair_loss_contrastive(P(vd), P(dv), *[P(t) for t in a], P(Gd), len(slots), H,
                                     int(max(wc)) if max_classes is None else max_classes, C.c_float(scale), P(loss), S()))
    out = host(loss), (host(dv) if grads else None)
    del keep
    return out


def run_table(vec, slots, pos_cls, win_row, presence, reps, scale, groups=None):
    H = vec.shape[1]
    vd, pd, rd = f32(vec), f32(presence), f32(reps)
    dv = torch.zeros_like(vd)
    loss = torch.full((len(slots),), float('nan'), device=DEV)
    a = [i32(slots), i32(pos_cls), i32(win_row)]
    keep = set_groups(slots, groups)
    check(lib.stair_loss_contrastive_table(P(vd), P(dv), *[P(t) for t in a], P(pd), P(rd), len(slots), reps.shape[0], H,
                                           C.c_float(scale), P(loss), S()))
    out = host(loss), host(dv)
    del keep
    return out


def unit_rows(rng, n, H):
    g = rng.standard_normal((n, H))
    return (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)


def test_contrastive_kernel_matches_reference_fixture():
    """Filter / ToAction / Superlative cases of criteria.npz: the prediction is unit-norm, so L2Normalize leaves it (to
    rounding) and the loss is the reference's; positive = row 0 of the window.  The window sits behind another one."""
    z, meta = load_golden('criteria')
    n = 0
    for i, case in enumerate(meta['cases']):
        if case['module'] not in SL.CONTRASTIVE:
            continue
        pred, gold = z['c%d/pred' % i], z[case['gold']]
        Gm = np.concatenate([np.ones((3, pred.size), np.float32), gold])
        vec = np.zeros((3, pred.size), dtype=np.float32)
        vec[1] = pred
        loss, dv = run_contrastive(vec, [1], [3], [3], [gold.shape[0]], Gm, 1.0)
        ref = float(z['c%d/loss' % i])
        assert abs(loss[0] - ref) <= 2e-6 * max(1.0, abs(ref)), (i, case, loss[0], ref)
        _, ref_dv = contrastive_ref(pred, gold, 0, 1.0)
        assert_grad(dv[1], ref_dv, what=i)
        assert (dv[[0, 2]] == 0).all()
        n += 1
    assert n == 6


@pytest.mark.parametrize('H', [64, 300, 512])
def test_contrastive_kernel_windows_vs_fp64(H):
    """Windows of C in {1, 2, 63, 64, 65, 214, 1000} classes in ONE launch, positives anywhere in the window, several items
    per window, unit class rows; one window's rows scaled by 100 (a saturated softmax: most gradient terms are exact
    zeros in fp32 and the kernel skips them).  scale != 1."""
    rng = np.random.default_rng(H)
    sizes = [1, 2, 63, 64, 65, 214, 1000, 40]
    G, ws, wc = [], [], []
    for k, c in enumerate(sizes):
        ws.append(sum(wc)); wc.append(c)
        g = unit_rows(rng, c, H)
        G.append(g * 100.0 if k == len(sizes) - 1 else g)
    G = np.concatenate(G).astype(np.float32)
    items = []                                                    # (window, positive index in the window)
    for k, c in enumerate(sizes):
        for p in sorted({0, c - 1, int(rng.integers(0, c)), c // 2}):
            items.append((k, p))
    n = len(items)
    vec = np.full((2 * n + 1, H), 0.25, dtype=np.float32)
    slots = 1 + 2 * np.arange(n)
    vec[slots] = rng.standard_normal((n, H)).astype(np.float32) * rng.uniform(0.1, 10, (n, 1)).astype(np.float32)
    k_last = len(sizes) - 1
    for j, (k, p) in enumerate(items):                           # saturated window: positive far from the top logit
        if k == k_last:
            lg = G[ws[k]:ws[k] + wc[k]] @ (vec[slots[j]] / np.linalg.norm(vec[slots[j]]))
            items[j] = (k, int(np.argsort(lg)[j % 3]))
    pos = [ws[k] + p for k, p in items]
    scale = 0.6
    loss, dv = run_contrastive(vec, slots, pos, [ws[k] for k, _ in items], [wc[k] for k, _ in items], G, scale)
    ref_dv = np.zeros(vec.shape)
    for j, (k, p) in enumerate(items):
        rl, rg = contrastive_ref(vec[slots[j]], G[ws[k]:ws[k] + wc[k]], p, scale)
        assert_losses(loss[j:j + 1], [rl], what=(H, sizes[k], p))
        ref_dv[slots[j]] = rg
    assert_grad(dv, ref_dv, what=H)
    assert_rows(dv, ref_dv, slots, 1e-4, 'd_vec per item')
    owned = np.zeros(vec.shape, dtype=bool)
    owned[slots] = True
    assert_unowned_zero(dv, owned)


def table_case(rng, H, n_cls, n_win, per_win, n):
    reps = unit_rows(rng, n_cls, H)
    presence = np.zeros((n_win, n_cls), dtype=np.float32)
    pools = []
    for w in range(n_win):
        pool = np.sort(rng.choice(n_cls, size=per_win[w], replace=False))
        presence[w, pool] = rng.choice([1.0, 2.0, 3.0], size=pool.size)     # summed over ranks: any count > 0 is present
        pools.append(pool)
    win_row = rng.integers(0, n_win, n)
    pos_cls = np.array([pools[w][rng.integers(0, len(pools[w]))] for w in win_row])
    vec = np.full((n + 3, H), -0.5, dtype=np.float32)
    slots = 2 + np.arange(n)
    vec[slots] = rng.standard_normal((n, H)).astype(np.float32)
    return reps, presence, pools, win_row, pos_cls, vec, slots


@pytest.mark.parametrize('H,n_cls', [(64, 214), (300, (LDS_FLOATS - 300) // 3), (512, (LDS_FLOATS - 512) // 3)])
def test_contrastive_table_kernel_vs_fp64_and_list_form(H, n_cls):
    """Presence-matrix form: most classes absent from every window, n_cls up to the largest the 60 KB LDS check admits.
    Matches fp64 on the pooled rows, and the list form (the same pools as explicit windows) gives the same values."""
    rng = np.random.default_rng(n_cls)
    n_win = 5
    per_win = [1, 2, 37, 65, min(n_cls, 300)]
    reps, presence, pools, win_row, pos_cls, vec, slots = table_case(rng, H, n_cls, n_win, per_win, 40)
    scale = 1.5
    loss, dv = run_table(vec, slots, pos_cls, win_row, presence, reps, scale)
    ref_dv = np.zeros(vec.shape)
    for j, w in enumerate(win_row):
        p = int(np.searchsorted(pools[w], pos_cls[j]))
        rl, rg = contrastive_ref(vec[slots[j]], reps[pools[w]], p, scale)
        assert_losses(loss[j:j + 1], [rl], what=(H, n_cls, w))
        ref_dv[slots[j]] = rg
    assert_grad(dv, ref_dv, what=(H, n_cls))
    assert_rows(dv, ref_dv, slots, 1e-4, 'd_vec per item')
    owned = np.zeros(vec.shape, dtype=bool)
    owned[slots] = True
    assert_unowned_zero(dv, owned)
    # the list form over the same pools: window w = reps[pools[w]] at row offset start[w]
    start = np.concatenate([[0], np.cumsum([len(p) for p in pools])[:-1]])
    G = np.concatenate([reps[p] for p in pools])
    lpos = [start[w] + int(np.searchsorted(pools[w], c)) for w, c in zip(win_row, pos_cls)]
    lloss, ldv = run_contrastive(vec, slots, lpos, start[win_row], [len(pools[w]) for w in win_row], G, scale)
    assert_losses(lloss, loss, tol=2e-6, what='list vs table')
    assert_grad(ldv, dv, tol=2e-6, what='list vs table')
    # one class more than the LDS admits: refused before launch
    over = (LDS_FLOATS - H) // 3 + 1
    big = np.zeros((1, over), dtype=np.float32)
    big[0, 0] = 1.0
    with pytest.raises(StairError):
        run_table(vec[:3], [2], [0], [0], big, unit_rows(rng, over, H), 1.0)


@pytest.mark.parametrize('H', [64, 512])
def test_contrastive_list_form_lds_bound(H):
    """The list form sizes its LDS from max_classes: the largest window the 60 KB check admits runs and matches fp64;
    one class more raises StairError instead of launching."""
    rng = np.random.default_rng(5 + H)
    c = (LDS_FLOATS - H) // 3
    G = unit_rows(rng, c, H)
    vec = np.zeros((3, H), dtype=np.float32)
    vec[1] = rng.standard_normal(H)
    loss, dv = run_contrastive(vec, [1, 1], [17, c - 1], [0, 0], [c, c], G, 1.0)
    for j, p in enumerate([17, c - 1]):
        rl, _ = contrastive_ref(vec[1], G, p, 1.0)
        assert_losses(loss[j:j + 1], [rl])
    ref = contrastive_ref(vec[1], G, 17, 1.0)[1] + contrastive_ref(vec[1], G, c - 1, 1.0)[1]
    assert_grad(dv[1], ref)
    with pytest.raises(StairError):
        run_contrastive(vec, [1], [0], [0], [1], G, 1.0, max_classes=c + 1)


# ---------------------------------------------------------------------------------------------------------------
# FilterFrame (pretrain head on every frame + softmax + BCE)

def filterframe_ref(xmap, slots, gold, lens, W, b, scale):
    """float64 autograd of BCELoss(softmax(x W^T + b), gold) over each item's first L frames (torch clamps the log at -100
    and the gradient's denominator at 1e-12, like the kernel)."""
    x = torch.tensor(xmap, dtype=torch.float64, requires_grad=True)
    Wt = torch.tensor(W, dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(b, dtype=torch.float64, requires_grad=True)
    losses, total = [], 0
    for i, (s, L) in enumerate(zip(slots, lens)):
        pr = torch.softmax(x[s, :L] @ Wt.t() + bt, dim=1)
        l = F.binary_cross_entropy(pr, torch.tensor(gold[i, :L], dtype=torch.float64))
        losses.append(float(l))
        total = total + l
    (total * scale).backward()
    return np.array(losses), x.grad.numpy(), Wt.grad.numpy(), bt.grad.numpy()


def run_filterframe(xmap, slots, gold, lens, W, b, scale, groups=None):
    n, T, O = gold.shape
    H = xmap.shape[2]
    xd, gd, Wd, bd = f32(xmap), f32(gold), f32(W), f32(b)
    dm, dW, db = torch.zeros_like(xd), torch.zeros_like(Wd), torch.zeros_like(bd)
    loss = torch.full((n,), float('nan'), device=DEV)
    s_d, len_d = i32(slots), i32(lens)
    keep = set_groups(slots, groups)
    check(lib.stair_loss_filterframe_len(P(xd), P(dm), P(s_d), P(gd), P(Wd), P(bd), P(dW), P(db), P(len_d), n, T, H, O,
                                         C.c_float(scale), P(loss), S()))
    out = host(loss), host(dm), host(dW), host(db)
    del keep
    return out


def filterframe_case(rng, T, O, H, lens, slots, n_slots):
    """Map tiles [n_slots, T, H] with the items at `slots`; head W [O, H] whose hidden unit 0 drives class 0 alone, so
    frames with x[t, 0] = +-300 saturate the softmax (class 0 at p = 1 or 0 in fp32: the -100 log clamp and the 1e-12
    gradient clamp); gold rows: random interval-like masks normalised to 1, some rows all zero, garbage past the clip."""
    n = len(lens)
    xmap = np.full((n_slots, T, H), 2.0, dtype=np.float32)
    gold = np.full((n, T, O), 0.3, dtype=np.float32)
    W = (rng.standard_normal((O, H)) * 0.1).astype(np.float32)
    W[:, 0] = 0.0
    W[0, 0] = 1.0
    b = (rng.standard_normal(O) * 0.3).astype(np.float32)
    for i, (s, L) in enumerate(zip(slots, lens)):
        x = rng.standard_normal((L, H)).astype(np.float32)
        sat = rng.random(L) < 0.25
        x[sat, 0] = np.where(rng.random(int(sat.sum())) < 0.5, 300.0, -300.0)
        xmap[s, :L] = x
        g = (rng.random((L, O)) < min(0.5, 3.0 / O)).astype(np.float32) * rng.uniform(0.1, 1.0, (L, O)).astype(np.float32)
        g[rng.random(L) < 0.2] = 0.0                              # no entity on these frames
        with np.errstate(invalid='ignore', divide='ignore'):
            g = g / g.sum(1, keepdims=True)
        g[~np.isfinite(g)] = 0.0
        gold[i, :L] = g
    return xmap, gold, W, b


@pytest.mark.parametrize('T,O,H', [(102, 150, 512), (426, 36, 64), (15360, 1, 64), (40, 36, 512), (24, 150, 64), (40, 36, 192), (24, 36, 448)])
def test_filterframe_kernel_vs_fp64(T, O, H):
    """T * O up to the LDS limit, O in {1, 36, 150}, H in {64, 192, 448, 512}, all-zero gold rows, saturated softmax frames, clips
    shorter than T; two items share a tile (atomic adds); d_map, dW, db vs fp64 autograd."""
    rng = np.random.default_rng(T * O + H)
    lens, slots = [T, max(1, T // 2), max(1, T // 2)], [1, 3, 3]     # items 1 and 2 share a tile (one clip)
    xmap, gold, W, b = filterframe_case(rng, T, O, H, lens, slots, 6)
    scale = 0.75
    loss, dm, dW, db = run_filterframe(xmap, slots, gold, lens, W, b, scale)
    ref_loss, ref_dm, ref_dW, ref_db = filterframe_ref(xmap, slots, gold, lens, W, b, scale)
    assert_losses(loss, ref_loss, what=(T, O, H))
    assert_grad(dm, ref_dm, what='d_map')
    assert_grad(dW, ref_dW, what='dW')
    assert_grad(db, ref_db, what='db')
    owned = np.zeros(xmap.shape, dtype=bool)
    for s, L in zip(slots, lens):
        owned[s, :L] = True
    assert_unowned_zero(dm, owned)
    if T * (O + 1) * 4 > 60 * 1024:
        with pytest.raises(StairError):                           # one more column than the LDS tile holds
            run_filterframe(xmap[:, :, :H], slots[:1], np.zeros((1, T, O + 1), np.float32), lens[:1],
                            np.zeros((O + 1, H), np.float32), np.zeros(O + 1, np.float32), 1.0)


def test_filterframe_kernel_matches_reference_fixture_at_offset():
    """criteria_filterframe.npz through losses.filterframe_target: every case, items at slots 2 and 4 of 6 in one launch."""
    z = np.load(os.path.join(GOLDEN, 'criteria_filterframe.npz'))
    meta = json.loads(bytes(z['meta']).decode())
    O, H = meta['O'], 64
    index = SL.object_index(meta['word2id'])
    for i, case in enumerate(meta['cases']):
        T = case['T']
        pred = z['c%d/pred' % i]
        gold = {k: tuple(v) for k, v in case['gold'].items()}
        tgt = SL.filterframe_target(gold, T, O, index)[None]
        xmap = np.zeros((6, T, H), dtype=np.float32)
        xmap[2, :, :O] = pred
        W = np.zeros((O, H), dtype=np.float32)
        W[:, :O] = np.eye(O)
        loss, dm, _, _ = run_filterframe(xmap, [2], tgt, [T], W, np.zeros(O, np.float32), 1.0)
        ref = float(z['c%d/loss' % i])
        assert abs(loss[0] - ref) <= 2e-6 * max(1.0, abs(ref)), (i, loss[0], ref)
        assert np.abs(dm[2, :, :O] - z['c%d/dpred' % i]).max() <= 2e-6, i
        assert (dm[[0, 1, 3, 4, 5]] == 0).all() and (dm[2, :, O:] == 0).all()


# ---------------------------------------------------------------------------------------------------------------
# decoder CE (validation loss) and the validation cosine

def run_decoder_ce(logits, answers):
    ld, ad = f32(logits), i32(answers)
    loss = torch.full((len(answers),), 123.0, device=DEV)
    check(lib.stair_loss_decoder_ce(P(ld), P(ad), P(loss), len(answers), logits.shape[1], S()))
    return host(loss)


def test_decoder_ce_matches_reference_fixture():
    z, meta = load_golden('criteria')
    i = [j for j, c in enumerate(meta['cases']) if c['module'] == 'decoder'][0]
    pred = z['c%d/pred' % i][None]
    loss = run_decoder_ce(np.concatenate([pred * 3, pred]), [2, meta['cases'][i]['gold']])
    ref = float(z['c%d/loss' % i])
    assert abs(loss[1] - ref) <= 2e-6 * max(1.0, abs(ref))


@pytest.mark.parametrize('A', [1, 2, 63, 64, 65, 172, 5000])
def test_decoder_ce_vs_fp64(A):
    """Logits up to +-80; answer -1 gives 0, answer >= A gives NaN (documented), everything else fp64 logsumexp - x[a]."""
    rng = np.random.default_rng(A)
    n = 37
    logits = (rng.uniform(-1, 1, (n, A)) * rng.choice([0.1, 5.0, 80.0], (n, 1))).astype(np.float32)
    answers = rng.integers(0, A, n)
    answers[3], answers[11], answers[20] = -1, A, A + 7
    answers[5] = int(np.argmax(logits[5]))
    answers[6] = int(np.argmin(logits[6]))
    loss = run_decoder_ce(logits, answers)
    x = logits.astype(np.float64)
    m = x.max(1)
    ref = m + np.log(np.exp(x - m[:, None]).sum(1)) - x[np.arange(n), np.clip(answers, 0, A - 1)]
    ok = (answers >= 0) & (answers < A)
    assert_losses(loss[ok], ref[ok], what=A)
    assert loss[3] == 0.0 and np.isnan(loss[11]) and np.isnan(loss[20])


def run_cosine(vec, slots, reps, seg_off):
    vd, od = f32(vec), torch.full((len(slots),), 9.0, device=DEV)
    rd = f32(reps) if reps is not None else None
    s_d, o_d = i32(slots), i32(seg_off)
    check(lib.stair_score_cosine_to_mean(P(vd), P(s_d), P(rd), P(o_d), P(od), len(slots), vec.shape[1], S()))
    return host(od)


@pytest.mark.parametrize('H', [1, 300, 512, 1000])
def test_cosine_to_mean_vs_fp64(H):
    """dot(x, mean) / (max(|x|, 1e-8) max(|mean|, 1e-8)): empty segments (0), one row, many rows, x = 0."""
    rng = np.random.default_rng(H + 1)
    counts = [0, 1, 2, 5, 0, 64, 130, 3, 1]
    n = len(counts)
    vec = rng.standard_normal((n + 2, H)).astype(np.float32)
    slots = np.arange(n) + 1
    vec[slots[3]] = 0.0                                           # x = 0
    reps = unit_rows(rng, sum(counts), H)
    off = np.concatenate([[0], np.cumsum(counts)])
    got = run_cosine(vec, slots, reps, off)
    for i, c in enumerate(counts):
        if c == 0:
            assert got[i] == 0.0
            continue
        x, m = vec[slots[i]].astype(np.float64), reps[off[i]:off[i + 1]].astype(np.float64).mean(0)
        ref = x @ m / (max(np.linalg.norm(x), 1e-8) * max(np.linalg.norm(m), 1e-8))
        assert abs(got[i] - ref) <= 1e-5, (H, c, got[i], ref)
    assert got[3] == 0.0
    # every segment empty: no class representation at all (reps = NULL)
    assert (run_cosine(vec, slots[:3], None, np.zeros(4)) == 0.0).all()


# ---------------------------------------------------------------------------------------------------------------
# grouping (stair_loss_groups): items that share a gradient slot walked in order by one workgroup

def grouped_checks(run, ref_loss, ref_d, what):
    """run(mode) -> (loss, arena gradient, *extra).  Grouped twice: matches fp64 and is bit-identical; then a launch without a
    new stair_loss_groups call (ungrouped, atomic) and one with n_groups > n (falls back to ungrouped): both match fp64."""
    a, b = run('slot'), run('slot')
    assert_losses(a[0], ref_loss, what=what)
    assert_grad(a[1], ref_d, what=what)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), what
    for mode in (None, 'too_many'):
        c = run(mode)
        assert_losses(c[0], ref_loss, what=(what, mode))
        assert_grad(c[1], ref_d, what=(what, mode))
    return a


def test_grouped_launches_vs_fp64():
    rng = np.random.default_rng(11)
    # attention: groups of 1..4 items on a slot (same K and clip inside a group), ragged clips
    T, spec = 64, []
    for g, (K, L) in enumerate([(1, 64), (2, 64), (1, 50), (2, 33), (1, 17)]):
        for r in range(1 + g % 4):
            fam = interval_families(L, rng)
            spec.append((K, [fam[(3 * r + g + k) % len(fam)][1] for k in range(K)], L))
    att, items, _ = attention_arena(spec, T, rng)
    at, shared = {}, []
    for K, ivs, L in spec:                                        # items of one (K, L) group share the first one's slot
        s = at.setdefault((K, L), items[len(shared)][0])
        shared.append((s, K, ivs, L))
    items = [shared[j] for j in rng.permutation(len(shared))]     # groups interleaved in the batch
    ref_loss, ref_d, _ = attention_ref(att, items, 0.5)
    grouped_checks(lambda mode: run_attention(att, items, T, 0.5, groups=mode), ref_loss, ref_d, 'attention')
    # heads
    for nout in (2, 1):
        H, n = 300, 400
        slots = rng.integers(0, 60, n) * 2 + 1
        vec = rng.standard_normal((122, H)).astype(np.float32) * 2
        W = (rng.standard_normal((nout, H)) / math.sqrt(H)).astype(np.float32)
        b = rng.standard_normal(nout).astype(np.float32)
        labels = rng.integers(0, 2, n)
        ref = head_ref(vec, slots, labels, W, b, 0.5)
        a = grouped_checks(lambda mode: run_head(vec, slots, labels, W, b, 0.5, groups=mode), ref[0], ref[1], ('head', nout))
        assert_grad(a[2], ref[2], what='dW')
        assert_grad(a[3], ref[3], what='db')
    # contrastive, list form
    H = 512
    G = unit_rows(rng, 300, H)
    ws, wc = np.array([0, 100, 140]), np.array([100, 40, 160])
    n = 90
    win = rng.integers(0, 3, n)
    slots = rng.integers(0, 25, n) + 2
    pos = ws[win] + rng.integers(0, 1000, n) % wc[win]
    vec = rng.standard_normal((30, H)).astype(np.float32)
    ref_loss, ref_d = np.zeros(n), np.zeros(vec.shape)
    for j in range(n):
        rl, rg = contrastive_ref(vec[slots[j]], G[ws[win[j]]:ws[win[j]] + wc[win[j]]], pos[j] - ws[win[j]], 0.5)
        ref_loss[j] = rl
        ref_d[slots[j]] += rg
    grouped_checks(lambda mode: run_contrastive(vec, slots, pos, ws[win], wc[win], G, 0.5, groups=mode), ref_loss, ref_d,
                   'contrastive')
    # contrastive, table form
    reps, presence, pools, win_row, pos_cls, vec, _ = table_case(rng, 300, 700, 3, [20, 64, 200], n)
    slots = rng.integers(0, 20, n) + 2
    ref_loss, ref_d = np.zeros(n), np.zeros(vec.shape)
    for j, w in enumerate(win_row):
        rl, rg = contrastive_ref(vec[slots[j]], reps[pools[w]], int(np.searchsorted(pools[w], pos_cls[j])), 0.5)
        ref_loss[j] = rl
        ref_d[slots[j]] += rg
    grouped_checks(lambda mode: run_table(vec, slots, pos_cls, win_row, presence, reps, 0.5, groups=mode), ref_loss, ref_d,
                   'contrastive table')
    # FilterFrame: three items on tile 1, two on tile 4 (a tile is one clip: same length inside a group)
    T, O, H = 40, 36, 128
    slots, lens = [1, 4, 1, 1, 4], [40, 29, 40, 40, 29]
    xmap, gold, W, b = filterframe_case(rng, T, O, H, lens, slots, 6)
    ref = filterframe_ref(xmap, slots, gold, lens, W, b, 0.5)
    a = grouped_checks(lambda mode: run_filterframe(xmap, slots, gold, lens, W, b, 0.5, groups=mode), ref[0], ref[1], 'filterframe')
    assert_grad(a[2], ref[2], what='dW')
    assert_grad(a[3], ref[3], what='db')
