"""The audit decoders on the GPU (csrc/audit.hip, stair_amd/audit.py) against the numpy restatement of tests/audit_ref.py: the three
launchers on raw arrays built so that every decision is an exact comparison, then audit_batch and evaluate.audit end to end.
Inputs are built once on the CPU (lru_cache) and left unchanged.

Bounds.  iou: two fp32 sums of at most 141 terms in [0, 1], each within 141 * 2^-24 = 8.4e-6 relative, so the ratio is within
twice that: 2e-5.  Head score: (H + 1) 2^-24 (sum_h |w_h v_h| + |b|) per item.  Similarities: b = 2 (H + 2) 2^-24 (unit-size
terms: a dot product of H terms and two norms)."""
import functools

import numpy as np
import pytest
import torch

import audit_ref as R
from helpers import PRETRAIN_MODULES
from stair_amd import spec, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
IOU_TOL = 2e-5
THR = 0.5
NAN = float('nan')
_d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- attention rows --------------------------------------------------------------------------------------------------------------
def _row_patterns(L):
    """rows of L frames from the value set {0.25, 0.375, 0.5, 0.75, 0.875, 1.0, NaN}: every comparison with 0.5 and between two of
    them is exact in fp32"""
    f = lambda fill: np.full(L, fill, dtype=np.float32)
    rows = {'all_off': f(0.25), 'all_on': f(0.75), 'all_nan': f(NAN)}
    a = f(0.25); a[L // 2] = 0.5; rows['at_threshold'] = a
    a = f(0.25); a[L // 3] = 0.875; a[L - 1] = 0.875; rows['two_equal_maxima'] = a
    a = f(0.75); a[0] = 1.0; rows['peak_first'] = a
    a = f(0.75); a[L - 1] = 1.0; rows['peak_last'] = a
    a = f(0.25); a[L // 3] = 0.375; rows['peak_off'] = a
    a = f(0.75); a[L // 2] = NAN; a[L - 1] = 1.0; rows['nan_splits_a_run'] = a
    a = f(NAN); a[L // 2] = 0.75; rows['one_comparable'] = a
    if L >= 7:
        a = f(0.25); a[1:3] = 0.75; a[L - 3:L - 1] = 0.75; a[L - 2] = 1.0; rows['two_runs_peak_in_second'] = a
        a = f(0.25); a[1:3] = 0.75; a[2] = 0.875; a[L - 3:L - 1] = 0.75; rows['two_runs_peak_in_first'] = a
    if L >= 71:
        a = f(0.25); a[60:71] = 0.75; a[66] = 0.875; rows['run_across_chunks_peak_right'] = a
        a = f(0.25); a[60:71] = 0.75; a[61] = 0.875; rows['run_across_chunks_peak_left'] = a
        a = f(0.75); a[63] = 0.25; a[64] = 1.0; rows['off_frame_ends_chunk'] = a
        a = f(0.75); a[64] = 0.25; a[63] = 1.0; rows['off_frame_starts_chunk'] = a
    if L >= 130:
        a = f(0.75); a[100] = 1.0; a[3] = 0.25; rows['run_over_three_chunks'] = a
    return rows


@functools.lru_cache(maxsize=None)
def _attention_case(T, ragged):
    lens_cycle = [1, T, T // 2 + 1, max(1, T - 1), min(T, 71), min(T, 130)] if ragged else [T]
    items = []                                          # (L, [row names], [rows], gold intervals or None)
    for L in sorted(set(lens_cycle)):
        pats = _row_patterns(L)
        names = sorted(pats)
        i = 0
        while i < len(names):
            k = 2 if (len(items) % 3 == 1 and i + 1 < len(names)) else 1
            golds = [None, [(0.3 * L, 0.7 * L + 0.25)] * 2, [(min(L - 1, 2) + 0.25, min(L - 1, 2) + 0.75), (-1.5, L + 3.0)],
                     [(0.0, float(L)), (L - 0.5, L - 0.25)], [(L / 3 + 0.125, L / 3 + 0.125), (0.4, 0.6)]][len(items) % 5]
            items.append((L, names[i:i + k], [pats[n] for n in names[i:i + k]], golds))
            i += k
    n = len(items)
    K = np.asarray([len(it[1]) for it in items], dtype=np.int32)
    n_rows = int(K.sum())
    rng = np.random.RandomState(T * 2 + ragged)
    # the arena: the items' rows in a shuffled order among rows nobody reads (filled with 2.0, like the frames at and beyond len)
    att = np.full((n_rows + 5, T), 2.0, dtype=np.float32)
    order = rng.permutation(n)
    slot, at = np.zeros(n, dtype=np.int32), 2
    for i in order:
        slot[i] = at
        for r, row in enumerate(items[i][2]):
            att[at + r, :items[i][0]] = row
        at += K[i]
    iv_off = np.concatenate([[0], np.cumsum(K)]).astype(np.int32)
    iv = np.zeros((n_rows, 2), dtype=np.float64)
    has = np.zeros(n, dtype=np.int32)
    want = []
    for i, (L, names, rows, golds) in enumerate(items):
        has[i] = golds is not None
        for r in range(K[i]):
            if golds is not None:
                iv[iv_off[i] + r] = golds[r]
            want.append(R.decode_attention(att[slot[i] + r], L, np.float32(THR), gold=golds[r] if golds is not None else None))
    lens = np.asarray([it[0] for it in items], dtype=np.int32)
    return dict(att=att, slot=slot, K=K, iv_off=iv_off, iv=iv, has=has, lens=lens, want=want, n_rows=n_rows,
                names=[nm for it in items for nm in it[1]])


def _check_attention(got, want, names, gold=True):
    start, end, peak, on, value, iou = [t.cpu().numpy() for t in got]
    for key, arr in (('start', start), ('end', end), ('peak', peak), ('on', on)):
        ref = np.asarray([w[key] for w in want])
        assert np.array_equal(arr, ref), (key, [(names[j], int(arr[j]), int(ref[j])) for j in np.flatnonzero(arr != ref)])
    np.testing.assert_array_equal(value, np.asarray([w['peak_value'] for w in want], dtype=np.float32))       # (NaN equals NaN here)
    ref = np.asarray([w['iou'] if gold else -1.0 for w in want])
    scored = ref >= 0
    assert np.array_equal(iou[~scored], ref[~scored])
    err = np.abs(iou[scored].astype(np.float64) - ref[scored])
    print('attention: %d rows, %d scored, max |iou - float64| = %.3g (bound %.1g)' % (ref.size, scored.sum(), err.max() if err.size else 0, IOU_TOL))
    assert (err <= IOU_TOL).all(), [(names[j], float(iou[j]), float(ref[j])) for j in np.flatnonzero(scored)[err > IOU_TOL]]


@pytest.mark.parametrize('ragged', [False, True], ids=['len_null', 'ragged'])
@pytest.mark.parametrize('T', [1, 7, 64, 65, 141])
def test_attention_rows(T, ragged):
    from stair_amd import ops
    c = _attention_case(T, ragged)
    assert set(c['K'].tolist()) == ({1, 2} if len(c['K']) > 1 else {1})
    if ragged:
        assert 1 in c['lens'] and T in c['lens']
    if T == 141:
        assert any(n.startswith('run_across_chunks') for n in c['names'])
    args = (_d(c['att']), _d(c['slot']), _d(c['K']), _d(c['iv_off']), c['n_rows'], THR)
    lens = _d(c['lens']) if ragged else None
    got = ops.audit_attention(*args, lens=lens, intervals=_d(c['iv']), has_gold=_d(c['has']))
    torch.cuda.synchronize()
    _check_attention(got, c['want'], c['names'])
    assert c['has'].min() == 0 and c['has'].max() == 1
    # no gold at all (intervals NULL): the same decode, every iou -1; the outputs are stored anew (pre-filled with garbage)
    out = [torch.full((c['n_rows'],), 77, dtype=torch.int32, device=DEV) for _ in range(4)] + [torch.full((c['n_rows'],), 77.0, device=DEV) for _ in range(2)]
    ops.audit_attention(*args, lens=lens, out=out)
    torch.cuda.synchronize()
    _check_attention(out, c['want'], c['names'], gold=False)


# ---- heads -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _head_case(H, nout):
    rng = np.random.RandomState(100 * nout + H)
    n = 41
    W = (rng.uniform(-1, 1, (nout, H)) / np.sqrt(H)).astype(np.float32)
    b = np.asarray([0.125, 0.125] if nout == 2 else [0.5], dtype=np.float32)
    point = 0.0 if nout == 2 else 0.5
    vec = rng.uniform(-1, 1, (n + 4, H)).astype(np.float32)
    slot = (rng.permutation(n) + 2).astype(np.int32)
    vec[slot[0]] = 0.0                                   # z1 == z0 exactly (nout 2: pred 0) / score exactly 0.5 (nout 1: pred 1)
    for i in range(1, n):                                # every other margin beyond 1e-3: rows are redrawn until theirs is
        while abs(R.head_score(vec[slot[i]], W, b) - point) <= 1e-3:
            vec[slot[i]] = rng.uniform(-1, 1, H).astype(np.float32)
    label = np.asarray([(-1, 0, 1)[i % 3] for i in range(n)], dtype=np.int32)
    score64 = np.asarray([R.head_score(vec[s], W, b) for s in slot])
    bound = np.asarray([R.head_bound(vec[s], W, b) for s in slot])
    return dict(W=W, b=b, vec=vec, slot=slot, label=label, score64=score64, bound=bound, point=point)


def _check_head(pred, score, correct, score64, bound, label, nout):
    err = np.abs(score.astype(np.float64) - score64)
    print('head nout=%d: %d items, max |score - float64| / bound = %.3g' % (nout, score.size, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all(), (err.max(), bound[np.argmax(err)])
    assert np.array_equal(pred, np.asarray([R.head_pred(s, nout) for s in score]))                  # the decision of the returned score
    want = np.where(label < 0, -1, (pred == (label != 0)).astype(np.int32))
    assert np.array_equal(correct, want)


@pytest.mark.parametrize('nout', [1, 2])
@pytest.mark.parametrize('H', [64, 512])
def test_head_items(H, nout):
    from stair_amd import ops
    c = _head_case(H, nout)
    margin = np.abs(c['score64'] - c['point'])
    assert margin[0] == 0.0 and (margin[1:] > 1e-3).all()             # asserted before the launch, no item left out
    pred, score, correct = [t.cpu().numpy() for t in ops.audit_head(_d(c['vec']), _d(c['slot']), _d(c['W']), _d(c['b']), label=_d(c['label']))]
    _check_head(pred, score, correct, c['score64'], c['bound'], c['label'], nout)
    assert np.array_equal(pred, np.asarray([R.head_pred(s, nout) for s in c['score64']]))       # the float64 decision, every item
    assert score[0] == c['point'] and pred[0] == (0 if nout == 2 else 1)
    assert set(correct.tolist()) == {-1, 0, 1}
    # zero weights: every item ties (nout 2: class 0) or sits on the bias
    p0, s0, c0 = [t.cpu().numpy() for t in ops.audit_head(_d(c['vec']), _d(c['slot'][:5]), _d(np.zeros_like(c['W'])), _d(c['b']))]
    assert (s0 == c['point']).all() and (p0 == (0 if nout == 2 else 1)).all() and (c0 == -1).all()


# ---- ranks -----------------------------------------------------------------------------------------------------------------------
RANK_SHAPES = [(1, 64), (5, 64), (65, 64), (214, 512), (214, 320)]
sim_bound = lambda H: 2.0 * (H + 2) * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _constructed_table(n_cls, H):
    """orthonormal queries and unit keys with prescribed coordinates along them: sim(query i, class c) = A[c, i] up to rounding, the
    values of a query pairwise 3e-3 (1e-2 for small tables) apart; one class is a bit-identical copy of another"""
    rng = np.random.RandomState(n_cls * 7 + H)
    nq = 6
    basis = np.linalg.qr(rng.normal(size=(H, nq + 1)))[0].T                # [nq + 1, H] orthonormal rows; the last carries the remainder
    step = 3e-3 if n_cls > 100 else 1e-2
    A = np.stack([(rng.permutation(n_cls) - (n_cls - 1) / 2.0) * step for _ in range(nq)], axis=1)      # [n_cls, nq]
    rest = np.sqrt(1.0 - (A * A).sum(axis=1))
    keys = (A @ basis[:nq] + rest[:, None] * basis[nq]).astype(np.float32)
    copy_of = None
    if n_cls >= 5:
        copy_of = (n_cls - 2, 1)                         # class n_cls - 2 becomes a copy of class 1
        keys[copy_of[0]] = keys[copy_of[1]]
    queries = np.concatenate([(basis[:nq] * np.asarray([1.0, 0.5, 2.0, 1.0, 3.0, 0.25])[:, None]), np.zeros((1, H))]).astype(np.float32)
    sims = np.stack([R.cosine_sims(q, keys) for q in queries])            # float64, of the fp32 arrays
    # items: (query, gold classes)
    items = []
    for qi in range(nq):
        order = np.argsort(-sims[qi], kind='stable')
        best, worst = int(order[0]), int(order[-1])
        golds = [[], [best], [worst], [worst, int(order[len(order) // 2])]]
        if copy_of:
            golds += [[copy_of[1]], [copy_of[0]], [copy_of[0], worst]]
        for g in golds:
            items.append((qi, sorted(set(g))))
    items += [(nq, []), (nq, [n_cls - 1])]                # the zero query
    n = len(items)
    vec = rng.normal(size=(n + 3, H)).astype(np.float32)
    slot = (rng.permutation(n) + 1).astype(np.int32)
    for j, (qi, _) in enumerate(items):
        vec[slot[j]] = queries[qi]
    gold_off = np.concatenate([[0], np.cumsum([len(g) for _, g in items])]).astype(np.int32)
    gold_cls = np.asarray([c for _, g in items for c in g], dtype=np.int32)
    return dict(keys=keys, vec=vec, slot=slot, items=items, sims=sims, gold_off=gold_off, gold_cls=gold_cls, copy_of=copy_of, nq=nq)


def _assert_separated(c):
    """every query's float64 similarities pairwise >= 1e-3 apart, the deliberate copy (bit-identical rows) apart; the zero query's are all 0"""
    keys = c['keys']
    for qi in range(c['nq']):
        s = c['sims'][qi]
        order = np.argsort(s)
        for a, b in zip(order[:-1], order[1:]):
            if np.array_equal(keys[a], keys[b]):
                assert s[a] == s[b]
            else:
                assert s[b] - s[a] >= 1e-3, (qi, a, b, s[a], s[b])
    assert (c['sims'][c['nq']] == 0).all()


@pytest.mark.parametrize('n_cls,H', RANK_SHAPES)
def test_rank_on_a_constructed_table(n_cls, H):
    from stair_amd import ops
    c = _constructed_table(n_cls, H)
    _assert_separated(c)                                 # on the CPU, before the launch, no item left out
    gold = dict(gold_off=_d(c['gold_off']), gold_cls=_d(c['gold_cls']) if c['gold_cls'].size else None, gold_cls_host=c['gold_cls'])
    for k in sorted({min(5, n_cls), n_cls}):
        top, top_sim, rank, best = [t.cpu().numpy() for t in ops.audit_rank(_d(c['vec']), _d(c['slot']), _d(c['keys']), k, **gold)]
        for j, (qi, g) in enumerate(c['items']):
            want = R.decode_rank(c['sims'][qi], k, g)
            assert top[j].tolist() == want['top'], (j, qi, g, top[j].tolist(), want['top'])
            assert rank[j] == want['rank'], (j, qi, g, rank[j], want['rank'])
            assert np.abs(top_sim[j] - np.asarray(want['top_sim'])).max() <= sim_bound(H)
            if g:
                assert abs(best[j] - want['best_gold_sim']) <= sim_bound(H)
            else:
                assert best[j] == -np.inf
        zero = [j for j, (qi, _) in enumerate(c['items']) if qi == c['nq']]
        assert [rank[j] for j in zero] == [0, 1] and all(top[j].tolist() == list(range(k)) and (top_sim[j] == 0).all() for j in zero)
    if c['copy_of']:                                     # the gold row's copy elsewhere in the table does not worsen the rank
        by_gold = {tuple(g): rank[j] for j, (qi, g) in enumerate(c['items']) if qi == 0}
        assert by_gold[(c['copy_of'][0],)] == by_gold[(c['copy_of'][1],)]
    # no gold at all (gold_off NULL): the same lists, rank 0
    top2, _, rank2, _ = [t.cpu().numpy() for t in ops.audit_rank(_d(c['vec']), _d(c['slot']), _d(c['keys']), n_cls)]
    assert np.array_equal(top2, top) and (rank2 == 0).all()


def _check_rank_with_tolerance(top, top_sim, rank, best, sims64, golds, H):
    """the tolerance-aware checks of a rank launch against float64 similarities sims64 [n, n_cls]; nothing is left out"""
    b = sim_bound(H)
    n, k = top.shape
    worst = 0.0
    for j in range(n):
        s = sims64[j]
        assert len(set(top[j].tolist())) == k and (top[j] >= 0).all() and (top[j] < s.size).all()
        err = np.abs(top_sim[j].astype(np.float64) - s[top[j]])
        worst = max(worst, float(err.max()))
        assert (err <= b).all(), (j, err.max(), b)
        assert (np.diff(top_sim[j]) <= 0).all()                                            # best first
        others = np.setdiff1d(np.arange(s.size), top[j])
        assert (s[others] <= float(top_sim[j][-1]) + 2 * b).all()                          # nothing better was passed over
        if len(golds[j]):
            g = max(s[c] for c in golds[j])
            assert 1 + int((s > g + 2 * b).sum()) <= rank[j] <= 1 + int((s > g - 2 * b).sum()), (j, rank[j])
            assert abs(best[j] - g) <= b
        else:
            assert rank[j] == 0
    return worst


@pytest.mark.parametrize('n_cls,H', RANK_SHAPES)
def test_rank_on_a_random_table(n_cls, H):
    from stair_amd import ops
    rng = np.random.RandomState(n_cls + H)
    n = 37
    keys = rng.normal(size=(n_cls, H)).astype(np.float32)
    vec = rng.normal(size=(n + 2, H)).astype(np.float32)
    slot = (rng.permutation(n) + 1).astype(np.int32)
    golds = [sorted(set(rng.randint(0, n_cls, size=j % 3).tolist())) for j in range(n)]
    gold_off = np.concatenate([[0], np.cumsum([len(g) for g in golds])]).astype(np.int32)
    gold_cls = np.asarray([c for g in golds for c in g], dtype=np.int32)
    sims64 = np.stack([R.cosine_sims(vec[s], keys) for s in slot])
    k = min(5, n_cls)
    out = [t.cpu().numpy() for t in ops.audit_rank(_d(vec), _d(slot), _d(keys), k, gold_off=_d(gold_off), gold_cls=_d(gold_cls), gold_cls_host=gold_cls)]
    worst = _check_rank_with_tolerance(*out, sims64, golds, H)
    print('rank %d x %d: max |sim - float64| = %.3g (bound %.3g)' % (n_cls, H, worst, sim_bound(H)))
    # the similarities and the order are stair_cosine_topk's
    idx, sim = ops.cosine_topk(_d(vec), _d(keys), k, q_idx=_d(slot))
    assert np.array_equal(idx.cpu().numpy(), out[0]) and np.array_equal(sim.cpu().numpy(), out[1])


# ---- end to end ------------------------------------------------------------------------------------------------------------------
TINY = dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, answer_vocab_length=16, object_types=10, have_pretrain_head=True)


@functools.lru_cache(maxsize=None)
def _model(H, max_len):
    from stair_amd.module_net import VideoNMN
    config = dict(TINY, max_video_length=max_len) if H == 64 else dict(spec.DEFAULT_CONFIG, max_video_length=max_len, have_pretrain_head=True)
    w = synth.make_weights(config, 11)
    model = VideoNMN(config, pretrain_modules=set(PRETRAIN_MODULES))
    model.load_state_dict({k: torch.from_numpy(w[k].copy()) for k in spec.state_dict_keys(config)})
    return model.to(DEV)


@functools.lru_cache(maxsize=None)
def _questions(H, max_len, frames, n_gold, n_plain):
    """n_gold questions over the twelve forms with synthetic gold, then n_plain without sg_res_by_step; frames: T or a tuple cycled"""
    config = _model(H, max_len).config
    qs = []
    for i in range(n_gold + n_plain):
        T = frames[i % len(frames)] if isinstance(frames, tuple) else frames
        q = synth.make_question(config, 5, i, form=synth.ALL_FORMS[i % 12], T=T)
        if i < n_gold:
            q['sg_res_by_step'] = synth.make_gold(config, 9, q, T=T)
        q['video_id'] = 'clip%d' % i
        qs.append(q)
    return qs


@functools.lru_cache(maxsize=None)
def _table(H, max_len, frames, n_gold, n_plain):
    from stair_amd import losses
    return losses.ClassTable.from_questions(_questions(H, max_len, frames, n_gold, n_plain))


def _audit_and_check(model, qs, table):
    from stair_amd import audit, losses, ops
    H, top = model.config['hidden_size'], 5
    res = model.forward_batch(qs)
    logits, pred = res.logits.clone(), res.pred.clone()
    batch = audit.audit_batch(model, res, qs, class_table=table, threshold=THR, top=top)
    assert batch._fetched is None                         # nothing has come to the host yet
    T = res.info.T
    frames = res.question_frames
    # the node set: supervised_nodes' for every question
    want_nodes = {(qi, step) for qi, q in enumerate(qs) for step, i in losses.supervised_nodes(q, model.pretrain_modules).items()
                  if q['nmn_program_list'][i] in audit.AUDITED}
    got_nodes = set(zip(batch.att_q.tolist(), batch.att_idx.tolist())) | set(zip(batch.head_q.tolist(), batch.head_idx.tolist())) | \
        set(zip(batch.cont_q.tolist(), batch.cont_idx.tolist()))
    assert got_nodes == want_nodes and len(want_nodes) > len(qs)
    assert batch.att_q.size + batch.head_q.size + batch.cont_q.size == len(want_nodes) + int((batch.att_row > 0).sum())
    gold_of = lambda qi, step: (qs[qi].get('sg_res_by_step') or {}).get(step)
    # attention rows from the values res.related_attn / res.node hand out
    want, names = [], []
    for r in range(batch.att_q.size):
        qi, pos, step, row = int(batch.att_q[r]), int(batch.att_pos[r]), int(batch.att_idx[r]), int(batch.att_row[r])
        module = qs[qi]['nmn_program_list'][pos]
        assert module == audit.ATTENTION[batch.att_module[r]]
        values = res.related_attn(qi, pos) if module == 'Temporal' else res.node(qi, pos).reshape(-1, T)[row]
        g = gold_of(qi, step)
        g = None if g is None else (tuple(g[row]) if module == 'Localize' else tuple(g))
        want.append(R.decode_attention(values.cpu().numpy(), int(frames[qi]) if frames is not None else T, np.float32(THR), gold=g))
        names.append('%s q%d pos%d row%d' % (module, qi, pos, row))
    _check_attention([torch.from_numpy(np.asarray(getattr(batch, f))) for f in ('start', 'end', 'peak', 'on', 'peak_value', 'iou')], want, names)
    # heads
    score64, bound, labels = [], [], []
    for i in range(batch.head_q.size):
        qi, pos, step = int(batch.head_q[i]), int(batch.head_pos[i]), int(batch.head_idx[i])
        module = audit.HEADS[batch.head_module[i]]
        assert module == qs[qi]['nmn_program_list'][pos]
        head = model.submodules[module].pretrain_head
        x, W, b = res.node(qi, pos).cpu().numpy(), head.weight.detach().cpu().numpy(), head.bias.detach().cpu().numpy()
        score64.append(R.head_score(x, W, b)); bound.append(R.head_bound(x, W, b))
        g = gold_of(qi, step)
        labels.append(-1 if g is None else int(bool(g)))
    score64, bound, labels = np.asarray(score64), np.asarray(bound), np.asarray(labels, dtype=np.int32)
    assert np.array_equal(batch.label, labels)
    for code, nout in ((0, 2), (1, 2), (2, 1)):
        m = batch.head_module == code
        if m.any():
            _check_head(batch.pred[m], batch.score[m], batch.correct[m], score64[m], bound[m], labels[m], nout)
            point = 0.0 if nout == 2 else 0.5
            sure = np.abs(score64[m] - point) > bound[m]                                   # the float64 decision wherever rounding cannot turn it
            assert np.array_equal(batch.pred[m][sure], np.asarray([R.head_pred(s, nout) for s in score64[m]])[sure])
    # ranks against the encoded table of the same run
    if batch.cont_q.size:
        x, seq_off, max_len = table.device_rows(torch.device(DEV), model.config['text_size'])
        with torch.no_grad():
            reps = ops.l2normalize(ops.lstm_bidir(x, seq_off, max_len, [w.detach() for w in model._lstm_weights('text_encoder')])[1]).cpu().numpy()
        sims64, golds = [], []
        for i in range(batch.cont_q.size):
            qi, pos, step = int(batch.cont_q[i]), int(batch.cont_pos[i]), int(batch.cont_idx[i])
            assert audit.CONTRASTIVE[batch.cont_module[i]] == qs[qi]['nmn_program_list'][pos]
            sims64.append(R.cosine_sims(res.node(qi, pos).cpu().numpy(), reps))
            g = gold_of(qi, step)
            golds.append([] if g is None else sorted(table.index[name] for name, _ in g))
            assert batch.gold_cls[batch.gold_off[i]: batch.gold_off[i + 1]].tolist() == [table.index[name] for name, _ in (g or [])]
        assert batch.top.shape == (batch.cont_q.size, min(top, len(table)))
        _check_rank_with_tolerance(batch.top, batch.top_sim, batch.rank, batch.best_gold_sim, np.stack(sims64), golds, H)
    # the ungolded questions are decoded and not scored
    plain = np.asarray(['sg_res_by_step' not in q for q in qs])
    assert plain.sum() == 4
    assert (batch.iou[plain[batch.att_q]] == -1).all() and plain[batch.att_q].any() and (batch.peak[plain[batch.att_q]] >= 0).all()
    assert (batch.correct[plain[batch.head_q]] == -1).all() and plain[batch.head_q].any()
    assert (batch.rank[plain[batch.cont_q]] == 0).all() and plain[batch.cont_q].any() and (batch.top[plain[batch.cont_q]] >= 0).all()
    assert (batch.iou >= 0).any() and (batch.correct >= 0).any() and (batch.rank > 0).any()
    # the pass itself is untouched
    assert torch.equal(res.logits, logits) and torch.equal(res.pred, pred)
    recs = batch.records(qs, table)
    assert set(recs) == {q['qa_id'] for q in qs} and sum(len(v) for v in recs.values()) == len(want_nodes)
    return batch


# Clips of 24 frames, equal and ragged, run at max_video_length 40: a configuration of max_video_length <= 32 has Linear(T, T)
# relate nets and admits only clips of exactly max_video_length frames, so it cannot hold a ragged batch; 24 and 8 are such
# configurations (8: packed tiles) and run with equal clips.
@pytest.mark.parametrize('max_len,frames', [(40, 24), (40, (24, 9, 17, 3, 24, 13)), (24, 24), (8, 8)],
                         ids=['equal', 'ragged', 'linear_temporal_24', 'linear_temporal_8'])
def test_audit_batch_end_to_end(max_len, frames):
    args = (64, max_len, frames, 24, 4)
    qs = _questions(*args)
    batch = _audit_and_check(_model(64, max_len), qs, _table(*args))
    assert not batch.skipped


def test_audit_batch_on_the_fused_tile_path():
    args = (512, 64, 64, 20, 4)
    _audit_and_check(_model(512, 64), _questions(*args), _table(*args))


def _from_records(records, top):
    """report recomputed from the rendered records"""
    from stair_amd import audit
    vals = {}
    for per_q in records.values():
        for node in per_q.values():
            m = node['module']
            if m in audit.ATTENTION:
                vals.setdefault(m, ('attention', []))[1].extend([-1.0] * len(node['interval']) if node['iou'] is None else node['iou'])
            elif m in audit.HEADS:
                vals.setdefault(m, ('head', []))[1].append(-1 if node['correct'] is None else int(node['correct']))
            else:
                vals.setdefault(m, ('contrastive', []))[1].append(0 if node['rank'] is None else node['rank'])
    return {m: audit.module_report(kind, v, top=top) for m, (kind, v) in vals.items()}


def _same_report(a, b):
    assert set(a) == set(b)
    for m in a:
        if m == 'skipped':
            assert a[m] == b[m]
            continue
        assert set(a[m]) == set(b[m])
        for key in a[m]:
            x, y = a[m][key], b[m][key]
            assert x == y or (np.isnan(x) and np.isnan(y)), (m, key, x, y)


def test_evaluate_audit():
    from stair_amd import audit, evaluate as E
    from stair_amd.clip_library import ClipLibrary
    args = (64, 40, (24, 9, 17, 3, 24, 13), 24, 4)
    model, qs, table = _model(64, 40), _questions(*args), _table(*args)
    unk = 15
    acc, report, records = E.audit(model, qs, unk, class_table=table, batch_size=1024, records=True)
    assert acc == E.evaluate(model, qs, unk, batch_size=1024)[0]
    from stair_amd import losses
    present = {q['nmn_program_list'][i] for q in qs for i in losses.supervised_nodes(q, model.pretrain_modules).values()} & audit.AUDITED
    assert {'Localize', 'Temporal', 'ExistsFrame', 'Exists', 'Equals', 'Filter', 'ToAction'} <= present     # (Xor and Superlative only ever stand at the root)
    assert set(report) == present and all(r['n'] > 0 and r['n_scored'] > 0 for r in report.values())
    _same_report(_from_records(records, 5), report)         # (the records hold a module's nodes in the order of its arrays)
    # the batch size does not show
    acc5, report5, records5 = E.audit(model, qs, unk, class_table=table, batch_size=5, records=True)
    assert acc5 == acc and records5 == records
    _same_report(report5, report)
    # nor does the source of the clips
    clips = [torch.as_tensor(q['video_features']) for q in qs]
    ids = [q['video_id'] for q in qs]
    bare = [{k: v for k, v in q.items() if k != 'video_features'} for q in qs]
    cache = model.encode_clips(clips, ids=ids)
    acc_c, report_c, records_c = E.audit(model, bare, unk, class_table=table, batch_size=7, records=True, clip_cache=cache)
    cap = max(c.shape[0] for c in clips)
    padded = torch.zeros(len(clips), cap, clips[0].shape[1])
    for r, c in enumerate(clips):
        padded[r, :c.shape[0]] = c
    library = ClipLibrary(cap, clips[0].shape[1], DEV, torch.float32)
    library.add(padded, ids=ids, video_len=[int(c.shape[0]) for c in clips])
    acc_l, report_l, records_l = E.audit(model, bare, unk, class_table=table, batch_size=7, records=True, clip_library=library)
    assert acc_c == acc and acc_l == acc and records_c == records and records_l == records
    _same_report(report_c, report); _same_report(report_l, report)
    # without a class table the contrastive modules are absent and reported as skipped
    acc_n, report_n = E.audit(model, qs, unk, batch_size=1024)
    assert acc_n == acc and set(report_n) == (present - set(audit.CONTRASTIVE)) | {'skipped'}
    assert report_n['skipped'] == {m: report[m]['n'] for m in present & set(audit.CONTRASTIVE)} and report_n['skipped']
    for m in present - set(audit.CONTRASTIVE):
        _same_report({m: report_n[m]}, {m: report[m]})
