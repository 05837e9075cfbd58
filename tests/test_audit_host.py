"""Host side of the audit pass (stair_amd/audit.py, csrc/audit.hip), no GPU: hand-worked cases of the numpy restatement the GPU
tests compare against (tests/audit_ref.py), the three entry points bound, every argument set the launchers refuse -- on the host,
before anything is enqueued, with its whole message in stair_last_error (the addresses are fake, non-null and 16-byte aligned;
nothing dereferences them) -- and the refusals of audit_batch that need no device."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import audit_ref as R
from helpers import PRETRAIN_MODULES, build_plan
from stair_amd import _lib, audit, losses, spec, synth
from stair_amd._lib import PlanInfo, check, lib

P = [0x10000 + 0x100 * i for i in range(16)]        # fake device addresses
NAN = float('nan')


# ---- the restatement itself ------------------------------------------------------------------------------------------------------
def test_restatement_attention_by_hand():
    f = lambda *v: np.asarray(v, dtype=np.float32)
    d = R.decode_attention(f(0.1, 0.6, 0.7, 0.6, 0.2, 0.9), 6, 0.5)
    assert (d['start'], d['end'], d['peak'], d['on'], d['iou']) == (5, 6, 5, 4, -1.0) and d['peak_value'] == np.float32(0.9)
    # two equal maxima: the first wins, and its run is reported
    d = R.decode_attention(f(0.1, 0.8, 0.7, 0.2, 0.8, 0.8), 6, 0.5)
    assert (d['start'], d['end'], d['peak'], d['on']) == (1, 3, 1, 4)
    # the value equal to the threshold is on; frames at and beyond L are not seen
    d = R.decode_attention(f(0.5, 0.5, 0.25, 2.0, 2.0), 3, 0.5)
    assert (d['start'], d['end'], d['peak'], d['on']) == (0, 2, 0, 2)
    # peak frame off: the empty interval at the peak; all NaN: no peak
    d = R.decode_attention(f(0.1, 0.3, 0.2), 3, 0.5)
    assert (d['start'], d['end'], d['peak'], d['on']) == (1, 1, 1, 0)
    d = R.decode_attention(f(NAN, NAN), 2, 0.5)
    assert (d['start'], d['end'], d['peak'], d['on']) == (0, 0, -1, 0) and np.isnan(d['peak_value'])
    # a NaN frame splits a run and is never the peak
    d = R.decode_attention(f(0.9, NAN, 0.95, 0.9), 4, 0.5)
    assert (d['start'], d['end'], d['peak'], d['on']) == (2, 4, 2, 3)


def test_restatement_iou_by_hand():
    # span_to_attention of (1.5, 3.25) on 6 frames: frame 1 gets 0.5, frame 2 gets 1, frame 3 gets 0.25
    g = R.span_mask(1.5, 3.25, 6)
    assert np.allclose(g, [0, 0.5, 1, 0.25, 0, 0], atol=1e-12)
    row = np.asarray([0, 0, 0.9, 0.8, 0, 0], dtype=np.float32)            # decoded [2, 4)
    d = R.decode_attention(row, 6, 0.5, gold=(1.5, 3.25))
    assert (d['start'], d['end']) == (2, 4) and abs(d['iou'] - 1.25 / 2.5) < 1e-12
    # an interval inside one frame: everything in frame floor(end)
    assert np.allclose(R.span_mask(2.25, 2.75, 6), [0, 0, 0.5, 0, 0, 0], atol=1e-12)
    # empty decoded interval against a gold: 0; no decoded frame and an (almost) empty gold: denominator > 0 still
    assert R.decode_attention(np.asarray([0.1, 0.2], dtype=np.float32), 2, 0.5, gold=(0.0, 2.0))['iou'] == 0.0


def test_restatement_head_and_rank_by_hand():
    W = np.asarray([[1, 0], [0, 2]], dtype=np.float32); b = np.asarray([0.5, 0.25], dtype=np.float32)
    assert R.head_score([1, 1], W, b) == 2.25 - 1.5 and R.head_pred(0.75, 2) == 1
    assert R.head_pred(0.0, 2) == 0 and R.head_pred(0.5, 1) == 1 and R.head_pred(0.4999, 1) == 0
    assert R.head_score([2, 3], W[:1], b[:1]) == 2.5
    sims = np.asarray([0.1, 0.9, 0.9, -0.2, 0.5])
    d = R.decode_rank(sims, 3, [4])
    assert d['top'] == [1, 2, 4] and d['rank'] == 3 and d['best_gold_sim'] == 0.5
    assert R.decode_rank(sims, 2, [2, 3])['rank'] == 1            # the best of the gold classes counts; the identical row 1 is not better
    assert R.decode_rank(sims, 5, [])['rank'] == 0 and R.decode_rank(sims, 5, [])['top'] == [1, 2, 4, 0, 3]
    assert np.allclose(R.cosine_sims([0, 0], [[1, 0], [0, 1]]), [0, 0])
    assert np.allclose(R.cosine_sims([3, 4], [[1, 0], [0, 2]]), [0.6, 0.8])


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_the_three_entry_points_are_bound():
    bound = {name for name, _, _ in _lib.SIGNATURES}
    for name in ('stair_audit_attention', 'stair_audit_head', 'stair_audit_rank'):
        assert name in bound and hasattr(lib, name)
    assert lib.stair_abi_version() == 7


ATT = dict(att=P[0], att_rows=8, slot=P[1], K=P[2], len=None, iv_off=P[3], intervals=None, has_gold=None, n=3, T=24, threshold=0.5,
           start=P[4], end=P[5], peak=P[6], on=P[7], peak_value=P[8], iou=P[9])
HEAD = dict(nout=2, vec=P[0], vec_rows=8, slot=P[1], label=None, W=P[2], b=P[3], n=3, H=64, pred=P[4], score=P[5], correct=P[6])
GOLD_OK = np.asarray([0, 4, 2], dtype=np.int32)
RANK = dict(vec=P[0], vec_rows=8, slot=P[1], reps=P[2], n_cls=5, H=64, gold_off=P[3], gold_cls=P[4], gold_cls_host=None, n_gold=0,
            n=3, k=2, top=P[5], top_sim=P[6], rank=P[7], best_gold_sim=P[8])


def _call(fn, fields):
    args = [C.c_float(v) if k == 'threshold' else (v.ctypes.data if isinstance(v, np.ndarray) else v) for k, v in fields.items()]
    return fn(*args, None)


REFUSED = [
    ('att_T0', 'stair_audit_attention', dict(ATT, T=0), 'T must be at least 1'),
    ('att_nan_threshold', 'stair_audit_attention', dict(ATT, threshold=NAN), 'the threshold is NaN'),
    ('att_negative_n', 'stair_audit_attention', dict(ATT, n=-1), 'n must not be negative'),
    ('att_null_att', 'stair_audit_attention', dict(ATT, att=None), 'null att arena'),
    ('att_null_slot', 'stair_audit_attention', dict(ATT, slot=None), 'null slot / K / iv_off'),
    ('att_null_iv_off', 'stair_audit_attention', dict(ATT, iv_off=None), 'null slot / K / iv_off'),
    ('att_null_output', 'stair_audit_attention', dict(ATT, peak_value=None), 'null output'),
    ('att_null_iou', 'stair_audit_attention', dict(ATT, iou=None), 'null output'),
    ('head_nout0', 'stair_audit_head', dict(HEAD, nout=0), 'head width must be 1 (Equals) or 2 (Exists/Xor)'),
    ('head_nout3', 'stair_audit_head', dict(HEAD, nout=3), 'head width must be 1 (Equals) or 2 (Exists/Xor)'),
    ('head_H0', 'stair_audit_head', dict(HEAD, H=0), 'H must be at least 1'),
    ('head_null_vec', 'stair_audit_head', dict(HEAD, vec=None), 'null vec arena'),
    ('head_null_slot', 'stair_audit_head', dict(HEAD, slot=None), 'null slot / W / b'),
    ('head_null_weight', 'stair_audit_head', dict(HEAD, W=None), 'null slot / W / b'),
    ('head_null_output', 'stair_audit_head', dict(HEAD, score=None), 'null output'),
    ('rank_k0', 'stair_audit_rank', dict(RANK, k=0), 'k must be in 1..n_cls'),
    ('rank_k_above_table', 'stair_audit_rank', dict(RANK, k=6), 'k must be in 1..n_cls'),
    ('rank_no_classes', 'stair_audit_rank', dict(RANK, n_cls=0), 'the class table is empty'),
    ('rank_too_many_classes', 'stair_audit_rank', dict(RANK, n_cls=1025), 'at most 1024 classes'),
    ('rank_gold_above_table', 'stair_audit_rank', dict(RANK, gold_cls_host=np.asarray([0, 5, 2], dtype=np.int32), n_gold=3),
     'gold class 5 (entry 1) is outside the table of 5 classes'),
    ('rank_gold_negative', 'stair_audit_rank', dict(RANK, gold_cls_host=np.asarray([0, 4, -1], dtype=np.int32), n_gold=3),
     'gold class -1 (entry 2) is outside the table of 5 classes'),
    ('rank_null_vec', 'stair_audit_rank', dict(RANK, gold_cls_host=GOLD_OK, n_gold=3, vec=None), 'null vec arena'),
    ('rank_null_slot', 'stair_audit_rank', dict(RANK, slot=None), 'null slot / reps'),
    ('rank_null_reps', 'stair_audit_rank', dict(RANK, reps=None), 'null slot / reps'),
    ('rank_gold_off_alone', 'stair_audit_rank', dict(RANK, gold_cls=None, n_gold=3), 'gold_off without gold_cls'),
    ('rank_null_output', 'stair_audit_rank', dict(RANK, rank=None), 'null output'),
    ('rank_unaligned', 'stair_audit_rank', dict(RANK, reps=0x20004), 'vec and reps must be 16-byte aligned'),
]


@pytest.mark.parametrize('name,fields,message', [pytest.param(*c[1:], id=c[0]) for c in REFUSED])
def test_refused_before_any_launch_with_its_message(name, fields, message):
    assert _call(getattr(lib, name), fields) != 0
    assert lib.stair_last_error().decode() == '%s: %s' % (name, message)


@pytest.mark.parametrize('name,fields', [('stair_audit_attention', ATT), ('stair_audit_head', HEAD), ('stair_audit_rank', RANK)])
def test_no_items_is_no_launch(name, fields):
    """n == 0 returns 0 whatever the pointers: nothing is enqueued (there is no device here to enqueue on)"""
    null = {k: None for k, v in fields.items() if isinstance(v, int) and v >= 0x10000}
    assert _call(getattr(lib, name), dict(fields, n=0, **null)) == 0


# ---- audit_batch, the refusals that need no device ------------------------------------------------------------------------------
TINY = dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, answer_vocab_length=16, max_video_length=24, object_types=10)


class _HostResult:
    """What audit_batch reads of a BatchResult before it touches the device, from a plan built on the host"""

    def __init__(self, config, questions, T):
        self.ctx, self.plan, rc, self._prog_off = build_plan(config, [q['nmn_program_list'] for q in questions],
                                                             [q['prog_str_to_question_tokens'] for q in questions],
                                                             [q['question'].shape[0] for q in questions], T)
        assert rc == 0, lib.stair_last_error()
        self.info = PlanInfo()
        check(lib.stair_plan_get_info(self.plan, C.byref(self.info)))
        self.pred = types.SimpleNamespace(device=torch.device('cpu'))
        self.question_frames = None

    def node_table(self):
        tab = tuple(np.empty(self.info.n_nodes, dtype=np.int32) for _ in range(5))
        check(lib.stair_plan_nodes(self.plan, *[t.ctypes.data_as(C.POINTER(C.c_int32)) for t in tab], self.info.n_nodes))
        return tab

    def close(self):
        lib.stair_plan_destroy(self.plan)
        lib.stair_ctx_destroy(self.ctx)


def _host_case(config, forms, gold):
    from stair_amd.module_net import VideoNMN
    qs = [synth.make_question(config, 0, i, form=f, with_video=False) for i, f in enumerate(forms)]
    for q in qs:
        q['sg_res_by_step'] = gold(q)
    return VideoNMN(config, pretrain_modules=PRETRAIN_MODULES), qs, _HostResult(config, qs, config['max_video_length'])


def _gold_for(q, module, value):
    prog, idx = q['nmn_program_list'], q['nmn_program_idx']
    return {idx[i]: value for i in range(1, len(prog)) if prog[i] == module and idx[i] is not None}


def test_audit_batch_refuses_a_head_module_without_pretrain_heads():
    model, qs, res = _host_case(dict(TINY, have_pretrain_head=False), ['P0', 'P1'], lambda q: {})
    try:
        with pytest.raises(RuntimeError, match=r'Exists loss needs have_pretrain_head \(modules.py\)'):
            audit.audit_batch(model, res, qs)
    finally:
        res.close()


def test_audit_batch_refuses_a_gold_class_the_table_does_not_hold():
    emb = lambda c: synth.class_embedding(TINY, 0, c)
    model, qs, res = _host_case(TINY, ['P1', 'P4'], lambda q: _gold_for(q, 'Filter', [('class_7', emb(7))]))
    table = losses.ClassTable(['class_1', 'class_2'], [emb(1), emb(2)])
    try:
        with pytest.raises(KeyError, match=r"class 'class_7' is not in the ClassTable \(build it from the whole dataset: ClassTable.from_questions\)"):
            audit.audit_batch(model, res, qs, class_table=table)
    finally:
        res.close()


def test_audit_batch_refuses_a_gold_end_the_criterion_cannot_index():
    model, qs, res = _host_case(TINY, ['P1', 'P6'], lambda q: _gold_for(q, 'Temporal', (2.0, -30.0)))
    try:
        with pytest.raises(ValueError, match=r'Temporal at program position 4 of question 1: gold interval end -30.0 lies before the first '
                                             r'frame of its 24-frame clip'):
            audit.audit_batch(model, res, qs)
    finally:
        res.close()


def test_audit_batch_checks_the_question_count():
    model, qs, res = _host_case(TINY, ['P1', 'P6'], lambda q: {})
    try:
        with pytest.raises(ValueError, match='1 questions for a plan of 2'):
            audit.audit_batch(model, res, qs[:1])
    finally:
        res.close()


def test_module_report_is_a_function_of_the_node_values():
    rep = audit.module_report('attention', [-1, 0.0, 0.3, 0.5, 1.0])
    assert rep == {'n': 5, 'n_scored': 4, 'mean_iou': 0.45, 'recall@0.3': 0.75, 'recall@0.5': 0.5, 'recall@0.7': 0.25}
    assert audit.module_report('head', [1, 0, -1, 1]) == {'n': 4, 'n_scored': 3, 'accuracy': 2 / 3}
    rep = audit.module_report('contrastive', [1, 4, 0, 10], top=5)
    assert rep == {'n': 4, 'n_scored': 3, 'hit@1': 1 / 3, 'hit@top': 2 / 3, 'mrr': (1 + 0.25 + 0.1) / 3}
    rep = audit.module_report('contrastive', [0, 0])
    assert rep['n'] == 2 and rep['n_scored'] == 0 and all(np.isnan(rep[k]) for k in ('hit@1', 'hit@top', 'mrr'))
    assert np.isnan(audit.module_report('attention', [])['mean_iou'])
