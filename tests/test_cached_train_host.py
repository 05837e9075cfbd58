"""Training plans of encoded clips (STAIR_PLAN_TRAIN | STAIR_PLAN_VIDEO_ENCODED, include/stair_hip.h) on the host: the plan builder,
stair_plan_set_encoded_video[_grad] and stair_plan_touched enqueue nothing, so no GPU is needed.

The rule: such a plan exists only while all eight tensors of the video encoder are frozen (stair_ctx_set_trainable(ctx, id, 0))."""
import ctypes as C

import numpy as np
import pytest

from stair_amd import spec, synth
from stair_amd._lib import lib, check, PlanInfo, StairError
from helpers import plan_ctx, pack_programs, int32_ptr as ip

TRAIN, NO_CSE, EXT_PROJ, ENCODED = 1, 2, 4, 8
T = 64


def _forms(config):
    qs = [synth.make_question(config, 0, i, form=f, with_video=False) for i, f in enumerate(synth.ALL_FORMS)]
    return ([q['nmn_program_list'] for q in qs], [q['prog_str_to_question_tokens'] for q in qs], [q['question'].shape[0] for q in qs])


def _names(h):
    return [lib.stair_weight_name(h, i).decode() for i in range(lib.stair_weight_count(h))]


def _build(config, flags, frozen=True, thaw=None, voq=None, n_videos=None, video_len=None, frames=T):
    """a context with the video encoder frozen (but the tensor `thaw`), and the plan of the 12 forms in it: (ctx, plan, rc)"""
    h = plan_ctx(config)
    enc = [i for i, n in enumerate(_names(h)) if '.video_encoder.' in n]
    assert len(enc) == 8
    if frozen:
        for i in enc:
            check(lib.stair_ctx_set_trainable(h, i, 0))
    if thaw is not None:
        check(lib.stair_ctx_set_trainable(h, enc[thaw], 1))
    programs, spans, q_lens = _forms(config)
    arrays = pack_programs(programs, spans, q_lens)
    n = len(programs)
    n_videos = n if n_videos is None else n_videos
    plan = C.c_void_p()
    rc = lib.stair_plan_build_ragged(h, n, *[ip(a) for a in arrays], n_videos, ip(np.asarray(voq, np.int32)) if voq is not None else None,
                                     ip(np.asarray(video_len, np.int32)) if video_len is not None else None, frames, flags, C.byref(plan))
    return h, plan, rc


def _describe(h, plan):
    info = PlanInfo()
    check(lib.stair_plan_get_info(plan, C.byref(info)))
    tab = [np.empty(info.n_nodes, np.int32) for _ in range(5)]
    check(lib.stair_plan_nodes(plan, *[ip(a) for a in tab], info.n_nodes))
    cap = 8192
    nm = (C.c_char_p * cap)(); beg = (C.c_int64 * cap)(); end = (C.c_int64 * cap)()
    k = lib.stair_plan_regions(plan, h, nm, beg, end, cap)
    assert 0 < k < cap
    regs = sorted((beg[i], end[i], nm[i].decode()) for i in range(k))
    sf, cl = C.c_int32(), C.c_int32()
    check(lib.stair_plan_store_first_counts(plan, C.byref(sf), C.byref(cl)))
    return info, tab, regs, (sf.value, cl.value)


@pytest.mark.parametrize('shared', [False, True])
@pytest.mark.parametrize('extra', [0, NO_CSE, EXT_PROJ])
def test_encoded_training_plan_builds_with_the_training_plans_nodes_and_no_video_encoder_regions(shared, extra):
    config = dict(spec.DEFAULT_CONFIG)
    H = config['hidden_size']
    kw = dict(voq=[i // 3 for i in range(12)], n_videos=4) if shared else {}
    n_vid = 4 if shared else 12
    got = {}
    for flags in (TRAIN, TRAIN | ENCODED):
        h, plan, rc = _build(config, flags | extra, **kw)
        assert rc == 0, lib.stair_last_error()
        got[flags] = _describe(h, plan)
        lib.stair_plan_destroy(plan)
        lib.stair_ctx_destroy(h)
    (pi, pt, pr, pm), (ei, et, er, em) = got[TRAIN], got[TRAIN | ENCODED]
    fields = [f for f, _ in PlanInfo._fields_ if f.startswith('n_')] + ['T']
    assert [getattr(ei, f) for f in fields] == [getattr(pi, f) for f in fields]           # nodes, slots, levels, CSE, staging slots
    assert ei.gvec_off >= 0 and ei.gmap_off >= 0 and ei.gatt_off >= 0 and em == pm        # gradient arenas, first-touch marks
    if shared and not extra & NO_CSE:
        assert ei.n_aliased > 0
    for a, b in zip(pt, et):
        assert np.array_equal(a, b)
    names, plain = {r[2] for r in er}, {r[2] for r in pr}
    video_only = {'xpv', 'wplanes', 'coop', 'vhn', 'cv', 'tnenc0'}
    assert {'cv', 'tnenc0', 'coop', 'vhn'} <= plain and (extra & EXT_PROJ or {'xpv', 'wplanes'} <= plain)
    assert not names & video_only, names & video_only
    assert {'ct', 'hprev', 'tnenc1', 'coop2', 'map', 'gblock', 'discard', 'END'} <= names and (extra & EXT_PROJ or 'xpt' in names)
    # the same buckets own the same regions
    assert sorted(n for n in names if n.startswith('b')) == sorted(n for n in plain if n.startswith('b'))
    size = lambda regs, name: [e - b for b, e, n in regs if n == name][0]
    rows_q = sum(_forms(config)[2])
    assert size(er, 'hprev') == rows_q * H and size(pr, 'hprev') == (n_vid * T + rows_q) * H           # the text rows only
    for a, b in zip(er, er[1:]):
        assert a[1] <= b[0], ('overlap', a, b)
    # xpv 4H (inside the workspace unless the projections live in the caller's buffer), cv H and hprev H per frame
    per_frame = (2 if extra & EXT_PROJ else 6) * H
    assert pi.workspace_bytes - ei.workspace_bytes >= n_vid * T * per_frame * 4
    if extra & EXT_PROJ:            # ... where the text projection runs with n_videos = 0, as in inference
        h = plan_ctx(config)
        assert lib.stair_projection_floats(h, n_vid, T, rows_q) - lib.stair_projection_floats(h, 0, T, rows_q) >= n_vid * T * 4 * H
        lib.stair_ctx_destroy(h)


@pytest.mark.parametrize('thaw', [0, 3, 7])
def test_one_thawed_tensor_refuses_the_build_naming_both_flags(thaw):
    config = dict(spec.DEFAULT_CONFIG)
    h, plan, rc = _build(config, TRAIN | ENCODED, thaw=thaw)
    msg = lib.stair_last_error().decode()
    lib.stair_ctx_destroy(h)
    assert rc != 0 and 'STAIR_PLAN_VIDEO_ENCODED' in msg and 'STAIR_PLAN_TRAIN' in msg and 'frozen' in msg and 'stair_ctx_set_trainable' in msg, msg
    # inference on encoded clips does not care about the flags
    h, plan, rc = _build(config, ENCODED, frozen=False)
    assert rc == 0
    lib.stair_plan_destroy(plan)
    lib.stair_ctx_destroy(h)


def test_dropout_is_set_as_on_any_training_plan():
    config = dict(spec.DEFAULT_CONFIG)
    h, plan, rc = _build(config, TRAIN | ENCODED | NO_CSE, voq=[i // 3 for i in range(12)], n_videos=4)
    assert rc == 0
    check(lib.stair_plan_set_dropout(plan, C.c_float(0.1), C.c_uint64(7)))
    lib.stair_plan_destroy(plan)
    h2, plan, rc = _build(config, TRAIN | ENCODED, voq=[i // 3 for i in range(12)], n_videos=4)
    with pytest.raises(StairError, match='STAIR_PLAN_NO_CSE'):
        check(lib.stair_plan_set_dropout(plan, C.c_float(0.1), C.c_uint64(7)))
    lib.stair_plan_destroy(plan)
    lib.stair_ctx_destroy(h)
    lib.stair_ctx_destroy(h2)


def test_the_gradient_setters_refusals_one_message_each():
    config = dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, answer_vocab_length=16, max_video_length=64, object_types=10)
    H = config['hidden_size']
    lens = [3, 17, 40, 64]
    kw = dict(voq=[i % 4 for i in range(12)], n_videos=4, video_len=lens)
    enc, d_enc = C.c_void_p(256), C.c_void_p(4096)         # aligned non-null addresses: the setters only record them (nothing is launched here)
    setg = lib.stair_plan_set_encoded_video_grad
    # a plan that is not train and encoded
    for flags in (TRAIN, ENCODED):
        h, plan, rc = _build(config, flags, **kw)
        assert rc == 0
        with pytest.raises(StairError, match=r'STAIR_PLAN_TRAIN \| STAIR_PLAN_VIDEO_ENCODED'):
            check(setg(plan, d_enc, 64 * H, 64))
        lib.stair_plan_destroy(plan)
        lib.stair_ctx_destroy(h)
    h, plan, rc = _build(config, TRAIN | ENCODED, **kw)
    assert rc == 0, lib.stair_last_error()
    with pytest.raises(StairError, match='stair_plan_set_encoded_video first'):
        check(setg(plan, d_enc, 64 * H, 64))
    check(setg(plan, None, 0, 0))                           # withdrawing is always possible
    check(lib.stair_plan_set_encoded_video(plan, enc, 64 * H, 64, ip(np.asarray([7, 2, 9, 5], np.int32))))
    with pytest.raises(StairError, match='16-byte aligned'):
        check(setg(plan, C.c_void_p(4100), 64 * H, 64))
    with pytest.raises(StairError, match='multiple of 4 floats'):
        check(setg(plan, d_enc, 64 * H + 2, 64))
    with pytest.raises(StairError, match='clip stride smaller'):
        check(setg(plan, d_enc, 63 * H, 64))
    with pytest.raises(StairError, match=r'video_len\[3\] = 64 frames exceed the gradient\'s rows_cap = 40'):
        check(setg(plan, d_enc, 40 * H, 40))
    check(setg(plan, d_enc, 64 * H, 64))
    check(setg(plan, d_enc, 80 * H, 72))                    # rows_cap above T, a padded stride
    check(setg(plan, None, 0, 0))
    # two plan clips on one row: fine for the gather, refused for its adjoint
    check(lib.stair_plan_set_encoded_video(plan, enc, 64 * H, 64, ip(np.asarray([7, 2, 2, 5], np.int32))))
    with pytest.raises(StairError, match='not pairwise distinct.*row 2'):
        check(setg(plan, d_enc, 64 * H, 64))
    lib.stair_plan_destroy(plan)
    lib.stair_ctx_destroy(h)


def test_touched_reports_nothing_for_the_encoder():
    config = dict(spec.DEFAULT_CONFIG)
    h, plan, rc = _build(config, TRAIN | ENCODED)
    assert rc == 0
    names = _names(h)
    arr = (C.c_int32 * len(names))()
    check(lib.stair_plan_touched(h, plan, arr, len(names)))
    touched = dict(zip(names, arr))
    assert not any(v for n, v in touched.items() if '.video_encoder.' in n)
    assert all(v for n, v in touched.items() if '.text_encoder.' in n or '.decoder.' in n)
    # thawed after the build: the plan still has no video encoder to send a gradient to
    for i, n in enumerate(names):
        check(lib.stair_ctx_set_trainable(h, i, 1))
    check(lib.stair_plan_touched(h, plan, arr, len(names)))
    assert not any(v for n, v in zip(names, arr) if '.video_encoder.' in n) and sum(arr) == sum(touched.values())
    lib.stair_plan_destroy(plan)
    lib.stair_ctx_destroy(h)
