"""CPU tests of the frozen-weight switch of the C ABI (stair_ctx_set_trainable / stair_ctx_get_trainable): host state of the
context and the mask stair_plan_touched reports.  No kernel is launched here; what a reverse pass does with the flags is
tests/test_gpu_frozen.py."""
import ctypes as C

import numpy as np

from stair_amd import spec, synth
from stair_amd._lib import lib, check
from helpers import plan_ctx as _ctx, pack_programs, int32_ptr as ip


def _flag(h, i):
    v = C.c_int32(-7)
    check(lib.stair_ctx_get_trainable(h, i, C.byref(v)))
    return v.value


def test_set_get_round_trip_default_and_range():
    h = _ctx(dict(spec.DEFAULT_CONFIG))
    try:
        n = lib.stair_weight_count(h)
        assert n > 80
        assert [_flag(h, i) for i in range(n)] == [1] * n               # every weight is trainable until told otherwise
        check(lib.stair_ctx_set_trainable(h, 3, 0))
        check(lib.stair_ctx_set_trainable(h, n - 1, 0))
        assert [i for i in range(n) if _flag(h, i) == 0] == [3, n - 1]
        check(lib.stair_ctx_set_trainable(h, 3, 5))                     # any non-zero value thaws, and reads back as 1
        assert _flag(h, 3) == 1 and _flag(h, n - 1) == 0
        v = C.c_int32(0)
        for bad in (-1, n, n + 100):
            assert lib.stair_ctx_set_trainable(h, bad, 0) != 0 and b'out of range' in lib.stair_last_error()
            assert lib.stair_ctx_get_trainable(h, bad, C.byref(v)) != 0 and b'out of range' in lib.stair_last_error()
        assert lib.stair_ctx_get_trainable(h, 0, None) != 0 and b'null' in lib.stair_last_error()
        assert lib.stair_ctx_set_trainable(None, 0, 0) != 0 and b'null' in lib.stair_last_error()
        assert [i for i in range(n) if _flag(h, i) == 0] == [n - 1]     # the refused calls changed nothing
        other = _ctx(dict(spec.DEFAULT_CONFIG))                         # the flags live in the context
        assert _flag(other, n - 1) == 1
        lib.stair_ctx_destroy(other)
    finally:
        lib.stair_ctx_destroy(h)


def test_touched_is_zero_exactly_for_the_frozen_weights():
    """A 12-form training plan (built as tests/test_abi.py builds it): stair_plan_touched reports 0 for every frozen id and what it
    always reported for the rest; thawing brings the old mask back; the plan itself does not change (same workspace)."""
    config = dict(spec.DEFAULT_CONFIG)
    names = sorted(synth.CORPUS)
    qs = [synth.make_question(config, 0, i, form=name, with_video=False) for i, name in enumerate(names)]
    h = _ctx(config)
    plan = C.c_void_p()
    try:
        prog_off, tokens, lo, hi, q_off = pack_programs([q['nmn_program_list'] for q in qs], [q['prog_str_to_question_tokens'] for q in qs],
                                                        [q['question'].shape[0] for q in qs])
        check(lib.stair_plan_build(h, len(qs), ip(prog_off), ip(tokens), ip(lo), ip(hi), ip(q_off), 64, 1, C.byref(plan)))
        n = lib.stair_weight_count(h)
        wname = [lib.stair_weight_name(h, i).decode() for i in range(n)]

        def touched():
            arr = np.full(n, -1, np.int32)
            check(lib.stair_plan_touched(h, plan, ip(arr), n))
            return arr
        base = touched()
        assert set(base.tolist()) == {0, 1} and base.sum() > 60
        # an encoder (all eight tensors), one Linear weight without its bias, a module, and a weight no program of the batch uses
        frozen = [i for i, nme in enumerate(wname) if '.video_encoder.' in nme or nme == 'submodules.decoder.3.weight' or
                  nme.startswith('submodules.Filter.')]
        unused = [i for i in range(n) if base[i] == 0]
        frozen += unused[:1]
        assert sum('.video_encoder.' in wname[i] for i in frozen) == 8 and len(frozen) > 12 and all(base[i] == 1 for i in frozen[:-1])
        for i in frozen:
            check(lib.stair_ctx_set_trainable(h, i, 0))
        got = touched()
        for i in range(n):
            assert got[i] == (0 if i in frozen else base[i]), wname[i]
        assert got[wname.index('submodules.decoder.3.bias')] == 1 and got[wname.index('submodules.FilterFrame.param.representation.0.weight')] == 1
        for i in frozen:
            check(lib.stair_ctx_set_trainable(h, i, 1))
        assert np.array_equal(touched(), base)
        # a training plan lays out the region a frozen weight's gradient goes to, large enough for the largest weight
        cap = 8192
        nm = (C.c_char_p * cap)(); beg = (C.c_int64 * cap)(); end = (C.c_int64 * cap)()
        k = lib.stair_plan_regions(plan, h, nm, beg, end, cap)
        disc = [(beg[i], end[i]) for i in range(k) if nm[i] == b'discard']
        assert len(disc) == 1 and disc[0][1] - disc[0][0] >= max(lib.stair_weight_numel(h, i) for i in range(n))
    finally:
        if plan:
            lib.stair_plan_destroy(plan)
        lib.stair_ctx_destroy(h)
