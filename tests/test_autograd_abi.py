"""CPU tests of the autograd entry point's ABI (stair_plan_backward_dlogits): the symbol is exported and bound, and argument
errors are reported before anything is enqueued -- so every call below returns without touching device memory (the pointers
are aligned non-null placeholders)."""
import ctypes as C

import numpy as np
import pytest

from stair_amd import _lib, spec, synth
from stair_amd._lib import StairConfig, check, lib

FAKE = C.c_void_p(256)             # aligned, non-null; never dereferenced because every call fails its checks first


def test_dlogits_backward_is_exported_and_bound():
    assert hasattr(lib, 'stair_plan_backward_dlogits')
    assert 'stair_plan_backward_dlogits' in {name for name, _, _ in _lib.SIGNATURES}
    assert lib.stair_abi_version() == 7


def test_autograd_module_imports():
    from stair_amd import autograd
    from stair_amd.module_net import VideoNMN
    assert issubclass(autograd.PlanLogits, __import__('torch').autograd.Function)
    assert callable(VideoNMN.logits)


def _ctx_and_plan(train):
    config = dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, answer_vocab_length=16, max_video_length=40, object_types=10)
    cfg = StairConfig(config['hidden_size'], config['video_size'], config['text_size'], config['answer_vocab_length'],
                      config['max_video_length'], config['object_types'], 1)
    h = C.c_void_p()
    check(lib.stair_ctx_create(C.byref(cfg), C.byref(h)))
    q = synth.make_question(config, 0, 0, form='P1', with_video=False)
    enc = np.asarray(spec.encode_program(q['nmn_program_list']), dtype=np.int32)
    prog_off = np.asarray([0, len(enc)], np.int32)
    lo = np.zeros(len(enc), np.int32); hi = np.zeros(len(enc), np.int32)
    for i, c in enumerate(enc):
        if c == spec.TOK_SPAN:
            lo[i], hi[i] = q['prog_str_to_question_tokens'][i]
    q_off = np.asarray([0, q['question'].shape[0]], np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    plan = C.c_void_p()
    check(lib.stair_plan_build(h, 1, ip(prog_off), ip(enc), ip(lo), ip(hi), ip(q_off), 40, 1 if train else 0, C.byref(plan)))
    return h, plan


def _call(h, plan, ws=FAKE, d_logits=FAKE, nbytes=1 << 40):
    return lib.stair_plan_backward_dlogits(h, plan, FAKE, FAKE, ws, nbytes, d_logits, None, None, 0, None)


@pytest.mark.parametrize('which', ['ctx', 'plan', 'workspace', 'd_logits'])
def test_null_arguments_are_rejected(which):
    h, plan = _ctx_and_plan(train=True)
    try:
        args = dict(h=h, plan=plan)
        kw = {}
        if which == 'ctx':
            args['h'] = None
        elif which == 'plan':
            args['plan'] = None
        elif which == 'workspace':
            kw['ws'] = None
        else:
            kw['d_logits'] = None
        assert _call(args['h'], args['plan'], **kw) != 0
        assert b'null argument' in lib.stair_last_error()
    finally:
        lib.stair_plan_destroy(plan)
        lib.stair_ctx_destroy(h)


def test_inference_plan_is_rejected():
    h, plan = _ctx_and_plan(train=False)
    try:
        assert _call(h, plan) != 0
        assert b'STAIR_PLAN_TRAIN' in lib.stair_last_error()
    finally:
        lib.stair_plan_destroy(plan)
        lib.stair_ctx_destroy(h)


def test_small_workspace_and_misaligned_gradients_are_rejected():
    h, plan = _ctx_and_plan(train=True)
    try:
        assert _call(h, plan, nbytes=16) != 0
        assert b'workspace too small' in lib.stair_last_error()
        rc = lib.stair_plan_backward_dlogits(h, plan, FAKE, FAKE, FAKE, 1 << 40, FAKE, C.c_void_p(260), None, 0, None)
        assert rc != 0 and b'16-byte aligned' in lib.stair_last_error()
    finally:
        lib.stair_plan_destroy(plan)
        lib.stair_ctx_destroy(h)
