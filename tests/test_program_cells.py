"""The plan builder on every producer -> consumer operand pair it admits, and on every pair it must refuse (host code only: no
kernel is launched).  The corpus is tests/program_cells.py: one tiny program per (consumer slot, producer)."""
import ctypes as C

import numpy as np
import pytest

import program_cells as PC
from oracle import nmn_oracle as O
from stair_amd import spec, synth
from stair_amd._lib import lib, check, PlanInfo
from helpers import plan_ctx, pack_programs, int32_ptr

CONFIG = dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, answer_vocab_length=16, max_video_length=40, object_types=10)
T = 24
TRAIN, NO_CSE = 1, 2            # include/stair_hip.h STAIR_PLAN_TRAIN, STAIR_PLAN_NO_CSE
FLAGS = [0, TRAIN, NO_CSE, TRAIN | NO_CSE]
CELLS = PC.cells()


@pytest.fixture(scope='module')
def ctx():
    h = plan_ctx(CONFIG)
    yield h
    lib.stair_ctx_destroy(h)


def _qs(cells):
    return [PC.question(CONFIG, 0, k, T, program=c.program, with_video=False) for k, c in enumerate(cells)]


def _build(h, qs, flags, voq=None, n_videos=None, video_len=None):
    """(plan, rc, prog_off) of a batch of question dicts in the context h"""
    prog_off, tokens, lo, hi, q_off = pack_programs([q['nmn_program_list'] for q in qs], [q['prog_str_to_question_tokens'] for q in qs],
                                                    [q['question'].shape[0] for q in qs])
    arrays = [int32_ptr(a) for a in (prog_off, tokens, lo, hi, q_off)]
    plan = C.c_void_p()
    if voq is None:
        rc = lib.stair_plan_build(h, len(qs), *arrays, T, flags, C.byref(plan))
    else:
        voq = np.asarray(voq, np.int32)
        if video_len is None:
            rc = lib.stair_plan_build_shared(h, len(qs), *arrays, n_videos, int32_ptr(voq), T, flags, C.byref(plan))
        else:
            vl = np.asarray(video_len, np.int32)
            rc = lib.stair_plan_build_ragged(h, len(qs), *arrays, n_videos, int32_ptr(voq), int32_ptr(vl), T, flags, C.byref(plan))
    return plan, rc, prog_off


def _nodes(plan, n):
    tab = tuple(np.empty(n, dtype=np.int32) for _ in range(5))
    check(lib.stair_plan_nodes(plan, *(int32_ptr(a) for a in tab), n))
    return tab          # kind, slot, aux, level, rel


def _check_nodes(plan, prog_off, cells):
    """the kind of every slot template's node is the table's, that of the producer's node the producer's, levels are the reference's"""
    kind, _, _, level, _ = _nodes(plan, int(prog_off[-1]))
    for q, c in enumerate(cells):
        o = int(prog_off[q])
        assert list(level[o: o + len(c.program)]) == O.module_levels(c.program), c
        assert kind[o + c.hole] == PC.KIND_CODE[c.producer_kind], c
        if c.consumer is not None:
            assert kind[o + c.consumer] == PC.KIND_CODE[c.out_kind], c
        assert kind[o] == PC.KIND_CODE[PC.VEC], c


# ---- the corpus is what it claims ------------------------------------------------------------------------------------------------
def test_every_cell_is_a_valid_program():
    assert len(CELLS) == 371 == sum(len(PC.PRODUCERS[kind]) for _, kind, _ in PC.SLOTS)
    for c in CELLS:
        assert O.program_is_valid(c.program), c
        assert sum(t in O.ARITY for t in c.program) <= 7, c
        words = [t for t in c.program if t not in O.ARITY and t not in O.WORDS_TO_KEEP]
        assert len(set(words)) == len(words), c                 # every span word is a token of its own


def test_stack_walk_finds_exactly_the_tables_pairs():
    """Read off each program, by the interpreter's stack walk, which operand of which module the producer's subtree fills: the
    set of (slot, producer) is slots x producers, none missing and none doubled."""
    seen = set()
    for c in CELLS:
        ch = O.children_of(c.program)
        # the producer: the subtree at the hole is the producer's tokens
        def size(i):
            return 1 + sum(size(j) for j in ch[i])
        assert size(c.hole) == c.producer_len, c
        sub = ['w' if t.startswith('w') and t[1:].isdigit() else t for t in c.program[c.hole: c.hole + c.producer_len]]
        assert sub == PC._expand(c.producer), c
        # the consumer: the hole's parent is the module the slot template names, at the operand where the template has its X
        par, op = PC.parent_of(c.program, c.hole)
        toks = PC._expand(c.slot)
        if c.slot == 'X':
            assert (par, op) == (None, None) and c.hole == 0, c
        else:
            tpar, top = PC.parent_of(toks, toks.index('X'))
            assert c.program[par] == toks[tpar] and op == top and par - c.consumer == tpar, c
            assert c.program[c.consumer] == toks[0], c
        key = (c.slot, c.producer)
        assert key not in seen, c
        seen.add(key)
    assert seen == {(slot, p) for slot, kind, _ in PC.SLOTS for p in PC.PRODUCERS[kind]}


def test_cells_reach_every_pair_the_forms_reach():
    of_cells, of_forms = set(), set()
    for c in CELLS:
        of_cells |= PC.pairs_of(c.program)
    for form in synth.ALL_FORMS:
        of_forms |= PC.pairs_of(synth.CORPUS[form][0])
    assert of_forms <= of_cells, of_forms - of_cells
    assert (len(of_forms), len(of_cells)) == (61, 351)          # by pairs_of's naming, the roots counted


# ---- admitted pairs build --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('flags', FLAGS)
def test_every_cell_builds_alone(ctx, flags):
    qs = _qs(CELLS)
    for q, c in zip(qs, CELLS):
        plan, rc, prog_off = _build(ctx, [q], flags)
        assert rc == 0, (c, lib.stair_last_error())
        try:
            _check_nodes(plan, prog_off, [c])
        finally:
            lib.stair_plan_destroy(plan)


@pytest.mark.parametrize('flags', FLAGS)
@pytest.mark.parametrize('layout', ['own', 'shared', 'ragged'])
def test_all_cells_build_as_one_batch(ctx, flags, layout):
    """one clip per question; all cells on 3 shared clips; 3 shared clips of 3, 17 and 24 frames"""
    qs = _qs(CELLS)
    voq = None if layout == 'own' else [k % 3 for k in range(len(qs))]
    plan, rc, prog_off = _build(ctx, qs, flags, voq, 3, [3, 17, 24] if layout == 'ragged' else None)
    assert rc == 0, lib.stair_last_error()
    try:
        _check_nodes(plan, prog_off, CELLS)
        info = PlanInfo()
        check(lib.stair_plan_get_info(plan, C.byref(info)))
        assert info.n_questions == len(CELLS)
        assert info.n_levels == 1 + max(max(O.module_levels(c.program)) for c in CELLS)
        assert (info.n_aliased > 0) == (not flags & NO_CSE)       # (`And F1 F1`: a subexpression twice in ONE program)
    finally:
        lib.stair_plan_destroy(plan)


# ---- every wrong-kind pair is refused loudly -------------------------------------------------------------------------------------
def test_every_wrong_kind_pair_is_refused(ctx):
    bad = PC.refused()
    assert len(bad) > 600
    kinds = {(c.kind, c.producer_kind) for c in bad}
    assert all((PC.VEC, k) in kinds for k in (PC.STR, PC.PAIR, PC.MAP, PC.FRAME, PC.ATT))
    for flags in (0, TRAIN):
        for k, c in enumerate(bad):
            q = PC.question(CONFIG, 0, k, T, program=c.program, with_video=False)
            plan, rc, _ = _build(ctx, [q], flags)
            assert rc != 0 and not plan, c
            err = lib.stair_last_error().decode()
            if c.slot == 'X':               # no consumer: the decoder refuses the root
                assert 'program root must produce a [H] vector' in err, (c, err)
                continue
            par, _ = PC.parent_of(c.program, c.hole)
            assert err.startswith('stair_plan_build: operand kind mismatch (') and \
                err.endswith(') at question 0, token %d (%s)' % (par, c.program[par])), (c, err)


# ---- shared clips: aliases and the store-first marks -----------------------------------------------------------------------------
@pytest.mark.parametrize('config', [CONFIG, dict(CONFIG, hidden_size=512)], ids=['H64', 'H512'])
def test_shared_clips_alias_nodes_and_cover_every_gradient_tile(config):
    """All cells on 3 shared clips with CSE: nodes are aliased and every gradient tile of the map arena is either stored by its
    first writer or cleared, never both and never neither (hidden size 64 runs no tile chain: everything is cleared)."""
    h = plan_ctx(config)
    try:
        qs = _qs(CELLS)
        plan, rc, _ = _build(h, qs, TRAIN, [k % 3 for k in range(len(qs))], 3)
        assert rc == 0, lib.stair_last_error()
        try:
            info = PlanInfo()
            check(lib.stair_plan_get_info(plan, C.byref(info)))
            assert info.n_aliased > 0 and info.n_map_stage > 0 and info.n_vec_stage > 0 and info.n_att_stage > 0
            a, b = C.c_int32(-1), C.c_int32(-1)
            assert lib.stair_plan_store_first_counts(plan, C.byref(a), C.byref(b)) == 0, lib.stair_last_error()
            assert a.value >= 0 and b.value >= 0 and a.value + b.value == info.n_map + info.n_map_stage
            if config['hidden_size'] == 64:
                assert a.value == 0
            else:
                assert a.value > 0 and b.value > 0
        finally:
            lib.stair_plan_destroy(plan)
    finally:
        lib.stair_ctx_destroy(h)
