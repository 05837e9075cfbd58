"""CPU tests of the drop-in boundary: the C-ABI library loads and exports every symbol the header
declares, its weight table equals the reference's state_dict keys, the VideoNMN mirror has the
reference's state_dict layout, and the plan builder (host-only code) levels programs exactly like
utils/program_parser.py::stat_module_levels.  No kernel is launched here."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from stair_amd import spec, synth
from stair_amd import _lib
from stair_amd._lib import lib, check, StairConfig, PlanInfo, StairError
from helpers import GOLDEN, plan_ctx as _ctx, pack_programs, build_plan as _build, int32_ptr as ip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_are_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'stair_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(stair_[a-z0-9_]+)\s*\(', header))
    bound = {name for name, _, _ in _lib.SIGNATURES}
    assert declared == bound, (declared ^ bound)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.stair_abi_version() == 7


CONFIGS = [
    dict(spec.DEFAULT_CONFIG),
    dict(spec.DEFAULT_CONFIG, have_pretrain_head=False),
    dict(spec.DEFAULT_CONFIG, max_video_length=8, video_size=4096),
    dict(spec.DEFAULT_CONFIG, max_video_length=150),          # args.py:29 default -> k = round(37.5) = 38
    dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, answer_vocab_length=16, max_video_length=40, object_types=10),
]


@pytest.mark.parametrize('config', CONFIGS)
def test_weight_table_matches_spec(config):
    h = _ctx(config)
    try:
        table = spec.weight_table(config)
        assert lib.stair_weight_count(h) == len(table)
        for i, (name, shape) in enumerate(table):
            assert lib.stair_weight_name(h, i).decode() == name
            assert lib.stair_weight_numel(h, i) == int(np.prod(shape)), name
    finally:
        lib.stair_ctx_destroy(h)


def test_bad_config_is_rejected():
    cfg = StairConfig(100, 2048, 300, 172, 64, 36, 1)
    h = C.c_void_p()
    assert lib.stair_ctx_create(C.byref(cfg), C.byref(h)) != 0
    assert b'hidden_size' in lib.stair_last_error()


def test_context_options_are_per_context():
    """stair_ctx_set_option / stair_ctx_get_option: overrides live in the context (host state only, no GPU needed), -1 = inherit."""
    cfg = StairConfig(512, 2048, 300, 172, 64, 36, 1)
    a, b = C.c_void_p(), C.c_void_p()
    assert lib.stair_ctx_create(C.byref(cfg), C.byref(a)) == 0 and lib.stair_ctx_create(C.byref(cfg), C.byref(b)) == 0
    v = C.c_int32(7)
    for opt in range(5):
        assert lib.stair_ctx_get_option(a, opt, C.byref(v)) == 0 and v.value == -1
    assert lib.stair_ctx_set_option(a, 0, 0) == 0 and lib.stair_ctx_set_option(a, 1, 0) == 0
    assert lib.stair_ctx_get_option(a, 0, C.byref(v)) == 0 and v.value == 0
    assert lib.stair_ctx_get_option(b, 0, C.byref(v)) == 0 and v.value == -1            # the other context is untouched
    assert lib.stair_ctx_set_option(a, 0, -5) == 0 and lib.stair_ctx_get_option(a, 0, C.byref(v)) == 0 and v.value == -1
    assert lib.stair_ctx_set_option(a, 0, 9) != 0 and b'matmul mode' in lib.stair_last_error()
    assert lib.stair_ctx_set_option(a, 5, 1) != 0 and b'unknown option' in lib.stair_last_error()
    lib.stair_ctx_destroy(a); lib.stair_ctx_destroy(b)


@pytest.mark.parametrize('heads', [True, False])
def test_videonmn_state_dict_layout(heads):
    from stair_amd.module_net import VideoNMN
    config = dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, answer_vocab_length=16, max_video_length=40,
                  object_types=10, have_pretrain_head=heads)
    m = VideoNMN(config)
    sd = m.state_dict()
    assert list(sd.keys()) == spec.state_dict_keys(config)
    shapes = dict(spec.weight_table(config))
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(shapes[spec.WEIGHT_ALIASES.get(k, k)]), k
    # Superlative.localize_module IS Localize (module_net.py:31-32)
    assert sd['submodules.Superlative.localize_module.video_linear.0.weight'].data_ptr() == \
        sd['submodules.Localize.video_linear.0.weight'].data_ptr()
    # loading a reference-layout checkpoint works
    w = synth.make_weights(config, 3)
    import torch
    m.load_state_dict({k: torch.from_numpy(w[k].copy()) for k in spec.state_dict_keys(config)})
    assert np.array_equal(m.state_dict()['submodules.decoder.3.bias'].numpy(), w['submodules.decoder.3.bias'])


def test_plan_levels_match_reference_stat_module_levels():
    progs = json.load(open(os.path.join(GOLDEN, 'programs.json')))
    progs.pop('_nary_mappings')
    config = dict(spec.DEFAULT_CONFIG)
    names = sorted(progs)
    qs = [synth.make_question(config, 0, i, form=name, with_video=False) for i, name in enumerate(names)]
    h, plan, rc, prog_off = _build(config, [q['nmn_program_list'] for q in qs],
                                   [q['prog_str_to_question_tokens'] for q in qs], [q['question'].shape[0] for q in qs], 64)
    assert rc == 0, lib.stair_last_error()
    try:
        for qi, name in enumerate(names):
            lv = []
            for i in range(len(progs[name]['nmn'])):
                k, s, a, l, r = (C.c_int32() for _ in range(5))
                check(lib.stair_plan_node(plan, int(prog_off[qi] + i), C.byref(k), C.byref(s), C.byref(a), C.byref(l), C.byref(r)))
                lv.append(l.value)
            assert lv == progs[name]['levels'], name
        info = PlanInfo()
        check(lib.stair_plan_get_info(plan, C.byref(info)))
        assert info.n_questions == len(names) and info.n_levels == 1 + max(max(p['levels']) for p in progs.values())
        assert info.workspace_bytes > 0 and info.vec_off % config['hidden_size'] == 0 and info.map_off % config['hidden_size'] == 0
    finally:
        lib.stair_plan_destroy(plan)
        lib.stair_ctx_destroy(h)


KIND = 'stair_plan_build: operand kind mismatch (%s) at question 0, token %d (%s)'


@pytest.mark.parametrize('program,msg', [
    (['Filter', 'video'], 'stack underflow'),                              # invalid: missing operand
    (['video', 'video'], 'stack holds 2'),                                 # assert len(stack)==1, module_net.py:135
    (['Temporal', 'while', 'video', 'Localize', 'video', 'x'], 'root must produce'),   # root is a [T,H] map
    (['Filter', 'dish', 'objects'], 'kind mismatch'),                      # feat is not a map
    (['Exists', 'dish', 'Filter', 'video', 'max'], 'Filter keyword'),      # KeyError 'max' in the reference
    # every operand-kind refusal of the builder, and the second refusals of Filter, FilterFrame and Temporal for a keyword or mode
    # the module has no variant for: the whole message
    (['And', 'dish', 'video'], KIND % ('needs two [H] vectors or two [T] frame attentions', 0, 'And')),
    (['AttnVideo', 'dish', 'video'], KIND % ('AttnVideo(feat [T,H], attn [T])', 0, 'AttnVideo')),
    (['Choose', 'video', 'a', 'b'], KIND % ('Choose(kw1 [H], kw2 [H], query [H])', 0, 'Choose')),
    (['Compare', 'video', 'a'], KIND % ('needs two [H] vectors', 0, 'Compare')),
    (['ExistsFrame', 'video', 'a'], KIND % ('ExistsFrame(keyword [H], feat [T,H])', 0, 'ExistsFrame')),
    (['Filter', 'dish', 'objects'], KIND % ('Filter(feat [T,H], keyword)', 0, 'Filter')),
    (['Exists', 'dish', 'Filter', 'video', 'max'],
     KIND % ('Filter keyword must be a [H] vector or actions/objects/relations (modules.py:346-351)', 2, 'Filter')),
    (['FilterFrame', 'dish', 'actions'], KIND % ('FilterFrame(feat [T,H], keyword)', 0, 'FilterFrame')),
    (['FilterFrame', 'video', 'objects'],
     KIND % ('FilterFrame keyword must be a [H] vector or relations/actions (modules.py:384-388)', 0, 'FilterFrame')),
    (['HasItem', 'dish'], KIND % ('HasItem(feat [T,H])', 0, 'HasItem')),
    (['Localize', 'dish', 'a'], KIND % ('Localize(feat [T,H], keyword [H] or [2,H])', 0, 'Localize')),
    (['Relate', 'forward', 'video'], KIND % ('Relate(mode, attn [T])', 0, 'Relate')),
    (['Superlative', 'max', 'video', 'dish'], KIND % ('Superlative(mode, actions [Ka,H], feat [T,H])', 0, 'Superlative')),
    (['Temporal', 'while', 'dish', 'video'], KIND % ('Temporal(mode, feat [T,H], attention [K,T])', 0, 'Temporal')),
    (['Temporal', 'max', 'video', 'Localize', 'video', 'x'],
     KIND % ('Temporal mode must be while/before/after/between (modules.py:263,279)', 0, 'Temporal')),
    (['Array2', 'video', 'a'], KIND % ('Array2(a [H], b [H])', 0, 'Array2')),
])
def test_invalid_programs_are_rejected(program, msg):
    config = dict(spec.DEFAULT_CONFIG)
    spans = {i: (1, 2) for i in range(len(program))}
    h, plan, rc, _ = _build(config, [program], [spans], [8], 64)
    try:
        assert rc != 0
        err = lib.stair_last_error().decode()
        assert err == msg if msg.startswith('stair_plan_build:') else msg in err, err
    finally:
        lib.stair_ctx_destroy(h)


def test_linear_temporal_requires_full_length():
    config = dict(spec.DEFAULT_CONFIG, max_video_length=8)
    h, plan, rc, _ = _build(config, [['Filter', 'video', 'objects']], [{}], [8], 6)
    assert rc != 0 and b'max_video_length' in lib.stair_last_error()
    lib.stair_ctx_destroy(h)


def _build_forms(L, T, forms, flags):
    """rc and message of stair_plan_build for one question per form at max_video_length L, T frames (tiny configuration)"""
    config = dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, answer_vocab_length=16, max_video_length=L, object_types=10)
    qs = [synth.make_question(config, 0, i, form=f, with_video=False) for i, f in enumerate(forms)]
    h, plan, rc, _ = _build(config, [q['nmn_program_list'] for q in qs], [q['prog_str_to_question_tokens'] for q in qs],
                            [q['question'].shape[0] for q in qs], T, flags)
    msg = lib.stair_last_error().decode() if rc else ''
    if rc == 0:
        lib.stair_plan_destroy(plan)
    lib.stair_ctx_destroy(h)
    return rc, msg


def test_training_plans_beyond_the_backward_limits_are_refused_at_build():
    """include/stair_hip.h, stair_plan_build: a STAIR_PLAN_TRAIN plan whose reverse pass a launcher would refuse -- Superlative beyond
    T = 113 (the T x T score images of its backward kernel in 160 KB of LDS), Temporal before/after/between beyond Conv1d filters of
    k = 35 (max_video_length 141; round half to even makes 142 -> 36) -- is refused when it is built, with the limit in the message;
    the last admitted sizes build, and so do inference plans of the refused ones.  P3 = Superlative(max, ..), P5 = Temporal before and
    after, P6 = Temporal while (no relate nets: no bound)."""
    TRAIN = 1
    assert _build_forms(141, 113, ['P3', 'P5', 'C1'], TRAIN)[0] == 0
    rc, msg = _build_forms(141, 114, ['P1', 'P3'], TRAIN)
    assert rc != 0 and 'Superlative' in msg and 'T <= 113' in msg and 'T = 114' in msg, msg
    assert _build_forms(141, 114, ['P1', 'P5', 'P6'], TRAIN)[0] == 0            # no Superlative node: T = 114 trains
    assert _build_forms(141, 114, ['P1', 'P3'], 0)[0] == 0
    assert _build_forms(141, 141, ['P3', 'P5', 'C1'], 0)[0] == 0
    assert _build_forms(141, 64, ['P5'], TRAIN)[0] == 0
    rc, msg = _build_forms(142, 64, ['P1', 'P5'], TRAIN)
    assert rc != 0 and 'Temporal before/after/between' in msg and 'k <= 35' in msg and 'max_video_length <= 141' in msg and '= 36' in msg, msg
    assert _build_forms(142, 64, ['P1', 'P6'], TRAIN)[0] == 0                   # `while` has no relate nets
    assert _build_forms(142, 64, ['P1', 'P5'], 0)[0] == 0
    assert _build_forms(150, 150, ['P3', 'P5', 'C1'], 0)[0] == 0                # args.py:29's default stays an inference size


@pytest.mark.parametrize('train', [False, True])
def test_workspace_regions_are_disjoint(train):
    """Every region of the plan's workspace layout (arenas, per-bucket saves, gradient arenas, scratch) must be
    disjoint from every other one, for all 12 program forms in one batch -- and together they must cover the workspace:
    the list is what the builder recorded while it assigned the offsets, so a region that is missing from it shows as a
    hole.  The only holes allowed are alignment padding: every region is aligned to 64 or to H floats (H = 512 here, a
    multiple of 64), and empty regions in between add no more than one such alignment."""
    config = dict(spec.DEFAULT_CONFIG)
    names = sorted(synth.CORPUS)
    qs = [synth.make_question(config, 0, i, form=name, with_video=False) for i, name in enumerate(names)]
    h = _ctx(config)
    n = len(qs)
    prog_off, tokens, lo, hi, q_off = pack_programs([q['nmn_program_list'] for q in qs], [q['prog_str_to_question_tokens'] for q in qs],
                                                    [q['question'].shape[0] for q in qs])
    plan = C.c_void_p()
    check(lib.stair_plan_build(h, n, ip(prog_off), ip(tokens), ip(lo), ip(hi), ip(q_off), 64, 1 if train else 0, C.byref(plan)))
    cap = 8192
    nm = (C.c_char_p * cap)(); beg = (C.c_int64 * cap)(); end = (C.c_int64 * cap)()
    k = lib.stair_plan_regions(plan, h, nm, beg, end, cap)
    assert 0 < k < cap
    regs = sorted((beg[i], end[i], nm[i].decode()) for i in range(k))
    for a, b in zip(regs, regs[1:]):
        assert a[1] <= b[0], ('overlap', a, b)
    info = PlanInfo()
    check(lib.stair_plan_get_info(plan, C.byref(info)))
    assert regs[-1][2] == 'END' and regs[-1][0] * 4 == info.workspace_bytes
    assert nm[k - 1] == b'END'
    assert regs[0][0] == 0, regs[0]
    bound = max(64, config['hidden_size'])
    for a, b in zip(regs, regs[1:]):
        assert b[0] - a[1] < bound, ('hole of %d floats' % (b[0] - a[1]), a, b)
    lib.stair_plan_destroy(plan)
    lib.stair_ctx_destroy(h)


@pytest.mark.parametrize('train', [False, True])
def test_external_projection_plan_leaves_the_projection_regions_out(train):
    """STAIR_PLAN_EXT_PROJECTION (ABI 6): the encoders' input-projection regions move to a caller-owned buffer whose size depends on the
    batch shape alone (stair_projection_floats) -- the workspace shrinks by exactly that much, the remaining regions stay disjoint, and a
    buffer that is too small, or a plan built without the flag, is refused."""
    config = dict(spec.DEFAULT_CONFIG)
    qs = [synth.make_question(config, 0, i, form=name, with_video=False) for i, name in enumerate(sorted(synth.CORPUS))]
    programs = [q['nmn_program_list'] for q in qs]
    h = _ctx(config)
    n = len(qs)
    prog_off, tokens, lo, hi, q_off = pack_programs(programs, [q['prog_str_to_question_tokens'] for q in qs], [q['question'].shape[0] for q in qs])
    sizes = {}
    for ext in (0, 4):
        plan = C.c_void_p()
        check(lib.stair_plan_build(h, n, ip(prog_off), ip(tokens), ip(lo), ip(hi), ip(q_off), 64, (1 if train else 0) | ext, C.byref(plan)))
        info = PlanInfo()
        check(lib.stair_plan_get_info(plan, C.byref(info)))
        sizes[ext] = info.workspace_bytes
        cap = 8192
        nm = (C.c_char_p * cap)(); beg = (C.c_int64 * cap)(); end = (C.c_int64 * cap)()
        k = lib.stair_plan_regions(plan, h, nm, beg, end, cap)
        regs = sorted((beg[i], end[i], nm[i].decode()) for i in range(k))
        for a, b in zip(regs, regs[1:]):
            assert a[1] <= b[0], ('overlap', a, b)
        assert ('xpv' in {r[2] for r in regs}) == (ext == 0)
        nf = lib.stair_projection_floats(h, n, 64, int(q_off[-1]))
        assert nf > n * 64 * 4 * config['hidden_size']
        dummy = C.c_void_p(256)               # an aligned non-null address: the setter only records it (nothing is launched here)
        if ext:
            with pytest.raises(StairError, match='too small'):
                check(lib.stair_plan_set_projection(h, plan, dummy, nf - 1))
            check(lib.stair_plan_set_projection(h, plan, dummy, nf))
        else:
            with pytest.raises(StairError, match='EXT_PROJECTION'):
                check(lib.stair_plan_set_projection(h, plan, dummy, nf))
        lib.stair_plan_destroy(plan)
    saved = sizes[0] - sizes[4] - 4 * lib.stair_projection_floats(h, n, 64, int(q_off[-1]))
    assert 0 <= saved < 16384            # (alignment of the regions laid out behind them)
    assert lib.stair_projection_floats(h, -1, 64, 10) == -1
    lib.stair_ctx_destroy(h)


def test_common_subexpressions_are_aliased_not_recomputed():
    """STAIR_PLAN_NO_CSE off (default): nodes that depend only on the clip / keyword strings / identical spans alias the first
    occurrence -- across questions about one clip and inside one program (P0 evaluates the same Localize / Temporal / Filter
    chain twice); with the flag every node gets a slot of its own, as module_net.py:100-106 computes it."""
    from stair_amd._lib import PlanInfo
    config = dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, answer_vocab_length=16, max_video_length=40, object_types=10)
    h = _ctx(config)
    forms = ['P1', 'P1', 'P3', 'P3', 'P0', 'P7']
    progs = [synth.CORPUS[f][0] for f in forms]
    n = len(progs)
    # every span token of a program gets the span (1 + its phrase id): equal phrases -> equal spans
    spans = []
    for prog in progs:
        phrase = {}
        spans.append({i: (1 + phrase.setdefault(t, len(phrase)), 2 + phrase[t]) for i, t in enumerate(prog)
                      if t not in spec.OP_CODE and t not in spec.KW_CODE})
    prog_off, tokens, lo, hi, q_off = pack_programs(progs, spans, [9] * n)
    clip = np.asarray([0, 0, 1, 1, 2, 0], dtype=np.int32)       # questions 0, 1, 5 ask about clip 0; 2, 3 about clip 1
    info = {}
    slots = {}
    for flag in (0, 2):
        plan = C.c_void_p()
        check(lib.stair_plan_build_shared(h, n, ip(prog_off), ip(tokens), ip(lo), ip(hi), ip(q_off), 3, ip(clip), 40, flag, C.byref(plan)))
        inf = PlanInfo()
        check(lib.stair_plan_get_info(plan, C.byref(inf)))
        if flag == 2:
            # dropout on a TRAINING plan: every occurrence draws its own mask in the reference (module_net.py:100-106 under
            # model.train()), so a plan that shares nodes refuses p > 0 and an unshared one takes it
            for fl, ok in ((1, False), (1 | 2, True)):
                tplan = C.c_void_p()
                check(lib.stair_plan_build_shared(h, n, ip(prog_off), ip(tokens), ip(lo), ip(hi), ip(q_off), 3, ip(clip), 40, fl, C.byref(tplan)))
                rc = lib.stair_plan_set_dropout(tplan, C.c_float(0.25), C.c_uint64(7))
                assert (rc == 0) == ok, (fl, rc)
                if not ok:
                    assert b'STAIR_PLAN_NO_CSE' in lib.stair_last_error()
                    assert lib.stair_plan_set_dropout(tplan, C.c_float(0.0), C.c_uint64(0)) == 0
                lib.stair_plan_destroy(tplan)
        info[flag] = inf
        tab = [np.empty(inf.n_nodes, np.int32) for _ in range(5)]
        check(lib.stair_plan_nodes(plan, *[ip(t) for t in tab], inf.n_nodes))
        slots[flag] = tab
        lib.stair_plan_destroy(plan)
    assert info[2].n_aliased == 0 and info[0].n_aliased > 10
    assert info[0].n_map < info[2].n_map and info[0].n_vec < info[2].n_vec and info[0].workspace_bytes < info[2].workspace_bytes
    kind, slot = slots[0][0], slots[0][1]
    # question 1 is question 0 again on the same clip, but 'dish' is its own words: Filter(video, objects) is shared, Exists is not
    p0, p1 = prog_off[0], prog_off[1]
    assert slot[p0 + 2] == slot[p1 + 2] and slot[p0 + 0] != slot[p1 + 0]
    # P7 on clip 0 reuses that same Filter(video, objects) node (its token 10)
    p5 = prog_off[5]
    assert progs[5][10] == 'Filter' and slot[p5 + 10] == slot[p0 + 2]
    # P3 = Superlative(max, FilterFrame(video, actions), video): the whole program depends on the clip only
    p2, p3 = prog_off[2], prog_off[3]
    assert slot[p2 + 0] == slot[p3 + 0]
    # inside P0 the two identical Filter(Temporal(between, video, Localize(video, Array2(..))), holding) chains are one
    p4 = prog_off[4]
    assert progs[4][3] == 'Filter' and progs[4][17] == 'Filter' and slot[p4 + 3] == slot[p4 + 17]
    assert np.array_equal(slots[0][3], slots[2][3])              # levels do not change
    # without sharing every module node owns its slot
    k2, s2 = slots[2][0], slots[2][1]
    mods = [(k2[i], s2[i]) for q in range(n) for i in range(prog_off[q], prog_off[q + 1]) if progs[q][i - prog_off[q]] in spec.ARITY and progs[q][i - prog_off[q]] != 'Array2']
    assert len(set(mods)) == len(mods)
