"""First-touch stores of the backward pass, plan side (host code only, no kernel is launched): which gradient tiles of the
map arena a training plan marks as stored by their first writer (a tile chain that writes the whole [T, H] tile) and which it
lists for the clear, reported by stair_plan_store_first_counts."""
import ctypes as C

import numpy as np
import pytest

from stair_amd import spec, synth
from stair_amd._lib import lib, check, PlanInfo
from helpers import build_plan


def _counts(config, programs, spans, q_lens, T, video_of_question=None, n_videos=None, video_len=None, train=True):
    """(n_store_first, n_cleared, PlanInfo) of the plan of a batch."""
    h, plan, rc, _ = build_plan(config, programs, spans, q_lens, T, 1 if train else 0, video_of_question, n_videos, video_len)
    try:
        assert rc == 0, lib.stair_last_error()
        info = PlanInfo()
        check(lib.stair_plan_get_info(plan, C.byref(info)))
        a, b = C.c_int32(-1), C.c_int32(-1)
        rc = lib.stair_plan_store_first_counts(plan, C.byref(a), C.byref(b))
        return rc, a.value, b.value, info
    finally:
        if plan:
            lib.stair_plan_destroy(plan)
        lib.stair_ctx_destroy(h)


def _one(program):
    """One question with a hand-written program at the full configuration: (stored, cleared, n_map, n_map_stage)."""
    spans = {i: (1 + i % 14, 2 + i % 14) for i in range(len(program))}       # different keywords: no common subexpressions
    rc, stored, cleared, info = _counts(dict(spec.DEFAULT_CONFIG), [program], [spans], [16], 64)
    assert rc == 0, lib.stair_last_error()
    assert stored + cleared == info.n_map + info.n_map_stage
    return stored, cleared, info.n_map, info.n_map_stage


def test_clip_read_by_one_filter_is_stored():
    # the clip tile is the only map value; Filter's chain is its only (hence first) writer
    assert _one(['Exists', 'dish', 'Filter', 'video', 'objects']) == (1, 0, 1, 0)


def test_clip_read_by_row_kernels_only_is_cleared():
    # the clip is read by AttnVideo (level 2) and ExistsFrame (level 1), both row kernels: cleared.  AttnVideo's output tile is read
    # by Filter alone: stored.
    assert _one(['Filter', 'AttnVideo', 'video', 'ExistsFrame', 'cup', 'video', 'cup']) == (1, 1, 2, 0)


def test_two_filters_at_one_level_store_the_slot_and_the_staging_tile():
    # both Filters (different weights: not one common subexpression) read the clip at level 1: the first writes the slot, the second
    # its staging tile, each for the first time
    assert _one(['Equals', 'Filter', 'video', 'holding', 'Filter', 'video', 'objects']) == (2, 0, 1, 1)


def test_chains_at_two_levels_mark_only_the_higher_one():
    # the clip is read by Temporal (level 2) and by Localize (level 1): the backward pass reaches Temporal first, its chain stores the
    # clip's tile and Localize's adds -- one mark for that tile; the second mark is Temporal's output tile, read by Filter alone
    assert _one(['Choose', 'dish', 'blanket', 'Filter', 'Temporal', 'while', 'video', 'Localize', 'video', 'holding_a_dish',
                 'holding']) == (2, 0, 2, 0)


def test_row_kernel_above_a_chain_keeps_the_clear():
    # AttnVideo (level 3, a row kernel) is the clip tile's first writer, so the tile is cleared although Temporal and Localize below are
    # chains; AttnVideo's and Temporal's output tiles have one chain reader each (Filter, HasItem... see P2) and FilterFrame's has HasItem
    stored, cleared, n_map, n_stage = _one(synth.CORPUS['P2'][0])
    assert cleared >= 1 and stored >= 1


def test_clip_no_map_module_reads_is_cleared():
    # no module reads the clip; its gradient tile still feeds BPTT and must be zero
    stored, cleared, n_map, n_stage = _one(['Exists', 'door', 'ToAction', 'holding', 'dish'])
    assert (stored, n_stage) == (0, 0) and cleared == n_map >= 1


@pytest.mark.parametrize('n_q,shared,ragged', [(48, False, False), (256, True, False), (256, True, True), (2048, False, False)])
def test_counts_cover_every_map_tile_of_a_mixed_batch(n_q, shared, ragged):
    config = dict(spec.DEFAULT_CONFIG)
    qs = [synth.make_question(config, 21, i, T=64, forms=synth.ALL_FORMS, with_video=False) for i in range(n_q)]
    n_videos = n_q // 2 if shared else n_q
    voq = [i % n_videos for i in range(n_q)] if (shared or ragged) else None
    vl = [64 - (i * 7) % 40 for i in range(n_videos)] if ragged else None
    rc, stored, cleared, info = _counts(config, [q['nmn_program_list'] for q in qs], [q['prog_str_to_question_tokens'] for q in qs],
                                        [q['question'].shape[0] for q in qs], 64, voq, n_videos, vl)
    assert rc == 0, lib.stair_last_error()
    assert stored + cleared == info.n_map + info.n_map_stage
    assert stored > 0 and cleared > 0          # (C0's AttnVideo reads the clip above every chain: some tiles stay in the clear)
    if shared:
        assert info.n_map_stage > 0
    print('n_q=%d shared=%s ragged=%s: %d of %d map gradient tiles stored by their first writer, %d cleared'
          % (n_q, shared, ragged, stored, info.n_map + info.n_map_stage, cleared))


def test_inference_plans_have_no_counts():
    program = ['Exists', 'dish', 'Filter', 'video', 'objects']
    rc, _, _, _ = _counts(dict(spec.DEFAULT_CONFIG), [program], [{i: (1, 2) for i in range(len(program))}], [8], 64, train=False)
    assert rc != 0 and b'STAIR_PLAN_TRAIN' in lib.stair_last_error()


def test_a_configuration_without_tile_chains_marks_nothing():
    """hidden_size 64 runs the launch-per-layer backward: every tail adds, so every tile is in the clear."""
    config = dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, answer_vocab_length=16, max_video_length=40, object_types=10)
    program = ['Equals', 'Filter', 'video', 'holding', 'Filter', 'video', 'objects']
    rc, stored, cleared, info = _counts(config, [program], [{i: (1, 2) for i in range(len(program))}], [8], 40)
    assert rc == 0, lib.stair_last_error()
    assert stored == 0 and cleared == info.n_map + info.n_map_stage == 2
