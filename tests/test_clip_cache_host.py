"""Plans of cached clip encodings (STAIR_PLAN_VIDEO_ENCODED, include/stair_hip.h) and the ClipCache bookkeeping, on the host: the
plan builder and stair_plan_set_encoded_video enqueue nothing, so no GPU is needed."""
import ctypes as C

import numpy as np
import pytest
import torch

from stair_amd import spec, synth
from stair_amd._lib import lib, check, PlanInfo, StairError
from stair_amd.clip_cache import ClipCache
from helpers import build_plan, int32_ptr as ip

ENCODED, TRAIN = 8, 1
T = 64


def _forms(config):
    qs = [synth.make_question(config, 0, i, form=f, with_video=False) for i, f in enumerate(synth.ALL_FORMS)]
    assert len(qs) == 12
    return ([q['nmn_program_list'] for q in qs], [q['prog_str_to_question_tokens'] for q in qs], [q['question'].shape[0] for q in qs])


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
    return info, tab, regs


@pytest.mark.parametrize('shared', [False, True])
def test_encoded_plan_has_the_plain_plans_nodes_and_no_video_encoder_regions(shared):
    config = dict(spec.DEFAULT_CONFIG)
    H = config['hidden_size']
    kw = dict(video_of_question=[i // 3 for i in range(12)], n_videos=4) if shared else {}
    n_vid = 4 if shared else 12
    got = {}
    for flags in (0, ENCODED):
        h, plan, rc, _ = build_plan(config, *_forms(config), T, flags, **kw)
        assert rc == 0, lib.stair_last_error()
        got[flags] = _describe(h, plan)
        lib.stair_plan_destroy(plan)
        lib.stair_ctx_destroy(h)
    (pi, pt, pr), (ei, et, er) = got[0], got[ENCODED]
    assert (ei.n_nodes, ei.n_levels, ei.n_aliased) == (pi.n_nodes, pi.n_levels, pi.n_aliased)
    assert (ei.n_vec, ei.n_map, ei.n_att) == (pi.n_vec, pi.n_map, pi.n_att)
    if shared:
        assert ei.n_aliased > 0
    for a, b in zip(pt, et):
        assert np.array_equal(a, b)
    names = {r[2] for r in er}
    assert 'xpv' in {r[2] for r in pr}
    assert not names & {'xpv', 'wplanes', 'coop', 'vhn'}, names
    assert {'xpt', 'coop2', 'map', 'END'} <= names
    for a, b in zip(er, er[1:]):
        assert a[1] <= b[0], ('overlap', a, b)
    assert pi.workspace_bytes - ei.workspace_bytes >= n_vid * T * 4 * H * 4


def test_encoded_training_plan_is_refused_naming_both_flags():
    config = dict(spec.DEFAULT_CONFIG)
    h, plan, rc, _ = build_plan(config, *_forms(config), T, ENCODED | TRAIN)
    msg = lib.stair_last_error().decode()
    lib.stair_ctx_destroy(h)
    assert rc != 0 and 'STAIR_PLAN_VIDEO_ENCODED' in msg and 'STAIR_PLAN_TRAIN' in msg, msg


def test_set_encoded_video_refuses_a_short_cache_and_a_plain_plan():
    config = dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, answer_vocab_length=16, max_video_length=64, object_types=10)
    H = config['hidden_size']
    lens = [3, 17, 40, 64]
    rows = np.asarray([7, 2, 2, 5], np.int32)
    enc = C.c_void_p(256)             # an aligned non-null address: the setter only records it (nothing is launched here)
    h, plan, rc, _ = build_plan(config, *_forms(config), T, ENCODED, video_of_question=[i % 4 for i in range(12)], n_videos=4, video_len=lens)
    assert rc == 0, lib.stair_last_error()
    with pytest.raises(StairError, match=r'video_len\[3\] = 64 frames exceed the cache\'s rows_cap = 40'):
        check(lib.stair_plan_set_encoded_video(plan, enc, 40 * H, 40, ip(rows)))
    with pytest.raises(StairError, match='clip stride'):
        check(lib.stair_plan_set_encoded_video(plan, enc, 63 * H, 64, ip(rows)))
    with pytest.raises(StairError, match='negative'):
        check(lib.stair_plan_set_encoded_video(plan, enc, 64 * H, 64, ip(np.asarray([0, -1, 0, 0], np.int32))))
    check(lib.stair_plan_set_encoded_video(plan, enc, 64 * H, 64, ip(rows)))
    check(lib.stair_plan_set_encoded_video(plan, enc, 80 * H, 72, ip(rows)))
    lib.stair_plan_destroy(plan)
    lib.stair_ctx_destroy(h)
    h, plan, rc, _ = build_plan(config, *_forms(config), T, 0)
    with pytest.raises(StairError, match='STAIR_PLAN_VIDEO_ENCODED'):
        check(lib.stair_plan_set_encoded_video(plan, enc, 64 * H, 64, ip(rows)))
    lib.stair_plan_destroy(plan)
    lib.stair_ctx_destroy(h)


def test_text_projection_alone_has_no_video_regions():
    config = dict(spec.DEFAULT_CONFIG)
    h, plan, rc, _ = build_plan(config, *_forms(config), T, ENCODED | 4)
    assert rc == 0
    q_rows = sum(_forms(config)[2])
    nf0, nf = lib.stair_projection_floats(h, 0, T, q_rows), lib.stair_projection_floats(h, 12, T, q_rows)
    assert 0 < nf0 < nf - 12 * T * 4 * config['hidden_size']
    with pytest.raises(StairError, match='too small'):
        check(lib.stair_plan_set_projection(h, plan, C.c_void_p(256), nf0 - 1))
    check(lib.stair_plan_set_projection(h, plan, C.c_void_p(256), nf0))
    assert lib.stair_encode_clips_ws_bytes(h, 0, T, 32) == -1 and lib.stair_encode_clips_ws_bytes(h, 5, T, T) > 5 * T * 4 * 512 * 4
    assert lib.stair_encode_clips_ws_bytes(h, 5, 40, 64) - lib.stair_encode_clips_ws_bytes(h, 5, 40, 40) >= 5 * 40 * 512 * 4
    lib.stair_plan_destroy(plan)
    lib.stair_ctx_destroy(h)


class _Stub:
    """what VideoNMN hands a ClipCache, without a device: records the chunks, writes each clip's length into its rows"""

    def __init__(self):
        self.calls, self.state = [], ('bf16x3', 0)

    def encode(self, video, lens, out):
        self.calls.append((tuple(video.shape), video.dtype, lens.tolist()))
        assert out.shape[0] == video.shape[0]
        out.zero_()
        for i, L in enumerate(lens):
            out[i, :L] = float(L)

    def stamp(self):
        return self.state


def test_clip_cache_bookkeeping_on_a_stub():
    stub = _Stub()
    cache = ClipCache(8, 4, stub.encode, stub.stamp, 'cpu')
    assert len(cache) == 0 and cache.matmul_mode == 'bf16x3'
    clips = [torch.full((L, 6), float(L)) for L in (3, 8, 5)]
    rows = cache.add(clips, ids=['a', 'b', 'c'], batch_size=2)
    assert rows.tolist() == [0, 1, 2] and len(cache) == 3 and 'b' in cache and 'z' not in cache
    assert stub.calls == [((2, 8, 6), torch.float32, [3, 8]), ((1, 5, 6), torch.float32, [5])]      # chunks padded to their own longest clip
    assert cache.rows(['c', 'a', 'a']).tolist() == [2, 0, 0] and cache.rows(['c']).dtype == np.int32
    assert cache.lengths.tolist() == [3, 8, 5] and tuple(cache.enc.shape) == (3, 8, 4)
    with pytest.raises(KeyError, match="'nope'"):
        cache.rows(['a', 'nope'])
    # add() appends: earlier rows keep their number and their content when the storage grows
    before = cache.enc.clone()
    more = torch.zeros(4, 7, 6, dtype=torch.bfloat16)
    assert cache.add(more, ids=[10, 11, 12, 13], video_len=[7, 1, 2, 7]).tolist() == [3, 4, 5, 6]
    assert stub.calls[-1] == ((4, 7, 6), torch.bfloat16, [7, 1, 2, 7])
    assert torch.equal(cache.enc[:3], before) and cache.rows([12, 'b']).tolist() == [5, 1]
    assert cache.enc[4, 0, 0] == 1.0 and cache.enc[4, 1:].abs().max() == 0
    assert cache.add([torch.zeros(2, 6)]).tolist() == [7] and 7 in cache          # default ids: the row numbers
    n = len(cache)
    for bad, kw in (([torch.zeros(9, 6)], {}), ([torch.zeros(2, 6)], dict(ids=['a'])), ([torch.zeros(2, 6)] * 2, dict(ids=['x', 'x'])),
                    ([torch.zeros(2, 6)], dict(ids=['p', 'q'])), (torch.zeros(2, 3, 6), dict(video_len=[4, 1]))):
        with pytest.raises(ValueError):
            cache.add(bad, **kw)
    assert len(cache) == n and 'p' not in cache
    # a stale cache raises, it does not answer
    stub.state = ('bf16x3', 1)
    with pytest.raises(ValueError, match='re-encode'):
        cache.check()
    with pytest.raises(ValueError, match='stale'):
        cache.add([torch.zeros(2, 6)])
    stub.state = ('f32', 0)
    with pytest.raises(ValueError, match="matmul mode 'bf16x3'.*re-encode"):
        cache.check()
