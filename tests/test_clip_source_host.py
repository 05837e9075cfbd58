"""Where a plan's clips come from, on the host (no GPU: a CPU model, CPU tensors, a stub ClipCache): a ClipCache (run_programs(clips=),
logits(clips=)) and caller-made encodings (logits(encoded=)) that name the same rows with the same lengths yield the same plan clips,
and every refusal of the three forms raises its exception and message before any plan is built."""
import numpy as np
import pytest
import torch

from stair_amd import spec, synth
from stair_amd._lib import lib
from stair_amd.clip_cache import ClipCache
from stair_amd.module_net import VideoNMN

TINY = dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, answer_vocab_length=16, max_video_length=40, object_types=10)
LENS = [40, 24, 17, 40, 9]


def _plan_clips(model, n, video_index, clips=None, encoded=None, video_len=None):
    """(rows of the plan's clips in order of first use, clip of every question, frames of every clip, T) of an inference pass"""
    if hasattr(model, '_clip_source'):
        s = model._clip_source(n, None, video_index, video_len, clips, encoded)
        return s.rows, s.index, np.full(s.n_videos, s.T, np.int32) if s.lens is None else s.lens, s.T
    if clips is not None:
        return model._run_cached_args(clips, None, video_index, video_len, n, False, None)
    return model._encoded_args(encoded, video_index, video_len, n)


def _cache(model, lens, rows_cap=None):
    """a ClipCache without a device, as test_clip_cache_host.py builds one: the stub writes each clip's length into its rows"""
    def encode(video, clen, out):
        out.zero_()
        for i, L in enumerate(clen):
            out[i, :L] = float(L)
    cache = ClipCache(rows_cap or model.config['max_video_length'], model.config['hidden_size'], encode, lambda: ('f32', 0), 'cpu')
    cache.add([torch.zeros(L, model.config['video_size']) for L in lens])
    return cache


def _batch(config, n=12):
    qs = [synth.make_question(config, 0, i, form=synth.ALL_FORMS[i % 12], with_video=False) for i in range(n)]
    question = torch.cat([torch.as_tensor(q['question']) for q in qs]).float()
    return ([q['nmn_program_list'] for q in qs], [q['prog_str_to_question_tokens'] for q in qs]), question, [q['question'].shape[0] for q in qs]


@pytest.fixture
def builds():
    """counts the plans built while the test runs (a wrapper on the library's stair_plan_build_ragged, taken off afterwards)"""
    real, calls = lib.stair_plan_build_ragged, []

    def counting(*args):
        calls.append(1)
        return real(*args)
    lib.stair_plan_build_ragged = counting
    yield calls
    lib.stair_plan_build_ragged = real


@pytest.mark.parametrize('rows', [[0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1],          # in order, with repeats
                                  [3, 3, 0, 4, 4, 4, 1, 0, 3, 1, 0, 4],          # out of order; row 2 is not used
                                  [2] * 12,                                       # one clip for all
                                  [4, 2, 1, 4, 2, 1, 4, 2, 1, 4, 2, 1]])         # the 40-frame clips are not used: T = 24
def test_cache_and_encodings_yield_the_same_plan_clips(rows):
    model = VideoNMN(TINY)
    cache = _cache(model, LENS)
    got_c = _plan_clips(model, len(rows), rows, clips=cache)
    got_e = _plan_clips(model, len(rows), rows, encoded=cache.enc.clone(), video_len=LENS)
    first_use = list(dict.fromkeys(rows))
    want = (first_use, [first_use.index(r) for r in rows], [LENS[r] for r in first_use], max(LENS[r] for r in first_use))
    for got in (got_c, got_e):
        used, index, lens, T = got
        assert (list(used), list(index), list(lens), int(T)) == want
        assert all(np.asarray(a).dtype == np.int32 for a in (used, index, lens))


def test_encodings_without_video_index_or_video_len():
    model = VideoNMN(TINY)
    enc = torch.zeros(12, 24, TINY['hidden_size'])
    used, index, lens, T = _plan_clips(model, 12, None, encoded=enc)          # question q asks about clip q, every clip has 24 frames
    assert list(used) == list(range(12)) and list(index) == list(range(12)) and list(lens) == [24] * 12 and T == 24


def test_refusals_raise_before_any_plan_is_built(builds):
    model = VideoNMN(TINY)
    H = TINY['hidden_size']
    cache = _cache(model, LENS)
    head, question, q_lens = _batch(TINY)
    rows = [3, 3, 0, 4, 4, 4, 1, 0, 3, 1, 0, 4]
    enc = cache.enc.clone()
    video = torch.zeros(5, 40, TINY['video_size'])

    def cached(**kw):
        return model.run_programs(*head, kw.pop('video', None), question, q_lens, clips=cache, **kw)

    def encoded(e, **kw):
        return model.logits(*head, kw.pop('video', None), question, q_lens, encoded=e, **kw)

    # a trainable video encoder (the model as constructed) under train=True / grad mode
    with pytest.raises(ValueError, match='training on cached encodings needs a frozen video encoder'):
        cached(video_index=rows, train=True)
    with pytest.raises(ValueError, match='training on cached encodings needs a frozen video encoder'):
        model.logits(*head, None, question, q_lens, clips=cache, video_index=rows)
    with pytest.raises(ValueError, match='training on cached encodings needs a frozen video encoder'):
        encoded(enc.clone().requires_grad_(True), video_index=rows, video_len=LENS)
    # dropout without train=True
    with pytest.raises(ValueError, match=r'dropout is a training-mode operation \(train=True\); this pass on cached clips is inference'):
        cached(video_index=rows, dropout=(0.1, 3))
    with torch.no_grad():                   # (the encodings form under no_grad is inference: the checks of its arguments are reached)
        # video given together with the encodings
        with pytest.raises(ValueError, match='video given together with clips: a pass on cached clips takes video=None and no video_len'):
            cached(video=video, video_index=rows)
        with pytest.raises(ValueError, match='video given together with clips: a pass on cached clips takes video=None and no video_len'):
            cached(video_index=rows, video_len=LENS)
        with pytest.raises(ValueError, match='video given together with clips= / encoded=: a pass on encoded clips takes video=None'):
            encoded(enc, video=video, video_index=rows)
        with pytest.raises(ValueError, match='video given together with clips= / encoded=: a pass on encoded clips takes video=None'):
            model.logits(*head, None, question, q_lens, clips=cache, encoded=enc, video_index=rows)
        # no video_index
        with pytest.raises(ValueError, match='video_index is required with clips=: the cache row of every question'):
            cached()
        with pytest.raises(ValueError, match='video_index is required when encoded holds another number of clips than there are questions'):
            encoded(enc, video_len=LENS)
        # a row out of range, a row per question
        for bad in ([5] + rows[1:], [-1] + rows[1:], rows[:-1], np.zeros((12, 1), np.int32)):
            with pytest.raises(ValueError, match=r'video_index must hold one row of the cache \(0 \.\. 4\) per question'):
                cached(video_index=bad)
            with pytest.raises(ValueError, match=r'video_index must hold one row of encoded \(0 \.\. 4\) per question'):
                encoded(enc, video_index=bad, video_len=LENS)
        # encodings of the wrong shape, dtype, layout or frame count
        for bad in (enc[:, :, :H - 4], enc[0], enc[:0], 'enc'):
            with pytest.raises(ValueError, match=r'encoded must be a float32 \[n_clips, T, 64\] tensor of clip encodings, got shape'):
                encoded(bad, video_index=rows, video_len=LENS)
        for bad in (enc.double(), enc.transpose(0, 1), enc[:, ::2]):
            with pytest.raises(ValueError, match="encoded must be a contiguous float32 tensor on the model's device cpu"):
                encoded(bad, video_index=rows, video_len=LENS)
        with pytest.raises(ValueError, match='encoded holds 41 frames per clip, max_video_length is 40'):
            encoded(torch.zeros(5, 41, H), video_index=rows)
        for bad in (LENS[:-1], [0] + LENS[1:], [41] + LENS[1:]):
            with pytest.raises(ValueError, match=r'video_len must hold the frames \(1 \.\. 40\) of each of the 5 encoded clips'):
                encoded(enc, video_index=rows, video_len=bad)
        # a cache of another configuration
        with pytest.raises(ValueError, match='the clip cache belongs to another configuration or device'):
            model.run_programs(*head, None, question, q_lens, clips=ClipCache(40, 32, None, lambda: ('f32', 0), 'cpu'), video_index=rows)
    assert not builds


def test_linear_temporal_configuration_refuses_a_short_clip_in_both_forms(builds):
    config = dict(TINY, max_video_length=8)
    model = VideoNMN(config)
    cache = _cache(model, [8, 8, 5])
    head, question, q_lens = _batch(config)
    full, short = [0, 1] * 6, [0, 2] * 6
    assert _plan_clips(model, 12, full, clips=cache)[3] == 8
    with torch.no_grad():
        with pytest.raises(ValueError, match=r'Linear-Temporal configurations \(max_video_length <= 32\) need every clip at max_video_length = 8 frames'):
            model.run_programs(*head, None, question, q_lens, clips=cache, video_index=short)
        with pytest.raises(ValueError, match=r'Linear-Temporal configurations \(max_video_length <= 32\) need every clip at max_video_length = 8 frames'):
            model.logits(*head, None, question, q_lens, encoded=cache.enc.clone(), video_index=short, video_len=[8, 8, 5])
    # a Linear-Temporal plan has T = max_video_length whatever the clips' rows hold
    assert _plan_clips(model, 12, full, encoded=cache.enc.clone(), video_len=[8, 8, 5])[3] == 8
    assert not builds
