"""One batch through every clip source of the batched pass (`-m gpu`): the clip features (run_programs(video, video_index,
video_len)), a ClipCache of them (run_programs(clips=cache, video_index=rows)) and the cache's encodings handed in as the caller's own
(logits(encoded=cache.enc, video_index=rows, video_len=cache.lengths)).

The last two read the same encodings through the same plan: same bits, same launches.  The first against the second is the comparison
of test_gpu_clip_cache.py::test_cached_logits_match_oracle_and_direct_pass -- the cache is filled in one call from the very tensor
the direct pass encodes, so the logits are bit-identical -- and one Trainer.step on either source with the video encoder frozen is
test_gpu_cached_train.py::test_cached_step_equals_the_direct_frozen_step_bit_for_bit at this shape.

Shape: the tiny configuration of smoke() (H = 64, V = 128, max_video_length = 40), the 12 program forms over 5 clips of 40, 24, 17,
40 and 9 frames, questions assigned to the clips with repeats and out of order; the three inference passes in fp32 matmul mode, the training steps in the default mode (the one
in which a step is bit-reproducible: see the test's docstring)."""
import functools

import pytest
import torch

from stair_amd import ops, spec, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TINY = dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, answer_vocab_length=16, max_video_length=40, object_types=10)
LENS = [40, 24, 17, 40, 9]
ROWS = [3, 3, 0, 4, 4, 4, 1, 0, 3, 1, 0, 2]            # the clip of every question: first use in the order 3, 0, 4, 1, 2
FIRST_USE = [3, 0, 4, 1, 2]


def _model(matmul_mode='f32'):
    from stair_amd.module_net import VideoNMN
    weights = synth.make_weights(TINY, 3)
    model = VideoNMN(TINY)
    model.load_state_dict({k: torch.from_numpy(weights[k].copy()) for k in spec.state_dict_keys(TINY)})
    model = model.to(DEV)
    model.set_option('matmul_mode', matmul_mode)
    return model


@functools.lru_cache(maxsize=None)
def _batch():
    """(programs and spans, padded clips with zeros behind each clip's frames, question rows, q_lens, answers): built once, left unchanged"""
    qs = [synth.make_question(TINY, 3, i, form=synth.ALL_FORMS[i], with_video=False) for i in range(12)]
    video = torch.randn(5, 40, TINY['video_size'], generator=torch.Generator().manual_seed(5))
    for c, L in enumerate(LENS):
        video[c, L:] = 0
    question = torch.cat([torch.as_tensor(q['question']) for q in qs]).to(DEV, torch.float32).contiguous()
    answers = torch.tensor([q['answer'] for q in qs], dtype=torch.int32, device=DEV)
    head = ([q['nmn_program_list'] for q in qs], [q['prog_str_to_question_tokens'] for q in qs])
    return head, video.to(DEV), question, [q['question'].shape[0] for q in qs], answers


def _encoded_pass(model, head, question, q_lens, enc, rows, lens):
    """the BatchResult of the inference pass behind logits(encoded=enc, ...), which hands out the logits alone"""
    if hasattr(model, '_run'):
        return model._run(model._clip_source(len(rows), None, rows, lens, None, enc), *head, question, q_lens, False, None, None, True)
    return model._run_cached(*head, question, q_lens, None, True, None, *model._encoded_args(enc, rows, lens, len(rows)), enc=enc)


def test_three_sources_one_pass():
    head, video, question, q_lens, _ = _batch()
    model = _model()
    cache = model.encode_clips(video, video_len=LENS)           # one call over the tensor the direct pass reads
    assert cache.matmul_mode == 'f32' and cache.lengths.tolist() == LENS
    a = model.run_programs(*head, video, question, q_lens, video_index=ROWS, video_len=LENS)
    a_logits, a_frames = a.logits.clone(), a.question_frames
    with ops.kernel_accounting() as acct_b:
        b = model.run_programs(*head, None, question, q_lens, clips=cache, video_index=ROWS)
    b_logits, b_pred = b.logits.clone(), b.pred.clone()
    with torch.no_grad(), ops.kernel_accounting() as acct_c:
        c_logits = model.logits(*head, None, question, q_lens, encoded=cache.enc, video_index=ROWS, video_len=cache.lengths).clone()
    c = _encoded_pass(model, head, question, q_lens, cache.enc, ROWS, cache.lengths)
    torch.cuda.synchronize()
    # (b), (c): the same encodings through the same plan
    assert torch.equal(b_logits, c_logits) and torch.equal(c.logits, c_logits)
    assert acct_b.table == acct_c.table and acct_b.table['gather_encoded_video'][0] == 1, (acct_b.table, acct_c.table)
    assert list(b.clip_rows) == list(c.clip_rows) == FIRST_USE
    assert list(b.question_frames) == list(c.question_frames) == [LENS[r] for r in ROWS] == list(a_frames)
    assert b.info.T == c.info.T == a.info.T == 40
    assert b._video is None and c._video is None and b._clips is cache and c._clips is None and c._enc.data_ptr() == cache.enc.data_ptr()
    # (a), (b): same clips, same composition of the encoder pass: bit-identical
    diff = float((a_logits - b_logits).abs().max())
    print('clip sources: max |cached - direct| = %.3g, largest logit %.3g' % (diff, float(a_logits.abs().max())))
    assert float(a_logits.abs().max()) > 0
    assert torch.equal(b_logits, a_logits), diff
    # a captured pass of (b) replays to the same bits
    cap = model.run_programs(*head, None, question, q_lens, clips=cache, video_index=ROWS).capture_graph()
    model.run_programs(*head, video, question, q_lens, video_index=ROWS, video_len=LENS)       # another batch through the shared workspace
    cap.logits.zero_()
    logits, pred = cap.replay()
    torch.cuda.synchronize()
    assert torch.equal(logits, b_logits) and torch.equal(pred, b_pred) and cap.result._clips is cache


def test_one_frozen_step_on_the_cache_equals_the_step_on_the_clips():
    """Bit for bit, in the matmul mode in which test_gpu_cached_train.py makes the claim: the default one (split bf16), where a
    training step is bit-reproducible.  In f32 mode it is not, on either source: measured on MI355X at this shape, two runs of the
    SAME step on the clips differ in 11-13 of 113 gradient tensors by up to 9.3e-10 (text encoder W_ih / W_hh, Filter, Temporal), two
    runs on the cache in 9-12, and cache against clips in 13-14 by the same 9.3e-10 (parameters after Adam: 7.8e-07) -- run-to-run
    rounding of that mode's sums, with equal losses.  In the default mode all three comparisons differ in 0 of 113."""
    from stair_amd.train import Trainer
    head, video, question, q_lens, answers = _batch()
    got = {}
    for cached in (False, True):
        model = _model(None)
        tr = Trainer(model, dropout=0.0, lr=1e-3, freeze=('video_encoder',))
        before = tr.flat_p.clone()
        if cached:
            cache = model.encode_clips(video, video_len=LENS)
            loss, res = tr.step(*head, None, question, q_lens, answers, video_index=ROWS, clips=cache)
            assert res._video is None and list(res.clip_rows) == FIRST_USE
        else:
            loss, res = tr.step(*head, video, question, q_lens, answers, video_index=ROWS, video_len=LENS)
        tr.check()
        assert res.info.T == 40 and list(res.question_frames) == [LENS[r] for r in ROWS]
        got[cached] = (loss.clone(), tr.flat_g.clone(), tr.flat_p.clone())
        assert not torch.equal(tr.flat_p, before)                   # the step did move the weights
    cache.check()                                                   # ... but not the encoder's: the cache is still fresh
    for what, x, y in zip(('loss', 'gradients', 'parameters'), got[False], got[True]):
        print('frozen step, %s: max |cached - direct| = %.3g' % (what, float((x - y).abs().max())))
    for what, x, y in zip(('loss', 'gradients', 'parameters'), got[False], got[True]):
        assert torch.equal(x, y), what
