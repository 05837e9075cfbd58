"""Questions answered from cached clip encodings (VideoNMN.encode_clips -> ClipCache -> run_programs(clips=...) /
forward_batch(clip_cache=...); STAIR_PLAN_VIDEO_ENCODED, stair_encode_clips, stair_plan_set_encoded_video).

The cached pass must compute what the direct pass computes: the gather puts the cached rows into the plan's map slots bit for bit
with exact zeros behind each clip's end, the logits match the oracle (1e-4, same top-1) and the direct pass on the same questions
(2e-6, the bound between two batch compositions of the same questions, tests/test_gpu_ragged.py), the video encoder does not run, a
captured pass replays bit for bit, and a cache that no longer belongs to the model's weights or matmul mode raises.

Observed on MI355X: with the cache filled from the very clip tensors the direct pass encodes, in one call over the same clips,
max |cached logits - direct logits| is 0 at both sizes (tiny fp32; full fp32 and bf16 clips) -- the encoder's rows do not depend on
whether the text recurrence shares its launch -- so test_cached_logits_match_oracle_and_direct_pass asserts equality there; against
another batch composition (a subset of the questions, a cache filled in chunks) the bound is the 2e-6 of tests/test_gpu_ragged.py."""
import functools
import json
import os

import pytest
import torch

from oracle import nmn_oracle as O
from stair_amd import ops, spec, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LENS = (3, 17, 40, 64)
TINY = dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, answer_vocab_length=16, max_video_length=64, object_types=10)
FULL = dict(spec.DEFAULT_CONFIG)
BOUND_DIRECT = 2e-6


def _maxerr(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) if a.numel() else 0.0


def _model(config, seed):
    from stair_amd.module_net import VideoNMN
    weights = synth.make_weights(config, seed)
    model = VideoNMN(config)
    model.load_state_dict({k: torch.from_numpy(weights[k].copy()) for k in spec.state_dict_keys(config)})
    return model.to(DEV), weights


@functools.lru_cache(maxsize=None)
def _case(size, bf16):
    """(config, model, weights, questions with 'video_id' = their index, cache of their clips, direct logits): built once, left unchanged"""
    config, n = (TINY, 36) if size == 'tiny' else (FULL, 24)
    model, weights = _model(config, 4)
    qs = [synth.make_question(config, 4, i, form=synth.ALL_FORMS[i % len(synth.ALL_FORMS)], T=LENS[(i // 3) % len(LENS)]) for i in range(n)]
    for i, q in enumerate(qs):
        q['video_id'] = i
        if bf16:
            q['video_features'] = torch.as_tensor(q['video_features']).to(torch.bfloat16)
    cache = model.encode_clips([q['video_features'] for q in qs], ids=list(range(n)))
    direct = model.forward_batch(qs).logits.clone()
    return config, model, weights, qs, cache, direct


def _dirty_workspace(config, model):
    """a 64-frame batch through the same model: the shared workspace then holds non-zero rows where a shorter clip's zero tail must go"""
    qs = [synth.make_question(config, 77, i, form=synth.ALL_FORMS[i % 12], T=64) for i in range(12)]
    res = model.forward_batch(qs)
    assert res.info.T == 64 and float(res.logits.abs().max()) > 0


def _check_gather(res, cache, H):
    info = res.info
    maps = res._arena(info.map_off, info.n_map * info.T, H).view(info.n_map, info.T, H)
    assert len(res.clip_rows) <= info.n_map
    for v, row in enumerate(res.clip_rows):
        L = int(cache.lengths[row])
        assert L <= info.T
        assert torch.equal(maps[v, :L].view(torch.int32), cache.enc[row, :L].view(torch.int32)), (v, row)       # byte-identical
        assert int((maps[v, L:].view(torch.int32) != 0).sum()) == 0, (v, row, L)                                # exact (+0) zeros behind it
        assert int((cache.enc[row, L:].view(torch.int32) != 0).sum()) == 0
        assert float(cache.enc[row, :L].abs().max()) > 0


@pytest.mark.parametrize('size', ['tiny', 'full'])
@pytest.mark.parametrize('case', ['cap_above_T', 'cap_equals_T', 'permuted_repeats', 'one_clip'])
def test_gather_is_exact(size, case):
    config, model, _, qs, cache, direct = _case(size, False)
    H = config['hidden_size']
    frames = [q['video_features'].shape[0] for q in qs]
    if case == 'cap_above_T':               # the cache keeps 64 rows per clip, the plan's T is 40
        pick = [i for i, L in enumerate(frames) if L <= 40]
    elif case == 'cap_equals_T':
        pick = list(range(len(qs)))
    elif case == 'permuted_repeats':        # rows out of order and repeated
        pick = [7, 2, 2, 5, 0]
    else:
        pick = [9]                          # (a 64-frame clip)
    _dirty_workspace(config, model)
    batch = [qs[i] for i in pick]
    res = model.forward_batch(batch, clip_cache=cache)
    want_T = max(frames[i] for i in pick)
    assert res.info.T == want_T and cache.rows_cap == 64 and res._video is None
    assert (want_T < cache.rows_cap) == (case in ('cap_above_T', 'permuted_repeats'))
    first_use = list(dict.fromkeys(pick))
    assert list(res.clip_rows) == first_use
    _check_gather(res, cache, H)
    assert _maxerr(res.logits, direct[pick]) < BOUND_DIRECT


@pytest.mark.parametrize('size,bf16', [('tiny', False), ('full', False), ('full', True)])
def test_cached_logits_match_oracle_and_direct_pass(size, bf16):
    config, model, weights, qs, cache, direct = _case(size, bf16)
    res = model.forward_batch(qs, clip_cache=cache)
    logits, pred = res.logits.cpu(), res.pred.cpu()
    assert sorted(set(int(x) for x in res.question_frames)) == sorted(LENS)
    w = O.to_torch(weights)
    worst = 0.0
    for i, q in enumerate(qs):
        v = q['video_features']
        ref = O.forward(w, config, dict(q, video_features=v.float() if isinstance(v, torch.Tensor) else v), return_res_by_step=False)['logits']
        worst = max(worst, _maxerr(logits[i], ref))
        assert _maxerr(logits[i], ref) < 1e-4, (q['form'], _maxerr(logits[i], ref))
        assert int(pred[i]) == int(torch.argmax(ref)), q['form']
    diff = _maxerr(logits, direct)
    print('clip cache %s bf16=%s: max |cached - oracle| = %.3g, max |cached - direct| = %.3g' % (size, bf16, worst, diff))
    assert torch.equal(logits, direct.cpu()), diff          # same clips, same composition of the encoder pass: bit-identical


def test_every_node_matches_the_direct_pass_and_is_zero_behind_the_clips_end():
    from stair_amd.module_net import VAL_MAP, VAL_ATT, VAL_FRAME
    config, model, _, qs, cache, _ = _case('tiny', False)
    d = model.forward_batch(qs)
    want = [[d.node(q, i).clone() if isinstance(d.node(q, i), torch.Tensor) else d.node(q, i) for i in range(len(qs[q]['nmn_program_list']))]
            for q in range(len(qs))]
    _dirty_workspace(config, model)
    res = model.forward_batch(qs, clip_cache=cache)
    checked = padded = 0
    for q in range(len(qs)):
        L = qs[q]['video_features'].shape[0]
        for i in range(len(qs[q]['nmn_program_list'])):
            got = res.node(q, i)
            if not isinstance(got, torch.Tensor):
                assert got == want[q][i]
                continue
            assert _maxerr(got, want[q][i]) < BOUND_DIRECT, (q, i, qs[q]['nmn_program_list'][i])
            checked += 1
            kind = res.node_info(q, i)[0]
            if kind in (VAL_MAP, VAL_ATT, VAL_FRAME) and L < res.info.T:
                tail = got[L:] if kind in (VAL_MAP, VAL_FRAME) else got[:, L:]
                assert tail.numel() and int((tail != 0).sum()) == 0, (q, i, qs[q]['nmn_program_list'][i])
                padded += 1
    assert checked > 200 and padded > 50, (checked, padded)


def test_cache_filled_in_chunks_gives_the_same_logits():
    config, model, _, qs, cache, _ = _case('tiny', False)
    clips = [q['video_features'] for q in qs]
    whole = model.forward_batch(qs, clip_cache=cache).logits.clone()
    chunked = model.encode_clips(clips, ids=list(range(len(qs))), batch_size=5)
    single = model.encode_clips(clips[:1], ids=[0])
    for i in range(1, len(qs)):
        single.add(clips[i:i + 1], ids=[i])
    assert len(chunked) == len(single) == len(cache) and single.lengths.tolist() == cache.lengths.tolist()
    for other in (chunked, single):
        assert _maxerr(model.forward_batch(qs, clip_cache=other).logits, whole) < BOUND_DIRECT
        assert _maxerr(other.enc, cache.enc) < BOUND_DIRECT


def test_shared_cached_clips_alias_and_cse_changes_no_bit():
    config, model, _, qs, cache, direct = _case('full', False)
    batch = []
    for i in range(24):                     # questions 3k, 3k+1, 3k+2 ask about the clip of 3k
        batch.append(dict(qs[i], video_id=3 * (i // 3), video_features=qs[3 * (i // 3)]['video_features']))
    rows = cache.rows([b['video_id'] for b in batch])
    args = ([b['nmn_program_list'] for b in batch], [b['prog_str_to_question_tokens'] for b in batch])
    question = torch.cat([torch.as_tensor(b['question']) for b in batch]).to(DEV, torch.float32).contiguous()
    q_lens = [b['question'].shape[0] for b in batch]
    on = model.run_programs(*args, None, question, q_lens, clips=cache, video_index=rows, cse=True)
    on_logits = on.logits.clone()
    assert on.info.n_aliased > 0 and len(on.clip_rows) == 8 and on.info.n_map >= 8
    off = model.run_programs(*args, None, question, q_lens, clips=cache, video_index=rows, cse=False)
    assert off.info.n_aliased == 0
    assert torch.equal(on_logits, off.logits)
    assert _maxerr(on_logits, model.forward_batch(batch).logits) < BOUND_DIRECT


def test_the_video_encoder_does_not_run():
    config, model, _, qs, cache, _ = _case('full', True)
    H, Ep = config['hidden_size'], (config['text_size'] + 31) // 32 * 32
    rows_q = sum(q['question'].shape[0] for q in qs)
    with ops.kernel_accounting() as direct:
        model.forward_batch(qs)
    assert direct.table['gemm_planes'][0] == 2                       # the control: video and text projections
    with ops.kernel_accounting() as acct:
        res = model.forward_batch(qs, clip_cache=cache)
        torch.cuda.synchronize()
    t = acct.table
    assert t['gemm_planes'][0] == 1 and t['gemm_planes'][2] == 2 * rows_q * 4 * H * Ep, t['gemm_planes']
    rec = {k: v for k, v in t.items() if k.startswith('lstm_rec')}
    assert 'lstm_rec_coop_pair' not in rec and sum(v[0] for v in rec.values()) == 1, rec
    assert sum(v[2] for v in rec.values()) == 2 * 2 * rows_q * 4 * (H // 2) * (H // 2), rec          # the text encoder's alone
    n_vid, T = len(res.clip_rows), res.info.T
    assert t['gather_encoded_video'][:2] == (1, 2 * n_vid * T * H * 4), t['gather_encoded_video']
    assert 'gather_encoded_video' not in direct.table


def test_captured_cached_plan_replays_bit_exactly():
    config, model, _, qs, cache, _ = _case('full', False)
    eager = model.forward_batch(qs, clip_cache=cache)
    want, want_pred = eager.logits.clone(), eager.pred.clone()
    cap = model.forward_batch(qs, clip_cache=cache).capture_graph()
    for rep in range(3):
        model.forward_batch(qs[:5])                 # another batch through the shared workspace in between
        cap.logits.zero_()
        logits, pred = cap.replay()
        torch.cuda.synchronize()
        assert torch.equal(logits, want) and torch.equal(pred, want_pred), rep
    assert cap.result._clips is cache


def _pack(qs):
    video = torch.stack([torch.as_tensor(q['video_features']).float() for q in qs]).to(DEV).contiguous()
    question = torch.cat([torch.as_tensor(q['question']) for q in qs]).to(DEV, torch.float32).contiguous()
    answers = torch.tensor([q['answer'] for q in qs], dtype=torch.int32, device=DEV)
    return ([q['nmn_program_list'] for q in qs], [q['prog_str_to_question_tokens'] for q in qs], video, question,
            [q['question'].shape[0] for q in qs], answers)


def test_refusals():
    config = TINY
    model, weights = _model(config, 6)
    qs = [synth.make_question(config, 6, i, form=synth.ALL_FORMS[i], T=40) for i in range(12)]
    for i, q in enumerate(qs):
        q['video_id'] = 'clip%d' % i
    fresh = lambda: model.encode_clips([q['video_features'] for q in qs], ids=[q['video_id'] for q in qs])
    cache = fresh()
    model.forward_batch(qs, clip_cache=cache)
    with pytest.raises(ValueError, match='training on cached encodings'):
        model.forward_batch(qs, clip_cache=cache, train=True)
    with pytest.raises(ValueError, match='dropout'):
        model.forward_batch(qs, clip_cache=cache, dropout=(0.1, 3))
    with pytest.raises(KeyError, match='clip99'):
        model.forward_batch([dict(qs[0], video_id='clip99')], clip_cache=cache)
    with pytest.raises(ValueError, match='video_index is required'):
        model.run_programs(*_pack(qs)[:2], None, *_pack(qs)[3:5], clips=cache)
    with pytest.raises(ValueError, match='video_index must hold'):
        model.run_programs(*_pack(qs)[:2], None, *_pack(qs)[3:5], clips=cache, video_index=[12] * 12)
    # another matmul mode than the cache was made in: process-wide, and as this model's own option
    ops.set_matmul_mode('f32')
    try:
        with pytest.raises(ValueError, match='matmul mode.*re-encode'):
            model.forward_batch(qs, clip_cache=cache)
    finally:
        ops.set_matmul_mode('bf16x3')
    model.set_option('matmul_mode', 'f32')
    with pytest.raises(ValueError, match='matmul mode.*re-encode'):
        model.forward_batch(qs, clip_cache=cache)
    model.set_option('matmul_mode', None)
    model.forward_batch(qs, clip_cache=cache)
    # the video-encoder weights changed: an in-place update, load_state_dict with other weights, one Trainer.step
    with torch.no_grad():
        model.submodules['video_encoder'].bias_ih_l0.add_(1e-3)
    with pytest.raises(ValueError, match='stale.*re-encode'):
        model.forward_batch(qs, clip_cache=cache)
    cache = fresh()
    model.forward_batch(qs, clip_cache=cache)
    other = synth.make_weights(config, 7)
    model.load_state_dict({k: torch.from_numpy(other[k].copy()) for k in spec.state_dict_keys(config)})
    with pytest.raises(ValueError, match='stale.*re-encode'):
        model.forward_batch(qs, clip_cache=cache)
    from stair_amd.train import Trainer
    tr = Trainer(model, dropout=0.0, lr=1e-3)
    cache = fresh()
    before = model.forward_batch(qs, clip_cache=cache).logits.clone()
    tr.step(*_pack(qs))
    tr.check()
    with pytest.raises(ValueError, match='stale.*re-encode'):
        model.forward_batch(qs, clip_cache=cache)
    after = model.forward_batch(qs, clip_cache=fresh()).logits
    assert _maxerr(after, model.forward_batch(qs).logits) < BOUND_DIRECT and _maxerr(after, before) > 1e-5      # the step did move the answers


def test_linear_temporal_configuration_refuses_a_short_clip():
    config = dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, answer_vocab_length=16, max_video_length=8, object_types=10)   # the tiny_linear shape
    model, _ = _model(config, 2)
    qs = [synth.make_question(config, 2, i, form=synth.ALL_FORMS[i], T=8) for i in range(12)]
    for i, q in enumerate(qs):
        q['video_id'] = i
    clips = [q['video_features'] for q in qs]
    cache = model.encode_clips(clips, ids=list(range(12)))
    assert cache.rows_cap == 8
    assert _maxerr(model.forward_batch(qs, clip_cache=cache).logits, model.forward_batch(qs).logits) < BOUND_DIRECT
    cache.add([torch.as_tensor(clips[0])[:5]], ids=['short'])
    with pytest.raises(ValueError, match='max_video_length = 8'):
        model.forward_batch([dict(qs[0], video_id='short'), qs[1]], clip_cache=cache)
    with pytest.raises(ValueError, match='rows_cap'):
        cache.add([torch.zeros(9, 128)], ids=['long'])


def test_evaluate_drivers_return_the_same_with_a_cache():
    from stair_amd import data as D, evaluate as E
    mini = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'agqa_mini')
    recs = D.filter_records(D.load_question_records(os.path.join(mini, 'records.json')), 'valid')
    clips = D.load_clip_features(os.path.join(mini, 'clips'), {r['video_id'] for r in recs}, 10)
    vocab = D.load_answer_vocab(os.path.join(mini, 'vocab.json'))
    ds = D.AGQAQuestions(recs, clips, D.load_glove(os.path.join(mini, 'glove.txt')), vocab, split='valid',
                         video_secs=json.load(open(os.path.join(mini, 'video_secs.json'))), tokenize=str.split)
    config = dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=16, text_size=8, answer_vocab_length=ds.answer_vocab_length(),
                  max_video_length=40, object_types=10)
    model, _ = _model(config, 5)
    items = [ds[i] for i in range(len(ds))]
    ids = sorted(clips)
    cache = model.encode_clips([clips[k] for k in ids], ids=ids, batch_size=3)
    assert E.predict(model, items, batch_size=4, clip_cache=cache) == E.predict(model, items, batch_size=4)
    unk = vocab['word2id']['<UNK>']
    assert E.evaluate(model, items, unk, batch_size=3, clip_cache=cache) == E.evaluate(model, items, unk, batch_size=3)
    phrases = ['phrase %d' % c for c in range(12)]
    embs = [synth.class_embedding(config, 5, c) for c in range(12)]
    got = E.filter_text_results(model, items, phrases, embs, batch_size=5, top=3, clip_cache=cache)
    assert got == E.filter_text_results(model, items, phrases, embs, batch_size=5, top=3)
    assert sum(len(v) for v in got.values()) == sum(it['nmn_program_list'].count('Filter') for it in items)
    acc, valid = E.evaluate_by_module(model, items, unk, batch_size=4, module_loss_weight=0, clip_cache=cache)
    acc0, valid0 = E.evaluate_by_module(model, items, unk, batch_size=4, module_loss_weight=0)
    assert acc == acc0 and abs(valid['decoder'] - valid0['decoder']) < 1e-5
