"""GPU tests (`-m gpu`) of training on cached clip encodings (STAIR_PLAN_TRAIN | STAIR_PLAN_VIDEO_ENCODED: run_programs(train=True,
clips=...), Trainer.step(clips=...), VideoNMN.logits(clips=...) / (encoded=...)) and of the gradient of the encodings
(stair_plan_set_encoded_video_grad, the gather's adjoint).

The rule: such a pass exists only while all eight tensors of the video encoder are frozen.  What it must compute is what the direct
step with freeze=('video_encoder',) computes on the same questions -- with the cache filled in one call from the very clip tensors
both passes run the same kernels on the same bits, so the comparisons below are torch.equal.

Shapes: the TINY configuration of test_gpu_clip_cache.py (H = 64: launch-per-layer path, one-workgroup LSTM, clips of 3 / 17 / 40 / 64
frames, two questions per clip), the default H = 512 configuration at T = 64 (fused chains, NO_DX / first-touch marks, cooperative
recurrence) and at T = 24 (packed tiles)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import nmn_oracle as O
from stair_amd import ops, spec, synth
from stair_amd._lib import StairError, check, lib
from test_gpu_frozen import (BWD_RECURRENCES, FROZEN_TINY, LR, MAX_NORM, P, _check_final, _oracle_run, _segments, _tol)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LENS = (3, 17, 40, 64)
TINY = dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, answer_vocab_length=16, max_video_length=64, object_types=10)
FULL = dict(spec.DEFAULT_CONFIG)
SHAPES = {'tiny': (TINY, 24, 12, [LENS[c % 4] for c in range(12)]), 'full64': (FULL, 32, 16, [64] * 16), 'full24': (FULL, 24, 12, [24] * 12)}
FREEZE = ('video_encoder',)


@pytest.fixture(params=['f32', 'bf16x3'])
def matmul(request):
    ops.set_matmul_mode(request.param)
    yield request.param
    ops.set_matmul_mode('bf16x3')


@pytest.fixture
def f32():
    ops.set_matmul_mode('f32')
    yield 'f32'
    ops.set_matmul_mode('bf16x3')


def _model(config, seed=5, frozen=True):
    from stair_amd.module_net import VideoNMN
    m = VideoNMN(config)
    w = synth.make_weights(config, seed)
    m.load_state_dict({k: torch.from_numpy(w[k].copy()) for k in spec.state_dict_keys(config)})
    m = m.to(DEV)
    if frozen:
        _freeze(m)
    return m


def _freeze(model, on=True):
    for n, p in model.named_parameters():
        if '.video_encoder.' in n:
            p.requires_grad_(not on)


class _Case:
    """One batch: questions (two per clip, in clip order, so that the cached plan numbers its clips as the direct one does), the
    padded clips on the device with zeros behind each clip's frames, and the arguments of both forms of a step."""

    def __init__(self, size):
        self.config, n_q, self.n_clips, self.lens = SHAPES[size]
        config, self.T = self.config, max(self.lens)
        self.vidx = [i * self.n_clips // n_q for i in range(n_q)]
        self.qs = []
        for i in range(n_q):
            q = synth.make_question(config, 21, i, form=synth.ALL_FORMS[i % 12], with_video=False)
            q['sg_res_by_step'] = synth.make_gold(config, 3, q, T=self.lens[self.vidx[i]])
            self.qs.append(q)
        g = torch.Generator().manual_seed(9)
        video = torch.randn(self.n_clips, self.T, config['video_size'], generator=g)
        for c, L in enumerate(self.lens):
            video[c, L:] = 0
        self.video = video.to(DEV)
        self.question = torch.cat([torch.as_tensor(q['question']) for q in self.qs]).to(DEV)
        self.answers = torch.tensor([q['answer'] for q in self.qs], dtype=torch.int32, device=DEV)
        self.head = ([q['nmn_program_list'] for q in self.qs], [q['prog_str_to_question_tokens'] for q in self.qs])
        self.q_lens = [q['question'].shape[0] for q in self.qs]
        self.ragged = len(set(self.lens)) > 1

    def cache(self, model):
        """the clips through the model's encoder, in ONE call from the tensor the direct pass reads"""
        return model.encode_clips(self.video, ids=list(range(self.n_clips)), video_len=self.lens)

    def direct(self):
        return (*self.head, self.video, self.question, self.q_lens), dict(video_index=self.vidx, video_len=self.lens if self.ragged else None)

    def cached(self, cache):
        return (*self.head, None, self.question, self.q_lens), dict(video_index=self.vidx, clips=cache)


@functools.lru_cache(maxsize=None)
def _case(size):
    return _Case(size)


def _trainer_step(size, cached, dropout=0.0, supervised=False, steps=1, skip='ever'):
    """`steps` Trainer.step calls with the video encoder frozen, on the clips or on a cache of them: what the comparisons need"""
    from stair_amd.train import Trainer
    case = _case(size)
    model = _model(case.config, frozen=False)
    tr = Trainer(model, dropout=dropout, dropout_seed=11, lr=1e-3, freeze=FREEZE, skip_untouched=skip)
    w0 = {n: w.clone() for n, w in _segments(tr, tr.flat_p).items()}
    cache = case.cache(model) if cached else None
    args, kw = case.cached(cache) if cached else case.direct()
    if supervised:
        kw = dict(kw, questions=case.qs)
    out = dict(losses=[], grads=[], module_losses=[])
    for it in range(steps):
        loss, res = tr.step(*args, case.answers, **kw)
        out['losses'].append(loss.clone())
        out['grads'].append({n: g.clone() for n, g in _segments(tr, tr.flat_g).items()})
        if supervised:
            out['module_losses'].append({k: v.clone() for k, v in tr.module_losses.items()})
    tr.check()
    out.update(model=model, tr=tr, cache=cache, res=res, w0=w0, weights={n: w.clone() for n, w in _segments(tr, tr.flat_p).items()},
               touched=dict(zip(model._weight_names, res.touched())), steps=dict(zip(model._weight_names, tr.steps.cpu().tolist())),
               m1=_segments(tr, tr.exp_avg.clone()), m2=_segments(tr, tr.exp_avg_sq.clone()))
    return out


@functools.lru_cache(maxsize=None)
def _direct_step(size, dropout=0.0, supervised=False):
    """the reference of the bit-level comparisons: the direct frozen step, computed once per case and left unchanged"""
    out = _trainer_step(size, False, dropout, supervised)
    return {k: out[k] for k in ('losses', 'grads', 'weights', 'module_losses')}


def _same_step(got, ref, what):
    names = list(ref['weights'])
    worst = 0.0
    for a, b in zip(got['losses'], ref['losses']):
        worst = max(worst, float((a - b).abs().max()))
    for n in names:
        worst = max(worst, float((got['grads'][0][n] - ref['grads'][0][n]).abs().max()), float((got['weights'][n] - ref['weights'][n]).abs().max()))
    print('%s: max |cached - direct| over losses, gradients and weights = %.3g' % (what, worst))
    assert torch.equal(got['losses'][0], ref['losses'][0]), what
    for n in names:
        assert torch.equal(got['grads'][0][n], ref['grads'][0][n]), (what, 'gradient', n)
        assert torch.equal(got['weights'][n], ref['weights'][n]), (what, 'weight', n)
    moved = sum(1 for n in names if not torch.equal(got['weights'][n], got['w0'][n]))
    assert moved >= 4 and float(got['losses'][0].abs().max()) > 0, moved
    for n in names:
        if '.video_encoder.' in n:
            assert not got['touched'][n] and got['steps'][n] == 0.0, n
            assert int((got['grads'][0][n] != 0).sum()) == 0 and torch.equal(got['weights'][n], got['w0'][n]), n
            assert int((got['m1'][n] != 0).sum()) == 0 and int((got['m2'][n] != 0).sum()) == 0, n
    got['cache'].check()                                # the encoder kept its torch version: the cache is still fresh


# ---------------------------------------------------------------------------------------------------------------------------
# 1, 2: bit for bit against the direct frozen step -- plain, under dropout, supervised
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', ['tiny', 'full64', 'full24'])
def test_cached_step_equals_the_direct_frozen_step_bit_for_bit(size):
    got = _trainer_step(size, True)
    assert got['res']._video is None and len(got['res'].clip_rows) == _case(size).n_clips and got['res'].info.T == _case(size).T
    _same_step(got, _direct_step(size), size)


@pytest.mark.parametrize('size', ['tiny', 'full64'])
def test_cached_step_under_dropout_equals_the_direct_one(size):
    """One seed, a NO_CSE plan on both sides (dropout draws a mask per occurrence): a shifted dropout site would change every bit."""
    got = _trainer_step(size, True, dropout=0.1)
    assert got['res'].info.n_aliased == 0
    ref = _direct_step(size, 0.1)
    assert not torch.equal(ref['losses'][0], _direct_step(size)['losses'][0])           # the masks do act
    _same_step(got, ref, size + ' dropout')


@pytest.mark.parametrize('size', ['tiny', 'full64'])
def test_cached_supervised_step_equals_the_direct_one(size):
    """questions=: the per-module criteria inject gradients into the arenas, the reverse pass keeps them (STAIR_BWD_KEEP_ARENAS)."""
    got = _trainer_step(size, True, supervised=True)
    ref = _direct_step(size, 0.0, True)
    assert got['module_losses'][0] and set(got['module_losses'][0]) == set(ref['module_losses'][0])
    for k, v in ref['module_losses'][0].items():
        assert torch.equal(v, got['module_losses'][0][k]), k
    assert not torch.equal(ref['grads'][0][P + 'text_encoder.weight_hh_l0'], _direct_step(size)['grads'][0][P + 'text_encoder.weight_hh_l0'])
    _same_step(got, ref, size + ' supervised')


def test_two_cached_steps_with_skip_untouched_window_equal_the_direct_ones():
    """The other form of skip_untouched, over two steps (the second one reads the first one's moments and step counts)."""
    got, ref = _trainer_step('tiny', True, steps=2, skip='window'), _trainer_step('tiny', False, steps=2, skip='window')
    for it in range(2):
        assert torch.equal(got['losses'][it], ref['losses'][it]), it
        for n in ref['weights']:
            assert torch.equal(got['grads'][it][n], ref['grads'][it][n]), (it, n)
    for n in ref['weights']:
        assert torch.equal(got['weights'][n], ref['weights'][n]) and got['steps'][n] == ref['steps'][n], n
        assert torch.equal(got['m1'][n], ref['m1'][n]) and torch.equal(got['m2'][n], ref['m2'][n]), n
    assert not torch.equal(got['losses'][0], got['losses'][1])
    got['cache'].check()


# ---------------------------------------------------------------------------------------------------------------------------
# the reverse pass alone: the encoder's bound buffers, kernel accounting (3)
# ---------------------------------------------------------------------------------------------------------------------------
def _raw_pass(size, cached, sentinel=123.0):
    """run_programs(train=True) + BatchResult.backward into buffers of the caller's own, bound while every weight is trainable; then
    the video encoder is frozen and its buffers are filled with a sentinel (`_raw_backward` of test_gpu_frozen.py)."""
    case = _case(size)
    model = _model(case.config, frozen=False)
    params = dict(model.named_parameters())
    names = model._weight_names
    for n in names:
        params[n].grad = torch.zeros_like(params[n])
    model._bind_grads()
    _freeze(model)
    for n in names:
        if '.video_encoder.' in n:
            params[n].grad.fill_(sentinel)
    args, kw = case.cached(case.cache(model)) if cached else case.direct()
    with ops.kernel_accounting() as fwd:
        res = model.run_programs(*args, train=True, **kw)
    with ops.kernel_accounting() as bwd:
        loss = res.backward(case.answers, 1.0 / len(case.qs))
    torch.cuda.synchronize()
    res.check()
    return dict(grads={n: params[n].grad.clone() for n in names}, loss=loss.clone(), logits=res.logits.clone(), fwd=dict(fwd.table),
                bwd=dict(bwd.table), res=res)


@pytest.mark.parametrize('size', ['tiny', 'full64'])
def test_reverse_pass_alone_keeps_the_encoders_buffers_and_runs_no_video_encoder(size):
    case = _case(size)
    H, Ep = case.config['hidden_size'], (case.config['text_size'] + 31) // 32 * 32
    rows_q = sum(case.q_lens)
    d, c = _raw_pass(size, False), _raw_pass(size, True)
    assert torch.equal(c['logits'], d['logits']) and torch.equal(c['loss'], d['loss'])
    for n, g in c['grads'].items():
        if '.video_encoder.' in n:
            assert torch.equal(g, torch.full_like(g, 123.0)), 'bound buffer of frozen %s was written' % n
        else:
            assert torch.equal(g, d['grads'][n]), n
    assert float(c['grads'][P + 'text_encoder.weight_ih_l0'].abs().max()) > 0
    # forward: one gather, the text projection and the text recurrence alone
    t = c['fwd']
    print(size, 'forward', {k: v[0] for k, v in sorted(t.items())})
    assert t['gather_encoded_video'][:2] == (1, 2 * case.n_clips * case.T * H * 4) and 'gather_encoded_video' not in d['fwd']
    rec = {k: v for k, v in t.items() if k.startswith('lstm_rec')}
    assert 'lstm_rec_coop_pair' not in rec and sum(v[0] for v in rec.values()) == 1, rec
    if size == 'full64':
        assert sum(v[2] for v in rec.values()) == 2 * 2 * rows_q * 4 * (H // 2) * (H // 2), rec          # the text encoder's alone
        assert t['gemm_planes'][0] == 1 and t['gemm_planes'][2] == 2 * rows_q * 4 * H * Ep, t['gemm_planes']     # the text projection alone
    # the control: the direct pass does run the video recurrence and projection
    flops = lambda tab, pre: sum(v[2] for k, v in tab.items() if k.startswith(pre))
    assert flops(d['fwd'], 'lstm_rec') > flops(t, 'lstm_rec') and flops(d['fwd'], 'gemm') > flops(t, 'gemm'), sorted(d['fwd'])
    for k in t:                                             # nothing but the gather that the direct pass does not launch too
        assert k == 'gather_encoded_video' or k.startswith('lstm_rec') or k in d['fwd'], k
    # reverse: the frozen-encoder pass the project already has -- the same launches, no BPTT of the video encoder, no dW_ih product
    b = c['bwd']
    print(size, 'reverse', {k: v[0] for k, v in sorted(b.items())})
    assert {k: v[0] for k, v in b.items()} == {k: v[0] for k, v in d['bwd'].items()}
    assert 'gemm_tn_tr' not in b and 'enc_input_grad' not in b and 'scatter_encoded_video_grad' not in b
    assert sum(b[k][0] for k in BWD_RECURRENCES if k in b) == 1 and 'lstm_bwd_coop_pair' not in b, sorted(b)
    if size == 'full64':
        assert b.get('lstm_bwd_coop', (0,))[0] == 1 and 'tile_mlp' in b     # the single form of the cooperative kernel, the fused chains


# ---------------------------------------------------------------------------------------------------------------------------
# 4: against torch autograd + torch.optim.Adam on the oracle (the set-up and bounds of test_frozen_steps_match_torch_adam_over_the_rest)
# ---------------------------------------------------------------------------------------------------------------------------
def _cached_pack(model, qs, T):
    lens = [int(q['video_features'].shape[0]) for q in qs]
    video = torch.stack([torch.nn.functional.pad(torch.as_tensor(q['video_features']), (0, 0, 0, T - L)) for q, L in zip(qs, lens)]).to(DEV)
    cache = model.encode_clips(video, ids=list(range(len(qs))), video_len=lens)
    question = torch.cat([torch.as_tensor(q['question']) for q in qs]).to(DEV)
    answers = torch.tensor([q['answer'] for q in qs], dtype=torch.int32, device=DEV)
    return cache, ([q['nmn_program_list'] for q in qs], [q['prog_str_to_question_tokens'] for q in qs], None, question,
                   [q['question'].shape[0] for q in qs], answers)


@pytest.mark.parametrize('max_grad_norm', [None, MAX_NORM])
def test_cached_steps_match_torch_adam_over_the_rest(max_grad_norm, matmul):
    from stair_amd.train import Trainer
    ora = _oracle_run(max_grad_norm, FROZEN_TINY)
    config, steps = ora['config'], ora['steps']
    model = _model(config, 0, frozen=False)
    tr = Trainer(model, lr=LR, scheduler_total_iters=10, skip_untouched='ever', dropout=0.0, max_grad_norm=max_grad_norm, freeze=FROZEN_TINY)
    for it, (qs, weight) in enumerate(ora['windows']):
        tr.decoder_loss_weight = weight
        cache, args = _cached_pack(model, qs, 40)           # (made anew per window: any window's cache is fresh, the encoder never moves)
        tr.step(*args, video_index=list(range(len(qs))), clips=cache)
        torch.cuda.synchronize()
        g = _segments(tr, tr.flat_g)
        for n in ora['frozen']:
            assert int((g[n] != 0).sum()) == 0, n
        if max_grad_norm is not None:
            norm = float(tr.grad_norm.cpu()[0])
            bound = float(np.sqrt(sum(x.numel() * _tol(x) ** 2 for x in steps[it]['grads'].values() if x is not None)))
            assert abs(norm - steps[it]['norm']) <= bound, (it, norm, steps[it]['norm'], bound)
    tr.check()
    cache.check()
    _check_final(model, ora, matmul)


def test_cached_step_on_a_ragged_window_matches_torch(matmul):
    from stair_amd.train import Trainer
    ora = _oracle_run(None, ('video_encoder',), ragged=True)
    qs = ora['windows'][0][0]
    assert [int(q['video_features'].shape[0]) for q in qs] == [24, 40, 40, 17]
    model = _model(ora['config'], 0, frozen=False)
    tr = Trainer(model, lr=LR, scheduler_total_iters=10, dropout=0.0, freeze=('video_encoder',))
    cache, args = _cached_pack(model, qs, 40)
    _, res = tr.step(*args, video_index=[0, 1, 2, 3], clips=cache)
    tr.check()
    assert sorted(int(x) for x in res.question_frames) == [17, 24, 40, 40]
    g = _segments(tr, tr.flat_g)
    for n in ora['names']:
        ref = ora['steps'][0]['grads'][n]
        if n in ora['frozen']:
            assert ref is None and int((g[n] != 0).sum()) == 0, n
        elif ref is not None:
            assert float((g[n].cpu() - ref.reshape(-1)).abs().max()) < _tol(ref), n
    _check_final(model, ora, matmul)


# ---------------------------------------------------------------------------------------------------------------------------
# 5: the gradient of the encodings
# ---------------------------------------------------------------------------------------------------------------------------
def _R(n, A, seed=7):
    return torch.from_numpy(np.random.RandomState(seed).randn(n, A).astype(np.float32))


@pytest.mark.parametrize('size', ['tiny', 'full64'])
def test_gradient_of_the_encodings_matches_autograd_of_the_oracle(size, f32):
    """A random linear loss on the logits; the oracle differentiates it with respect to its own encoder output (`video_feat`) question
    by question, and a clip's gradient is the sum over the questions that share it.  The bound is the autograd tests' bound for
    input gradients: 2e-4 of the largest reference entry."""
    case = _case(size)
    config, n_q = case.config, 12                          # (the first 12 questions: every form, six clips -- the oracle runs on the host)
    H, A = config['hidden_size'], config['answer_vocab_length']
    R = _R(n_q, A)
    w = O.to_torch(synth.make_weights(config, 5))
    clips_used = sorted(set(case.vidx[:n_q]))
    ref = torch.zeros(case.n_clips, case.T, H)
    for i in range(n_q):
        c = case.vidx[i]
        L = case.lens[c]
        q = {k: v for k, v in case.qs[i].items() if k != 'sg_res_by_step'}
        clip = case.video[c, :L].cpu().requires_grad_(True)         # (so that the encoder's output is part of the graph)
        r = O.forward(w, config, dict(q, video_features=clip), return_res_by_step=False, explicit_lstm=True)
        if not r['logits'].requires_grad:                             # a program that does not read its clip
            continue
        (gv,) = torch.autograd.grad((r['logits'] * R[i]).sum(), r['video_feat'], allow_unused=True)
        if gv is not None:
            ref[c, :L] += gv
    assert float(ref.abs().max()) > 0
    model = _model(config)
    enc = case.cache(model).enc.clone().requires_grad_(True)
    logits = model.logits(case.head[0][:n_q], case.head[1][:n_q], None, case.question[:sum(case.q_lens[:n_q])], case.q_lens[:n_q],
                          encoded=enc, video_index=case.vidx[:n_q], video_len=case.lens)
    assert logits.grad_fn is not None
    (logits * R.to(DEV)).sum().backward()
    got = enc.grad
    assert got is not None and tuple(got.shape) == tuple(enc.shape) == (case.n_clips, 64, H)
    tol = 2e-4 * float(ref.abs().max())
    err = float((got[:, :case.T].cpu() - ref).abs().max())
    print('%s: max |d_enc - oracle| = %.3g (bound %.3g, largest entry %.3g)' % (size, err, tol, float(ref.abs().max())))
    assert err < tol, (err, tol)
    for c in range(case.n_clips):
        if c not in clips_used:
            assert int((got[c] != 0).sum()) == 0, c       # a clip that no question reads
        else:
            assert int((got[c, case.lens[c]:] != 0).sum()) == 0 and float(got[c, :case.lens[c]].abs().max()) > 0, c


@pytest.mark.parametrize('size,rows_cap', [('tiny', 64), ('tiny', 72), ('full64', 64)])
def test_gradient_rows_through_the_abi_into_a_nan_filled_buffer(size, rows_cap):
    """Permuted rows with a gap, a plan whose T lies below rows_cap, a padded clip stride: the rows of the plan's clips are the map
    arena's gradient tiles bit for bit, exact zeros follow up to rows_cap - 1, nothing else is written."""
    case = _case(size)
    H, A = case.config['hidden_size'], case.config['answer_vocab_length']
    model = _model(case.config)
    cache = case.cache(model)
    pick = [i for i in range(len(case.qs)) if case.lens[case.vidx[i]] <= 40][:9] if size == 'tiny' else list(range(10))
    order = pick[3:] + pick[:3]                             # first use is out of row order
    rows = [case.vidx[i] for i in order]
    q_off = np.concatenate([[0], np.cumsum(case.q_lens)])
    question = torch.cat([case.question[q_off[i]: q_off[i + 1]] for i in order]).contiguous()
    res = model.run_programs([case.head[0][i] for i in order], [case.head[1][i] for i in order], None, question,
                             [case.q_lens[i] for i in order], train=True, video_index=rows, clips=cache)
    T = res.info.T
    assert T == (40 if size == 'tiny' else 64) and (T < rows_cap) == (size == 'tiny' or rows_cap > 64)
    assert list(res.clip_rows) == list(dict.fromkeys(rows)) and list(res.clip_rows) != sorted(res.clip_rows)
    params = dict(model.named_parameters())
    for n in model._weight_names:
        params[n].grad = torch.zeros_like(params[n])
    stride = (rows_cap + 8) * H
    buf = torch.full((case.n_clips + 1, stride), float('nan'), device=DEV)
    check(lib.stair_plan_set_encoded_video_grad(res._plan, C.c_void_p(buf.data_ptr()), stride, rows_cap))
    with ops.kernel_accounting() as acct:
        res.backward_dlogits(_R(len(order), A).to(DEV))
    torch.cuda.synchronize()
    res.check()
    assert acct.table['scatter_encoded_video_grad'][:2] == (1, 2 * len(res.clip_rows) * T * H * 4)
    gmap = res.grad_arena('map')
    used = set(int(r) for r in res.clip_rows)
    for v, row in enumerate(res.clip_rows):
        L = case.lens[row]
        tile = buf[row].view(-1, H)
        assert torch.equal(tile[:L].view(torch.int32), gmap[v, :L].view(torch.int32)), (v, row)
        assert float(tile[:L].abs().max()) > 0
        assert int((tile[L:rows_cap].view(torch.int32) != 0).sum()) == 0, (v, row, L)      # exact (+0) zeros
        assert bool(torch.isnan(tile[rows_cap:]).all()), (v, row)                           # the padding of the stride
    for row in range(case.n_clips + 1):
        if row not in used:
            assert bool(torch.isnan(buf[row]).all()), row
    assert len(used) < case.n_clips


@pytest.mark.parametrize('size', ['tiny', 'full64'])
def test_requesting_the_gradient_changes_no_parameter_gradient(size):
    case = _case(size)
    model = _model(case.config)
    cache = case.cache(model)
    R = _R(len(case.qs), case.config['answer_vocab_length']).to(DEV)
    params = dict(model.named_parameters())
    out = {}
    for want in (False, True):
        for p in params.values():
            p.grad = None
        enc = cache.enc.clone().requires_grad_(want)
        logits = model.logits(*case.head, None, case.question, case.q_lens, encoded=enc, video_index=case.vidx, video_len=case.lens)
        with ops.kernel_accounting() as acct:
            (logits * R).sum().backward()
        torch.cuda.synchronize()
        out[want] = ({n: (None if params[n].grad is None else params[n].grad.clone()) for n in model._weight_names}, enc.grad, dict(acct.table))
    (g0, e0, t0), (g1, e1, t1) = out[False], out[True]
    assert e0 is None and e1 is not None and float(e1.abs().max()) > 0
    assert 'scatter_encoded_video_grad' not in t0 and t1['scatter_encoded_video_grad'][0] == 1
    assert not [k for k in ('gemm_tn_tr', 'enc_input_grad', 'lstm_bwd_coop_pair') if k in t1], sorted(t1)       # still no BPTT of the video encoder
    some = 0
    for n in model._weight_names:
        assert (g0[n] is None) == (g1[n] is None), n
        if '.video_encoder.' in n:
            assert g1[n] is None, n
        elif g0[n] is not None:
            assert torch.equal(g0[n], g1[n]), n
            some += 1
    assert some > 20
    # the same through a ClipCache: autograd over the cache, no gradient goes to it
    for p in params.values():
        p.grad = None
    logits = model.logits(*case.head, None, case.question, case.q_lens, clips=cache, video_index=case.vidx)
    (logits * R).sum().backward()
    for n in model._weight_names:
        assert (g0[n] is None) == (params[n].grad is None) and (g0[n] is None or torch.equal(g0[n], params[n].grad)), n
    cache.check()


def test_autograd_semantics_of_the_encoded_form():
    case = _case('tiny')
    model = _model(case.config)
    enc = case.cache(model).enc.clone().requires_grad_(True)
    n_q = 6                                                 # clips 0 .. 2 are read, the others are not
    args = (case.head[0][:n_q], case.head[1][:n_q], None, case.question[:sum(case.q_lens[:n_q])], case.q_lens[:n_q])
    logits = model.logits(*args, encoded=enc, video_index=case.vidx[:n_q], video_len=case.lens)
    loss = logits.square().sum()
    (g,) = torch.autograd.grad(loss, enc, retain_graph=True)
    assert tuple(g.shape) == tuple(enc.shape) and float(g[:3].abs().max()) > 0 and int((g[3:] != 0).sum()) == 0
    with pytest.raises(RuntimeError, match='has been through backward'):
        torch.autograd.grad(loss, enc)
    # without grad mode, or with nothing that requires grad, the pass is inference on the same rows
    with torch.no_grad():
        plain = model.logits(*args, encoded=enc, video_index=case.vidx[:n_q], video_len=case.lens)
    assert plain.grad_fn is None and float((plain - logits.detach()).abs().max()) < 2e-6


# ---------------------------------------------------------------------------------------------------------------------------
# 6: staleness
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_cache_is_fresh_after_several_cached_steps():
    case = _case('tiny')
    got = _trainer_step('tiny', True, steps=3)
    model, cache = got['model'], got['cache']
    cache.check()
    assert not torch.equal(got['losses'][0], got['losses'][2])                      # the steps did move the answers
    args, kw = case.cached(cache)
    cached = model.run_programs(*args, **kw).logits.clone()
    args, kw = case.direct()
    assert torch.equal(cached, model.run_programs(*args, **kw).logits)
    assert got['steps'][P + 'text_encoder.weight_hh_l0'] == 3.0 and got['steps'][P + 'video_encoder.weight_hh_l0'] == 0.0
    # forward_batch(train=True, clip_cache=...): the same training pass from the question dicts, clips looked up by 'video_id'
    args, kw = case.cached(cache)
    want = model.run_programs(*args, train=True, **kw).logits.clone()
    res = model.forward_batch([dict(q, video_id=case.vidx[i]) for i, q in enumerate(case.qs)], train=True, clip_cache=cache)
    assert res.info.gvec_off >= 0 and res._video is None and torch.equal(res.logits, want)


# ---------------------------------------------------------------------------------------------------------------------------
# 7: refusals -- each raises with its message before anything is enqueued
# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing():
    from stair_amd.train import Trainer
    case = _case('tiny')
    model = _model(case.config, frozen=False)
    tr = Trainer(model, dropout=0.0, lr=1e-3)              # nothing frozen
    cache = case.cache(model)
    args, kw = case.cached(cache)
    H = case.config['hidden_size']
    with ops.kernel_accounting() as acct:
        # a trainable encoder
        with pytest.raises(ValueError, match='training on cached encodings needs a frozen video encoder'):
            tr.step(*args, case.answers, **kw)
        assert tr.iters == 0 and tr.questions_seen == 0
        with pytest.raises(ValueError, match='training on cached encodings needs a frozen video encoder'):
            model.run_programs(*args, train=True, **kw)
        with pytest.raises(ValueError, match='training on cached encodings needs a frozen video encoder'):
            model.logits(*args, clips=cache, video_index=case.vidx)
        enc = cache.enc.clone().requires_grad_(True)
        with pytest.raises(ValueError, match='training on cached encodings needs a frozen video encoder'):
            model.logits(*args, encoded=enc, video_index=case.vidx, video_len=case.lens)
        one = dict(model.named_parameters())[P + 'video_encoder.bias_hh_l0_reverse']
        _freeze(model)
        one.requires_grad_(True)                            # seven of eight frozen is not frozen
        with pytest.raises(ValueError, match='training on cached encodings needs a frozen video encoder'):
            model.run_programs(*args, train=True, **kw)
        _freeze(model)
        # video given together with clips
        with pytest.raises(ValueError, match='video given together with clips'):
            model.run_programs(*case.head, case.video, case.question, case.q_lens, train=True, **kw)
        with pytest.raises(ValueError, match='video given together with clips'):
            tr.step(*case.head, case.video, case.question, case.q_lens, case.answers, **kw)
        with pytest.raises(ValueError, match='video given together with clips'):
            model.logits(*case.head, case.video, case.question, case.q_lens, encoded=enc)
        # encoded of the wrong shape or device
        for bad in (enc[:, :, :H - 4], enc[0], enc.detach().cpu(), enc.detach().double(), enc.detach().transpose(0, 1)):
            with pytest.raises(ValueError, match='encoded must be'):
                model.logits(*args, encoded=bad, video_index=case.vidx, video_len=case.lens)
        with pytest.raises(ValueError, match='video_len must hold'):
            model.logits(*args, encoded=enc, video_index=case.vidx, video_len=case.lens[:-1])
        with pytest.raises(ValueError, match='video_index must hold'):
            model.logits(*args, encoded=enc, video_index=[case.n_clips] * len(case.qs), video_len=case.lens)
        with pytest.raises(ValueError, match='dropout'):
            model.run_programs(*args, dropout=(0.1, 3), **kw)           # inference on cached clips, as before
    assert not acct.table, sorted(acct.table)
    # thawing between build and backward: the reverse pass checks the eight flags again
    res = model.run_programs(*args, train=True, **kw)
    for n in model._weight_names:
        p = dict(model.named_parameters())[n]
        p.grad = torch.zeros_like(p)
    one.requires_grad_(True)
    with ops.kernel_accounting() as acct:
        with pytest.raises(StairError, match='made trainable after the plan was built.*training on cached encodings'):
            res.backward(case.answers, 1.0)
    assert not acct.table, sorted(acct.table)
    one.requires_grad_(False)
    res.backward(case.answers, 1.0)                         # frozen again: the pass runs
    torch.cuda.synchronize()
    res.check()
    # no gradient for the clips of a pass that has none; the gradient buffer has the encodings' shape
    res = model.run_programs(*args, train=True, **kw)
    d_logits = torch.zeros(len(case.qs), case.config['answer_vocab_length'], device=DEV)
    with pytest.raises(ValueError, match='no video'):
        res.backward_dlogits(d_logits, d_video=torch.zeros_like(case.video))
    with pytest.raises(ValueError, match='d_encoded must have the shape'):
        res.backward_dlogits(d_logits, d_encoded=torch.zeros(3, 64, H, device=DEV))
