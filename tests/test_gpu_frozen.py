"""GPU tests (`-m gpu`) of frozen parameters (requires_grad = False; Trainer(freeze=...); stair_ctx_set_trainable): a frozen
weight gets no gradient and no update, its bound gradient buffer is not touched, the gradients and updates of everything else
are those of the unfrozen step, and the reverse pass does not launch what only frozen weights needed.

Fused path (hidden size 512): bit level against the unfrozen step.  Launch-per-layer path (the tiny configuration): against torch
autograd + torch.optim.Adam on the oracle's weights with the same tensors requires_grad_(False), in test_gpu_grad_clip.py's
set-up and under its bounds.  The chain kernel's "no input gradient" marker (STAIR_TILE_NO_DX), which the plan sets on clip tiles
while the video encoder's block is left out, is also checked as a building block."""
import functools
import math

import pytest
import torch

from oracle import nmn_oracle as O
from stair_amd import ops, spec, synth
from helpers import load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
P = 'submodules.'


@pytest.fixture(params=['f32', 'bf16x3'])
def matmul(request):
    ops.set_matmul_mode(request.param)
    yield request.param
    ops.set_matmul_mode('bf16x3')


def _model(config, seed=0):
    from stair_amd.module_net import VideoNMN
    m = VideoNMN(config)
    w = synth.make_weights(config, seed)
    m.load_state_dict({k: torch.from_numpy(w[k].copy()) for k in spec.state_dict_keys(config)})
    return m.to(DEV)


def _pack(qs):
    video = torch.stack([torch.as_tensor(q['video_features']) for q in qs]).to(DEV)
    question = torch.cat([torch.as_tensor(q['question']) for q in qs]).to(DEV)
    return ([q['nmn_program_list'] for q in qs], [q['prog_str_to_question_tokens'] for q in qs], video, question,
            [q['question'].shape[0] for q in qs], torch.tensor([q['answer'] for q in qs], dtype=torch.int32, device=DEV))


def _tol(g_ref):
    """the project's gradient tolerance (test_backward_matches_autograd_of_oracle; `_tol` of test_gpu_grad_clip.py)"""
    return 2e-4 * max(float(g_ref.abs().max()), 1e-3)


def _is_frozen(name, prefixes):
    short = name[len(P):]
    return any(short == pre or short.startswith(pre + '.') for pre in prefixes)


def _segments(tr, flat):
    return {n: flat[o: o + p.numel()] for n, o, p in zip(tr.model._weight_names, tr.offsets, tr._params)}


# ---------------------------------------------------------------------------------------------------------------------------
# fused path, bit level
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _full_size_batch(n_q=64, clips=32):
    """the set-up of test_training_step_is_bit_reproducible"""
    config = dict(spec.DEFAULT_CONFIG)
    qs = [synth.make_question(config, 21, i, T=64, forms=synth.ALL_FORMS, with_video=False) for i in range(n_q)]
    g = torch.Generator().manual_seed(9)
    video = torch.randn(clips, 64, config['video_size'], generator=g).to(torch.bfloat16).to(DEV)
    question = torch.cat([torch.as_tensor(q['question']) for q in qs]).to(DEV)
    answers = torch.tensor([q['answer'] for q in qs], dtype=torch.int32, device=DEV)
    args = ([q['nmn_program_list'] for q in qs], [q['prog_str_to_question_tokens'] for q in qs], video, question,
            [q['question'].shape[0] for q in qs], answers)
    return config, args, [i % clips for i in range(n_q)]


BWD_RECURRENCES = ('lstm_bwd_coop_pair', 'lstm_bwd_coop', 'lstm_bwd_x3', 'lstm_bwd_f32')
TN_PRODUCTS = ('gemm_tn_x3tr', 'gemm_tn_bf16x3', 'gemm_tn_bf16x3_t256', 'gemm_tn_tr')


def _launches(table, keys):
    return sum(table[k][0] for k in keys if k in table)


@functools.lru_cache(maxsize=None)
def _unfrozen_step():
    """One unfrozen Trainer.step on the full-size batch, computed once and left unchanged: per-tensor gradients, the weights after
    the step, and the kernel accounting of the reverse pass alone (BatchResult.backward into the caller's own buffers)."""
    from stair_amd.train import Trainer
    config, args, vidx = _full_size_batch()
    model = _model(config, 5)
    own = _raw_backward(model, args, vidx, ())
    tr = Trainer(model, dropout=0.0, lr=1e-3)
    tr.step(*args, video_index=vidx)
    tr.check()
    grads = {n: g.clone() for n, g in _segments(tr, tr.flat_g).items()}
    weights = {n: w.clone() for n, w in _segments(tr, tr.flat_p).items()}
    for n in grads:                                     # the caller's-own-buffer pass IS the trainer's pass
        assert torch.equal(own['grads'][n].reshape(-1), grads[n]), n
    return dict(grads=grads, weights=weights, table=own['table'])


def _raw_backward(model, args, vidx, prefixes, sentinel=123.0):
    """run_programs(train=True) + BatchResult.backward with gradient buffers of the caller's own: every buffer is bound while its
    weight is still trainable, then the weights under `prefixes` are frozen and their buffers filled with a sentinel."""
    params = dict(model.named_parameters())
    names = model._weight_names
    for n in names:
        params[n].requires_grad_(True)
        params[n].grad = torch.zeros_like(params[n])
    model._bind_grads()                                 # (all trainable: every buffer reaches the context)
    for n in names:
        if _is_frozen(n, prefixes):
            params[n].requires_grad_(False)
            params[n].grad.fill_(sentinel)
    res = model.run_programs(*args[:5], train=True, video_index=vidx)
    with ops.kernel_accounting() as acct:
        res.backward(args[5], 1.0 / len(args[0]))
    torch.cuda.synchronize()
    res.check()
    out = dict(grads={n: params[n].grad.clone() for n in names}, table=dict(acct.table), touched=dict(zip(names, res.touched())))
    for n in names:
        params[n].requires_grad_(True)
    return out


def _prefixes(case, names):
    if case == 'decoder_only':
        return tuple(sorted({n.split('.')[1] for n in names} - {'decoder'}))
    return {'video_encoder': ('video_encoder',), 'text_encoder': ('text_encoder',), 'both_encoders': ('video_encoder', 'text_encoder'),
            'Filter': ('Filter',), 'one_weight': ('Localize.video_linear.0.weight',)}[case]


def test_the_unfrozen_pass_takes_the_paired_cooperative_recurrence():
    """Otherwise the encoder cases below prove nothing about the hand-over from the paired to the single form."""
    table = _unfrozen_step()['table']
    assert table.get('lstm_bwd_coop_pair', (0,))[0] == 1 and 'lstm_bwd_coop' not in table, sorted(table)
    assert 'tile_mlp' in table and table['vec_group'][0] > 2 and 'gemm_tn_tr' in table and 'grad_fanin_kernel' in table


@pytest.mark.parametrize('case', ['video_encoder', 'text_encoder', 'both_encoders', 'decoder_only', 'Filter', 'one_weight'])
def test_frozen_step_against_the_unfrozen_step_bit_for_bit(case):
    from stair_amd.train import Trainer
    config, args, vidx = _full_size_batch()
    base = _unfrozen_step()
    model = _model(config, 5)
    names = model._weight_names
    prefixes = _prefixes(case, names)
    frozen = {n for n in names if _is_frozen(n, prefixes)}
    assert frozen and len(frozen) < len(names)
    if case == 'one_weight':
        assert frozen == {P + 'Localize.video_linear.0.weight'} and base['grads'][P + 'Localize.video_linear.0.bias'].abs().max() > 0

    # the reverse pass alone, into the caller's own buffers: the frozen ones keep their sentinel, the others hold the unfrozen gradient
    own = _raw_backward(model, args, vidx, prefixes)
    for n in names:
        g = own['grads'][n].reshape(-1)
        if n in frozen:
            assert torch.equal(g, torch.full_like(g, 123.0)), 'bound buffer of frozen %s was written' % n
            assert not own['touched'][n], n
        else:
            assert torch.equal(g, base['grads'][n]), 'gradient of %s differs from the unfrozen pass' % n
    table = own['table']
    print(case, {k: v[0] for k, v in sorted(table.items())})
    if case in ('video_encoder', 'text_encoder'):       # the other recurrence runs alone, in the single form
        assert table.get('lstm_bwd_coop', (0,))[0] == 1 and 'lstm_bwd_coop_pair' not in table, sorted(table)
    if case in ('video_encoder', 'both_encoders', 'decoder_only'):
        assert 'gemm_tn_tr' not in table                # (dW_ih of the video encoder on the stored bf16 rows)
    if case in ('both_encoders', 'decoder_only'):
        # skipping is real: no reverse recurrence, no encoder weight-gradient product (2 x dW_ih + 2 x dW_hh per encoder), no
        # input-gradient product
        assert not [k for k in BWD_RECURRENCES + ('enc_input_grad',) if k in table], sorted(table)
        assert _launches(base['table'], TN_PRODUCTS) - _launches(table, TN_PRODUCTS) >= 8
    if case == 'both_encoders':
        assert table['tile_mlp'][0] == base['table']['tile_mlp'][0] and table['vec_group'][0] == base['table']['vec_group'][0]
    if case == 'decoder_only':
        # ... and no tile, row or vec-group launch of the level walk: what is left is the decoder's own d(hidden) product (ONE
        # grouped launch) in front of its two weight-gradient products
        walk = [k for k in table if 'bwd' in k or k in ('tile_mlp', 'grad_fanin_kernel', 'mask_relu_kernel', 'bcast_mask_relu_kernel',
                                                        'weighted_colsum_kernel', 'scale_rows_kernel')]
        assert not walk, walk
        assert table['vec_group'][0] == 1 and _launches(table, TN_PRODUCTS) == 2, table
    if case == 'Filter':                                # six deferred products (Filter's six Linear layers) are not launched
        assert _launches(base['table'], TN_PRODUCTS) - _launches(table, TN_PRODUCTS) >= 1

    # one optimizer step through the Trainer's convenience
    tr = Trainer(model, dropout=0.0, lr=1e-3, freeze=prefixes)
    params = dict(model.named_parameters())
    assert {n for n in names if not params[n].requires_grad} == frozen
    w0 = {n: w.clone() for n, w in _segments(tr, tr.flat_p).items()}
    _, res = tr.step(*args, video_index=vidx)
    tr.check()
    g, w = _segments(tr, tr.flat_g), _segments(tr, tr.flat_p)
    m1, m2 = _segments(tr, tr.exp_avg), _segments(tr, tr.exp_avg_sq)
    steps = dict(zip(names, tr.steps.cpu().tolist()))
    touched = dict(zip(names, res.touched()))
    for n in names:
        if n in frozen:
            assert not touched[n] and steps[n] == 0.0, n
            assert int((g[n] != 0).sum()) == 0, 'frozen %s has a gradient' % n
            assert torch.equal(w[n], w0[n]) and int((m1[n] != 0).sum()) == 0 and int((m2[n] != 0).sum()) == 0, 'frozen %s moved' % n
        else:
            assert torch.equal(g[n], base['grads'][n]), n
            assert torch.equal(w[n], base['weights'][n]), n
    assert sum(1 for n in names if n not in frozen and not torch.equal(w[n], w0[n])) >= 4      # the step did move the rest


def test_two_frozen_runs_are_bit_identical():
    from stair_amd.train import Trainer
    config, args, vidx = _full_size_batch()
    runs = []
    for rep in range(2):
        tr = Trainer(_model(config, 5), dropout=0.0, lr=1e-3, freeze=('video_encoder', 'Filter'))
        grads = []
        for it in range(2):
            tr.step(*args, video_index=vidx)
            grads.append(tr.flat_g.clone())
        tr.check()
        runs.append((grads, tr.flat_p.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone()))
    for it in range(2):
        assert torch.equal(runs[0][0][it], runs[1][0][it])
    for a, b in zip(runs[0][1:], runs[1][1:]):
        assert torch.equal(a, b)
    assert float(runs[0][0][1].abs().max()) > 0 and not torch.equal(runs[0][0][0], runs[0][0][1])


def test_a_schedule_may_thaw_between_steps():
    """The flags are read at every step: frozen in step 1 (no update, step count 0), thawed for step 2 (the first step in which the
    weight is trainable and used: Adam step 1 for it, step 2 for the rest); and a weight frozen AFTER it was touched once keeps
    its bits although 'ever' remembers it."""
    from stair_amd.train import Trainer
    config, args, vidx = _full_size_batch()
    model = _model(config, 5)
    tr = Trainer(model, dropout=0.0, lr=1e-3, freeze=('video_encoder',))
    names = model._weight_names
    params = dict(model.named_parameters())
    enc = [n for n in names if '.video_encoder.' in n]
    w0 = {n: w.clone() for n, w in _segments(tr, tr.flat_p).items()}
    tr.step(*args, video_index=vidx)
    for n in enc:
        params[n].requires_grad_(True)
    dec = [n for n in names if '.decoder.' in n]
    for n in dec:
        params[n].requires_grad_(False)
    w1 = {n: w.clone() for n, w in _segments(tr, tr.flat_p).items()}
    m1 = {n: m.clone() for n, m in _segments(tr, tr.exp_avg).items()}
    tr.step(*args, video_index=vidx)
    tr.check()
    w2, g2, m2 = _segments(tr, tr.flat_p), _segments(tr, tr.flat_g), _segments(tr, tr.exp_avg)
    steps = dict(zip(names, tr.steps.cpu().tolist()))
    for n in enc:
        assert torch.equal(w1[n], w0[n]) and not torch.equal(w2[n], w1[n]) and steps[n] == 1.0 and float(g2[n].abs().max()) > 0, n
    for n in dec:
        assert not torch.equal(w1[n], w0[n]) and torch.equal(w2[n], w1[n]) and torch.equal(m2[n], m1[n]) and steps[n] == 1.0, n
        assert int((g2[n] != 0).sum()) == 0, n
    assert steps[P + 'text_encoder.weight_hh_l0'] == 2.0


def test_input_gradient_overrides_the_skip():
    """Video encoder frozen, but the clips want a gradient (model.logits with video.requires_grad_()): BPTT runs, video.grad is
    the unfrozen one bit for bit, the encoder's .grad stays None and its weight products are not launched."""
    config, args, vidx = _full_size_batch()
    progs, spans, video, question, q_lens, answers = args
    model = _model(config, 5)
    params = dict(model.named_parameters())
    enc = [n for n in model._weight_names if '.video_encoder.' in n]
    out = {}
    for frozen in (False, True):
        for n in model._weight_names:
            params[n].grad = None
            params[n].requires_grad_(not (frozen and n in enc))
        v = video.clone().requires_grad_(True)
        logits = model.logits(progs, spans, v, question, q_lens, video_index=vidx)
        loss = torch.nn.functional.cross_entropy(logits, answers.long(), reduction='sum') / len(progs)
        with ops.kernel_accounting() as acct:
            loss.backward()
        torch.cuda.synchronize()
        out[frozen] = (v.grad.clone(), {n: (None if params[n].grad is None else params[n].grad.clone()) for n in model._weight_names},
                       dict(acct.table))
    (gv0, gp0, t0), (gv1, gp1, t1) = out[False], out[True]
    assert float(gv0.float().abs().max()) > 0 and torch.equal(gv0, gv1)
    assert 'enc_input_grad' in t1 and _launches(t1, BWD_RECURRENCES) >= 1 and 'gemm_tn_tr' in t0 and 'gemm_tn_tr' not in t1, sorted(t1)
    for n in model._weight_names:
        if n in enc:
            assert gp1[n] is None and gp0[n] is not None, n
        else:
            assert (gp0[n] is None) == (gp1[n] is None), n
            if gp0[n] is not None:
                assert torch.equal(gp0[n], gp1[n]), n


# ---------------------------------------------------------------------------------------------------------------------------
# against torch, launch-per-layer path (test_gpu_grad_clip.py's three windows: all 12 forms, T = 40)
# ---------------------------------------------------------------------------------------------------------------------------
WINDOWS = [['P1', 'P4', 'P1', 'P4'], ['P0', 'P2', 'P3', 'P5'], ['P6', 'P7', 'C0', 'C1']]
LOSS_WEIGHTS = [10.0, 1.0, 1.0]
MAX_NORM, LR = 2.0, 2e-4
FROZEN_TINY = ('video_encoder', 'Filter', 'Localize.video_linear.0.weight', 'decoder.3.bias')


def _windows(config):
    out, qid = [], 100
    for forms in WINDOWS:
        out.append([synth.make_question(config, 5, qid + i, form=f, T=40) for i, f in enumerate(forms)])
        qid += len(forms)
    return out


def _ragged_window(config):
    return [synth.make_question(config, 5, 300 + i, form=f, T=L) for i, (f, L) in enumerate(zip(WINDOWS[1], (24, 40, 40, 17)))]


@functools.lru_cache(maxsize=None)
def _oracle_run(max_grad_norm, prefixes, ragged=False):
    """The steps on the oracle (CPU, once per case): the frozen tensors requires_grad_(False), torch Adam (and clip_grad_norm_)
    over the rest.  Per step the gradients and their norm; the initial and the final weights."""
    z, meta = load_golden('tiny_conv')
    config = meta['config']
    names = [n for n, _ in spec.weight_table(config)]
    wts = synth.make_weights(config, 0)
    frozen = {n for n in names if _is_frozen(n, prefixes)}
    w = {k: torch.from_numpy(wts[k].copy()).requires_grad_(k not in frozen) for k in names}
    live = [w[n] for n in names if n not in frozen]
    opt = torch.optim.Adam(live, lr=LR)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda it: 1.0 + (0.1 - 1.0) / 10 * it if it <= 10 else 0.1)
    steps = []
    windows = [(_ragged_window(config), 1.0)] if ragged else list(zip(_windows(config), LOSS_WEIGHTS))
    for qs, weight in windows:
        total = 0.0
        for q in qs:
            logits = O.forward(w, config, q, return_res_by_step=False, explicit_lstm=True)['logits']
            total = total + torch.nn.functional.cross_entropy(logits.unsqueeze(0), torch.tensor([q['answer']])) * (weight / len(qs))
        total.backward()
        grads = {n: (None if w[n].grad is None else w[n].grad.detach().clone()) for n in names}
        norm = None
        if max_grad_norm is not None:
            norm = float(torch.nn.utils.clip_grad_norm_(live, max_grad_norm))
        opt.step(); opt.zero_grad(set_to_none=False); sched.step()
        steps.append(dict(grads=grads, norm=norm))
    return dict(config=config, names=names, frozen=frozen, steps=steps, initial={n: torch.from_numpy(wts[n].copy()) for n in names},
                final={n: w[n].detach().clone() for n in names}, windows=windows)


def _check_final(model, ora, matmul):
    got = dict(model.named_parameters())
    for n in ora['names']:
        have = got[n].detach().cpu()
        if n in ora['frozen']:
            assert torch.equal(have, ora['initial'][n]), 'frozen %s moved' % n
            continue
        diff = (have - ora['final'][n]).abs()
        if matmul == 'f32':                                   # test_clipped_steps_match_torch_clip_then_adam's own bounds
            assert float(diff.max()) < 2e-5, (n, float(diff.max()))
        else:
            assert float((diff < 2e-5).float().mean()) > 0.995, (n, float((diff < 2e-5).float().mean()))
            assert float(diff.max()) < 2.5e-4, (n, float(diff.max()))


@pytest.mark.parametrize('max_grad_norm', [None, MAX_NORM])
def test_frozen_steps_match_torch_adam_over_the_rest(max_grad_norm, matmul):
    from stair_amd.train import Trainer
    ora = _oracle_run(max_grad_norm, FROZEN_TINY)
    config, names, steps = ora['config'], ora['names'], ora['steps']
    assert len(ora['frozen']) == 8 + 20 + 2 and any(s['grads'][P + 'Localize.video_linear.0.bias'] is not None for s in steps)
    for s in steps:
        assert all(s['grads'][n] is None for n in ora['frozen'])
    model = _model(config, 0)
    tr = Trainer(model, lr=LR, scheduler_total_iters=10, skip_untouched='ever', dropout=0.0, max_grad_norm=max_grad_norm, freeze=FROZEN_TINY)
    assert set(model._weight_names) == set(names)
    for it, (qs, weight) in enumerate(ora['windows']):
        tr.decoder_loss_weight = weight
        tr.step(*_pack(qs))
        torch.cuda.synchronize()
        g = _segments(tr, tr.flat_g)
        for n in ora['frozen']:
            assert int((g[n] != 0).sum()) == 0, n
        if max_grad_norm is not None:
            norm, coef = (float(x) for x in tr.grad_norm.cpu())
            # every entry of a trainable tensor t may be off by tol_t, so the norm by sqrt(sum_t numel_t tol_t^2); frozen tensors
            # count for nothing, as in clip_grad_norm_ over parameters without a gradient
            bound = math.sqrt(sum(x.numel() * _tol(x) ** 2 for x in steps[it]['grads'].values() if x is not None))
            print('step %d: norm %.7g (oracle %.7g, bound %.3g), coefficient %.7g' % (it, norm, steps[it]['norm'], bound, coef))
            assert abs(norm - steps[it]['norm']) <= bound, (it, norm, steps[it]['norm'], bound)
            by_name = tr.grad_norms_by_name()
            assert all(by_name[n] == 0.0 for n in ora['frozen'])
            assert abs(math.sqrt(sum(v * v for v in by_name.values())) - norm) <= 1e-5 * norm
    tr.check()
    if max_grad_norm is not None:
        assert steps[0]['norm'] > MAX_NORM                    # the case does clip
    _check_final(model, ora, matmul)


def test_frozen_video_encoder_on_a_ragged_window(matmul):
    from stair_amd.train import Trainer
    ora = _oracle_run(None, ('video_encoder',), ragged=True)
    config = ora['config']
    qs = ora['windows'][0][0]
    lens = [int(q['video_features'].shape[0]) for q in qs]
    assert lens == [24, 40, 40, 17]
    model = _model(config, 0)
    tr = Trainer(model, lr=LR, scheduler_total_iters=10, dropout=0.0, freeze=('video_encoder',))
    video = torch.stack([torch.nn.functional.pad(torch.as_tensor(q['video_features']), (0, 0, 0, 40 - L)) for q, L in zip(qs, lens)]).to(DEV)
    progs, spans, _, question, q_lens, answers = _pack([dict(q, video_features=video[i].cpu()) for i, q in enumerate(qs)])
    tr.step(progs, spans, video, question, q_lens, answers, video_len=lens)
    tr.check()
    g = _segments(tr, tr.flat_g)
    for n in ora['names']:
        ref = ora['steps'][0]['grads'][n]
        if n in ora['frozen']:
            assert ref is None and int((g[n] != 0).sum()) == 0, n
        elif ref is not None:
            assert float((g[n].cpu() - ref.reshape(-1)).abs().max()) < _tol(ref), n
    _check_final(model, ora, matmul)


# ---------------------------------------------------------------------------------------------------------------------------
# supervised step, cache
# ---------------------------------------------------------------------------------------------------------------------------
def test_supervised_step_with_a_frozen_head_and_module():
    """One window with the per-module criteria (questions=): a frozen pre-train head passes no dW / db to its criterion (the
    gradient of the node it scores is still injected), a frozen Localize drops its products; the other gradients are those of
    the unfrozen step (float atomics on this path: the gradient tolerance), the frozen ones zero, the frozen weights unchanged."""
    from stair_amd.train import Trainer
    z, meta = load_golden('tiny_conv')
    config, T = meta['config'], meta['T']
    qs = []
    for i, f in enumerate(synth.ALL_FORMS):
        q = synth.make_question(config, 8, 50 + i, form=f, T=T)
        qs.append(dict(q, sg_res_by_step=synth.make_gold(config, 3, q, T=T)))
    prefixes = None
    out = {}
    for frozen in (False, True):
        model = _model(config, 0)
        if frozen:      # one of the pre-train heads the window's gold does score
            head = [k for k in ('Exists', 'Xor', 'Equals') if k in out[False][3]][0]
            prefixes = (head + '.pretrain_head', 'Localize')
        tr = Trainer(model, lr=LR, dropout=0.0, freeze=prefixes if frozen else ())
        w0 = tr.flat_p.clone()
        tr.step(*_pack(qs), questions=qs)
        tr.check()
        assert any(k in tr.module_losses for k in ('Exists', 'Xor', 'Equals')) and 'attention' in tr.module_losses
        out[frozen] = (_segments(tr, tr.flat_g.clone()), _segments(tr, tr.flat_p.clone()), _segments(tr, w0),
                       {k: v.clone() for k, v in tr.module_losses.items()})
    names = list(out[False][0])
    hit = {n for n in names if _is_frozen(n, prefixes)}
    assert P + prefixes[0] + '.weight' in hit and P + 'Localize.video_linear.3.bias' in hit and len(hit) == 2 + 6
    for n in hit:
        assert float(out[False][0][n].abs().max()) > 0, n            # the unfrozen step does train them
    for k, v in out[False][3].items():
        assert torch.equal(v, out[True][3][k]), k                     # the criteria's values do not depend on the flags
    for n in names:
        g0, g1 = out[False][0][n], out[True][0][n]
        if n in hit:
            assert int((g1 != 0).sum()) == 0 and torch.equal(out[True][1][n], out[True][2][n]), n
        else:
            assert float((g1 - g0).abs().max()) <= _tol(g0), (n, float((g1 - g0).abs().max()), _tol(g0))
            assert torch.equal(out[True][1][n], out[True][2][n]) == torch.equal(out[False][1][n], out[False][2][n]), n


def test_a_clip_cache_stays_fresh_while_the_video_encoder_is_frozen():
    from stair_amd.train import Trainer
    config = dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, answer_vocab_length=16, max_video_length=64, object_types=10)
    qs = [synth.make_question(config, 6, i, form=synth.ALL_FORMS[i], T=40) for i in range(12)]
    for i, q in enumerate(qs):
        q['video_id'] = 'clip%d' % i
    for freeze in (('video_encoder',), ()):
        model = _model(config, 6)
        tr = Trainer(model, dropout=0.0, lr=1e-3, freeze=freeze)
        cache = model.encode_clips([q['video_features'] for q in qs], ids=[q['video_id'] for q in qs])
        before = model.forward_batch(qs, clip_cache=cache).logits.clone()
        for it in range(2):
            tr.step(*_pack(qs))
        tr.check()
        if freeze:
            cache.check()
            cached = model.forward_batch(qs, clip_cache=cache).logits.clone()
            assert torch.equal(cached, model.forward_batch(qs).logits)
            assert float((cached - before).abs().max()) > 1e-5            # the steps did move the answers
        else:
            with pytest.raises(ValueError, match='stale.*re-encode'):
                model.forward_batch(qs, clip_cache=cache)


# ---------------------------------------------------------------------------------------------------------------------------
# the chain kernel's "no input gradient" marker (STAIR_TILE_NO_DX), as a building block
# ---------------------------------------------------------------------------------------------------------------------------
NO_DX = 0x20000000


def _chain(x, mask_in, mask_mid, w3, w0, out, out_idx):
    """Two-layer backward chain as stair_plan_backward queues it for Filter / Localize (mlp_tail_fused): dZ2 = x * relu'(mask_in)
    (kept), dZ1 = (dZ2 W3) * relu'(mask_mid) (kept), out[out_idx] += dZ1 W0, exclusively.  Returns (dZ2, dZ1)."""
    import ctypes as C
    from stair_amd._lib import TileMlpArgs, check, lib
    cnt, T, H = x.shape
    a = TileMlpArgs()
    a.X, a.x_gstride = x.data_ptr(), T * H
    a.in_mask, a.in_mask_gstride, a.in_scale, a.act_scale = mask_in.data_ptr(), T * H, 1.0, 1.0
    dz2, dz1 = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
    a.save_in = dz2.data_ptr()
    p3, p0 = ops.pack_wfrag(w3, transpose=True), ops.pack_wfrag(w0, transpose=True)
    a.W[0], a.act[0], a.act_mask[0], a.save[0] = p3.data_ptr(), 3, mask_mid.data_ptr(), dz1.data_ptr()
    a.W[1], a.n_layers = p0.data_ptr(), 2
    a.tail, a.out, a.out_gstride, a.out_idx, a.acc_exclusive = 6, out.data_ptr(), T * H, out_idx.data_ptr(), 1
    a.cnt, a.T, a.H = cnt, T, H
    check(lib.stair_tile_mlp_fwd(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return dz2, dz1


@pytest.mark.parametrize('T,cnt,marked', [(64, 5, (1, 3)),             # one instance per tile: two tiles end early
                                          (16, 7, (0, 1, 2, 3, 5)),    # four per tile: tile 0 all marked (dropped), tile 1 mixed (computed)
                                          (80, 3, (0, 2)),             # two segments per instance: both of a marked instance end early
                                          (37, 2, (1,))])             # an odd frame count
def test_chain_marker_drops_the_last_product_and_nothing_else(T, cnt, marked):
    H = 512
    g = torch.Generator().manual_seed(T)
    rnd = lambda *s: torch.randn(*s, generator=g).to(DEV)
    x, m_in, m_mid = rnd(cnt, T, H), rnd(cnt, T, H), rnd(cnt, T, H)
    w3, w0 = rnd(H, H) / 22.0, rnd(H, H) / 22.0
    base = rnd(cnt, T, H)                                   # what the gradient tiles hold before the launch
    plain_idx = torch.arange(cnt, dtype=torch.int32, device=DEV)
    out_ref = base.clone()
    ref = _chain(x, m_in, m_mid, w3, w0, out_ref, plain_idx)
    assert float((out_ref - base).abs().max()) > 0
    mark_idx = plain_idx.clone()
    for i in marked:
        mark_idx[i] |= NO_DX
    out = base.clone()
    got = _chain(x, m_in, m_mid, w3, w0, out, mark_idx)
    for a, b in zip(ref, got):
        assert torch.equal(a, b)                            # every dZ save is written as without the marker
    P = 64 // T if T <= 32 else 1
    for i in range(cnt):
        tile = range(i // P * P, min(i // P * P + P, cnt))
        dropped = all(j in marked for j in tile)            # a packed tile ends early only when all its instances are marked
        assert torch.equal(out[i], base[i] if dropped else out_ref[i]), (i, dropped)
    assert any(all(j in marked for j in range(i // P * P, min(i // P * P + P, cnt))) for i in range(cnt))
