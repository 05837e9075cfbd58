"""GPU tests (`-m gpu`) of Trainer(max_grad_norm=...): clipping by global gradient norm between the exchange and Adam, on the
device, against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on the oracle's weights; the refusal of a step whose
gradient norm is not finite; the norm telemetry.  The reference loop has no clipping (train_module.py:408-412), so the
yardstick is torch's own clip on autograd gradients of the oracle."""
import math

import pytest
import torch

from oracle import nmn_oracle as O
from stair_amd import spec, synth
from helpers import load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(params=['f32', 'bf16x3'])
def matmul(request):
    from stair_amd import ops
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


WINDOWS = [['P1', 'P4', 'P1', 'P4'], ['P0', 'P2', 'P3', 'P5'], ['P6', 'P7', 'C0', 'C1']]     # test_trainer_steps_match_torch_adam's
LOSS_WEIGHTS = [10.0, 1.0, 1.0]                 # the first window's decoder loss ten times heavier: a hard clip, none, a mild one
MAX_NORM, LR, B1 = 2.0, 2e-4, 0.9


def _windows(config):
    out, qid = [], 100
    for forms in WINDOWS:
        out.append([synth.make_question(config, 5, qid + i, form=f, T=40) for i, f in enumerate(forms)])
        qid += len(forms)
    return out


_ORACLE = {}


def _oracle_run():
    """Three clipped Adam steps on the oracle (CPU, computed once): per step the unclipped gradients, their norm and the
    coefficient; torch's exp_avg after the first step; the final weights."""
    if _ORACLE:
        return _ORACLE
    z, meta = load_golden('tiny_conv')
    config = meta['config']
    names = [n for n, _ in spec.weight_table(config)]
    wts = synth.make_weights(config, 0)
    w = {k: torch.from_numpy(wts[k].copy()).requires_grad_(True) for k in names}
    opt = torch.optim.Adam([w[n] for n in names], lr=LR)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda it: 1.0 + (0.1 - 1.0) / 10 * it if it <= 10 else 0.1)
    steps = []
    for qs, weight in zip(_windows(config), LOSS_WEIGHTS):
        total = 0.0
        for q in qs:
            logits = O.forward(w, config, q, return_res_by_step=False, explicit_lstm=True)['logits']
            total = total + torch.nn.functional.cross_entropy(logits.unsqueeze(0), torch.tensor([q['answer']])) * (weight / len(qs))
        total.backward()
        grads = {n: (None if w[n].grad is None else w[n].grad.detach().clone()) for n in names}
        norm = float(torch.nn.utils.clip_grad_norm_([w[n] for n in names], MAX_NORM))
        coef = float(torch.clamp(MAX_NORM / (torch.tensor(norm, dtype=torch.float32) + 1e-6), max=1.0))
        opt.step(); opt.zero_grad(set_to_none=False); sched.step()
        st = dict(grads=grads, norm=norm, coef=coef)
        if not steps:
            st['exp_avg'] = {n: opt.state[w[n]]['exp_avg'].clone() for n in names if w[n] in opt.state}
        steps.append(st)
    _ORACLE.update(config=config, names=names, steps=steps, final={n: w[n].detach().clone() for n in names})
    return _ORACLE


def _tol(g_ref):
    """the project's gradient tolerance (test_backward_matches_autograd_of_oracle)"""
    return 2e-4 * max(float(g_ref.abs().max()), 1e-3)


def test_clipped_steps_match_torch_clip_then_adam(matmul):
    from stair_amd.train import Trainer
    ora = _oracle_run()
    config, names, steps = ora['config'], ora['names'], ora['steps']
    print('oracle norms', [s['norm'] for s in steps], 'coefficients', [s['coef'] for s in steps])
    # the pattern the case is built for, on the oracle alone: a hard clip, no clip, a mild clip
    assert steps[0]['coef'] < 0.2 and steps[1]['coef'] == 1.0 and steps[2]['coef'] < 1.0

    model = _model(config, 0)
    tr = Trainer(model, lr=LR, scheduler_total_iters=10, skip_untouched='ever', dropout=0.0, max_grad_norm=MAX_NORM)
    got_norms = []
    for it, (qs, weight) in enumerate(zip(_windows(config), LOSS_WEIGHTS)):
        tr.decoder_loss_weight = weight                       # read every step
        _, res = tr.step(*_pack(qs))
        torch.cuda.synchronize()
        norm, coef = (float(x) for x in tr.grad_norm.cpu())
        got_norms.append((norm, coef))
        own = math.sqrt(float((tr.flat_g.double() ** 2).sum()))
        print('step %d: norm %.7g (own fp64 %.7g, oracle %.7g), coefficient %.7g (oracle %.7g)' % (it, norm, own, steps[it]['norm'], coef,
                                                                                           steps[it]['coef']))
        assert abs(norm - own) <= 2e-6 * own                  # the kernel's bound (tests/test_gpu_grad_norm.py)
        # against the oracle: every entry of tensor t may be off by tol_t, so the norm by sqrt(sum_t numel_t tol_t^2)
        bound = math.sqrt(sum(g.numel() * _tol(g) ** 2 for g in steps[it]['grads'].values() if g is not None))
        assert abs(norm - steps[it]['norm']) <= bound, (it, norm, steps[it]['norm'], bound)
        by_name = tr.grad_norms_by_name()
        assert list(by_name) == list(model._weight_names) and set(by_name) == set(names)
        for nme, t in zip(model._weight_names, res.touched()):
            if not t:
                assert by_name[nme] == 0.0, nme
        assert sum(1 for v in by_name.values() if v > 0) > 10
        assert abs(math.sqrt(sum(v * v for v in by_name.values())) - norm) <= 1e-5 * norm
        if it == 0:
            # an unclipped first step would be off by 1 / coefficient = 7.6 x: the tolerance is the gradient tolerance carried
            # through exp_avg = (1 - beta1) * coefficient * g
            offs = dict(zip(model._weight_names, tr.offsets))
            for n, ref in steps[0]['exp_avg'].items():
                g_ref = steps[0]['grads'][n]
                if g_ref is None:
                    continue
                got = tr.exp_avg[offs[n]: offs[n] + ref.numel()].view_as(ref).cpu()
                tol = _tol(g_ref) * (1 - B1) * steps[0]['coef']
                assert float((got - ref).abs().max()) <= tol, (n, float((got - ref).abs().max()), tol)
    assert got_norms[0][1] < 0.2 and got_norms[1][1] == 1.0 and got_norms[2][1] < 1.0
    assert tr.finished_grad_norms() == [(i, n_, c_) for i, (n_, c_) in enumerate(got_norms)]
    assert tr.finished_grad_norms() == []
    tr.check()
    got = dict(model.named_parameters())
    for n in names:
        diff = (got[n].detach().cpu() - ora['final'][n]).abs()
        if matmul == 'f32':                                   # test_trainer_steps_match_torch_adam's own bounds
            assert float(diff.max()) < 2e-5, (n, float(diff.max()))
        else:
            assert float((diff < 2e-5).float().mean()) > 0.995, (n, float((diff < 2e-5).float().mean()))
            assert float(diff.max()) < 2.5e-4, (n, float(diff.max()))


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


def test_measuring_changes_nothing_and_clipping_is_bit_reproducible():
    from stair_amd.train import Trainer
    config, args, vidx = _full_size_batch()

    def run(max_grad_norm):
        tr = Trainer(_model(config, 5), dropout=0.0, lr=1e-3, max_grad_norm=max_grad_norm)
        for it in range(2):
            tr.step(*args, video_index=vidx)
        tr.check()
        norms = tr.finished_grad_norms() if max_grad_norm is not None else None
        return (tr.flat_p.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone()), norms

    plain, _ = run(None)
    measured, norms = run(float('inf'))
    assert [s for s, _, _ in norms] == [0, 1] and all(c == 1.0 for _, _, c in norms) and norms[0][1] > 0
    for a, b in zip(plain, measured):
        assert torch.equal(a, b)                              # max_grad_norm = inf: the same bits as no clipping at all
    clip_at = 0.5 * norms[0][1]
    one, n1 = run(clip_at)
    two, n2 = run(clip_at)
    assert n1 == n2 and n1[0][2] < 1.0 and abs(n1[0][2] - 0.5) < 1e-3 and n1[0][1] == norms[0][1]
    for a, b in zip(one, two):
        assert torch.equal(a, b)
    assert not torch.equal(one[1], plain[1])                  # ... and the clip did reach the moments


def test_nonfinite_step_is_refused_and_named():
    from stair_amd._lib import StairError
    from stair_amd.train import Trainer
    z, meta = load_golden('tiny_conv')
    config = meta['config']
    windows = _windows(config)
    tr = Trainer(_model(config, 0), lr=LR, dropout=0.0, max_grad_norm=float('inf'))
    tr.step(*_pack(windows[0]))
    tr.check()
    before = [t.clone() for t in (tr.flat_p, tr.exp_avg, tr.exp_avg_sq, tr.steps, tr.touched)]
    assert float(tr.steps.max()) == 1.0
    tr.inject_nonfinite = True
    tr.step(*_pack(windows[1]))
    tr.inject_nonfinite = False
    torch.cuda.synchronize()
    for a, b in zip(before, (tr.flat_p, tr.exp_avg, tr.exp_avg_sq, tr.steps, tr.touched)):
        assert torch.equal(a, b)
    assert int(tr.guard) == 2
    assert not math.isfinite(float(tr.grad_norm[0]))
    with pytest.raises(StairError) as err:
        tr.check()
    assert 'non-finite gradient norm in optimizer step 1' in str(err.value) and 'recurrence' not in str(err.value)
    tr.step(*_pack(windows[1]))                               # the caller goes on: a healthy step applies
    tr.check()
    assert int(tr.guard) == 0 and float(tr.steps.max()) == 2.0 and not torch.equal(tr.flat_p, before[0])
    assert math.isfinite(float(tr.grad_norm[0])) and float(tr.grad_norm[0]) > 0
    assert bool(tr.flat_p.isfinite().all()) and bool(tr.exp_avg.isfinite().all()) and bool(tr.exp_avg_sq.isfinite().all())


@pytest.mark.parametrize('bad', [0, -1, 'x', float('nan'), True])
def test_max_grad_norm_argument_is_checked(bad):
    from stair_amd.train import Trainer
    z, meta = load_golden('tiny_conv')
    with pytest.raises(ValueError):
        Trainer(_model(meta['config'], 0), max_grad_norm=bad)


def test_default_trainer_measures_nothing():
    from stair_amd.train import Trainer
    z, meta = load_golden('tiny_conv')
    tr = Trainer(_model(meta['config'], 0), dropout=0.0)
    assert tr.max_grad_norm is None and tr.grad_norm is None and tr.seg_grad_norm is None
    with pytest.raises(RuntimeError):
        tr.grad_norms_by_name()
