"""Plans with clips of more than 64 frames at hidden size 512 (run with `-m gpu` on an MI355X): with stair_set_tile_split on (the
default) their map-level modules run on the fused tile operators as 64-row segments (csrc/tile_mlp.hip, SPLIT forms), and everything
stair_plan_run / stair_plan_backward hang off `fused` comes on with them: the grouped vector-level launches, first-touch gradient
stores, dropout drawn inside the operators, the bit-reproducible step.

H = 512, V = 128, one question per program form.  Bounds: those of tests/test_gpu_shape_contract.py for the same quantities (logits
1e-4 and the same top-1 against the oracle; gradients by its rule for the split-bf16 kernels, the helpers copied from there), of
tests/test_gpu_tile_fused.py::test_fused_and_sequenced_paths_agree_under_dropout for the switch on against off.  A reference is
computed once per shape and shared."""
import functools

import numpy as np
import pytest
import torch

from oracle import nmn_oracle as O
from stair_amd import spec, synth
from stair_amd._lib import lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RAGGED = (100, 70, 64, 33, 9)
# row kernels that only the launch-per-layer sequences of the tile modules launch (Filter, HasItem / FilterFrame, Temporal)
SEQUENCED_ONLY = ('sum_rows_kernel', 'rowdot_sigmoid_kernel', 'layernorm_kernel')


@pytest.fixture(autouse=True)
def default_switches():
    yield
    lib.stair_set_tile_split(-1)
    lib.stair_set_tile_queue(-1)


def _maxerr(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) if a.numel() else 0.0


def _config(L):
    return dict(spec.DEFAULT_CONFIG, video_size=128, answer_vocab_length=16, max_video_length=L, object_types=10)


def _model(config, seed=1, split=None):
    from stair_amd.module_net import VideoNMN
    m = VideoNMN(config)
    w = synth.make_weights(config, seed)
    m.load_state_dict({k: torch.from_numpy(w[k].copy()) for k in spec.state_dict_keys(config)})
    m = m.to(DEV)
    if split is not None:
        m.set_option('tile_split', split)
    return m


@functools.lru_cache(maxsize=None)
def _questions(L, T, lens=None):
    """12 questions, question i of program form synth.ALL_FORMS[i]; lens: clip i has lens[i % len(lens)] frames"""
    config = _config(L)
    qs = [synth.make_question(config, 5, i, form=f, T=(lens[i % len(lens)] if lens else T)) for i, f in enumerate(synth.ALL_FORMS)]
    assert [q['form'] for q in qs] == list(synth.ALL_FORMS)
    return config, qs


@functools.lru_cache(maxsize=None)
def _forward_reference(L, T):
    config, qs = _questions(L, T)
    w = O.to_torch(synth.make_weights(config, 1))
    with torch.no_grad():
        return [O.forward(w, config, q, return_res_by_step=False)['logits'] for q in qs]


@functools.lru_cache(maxsize=None)
def _backward_reference(L, T, lens=None):
    """autograd of the mean decoder CE through the oracle, every parameter (every question at its own length)"""
    config, qs = _questions(L, T, lens)
    names = [n for n, _ in spec.weight_table(config)]
    weights = synth.make_weights(config, 1)
    w = {k: torch.from_numpy(weights[k].copy()).requires_grad_(True) for k in names}
    total, per_q, logits = 0.0, [], []
    for q in qs:
        lg = O.forward(w, config, q, return_res_by_step=False, explicit_lstm=True)['logits']
        ce = torch.nn.functional.cross_entropy(lg.unsqueeze(0), torch.tensor([q['answer']]))
        per_q.append(float(ce.detach())); logits.append(lg.detach())
        total = total + ce / len(qs)
    total.backward()
    return names, {n: w[n].grad for n in names}, per_q, logits


def _train_step(config, qs, split=None, dropout=None):
    from stair_amd import ops
    model = _model(config, 1, split)
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    with ops.kernel_accounting() as acct:
        res = model.forward_batch(qs, train=True, dropout=dropout)
        res.forward_ws = res._ws.clone()            # what the forward pass saved (the backward pass reuses parts of it)
        nodes = []
        for qi, q in enumerate(qs):
            for i in range(len(q['nmn_program_list'])):
                v = res.node(qi, i)
                if isinstance(v, torch.Tensor):
                    nodes.append(v.detach().cpu().clone())
        losses = res.backward(torch.tensor([q['answer'] for q in qs], dtype=torch.int32, device=DEV), 1.0 / len(qs))
        torch.cuda.synchronize()
    res.nodes = nodes
    return res, losses, {n: p.grad.detach().cpu() for n, p in model.named_parameters()}, acct


# ---- the gradient rule of tests/test_gpu_shape_contract.py for the split-bf16 kernels (copied) ----------------------------------
def _strict_misses(names, got, grads):
    worst, bad = (0.0, ''), []
    for n in names:
        ref = grads[n] if grads[n] is not None else torch.zeros_like(got[n])
        err, tol = _maxerr(got[n], ref), 2e-4 * max(float(ref.abs().max()), 1e-3)
        worst = max(worst, (err / tol, n))
        if not err < tol:
            bad.append((n, err, float(ref.abs().max())))
    return worst, bad


def _gradients_through_hip_masks(config, qs, res):
    """The oracle's gradients with every module / decoder ReLU differentiated through the mask the HIP forward pass produced
    (tests/helpers.py::_ForcedMasks), and the number of sites at which the two implementations' masks differ."""
    from helpers import _ForcedMasks
    res._ws.copy_(res.forward_ws)
    names = [n for n, _ in spec.weight_table(config)]
    weights = synth.make_weights(config, 1)
    w = {k: torch.from_numpy(weights[k].copy()).requires_grad_(True) for k in names}
    flips = sites = 0
    for qi, q in enumerate(qs):
        fm = _ForcedMasks(res, qi, q['nmn_program_list'])
        with fm:
            orig_lin = O._lin

            def lin(w_, prefix, x, _fm=fm, _orig=orig_lin):     # the decoder's relu is the last one: its mask is queued behind the modules'
                if prefix.endswith('decoder.0'):
                    _fm.decoder()
                return _orig(w_, prefix, x)
            O._lin = lin
            try:
                lg = O.forward(w, config, q, return_res_by_step=False, explicit_lstm=True)['logits']
            finally:
                O._lin = orig_lin
        ce = torch.nn.functional.cross_entropy(lg.unsqueeze(0), torch.tensor([q['answer']]))
        (ce / len(qs)).backward()
        flips, sites = flips + fm.flips, sites + fm.sites
    return {n: w[n].grad for n in names}, flips, sites


FRAC_OUTSIDE_STRICT = 0.3


def _check_split(tag, names, got, grads, config, qs, res):
    """relative L2 per tensor, a loose max-abs bound, and the fraction of entries outside the strict elementwise bound; a miss is
    accepted only if ReLU masks differ (at most 1 in 10 000 sites) and, through the HIP pass's masks, every parameter is strict"""
    worst_l2, worst_frac, bad = (0.0, ''), (0.0, ''), []
    for n in names:
        ref = grads[n]
        if ref is None:
            continue
        g = got[n]
        rel_l2 = float((g - ref).norm() / ref.norm().clamp_min(1e-12))
        lim = 1e-2 if ref.numel() >= 64 else 2e-2
        worst_l2 = max(worst_l2, (rel_l2 / lim, n))
        if not rel_l2 < lim:
            bad.append((n, 'rel_l2', rel_l2))
        if not float((g - ref).abs().max()) < 0.05 * float(ref.abs().max()) + 3e-6:
            bad.append((n, 'max_abs', float((g - ref).abs().max()), float(ref.abs().max())))
        if ref.numel() >= 512:
            frac = float(((g - ref).abs() > 2e-4 * float(ref.abs().max()) + 1e-9).float().mean())
            worst_frac = max(worst_frac, (frac, n))
    print('LONGCLIP: backward %s worst rel. L2 / limit = %.3g in %s; largest fraction outside 2e-4 max|g| = %.3g in %s' % (
        (tag,) + worst_l2 + worst_frac))
    if bad or not worst_frac[0] < FRAC_OUTSIDE_STRICT:
        forced, flips, sites = _gradients_through_hip_masks(config, qs, res)
        worst, bad_forced = _strict_misses(names, got, forced)
        print('LONGCLIP: backward %s ReLU masks that differ: %d of %d; through the HIP masks worst error / tolerance = %.3g in %s' % (
            (tag, flips, sites) + worst))
        assert 0 < flips <= 1e-4 * sites, (flips, sites, bad, worst_frac)
        assert not bad_forced, bad_forced


def _check_logits(tag, res, logits):
    worst = max(_maxerr(res.logits[i], lg) for i, lg in enumerate(logits))
    print('LONGCLIP: forward %s worst error / tolerance = %.3g' % (tag, worst / 1e-4))
    for i, lg in enumerate(logits):
        assert _maxerr(res.logits[i], lg) < 1e-4, (i, _maxerr(res.logits[i], lg))
        assert int(res.pred[i]) == int(torch.argmax(lg)), i


def _check_fused(acct):
    assert 'tile_mlp' in acct.table and 'vec_group' in acct.table, sorted(acct.table)
    assert not set(SEQUENCED_ONLY) & set(acct.table), sorted(acct.table)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L,T', [(100, 100), (141, 141)])
def test_forward_of_long_clips_runs_fused_and_matches_the_oracle(L, T):
    from stair_amd import ops
    config, qs = _questions(L, T)
    model = _model(config)
    with ops.kernel_accounting() as acct:
        res = model.forward_batch(qs)
        torch.cuda.synchronize()
    _check_fused(acct)
    _check_logits('L=%d T=%d' % (L, T), res, _forward_reference(L, T))
    # the control: with the switch off the same plan runs the launch-per-layer sequences
    off = _model(config, split=0)
    with ops.kernel_accounting() as acct_off:
        res_off = off.forward_batch(qs)
        torch.cuda.synchronize()
    assert 'tile_mlp' not in acct_off.table and set(SEQUENCED_ONLY) <= set(acct_off.table), sorted(acct_off.table)
    assert _maxerr(res_off.logits, res.logits) < 2e-5


@pytest.mark.parametrize('L,T', [(100, 100), (140, 113)])
def test_training_step_of_long_clips_against_the_oracle(L, T):
    """one step in the default matmul mode; T = 113 at max_video_length 140 is the training limit (Superlative's backward image,
    Conv1d filters of k = 35), every form: Superlative (P3, C1) and Temporal before / after / between among them"""
    config, qs = _questions(L, T)
    names, grads, per_q, logits = _backward_reference(L, T)
    res, losses, got, acct = _train_step(config, qs)
    _check_fused(acct)
    _check_logits('train L=%d T=%d' % (L, T), res, logits)
    assert np.allclose(losses.cpu().numpy(), per_q, rtol=1e-5, atol=2e-5)
    _check_split('L=%d T=%d' % (L, T), names, got, grads, config, qs, res)


def test_ragged_training_step_of_long_clips():
    """T = 100 with clips of 100, 70, 64, 33 and 9 frames: a partial second segment, and second segments with no live frame at all
    (not computed, zeros).  Frames behind a clip's end are exact zeros in every map / attention node output."""
    config, qs = _questions(100, 100, RAGGED)
    names, grads, per_q, logits = _backward_reference(100, 100, RAGGED)
    res, losses, got, acct = _train_step(config, qs)
    assert sorted(set(int(x) for x in res.question_frames)) == sorted(RAGGED)
    _check_fused(acct)
    _check_logits('ragged T=100', res, logits)
    assert np.allclose(losses.cpu().numpy(), per_q, rtol=1e-5, atol=2e-5)
    _check_split('ragged T=100', names, got, grads, config, qs, res)
    res._ws.copy_(res.forward_ws)
    checked = 0
    for qi, q in enumerate(qs):
        ln = int(res.question_frames[qi])
        for i in range(len(q['nmn_program_list'])):
            v = res.node(qi, i)
            if ln >= 100 or not isinstance(v, torch.Tensor):
                continue
            if tuple(v.shape[-2:]) == (100, 512):               # a [T, H] map
                assert float(v[ln:].abs().max()) == 0.0, (qi, i)
                checked += 1
            elif v.shape[-1] == 100:                            # [T] or [K, T] attention rows
                assert float(v[..., ln:].abs().max()) == 0.0, (qi, i)
                checked += 1
    assert checked > 20, checked


@pytest.mark.parametrize('dropout', [None, (0.25, 7)], ids=['plain', 'dropout'])
def test_switch_on_agrees_with_switch_off(dropout):
    """same batch, same seed: the segmented operators against the launch-per-layer sequences, under the bounds of
    tests/test_gpu_tile_fused.py::test_fused_and_sequenced_paths_agree_under_dropout"""
    config, qs = _questions(100, 100)
    out = {}
    for split in (1, 0):
        res, losses, grads, acct = _train_step(config, qs, split=split, dropout=dropout)
        assert ('tile_mlp' in acct.table) == bool(split), sorted(acct.table)
        out[split] = (res.logits.cpu().clone(), res.nodes, losses.cpu().clone(), grads)
    assert float((out[1][0] - out[0][0]).abs().max()) < 5e-5
    zeros = 0
    for a, b in zip(out[1][1], out[0][1]):
        assert float((a - b).abs().max()) < 5e-5 * max(1.0, float(b.abs().max()))
        assert torch.equal(a == 0, b == 0) or float(((a == 0) != (b == 0)).float().mean()) < 1e-4     # the same elements dropped
        zeros += int((b == 0).sum())
    assert not dropout or zeros > 1000
    assert torch.allclose(out[1][2], out[0][2], rtol=2e-5, atol=2e-5)
    gmax = max(float(g.abs().max()) for g in out[0][3].values())
    tight = 0
    for n, g in out[0][3].items():
        dd = (out[1][3][n] - g).abs()
        scale = max(float(g.abs().max()), 1e-3 * gmax)
        assert float(dd.norm()) <= 3e-2 * max(float(g.norm()), 1e-3 * gmax), n
        assert float(dd.max()) <= 0.1 * scale, n
        tight += float(dd.max()) < 4e-4 * scale
    assert tight >= 0.8 * len(out[0][3]), tight


def test_training_step_of_long_clips_is_reproducible_under_dropout():
    """two fresh trainers, T = 100, dropout 0.25: the gradient bucket and the weights after Adam bit for bit -- what DESIGN section 3
    used to list as order-dependent (the unfused operator sequences at T > 64)"""
    from stair_amd import ops
    from stair_amd.train import Trainer
    config, qs = _questions(100, 100)
    video = torch.stack([torch.as_tensor(q['video_features']) for q in qs]).to(DEV)
    question = torch.cat([torch.as_tensor(q['question']) for q in qs]).to(DEV)
    args = ([q['nmn_program_list'] for q in qs], [q['prog_str_to_question_tokens'] for q in qs], video, question,
            [q['question'].shape[0] for q in qs], torch.tensor([q['answer'] for q in qs], dtype=torch.int32, device=DEV))
    runs = []
    for _ in range(2):
        tr = Trainer(_model(config, 5), dropout=0.25, lr=1e-3)
        with ops.kernel_accounting() as acct:
            tr.step(*args)
        tr.check()
        torch.cuda.synchronize()
        runs.append((tr.flat_g.clone(), tr.flat_p.clone()))
        _check_fused(acct)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert float(runs[0][0].abs().max()) > 0


@pytest.mark.parametrize('queue', [1, 0])
def test_captured_long_clip_plan_replays_bit_exactly(queue):
    config, qs = _questions(100, 100)
    model = _model(config, 4)
    lib.stair_set_tile_queue(queue)
    want = model.forward_batch(qs).logits.clone()
    cap = model.forward_batch(qs).capture_graph()
    for rep in range(4):
        cap.logits.zero_()
        logits, _ = cap.replay()
        torch.cuda.synchronize()
        assert torch.equal(logits, want), rep
    off = cap.result.info.status_off
    assert int(cap._ws[off + 16: off + 20].view(torch.int32).abs().sum()) == 0


@pytest.mark.parametrize('L,T', [(64, 64), (8, 8)])
def test_short_clips_do_not_see_the_switch(L, T):
    """T <= 64 takes none of the new code: logits and every gradient bit for bit with the switch on and off"""
    config, qs = _questions(L, T)
    out = {}
    for split in (1, 0):
        res, losses, grads, acct = _train_step(config, qs, split=split)
        assert 'tile_mlp' in acct.table
        out[split] = (res.logits.cpu().clone(), grads)
    assert torch.equal(out[1][0], out[0][0])
    for n, g in out[0][1].items():
        assert torch.equal(out[1][1][n], g), n
