"""GPU tests of the SHAPES include/stair_hip.h admits and no other file reaches (run with `-m gpu` on an MI355X):

  * hidden sizes 192, 320, 384, 448 (LSTM Hh = 96, 160, 192, 224: tile counts that are no power of two, odd k-block counts, the
    fp32 recurrence between split GEMMs; row walks with a whole trip and a partial one; 3, 5, 6, 7 column chunks), forward and
    backward, and the backward pass at H = 256 (the one-pass LayerNorm adjoint for H = 256, the H % 256 == 0 slab layout);
  * the README's I3D shape (V = 1024, T = 64) at full hidden size;
  * frame counts up to the training limit (T = 113: the largest LDS image of Superlative's backward kernel; max_video_length
    140: the largest admitted Conv1d filters, k = 35 / 71 taps) and, forward only, beyond 128 frames (Superlative's per-pair
    fallback).  tests/test_abi.py holds the host side: training plans beyond those limits are refused when they are built.

Every comparison is against the oracle (oracle/nmn_oracle.py, differentiable torch code on the CPU) run on the same seeded
inputs, with the bounds of the tests these are modelled on (tests/test_gpu_parity.py, tests/test_gpu_train.py,
tests/test_gpu_ragged.py).  A reference is computed once per shape and shared by the tests and matmul modes that need it.
Each test prints its worst error / tolerance behind the tag SHAPE: (DESIGN.md section 4 has the table)."""
import functools

import numpy as np
import pytest
import torch

from oracle import nmn_oracle as O
from stair_amd import spec, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(params=['f32', 'bf16x3'])
def matmul(request):
    """Every test that takes it runs under the exact fp32 MFMA and under the default split-precision kernels."""
    from stair_amd import ops
    ops.set_matmul_mode(request.param)
    yield request.param
    ops.set_matmul_mode('bf16x3')


def _tol(matmul, exact, split):
    return exact if matmul == 'f32' else split


def _maxerr(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) if a.numel() else 0.0


def _model(config, seed):
    from stair_amd.module_net import VideoNMN
    m = VideoNMN(config)
    w = synth.make_weights(config, seed)
    m.load_state_dict({k: torch.from_numpy(w[k].copy()) for k in spec.state_dict_keys(config)})
    return m.to(DEV)


def _config(H, V, L):
    if (H, L) == (512, 64):                  # the I3D shape keeps the full-size answer vocabulary and head width
        return dict(spec.DEFAULT_CONFIG, video_size=V)
    return dict(spec.DEFAULT_CONFIG, hidden_size=H, video_size=V, answer_vocab_length=16, max_video_length=L, object_types=10)


def _recurrence(Hh, matmul):
    """the names csrc/lstm.hip's launchers report: the split recurrence needs Hh % 64 == 0 (it walks k blocks in pairs)"""
    split = matmul != 'f32' and Hh % 64 == 0
    return ('lstm_rec_x3', 'lstm_bwd_x3') if split else ('lstm_rec_f32', 'lstm_bwd_f32')


# ---------------------------------------------------------------------------------------------
# 1. LSTM building block at Hh = 96, 160, 192, 224
# ---------------------------------------------------------------------------------------------
LSTM_I = 132                                                          # a multiple of 4, not of 32
LSTM_LENS = [5, 1, 9, 9, 3, 2, 7, 4, 6, 8, 1, 3, 5, 9, 2, 4, 7]      # 17: the second 16-sequence workgroup holds ONE sequence; length 1 in both
LSTM_NAMES = ['submodules.video_encoder.' + n + sfx for sfx in ('', '_reverse')
              for n in ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0')]


@functools.lru_cache(maxsize=None)
def _lstm_reference(Hh):
    """Inputs, the oracle's outputs per sequence and autograd's parameter gradients of sum(out * d_out) + sum(h_n * d_hn)."""
    cfg = dict(spec.DEFAULT_CONFIG, hidden_size=2 * Hh, video_size=LSTM_I, max_video_length=64)
    w = {k: v.clone().requires_grad_(k in LSTM_NAMES) for k, v in O.to_torch(synth.make_weights(cfg, 4)).items()}
    g = torch.Generator().manual_seed(Hh + LSTM_I)
    xs = [torch.randn(n, LSTM_I, generator=g) for n in LSTM_LENS]
    d_outs = [torch.randn(n, 2 * Hh, generator=g) for n in LSTM_LENS]
    d_hn = torch.randn(len(LSTM_LENS), 2 * Hh, generator=g)
    loss, outs, hns = 0, [], []
    for s, x in enumerate(xs):
        ro, rh = O.lstm_bidir_explicit(w, 'video_encoder', x)
        outs.append(ro.detach()); hns.append(rh.detach().reshape(-1))
        loss = loss + (ro * d_outs[s]).sum() + (rh.reshape(-1) * d_hn[s]).sum()
    loss.backward()
    return dict(xs=xs, d_outs=d_outs, d_hn=d_hn, outs=outs, hns=hns, weights=[w[n].detach() for n in LSTM_NAMES],
                grads=[w[n].grad for n in LSTM_NAMES])


@pytest.mark.parametrize('Hh', [96, 160, 192, 224])
def test_lstm_forward_at_in_between_hidden_sizes(Hh, matmul):
    from stair_amd import ops
    r = _lstm_reference(Hh)
    off = torch.tensor(np.concatenate([[0], np.cumsum(LSTM_LENS)]), dtype=torch.int32)
    with ops.kernel_accounting() as acct:
        out, h_n = ops.lstm_bidir(torch.cat(r['xs']).to(DEV), off.to(DEV), max(LSTM_LENS), [w.to(DEV) for w in r['weights']])
    want = _recurrence(Hh, matmul)[0]
    assert want in acct.table and not ({'lstm_rec_x3', 'lstm_rec_f32'} - {want}) & set(acct.table), sorted(acct.table)
    tol = _tol(matmul, 2e-5, 1e-4)
    errs = [max(_maxerr(out[off[s]:off[s + 1]], r['outs'][s]), _maxerr(h_n[s], r['hns'][s])) for s in range(len(LSTM_LENS))]
    print('SHAPE: lstm forward Hh=%d %s %s worst error / tolerance = %.3g' % (Hh, matmul, want, max(errs) / tol))
    for s, e in enumerate(errs):
        assert e < tol, (s, e)


@pytest.mark.parametrize('Hh', [96, 160, 192, 224])
def test_lstm_backward_at_in_between_hidden_sizes(Hh, matmul):
    from stair_amd import ops
    r = _lstm_reference(Hh)
    off = torch.tensor(np.concatenate([[0], np.cumsum(LSTM_LENS)]), dtype=torch.int32).to(DEV)
    X = torch.cat(r['xs']).to(DEV)
    ws = [w.to(DEV) for w in r['weights']]
    with ops.kernel_accounting() as acct:
        out, h_n, gates, cbuf = ops.lstm_bidir(X, off, max(LSTM_LENS), ws, save=True)
        grads = ops.lstm_bidir_bwd(X, off, max(LSTM_LENS), ws, out, gates, cbuf, torch.cat(r['d_outs']).to(DEV), r['d_hn'].to(DEV))
    rec, bwd = _recurrence(Hh, matmul)
    assert rec in acct.table and bwd in acct.table, sorted(acct.table)
    assert not ({'lstm_rec_x3', 'lstm_rec_f32', 'lstm_bwd_x3', 'lstm_bwd_f32'} - {rec, bwd}) & set(acct.table), sorted(acct.table)
    worst = (0.0, '')
    for n, gr, ref in zip(LSTM_NAMES, grads, r['grads']):
        worst = max(worst, (_maxerr(gr, ref) / (2e-4 * max(1.0, float(ref.abs().max()))), n))
    print('SHAPE: lstm backward Hh=%d %s %s worst error / tolerance = %.3g in %s' % (Hh, matmul, bwd, worst[0], worst[1]))
    for n, gr, ref in zip(LSTM_NAMES, grads, r['grads']):
        scale = max(1.0, float(ref.abs().max()))
        assert _maxerr(gr, ref) < 2e-4 * scale, (n, _maxerr(gr, ref), scale)


@pytest.mark.parametrize('Hh', [96, 160, 192, 224])
def test_lstm_padded_storage_at_in_between_hidden_sizes(Hh):
    """Rows at one stride with a seq_len array and zero padding rows (how a plan with mixed clip lengths stores its clips): `out`
    rows past each length are exactly zero, the rest equals the per-sequence oracle.  Default (split) matmul mode: at Hh = 96, 160,
    224 that is the fp32 recurrence behind a split-precision input projection."""
    from stair_amd import ops
    assert ops.get_matmul_mode() == 'bf16x3'
    r = _lstm_reference(Hh)
    n, stride = len(LSTM_LENS), max(LSTM_LENS)
    X = torch.zeros(n * stride, LSTM_I)
    for s, x in enumerate(r['xs']):
        X[s * stride: s * stride + LSTM_LENS[s]] = x
    off = torch.arange(n + 1, dtype=torch.int32) * stride
    seq_len = torch.tensor(LSTM_LENS, dtype=torch.int32)
    with ops.kernel_accounting() as acct:
        out, h_n = ops.lstm_bidir(X.to(DEV), off.to(DEV), stride, [w.to(DEV) for w in r['weights']], seq_len=seq_len.to(DEV))
    assert _recurrence(Hh, 'bf16x3')[0] in acct.table, sorted(acct.table)
    out, h_n = out.cpu(), h_n.cpu()
    worst = 0.0
    for s in range(n):
        rows = out[s * stride: (s + 1) * stride]
        assert float(rows[LSTM_LENS[s]:].abs().max()) == 0.0 if LSTM_LENS[s] < stride else True, s
        worst = max(worst, _maxerr(rows[:LSTM_LENS[s]], r['outs'][s]), _maxerr(h_n[s], r['hns'][s]))
    print('SHAPE: lstm padded Hh=%d bf16x3 %s worst error / tolerance = %.3g' % (Hh, _recurrence(Hh, 'bf16x3')[0], worst / 1e-4))
    assert worst < 1e-4, worst


# ---------------------------------------------------------------------------------------------
# 2. / 3. / 5. whole model: references shared by the tests below
# ---------------------------------------------------------------------------------------------
def _questions(config, T, bf16=False):
    """12 questions: question i has program form synth.ALL_FORMS[i] (synth.make_questions would DRAW a form per question)"""
    qs = [synth.make_question(config, 5, i, form=f, T=T) for i, f in enumerate(synth.ALL_FORMS)]
    assert [q['form'] for q in qs] == list(synth.ALL_FORMS)
    if bf16:
        for q in qs:
            q['video_features'] = torch.as_tensor(q['video_features']).to(torch.bfloat16)
    return qs


def _oracle_q(q):
    v = q['video_features']
    return dict(q, video_features=v.float() if isinstance(v, torch.Tensor) else v)


@functools.lru_cache(maxsize=None)
def _forward_reference(H, V, L, T, bf16=False):
    """12 questions, one per program form, and the oracle's logits of every one (the full-size I3D shape: every other one, which
    keeps both Superlative forms, P3 and C1, among those compared)"""
    config = _config(H, V, L)
    qs = _questions(config, T, bf16)
    w = O.to_torch(synth.make_weights(config, 1))
    pick = [qi for qi in range(12) if H < 512 or qi % 2 == 1]
    assert {'P3', 'C1'} <= {qs[qi]['form'] for qi in pick}
    with torch.no_grad():
        ref = {qi: O.forward(w, config, _oracle_q(qs[qi]), return_res_by_step=False)['logits'] for qi in pick}
    return config, qs, ref


def _oracle_gradients(config, qs):
    names = [n for n, _ in spec.weight_table(config)]
    weights = synth.make_weights(config, 1)
    w = {k: torch.from_numpy(weights[k].copy()).requires_grad_(True) for k in names}
    total, per_q, logits = 0.0, [], []
    for q in qs:
        lg = O.forward(w, config, _oracle_q(q), return_res_by_step=False, explicit_lstm=True)['logits']
        ce = torch.nn.functional.cross_entropy(lg.unsqueeze(0), torch.tensor([q['answer']]))       # train_module.py:193-194
        per_q.append(float(ce.detach())); logits.append(lg.detach())
        total = total + ce / len(qs)
    total.backward()
    return names, {n: w[n].grad for n in names}, per_q, logits


@functools.lru_cache(maxsize=None)
def _backward_reference(H, V, L, T):
    """the same 12 questions: autograd of the mean decoder CE through the oracle, every parameter"""
    config = _config(H, V, L)
    qs = _questions(config, T)
    return (config, qs) + _oracle_gradients(config, qs)


def _check_forward(tag, matmul, H, res, ref, acct):
    worst = 0.0
    for qi, lg in ref.items():
        worst = max(worst, _maxerr(res.logits[qi], lg))
    rec = _recurrence(H // 2, matmul)[0]
    if H == 512 and rec not in acct.table:          # Hh = 256: the cooperative recurrence where its workgroups are co-resident
        rec = 'lstm_rec_coop'
    print('SHAPE: forward %s %s %s worst error / tolerance = %.3g' % (tag, matmul, rec, worst / 1e-4))
    assert any(k.startswith(rec) for k in acct.table), sorted(acct.table)
    for qi, lg in ref.items():
        assert _maxerr(res.logits[qi], lg) < 1e-4, (qi, _maxerr(res.logits[qi], lg))           # the project's contract
        assert int(res.pred[qi]) == int(torch.argmax(lg)), qi


def _train_step(config, qs):
    from stair_amd import ops
    model = _model(config, 1)
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    with ops.kernel_accounting() as acct:
        res = model.forward_batch(qs, train=True)
        res.forward_ws = res._ws.clone()            # what the forward pass saved (the backward pass reuses parts of it): _gradients_through_hip_masks
        losses = res.backward(torch.tensor([q['answer'] for q in qs], dtype=torch.int32, device=DEV), 1.0 / len(qs))
        torch.cuda.synchronize()
    return res, losses, {n: p.grad.detach().cpu() for n, p in model.named_parameters()}, acct


def _strict_misses(names, got, grads):
    """(worst error / tolerance, its tensor), [tensors outside]: the elementwise bound of tests/test_gpu_train.py::
    test_backward_on_odd_shapes for every parameter; a parameter no program of the batch uses must have a zero gradient"""
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
    (tests/helpers.py::_ForcedMasks, as test_full_size_gradients_are_strict_given_the_same_relu_masks does), and the
    number of sites at which the two implementations' masks differ."""
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
                lg = O.forward(w, config, _oracle_q(q), return_res_by_step=False, explicit_lstm=True)['logits']
            finally:
                O._lin = orig_lin
        ce = torch.nn.functional.cross_entropy(lg.unsqueeze(0), torch.tensor([q['answer']]))
        (ce / len(qs)).backward()
        flips, sites = flips + fm.flips, sites + fm.sites
    return {n: w[n].grad for n in names}, flips, sites


def _check_strict(tag, names, got, grads, config=None, qs=None, res=None):
    """Every parameter at the strict elementwise bound.  The bound compares two implementations of a function with kinks: where a
    ReLU input lies within fp32 rounding of zero, the MFMA's and ATen's summation orders can put it on different sides, and that
    unit's row of the layer's weight gradient moves by one sample's contribution.  With millions of ReLU
    sites that happens in exact-fp32 mode too.  Where the plain comparison misses and the caller hands over the pass (`res`), the
    miss must BE such a flip: some masks differ (at most 1 in 100 000), and with the oracle differentiated through the HIP
    pass's masks every parameter is inside the same strict bound."""
    worst, bad = _strict_misses(names, got, grads)
    print('SHAPE: backward %s worst error / tolerance = %.3g in %s' % (tag, worst[0], worst[1]))
    if bad and res is not None:
        forced, flips, sites = _gradients_through_hip_masks(config, qs, res)
        worst, bad_forced = _strict_misses(names, got, forced)
        print('SHAPE: backward %s ReLU masks that differ: %d of %d; through the HIP masks worst error / tolerance = %.3g in %s' % (
            (tag, flips, sites) + worst))
        assert 0 < flips <= 1e-5 * sites, (flips, sites, bad)
        assert not bad_forced, bad_forced
        return
    assert not bad, bad


FRAC_OUTSIDE_STRICT = 0.3            # tests/test_gpu_train.py::test_full_size_backward_sample, bf16x3


def _check_split(tag, names, got, grads, config, qs, res):
    """the criterion and constants of tests/test_gpu_train.py::test_full_size_backward_sample for the split kernels: relative L2 per
    tensor, a loose max-abs bound, and the fraction of entries outside the strict elementwise bound (a ReLU input inside the split
    products' rounding band of zero flips its mask and moves one row of a weight gradient; everything else agrees)"""
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
    print('SHAPE: backward %s worst rel. L2 / limit = %.3g in %s; largest fraction outside 2e-4 max|g| = %.3g in %s' % (
        (tag,) + worst_l2 + worst_frac))
    if bad or not worst_frac[0] < FRAC_OUTSIDE_STRICT:
        # a miss in split mode is accepted only as what _check_strict accepts: masks differ, and through the HIP masks all is strict
        forced, flips, sites = _gradients_through_hip_masks(config, qs, res)
        worst, bad_forced = _strict_misses(names, got, forced)
        print('SHAPE: backward %s ReLU masks that differ: %d of %d; through the HIP masks worst error / tolerance = %.3g in %s' % (
            (tag, flips, sites) + worst))
        assert 0 < flips <= 1e-4 * sites, (flips, sites, bad, worst_frac)      # (test_full_size_gradients_are_strict_given_the_same_relu_masks)
        assert not bad_forced, bad_forced


# ---------------------------------------------------------------------------------------------
# 2. whole model at H = 192, 320, 384, 448, and backward at 256
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,V,L,T', [(192, 132, 40, 7), (320, 128, 64, 33), (384, 260, 8, 8), (448, 128, 100, 100)])
def test_in_between_hidden_sizes_against_oracle(H, V, L, T, matmul):
    """All 12 program forms in one batch (Conv1d and Linear(T,T) Temporal nets, T below and at max_video_length, feature sizes that
    are no multiple of 32): every question's logits against the oracle."""
    from stair_amd import ops
    config, qs, ref = _forward_reference(H, V, L, T)
    model = _model(config, 1)
    with ops.kernel_accounting() as acct:
        res = model.forward_batch(qs)
        torch.cuda.synchronize()
    _check_forward('H=%d V=%d L=%d T=%d' % (H, V, L, T), matmul, H, res, ref, acct)


@pytest.mark.parametrize('H,L,T', [(192, 40, 7), (256, 40, 33), (320, 64, 33), (384, 8, 8), (448, 100, 100)])
def test_backward_at_in_between_hidden_sizes(H, L, T, matmul):
    """Every parameter gradient of the decoder CE against autograd of the oracle.  H = 256 is the one size at which the one-pass
    LayerNorm adjoint for H = 256 runs (asserted: the launcher reports the form it chose); the other sizes take the two-kernel
    form, walking rows in a whole trip and a partial one."""
    config, qs, names, grads, per_q, logits = _backward_reference(H, 128, L, T)
    res, losses, got, acct = _train_step(config, qs)
    assert np.allclose(losses.cpu().numpy(), per_q, rtol=1e-5, atol=2e-5)
    rec, bwd = _recurrence(H // 2, matmul)
    assert rec in acct.table and bwd in acct.table, sorted(acct.table)
    ln = {'layernorm_bwd_fused_kernel', 'layernorm_bwd_kernel+param_grad'} & set(acct.table)
    assert ln == {'layernorm_bwd_fused_kernel' if H == 256 else 'layernorm_bwd_kernel+param_grad'}, sorted(acct.table)
    tag = 'H=%d L=%d T=%d %s %s' % (H, L, T, matmul, bwd)
    if matmul == 'f32':
        _check_strict(tag, names, got, grads, config, qs, res)
    else:
        _check_split(tag, names, got, grads, config, qs, res)


RAGGED_LENS = (3, 17, 40, 64)


def test_mixed_clip_lengths_training_gradients_at_h320():
    """tests/test_gpu_ragged.py's training case at H = 320 (max_video_length 64, clips of 3, 17, 40 and 64 frames in one launch
    batch): per-question losses and every parameter gradient against the oracle run on each question at its own length; exact-fp32
    products, strict elementwise bound."""
    from stair_amd import ops
    config = _config(320, 128, 64)
    qs = [synth.make_question(config, 1, i, form=synth.ALL_FORMS[i], T=RAGGED_LENS[(i // 3) % len(RAGGED_LENS)]) for i in range(12)]
    names, grads, per_q, logits = _oracle_gradients(config, qs)
    ops.set_matmul_mode('f32')
    try:
        res, losses, got, acct = _train_step(config, qs)
    finally:
        ops.set_matmul_mode('bf16x3')
    assert sorted(set(int(x) for x in res.question_frames)) == sorted(RAGGED_LENS)
    for i, lg in enumerate(logits):
        assert _maxerr(res.logits[i], lg) < 1e-4 and int(res.pred[i]) == int(torch.argmax(lg)), (qs[i]['form'], _maxerr(res.logits[i], lg))
    assert np.allclose(losses.cpu().numpy(), per_q, rtol=1e-5, atol=1e-5)
    _check_strict('H=320 L=64 T=3,17,40,64 f32 lstm_bwd_f32', names, got, grads)


# ---------------------------------------------------------------------------------------------
# 3. the README's I3D shape: V = 1024, T = 64 at full hidden size
# ---------------------------------------------------------------------------------------------
def test_i3d_shape_against_oracle(matmul):
    from stair_amd import ops
    config, qs, ref = _forward_reference(512, 1024, 64, 64)
    assert qs[0]['video_features'].shape == (64, 1024) and config['answer_vocab_length'] == 172
    model = _model(config, 1)
    with ops.kernel_accounting() as acct:
        res = model.forward_batch(qs)
        torch.cuda.synchronize()
    _check_forward('H=512 V=1024 L=64 T=64', matmul, 512, res, ref, acct)


def test_i3d_shape_on_bf16_stored_clips():
    """The same shape with the clips stored as bf16 (the plane GEMM reads them: K = 1024); the oracle is fed the same rounded values,
    so the 1e-4 bound applies unchanged (tests/test_gpu_planes.py)."""
    from stair_amd import ops
    assert ops.get_matmul_mode() == 'bf16x3'
    config, qs, ref = _forward_reference(512, 1024, 64, 64, True)
    model = _model(config, 1)
    with ops.kernel_accounting() as acct:
        res = model.forward_batch(qs)
        torch.cuda.synchronize()
    assert res._video.dtype == torch.bfloat16 and 'gemm_planes' in acct.table, sorted(acct.table)
    _check_forward('H=512 V=1024 L=64 T=64 bf16 clips', 'bf16x3', 512, res, ref, acct)


# ---------------------------------------------------------------------------------------------
# 5. frame counts up to the training limit, and beyond 128 frames forward
# ---------------------------------------------------------------------------------------------
def test_training_at_the_frame_limits():
    """T = 113 frames at max_video_length 140, one question per form (P0: `between`, P2 / C3: `after`, P5 / C1: `before`), exact-fp32 products: the largest LDS image of Superlative's backward
    kernel (P3 and C1 carry it: 161 816 of 163 840 bytes) and the largest admitted Conv1d filters (k = 35; 71 taps in the third
    layer).  Logits and every parameter gradient against the oracle at the strict bound."""
    from stair_amd import ops
    config, qs, names, grads, per_q, logits = _backward_reference(64, 128, 140, 113)
    ops.set_matmul_mode('f32')
    try:
        res, losses, got, acct = _train_step(config, qs)
    finally:
        ops.set_matmul_mode('bf16x3')
    for k in ('cosine_attn_grouped_kernel', 'cosine_attn_bwd_grouped_kernel', 'temporal_relate_bwd_kernel'):
        assert k in acct.table, (k, sorted(acct.table))
    worst = 0.0
    for i, lg in enumerate(logits):
        worst = max(worst, _maxerr(res.logits[i], lg))
        assert _maxerr(res.logits[i], lg) < 1e-4 and int(res.pred[i]) == int(torch.argmax(lg)), (qs[i]['form'], _maxerr(res.logits[i], lg))
    print('SHAPE: forward H=64 V=128 L=140 T=113 f32 lstm_rec_f32 worst error / tolerance = %.3g' % (worst / 1e-4))
    assert np.allclose(losses.cpu().numpy(), per_q, rtol=1e-5, atol=1e-5)
    _check_strict('H=64 L=140 T=113 f32 lstm_bwd_f32', names, got, grads, config, qs, res)


def test_forward_beyond_128_frames(matmul):
    """T = 141 frames at max_video_length 141 (an inference size: training plans stop at 113 frames): Superlative leaves the grouped
    kernel (T <= 128) for the per-pair cosine kernel.  All 12 forms; P3 and C1 are the Superlative ones."""
    from stair_amd import ops
    config, qs, ref = _forward_reference(64, 128, 141, 141)
    model = _model(config, 1)
    with ops.kernel_accounting() as acct:
        res = model.forward_batch(qs)
        torch.cuda.synchronize()
    assert 'cosine_attn_grouped_kernel' not in acct.table, sorted(acct.table)        # (Superlative alone launches the grouped form)
    _check_forward('H=64 V=128 L=141 T=141', matmul, 64, res, ref, acct)
