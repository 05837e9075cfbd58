"""The value-edge corpus (tests/value_edges.py) on the reference side alone, CPU: the corpus reaches its edges IN THE ORACLE, so the
GPU tests of tests/test_gpu_value_edges.py cannot pass vacuously, and the bounds those tests apply are at least four times what
fp32 rounding of the oracle itself costs -- the HIP path adds a summation order of its own on top of that rounding.

Per batch (the init weights over every program x clip regime, and one batch per weight variant) the oracle runs once in fp64 and
once in fp32 with its video encoder replaced by the identity, at the `tiny` geometry (H = 64).  Checked per node and per question:
  - the edge counts of value_edges.EdgeCounter, each > 0 in the batch that is there to produce it;
  - every value and gradient finite, every parameter gradient below 2^17 (half the fixed-point range of the deterministic sums);
  - fp32 against fp64 within a quarter of the GPU bound (nodes 2e-5 max(1, max|ref|); gradients 2e-4 of the question's largest entry,
    floor 1e-6; parameter gradients 2e-4 of the tensor's largest entry, floor 1e-3), or the (geometry, batch, quantity) is in
    value_edges.ILL_CONDITIONED with its measured ratio.  One batch has such entries: under `hasitem_sat` on the `large` clips the
    sigmoid of HasItem sits at logits near +-16, where fp32 rounds 1 - s to a few ulps and s (1 - s) with it.  The same at hidden
    size 512 at the node bound of its mode (test_fp32_oracle_lies_within_a_quarter_of_the_gpu_bounds_h512);
  - exact zeros where the construction says so: `XorFrame u u`, d_encoded where no path reaches the clip."""
import pytest
import torch

import program_cells as PC
import value_edges as VE
from oracle import nmn_oracle as O

GEOMETRY = 'tiny'

# the edges each batch is there to produce (EdgeCounter keys)
WANTED = {
    'init': ('cos_zero_rows', 'cos_small_norms', 'tie_min', 'tie_abs', 'tie_choose', 'tie_superlative', 'sigmoid_saturated'),
    'dense_const': ('layernorm_flat_rows',),
    'dense_dead': ('layernorm_flat_rows', 'dead_layers'),
    'filter_dead': ('dead_layers',),
    'beta_large': (),
    'beta_flat': ('tie_relate',),
    'relate_sat': ('sigmoid_beyond_10',),
    'hasitem_sat': ('sigmoid_saturated', 'tie_min', 'tie_abs'),
    'localize_tiny': ('cos_small_norms',),
    'localize_zero': ('cos_zero_rows',),
    'keyword_tiny': ('cos_small_norms',),
}


@pytest.fixture(scope='module', params=VE.BATCHES)
def both(request):
    return VE.oracle_pass(GEOMETRY, request.param, torch.float64), VE.oracle_pass(GEOMETRY, request.param, torch.float32)


def test_corpus_shape():
    progs = VE.programs()
    assert len(PC.SLOTS) + len(VE.EXTRA) == 57 and len(progs) == 46       # 11 slots give a program another slot gave
    assert len({tuple(p.tokens) for p in progs}) == len(progs)
    assert len(VE.cases('init')) == 46 * 8
    for b in VE.BATCHES[1:]:
        n = len(VE.cases(b))
        assert 0 < n and n % len(VE.VARIANT_CLIPS) == 0, b
    # a shared span: every `u` of a program has the span of the first
    qs = VE.questions(VE.GEOMETRIES[GEOMETRY], 'hasitem_sat')
    assert all(q['encoded'].shape == (VE.T, 64) for q in qs)
    q = [q for q in VE.questions(VE.GEOMETRIES[GEOMETRY], 'init') if 'Choose u u F1' in q['qa_id']][0]
    at = [i for i, t in enumerate(q['nmn_program_list']) if t == 'u']
    assert len(at) == 2 and q['prog_str_to_question_tokens'][at[0]] == q['prog_str_to_question_tokens'][at[1]]


def test_corpus_reaches_its_edges_in_the_oracle(both):
    f64, f32 = both
    print('%s: %d questions; edges in fp64 %s; in fp32 %s' % (f64.batch, len(f64.qs), f64.edges, f32.edges))
    for key in WANTED[f64.batch]:
        assert f64.edges[key] > 0 and f32.edges[key] > 0, (f64.batch, key, f64.edges[key], f32.edges[key])
    if f64.batch == 'beta_large':
        # beta = 200 linspace(0, 1) over max_video_length = 40 entries steps by 5.13 per frame: the softmax of Relate peaks above
        # 0.99 at one end and underflows to exact zeros in fp32 at the other (exactly one-hot it is not: exp(-5.13) = 5.9e-3)
        n = 0
        for q, steps in zip(f32.qs, f32.steps):
            for i, t in enumerate(q['nmn_program_list']):
                if t == 'Relate':
                    s = steps[i]
                    assert float(s.max()) > 0.99 and int((s == 0).sum()) > 0, q['qa_id']
                    n += 1
        assert n > 0


def test_corpus_is_finite_and_inside_the_fixed_point_range(both):
    for g in both:
        worst_dw = worst_denc = 0.0
        for k, q in enumerate(g.qs):
            assert torch.isfinite(g.logits[k]).all(), q['qa_id']
            for s in g.steps[k]:
                assert s is None or torch.isfinite(s).all(), q['qa_id']
            assert torch.isfinite(g.d_encoded[k]).all() and torch.isfinite(g.d_question[k]).all(), q['qa_id']
            worst_denc = max(worst_denc, float(g.d_encoded[k].abs().max()))
        for n, d in g.grads.items():
            if d is not None:
                assert torch.isfinite(d).all(), n
                worst_dw = max(worst_dw, float(d.abs().max()))
        print('%s %s: max |dW| = %.4g, max |d_encoded| = %.4g' % (g.batch, g.logits[0].dtype, worst_dw, worst_denc))
        assert worst_dw < VE.GRAD_LIMIT, (g.batch, worst_dw)


def test_exact_zeros_by_construction(both):
    f64, f32 = both
    n_xor = n_short = 0
    for g in both:
        for k, q in enumerate(g.qs):
            for i in VE.xor_of_equal_operands(q['nmn_program_list']):
                assert float(g.steps[k][i].abs().max()) == 0.0, (q['qa_id'], i)
                n_xor += 1
            n_short += int(q['video_len'] < VE.T)
            assert g.d_encoded[k].shape[0] == q['video_len']
    assert n_xor > 0 and (n_short > 0 or f64.batch != 'init')


def _report_and_hold(geometry, batch, ratios):
    for what, ratio in sorted(ratios.items()):
        if ratio >= 0.2:
            print('%s %s %s: oracle fp32 against fp64, error / bound %.3g' % (geometry, batch, what, ratio))
    for kind in ('logits', 'node', 'd_encoded', 'd_question', 'params'):
        print('%s %s %s: worst error / bound %.3g at %s'
              % ((geometry, batch, kind) + max(((r, k) for k, r in ratios.items() if k.startswith(kind + '@')), default=(0.0, '-'))))
    VE.hold_to_a_quarter(VE.ILL_CONDITIONED, (geometry, batch), ratios)


def test_fp32_oracle_lies_within_a_quarter_of_the_gpu_bounds(both):
    f64, f32 = both
    ratios, exact = VE.compare_passes(f64, f32, VE.NODE_TOL['f32'])
    assert not exact, exact        # where the fp64 gradient is identically zero the fp32 one is too
    _report_and_hold(GEOMETRY, f64.batch, ratios)


@pytest.mark.parametrize('batch', VE.BATCHES)
def test_fp32_oracle_lies_within_a_quarter_of_the_gpu_bounds_h512(batch):
    """The same at hidden size 512, at the node bound of its mode (1e-4).  At this width the two precisions take different sides of
    a ReLU kink now and then (tests/test_gpu_program_cells.py), so the fp32 pass is differentiated through the masks of the fp64 pass,
    as the GPU test differentiates the oracle through the HIP pass's; at most 1e-5 of the sites disagree.  About 50 s of CPU for the
    largest batch."""
    config = VE.GEOMETRIES['h512']
    masks = VE.ReluMasks()
    f64 = VE.run_oracle(config, batch, torch.float64, count=False, masks=masks)
    masks.replay = True
    f32 = VE.run_oracle(config, batch, torch.float32, count=False, masks=masks)
    print('h512 %s: %d of %d ReLU sites differ in sign between the two passes' % (batch, masks.flips, masks.sites))
    assert masks.sites > 0 and masks.flips <= 1e-5 * masks.sites
    for g in (f64, f32):
        assert all(torch.isfinite(x).all() for x in g.logits + g.d_encoded + g.d_question)
        assert all(float(d.abs().max()) < VE.GRAD_LIMIT for d in g.grads.values() if d is not None)
    ratios, exact = VE.compare_passes(f64, f32, VE.NODE_TOL['bf16x3'])
    assert not exact, exact
    _report_and_hold('h512', batch, ratios)


LSTM_NAMES = ['submodules.video_encoder.' + n + sfx for sfx in ('', '_reverse')
              for n in ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0')]


def _lstm_pass(case, dtype, scale, counts=None):
    """(outputs and final states of every sequence in one vector, {weight: gradient}) of the saturated LSTM of `case`"""
    Hh, I, lens = VE.LSTM_CASES[case]
    g = torch.Generator().manual_seed(Hh + I)
    d_outs = [torch.randn(L, 2 * Hh, generator=g, dtype=torch.float64) for L in lens]
    d_hn = torch.randn(len(lens), 2 * Hh, generator=g, dtype=torch.float64)
    w, xs = VE.saturated_lstm(Hh, I, lens, dtype, scale)
    for n in LSTM_NAMES:
        w[n].requires_grad_(True)
    orig = torch.sigmoid, torch.tanh

    def sigmoid(x):
        y = orig[0](x)
        yf = y.detach().float()
        counts['sig0'] += int((yf < 1e-7).sum()); counts['sig1'] += int((yf == 1).sum())
        counts['mid'] += int(((yf > 0.1) & (yf < 0.9)).sum())
        return y

    def tanh(x):
        y = orig[1](x)
        yf = y.detach().float()
        counts['tanh_lo'] += int((yf == -1).sum()); counts['tanh_hi'] += int((yf == 1).sum())
        return y
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        if counts is not None:
            torch.sigmoid, torch.tanh = sigmoid, tanh
        outs, loss = [], 0
        for s, x in enumerate(xs):
            ro, rh = O.lstm_bidir_explicit(w, 'video_encoder', x)
            outs.append(torch.cat([ro.detach().reshape(-1), rh.detach().reshape(-1)]))
            loss = loss + (ro * d_outs[s].to(dtype)).sum() + (rh.reshape(-1) * d_hn[s].to(dtype)).sum()
        torch.sigmoid, torch.tanh = orig
        loss.backward()
    finally:
        torch.sigmoid, torch.tanh = orig
        torch.set_num_threads(threads)
    return torch.cat(outs).double(), {n: w[n].grad.double() for n in LSTM_NAMES}


@pytest.mark.parametrize('mode', list(VE.LSTM_INPUT_SCALE))
@pytest.mark.parametrize('case', list(VE.LSTM_CASES))
def test_saturated_lstm_saturates_and_fp32_lies_within_a_quarter(case, mode):
    """value_edges.saturated_lstm at the input scale of each matmul mode: gates below 1e-7 and at exactly 1.0 and tanh at exactly +-1.0 in fp32,
    and units in the linear range between (counted inside the oracle).  The oracle in fp32 lies within a quarter of the bounds
    tests/test_gpu_value_edges.py applies to the kernels in that mode -- outputs 2e-5 / 1e-4, weight gradients 2e-4 of max(1, largest
    entry) -- or the (case, mode, quantity) is in value_edges.LSTM_ILL_CONDITIONED with the difference measured here."""
    counts = dict(sig0=0, sig1=0, tanh_lo=0, tanh_hi=0, mid=0)
    scale = VE.LSTM_INPUT_SCALE[mode]
    ref = _lstm_pass(case, torch.float64, scale)
    out, grads = _lstm_pass(case, torch.float32, scale, counts)
    print('saturated lstm %s x %g: %s' % (case, scale, counts))
    assert all(v > 0 for v in counts.values()), counts
    assert torch.isfinite(ref[0]).all() and all(torch.isfinite(g).all() for g in ref[1].values())
    rows = [('out', float((out - ref[0]).abs().max()), 2e-5 if mode == 'f32' else 1e-4)]
    rows += [(n, float((grads[n] - ref[1][n]).abs().max()), 2e-4 * max(1.0, float(ref[1][n].abs().max()))) for n in LSTM_NAMES]
    for what, err, bound in rows:
        print('saturated lstm %s %s %s: oracle fp32 against fp64 %.3g = %.3g of the bound' % (case, mode, what, err, err / bound))
    VE.hold_to_a_quarter(VE.LSTM_ILL_CONDITIONED, (case, mode), {what: err / bound for what, err, bound in rows})
