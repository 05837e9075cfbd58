"""GPU tests of the value-edge corpus (tests/value_edges.py): the kernels at the VALUES random initialisation never produces -- norms
under the cosine clamp, exact ties, saturated sigmoids / tanhs / softmaxes, zero-variance LayerNorm rows, dead ReLU layers, logit
rows of -inf and NaN.  tests/test_value_edges_host.py shows on the CPU that the corpus reaches each of these in the oracle and that
the bounds applied here are at least four times the oracle's own fp32 rounding.

Plan level, per batch of the corpus (the clip ENCODINGS are the caller's own, VideoNMN's `encoded=` route, so `video` holds exactly
the crafted rows; the video encoder is frozen, as that route demands), with cse=True and cse=False:
  (a) logits, top-1 and EVERY module node against the fp64 oracle: tol max(1, max|ref|), tol 2e-5 in f32 mode, 1e-4 in bf16x3;
  (b) d_encoded and d_question question by question (2e-4 of the question's largest entry, floor 1e-6) and the parameter gradients
      (2e-4 of the tensor's largest entry, floor 1e-3) of the custom loss of tests/test_gpu_autograd.py; the quantities of
      value_edges.ILL_CONDITIONED -- single questions, nodes and tensors -- get 4 x the difference listed there for the oracle in
      fp32 against the oracle in fp64;
  (c) nothing non-finite anywhere (the oracle is finite everywhere: host test);
  (d) exact zeros where the fp64 oracle is zero by construction: XorFrame of two equal operands, every gradient the oracle has
      identically zero (behind a dead layer, behind |a - a|, a clip no path reads), d_encoded of the frames >= video_len;
  (e) cse=True and cse=False bit-equal in logits and every node.
Geometry `tiny` (H = 64, f32 mode): the launch-per-layer row kernels.  Geometry `h512` (bf16x3): the fused tile tails and the
backward chains; there the oracle differentiates through the HIP pass's ReLU masks (helpers._ForcedMasks) under the three flip
conditions of tests/test_gpu_program_cells.py.

Building blocks through the C ABI against fp64 autograd on the same edges: cosine attention forward / backward with zero rows and
rows of norm 1e-9, the Temporal relate nets on all-0 / all-1 / one-hot attentions with a last layer x 50, the sigmoid epilogue of
both GEMMs at |x| up to 1e4, cosine top-k on zero and duplicate rows, the LSTM recurrences with every gate saturated on some units.

argmax: the plan's answer index against torch.argmax on rows with ties, -inf and NaN (set through the decoder's bias).

Kernels this file made change (csrc/):
  argmax_kernel (rowops.hip)                  a row of -inf, a row of NaN: index 0x7fffffff instead of 0; a NaN in a row: skipped
                                              instead of chosen.  Now a NaN beats everything and the first index wins.
  cosine_attn_bwd_kernel (rowops_bwd.hip)     0 < ||f|| < 1e-8 (the `tiny` clips under ExistsFrame; test_cosine_attn_under_the_clamp_
                                              matches_autograd, rows of norm 1e-9): the kernel subtracted cos f / nf^2 (and cos k /
                                              nk^2) with the CLAMPED norm, a term autograd of clamp_min does not have: dF = dcos k^ /
                                              eps alone.  With f = 0 the two coincide, which is why zero rows never showed it.
  cosine_attn_bwd_grouped_kernel              the same term, in Localize / Superlative.  Both sides of that cosine come out of Linear
  (rowops_bwd.hip)                            layers, so only the batches `localize_tiny` (every frame row 1e-10) and `keyword_tiny`
                                              (every keyword row 1e-10) reach it, on both geometries (MFMA form and scalar form).
"""
import functools

import numpy as np
import pytest
import torch

import value_edges as VE
from helpers import _ForcedMasks, oracle_weights
from oracle import nmn_oracle as O
from stair_amd import spec, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MAP_LEVEL = ('Filter', 'FilterFrame', 'HasItem', 'Localize', 'Superlative', 'Temporal')     # each saves a [frames, H] ReLU mask


@pytest.fixture
def f32():
    from stair_amd import ops
    ops.set_matmul_mode('f32')
    yield 'f32'
    ops.set_matmul_mode('bf16x3')


@pytest.fixture(params=['f32', 'bf16x3'])
def matmul(request):
    from stair_amd import ops
    ops.set_matmul_mode(request.param)
    yield request.param
    ops.set_matmul_mode('bf16x3')


# ---- the HIP side --------------------------------------------------------------------------------------------------------------
def _model(config, batch):
    from stair_amd.module_net import VideoNMN
    w = VE.weights(config, batch)
    m = VideoNMN(config)
    m.load_state_dict({k: torch.from_numpy(w[k].copy()) for k in spec.state_dict_keys(config)})
    m = m.to(DEV)
    for n, p in m.named_parameters():           # a pass on caller-made encodings has no video encoder to train
        if '.video_encoder.' in n:
            p.requires_grad_(False)
    return m


@functools.lru_cache(maxsize=None)
def _inputs(geometry, batch):
    qs = VE.questions(VE.GEOMETRIES[geometry], batch)
    enc = torch.from_numpy(np.stack([q['encoded'] for q in qs])).to(DEV).contiguous()
    question = torch.cat([torch.as_tensor(q['question']) for q in qs]).to(DEV).contiguous()
    return ([q['nmn_program_list'] for q in qs], [q['prog_str_to_question_tokens'] for q in qs], enc, question,
            [q['question'].shape[0] for q in qs], [q['video_len'] for q in qs])


def _run(model, geometry, batch, train, cse):
    progs, spans, enc, question, q_lens, lens = _inputs(geometry, batch)
    n = len(progs)
    src = model._clip_source(n, None, np.arange(n), lens, None, enc, train, None)
    return model._run(src, progs, spans, question, q_lens, train, None, None, cse)


def _train_pass(model, geometry, batch, R, cse=True):
    """One training pass with the custom loss: (result, d_encoded [n, T, H], d_question, {parameter: gradient}), on the host"""
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    res = _run(model, geometry, batch, True, cse)
    assert list(res.clip_rows) == list(range(res.info.n_questions))
    lg = res.logits.clone().requires_grad_(True)
    VE.custom_loss(lg, R.to(DEV)).backward()
    de = torch.full(res._enc.shape, float('nan'), dtype=torch.float32, device=DEV)        # both are OVERWRITTEN by the pass
    dq = torch.full(res._question.shape, float('nan'), dtype=torch.float32, device=DEV)
    res.backward_dlogits(lg.grad.contiguous(), d_question=dq, d_encoded=de)
    res.check()
    return res, de.cpu(), dq.cpu(), {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters()}


def _fit(got, ref):
    """a node's value cut to the frames of the question's clip (a ragged batch pads every [T, H] map and [.., T] row to the longest)"""
    got = got.detach().float().cpu()
    if got.shape != ref.shape:
        got = got[:ref.shape[0]] if ref.dim() == 2 and got.shape[-1] == ref.shape[-1] else got[..., :ref.shape[-1]]
    return got


def _nodes(res, g):
    return [[res.node(q, i).detach().cpu().clone() if s is not None else None for i, s in enumerate(steps)] for q, steps in enumerate(g.steps)]


def _check_forward(res, g, geometry, tol):
    """(a), (c), (d): logits, top-1 and every module node of every question against the oracle; returns (nodes compared, failures)"""
    logits, pred = res.logits.cpu(), res.pred.cpu()
    A = g.config['answer_vocab_length']
    assert torch.isfinite(logits).all() and bool(((pred >= 0) & (pred < A)).all())
    worst, fails, n_nodes, n_xor = {}, [], 0, 0
    for k, q in enumerate(g.qs):
        regime, prog = VE.regime_of(q), q['nmn_program_list']
        err, bound = VE.node_err(logits[k], g.logits[k], tol)
        bound *= VE.widen(geometry, g.batch, 'logits@' + q['qa_id'])
        worst[regime] = max(worst.get(regime, (0.0, '')), (err / bound, '%s logits' % q['qa_id']))
        if not err < bound:
            fails.append((q['qa_id'], 'logits', err, bound))
        top = torch.topk(g.logits[k], 2).values
        if float(top[0] - top[1]) > bound:
            assert int(pred[k]) == int(torch.argmax(g.logits[k])), q['qa_id']
        assert res.levels(k) == O.module_levels(prog), q['qa_id']
        zero = set(VE.xor_of_equal_operands(prog))
        for i, ref in enumerate(g.steps[k]):
            if ref is None or prog[i] not in O.ARITY:
                continue
            got = _fit(res.node(k, i), ref)
            assert got.shape == ref.shape, (q['qa_id'], i, got.shape, ref.shape)
            assert torch.isfinite(got).all(), (q['qa_id'], i, prog[i])
            if i in zero:
                assert float(got.abs().max()) == 0.0, (q['qa_id'], i, 'XorFrame of equal operands must be an exact zero')
                n_xor += 1
            err, bound = VE.node_err(got, ref, tol)
            bound *= VE.widen(geometry, g.batch, 'node@%s@%d' % (q['qa_id'], i))
            worst[regime] = max(worst[regime], (err / bound, '%s node %d %s' % (q['qa_id'], i, prog[i])))
            if not err < bound:
                fails.append((q['qa_id'], i, prog[i], err, bound))
            n_nodes += 1
    for regime, (ratio, where) in worst.items():
        print('%s %s, %s clips: forward, worst error / bound %.3g at %s' % (geometry, g.batch, regime, ratio, where))
    print('%s %s: %d questions, %d module nodes compared, %d exact-zero XorFrame nodes' % (geometry, g.batch, len(g.qs), n_nodes, n_xor))
    assert n_nodes == sum(t in O.ARITY for q in g.qs for t in q['nmn_program_list'])
    return n_nodes, fails


def _check_input_gradients(g, geometry, de, dq):
    """(b), (c), (d): d_encoded and d_question question by question; returns (gradient tensors compared, failures)"""
    worst, fails, n, n_zero, off = {}, [], 0, 0, 0
    for k, q in enumerate(g.qs):
        regime, f, rows = VE.regime_of(q), q['video_len'], q['question'].shape[0]
        assert torch.count_nonzero(de[k, f:]) == 0, (q['qa_id'], 'd_encoded behind the clip\'s frames')
        for what, got, ref in (('d_encoded', de[k, :f], g.d_encoded[k]), ('d_question', dq[off:off + rows], g.d_question[k])):
            assert torch.isfinite(got).all(), (q['qa_id'], what)
            err, bound = VE.grad_err(got, ref)
            if bound == 0.0:
                assert err == 0.0, (q['qa_id'], what, 'the oracle\'s gradient is identically zero: exact zeros', err)
                n_zero += 1
            else:
                bound *= VE.widen(geometry, g.batch, '%s@%s' % (what, q['qa_id']))
                worst[regime] = max(worst.get(regime, (0.0, '')), (err / bound, '%s %s' % (q['qa_id'], what)))
                if not err < bound:
                    fails.append((q['qa_id'], what, err, bound))
            n += 1
        off += rows
    for regime, (ratio, where) in worst.items():
        print('%s %s, %s clips: input gradients, worst error / bound %.3g at %s' % (geometry, g.batch, regime, ratio, where))
    print('%s %s: %d input gradient tensors compared, %d of them identically zero' % (geometry, g.batch, n, n_zero))
    return n, fails


def _check_param_gradients(g, geometry, grads, by_family=False):
    """(b), (c), (d): the parameter gradients summed over the batch.  by_family: the rule of test_gpu_program_cells.py for tensors of
    fewer than 64 elements at hidden size 512 (2e-4 of the largest entry of the layers of one net)."""
    family_max = {}
    for n in g.names:
        if g.grads[n] is not None:
            fam = n.rsplit('.', 2)[0]
            family_max[fam] = max(family_max.get(fam, 0.0), float(g.grads[n].abs().max()))
    worst, count, fails = (0.0, ''), 0, []
    for n in g.names:
        ref, got = g.grads[n], grads[n].float()
        assert torch.isfinite(got).all(), n
        if ref is None or float(ref.abs().max()) == 0.0:
            assert float(got.abs().max()) == 0.0, (g.batch, n, 'no question reaches it, or only through a dead layer: exact zeros')
            continue
        scale = family_max[n.rsplit('.', 2)[0]] if by_family and ref.numel() < 64 else float(ref.abs().max())
        bound = VE.REL * max(scale, 1e-3) * VE.widen(geometry, g.batch, 'params@' + n)
        err = float((got.double() - ref.double()).abs().max())
        worst = max(worst, (err / bound, n))
        if not err < bound:
            fails.append((n, err, bound))
        count += 1
    print('%s %s: %d parameter gradients compared, worst error / bound %.3g at %s' % ((geometry, g.batch, count) + worst))
    return count, fails


def _check_cse_bit_equal(runs, g):
    """(e)"""
    assert torch.equal(runs[True][0], runs[False][0]), (g.batch, 'logits')
    n = 0
    for q, (a, b) in enumerate(zip(runs[True][1], runs[False][1])):
        for i, (x, y) in enumerate(zip(a, b)):
            if x is not None:
                assert torch.equal(x, y), (g.qs[q]['qa_id'], i)
                n += 1
    assert n > 0


# ---- plan level, H = 64: the row kernels ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('batch', VE.BATCHES)
def test_plan_on_value_edges_matches_oracle_tiny(batch, f32):
    g = VE.oracle_pass('tiny', batch)
    runs = {}
    for cse in (True, False):
        model = _model(g.config, batch)
        res, de, dq, grads = _train_pass(model, 'tiny', batch, g.R, cse=cse)
        assert res.info.n_questions == len(g.qs)
        runs[cse] = (res.logits.cpu().clone(), _nodes(res, g))
        (n_nodes, f1), (n_in, f2), (n_par, f3) = (_check_forward(res, g, 'tiny', VE.NODE_TOL['f32']),
                                                  _check_input_gradients(g, 'tiny', de, dq), _check_param_gradients(g, 'tiny', grads))
        print('tiny %s cse=%s: %d nodes and %d gradient tensors compared' % (batch, cse, n_nodes, n_in + n_par))
        assert not f1 + f2 + f3, f1 + f2 + f3
        del res
    _check_cse_bit_equal(runs, g)


# ---- plan level, H = 512, default product mode: the fused tile tails, under the HIP pass's ReLU masks ---------------------------------
@functools.lru_cache(maxsize=None)
def _masked(batch):
    """The fp64 oracle of a batch at hidden size 512, every question differentiated through the ReLU masks of the HIP pass (read from
    a fresh forward run of the training plan, before any backward pass touches its workspace); forward values are the oracle's own.
    g.hip_logits: the logits of the run the masks were read from; g.sites, g.flips, g.flip_reach as in test_gpu_program_cells.py."""
    from stair_amd import ops
    assert ops.get_matmul_mode() == 'bf16x3'
    config = VE.GEOMETRIES['h512']
    res = _run(_model(config, batch), 'h512', batch, True, True)
    stats = dict(sites=0, flips=0, reach=(0.0, ''))

    def forward(k, w, d):
        fm = _ForcedMasks(res, k, d['nmn_program_list'])
        r = fm.forward(w, config, d, return_res_by_step=False, return_result_of_each_step=True, explicit_lstm=True)
        stats['sites'] += fm.sites
        stats['flips'] += fm.flips
        stats['reach'] = max(stats['reach'], (fm.flip_reach, d['qa_id']))
        return r
    g = VE.run_oracle(config, batch, torch.float64, forward=forward, count=False)
    g.hip_logits = res.logits.cpu().clone()
    g.sites, g.flips, g.flip_reach = stats['sites'], stats['flips'], stats['reach']
    return g


@pytest.mark.parametrize('batch', VE.BATCHES)
def test_plan_on_value_edges_matches_oracle_h512(batch):
    from stair_amd import ops
    g = _masked(batch)
    # the conditions under which a comparison under forced masks means anything (test_gpu_program_cells.py)
    floor = sum(q['video_len'] * 512 * sum(t in MAP_LEVEL for t in q['nmn_program_list']) for q in g.qs)
    print('h512 %s: %d ReLU sites (at least %d wanted), %d flips, largest |pre-activation| / bound at a flip %.3g (%s)'
          % (batch, g.sites, floor, g.flips, g.flip_reach[0] / 1e-4, g.flip_reach[1]))
    assert g.sites >= floor > 0
    assert g.flips < 1e-4 * g.sites
    assert g.flip_reach[0] < 1e-4, g.flip_reach
    runs = {}
    for cse in (True, False):
        model = _model(g.config, batch)
        with ops.kernel_accounting() as acct:
            res, de, dq, grads = _train_pass(model, 'h512', batch, g.R, cse=cse)
        assert 'tile_mlp' in acct.table and 'vec_group' in acct.table, sorted(acct.table)
        assert torch.equal(res.logits.cpu(), g.hip_logits), 'this pass is not the pass the masks were read from'
        runs[cse] = (res.logits.cpu().clone(), _nodes(res, g))
        (n_nodes, f1), (n_in, f2), (n_par, f3) = (_check_forward(res, g, 'h512', VE.NODE_TOL['bf16x3']), _check_input_gradients(g, 'h512', de, dq),
                                                  _check_param_gradients(g, 'h512', grads, by_family=True))
        print('h512 %s cse=%s: %d nodes and %d gradient tensors compared' % (batch, cse, n_nodes, n_in + n_par))
        assert not f1 + f2 + f3, f1 + f2 + f3
        del res
    _check_cse_bit_equal(runs, g)


# ---- argmax ------------------------------------------------------------------------------------------------------------------------
def _logit_rows(A):
    inf, nan = float('inf'), float('nan')
    base = torch.linspace(-1, 1, A)
    rows = {'tie of the two largest': base.clone(), 'all equal': torch.full((A,), 0.25), 'all -inf': torch.full((A,), -inf),
            'one NaN': base.clone(), 'all NaN': torch.full((A,), nan), '-inf but one': torch.full((A,), -inf),
            'two NaN': base.clone(), 'NaN before the maximum': base.clone()}
    rows['tie of the two largest'][[3, A - 2]] = 5.0
    rows['one NaN'][A // 2] = nan
    rows['-inf but one'][A - 1] = -3.0
    rows['two NaN'][[A - 1, 5]] = nan
    rows['NaN before the maximum'][1] = nan
    rows['NaN before the maximum'][A - 3] = 9.0
    return rows


@pytest.mark.parametrize('A', [16, 200])
def test_argmax_equals_torch_on_ties_inf_and_nan(A, f32):
    """stair_plan_run's answer index (argmax_kernel) on logit rows no random weights produce.  The ABI takes no logits, so the rows
    are set through the decoder: decoder.3.weight = 0 and decoder.3.bias = the row make every question's logits that row (0 * h +
    b); the logits are read back and `pred` must equal torch.argmax of what was read, and lie in [0, A).  A = 200: more classes than
    lanes.  Before the fix a row of -inf or of NaN gave 0x7fffffff and a NaN inside a row was skipped."""
    config = dict(VE.GEOMETRIES['tiny'], answer_vocab_length=A)
    from stair_amd.module_net import VideoNMN
    w = synth.make_weights(config, 0)
    model = VideoNMN(config)
    model.load_state_dict({k: torch.from_numpy(w[k].copy()) for k in spec.state_dict_keys(config)})
    model = model.to(DEV)
    qs = [synth.make_question(config, 0, i, form=synth.ALL_FORMS[i], T=24) for i in range(3)]
    video = torch.stack([torch.as_tensor(q['video_features']) for q in qs]).to(DEV).contiguous()
    question = torch.cat([torch.as_tensor(q['question']) for q in qs]).to(DEV).contiguous()
    args = ([q['nmn_program_list'] for q in qs], [q['prog_str_to_question_tokens'] for q in qs], video, question,
            [q['question'].shape[0] for q in qs])
    sd = dict(model.named_parameters())
    with torch.no_grad():
        sd['submodules.decoder.3.weight'].zero_()
    for name, row in _logit_rows(A).items():
        with torch.no_grad():
            sd['submodules.decoder.3.bias'].copy_(row)
        res = model.run_programs(*args)
        logits, pred = res.logits.cpu(), res.pred.cpu()
        for k in range(len(qs)):
            assert torch.equal(torch.nan_to_num(logits[k], nan=1e30), torch.nan_to_num(row, nan=1e30)), (name, 'the crafted row did not arrive')
            assert 0 <= int(pred[k]) < A, (name, int(pred[k]))
            assert int(pred[k]) == int(torch.argmax(logits[k])), (name, int(pred[k]), int(torch.argmax(logits[k])))


# ---- building blocks -------------------------------------------------------------------------------------------------------------
SHAPES = [(3, 8, 64), (3, 33, 192), (4, 64, 512)]


def _cosine_case(G, T, H, case):
    """F [G, T, H], K [6, H] in float32 with the case's edge rows, 5 pairs that reach every edge row, d_att"""
    g = torch.Generator().manual_seed(G + T + H)
    F = torch.randn(G, T, H, generator=g)
    K = torch.randn(6, H, generator=g)
    d_att = torch.randn(5, T, generator=g, dtype=torch.float64)
    if case in ('zero_f', 'all'):
        F[0, 0] = 0
        F[G - 1, T - 1] = 0
        F[1, 2:5] = 0
    if case in ('zero_k', 'all'):
        K[0] = 0
    if case in ('tiny', 'all'):                 # norm 1e-9: under the 1e-8 clamp, not zero
        F[0, 1] *= 1e-9 / F[0, 1].norm()
        F[G - 1, T - 2] *= 1e-9 / F[G - 1, T - 2].norm()
        K[1] *= 1e-9 / K[1].norm()
    f_idx = torch.tensor([0, G - 1, 1, 0, G - 1], dtype=torch.int32)
    k_idx = torch.tensor([0, 1, 2, 1, 0], dtype=torch.int32)         # tiles and rows are shared by pairs
    return F, K, f_idx, k_idx, d_att


@pytest.mark.parametrize('case', ['zero_f', 'zero_k', 'tiny', 'all'])
@pytest.mark.parametrize('G,T,H', SHAPES)
def test_cosine_attn_under_the_clamp_matches_autograd(G, T, H, case):
    """stair_cosine_attn_fwd / _bwd where the 1e-8 clamp of nn.CosineSimilarity is active, against fp64 autograd of the oracle's
    operator (clamp_min: the clamped norm is a constant, dF = dcos k^ / eps).  Bounds of test_cosine_attn_backward_matches_autograd:
    1e-5 forward, 2e-5 of the largest gradient entry backward -- gradients behind the clamp are ~1e8 and the bound scales with them.
    Before the fix cosine_attn_bwd_kernel failed `tiny` and `all`: it kept the -cos f / nf^2 term with nf = eps (1e-2 relative)."""
    from stair_amd import ops
    F32, K32, f_idx, k_idx, d_att = _cosine_case(G, T, H, case)
    F, K = F32.double().requires_grad_(True), K32.double().requires_grad_(True)
    att = torch.stack([O.op_existsframe(K[int(k_idx[p])], F[int(f_idx[p])]).reshape(T) for p in range(5)])
    (att * d_att).sum().backward()
    assert torch.isfinite(F.grad).all() and torch.isfinite(K.grad).all()
    norms = torch.cat([F32.reshape(-1, H).norm(dim=1), K32.norm(dim=1)])
    assert int((norms < 1e-8).sum()) > 0
    d = lambda t: t.detach().float().to(DEV)
    got = ops.cosine_attn(d(F), f_idx.to(DEV), d(K), k_idx.to(DEV), 5, T, H)
    assert torch.isfinite(got).all()
    assert float((got.cpu().double() - att.detach()).abs().max()) < 1e-5
    dF, dK = ops.cosine_attn_bwd(d(F), f_idx.to(DEV), d(K), k_idx.to(DEV), d(d_att), 5, T, H)
    for what, a, ref in (('dF', dF, F.grad), ('dK', dK, K.grad)):
        assert torch.isfinite(a).all(), what
        scale = max(1.0, float(ref.abs().max()))
        err = float((a.cpu().double() - ref).abs().max())
        print('cosine_attn %s (%d, %d, %d) %s: error / bound %.3g, largest entry %.3g' % (case, G, T, H, what, err / (2e-5 * scale), scale))
        assert err < 2e-5 * scale, (what, err, scale)


@pytest.mark.parametrize('mode', ['while', 'before', 'after', 'between'])
@pytest.mark.parametrize('T,conv', [(64, True), (24, True), (8, False)])
def test_temporal_relate_saturated_matches_autograd(mode, T, conv):
    """stair_temporal_relate_fwd / _bwd with the last layer x 50 (a saturated sigmoid_acc) on attentions that are all 0, all 1 and
    one-hot, against fp64 autograd of the oracle's relate nets; bounds of test_temporal_relate_backward_matches_autograd."""
    from stair_amd import ops
    config = dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, max_video_length=T if not conv else 64)
    w = {k: (v.double() if 'Temporal.relate' in k else v) for k, v in oracle_weights(config, seed=3).items()}
    for m in VE.RELATE_MODES:
        for p in ('weight', 'bias'):
            w['submodules.Temporal.relate.%s.4.%s' % (m, p)] = w['submodules.Temporal.relate.%s.4.%s' % (m, p)] * 50
    w = {k: (v.requires_grad_(True) if 'Temporal.relate' in k else v) for k, v in w.items()}
    g = torch.Generator().manual_seed(T)
    n, Ks = 5, [1, 2, 1, 2, 2]
    rows = sum(Ks)
    att = torch.zeros(rows, T, dtype=torch.float64)
    att[1:3] = 1.0                  # instance 1: both rows all 1 (mean 1)
    att[3, T // 2] = 1.0            # instance 2: one-hot
    att[4, 0] = 1.0                 # instance 3: two one-hot rows, mean of two spikes of 0.5 at either end
    att[5, T - 1] = 1.0
    att[6] = 1.0                    # instance 4: all 1 and all 0, mean 0.5 everywhere
    att.requires_grad_(True)
    d_out = torch.randn(n, T, generator=g, dtype=torch.float64)
    starts = np.concatenate([[0], np.cumsum(Ks)])[:-1]
    outs = [O.temporal_relate(w, mode, att[int(starts[i]): int(starts[i]) + Ks[i]].mean(dim=0)) for i in range(n)]
    (torch.stack(outs) * d_out).sum().backward()
    modes = {'while': 0, 'before': 1, 'after': 2, 'between': 3}
    names = ['submodules.Temporal.relate.%s.%d.%s' % (mode, l, p) for l in (0, 2, 4) for p in ('weight', 'bias')] if mode != 'while' else None
    w6 = [w[nm].detach().float().reshape(-1 if conv and nm.endswith('weight') else w[nm].shape).contiguous().to(DEV) for nm in names] if names else [None] * 6
    d = lambda t: t.detach().float().to(DEV)
    att_idx = torch.tensor(starts, dtype=torch.int32, device=DEV)
    att_k = torch.tensor(Ks, dtype=torch.int32, device=DEV)
    ksize = int(w['submodules.Temporal.relate.before.0.weight'].numel()) if conv else 0
    got = ops.temporal_relate(d(att), att_idx, att_k, n, T, modes[mode], conv, ksize, w6)
    ref = torch.stack(outs).detach()
    assert torch.isfinite(got).all()
    assert float((got.cpu().double() - ref).abs().max()) < 1e-5
    d_att, dws = ops.temporal_relate_bwd(d(att), att_idx, att_k, d(d_out), n, T, modes[mode], conv, ksize, w6)
    assert torch.isfinite(d_att).all()
    assert float((d_att.cpu().double() - att.grad).abs().max()) < 2e-5 * max(1.0, float(att.grad.abs().max()))
    if names:
        for nm, dw in zip(names, dws):
            r = w[nm].grad.reshape(dw.shape)
            assert torch.isfinite(dw).all(), nm
            assert float((dw.cpu().double() - r).abs().max()) < 2e-5 * max(1.0, float(r.abs().max())), nm


def _saturating_rows(M, K):
    """x [M, K] whose entries walk through +-{0, 0.5, 20, 100, 1e4}: with an identity weight the GEMM's pre-activations are these"""
    vals = torch.tensor([0.0, 0.5, -0.5, 20.0, -20.0, 100.0, -100.0, 1e4, -1e4, 16.0, -17.0, 88.0, -88.5, 104.0, -104.0, 3.0])
    return vals[(torch.arange(M)[:, None] * 5 + torch.arange(K)[None, :]) % len(vals)].contiguous()


@pytest.mark.parametrize('planes', [False, True])
def test_gemm_sigmoid_epilogue_saturated(planes):
    """act = 2 of stair_gemm_f32 and stair_gemm_planes (sigmoid_acc) at |x| in {20, 100, 1e4} and at the points where exp(-x)
    overflows: finite, inside [0, 1], and within 2e-6 of the fp64 sigmoid -- the output is at most 1 and an expf and a division of a few
    ulp each (2^-23) cannot cost more; the pre-activations are exact (identity weight, zero bias but for one column)."""
    from stair_amd import ops
    M, N, K = 256, 256, 64
    x = _saturating_rows(M, K)
    w = torch.zeros(N, K)
    w[torch.arange(N), torch.arange(N) % K] = 1.0
    b = torch.zeros(N)
    b[7] = 0.25
    if planes:
        x_hi, x_lo = ops.split_planes(x.to(DEV))
        w_hi, w_lo = ops.split_planes(w.to(DEV))
        y = ops.gemm_planes(x_hi, x_lo, w_hi, w_lo, b.to(DEV), 'sigmoid')
    else:
        y = ops.linear(x.to(DEV), w.to(DEV), b.to(DEV), act='sigmoid')
    pre = x.double()[:, torch.arange(N) % K] + b.double()
    ref = torch.sigmoid(pre)
    y = y.cpu()
    assert torch.isfinite(y).all() and float(y.min()) >= 0.0 and float(y.max()) <= 1.0
    assert float((y.double() - ref).abs().max()) < 2e-6
    assert bool((y[pre >= 20] > 0.999999).all()) and bool((y[pre <= -104] == 0).all()) and bool((y[pre >= 100] == 1).all())


@pytest.mark.parametrize('n,C,H,k', [(6, 70, 96, 10), (6, 214, 512, 10)])
def test_cosine_topk_zero_and_duplicate_rows(n, C, H, k):
    """stair_cosine_topk with a zero query (every similarity 0 through the clamp: the first k candidates in order), zero keys and
    groups of duplicate keys: similarities within 2e-6 of fp64 (test_cosine_topk_matches_torch's bound), best first, and equal
    similarities keep the lower index, as the header says."""
    from stair_amd import ops
    g = torch.Generator().manual_seed(C + H)
    rows = torch.randn(n, H, generator=g)
    keys = torch.randn(C, H, generator=g)
    rows[0] = 0
    rows[1] *= 1e-9 / rows[1].norm()
    dup = [(2, 9, 40), (3, C - 1)]
    for grp in dup:
        for j in grp[1:]:
            keys[j] = keys[grp[0]]
    keys[[5, 6, 30]] = 0
    keys[7] *= 1e-9 / keys[7].norm()
    rows[2] = keys[2]                           # the duplicates of key 2 are this query's best, at similarity 1
    idx, sim = ops.cosine_topk(rows.to(DEV), keys.to(DEV), k)
    idx, sim = idx.cpu().long(), sim.cpu().double()
    ref = O.cos_rows(rows.double().unsqueeze(1), keys.double().unsqueeze(0))
    assert torch.isfinite(sim).all()
    assert idx[0].tolist() == list(range(k)) and float(sim[0].abs().max()) == 0.0
    assert idx[2, :3].tolist() == [2, 9, 40]
    assert float((sim - ref.gather(1, idx)).abs().max()) < 2e-6
    assert float((sim - torch.sort(ref, dim=1, descending=True).values[:, :k]).abs().max()) < 2e-6
    assert bool((sim[:, :-1] >= sim[:, 1:]).all())
    for r in range(n):
        row = idx[r].tolist()
        assert len(set(row)) == k and all(0 <= c < C for c in row)
        for a, b2 in zip(range(k - 1), range(1, k)):
            if float(sim[r, a]) == float(sim[r, b2]):
                assert row[a] < row[b2], (r, row)
        for grp in dup:                           # of a group of duplicates the lower indices come first
            pos = [row.index(j) for j in grp if j in row]
            assert pos == sorted(pos) and [j in row for j in grp] == sorted([j in row for j in grp], reverse=True), (r, row)


LSTM_NAMES = ['submodules.video_encoder.' + n + sfx for sfx in ('', '_reverse')
              for n in ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0')]
LSTM_CASES = VE.LSTM_CASES


@functools.lru_cache(maxsize=None)
def _lstm_case(name, mode):
    """A saturated bidirectional LSTM in fp64 (value_edges.saturated_lstm) with its outputs and, for a random d_out / d_hn, the
    gradients of its weights: computed once; nobody writes to it"""
    Hh, I, lens = LSTM_CASES[name]
    w, xs = VE.saturated_lstm(Hh, I, lens, torch.float64, VE.LSTM_INPUT_SCALE[mode])
    for n in LSTM_NAMES:
        w[n].requires_grad_(True)
    g = torch.Generator().manual_seed(Hh + I)
    d_outs = [torch.randn(L, 2 * Hh, generator=g, dtype=torch.float64) for L in lens]
    d_hn = torch.randn(len(lens), 2 * Hh, generator=g, dtype=torch.float64)
    outs, loss = [], 0
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        for s, x in enumerate(xs):
            ro, rh = O.lstm_bidir_explicit(w, 'video_encoder', x)
            outs.append((ro.detach(), rh.detach().reshape(-1)))
            loss = loss + (ro * d_outs[s]).sum() + (rh.reshape(-1) * d_hn[s]).sum()
        loss.backward()
    finally:
        torch.set_num_threads(threads)
    return w, xs, d_outs, d_hn, outs


@pytest.mark.parametrize('name,coop', [('Hh32', True), ('Hh256', True), ('Hh256', False)])
def test_lstm_with_saturated_gates_matches_oracle(name, coop, matmul):
    """stair_lstm_bidir_fwd / _bwd (sigmoid_fast, tanh_fast: v_exp_f32 + v_rcp_f32) with b_ih shifted by +-20, so that every gate sits
    at 0 or 1 and g at +-1 on some units, and inputs x 30 (f32 mode) or x 3 (bf16x3 mode, whose products would not fit its bound at
    pre-activations of +-40: value_edges.LSTM_INPUT_SCALE), against the written-out oracle LSTM in fp64 and its autograd.  Bounds of
    test_lstm_matches_explicit_oracle (2e-5 in f32 mode, 1e-4 in bf16x3) and test_lstm_backward_matches_autograd_of_oracle (2e-4 of
    max(1, largest entry)).  tests/test_value_edges_host.py holds the oracle in fp32 to a quarter of them; the one quantity that is
    not -- the outputs at Hh = 256 in f32 mode, 0.27 -- gets 4 x the listed figure (value_edges.LSTM_ILL_CONDITIONED).  Hh = 256 on
    the cooperative and on the one-workgroup kernels."""
    from stair_amd import ops
    Hh, I, lens = LSTM_CASES[name]
    w, xs, d_outs, d_hn, outs = _lstm_case(name, matmul)
    off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32).to(DEV)
    X = torch.cat(xs).float().to(DEV)
    ws = [w[n].detach().float().to(DEV) for n in LSTM_NAMES]
    out, h_n, gates, cbuf = ops.lstm_bidir(X, off, max(lens), ws, save=True, coop=coop)
    out_c, hn_c = out.cpu().double(), h_n.cpu().double()
    assert torch.isfinite(out_c).all() and torch.isfinite(hn_c).all()
    tol = (2e-5 if matmul == 'f32' else 1e-4) * VE.lstm_widen(name, matmul, 'out')
    worst, o = 0.0, 0
    for s, L in enumerate(lens):
        worst = max(worst, float((out_c[o:o + L] - outs[s][0]).abs().max()), float((hn_c[s] - outs[s][1]).abs().max()))
        o += L
    print('saturated lstm %s coop=%s %s: forward error / bound %.3g' % (name, coop, matmul, worst / tol))
    assert worst < tol
    grads = ops.lstm_bidir_bwd(X, off, max(lens), ws, out, gates, cbuf, torch.cat(d_outs).float().to(DEV), d_hn.float().to(DEV), coop=coop)
    for n, gr in zip(LSTM_NAMES, grads):
        ref = w[n].grad
        assert torch.isfinite(gr).all(), n
        bound = 2e-4 * max(1.0, float(ref.abs().max())) * VE.lstm_widen(name, matmul, n)
        err = float((gr.cpu().double() - ref).abs().max())
        print('saturated lstm %s coop=%s %s: %s error / bound %.3g' % (name, coop, matmul, n, err / bound))
        assert err < bound, (n, err, bound)


# ---- the fused tile operator's tails on the same edges (stair_tile_mlp_fwd, hidden size 512) -------------------------------------------
P_ = 'submodules.'


def _tile_weights(seed, edit=None):
    """(oracle weights in fp64 of the float32 values, the same on the device) of the default configuration, `edit` applied first"""
    w = {k: v.clone() for k, v in oracle_weights(dict(spec.DEFAULT_CONFIG), seed).items()}
    if edit is not None:
        edit(w)
    dw = {k: v.to(DEV) for k, v in w.items() if k.startswith(P_) and '_encoder' not in k}
    return {k: v.double() for k, v in w.items()}, dw


def _lin3(dw, prefix, act):
    return (dw[prefix + '.weight'], dw[prefix + '.bias'], act)


@pytest.mark.parametrize('T', [8, 33])
@pytest.mark.parametrize('fill', [0.0, 1e-10])
def test_tile_cosine_tail_on_rows_under_the_clamp(T, fill):
    """Tail COSINE (Localize) on a tile whose rows after the last layer are all zero (zero weight and bias in video_linear.3) or all
    1e-10 (norm 2.3e-9, under the 1e-8 clamp): the attention against K = 1 and 2 keyword rows, one of them a zero row, against the
    oracle's op_localize in fp64; 2e-5, the bound of test_tile_localize_matches_oracle.  T = 8: packed tiles; T = 33: plain ones."""
    from stair_amd import ops

    def edit(w):
        w[P_ + 'Localize.video_linear.3.weight'].zero_()
        w[P_ + 'Localize.video_linear.3.bias'].fill_(fill)
    w, dw = _tile_weights(0, edit)
    g = torch.Generator().manual_seed(100 + T)
    feat = torch.randn(5, T, 512, generator=g)
    x_idx = torch.tensor([0, 3, 3, 1, 4, 2], dtype=torch.int32)
    K = [1, 2, 1, 2, 2, 1]
    kb = torch.randn(sum(K), 512, generator=g)            # the keyword_linear rows, handed in as they are
    kb[1] = 0
    first = np.concatenate([[0], np.cumsum(K)])[:-1]
    att = torch.zeros(sum(K) + 3, T, device=DEV)
    att_idx = torch.arange(sum(K), dtype=torch.int32) + 2
    i32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.int32).to(DEV)
    ops.tile_mlp(feat.to(DEV), [_lin3(dw, P_ + 'Localize.video_linear.0', 'relu'), _lin3(dw, P_ + 'Localize.video_linear.3', None)],
                 'cosine', x_idx=x_idx.to(DEV), kb=kb.to(DEV), pair_first=i32(first), pair_cnt=i32(K), att_idx=att_idx.to(DEV), att=att)
    assert torch.isfinite(att).all()
    for i in range(len(K)):
        f = O._mlp2(w, P_ + 'Localize.video_linear', feat[int(x_idx[i])].double(), relu_last=False)
        assert float(f.norm(dim=1).max()) < 1e-8
        ref = (O.cos_rows(f.unsqueeze(0), kb[first[i]: first[i] + K[i]].double().unsqueeze(1)) + 1) * 0.49
        got = att[2 + first[i]: 2 + first[i] + K[i]].cpu().double()
        assert float((got - ref).abs().max()) < 2e-5, i
        if fill == 0.0:
            assert bool((got == got[0, 0]).all()) and abs(float(got[0, 0]) - 0.49) < 1e-7, i       # cos = 0 exactly


@pytest.mark.parametrize('T', [8, 33])
@pytest.mark.parametrize('bias', [0.5, -0.5])
def test_tile_layernorm_tail_and_backward_chain_on_zero_variance_rows(T, bias):
    """Tail LAYERNORM and the ln_bwd chain (tile_temporal_bwd) of Temporal, y = LayerNorm(ReLU(Lin(r_t feat_t))), where rows have
    zero variance: the dense bias is one constant and r_t = 0 on every third frame and on one whole instance, so those rows are
    exactly 0.5 everywhere (rstd = 1 / sqrt(eps) = 316) or, with bias -0.5, exactly 0 behind a dead ReLU (dZ must be an exact zero
    there); the other rows are ordinary.  Against fp64 autograd of the same formula, bounds of
    test_tile_hasitem_and_temporal_match_oracle (5e-5) and test_temporal_backward_chain_matches_autograd (3e-5 of max(1, largest)).
    The ordinary rows of the dead form are sparse (a third of the units alive), their rstd and dZ three times those of the tests
    these bounds come from, and the bf16x3 products of the chain scale with them: measured on an MI355X the tail is at 0.99 of its
    bound at T = 33 and drs at 0.89; every other quantity is below 0.2, the flat rows are exact."""
    from stair_amd import ops
    H, n = 512, 9
    g = torch.Generator().manual_seed(11 * n + T)
    feat = torch.randn(n + 1, T, H, generator=g)
    fidx = torch.randperm(n + 1, generator=g)[:n].to(torch.int32)
    rs = 1.0 + torch.rand(n + 4, T, generator=g)              # (at least 1: with the bias at -0.5 a third of an ordinary row's units stay
    ridx = torch.randperm(n + 4, generator=g)[:n].to(torch.int32)       # alive, so its variance stands well clear of eps)
    rs[:, ::3] = 0
    rs[int(ridx[2])] = 0
    w = torch.randn(H, H, generator=g) / H ** 0.5
    b = torch.full((H,), bias)
    gamma = 1.0 + 0.1 * torch.randn(H, generator=g); beta = 0.1 * torch.randn(H, generator=g)
    dy = torch.randn(n + 2, T, H, generator=g)
    yidx = torch.randperm(n + 2, generator=g)[:n].to(torch.int32)
    F = feat.double().requires_grad_(True); R = rs.double().requires_grad_(True)
    G = gamma.double().requires_grad_(True); Bt = beta.double().requires_grad_(True)
    z = (R[ridx.long()].unsqueeze(-1) * F[fidx.long()]) @ w.double().t() + b.double()
    z.retain_grad()
    a = torch.relu(z)
    flat = (a.detach() == a.detach()[..., :1]).all(dim=-1)
    assert int(flat.sum()) >= n * ((T + 2) // 3) + T - (T + 2) // 3
    y = torch.nn.functional.layer_norm(a, (H,), G, Bt, 1e-5)
    (y * dy[yidx.long()].double()).sum().backward()
    d = lambda t: t.to(DEV)
    # forward: the tail
    out = torch.empty(n, T, H, device=DEV)
    saves, _ = ops.tile_mlp(d(feat), [(d(w), d(b), 'relu')], 'layernorm', x_idx=d(fidx), row_scale=d(rs), rs_idx=d(ridx), save=True, out=out,
                            gamma=d(gamma), beta=d(beta), eps=1e-5)
    assert torch.isfinite(out).all()
    err = float((out.cpu().double() - y.detach()).abs().max())
    print('zero-variance rows T=%d bias=%g: LayerNorm tail error / bound %.3g' % (T, bias, err / 5e-5))
    assert err < 5e-5
    assert torch.equal(saves[0].cpu()[flat], torch.full((int(flat.sum()), H), max(bias, 0.0)))          # the flat rows are exact
    # backward: the chain
    dfeat0 = torch.randn(n + 1, T, H, generator=g); drs0 = torch.randn(n + 4, T, generator=g)
    dgamma0 = torch.randn(H, generator=g); dbeta0 = torch.randn(H, generator=g)
    dfeat, drs, dgamma, dbeta = d(dfeat0.clone()), d(drs0.clone()), d(dgamma0.clone()), d(dbeta0.clone())
    dz = ops.tile_temporal_bwd(d(dy), d(a.detach().float()), d(gamma), d(w), d(feat), d(rs), dfeat, drs, dgamma, dbeta,
                               dy_idx=d(yidx), feat_idx=d(fidx), rs_idx=d(ridx), dfeat_idx=d(fidx), exclusive=True)

    def close(got, ref, what):
        assert torch.isfinite(got).all(), what
        err = float((got.cpu().double() - ref).abs().max())
        print('zero-variance rows T=%d bias=%g: %s error / bound %.3g, largest entry %.3g' % (T, bias, what, err / (3e-5 * max(1.0, float(ref.abs().max()))), float(ref.abs().max())))
        assert err < 3e-5 * max(1.0, float(ref.abs().max())), (what, err)
    close(dz, z.grad, 'dZ')
    close(dfeat - d(dfeat0), F.grad, 'dfeat')
    close(drs - d(drs0), R.grad, 'drs')
    close(dgamma - d(dgamma0), G.grad, 'dgamma')
    close(dbeta - d(dbeta0), Bt.grad, 'dbeta')
    if bias < 0:
        assert float(dz.cpu()[flat].abs().max()) == 0.0, 'dZ behind a dead ReLU row must be an exact zero'


@pytest.mark.parametrize('T', [8, 33])
@pytest.mark.parametrize('shift', [30.0, -30.0, 200.0, -200.0])
def test_tile_rowdot_sigmoid_saturated(T, shift):
    """Tail ROWDOT_SIGMOID (HasItem) with its bias moved by +-30 and +-200, and mid_rowdot (FilterFrame's attention between layers 2
    and 3) with the per-tile term `extra` at those values: sigmoid_acc at |logit| = 30 and 200, against the oracle's operators in
    fp64; 1e-5, the bound of test_tile_hasitem_and_temporal_match_oracle / test_tile_filterframe_matches_oracle for these rows."""
    from stair_amd import ops

    def edit(w):
        w[P_ + 'HasItem.param.3.bias'] += shift
    w, dw = _tile_weights(3, edit)
    g = torch.Generator().manual_seed(100 + T)
    feat = torch.randn(5, T, 512, generator=g)
    att = torch.zeros(8, T, device=DEV)
    oi = torch.tensor([1, 7, 3, 4, 0], dtype=torch.int32, device=DEV)
    ops.tile_mlp(feat.to(DEV), [_lin3(dw, P_ + 'HasItem.param.0', 'relu')], 'rowdot_sigmoid', out=att, out_idx=oi, out_gstride=T,
                 vw=dw[P_ + 'HasItem.param.3.weight'].reshape(-1).contiguous(), vb=dw[P_ + 'HasItem.param.3.bias'])
    assert torch.isfinite(att).all() and float(att.min()) >= 0.0 and float(att.max()) <= 1.0
    for i in range(5):
        ref = O.op_hasitem(w, feat[i].double()).reshape(T)
        assert float((att[int(oi[i])].cpu().double() - ref).abs().max()) < 1e-5, i
    if abs(shift) == 200:
        assert bool((att[oi.long()] == (1.0 if shift > 0 else 0.0)).all())
    # FilterFrame's attention: sigmoid(f . wa[:512] + bias + extra), extra = the keyword's share of the attention row
    pre = P_ + 'FilterFrame.param.representation'
    layers = [_lin3(dw, pre + '.0', 'relu'), _lin3(dw, pre + '.3', 'relu'), _lin3(dw, P_ + 'FilterFrame.dense.0', 'relu')]
    wa = dw[P_ + 'FilterFrame.attention.0.weight'].reshape(-1)
    extra = torch.tensor([shift, -shift, shift, 0.0, shift / 2])
    out = torch.zeros(5, T, 512, device=DEV)
    saves, rs = ops.tile_mlp(feat.to(DEV), layers, 'store', save=True, mid_rowdot=(wa[:512].contiguous(), dw[P_ + 'FilterFrame.attention.0.bias'],
                                                                              extra.to(DEV)), out=out)
    assert torch.isfinite(rs).all() and torch.isfinite(out).all()
    for i in range(5):
        f = O._mlp2(w, pre, feat[i].double())
        a = torch.sigmoid(f @ w[P_ + 'FilterFrame.attention.0.weight'].reshape(-1)[:512] + w[P_ + 'FilterFrame.attention.0.bias'] + extra[i].double())
        assert float((rs[i].cpu().double() - a.reshape(-1)).abs().max()) < 1e-5, i
        ref = torch.relu(O._lin(w, P_ + 'FilterFrame.dense.0', a.reshape(-1, 1) * f))
        assert float((out[i].cpu().double() - ref).abs().max()) < 3e-5 * max(1.0, float(ref.abs().max())), i
