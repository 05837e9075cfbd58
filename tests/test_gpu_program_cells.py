"""GPU tests of the cell corpus (tests/program_cells.py): one tiny program per producer -> consumer operand pair the plan builder
admits, all run as ONE batch, every module node and -- question by question -- the input gradients against the oracle.

The whole-path tests elsewhere run the twelve forms of synth.ALL_FORMS and compare gradients summed over the batch; here a wrong
gradient in one small subtree has nowhere to hide: d_video[q] and question q's rows of d_question are held to 2e-4 of THAT
question's own largest gradient (floor 1e-6: the smallest non-zero per-question max|d_video| of the corpus is 6.9e-6), and where
the oracle's gradient is identically zero -- a program that never reads the clip, Superlative over a single action, whose softmax
weight is exactly 1 -- the kernels' must be exact zeros.  The yardstick is the reference side alone: the oracle in fp32 against
the oracle in fp64 differs per question by at most 3e-7 (logits), 7e-7 (d_video) and 1.2e-6 (d_question) relative on this corpus.

One oracle pass (forward + autograd, CPU, a few seconds) per geometry, shared by the tests of that geometry (_geometry)."""
import functools

import pytest
import torch

import program_cells as PC
from oracle import nmn_oracle as O
from stair_amd import spec
from helpers import _ForcedMasks
from test_gpu_autograd import _R, _check_params, _close, _custom, _model, _weights

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEED = 0
REL = 2e-4                  # the project's gradient bound, here per question
FLOOR = 1e-6
ZERO_D_VIDEO_CELLS = 36     # cells whose clip gets no gradient at all in the ORACLE (counted there, on the CPU)

# Cells checked with the oracle differentiating through the HIP pass's own ReLU masks (helpers._ForcedMasks), because a
# pre-activation of theirs lies within rounding of zero and the two implementations pick different sides of the kink:
# {geometry: {cell name: masks that differ}}.  Same 2e-4 bound.  Every other cell is checked against the plain oracle.
FORCED_MASKS = {}


def _tiny(L):
    return dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, answer_vocab_length=16, max_video_length=L, object_types=10)


# name -> (config, T, cells, clips shared (cell k on clip k % 3), frames per question or None)
GEOMETRIES = {
    'conv': lambda: (_tiny(40), 24, PC.cells(), False, None),                       # Conv1d Temporal nets, one 64-row tile per clip
    'conv_shared': lambda: (_tiny(40), 24, PC.cells(), True, None),
    'linear8': lambda: (_tiny(8), 8, PC.map_frame_att_cells(), False, None),         # Linear Temporal nets, 8 clips per packed tile
    'long70': lambda: (_tiny(100), 70, PC.map_frame_att_cells(), False, None),       # two segments, the second of 6 rows
    'ragged': lambda: (_tiny(40), 24, PC.map_frame_att_cells(), False, (3, 17, 24)),
    # the reference's hidden size (fused tile operators, grouped vector-level launches: the bit-reproducible step); no oracle
    'h512': lambda: (dict(_tiny(40), hidden_size=512), 24, PC.cells(), False, None),
    'h512_shared': lambda: (dict(_tiny(40), hidden_size=512), 24, PC.cells(), True, None),
}


class Geometry:
    pass


@functools.lru_cache(maxsize=None)
def _geometry(name):
    """The questions of a geometry and the oracle on them: per question the logits, every step's value, d_video and d_question of
    the custom loss of test_gpu_autograd.py, and the parameter gradients summed over the batch.  Computed once; nobody writes to it."""
    g = Geometry()
    g.name = name
    g.config, g.T, g.cells, g.shared, lens = GEOMETRIES[name]()
    g.qs = PC.questions(g.config, SEED, g.T, g.cells)
    n = len(g.qs)
    g.frames = None if lens is None else [lens[k % len(lens)] for k in range(n)]
    g.R = _R(n, g.config['answer_vocab_length'])
    g.names, g.w = _weights(g.config, SEED)
    leaf = lambda a: torch.as_tensor(a).float().clone().requires_grad_(True)
    g.clips = [leaf(g.qs[c]['video_features']) for c in range(3)] if g.shared else None
    g.index = [k % 3 for k in range(n)] if g.shared else None
    g.logits, g.steps, g.d_video, g.d_question = [], [], [], []
    if name.startswith('h512'):
        return g
    for k, q in enumerate(g.qs):
        v = g.clips[k % 3] if g.shared else leaf(q['video_features'][:g.frames[k]] if g.frames else q['video_features'])
        qq = leaf(q['question'])
        r = O.forward(g.w, g.config, dict(q, video_features=v, question=qq), return_res_by_step=False,
                      return_result_of_each_step=True, explicit_lstm=True)
        _custom(r['logits'].unsqueeze(0), g.R[k:k + 1]).backward()
        g.logits.append(r['logits'].detach())
        g.steps.append([s.detach() if isinstance(s, torch.Tensor) else None for _, s in r['result_of_each_step']])
        if not g.shared:
            g.d_video.append(v.grad if v.grad is not None else torch.zeros_like(v))
        g.d_question.append(qq.grad)
    if g.shared:
        g.d_video = [c.grad for c in g.clips]
    return g


@pytest.fixture(scope='module', params=['conv', 'linear8', 'long70', 'ragged'])
def geo(request):
    return _geometry(request.param)


@pytest.fixture(scope='module')
def conv():
    return _geometry('conv')


@pytest.fixture(scope='module')
def conv_shared():
    return _geometry('conv_shared')


@pytest.fixture(params=['f32', 'bf16x3'])
def matmul(request):
    from stair_amd import ops
    ops.set_matmul_mode(request.param)
    yield request.param
    ops.set_matmul_mode('bf16x3')


@pytest.fixture
def f32():
    from stair_amd import ops
    ops.set_matmul_mode('f32')
    yield 'f32'
    ops.set_matmul_mode('bf16x3')


# ---- the HIP side --------------------------------------------------------------------------------------------------------------
def _inputs(g):
    """(programs, spans, video [n or 3, T, V] zero-padded behind a short clip's frames, question rows, q_lens, video_len)"""
    if g.shared:
        video = torch.stack([c.detach() for c in g.clips])
    else:
        video = torch.stack([torch.as_tensor(q['video_features']) for q in g.qs])
        if g.frames:
            video = video * (torch.arange(g.T)[None, :] < torch.tensor(g.frames)[:, None]).unsqueeze(-1)
    question = torch.cat([torch.as_tensor(q['question']) for q in g.qs])
    return ([q['nmn_program_list'] for q in g.qs], [q['prog_str_to_question_tokens'] for q in g.qs], video.to(DEV).contiguous(),
            question.to(DEV).contiguous(), [q['question'].shape[0] for q in g.qs], g.frames)


def _run(model, g, train=False, cse=True):
    progs, spans, video, question, q_lens, frames = _inputs(g)
    return model.run_programs(progs, spans, video, question, q_lens, train=train, video_index=g.index, video_len=frames, cse=cse)


def _train_pass(model, g, cse=True):
    """One training pass of the batch with the custom loss: (result, d_video, d_question, {parameter: gradient}) on the host"""
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    res = _run(model, g, train=True, cse=cse)
    lg = res.logits.clone().requires_grad_(True)
    _custom(lg, g.R.to(DEV)).backward()
    dv = torch.full(res._video.shape, float('nan'), dtype=torch.float32, device=DEV)      # both are OVERWRITTEN by the pass
    dq = torch.full(res._question.shape, float('nan'), dtype=torch.float32, device=DEV)
    res.backward_dlogits(lg.grad.contiguous(), d_video=dv, d_question=dq)
    res.check()
    return res, dv.cpu(), dq.cpu(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def _fit(got, ref):
    """a node's value cut to the frames of the question's clip (ragged batches pad every [T, H] map and [.., T] row to the longest)"""
    got = got.detach().float().cpu()
    if got.shape != ref.shape:
        got = got[:ref.shape[0]] if ref.dim() == 2 and got.shape[-1] == ref.shape[-1] else got[..., :ref.shape[-1]]
    return got


def _node_values(res, g):
    return [[res.node(q, i).detach().cpu().clone() if s is not None else None for i, s in enumerate(steps)] for q, steps in enumerate(g.steps)]


def _check_forward(res, g, tol):
    """logits, top-1 answer and EVERY module node of every question against the oracle; returns the number of nodes compared"""
    logits, pred = res.logits.cpu(), res.pred.cpu()
    worst, n_nodes = (0.0, ''), 0
    for q, c in enumerate(g.cells):
        ref = g.logits[q]
        bound = tol * max(1.0, float(ref.abs().max()))
        err = float((logits[q] - ref).abs().max())
        worst = max(worst, (err / bound, '%s logits' % c))
        assert err < bound, (c, 'logits', err, bound)
        top = torch.topk(ref, 2).values
        if float(top[0] - top[1]) > bound:
            assert int(pred[q]) == int(torch.argmax(ref)), c
        assert res.levels(q) == O.module_levels(c.program), c
        for i, ref in enumerate(g.steps[q]):
            if ref is None or c.program[i] not in O.ARITY:
                continue
            got = _fit(res.node(q, i), ref)
            assert got.shape == ref.shape, (c, i, got.shape, ref.shape)
            bound = tol * max(1.0, float(ref.abs().max()))
            err = float((got - ref).abs().max())
            worst = max(worst, (err / bound, '%s node %d %s' % (c, i, c.program[i])))
            assert err < bound, (c, i, c.program[i], err, bound)
            n_nodes += 1
    print('%s: %d cells, %d module nodes, worst error / bound %.3g at %s' % ((g.name, len(g.cells), n_nodes) + worst))
    assert n_nodes == sum(t in O.ARITY for c in g.cells for t in c.program)
    return n_nodes


def _rows(g, q):
    off = sum(x['question'].shape[0] for x in g.qs[:q])
    return slice(off, off + g.qs[q]['question'].shape[0])


def _err(got, ref):
    """(error, bound) of one question's gradient: 2e-4 of its own largest entry, floor 1e-6; an all-zero reference wants exact zeros"""
    if float(ref.abs().max()) == 0.0:
        return float(got.abs().max()), 0.0
    return float((got - ref).abs().max()), REL * max(float(ref.abs().max()), FLOOR)


def _forced_oracle(model, g, which):
    """{q: (d_video, d_question, flips)} of the questions `which`, the oracle differentiating through the ReLU masks of a HIP pass
    (read from a fresh forward run of the training plan, before any backward pass touches its workspace)"""
    res = _run(model, g, train=True)
    out = {}
    for q in which:
        d = g.qs[q]
        v = torch.as_tensor(d['video_features'][:g.frames[q]] if g.frames else d['video_features']).float().clone().requires_grad_(True)
        qq = torch.as_tensor(d['question']).float().clone().requires_grad_(True)
        w = {k: t.detach() for k, t in g.w.items()}
        fm = _ForcedMasks(res, q, d['nmn_program_list'])
        lg = fm.forward(w, g.config, dict(d, video_features=v, question=qq), return_res_by_step=False, explicit_lstm=True)['logits']
        _custom(lg.unsqueeze(0), g.R[q:q + 1]).backward()
        out[q] = (v.grad if v.grad is not None else torch.zeros_like(v), qq.grad, fm.flips)
    return out


def _check_input_gradients(model, g, dv, dq):
    """Question by question: d_video[q] (exact zeros behind a short clip's frames) and the question's rows of d_question.  The cells
    of FORCED_MASKS[g.name] are held to the oracle under the HIP pass's masks, every other cell to the plain oracle."""
    listed = FORCED_MASKS.get(g.name, {})
    names = [c.name for c in g.cells]
    assert set(listed) <= set(names)
    fails, worst, n_zero, n_checked = {}, (0.0, ''), 0, 0
    for q, c in enumerate(g.cells):
        f = g.frames[q] if g.frames else g.T
        assert torch.count_nonzero(dv[q, f:]) == 0, (c, 'd_video behind the clip\'s frames')
        n_zero += int(float(g.d_video[q].abs().max()) == 0.0)
        n_checked += 1
        if c.name in listed:
            continue
        for what, got, ref in (('d_video', dv[q, :f], g.d_video[q]), ('d_question', dq[_rows(g, q)], g.d_question[q])):
            err, bound = _err(got, ref)
            if bound == 0.0:
                assert err == 0.0, (c, what, 'must be exact zeros', err)
            else:
                worst = max(worst, (err / bound, '%s %s' % (c, what)))
                if not err < bound:
                    fails.setdefault(q, []).append((what, err, bound))
    print('%s: %d cells, %d with an all-zero d_video, worst error / bound %.3g at %s' % ((g.name, n_checked, n_zero) + worst))
    forced = _forced_oracle(model, g, sorted(set(fails) | {names.index(n) for n in listed})) if fails or listed else {}
    for q, why in fails.items():            # not listed: report what the forced masks would say, then fail
        fv, fq, flips = forced[q]
        f = g.frames[q] if g.frames else g.T
        print('FAILS %s: %s; under the HIP masks (%d differ): d_video %s, d_question %s'
              % (g.cells[q], why, flips, _err(dv[q, :f], fv), _err(dq[_rows(g, q)], fq)))
    assert not fails, [(g.cells[q].name, why) for q, why in fails.items()]
    checked_forced = set()
    for n in listed:
        q = names.index(n)
        fv, fq, flips = forced[q]
        f = g.frames[q] if g.frames else g.T
        for what, got, ref in (('d_video', dv[q, :f], fv), ('d_question', dq[_rows(g, q)], fq)):
            err, bound = _err(got, ref)
            assert err < bound or err == bound == 0.0, (n, what, 'under the HIP masks', err, bound)
        assert flips == listed[n], (n, flips)
        checked_forced.add(n)
    assert checked_forced == set(listed)
    assert n_checked == len(g.cells)
    return n_zero


def _check_param_gradients(model, g, grads):
    """the parameter gradients summed over the batch by test_gpu_autograd._check_params; a weight no cell reaches holds exact zeros"""
    for n, p in model.named_parameters():
        p.grad = grads[n].clone()
        if g.w[n].grad is None and 'Filter.attention' not in n:
            assert float(p.grad.abs().max()) == 0.0, n
            p.grad = None
    _check_params(model, g.names, g.w, REL)


# ---- (a) forward: every node of every cell -------------------------------------------------------------------------------------
def test_every_cell_node_matches_oracle(geo, matmul):
    g = geo
    model = _model(g.config, SEED)
    res = _run(model, g)
    assert res.info.n_questions == len(g.cells) == {'conv': 371}.get(g.name, 74)
    _check_forward(res, g, 2e-5 if matmul == 'f32' else 1e-4)


# ---- (b), (d) backward: input gradients question by question, exact-fp32 products -------------------------------------------------
def test_every_cell_input_gradients_match_oracle(geo, f32):
    g = geo
    model = _model(g.config, SEED)
    res, dv, dq, grads = _train_pass(model, g)
    assert res.info.n_questions == len(g.cells)
    n_zero = _check_input_gradients(model, g, dv, dq)
    if g.name == 'conv':
        assert n_zero == ZERO_D_VIDEO_CELLS
    _check_param_gradients(model, g, grads)


# ---- (c) shared clips, with and without common subexpressions -------------------------------------------------------------------
def test_shared_clips_cse_is_bit_equal_and_gradients_match(conv_shared, f32):
    g = conv_shared
    model = _model(g.config, SEED)
    runs = {}
    for cse in (True, False):
        res, dv, dq, grads = _train_pass(model, g, cse=cse)
        assert (res.info.n_aliased > 0) == cse and res._video.shape[0] == 3
        runs[cse] = (res.logits.cpu().clone(), _node_values(res, g), dv, dq, grads)
        if cse:
            assert res.info.n_map_stage > 0 and res.info.n_vec_stage > 0 and res.info.n_att_stage > 0
            _check_forward(res, g, 2e-5)
        # the oracle's sums over the questions of each clip
        _check_param_gradients(model, g, grads)
        _close(dv, torch.stack(g.d_video), REL, 'd_video per clip, cse=%s' % cse)
        for q in range(len(g.cells)):
            err, bound = _err(dq[_rows(g, q)], g.d_question[q])
            assert err < bound, (g.cells[q], 'd_question', cse, err, bound)
    assert torch.equal(runs[True][0], runs[False][0])
    n = 0
    for q, (a, b) in enumerate(zip(runs[True][1], runs[False][1])):
        for i, (x, y) in enumerate(zip(a, b)):
            if x is not None:
                assert torch.equal(x, y), (g.cells[q], i)
                n += 1
    assert n == sum(s is not None for steps in g.steps for s in steps) > 1515


# ---- (e) reproducibility ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['h512', 'h512_shared'])
def test_cell_batch_training_pass_is_bit_reproducible(name):
    """Two training passes of the full cell batch, own clips and 3 shared clips (aliased nodes, staging slots in all three
    arenas): bit-identical parameter gradients and input gradients -- the fan-in staging and the first-touch stores of the new pairs
    keep what test_training_step_is_bit_reproducible asserts for the forms.  At hidden size 512 and in the default product mode,
    as there: that is where the step is reproducible at all.  Other hidden sizes and the exact-fp32 mode run the unfused operator
    sequences, whose sums depend on the order of their atomics, with these programs as with the forms."""
    from stair_amd import ops
    g = _geometry(name)
    runs = []
    for rep in range(2):
        model = _model(g.config, SEED)
        with ops.kernel_accounting() as acct:
            res, dv, dq, grads = _train_pass(model, g)
        assert 'tile_mlp' in acct.table
        if g.shared:
            assert res.info.n_aliased > 0 and res.info.n_map_stage > 0 and res.info.n_vec_stage > 0 and res.info.n_att_stage > 0
        runs.append((dv, dq, grads))
        del res
    assert not torch.isnan(runs[0][0]).any() and not torch.isnan(runs[0][1]).any()
    assert float(runs[0][0].abs().max()) > 0
    differ = [n for n in runs[0][2] if not torch.equal(runs[0][2][n], runs[1][2][n])]
    assert not differ, differ
    assert torch.equal(runs[0][0], runs[1][0]), 'd_video'
    assert torch.equal(runs[0][1], runs[1][1]), 'd_question'
