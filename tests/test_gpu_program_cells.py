"""GPU tests of the cell corpus (tests/program_cells.py): one tiny program per producer -> consumer operand pair the plan builder
admits, all run as ONE batch, every module node and -- question by question -- the input gradients against the oracle.

The whole-path tests elsewhere run the twelve forms of synth.ALL_FORMS and compare gradients summed over the batch; here a wrong
gradient in one small subtree has nowhere to hide: d_video[q] and question q's rows of d_question are held to 2e-4 of THAT
question's own largest gradient (floor 1e-6: the smallest non-zero per-question max|d_video| of the corpus is 6.9e-6), and where
the oracle's gradient is identically zero -- a program that never reads the clip, Superlative over a single action, whose softmax
weight is exactly 1 -- the kernels' must be exact zeros.  The yardstick is the reference side alone: the oracle in fp32 against
the oracle in fp64 differs per question by at most 3e-7 (logits), 7e-7 (d_video) and 1.2e-6 (d_question) relative on this corpus.

One oracle pass (forward + autograd, CPU, a few seconds) per geometry, shared by the tests of that geometry (_geometry).

Hidden size 512, default bf16x3 products -- the fused tile operators (packed and segmented tiles), the grouped vector-level
launches, backward tile chains with first-touch stores and fan-in staging rows: the path bench.py times.  There the oracle
differentiates through the ReLU masks of the HIP pass (_masked_geometry, helpers._ForcedMasks) for EVERY cell, because at this
width the plain oracle cannot be the yardstick: on the 371 cells (T = 24, V = 128, seed 0) the oracle in fp32 and in fp64 already
take different sides of one ReLU kink among 21 210 624 sites (cell `AttnVideo X HI <- AttnVideo video HI`, fp64 pre-activation
8e-5 of the forward bound), which moves that cell's d_video by 6.6e-3 of its maximum and Filter.param.objects.3.bias of the
batch sum by 3.7e-4, while no cell without a flip differs by more than 2e-4 per question (logits 4.5e-7, d_question 8.5e-7;
d_video is identically zero in 34 cells at this width).  Forced masks leave the oracle's forward values as they are, so the
same pass gives the node values, and given equal masks the bounds are the file's: nodes 1e-4, gradients 2e-4 per question.
The flips are conditions, not measurements:
  - more than 2e7 sites are compared on the full corpus (every [frames, H] mask of every map-level module on the small ones);
  - fewer than 1e-4 of them disagree (the share test_full_size_gradients_are_strict_given_the_same_relu_masks allows);
  - at every disagreement the oracle's |pre-activation| is below the forward bound of that tensor, 1e-4 * max(1, max|ref|):
    an activation that passed the forward check cannot differ in sign anywhere else, so a gradient cannot be made to fit by a
    mask the kernels had no right to.
Shared clips at this width are checked GPU against GPU (sharing, cse=False, and the expanded batch the oracle has judged)."""
import functools
import time

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


def _wide(L):
    return dict(_tiny(L), hidden_size=512)


# name -> (config, T, cells, clips shared (cell k on clip k % 3), frames per question or None)
GEOMETRIES = {
    'conv': lambda: (_tiny(40), 24, PC.cells(), False, None),                       # Conv1d Temporal nets, one 64-row tile per clip
    'conv_shared': lambda: (_tiny(40), 24, PC.cells(), True, None),
    'linear8': lambda: (_tiny(8), 8, PC.map_frame_att_cells(), False, None),         # Linear Temporal nets, 8 clips per packed tile
    'long70': lambda: (_tiny(100), 70, PC.map_frame_att_cells(), False, None),       # two segments, the second of 6 rows
    'ragged': lambda: (_tiny(40), 24, PC.map_frame_att_cells(), False, (3, 17, 24)),
    # the reference's hidden size (fused tile operators, grouped vector-level launches: the bit-reproducible step).  Own clips: the
    # oracle under the HIP pass's masks (_masked_geometry); shared clips: GPU against GPU
    'h512': lambda: (_wide(40), 24, PC.cells(), False, None),
    'h512_shared': lambda: (_wide(40), 24, PC.cells(), True, None),
    'linear8_h512': lambda: (_wide(8), 8, PC.map_frame_att_cells(), False, None),    # 8 clips per packed tile
    'long70_h512': lambda: (_wide(100), 70, PC.map_frame_att_cells(), False, None),  # two segments, the second of 6 rows
    'ragged_h512': lambda: (_wide(40), 24, PC.map_frame_att_cells(), False, (3, 17, 24)),
}
MASKED = ['h512', 'linear8_h512', 'long70_h512', 'ragged_h512']
ZERO_D_VIDEO_CELLS_H512 = 34   # as ZERO_D_VIDEO_CELLS, geometry 'h512'
MAP_LEVEL = ('Filter', 'FilterFrame', 'HasItem', 'Localize', 'Superlative', 'Temporal')     # each saves a [frames, H] ReLU mask


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
    if 'h512' in name:           # the oracle of these needs a HIP pass's masks: _masked_geometry
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
def _inputs(g, expand=False):
    """(programs, spans, video [n or 3, T, V] zero-padded behind a short clip's frames, question rows, q_lens, video_len);
    expand: every question of a shared geometry gets a copy of its clip"""
    if g.shared:
        video = torch.stack([g.clips[c].detach() for c in (g.index if expand else range(3))])
    else:
        video = torch.stack([torch.as_tensor(q['video_features']) for q in g.qs])
        if g.frames:
            video = video * (torch.arange(g.T)[None, :] < torch.tensor(g.frames)[:, None]).unsqueeze(-1)
    question = torch.cat([torch.as_tensor(q['question']) for q in g.qs])
    return ([q['nmn_program_list'] for q in g.qs], [q['prog_str_to_question_tokens'] for q in g.qs], video.to(DEV).contiguous(),
            question.to(DEV).contiguous(), [q['question'].shape[0] for q in g.qs], g.frames)


def _run(model, g, train=False, cse=True, expand=False):
    progs, spans, video, question, q_lens, frames = _inputs(g, expand)
    return model.run_programs(progs, spans, video, question, q_lens, train=train, video_index=None if expand else g.index,
                              video_len=frames, cse=cse)


def _train_pass(model, g, cse=True, expand=False):
    """One training pass of the batch with the custom loss: (result, d_video, d_question, {parameter: gradient}) on the host"""
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    res = _run(model, g, train=True, cse=cse, expand=expand)
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


# ---- (f) hidden size 512, default product mode: the oracle under the HIP pass's masks ------------------------------------------------
@functools.lru_cache(maxsize=None)
def _masked_geometry(name):
    """A geometry of MASKED with the oracle on it, every question differentiated through the ReLU masks of the HIP pass: read from
    a fresh forward run of the training plan before any backward pass touches its workspace, as _forced_oracle does.  Forward
    values are the oracle's own.  Also g.w[n].grad, the parameter gradients summed over the batch; g.hip_logits, the logits of the
    run the masks were read from (the forward pass at this width is reproducible bit for bit, so a test's own training pass must
    give the same ones -- asserted there -- and hence the same masks); g.sites, g.flips; g.flip_reach, (the largest oracle
    |pre-activation| at a flip / max(1, max of that activation), the cell) ; g.seconds, the oracle's wall time.
    One intra-op thread: a cell takes 55 ms that way and 123 ms with 16 threads.  Computed once; nobody writes to it."""
    from stair_amd import ops
    assert ops.get_matmul_mode() == 'bf16x3'
    g = _geometry.__wrapped__(name)         # a Geometry of its own: _geometry(name) stays without an oracle
    assert not g.shared
    model = _model(g.config, SEED)
    res = _run(model, g, train=True)
    g.hip_logits = res.logits.cpu().clone()
    g.sites, g.flips, g.flip_reach = 0, 0, (0.0, '')
    leaf = lambda a: torch.as_tensor(a).float().clone().requires_grad_(True)
    threads, t0 = torch.get_num_threads(), time.perf_counter()
    torch.set_num_threads(1)
    try:
        for k, (q, c) in enumerate(zip(g.qs, g.cells)):
            v, qq = leaf(q['video_features'][:g.frames[k]] if g.frames else q['video_features']), leaf(q['question'])
            fm = _ForcedMasks(res, k, q['nmn_program_list'])
            r = fm.forward(g.w, g.config, dict(q, video_features=v, question=qq), return_res_by_step=False,
                           return_result_of_each_step=True, explicit_lstm=True)
            _custom(r['logits'].unsqueeze(0), g.R[k:k + 1]).backward()
            g.logits.append(r['logits'].detach())
            g.steps.append([s.detach() if isinstance(s, torch.Tensor) else None for _, s in r['result_of_each_step']])
            g.d_video.append(v.grad if v.grad is not None else torch.zeros_like(v))
            g.d_question.append(qq.grad)
            g.sites, g.flips, g.flip_reach = g.sites + fm.sites, g.flips + fm.flips, max(g.flip_reach, (fm.flip_reach, c.name))
    finally:
        torch.set_num_threads(threads)
    g.seconds = time.perf_counter() - t0
    g.n_zero = sum(float(d.abs().max()) == 0.0 for d in g.d_video)
    print('%s: oracle under the HIP masks: %d cells in %.1f s, %d ReLU sites, %d flips, largest |pre-activation| / bound at a flip '
          '%.3g (%s), %d cells with an all-zero d_video' % (name, len(g.cells), g.seconds, g.sites, g.flips, g.flip_reach[0] / 1e-4,
                                                          g.flip_reach[1], g.n_zero))
    return g


@pytest.fixture(scope='module', params=MASKED)
def wide(request):
    return _masked_geometry(request.param)


def _fused_train_pass(g):
    """a training pass of a fresh model on the fused path (asserted), whose forward values are those the masks were read from"""
    from stair_amd import ops
    assert ops.get_matmul_mode() == 'bf16x3'
    model = _model(g.config, SEED)
    with ops.kernel_accounting() as acct:
        res, dv, dq, grads = _train_pass(model, g)
    assert 'tile_mlp' in acct.table and 'vec_group' in acct.table, sorted(acct.table)
    assert res.info.n_questions == len(g.cells) == (371 if g.name == 'h512' else 74)
    assert torch.equal(res.logits.cpu(), g.hip_logits), 'this pass is not the pass the masks were read from'
    return model, res, dv, dq, grads


def test_fused_path_every_cell_node_matches_oracle(wide):
    g = wide
    model, res, dv, dq, grads = _fused_train_pass(g)
    _check_forward(res, g, 1e-4)


def test_fused_path_relu_flips_stay_inside_the_forward_bound(wide):
    """the conditions under which the gradient tests below mean anything (module docstring)"""
    g = wide
    frames = lambda k: g.frames[k] if g.frames else g.T
    floor = 2e7 if g.name == 'h512' else sum(frames(k) * g.config['hidden_size'] * sum(t in MAP_LEVEL for t in c.program)
                                            for k, c in enumerate(g.cells))
    print('%s: %d ReLU sites (at least %d wanted), %d flips, largest |pre-activation| / bound at a flip %.3g (%s)'
          % (g.name, g.sites, floor, g.flips, g.flip_reach[0] / 1e-4, g.flip_reach[1]))
    assert g.sites > floor > 0
    assert g.flips < 1e-4 * g.sites
    assert g.flip_reach[0] < 1e-4, g.flip_reach


def test_fused_path_every_cell_input_gradients_match_oracle(wide):
    g = wide
    assert g.name not in FORCED_MASKS           # every cell of these is under the masks already
    model, res, dv, dq, grads = _fused_train_pass(g)
    n_zero = _check_input_gradients(model, g, dv, dq)
    assert n_zero == g.n_zero
    if g.name == 'h512':
        assert n_zero == ZERO_D_VIDEO_CELLS_H512


def _check_param_gradients_by_family(g, grads):
    """_check_param_gradients with the rule of test_full_size_gradients_are_strict_given_the_same_relu_masks for the tensors of
    fewer than 64 elements: 2e-4 of the largest gradient entry of their FAMILY (the layers of one net: `a.b.N.weight` -> `a.b`).
    Those are the filters and scalar biases of Temporal's relate nets, sums over frames and cells with heavy cancellation, whose
    terms carry the bf16x3 products' 4e-6 each.  One of them needs the rule: on the 371 cells the 1-element
    Temporal.relate.after.2.bias (-2.64e-3) is 1.08e-6 off, 2.04 x the bound of its own value; 1.33e-6 (2.53 x) with the tile
    operators switched off, 8.2e-8 (0.156 x) in exact-fp32 mode under that mode's masks -- product rounding, not a lost term;
    every other tensor is below 0.23 x its own bound.  Every tensor of 64 elements and more keeps _check_params' bound of its own
    largest entry (floor 1e-3, as there); a weight no cell reaches holds exact zeros."""
    family_max = {}
    for n in g.names:
        if g.w[n].grad is not None:
            fam = n.rsplit('.', 2)[0]
            family_max[fam] = max(family_max.get(fam, 0.0), float(g.w[n].grad.abs().max()))
    worst, worst_small, fails = (0.0, ''), (0.0, 0.0, ''), []
    assert set(grads) >= set(g.names)
    for n in g.names:
        ref, got = g.w[n].grad, grads[n].float().cpu()
        if ref is None:
            assert float(got.abs().max()) == 0.0, (n, 'no cell reaches it: exact zeros')
            continue
        small = ref.numel() < 64
        err = float((got - ref).abs().max())
        own = REL * max(float(ref.abs().max()), 1e-3)
        bound = REL * max(family_max[n.rsplit('.', 2)[0]], 1e-3) if small else own
        if small:
            worst_small = max(worst_small, (err / bound, err / own, n))
        else:
            worst = max(worst, (err / bound, n))
        if not err < bound:
            fails.append((n, err, bound))
    print('%s: parameter gradients: worst error / bound %.3g at %s; tensors of < 64 elements, by family: %.3g (%.3g of its own '
          'bound) at %s' % ((g.name,) + worst + worst_small))
    assert not fails, fails


def test_fused_path_parameter_gradients_match_oracle(wide):
    g = wide
    model, res, dv, dq, grads = _fused_train_pass(g)
    _check_param_gradients_by_family(g, grads)


# ---- (g) shared clips at hidden size 512: sharing, no sharing and the expanded batch, GPU against GPU ---------------------------------
def test_fused_path_shared_clips_equal_the_expanded_batch():
    """Three clips, cell k on clip k % 3: the batch with common subexpressions shared, with cse=False, and expanded (every question
    owns a copy of its clip: the code test_fused_path_* hold to the oracle).  Forward values are row-independent on this path: every
    node and the logits are bit-equal, so the ReLU masks are equal and what is left between the gradients is the order of sums:
    d_question per question, d_video summed per clip and every parameter gradient within 2e-4 of the tensor's largest entry."""
    from stair_amd import ops
    assert ops.get_matmul_mode() == 'bf16x3'
    g = _geometry('h512_shared')
    runs = {}
    for how in ('cse', 'no_cse', 'expanded'):
        model = _model(g.config, SEED)
        with ops.kernel_accounting() as acct:
            res, dv, dq, grads = _train_pass(model, g, cse=how != 'no_cse', expand=how == 'expanded')
        assert 'tile_mlp' in acct.table and 'vec_group' in acct.table, sorted(acct.table)
        assert not torch.isnan(dv).any() and not torch.isnan(dq).any()
        if how == 'expanded':
            assert res._video.shape[0] == len(g.cells)
            dv = torch.zeros(3, *dv.shape[1:]).index_add_(0, torch.tensor(g.index), dv)
        else:
            assert (res.info.n_aliased > 0) == (how == 'cse') and res._video.shape[0] == 3
        if how == 'cse':
            assert res.info.n_map_stage > 0 and res.info.n_vec_stage > 0 and res.info.n_att_stage > 0
        nodes = [[res.node(q, i).detach().cpu().clone() for i, t in enumerate(c.program) if t in O.ARITY] for q, c in enumerate(g.cells)]
        runs[how] = (res.logits.cpu().clone(), nodes, dv, dq, grads)
        del res
    ref = runs['expanded']
    assert sum(len(x) for x in ref[1]) == sum(t in O.ARITY for c in g.cells for t in c.program)
    assert float(ref[2].abs().max()) > 0
    for how in ('cse', 'no_cse'):
        got = runs[how]
        assert torch.equal(got[0], ref[0]), (how, 'logits')
        for q, (a, b) in enumerate(zip(got[1], ref[1])):
            for k, (x, y) in enumerate(zip(a, b)):
                assert torch.equal(x, y), (how, g.cells[q], 'module node %d' % k)
        worst = (0.0, '')
        for q in range(len(g.cells)):
            err, bound = _err(got[3][_rows(g, q)], ref[3][_rows(g, q)])
            worst = max(worst, (err / bound if bound else float(err > 0), '%s d_question' % g.cells[q]))
            assert err < bound or err == bound == 0.0, (how, g.cells[q], 'd_question', err, bound)
        for c in range(3):
            err, bound = _err(got[2][c], ref[2][c])
            worst = max(worst, (err / bound, 'd_video of clip %d' % c))
            assert err < bound, (how, 'd_video of clip %d' % c, err, bound)
        for n, r in ref[4].items():
            err, bound = _err(got[4][n].cpu(), r.cpu())
            if bound:
                worst = max(worst, (err / bound, n))
            assert err < bound or err == bound == 0.0, (how, n, err, bound)
        print('h512_shared, %s against the expanded batch: worst error / bound %.3g at %s' % ((how,) + worst))
