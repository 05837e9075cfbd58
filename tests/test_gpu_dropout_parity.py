"""Training-mode dropout against the oracle, with the kernels' own masks (`-m gpu`).

nn.Dropout(0.25) is the recipe the reference trains with (args.py:31); the library draws it inside the fused tile operators, the
grouped vector-level launches and the row kernels (stair_plan_set_dropout).  torch's Philox stream cannot be matched, and need
not be: a dropped element is an exact zero of a tensor the training plan exposes, so the keep mask C a pass used is read back
(helpers._ForcedMasks, dropout-aware form) and handed to the oracle through its dropout hook -- whose `D` positions are pinned
to the reference's own train() mode by tests/golden/dropout.npz (tests/test_oracle_golden.py).  With the masks equal, a dropout
pass is held to the bounds of the dropout-free tests:

  (a) logits 1e-4, every node 2e-5 * max(1, max|ref|); frames behind a short clip's end are exact zeros;
  (b) per-question CE rtol 1e-5 / atol 2e-5; every parameter gradient 2e-4 * max(max|g|, 1e-3), tensors under 64 entries
      against their family's maximum (test_full_size_gradients_are_strict_given_the_same_relu_masks);
  (c) the sites drop, and only they: C set where the oracle's pre-activation is <= 0 at fewer than 1e-4 of the sites; per site
      kind the kept fraction among the oracle's clearly positive entries within (1 - p) +- (6 sqrt(p (1 - p) / N) + 1e-4) -- a
      site that never drops reads 1.0, one that drops twice 0.5625; no exact zero at the outputs the reference does not drop;
  (d) two independent keep masks agree at p^2 + (1 - p)^2 = 0.625 of their elements: a node's `.0` / `.3` masks, elements 4k /
      4k + 1 (the generator cuts four 16-bit lanes from one hash), the same node of two questions that share program and clip,
      the same batch under seeds s and s + 1 -- each within 6 sigma of its sample size;
  (e) the same statistics on stair_dropout_fwd alone.

One HIP pass and one oracle pass per configuration, shared by its checks.  Each test prints its figures behind the tag
DROPOUT: (DESIGN.md section 4 has the table)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import nmn_oracle as O
from stair_amd import spec, synth
from helpers import _ForcedMasks

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
P = 0.25
AGREE = P * P + (1 - P) * (1 - P)                 # 0.625: two independent Bernoulli(1 - p) masks agree
WSEED, QSEED, DSEED = 3, 4, 7                     # weights, questions, dropout
RAGGED_LENS = [64, 17, 40, 64, 33, 8, 51, 64, 29, 12, 64, 45]
TINY = dict(answer_vocab_length=16, object_types=10)
SITE_KINDS = {'ToAction.param.0', 'HasItem.param.0', 'HasItem.param.3', 'Exists.param.0', 'Exists.param.3',
              'Localize.video_linear.0', 'Superlative.localize.0', 'Temporal.dense.0', 'Filter.param.0', 'Filter.param.3',
              'FilterFrame.param.0', 'FilterFrame.param.3', 'FilterFrame.dense.0', 'decoder.0'}
UNDROPPED = {'Superlative', 'Filter', 'Compare', 'Equals', 'Xor', 'ToAction'}       # outputs with a ReLU and no nn.Dropout behind it

# name -> (config, T or per-form clip lengths, matmul mode, stair_set_tile_mlp, oracle dtype)
CONFIGS = {
    'full_fused': (dict(spec.DEFAULT_CONFIG), 64, 'bf16x3', -1, torch.float64),
    'full_fused_ragged': (dict(spec.DEFAULT_CONFIG), RAGGED_LENS, 'bf16x3', -1, torch.float64),
    'full_sequenced': (dict(spec.DEFAULT_CONFIG), 64, 'bf16x3', 0, torch.float64),
    'tiny_conv_f32': (dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, max_video_length=64, **TINY), 40, 'f32', -1, torch.float64),
    'tiny_conv_bf16x3': (dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, max_video_length=64, **TINY), 40, 'bf16x3', -1, torch.float64),
    'tiny_linear_f32': (dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, max_video_length=24, **TINY), 24, 'f32', -1, torch.float64),
    'tiny_linear_bf16x3': (dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, max_video_length=24, **TINY), 24, 'bf16x3', -1, torch.float64),
    'h320_f32': (dict(spec.DEFAULT_CONFIG, hidden_size=320, video_size=128, max_video_length=40, **TINY), 33, 'f32', -1, torch.float64),
}


def _model(config, seed):
    from stair_amd.module_net import VideoNMN
    m = VideoNMN(config)
    w = synth.make_weights(config, seed)
    m.load_state_dict({k: torch.from_numpy(w[k].copy()) for k in spec.state_dict_keys(config)})
    return m.to(DEV)


def _questions(config, T):
    """24 questions: the 12 program forms, then the same 12 again -- the same program about the same clip (one array object: one
    encoder pass); under dropout nothing else is shared, each occurrence draws its own masks"""
    lens = T if isinstance(T, list) else [T] * 12
    qs = [synth.make_question(config, QSEED, i, form=f, T=lens[i]) for i, f in enumerate(synth.ALL_FORMS)]
    return qs + [dict(q) for q in qs]


def _sixsigma(n):
    return 6.0 * (AGREE * (1 - AGREE) / max(n, 1)) ** 0.5


def _agreement(pairs):
    """[(mask a, mask b, where both count)] -> (fraction of the counted elements at which a == b, their number)"""
    n = sum(int(w.sum()) for _, _, w in pairs)
    same = sum(int(((a == b) & w).sum()) for a, b, w in pairs)
    return same / max(n, 1), n


def _video_fed(program):
    """tokens whose FIRST Linear reads the encoder's frames directly: its pre-activation does not depend on any mask"""
    ch = O.children_of(program)
    feat = {'Filter': 0, 'FilterFrame': 0, 'HasItem': 0, 'Localize': 0, 'Superlative': 2}
    return [i for i, tok in enumerate(program) if tok in feat and program[ch[i][feat[tok]]] == 'video']


def _cut(got, ref):
    """a node of the launch batch ([T, H] map, [K, T] / [T] attention; T = the longest clip) cut to the question's own frames:
    (the clip's part in the oracle's shape, what lies behind it)"""
    if got.numel() == ref.numel():
        return got.reshape(ref.shape), got.new_zeros(0)
    if ref.dim() == 2 and got.shape[-1] == ref.shape[-1]:                    # map: rows are frames
        return got[:ref.shape[0]], got[ref.shape[0]:]
    Tq = ref.shape[-1]                                                      # attention: the last axis is frames
    g = got.reshape(-1, got.shape[-1])
    return g[:, :Tq].reshape(ref.shape), g[:, Tq:]


def oracle_pass(config, qs, res, dtype=torch.float64, explicit=False):
    """The mask-fed oracle over the batch (reads res.saved / res.node: call it before the pass goes backward): autograd of the
    mean decoder CE, and every figure of checks (a), (c), (d) that needs the live workspace."""
    names = [n for n, _ in spec.weight_table(config)]
    weights = synth.make_weights(config, WSEED)
    w = {k: torch.from_numpy(weights[k].copy()).to(dtype).requires_grad_(True) for k in names}
    out = dict(names=names, ce=[], logits=[], fms=[], worst_node=(0.0, ''), pad_nonzero={}, nodes=0, sites=0, flips=0, kept={}, plain_zero={})
    for qi, q in enumerate(qs):
        fm = _ForcedMasks(res, qi, q['nmn_program_list'], p=P)
        d = dict(q, video_features=torch.as_tensor(q['video_features']).to(dtype), question=torch.as_tensor(q['question']).to(dtype))
        r = fm.forward(w, config, d, return_res_by_step=False, return_result_of_each_step=True, pretrain_modules=frozenset(),
                       explicit_lstm=explicit)
        ce = torch.nn.functional.cross_entropy(r['logits'].unsqueeze(0), torch.tensor([q['answer']]))
        (ce / len(qs)).backward()
        out['ce'].append(float(ce.detach()))
        out['logits'].append(r['logits'].detach())
        for i, (_, ref) in enumerate(r['result_of_each_step']):
            if not isinstance(ref, torch.Tensor):
                continue
            ref = ref.detach()
            got, behind = _cut(res.node(qi, i).detach().cpu(), ref)
            tok = q['nmn_program_list'][i]
            err = float((got.to(dtype) - ref).abs().max()) / (2e-5 * max(1.0, float(ref.abs().max())))
            out['worst_node'] = max(out['worst_node'], (err, '%s %s[%d]' % (q['form'], tok, i)))
            out['nodes'] += 1
            if behind.numel():
                kind = tok if tok in O.ARITY else 'span'
                pn = out['pad_nonzero'].setdefault(kind, [0, 0])
                pn[0] += behind.numel()
                pn[1] += int((behind != 0).sum())
        out['sites'] += fm.sites
        out['flips'] += fm.flips
        for k, (n, kept) in fm.kept.items():
            t = out['kept'].setdefault(k, [0, 0])
            t[0] += n
            t[1] += kept
        for k, n in fm.plain_zero.items():
            out['plain_zero'][k] = out['plain_zero'].get(k, 0) + n
        out['fms'].append(fm)
    out['grads'] = {n: w[n].grad for n in names}
    # (d) mask statistics from the recorded (C, clearly positive) of every dropout call
    layers, lanes, twins = [], [], []
    half = len(qs) // 2
    for qi, fm in enumerate(out['fms']):
        for (tok, k), (m, pos) in fm.record.items():
            if (tok, k + 1) in fm.record and fm.record[(tok, k + 1)][0].shape == m.shape:
                m2, pos2 = fm.record[(tok, k + 1)]
                layers.append((m, m2, pos & pos2))
            f, fp = m.reshape(-1), pos.reshape(-1)
            n4 = f.numel() // 4 * 4
            lanes.append((f[0:n4:4], f[1:n4:4], fp[0:n4:4] & fp[1:n4:4]))
            if qi < half and qs[qi + half]['nmn_program_list'] == qs[qi]['nmn_program_list']:
                m2, pos2 = out['fms'][qi + half].record[(tok, k)]
                twins.append((m, m2, pos & pos2))
    out['agree'] = {'layers .0/.3': _agreement(layers), 'elements 4k/4k+1': _agreement(lanes), 'twin questions': _agreement(twins)}
    return out


def _first_layer_masks(res, qs):
    return {(qi, i): res.saved(qi, i, 0).detach().cpu() != 0 for qi, q in enumerate(qs) for i in _video_fed(q['nmn_program_list'])}


@functools.lru_cache(maxsize=None)
def _run(name):
    """One dropout pass of configuration `name` on the GPU -- forward, the mask-fed oracle on its workspace, backward, and a second
    forward under the next seed -- shared by the checks below."""
    from stair_amd import ops
    from stair_amd._lib import lib
    config, T, matmul, tile_mlp, dtype = CONFIGS[name]
    qs = _questions(config, T)
    ops.set_matmul_mode(matmul)
    lib.stair_set_tile_mlp(tile_mlp)
    try:
        model = _model(config, WSEED)
        for p in model.parameters():
            p.grad = torch.zeros_like(p)
        with ops.kernel_accounting() as acct:
            res = model.forward_batch(qs, train=True, dropout=(P, DSEED))
            torch.cuda.synchronize()
        out = oracle_pass(config, qs, res, dtype)
        out['hip_logits'] = res.logits.cpu()
        first = _first_layer_masks(res, qs)
        with ops.kernel_accounting() as acct_b:
            loss = res.backward(torch.tensor([q['answer'] for q in qs], dtype=torch.int32, device=DEV), 1.0 / len(qs))
            torch.cuda.synchronize()
        out['hip_ce'] = loss.cpu().numpy()
        out['hip_grads'] = {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters()}
        out['kernels'] = set(acct.table) | set(acct_b.table)
        nxt = _first_layer_masks(model.forward_batch(qs, train=True, dropout=(P, DSEED + 1)), qs)
        pairs = []
        for (qi, i), m in first.items():
            c, pos = out['fms'][qi].record[(i, 0)]
            assert torch.equal(_ForcedMasks._fit(m, c.shape), c)
            pairs.append((c, _ForcedMasks._fit(nxt[(qi, i)], c.shape), pos))
        out['agree']['seeds s/s+1'] = _agreement(pairs)
        out['fms'] = None                                  # (the recorded masks are not needed any more)
    finally:
        lib.stair_set_tile_mlp(-1)
        ops.set_matmul_mode('bf16x3')
    return out


def check_forward(tag, r, hip_logits):
    worst = max(float((hip_logits[qi].double() - lg.double()).abs().max()) for qi, lg in enumerate(r['logits']))
    print('DROPOUT: %s forward: worst logit error / 1e-4 = %.3g; worst node error / tolerance = %.3g in %s (%d nodes); frames behind '
          'a clip\'s end [entries, nonzero] by module: %s' % (tag, worst / 1e-4, r['worst_node'][0], r['worst_node'][1], r['nodes'],
                                                             r['pad_nonzero']))
    assert worst < 1e-4, worst
    assert r['worst_node'][0] < 1.0 and r['nodes'] > 150, r['worst_node']


def check_gradients(tag, r, hip_ce, hip_grads):
    grads, names = r['grads'], r['names']
    family_max = {}
    for n in names:
        if grads[n] is not None:
            fam = n.rsplit('.', 2)[0]
            family_max[fam] = max(family_max.get(fam, 0.0), float(grads[n].abs().max()))
    worst, n_checked = (0.0, ''), 0
    for n in names:
        ref = grads[n]
        if ref is None:                                   # no program of the batch reaches it
            assert float(hip_grads[n].abs().max()) == 0.0, n
            continue
        scale = float(ref.abs().max()) if ref.numel() >= 64 else family_max[n.rsplit('.', 2)[0]]
        tol = 2e-4 * max(scale, 1e-3)
        worst = max(worst, (float((hip_grads[n].to(ref.dtype) - ref).abs().max()) / tol, n))
        n_checked += 1
    ce_err = float(np.abs(np.asarray(hip_ce, dtype=np.float64) - np.asarray(r['ce'])).max())
    print('DROPOUT: %s gradients: worst error / (2e-4 max|g|) = %.3g in %s (%d tensors); worst |CE - oracle| = %.3g'
          % (tag, worst[0], worst[1], n_checked, ce_err))
    assert np.allclose(hip_ce, r['ce'], rtol=1e-5, atol=2e-5)
    assert worst[0] < 1.0 and n_checked > 90, worst


def check_sites(tag, r, kinds=SITE_KINDS):
    fr = {k: (kept / max(n, 1), n) for k, (n, kept) in sorted(r['kept'].items())}
    print('DROPOUT: %s sites: %d compared, kept where the oracle is <= 0: %d; kept fraction (N) by site kind: %s; exact zeros at '
          'undropped outputs: %s' % (tag, r['sites'], r['flips'], ', '.join('%s %.4f (%d)' % (k, f, n) for k, (f, n) in fr.items()),
                                     r['plain_zero']))
    assert r['flips'] < 1e-4 * r['sites'], (r['flips'], r['sites'])
    assert set(fr) == set(kinds), sorted(set(fr) ^ set(kinds))
    for k, (f, n) in fr.items():
        assert n >= 50 and abs(f - (1 - P)) <= 6.0 * (P * (1 - P) / n) ** 0.5 + 1e-4, (k, f, n)
    assert set(r['plain_zero']) == UNDROPPED and not any(r['plain_zero'].values()), r['plain_zero']


def check_independence(tag, r):
    print('DROPOUT: %s mask agreement (0.625 for independent masks): %s' % (
        tag, ', '.join('%s %.4f (N = %d, 6 sigma = %.4f)' % (k, a, n, _sixsigma(n)) for k, (a, n) in r['agree'].items())))
    for k, (a, n) in r['agree'].items():
        assert n > 1000 and abs(a - AGREE) <= _sixsigma(n), (k, a, n)


@pytest.mark.parametrize('name', list(CONFIGS))
def test_dropout_forward_matches_mask_fed_oracle(name):
    """(a) logits and every node; the code path the configuration is meant to reach really ran."""
    r = _run(name)
    if name.startswith('full_fused'):
        assert 'tile_mlp' in r['kernels'], sorted(r['kernels'])
    if name == 'full_sequenced':
        assert 'tile_mlp' not in r['kernels'], sorted(r['kernels'])
    check_forward(name, r, r['hip_logits'])


def test_dropout_padding_frames_of_short_clips_are_exact_zeros():
    """(a), second half: in the batch of mixed clip lengths every node's frames behind its clip's end are exact zeros (the operators
    compute whole [T, H] tiles and [T] rows; a ragged plan zeroes what lies behind each clip's end when its levels have run,
    include/stair_hip.h stair_plan_build_ragged)."""
    r = _run('full_fused_ragged')
    print('DROPOUT: full_fused_ragged frames behind a clip\'s end [entries, nonzero] by module: %s' % r['pad_nonzero'])
    assert sum(n for n, _ in r['pad_nonzero'].values()) > 100000
    assert all(nz == 0 for _, nz in r['pad_nonzero'].values()), r['pad_nonzero']


@pytest.mark.parametrize('name', list(CONFIGS))
def test_dropout_gradients_match_mask_fed_oracle(name):
    """(b) per-question CE and every parameter gradient, elementwise."""
    r = _run(name)
    check_gradients(name, r, r['hip_ce'], r['hip_grads'])


@pytest.mark.parametrize('name', list(CONFIGS))
def test_dropout_sites_drop_and_only_they(name):
    """(c) flips, kept fraction per site kind, no zeros where the reference has no nn.Dropout."""
    check_sites(name, _run(name))


@pytest.mark.parametrize('name', list(CONFIGS))
def test_dropout_masks_are_independent(name):
    """(d) layers of a node, neighbouring elements, twin questions, neighbouring seeds."""
    check_independence(name, _run(name))


def test_dropout_generator_statistics():
    """(e) stair_dropout_fwd alone on [300, 512] rows, p = 0.25: elements 4k / 4k + 1, seeds s / s + 1, sites k / k + 1."""
    from stair_amd._lib import lib, check
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = torch.randn(300, 512, device=DEV) + 3.0                       # no zeros in the input

    def keep(seed, site):
        y = x.clone()
        check(lib.stair_dropout_fwd(C.c_void_p(y.data_ptr()), 512, None, 300, 512, C.c_float(P), C.c_uint64(seed), C.c_uint32(site), stream))
        return (y != 0).cpu()
    everywhere = torch.ones(300, 512, dtype=torch.bool)
    stats = {}
    for seed, site in ((7, 3), (2 ** 40 + 5, 0xffff)):
        a = keep(seed, site)
        f = a.reshape(-1)
        stats['elements 4k/4k+1 (%d, %d)' % (seed, site)] = _agreement([(f[0::4], f[1::4], everywhere.reshape(-1)[0::4])])
        stats['seeds s/s+1 (%d, %d)' % (seed, site)] = _agreement([(a, keep(seed + 1, site), everywhere)])
        stats['sites k/k+1 (%d, %d)' % (seed, site)] = _agreement([(a, keep(seed, site + 1), everywhere)])
        stats['kept (%d, %d)' % (seed, site)] = (float(a.float().mean()), a.numel())
    print('DROPOUT: generator: %s' % ', '.join('%s %.4f (N = %d)' % (k, v, n) for k, (v, n) in stats.items()))
    for k, (v, n) in stats.items():
        if k.startswith('kept'):
            assert abs(v - (1 - P)) <= 6.0 * (P * (1 - P) / n) ** 0.5 + 1e-4, (k, v)
        else:
            assert abs(v - AGREE) <= _sixsigma(n), (k, v, n)


# ---------------------------------------------------------------------------------------------
# 6. the supervised step: Trainer.step(..., questions=...) with dropout = 0.25
# ---------------------------------------------------------------------------------------------
def _oracle_view(q):
    """class-name golds as torch tensors, as the reference's dataset hands them over"""
    q = dict(q)
    q['sg_res_by_step'] = {k: ([(n, torch.from_numpy(e)) for n, e in v] if isinstance(v, list) else v)
                           for k, v in q['sg_res_by_step'].items()}
    return q


@functools.lru_cache(maxsize=None)
def _run_supervised(matmul):
    """tests/test_gpu_train.py::test_intermediate_supervision_losses_and_gradients' set-up (tiny Conv1d configuration, the 12 golden
    questions and 12 more, golds from synth.make_gold, one contrastive window) as ONE Trainer step under dropout.  The step goes
    forward and backward in one call, so its masks are read from a replay of the forward pass under the step's seed (lr = 0: the
    weights are the step's; the replayed logits must equal the step's bit for bit)."""
    from oracle import nmn_losses as OL
    from stair_amd import losses as L, ops
    from stair_amd.train import Trainer
    from helpers import load_golden, question_for
    z, meta = load_golden('tiny_conv')
    config, T = meta['config'], meta['T']
    qs = [question_for(meta, q) for q in meta['questions']] + [synth.make_question(config, 8, 50 + i, form=f, T=T) for i, f in enumerate(synth.ALL_FORMS)]
    qs = [dict(q, sg_res_by_step=synth.make_gold(config, 3, q, T=T)) for q in qs]
    assert sum(len(q['sg_res_by_step']) for q in qs) > 40
    ops.set_matmul_mode(matmul)
    try:
        model = _model(config, WSEED)
        model.pretrain_modules = set(L.CRITERION_MODULES)
        tr = Trainer(model, lr=0.0, dropout=P, dropout_seed=DSEED, skip_untouched='window')
        video = torch.stack([torch.as_tensor(q['video_features']) for q in qs]).to(DEV)
        question = torch.cat([torch.as_tensor(q['question']) for q in qs]).to(DEV)
        progs, spans = [q['nmn_program_list'] for q in qs], [q['prog_str_to_question_tokens'] for q in qs]
        q_lens = [q['question'].shape[0] for q in qs]
        answers = torch.tensor([q['answer'] for q in qs], dtype=torch.int32, device=DEV)
        dec, res = tr.step(progs, spans, video, question, q_lens, answers, questions=qs)
        tr.check()
        out = dict(hip_ce=dec.cpu().numpy(), hip_logits=res.logits.cpu().clone(),
                   hip_module={k: v.cpu().clone() for k, v in tr.module_losses.items()},
                   hip_grads={n: p.grad.detach().cpu().clone() for n, p in model.named_parameters()})
        replay = model.run_programs(progs, spans, video, question, q_lens, train=True, dropout=(P, DSEED))
        torch.cuda.synchronize()
        assert torch.equal(replay.logits.cpu(), out['hip_logits'])
        names = [n for n, _ in spec.weight_table(config)]
        weights = synth.make_weights(config, WSEED)
        w = {k: torch.from_numpy(weights[k].copy()).requires_grad_(True) for k in names}
        fms = []

        def forward(qi, w_, config_, q, **kwargs):
            fms.append(_ForcedMasks(replay, qi, q['nmn_program_list'], p=P))
            return fms[-1].forward(w_, config_, q, **kwargs)
        total, det = OL.window_loss(w, config, [_oracle_view(q) for q in qs], L.CRITERION_MODULES, gradient_accumulation=len(qs),
                                    explicit_lstm=True, forward=forward)
        total.backward()
    finally:
        ops.set_matmul_mode('bf16x3')
    out.update(names=names, grads={n: w[n].grad for n in names}, ce=det['decoder'], det=det,
               sites=sum(f.sites for f in fms), flips=sum(f.flips for f in fms))
    return out


@pytest.mark.parametrize('matmul', ['f32', 'bf16x3'])
def test_supervised_dropout_step_matches_mask_fed_oracle(matmul):
    """Configuration 6: the per-module criteria (oracle/nmn_losses.py) evaluated on the mask-fed forward pass against
    Trainer.module_losses, and the parameter gradients of the whole window -- decoder CE plus every intermediate loss, pretrain
    heads included -- as in (b)."""
    r = _run_supervised(matmul)
    det = r['det']
    ref_mod = sorted(x[3] for x in det['module'])
    got_mod = sorted(torch.cat([v for k, v in r['hip_module'].items() if k != 'contrastive']).tolist())
    ref_c = sorted(x[3] for x in det['contrastive'])
    got_c = sorted(r['hip_module']['contrastive'].tolist())
    worst = max(abs(a - b) / (2e-6 + 2e-5 * abs(b)) for a, b in zip(got_mod + got_c, ref_mod + ref_c))
    print('DROPOUT: supervised %s criteria: %d module + %d contrastive losses, worst error / (2e-5 rel + 2e-6) = %.3g; sites %d, kept '
          'where the oracle is <= 0: %d' % (matmul, len(ref_mod), len(ref_c), worst, r['sites'], r['flips']))
    assert len(ref_mod) == len(got_mod) and np.allclose(got_mod, ref_mod, rtol=2e-5, atol=2e-6)
    assert len(ref_c) == len(got_c) > 5 and np.allclose(got_c, ref_c, rtol=2e-5, atol=2e-6)
    assert r['flips'] < 1e-4 * r['sites']
    check_gradients('supervised ' + matmul, r, r['hip_ce'], r['hip_grads'])
    assert r['grads']['submodules.Exists.pretrain_head.weight'] is not None
