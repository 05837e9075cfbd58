"""GPU tests (`-m gpu`) of the VALUE RANGE of the weight gradients: non-finite and oversized contributions through the 64-bit
fixed-point sums (csrc/common.h det_shadow, kFxScale, kFxRange; the Temporal chain's accumulators in csrc/tile_mlp.hip).

A float sum carries NaN and inf to its result; a conversion to int64 does not, and a 64-bit sum wraps.  The contract pinned here:
a gradient element that receives a NaN / inf contribution, or whose contribution or sum leaves the fixed-point range, comes out
NON-FINITE -- never finite and wrong; everything inside the range is unchanged.  The guard of stair_grad_norm, the trainer's refusal
of a non-finite step and the cooperative BPTT's "NaN into every weight gradient" all rest on it.

References are fp64 / fp32 torch autograd of the oracle (oracle/nmn_oracle.py), never the library.  "The bound" is the project's
gradient bound (test_gpu_autograd._close): 2e-4 of the reference tensor's largest entry.

  A  the Temporal chain on its own (packed, plain, full and segmented tiles)
  B  the whole reverse pass at H = 64, all 12 program forms, both matmul modes; the float-atomic path as the control
  C  the same at H = 512 (fused tile chains, grouped row-wise layers, slab products, deferred products, cooperative BPTT)
  D  the trainer: a step whose non-finite value arises INSIDE the pass is refused, an oversized one is refused or right"""
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from oracle import nmn_oracle as O
from stair_amd import spec, synth
from helpers import load_golden, question_for
import test_gpu_autograd as A
from test_gpu_autograd import matmul, f32          # noqa: F401  (fixtures: the matmul modes, restored afterwards)
import test_gpu_grad_clip as G

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the usable range of a contribution and of a sum, in gradient units: the number stated next to kFxScale
FX_RANGE = float(re.search(r'constexpr float kFxRange = ([0-9.]+)f;', open(os.path.join(ROOT, 'stair_amd', 'csrc', 'common.h')).read()).group(1))
# Whole-pass tests know a tensor's gradient, not the terms it was summed from (slab partials, per-workgroup sums), which can exceed
# the sum where they cancel.  A tensor "must be right" when its largest entry is at most 1/32 of the documented range (2^13: on the
# CPU oracle 20 / 26 / 17 tensors of tiny_conv / tiny_linear / the full-width case at 2^22), and "may be non-finite" from 2^20 on
# (beyond anything an int64 at scale 2^44 holds: 29 / 19 / 15 tensors); what lies between is unconstrained.
MUST_BE_RIGHT = FX_RANGE / 32
MAY_OVERFLOW = 2.0 ** 20
SCALE = 2.0 ** 22
REL = 2e-4


def _finite(t):
    return bool(torch.isfinite(t).all())


def _err(got, ref):
    return float((got.double().cpu() - ref.double()).abs().max())


# =============================================================================================
# A. the Temporal chain on its own
# =============================================================================================
H = 512
_CHAIN = {}


def _chain_inputs(T):
    """n = 3 instances of test_temporal_backward_chain_matches_autograd's problem (shared feature tiles: atomic accumulation)"""
    if T not in _CHAIN:
        n = 3
        g = torch.Generator().manual_seed(100 + T)
        nf = 2
        c = dict(n=n, nf=nf, feat=torch.randn(nf, T, H, generator=g), fidx=torch.randint(0, nf, (n,), generator=g, dtype=torch.int32),
                 rs=torch.rand(n + 4, T, generator=g), w=torch.randn(H, H, generator=g) / H ** 0.5, b=torch.randn(H, generator=g) * 0.1,
                 gamma=1.0 + 0.1 * torch.randn(H, generator=g), beta=0.1 * torch.randn(H, generator=g), dy=torch.randn(n + 2, T, H, generator=g))
        c['ridx'] = torch.randperm(n + 4, generator=g)[:n].to(torch.int32)
        c['yidx'] = torch.randperm(n + 2, generator=g)[:n].to(torch.int32)
        _CHAIN[T] = c
    return _CHAIN[T]


def _chain_reference(c, dy):
    """fp64 autograd of y = LayerNorm(ReLU(Lin(r_t feat_t))) against the gradient tiles dy; also the saved post-ReLU rows, and
    per (instance, 64-row segment) the terms of d gamma / d beta [n, segments, H]: the finest pieces a tile sums before converting"""
    F = c['feat'].double().requires_grad_(True); R = c['rs'].double().requires_grad_(True)
    Gm = c['gamma'].double().requires_grad_(True); Bt = c['beta'].double().requires_grad_(True)
    z = (R[c['ridx'].long()].unsqueeze(-1) * F[c['fidx'].long()]) @ c['w'].double().t() + c['b'].double()
    z.retain_grad()
    a = torch.relu(z)
    y = torch.nn.functional.layer_norm(a, (H,), Gm, Bt, 1e-5)
    d = dy[c['yidx'].long()].double()
    (y * d).sum().backward()
    xhat = torch.nn.functional.layer_norm(a.detach(), (H,), None, None, 1e-5)
    T = a.shape[1]
    segs = [(f0, min(f0 + 64, T)) for f0 in range(0, T, 64)]
    tg = torch.stack([(d[:, f0:f1] * xhat[:, f0:f1]).sum(1) for f0, f1 in segs], 1)
    tb = torch.stack([d[:, f0:f1].sum(1) for f0, f1 in segs], 1)
    return dict(a=a.detach().float(), dz=z.grad, dfeat=F.grad, drs=R.grad, dgamma=Gm.grad, dbeta=Bt.grad, terms=dict(dgamma=tg, dbeta=tb))


def _chain_run(c, dy, a_saved):
    from stair_amd import ops
    d = lambda t: t.to(DEV)
    n, T = c['n'], dy.shape[1]
    out = dict(dfeat=torch.zeros(c['nf'], T, H, device=DEV), drs=torch.zeros(n + 4, T, device=DEV), dgamma=torch.zeros(H, device=DEV),
               dbeta=torch.zeros(H, device=DEV))
    out['dz'] = ops.tile_temporal_bwd(d(dy), d(a_saved), d(c['gamma']), d(c['w']), d(c['feat']), d(c['rs']), out['dfeat'], out['drs'],
                                      out['dgamma'], out['dbeta'], dy_idx=d(c['yidx']), feat_idx=d(c['fidx']), rs_idx=d(c['ridx']),
                                      dfeat_idx=d(c['fidx']), exclusive=False)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _float_paths(got, ref, bad):
    """dZ, d feat, d r are plain float paths, and rows do not mix: non-finite wherever the reference is, finite and within the bound
    wherever it is not"""
    for k in ('dz', 'dfeat', 'drs'):
        nf = ~torch.isfinite(ref[k])
        if bool(torch.isfinite(got[k][nf]).any()):
            bad.append((k, 'finite where the reference is not', int(torch.isfinite(got[k][nf]).sum())))
        fin = ~nf
        if not _finite(got[k][fin]):
            bad.append((k, 'non-finite where the reference is finite', int((~torch.isfinite(got[k][fin])).sum())))
            continue
        tol = REL * float(ref[k][fin].abs().max())
        e = _err(got[k][fin], ref[k][fin])
        if not e < tol:
            bad.append((k, e, tol))


@pytest.mark.parametrize('T', [8, 33, 64, 100])
@pytest.mark.parametrize('variant', ['nan', 'inf_row'])
def test_temporal_chain_poison(T, variant):
    """One NaN element / one whole +inf row in the gradient tiles: per COLUMN of d gamma / d beta, non-finite in the fp64 reference
    -> non-finite in the result, every other column finite and within the bound.  T = 8: three clips packed into one tile; 33: a
    partly filled tile; 64: full tiles; 100: two segments per clip, the poisoned row in the second."""
    c = _chain_inputs(T)
    dy = c['dy'].clone()
    if variant == 'nan':
        dy[int(c['yidx'][1]), T // 2, 77] = float('nan')
    else:
        dy[int(c['yidx'][0]), T - 1, :] = float('inf')
    ref = _chain_reference(c, dy)
    got = _chain_run(c, dy, ref['a'])
    bad = []
    for k in ('dgamma', 'dbeta'):
        nf = ~torch.isfinite(ref[k])
        assert int(nf.sum()) == (1 if variant == 'nan' else H), k          # the case is what it claims to be
        hidden = nf & torch.isfinite(got[k])
        if bool(hidden.any()):
            cols = hidden.nonzero().flatten().tolist()
            bad.append((k, '%d non-finite columns came out finite' % len(cols), cols[:4], got[k][hidden][:4].tolist()))
        fin = ~nf
        if bool(fin.any()):
            if not _finite(got[k][fin]):
                bad.append((k, 'non-finite columns beside the poisoned ones', int((~torch.isfinite(got[k][fin])).sum())))
            else:
                tol = REL * float(ref[k][fin].abs().max())
                e = _err(got[k][fin], ref[k][fin])
                if not e < tol:
                    bad.append((k, e, tol))
    _float_paths(got, ref, bad)
    print('T=%d %s:' % (T, variant), bad)
    assert not bad, bad


@pytest.mark.parametrize('T', [8, 33, 64, 100])
@pytest.mark.parametrize('variant', ['scaled', 'scaled_edge'])
def test_temporal_chain_scaled(T, variant):
    """dy times 2^k (exact in fp64, so the reference is the unscaled one times 2^k).  'scaled': k puts the largest reference |d gamma|
    into [2^21, 2^22); 'scaled_edge': 16 times less, so that columns on both sides of the range exist.
    Per column, from the reference's own terms (the sums over an instance's 64-row segment, the finest pieces a tile converts): when
    the terms' magnitudes add up to less than the range, every partial sum of every grouping is inside it -> the column is finite and
    within the bound; every other column -- all whose reference exceeds 2^20 among them -- is within the bound or NON-FINITE.
    (Asking every column up to 2^20 to be right is not possible: at scale 2^44 an int64 ends at 2^19.  What the contract promises is
    asked: right inside the documented range, never finite and wrong outside it.)"""
    c = _chain_inputs(T)
    base = _chain_reference(c, c['dy'])
    k = math.ceil(math.log2(2.0 ** 21 / float(base['dgamma'].abs().max()))) - (4 if variant == 'scaled_edge' else 0)
    s = 2.0 ** k
    top = s * float(base['dgamma'].abs().max())
    assert (2.0 ** 21 <= top < 2.0 ** 22) if variant == 'scaled' else (2.0 ** 17 <= top < 2.0 ** 18)
    got = _chain_run(c, c['dy'] * s, base['a'])
    ref = {k_: v * s for k_, v in base.items() if k_ not in ('a', 'terms')}
    bad, counts = [], {}
    for k_ in ('dgamma', 'dbeta'):
        reach = s * base['terms'][k_].abs().sum(dim=(0, 1))               # [H]: sum of the terms' magnitudes
        must = reach < 0.999 * FX_RANGE                                    # (the kernel's terms are float sums: a hair of margin)
        tol = REL * float(ref[k_].abs().max())
        err = (got[k_].double() - ref[k_]).abs()
        fin = torch.isfinite(got[k_])
        wrong_inside = must & ~(fin & (err < tol))
        wrong_outside = ~must & fin & ~(err < tol)
        counts[k_] = dict(must=int(must.sum()), beyond_2_20=int((ref[k_].abs() > MAY_OVERFLOW).sum()), non_finite=int((~fin).sum()))
        if bool(wrong_inside.any()):
            i = wrong_inside.nonzero().flatten()
            bad.append((k_, '%d columns inside the range are wrong' % len(i), got[k_][i][:4].tolist(), ref[k_][i][:4].tolist()))
        if bool(wrong_outside.any()):
            i = wrong_outside.nonzero().flatten()
            bad.append((k_, '%d columns outside the range are finite and wrong (%d of them beyond 2^20)' %
                        (len(i), int((ref[k_][i].abs() > MAY_OVERFLOW).sum())), got[k_][i][:4].tolist(), ref[k_][i][:4].tolist()))
    if variant == 'scaled':
        assert counts['dgamma']['beyond_2_20'] >= 1
    else:
        assert counts['dgamma']['must'] + counts['dbeta']['must'] >= 1
    _float_paths(got, ref, bad)
    print('T=%d %s, 2^%d:' % (T, variant, k), counts, bad)
    assert not bad, bad


# =============================================================================================
# B, C. the whole reverse pass
# =============================================================================================
_CASES = {}


def _case(key):
    """(config, weight seed, questions, R) of a whole-pass case, made once"""
    if key not in _CASES:
        if key in ('tiny_conv', 'tiny_linear'):
            z, meta = load_golden(key)
            config, seed = meta['config'], meta['seed']
            qs = [question_for(meta, q) for q in meta['questions']]
            assert qs[0]['form'] == 'P0' and qs[5]['form'] == 'P5'
        else:                                               # test_custom_loss_on_odd_shapes's (512, 40, 33), 12 or 24 clips
            config = dict(spec.DEFAULT_CONFIG, hidden_size=512, video_size=128, answer_vocab_length=16, max_video_length=40, object_types=10)
            seed, qs = 1, synth.make_questions(config, 5, {'wide': 12, 'wide24': 24}[key], forms=synth.ALL_FORMS, T=33)
        _CASES[key] = (config, seed, qs, A._R(len(qs), config['answer_vocab_length']))
    return _CASES[key]


_ORACLE = {}


def _oracle_grads(key, which, poison=None):
    """Oracle parameter gradients {name: tensor or None} of the custom loss over the questions `which` of a case (a tuple of
    indices), with R[i, 3] = value for poison = (i, value), i counting within `which`; computed once and left unchanged."""
    k = (key, which, None if poison is None else (poison[0], repr(poison[1])))
    if k not in _ORACLE:
        config, seed, qs, R = _case(key)
        idx = list(which)
        R = R[idx].clone()
        if poison is not None:
            R[poison[0], 3] = poison[1]
        names, w, _, _ = A._oracle(config, seed, [qs[i] for i in idx], R)
        _ORACLE[k] = {n: (None if w[n].grad is None else w[n].grad.detach().clone()) for n in names}
    return _ORACLE[k]


def _run(key, R):
    """the library's parameter gradients of the custom loss through VideoNMN.logits, as CPU tensors (None: untouched)"""
    config, seed, qs, _ = _case(key)
    model = A._model(config, seed)
    progs, spans, video, question, q_lens, _ = A._pack(qs)
    logits = model.logits(progs, spans, video, question, q_lens)
    A._custom(logits, R.to(DEV)).backward()
    torch.cuda.synchronize()
    return {n: (None if p.grad is None else p.grad.detach().cpu()) for n, p in model.named_parameters()}


def _right(got, ref, name, bad, rel=REL, scale=1.0):
    """finite and within the bound of the (scaled) reference; a tensor without a reference gradient stays untouched"""
    if ref is None:
        if got is not None and float(got.abs().max()) != 0.0:         # (nan != 0.0 as well)
            bad.append((name, 'untouched in the oracle', float(got.abs().max())))
        return
    if got is None or not _finite(got):
        bad.append((name, 'missing' if got is None else 'non-finite where the oracle is finite'))
        return
    tol = rel * scale * max(float(ref.abs().max()), 1e-3)        # (the project's bound, floor included, is linear in the loss scale)
    e = _err(got, ref * scale)
    if not e < tol:
        bad.append((name, e, tol))


def _poison_check(key, q, value, rel=REL, l2=None):
    """R[q, 3] = value.  By linearity of the sum over questions the oracle of the poisoned question ALONE tells which tensors it
    reaches (a gradient at all) and which of those are non-finite; the others' gradients are the oracle of the remaining questions.
      every tensor that is non-finite in the oracle is non-finite in the result;
      every tensor the poisoned question does not reach is finite and within the bound of the other questions' gradient.
    A reached tensor whose oracle gradient is finite is not asserted finite: torch SELECTS where the kernels multiply by a 0/1 mask,
    and 0 * inf differs between them.  The other way round: a tensor whose gradient from the CLEAN question is exactly zero has a
    derivative that is zero whatever arrives from above -- Filter's attention Linear feeds a softmax over ONE element in the forms
    with a single keyword -- and the oracle's NaN there is 0 * NaN.  The library does not run that product at all
    (test_gpu_autograd._check_params accepts its exact zero), and no value is hidden by it: such tensors are not required to be
    non-finite (2 of the 50 at q = 0, none at q = 5)."""
    config, seed, qs, R = _case(key)
    others = tuple(i for i in range(len(qs)) if i != q)
    alone = _oracle_grads(key, (q,), (0, value))             # (the lone question is row 0 of its own R)
    rest = _oracle_grads(key, others)
    reached = {n for n, g in alone.items() if g is not None}
    clean = _oracle_grads(key, (q,))
    dead = {n for n in reached if float(clean[n].abs().max()) == 0.0}
    nonfinite = {n for n in reached if not _finite(alone[n])} - dead
    assert len(nonfinite) >= 30, (len(nonfinite), len(reached))            # (checked on the CPU: 50 to 54 at H = 64, 36 at H = 512)
    Rp = R.clone(); Rp[q, 3] = value
    got = _run(key, Rp)
    hidden, bad = [], []
    for n in alone:
        if n in nonfinite:
            if got[n] is None or _finite(got[n]):
                hidden.append((n, None if got[n] is None else float(got[n].abs().max())))
        elif n not in reached:
            if l2 is None:
                _right(got[n], rest[n], n, bad, rel)
            elif rest[n] is not None:                        # (full width, split products: the project's L2 criterion)
                if got[n] is None or not _finite(got[n]) or not float((got[n] - rest[n]).norm() / rest[n].norm().clamp_min(1e-12)) < l2:
                    bad.append((n, 'outside the L2 bound'))
    print('%s q=%d %r: %d of %d reached tensors non-finite in the oracle; came out finite: %d %s; unreached tensors wrong: %s' %
          (key, q, value, len(nonfinite), len(reached), len(hidden), hidden[:6], bad))
    assert not hidden and not bad, (hidden, bad)


def _scale_check(key):
    """R times 2^22 (the fp32 oracle is exactly linear in a power of two and stays finite).  Per tensor, by S * max|ref|:
    at most MUST_BE_RIGHT: finite and within the bound; from 2^20 on: within the bound or containing a non-finite element; in
    between: unconstrained.  A tensor whose reference is all zero stays exactly zero."""
    config, seed, qs, R = _case(key)
    ref = _oracle_grads(key, tuple(range(len(qs))))
    got = _run(key, R * SCALE)
    bad, cnt = [], dict(must=0, may=0, between=0)
    for n, r in ref.items():
        top = 0.0 if r is None else SCALE * float(r.abs().max())
        if r is None:
            _right(got[n], None, n, bad)
        elif top == 0.0:
            if got[n] is None or float(got[n].abs().max()) != 0.0:
                bad.append((n, 'all zero in the oracle'))
        elif top <= MUST_BE_RIGHT:
            cnt['must'] += 1
            _right(got[n], r, n, bad, scale=SCALE)
        elif top >= MAY_OVERFLOW:
            cnt['may'] += 1
            if got[n] is None:
                bad.append((n, 'missing'))
            elif _finite(got[n]):
                tol = REL * top
                e = _err(got[n], r * SCALE)
                if not e < tol:
                    bad.append((n, 'finite and wrong', e, tol, top))
        else:
            cnt['between'] += 1
    print(key, 'x 2^22:', cnt, bad)
    assert cnt['must'] >= 10 and cnt['may'] >= 10, cnt
    assert not bad, bad


@pytest.mark.parametrize('value', [float('nan'), float('inf')], ids=['nan', 'inf'])
@pytest.mark.parametrize('q', [0, 5])
@pytest.mark.parametrize('name', ['tiny_conv', 'tiny_linear'])
def test_reverse_pass_poison(name, q, value, matmul):
    _poison_check(name, q, value)


@pytest.mark.parametrize('name', ['tiny_conv', 'tiny_linear'])
def test_reverse_pass_scaled(name, matmul):
    _scale_check(name)


def test_full_width_poison(f32):
    """H = 512, L = 40, T = 33, exact products: the fused tile chains, the grouped row-wise layers, the slab products and the
    per-weight deferred products run here"""
    _poison_check('wide', 0, float('nan'))


def test_full_width_scaled(f32):
    _scale_check('wide')


def test_full_width_cooperative_poison():
    """24 clips in the default (split) mode: the cooperative recurrences run -- their hand-offs go through flag words with bounded
    spins, NaN values are ordinary data there -- and the NaN survives them.  Split products at this width are held to the project's
    L2 criterion of test_full_size_backward_sample (1e-2), not the elementwise bound."""
    from stair_amd import ops
    with ops.kernel_accounting() as acct:
        _poison_check('wide24', 0, float('nan'), l2=1e-2)
    coop = sorted(k for k in acct.table if k.startswith('lstm_bwd_coop'))      # (lstm_bwd_coop_pair: both encoders' BPTT in one launch)
    print('cooperative BPTT launches:', {k: acct.table[k][0] for k in coop})
    assert coop, sorted(acct.table)



def test_float_atomic_control_in_a_fresh_process():
    """STAIR_DETERMINISTIC=0 (read once per process): every gradient sum is a float atomic, which carries NaN and inf by itself.  The
    poison cases of this file must pass there whatever the fixed-point conversion does: the control of the cases, not of the code."""
    env = dict(os.environ, STAIR_DETERMINISTIC='0')
    cmd = [sys.executable] + (['-s'] if sys.flags.no_user_site else []) + ['-m', 'pytest', os.path.abspath(__file__), '-q', '-m', 'gpu', '-k', 'poison',
                                                                            '-p', 'no:cacheprovider']
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert re.search(r'\b\d+ passed', r.stdout) and ' failed' not in r.stdout and ' skipped' not in r.stdout, r.stdout[-500:]


# =============================================================================================
# D. the trainer
# =============================================================================================
def _trainer(config, supervised, **kw):
    from stair_amd import losses as L
    from stair_amd.train import Trainer
    model = G._model(config, 0)
    if supervised:
        model.pretrain_modules = set(L.CRITERION_MODULES)
    return Trainer(model, lr=G.LR, dropout=0.0, **kw)


def _window_args(config, qs, supervised):
    if not supervised:
        return G._pack(qs), {}
    gold = []
    for q in qs:
        q = dict(q)
        q['sg_res_by_step'] = synth.make_gold(config, 3, q, T=40)
        gold.append(q)
    assert sum(len(q['sg_res_by_step']) for q in gold) > 0
    return G._pack(gold), dict(questions=gold)


@pytest.mark.parametrize('supervised', [False, True], ids=['decoder_only', 'supervised'])
def test_trainer_refuses_poisoned_features(supervised):
    """One +inf among one clip's features -- a corrupted feature file: the non-finite values arise INSIDE the passes and reach the
    gradient bucket through the kernels' own sums, not through the test hook behind them.  Supervised: launch_module_losses opens
    the shadow scope early and the criteria heads add through it.  Everything test_nonfinite_step_is_refused_and_named asserts."""
    from stair_amd._lib import StairError
    z, meta = load_golden('tiny_conv')
    config = meta['config']
    windows = G._windows(config)
    tr = _trainer(config, supervised, max_grad_norm=float('inf'))
    args, kw = _window_args(config, windows[0], supervised)
    tr.step(*args, **kw)
    tr.check()
    before = [t.clone() for t in (tr.flat_p, tr.exp_avg, tr.exp_avg_sq, tr.steps, tr.touched)]
    assert float(tr.steps.max()) == 1.0
    args, kw = _window_args(config, windows[1], supervised)
    bad = list(args)
    bad[2] = args[2].clone()
    bad[2][1, 17, 5] = float('inf')
    tr.step(*bad, **kw)
    torch.cuda.synchronize()
    print('non-finite entries of the gradient bucket:', int((~torch.isfinite(tr.flat_g)).sum()), 'of', tr.flat_g.numel(), 'guard', int(tr.guard))
    for a, b in zip(before, (tr.flat_p, tr.exp_avg, tr.exp_avg_sq, tr.steps, tr.touched)):
        assert torch.equal(a, b)
    assert int(tr.guard) == 2
    assert not math.isfinite(float(tr.grad_norm[0]))
    with pytest.raises(StairError) as err:
        tr.check()
    assert 'non-finite gradient norm in optimizer step 1' in str(err.value) and 'recurrence' not in str(err.value)
    tr.step(*args, **kw)                                      # the caller goes on: a healthy step applies
    tr.check()
    assert int(tr.guard) == 0 and float(tr.steps.max()) == 2.0 and not torch.equal(tr.flat_p, before[0])
    assert math.isfinite(float(tr.grad_norm[0])) and float(tr.grad_norm[0]) > 0
    assert bool(tr.flat_p.isfinite().all()) and bool(tr.exp_avg.isfinite().all()) and bool(tr.exp_avg_sq.isfinite().all())


_BIG = {}


def _oracle_big_step():
    """clip_grad_norm_(1.0) + Adam on the oracle for one window whose decoder loss weighs 2^22 * G (fp32: finite), computed once"""
    if not _BIG:
        z, meta = load_golden('tiny_conv')
        config = meta['config']
        names = [n for n, _ in spec.weight_table(config)]
        wts = synth.make_weights(config, 0)
        w = {k: torch.from_numpy(wts[k].copy()).requires_grad_(True) for k in names}
        opt = torch.optim.Adam([w[n] for n in names], lr=G.LR)
        qs = G._windows(config)[1]
        total = 0.0
        for q in qs:
            logits = O.forward(w, config, q, return_res_by_step=False, explicit_lstm=True)['logits']
            total = total + torch.nn.functional.cross_entropy(logits.unsqueeze(0), torch.tensor([q['answer']])) * SCALE
        total.backward()
        grads = {n: (None if w[n].grad is None else w[n].grad.detach().clone()) for n in names}
        assert all(_finite(g) for g in grads.values() if g is not None)
        norm = float(torch.nn.utils.clip_grad_norm_([w[n] for n in names], 1.0))
        coef = float(torch.clamp(1.0 / (torch.tensor(norm, dtype=torch.float32) + 1e-6), max=1.0))
        opt.step()
        _BIG.update(config=config, names=names, grads=grads, norm=norm, coef=coef,
                    exp_avg={n: opt.state[w[n]]['exp_avg'].clone() for n in names if w[n] in opt.state},
                    final={n: w[n].detach().clone() for n in names})
    return _BIG


def test_trainer_oversized_step_is_refused_or_right(matmul):
    """decoder_loss_weight = 2^22 * G with max_grad_norm = 1: gradients up to ~1e7, far outside the fixed-point range.  The step is
    either refused, with everything test_nonfinite_step_is_refused_and_named asserts of a refused step, or what it applied is
    clip-then-Adam on the oracle gradient, by the comparison of test_clipped_steps_match_torch_clip_then_adam."""
    from stair_amd._lib import StairError
    ora = _oracle_big_step()
    config, names = ora['config'], ora['names']
    tr = _trainer(config, False, scheduler_total_iters=10, skip_untouched='ever', max_grad_norm=1.0)
    model = tr.model
    qs = G._windows(config)[1]
    before = [t.clone() for t in (tr.flat_p, tr.exp_avg, tr.exp_avg_sq, tr.steps, tr.touched)]
    tr.decoder_loss_weight = SCALE * len(qs)
    tr.step(*G._pack(qs))
    torch.cuda.synchronize()
    norm, coef = (float(x) for x in tr.grad_norm.cpu())
    print('guard %d, norm %.7g (oracle %.7g), coefficient %.7g (oracle %.7g), largest oracle entry %.3g' %
          (int(tr.guard), norm, ora['norm'], coef, ora['coef'], max(float(g.abs().max()) for g in ora['grads'].values() if g is not None)))
    if int(tr.guard) != 0:
        assert int(tr.guard) == 2 and not math.isfinite(norm)
        for a, b in zip(before, (tr.flat_p, tr.exp_avg, tr.exp_avg_sq, tr.steps, tr.touched)):
            assert torch.equal(a, b)
        with pytest.raises(StairError) as err:
            tr.check()
        assert 'non-finite gradient norm in optimizer step 0' in str(err.value)
        return
    tr.check()
    bound = math.sqrt(sum(g.numel() * G._tol(g) ** 2 for g in ora['grads'].values() if g is not None))
    assert abs(norm - ora['norm']) <= bound, (norm, ora['norm'], bound)
    offs = dict(zip(model._weight_names, tr.offsets))
    for n, ref in ora['exp_avg'].items():
        g_ref = ora['grads'][n]
        if g_ref is None:
            continue
        got = tr.exp_avg[offs[n]: offs[n] + ref.numel()].view_as(ref).cpu()
        tol = G._tol(g_ref) * (1 - G.B1) * ora['coef']
        assert float((got - ref).abs().max()) <= tol, (n, float((got - ref).abs().max()), tol)
    got = dict(model.named_parameters())
    for n in names:
        diff = (got[n].detach().cpu() - ora['final'][n]).abs()
        if matmul == 'f32':
            assert float(diff.max()) < 2e-5, (n, float(diff.max()))
        else:
            assert float((diff < 2e-5).float().mean()) > 0.995, (n, float((diff < 2e-5).float().mean()))
            assert float(diff.max()) < 2.5e-4, (n, float(diff.max()))
