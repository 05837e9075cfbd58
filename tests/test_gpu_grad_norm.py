"""GPU tests (`-m gpu`) of stair_grad_norm and stair_adam_step_scaled through the C ABI, no model: per-tensor and global
gradient norms of a flat bucket, the clip coefficient, the non-finite bit of the guard word, and Adam with the coefficient
applied inside the kernel against torch.optim.Adam + torch.nn.utils.clip_grad_norm_ on CPU fp32.

Gradients are randn x s with s per segment in [1e-3, 1e3] (squares stay out of the fp32 subnormals); the padding between a
segment's element count and the end of its last 256-float block is NaN in EVERY case, so a kernel that looks at it fails.
The reference is the sum of squares in torch fp64 over the real elements only.

Bound on the norms, 2e-6 relative: at most 11 fp32 roundings enter a block partial (1 square, 3 in-lane adds, 6 butterfly
levels, 1 store; the compiler may fuse a square into its add, which only removes roundings), so a block's sum of squares is
within 11 x 6e-8 = 6.6e-7; everything above the block partial is fp64.  sqrt halves that and the final fp32 rounding adds 6e-8:
3.9e-7 worst case, 2e-6 is about 4 x that."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEG = 256
NORM_RTOL = 2e-6


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Flat:
    """Segments of `numels` floats on 256-float blocks; segment i lies at memory position mem_pos[i] (a permutation)."""

    def __init__(self, numels, mem_pos=None, tail_blocks=0):
        mem_pos = list(range(len(numels))) if mem_pos is None else mem_pos
        assert sorted(mem_pos) == list(range(len(numels)))
        blocks = [(m + SEG - 1) // SEG for m in numels]
        self.numels, self.first = list(numels), [0] * len(numels)
        total = 0
        for pos in range(len(numels)):
            i = mem_pos.index(pos)
            self.first[i] = total
            total += blocks[i]
        self.n = (total + tail_blocks) * SEG
        self.first_d = torch.tensor(self.first, dtype=torch.int32, device=DEV)
        self.numel_d = torch.tensor(self.numels, dtype=torch.int64, device=DEV)
        self.seg_of_block = torch.zeros(self.n // SEG, dtype=torch.int32)
        for i, (f, b) in enumerate(zip(self.first, blocks)):
            self.seg_of_block[f: f + b] = i
        self.seg_of_block = self.seg_of_block.to(DEV)

    def fill(self, values, pad=float('nan')):
        """flat fp32 buffer (CPU) holding values[i] in segment i and `pad` everywhere else"""
        flat = torch.full((self.n,), pad, dtype=torch.float32)
        for v, f in zip(values, self.first):
            flat[f * SEG: f * SEG + v.numel()] = v
        return flat

    def random(self, seed):
        g = torch.Generator().manual_seed(seed)
        out = []
        for m in self.numels:
            s = 10.0 ** float(torch.empty(1).uniform_(-3, 3, generator=g))
            out.append(torch.randn(m, generator=g) * s)
        return out


def _reference(values):
    sq = [float((v.double() ** 2).sum()) for v in values]
    return [math.sqrt(x) for x in sq], math.sqrt(sum(sq))


def _grad_norm(flat, grads_cpu, max_norm=float('inf'), guard=0):
    from stair_amd._lib import check, lib
    g = grads_cpu.to(DEV)
    scratch = torch.full((flat.n // SEG,), float('nan'), device=DEV)
    seg_norm = torch.full((len(flat.numels),), -1.0, device=DEV)
    out = torch.full((2,), -1.0, device=DEV)
    guard_d = torch.tensor([guard], dtype=torch.int32, device=DEV)
    check(lib.stair_grad_norm(P(g), flat.n, P(flat.first_d), P(flat.numel_d), len(flat.numels), C.c_float(max_norm), P(scratch),
                              P(seg_norm), P(out), P(guard_d), _stream()))
    torch.cuda.synchronize()
    return seg_norm.cpu(), out.cpu(), int(guard_d.cpu()[0])


def _torch_coef(norm_f32, max_norm):
    """clip_grad_norm_'s own expression on an fp32 tensor (torch/nn/utils/clip_grad.py)"""
    clip_coef = max_norm / (norm_f32 + 1e-6)
    return torch.clamp(clip_coef, max=1.0)


def _check_norms(flat, values, seg_norm, out):
    ref_seg, ref_total = _reference(values)
    print('global norm %.9g (fp64 %.9g, rel. error %.3g)' % (float(out[0]), ref_total, abs(float(out[0]) - ref_total) / ref_total))
    worst = 0.0
    for i, r in enumerate(ref_seg):
        worst = max(worst, abs(float(seg_norm[i]) - r) / r)
        assert abs(float(seg_norm[i]) - r) <= NORM_RTOL * r, (i, float(seg_norm[i]), r)
    print('worst per-segment rel. error %.3g' % worst)
    assert abs(float(out[0]) - ref_total) <= NORM_RTOL * ref_total, (float(out[0]), ref_total)


CASES = {
    'one_element': ([1], None),
    'mixed_permuted': ([1, 255, 256, 257, 1000, 64 * 256 + 3, 70000], [3, 6, 0, 5, 1, 4, 2]),
    'many_small': ([7] * 300, [(i * 7) % 300 for i in range(300)]),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_norms_match_fp64_over_the_real_elements(case):
    numels, mem_pos = CASES[case]
    flat = Flat(numels, mem_pos)
    if case == 'one_element':
        assert flat.n == 256
    values = flat.random(3)
    seg_norm, out, guard = _grad_norm(flat, flat.fill(values))
    _check_norms(flat, values, seg_norm, out)
    assert float(out[1]) == 1.0 and guard == 0


def test_large_buffer_is_bit_reproducible():
    """2^22 + 256 floats in two segments (16384 block partials in one segment: every thread of the final workgroup takes
    several), run twice on fresh outputs."""
    flat = Flat([(1 << 22) - 3, 100])
    assert flat.n == (1 << 22) + 256
    values = flat.random(5)
    grads = flat.fill(values)
    a = _grad_norm(flat, grads, max_norm=1.0)
    b = _grad_norm(flat, grads, max_norm=1.0)
    _check_norms(flat, values, a[0], a[1])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])          # bit for bit
    assert float(a[1][1]) < 1.0


def test_clip_coefficient_is_torchs_expression_exactly():
    flat = Flat([1, 255, 256, 257, 1000, 64 * 256 + 3, 70000], [3, 6, 0, 5, 1, 4, 2])
    grads = flat.fill(flat.random(7))
    _, out, _ = _grad_norm(flat, grads)
    norm = float(out[0])
    assert float(out[1]) == 1.0                                          # max_norm = +inf
    seen = set()
    for max_norm in (0.1 * norm, 0.5 * norm, norm * (1 - 1e-7), norm, norm * (1 + 2e-6), 2.0 * norm, 1.2345, float('inf')):
        _, o, _ = _grad_norm(flat, grads, max_norm=max_norm)
        assert float(o[0]) == norm
        want = _torch_coef(o[0], float(torch.tensor(max_norm, dtype=torch.float32)))
        assert want.dtype == torch.float32
        assert float(o[1]) == float(want), (max_norm, float(o[1]), float(want))
        seen.add(float(o[1]) < 1.0)
    assert seen == {True, False}
    zeros = flat.fill([torch.zeros(m) for m in flat.numels])
    seg_norm, o, guard = _grad_norm(flat, zeros, max_norm=0.5)
    assert float(o[0]) == 0.0 and float(o[1]) == 1.0 and guard == 0 and float(seg_norm.abs().max()) == 0.0


def test_argument_checks():
    from stair_amd._lib import lib
    flat = Flat([300, 7])
    g = torch.zeros(flat.n + 4, device=DEV)
    scratch, seg_norm, out = torch.zeros(flat.n // SEG, device=DEV), torch.zeros(2, device=DEV), torch.zeros(2, device=DEV)
    call = lambda gp, n, mn, outp=P(out): lib.stair_grad_norm(gp, n, P(flat.first_d), P(flat.numel_d), 2, C.c_float(mn), P(scratch),
                                                             P(seg_norm), outp, None, _stream())
    assert call(P(g), flat.n, 1.0) == 0                                   # a null guard is allowed
    assert call(P(g), flat.n - 1, 1.0) != 0                               # n % 256
    assert call(C.c_void_p(g.data_ptr() + 4), flat.n, 1.0) != 0           # alignment
    assert call(None, flat.n, 1.0) != 0 and call(P(g), flat.n, 1.0, None) != 0
    assert call(P(g), flat.n, 0.0) != 0 and call(P(g), flat.n, -1.0) != 0 and call(P(g), flat.n, float('nan')) != 0
    assert b'stair_grad_norm' in lib.stair_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize('bad', [float('inf'), float('nan')])
def test_nonfinite_gradient_sets_bit_1_of_the_guard(bad):
    flat = Flat([1, 255, 256, 257, 1000, 64 * 256 + 3, 70000], [3, 6, 0, 5, 1, 4, 2])
    values = flat.random(11)
    good = flat.fill(values)
    values[4][500] = bad                                                  # a middle segment, a middle block
    poisoned = flat.fill(values)
    assert _grad_norm(flat, good, guard=0)[2] == 0
    assert _grad_norm(flat, good, guard=1)[2] == 1
    assert _grad_norm(flat, poisoned, guard=0)[2] == 2
    assert _grad_norm(flat, poisoned, guard=1)[2] == 3
    seg_norm, out, _ = _grad_norm(flat, poisoned, max_norm=1.0)
    assert not math.isfinite(float(out[0])) and not math.isfinite(float(seg_norm[4]))
    ref_seg, _ = _reference(values)
    for i in (0, 1, 2, 3, 5, 6):                                          # the other tensors' norms are still theirs
        assert abs(float(seg_norm[i]) - ref_seg[i]) <= NORM_RTOL * ref_seg[i], i


# ---- stair_adam_step_scaled ------------------------------------------------------------------------------------------------------

ADAM_NUMELS, ADAM_POS, UNTOUCHED = [300, 256, 1000, 7, 513], [2, 0, 4, 1, 3], 3
LR, B1, B2, EPS, MAX_NORM = 1e-3, 0.9, 0.999, 1e-8, 1.0
STEP_NORMS = (10.0, 0.5, 1.0 / 0.9)                                       # coefficients ~0.1, exactly 1, ~0.9


def _adam(flat, p, g, m, v, touched, steps, guard, scale, scaled_entry=True, weight_decay=0.0):
    from stair_amd._lib import check, lib
    args = (P(p), P(g), P(m), P(v), P(flat.seg_of_block), P(touched), P(steps), C.c_float(LR), C.c_float(B1), C.c_float(B2),
            C.c_float(EPS), C.c_float(weight_decay), flat.n, P(guard))
    if scaled_entry:
        check(lib.stair_adam_step_scaled(*args, P(scale), _stream()))
    else:
        check(lib.stair_adam_step(*args, _stream()))


def _adam_problem():
    flat = Flat(ADAM_NUMELS, ADAM_POS)
    gen = torch.Generator().manual_seed(21)
    params = [torch.empty(m).uniform_(-1, 1, generator=gen) for m in ADAM_NUMELS]
    grads = []
    for norm in STEP_NORMS:
        gs = [torch.randn(m, generator=gen) for m in ADAM_NUMELS]
        gs[UNTOUCHED] = torch.zeros(ADAM_NUMELS[UNTOUCHED])
        total = math.sqrt(sum(float((x.double() ** 2).sum()) for x in gs))
        grads.append([x * (norm / total) for x in gs])
    return flat, params, grads


def _scaled_adam_against_torch(weight_decay):
    """Three steps of stair_grad_norm + stair_adam_step_scaled on _adam_problem() against clip_grad_norm_ + torch.optim.Adam.

    With weight_decay the gradient Adam sees is coef * g + weight_decay * p, two terms of either sign: what the kernel owes is a
    relative error per term, so the bounds are taken of the terms' magnitude |coef g| + weight_decay |p| (`mag`), not of their
    sum -- exp_avg 1e-5 * sum of (1 - b1) mag, exp_avg_sq 2e-5 * sum of (1 - b2) |coef g + weight_decay p| mag (the square's error
    is twice the entry times the entry's error).  Without decay both reduce to the bounds of the entry itself, which are kept."""
    flat, params, grads = _adam_problem()
    ref_p = [torch.nn.Parameter(x.clone()) for x in params]
    live = [q for i, q in enumerate(ref_p) if i != UNTOUCHED]
    opt = torch.optim.Adam(live, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=weight_decay)

    p = flat.fill(params, pad=0.0).to(DEV)
    m, v = torch.zeros(flat.n, device=DEV), torch.zeros(flat.n, device=DEV)
    touched = torch.tensor([0 if i == UNTOUCHED else 1 for i in range(len(ADAM_NUMELS))], dtype=torch.int32, device=DEV)
    steps = torch.zeros(len(ADAM_NUMELS), device=DEV)
    guard = torch.zeros(1, dtype=torch.int32, device=DEV)
    scratch, seg_norm, out = torch.empty(flat.n // SEG, device=DEV), torch.empty(len(ADAM_NUMELS), device=DEV), torch.empty(2, device=DEV)
    from stair_amd._lib import check, lib
    coefs = []
    term_mag = [torch.zeros(n_) for n_ in ADAM_NUMELS]                     # sum of |terms| that entered exp_avg
    sq_mag = [torch.zeros(n_) for n_ in ADAM_NUMELS]                       # sum of |entry| x |terms| that entered exp_avg_sq
    for it, gs in enumerate(grads):
        for i, q in enumerate(ref_p):
            q.grad = None if i == UNTOUCHED else gs[i].clone()
        ref_norm = torch.nn.utils.clip_grad_norm_(live, MAX_NORM)
        ref_coef = min(1.0, MAX_NORM / (float(ref_norm) + 1e-6))
        p_before = [q.detach().clone() for q in ref_p]
        opt.step()
        g = flat.fill(gs).to(DEV)                                         # NaN padding: the norm must not see it
        check(lib.stair_grad_norm(P(g), flat.n, P(flat.first_d), P(flat.numel_d), len(ADAM_NUMELS), C.c_float(MAX_NORM), P(scratch),
                                  P(seg_norm), P(out), P(guard), _stream()))
        steps += touched.float()
        g_before = g.clone()
        _adam(flat, p, g, m, v, touched, steps, guard, out[1:], weight_decay=weight_decay)
        torch.cuda.synchronize()
        coefs.append(float(out[1]))
        assert abs(float(out[0]) - float(ref_norm)) <= 4e-6 * float(ref_norm)      # two fp32 evaluations, 2e-6 each
        assert int(guard[0]) == 0
        gb, ga = g_before.cpu(), g.cpu()
        assert torch.equal(gb[~gb.isnan()], ga[~ga.isnan()])              # the gradients are not written back
        pc, mc, vc = p.cpu(), m.cpu(), v.cpu()
        for i, q in enumerate(ref_p):
            lo = flat.first[i] * SEG
            sl = slice(lo, lo + ADAM_NUMELS[i])
            if i == UNTOUCHED:
                assert torch.equal(pc[sl], params[i]) and float(mc[sl].abs().max()) == 0.0 and float(vc[sl].abs().max()) == 0.0
                continue
            st = opt.state[q]
            mag = ref_coef * gs[i].abs() + weight_decay * p_before[i].abs()
            entry = ref_coef * gs[i] + weight_decay * p_before[i]
            term_mag[i] = B1 * term_mag[i] + (1 - B1) * mag
            sq_mag[i] = B2 * sq_mag[i] + (1 - B2) * entry.abs() * mag
            assert bool(((mc[sl] - st['exp_avg']).abs() <= 1e-5 * term_mag[i]).all()), (it, i)
            assert bool(((vc[sl] - st['exp_avg_sq']).abs() <= 2e-5 * sq_mag[i]).all()), (it, i)
            if weight_decay == 0.0:                                       # one term per step: the bounds are of the entry itself
                if it == 0:
                    torch.testing.assert_close(mc[sl], st['exp_avg'], rtol=1e-5, atol=0.0)
                torch.testing.assert_close(vc[sl], st['exp_avg_sq'], rtol=2e-5, atol=0.0)
            assert float((pc[sl] - q.detach()).abs().max()) <= 1e-6, (it, i)
    print('coefficients', coefs)
    assert 0.09 < coefs[0] < 0.11 and coefs[1] == 1.0 and 0.85 < coefs[2] < 0.95
    return flat, params, grads, coefs, m.cpu()


def test_scaled_adam_matches_torch_clip_then_adam():
    """Adam is almost invariant to a constant gradient scale, so the coefficient changes strongly from step to step (~0.1, 1, ~0.9)
    and the moments are compared too.  exp_avg: the coefficient's 2e-6 enters each term once -> rtol 1e-5 of the terms' magnitude
    (= of the entry itself after the first step, where there is one term; later steps add terms of either sign, and a relative error
    per TERM is what the kernel owes); exp_avg_sq: twice, all terms positive -> rtol 2e-5 of the entry; parameters 1e-6 absolute."""
    _scaled_adam_against_torch(0.0)


def test_scaled_adam_with_weight_decay_adds_the_decay_to_the_clipped_gradient():
    """The same problem with weight_decay = 0.01 against torch.optim.Adam(weight_decay=0.01) after clip_grad_norm_: torch clips g,
    then Adam adds weight_decay * p to the CLIPPED gradient.  The first step (coefficient ~0.1) tells the two orders apart: had the
    kernel scaled g + weight_decay * p, every exp_avg entry would be off by (1 - b1) (1 - coef) weight_decay |p| -- shown here to
    exceed the bound in nearly every entry, so the comparison inside _scaled_adam_against_torch cannot pass by luck."""
    wd = 0.01
    flat, params, grads, coefs, _ = _scaled_adam_against_torch(wd)
    n = far = 0
    for i, (pp, gg) in enumerate(zip(params, grads[0])):
        if i == UNTOUCHED:
            continue
        wrong_order = (1 - B1) * (1 - coefs[0]) * wd * pp.abs()          # |exp_avg error| of "add the decay, then scale" at step 1
        bound = 1e-5 * (1 - B1) * (coefs[0] * gg.abs() + wd * pp.abs())
        n, far = n + pp.numel(), far + int((wrong_order > 10 * bound).sum())
    print('entries where the other order is > 10 bounds away: %d of %d' % (far, n))
    assert far > 0.99 * n


def test_null_scale_is_stair_adam_step_and_a_set_guard_changes_nothing():
    flat, params, grads = _adam_problem()
    touched = torch.tensor([0 if i == UNTOUCHED else 1 for i in range(len(ADAM_NUMELS))], dtype=torch.int32, device=DEV)
    g = flat.fill(grads[0], pad=0.0).to(DEV)
    runs = []
    for scaled_entry in (False, True):
        p = flat.fill(params, pad=0.0).to(DEV)
        m, v = torch.zeros(flat.n, device=DEV), torch.zeros(flat.n, device=DEV)
        steps = torch.zeros(len(ADAM_NUMELS), device=DEV)
        for it in range(2):
            steps += touched.float()
            _adam(flat, p, g, m, v, touched, steps, None, None, scaled_entry)
        runs.append((p.clone(), m.clone(), v.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert not torch.equal(runs[0][0], flat.fill(params, pad=0.0).to(DEV))
    # a scale of 0.25 is not a no-op, and a set guard (either cause) refuses the step
    p, m, v = (t.clone() for t in runs[1])
    steps = torch.full((len(ADAM_NUMELS),), 3.0, device=DEV)
    scale = torch.tensor([0.25], device=DEV)
    for word in (1, 2, 3):
        guard = torch.tensor([word], dtype=torch.int32, device=DEV)
        _adam(flat, p, g, m, v, touched, steps, guard, scale)
        assert torch.equal(p, runs[1][0]) and torch.equal(m, runs[1][1]) and torch.equal(v, runs[1][2])
    _adam(flat, p, g, m, v, touched, steps, torch.zeros(1, dtype=torch.int32, device=DEV), scale)
    ref_m = B1 * runs[1][1] + (1 - B1) * 0.25 * g
    sl = slice(flat.first[0] * SEG, flat.first[0] * SEG + ADAM_NUMELS[0])
    torch.testing.assert_close(m[sl], ref_m[sl], rtol=1e-6, atol=1e-9)
    assert not torch.equal(p, runs[1][0])
