"""Shared helpers for the parity tests (oracle is test infrastructure; see oracle/nmn_oracle.py)."""
import ctypes as C
import json
import os

import numpy as np
import torch

from stair_amd import spec, synth
from oracle import nmn_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
PRETRAIN_MODULES = frozenset({'Exists', 'Xor', 'Equals', 'Filter', 'ToAction', 'FilterFrame', 'ExistsFrame',
                              'Superlative', 'Localize', 'Temporal', 'decoder'})


def plan_ctx(config):
    """a library context (stair_ctx_create) for `config`; the caller destroys it"""
    from stair_amd._lib import lib, check, StairConfig
    cfg = StairConfig(config['hidden_size'], config['video_size'], config['text_size'], config['answer_vocab_length'],
                      config['max_video_length'], config['object_types'], 1 if config['have_pretrain_head'] else 0)
    h = C.c_void_p()
    check(lib.stair_ctx_create(C.byref(cfg), C.byref(h)))
    return h


def int32_ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def pack_programs(programs, spans, q_lens):
    """The arrays stair_plan_build* takes for a batch: (prog_off, tokens, lo, hi, q_off).  programs: token-name lists;
    spans[q][i] = (lo, hi) of span token i of program q; q_lens: words per question."""
    enc = [np.asarray(spec.encode_program(p), dtype=np.int32) for p in programs]
    n = len(programs)
    prog_off = np.zeros(n + 1, np.int32); np.cumsum([len(e) for e in enc], out=prog_off[1:])
    tokens = np.concatenate(enc)
    lo = np.zeros(len(tokens), np.int32); hi = np.zeros(len(tokens), np.int32)
    for q in range(n):
        for i, c in enumerate(enc[q]):
            if c == spec.TOK_SPAN:
                lo[prog_off[q] + i], hi[prog_off[q] + i] = spans[q][i]
    q_off = np.zeros(n + 1, np.int32); np.cumsum(q_lens, out=q_off[1:])
    return prog_off, tokens, lo, hi, q_off


def build_plan(config, programs, spans, q_lens, T, flags=0, video_of_question=None, n_videos=None, video_len=None):
    """stair_plan_build (or _shared / _ragged, by the arguments given) of a batch in a fresh context: (ctx, plan, rc, prog_off).
    rc != 0: no plan, the message is in stair_last_error; the caller destroys what it got."""
    from stair_amd._lib import lib
    h = plan_ctx(config)
    prog_off, tokens, lo, hi, q_off = pack_programs(programs, spans, q_lens)
    n = len(programs)
    arrays = [int32_ptr(a) for a in (prog_off, tokens, lo, hi, q_off)]
    plan = C.c_void_p()
    if video_of_question is None:
        rc = lib.stair_plan_build(h, n, *arrays, T, flags, C.byref(plan))
    else:
        voq = np.asarray(video_of_question, np.int32)
        if video_len is None:
            rc = lib.stair_plan_build_shared(h, n, *arrays, n_videos, int32_ptr(voq), T, flags, C.byref(plan))
        else:
            vl = np.asarray(video_len, np.int32)
            rc = lib.stair_plan_build_ragged(h, n, *arrays, n_videos, int32_ptr(voq), int32_ptr(vl), T, flags, C.byref(plan))
    return h, plan, rc, prog_off


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    meta = json.loads(bytes(z['meta']).decode())
    return z, meta


def oracle_weights(config, seed=0):
    return O.to_torch(synth.make_weights(config, seed))


def question_for(meta, q):
    return synth.make_question(meta['config'], meta['seed'], q['qid'], form=q['form'], T=meta['T'])


def compare_with_reference_grads(fixture, get_grad, tol_rel=2e-4):
    """Check gradients against tests/golden/<fixture>.npz (the reference's own loss.backward()).
    get_grad(name) -> flat float tensor/ndarray of the full gradient (or None)."""
    z, meta = load_golden(fixture)
    stride, thr = meta['stride_large'], meta['large_threshold']
    worst = (0.0, '')
    n_checked = 0
    for key in z.files:
        if not key.startswith('grad/'):
            continue
        name = key[5:]
        if name.startswith('submodules.Superlative.localize_module.'):
            continue                                           # alias of Localize.* (same tensor, module_net.py:31-32)
        ref = np.asarray(z[key], dtype=np.float64)
        g = get_grad(name)
        assert g is not None, name
        g = np.asarray(torch.as_tensor(g).detach().cpu().reshape(-1), dtype=np.float64)
        if g.size > thr:
            g = g[::stride]
        assert g.shape == ref.shape, (name, g.shape, ref.shape)
        tol = tol_rel * max(float(np.abs(ref).max()), 1e-3)
        err = float(np.abs(g - ref).max()) if ref.size else 0.0
        worst = max(worst, (err / tol, name))
        assert err < tol, (name, err, tol)
        n_checked += 1
    assert n_checked > 80
    return worst, z, meta


def window_fixture():
    """tests/golden/window.npz (the reference's own train_module.main() run for two 32-question windows): returns
    (z, meta, questions with numpy golds, per-window reference records).  A record = {'module': [...], 'decoder':
    [...], 'contrastive': [...]} -- the criterion values in the reference's call order, split by kind (the contrastive
    modules are only ever scored in the pooled pass at the end of a window, train_module.py:360-366,388-406)."""
    z, meta = load_golden('window')
    config, T = meta['config'], meta['T']
    qs = []
    for i, form in enumerate(meta['forms']):
        q = synth.make_question(config, meta['question_seed'], i, form=form, T=T)
        q['sg_res_by_step'] = synth.make_gold(config, meta['gold_seed'], q, T=T, keep=meta['gold_keep'])
        qs.append(q)
    records, cur, n_dec = [], {'module': [], 'decoder': [], 'contrastive': []}, 0
    for module, value in zip(meta['loss_modules'], z['loss_values']):
        if module in ('Filter', 'Superlative', 'ToAction'):
            cur['contrastive'].append((module, float(value)))
            continue
        if n_dec == meta['window']:                            # first non-contrastive call after a full window
            records.append(cur)
            cur, n_dec = {'module': [], 'decoder': [], 'contrastive': []}, 0
        if module == 'decoder':
            cur['decoder'].append(float(value))
            n_dec += 1
        else:
            cur['module'].append((module, float(value)))
    records.append(cur)
    assert len(records) * meta['window'] == len(qs)
    return z, meta, qs, records


def window_weights(z, meta, window_no, name, tensor):
    """The reference's value of parameter `name` after `window_no` optimizer steps, and `tensor` subsampled the same way."""
    ref = np.asarray(z['w%d/%s' % (window_no, name)], dtype=np.float64)
    t = np.asarray(torch.as_tensor(tensor).detach().cpu().reshape(-1), dtype=np.float64)
    if t.size > meta['large_threshold']:
        t = t[::meta['stride_large']]
    assert t.shape == ref.shape, (name, t.shape, ref.shape)
    return ref, t


class _ForcedMasks:
    """Runs the oracle with the ReLU masks of ANOTHER implementation in its backward pass.

    A ReLU's derivative is 0 or 1 on either side of a kink; two correct implementations whose pre-activations differ by
    rounding pick different sides for the few inputs that lie within that rounding of zero, and the gradient is discontinuous
    there (test_bf16_feature_step_at_full_size_gradients_and_adam counts them).  Here the oracle keeps its own forward values
    but differentiates every module / decoder ReLU with the mask the HIP pass used (its saved activation > 0,
    stair_plan_saved_offset) -- a valid sub-gradient of the same function wherever the two agree in sign, i.e. everywhere but
    at those kinks -- so what is left between the two gradients is arithmetic, and the strict elementwise bound applies.
    The relus of Temporal's tiny relate nets ([T]-sized, recomputed by the HIP backward kernel, not saved) keep the oracle's
    own masks.

    Dropout-aware form (p = the nn.Dropout probability of a pass run with dropout=(p, seed)): a dropped element is an exact zero
    of a tensor the training plan exposes, so the keep mask C the kernels used is read back -- C = (HIP's post-dropout
    activation != 0) -- and handed to the oracle through its dropout hook (`self.hook`, oracle/nmn_oracle.py `dropout=`).  At a
    ReLU + Dropout site the oracle then computes clamp_min(z, 0) * C / (1 - p), backward g * C / (1 - p).  Where C comes from:
    saved(q, i, 0 / 1) for the tile MLP layers, the Exists / ToAction hidden rows and Temporal's pre-LayerNorm rows;
    saved(q, None) for the decoder's hidden row; node(q, i) where the site is the node's output (Exists .3, FilterFrame's dense
    layer, HasItem's sigmoid -- never 0 itself, so there the mask is exact).  Clips shorter than the batch's longest: the first
    rows of a saved tile / attention row are the clip's.  Collected on the way:
      sites, flips     ReLU sites compared and disagreements.  Plain sites: (z > 0) != mask.  ReLU + Dropout sites: C set where the
                       oracle's z <= 0 (the other side is what dropout does)
      flip_reach       (no dropout) the largest oracle |pre-activation| at a disagreement, over max(1, max of that tensor's
                       activation): a forward comparison at tolerance tol leaves room for a flip only where this is below tol
      kept[kind]       [entries whose oracle pre-activation is positive by more than `bound(ref)`, those of them with C set]
      plain_zero[kind] exact zeros at outputs the reference does NOT drop, where the oracle's value is positive beyond the bound
      record[(i, k)]   (C, positive-beyond-bound) of dropout call k of token i ('decoder': the decoder's), for mask statistics"""

    class _Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, z, mask):
            ctx.save_for_backward(mask)
            return z.clamp_min(0)

        @staticmethod
        def backward(ctx, g):
            (mask,) = ctx.saved_tensors
            return g * mask, None

    def __init__(self, res, qi, program, p=None):
        self.res, self.qi, self.program, self.p = res, qi, program, p
        self.order = [i for i in range(len(program) - 1, -1, -1) if program[i] in O.ARITY]      # the interpreter's module calls
        self.queue, self.flips, self.sites, self.flip_reach = [], 0, 0, 0.0
        self.dqueue, self.kept, self.plain_zero, self.record = [], {}, {}, {}
        self.token = None

    @staticmethod
    def bound(ref):
        """the forward bound of the node comparisons: 2e-5 * max(1, max|ref|)"""
        return 2e-5 * max(1.0, float(ref.detach().abs().max())) if ref.numel() else 2e-5

    @staticmethod
    def _fit(m, shape):
        """a [T, H] tile or [T] row of the launch batch cut to the clip's own frames"""
        if m.numel() != int(np.prod(shape)):
            m = m.reshape(-1, shape[-1])[:shape[0]] if len(shape) == 2 else m.reshape(-1)[:shape[-1]]
        return m.reshape(shape)

    def _masks_for(self, i):
        """the ReLU masks of token i's module call in the order the oracle calls torch.relu: None (the oracle's own), a mask, or
        under dropout (mask, kind) for a ReLU the reference follows with an nn.Dropout; and the dropout calls it must make"""
        prog, res, qi, drop = self.program[i], self.res, self.qi, self.p is not None
        sv = lambda which: res.saved(qi, i, which).detach().cpu() > 0
        out = lambda: res.node(qi, i).detach().cpu() > 0
        if drop:              # a dropped element is an exact zero; anything else was kept (a negative value would count as a flip)
            sv = lambda which: res.saved(qi, i, which).detach().cpu() != 0
            out = lambda: res.node(qi, i).detach().cpu() != 0
        D = (lambda m, kind: (m, prog + '.' + kind)) if drop else (lambda m, kind: m)
        plain = (lambda m: (m, None)) if drop else (lambda m: m)
        if prog == 'Filter':
            relus, sites = [D(sv(0), 'param.0'), D(sv(1), 'param.3'), plain(out())], ['Filter.param.*.0', 'Filter.param.*.3']
        elif prog == 'FilterFrame':
            relus = [D(sv(0), 'param.0'), D(sv(1), 'param.3'), D(out(), 'dense.0')]
            sites = ['FilterFrame.param.*.0', 'FilterFrame.param.*.3', 'FilterFrame.dense.0']
        elif prog == 'HasItem':
            relus, sites = [D(sv(0), 'param.0')], ['HasItem.param.0', 'HasItem.param.3']
        elif prog == 'Localize':
            relus, sites = [D(sv(0), 'video_linear.0')], ['Localize.video_linear.0']
        elif prog == 'Superlative':
            relus, sites = [D(sv(0), 'localize.0'), plain(out())], ['Localize.video_linear.0']
        elif prog == 'Temporal':
            mode = self.program[i + 1]
            relus, sites = ([None, None] if mode != 'while' else []) + [D(sv(0), 'dense.0')], ['Temporal.dense.0']
        elif prog == 'Exists':
            relus, sites = [D(sv(0), 'param.0'), D(out(), 'param.3')], ['Exists.param.0', 'Exists.param.3']
        elif prog == 'ToAction':
            relus, sites = [D(sv(0), 'param.0'), plain(out())], ['ToAction.param.0']
        elif prog in ('Xor', 'Equals', 'Compare'):
            relus, sites = [plain(out())], []
        else:
            relus, sites = [], []
        return relus, (sites if drop else [])

    def _count(self, kind, pos, m):
        k = self.kept.setdefault(kind, [0, 0])
        k[0] += int(pos.sum())
        k[1] += int((pos & m).sum())

    def __enter__(self):
        self._relu, self._run = torch.relu, O.run_module

        def relu(z):
            if not self.queue:
                return self._relu(z)
            m = self.queue.pop(0)
            if m is None:
                return self._relu(z)
            kind = plain_site = None
            if isinstance(m, tuple):                      # dropout-aware form
                m, kind = m
                plain_site = kind is None
            m = self._fit(m, z.shape)
            self.sites += m.numel()
            zd = z.detach()
            if kind is not None:
                self.flips += int((m & (zd <= 0)).sum())
                pos = zd > self.bound(zd.clamp_min(0))
                self._count(kind, pos, m)
                self._pending = (m, pos, kind)
            else:
                differ = (zd > 0) != m
                self.flips += int(differ.sum())
                if bool(differ.any()):
                    self.flip_reach = max(self.flip_reach, float(zd[differ].abs().max()) / max(1.0, float(zd.max())))
                if plain_site:
                    name = self.program[self.token] if self.token != 'decoder' else 'decoder'
                    self.plain_zero[name] = self.plain_zero.get(name, 0) + int((~m & (zd > self.bound(zd.clamp_min(0)))).sum())
            return self._Fn.apply(z, m.to(z.dtype))

        def run_module(w, prog, params, dropout=None):
            i = self.order.pop(0)
            assert self.program[i] == prog
            self.token, self._ordinal, self._pending = i, 0, None
            self.queue, self.dqueue = self._masks_for(i)
            r = self._run(w, prog, params, dropout=dropout)
            assert not self.queue, (prog, len(self.queue))
            assert not self.dqueue, (prog, 'the oracle made no dropout call at', self.dqueue)
            return r
        torch.relu, O.run_module = relu, run_module
        return self

    def hook(self, site, y):
        """the oracle's nn.Dropout: y * C / (1 - p) with the keep mask of the HIP pass"""
        import fnmatch
        assert self.dqueue, ('the oracle drops at %s, where the plan of token %s exposes no dropout site' % (site, self.token))
        want = self.dqueue.pop(0)
        assert fnmatch.fnmatchcase(site, want), (site, want)
        if site == 'HasItem.param.3':                     # behind the sigmoid: no ReLU, the node's value itself tells
            m = self._fit(self.res.node(self.qi, self.token).detach().cpu() != 0, y.shape)
            pos = y.detach() > self.bound(y)
            self.sites += m.numel()
            self._count('HasItem.param.3', pos, m)
        else:
            assert self._pending is not None, site       # the ReLU in front of this Dropout took a (mask, kind) entry
            m, pos, _ = self._pending
            self._pending = None
        self.record[(self.token, self._ordinal)] = (m, pos)
        self._ordinal += 1
        return y * (m.to(y.dtype) / (1.0 - self.p))

    def decoder(self):
        m = self.res.saved(self.qi, None).detach().cpu()
        m = m != 0 if self.p is not None else m > 0
        self.token, self._ordinal, self._pending = 'decoder', 0, None
        self.queue = [(m, 'decoder.0')] if self.p is not None else [m]
        self.dqueue = ['decoder.0'] if self.p is not None else []

    def __exit__(self, *exc):
        torch.relu, O.run_module = self._relu, self._run
        return False

    def forward(self, w, config, q, **kwargs):
        """O.forward of question q inside this context, the decoder's mask queued when the interpreter has run every module
        (its ReLU is the last one of the pass) and, in the dropout-aware form, the hook in place."""
        orig_lin = O._lin

        def lin(w_, prefix, x):
            if prefix.endswith('decoder.0'):
                assert not self.order, self.order
                self.decoder()
            return orig_lin(w_, prefix, x)
        if self.p is not None:
            kwargs['dropout'] = self.hook
        with self:
            O._lin = lin
            try:
                r = O.forward(w, config, q, **kwargs)
            finally:
                O._lin = orig_lin
        assert not self.queue and not self.dqueue, (self.queue, self.dqueue)
        return r
