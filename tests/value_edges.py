"""The value-edge corpus: programs, clip encodings and weight variants that put the VALUES into the kernels which random
initialisation never produces -- norms under the cosine clamp, exact ties, saturated activations, zero-variance LayerNorm rows,
dead ReLU layers (support module, no tests; the shape-space counterpart is tests/program_cells.py).

Everything is a pure function of a seed (stair_amd.synth's counter-based generator).

  CLIPS       clip ENCODINGS [T = 24, H], handed to the plan as the caller's own (VideoNMN.logits(encoded=...)), so that a program's
              `video` operand holds exactly the crafted rows; the oracle reads the same rows with its video encoder replaced by
              the identity (identity_encoder)
  programs()  every template of program_cells.SLOTS filled with the first producer of its kind, and the tie / zero programs of
              EXTRA.  In a template `w` is a span word of its own and `u` a span word whose every occurrence in the program gets
              the SAME span, hence a bit-identical vector: `XorFrame u u` is an exact zero vector, `Choose u u F1` has cos1 == cos2.
              HI' = `XorFrame HI XorFrame HI HI` is |HI - 0|: a slot of its own that holds the values of HI bit for bit, with and
              without common-subexpression sharing -- two DIFFERENT slots with equal values for And (an exact tie in every frame)
              and XorFrame (an exact zero whose gradient is sign(0) = 0)
  VARIANTS    edits of a copy of the seed-0 weights
  BATCHES     'init': one question per (program, clip regime), all in one batch; one batch per weight variant over the programs
              that reach the touched module, on the clips of VARIANT_CLIPS

oracle_pass(geometry, batch, dtype) runs the oracle over a batch (values of every step, the gradient of the custom loss of
tests/test_gpu_autograd.py for the encodings, the question rows and the parameters); EdgeCounter counts, inside the oracle, how
often each edge is actually reached.

The bounds are those of tests/test_gpu_program_cells.py.  ILL_CONDITIONED lists the (geometry, batch, quantity) triples -- one
question's gradient, one node, one tensor -- at which the oracle in fp32 differs from the oracle in fp64 by more than a quarter of
that bound, with the measured difference: those get 4 x the measured difference as their bound (tests/test_value_edges_host.py
measures; the figure never comes from HIP output).  Where the bf16x3 mode's own products would not fit the ordinary bounds, the
inputs of that mode are drawn at a smaller scale instead (LARGE, HASITEM_FACTOR, LSTM_INPUT_SCALE).
"""
import contextlib
import functools

import numpy as np
import torch
import torch.nn.functional as F

import program_cells as PC
from oracle import nmn_oracle as O
from stair_amd import spec, synth

SEED = 0
T = 24
NODE_TOL = {'f32': 2e-5, 'bf16x3': 1e-4}      # of max(1, max|ref|), per node
REL, FLOOR = 2e-4, 1e-6                       # gradients: of the question's largest entry
GRAD_LIMIT = float(2 ** 17)                   # half the fixed-point range of the deterministic gradient sums

GEOMETRIES = {
    'tiny': dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, answer_vocab_length=16, max_video_length=40, object_types=10),
    'h512': dict(spec.DEFAULT_CONFIG, hidden_size=512, video_size=128, answer_vocab_length=16, max_video_length=40, object_types=10),
}

# `large` clips are N(0, 1) x LARGE and hasitem_sat multiplies HasItem.param.3.weight by HASITEM_FACTOR.  Hidden size 512 runs in the
# bf16x3 mode, whose products carry 2^-17 of their operands (128 x fp32's rounding) under a node bound only 5 x the f32 mode's: at
# x 64 a Filter output is ~1e3 and `And w F1`, bounded by max(1, its own largest entry) = 1, inherits 6e-4 of it.  The inputs of that
# geometry are therefore drawn at a smaller scale, at which the ordinary bounds hold; the bounds themselves stay.
LARGE = {64: 64.0, 512: 4.0}
HASITEM_FACTOR = {64: 100.0, 512: 10.0}
CLIPS = ['plain', 'zero_rows', 'all_zero', 'one_frame', 'two_frames', 'large', 'tiny', 'short_zero_tail']
VARIANT_CLIPS = ['plain', 'zero_rows', 'large']
ZERO_ROWS = [0, 7, 8, 9, T - 1]
SHORT = 17


def encoding(H, seed, key, regime):
    """([T, H] float32 rows, frames) of one clip"""
    x = synth.normal(seed, key + '/enc', (T, H)).astype(np.float32)
    frames = T
    if regime == 'zero_rows':
        x[ZERO_ROWS] = 0
    elif regime == 'all_zero':
        x[:] = 0
    elif regime == 'one_frame':
        x[:] = x[0].copy()
    elif regime == 'two_frames':
        a, b = x[0].copy(), x[1].copy()
        x[0::2], x[1::2] = a, b
    elif regime == 'large':
        x *= np.float32(LARGE[H])
    elif regime == 'tiny':            # every row norm under the 1e-8 clamp (8e-10 at H = 64, 2.3e-9 at H = 512), squares normal fp32
        x *= np.float32(1e-10)
    elif regime == 'short_zero_tail':
        frames = SHORT
        x[SHORT - 1:] = 0
    else:
        assert regime == 'plain', regime
    return x, frames


# ---- programs ------------------------------------------------------------------------------------------------------------------
MACROS = dict(PC.MACROS, **{"HI'": 'XorFrame HI XorFrame HI HI', 'Z': 'XorFrame u u'})
EXTRA = [
    ("And HI HI'", PC.FRAME),
    ("XorFrame HI HI'", PC.FRAME),
    ('ExistsFrame Z video', PC.FRAME),
    ('Choose Z w F1', PC.VEC),
    ('Localize video Z', PC.ATT),
    ('ExistsFrame w AttnVideo video XorFrame HI HI', PC.FRAME),        # a zero map at an interior node
    ('Relate forward XorFrame HI HI', PC.FRAME),
    ('Temporal before video Localize video Z', PC.MAP),
    ('Choose u u F1', PC.VEC),
    ('Superlative max Array2 u u video', PC.VEC),
    ('Z', PC.VEC),                                                     # the decoder reads an exact zero root
]


def _expand(text):
    out = []
    for tok in text.split():
        out += _expand(MACROS[tok]) if tok in MACROS else [tok]
    return out


class Program:
    def __init__(self, name, body, out_kind):
        closed = _expand(PC.CLOSE[out_kind])
        at = closed.index('X')
        self.name = name
        self.tokens = PC._name_words(closed[:at] + body + closed[at + 1:])
        assert O.program_is_valid(self.tokens), name

    def __repr__(self):
        return 'Program(%s)' % self.name


@functools.lru_cache(maxsize=None)
def programs():
    out = []
    for slot, kind, out_kind in PC.SLOTS:
        c = PC.Cell(slot, kind, out_kind, PC.PRODUCERS[kind][0], kind)
        out.append(Program(c.name, [t if not t.startswith('w') or not t[1:].isdigit() else 'w' for t in c.program], PC.VEC))
    out += [Program(text, _expand(text), kind) for text, kind in EXTRA]
    seen = set()            # several slots give one program once the first producer fills them (`And X HI` and `And HI X` with HI): kept once
    return [p for p in out if not (tuple(p.tokens) in seen or seen.add(tuple(p.tokens)))]


def xor_of_equal_operands(program):
    """positions of the XorFrame nodes whose two operands are the same subtree token for token (`u` against `u`, HI against HI):
    their value is an exact zero in any arithmetic"""
    ch = O.children_of(program)

    def end(i):
        return i + 1 if not ch[i] else end(ch[i][-1])
    return [i for i, t in enumerate(program)
            if t == 'XorFrame' and program[ch[i][0]:end(ch[i][0])] == program[ch[i][1]:end(ch[i][1])]]


# ---- weight variants -----------------------------------------------------------------------------------------------------------
P = 'submodules.'
RELATE_MODES = ('before', 'after', 'between')


def _dense(bias):
    def edit(w):
        w[P + 'Temporal.dense.0.weight'][:] = 0
        w[P + 'Temporal.dense.0.bias'][:] = bias
    return edit


def _filter_dead(w):
    w[P + 'Filter.param.objects.0.bias'][:] = -100


def _beta_large(w):
    b = w[P + 'Relate.beta']
    b[:] = 200 * np.linspace(0, 1, b.size, dtype=np.float32).reshape(b.shape)


def _beta_flat(w):
    w[P + 'Relate.beta'][:] = 0.25


def _relate_sat(w):
    for m in RELATE_MODES:
        for p in ('weight', 'bias'):
            w[P + 'Temporal.relate.%s.4.%s' % (m, p)] *= 50


def _hasitem_sat(w):
    v = w[P + 'HasItem.param.3.weight']
    v *= HASITEM_FACTOR[v.shape[-1]]


def _const_layer(prefix, fill):
    def edit(w):
        w[P + prefix + '.weight'][:] = 0
        w[P + prefix + '.bias'][:] = fill
    return edit


def _reads_localize(p):
    return 'Localize' in p or 'Superlative' in p


# name -> (edit, does a program reach the touched module)
VARIANTS = {
    'dense_const': (_dense(0.5), lambda p: 'Temporal' in p),            # zero-variance LayerNorm rows
    'dense_dead': (_dense(-0.5), lambda p: 'Temporal' in p),            # ... exactly 0, relu' = 0 everywhere
    'filter_dead': (_filter_dead, lambda p: any(p[i] == 'Filter' and p[c[1]] == 'objects' for i, c in enumerate(O.children_of(p)) if c)),
    'beta_large': (_beta_large, lambda p: 'Relate' in p),               # a softmax over steps of 5.1: exact zeros in fp32 far from the peak
    'beta_flat': (_beta_flat, lambda p: 'Relate' in p),                 # not in the issue's list: equal frames give an exactly uniform softmax
    'relate_sat': (_relate_sat, lambda p: any(m in p for m in RELATE_MODES)),
    'hasitem_sat': (_hasitem_sat, lambda p: 'HasItem' in p),            # attentions exactly 0.0 / 1.0
    # not in the issue's list: the only way under the clamp for the cosine of Localize / Superlative, whose two sides come out of
    # Linear layers with random biases (cosine_attn_bwd_grouped_kernel, the COSINE tail): every frame row 1e-10 (norm 8e-10 / 2.3e-9)
    # or 0, every keyword row 1e-10
    'localize_tiny': (_const_layer('Localize.video_linear.3', 1e-10), _reads_localize),
    'localize_zero': (_const_layer('Localize.video_linear.3', 0.0), _reads_localize),
    # (not Superlative over two actions: both keyword rows are then the same vector, and the clip's gradient is zero by a cancellation
    # that holds in exact arithmetic only)
    'keyword_tiny': (_const_layer('Localize.keyword_linear.0', 1e-10), lambda p: _reads_localize(p) and not ('Superlative' in p and 'Array2' in p)),
}
# the gradient behind an active clamp carries 1 / eps = 1e8: the custom loss of these batches is scaled down so that every parameter
# gradient stays under GRAD_LIMIT (tests/test_value_edges_host.py checks it)
R_SCALE = {'localize_tiny': 1e-6, 'localize_zero': 1e-6, 'keyword_tiny': 1e-7}
BATCHES = ['init'] + list(VARIANTS)


def weights(config, batch):
    """{name: float32 ndarray} of the seed-0 weights with the batch's variant applied to a copy"""
    w = {k: v.copy() for k, v in synth.make_weights(config, SEED).items()}
    for alias, canon in spec.WEIGHT_ALIASES.items():
        w[alias] = w[canon]
    if batch != 'init':
        VARIANTS[batch][0](w)
    return w


def cases(batch):
    """[(program, clip regime)] of a batch"""
    if batch == 'init':
        return [(p, r) for p in programs() for r in CLIPS]
    reach = VARIANTS[batch][1]
    return [(p, r) for p in programs() if reach(p.tokens) for r in VARIANT_CLIPS]


def questions(config, batch):
    """The question dicts of a batch (layout of program_cells.question): 'encoded' the clip's [T, H] rows, 'video_len' its frames,
    'video_features' the rows the oracle reads under identity_encoder (cut to the clip's frames); every `u` of a program has the
    span of the first one"""
    out = []
    for k, (p, regime) in enumerate(cases(batch)):
        d = PC.question(config, SEED, k, T, program=p.tokens, with_video=False)
        shared = [i for i, t in enumerate(p.tokens) if t == 'u']
        for i in shared:
            d['prog_str_to_question_tokens'][i] = d['prog_str_to_question_tokens'][shared[0]]
        d['encoded'], d['video_len'] = encoding(config['hidden_size'], SEED, 'edge/%s/%d' % (batch, k), regime)
        d['video_features'] = d['encoded'][:d['video_len']]
        d['qa_id'] = '%s | %s | %s' % (batch, p.name, regime)
        out.append(d)
    return out


# ---- the oracle on the corpus --------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def identity_encoder():
    """the oracle's video encoder replaced by the identity for the duration: `video_features` ARE the encodings"""
    orig = O.encode_video
    O.encode_video = lambda w, video, explicit=False: video
    try:
        yield
    finally:
        O.encode_video = orig


class EdgeCounter:
    """Counts, inside the oracle, the value edges its operators are fed (a context manager; patches are undone on exit):
      cos_zero_rows / cos_small_norms   rows entering a cosine that are exactly 0 / whose norm is below the 1e-8 clamp
      tie_min / tie_abs                 elements with a == b entering torch.minimum / |a - b| from two tensors
      tie_choose                        Choose calls with cos1 == cos2
      tie_superlative / tie_relate      softmax inputs of Superlative / Relate holding two equal entries
      sigmoid_saturated                 sigmoid outputs equal to 0.0 or 1.0 (in fp32)
      sigmoid_beyond_10                 sigmoid inputs with |x| > 10: the derivative is below 5e-5
      layernorm_flat_rows               LayerNorm rows of zero variance
      dead_layers                       ReLU calls whose every pre-activation is <= 0"""
    KEYS = ('cos_zero_rows', 'cos_small_norms', 'tie_min', 'tie_abs', 'tie_choose', 'tie_superlative', 'tie_relate',
            'sigmoid_saturated', 'sigmoid_beyond_10', 'layernorm_flat_rows', 'dead_layers')

    def __init__(self):
        self.n = dict.fromkeys(self.KEYS, 0)

    @staticmethod
    def _has_tie(x):
        x = x.detach().reshape(-1)
        return x.numel() > 1 and int(torch.unique(x).numel()) < x.numel()

    def __enter__(self):
        n = self.n
        self._saved = [(O, k, getattr(O, k)) for k in ('cos_rows', 'op_and', 'op_xorframe', 'op_choose', 'op_superlative', 'op_relate')]
        self._saved += [(torch, 'sigmoid', torch.sigmoid), (torch, 'relu', torch.relu), (torch, 'softmax', torch.softmax),
                        (F, 'layer_norm', F.layer_norm)]
        orig = {k: f for _, k, f in self._saved}
        where = []

        def cos_rows(a, b, eps=1e-8):
            for x in (a, b):
                norms = x.detach().reshape(-1, x.shape[-1]).norm(dim=-1)
                n['cos_zero_rows'] += int((norms == 0).sum())
                n['cos_small_norms'] += int((norms < eps).sum())
            return orig['cos_rows'](a, b, eps)

        def op_and(a, b):
            n['tie_min'] += int((a.detach() == b.detach()).sum()) if a is not b else 0
            return orig['op_and'](a, b)

        def op_xorframe(a, b):
            n['tie_abs'] += int((a.detach() == b.detach()).sum()) if a is not b else 0
            return orig['op_xorframe'](a, b)

        def op_choose(kw1, kw2, query):
            c1, c2 = (orig['cos_rows'](k.detach().unsqueeze(0), query.detach().unsqueeze(0)) for k in (kw1, kw2))
            n['tie_choose'] += int(bool(c1 == c2))
            return orig['op_choose'](kw1, kw2, query)

        def softmax(x, dim):
            if where:
                n['tie_' + where[-1]] += int(self._has_tie(x))
            return orig['softmax'](x, dim=dim)

        def tagged(name, tag):
            def f(*a, **kw):
                where.append(tag)
                try:
                    return orig[name](*a, **kw)
                finally:
                    where.pop()
            return f

        def sigmoid(x):
            y = orig['sigmoid'](x)
            yf = y.detach().float()
            n['sigmoid_saturated'] += int(((yf == 0) | (yf == 1)).sum())
            n['sigmoid_beyond_10'] += int((x.detach().abs() > 10).sum())
            return y

        def relu(x):
            n['dead_layers'] += int(x.numel() > 1 and bool((x.detach() <= 0).all()))
            return orig['relu'](x)

        def layer_norm(x, shape, *a, **kw):
            rows = x.detach().reshape(-1, x.shape[-1])
            n['layernorm_flat_rows'] += int((rows == rows[:, :1]).all(dim=1).sum())
            return orig['layer_norm'](x, shape, *a, **kw)
        new = dict(cos_rows=cos_rows, op_and=op_and, op_xorframe=op_xorframe, op_choose=op_choose, softmax=softmax, sigmoid=sigmoid,
                   relu=relu, layer_norm=layer_norm, op_superlative=tagged('op_superlative', 'superlative'),
                   op_relate=tagged('op_relate', 'relate'))
        for mod, k, _ in self._saved:
            setattr(mod, k, new[k])
        return self

    def __exit__(self, *exc):
        for mod, k, f in self._saved:
            setattr(mod, k, f)
        return False


class ReluMasks:
    """record: keeps the mask (z > 0) of every torch.relu call of a pass, per question; replay: a second pass of the same questions
    differentiates every ReLU with the recorded mask (its forward values stay its own) and counts the sites where its own sign differs
    (`flips` of `sites`) -- what helpers._ForcedMasks does with the masks of a HIP pass, between two oracle passes"""

    class _Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, z, mask):
            ctx.save_for_backward(mask)
            return z.clamp_min(0)

        @staticmethod
        def backward(ctx, g):
            (mask,) = ctx.saved_tensors
            return g * mask, None

    def __init__(self):
        self.store, self.replay, self.flips, self.sites, self._q = {}, False, 0, 0, None

    def begin(self, k):
        self._q = self.store.setdefault(k, []) if not self.replay else list(self.store[k])

    def __enter__(self):
        self._relu = torch.relu

        def relu(z):
            if not self.replay:
                self._q.append(z.detach() > 0)
                return self._relu(z)
            m = self._q.pop(0)
            self.sites += m.numel()
            self.flips += int(((z.detach() > 0) != m).sum())
            return self._Fn.apply(z, m.to(z.dtype))
        torch.relu = relu
        return self

    def __exit__(self, *exc):
        torch.relu = self._relu
        return False


def custom_R(n, A, batch, seed=7):
    """the coefficients of the custom loss of tests/test_gpu_autograd.py (_R), times the batch's R_SCALE"""
    return torch.from_numpy(np.random.RandomState(seed).randn(n, A).astype(np.float32)) * np.float32(R_SCALE.get(batch, 1.0))


def custom_loss(logits, R):
    return (logits.log_softmax(-1) * R.to(logits.dtype)).sum()


class Pass:
    """what oracle_pass keeps: per question logits, steps (a tensor per program token that has one), d_encoded [frames, H] and
    d_question; grads {parameter: gradient summed over the batch, or None}; edges (EdgeCounter.n)"""


def run_oracle(config, batch, dtype, forward=None, count=True, masks=None):
    """The oracle over a batch in `dtype`, its video encoder the identity.  forward(k, w, q) -> O.forward's dict with
    return_result_of_each_step (default: O.forward itself; the H = 512 tests pass the forward of a helpers._ForcedMasks).
    masks: a ReluMasks that records or replays."""
    qs = questions(config, batch)
    names = [n for n, _ in spec.weight_table(config)]
    wnp = weights(config, batch)
    w = {k: torch.from_numpy(wnp[k]).to(dtype).requires_grad_(True) for k in names}
    for alias, canon in spec.WEIGHT_ALIASES.items():
        w[alias] = w[canon]
    R = custom_R(len(qs), config['answer_vocab_length'], batch)
    g = Pass()
    g.config, g.batch, g.qs, g.names, g.w, g.R = config, batch, qs, names, w, R
    g.logits, g.steps, g.d_encoded, g.d_question = [], [], [], []
    counter = EdgeCounter() if count else contextlib.nullcontext()
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                     # tiny operators: one thread is the fastest
    try:
        with identity_encoder(), counter, (masks or contextlib.nullcontext()):
            for k, q in enumerate(qs):
                if masks is not None:
                    masks.begin(k)
                v = torch.from_numpy(q['video_features']).to(dtype).clone().requires_grad_(True)
                qq = torch.from_numpy(q['question']).to(dtype).clone().requires_grad_(True)
                d = dict(q, video_features=v, question=qq)
                if forward is None:
                    r = O.forward(w, config, d, return_res_by_step=False, return_result_of_each_step=True, explicit_lstm=True)
                else:
                    r = forward(k, w, d)
                custom_loss(r['logits'].unsqueeze(0), R[k:k + 1]).backward()
                g.logits.append(r['logits'].detach())
                g.steps.append([s.detach() if isinstance(s, torch.Tensor) else None for _, s in r['result_of_each_step']])
                g.d_encoded.append(v.grad if v.grad is not None else torch.zeros_like(v))
                g.d_question.append(qq.grad if qq.grad is not None else torch.zeros_like(qq))
    finally:
        torch.set_num_threads(threads)
    g.grads = {n: w[n].grad for n in names}
    g.edges = counter.n if count else None
    return g


@functools.lru_cache(maxsize=None)
def oracle_pass(geometry, batch, dtype=torch.float64):
    """run_oracle of a geometry's batch, computed once; nobody writes to it"""
    return run_oracle(GEOMETRIES[geometry], batch, dtype)


def regime_of(q):
    return q['qa_id'].rsplit(' | ', 1)[1]


def compare_passes(ref, other, tol):
    """{quantity: |other - ref| / bound} and [(question, quantity, error) where ref is identically zero and other is not].  Quantities,
    the keys of ILL_CONDITIONED: per question 'logits@<qa_id>', 'd_encoded@<qa_id>', 'd_question@<qa_id>'; per node
    'node@<qa_id>@<position>'; per tensor 'params@<name>' (the sum over the batch)."""
    ratios, exact = {}, []
    for k, q in enumerate(ref.qs):
        prog = q['nmn_program_list']
        err, bound = node_err(other.logits[k], ref.logits[k], tol)
        ratios['logits@' + q['qa_id']] = err / bound
        for i, r in enumerate(ref.steps[k]):
            if r is None or prog[i] not in O.ARITY:
                continue
            err, bound = node_err(other.steps[k][i], r, tol)
            ratios['node@%s@%d' % (q['qa_id'], i)] = err / bound
        for what, got, r in (('d_encoded', other.d_encoded[k], ref.d_encoded[k]), ('d_question', other.d_question[k], ref.d_question[k])):
            err, bound = grad_err(got, r)
            if bound == 0.0:
                if err != 0.0:
                    exact.append((q['qa_id'], what, err))
            else:
                ratios['%s@%s' % (what, q['qa_id'])] = err / bound
    for n in ref.names:
        r, got = ref.grads[n], other.grads[n]
        assert (r is None) == (got is None), n
        if r is not None:
            err = float((got.double() - r.double()).abs().max())
            ratios['params@' + n] = err / (REL * max(float(r.abs().max()), 1e-3))
    return ratios, exact


def grad_err(got, ref):
    """(error, bound) of one question's gradient: REL of its own largest entry, floor FLOOR; an all-zero reference wants exact zeros"""
    ref = ref.double()
    if float(ref.abs().max()) == 0.0:
        return float(got.abs().max()), 0.0
    return float((got.double() - ref).abs().max()), REL * max(float(ref.abs().max()), FLOOR)


def node_err(got, ref, tol):
    ref = ref.double()
    return float((got.double() - ref).abs().max()), tol * max(1.0, float(ref.abs().max()))


# (geometry, batch, quantity) -> the measured difference between the oracle in fp32 and the oracle in fp64 over the ordinary bound,
# for the quantities where that exceeds a quarter; quantities as in compare_passes: one question's gradient, one node, one tensor.  A
# GPU comparison of a listed quantity gets 4 x the measured difference, i.e. max(1, 4 x ratio) x the ordinary bound; everything
# unlisted is under a quarter and keeps the ordinary bound.  tests/test_value_edges_host.py measures all of it on the CPU; no figure
# comes from HIP output.
# hasitem_sat at H = 64: HasItem.param.3.weight x 100 on the clips x 64 puts logits near +-16, where s rounds to within a few ulps of 1
# in fp32 and the derivative s (1 - s) loses its digits.  Measured 1.20, 0.92, 1.21, 5.86 and 1.22; listed with a quarter of headroom.
ILL_CONDITIONED = {
    ('tiny', 'hasitem_sat', 'd_encoded@hasitem_sat | XorFrame X EF <- HI | large'): 1.5,
    ('tiny', 'hasitem_sat', 'params@submodules.HasItem.param.0.bias'): 1.15,
    ('tiny', 'hasitem_sat', 'params@submodules.HasItem.param.0.weight'): 1.52,
    ('tiny', 'hasitem_sat', 'params@submodules.HasItem.param.3.bias'): 7.3,
    ('tiny', 'hasitem_sat', 'params@submodules.HasItem.param.3.weight'): 1.53,
    # a one-element sum over 368 questions with heavy cancellation: measured 0.311
    ('h512', 'init', 'params@submodules.Temporal.relate.between.0.bias'): 0.39,
}
QUARTER = 0.25


def widen(geometry, batch, quantity):
    """the factor on the ordinary bound of a quantity: 1, or 4 x the ratio measured on the reference side (ILL_CONDITIONED)"""
    r = ILL_CONDITIONED.get((geometry, batch, quantity))
    return 1.0 if r is None else max(1.0, 4.0 * r)


def hold_to_a_quarter(table, prefix, measured):
    """The rule of both literal tables.  measured: {quantity: error / bound} of the oracle in fp32 against fp64.  A quantity that is
    not in `table` under `prefix` is under a quarter of its bound; a listed one is not above its listed figure (which is written with
    headroom: the fp32 sums differ between CPUs); no entry of the table is left without a measurement."""
    for what, ratio in measured.items():
        listed = table.get(prefix + (what,))
        if listed is None:
            assert ratio < QUARTER, (prefix, what, ratio)
        else:
            assert ratio <= listed, (prefix, what, ratio, listed)
    stale = [k for k in table if k[:len(prefix)] == prefix and k[len(prefix)] not in measured]
    assert not stale, stale


# ---- a saturated LSTM ----------------------------------------------------------------------------------------------------------
LSTM_CASES = {'Hh32': (32, 128, [5, 1, 9, 9, 3]), 'Hh256': (256, 300, [12] * 33)}
# N(0, 1) inputs x LSTM_INPUT_SCALE[mode]: 30 in the f32 mode; 3 in the bf16x3 mode, whose products carry 2^-17 of pre-activations
# that reach +-40 at x 30 (2e-4 on the outputs, against a bound of 1e-4).  The gates saturate through the +-20 on b_ih either way.
LSTM_INPUT_SCALE = {'f32': 30.0, 'bf16x3': 3.0}
# (case, matmul mode, quantity) -> error / bound of the written-out oracle LSTM in fp32 against fp64 on that mode's inputs, where it
# exceeds a quarter; the kernels then get 4 x it.  Measured by tests/test_value_edges_host.py, never on HIP output.
# Hh256, f32 mode: measured 0.270 (5.4e-6 against 2e-5), listed with a quarter of headroom.
LSTM_ILL_CONDITIONED = {
    ('Hh256', 'f32', 'out'): 0.34,
}


def lstm_widen(case, mode, quantity):
    r = LSTM_ILL_CONDITIONED.get((case, mode, quantity))
    return 1.0 if r is None else max(1.0, 4.0 * r)


def saturated_lstm(Hh, I, lens, dtype, scale=30.0):
    """({name: tensor} of a video encoder's eight tensors, [x_s [L_s, I]]) in `dtype`: the seed-4 weights of
    test_lstm_matches_explicit_oracle with b_ih shifted by +20 on every fourth unit of every gate and by -20 on the units after
    them, and N(0, 1) inputs x `scale` -- every gate (i, f, o at 0 and at 1, g at -1 and +1) is saturated on some units at every step,
    while the units in between stay in the gates' linear range"""
    config = dict(spec.DEFAULT_CONFIG, hidden_size=2 * Hh, video_size=I, max_video_length=64)
    w = {k: torch.from_numpy(v.copy()) for k, v in synth.make_weights(config, 4).items() if '.video_encoder.' in k}
    shift = torch.zeros(4 * Hh)
    shift[0::4], shift[1::4] = 20.0, -20.0
    for sfx in ('', '_reverse'):
        w[P + 'video_encoder.bias_ih_l0' + sfx] += shift
    xs = [torch.from_numpy(synth.normal(SEED, 'lstm/%d/%d/%d' % (Hh, I, s), (L, I))) * scale for s, L in enumerate(lens)]
    return {k: v.to(dtype) for k, v in w.items()}, [x.to(dtype) for x in xs]
