"""GPU tests of torch autograd through VideoNMN.logits (stair_amd/autograd.py, stair_plan_backward_dlogits): a loss that is not the
decoder CE, parameter gradients AND input gradients (video, question) against torch autograd of the oracle, the CE path against the
native CE backward, ragged / shared clips, bf16 clips, full size, autograd semantics and finite differences."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import nmn_oracle as O
from stair_amd import spec, synth
from helpers import load_golden, question_for

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


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


def _model(config, seed=0):
    from stair_amd.module_net import VideoNMN
    m = VideoNMN(config)
    w = synth.make_weights(config, seed)
    m.load_state_dict({k: torch.from_numpy(w[k].copy()) for k in spec.state_dict_keys(config)})
    return m.to(DEV)


def _weights(config, seed):
    names = [n for n, _ in spec.weight_table(config)]
    w = synth.make_weights(config, seed)
    return names, {k: torch.from_numpy(w[k].copy()).requires_grad_(True) for k in names}


def _R(n, A, seed=7):
    return torch.from_numpy(np.random.RandomState(seed).randn(n, A).astype(np.float32))


def _custom(logits, R):
    return (logits.log_softmax(-1) * R).sum()


def _oracle(config, seed, qs, R, frames=None):
    """Oracle parameter gradients and per-question input gradients of the custom loss."""
    names, w = _weights(config, seed)
    vids, ques, total = [], [], 0.0
    for i, q in enumerate(qs):
        q = dict(q)
        v = torch.as_tensor(q['video_features']).float()
        if frames is not None:
            v = v[:frames[i]]
        q['video_features'] = v.clone().requires_grad_(True)
        q['question'] = torch.as_tensor(q['question']).float().clone().requires_grad_(True)
        logits = O.forward(w, config, q, return_res_by_step=False, explicit_lstm=True)['logits']
        total = total + _custom(logits.unsqueeze(0), R[i:i + 1])
        vids.append(q['video_features']); ques.append(q['question'])
    total.backward()
    zero_if_none = lambda x: x.grad if x.grad is not None else torch.zeros_like(x)     # an input no program of the batch reads
    return names, w, [zero_if_none(v) for v in vids], [zero_if_none(q) for q in ques]


def _pack(qs, video_dtype=torch.float32):
    video = torch.stack([torch.as_tensor(q['video_features']) for q in qs]).to(DEV, video_dtype).contiguous()
    question = torch.cat([torch.as_tensor(q['question']) for q in qs]).to(DEV).contiguous()
    return ([q['nmn_program_list'] for q in qs], [q['prog_str_to_question_tokens'] for q in qs], video, question,
            [q['question'].shape[0] for q in qs], torch.tensor([q['answer'] for q in qs], dtype=torch.int32, device=DEV))


def _close(got, ref, rel, what):
    tol = rel * max(float(ref.abs().max()), 1e-3)
    err = float((got.float().cpu() - ref).abs().max())
    assert err < tol, (what, err, tol)


def _check_params(model, names, w, rel=2e-4):
    got = dict(model.named_parameters())
    for n in names:
        ref, g = w[n].grad, got[n].grad
        if ref is None:
            assert g is None or ('Filter.attention' in n and float(g.abs().max()) == 0.0), n      # untouched -> None
            continue
        assert g is not None, n
        _close(g, ref, rel, n)


def _custom_run(config, seed, qs, T=None, rel=2e-4):
    R = _R(len(qs), config['answer_vocab_length'])
    names, w, gv, gq = _oracle(config, seed, qs, R)
    model = _model(config, seed)
    progs, spans, video, question, q_lens, _ = _pack(qs)
    video.requires_grad_(True); question.requires_grad_(True)
    logits = model.logits(progs, spans, video, question, q_lens)
    assert logits.grad_fn is not None
    _custom(logits, R.to(DEV)).backward()
    _check_params(model, names, w, rel)
    _close(video.grad, torch.stack(gv), rel, 'd_video')
    _close(question.grad, torch.cat(gq), rel, 'd_question')
    return model


@pytest.mark.parametrize('name', ['tiny_conv', 'tiny_linear', 'tiny_conv_t24'])
def test_custom_loss_matches_autograd_of_oracle(name, matmul):
    """All 12 program forms, a loss that is not CE: every parameter gradient, d_video and d_question."""
    z, meta = load_golden(name)
    qs = [question_for(meta, q) for q in meta['questions']]
    _custom_run(meta['config'], meta['seed'], qs)


def test_cross_entropy_through_autograd_equals_native_backward(matmul):
    z, meta = load_golden('tiny_conv')
    config = meta['config']
    qs = [question_for(meta, q) for q in meta['questions']]
    s = 1.0 / len(qs)
    model = _model(config, meta['seed'])
    progs, spans, video, question, q_lens, answers = _pack(qs)
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    res = model.run_programs(progs, spans, video, question, q_lens, train=True)
    res.backward(answers, s)
    native = {n: p.grad.clone() for n, p in model.named_parameters()}
    for p in model.parameters():
        p.grad = None
    logits = model.logits(progs, spans, video, question, q_lens)
    (F.cross_entropy(logits, answers.long(), reduction='sum') * s).backward()
    # (the two seeds differ by the fp32 rounding of two softmax implementations, ~1e-7 relative: a tensor whose gradient is a sum
    # that cancels down to ~1e-6 -- Localize's keyword bias -- sees that as ~1e-10 absolute, hence the floor)
    for n, p in model.named_parameters():
        if p.grad is None:
            assert float(native[n].abs().max()) == 0.0, n
            continue
        assert float((p.grad - native[n]).abs().max()) <= 1e-5 * float(native[n].abs().max()) + 1e-9, n


@pytest.mark.parametrize('H,L,T', [(64, 40, 7), (128, 40, 33), (128, 2, 2), (512, 8, 8), (512, 40, 33), (64, 100, 100)])
def test_custom_loss_on_odd_shapes(H, L, T, f32):
    config = dict(spec.DEFAULT_CONFIG, hidden_size=H, video_size=128, answer_vocab_length=16, max_video_length=L, object_types=10)
    qs = synth.make_questions(config, 5, 12, forms=synth.ALL_FORMS, T=T)
    _custom_run(config, 1, qs)


def test_ragged_clips_input_gradients(f32):
    config = dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, answer_vocab_length=16, max_video_length=64, object_types=10)
    T = 40
    qs = synth.make_questions(config, 9, 8, forms=synth.ALL_FORMS, T=T)
    frames = np.random.RandomState(3).randint(9, T + 1, size=len(qs)).astype(np.int32)
    frames[0] = T
    R = _R(len(qs), config['answer_vocab_length'])
    names, w, gv, gq = _oracle(config, 1, qs, R, frames=frames)
    model = _model(config, 1)
    progs, spans, video, question, q_lens, _ = _pack(qs)
    mask = (torch.arange(T, device=DEV)[None, :] < torch.as_tensor(frames, device=DEV)[:, None]).unsqueeze(-1)
    video = (video * mask).contiguous().requires_grad_(True)
    question.requires_grad_(True)
    _custom(model.logits(progs, spans, video, question, q_lens, video_len=frames), R.to(DEV)).backward()
    dv = video.grad.cpu()
    for i, f in enumerate(frames):
        assert torch.count_nonzero(dv[i, f:]) == 0, i                      # exact zeros past the clip's length
        _close(dv[i, :f], gv[i], 2e-4, 'd_video[%d]' % i)
    _close(question.grad, torch.cat(gq), 2e-4, 'd_question')
    _check_params(model, names, w)


def test_shared_clip_input_gradients_equal_expanded_batch(matmul):
    z, meta = load_golden('tiny_conv')
    config = meta['config']
    qs = [question_for(meta, q) for q in meta['questions']]
    R = _R(len(qs), config['answer_vocab_length']).to(DEV)
    model = _model(config, meta['seed'])
    progs, spans, video, question, q_lens, _ = _pack(qs)
    index = [i % 3 for i in range(len(qs))]
    clips = video[:3].clone()
    expanded = clips[index].contiguous().requires_grad_(True)
    _custom(model.logits(progs, spans, expanded, question, q_lens), R).backward()
    ref = torch.zeros_like(clips).index_add_(0, torch.tensor(index, device=DEV), expanded.grad)
    shared = clips.clone().requires_grad_(True)
    _custom(model.logits(progs, spans, shared, question, q_lens, video_index=index), R).backward()
    tol = (2e-5 if matmul == 'f32' else 1e-4) * max(float(ref.abs().max()), 1e-3)
    assert float((shared.grad - ref).abs().max()) < tol


def test_bf16_clips_match_fp32_path_on_rounded_values():
    """bf16 clips (bf16x3 mode): d_video w.r.t. the stored values equals the fp32 path fed the same rounded values."""
    config = dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, answer_vocab_length=16, max_video_length=40, object_types=10)
    qs = synth.make_questions(config, 4, 12, forms=synth.ALL_FORMS, T=40)
    R = _R(len(qs), config['answer_vocab_length']).to(DEV)
    model = _model(config, 2)
    progs, spans, video, question, q_lens, _ = _pack(qs)
    v16 = video.to(torch.bfloat16).contiguous()
    out = {}
    for name, v in (('bf16', v16.clone()), ('f32', v16.float().contiguous())):
        v.requires_grad_(True)
        for p in model.parameters():
            p.grad = None
        _custom(model.logits(progs, spans, v, question, q_lens), R).backward()
        assert v.grad.dtype == v.dtype
        out[name] = (v.grad.float(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    # the bf16 gradient is rounded to bf16 on return (its dtype): compare at that rounding, 2^-8 relative
    ref = out['f32'][0]
    assert float((out['bf16'][0] - ref).abs().max()) < 4e-3 * float(ref.abs().max()) + 1e-6
    for n, g in out['f32'][1].items():
        assert float((out['bf16'][1][n] - g).abs().max()) < 1e-4 * max(float(g.abs().max()), 1e-3), n
    # and the fp32 values themselves, through the thin wrapper
    d = {}
    for name, v in (('bf16', v16), ('f32', v16.float().contiguous())):
        for p in model.parameters():
            p.grad = torch.zeros_like(p)
        res = model.run_programs(progs, spans, v, question, q_lens, train=True)
        dv = torch.empty(v.shape, dtype=torch.float32, device=DEV)
        res.backward_dlogits(torch.ones_like(res.logits) * 0.01, d_video=dv)
        d[name] = dv
    assert float((d['bf16'] - d['f32']).abs().max()) < 2e-4 * float(d['f32'].abs().max())


def test_full_size_input_gradients(matmul):
    config = dict(spec.DEFAULT_CONFIG)
    qs = [synth.make_question(config, 21, i, form=f) for i, f in enumerate(['P0', 'P2', 'P3', 'P5', 'C0', 'C1'])]
    R = _R(len(qs), config['answer_vocab_length'])
    names, w, gv, gq = _oracle(config, 3, qs, R)
    model = _model(config, 3)
    progs, spans, video, question, q_lens, _ = _pack(qs)
    video.requires_grad_(True); question.requires_grad_(True)
    _custom(model.logits(progs, spans, video, question, q_lens), R.to(DEV)).backward()
    lim = 3e-3 if matmul == 'f32' else 1e-2          # test_full_size_backward_sample's criterion (ReLU-kink flips)
    for g, ref, what in ((video.grad, torch.stack(gv), 'd_video'), (question.grad, torch.cat(gq), 'd_question')):
        g = g.cpu()
        rel_l2 = float((g - ref).norm() / ref.norm().clamp_min(1e-12))
        assert rel_l2 < lim, (what, rel_l2)
        assert float((g - ref).abs().max()) < 0.05 * float(ref.abs().max()) + 3e-6, what


def _sem_batch(seed=0, n=6):
    config = dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, answer_vocab_length=16, max_video_length=40, object_types=10)
    qs = synth.make_questions(config, seed, n, forms=synth.ALL_FORMS, T=40, start=100 * seed)
    return config, qs


def test_autograd_semantics():
    config, qs = _sem_batch(0)
    _, qs2 = _sem_batch(1)
    model = _model(config, 0)
    params = [p for _, p in model.named_parameters()]
    R = _R(len(qs), config['answer_vocab_length']).to(DEV)
    a, b = _pack(qs), _pack(qs2)

    def loss_of(batch):
        progs, spans, video, question, q_lens, _ = batch
        return _custom(model.logits(progs, spans, video, question, q_lens), R)

    # torch.autograd.grad
    g1 = torch.autograd.grad(loss_of(a), params, allow_unused=True)
    assert all(p.grad is None for p in params)
    # .grad accumulates over two backward() calls
    loss_of(a).backward()
    loss_of(a).backward()
    for p, g in zip(params, g1):
        if g is None:
            assert p.grad is None
        else:
            assert torch.allclose(p.grad, 2 * g, rtol=1e-6, atol=1e-7 * float(g.abs().max()))
    # two outstanding forwards, one backward of their sum == two separate backwards
    gb = torch.autograd.grad(loss_of(b), params, allow_unused=True)
    la, lb = loss_of(a), loss_of(b)
    gs = torch.autograd.grad(la + lb, params, allow_unused=True)
    for x, y, s in zip(g1, gb, gs):
        ref = (x if x is not None else 0) + (y if y is not None else 0)
        if s is None:
            assert x is None and y is None
        else:
            assert torch.allclose(s, ref, rtol=1e-5, atol=1e-6 * float(ref.abs().max()))
    # a second backward through the same logits raises, with and without retain_graph
    loss = loss_of(a)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='backward'):
        loss.backward(retain_graph=True)
    loss = loss_of(a)
    loss.backward()
    with pytest.raises(RuntimeError):
        loss.backward()
    # no_grad: an inference plan, bit-identical to run_programs
    progs, spans, video, question, q_lens, answers = a
    with torch.no_grad():
        lg = model.logits(progs, spans, video, question, q_lens)
    assert lg.grad_fn is None
    assert torch.equal(lg, model.run_programs(progs, spans, video, question, q_lens).logits)
    # a Trainer used afterwards binds its own gradient buffers again: same step as on a fresh model
    from stair_amd.train import Trainer
    fresh = _model(config, 0)
    for m in (model, fresh):
        for p in m.parameters():
            p.grad = None
        tr = Trainer(m, lr=2e-4, scheduler_total_iters=10, skip_untouched='ever', dropout=0.0)
        tr.step(progs, spans, video, question, q_lens, answers)
    torch.cuda.synchronize()
    for (n, p), (_, q) in zip(model.named_parameters(), fresh.named_parameters()):
        assert torch.equal(p.detach(), q.detach()), n


def test_finite_differences(f32):
    config, qs = _sem_batch(2, n=4)
    model = _model(config, 0)
    progs, spans, video, question, q_lens, _ = _pack(qs)
    R = _R(len(qs), config['answer_vocab_length']).to(DEV)
    video.requires_grad_(True); question.requires_grad_(True)
    _custom(model.logits(progs, spans, video, question, q_lens), R).backward()
    gen = torch.Generator(device='cpu').manual_seed(5)
    with torch.no_grad():
        for x, g in ((video, video.grad), (question, question.grad)):
            # a random direction with a component along the gradient, so that the directional derivative stands well clear of
            # the forward pass's rounding noise divided by the step
            r = torch.randn(x.shape, generator=gen).to(DEV)
            u = r / r.norm() + g / g.norm()
            u /= u.norm()
            eps = 1e-4 * float(x.norm())             # a short step: few ReLU / max kinks lie inside it
            base = x.detach().clone()
            vals = []
            for sgn in (1.0, -1.0):
                x.copy_(base + sgn * eps * u)
                vals.append(float(_custom(model.logits(progs, spans, video, question, q_lens).double(), R.double())))
            x.copy_(base)
            fd = (vals[0] - vals[1]) / (2 * eps)
            an = float((g * u).sum())
            assert abs(fd - an) < 1e-2 * abs(an) + 1e-5, (fd, an)
