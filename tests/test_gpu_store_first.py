"""GPU test of the backward pass's first-touch stores (`-m gpu`): a reverse pass that stores the first contribution to a
gradient tile and clears only the tiles no chain stores must leave exactly the gradients of the pass that clears every arena
and adds every contribution (STAIR_BWD_KEEP_ARENAS after stair_plan_zero_grads, where the marks are ignored).  The decoder-only
step is bit-reproducible (test_training_step_is_bit_reproducible), so a single differing bit is a defect; -0 against +0 is the
one difference a store may make, and torch.equal takes the two for equal."""
import ctypes as C

import pytest
import torch

from stair_amd import spec, synth
from stair_amd._lib import lib, check

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _model(config, seed=0):
    from stair_amd.module_net import VideoNMN
    m = VideoNMN(config)
    w = synth.make_weights(config, seed)
    m.load_state_dict({k: torch.from_numpy(w[k].copy()) for k in spec.state_dict_keys(config)})
    return m.to(DEV)


@pytest.mark.parametrize('ragged', [False, True])
@pytest.mark.parametrize('shared', [False, True])
@pytest.mark.parametrize('n_q', [48, 256])
def test_store_first_equals_clear_and_add(n_q, shared, ragged):
    config = dict(spec.DEFAULT_CONFIG)
    T = 64
    qs = [synth.make_question(config, 21, i, T=T, forms=synth.ALL_FORMS, with_video=False) for i in range(n_q)]
    clips = n_q // 2 if shared else n_q
    g = torch.Generator().manual_seed(9)
    video = torch.randn(clips, T, config['video_size'], generator=g).to(DEV)
    vidx = [i % clips for i in range(n_q)] if shared else None
    vlen = None
    if ragged:
        vlen = [T - (i * 7) % 40 for i in range(clips)]
        for i, l in enumerate(vlen):
            video[i, l:] = 0
    question = torch.cat([torch.as_tensor(q['question']) for q in qs]).to(DEV)
    q_lens = [q['question'].shape[0] for q in qs]
    answers = torch.tensor([q['answer'] for q in qs], dtype=torch.int32, device=DEV)
    progs, spans = [q['nmn_program_list'] for q in qs], [q['prog_str_to_question_tokens'] for q in qs]

    model = _model(config, 5)
    for p in model.parameters():
        p.grad = torch.zeros_like(p)

    def one_pass(keep):
        for p in model.parameters():
            p.grad.zero_()
        res = model.run_programs(progs, spans, video, question, q_lens, train=True, video_index=vidx, video_len=vlen)
        if keep:
            res.zero_grad_arenas()
        loss = res.backward(answers, 1.0 / n_q, keep_arenas=keep)
        res.check()
        out = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
        for kind in ('vec', 'map', 'att'):
            out['arena.' + kind] = res.grad_arena(kind).clone()
        out['loss'] = loss.clone()
        a, b = C.c_int32(), C.c_int32()
        check(lib.stair_plan_store_first_counts(res._plan, C.byref(a), C.byref(b)))
        return out, a.value, b.value, res.info

    first, stored, cleared, info = one_pass(False)
    assert stored > 0 and stored + cleared == info.n_map + info.n_map_stage         # the case really runs the store path
    if shared:
        assert info.n_map_stage > 0
    added, _, _, _ = one_pass(True)
    assert float(first['arena.map'].abs().max()) > 0
    for name in added:
        assert int(first[name].isnan().sum()) == 0, name
        assert torch.equal(first[name], added[name]), '%s: %d elements differ' % (name, int((first[name] != added[name]).sum()))
    again, _, _, _ = one_pass(False)                    # and over the arenas the adding pass left behind: nothing stale is read
    for name in added:
        assert torch.equal(again[name], added[name]), name
