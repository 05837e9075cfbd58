"""The device-resident clip library and word table on the GPU (`-m gpu`): stair_gather_clips / stair_gather_words against torch, and
every pass fed by row ids (run_programs, Trainer.step, logits under autograd, encode_clips, two data-parallel ranks) against the same
pass fed densely.  No tolerance anywhere: the gathers must produce the very bytes the host packing produces, and everything
downstream is then the same launches on the same data.

Shapes: the configuration of test_training_step_is_bit_reproducible (hidden size 512, default matmul mode -- the one in which a
training step is bit-reproducible) with V = 128 and max_video_length = 40; 48 questions over the twelve program forms about five
clips of 17, 3, 24, 17 and 24 frames, named out of order and with repeats, from a library of eight (a 40-frame clip among the unused)."""
import ctypes as C
import functools
import os
import socket
import tempfile

import numpy as np
import pytest
import torch

from stair_amd import spec, synth
from stair_amd._lib import check, lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CONFIG = dict(spec.DEFAULT_CONFIG, video_size=128, max_video_length=40)
LIB_LENS = [17, 3, 24, 24, 40, 3, 17, 9]
USED = [6, 1, 2, 0, 3]                                  # library rows in order of first use: 17, 3, 24, 17, 24 frames
N_Q = 48
ROWS = [USED[(q * 3 + q // 5) % 5] if q >= 5 else USED[q] for q in range(N_Q)]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- the kernels ------------------------------------------------------------------------------------------------------------------
def _gather_clips(store, rows, lens, T):
    n, (N, cap, V) = len(rows), store.shape
    out = torch.full((n, T, V), float('nan'), dtype=store.dtype, device=DEV)
    d_rows = torch.tensor(rows, dtype=torch.int32, device=DEV)
    d_lens = torch.tensor(lens, dtype=torch.int32, device=DEV) if lens is not None else None
    check(lib.stair_gather_clips(C.c_void_p(store.data_ptr()), store.element_size(), cap * V, cap, V, C.c_void_p(d_rows.data_ptr()),
                                 C.c_void_p(d_lens.data_ptr() if d_lens is not None else None), n, T, C.c_void_p(out.data_ptr()), _stream()))
    return out


def _library_tensor(N, cap, V, dtype, lens, seed):
    """[N, cap, V] random clips with NaN behind every clip's end (lens[r] frames of row r are data)"""
    store = torch.randn(N, cap, V, generator=torch.Generator().manual_seed(seed)).to(dtype)
    for r, L in enumerate(lens):
        store[r, L:] = float('nan')
    return store.to(DEV)


def _expect(store, rows, lens, T):
    idx = torch.tensor(rows, dtype=torch.long, device=DEV)
    cap = store.shape[1]
    src = store.index_select(0, idx)[:, :min(cap, T)]
    want = torch.zeros(len(rows), T, store.shape[2], dtype=store.dtype, device=DEV)
    keep = torch.arange(min(cap, T), device=DEV)[None, :] < torch.tensor(lens, device=DEV)[:, None]
    want[:, :min(cap, T)] = torch.where(keep[:, :, None], src, torch.zeros_like(src))
    return want


@pytest.mark.parametrize('T', [5, 9])
@pytest.mark.parametrize('n', [1, 17])
def test_gather_clips_bf16_against_index_select(T, n):
    cap, V, N = 9, 32, 6
    lib_lens = [1, T, 2, min(T, 4), T, 3]               # 1, T and values between
    store = _library_tensor(N, cap, V, torch.bfloat16, lib_lens, 1)
    rows = [N - 1 - (i % N) for i in range(n)] if n > 1 else [1]        # reversed, with repeats
    lens = [lib_lens[r] for r in rows]
    got = _gather_clips(store, rows, lens, T)
    torch.cuda.synchronize()
    want = _expect(store, rows, lens, T)
    assert not bool(torch.isnan(got.float()).any())
    assert torch.equal(got, want)
    for v, L in enumerate(lens):
        assert bool((got[v, L:].view(torch.int16) == 0).all())          # zeros exact: +0, every bit


def test_gather_clips_fp32_rows_of_528_bytes():
    cap, V, N, T = 9, 132, 5, 7                         # V a multiple of 4 but not of 32
    lib_lens = [7, 1, 4, 6, 2]
    store = _library_tensor(N, cap, V, torch.float32, lib_lens, 2)
    rows = [4, 3, 2, 1, 0, 0, 4, 2]
    lens = [lib_lens[r] for r in rows]
    got = _gather_clips(store, rows, lens, T)
    torch.cuda.synchronize()
    assert torch.equal(got, _expect(store, rows, lens, T))
    assert bool((got.view(torch.int32)[torch.isnan(store.index_select(0, torch.tensor(rows, device=DEV))[:, :T])] == 0).all())


def test_gather_clips_spanning_several_grid_chunks():
    cap = T = 64                                        # a clip of 64 x 2048 bf16 is 16384 16-byte units: 8 chunks of the grid
    lib_lens = [64, 1, 37, 50]
    store = _library_tensor(4, cap, 2048, torch.bfloat16, lib_lens, 3)
    rows = [2, 0, 3]
    lens = [lib_lens[r] for r in rows]
    got = _gather_clips(store, rows, lens, T)
    torch.cuda.synchronize()
    assert torch.equal(got, _expect(store, rows, lens, T)) and not bool(torch.isnan(got.float()).any())


@pytest.mark.parametrize('T', [5, 9, 12])
def test_gather_clips_without_lens(T):
    cap, V = 9, 32
    frames = min(cap, T)                                # lens == NULL: every clip has min(rows_cap, T) frames
    store = _library_tensor(4, cap, V, torch.bfloat16, [frames] * 4, 4)
    rows = [3, 1, 1, 0, 2]
    got = _gather_clips(store, rows, None, T)
    torch.cuda.synchronize()
    assert torch.equal(got, _expect(store, rows, [frames] * len(rows), T)) and not bool(torch.isnan(got.float()).any())


def test_gather_clips_refuses_bad_scalars():
    from stair_amd._lib import StairError
    store = torch.zeros(2, 4, 32, dtype=torch.bfloat16, device=DEV)
    idx = torch.zeros(2, dtype=torch.int32, device=DEV)
    out = torch.zeros(2, 4, 32, dtype=torch.bfloat16, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    for args, msg in (((p(store), 3, 128, 4, 32, p(idx), None, 2, 4, p(out)), 'elem_bytes must be 2'),
                      ((p(store), 2, 128, 4, 28, p(idx), None, 2, 4, p(out)), 'multiple of 16 bytes'),
                      ((p(store), 2, 64, 4, 32, p(idx), None, 2, 4, p(out)), 'clip_stride_elems must be at least rows_cap'),
                      ((C.c_void_p(store.data_ptr() + 2), 2, 128, 4, 32, p(idx), None, 2, 4, p(out)), '16-byte aligned'),
                      ((p(store), 2, 128, 4, 32, None, None, 2, 4, p(out)), 'null argument')):
        with pytest.raises(StairError, match=msg):
            check(lib.stair_gather_clips(*args, _stream()))
    with pytest.raises(StairError, match='E must be a positive multiple of 4'):
        check(lib.stair_gather_words(p(out), 6, 4, p(idx), 2, p(out), _stream()))


@pytest.mark.parametrize('E', [4, 300])
@pytest.mark.parametrize('n', [1, 1000])
def test_gather_words_against_index_select(E, n):
    rows = 37
    table = torch.randn(rows, E, generator=torch.Generator().manual_seed(E)).to(DEV)
    ids = (np.arange(n) * 7 % rows).astype(np.int32)
    ids[0], ids[-1] = rows - 1, 0                       # the last and the first table row; with n = 1000 every row repeats
    if n > 2:
        ids[1] = ids[2] = 0
    d_ids = torch.from_numpy(ids).to(DEV)
    out = torch.full((n, E), float('nan'), device=DEV)
    check(lib.stair_gather_words(C.c_void_p(table.data_ptr()), E, rows, C.c_void_p(d_ids.data_ptr()), n, C.c_void_p(out.data_ptr()), _stream()))
    torch.cuda.synchronize()
    assert torch.equal(out, table.index_select(0, d_ids.long()))


# ---- the passes -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _weights(max_len):
    return synth.make_weights(dict(CONFIG, max_video_length=max_len), 5)


def _model(config=CONFIG, supervised=False):
    from stair_amd import losses as L
    from stair_amd.module_net import VideoNMN
    w = _weights(config['max_video_length'])
    model = VideoNMN(config, pretrain_modules=set(L.CRITERION_MODULES) if supervised else set())
    model.load_state_dict({k: torch.from_numpy(w[k].copy()) for k in spec.state_dict_keys(config)})
    return model.to(DEV)


@functools.lru_cache(maxsize=None)
def _questions(max_len=40, gold_T=None):
    config = dict(CONFIG, max_video_length=max_len)
    qs = [synth.make_question(config, 21, i, form=synth.ALL_FORMS[i % 12], with_video=False) for i in range(N_Q)]
    if gold_T:
        for q in qs:
            sg = synth.make_gold(config, 3, q, T=gold_T, keep=1.0)
            q['sg_res_by_step'] = {k: ([(n, torch.from_numpy(np.asarray(e))) for n, e in v] if isinstance(v, list) else v) for k, v in sg.items()}
    return qs


def _dense(clips, rows):
    """what the host packing hands a pass whose questions ask about the clips `rows`: the distinct clips in order of first use, padded
    with zeros to the longest of them, the clip of every question and the clips' lengths"""
    first_use = list(dict.fromkeys(int(r) for r in rows))
    lens = [int(clips[r].shape[0]) for r in first_use]
    video = torch.stack([torch.nn.functional.pad(clips[r], (0, 0, 0, max(lens) - clips[r].shape[0])) for r in first_use]).to(DEV).contiguous()
    return dict(video=video, video_index=[first_use.index(int(r)) for r in rows], video_len=lens)


@functools.lru_cache(maxsize=None)
def _inputs(dtype, lens=tuple(LIB_LENS), max_len=40, gold_T=None):
    """One batch in both forms, built once and left unchanged.  Dense: the used clips packed on the host in order of first use,
    padded to the longest with zeros, and the embedded question rows.  By row id: a ClipLibrary of all the clips (made from a padded
    tensor with NaN behind each clip's end) with the library row of every question, and a WordTable that holds the question rows
    shuffled among rows no question reads, with the row of every word."""
    from stair_amd.clip_library import ClipLibrary
    from stair_amd.data import WordTable
    qs = _questions(max_len, gold_T)
    V, cap = CONFIG['video_size'], max(lens)
    g = torch.Generator().manual_seed(7)
    clips = [torch.randn(L, V, generator=g).to(dtype) for L in lens]
    padded = torch.full((len(lens), cap, V), float('nan'), dtype=dtype)
    for r, c in enumerate(clips):
        padded[r, :c.shape[0]] = c
    library = ClipLibrary(cap, V, DEV, dtype)
    library.add(padded, ids=['clip%d' % r for r in range(len(lens))], video_len=list(lens))
    first_use = list(dict.fromkeys(ROWS))
    dense = _dense(clips, ROWS)
    question = torch.cat([torch.as_tensor(q['question']) for q in qs]).to(torch.float32)
    n_words = question.shape[0]
    perm = torch.randperm(n_words + 13, generator=g)
    table = torch.randn(n_words + 13, question.shape[1], generator=g)
    ids = perm[:n_words]
    table[ids] = question
    words = WordTable(['w%d' % i for i in range(n_words + 13)], table.to(DEV).contiguous())
    head = ([q['nmn_program_list'] for q in qs], [q['prog_str_to_question_tokens'] for q in qs])
    answers = torch.tensor([q['answer'] for q in qs], dtype=torch.int32, device=DEV)
    return dict(head=head, q_lens=[q['question'].shape[0] for q in qs], answers=answers, dense=dense, question=question.to(DEV).contiguous(),
                library=library, clips=clips, rows=np.asarray(ROWS, np.int32), words=words, ids=ids.numpy().astype(np.int32), qs=qs, first_use=first_use)


def _nodes(res):
    out = []
    for q, prog in enumerate(res._programs):
        for i in range(len(prog)):
            v = res.node(q, i)
            out.append(v.clone() if isinstance(v, torch.Tensor) else v)
    return out


def _same_pass(model, b):
    """run_programs by row ids against the dense call: logits, pred and every node of every question, bit for bit"""
    a = model.run_programs(*b['head'], b['dense']['video'], b['question'], b['q_lens'], video_index=b['dense']['video_index'],
                           video_len=b['dense']['video_len'])
    a_logits, a_pred, a_nodes, a_T, a_frames = a.logits.clone(), a.pred.clone(), _nodes(a), a.info.T, a.question_frames
    r = model.run_programs(*b['head'], None, None, b['q_lens'], video_index=b['rows'], library=b['library'], question_ids=b['ids'],
                           words=b['words'])
    torch.cuda.synchronize()
    assert float(a_logits.abs().max()) > 0 and r.info.T == a_T
    assert torch.equal(r.logits, a_logits) and torch.equal(r.pred, a_pred)
    assert (a_frames is None and r.question_frames is None) or list(a_frames) == list(r.question_frames)
    assert torch.equal(r._video, b['dense']['video']) and torch.equal(r._question, b['question'])     # the very bytes of the host packing
    assert list(r._src.library_rows) == b['first_use']
    r_nodes = _nodes(r)
    assert len(r_nodes) == len(a_nodes)
    for x, y in zip(a_nodes, r_nodes):
        assert torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_forward_by_row_ids_equals_the_dense_pass(dtype):
    b = _inputs(dtype)
    assert b['dense']['video'].shape[1] == 24 and sorted(set(b['dense']['video_len'])) == [3, 17, 24]
    _same_pass(_model(), b)


def test_forward_with_every_clip_at_full_length():
    b = _inputs(torch.bfloat16, lens=(24,) * 8)                  # video_len collapses to None on both sides
    model = _model()
    assert model._clip_source(N_Q, None, b['rows'], None, library=b['library']).lens is None
    _same_pass(model, b)


def test_forward_at_a_linear_temporal_configuration():
    config = dict(CONFIG, max_video_length=8)
    _same_pass(_model(config), _inputs(torch.bfloat16, lens=(8,) * 8, max_len=8))


def test_forward_batch_and_predict_look_clips_up_by_video_id():
    from stair_amd import evaluate
    b = _inputs(torch.float32)
    model = _model()
    host = b['library'].clips.cpu()
    items = [dict(q, video_id='clip%d' % r, video_features=host[r, :LIB_LENS[r]].clone()) for q, r in zip(b['qs'], ROWS)]
    a = model.forward_batch(items)
    a_logits = a.logits.clone()
    r = model.forward_batch([{k: v for k, v in d.items() if k != 'video_features'} for d in items], clip_library=b['library'])
    torch.cuda.synchronize()
    assert torch.equal(r.logits, a_logits)
    assert evaluate.predict(model, items, batch_size=32, clip_library=b['library']) == evaluate.predict(model, items, batch_size=32)


def _steps(b, by_rows, supervised=False, **trainer_kw):
    from stair_amd.train import Trainer
    tr = Trainer(_model(supervised=supervised), lr=1e-3, **trainer_kw)
    out = []
    for it in range(2):
        qs = b['qs'] if supervised else None
        if by_rows:
            loss, res = tr.step(*b['head'], None, None, b['q_lens'], b['answers'], questions=qs, video_index=b['rows'], library=b['library'],
                                question_ids=b['ids'], words=b['words'])
        else:
            loss, res = tr.step(*b['head'], b['dense']['video'], b['question'], b['q_lens'], b['answers'], questions=qs,
                                video_index=b['dense']['video_index'], video_len=b['dense']['video_len'])
        out += [loss.clone(), tr.flat_g.clone()]
    tr.check()
    return out + [tr.flat_p.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone(), tr.steps.clone()]


@pytest.mark.parametrize('case', ['plain', 'supervised', 'dropout_clipped'])
def test_two_steps_by_row_ids_equal_two_dense_steps(case):
    kw = dict(plain=dict(dropout=0.0), supervised=dict(dropout=0.0, contrastive_window=8),
              dropout_clipped=dict(dropout=0.25, dropout_seed=11, max_grad_norm=0.5))[case]
    b = _inputs(torch.bfloat16, gold_T=24 if case == 'supervised' else None)
    dense = _steps(b, False, supervised=case == 'supervised', **kw)
    rows = _steps(b, True, supervised=case == 'supervised', **kw)
    names = ('loss0', 'flat_g0', 'loss1', 'flat_g1', 'flat_p', 'exp_avg', 'exp_avg_sq', 'steps')
    assert float(dense[1].abs().max()) > 0 and not torch.equal(dense[1], dense[3])
    for nme, x, y in zip(names, dense, rows):
        assert torch.equal(x, y), nme


def test_encode_clips_from_the_library():
    b = _inputs(torch.bfloat16)
    model = _model()
    host = b['library'].clips.cpu()
    clips = [host[r, :L].clone() for r, L in enumerate(LIB_LENS)]
    want = model.encode_clips(clips, ids=b['library'].ids)
    got = model.encode_clips(library=b['library'])
    torch.cuda.synchronize()
    assert got.lengths.tolist() == want.lengths.tolist() == LIB_LENS and torch.equal(got.enc, want.enc)
    assert got.rows(['clip3', 'clip0']).tolist() == [3, 0]
    some = model.encode_clips(library=b['library'], ids=['clip6', 'clip1', 'clip2'])
    assert some.lengths.tolist() == [17, 3, 24] and torch.equal(some.enc, model.encode_clips([clips[6], clips[1], clips[2]]).enc)
    a = model.run_programs(*b['head'], None, b['question'], b['q_lens'], clips=want, video_index=b['rows']).logits.clone()
    r = model.run_programs(*b['head'], None, b['question'], b['q_lens'], clips=got, video_index=b['rows']).logits
    torch.cuda.synchronize()
    assert torch.equal(a, r) and float(a.abs().max()) > 0


def test_logits_under_autograd_by_row_ids():
    b = _inputs(torch.bfloat16)
    grads = []
    for by_rows in (False, True):
        model = _model()
        if by_rows:
            out = model.logits(*b['head'], None, None, b['q_lens'], video_index=b['rows'], library=b['library'], question_ids=b['ids'],
                               words=b['words'])
        else:
            out = model.logits(*b['head'], b['dense']['video'], b['question'], b['q_lens'], video_index=b['dense']['video_index'],
                               video_len=b['dense']['video_len'])
        assert out.grad_fn is not None
        torch.nn.functional.cross_entropy(out, b['answers'].long(), label_smoothing=0.1).backward()
        grads.append({k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
    torch.cuda.synchronize()
    assert grads[0].keys() == grads[1].keys() and any('video_encoder' in k for k in grads[0])
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k
    with pytest.raises(ValueError, match='library= given together with a video= that requires grad: a library is data'):
        model.logits(*b['head'], b['dense']['video'].float().requires_grad_(True), None, b['q_lens'], video_index=b['rows'],
                     library=b['library'], question_ids=b['ids'], words=b['words'])


# ---- two data-parallel ranks --------------------------------------------------------------------------------------------------------
def _dp_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    from stair_amd.train import Trainer
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        b = _inputs(torch.bfloat16)
        mine = list(range(rank, N_Q, world))
        head = ([b['head'][0][i] for i in mine], [b['head'][1][i] for i in mine])
        q_lens, answers = [b['q_lens'][i] for i in mine], b['answers'][mine]
        off = np.concatenate([[0], np.cumsum(b['q_lens'])])
        word_pos = np.concatenate([np.arange(off[i], off[i + 1]) for i in mine])
        state = {}
        for by_rows in (False, True):           # the same rank runs the same shard both ways, one step each, in the same group
            tr = Trainer(_model(), world=world, rank=rank, dropout=0.0, lr=1e-3, global_batch=N_Q)
            if by_rows:                         # every rank holds the whole library and the whole table
                loss, _ = tr.step(*head, None, None, q_lens, answers, video_index=b['rows'][mine], library=b['library'],
                                  question_ids=b['ids'][word_pos], words=b['words'])
            else:                               # the dense call gets its shard's clips packed on the host
                dense = _dense(b['clips'], b['rows'][mine])
                loss, _ = tr.step(*head, dense['video'], b['question'][torch.from_numpy(word_pos).to(DEV)].contiguous(), q_lens, answers,
                                  video_index=dense['video_index'], video_len=dense['video_len'])
            tr.check()
            state[by_rows] = [t.cpu().clone() for t in (loss, tr.flat_g, tr.flat_p, tr.exp_avg, tr.exp_avg_sq, tr.steps)]
        torch.save(state, os.path.join(out_dir, 'rank%d.pt' % rank))
    finally:
        dist.destroy_process_group()


def test_two_rank_step_by_row_ids_equals_the_dense_two_rank_step():
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_dp_worker, args=(2, port, d), nprocs=2, join=True)
        ranks = [torch.load(os.path.join(d, 'rank%d.pt' % r)) for r in range(2)]
    for r in ranks:
        assert float(r[False][1].abs().max()) > 0
        for nme, x, y in zip(('loss', 'flat_g', 'flat_p', 'exp_avg', 'exp_avg_sq', 'steps'), r[False], r[True]):
            assert torch.equal(x, y), nme
    assert torch.equal(ranks[0][True][2], ranks[1][True][2])        # both ranks hold the same weights after the step
