"""Stopping and resuming at world = 2 (`-m gpu`): two processes on one card, ranks of a gloo group, with the questions, the model,
the round-robin shards and the packing of tests/test_gpu_dp.py at the sizes of its bit-identical case (its `full_size`: the
default configuration with 40 frames, stored-bf16 clips, a ragged 7 + 6 split).  Every rank first takes two uninterrupted
steps; then a fresh Trainer takes step A, rank 0 writes the checkpoint, BOTH ranks tear down, load the same files and take
step B.  Dropout is on: its masks are a function of dropout_seed + iters * world + rank, so a resumed rank draws the masks of
its own second step only if `iters` came back.  The learning rate changes between the steps (scheduler_total_iters = 3)."""
import gc
import os
import tempfile

import pytest
import torch

import test_gpu_dp as DP
from stair_amd import spec

pytestmark = pytest.mark.gpu


def _trainer(model, rank, world):
    from stair_amd.train import Trainer
    return Trainer(model, world=world, rank=rank, dropout=0.25, dropout_seed=11, contrastive_window=DP.WINDOW, lr=1e-3,
                   scheduler_total_iters=3)


def _step(tr, mine, dev):
    progs, spans, video, question, q_lens, answers = DP._pack(mine, dev, True)
    loss, _ = tr.step(progs, spans, video, question, q_lens, answers)
    return loss.cpu().clone(), tr.flat_g.cpu().clone()


def _snapshot(tr, steps):
    tr.check()
    return {'params': tr.flat_p.cpu().clone(), 'exp_avg': tr.exp_avg.cpu().clone(), 'exp_avg_sq': tr.exp_avg_sq.cpu().clone(),
            'steps': tr.steps.cpu().clone(), 'touched': tr.touched.cpu().clone(), 'iters': tr.iters, 'seen': tr.questions_seen,
            'loss': [s[0] for s in steps], 'grad': [s[1] for s in steps]}


def _rank(rank, world, port, out_dir):
    import torch.distributed as dist
    from stair_amd import data as D, losses as L
    DP.CONFIG = dict(spec.DEFAULT_CONFIG, max_video_length=40)            # in this child process: what DP._worker(full_size=True) sets
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        dev = torch.device('cuda', 0)
        mine = DP._questions(False)[rank::world]
        # run 1: two uninterrupted steps
        tr = _trainer(DP._model(dev), rank, world)
        out = {'run1': _snapshot(tr, [_step(tr, mine, dev), _step(tr, mine, dev)])}
        del tr
        gc.collect()
        # run 2: step A, rank 0 saves, both ranks tear down and load what rank 0 wrote, step B
        ck = os.path.join(out_dir, 'ck')
        tr = _trainer(DP._model(dev), rank, world)
        steps = [_step(tr, mine, dev)]
        if rank == 0:
            D.save_checkpoint(ck, tr.model, DP.CONFIG, tr)
        else:
            tr.check()
        del tr
        gc.collect()
        torch.cuda.empty_cache()
        dist.barrier()                                                    # the files are complete before any rank reads them
        model, _ = D.load_checkpoint(ck, device=dev, pretrain_modules=L.CRITERION_MODULES)
        tr = _trainer(model, rank, world)
        tr.load_state_dict(D.load_trainer_state(ck))
        steps.append(_step(tr, mine, dev))
        out['run2'] = _snapshot(tr, steps)
        torch.save(out, os.path.join(out_dir, 'resume%d.pt' % rank))
    finally:
        dist.destroy_process_group()


def test_two_ranks_resume_from_rank_0s_checkpoint_bit_for_bit():
    import torch.multiprocessing as mp
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_rank, args=(2, DP._free_port(), d), nprocs=2, join=True)
        ranks = [torch.load(os.path.join(d, 'resume%d.pt' % r)) for r in range(2)]
    for r in range(2):
        one, two = ranks[r]['run1'], ranks[r]['run2']
        for key in ('params', 'exp_avg', 'exp_avg_sq', 'steps', 'touched'):
            assert torch.equal(one[key], two[key]), (r, key)
        for it in range(2):
            assert torch.equal(one['loss'][it], two['loss'][it]) and torch.equal(one['grad'][it], two['grad'][it]), (r, it)
        assert one['iters'] == two['iters'] == 2 and one['seen'] == two['seen'] == 2 * DP.N_Q
    for key in ('params', 'exp_avg', 'exp_avg_sq', 'steps', 'touched'):
        assert torch.equal(ranks[0]['run2'][key], ranks[1]['run2'][key]), key      # both ranks hold the same state afterwards
    assert float(ranks[0]['run1']['grad'][1].abs().max()) > 0
    assert not torch.equal(ranks[0]['run1']['grad'][0], ranks[0]['run1']['grad'][1])
