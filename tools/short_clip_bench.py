#!/usr/bin/env python3
"""Packed tiles at the reference's first published setting (BASELINE.json configs[0]: T = 8 frames of 4096 features, H = 512; bf16
clips, default matmul mode), 2048 questions, in ONE process on one model / trainer: blocks alternate between
  off  set_option('tile_pack', 0)  -- one module instance per 64-row tile, as before
  on   set_option('tile_pack', 1)  -- 64 / T = 8 instances per tile
after a warm-up.  Per block: ms per training step and per inference batch (device events around the block's whole steps), and the
tile operators' own device time per training step (stair_tile_timing: events around every tile launch, in steps of their own so
that the events do not sit inside the timed steps).  Per setting: every block's figures, their mean, and the spread (max - min)
between the repeated blocks -- a difference between the settings below that spread is not resolved.  Prints one JSON line; --out
writes it (profiles/short_clip_pack_b2048.json; an existing "default_bench" entry of that file -- bench.py's default line on this
commit and on its parent -- is kept).  Needs a GPU: there is no fallback."""
import argparse
import ctypes as C
import gc
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from stair_amd import losses as L, ops, spec, synth  # noqa: E402
from stair_amd._lib import lib  # noqa: E402
from stair_amd.module_net import VideoNMN  # noqa: E402
from stair_amd.train import Trainer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--questions', type=int, default=2048)
ap.add_argument('--steps', type=int, default=10, help='steps per timed block')
ap.add_argument('--blocks', type=int, default=4, help='timed blocks per setting (at least 3)')
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--tile-steps', type=int, default=3, help='steps per block run under stair_tile_timing')
ap.add_argument('--out', default=None)
a = ap.parse_args()
if a.blocks < 3:
    ap.error('--blocks must be at least 3: the spread between repeated blocks is the resolution of the comparison')
if not torch.cuda.is_available():
    sys.exit('short_clip_bench.py needs a GPU')
dev = torch.device('cuda:0')
T = 8
config = dict(spec.DEFAULT_CONFIG, video_size=4096, max_video_length=T)
B = a.questions

model = VideoNMN(config, pretrain_modules=set(L.CRITERION_MODULES))
w = synth.make_weights(config, 0)
model.load_state_dict({k: torch.from_numpy(w[k].copy()) for k in spec.state_dict_keys(config)})
model = model.to(dev)
qs, video, question, q_lens = bench.make_batch(config, B, T, seed=0, device=dev, features='bf16')
progs, spans = [q['nmn_program_list'] for q in qs], [q['prog_str_to_question_tokens'] for q in qs]
answers = torch.tensor([q['answer'] for q in qs], dtype=torch.int32, device=dev)
tr = Trainer(model, dropout=0.0)
gc.collect()
gc.freeze()


def train_step():
    tr.step(progs, spans, video, question, q_lens, answers, global_batch=B)


def infer():
    model.run_programs(progs, spans, video, question, q_lens)


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def work_items():
    n = C.c_int64(0)
    lib.stair_tile_work_items(C.byref(n), 1)
    return n.value


for _ in range(a.warmup):
    train_step()
    infer()
torch.cuda.synchronize()
settings = [('off', 0), ('on', 1)]
keys = ('train_ms_per_step', 'infer_ms_per_batch', 'tile_ms_per_train_step')
ms = {name: {k: [] for k in keys} for name, _ in settings}
items, launches = {}, {}
for blk in range(a.blocks):
    for name, value in settings:
        model.set_option('tile_pack', value)
        train_step(); infer()                                       # one untimed step of each kind after the switch
        torch.cuda.synchronize()
        ms[name]['train_ms_per_step'].append(timed(train_step, a.steps))
        ms[name]['infer_ms_per_batch'].append(timed(infer, a.steps))
        work_items()
        lib.stair_tile_timing(1)
        for _ in range(a.tile_steps):
            train_step()
        torch.cuda.synchronize()
        t, nl = C.c_double(0.0), C.c_int32(0)
        lib.stair_tile_timing_read(C.byref(t), C.byref(nl))
        lib.stair_tile_timing(0)
        ms[name]['tile_ms_per_train_step'].append(t.value / a.tile_steps)
        items[name], launches[name] = work_items() // a.tile_steps, nl.value // a.tile_steps
model.set_option('tile_pack', None)
tr.check()

out = {'config': 'BASELINE configs[0]', 'questions': B, 'T': T, 'video_size': config['video_size'], 'hidden_size': config['hidden_size'],
       'features': 'bf16', 'matmul_mode': ops.get_matmul_mode(), 'pack_factor': int(lib.stair_tile_pack_factor(T)),
       'steps_per_block': a.steps, 'tile_steps_per_block': a.tile_steps, 'blocks': a.blocks, 'warmup': a.warmup,
       'tile_work_items_per_train_step': items, 'tile_launches_per_train_step': launches}
for name, _ in settings:
    out[name] = {}
    for k in keys:
        v = ms[name][k]
        out[name][k] = {'blocks': [round(x, 4) for x in v], 'mean': round(sum(v) / len(v), 4), 'spread': round(max(v) - min(v), 4)}
out['on_minus_off_ms'] = {k: round(out['on'][k]['mean'] - out['off'][k]['mean'], 4) for k in keys}
out['resolved'] = {k: bool(out['off'][k]['mean'] - out['on'][k]['mean'] > max(out['on'][k]['spread'], out['off'][k]['spread'])) for k in keys}
if a.out and os.path.exists(a.out):
    try:
        old = json.load(open(a.out))
        if 'default_bench' in old:
            out['default_bench'] = old['default_bench']
    except ValueError:
        pass
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, 'w') as f:
        f.write(line + '\n')
