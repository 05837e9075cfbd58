#!/usr/bin/env python3
"""Segmented tiles on long clips (T > 64 frames; H = 512, V = 2048, bf16 clips, default matmul mode), 2048 questions, in ONE process
on one model / trainer per frame count: blocks alternate between
  off  set_option('tile_split', 0)  -- the map-level modules run their launch-per-layer sequences, as every plan of T > 64 did
  on   set_option('tile_split', 1)  -- the fused tile operators on 64-row segments, and everything a plan hangs off them
after a warm-up.  Frame counts: T = 128 at max_video_length 128, and T = 100 at max_video_length 100.  Training plans with a
Superlative node stop at 113 frames, so the T = 128 batch draws its programs from the forms without one (recorded as "forms").
Per block: ms per training step and per inference batch (device events around the block's whole steps), the tile operators' own
device time per training step (stair_tile_timing, in steps of their own), and the launches of a training step that the library's
kernel accounting counts.  Per setting: every block's figures, their mean, and the spread (max - min) between the repeated
blocks -- a difference between the settings below that spread is reported as not resolved.  Prints one JSON line; --out writes it
(profiles/long_clip_tiles_b2048.json; an existing "default_bench" entry of that file -- bench.py's default line on this commit
and on its parent -- is kept).  Needs a GPU: there is no fallback."""
import argparse
import ctypes as C
import gc
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stair_amd import losses as L, ops, spec, synth  # noqa: E402
from stair_amd._lib import lib  # noqa: E402
from stair_amd.module_net import VideoNMN  # noqa: E402
from stair_amd.train import Trainer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--questions', type=int, default=2048)
ap.add_argument('--frames', type=int, nargs='+', default=[128, 100])
ap.add_argument('--steps', type=int, default=5, help='steps per timed block')
ap.add_argument('--blocks', type=int, default=3, help='timed blocks per setting (at least 3)')
ap.add_argument('--warmup', type=int, default=2)
ap.add_argument('--tile-steps', type=int, default=2, help='steps per block run under stair_tile_timing')
ap.add_argument('--out', default=None)
a = ap.parse_args()
if a.blocks < 3:
    ap.error('--blocks must be at least 3: the spread between repeated blocks is the resolution of the comparison')
if not torch.cuda.is_available():
    sys.exit('long_clip_bench.py needs a GPU')
dev = torch.device('cuda:0')
B = a.questions
SUPERLATIVE_TRAIN_MAX = 113
keys = ('train_ms_per_step', 'infer_ms_per_batch', 'tile_ms_per_train_step')
settings = [('off', 0), ('on', 1)]


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


def measure(T):
    config = dict(spec.DEFAULT_CONFIG, video_size=2048, max_video_length=T)
    forms = [f for f in synth.PAPER_FORMS if T <= SUPERLATIVE_TRAIN_MAX or 'Superlative' not in synth.make_question(config, 0, 0, form=f, T=T, with_video=False)['nmn_program_list']]
    model = VideoNMN(config, pretrain_modules=set(L.CRITERION_MODULES))
    w = synth.make_weights(config, 0)
    model.load_state_dict({k: torch.from_numpy(w[k].copy()) for k in spec.state_dict_keys(config)})
    model = model.to(dev)
    qs = [synth.make_question(config, 0, i, T=T, forms=forms, with_video=False) for i in range(B)]
    g = torch.Generator(device=dev).manual_seed(1234)
    video = torch.randn(B, T, config['video_size'], device=dev, generator=g).to(torch.bfloat16)
    q_lens = [q['question'].shape[0] for q in qs]
    question = torch.randn(sum(q_lens), config['text_size'], device=dev, generator=g)
    progs, spans = [q['nmn_program_list'] for q in qs], [q['prog_str_to_question_tokens'] for q in qs]
    answers = torch.tensor([q['answer'] for q in qs], dtype=torch.int32, device=dev)
    tr = Trainer(model, dropout=0.0)
    gc.collect()

    def train_step():
        tr.step(progs, spans, video, question, q_lens, answers, global_batch=B)

    def infer():
        model.run_programs(progs, spans, video, question, q_lens)

    for _, value in settings:
        model.set_option('tile_split', value)
        for _ in range(a.warmup):
            train_step()
            infer()
    torch.cuda.synchronize()
    ms = {name: {k: [] for k in keys} for name, _ in settings}
    items, tile_launches, launches = {}, {}, {}
    for blk in range(a.blocks):
        for name, value in settings:
            model.set_option('tile_split', value)
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
            items[name], tile_launches[name] = work_items() // a.tile_steps, nl.value // a.tile_steps
            with ops.kernel_accounting() as acct:
                train_step()
                torch.cuda.synchronize()
            launches[name] = sum(v[0] for v in acct.table.values())
    model.set_option('tile_split', None)
    tr.check()
    out = {'T': T, 'max_video_length': T, 'forms': forms, 'segments': int(lib.stair_tile_segments(T)),
           'tile_work_items_per_train_step': items, 'tile_launches_per_train_step': tile_launches,
           'accounted_launches_per_train_step': launches}
    for name, _ in settings:
        out[name] = {}
        for k in keys:
            v = ms[name][k]
            out[name][k] = {'blocks': [round(x, 4) for x in v], 'mean': round(sum(v) / len(v), 4), 'spread': round(max(v) - min(v), 4)}
    out['on_minus_off_ms'] = {k: round(out['on'][k]['mean'] - out['off'][k]['mean'], 4) for k in ('train_ms_per_step', 'infer_ms_per_batch')}
    out['resolved'] = {k: bool(abs(out['off'][k]['mean'] - out['on'][k]['mean']) > max(out['on'][k]['spread'], out['off'][k]['spread']))
                       for k in ('train_ms_per_step', 'infer_ms_per_batch')}
    del tr, model
    gc.collect()
    torch.cuda.empty_cache()
    return out


out = {'questions': B, 'video_size': 2048, 'hidden_size': 512, 'features': 'bf16', 'matmul_mode': ops.get_matmul_mode(),
       'steps_per_block': a.steps, 'tile_steps_per_block': a.tile_steps, 'blocks': a.blocks, 'warmup': a.warmup,
       'runs': [measure(T) for T in a.frames]}
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
