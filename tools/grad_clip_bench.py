#!/usr/bin/env python3
"""Cost of Trainer(max_grad_norm=...) at the bench workload (2048 questions, BASELINE.json configs[1]: T = 64, V = 2048, bf16 clips,
default matmul mode) in ONE process on one trainer: blocks of steps alternate between
  none  max_grad_norm = None         -- the step as it was: stair_adam_step, nothing else launched
  inf   max_grad_norm = inf          -- stair_grad_norm (two launches) + stair_adam_step_scaled, coefficient exactly 1
  clip  max_grad_norm = 0.5 x the first measured norm  -- the same launches, coefficient < 1
after a warm-up, each block timed with device events around its whole steps.  Per variant: ms per step of every block, their
mean, and the spread (max - min) between the repeated blocks -- a difference between variants below that spread is not
resolved.  Prints one JSON line; --out writes it (profiles/grad_clip_bench_b2048.json; an existing "default_bench" entry of that
file -- bench.py's default line on this commit and on its parent -- is kept)."""
import argparse
import gc
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from stair_amd import losses as L, ops, spec, synth  # noqa: E402
from stair_amd.module_net import VideoNMN  # noqa: E402
from stair_amd.train import Trainer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--questions', type=int, default=2048)
ap.add_argument('--T', type=int, default=64)
ap.add_argument('--steps', type=int, default=10, help='steps per timed block')
ap.add_argument('--blocks', type=int, default=4, help='timed blocks per variant')
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--out', default=None)
a = ap.parse_args()
dev = torch.device('cuda:0')
config = dict(spec.DEFAULT_CONFIG)
B, T = a.questions, a.T

model = VideoNMN(config, pretrain_modules=set(L.CRITERION_MODULES))
w = synth.make_weights(config, 0)
model.load_state_dict({k: torch.from_numpy(w[k].copy()) for k in spec.state_dict_keys(config)})
model = model.to(dev)
qs, video, question, q_lens = bench.make_batch(config, B, T, seed=0, device=dev, features='bf16')
progs, spans = [q['nmn_program_list'] for q in qs], [q['prog_str_to_question_tokens'] for q in qs]
answers = torch.tensor([q['answer'] for q in qs], dtype=torch.int32, device=dev)
tr = Trainer(model, dropout=0.0, max_grad_norm=float('inf'))       # allocates the norm buffers; the variant is switched per block
gc.collect()
gc.freeze()


def step():
    tr.step(progs, spans, video, question, q_lens, answers, global_batch=B)


for _ in range(a.warmup):
    step()
torch.cuda.synchronize()
first_norm = tr.finished_grad_norms()[0][1]
variants = [('none', None), ('inf', float('inf')), ('clip', 0.5 * first_norm)]
ms = {name: [] for name, _ in variants}
coef = {}
for blk in range(a.blocks):
    for name, value in variants:
        tr.max_grad_norm = value
        step()                                                      # one untimed step after the switch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            step()
        e1.record()
        torch.cuda.synchronize()
        ms[name].append(e0.elapsed_time(e1) / a.steps)
        if value is not None:
            coef[name] = float(tr.grad_norm[1])
tr.max_grad_norm = float('inf')
tr.check()
tr.finished_grad_norms()

out = {'questions': B, 'T': T, 'features': 'bf16', 'matmul_mode': ops.get_matmul_mode(), 'steps_per_block': a.steps, 'blocks': a.blocks,
       'warmup': a.warmup, 'parameters': int(sum(p.numel() for p in model.parameters())), 'tensors': len(model._weight_names),
       'bucket_floats': tr.n, 'first_norm': first_norm, 'last_coefficient': coef, 'ms_per_step': {}}
for name, _ in variants:
    v = ms[name]
    out['ms_per_step'][name] = {'blocks': [round(x, 4) for x in v], 'mean': round(sum(v) / len(v), 4), 'spread': round(max(v) - min(v), 4)}
mean = lambda k: out['ms_per_step'][k]['mean']
out['inf_minus_none_ms'] = round(mean('inf') - mean('none'), 4)
out['clip_minus_none_ms'] = round(mean('clip') - mean('none'), 4)
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
