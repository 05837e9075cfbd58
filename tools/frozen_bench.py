#!/usr/bin/env python3
"""What a frozen parameter set saves at the bench workload (2048 questions, BASELINE.json configs[1]: T = 64, V = 2048, bf16 clips,
default matmul mode) in ONE process on one trainer: blocks of steps alternate between the legs
  none            every parameter trainable: the step as it always was
  video_encoder   submodules.video_encoder.* frozen: no reverse recurrence and no dW_ih / dW_hh products of the video encoder
  both_encoders   both bi-LSTMs frozen: no BPTT at all
  decoder_only    everything but submodules.decoder.* frozen: the reverse pass ends behind the decoder's weight gradients
after a warm-up, each block timed with device events around its whole steps (forward + backward + Adam).  The legs are switched
with requires_grad_ on the parameters -- Trainer.step reads the flags at every step.  Per leg: ms per step of every block, their
mean, and the spread (max - min) between the repeated blocks; a difference between two legs below that spread is not resolved.
Prints one JSON line; --out writes it (profiles/frozen_step_b2048.json; an existing "default_bench" entry of that file -- bench.py's
default line on this commit and on its parent, measured in one call -- is kept)."""
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
ap.add_argument('--blocks', type=int, default=4, help='timed blocks per leg')
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
tr = Trainer(model, dropout=0.0)
params = dict(model.named_parameters())
names = model._weight_names
gc.collect()
gc.freeze()

LEGS = [('none', lambda n: False),
        ('video_encoder', lambda n: '.video_encoder.' in n),
        ('both_encoders', lambda n: '_encoder.' in n),
        ('decoder_only', lambda n: '.decoder.' not in n)]


def step():
    tr.step(progs, spans, video, question, q_lens, answers, global_batch=B)


for _ in range(a.warmup):
    step()
torch.cuda.synchronize()
ms = {name: [] for name, _ in LEGS}
launches = {}
for blk in range(a.blocks):
    for name, frozen in LEGS:
        for n in names:
            params[n].requires_grad_(not frozen(n))
        if blk == 0:                                                # the untimed step after the switch, with the launch table of the leg
            with ops.kernel_accounting() as acct:
                step()
            launches[name] = {k: v[0] for k, v in sorted(acct.table.items())}
        else:
            step()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            step()
        e1.record()
        torch.cuda.synchronize()
        ms[name].append(e0.elapsed_time(e1) / a.steps)
for n in names:
    params[n].requires_grad_(True)
tr.check()

out = {'questions': B, 'T': T, 'features': 'bf16', 'matmul_mode': ops.get_matmul_mode(), 'steps_per_block': a.steps, 'blocks': a.blocks,
       'warmup': a.warmup, 'tensors': len(names), 'frozen_tensors': {name: sum(1 for n in names if frozen(n)) for name, frozen in LEGS},
       'ms_per_step': {}, 'saving_ms': {}, 'launches_per_step': launches}
for name, _ in LEGS:
    v = ms[name]
    out['ms_per_step'][name] = {'blocks': [round(x, 4) for x in v], 'mean': round(sum(v) / len(v), 4), 'spread': round(max(v) - min(v), 4)}
for name, _ in LEGS[1:]:
    out['saving_ms'][name] = round(out['ms_per_step']['none']['mean'] - out['ms_per_step'][name]['mean'], 4)
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
