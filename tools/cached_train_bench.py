#!/usr/bin/env python3
"""What training on cached clip encodings saves at the bench workload (2048 questions, BASELINE.json configs[1]: T = 64, V = 2048, bf16
clips, default matmul mode) with the video encoder frozen, in ONE process on one trainer: blocks of steps alternate between the legs
  direct          Trainer.step on the clips, submodules.video_encoder.* frozen (the `video_encoder` leg of tools/frozen_bench.py)
  cached          the same step on a ClipCache of the same clips (Trainer.step(clips=...)): one gather in place of the video
                  projection and recurrence, none of the encoder's training saves in the workspace
  cached_shared8  the cache with 8 questions per clip (questions / 8 clips)
after a warm-up, each block timed with device events around its whole steps (forward + backward + Adam).  Per leg: ms per step of
every block, their mean, and the spread (max - min) between the repeated blocks; a difference between two legs below that spread is
not resolved.  Also recorded: the workspace bytes of each leg's plan and the launch table of one step.
Prints one JSON line; --out writes it (profiles/cached_train_b2048.json; an existing "default_bench" or "grad_kernel" entry of that
file -- figures measured in runs of their own -- is kept).

--grad-steps N: instead of the legs, N reverse passes that request the gradient of the encodings (VideoNMN.logits(encoded=...)), for
a kernel-trace run of its own (rocprofv3 --kernel-trace --stats -- python tools/cached_train_bench.py --grad-steps 5): the time of
scatter_encoded_video_grad_kernel against its byte bound 2 * n_vid * T * H * 4 and against the gather."""
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
ap.add_argument('--grad-steps', type=int, default=0)
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
tr = Trainer(model, dropout=0.0, freeze=('video_encoder',))
cache = model.encode_clips(video, ids=list(range(B)))          # (after the Trainer: it moved the parameters into its flat buffer)
torch.cuda.synchronize()
gc.collect()
gc.freeze()

if a.grad_steps:
    H = config['hidden_size']
    enc = cache.enc.clone().requires_grad_(True)
    for _ in range(a.grad_steps):
        enc.grad = None
        logits = model.logits(progs, spans, None, question, q_lens, encoded=enc, video_index=list(range(B)))
        torch.nn.functional.cross_entropy(logits, answers.long(), reduction='sum').backward()
    torch.cuda.synchronize()
    print(json.dumps({'grad_steps': a.grad_steps, 'clips': B, 'T': T, 'byte_bound': 2 * B * T * H * 4,
                      'd_enc_max': float(enc.grad.abs().max())}))
    sys.exit(0)

rows = list(range(B))
shared = [i // 8 for i in range(B)]
LEGS = [('direct', lambda: tr.step(progs, spans, video, question, q_lens, answers, global_batch=B)),
        ('cached', lambda: tr.step(progs, spans, None, question, q_lens, answers, global_batch=B, video_index=rows, clips=cache)),
        ('cached_shared8', lambda: tr.step(progs, spans, None, question, q_lens, answers, global_batch=B, video_index=shared, clips=cache))]

for _ in range(a.warmup):
    for _, step in LEGS:
        step()
torch.cuda.synchronize()
ms = {name: [] for name, _ in LEGS}
launches, workspace = {}, {}
for blk in range(a.blocks):
    for name, step in LEGS:
        if blk == 0:                                                # the untimed step after the switch, with the launch table of the leg
            with ops.kernel_accounting() as acct:
                _, res = step()
            launches[name] = {k: v[0] for k, v in sorted(acct.table.items())}
            workspace[name] = int(res.info.workspace_bytes)
            del res
        else:
            step()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            step()
        e1.record()
        torch.cuda.synchronize()
        ms[name].append(e0.elapsed_time(e1) / a.steps)
tr.check()
cache.check()                                                       # the frozen encoder never moved: the cache is still fresh

out = {'questions': B, 'T': T, 'features': 'bf16', 'matmul_mode': ops.get_matmul_mode(), 'steps_per_block': a.steps, 'blocks': a.blocks,
       'warmup': a.warmup, 'clips': {'direct': B, 'cached': B, 'cached_shared8': (B + 7) // 8}, 'workspace_bytes': workspace,
       'ms_per_step': {}, 'saving_ms': {}, 'launches_per_step': launches}
for name, _ in LEGS:
    v = ms[name]
    out['ms_per_step'][name] = {'blocks': [round(x, 4) for x in v], 'mean': round(sum(v) / len(v), 4), 'spread': round(max(v) - min(v), 4)}
for name, _ in LEGS[1:]:
    out['saving_ms'][name] = round(out['ms_per_step']['direct']['mean'] - out['ms_per_step'][name]['mean'], 4)
if a.out and os.path.exists(a.out):
    try:
        old = json.load(open(a.out))
        for key in ('default_bench', 'grad_kernel'):
            if key in old:
                out[key] = old[key]
    except ValueError:
        pass
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, 'w') as f:
        f.write(line + '\n')
