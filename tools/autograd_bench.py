#!/usr/bin/env python3
"""Cost of the torch-autograd path (VideoNMN.logits, stair_amd/autograd.py) at the bench workload: 2048 questions, T = 64, V = 2048,
bf16 clips, default matmul mode.  Milliseconds per step (forward + backward, no optimizer) for
  (a) run_programs(train=True) + res.backward(answers)            -- the native CE path the Trainer uses
  (b) model.logits + F.cross_entropy in torch + backward           -- parameter gradients only
  (c) (b) with video and question requiring grad                   -- plus d_video and d_question
and the video encoder's input-gradient product on its own (the launch stair_plan_backward_dlogits makes: [M, 8 Hh] x [8 Hh, V] through
the library's NT GEMM, timed here through stair_gemm_f32 at the same shape) with its TFLOP/s.  Prints one JSON line; --out writes it."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stair_amd import ops, spec, synth  # noqa: E402
from stair_amd.module_net import VideoNMN  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--questions', type=int, default=2048)
ap.add_argument('--T', type=int, default=64)
ap.add_argument('--steps', type=int, default=5)
ap.add_argument('--warmup', type=int, default=2)
ap.add_argument('--only', default='abcd', help='which measurements to run (a, b, c, d = the dX launch alone)')
ap.add_argument('--out', default=None)
a = ap.parse_args()
dev = torch.device('cuda:0')
config = dict(spec.DEFAULT_CONFIG)
B, T = a.questions, a.T

model = VideoNMN(config)
w = synth.make_weights(config, 0)
model.load_state_dict({k: torch.from_numpy(w[k].copy()) for k in spec.state_dict_keys(config)})
model.to(dev)
params = [p for _, p in model.named_parameters()]

# the bench generator (bench.make_batch): programs from the deterministic corpus, features drawn on the GPU, clips stored in bf16
qs = [synth.make_question(config, 0, i, T=T, with_video=False) for i in range(B)]
g = torch.Generator(device=dev).manual_seed(1234)
video = torch.randn(B, T, config['video_size'], device=dev, generator=g).to(torch.bfloat16)
q_lens = [q['question'].shape[0] for q in qs]
question = torch.randn(sum(q_lens), config['text_size'], device=dev, generator=g)
progs, spans = [q['nmn_program_list'] for q in qs], [q['prog_str_to_question_tokens'] for q in qs]
answers = torch.tensor([q['answer'] for q in qs], dtype=torch.int32, device=dev)


def timed(fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.steps


def step_native():
    res = model.run_programs(progs, spans, video, question, q_lens, train=True)
    res.backward(answers)


def step_autograd(inputs):
    v = video.detach().requires_grad_(inputs)
    q = question.detach().requires_grad_(inputs)
    for p in params:
        p.grad = None
    logits = model.logits(progs, spans, v, q, q_lens)
    F.cross_entropy(logits, answers.long(), reduction='sum').backward()


out = {'questions': B, 'T': T, 'V': config['video_size'], 'features': 'bf16', 'matmul_mode': ops.get_matmul_mode(),
       'steps': a.steps, 'warmup': a.warmup}
if 'a' in a.only:
    for p in params:
        p.grad = torch.zeros_like(p)
    out['a_native_ce_ms'] = timed(step_native)
if 'b' in a.only:
    out['b_autograd_params_ms'] = timed(lambda: step_autograd(False))
if 'c' in a.only:
    out['c_autograd_inputs_ms'] = timed(lambda: step_autograd(True))
if 'd' in a.only:
    Hh = config['hidden_size'] // 2
    M, N, K = B * T, config['video_size'], 8 * Hh
    dg = torch.randn(M, K, device=dev, generator=g) * 1e-3
    wt = torch.randn(N, K, device=dev, generator=g) * 0.02
    ms = timed(lambda: ops.linear(dg, wt))
    out['dx_video_ms'] = ms
    out['dx_video_tflops'] = 2.0 * M * N * K / (ms * 1e-3) / 1e12
    out['dx_shape'] = [M, N, K]
if 'a_native_ce_ms' in out and 'b_autograd_params_ms' in out:
    out['b_over_a'] = out['b_autograd_params_ms'] / out['a_native_ce_ms']
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, 'w') as f:
        f.write(line + '\n')
