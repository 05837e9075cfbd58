#!/usr/bin/env python3
"""The audit pass beside the inference pass it reads, at the bench shape: 2048 questions of the 12 program forms with synthetic gold,
H = 512, T = 64 frames of 2048 bf16 features from a device-resident ClipLibrary, a ClassTable of 214 classes; ONE process, one model.
Three legs alternate in blocks after a warm-up of each:
  a  forward_batch alone
  b  forward_batch + audit.audit_batch, its arrays read to the host (one copy)
  c  forward_batch + the per-node loop that was the only way before: res.node / res.related_attn of every supervised node copied
     to the host one by one (a device-to-host copy and a synchronisation each)
Per leg: ms per pass of every timed block (device events around the block's whole passes and a synchronise; a block runs as many
passes as fill --window-ms), their mean and the spread (max - min) between the repeated blocks.  Relation checked: b is faster
than c by more than the larger spread.  Prints one JSON line; --out writes it (profiles/audit_b2048.json; the "audit_kernels" and
"default_bench" entries already there are kept).

--leg NAME: only that leg, --passes times after the warm-up and nothing else -- the run to put under
`rocprofv3 --kernel-trace --stats` (profile in a run of its own: tracing slows the host); --kernel-stats FILE then reads that run's
*_kernel_stats.csv and adds the "audit_kernels" entry to --out: each audit kernel's calls and times, and for the rank kernel the
n * n_cls * H * 4 bytes it reads from L2 over its mean time.  Needs a GPU: there is no fallback."""
import argparse
import csv
import gc
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument('--questions', type=int, default=2048)
ap.add_argument('--blocks', type=int, default=4, help='timed blocks per leg (at least 3)')
ap.add_argument('--window-ms', type=float, default=600.0, help='least length of a timed block')
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--leg', default=None)
ap.add_argument('--passes', type=int, default=20)
ap.add_argument('--kernel-stats', default=None)
ap.add_argument('--rank-items', type=int, default=None, help='with --kernel-stats: contrastive nodes per pass (the "nodes" entry of --out)')
ap.add_argument('--out', default=None)
a = ap.parse_args()
T, N_CLS = 64, 214


def merge_out(doc_update):
    doc = {}
    if a.out and os.path.exists(a.out):
        try:
            doc = json.load(open(a.out))
        except ValueError:
            doc = {}
    doc_update(doc)
    line = json.dumps(doc)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if a.kernel_stats:          # no GPU work: fold a profiler run's figures into the result file
    rows = [r for r in csv.DictReader(open(a.kernel_stats)) if 'audit_' in r['Name']]
    if not rows:
        sys.exit('no audit kernel in %s' % a.kernel_stats)

    def fold(doc):
        n_rank = a.rank_items if a.rank_items is not None else doc.get('nodes', {}).get('contrastive')
        entry = {'source': 'rocprofv3 --kernel-trace --stats, a run of its own over leg b'}
        for r in rows:
            name = r['Name'].split('(')[0].split('::')[-1].replace('void ', '')
            k = {'calls': int(r['Calls']), 'mean_us': round(float(r['AverageNs']) * 1e-3, 2), 'min_us': round(float(r['MinNs']) * 1e-3, 2),
                 'max_us': round(float(r['MaxNs']) * 1e-3, 2)}
            if 'audit_rank' in name and n_rank:
                nbytes = n_rank * N_CLS * 512 * 4
                k.update(items=n_rank, l2_read_bytes=nbytes, l2_read_TB_per_s=round(nbytes / (float(r['AverageNs']) * 1e-9) / 1e12, 3))
            entry[name] = k
        doc['audit_kernels'] = entry
    merge_out(fold)
    sys.exit(0)

import torch  # noqa: E402

from stair_amd import audit, losses, ops, spec, synth  # noqa: E402
from stair_amd.clip_library import ClipLibrary  # noqa: E402
from stair_amd.module_net import VideoNMN  # noqa: E402

if a.blocks < 3:
    ap.error('--blocks must be at least 3: the spread between repeated blocks is the resolution of the comparison')
if not torch.cuda.is_available():
    sys.exit('audit_bench.py needs a GPU')
dev = torch.device('cuda:0')
config = dict(spec.DEFAULT_CONFIG, have_pretrain_head=True)
B = a.questions

model = VideoNMN(config, pretrain_modules=set(losses.CRITERION_MODULES))
w = synth.make_weights(config, 0)
model.load_state_dict({k: torch.from_numpy(w[k].copy()) for k in spec.state_dict_keys(config)})
model = model.to(dev)
qs = [synth.make_question(config, 0, i, form=synth.ALL_FORMS[i % len(synth.ALL_FORMS)], T=T, with_video=False) for i in range(B)]
for i, q in enumerate(qs):
    q['sg_res_by_step'] = synth.make_gold(config, 3, q, T=T)
    q['video_id'] = i
table = losses.ClassTable(['class_%d' % c for c in range(N_CLS)], [synth.class_embedding(config, 3, c) for c in range(N_CLS)])
g = torch.Generator(device=dev).manual_seed(1234)
library = ClipLibrary(T, config['video_size'], dev, torch.bfloat16)
library.add(torch.randn(B, T, config['video_size'], device=dev, generator=g).to(torch.bfloat16), ids=list(range(B)))
nodes = [(qi, i, q['nmn_program_list'][i]) for qi, q in enumerate(qs) for i in sorted(losses.supervised_nodes(q, model.pretrain_modules).values())
         if q['nmn_program_list'][i] in audit.AUDITED]


def leg_a():
    return model.forward_batch(qs, clip_library=library)


def leg_b():
    res = model.forward_batch(qs, clip_library=library)
    batch = audit.audit_batch(model, res, qs, class_table=table)
    return res, batch, batch.iou                      # the first read brings every array to the host


def leg_c():
    res = model.forward_batch(qs, clip_library=library)
    got = [(res.related_attn(qi, i) if m == 'Temporal' else res.node(qi, i)).cpu() for qi, i, m in nodes]
    return res, got


legs = {'a': leg_a, 'b': leg_b, 'c': leg_c}
gc.collect()
gc.freeze()


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


if a.leg:
    for _ in range(a.warmup):
        legs[a.leg]()
    torch.cuda.synchronize()
    print(json.dumps({'leg': a.leg, 'passes': a.passes, 'ms_per_pass': round(timed(legs[a.leg], a.passes), 4)}))
    sys.exit(0)

passes = {}
for name, fn in legs.items():
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    passes[name] = max(2, int(math.ceil(a.window_ms / timed(fn, 2))))       # passes that fill the window, from a pilot timing
ms = {name: [] for name in legs}
for blk in range(a.blocks):
    for name, fn in legs.items():
        ms[name].append(timed(fn, passes[name]))
_, batch, _ = leg_b()

out = {'config': 'bench shape, inference: forward_batch from a ClipLibrary', 'questions': B, 'T': T, 'video_size': config['video_size'], 'features': 'bf16',
       'hidden_size': config['hidden_size'], 'classes': N_CLS, 'forms': len(synth.ALL_FORMS), 'matmul_mode': ops.get_matmul_mode(),
       'blocks': a.blocks, 'window_ms': a.window_ms, 'warmup': a.warmup, 'passes_per_block': passes,
       'nodes': {'audited': len(nodes), 'attention_rows': int(batch.att_q.size), 'heads': int(batch.head_q.size), 'contrastive': int(batch.cont_q.size),
                 'scored_attention_rows': int((batch.iou >= 0).sum()), 'scored_heads': int((batch.correct >= 0).sum()),
                 'scored_contrastive': int((batch.rank > 0).sum())},
       'audit_output_bytes': int(sum(v[1] for v in batch._views.values())), 'legs': {}}
for name in legs:
    v = ms[name]
    mean = sum(v) / len(v)
    out['legs'][name] = {'ms_per_pass_blocks': [round(x, 4) for x in v], 'mean_ms': round(mean, 4), 'spread_ms': round(max(v) - min(v), 4),
                         'questions_per_s': round(B / mean * 1e3, 1)}
la, lb, lc = (out['legs'][k] for k in 'abc')
spread = max(lb['spread_ms'], lc['spread_ms'])
out['relations'] = {'audit_ms_per_pass_b_minus_a': round(lb['mean_ms'] - la['mean_ms'], 4), 'per_node_loop_ms_per_pass_c_minus_a': round(lc['mean_ms'] - la['mean_ms'], 4),
                    'c_over_b': round(lc['mean_ms'] / lb['mean_ms'], 3), 'larger_spread_ms': spread,
                    'b_faster_than_c_beyond_spread': bool(lc['mean_ms'] - lb['mean_ms'] > spread)}
out['report_sample'] = {m: audit.module_report(kind, vals) for m, (kind, vals) in sorted(audit.module_values(batch).items())}


def whole(doc):             # everything anew; the profiler run's entry and the hand-recorded bench.py lines stay
    kept = {k: doc[k] for k in ('audit_kernels', 'default_bench') if k in doc}
    doc.clear()
    doc.update(out)
    doc.update(kept)


merge_out(whole)
