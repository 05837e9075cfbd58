#!/usr/bin/env python3
"""Answering from cached clip encodings against encoding every clip again, at BASELINE.json configs[1]'s shape (2048 questions of
the 12 program forms, T = 64 frames of 2048 bf16 features, H = 512, A = 172), inference, in ONE process on one model.  Four legs
alternate after a warm-up of each:
  direct_own      run_programs on 2048 clips, one per question (the video bi-LSTM runs on all of them)
  direct_shared8  256 clips, 8 questions per clip (video_index: the encoder runs once per clip of the batch)
  cached_own      the 2048 clips from a ClipCache (encode_clips, before the timed part): no video encoder in the pass
  cached_shared8  256 cached clips, 8 questions per clip
Per leg: ms per pass of every timed block (device events around the block's whole passes; a block runs as many passes as fill
--window-ms), their mean and the spread (max - min) between the repeated blocks.  Per pairing: cached / direct, and whether the
cached leg is slower than its direct leg by more than the larger spread (the condition this file exists to check).  The one-time
cost of encode_clips for the 2048 clips (host clock around the call and a synchronise; several repeats) stands beside them, with
the number of questions per clip after which the cache has paid for itself.  The logits of each cached leg are compared with its
direct leg's.  Prints one JSON line; --out writes it (profiles/clip_cache_infer_b2048.json; a "gather_kernel" entry already there
is kept).

--leg NAME: only that leg, --passes times after the warm-up and nothing else -- the run to put under
`rocprofv3 --kernel-trace --stats` for the gather kernel's own time (profile in a run of its own: tracing slows the host);
--kernel-stats FILE then reads that run's *_kernel_stats.csv and adds the "gather_kernel" entry to --out: its bytes (read once +
written once, as the launcher accounts them) over its mean time, against the 8 TB/s HBM peak.  Needs a GPU: there is no fallback."""
import argparse
import csv
import gc
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument('--questions', type=int, default=2048)
ap.add_argument('--blocks', type=int, default=4, help='timed blocks per leg (at least 3)')
ap.add_argument('--window-ms', type=float, default=600.0, help='least length of a timed block')
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--encode-repeats', type=int, default=3)
ap.add_argument('--leg', default=None)
ap.add_argument('--passes', type=int, default=20)
ap.add_argument('--kernel-stats', default=None)
ap.add_argument('--out', default=None)
a = ap.parse_args()
HBM_PEAK = 8.0e12
T, PER_CLIP = 64, 8


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
    rows = [r for r in csv.DictReader(open(a.kernel_stats)) if 'gather_encoded_video_kernel' in r['Name']]
    if len(rows) != 1:
        sys.exit('expected one gather_encoded_video_kernel row in %s, found %d' % (a.kernel_stats, len(rows)))
    r = rows[0]
    nbytes = 2 * a.questions * T * 512 * 4
    mean_s = float(r['AverageNs']) * 1e-9
    entry = {'source': 'rocprofv3 --kernel-trace --stats, a run of its own over the cached_own leg', 'clips': a.questions, 'calls': int(r['Calls']),
             'mean_us': round(mean_s * 1e6, 2), 'min_us': round(float(r['MinNs']) * 1e-3, 2), 'max_us': round(float(r['MaxNs']) * 1e-3, 2),
             'bytes_read_plus_written': nbytes, 'achieved_TB_per_s': round(nbytes / mean_s / 1e12, 3),
             'fraction_of_hbm_peak_8_TB_per_s': round(nbytes / mean_s / HBM_PEAK, 3), 'floor_us_at_peak': round(nbytes / HBM_PEAK * 1e6, 2)}
    merge_out(lambda doc: doc.__setitem__('gather_kernel', entry))
    sys.exit(0)

import torch  # noqa: E402

from stair_amd import ops, spec, synth  # noqa: E402
from stair_amd.module_net import VideoNMN  # noqa: E402

if a.blocks < 3:
    ap.error('--blocks must be at least 3: the spread between repeated blocks is the resolution of the comparison')
if not torch.cuda.is_available():
    sys.exit('clip_cache_bench.py needs a GPU')
dev = torch.device('cuda:0')
config = dict(spec.DEFAULT_CONFIG)
B = a.questions
assert B % PER_CLIP == 0

model = VideoNMN(config)
w = synth.make_weights(config, 0)
model.load_state_dict({k: torch.from_numpy(w[k].copy()) for k in spec.state_dict_keys(config)})
model = model.to(dev)
qs = [synth.make_question(config, 0, i, form=synth.ALL_FORMS[i % len(synth.ALL_FORMS)], T=T, with_video=False) for i in range(B)]
g = torch.Generator(device=dev).manual_seed(1234)
video = torch.randn(B, T, config['video_size'], device=dev, generator=g).to(torch.bfloat16)       # the stored clip-feature format
q_lens = [q['question'].shape[0] for q in qs]
question = torch.randn(sum(q_lens), config['text_size'], device=dev, generator=g)
progs, spans = [q['nmn_program_list'] for q in qs], [q['prog_str_to_question_tokens'] for q in qs]
shared_index = [i // PER_CLIP for i in range(B)]
shared_video = video[:B // PER_CLIP].contiguous()
own_index = list(range(B))

encode_ms = []
for _ in range(a.encode_repeats):
    cache = None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cache = model.encode_clips(video)
    torch.cuda.synchronize()
    encode_ms.append((time.perf_counter() - t0) * 1e3)

legs = {
    'direct_own': lambda: model.run_programs(progs, spans, video, question, q_lens),
    'direct_shared8': lambda: model.run_programs(progs, spans, shared_video, question, q_lens, video_index=shared_index),
    'cached_own': lambda: model.run_programs(progs, spans, None, question, q_lens, clips=cache, video_index=own_index),
    'cached_shared8': lambda: model.run_programs(progs, spans, None, question, q_lens, clips=cache, video_index=shared_index),
}
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

passes, logits = {}, {}
for name, fn in legs.items():
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    passes[name] = max(3, int(math.ceil(a.window_ms / timed(fn, 5))))       # passes that fill the window, from a pilot timing
    logits[name] = fn().logits.clone()
ms = {name: [] for name in legs}
for blk in range(a.blocks):
    for name, fn in legs.items():
        ms[name].append(timed(fn, passes[name]))
with ops.kernel_accounting() as acct:
    legs['cached_own']()
    torch.cuda.synchronize()

out = {'config': 'BASELINE configs[1] shape, inference', 'questions': B, 'T': T, 'video_size': config['video_size'], 'features': 'bf16',
       'hidden_size': config['hidden_size'], 'answer_vocab_length': config['answer_vocab_length'], 'forms': len(synth.ALL_FORMS),
       'matmul_mode': ops.get_matmul_mode(), 'blocks': a.blocks, 'window_ms': a.window_ms, 'warmup': a.warmup, 'passes_per_block': passes,
       'legs': {}}
for name in legs:
    v = ms[name]
    mean = sum(v) / len(v)
    out['legs'][name] = {'ms_per_pass_blocks': [round(x, 4) for x in v], 'mean_ms': round(mean, 4), 'spread_ms': round(max(v) - min(v), 4),
                         'questions_per_s': round(B / mean * 1e3, 1)}
out['pairings'] = {}
for d, c in (('direct_own', 'cached_own'), ('direct_shared8', 'cached_shared8')):
    ld, lc = out['legs'][d], out['legs'][c]
    spread = max(ld['spread_ms'], lc['spread_ms'])
    out['pairings'][c + '_vs_' + d] = {'cached_over_direct': round(lc['mean_ms'] / ld['mean_ms'], 4), 'saved_ms_per_pass': round(ld['mean_ms'] - lc['mean_ms'], 4),
                                       'spread_ms': spread, 'cached_slower_beyond_spread': bool(lc['mean_ms'] - ld['mean_ms'] > spread),
                                       'max_abs_logit_difference': float((logits[c] - logits[d]).abs().max())}
own = out['pairings']['cached_own_vs_direct_own']
steady = min(encode_ms[1:]) if len(encode_ms) > 1 else encode_ms[0]
out['encode_clips'] = {'clips': B, 'ms_per_call': [round(x, 3) for x in encode_ms], 'note': 'host clock around encode_clips + synchronise; the first call '
                       'also loads the kernels', 'ms_per_clip': round(steady / B, 5),
                       # a direct pass spends saved_ms_per_pass on B clips: encoding a clip once costs as much as asking this many questions about it directly
                       'passes_until_paid_back': round(steady / own['saved_ms_per_pass'], 2) if own['saved_ms_per_pass'] > 0 else None}
out['gather_accounting'] = {'launches': acct.table['gather_encoded_video'][0], 'bytes': acct.table['gather_encoded_video'][1]}


def whole(doc):             # everything anew; the profiler run's entry stays
    kept = doc.get('gather_kernel')
    doc.clear()
    doc.update(out)
    if kept is not None:
        doc['gather_kernel'] = kept


merge_out(whole)
