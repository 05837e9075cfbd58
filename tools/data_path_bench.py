#!/usr/bin/env python
"""What a training step costs once its inputs have to get to the device: three legs at the bench shape (2048 questions about ~1850
distinct clips of 64 x 2048 bf16 drawn from a library of a few thousand, words from a table of a few thousand 300-float rows), whole
Trainer.steps timed on the wall clock after a final synchronise, host packing included, in alternating blocks.

  A  item dicts -> data.pack_questions (clips stacked, pinned, copied) -> Trainer.step(video=, question=)     -- the host-fed path
  B  the same items -> pack_questions(clip_library=, word_table=) -> Trainer.step(library=, question_ids=)     -- fed by row ids
  C  dense inputs resident before the timed region (what bench.py times)

    python tools/data_path_bench.py --out profiles/clip_library_b2048.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o leg_b -- python tools/data_path_bench.py --only B --blocks 1 --steps 10
    python tools/data_path_bench.py --kernel-stats DIR/.../leg_b_kernel_stats.csv --out profiles/clip_library_b2048.json   (adds the gathers)
"""
import argparse
import csv
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
for var in ('OMP_NUM_THREADS', 'MKL_NUM_THREADS'):
    os.environ.setdefault(var, '16')

import numpy as np          # noqa: E402
import torch                # noqa: E402

from stair_amd import data as D, spec, synth      # noqa: E402

HBM_BYTES_PER_S = 8e12


def merge_kernel_stats(path, out):
    """the two gather kernels' rows of a rocprofv3 --kernel-trace --stats run of leg B into the JSON, against bytes / 8 TB/s"""
    result = json.load(open(out))
    rows = list(csv.DictReader(open(path)))
    for key, name in (('gather_clips', 'gather_clips_kernel'), ('gather_words', 'gather_words_kernel')):
        hit = [r for r in rows if name in r.get('Name', '')]
        if not hit:
            raise SystemExit('%s: no row for %s' % (path, name))
        r = hit[0]
        calls, avg_ns = int(r['Calls']), float(r.get('AverageNs') or float(r['TotalDurationNs']) / int(r['Calls']))
        nbytes = result['gather_bytes_per_step'][key]
        result.setdefault('gather_kernels', {})[key] = dict(calls=calls, avg_us=avg_ns / 1e3, min_us=float(r['MinNs']) / 1e3, max_us=float(r['MaxNs']) / 1e3,
                                                            bytes=nbytes, hbm_floor_us=nbytes / HBM_BYTES_PER_S * 1e6,
                                                            fraction_of_hbm_peak=nbytes / HBM_BYTES_PER_S / (avg_ns * 1e-9))
    b_ms = result['legs']['B']['ms_per_step']
    result['gather_share_of_step_B'] = sum(k['avg_us'] for k in result['gather_kernels'].values()) / 1e3 / b_ms
    json.dump(result, open(out, 'w'), indent=1)
    print(json.dumps(result['gather_kernels']))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--batch', type=int, default=2048)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--library-clips', type=int, default=3000)
    ap.add_argument('--vocabulary', type=int, default=3000)
    ap.add_argument('--blocks', type=int, default=4, help='timed blocks per leg, alternated A B C A B C ...')
    ap.add_argument('--steps', type=int, default=4, help='training steps per block')
    ap.add_argument('--warmup', type=int, default=2, help='untimed steps per leg before the first block')
    ap.add_argument('--only', choices=['A', 'B', 'C'], help='run one leg alone (the profiled run of leg B)')
    ap.add_argument('--out', help='write the result as JSON')
    ap.add_argument('--kernel-stats', help='a rocprofv3 kernel_stats.csv of a leg-B run: merge the gather kernels into --out and exit')
    args = ap.parse_args()
    if args.kernel_stats is not None:
        if not (args.out and os.path.isfile(args.kernel_stats) and os.path.isfile(args.out)):
            ap.error('--kernel-stats needs an existing csv and the --out JSON of an earlier run')
        return merge_kernel_stats(args.kernel_stats, args.out)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    dev = torch.device('cuda', 0)
    from stair_amd.clip_library import ClipLibrary
    from stair_amd.module_net import VideoNMN
    from stair_amd.train import Trainer
    config = dict(spec.DEFAULT_CONFIG)
    B, T, V, E = args.batch, args.frames, config['video_size'], config['text_size']
    weights = synth.make_weights(config, 0)

    def trainer():
        model = VideoNMN(config)
        model.load_state_dict({k: torch.from_numpy(weights[k].copy()) for k in spec.state_dict_keys(config)})
        return Trainer(model.to(dev), dropout=0.0)

    # the data set: clips on the host (bf16, the stored format) and in a library, a vocabulary on the host and in a table
    g = torch.Generator().manual_seed(1)
    clips = {'v%05d' % i: torch.randn(T, V, generator=g).to(torch.bfloat16) for i in range(args.library_clips)}
    library = ClipLibrary.from_clips(clips, dev)
    vocab = torch.randn(args.vocabulary, E, generator=g)
    table = D.WordTable(['w%d' % i for i in range(args.vocabulary)], vocab.to(dev).contiguous())
    # 2048 questions about ~1850 distinct clips: 10 % of the questions ask about the clip of the question before
    rs = np.random.default_rng(2)
    names = list(clips)
    picks = rs.permutation(args.library_clips)[:B]
    for q in range(1, B):
        if rs.random() < 0.1:
            picks[q] = picks[q - 1]
    items = []
    for i in range(B):
        q = synth.make_question(config, 0, i, T=T, with_video=False)
        ids = rs.integers(0, args.vocabulary, q['question'].shape[0]).astype(np.int32)
        items.append(dict(nmn_program_list=q['nmn_program_list'], prog_str_to_question_tokens=q['prog_str_to_question_tokens'], answer=q['answer'],
                          video_id=names[picks[i]], video_features=clips[names[picks[i]]], question=vocab[torch.from_numpy(ids).long()],
                          question_ids=ids))
    n_distinct = len(set(picks.tolist()))
    resident = D.pack_questions(items, dev)             # leg C's inputs, made once
    torch.cuda.synchronize()
    h2d = {}

    def step_a(tr):
        b = D.pack_questions(items, dev)
        h2d['A'] = b.h2d_bytes
        tr.step(b.programs, b.spans, b.video, b.question, b.q_lens, b.answers, video_index=b.video_index, video_len=b.video_len)

    def step_b(tr):
        b = D.pack_questions(items, dev, clip_library=library, word_table=table)
        h2d['B'] = b.h2d_bytes + 4 * n_distinct        # + the library rows of the step's clips, which the pass uploads (no lengths: all T)
        tr.step(b.programs, b.spans, None, None, b.q_lens, b.answers, video_index=b.video_index, library=b.library, question_ids=b.question_ids,
                words=b.words)

    def step_c(tr):
        b = resident
        tr.step(b.programs, b.spans, b.video, b.question, b.q_lens, b.answers, video_index=b.video_index, video_len=b.video_len)

    legs = {k: (fn, trainer()) for k, fn in (('A', step_a), ('B', step_b), ('C', step_c)) if args.only in (None, k)}
    gc.collect()
    gc.freeze()
    for fn, tr in legs.values():
        for _ in range(args.warmup):
            fn(tr)
        tr.check()
    torch.cuda.synchronize()
    blocks = {k: [] for k in legs}
    for _ in range(args.blocks):
        for k, (fn, tr) in legs.items():
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn(tr)
            torch.cuda.synchronize()
            blocks[k].append((time.perf_counter() - t0) / args.steps * 1e3)
    for _, tr in legs.values():
        tr.check()
    n_words = int(sum(resident.q_lens))
    result = dict(shape=dict(questions=B, distinct_clips=n_distinct, library_clips=args.library_clips, frames=T, video_size=V, features='bf16',
                             words=n_words, vocabulary=args.vocabulary, blocks=args.blocks, steps_per_block=args.steps),
                  legs={k: dict(ms_per_step=float(np.median(v)), block_ms=[round(x, 3) for x in v], block_spread_ms=[min(v), max(v)],
                                questions_per_s=B / (float(np.median(v)) * 1e-3)) for k, v in blocks.items()},
                  h2d_bytes_per_step=h2d,
                  gather_bytes_per_step=dict(gather_clips=2 * n_distinct * T * V * 2, gather_words=2 * n_words * E * 4))
    ms = {k: v['ms_per_step'] for k, v in result['legs'].items()}
    if len(ms) == 3:
        result['B_over_C'], result['A_over_B'] = ms['B'] / ms['C'], ms['A'] / ms['B']
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(result, open(args.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
