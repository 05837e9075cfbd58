"""Host-side check of a change to the plan builder: builds a fixed set of plans with two builds of the library and compares
everything the ABI reports about them -- stair_plan_get_info (bytes), the five arrays of stair_plan_nodes, every (name, begin,
end) of stair_plan_regions in order, stair_plan_store_first_counts, stair_plan_saved_offset of every token (which = 0, 1) and of
every question's decoder row, the mask of stair_plan_touched -- and, with --upload (needs a GPU), the index image that
stair_plan_upload writes into a zeroed workspace.

    python tools/plan_compare.py --parent /path/to/parent/libstair_hip.so [--upload] [--out table.txt]

Each library is loaded in a process of its own (STAIR_LIB_PATH)."""
import argparse
import ctypes as C
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLAGS = {'infer': 0, 'train': 1, 'train_nocse': 3, 'train_ext': 5, 'infer_ext': 4}
RAGGED100 = [100, 17, 65, 100, 33, 8, 64, 96]
RAGGED24 = [24, 5, 17, 24, 9, 1, 16, 23]


def plans():
    """(name, config, forms or None, n questions, T, n_videos or None, clip lengths or None, {flag name: flags})"""
    from stair_amd import spec, synth
    full = dict(spec.DEFAULT_CONFIG)
    tiny = dict(full, hidden_size=64, video_size=128, answer_vocab_length=16, max_video_length=40, object_types=10)
    yield 'corpus12', full, sorted(synth.CORPUS), 12, 64, None, None, FLAGS
    yield 'mixed48', full, None, 48, 64, None, None, FLAGS
    yield 'mixed256_shared', full, None, 256, 64, 128, None, FLAGS
    yield 'mixed256_shared_ragged', full, None, 256, 64, 128, [64 - (i * 7) % 40 for i in range(128)], FLAGS
    yield 'mixed2048', full, None, 2048, 64, None, None, FLAGS
    yield 'tinyH64', tiny, sorted(synth.CORPUS), 12, 40, None, None, FLAGS
    three = {'flags0': 0, 'flags1': 1, 'flags3': 3}
    yield 'ragged_T100', full, None, 48, 100, 8, RAGGED100, three
    yield 'ragged_T24', full, None, 48, 24, 8, RAGGED24, three


UPLOAD = {'corpus12': ('infer', 'train'), 'mixed48': ('infer', 'train'), 'ragged_T100': ('flags0', 'flags1'), 'ragged_T24': ('flags0', 'flags1')}


def dump(path, upload):
    from stair_amd import spec, synth
    from stair_amd._lib import lib, check, StairConfig, PlanInfo
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    out = {}
    for name, config, forms, n, T, n_videos, lens, flagset in plans():
        if forms:
            qs = [synth.make_question(config, 0, i, form=f, with_video=False) for i, f in enumerate(forms)]
        else:
            qs = [synth.make_question(config, 21, i, T=T, forms=synth.ALL_FORMS, with_video=False) for i in range(n)]
        enc = [np.asarray(spec.encode_program(q['nmn_program_list']), dtype=np.int32) for q in qs]
        prog_off = np.zeros(n + 1, np.int32); np.cumsum([len(e) for e in enc], out=prog_off[1:])
        tokens = np.concatenate(enc)
        lo = np.zeros(len(tokens), np.int32); hi = np.zeros(len(tokens), np.int32)
        for q in range(n):
            for i, c in enumerate(enc[q]):
                if c == spec.TOK_SPAN:
                    lo[prog_off[q] + i], hi[prog_off[q] + i] = qs[q]['prog_str_to_question_tokens'][i]
        q_off = np.zeros(n + 1, np.int32); np.cumsum([q['question'].shape[0] for q in qs], out=q_off[1:])
        cfg = StairConfig(config['hidden_size'], config['video_size'], config['text_size'], config['answer_vocab_length'],
                          config['max_video_length'], config['object_types'], 1 if config['have_pretrain_head'] else 0)
        h = C.c_void_p()
        check(lib.stair_ctx_create(C.byref(cfg), C.byref(h)))
        for fname, flags in flagset.items():
            plan = C.c_void_p()
            if n_videos is None:
                check(lib.stair_plan_build(h, n, ip(prog_off), ip(tokens), ip(lo), ip(hi), ip(q_off), T, flags, C.byref(plan)))
            else:
                voq = np.asarray([i % n_videos for i in range(n)], np.int32)
                vl = np.asarray(lens if lens else [T] * n_videos, np.int32)
                check(lib.stair_plan_build_ragged(h, n, ip(prog_off), ip(tokens), ip(lo), ip(hi), ip(q_off), n_videos, ip(voq), ip(vl), T,
                                                  flags, C.byref(plan)))
            rec = {}
            info = PlanInfo()
            check(lib.stair_plan_get_info(plan, C.byref(info)))
            rec['info'] = bytes(info)
            tab = [np.empty(info.n_nodes, np.int32) for _ in range(5)]
            check(lib.stair_plan_nodes(plan, *[ip(t) for t in tab], info.n_nodes))
            rec['nodes'] = tab
            cap = 65536
            nm = (C.c_char_p * cap)(); beg = (C.c_int64 * cap)(); end = (C.c_int64 * cap)()
            k = lib.stair_plan_regions(plan, h, nm, beg, end, cap)
            assert 0 < k < cap
            rec['regions'] = [(nm[i].decode(), beg[i], end[i]) for i in range(k)]
            if flags & 1:
                a, b = C.c_int32(-1), C.c_int32(-1)
                check(lib.stair_plan_store_first_counts(plan, C.byref(a), C.byref(b)))
                rec['store_first'] = (a.value, b.value)
                off = C.c_int64()
                saved = []
                for tok in list(range(info.n_nodes)) + [-1 - q for q in range(n)]:
                    for which in (0, 1):
                        check(lib.stair_plan_saved_offset(plan, tok, which, C.byref(off)))
                        saved.append(off.value)
                rec['saved'] = np.asarray(saved, np.int64)
                nw = lib.stair_weight_count(h)
                touched = np.zeros(nw, np.int32)
                check(lib.stair_plan_touched(h, plan, ip(touched), nw))
                rec['touched'] = touched
            if upload and fname in UPLOAD.get(name, ()):
                import torch
                ws = torch.zeros(info.workspace_bytes // 4, dtype=torch.float32, device='cuda:0')
                check(lib.stair_plan_upload(plan, C.c_void_p(ws.data_ptr()), ws.numel() * 4, None))
                torch.cuda.synchronize()
                (ibeg, iend), = [(b_, e_) for nme, b_, e_ in rec['regions'] if nme == 'idx']
                rec['idx'] = ws[ibeg:iend].cpu().numpy().view(np.int32).copy()
                del ws
            out['%s/%s' % (name, fname)] = rec
            lib.stair_plan_destroy(plan)
        lib.stair_ctx_destroy(h)
    with open(path, 'wb') as f:
        pickle.dump(out, f)


def same(a, b):
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and np.array_equal(a, b)
    if isinstance(a, list) and a and isinstance(a[0], np.ndarray):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', help='the other build of libstair_hip.so')
    ap.add_argument('--upload', action='store_true', help='also compare the uploaded index image (GPU)')
    ap.add_argument('--out', help='write the table here too')
    ap.add_argument('--dump', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.dump:
        dump(args.dump, args.upload)
        return 0
    sides = {}
    with tempfile.TemporaryDirectory() as tmp:
        for side, libpath in (('parent', os.path.abspath(args.parent)), ('change', None)):
            env = dict(os.environ)
            env.pop('STAIR_LIB_PATH', None)
            if libpath:
                env['STAIR_LIB_PATH'] = libpath
            f = os.path.join(tmp, side + '.pkl')
            subprocess.check_call([sys.executable, os.path.abspath(__file__), '--dump', f] + (['--upload'] if args.upload else []), env=env)
            sides[side] = pickle.load(open(f, 'rb'))
    keys = ['info', 'nodes', 'regions', 'store_first', 'saved', 'touched', 'idx']
    lines = ['%-36s %s' % ('plan', ' '.join('%-11s' % k for k in keys)) + ' regions  idx ints']
    failures = 0
    assert list(sides['parent']) == list(sides['change'])
    for name, p in sides['parent'].items():
        c = sides['change'][name]
        cells = []
        for k in keys:
            if (k in p) != (k in c):
                cells.append('MISSING'); failures += 1
            elif k not in p:
                cells.append('-')
            elif same(p[k], c[k]):
                cells.append('equal')
            else:
                cells.append('DIFFER'); failures += 1
        lines.append('%-36s %s %7d %9s' % (name, ' '.join('%-11s' % x for x in cells), len(c['regions']), len(c['idx']) if 'idx' in c else '-'))
    lines.append('%d plans compared, %d differences' % (len(sides['parent']), failures))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    return 1 if failures else 0


if __name__ == '__main__':
    sys.exit(main())
