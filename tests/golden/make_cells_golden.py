#!/usr/bin/env python3
"""Golden vectors of the cell corpus (tests/program_cells.py) from the REFERENCE implementation on CPU.

Run in the build container only (needs /root/reference, which never travels to the GPU box):

    python tests/golden/make_cells_golden.py            writes tests/golden/cells.npz
    python tests/golden/make_cells_golden.py --check    recomputes and compares with the committed file, array by array, bit for bit

Like make_golden.py it imports the reference's VideoNMN behind the same stand-in modules, loads the synthetic weights of
stair_amd.synth and runs every cell -- all 371 of program_cells.cells() -- in two blocks:

    conv      tiny_conv   (H=64 V=128 A=16 max_video_length=40), T=24      Conv1d Temporal nets
    linear    tiny_linear (same, max_video_length=8), T=8                  Linear Temporal nets

Inputs are not stored: program_cells.question(config, seed, cell index, T) recreates them.  Stored, in fp32, data only:

    <block>/logits    [371, A]
    <block>/steps     one flat array: for every cell in order the results of the PRODUCER's node, of the hole's parent (the
                      module that reads the producer) and of the slot template's first module, each once, in program order

Every tensor-valued step of every cell would be 1.5 MB for the conv block alone, more than any fixture of this repository and than
a committed file may be, so the file keeps the logits and the nodes the cell is about; test_oracle_matches_reference_on_cells
checks the oracle's values of exactly those (the logits depend on every other node).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import make_golden as MG  # noqa: E402
import program_cells as PC  # noqa: E402

BLOCKS = [('conv', 'tiny_conv', 24), ('linear', 'tiny_linear', 8)]


def main():
    VideoNMN, _ = MG.import_reference()
    torch.manual_seed(0)
    torch.set_num_threads(4)
    cells = PC.cells()
    out, meta = {}, {'seed': MG.SEED, 'n_cells': len(cells), 'blocks': {}}
    for block, cname, T in BLOCKS:
        config = MG.CONFIGS[cname]
        model = MG.build_model(VideoNMN, config)
        model.pretrain_modules = set()              # raw module results, no pretrain heads
        logits, steps = [], []
        for k, c in enumerate(cells):
            d = PC.question(config, MG.SEED, k, T, program=c.program)
            data = {'question': torch.from_numpy(d['question']), 'video_features': torch.from_numpy(d['video_features']),
                    'prog_str_to_question_tokens': d['prog_str_to_question_tokens'],
                    'nmn_program_list': d['nmn_program_list'], 'nmn_program_idx': d['nmn_program_idx']}
            with torch.no_grad():
                r = model(data, return_res_by_step=False, return_result_of_each_step=True, test_mode=True)
            logits.append(MG.to_np(r['logits']).astype(np.float32))
            for i in PC.stored_nodes(c):
                res = r['result_of_each_step'][i][1]
                if isinstance(res, torch.Tensor):
                    steps.append(MG.to_np(res).astype(np.float32).reshape(-1))
        out[block + '/logits'] = np.stack(logits)
        out[block + '/steps'] = np.concatenate(steps)
        meta['blocks'][block] = {'config': config, 'T': T}
        print(block, out[block + '/logits'].shape, out[block + '/steps'].shape)
    out['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, 'cells.npz')
    if '--check' in sys.argv:
        z = np.load(path)
        assert sorted(z.files) == sorted(out)
        for k in out:
            assert z[k].dtype == out[k].dtype and z[k].shape == out[k].shape and z[k].tobytes() == out[k].tobytes(), k
        print('cells.npz: every array regenerated bit for bit')
        return
    np.savez_compressed(path, **out)
    print('cells.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
