#!/usr/bin/env python3
"""Regenerates tests/golden/dropout.npz by running the REFERENCE's VideoNMN in train() mode on CPU: the tiny Conv1d
configuration of make_golden.py (dropout = 0.25, as args.py:31), the 12 program forms, one forward pass per question under a fixed
torch seed.  torch's Philox stream cannot be reproduced elsewhere, but a mask can be RECORDED: forward hooks on every
nn.Dropout of the model note which elements each call kept (output != 0 where the input != 0; where the input is 0 the bit
says nothing and is stored as 0).  Fed back through the oracle's dropout hook (oracle/nmn_oracle.py `dropout=`), those masks
must reproduce the reference's train-mode logits and module results: that pins the oracle's `D` positions to the reference
itself (tests/test_oracle_golden.py::test_oracle_dropout_positions_match_reference_train_mode).

Stored -- masks and results only:
    q<qid>/keep/t<token>/<ordinal>   packed bits (np.packbits of the flattened mask): call number <ordinal> of an nn.Dropout
                                     inside the module call of program token <token> ('decoder': the decoder's)
    q<qid>/logits, q<qid>/step<i>    train-mode logits and every module / span result of the SAME pass (no pretrain heads)
    meta                             config, T, seeds, p, and per question the (token, ordinal, shape) of every call in call order

    python tests/golden/make_dropout_golden.py        (build container only: needs /root/reference)
"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G            # noqa: E402
from stair_amd import spec, synth  # noqa: E402

NAME, T = 'tiny_conv', 40
TORCH_SEED = 1234


def build_train_model(VideoNMN, config):
    with contextlib.redirect_stdout(io.StringIO()):
        model = VideoNMN(dict(config), pretrain_modules=set())
    weights = synth.make_weights(config, G.SEED)
    model.load_state_dict({k: torch.from_numpy(weights[k].copy()) for k in spec.state_dict_keys(config)})
    model.train()
    return model


class MaskRecorder:
    """Which program token's module call is running (forward pre / post hooks on the registered submodules; Superlative calls
    the Localize module from inside its own forward, which must not advance the interpreter's order) and what every
    nn.Dropout call kept."""

    def __init__(self, model):
        self.calls, self.order, self.depth, self.token = [], [], 0, None
        for name, mod in model.submodules.items():
            if name in ('video_encoder', 'text_encoder'):
                continue
            mod.register_forward_pre_hook(self._enter(name))
            mod.register_forward_hook(self._leave)
        for mod in model.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.register_forward_hook(self._dropout)

    def begin(self, program, registered):
        self.calls, self.depth, self.token = [], 0, None
        self.order = [i for i in range(len(program) - 1, -1, -1) if program[i] in registered]      # module_net.py:97-106
        self.program = program

    def _enter(self, name):
        def hook(mod, args):
            if self.depth == 0:
                if name == 'decoder':
                    assert not self.order
                    self.token = 'decoder'
                else:
                    self.token = self.order.pop(0)
                    while self.program[self.token] == 'Array2':      # modules.py:442 overrides __call__: no hooks fire for it
                        self.token = self.order.pop(0)
                    assert self.program[self.token] == name, (self.program[self.token], name)
                self.ordinal = 0
            self.depth += 1
        return hook

    def _leave(self, mod, args, out):
        self.depth -= 1

    def _dropout(self, mod, args, out):
        x = args[0]
        keep = (out != 0) & (x != 0)
        self.calls.append((self.token, self.ordinal, keep.detach().numpy().copy()))
        self.ordinal += 1


def main():
    VideoNMN, _ = G.import_reference()
    torch.set_num_threads(4)
    config = G.CONFIGS[NAME]
    assert config['dropout'] == 0.25
    model = build_train_model(VideoNMN, config)
    rec = MaskRecorder(model)
    registered = set(model.submodules.keys()) - {'video_encoder', 'text_encoder', 'decoder'}
    torch.manual_seed(TORCH_SEED)
    out, meta = {}, {'config': config, 'T': T, 'seed': G.SEED, 'torch_seed': TORCH_SEED, 'p': config['dropout'], 'questions': []}
    for qid, form in enumerate(synth.ALL_FORMS):
        d = synth.make_question(config, G.SEED, qid, form=form, T=T)
        data = {'question': torch.from_numpy(d['question']), 'video_features': torch.from_numpy(d['video_features']),
                'prog_str_to_question_tokens': d['prog_str_to_question_tokens'],
                'nmn_program_list': d['nmn_program_list'], 'nmn_program_idx': d['nmn_program_idx']}
        rec.begin(d['nmn_program_list'], registered)
        with torch.no_grad():
            r = model(data, return_res_by_step=False, return_result_of_each_step=True, test_mode=True)
        key = 'q%d/' % qid
        out[key + 'logits'] = G.to_np(r['logits'])
        for i, (params, res) in enumerate(r['result_of_each_step']):
            if isinstance(res, torch.Tensor):
                out[key + 'step%d' % i] = G.to_np(res)
        calls = []
        for token, ordinal, keep in rec.calls:
            out[key + 'keep/t%s/%d' % (token, ordinal)] = np.packbits(keep.reshape(-1))
            calls.append([token, ordinal, list(keep.shape)])
        meta['questions'].append({'qid': qid, 'form': form, 'calls': calls})
    out['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, 'dropout.npz')
    np.savez_compressed(path, **out)
    print('dropout', len(out), 'arrays,', os.path.getsize(path), 'bytes,',
          sum(len(q['calls']) for q in meta['questions']), 'nn.Dropout calls')


if __name__ == '__main__':
    main()
