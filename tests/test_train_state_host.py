"""CPU tests of stair_amd/train_state.py (the training state of a Trainer: validation, the atomic file, the torch.optim.Adam
translation) and of data.save_checkpoint's optional trainer argument.  No GPU, no library call: the states are built by hand
over real weight names of the tiny configuration."""
import copy
import os
import pickle

import pytest
import torch

from stair_amd import data as D, spec, train_state as TS

CONFIG = dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, answer_vocab_length=16, max_video_length=40, object_types=10)
TABLE = dict(spec.weight_table(CONFIG))
# six tensors under real names; the last one (Superlative) never gets a gradient
NAMES = ['submodules.Compare.param.0.weight', 'submodules.Compare.param.0.bias', 'submodules.Exists.param.3.weight',
         'submodules.Exists.pretrain_head.weight', 'submodules.Equals.pretrain_head.bias', 'submodules.Superlative.dense.0.bias']
UNTOUCHED = NAMES[-1]
SHAPES = {n: tuple(TABLE[n]) for n in NAMES}
NUMELS = [int(torch.Size(SHAPES[n]).numel()) for n in NAMES]


def _state(mode='ever'):
    g = torch.Generator().manual_seed(4)
    tensors = {}
    for n in NAMES:
        on = n != UNTOUCHED
        tensors[n] = {'exp_avg': torch.randn(SHAPES[n], generator=g) * on, 'exp_avg_sq': torch.rand(SHAPES[n], generator=g) * on,
                      'steps': 3 if on else 0, 'touched': int(on), 'ever': on, 'trainable': n != NAMES[1]}
    hyper = dict(copy.deepcopy(TS.HYPER), skip_untouched=mode, lr=1e-3, max_grad_norm=float('inf'), dropout=0.25, dropout_seed=7)
    return {'format': TS.FORMAT, 'names': list(NAMES), 'numels': list(NUMELS), 'tensors': tensors, 'iters': 3, 'questions_seen': 192,
            'world': 1, 'hyper': hyper}


def _equal(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_equal(v, b[k]) for k, v in a.items())
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def test_a_good_state_validates():
    TS.validate(_state(), NAMES, NUMELS)
    TS.validate(_state(), NAMES, NUMELS, SHAPES)
    TS.validate(_state('window'), NAMES, NUMELS, SHAPES)


def _missing_name(s):
    del s['tensors'][NAMES[2]]
    i = s['names'].index(NAMES[2])
    del s['names'][i], s['numels'][i]


def _extra_name(s):
    s['tensors']['submodules.Nope.weight'] = copy.deepcopy(s['tensors'][NAMES[0]])
    s['names'].append('submodules.Nope.weight')
    s['numels'].append(NUMELS[0])


def _wrong_shape(s):
    s['tensors'][NAMES[2]]['exp_avg'] = torch.zeros(3, 5)


def _float64(s):
    s['tensors'][NAMES[0]]['exp_avg_sq'] = s['tensors'][NAMES[0]]['exp_avg_sq'].double()


def _nan(s):
    s['tensors'][NAMES[3]]['exp_avg'][0, 1] = float('nan')


def _negative(s):
    s['tensors'][NAMES[4]]['exp_avg_sq'][0] = -1e-12


def _untouched_with_moments(s):
    s['tensors'][UNTOUCHED]['exp_avg'][1] = 0.5


def _unknown_format(s):
    s['format'] = 2


BAD = {'missing_name': (_missing_name, [NAMES[2], 'missing']),
       'extra_name': (_extra_name, ['submodules.Nope.weight', 'unexpected']),
       'wrong_shape': (_wrong_shape, [NAMES[2] + '.exp_avg', 'shape']),
       'float64_moment': (_float64, [NAMES[0] + '.exp_avg_sq', 'float64']),
       'nan_moment': (_nan, [NAMES[3] + '.exp_avg', 'NaN']),
       'negative_exp_avg_sq': (_negative, [NAMES[4] + '.exp_avg_sq', 'negative']),
       'untouched_with_moments': (_untouched_with_moments, [UNTOUCHED + '.exp_avg', 'touched']),
       'unknown_format': (_unknown_format, ['format', '2'])}


@pytest.mark.parametrize('case', sorted(BAD))
def test_validate_refuses_and_names_weight_and_field(case):
    spoil, words = BAD[case]
    s = _state()
    spoil(s)
    with pytest.raises(ValueError) as e:
        TS.validate(s, NAMES, NUMELS, SHAPES)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_validate_further_rules():
    s = _state()
    s['tensors'][NAMES[0]]['steps'] = -1
    with pytest.raises(ValueError, match='steps'):
        TS.validate(s, NAMES, NUMELS)
    s = _state()
    s['tensors'][UNTOUCHED]['steps'] = 2                    # touched == 0 but it has stepped
    with pytest.raises(ValueError, match='steps'):
        TS.validate(s, NAMES, NUMELS)
    # under 'window' the mask is per step: a tensor the LAST window did not touch keeps moments and steps
    s = _state('window')
    s['tensors'][NAMES[0]]['touched'] = 0
    TS.validate(s, NAMES, NUMELS, SHAPES)
    s['hyper']['skip_untouched'] = 'ever'
    with pytest.raises(ValueError, match=NAMES[0].replace('.', r'\.')):
        TS.validate(s, NAMES, NUMELS, SHAPES)
    # the frozen-and-once-touched tensor (NAMES[1]: not trainable, moments and steps from before) is fine
    assert not _state()['tensors'][NAMES[1]]['trainable'] and _state()['tensors'][NAMES[1]]['steps'] == 3
    s = _state()
    del s['hyper']['eps']
    with pytest.raises(ValueError, match='eps'):
        TS.validate(s, NAMES, NUMELS)
    with pytest.raises(ValueError, match='dict'):
        TS.validate([1, 2], NAMES, NUMELS)


def test_save_and_load_round_trip_every_field(tmp_path):
    s = _state()
    path = str(tmp_path / 'trainer_state.bin')
    TS.save(path, s)
    back = TS.load(path)
    assert _equal(s, back)
    TS.validate(back, NAMES, NUMELS, SHAPES)
    assert os.listdir(str(tmp_path)) == ['trainer_state.bin']             # no temporary file is left behind


def test_a_save_that_fails_leaves_the_earlier_file_whole(tmp_path, monkeypatch):
    path = str(tmp_path / 'trainer_state.bin')
    TS.save(path, _state())
    before = open(path, 'rb').read()
    seen = []

    def refuse(src, dst):
        seen.append((os.path.getsize(src), dst))                          # the temporary file has been written in full by now
        raise OSError('no rename today')
    later = _state()
    later['iters'] = 99
    monkeypatch.setattr(os, 'replace', refuse)
    with pytest.raises(OSError, match='no rename today'):
        TS.save(path, later)
    monkeypatch.undo()
    assert seen and seen[0][0] > 0 and seen[0][1] == path
    assert open(path, 'rb').read() == before
    assert os.listdir(str(tmp_path)) == ['trainer_state.bin']
    assert TS.load(path)['iters'] == 3


class _Boom:
    ran = []

    def __reduce__(self):
        return (_Boom.ran.append, ('executed',))


def test_a_pickled_object_is_refused_not_executed(tmp_path):
    path = str(tmp_path / 'trainer_state.bin')
    with open(path, 'wb') as f:
        pickle.dump(_Boom(), f)
    with pytest.raises(ValueError, match='not a training state'):
        TS.load(path)
    torch.save(_Boom(), path)
    with pytest.raises(ValueError, match='not a training state'):
        TS.load(path)
    assert _Boom.ran == []
    torch.save([1, 2, 3], path)                                            # loads, but is no state
    with pytest.raises(ValueError, match='does not hold a training state'):
        TS.load(path)
    with pytest.raises(FileNotFoundError, match='trainer_state.bin'):
        D.load_trainer_state(str(tmp_path / 'nowhere'))


# ---- torch.optim.Adam against itself ---------------------------------------------------------------------------------------------
LR, BETAS, EPS, WD = 1e-3, (0.8, 0.99), 1e-7, 0.01


def _toy():
    g = torch.Generator().manual_seed(12)
    params = [torch.nn.Parameter(torch.randn(SHAPES[n], generator=g)) for n in NAMES]
    grads = [[None if n == UNTOUCHED else torch.randn(SHAPES[n], generator=g) for n in NAMES] for _ in range(4)]
    return params, grads


def _steps(opt, params, grads):
    for gs in grads:
        for p, gr in zip(params, gs):
            p.grad = None if gr is None else gr.clone()
        opt.step()


def test_torch_adam_round_trip_and_resumed_run():
    params, grads = _toy()
    opt = torch.optim.Adam(params, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
    _steps(opt, params, grads[:2])
    sd = opt.state_dict()
    state = TS.from_torch_adam(sd, NAMES, shapes=SHAPES, iters=2, questions_seen=128)
    TS.validate(state, NAMES, NUMELS, SHAPES)
    assert state['hyper']['lr'] == LR and state['hyper']['betas'] == list(BETAS) and state['hyper']['weight_decay'] == WD
    assert state['tensors'][UNTOUCHED]['touched'] == 0 and state['tensors'][NAMES[0]]['steps'] == 2
    back, iters = TS.to_torch_adam(state, NAMES)
    assert iters == 2
    # the optimizer's own state_dict, exactly: same keys, equal tensors, no entry for the tensor without a gradient
    assert set(back) == set(sd) and sorted(back['state']) == sorted(sd['state']) == [0, 1, 2, 3, 4]
    assert len(back['param_groups']) == 1 and back['param_groups'][0] == sd['param_groups'][0]
    assert list(back['param_groups'][0]) == list(sd['param_groups'][0])
    for i, e in sd['state'].items():
        assert sorted(back['state'][i]) == sorted(e)
        for k, val in e.items():
            got = back['state'][i][k]
            if isinstance(val, torch.Tensor):
                assert isinstance(got, torch.Tensor) and got.dtype == val.dtype and got.shape == val.shape and torch.equal(got, val), (i, k)
            else:
                assert type(got) is type(val) and got == val, (i, k)
    # through a file as well, then into a fresh optimizer over copies of the weights: two more steps = four uninterrupted ones
    fresh = [torch.nn.Parameter(p.detach().clone()) for p in params]
    opt2 = torch.optim.Adam(fresh, lr=123.0)                              # every hyper-parameter comes from the loaded group
    opt2.load_state_dict(back)
    _steps(opt2, fresh, grads[2:])
    _steps(opt, params, grads[2:])
    for n, a, b in zip(NAMES, params, fresh):
        assert torch.equal(a, b), n
    assert not torch.equal(params[0], _toy()[0][0]) and torch.equal(params[-1], _toy()[0][-1])
    for i in range(5):
        for k in ('exp_avg', 'exp_avg_sq'):
            assert torch.equal(opt.state[params[i]][k], opt2.state[fresh[i]][k])
    assert params[-1] not in opt.state and fresh[-1] not in opt2.state


def test_from_torch_adam_checks_its_arguments():
    params, grads = _toy()
    opt = torch.optim.Adam(params, lr=LR)
    _steps(opt, params, grads[:1])
    sd = opt.state_dict()
    with pytest.raises(ValueError, match=UNTOUCHED.replace('.', r'\.')):  # no entry and no shape to make zero moments of
        TS.from_torch_adam(sd, NAMES)
    with pytest.raises(ValueError, match='lr'):
        TS.from_torch_adam(sd, NAMES, shapes=SHAPES, lr=1.0)
    with pytest.raises(ValueError, match='momentum'):
        TS.from_torch_adam(sd, NAMES, shapes=SHAPES, momentum=0.5)
    with pytest.raises(ValueError, match='no weight named'):
        TS.to_torch_adam(TS.from_torch_adam(sd, NAMES, shapes=SHAPES), NAMES + ['submodules.Nope.weight'])
    ams = torch.optim.Adam([torch.nn.Parameter(torch.zeros(2))], amsgrad=True).state_dict()
    with pytest.raises(ValueError, match='amsgrad'):
        TS.from_torch_adam(ams, ['submodules.Compare.param.0.bias'], shapes={})


# ---- data.save_checkpoint -------------------------------------------------------------------------------------------------------
class _Weights:
    """what save_checkpoint needs of a model"""

    def state_dict(self):
        return {n: torch.full(SHAPES[n], float(i)) for i, n in enumerate(NAMES)}


class _FakeTrainer:
    def state_dict(self):
        return _state()


def test_save_checkpoint_without_a_trainer_writes_the_two_files_and_no_third(tmp_path):
    out = str(tmp_path / 'ck')
    D.save_checkpoint(out, _Weights(), CONFIG)
    D.save_checkpoint(out, _Weights(), CONFIG, trainer=None)
    assert sorted(os.listdir(out)) == ['config.json', 'pytorch_model.bin']
    sd = torch.load(os.path.join(out, 'pytorch_model.bin'), weights_only=True)
    assert list(sd) == NAMES and all(torch.equal(sd[n], _Weights().state_dict()[n]) for n in NAMES)
    with pytest.raises(FileNotFoundError, match='trainer_state.bin'):
        D.load_trainer_state(out)


def test_save_checkpoint_with_a_trainer_adds_the_state_last(tmp_path, monkeypatch):
    out = str(tmp_path / 'ck')
    order, real = [], os.replace

    def spy(src, dst):
        order.append(os.path.basename(dst))
        real(src, dst)
    monkeypatch.setattr(os, 'replace', spy)
    D.save_checkpoint(out, _Weights(), CONFIG, trainer=_FakeTrainer())
    monkeypatch.undo()
    assert order == ['pytorch_model.bin', 'config.json', 'trainer_state.bin']
    assert sorted(os.listdir(out)) == ['config.json', 'pytorch_model.bin', 'trainer_state.bin']
    assert _equal(D.load_trainer_state(out), _state())

    class _Refusing:
        def state_dict(self):
            raise RuntimeError('refused step')
    stamp = {f: open(os.path.join(out, f), 'rb').read() for f in os.listdir(out)}
    with pytest.raises(RuntimeError, match='refused step'):           # the state is taken before any file is touched
        D.save_checkpoint(out, _Weights(), dict(CONFIG, hidden_size=1), trainer=_Refusing())
    assert {f: open(os.path.join(out, f), 'rb').read() for f in os.listdir(out)} == stamp
