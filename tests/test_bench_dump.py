"""CPU tests of bench.py's output dump (--dump-outputs) and its argument checks.  No kernel is launched here: the dump is fed
a stand-in batch result and the mirror model's initial weights."""
import importlib.util
import os
import subprocess
import sys
import types

import numpy as np
import torch

from stair_amd import losses as L, spec, synth
from stair_amd.module_net import VideoNMN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    s = importlib.util.spec_from_file_location('bench_under_test', os.path.join(ROOT, 'bench.py'))
    m = importlib.util.module_from_spec(s)
    s.loader.exec_module(m)
    return m


def test_dump_is_float32_bounded_and_the_same_every_time(tmp_path):
    bench = _bench()
    config = dict(spec.DEFAULT_CONFIG)
    weights = synth.make_weights(config, 0)
    model = VideoNMN(config, pretrain_modules=set(L.CRITERION_MODULES))
    model.load_state_dict({k: torch.from_numpy(weights[k].copy()) for k in spec.state_dict_keys(config)})
    g = torch.Generator().manual_seed(0)
    B, A = 2048, config['answer_vocab_length']
    res = types.SimpleNamespace(logits=torch.randn(B, A, generator=g), pred=torch.randint(0, A, (B,), generator=g))
    loss = torch.rand(B, generator=g)
    total = bench.dump_outputs(str(tmp_path / 'a'), model, config, loss, res)
    bench.dump_outputs(str(tmp_path / 'b'), model, config, loss, res)
    files = sorted(os.listdir(tmp_path / 'a'))
    assert files == sorted(os.listdir(tmp_path / 'b'))
    assert total == sum(np.load(tmp_path / 'a' / f).nbytes for f in files) <= 64 << 20
    for f in files:
        a, b = np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f)
        assert a.dtype == np.float32, f
        assert np.array_equal(a, b), f
    assert np.array_equal(np.load(tmp_path / 'a' / 'logits.npy'), res.logits.numpy())
    assert np.array_equal(np.load(tmp_path / 'a' / 'pred.npy'), res.pred.numpy().astype(np.float32))
    assert np.array_equal(np.load(tmp_path / 'a' / 'loss.npy'), loss.numpy())
    state = model.state_dict()
    assert {'param.%s.npy' % k for k in spec.state_dict_keys(config)} <= set(files)
    for k in spec.state_dict_keys(config):
        full = state[k].numpy().reshape(-1)
        got = np.load(tmp_path / 'a' / ('param.%s.npy' % k))
        if full.size <= bench.DUMP_PARAM_SAMPLE:
            assert np.array_equal(got, full), k
        else:                                   # a fixed seeded sample, in index order
            assert got.size == bench.DUMP_PARAM_SAMPLE
            assert np.array_equal(got, full[bench._seeded_sample(full.size, bench.DUMP_PARAM_SAMPLE)]), k
    # inference: logits and pred only
    bench.dump_outputs(str(tmp_path / 'c'), model, config, None, res)
    assert sorted(os.listdir(tmp_path / 'c')) == ['logits.npy', 'pred.npy']


def test_steps_below_one_is_refused_before_any_gpu_call():
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0'], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and '--steps' in r.stderr and r.stdout.strip() == ''
