"""bench.py --dump-outputs: what the file layout promises a build-to-build comparison (no GPU: the helper and the flags only)."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location('bench', os.path.join(ROOT, 'bench.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def _weights():
    rng = np.random.default_rng(7)
    return {'Conv/kernel': rng.standard_normal((3, 3, 3, 32)).astype(np.float32),
            'Conv_BN/moving_variance': rng.uniform(0.5, 2.0, 32).astype(np.float32),
            'decoder_conv0_pointwise/kernel': rng.standard_normal((1, 1, 304, 256)).astype(np.float32)}


def _read(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_flags(monkeypatch):
    b = _bench()
    monkeypatch.setattr('sys.argv', ['bench.py', '--steps', '7', '--warmup', '2', '--dump-outputs', 'out'])
    a = b.parse()
    assert (a.steps, a.warmup, a.dump_outputs) == (7, 2, 'out')
    monkeypatch.setattr('sys.argv', ['bench.py'])
    assert b.parse().dump_outputs is None
    monkeypatch.setattr('sys.argv', ['bench.py', '--steps', '0'])
    with pytest.raises(SystemExit):
        b.parse()


def test_everything_fits(tmp_path):
    b = _bench()
    w = _weights()
    files = b.dump_outputs(str(tmp_path), 1.25, w)
    got = _read(str(tmp_path))
    assert set(files) == set(got) == {'loss.npy', 'Conv.kernel.npy', 'Conv_BN.moving_variance.npy',
                                      'decoder_conv0_pointwise.kernel.npy'}
    assert got['loss.npy'].dtype == np.float64 and got['loss.npy'].tolist() == [1.25]
    for name, a in w.items():
        f = got[name.replace('/', '.') + '.npy']
        assert f.dtype == np.float32 and np.array_equal(f, a)


def test_sampled_under_the_budget_and_repeatable(tmp_path):
    b = _bench()
    w = _weights()
    budget = 64 * 1024
    b.dump_outputs(str(tmp_path / 'a'), 0.5, w, budget=budget)
    b.dump_outputs(str(tmp_path / 'b'), 0.5, w, budget=budget)
    sizes = sum(os.path.getsize(os.path.join(str(tmp_path / 'a'), f)) for f in os.listdir(str(tmp_path / 'a')))
    assert sizes <= budget
    ga, gb = _read(str(tmp_path / 'a')), _read(str(tmp_path / 'b'))
    assert set(ga) == set(gb)
    for f in ga:
        assert ga[f].dtype in (np.float32, np.float64) and np.array_equal(ga[f], gb[f]), f
    big = ga['decoder_conv0_pointwise.kernel.npy']
    full = w['decoder_conv0_pointwise/kernel'].reshape(-1)
    assert 0 < big.size < full.size and np.isin(big, full).all()
