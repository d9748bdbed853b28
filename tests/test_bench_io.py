"""bench.py's files: the output dump (--dump-outputs) and the prepared inputs
(--prepare-inputs).  No GPU: the functions are called on made-up results and
on a three-window batch."""
import os

import numpy as np

import bench
from pomfret_amd import WindowResult
from pomfret_amd.synth_aln import _SAVE_FIELDS, make_aln_batch


def _results(rng, n_windows, n_reads):
    o = WindowResult.alloc(n_windows, n_reads)
    o.decision[:] = rng.integers(-1, 2, n_windows)
    o.read_hp[:] = rng.integers(0, 3, n_reads)
    o.dir_table[:] = rng.integers(0, 5000, (n_windows, 2, 4))
    o.dir_fisher_p[:] = rng.random((n_windows, 2)) * 1e-12
    o.dir_score[:] = rng.random((n_windows, 2))
    o.win_n_reads[:] = rng.integers(0, 2000, n_windows)
    return o


def test_dump_outputs_whole(tmp_path):
    rng = np.random.default_rng(3)
    outs = [_results(rng, 5, 40), _results(rng, 3, 17)]
    bench.dump_outputs(str(tmp_path / "d"), outs)
    names = sorted(f[:-4] for f in os.listdir(tmp_path / "d"))
    assert names == sorted(f for f in WindowResult.__dataclass_fields__)
    for name in names:
        got = np.load(tmp_path / "d" / (name + ".npy"))
        want = np.concatenate([getattr(o, name) for o in outs])
        assert got.dtype == (np.float64 if name == "dir_fisher_p" else np.float32)
        assert got.shape == want.shape and np.array_equal(got, want)      # exact, Fisher p included


def test_dump_outputs_capped_sample_is_fixed(tmp_path):
    rng = np.random.default_rng(4)
    outs = [_results(rng, 64, 30_000), _results(rng, 64, 20_000)]
    cap = 60_000                                   # read_hp alone would take 200 kB
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), outs, max_bytes=cap)
    files = os.listdir(tmp_path / "a")
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= cap
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert np.array_equal(a, b)
        if f != "read_hp.npy":                     # the small fields are whole
            assert a.shape[0] == 128
    hp = np.load(tmp_path / "a" / "read_hp.npy")
    assert 0 < hp.shape[0] < 50_000
    # other values in the same shapes: the same elements are sampled
    for o in outs:
        o.read_hp += 1
    bench.dump_outputs(str(tmp_path / "c"), outs, max_bytes=cap)
    assert np.array_equal(np.load(tmp_path / "c" / "read_hp.npy"), hp + 1)


def test_prepared_inputs_round_trip(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "INPUT_CACHE", str(tmp_path / "inputs"))
    monkeypatch.setattr(bench, "WORKLOAD", dict(bench.WORKLOAD, n_windows=3, coverage=8))
    spec = bench.headline_spec(bench.WORKLOAD)
    path = bench.input_cache_dir(spec)
    assert path.startswith(str(tmp_path)) and not os.path.exists(path)
    assert bench.input_cache_dir(bench.headline_spec(bench.WORKLOAD, seed=1001)) != path
    bench.prepare_inputs()
    assert os.listdir(tmp_path / "inputs") == [os.path.basename(path)]      # no temporary directory left
    stamp = os.path.getmtime(os.path.join(path, "seq.npy"))
    bench.prepare_inputs()                                                   # already there: left alone
    assert os.path.getmtime(os.path.join(path, "seq.npy")) == stamp
    got, want = bench.load_inputs(path), make_aln_batch(spec)
    for k in _SAVE_FIELDS:
        a, b = getattr(got, k), getattr(want, k)
        assert a.dtype == b.dtype and np.array_equal(a, b), k
    assert np.array_equal(got.meta["orient"], want.meta["orient"])
    assert not got.seq.flags.writeable                                       # mapped read-only
