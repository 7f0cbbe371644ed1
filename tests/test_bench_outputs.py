"""bench.py's plain run, --full and --dump-outputs: the result line's keys, --steps, and the dumped arrays
(same inputs and same files from run to run; large arrays as a fixed seeded sample inside the byte budget)."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus", "config"}
FULL_ONLY = {"roofline", "cpu_baseline", "cfg5"}


def test_dump_outputs_samples_large_arrays(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 8 * 3 * 100)   # 100 entries per array
    rng = np.random.default_rng(0)
    arrays = {"small": rng.standard_normal((4, 5, 5)), "big": rng.standard_normal((10, 7, 9)), "s": np.array([2.5])}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in arrays}
    assert sorted(os.listdir(tmp_path / "a")) == ["big.npy", "s.npy", "small.npy"]
    assert all(v.dtype == np.float64 for v in got.values())
    assert np.array_equal(got["small"], arrays["small"]) and np.array_equal(got["s"], arrays["s"])
    # the sample: 100 distinct entries of the row-major array in index order, the same in every call
    idx = np.sort(np.random.default_rng(bench.SEED).choice(630, 100, replace=False))
    assert len(set(idx)) == 100 and np.array_equal(got["big"], arrays["big"].reshape(-1)[idx])
    assert np.array_equal(np.load(tmp_path / "b" / "big.npy"), got["big"])
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 8 * 3 * 100 + 3 * 128


def test_dump_budget_of_the_headline_workload():
    """order 10, n = 20, rank 256: 12 arrays, each at most its share of the budget -> under 64 MB with headers."""
    ranks = bench.tt_ranks(10, 20, 256)
    sizes = [1, 11] + [ranks[k] * 20 * ranks[k + 1] for k in range(10)]
    cap = bench.DUMP_MAX_BYTES // 8 // len(sizes)
    assert sum(8 * min(s, cap) + 128 for s in sizes) <= 64 * 10 ** 6


def _run(monkeypatch, capsys, argv):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    capsys.readouterr()
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_and_full_runs(handle, tmp_path, monkeypatch, capsys):
    """A plain run prints the headline keys only, --full adds the diagnostics to the same line; --steps is the
    number of timed steps; both runs start from the same inputs, so --dump-outputs writes the same arrays
    (each run rounds x steps + warmup times before the dump: 4 each)."""
    shape = ["--order", "5", "--mode", "6", "--rank", "12"]
    plain = _run(monkeypatch, capsys, shape + ["--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "p")])
    full = _run(monkeypatch, capsys, shape + ["--steps", "2", "--warmup", "2", "--dump-outputs", str(tmp_path / "f"),
                                              "--full", "--no-cpu", "--no-cfg5", "--no-extras"])
    assert HEADLINE <= set(plain) and not (FULL_ONLY & set(plain))
    assert HEADLINE | FULL_ONLY <= set(full)
    assert (plain["steps"], plain["warmup"], full["steps"], full["warmup"]) == (3, 1, 2, 2)
    ranks = bench.tt_ranks(5, 6, 12)
    gflop = (bench.flops_dot([6] * 5, ranks, ranks) + bench.flops_round([6] * 5, ranks)) / 1e9
    for line in (plain, full):
        assert line["unit"] == "GFLOP/s" and line["dtype"] == "f64" and line["higher_is_better"] is True
        assert line["ms_per_step"] > 0
        # value = algorithmic GFLOP of one step / the time of one step (both rounded in the line: 3 and 4 decimals)
        assert line["value"] == pytest.approx(gflop / (line["ms_per_step"] * 1e-3), rel=1e-2, abs=1e-3)
    assert "dot_ms" not in plain["config"] and full["config"]["dot_ms"] > 0 and full["roofline"]["launches_per_step"] > 0
    ranks = bench.tt_ranks(5, 6, 12)
    names = ["dot", "ranks"] + [f"core_{k:02d}" for k in range(5)]
    assert sorted(os.listdir(tmp_path / "p")) == sorted(n + ".npy" for n in names) == sorted(os.listdir(tmp_path / "f"))
    p = {n: np.load(tmp_path / "p" / f"{n}.npy") for n in names}
    f = {n: np.load(tmp_path / "f" / f"{n}.npy") for n in names}
    assert p["ranks"].tolist() == ranks and p["dot"].shape == (1,) and np.isfinite(p["dot"][0])
    for k in range(5):
        assert p[f"core_{k:02d}"].shape == (ranks[k], 6, ranks[k + 1]) and p[f"core_{k:02d}"].dtype == np.float64
    # same inputs, same number of rounds: fp64 results agree to rounding (1e-10 of each array's largest entry)
    for n in names:
        assert np.max(np.abs(p[n] - f[n])) <= 1e-10 * np.max(np.abs(p[n])), n
