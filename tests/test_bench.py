"""bench.py's contract: a plain run prints the headline figures only, --full adds everything else, --dump-outputs writes
what the last timed step computed (float64, bounded, a fixed sample of larger outputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_the_default():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"], ["--gpus", "2", "--dump-outputs", "out"]])
def test_bad_arguments_are_refused(argv):
    with pytest.raises(SystemExit):
        bench.parse_args(argv)


def test_write_outputs_whole_within_budget(tmp_path):
    a = np.arange(10, dtype=np.float64)
    b = np.linspace(0.0, 1.0, 5, dtype=np.float32)
    info = bench.write_outputs(str(tmp_path), {"a": a, "b": b})
    assert info == {"a": [10, 10], "b": [5, 5]}
    ra, rb = np.load(tmp_path / "a.npy"), np.load(tmp_path / "b.npy")
    assert ra.dtype == np.float64 and rb.dtype == np.float64
    assert np.array_equal(ra, a) and np.array_equal(rb, b.astype(np.float64))


def test_write_outputs_samples_the_longest_arrays_the_same_way_every_time(tmp_path):
    big = np.arange(200000, dtype=np.float64)
    small = np.arange(100, dtype=np.float64)
    budget = 2 * 4096 + 8 * 20000
    info = bench.write_outputs(str(tmp_path / "one"), {"big": big, "small": small}, budget=budget)
    bench.write_outputs(str(tmp_path / "two"), {"big": big, "small": small}, budget=budget)
    assert info["small"] == [100, 100] and info["big"][1] == 200000 and 0 < info["big"][0] < 20000
    total = sum(os.path.getsize(tmp_path / "one" / f) for f in os.listdir(tmp_path / "one"))
    assert total <= budget
    s1, s2 = np.load(tmp_path / "one" / "big.npy"), np.load(tmp_path / "two" / "big.npy")
    assert np.array_equal(s1, s2)                                # fixed positions
    assert np.all(np.diff(s1) > 0)                               # distinct entries, ascending order
    assert np.array_equal(np.load(tmp_path / "one" / "small.npy"), small)


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    """A plain run of the reduced workload: one compact JSON line with the headline keys and none of --full's, and the
    dumped outputs of the last timed step equal to the CPU oracle's on the same seeded inputs."""
    from oracle import oracle as orc
    from smcp_amd import problems
    from smcp_amd.symbolic import Symbolic
    out = tmp_path / "outputs"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--workload", "synth6k", "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    r = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in r, k
    assert r["steps"] == 3 and r["warmup"] == 1 and r["dtype"] == "f64" and r["higher_is_better"] is True
    assert r["value"] > 0 and abs(r["value"] * r["ms_per_step"] - 1e3) < 1.0
    assert not set(bench.FULL_ONLY + ("secondary",)) & set(r), sorted(r)
    assert len(lines[0]) < 4000

    # the same inputs as bench.py builds them (seeds 0, 1, 2), solved by the oracle
    pat, m, density, _ = bench.build_workload("synth6k")
    symb = Symbolic(pat)
    cptr, cidx, cval = problems.random_constraints(symb, m, density=density, seed=1)
    S = orc.Sym(symb)
    A = problems.random_factor_blkval(symb, seed=0)
    orc.llt(S, A)
    pos = symb.ccs_to_blk()
    msk = np.zeros(symb.blklen, dtype=bool)
    msk[pos] = True
    rng = np.random.default_rng(2)
    bx = rng.standard_normal(symb.blklen) * msk
    by = rng.standard_normal(m)
    Lh = A.copy()
    orc.cholesky(S, Lh)
    Yh = Lh.copy()
    orc.projected_inverse(S, Yh)
    K = orc.KKT(S, cptr, cidx, cval)
    xr, yr = K.solve(Lh, Yh, K.schur_factor(Lh, Yh), bx, by, 1.0)
    want = {"x": xr[pos], "y": yr, "cholesky_factor": Lh[pos], "projected_inverse": Yh[pos]}
    assert sorted(os.listdir(out)) == sorted(k + ".npy" for k in want)
    assert r["outputs"]["entries_written_of_computed"] == {k: [len(v), len(v)] for k, v in want.items()}
    for k, v in want.items():
        got = np.load(out / (k + ".npy"))
        assert got.dtype == np.float64 and got.shape == v.shape, k
        err = np.linalg.norm(got - v) / np.linalg.norm(v)
        assert err < 1e-9, (k, err)
