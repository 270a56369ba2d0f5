"""bench.py's own plumbing on a box without a GPU (`--cpu-selftest`: gloo, the oracle behind the front end, a tiny genome):
the line is ONE JSON object under 4 KB that parses from the tail of stdout, `--gpus 2` really runs two ranks, and the variables that
redirect the product pipeline to test stand-ins are refused outside the self-test."""
import json
import os
import subprocess
import sys

import pytest

from util import ROOT, refstar

BENCH = os.path.join(ROOT, "bench.py")
pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(ROOT, "oracle", "_build", "libstaramd_cli_oracle.so")), reason="oracle front end not built")


def _line(stdout):
    tail = stdout[-4096:]                       # what a driver that keeps the last 4 KB of stdout sees
    last = tail.strip().splitlines()[-1]
    return json.loads(last), len(last)


@pytest.mark.parametrize("gpus", [1, 2])
def test_line_is_compact_and_counts_ranks(gpus, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    p = subprocess.run([sys.executable, BENCH, "--cpu-selftest", "--gpus", str(gpus), "--steps", "2", "--warmup", "1", "--workdir", str(tmp_path)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    d, n = _line(p.stdout)
    assert n < 4000
    assert d["n_gpus"] == gpus and d["steps"] == 2 and d["warmup"] == 1 and d["scaling"] == "weak"
    for k in ("metric", "value", "unit", "ms_per_step", "dtype", "config", "roofline", "loaded_libs", "extra"):
        assert k in d
    assert "workload" in d["config"] and "model" not in d["config"]
    for k in ("bound", "kernel", "achieved", "peak", "frac", "traffic", "kernel_ms", "algorithmic_bytes_per_launch"):
        assert k in d["roofline"]
    assert "selftest" in d                      # a CPU run can never pass for a measurement
    assert d["full"] is False and "cpu_baseline" not in d and "full_size_parity" not in d      # a plain run: the headline only
    assert d["value"] > 0
    extra = json.load(open(d["extra"]))
    assert "counters_per_pair" in extra and "pipeline" in extra
    # reads processed by all ranks: every rank maps (steps) x 2000 pairs in the timed region
    assert abs(d["value"] * d["ms_per_step"] * d["steps"] * 1e3 - gpus * 2 * 2000) < 0.05 * gpus * 4000      # (value is rounded to 4 digits: ~1 % at this tiny rate)


def test_dump_outputs_are_the_last_step_and_repeat(tmp_path):
    """--dump-outputs: float arrays of one length, at most 64 MB, only reads of the last timed step, and the same arrays from a second run in a fresh work
    directory (genome, index and reads generated again from their seeds)"""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    got = []
    for run in ("a", "b"):
        out = tmp_path / ("dump_" + run)
        p = subprocess.run([sys.executable, BENCH, "--cpu-selftest", "--steps", "3", "--warmup", "1", "--workdir", str(tmp_path / ("work_" + run)), "--dump-outputs", str(out)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
        assert p.returncode == 0, p.stderr[-2000:]
        d, n = _line(p.stdout)
        assert d["steps"] == 3 and n < 4000
        files = sorted(os.listdir(out))
        assert files and all(f.endswith(".npy") for f in files)
        got.append({f: np.load(os.path.join(out, f)) for f in files})
    a, b = got
    assert sorted(a) == sorted(b)
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    lens = {len(x) for x in a.values()}
    assert len(lens) == 1 and lens.pop() > 1000
    for f in a:
        assert a[f].dtype in (np.float32, np.float64), f
        assert np.array_equal(a[f], b[f]), f
    ids = a["read_id.npy"]
    assert ids.min() >= 3 * 2000 and ids.max() < 4 * 2000           # the self-test maps 2000 pairs per step: ids 6000 .. 7999 are the last of 1 + 3 steps
    assert (a["pos.npy"] >= 0).all() and (a["ref.npy"] >= -1).all()


def test_full_run_and_its_legs(tmp_path):
    """--full runs the timed path of a plain run, then the reference on the same index and FASTQ (cpu_baseline) and the full-size parity against it
    (a plain run does neither: test_line_is_compact_and_counts_ranks); the optional legs run only behind --full"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    p = subprocess.run([sys.executable, BENCH, "--cpu-selftest", "--full", "--steps", "2", "--warmup", "1", "--workdir", str(tmp_path)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    d, n = _line(p.stdout)
    assert n < 4000 and d["full"] is True and d["steps"] == 2 and d["value"] > 0
    assert "cpu_baseline" in d and "full_size_parity" in d
    if refstar.have_ref():
        assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["kind"] == "reference"
        fp = d["full_size_parity"]
        assert fp["sam_records_star_amd"] > 0 and fp["sam_multiset_identical"] and fp["sj_out_tab_identical"] and fp["log_final_counters_identical"], fp
    else:                                       # oracle/_ref/STAR not built: the leg ran and says why it has no figure
        assert "error" in d["cpu_baseline"] and d["full_size_parity"] is None
    p = subprocess.run([sys.executable, BENCH, "--cpu-selftest", "--extra-legs", "--workdir", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, env=env)
    assert p.returncode != 0 and "--full" in p.stderr and p.stdout.strip() == ""


def test_world_size_must_match_gpus(tmp_path):
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, BENCH, "--cpu-selftest", "--gpus", "2", "--workdir", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, env=env)
    assert p.returncode != 0 and "WORLD_SIZE=1" in p.stderr


@pytest.mark.parametrize("var", ["STARAMD_CLI_LIB", "STARAMD_ENGINE_LIB"])
def test_stand_in_libraries_are_refused(var, tmp_path):
    env = {k: v for k, v in os.environ.items() if k != "WORLD_SIZE"}
    env[var] = os.path.join(ROOT, "oracle", "_build", "libstaramd_cli_replay.so")
    p = subprocess.run([sys.executable, BENCH, "--steps", "1", "--warmup", "0", "--workdir", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, env=env)
    assert p.returncode != 0 and var in p.stderr and p.stdout.strip() == ""
