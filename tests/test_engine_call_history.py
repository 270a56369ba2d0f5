"""The results of a batch depend on (index, tables, params, batch) alone, not on what the engine context did before.

Every other parity test calls the C ABI in one pattern: a fresh context, staramd_map_batch calls in sequence, the retry of an overflow straight after it.
A context carries state from call to call, though -- the resident results of an overflowed batch, prefetched uploads, grown pools, the batch in flight of
staramd_map_begin, tables and whitelists that can be replaced, an index that sharers follow.  Each scenario below is one call sequence (tests/history_run.py,
one process each); every result it receives is compared byte for byte with the oracle for the same (index, tables, params, batch).

    1  overflow(A) -> map_batch(A) with room: the resident results, no new launch
    2  overflow(A) -> map_begin(B) / map_end(B), |B| = |A| -> map_batch(A)
    3  overflow(A) -> map_resident -> map_batch(A): mapped again
    4  overflow(A) -> update_tables(--scoreGap -3) -> map_batch(A): A under the new parameters
    5  overflow(A) at BySJout stage 1 -> set_novel_junctions(whitelist, 2) -> map_batch(A)
    6  overflow(A) -> update_index (same genome) -> map_batch(A): mapped again
    7  overflow(A) -> mmMaxTotal / one base of a middle read / mate1Length edited in place -> map_batch(A): the edited batch
    8  a sharer's overflow(A) -> the owner's update_tables(--scoreGap -3) -> the sharer's map_batch(A)
    9  a batch that grows the pools, then a light one, and the other way round (tiny pools, --gpuResultSelect All)
   10  prefetch(B) -> map_batch(C) -> map_batch(B) (a prefetch hit); prefetch(B) -> cancel -> B's arrays refilled with D -> map_batch(D)
   11  map_begin(A) -> map_end(next=B) -> map_end; map_end into arrays too small -> map_end again with room
   12  batch geometry: 1, 2, 63, 64, 65, ... reads up to maxBatchReads and exactly maxBatchBases; a slice from an odd base offset
   13  the parameters of the 1st pass of a 2-pass chimeric run (resultSelect 2 without chimeric detection): exactly what resultSelect 1 returns, no partner

`-m gpu` runs them on the MI355X at the batch size of tests/test_gpu_parity.py; the CPU twin runs them on the wavefront emulator (engine.hip's host logic
unchanged, the kernels emulated) at the small batches it affords."""
import os
import pickle
import subprocess
import sys

import pytest

from util import refstar
from test_wave_emul import LIB as EMUL_LIB, CLANG, emul_lib  # noqa: F401  (emul_lib: the module fixture that builds the emulated engine)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEEDS_REF = pytest.mark.skipif(not refstar.have_ref(), reason="oracle/_ref/STAR missing (needed to build the index)")

SCENARIOS = list(range(1, 14))


def _run(dataset, scenario, n, tmp_path, sizes=(), emulated=False, timeout=900):
    from util import prepare
    os.makedirs(str(tmp_path), exist_ok=True)
    info = prepare(dataset, str(tmp_path), need_ref=False)
    pkl = os.path.join(str(tmp_path), "info.pkl")
    pickle.dump(info, open(pkl, "wb"))
    env = dict(os.environ)
    env.pop("STARAMD_ENGINE_LIB", None)
    if emulated:
        env["STARAMD_ENGINE_LIB"] = EMUL_LIB
        env["STARAMD_WIN_BLOCKS_BIG"] = "2"       # (the 64 blocks of the last k_windows launch own 3.9 GB of work space, which the emulated hipMalloc fills with its pattern)
    p = subprocess.run([sys.executable, os.path.join(HERE, "history_run.py"), pkl, str(tmp_path), str(scenario), str(n)] + [str(k) for k in sizes],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    last = (p.stdout.strip().splitlines() or [""])[-1]
    assert p.returncode == 0 and last.startswith("OK"), (last, p.stderr[-1500:])


def _dataset(scenario):
    return "pe150_chim" if scenario == 13 else "pe101"


# ---- on the wavefront emulator: <= 32 reads per batch, scenario 12 up to 65 -------------------------------------------------------------------------------
@NEEDS_REF
@pytest.mark.skipif(not os.path.exists(CLANG), reason="the host clang++ of ROCm missing")
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_call_history_emulated(scenario, tmp_path, emul_lib):
    _run(_dataset(scenario), scenario, 32, tmp_path, sizes=(1, 2, 63, 64, 65) if scenario == 12 else (), emulated=True)


# ---- on the MI355X: batches of 1,200 reads as tests/test_gpu_parity.py ------------------------------------------------------------------------------------
@pytest.mark.gpu
@NEEDS_REF
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_call_history(scenario, tmp_path, built):
    sizes = (1, 2, 63, 64, 65, 255, 256, 257, 1199, 1200) if scenario == 12 else ()
    _run(_dataset(scenario), scenario, 1200, tmp_path, sizes=sizes)


@pytest.mark.gpu
@NEEDS_REF
def test_call_history_geometry_single_end(tmp_path, built):
    """scenario 12 on 1x50 reads, which the lane kernel takes almost whole: up to 4096 reads (the data set's reads again where it has fewer)"""
    _run("se50", 12, 1200, tmp_path, sizes=(1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096))
