"""The routines and kernels of k_window.hip as compiled gfx950 code on the MI355X: the cases the CPU check (oracle/window_routines_check.cpp, tests/test_window_routines.py) writes
with --dump -- parameter blocks, chrBin, junction arrays, fabricated suffix-array entries, seed tables, launch geometries and the oracle's results -- through
tests/window_routines_gpu.hip: createExtendWindowsWithAlign and assignAlignToWindow with the table in LDS and in global memory, one wavefront per case; sjAlignSplit; the owner map
in LDS words and in a buffer; waveMax64 / waveMin32 / seedOfLane in every lane; then k_windows (first and middle launch), k_windows_big and k_order_* over the file's batches,
every buffer between verified guard bytes.  One child process under a time limit; the step of it that opens the GPU runs under a shorter one of its own.
Measured child timings: building the CPU check 12 s, check and dump 25 s here and 12 s on the GPU machine with the build (a case file of 5.8 MB: 480 window tables, 320 seed lists, 4 200
splits, 100 owner maps, 500 wave cases, 37 batches over 186 reads, 22 of them with the counters compared, the rarest class 4 cases), hipcc 9 s here and 2.5 s there, the harness 0.6 s on the MI355X (0.2 s of probes, 0.2 s
of batches); the whole test 16 s."""
import os
import subprocess
import sys

import pytest

from util import ROOT

pytestmark = pytest.mark.gpu
RUN = os.path.join(ROOT, "tests", "window_routines_run.py")
TIMEOUT = 600          # above the sum of the child's own limits (window_routines_run.py: 90 + 180 + 180 + 60 s); measured 12 + 25 + 9 + 0.6 s


def test_window_routines_on_hardware(tmp_path):
    p = subprocess.run([sys.executable, RUN, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=TIMEOUT)
    print(p.stdout[-3000:])
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    lines = [ln for ln in p.stdout.strip().splitlines() if ln.endswith("differences")]
    assert lines and lines[-1].endswith(": 0 differences"), p.stdout[-3000:]
