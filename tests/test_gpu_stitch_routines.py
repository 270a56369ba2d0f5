"""The wave-cooperative routines of k_stitch.hip as compiled gfx950 code on the MI355X: the cases the CPU check (oracle/stitch_routines_check.cpp, tests/test_stitch_routines.py)
writes with --dump -- genome, junction tables, reads, joins, extensions, look-ups, candidate logs and the restatements' results -- through tests/stitch_routines_gpu.hip, one
wavefront per case: coopExtend, coopStitch, coopSjdbFind / coopSjdbHash / sjdbHashFind, replayWindow and both forms of recordCandidate over LDS and global arenas, blocksOverlap.
Every lane's result is compared.  One child process under a time limit; the step of it that opens the GPU runs under a shorter one of its own.
Measured child timings: building the CPU check 8 s, check and dump 20 s (a case file of 15 MB: 11 000 extensions, 5 500 joins, 23 000 look-ups, 400 runs of 100 candidate logs, the
rarest class 27 cases), hipcc 12 s.  The harness itself is a few launches over those cases; its wall time on the device has not been measured yet, its limit is the 60 s of the seed
harness."""
import os
import subprocess
import sys

import pytest

from util import ROOT

pytestmark = pytest.mark.gpu
RUN = os.path.join(ROOT, "tests", "stitch_routines_run.py")
TIMEOUT = 480          # above the sum of the child's own limits (stitch_routines_run.py: 90 + 120 + 180 + 60 s)


def test_stitch_routines_on_hardware(tmp_path):
    p = subprocess.run([sys.executable, RUN, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=TIMEOUT)
    print(p.stdout[-3000:])
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    lines = [ln for ln in p.stdout.strip().splitlines() if ln.endswith("differences")]
    assert lines and lines[-1].endswith(": 0 differences"), p.stdout[-3000:]
