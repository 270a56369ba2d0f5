"""The kernels between the stitch walk and the result arrays as compiled gfx950 code on the MI355X: the cases the CPU check (oracle/tail_routines_check.cpp,
tests/test_tail_routines.py) writes with --dump -- parameter blocks, reads, DWinOut records, transcript and exon pools, candidate logs, block totals and the expected values of
the check's restatements -- through tests/tail_routines_gpu.hip: k_pack_reads, k_stitch_verify, k_stitch_replay (2 blocks, the dynamic LDS of launch depth 0, both arenas),
k_stitch_finish with chimSelectPartner, k_scan_local and k_scan_offsets each alone, then the six of them behind pass 0 and k_gather in the engine's order, every buffer between
guard bytes verified after each launch.  One child process under a time limit; the step of it that opens the GPU runs under a shorter one of its own.
Measured child timings: building the CPU check and writing the case file 3.4 s on the GPU machine (7.5 s elsewhere; a case file of 27.4 MB: 24 pack cases, 54 scans of block
totals, 180 batches over 22 000 reads and 54 000 windows, the rarest class 5 cases), hipcc 2.6 s, the harness 0.8 s on the MI355X (0.26 s of pack and scan cases, 0.08 s of replay
batches, 0.2 s of the tail in the engine's order); the whole test 7.4 s."""
import os
import subprocess
import sys

import pytest

from util import ROOT

pytestmark = pytest.mark.gpu
RUN = os.path.join(ROOT, "tests", "tail_routines_run.py")
TIMEOUT = 600          # above the sum of the child's own limits (tail_routines_run.py: 90 + 180 + 180 + 20 s); measured 3 + 0.4 + 2.7 + 0.8 s


def test_tail_routines_on_hardware(tmp_path):
    p = subprocess.run([sys.executable, RUN, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=TIMEOUT)
    print(p.stdout[-3000:])
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    lines = [ln for ln in p.stdout.strip().splitlines() if ln.endswith("differences")]
    assert lines and lines[-1].endswith(": 0 differences"), p.stdout[-3000:]
