"""The seed-search routines of k_seed.hip as compiled gfx950 code on the MI355X: the cases the CPU check (oracle/seed_routines_check.cpp, tests/test_seed_routines.py) writes with
--dump -- genomes, suffix arrays, SAindex, pieces, intervals and the oracle's results -- through tests/seed_routines_gpu.hip, one lane per case: k_sak_build's records bit for bit
against the emulator's, compareSeqToGenome with and without keys, both mmpRunT instantiations, seedLookup, and mmpRun over intervals of more than 2^32 entries (one set: a suffix array of 9.1 GB
on the device, zero but for its ends).  One child process under a time limit; the step of it that opens the GPU runs under a shorter one of its own."""
import os
import subprocess
import sys

import pytest

from util import ROOT

pytestmark = pytest.mark.gpu
RUN = os.path.join(ROOT, "tests", "seed_routines_run.py")
TIMEOUT = 420          # above the sum of the child's own limits (seed_routines_run.py: 90 + 60 + 120 + 60 s); the host steps take 7 s, 1 s and 13 s


def test_seed_routines_on_hardware(tmp_path):
    p = subprocess.run([sys.executable, RUN, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=TIMEOUT)
    print(p.stdout[-3000:])
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    lines = [ln for ln in p.stdout.strip().splitlines() if ln.endswith("differences")]
    assert lines and lines[-1].endswith(": 0 differences"), p.stdout[-3000:]
