"""The passes of the sequence insertion as compiled gfx950 code on the MI355X: the cases of tests/seq_insert_cases.h (tests/test_seq_insert_routines.py runs
them on the plain-loop backend) through tests/seq_insert_gpu.hip on the product's HipBackend, with the expected values restated on the host in the same
process, and seqInsertHost / sjdbInsertHost against the files the reference wrote (tests/golden/seq_insert).  One child process under a time limit; the step
of it that opens the GPU runs under a shorter one of its own; the first HIP error ends the harness."""
import os
import subprocess
import sys

import pytest

from util import ROOT

pytestmark = pytest.mark.gpu
RUN = os.path.join(ROOT, "tests", "seq_insert_run.py")
TIMEOUT = 420          # above the sum of the child's own limits (seq_insert_run.py: 300 + 60 s)


def test_seq_insert_routines_on_hardware(tmp_path):
    p = subprocess.run([sys.executable, RUN, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=TIMEOUT)
    print(p.stdout[-20000:])
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    lines = [ln for ln in p.stdout.strip().splitlines() if ln.endswith("differences")]
    assert lines and lines[-1].endswith(": 0 differences"), p.stdout[-3000:]
