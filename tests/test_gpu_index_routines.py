"""The passes of the index builder as compiled gfx950 code on the MI355X: the cases of oracle/index_routines_cases.h (tests/test_index_routines.py runs them on the
plain-loop backend) through tests/index_routines_gpu.hip on the product's HipBackend -- k_forEach, rocPRIM radix_sort_pairs through a double_buffer (stability with
end_bit 63, which buffer holds the result), in-place scans, readOne -- with the expected values restated on the host in the same process: text, prefixKey, bucketOf,
saiClassFast, suffixSort, packArray, buildSAindex, buildAll, sjdbSearchOne, sjdbInsertDevice, and buildAll / sjdbInsertHost against the files the reference wrote
(tests/golden/tiny_index); plus forEach over 2^31 + 300 work-items (two slices).  One child process under a time limit; the step of it that opens the GPU runs under a
shorter one of its own; the first HIP error ends the harness.
Measured child timings: building and running the CPU check 5.5 s on the GPU machine (5 + 12 s elsewhere), hipcc 8.8 s, the harness 3.5 s on the MI355X (1.7 s of
backend primitives, 1.1 s of text / order / SAindex / buildAll on 37 genomes, 0.2 s of 17 junction insertions, 0.02 s of fixtures; forEach over 2^31 + 300 empty
work-items 1.8 ms, so it stays a case of the harness and needs no step of its own); the whole test 18 s.  The harness's limit: 40 s, ten times its time."""
import os
import subprocess
import sys

import pytest

from util import ROOT

pytestmark = pytest.mark.gpu
RUN = os.path.join(ROOT, "tests", "index_routines_run.py")
TIMEOUT = 700          # above the sum of the child's own limits (index_routines_run.py: 90 + 240 + 240 + 40 s)


def test_index_routines_on_hardware(tmp_path):
    p = subprocess.run([sys.executable, RUN, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=TIMEOUT)
    print(p.stdout[-20000:])
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    lines = [ln for ln in p.stdout.strip().splitlines() if ln.endswith("differences")]
    assert lines and lines[-1].endswith(": 0 differences"), p.stdout[-3000:]
