"""The passes of the index builder (star_amd/csrc/index/index_core.h, sjdb_core.h) one at a time against independent restatements of the reference's
rules (oracle/index_routines_check.cpp, cases and comparisons in oracle/index_routines_cases.h; here on the plain-loop backend of oracle/loop_backend.h, the
gfx950 leg is tests/test_gpu_index_routines.py): buildText, prefixKey, bucketOf and saiClassFast at every text position against byte loops and a literal
funCalcSAiFromSA; suffixSort against std::sort with the padding rule stated directly (dSA[0, nSA) entry by entry, the dropped tail as a permutation, ISA as
the inverse, `rounds` held exactly to the longest common prefix); packArray / packedGetW against packedSet at widths 33, 34, 35, 36, 40, 63 and 3;
buildSAindex against the sequential walk of genomeSAindex.cpp at GstrandBit 32, 33 and 36 and L = 1, 2, 3, 6, 8, 12 (14 is left to bench.py --full); buildAll
byte for byte with its return codes and exact capacities between guard bytes; sjdbSearchOne against a linear scan, sjdbInsertDevice against stable_sort, a
two-pointer merge and the reference's SAindex patch rule (old N marks kept, new suffixes mark) over old indexes built by the brute-force order; the backend
primitives at n = 1 .. 3 000 001 against loops.  tests/golden/tiny_index (three genomes the REFERENCE indexed plain and with a GTF; make_index_golden.py)
holds the restatements, buildAll and sjdbInsertHost to the reference's own bytes -- needs neither the reference nor oracle/_ref.  The check classifies every
case from the expected side and fails when a class never occurred or a case was not compared.
Measured: 5 s of one core for the build, 12 s for the run: 196 cases (49 pack, 90 primitive, 37 genome, 17 insertion, 3 fixture cases); the rarest classes
(nSA 0, U = 2 in the last round, nInd <= 2, the N run of 600) have one case each by construction."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.environ.get("EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
FIXTURES = os.path.join("tests", "golden", "tiny_index")
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="the host clang++ of ROCm is missing")
N_CLASSES = 100


def build_check(exe, timeout=None):
    subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O2", "-Wno-unknown-attributes", "-Wno-unused-result", "oracle/index_routines_check.cpp", "-o", exe], cwd=ROOT, timeout=timeout)


def class_counts(out):
    return [int(ln.split()[-1]) for ln in out.splitlines() if ln.startswith("  ") and ln.split()[-1].isdigit()]


def compared(out):
    return [(int(m.group(1)), int(m.group(2))) for m in (re.match(r"compared (\d+) of (\d+) cases$", ln) for ln in out.splitlines()) if m]


def test_index_routines_against_restatements(tmp_path):
    exe = str(tmp_path / "index_routines_check")
    build_check(exe)
    p = subprocess.run([exe, FIXTURES], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(p.stdout[-14000:])
    lines = p.stdout.strip().splitlines()
    assert p.returncode == 0 and lines[-1].endswith(": 0 differences"), p.stdout[-4000:]
    counts = class_counts(p.stdout)
    assert len(counts) == N_CLASSES and min(counts) > 0, counts
    done = compared(p.stdout)
    assert len(done) == 1 and done[0][0] == done[0][1] and done[0][1] > 0, done
