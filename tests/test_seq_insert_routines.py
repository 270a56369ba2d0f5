"""The passes of the sequence insertion (star_amd/csrc/index/seq_core.h: --genomeFastaFiles at the mapping stage) one at a time against a serial restatement
of the reference's insertSeqSA (tests/seq_insert_check.cpp, cases and comparisons in tests/seq_insert_cases.h; here on the plain-loop backend of
oracle/loop_backend.h, the gfx950 leg is tests/test_gpu_seq_insert_routines.py): the re-basing of old entries, the work text, the search of every candidate
with the tie rule at a spacer on all four strand pairs, the ranks of the candidates against memcmp, the merged array word by word with the zero entry behind
it, the new genome text, the SAindex against the sequential walk, seqInsertHost between guard bytes with its return codes, the GstrandBit check with numbers
alone.  tests/golden/seq_insert (five cases the REFERENCE ran, each on a plain index plus a new junction and on an annotated index; make_seq_insert_golden.py)
holds the restatement, seqInsertHost and the chain seqInsertHost -> sjdbInsertHost to the reference's own bytes -- needs neither the reference nor oracle/_ref.
The check classifies every case from the expected side and fails when a class never occurred or a case was not compared.
Measured: 12 s of one core for the build, 2 s for the run: 25 cases."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.environ.get("EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
GOLDEN = os.path.join("tests", "golden", "seq_insert")
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="the host clang++ of ROCm is missing")
N_CLASSES = 41


def build_check(exe, timeout=None):
    subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O2", "-Wno-unknown-attributes", "-Wno-unused-result", "tests/seq_insert_check.cpp", "-o", exe], cwd=ROOT, timeout=timeout)


def class_counts(out):
    return [int(ln.split()[-1]) for ln in out.splitlines() if ln.startswith("  ") and ln.split()[-1].isdigit()]


def compared(out):
    return [(int(m.group(1)), int(m.group(2))) for m in (re.match(r"compared (\d+) of (\d+) cases$", ln) for ln in out.splitlines()) if m]


def verdict(out, returncode):
    """None when the output is that of a complete run without differences, else what is wrong"""
    lines = out.strip().splitlines()
    if returncode != 0 or not lines or not lines[-1].endswith(": 0 differences"):
        return "exit status %d, last line %r" % (returncode, lines[-1] if lines else "")
    counts, done = class_counts(out), compared(out)
    if len(counts) != N_CLASSES or min(counts) == 0:
        return "classes: %r" % (counts,)
    if len(done) != 1 or done[0][0] != done[0][1] or done[0][1] == 0:
        return "cases: %r" % (done,)
    return None


def test_seq_insert_routines_against_restatement(tmp_path):
    exe = str(tmp_path / "seq_insert_check")
    build_check(exe)
    p = subprocess.run([exe, GOLDEN], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(p.stdout[-14000:])
    assert verdict(p.stdout, p.returncode) is None, (verdict(p.stdout, p.returncode), p.stdout[-4000:])
    assert "entries differ from the from-scratch order" in p.stdout
