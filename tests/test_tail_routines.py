"""The seven kernels between the stitch walk and the result arrays, one at a time and then in the engine's order, on reads, windows, pools and candidate logs made by hand
(oracle/tail_routines_check.cpp, host build through the wavefront emulator's headers): k_pack_reads against its definition; k_stitch_verify against "incoming = the maximum of 0
and mm[f] of the windows before, queued iff sens[f] is smaller" (lists as sorted multisets, cursors, counters, minIn of queued windows alone); k_stitch_replay in 2 blocks with a
small LDS arena against the sequential list of oracle/cand_log_ref.h -- first and second attempt, a window that fits neither arena, pools exactly sufficient and one record short;
k_stitch_finish with chimSelectPartner against the oracle's trBest / per-read limit / no-good-window rules restated over the lists, Oracle::emitRead for layout and selection and
the host's partnerOverWindows restated over its arrays; k_scan_local and k_scan_offsets (1 .. 5000 block totals, chunks of 1, 2, 3 and 5) against loops; then verify -> replay ->
finish -> scan_local -> scan_offsets -> gather over batches of 1, 256, 257 and 700 reads against the arrays of Oracle::emitRead byte for byte, with result arrays exactly as large
as the totals and one transcript or one exon short, and with CUR_FLAGS set beforehand.  Every buffer lies between guard bytes verified after each launch.  The check classifies
every case from the reference side and fails when a class never occurred or a case was not compared.
Measured: 7 s of one core for the build, 0.5 s for the run: 24 pack cases, 54 scans of block totals, 180 batches over 22 000 reads and 54 000 windows; the rarest classes (a
packWords value, a batch size of the tail, CUR_FLAGS set) have 5 to 8 cases."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.environ.get("EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="the host clang++ of ROCm is missing")
N_CLASSES = 101


def build_check(exe, timeout=None):
    # -ffp-contract=off -fno-unroll-loops: the product's flags for k_stitch.hip
    subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-unroll-loops", "-Wno-unknown-attributes", "-Wno-unused-result", "-D_GNU_SOURCE",
                           "-I", "oracle/wave_emul", "-I", "star_amd/csrc/engine", "-I", "include", "-I", "oracle",
                           "oracle/tail_routines_check.cpp", "oracle/wave_emul/emu.cpp", "oracle/wave_emul/emu_lds.cpp", "-o", exe, "-ldl"], cwd=ROOT, timeout=timeout)


def class_counts(out):
    return [int(ln.split()[-1]) for ln in out.splitlines() if ln.startswith("  ") and ln.split()[-1].isdigit()]


def compared(out):
    return [(int(m.group(1)), int(m.group(2))) for m in (re.match(r"compared (\d+) of (\d+) cases$", ln) for ln in out.splitlines()) if m]


def test_tail_routines_against_restatements(tmp_path):
    exe = str(tmp_path / "tail_routines_check")
    build_check(exe)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(p.stdout[-14000:])
    lines = p.stdout.strip().splitlines()
    assert p.returncode == 0 and lines[-1].endswith(": 0 differences"), p.stdout[-4000:]
    counts = class_counts(p.stdout)
    assert len(counts) == N_CLASSES and min(counts) > 0, counts
    done = compared(p.stdout)
    assert len(done) == 1 and done[0][0] == done[0][1] and done[0][1] > 0, done
