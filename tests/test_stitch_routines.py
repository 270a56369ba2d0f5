"""The wave-cooperative routines of k_stitch.hip one at a time (oracle/stitch_routines_check.cpp, host build through the wavefront emulator's headers, every call one emulated
wavefront of 64 lanes): coopExtend against extendAlign and coopStitch against stitchAlignToTranscript of oracle/lane_routines_ref.h; coopSjdbFind, coopSjdbHash and sjdbHashFind
against a linear scan and binarySearch2 on tables of unique pairs of 1 .. 64^3 + 1 junctions, the hash tables filled by the product's own sjdbHashFill; replayWindow and both forms
of recordCandidate (recordCandidateImpl / compactArena over LDS and over global memory) against a sequential list after stitchWindowAligns.cpp:232-303 on synthetic candidate logs;
blocksOverlap against the oracle's.  Inputs are steered at the chunk boundaries of the 64-lane loops: scans, gaps, repeats and lists of more than 64 and more than 128 positions,
maxima in a second or later trip, runs of equal starts at every offset, hash clusters that wrap.  Every call must return the same values in all 64 lanes.  The check classifies
every case from the reference side and fails when a class never occurred.  About 50 s of one core with the build (8 s); the rarest class has about 100 cases."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.environ.get("EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="the host clang++ of ROCm is missing")
N_CLASSES = 102


def build_check(exe, timeout=None):
    # -ffp-contract=off -fno-unroll-loops: the product's flags for k_stitch.hip (coopExtend's pMMmax * double(...) comparisons are part of the result)
    subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-unroll-loops", "-Wno-unknown-attributes", "-Wno-unused-result", "-D_GNU_SOURCE",
                           "-I", "oracle/wave_emul", "-I", "star_amd/csrc/engine", "-I", "include", "-I", "oracle",
                           "oracle/stitch_routines_check.cpp", "oracle/wave_emul/emu.cpp", "oracle/wave_emul/emu_lds.cpp", "-o", exe, "-ldl"], cwd=ROOT, timeout=timeout)


def class_counts(out):
    return [int(ln.split()[-1]) for ln in out.splitlines() if ln.startswith("  ") and ln.split()[-1].isdigit()]


def test_stitch_routines_against_restatements(tmp_path):
    exe = str(tmp_path / "stitch_routines_check")
    build_check(exe)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    print(p.stdout[-12000:])
    lines = p.stdout.strip().splitlines()
    assert p.returncode == 0 and lines[-1].endswith(": 0 differences"), p.stdout[-4000:]
    counts = class_counts(p.stdout)
    assert len(counts) == N_CLASSES and min(counts) > 0, counts
