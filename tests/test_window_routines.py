"""The routines of k_window.hip one at a time and its kernels on batches made by hand (oracle/window_routines_check.cpp, host build through the wavefront emulator's headers).
Layer 1, every call one emulated wavefront of 64 lanes: createExtendWindowsWithAlign<false/true> against the oracle's anchor by anchor (return value, nW, limit flag, live rows),
assignAlignToWindow<false/true> against the oracle's seed by seed (the whole list, nwa, lrec, tooMany, overflow, nBlocks), sjAlignSplit against the oracle's % and / with offsets
around 2^32, ownInsert / ownLookup against "flank beats core, then the higher window" over LDS words and over a buffer, waveMax64 / waveMin32 / seedOfLane against loops.  Layer 2:
k_windows (first and middle launch), k_windows_big and k_order_* with the engine's launch shapes over fabricated suffix-array entries, seed tables, chrBin and junction arrays, per
read against buildWindows() of the oracle; places in the pools, work items, item classes, the order array, pool overflow and guard bytes around every buffer.  Reads that reach
alignWindowsPerReadNmax are compared in their status bit alone (the reference's map then points at an overwritten window); the check fails below 95 % of reads compared in full, when
the lanes of a wavefront disagree on a wave-uniform value, and when a class of cases never occurred.
DC_nSAenum and DC_nWindows are compared with what the launches of each geometry count for the oracle's run (chunks of 64, the stop at too many anchors, reads counted again after an
overflow: DESIGN.md 5.2) in every batch without a read at the limit: 58 of the 90 batches, all with non-zero values, 26 with reads counted again; a run in which none is compared fails.
About 55 s of one core with the build (12 s): 8 s for 900 window tables of 47 000 anchors, 990 seed lists of 63 000 seeds, 22 700 splits, 400 owner maps and 500 wave cases, 34 s
for 90 batches over 310 reads, 97.7 % of them compared in full.  A batch is ~0.4 s of the emulator, which keeps the classes of whole reads small: the rarest, a seed of 1000 loci, has
3 cases, a read with more than 1024 windows 4 (1.5 s each per geometry), one-locus reads on chromosomes from 0x3FFF 6, reads at the window limit 7; the rarest class of the routines
(a neighbour on another chromosome, a list of 63 rows, a compaction that leaves two rows) has 70 to 80.  No read has an est that passes 32 bits (4096 windows of 20 rows)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.environ.get("EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="the host clang++ of ROCm is missing")
N_CLASSES = 107


def build_check(exe, timeout=None):
    subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O2", "-Wno-unknown-attributes", "-Wno-unused-result", "-D_GNU_SOURCE", "-I", "oracle/wave_emul", "-I", "star_amd/csrc/engine",
                           "-I", "include", "-I", "oracle", "oracle/window_routines_check.cpp", "oracle/wave_emul/emu.cpp", "oracle/wave_emul/emu_lds.cpp", "-o", exe, "-ldl"], cwd=ROOT, timeout=timeout)


def class_counts(out):
    return [int(ln.split()[-1]) for ln in out.splitlines() if ln.startswith("  ") and ln.split()[-1].isdigit()]


def compared_share(out):
    return [float(m.group(1)) for m in (re.match(r"compared share ([0-9.]+)$", ln) for ln in out.splitlines()) if m]


def test_window_routines_against_oracle(tmp_path):
    exe = str(tmp_path / "window_routines_check")
    build_check(exe)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    print(p.stdout[-14000:])
    lines = p.stdout.strip().splitlines()
    assert p.returncode == 0 and lines[-1].endswith(": 0 differences"), p.stdout[-4000:]
    counts = class_counts(p.stdout)
    assert len(counts) == N_CLASSES and min(counts) > 0, counts
    share = compared_share(p.stdout)
    assert len(share) == 1 and share[0] >= 0.95, share
    compared = [m.groups() for m in (re.match(r"counters compared in (\d+) of \d+ batches, (\d+) of them with non-zero values$", ln) for ln in lines) if m]
    assert len(compared) == 1 and int(compared[0][1]) > 0, compared
