"""The seed-search routines of k_seed.hip one at a time (oracle/seed_routines_check.cpp, host build through the wavefront emulator's headers): k_sak_build's key records against a
base-by-base construction; compareSeqToGenome with keys, without keys and the oracle's; mmpRunT<u32> and mmpRunT<u64> against the oracle's maxMappableLength and a brute-force scan
of the interval, intervals of more than 2^32 entries included; seedLookup and nextPiece against base-by-base restatements.  Small adversarial genomes from the project's own index
twin.  The check classifies every case from the reference side and fails when a class never occurred, or when fewer than half of the searches are clean (the order total, the
brute-force scan binding)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.environ.get("EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="the host clang++ of ROCm is missing")
# 100 genomes of 4000 trials: about 30 s of one core with the build (7 s); the rarest class (a read's non-ACGT code inside the key) then has ~2000 cases, lookup kind 2 ~1000
TRIALS = 400000


def build_check(exe, timeout=None):
    subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O2", "-Wno-unknown-attributes", "-Wno-unused-result", "-D_GNU_SOURCE", "-I", "oracle/wave_emul", "-I", "star_amd/csrc/engine", "-I", "include", "-I", "oracle",
                           "oracle/seed_routines_check.cpp", "oracle/index_emul.cpp", "oracle/wave_emul/emu.cpp", "oracle/wave_emul/emu_lds.cpp", "-o", exe, "-ldl"], cwd=ROOT, timeout=timeout)


def test_seed_routines_against_oracle_and_brute_force(tmp_path):
    exe = str(tmp_path / "seed_routines_check")
    build_check(exe)
    p = subprocess.run([exe, str(TRIALS)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(p.stdout[-6000:])
    lines = p.stdout.strip().splitlines()
    assert p.returncode == 0 and lines[-1].endswith(": 0 differences"), p.stdout[-3000:]
    share = [float(m.group(1)) for m in (re.match(r"clean share ([0-9.]+)$", ln) for ln in lines) if m]
    assert len(share) == 1 and share[0] >= 0.5, share
    counts = [int(ln.split()[-1]) for ln in lines if ln.startswith("  ") and not ln.startswith("  clean / all") and not ln.startswith("  N / spacer") and ln.split()[-1].isdigit()]
    assert len(counts) >= 30 and min(counts) > 0, counts
