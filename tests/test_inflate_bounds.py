"""The bounds of k_inflate.hip on malformed input, on the CPU: tests/inflate_bounds_check.cpp takes the kernel source into a program of its own (host build
through the wave emulator's headers) compiled with -fsanitize=address,undefined, and runs every member of every vector of tests/inflate_vectors.py plus
2 000 seeded mutations of the well-formed ones, each with its compressed bytes and its output in heap blocks of their exact sizes.  Clean = no sanitizer
report, every mutation ends with a status or with zlib's bytes, and no decode takes more than 8 * csize + ISIZE trips.  Nothing is loaded into Python
under a sanitizer and nothing is preloaded: the program is linked with the sanitizers' runtimes and started as a child.  (The emulator's work-items are
fibers that never unwind; AddressSanitizer's fake stacks for use-after-return would pile up by the gigabyte, so that one check is left out.)"""
import os
import struct
import subprocess

import pytest

from util import ROOT, capi
import inflate_vectors as V

CLANG = os.environ.get("EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="the host clang++ of ROCm is missing")
MUTATIONS, SEED = 2000, 20261021


def members_file(path):
    """every member of every vector whose BSIZE chain can be walked: csize, isize, crc, expected status, bytes"""
    n_good = n_bad = 0
    with open(path, "wb") as f:
        for name, (data, _) in V.wellformed().items():
            for d, crc, isize in V.members_of(data):
                f.write(struct.pack("<IIII", len(d), isize, crc, 0) + d)
                n_good += 1
        for name, (data, member, status) in V.malformed().items():
            d, crc, isize = V.members_of(data)[member]
            f.write(struct.pack("<IIII", len(d), isize, crc, capi.InflateDevice.STATUS.index(status)) + d)
            n_bad += 1
    return n_good, n_bad


def test_bounds_program_is_clean(tmp_path):
    exe, vec = str(tmp_path / "inflate_bounds_check"), str(tmp_path / "members.bin")
    n_good, n_bad = members_file(vec)
    assert n_good > 60 and n_bad == len(V.malformed()) >= 25
    subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fsanitize-address-use-after-return=never", "-fno-omit-frame-pointer",
                           "-Wno-unknown-attributes", "-D_GNU_SOURCE", "-I", "oracle/wave_emul", "tests/inflate_bounds_check.cpp", "oracle/wave_emul/emu.cpp",
                           "oracle/wave_emul/emu_lds.cpp", "-o", exe, "-ldl", "-lz"], cwd=ROOT, timeout=600)
    p = subprocess.run([exe, vec, str(MUTATIONS), str(SEED)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("clean") and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, (p.stdout[-2000:], p.stderr[-4000:])
    assert "members: %d inflated, %d rejected as expected" % (n_good, n_bad) in p.stdout, p.stdout
    # the mutations are of all three kinds, and both outcomes occur (else the run shows nothing about one of them)
    words = p.stdout.replace(",", " ").replace(":", " ").split()
    flips, cuts, splices = (int(words[words.index(k) - 1]) for k in ("flips", "cuts", "splices"))
    rejected, inflated = int(words[words.index("rejected", words.index("splices")) - 1]), int(words[words.index("inflated", words.index("splices")) - 1])
    assert flips + cuts + splices == MUTATIONS and min(flips, cuts, splices) > MUTATIONS // 5 and rejected > MUTATIONS // 2 and inflated > 0, p.stdout
