"""Child process of tests/test_gpu_seq_insert_routines.py: one GPU step, under the time limit the parent sets.
    seq_insert_run.py <work dir>
builds tests/seq_insert_gpu.hip for gfx950 with hipcc and the product's HIPFLAGS (read from the Makefile) -- or takes oracle/_build/seq_insert_gpu where `make`
left one that is newer than its sources -- and runs the harness: the cases of tests/seq_insert_check.cpp on HipBackend, in a fresh process.  Every step has a
time limit of its own, the harness -- the only process that opens the GPU -- the shortest.  Exit status and output are the harness's; nothing is tried twice."""
import glob
import os
import re
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from test_seq_insert_routines import GOLDEN, verdict  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the harness: 25 small insertions; its limit is far above what they take and far below the parent's
T_HIPCC, T_HARNESS = 300, 60


def hipflags():
    for ln in open(os.path.join(ROOT, "Makefile")):
        m = re.match(r"HIPFLAGS\s*:?=\s*(.*)$", ln)
        if m:
            return m.group(1).split()
    raise RuntimeError("no HIPFLAGS in the Makefile")


def prebuilt():
    exe = os.path.join(ROOT, "oracle", "_build", "seq_insert_gpu")
    src = [os.path.join(ROOT, "tests", "seq_insert_gpu.hip"), os.path.join(ROOT, "tests", "seq_insert_cases.h"), os.path.join(ROOT, "oracle", "index_routines_cases.h")] + \
        glob.glob(os.path.join(ROOT, "star_amd", "csrc", "index", "*.h"))
    if os.path.isfile(exe) and os.access(exe, os.X_OK) and all(os.path.getmtime(exe) >= os.path.getmtime(s) for s in src):
        return exe
    return None


def main(work):
    t0 = time.time()
    harness = prebuilt()
    if harness is None:
        harness = os.path.join(work, "seq_insert_gpu")
        subprocess.check_call([HIPCC] + hipflags() + [os.path.join("tests", "seq_insert_gpu.hip"), "-o", harness], cwd=ROOT, timeout=T_HIPCC)
    t1 = time.time()
    try:
        p = subprocess.run([harness, GOLDEN], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=T_HARNESS)       # (on expiry the harness itself is killed)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        sys.stdout.write(out[-4000:])
        sys.stderr.write("the harness did not end within %d s and was killed\n" % T_HARNESS)
        return 5
    sys.stdout.write(p.stdout[-20000:])
    print("hipcc %.1f s, harness %.1f s" % (t1 - t0, time.time() - t1))
    bad = verdict(p.stdout, p.returncode)
    if bad:
        sys.stderr.write(bad + "\n")
        return p.returncode or 4
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
