"""Child process of tests/test_gpu_index_routines.py: one GPU step, under the time limit the parent sets.
    index_routines_run.py <work dir>
builds and runs the CPU check (oracle/index_routines_check.cpp on the plain-loop backend; it must end with 0 differences, every class present and every case
compared), builds tests/index_routines_gpu.hip for gfx950 with hipcc and the product's HIPFLAGS (read from the Makefile), and runs the harness -- the same cases
on HipBackend, plus forEach over 2^31 + 300 work-items -- in a fresh process.  Every step has a time limit of its own, the harness -- the only process that
opens the GPU -- the shortest.  Exit status and output are the harness's; nothing is tried twice."""
import os
import re
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from test_index_routines import build_check, class_counts, compared, N_CLASSES, FIXTURES  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# limits per step; their sum stays below the parent's (tests/test_gpu_index_routines.py: TIMEOUT).  Measured on the GPU machine: 5.5 s for both steps of the CPU check, 8.8 s, 3.5 s
# (forEach over 2^31 + 300 work-items alone: 1.8 ms).
# The harness: ten times what it took, and no less than 20 s (the margin is for a loaded machine)
T_CHECK_BUILD, T_CHECK, T_HIPCC, T_HARNESS = 90, 240, 240, 40


def hipflags():
    for ln in open(os.path.join(ROOT, "Makefile")):
        m = re.match(r"HIPFLAGS\s*:?=\s*(.*)$", ln)
        if m:
            return m.group(1).split()
    raise RuntimeError("no HIPFLAGS in the Makefile")


def main(work):
    check, harness = os.path.join(work, "index_routines_check"), os.path.join(work, "index_routines_gpu")
    t0 = time.time()
    build_check(check, timeout=T_CHECK_BUILD)
    p = subprocess.run([check, FIXTURES], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=T_CHECK)
    last = p.stdout.strip().splitlines()[-1] if p.stdout.strip() else ""
    counts, done = class_counts(p.stdout), compared(p.stdout)
    if p.returncode != 0 or not last.endswith(": 0 differences") or len(counts) != N_CLASSES or min(counts) == 0 or len(done) != 1 or done[0][0] != done[0][1]:
        sys.stderr.write("the CPU check fails (a difference, a class of cases that never occurred, or a case that was not compared):\n" + p.stdout[-6000:])
        return 3
    t1 = time.time()
    subprocess.check_call([HIPCC] + hipflags() + [os.path.join("tests", "index_routines_gpu.hip"), "-o", harness], cwd=ROOT, timeout=T_HIPCC)
    t2 = time.time()
    try:
        p = subprocess.run([harness, FIXTURES], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=T_HARNESS)       # (on expiry the harness itself is killed)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        sys.stdout.write(out[-4000:])
        sys.stderr.write("the harness did not end within %d s and was killed\n" % T_HARNESS)
        return 5
    sys.stdout.write(p.stdout[-20000:])
    print("CPU check %.1f s, hipcc %.1f s, harness %.1f s" % (t1 - t0, t2 - t1, time.time() - t2))
    lines = p.stdout.strip().splitlines()
    last = lines[-1] if lines else ""
    counts, done = class_counts(p.stdout), compared(p.stdout)
    if p.returncode != 0 or not last.endswith(": 0 differences") or len(counts) != N_CLASSES + 1 or min(counts) == 0 or len(done) != 1 or done[0][0] != done[0][1]:
        return p.returncode or 4
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
