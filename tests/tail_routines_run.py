"""Child process of tests/test_gpu_tail_routines.py: one GPU step, under the time limit the parent sets.
    tail_routines_run.py <work dir>
builds the CPU check (host clang++ through the wavefront emulator's headers) and lets it write its case file (--dump; the check itself must end with 0 differences, every class
present and every case compared), builds tests/tail_routines_gpu.hip for gfx950 with hipcc and the product's flags for k_stitch.hip, and runs the harness over that file in a fresh
process.  Every step has a time limit of its own, the harness -- the only process that opens the GPU -- the shortest.  Exit status and output are the harness's; nothing is tried
twice."""
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from test_tail_routines import build_check, class_counts, compared, N_CLASSES  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# limits per step; their sum stays below the parent's (tests/test_gpu_tail_routines.py: TIMEOUT); measured on the GPU machine: 3 s, 0.4 s, 2.7 s, 0.8 s (7 s, 0.5 s, 5 s without a GPU).
# The harness: ten times what it took, and no less than 20 s (the margin is for a loaded machine)
T_CHECK_BUILD, T_DUMP, T_HIPCC, T_HARNESS = 90, 180, 180, 20


def main(work):
    check, cases, harness = os.path.join(work, "tail_routines_check"), os.path.join(work, "cases.bin"), os.path.join(work, "tail_routines_gpu")
    t0 = time.time()
    build_check(check, timeout=T_CHECK_BUILD)
    p = subprocess.run([check, "--dump", cases], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=T_DUMP)
    last = p.stdout.strip().splitlines()[-1] if p.stdout.strip() else ""
    counts, done = class_counts(p.stdout), compared(p.stdout)
    if p.returncode != 0 or not last.endswith(": 0 differences") or len(counts) != N_CLASSES or min(counts) == 0 or len(done) != 1 or done[0][0] != done[0][1]:
        sys.stderr.write("the CPU check fails while writing the case file (a difference, a class of cases that is not in the file, or a case that was not compared):\n" + p.stdout[-6000:])
        return 3
    t1 = time.time()
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-result", os.path.join("tests", "tail_routines_gpu.hip"), "-o", harness], cwd=ROOT, timeout=T_HIPCC)
    t2 = time.time()
    try:
        p = subprocess.run([harness, cases], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=T_HARNESS)       # (on expiry the harness itself is killed)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        sys.stdout.write(out[-4000:])
        sys.stderr.write("the harness did not end within %d s and was killed\n" % T_HARNESS)
        return 5
    sys.stdout.write(p.stdout[-6000:])
    print("case file %.1f MB, rarest class %d cases; CPU check and dump %.1f s, hipcc %.1f s, harness %.1f s" % (os.path.getsize(cases) / 1e6, min(counts), t1 - t0, t2 - t1, time.time() - t2))
    lines = p.stdout.strip().splitlines()
    last = lines[-1] if lines else ""
    done = compared(p.stdout)
    if p.returncode != 0 or not last.endswith(": 0 differences") or len(done) != 1 or done[0][0] != done[0][1]:
        return p.returncode or 4
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
