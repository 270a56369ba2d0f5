"""Child process of tests/test_gpu_window_routines.py: one GPU step, under the time limit the parent sets.
    window_routines_run.py <work dir>
builds the CPU check (host clang++ through the wavefront emulator's headers) and lets it write its case file (--dump: three environments and the four special ones, every class
present), builds tests/window_routines_gpu.hip for gfx950 with hipcc and the product's flags, and runs the harness over that file in a fresh process.  Every step has a time limit
of its own, the harness -- the only process that opens the GPU -- the shortest.  Exit status and output are the harness's; nothing is tried twice."""
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from test_window_routines import build_check, class_counts, compared_share, N_CLASSES  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# limits per step; their sum stays below the parent's (tests/test_gpu_window_routines.py: TIMEOUT); measured: 12 s, 25 s, 9 s, 0.6 s
T_CHECK_BUILD, T_DUMP, T_HIPCC, T_HARNESS = 90, 180, 180, 60


def main(work):
    check, cases, harness = os.path.join(work, "window_routines_check"), os.path.join(work, "cases.bin"), os.path.join(work, "window_routines_gpu")
    t0 = time.time()
    build_check(check, timeout=T_CHECK_BUILD)
    p = subprocess.run([check, "--dump", cases], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=T_DUMP)
    last = p.stdout.strip().splitlines()[-1] if p.stdout.strip() else ""
    counts, share = class_counts(p.stdout), compared_share(p.stdout)
    if p.returncode != 0 or not last.endswith(": 0 differences") or len(counts) != N_CLASSES or min(counts) == 0 or len(share) != 1 or share[0] < 0.95:
        sys.stderr.write("the CPU check fails while writing the case file (a difference, or a class of cases that is not in the file):\n" + p.stdout[-6000:])
        return 3
    t1 = time.time()
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-result", os.path.join("tests", "window_routines_gpu.hip"), "-o", harness], cwd=ROOT, timeout=T_HIPCC)
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
    last = p.stdout.strip().splitlines()[-1] if p.stdout.strip() else ""
    if p.returncode != 0 or not last.endswith(": 0 differences"):
        return p.returncode or 4
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
