#!/usr/bin/env python3
"""Bug hunt for k_bgzf.hip: random segment lists (count, lengths including 0 and exact multiples of 0xff00, content from a menu: random bytes, few-letter
text, periodic data, runs, BAM-like records, and mixtures spliced at random offsets) x compression level -1..9, every member held to every property
of tests/test_bgzf_streams.py (framing, CRC, round trip, Huffman optimum, the form chosen, the parse rule, the bound).
usage (on a machine with an MI355X): python tests/tools/fuzz_bgzf.py [iterations] [seed]        one process, one compressor on GPU 0
On a machine WITHOUT a GPU:  FUZZ_EMUL=1 python tests/tools/fuzz_bgzf.py [iterations] [seed]     the same through the wave emulator's build of the kernel
The generator is tests/test_bgzf_emul.py::fuzz_call, so that a call found here can be replayed there as a named vector (fuzz_replay).  Ends at the
first failure and leaves the failing call in fuzz_bgzf_fail_<seed>_<iteration>.pkl (level, segments)."""
import os
import pickle
import random
import sys
import traceback

EMUL = os.environ.get("FUZZ_EMUL") == "1"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
from util import capi                      # noqa: E402
import test_bgzf_emul as E                 # noqa: E402
import test_bgzf_streams as S              # noqa: E402

IN_MAX = E.IN_MAX


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    bz = capi.BgzfDevice(lib_path=E.emul_lib()) if EMUL else capi.BgzfDevice(device=0)
    rng = random.Random(seed)
    reach, nblocks, nbytes = set(), 0, 0
    try:
        for it in range(iters):
            r = random.Random(rng.randrange(1 << 62))
            level, segs = E.fuzz_call(r)
            try:
                outs = bz.compress(level, segs)
                reach |= S.check_call(bz, level, segs, outs, parse=True)
            except Exception:              # noqa: BLE001  (any failure ends the hunt: nothing more is started on the GPU)
                path = os.path.abspath("fuzz_bgzf_fail_%d_%d.pkl" % (seed, it))
                pickle.dump({"level": level, "segments": segs}, open(path, "wb"))
                traceback.print_exc()
                print("FAILED at iteration %d (level %d, %d segments of %s bytes): the call is in %s" % (it, level, len(segs), [len(s) for s in segs], path))
                return 1
            nblocks += sum(-(-len(s) // IN_MAX) for s in segs)
            nbytes += sum(len(s) for s in segs)
            if it % 20 == 19:
                print("  %d calls, %d blocks, %.1f MB: clean" % (it + 1, nblocks, nbytes / 1e6), flush=True)
    finally:
        bz.close()
    print("fuzz_bgzf: %d calls, %d blocks, %.1f MB, seed %d, %s: 0 failures" % (iters, nblocks, nbytes / 1e6, seed, "emulator" if EMUL else "GPU"))
    print("reached: " + ", ".join(sorted(reach)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
