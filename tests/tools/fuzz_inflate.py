#!/usr/bin/env python3
"""Bug hunt for k_inflate.hip: random BGZF files -- a random list of segments (lengths including 0, 1, 0xff00 and 65536; content from a menu: random bytes,
few-letter text, periodic data, runs, BAM-like records, and mixtures), each segment a member written by a writer drawn at random: zlib at level 0..9 with
the strategies default / filtered / Huffman only / RLE / fixed, with sync and full flushes at random places (several blocks, empty stored blocks off the
byte boundary), or the bit writer of tests/inflate_vectors.py with random tokens under the fixed code.  The device's bytes must be zlib's.  One call
in four is then damaged (a flipped bit, a cut, a stray byte) and must end with a status, or with the bytes zlib reads from the same members.
usage (on a machine with an MI355X): python tests/tools/fuzz_inflate.py [iterations] [seed]
On a machine WITHOUT a GPU:  FUZZ_EMUL=1 python tests/tools/fuzz_inflate.py [iterations] [seed]     the same through the wave emulator's build of the kernel
(run tests/test_inflate_bounds.py first: it is the gate for damaged input).  Ends at the first failure and leaves the file in fuzz_inflate_fail_<seed>_<iteration>.bin."""
import os
import random
import sys
import traceback
import zlib

EMUL = os.environ.get("FUZZ_EMUL") == "1"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
from util import capi                      # noqa: E402
import inflate_vectors as V                # noqa: E402


def content(r, n):
    kind = r.randrange(6)
    if kind == 0:
        return bytes(r.randrange(256) for _ in range(n))
    if kind == 1:
        return bytes(r.choice(b"ACGT\n") for _ in range(n))
    if kind == 2:
        p = bytes(r.randrange(256) for _ in range(r.randrange(1, 40)))
        return (p * (n // len(p) + 1))[:n]
    if kind == 3:
        out = bytearray()
        while len(out) < n:
            out += bytes([r.randrange(256)]) * r.randrange(1, 600)
        return bytes(out[:n])
    if kind == 4:
        return V.record_stream(n, r.randrange(1 << 30))
    a = content(r, n // 2)
    return a + content(r, n - len(a))


def token_member(r, n):
    """about n bytes from random tokens under the fixed code: literals and matches of every length and of every distance that is in reach"""
    toks, out = [], bytearray()
    while len(out) < n:
        if out and r.randrange(3):
            L = r.choice([3, 4, 10, 11, 64, 65, 130, 257, 258, r.randrange(3, 259)])
            D = r.choice([1, 2, len(out), r.randrange(1, len(out) + 1)])
            D = min(D, len(out), 32768)
            toks.append((L, D))
            for _ in range(L):
                out.append(out[-D])
        else:
            b = r.randrange(256)
            toks.append(b); out.append(b)
        if len(out) > 65536:
            return token_member(r, n // 2)
    bw = V.BitW()
    V.fixed(bw, toks, 1)
    return bw.bytes(), bytes(out)


def write_member(r, data):
    if data and r.randrange(5) == 0:
        d, data = token_member(r, len(data))
        if len(d) <= 65536 - 26:
            return V.member(d, data), data
        data = data[:1000]
    level = r.randrange(10)
    z = zlib.compressobj(level, zlib.DEFLATED, -15, r.randrange(1, 10), r.choice([zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED]))
    cuts = sorted(r.randrange(len(data) + 1) for _ in range(r.choice([0, 0, 1, 3])))
    d, at = b"", 0
    for c in cuts:
        d += z.compress(data[at:c]) + z.flush(r.choice([zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH]))
        at = c
    d += z.compress(data[at:]) + z.flush()
    if len(d) > 65536 - 26:                 # (random bytes with flushes can outgrow a member: store them in two)
        half = len(data) // 2
        a, da = write_member(r, data[:half])
        b, db = write_member(r, data[half:])
        return a + b, da + db
    return V.member(d, data), data


def fuzz_file(r):
    members, datas = [], []
    for _ in range(r.choice([1, 2, 5, 9, 30])):
        n = r.choice([0, 1, 2, 100, 5000, 0xff00, 65536, r.randrange(70000) % 65537])
        m, data = write_member(r, content(r, n))
        members.append(m); datas.append(data)
    if r.randrange(2):
        members.append(V.EOF_MARKER)
    return b"".join(members), b"".join(datas)


def zlib_reads(f):
    """what zlib makes of the members of f, or None where it rejects one (or the BSIZE chain cannot be walked)"""
    try:
        out = b""
        for d, crc, isize in V.members_of(f):
            z = zlib.decompressobj(-15)
            got = z.decompress(d)
            if not z.eof or z.unused_data or zlib.crc32(got) != crc or len(got) != isize:
                return None
            out += got
        return out
    except Exception:  # noqa: BLE001
        return None


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    if EMUL:
        import test_inflate_emul as E
        dev = capi.InflateDevice(lib_path=E.emul_lib())
    else:
        dev = capi.InflateDevice(device=0)
    rng = random.Random(seed)
    n_members = n_bytes = n_damaged = n_rejected = 0
    for it in range(iters):
        r = random.Random(rng.randrange(1 << 62))
        f, want = fuzz_file(r)
        try:
            out, failed, status, n, stats = dev.host_file(f)
            assert (failed, status) == (-1, "OK") and out == want, (failed, status, len(out or b""), len(want))
            if r.randrange(4) == 0 and len(f) > 30:
                g = bytearray(f)
                kind = r.randrange(3)
                if kind == 0:
                    g[r.randrange(18, len(g))] ^= 1 << r.randrange(8)
                elif kind == 1:
                    g = g[:r.randrange(19, len(g))]
                else:
                    g.insert(r.randrange(18, len(g)), r.randrange(256))
                f = bytes(g)
                n_damaged += 1
                try:
                    out, failed, status, n, stats = dev.host_file(f)
                except RuntimeError as e:   # a damaged header: not BGZF any more
                    assert "--gpuBAMinflate Host" in str(e), str(e)
                    out, failed = None, 0
                if failed >= 0:
                    n_rejected += 1
                else:
                    assert out == zlib_reads(f), "accepted, but zlib does not read these members so"
        except Exception:  # noqa: BLE001  (any failure ends the hunt: nothing more is started on the GPU)
            path = os.path.abspath("fuzz_inflate_fail_%d_%d.bin" % (seed, it))
            open(path, "wb").write(f)
            traceback.print_exc()
            print("FAILED at iteration %d: the file is in %s" % (it, path))
            return 1
        n_members += n; n_bytes += len(want)
        if it % 20 == 19:
            print("  %d files, %d members, %.1f MB out: clean" % (it + 1, n_members, n_bytes / 1e6), flush=True)
    print("fuzz_inflate: %d files, %d members, %.1f MB, %d damaged (%d rejected), seed %d, %s: 0 failures" % (iters, n_members, n_bytes / 1e6, n_damaged, n_rejected, seed, "emulator" if EMUL else "GPU"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
