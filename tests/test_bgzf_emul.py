"""k_bgzf.hip (BGZF compression on the device, include/star_amd_bgzf.h) compiled for the host by the wave emulator (oracle/wave_emul): every member
is a valid gzip member (BSIZE, CRC32, ISIZE), the blocks are cut as the host path cuts them (0xff00 input bytes), the content round-trips, the bytes
do not depend on the order the lanes run in, and on BAM record streams levels 1, 6 and -1 stay within 1.15 x of host zlib at the same level.  The GPU
tests (tests/test_gpu_bgzf.py) hold the shipped library to the bytes made here, so every vector of synthetic_vectors() runs on the MI355X too;
edge_vectors() are the ones built for a branch of the kernel each, and tests/test_bgzf_streams.py asserts that they reach it.
Emulator time of test_synthetic_vectors over all vectors: 10 - 13 s per level on one CPU core, 60 s for the six levels (it was 20 s for three) (three runs of every vector and one of all at once)."""
import gzip
import math
import os
import random
import struct
import threading
import time
import zlib

import pytest

from util import _map, bam_parts, capi, emul_units_lib, oracle_lib, prepare, refstar, run_with_engine
import test_golden

IN_MAX = 0xff00
LEVELS = (0, 1, 2, 6, 9, -1)       # one level per row of the kernel's table and both ends: 3 is 2 again; 4, 5, 7, 8, 9 and -1 are 6 again
EOF_MARK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
_EDGE = {}


def emul_lib():
    """the library of the emulated device units (util.emul_units_lib: built once per process)"""
    return emul_units_lib()


def synthetic_vectors():
    r = random.Random(20261015)
    text = b"".join(b"read%06d\tACGT%s\t%d\n" % (i, bytes(r.choice(b"ACGT") for _ in range(r.randint(5, 40))), r.randint(0, 1 << 20)) for i in range(12000))
    return {
        "empty": [b""],
        "one_byte": [b"\x2a"],
        "exactly_ff00": [text[:IN_MAX]],
        "ff01": [text[:IN_MAX + 1]],
        "random_200k": [bytes(r.getrandbits(8) for _ in range(200000))],
        "zeros_1M": [bytes(1 << 20)],
        "several": [text[:1000], b"", bytes(70000), text[5000:200000], b"x", bytes(r.getrandbits(8) for _ in range(3000))],
        **edge_vectors(),
    }


SWEEP = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, IN_MAX - 1)
THRESHOLD_TAILS = tuple(range(64, 136, 3))


def _words(r, n, alphabet, pool, lo=3, hi=9):
    """n bytes of words drawn from a pool of `pool` random words over `alphabet`, separated by blanks"""
    ws = [bytes(r.choice(alphabet) for _ in range(r.randint(lo, hi))) for _ in range(pool)]
    out = bytearray()
    while len(out) < n:
        out += r.choice(ws) + b" "
    return bytes(out[:n])


def _planted(seed):
    """uniform random bytes with copies of earlier stretches planted on whole lane slices, 64..600 bytes after their source: flat literals (the fixed
    code is as good as any) and just enough matches to beat stored.  The seeds kept below are the ones on which the fixed form wins with matches in
    it (found with tests/test_bgzf_streams.py's restatement of the parse; test_reach fails if they stop doing it)."""
    r = random.Random(seed)
    n, k, nrep = r.randint(600, 3000), r.choice([144, 200, 256]), r.randint(10, 120)
    d = bytearray(r.randrange(k) for _ in range(n))
    sl = -(-n // 256)
    for _ in range(nrep):
        p = r.randrange(200, n - sl) // sl * sl
        q = r.randrange(max(0, p - 600), p - 64)
        d[p:p + sl] = d[q:q + sl]
    return bytes(d)


def _de_bruijn(k, order):
    """the lexicographically least de Bruijn sequence B(k, order) over 0..k-1 (Fredricksen-Kessler-Maiorana): every `order`-gram once, cyclically"""
    a, seq = [0] * (k * order), []

    def db(t, p):
        if t > order:
            if order % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return seq


def _skewed_without_matches(seed, k, chunk):
    """A Fibonacci multiset of k byte values (46366 bytes for k = 22) laid out greedily: at every position the most frequent value left (jittered) that
    gives the 4-gram ending there no usable match candidate -- the kernel's hash, the heads of the chunks before -- so that as many of the frequent
    values as possible stay literals and the literal/length code gets deep.  The deepest found this way is 15 bits (seed 1010: half the positions
    had no such value), which is the limit, not beyond it: see DESIGN 7.3."""
    r = random.Random(seed)
    vals, fib = r.sample(range(256), k), [1, 1]
    while len(fib) < k:
        fib.append(fib[-1] + fib[-2])
    left = dict(zip(vals, fib))
    left[vals[0]] -= 1                                          # the end-of-block symbol is one of the two ones
    n = sum(left.values())
    sl, d, head = -(-n // 256), bytearray(), {}
    h4 = lambda g: ((int.from_bytes(g, "little") * 0x9E3779B1) & 0xffffffff) >> 20
    for p in range(n):
        if p and p % chunk == 0:
            for q in range(p - chunk, p - 3):
                head[h4(d[q:q + 4])] = q
        opts = sorted((v for v in left if left[v]), key=lambda v: -left[v] * (0.7 + 0.6 * r.random()))
        pick, s = None, p - 3
        for v in opts:
            if s >= 0 and min(n, (s // sl + 1) * sl) - s >= 3:
                q = head.get(h4(bytes(d[s:p]) + bytes([v])))
                if q is not None and q < s // chunk * chunk and d[q:q + 3] == d[s:s + 3]:
                    continue
            pick = v
            break
        if pick is None:
            pick = opts[0]
        d.append(pick)
        left[pick] -= 1
    return bytes(d)


def fuzz_content(r, n):
    """n bytes from the menu of tests/tools/fuzz_bgzf.py"""
    kind = r.randrange(7)
    if kind == 0:
        return bytes(r.getrandbits(8) for _ in range(n))
    if kind == 1:                                                  # few-letter text
        a = bytes(r.sample(range(256), r.randint(1, 6)))
        return bytes(r.choice(a) for _ in range(n))
    if kind == 2:                                                  # periodic
        per = bytes(r.getrandbits(8) for _ in range(r.choice([1, 2, 3, 4, 5, 7, 31, 32, 33, 64, 97, 255, 256, 257, 1000, 32767, 32768, 32769])))
        return (per * (n // len(per) + 1))[:n]
    if kind == 3:                                                  # runs
        out = bytearray()
        while len(out) < n:
            out += bytes([r.getrandbits(8)]) * r.choice([1, 2, 3, 4, 5, 10, 100, 254, 255, 256, 257, 258, 259, 300, 1000, 5000])
        return bytes(out[:n])
    if kind == 4:                                                  # BAM-like records
        out = bytearray()
        i = r.randrange(1 << 20)
        while len(out) < n:
            l = r.choice([50, 76, 101, 150])
            name = b"read%08d\0" % i
            seq = bytes(r.getrandbits(8) & 0x77 | 0x11 for _ in range((l + 1) // 2))
            qual = bytes(r.choice(b"\x02\x0b\x19\x25\x28") for _ in range(l))
            rec = struct.pack("<iiBBHHHIiii", r.randrange(25), r.randrange(1 << 27), len(name), r.choice([0, 1, 3, 255]), 4681, 1, r.choice([99, 147, 83, 163, 77, 141]), l, r.randrange(25),
                              r.randrange(1 << 27), r.randrange(-500, 500)) + name + struct.pack("<I", l << 4) + seq + qual + b"NHC\x01HIC\x01ASC" + bytes([r.randrange(50, 200)]) + b"nMC\0"
            out += struct.pack("<I", len(rec)) + rec
            i += 1
        return bytes(out[:n])
    if kind == 5:                                                  # words from a pool
        return _words(r, n, bytes(r.sample(range(256), r.randint(2, 200))), r.randint(2, 400), 1, r.randint(2, 40))
    out = bytearray(fuzz_content(r, n))                                 # a mixture: pieces of other contents spliced in at random offsets
    for _ in range(r.randint(1, 8)):
        if n < 2:
            break
        a = r.randrange(n)
        piece = fuzz_content(r, r.randint(1, n - a))
        out[a:a + len(piece)] = piece
    return bytes(out[:n])


def fuzz_length(r):
    k = r.randrange(10)
    if k == 0:
        return r.choice([0, 1, 2, 3, 4, 5])
    if k == 1:
        return r.choice([1, 2, 3]) * IN_MAX + r.choice([-1, 0, 0, 1])
    if k == 2:
        return r.choice([255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025])
    if k < 6:
        return r.randint(6, 3000)
    if k < 9:
        return r.randint(3000, IN_MAX)
    return r.randint(IN_MAX, 3 * IN_MAX)


def fuzz_call(r):
    """(level, segments) of one call of tests/tools/fuzz_bgzf.py"""
    level = r.randint(-1, 9)
    return level, [fuzz_content(r, fuzz_length(r)) for _ in range(r.choice([1, 1, 1, 2, 3, 5, 8]))]


def fuzz_replay(seed, it):
    """call number `it` of `fuzz_bgzf.py N seed`"""
    rng = random.Random(seed)
    for _ in range(it):
        rng.randrange(1 << 62)
    return fuzz_call(random.Random(rng.randrange(1 << 62)))


def edge_vectors():
    """the vectors of tests/test_bgzf_streams.py::MUST_REACH: each is there for a branch of the kernel that the ones above do not reach"""
    if _EDGE:
        return dict(_EDGE)
    r = random.Random(20261016)
    rep = _words(r, IN_MAX, b"ACGTNacgt=\t:0123456789", 60)
    v = {"length_sweep": [rep[:n] for n in SWEEP]}             # ragged last slices, empty lanes, blocks too short for a 4-byte hash
    a = bytes(r.getrandbits(8) for _ in range(600))
    for gap in (32767, 32768, 32769):                           # the second `a` finds the first exactly `gap` back: the last distance deflate has, and one more
        v["gap_%d" % gap] = [a + bytes(r.choice(b"ab") for _ in range(gap - 600)) + a + bytes(r.choice(b"ab") for _ in range(400))]
    v["fixed_with_matches"] = [_planted(5199), _planted(5308)]
    perm = list(range(30, 127)); r.shuffle(perm)
    v["one_distance"] = [bytes(perm) * 31]                      # period 97 >= chunk, no repeat inside a period: every match is 97 back, one distance code + a dummy
    v["no_match"] = [bytes(b"etaoin"[x] for x in _de_bruijn(6, 4)) + b"eta"]     # 1299 bytes, every 4-gram once: no match, two dummy distance codes
    v["two_values"] = [bytes(r.choice(b"\x00\xff") for _ in range(5000))]          # lengths: 254 zeros in a row between the two literals -> 18 with 138
    v["all_values"] = [bytes(r.sample(range(256), 256)) * 40]           # every byte value equally often -> repeats (16) of one length
    r2 = random.Random(1011)                                    # a seed on which the code-length code comes out deeper than 7 bits: the fold runs
    n, k, pool = r2.randint(600, 3000), r2.randint(90, 144), r2.randint(20, 300)
    v["cl_fold"] = [_words(r2, n, bytes(r2.sample(range(144), k)), pool)]
    v["depth_15"] = [_skewed_without_matches(1010, 22, 64)]     # level 1: a literal/length code of exactly 15 bits, HCLEN 19
    # found by tests/tools/fuzz_bgzf.py's generator: mixtures whose literal/length tree is 16 deep at levels 1 and 6 (fuzz_bgzf.py N 4, call 117) and
    # 17 deep at the lazy levels (N 6, call 154) -- some 200 byte values near 70 each over a ladder of rare ones: the fold to 15 bits runs
    v["fold_15"] = [fuzz_replay(4, 117)[1][1][:IN_MAX], fuzz_replay(6, 154)[1][3][2 * IN_MAX:3 * IN_MAX]]
    head = bytes(r.getrandbits(8) for _ in range(2000))
    v["stored_threshold"] = [head + (b"ACGTACGGTCA" * 13)[:t] for t in THRESHOLD_TAILS]    # the Huffman form crosses n + 5 bytes inside the sweep
    _EDGE.update(v)
    return v


def bam_stream(info, d, tag):
    """the decompressed content of an Aligned.out.bam made by the oracle engine (--outBAMcompression 0)"""
    info = dict(info)
    info["extra"] = list(info.get("extra", [])) + ["--outSAMtype", "BAM", "Unsorted", "--outBAMcompression", "0", "--outSAMattributes", "All"]
    p = run_with_engine(info, os.path.join(d, tag + "_"), lambda g, p: oracle_lib.Oracle(g, p), batch_reads=700)
    return gzip.open(p + "Aligned.out.bam", "rb").read()


def host_sizes(seg, level):
    """member sizes of the host path (star_amd/csrc/host/bgzf.cpp: raw deflate of zlib, memLevel 8, default strategy)"""
    out = []
    for o in range(0, len(seg), IN_MAX):
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY)
        out.append(18 + len(co.compress(seg[o:o + IN_MAX]) + co.flush()) + 8)
    return out


def members(blob):
    """(content, BTYPE of the first deflate block) of every member; asserts the BGZF framing"""
    p, res = 0, []
    while p < len(blob):
        assert blob[p:p + 16] == bytes.fromhex("1f8b08040000000000ff060042430200"), blob[p:p + 16]
        bsize = struct.unpack("<H", blob[p + 16:p + 18])[0] + 1
        m = blob[p:p + bsize]
        assert len(m) == bsize and bsize <= 65536
        d = zlib.decompressobj(-15)
        data = d.decompress(m[18:-8])
        assert d.eof and d.unused_data == b""
        crc, isize = struct.unpack("<II", m[-8:])
        assert crc == zlib.crc32(data) and isize == len(data)
        assert gzip.decompress(m) == data
        res.append((data, (m[18] >> 1) & 3))
        p += bsize
    return res


def check(segs, outs, level):
    assert len(outs) == len(segs)
    for seg, out in zip(segs, outs):
        ms = members(out)
        assert [len(x) for x, _ in ms] == [min(IN_MAX, len(seg) - o) for o in range(0, len(seg), IN_MAX)]       # the host's split
        assert b"".join(x for x, _ in ms) == seg
        if level == 0:
            assert all(t == 0 for _, t in ms)


def compress_desc(bz, level, segs):
    """the same call with the emulated lanes in descending order (STARAMD_EMUL_ORDER is read by the first launch on a thread)"""
    res = {}
    old = os.environ.get("STARAMD_EMUL_ORDER")
    os.environ["STARAMD_EMUL_ORDER"] = "desc"
    try:
        t = threading.Thread(target=lambda: res.setdefault("out", bz.compress(level, segs)))
        t.start()
        t.join()
    finally:
        if old is None:
            del os.environ["STARAMD_EMUL_ORDER"]
        else:
            os.environ["STARAMD_EMUL_ORDER"] = old
    return res["out"]


@pytest.fixture(scope="module")
def bz():
    b = capi.BgzfDevice(lib_path=emul_lib())
    yield b
    b.close()


def _run_checked(bz, level, segs):
    outs = bz.compress(level, segs)
    check(segs, outs, level)
    assert bz.compress(level, segs) == outs
    assert compress_desc(bz, level, segs) == outs
    return outs


@pytest.mark.parametrize("level", LEVELS)
def test_synthetic_vectors(bz, level):
    for name, segs in synthetic_vectors().items():
        outs = _run_checked(bz, level, segs)
        if name == "random_200k":
            assert all(t == 0 for _, t in members(outs[0])), "incompressible blocks must be stored"
        if name == "empty":
            assert outs == [b""]
    allsegs = [s for segs in synthetic_vectors().values() for s in segs]     # every vector in one call
    check(allsegs, bz.compress(level, allsegs), level)


def test_stored_threshold_crossing(bz):
    """random bytes with a compressible tail that grows: short tails are stored, long ones are not, and each member is on the right side of n + 5
    bytes (what the Huffman form would have cost is recomputed in tests/test_bgzf_streams.py)"""
    segs = synthetic_vectors()["stored_threshold"]
    for level in (1, 2, 6):
        types = [members(o)[0][1] for o in bz.compress(level, segs)]
        assert types[0] == 0 and types[-1] == 2, (level, types)


def many_contents():
    """blocks of different kinds for many_calls: stored, dynamic text, zeros, fixed form with matches, one byte, the distance-32768 block, a folded
    code-length code"""
    v = synthetic_vectors()
    c = [v["random_200k"][0][:IN_MAX], v["exactly_ff00"][0], bytes(IN_MAX), v["fixed_with_matches"][0], b"\x2a", v["gap_32768"][0], v["cl_fold"][0]]
    assert all(0 < len(x) <= IN_MAX for x in c)
    return c


def many_calls(bz, grid, levels=(1, 6, 0)):
    """One call of 3 * grid + 5 blocks on a compressor that launches `grid` workgroups, so that every workgroup goes round its block loop three or
    four times and meets a different kind of block each time; before and after it the same contents one per call (the first trip of workgroup 0,
    nothing left over to see; and small -> large -> small on one handle, through the buffers' grow paths)."""
    c = many_contents()
    assert math.gcd(len(c), grid) == 1, (len(c), grid)
    nb = 3 * grid + 5
    segs = [c[i % len(c)] for i in range(nb)]
    res = {"grid": grid, "nb": nb, "bytes": sum(len(x) for x in segs)}
    for lv in levels:
        alone = [bz.compress(lv, [x])[0] for x in c]
        t0 = time.time()
        many = bz.compress(lv, segs)
        res[lv] = (alone, many, [bz.compress(lv, [x])[0] for x in c], time.time() - t0)
    return res


def check_many(res):
    c = many_contents()
    segs = [c[i % len(c)] for i in range(res["nb"])]
    assert res["nb"] >= 3 * res["grid"] + 5
    for lv in (1, 6, 0):
        alone, many, again, _ = res[lv]
        check(c, alone, lv)
        assert again == alone, lv
        assert len(many) == res["nb"]
        for i, m in enumerate(many):
            assert m == alone[i % len(c)], "level %d, block %d (kind %d, trip %d of workgroup %d)" % (lv, i, i % len(c), i // res["grid"], i % res["grid"])
        check(segs, many, lv)
    if {members(x)[0][1] for x in res[1][0]} != {0, 1, 2}:
        raise AssertionError("the contents no longer cover stored, fixed and dynamic")


def test_more_blocks_than_workgroups_emulated():
    """tests/test_gpu_bgzf.py::test_more_blocks_than_workgroups on the emulator, which launches 2 x 2 workgroups"""
    b = capi.BgzfDevice(lib_path=emul_lib())
    try:
        res = many_calls(b, 4)
    finally:
        b.close()
    assert res["nb"] == 17
    check_many(res)


def test_level_out_of_range(bz):
    with pytest.raises(RuntimeError, match="not in -1..9"):
        bz.compress(10, [b"abc"])


def _bam_case(bz, stream):
    for level in LEVELS:
        outs = _run_checked(bz, level, [stream])
        if level in (1, 6, -1):                                  # DESIGN 7.3 "Size against zlib": the cap holds against zlib at the same level
            dev, host = len(outs[0]), sum(host_sizes(stream, level))
            print("level %d: %d bytes, zlib %d, %.3f x" % (level, dev, host, dev / host))
            assert dev <= 1.15 * host, (level, dev, host, dev / host)


def test_bam_stream_tiny(bz, tmp_path, built):
    _bam_case(bz, bam_stream(test_golden._tiny_info(), str(tmp_path), "tiny"))


@pytest.mark.skipif(not refstar.have_ref(), reason="oracle/_ref/STAR not built (no /root/reference here)")
@pytest.mark.parametrize("name", ["pe150_indel", "pe150_chim"])
def test_bam_stream(bz, name, tmp_path, built):
    info = prepare(name, str(tmp_path), need_ref=False)
    _bam_case(bz, bam_stream(info, str(tmp_path), name))


def same_bam(a, b):
    """same records, same reference block, same header text but for the command line (@PG / @CO)"""
    (ta, ra, rr), (tb, rb, nr) = bam_parts(a), bam_parts(b)
    keep = lambda t: [l for l in t.split(b"\n") if not l.startswith((b"@PG", b"@CO"))]
    return ra == rb and rr == nr and keep(ta) == keep(tb)


def run_with_bgzf(info, prefix, engine_factory, bz, batch_reads=777):
    """util.run_with_engine with `bz` (a BgzfDevice, or None) installed as the run's BGZF compressor (HostRun.set_bgzf_device)"""
    argv = ["--genomeDir", info["idx"], "--readFilesIn"] + info["fastq"] + ["--outFileNamePrefix", prefix] + list(info.get("extra", []))
    run = capi.HostRun(argv)
    eng = engine_factory(run.genome, run.params)
    try:
        if bz is not None:
            run.set_bgzf_device(bz)
        while True:
            while True:
                b = run.next_batch(batch_reads)
                if b is None:
                    break
                run.emit(_map(eng, b).res)
            phase = run.next_phase()
            if phase == 0:
                break
            if phase == 1:
                eng.update_index(run.genome, run.params)
            else:
                eng.set_novel_junctions(*run.novel_junctions())
        run.finish()
    finally:
        eng.close()
        run.close()
    return prefix


@pytest.mark.parametrize("types", [["Unsorted"], ["Unsorted", "SortedByCoordinate"]])
def test_host_run_device_mode_emulated(bz, types, tmp_path, built):
    """--gpuBAMcompression Device through the hook, the emulated compressor behind it: the decompressed files equal the Host run's"""
    _device_mode_case(bz, test_golden._tiny_info(), types, tmp_path)


@pytest.mark.skipif(not refstar.have_ref(), reason="oracle/_ref/STAR not built (no /root/reference here)")
def test_host_run_device_mode_emulated_sorted_only_records(bz, tmp_path, built):
    """KeepPairs with both BAM files on reads that have one-mate alignments (the data of test_host_flags.test_keep_pairs: the 2nd mate of every 3rd pair
    is junk): the sorted file gets records that the unsorted one does not, and the device path has to be handed the unsorted file's records without them"""
    import test_host_flags
    info = test_host_flags._multicopy(tmp_path, seed=22)
    lines = open(info["fastq"][1]).read().split("\n")
    for i in range(0, len(lines) // 4, 3):
        lines[4 * i + 1] = ("ACGTTGCATGCCGATATCGGCTAGCTAGGATCCGATTTAGGCTCTAGAGCTCGATCGGGATATCCGCGATATTAGCAGCTACGACTAGCATCGACTAGC" * 3)[i % 7:i % 7 + len(lines[4 * i + 1])]
    junk = str(tmp_path / "junk_2.fq")
    open(junk, "w").write("\n".join(lines))
    info["fastq"] = [info["fastq"][0], junk]
    info["extra"] = ["--outFilterMultimapNmax", "50", "--outFilterMultimapScoreRange", "4", "--outFilterScoreMinOverLread", "0.3", "--outFilterMatchNminOverLread", "0.3"]
    outs = _device_mode_case(bz, info, ["Unsorted", "SortedByCoordinate"], tmp_path)
    assert len(bam_parts(outs["Device"] + "Aligned.out.bam")[2]) != len(bam_parts(outs["Device"] + "Aligned.sortedByCoord.out.bam")[2])      # (the case does occur in these reads)


def _device_mode_case(bz, info0, types, tmp_path):
    outs = {}
    for mode in ("Host", "Device"):
        info = dict(info0)
        info["extra"] = list(info.get("extra", [])) + ["--outSAMtype", "BAM"] + types + ["--outSAMunmapped", "Within", "KeepPairs", "--runThreadN", "3", "--gpuBAMcompression", mode]
        outs[mode] = run_with_bgzf(info, str(tmp_path / mode) + "_", lambda g, p: oracle_lib.Oracle(g, p), bz if mode == "Device" else None, batch_reads=300)
    for f in ["Aligned.out.bam"] + (["Aligned.sortedByCoord.out.bam"] if "SortedByCoordinate" in types else []):
        h, d = open(outs["Host"] + f, "rb").read(), open(outs["Device"] + f, "rb").read()
        assert d[-28:] == EOF_MARK
        assert same_bam(outs["Device"] + f, outs["Host"] + f), f
        assert d != h, "the records were not compressed by the device path"
    return outs
