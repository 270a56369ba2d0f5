"""k_signal.hip (--gpuSignal Device, include/star_amd_signal.h) compiled for the host by the wave emulator together with k_bamsort.hip and k_bgzf.hip:
the Signal.* files made from the device's runs are, byte for byte, those of the host path (writeSignal, pinned to the reference in tests/test_signal.py)
on the same fabricated BAM records -- through the host-records entry (the tool mode --runMode inputAlignmentsFromBAM --gpuSignal Device), through the
sorter (staramd_bamsort_finish_signal), and with the formatter alone.  Where oracle/_ref/STAR is built, its own inputAlignmentsFromBAM reads the same
fabricated BAM files.  The front end on the emulator is in tests/test_signal_frontend_emul.py; the GPU tests (tests/test_gpu_signal.py) run these vectors
through the shipped library."""
import os
import random
import struct
import subprocess
import tempfile
import zlib

import pytest

from util import capi, emul_units_lib, refstar
import test_bamsort_emul as S

T = 1024                        # positions per tile of k_signal_tiles
CH = 256                        # spans per LDS chunk
CHROMS = [("chrA", 700000), ("chrB", 3000), ("chrC", 5000), ("other1", 2000)]
CHR_NAMES = [c for c, _ in CHROMS]
CHR_LEN = [n for _, n in CHROMS]
BUG = "BUG: alignment extends past chromosome in the signal output"


def emul_lib():
    """the library of the emulated device units (util.emul_units_lib: built once per process)"""
    return emul_units_lib()


# ---- fabricated BAM ------------------------------------------------------------------------------------------------------------------------------

def nh_attr(nh, typ="C"):
    """the NH attribute with the given integer type; nh None = absent"""
    if nh is None:
        return b""
    return b"NH" + typ.encode() + struct.pack({"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[typ], nh)


def rec(tid, pos, cigar, flag=0, nh=1, typ="C", pre=b"", post=b"", name=b"r"):
    """one BAM record with its block_size word.  cigar: [(length, op letter)]; pre / post: attributes before / behind NH"""
    ops = b"".join(struct.pack("<I", n << 4 | "MIDNSHP=X".index(c)) for n, c in cigar)
    lseq = sum(n for n, c in cigar if c in "MIS=X")
    nm = name + b"\0"
    body = struct.pack("<iiIIiiii", tid, pos, len(nm), flag << 16 | len(cigar), lseq, -1, -1, 0) + nm + ops + b"\x11" * ((lseq + 1) // 2) + b"\x1e" * lseq
    body += pre + nh_attr(nh, typ) + post
    return struct.pack("<I", len(body)) + body


def key_of(r):
    tid, pos = struct.unpack("<ii", r[4:12])
    return ((1 << 64) - 1) if tid < 0 else (tid << 32 | pos)


def in_order(records):
    """coordinate order: by (tid, pos), unmapped last, ties in the given order"""
    return [records[i] for i in sorted(range(len(records)), key=lambda i: (key_of(records[i]), i))]


def bgzf(data):
    out = []
    for o in range(0, max(len(data), 1), 0xff00):
        chunk = data[o:o + 0xff00]
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        d = c.compress(chunk) + c.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(d) + 25) + d + struct.pack("<II", zlib.crc32(chunk), len(chunk)))
    return b"".join(out) + bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def write_bam(path, records, chroms=None):
    chroms = chroms or CHROMS
    text = b"@HD\tVN:1.4\tSO:coordinate\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (c.encode(), n) for c, n in chroms)
    head = b"BAM\1" + struct.pack("<I", len(text)) + text + struct.pack("<I", len(chroms))
    for c, n in chroms:
        head += struct.pack("<I", len(c) + 1) + c.encode() + b"\0" + struct.pack("<I", n)
    with open(path, "wb") as f:
        f.write(bgzf(head + b"".join(records)))
    return path


# ---- vectors -------------------------------------------------------------------------------------------------------------------------------------

def sum_order_nh():
    """NH of a stack of records on one position, drawn from {3, 5, 6, 7, 1}: the double sum of 1 / NH depends on the order"""
    r = random.Random(3)
    return [r.choice([3, 5, 6, 7, 1]) for _ in range(41)]


def _fsum(nhs):
    acc = 0.0
    for n in nhs:
        acc += 1.0 / n
    return acc


_VEC = {}


def vectors():
    """name -> records (bytes each) in coordinate order; the same for the emulator and, in tests/test_gpu_signal.py, the MI355X"""
    if _VEC:
        return _VEC
    r = random.Random(20261020)
    M = lambda n: [(n, "M")]
    v = _VEC
    v["empty"] = []
    # spans ending at T - 1, T, T + 1; one starting at T - 1; one M block over three tiles; an N that jumps ~488 tiles; two abutting spans of equal value across a boundary
    v["tile_edges"] = in_order([rec(0, T - 50, M(50)), rec(0, T - 49, M(50), nh=2), rec(0, T - 48, M(50), nh=3), rec(0, T - 1, M(30)),
                                rec(0, 3 * T + 500, M(2 * T + 100), nh=2), rec(0, 10 * T + 5, [(20, "M"), (500000, "N"), (20, "M")]),
                                rec(0, 20 * T - 10, M(10)), rec(0, 20 * T, M(10)), rec(0, 22 * T - 10, M(10)), rec(0, 22 * T, M(10), nh=2)])
    # more spans in one tile than one LDS chunk holds: CH - 1, CH and CH + 1 in tiles of their own, 2 * CH + 3 in a fourth
    recs = []
    for tile, k in ((30, CH - 1), (32, CH), (34, CH + 1), (36, 2 * CH + 3)):
        recs += [rec(0, tile * T + (i * 7) % 900, M(1 + i % 50), nh=r.choice([1, 1, 2, 3, 5, 7]), flag=r.choice([0, 16])) for i in range(k)]
    v["chunks"] = in_order(recs)
    v["sum_order"] = [rec(0, 40 * T + 7, M(5), nh=n) for n in sum_order_nh()]
    # NH in every integer type, behind a Z, an H and a B attribute, absent, 0, negative, of a non-integer type (reads as 0), in a record with an unknown type before it (absent)
    Z, H, B = b"XZZhello\0", b"XHH1AE3\0", b"XBBs" + struct.pack("<Ihhh", 3, 1, 2, 3)
    forms = [rec(1, 100 + 10 * i, M(40), nh=3, typ=t) for i, t in enumerate("cCsSiI")]
    forms += [rec(1, 200, M(40), nh=2, pre=Z), rec(1, 210, M(40), nh=5, pre=H), rec(1, 220, M(40), nh=7, pre=B), rec(1, 230, M(40), nh=6, pre=Z + H + B + b"ASC\x07", post=b"nMC\x01"),
              rec(1, 240, M(40), nh=None), rec(1, 250, M(40), nh=None, pre=Z), rec(1, 260, M(40), nh=0), rec(1, 270, M(40), nh=-1, typ="c"),
              rec(1, 280, M(40), nh=None, pre=b"NHA1"), rec(1, 290, M(40), nh=4, pre=b"XX?"), rec(1, 300, M(40), nh=300, typ="S"), rec(1, 310, M(40), nh=70000, typ="I")]
    v["nh_forms"] = in_order(forms)
    # duplicates, an unwanted reference (--outWigReferencesPrefix chr), a chromosome whose records are all duplicates (the wiggle header), unmapped records at the end
    v["skips_refs"] = in_order([rec(0, 500, M(30)), rec(0, 510, M(30), flag=0x400), rec(0, 520, M(30), nh=2, flag=0x410), rec(1, 50, M(20), nh=2),
                                rec(2, 100, M(50), flag=0x400), rec(2, 120, M(50), flag=0x400, nh=3), rec(3, 10, M(100)), rec(3, 40, M(100), nh=2),
                                rec(-1, -1, [], flag=4, nh=None), rec(-1, -1, [], flag=4, nh=0)])
    # the last base of a chromosome; the spare base behind it (no error: the reference's array has it)
    v["chr_end"] = in_order([rec(1, 3000 - 10, M(10)), rec(2, 5000 - 20, M(20), nh=2), rec(2, 5000 - 1, M(1))])
    v["spare_base"] = in_order([rec(1, 3000 - 9, M(10)), rec(2, 100, M(10))])
    v["past_end"] = in_order([rec(0, 100, M(10)), rec(1, 3000 - 8, M(10))])                         # reaches chrLength + 1
    # mates and strands: unpaired, mate 1 and mate 2, forward and reverse, with gaps, insertions and clips
    cig = [(5, "S"), (20, "M"), (2, "I"), (10, "M"), (3, "D"), (15, "M"), (1500, "N"), (25, "M"), (4, "S")]
    mates = []
    for i, fl in enumerate((0, 0x10, 0x41, 0x51, 0x81, 0x91, 0x43, 0x93, 0x63, 0xa3)):
        mates += [rec(0, 50 * T + 900 + 37 * i, cig, flag=fl, nh=1 + i % 3), rec(0, 60 * T + 11 * i, M(60), flag=fl, nh=1 + (i + 1) % 3)]
    v["mates"] = in_order(mates)
    v["no_nh"] = in_order([rec(0, 1000, M(30), nh=None), rec(0, 1010, M(30), nh=None, flag=0x10)])   # --outWigNorm RPM divides by 0 unique reads: inf
    v["no_unique"] = in_order([rec(0, 1000, M(30), nh=2), rec(0, 1010, M(30), nh=3, flag=0x10)])
    # a few thousand records over many tiles and two chromosomes, more tiles than the emulator's workgroups
    mix = [rec(0, r.randrange(100 * T, 160 * T), [(r.randint(1, 70), "M"), (r.choice([1, 90, 2500]), "N"), (r.randint(1, 70), "M")], flag=r.choice([0, 16, 0x43, 0x93, 0x400]),
               nh=r.choice([1, 1, 1, 2, 3, 4, 6, None])) for _ in range(3000)]
    mix += [rec(2, r.randrange(0, 4800), M(r.randint(1, 150)), flag=r.choice([0, 16]), nh=r.choice([1, 2, 7])) for _ in range(400)]
    v["mix"] = in_order(mix)
    return v


MANY_CHROMS = [("big", 3000000), ("small", 5000)]


def many_vector():
    """3 Mb of one chromosome under 60 000 records -- ~2850 occupied tiles, more than 8 workgroups on each of 256 CUs, deep stacks and empty stretches -- and
    20 000 spans in the five tiles of a second one: ~16 LDS chunks each.  For write_bam(path, records, MANY_CHROMS)"""
    r = random.Random(11)
    recs = [rec(0, min(r.randrange(0, 2990000), r.randrange(0, 2990000)), [(r.randint(1, 90), "M"), (r.choice([1, 200, 3000]), "N"), (r.randint(1, 90), "M")],
                flag=r.choice([0, 16, 0x43, 0x93]), nh=r.choice([1, 1, 1, 2, 3, 5, 6, 7])) for _ in range(60000)]
    recs += [rec(1, r.randrange(0, 4000), [(r.randint(1, 200), "M")], nh=r.choice([1, 3, 7])) for _ in range(20000)]
    return in_order(recs)


VECTOR_NAMES = ["empty", "tile_edges", "chunks", "sum_order", "nh_forms", "skips_refs", "chr_end", "spare_base", "past_end", "mates", "no_nh", "no_unique", "mix"]
REF_SAFE = ["empty", "tile_edges", "chunks", "sum_order", "skips_refs", "chr_end", "mates", "no_unique", "mix"]     # what a BAM reader other than ours is sure to take

FORMATS = {"bg": ["bedGraph"], "wig": ["wiggle"]}
BASIC = [(f, s, n, 0) for f in ("bg", "wig") for s in (1, 0) for n in (1, 0)]


def options(name):
    """(format, stranded, norm, type) combinations of a vector: every format x strand x norm at type 0; the types where mates matter"""
    opts = list(BASIC)
    if name in ("mates", "mix"):
        opts += [(f, s, n, t) for t in (1, 2) for f in ("bg", "wig") for s in (1, 0) for n in (1, 0)]
    elif name in ("tile_edges", "chr_end", "past_end", "skips_refs"):
        opts += [("bg", 1, 0, 1), ("wig", 0, 1, 2)]
    return opts


def wig_flags(fmt, strand, norm, typ, prefix=None):
    fl = ["--outWigType"] + FORMATS[fmt] + ([["read1_5p"], ["read2"]][typ - 1] if typ else [])
    fl += ["--outWigStrand", "Stranded" if strand else "Unstranded", "--outWigNorm", "RPM" if norm else "None"]
    return fl + (["--outWigReferencesPrefix", prefix] if prefix else [])


def flag_tag(flags):
    """a file-name part that tells option combinations apart (every run gets files of its own)"""
    return "".join(x[:2] if not x.startswith("--") else "" for x in flags)


def signal_files(prefix):
    d, b = os.path.dirname(prefix), os.path.basename(prefix)
    return {f[len(b):]: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.startswith(b + "Signal.")}


def tool_mode(bam, prefix, flags, device=False):
    """--runMode inputAlignmentsFromBAM in this process (everything happens in sah_create): the Signal.* files, or the error text"""
    try:
        capi.HostRun(["--runMode", "inputAlignmentsFromBAM", "--inputBAMfile", bam, "--outFileNamePrefix", prefix] + flags + (["--gpuSignal", "Device"] if device else [])).close()
    except RuntimeError as e:
        return str(e)
    return signal_files(prefix)


def host_expected(workdir, name, flags, tag="h"):
    """the host path (writeSignal) on a vector"""
    bam = os.path.join(workdir, name + ".bam")
    if not os.path.exists(bam):
        write_bam(bam, vectors()[name])
    return tool_mode(bam, os.path.join(workdir, "%s_%s%s_" % (name, tag, flag_tag(flags))), flags)


@pytest.fixture(scope="module")
def sg(built):
    s = capi.SignalDevice(lib_path=emul_lib())
    s.install()
    yield s
    capi.SignalDevice.uninstall()


@pytest.fixture(scope="module")
def work():
    return tempfile.mkdtemp(prefix="staramd_signal_vec_")


# ---- the vectors themselves ----------------------------------------------------------------------------------------------------------------------

def test_constants_and_vectors_cover_the_cases(sg):
    assert (sg.tile, sg.chunk) == (T, CH)
    nhs = sum_order_nh()
    assert struct.pack("<d", _fsum(nhs)) != struct.pack("<d", _fsum(nhs[::-1])), "the stack cannot tell the orders apart: a test bug"
    assert set(nhs) == {3, 5, 6, 7, 1}
    v = vectors()
    assert list(v) == VECTOR_NAMES
    for name, recs in v.items():
        assert [key_of(x) for x in recs] == sorted(key_of(x) for x in recs), name


@pytest.mark.parametrize("name", VECTOR_NAMES)
def test_host_records_entry(sg, work, name):
    """the tool mode with --gpuSignal Device (upload, the kernels, the formatter) against the tool mode without it"""
    for prefix in (None, "chr"):
        if prefix and name not in ("skips_refs", "mix"):
            continue
        for opt in options(name):
            flags = wig_flags(*opt, prefix=prefix)
            want = host_expected(work, name, flags)
            got = tool_mode(os.path.join(work, name + ".bam"), os.path.join(work, name + "_d%s_" % flag_tag(flags)), flags, device=True)
            if name == "past_end" and opt[3] == 0:                                              # (the other types count no block of these records)
                assert want == got == BUG, (opt, want, got)
                continue
            assert isinstance(want, dict) and len(want) == (4 if opt[1] else 2), (opt, want)
            assert got == want, (name, opt, prefix, [f for f in want if got.get(f) != want[f]] if isinstance(got, dict) else got)
    if name not in ("empty", "past_end"):
        assert sum(len(x) for x in want.values()) > 0


def test_what_the_vectors_show(sg, work):
    """the expected files hold what each vector is there for (a vector whose case never reaches the files would test nothing)"""
    bg = host_expected(work, "tile_edges", wig_flags("bg", 0, 0, 0))["Signal.Unique.str1.out.bg"].decode()
    assert "chrA\t%d\t%d\t1\n" % (20 * T - 10, 20 * T + 10) in bg                                   # one line across the tile boundary
    assert "chrA\t%d\t%d\t1\n" % (22 * T - 10, 22 * T) in bg
    um = host_expected(work, "sum_order", wig_flags("bg", 0, 0, 0))["Signal.UniqueMultiple.str1.out.bg"].decode()
    assert um == "chrA\t%d\t%d\t%g\n" % (40 * T + 7, 40 * T + 12, _fsum(sum_order_nh()))
    wig = host_expected(work, "skips_refs", wig_flags("wig", 0, 0, 0))["Signal.Unique.str1.out.wig"].decode()
    assert "variableStep chrom=chrC\nvariableStep chrom=other1\n" in wig                            # a header for the chromosome of duplicates only
    assert "other1" not in host_expected(work, "skips_refs", wig_flags("wig", 0, 0, 0, prefix="chr"), tag="hp")["Signal.Unique.str1.out.wig"].decode()
    inf = host_expected(work, "no_nh", wig_flags("bg", 1, 1, 0))
    assert b"\tinf\n" in inf["Signal.Unique.str1.out.bg"] and b"\tinf\n" in inf["Signal.UniqueMultiple.str2.out.bg"]
    assert host_expected(work, "spare_base", wig_flags("bg", 0, 0, 0))["Signal.Unique.str1.out.bg"].decode().startswith("chrB\t2991\tchrC\t")


def test_runs_of_the_device(sg):
    """the result itself: runs in order, none of value 0, none across a tile boundary; the normalisation words; the has-records flags"""
    v = vectors()
    runs, norm, has, past, stats = sg.host_records(v["tile_edges"], 0, True, CHR_LEN)
    assert not past and has == [1, 0, 0, 0] and norm == [1, 2, 3, 1, 2, 1, 1, 1, 1, 2]
    assert all(val != 0 and s < e and s // T == (e - 1) // T for _, _, s, e, val in runs)
    for tr in range(4):
        mine = [(tid, s, e) for tid, t, s, e, _ in runs if t == tr]
        assert mine == sorted(mine) and all(a[2] <= b[1] for a, b in zip(mine, mine[1:]) if a[0] == b[0]), tr
    tiles = {0, 1, 3, 4, 5, 10, (10 * T + 25 + 500000) // T, 19, 20, 21, 22}
    assert {s // T for _, _, s, e, _ in runs} == tiles and stats[2] == len(tiles)                  # nothing for the tiles the gap jumps over
    assert stats[0] == 10 and stats[1] == 1 + 2 + 2 + 2 + 3 + 2 + 4 and stats[3] == 24 * len(runs)
    runs, norm, has, past, _ = sg.host_records(v["skips_refs"], 0, False, CHR_LEN, wanted=[1, 1, 1, 0])
    assert has == [1, 1, 1, 0] and norm == [1, 1, 2, 2, 1, 3, 0, 0, 0, 0] and {r[0] for r in runs} == {0, 1} and {r[1] for r in runs} == {0, 1}
    runs, norm, has, past, _ = sg.host_records(v["nh_forms"], 0, False, CHR_LEN)
    assert norm == [3] * 6 + [2, 5, 7, 6, 0, 0, 0, 0xffffffff, 0, 0, 300, 70000]
    assert sg.host_records(v["past_end"], 0, False, CHR_LEN)[3] is True
    assert sg.host_records(v["mates"], 0, False, CHR_LEN, want_norm=False)[1] is None
    assert sg.host_records([], 0, True, CHR_LEN) == ([], None, [0, 0, 0, 0], False, [0] * 8)


def test_many_tiles_and_deep_stacks(sg, work):
    bam = write_bam(os.path.join(work, "many.bam"), many_vector(), MANY_CHROMS)
    flags = wig_flags("bg", 1, 1, 0)
    want = tool_mode(bam, os.path.join(work, "many_h_"), flags)
    assert isinstance(want, dict) and sum(len(x) for x in want.values()) > 1000000
    assert tool_mode(bam, os.path.join(work, "many_d_"), flags + ["--runThreadN", "3"], device=True) == want      # (with threads the tracks are written side by side)


def test_errors_of_the_entry(sg):
    with pytest.raises(RuntimeError, match="type 3 is not 0, 1 or 2"):
        sg.host_records([], 3, True, CHR_LEN)
    bad = rec(0, 5, [(5, "M")])
    with pytest.raises(RuntimeError, match="record 0 lies outside"):
        sg.host_records([bad[:-3]], 0, True, CHR_LEN)


# ---- through the sorter ---------------------------------------------------------------------------------------------------------------------------

def sorter_case(sg, bz, lib, recs, cuts, opt, workdir, tag, shuffle=None):
    """the records appended in len(cuts) + 1 appends (shuffled inside an append when asked: the sorter brings them back in order), finished with the tracks;
    returns (members, Signal.* files made by the formatter from the result or its error text)"""
    fmt, strand, norm, typ = opt
    with S._Env({"STARAMD_BAMSORT_SLAB_BYTES": 4096, "STARAMD_BAMSORT_ROUND_BLOCKS": 2}):
        bs = capi.BamSortDevice(bz, lib_path=lib)
    try:
        lo = 0
        for hi in list(cuts) + [len(recs)]:
            idx = list(range(lo, hi))
            if shuffle:
                shuffle.shuffle(idx)
            data, ks, off = b"", [], 0
            for i in idx:
                ks.append((key_of(recs[i]), i, off, len(recs[i]))); off += len(recs[i])
                data += recs[i]
            assert bs.append(data, ks)
            lo = hi
        out, (runs, nm, has, past, stats) = sg.sorter_tracks(bs, 1, typ, strand, CHR_LEN, want_norm=bool(norm))
    finally:
        bs.close()
    prefix = os.path.join(workdir, tag + "_")
    err = capi.signal_files_from_runs(["--runMode", "inputAlignmentsFromBAM", "--inputBAMfile", "x", "--outFileNamePrefix", prefix] + wig_flags(*opt), CHR_NAMES, CHR_LEN, runs, nm, has, past)
    return out, (err or signal_files(prefix))


@pytest.fixture(scope="module")
def bz():
    b = capi.BgzfDevice(lib_path=emul_lib())
    yield b
    b.close()


@pytest.mark.parametrize("name", VECTOR_NAMES)
def test_through_the_sorter(sg, bz, work, name):
    recs = vectors()[name]
    n = len(recs)
    cuts = [c for c in (n // 3, n // 2) if 0 < c < n]                                          # sum_order: the stack split over appends
    plain, _ = S.sort_vector(bz, emul_lib(), {"appends": [(b"".join(recs), [(key_of(x), i, sum(len(y) for y in recs[:i]), len(x)) for i, x in enumerate(recs)])] if recs else [],
                                              "env": {"STARAMD_BAMSORT_SLAB_BYTES": 4096, "STARAMD_BAMSORT_ROUND_BLOCKS": 2}}, 1)
    for k, opt in enumerate([("bg", 1, 1, 0), ("wig", 0, 0, 0), ("bg", 1, 0, 1), ("bg", 0, 1, 2)]):
        want = host_expected(work, name, wig_flags(*opt))
        out, got = sorter_case(sg, bz, emul_lib(), recs, cuts, opt, work, "%s_s%d" % (name, k), shuffle=random.Random(k) if k % 2 else None)
        assert got == want, (name, opt)
        assert out == plain, "staramd_bamsort_finish_signal changes the bytes of the BAM"


def test_sorter_is_reusable_and_plain_finish_is_unchanged(sg, bz, work):
    v = vectors()
    bs = capi.BamSortDevice(bz, lib_path=emul_lib())
    try:
        for name in ("mates", "empty", "chr_end"):
            recs = v[name]
            if recs:
                assert bs.append(b"".join(recs), [(key_of(x), i, sum(len(y) for y in recs[:i]), len(x)) for i, x in enumerate(recs)])
            out, res = sg.sorter_tracks(bs, 1, 0, True, CHR_LEN)
            assert res[4][0] == len(recs)
            if recs:
                assert bs.append(b"".join(recs), [(key_of(x), i, sum(len(y) for y in recs[:i]), len(x)) for i, x in enumerate(recs)])
            assert bs.finish(1) == out                                                          # the hook does not outlive its call
    finally:
        bs.close()


# ---- the formatter alone --------------------------------------------------------------------------------------------------------------------------

def _format(work, tag, flags, runs, norm, has, past=False):
    prefix = os.path.join(work, "fmt_%s_" % tag)
    err = capi.signal_files_from_runs(["--runMode", "inputAlignmentsFromBAM", "--inputBAMfile", "x", "--outFileNamePrefix", prefix] + flags, CHR_NAMES, CHR_LEN, runs, norm, has, past)
    return err or {k: v.decode() for k, v in signal_files(prefix).items()}


def test_formatter_alone(work, built):
    third, other = (1.0 / 3 + 1.0 / 5) + 1.0 / 7, (1.0 / 7 + 1.0 / 5) + 1.0 / 3
    runs = [(0, 0, 1000, 1024, 2.0), (0, 1, 1000, 1024, third), (0, 0, 1024, 1030, 2.0), (0, 0, 1030, 1040, 3.0), (0, 1, 1024, 1030, other),
            (0, 0, 1050, 1060, 3.0), (0, 3, 5, 7, 0.5), (2, 0, 0, 2, 1.0)]
    has = [1, 1, 1, 0]
    bg = _format(work, "bg", wig_flags("bg", 1, 0, 0), runs, None, has)
    assert bg["Signal.Unique.str1.out.bg"] == "chrA\t1000\t1030\t2\nchrA\t1030\t1040\t3\nchrA\t1050\t1060\t3\nchrC\t0\t2\t1\n"       # joined where they touch and hold the same bits only
    same = struct.pack("<d", third) == struct.pack("<d", other)
    assert bg["Signal.UniqueMultiple.str1.out.bg"] == ("chrA\t1000\t1030\t%g\n" % third if same else "chrA\t1000\t1024\t%g\nchrA\t1024\t1030\t%g\n" % (third, other))
    assert bg["Signal.Unique.str2.out.bg"] == "" and bg["Signal.UniqueMultiple.str2.out.bg"] == "chrA\t5\t7\t0.5\n"
    wig = _format(work, "wig", wig_flags("wig", 1, 0, 0), runs[-2:], None, has)
    assert wig["Signal.UniqueMultiple.str2.out.wig"] == "variableStep chrom=chrA\n6\t0.5\n7\t0.5\nvariableStep chrom=chrB\nvariableStep chrom=chrC\n"
    assert wig["Signal.Unique.str1.out.wig"] == "variableStep chrom=chrA\nvariableStep chrom=chrB\nvariableStep chrom=chrC\n1\t1\n2\t1\n"
    # normalisation: the words in order, 1e6 / nUniq and 1e6 / (nUniq + nMult), fixed with five digits; two tracks when unstranded
    nm = _format(work, "norm", wig_flags("bg", 0, 1, 0), [(0, 0, 10, 20, 1.0), (0, 1, 10, 20, 1.5)], [1, 0, 2, 1, 4], has)
    assert nm == {"Signal.Unique.str1.out.bg": "chrA\t10\t20\t%.5f\n" % (1e6 / 2), "Signal.UniqueMultiple.str1.out.bg": "chrA\t10\t20\t%.5f\n" % (1.5 * (1e6 / 2.75))}
    assert _format(work, "none", wig_flags("wig", 1, 1, 0), [], [], [0, 0, 0, 0]) == {"Signal.%s.str%d.out.wig" % (u, s): "" for u in ("Unique", "UniqueMultiple") for s in (1, 2)}
    assert _format(work, "bug", wig_flags("bg", 1, 1, 0), [], [], has, past=True) == BUG


# ---- the reference on the same fabricated BAM files ----------------------------------------------------------------------------------------------

@pytest.mark.skipif(not refstar.have_ref(), reason="oracle/_ref/STAR not built")
@pytest.mark.parametrize("name", REF_SAFE)
def test_reference_on_the_fabricated_bam(sg, work, name):
    opt = ("bg", 1, 1, 0) if name != "mates" else ("wig", 1, 0, 1)
    flags = wig_flags(*opt)
    host_expected(work, name, flags)
    ref = os.path.join(work, name + "_ref_")
    subprocess.check_call([refstar.REF_BIN, "--runMode", "inputAlignmentsFromBAM", "--inputBAMfile", os.path.join(work, name + ".bam"), "--outFileNamePrefix", ref] + flags,
                          stdout=subprocess.DEVNULL, cwd=work)
    want = signal_files(ref)
    assert len(want) == 4
    assert tool_mode(os.path.join(work, name + ".bam"), os.path.join(work, name + "_dr_"), flags, device=True) == want
