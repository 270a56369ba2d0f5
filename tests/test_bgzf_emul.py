"""k_bgzf.hip (BGZF compression on the device, include/star_amd_bgzf.h) compiled for the host by the wave emulator (oracle/wave_emul): every member
is a valid gzip member (BSIZE, CRC32, ISIZE), the blocks are cut as the host path cuts them (0xff00 input bytes), the content round-trips, the bytes
do not depend on the order the lanes run in, and on BAM record streams level 1 stays within 1.15 x of host zlib.  The GPU tests
(tests/test_gpu_bgzf.py) hold the shipped library to the bytes made here."""
import gzip
import os
import random
import struct
import subprocess
import tempfile
import threading
import zlib

import pytest

from util import ROOT, _map, bam_parts, capi, oracle_lib, prepare, refstar, run_with_engine
import test_golden

IN_MAX = 0xff00
LEVELS = (0, 1, 6, -1)
EOF_MARK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
_LIB = {}


def emul_lib():
    """k_bgzf.hip + the emulator's runtime in a temporary shared library (built once per process; oracle/ is only read)"""
    if "so" not in _LIB:
        d = tempfile.mkdtemp(prefix="staramd_bgzf_emul_")
        cl = os.environ.get("EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
        objs = []
        for src, fl in (("star_amd/csrc/engine/k_bgzf.hip", ["-x", "c++", "-std=c++17", "-O1", "-fPIC", "-Wno-unknown-attributes", "-I", "oracle/wave_emul"]),
                        ("oracle/wave_emul/emu.cpp", ["-std=c++17", "-O1", "-fPIC", "-D_GNU_SOURCE"]),
                        ("oracle/wave_emul/emu_lds.cpp", ["-std=c++17", "-O1", "-fPIC"])):
            o = os.path.join(d, os.path.basename(src) + ".o")
            subprocess.check_call([cl] + fl + ["-c", src, "-o", o], cwd=ROOT)
            objs.append(o)
        so = os.path.join(d, "libbgzf_emul.so")
        subprocess.check_call([cl, "-shared", "-fPIC"] + objs + ["-o", so, "-ldl"], cwd=ROOT)
        _LIB["so"] = so
    return _LIB["so"]


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
    }


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


def test_level_out_of_range(bz):
    with pytest.raises(RuntimeError, match="not in -1..9"):
        bz.compress(10, [b"abc"])


def _bam_case(bz, stream):
    for level in LEVELS:
        outs = _run_checked(bz, level, [stream])
        if level == 1:
            dev, host = len(outs[0]), sum(host_sizes(stream, 1))
            assert dev <= 1.15 * host, (dev, host, dev / host)


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
    outs = {}
    for mode in ("Host", "Device"):
        info = dict(test_golden._tiny_info())
        info["extra"] = ["--outSAMtype", "BAM"] + types + ["--outSAMunmapped", "Within", "KeepPairs", "--runThreadN", "3", "--gpuBAMcompression", mode]
        outs[mode] = run_with_bgzf(info, str(tmp_path / mode) + "_", lambda g, p: oracle_lib.Oracle(g, p), bz if mode == "Device" else None, batch_reads=300)
    for f in ["Aligned.out.bam"] + (["Aligned.sortedByCoord.out.bam"] if "SortedByCoordinate" in types else []):
        h, d = open(outs["Host"] + f, "rb").read(), open(outs["Device"] + f, "rb").read()
        assert d[-28:] == EOF_MARK
        assert same_bam(outs["Device"] + f, outs["Host"] + f), f
        assert d != h, "the records were not compressed by the device path"
