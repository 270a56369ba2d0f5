"""k_inflate.hip (--gpuBAMinflate Device, include/star_amd_inflate.h) compiled for the host by the wave emulator beside the four other stand-alone units:
every well-formed vector of tests/inflate_vectors.py gives zlib's bytes (the vectors are first held to zlib here, so no expectation comes from the code
under test), every malformed one the expected status at the expected member -- and the host path (gzread, through the tool mode) fails on it too --, with
the lanes in both orders; a file with more members than one sweep of the grid; the exports; and the tool mode through the emulated units: --gpuBAMinflate
Device writes the files of Host, with either form of the duplicate marking and of the signal tracks behind it."""
import os
import subprocess
import tempfile
import zlib

import pytest

from util import ROOT, capi, bam_parts
import inflate_vectors as V
import test_dedup_emul as D
import test_signal_emul as G

UNITS = ("k_bgzf", "k_bamsort", "k_signal", "k_dedup", "k_inflate")
COULD_NOT = "could not decompress --inputBAMfile"
_EMUL = {}


def emul_lib():
    """the five stand-alone device units + the wave emulator's runtime in a temporary shared library, built once per process; oracle/ is only read"""
    if "so" not in _EMUL:
        d = tempfile.mkdtemp(prefix="staramd_inflate_emul_")
        cl = os.environ.get("EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
        hipfl = ["-x", "c++", "-std=c++17", "-O1", "-fPIC", "-Wno-unknown-attributes", "-I", "oracle/wave_emul"]
        jobs = [("star_amd/csrc/engine/%s.hip" % u, hipfl) for u in UNITS]
        jobs += [("oracle/wave_emul/emu.cpp", ["-std=c++17", "-O1", "-fPIC", "-D_GNU_SOURCE"]), ("oracle/wave_emul/emu_lds.cpp", ["-std=c++17", "-O1", "-fPIC"])]
        procs, objs = [], []
        for src, fl in jobs:
            o = os.path.join(d, os.path.basename(src) + ".o")
            procs.append(subprocess.Popen([cl] + fl + ["-c", src, "-o", o], cwd=ROOT))
            objs.append(o)
        assert all(p.wait() == 0 for p in procs)
        so = os.path.join(d, "libinflate_units_emul.so")
        subprocess.check_call([cl, "-shared", "-fPIC"] + objs + ["-o", so, "-ldl"], cwd=ROOT)
        _EMUL["so"] = so
    return _EMUL["so"]


@pytest.fixture(scope="module")
def infl(built):
    d = capi.InflateDevice(lib_path=emul_lib())
    d.install()
    yield d
    capi.InflateDevice.uninstall()


@pytest.fixture(scope="module")
def work():
    return tempfile.mkdtemp(prefix="staramd_inflate_emul_vec_")


class Env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def expect_wellformed(got, file_bytes, datas, name):
    out, failed, status, n_members, stats = got
    want = b"".join(datas)
    assert (failed, status) == (-1, "OK"), (name, failed, status)
    assert out == want, (name, len(out), len(want))
    assert n_members == len(datas) and stats[0] == len(datas) and stats[1] == len(file_bytes) and stats[2] == len(want) and stats[5] == sum(1 for x in datas if not x), (name, stats)


def expect_malformed(got, member, status, name):
    out, failed, st, n_members, stats = got
    assert out is None and (failed, st) == (member, status), (name, failed, st)


def test_vectors_are_zlibs_and_reach_the_cases():
    """every well-formed vector against zlib.decompressobj(-15) and zlib.crc32; what the vectors reach between them.  An empty class fails"""
    W = V.wellformed()
    for name, (f, datas) in W.items():
        V.check_wellformed(name, f, datas)
    got = V.reach([f for f, _ in W.values()])
    assert not V.REACH_WANTED - got, sorted(V.REACH_WANTED - got)
    statuses = {s for _, _, s in V.malformed().values()} | {s for _, _, s in V.lenient().values()}
    assert statuses == set(capi.InflateDevice.STATUS[1:]), sorted(set(capi.InflateDevice.STATUS[1:]) ^ statuses)
    sizes = {len(d) for _, datas in W.values() for d in datas}
    assert {0, 1, 0xff00, 65536, 65505} <= sizes


@pytest.mark.parametrize("order", ["asc", "desc"])
def test_wellformed_vectors(infl, order):
    with Env(STARAMD_EMUL_ORDER=None if order == "asc" else "desc"):
        for name, (f, datas) in V.wellformed().items():
            expect_wellformed(infl.host_file(f), f, datas, name)


@pytest.mark.parametrize("order", ["asc", "desc"])
def test_malformed_vectors(infl, order):
    with Env(STARAMD_EMUL_ORDER=None if order == "asc" else "desc"):
        for name, (f, member, status) in list(V.malformed().items()) + list(V.lenient().items()):
            expect_malformed(infl.host_file(f), member, status, name)


def zlib_datas(f):
    """the data of every member of a file, by zlib alone (CRC and ISIZE checked)"""
    out = []
    for d, crc, isize in V.members_of(f):
        z = zlib.decompressobj(-15)
        got = z.decompress(d)
        assert z.eof and z.unused_data == b"" and zlib.crc32(got) == crc and len(got) == isize
        out.append(got)
    return out


def test_members_of_the_projects_own_writers(infl, work):
    """members written by the host library's bgzfCompress (a Processed.out.bam of the host path) and by the emulated k_bgzf.hip at levels 1 and 6"""
    bam = D.write_bam(os.path.join(work, "own_layout.bam"), D.vectors()["layout"])
    assert tool(bam, os.path.join(work, "own_h_"), DEDUP + ["--outBAMcompression", "6"]) is None
    f = open(os.path.join(work, "own_h_Processed.out.bam"), "rb").read()
    datas = zlib_datas(f)
    assert len(datas) >= 3 and sum(map(len, datas)) > 60000
    expect_wellformed(infl.host_file(f), f, datas, "bgzfCompress")
    bz = capi.BgzfDevice(lib_path=emul_lib())
    try:
        recs = V.record_stream(2 * V.IN_MAX + 777, 8)
        for level in (1, 6):
            f = b"".join(bz.compress(level, [recs, recs[:5000], b"", recs[100:101]])) + V.EOF_MARKER
            datas = zlib_datas(f)
            assert b"".join(datas) == recs + recs[:5000] + recs[100:101] and len(datas) == 6
            assert "dynamic" in V.reach([f])
            expect_wellformed(infl.host_file(f), f, datas, "k_bgzf level %d" % level)
    finally:
        bz.close()


def test_not_bgzf_is_an_error_that_names_the_host_path(infl):
    for name, (f, piece) in V.not_bgzf().items():
        with pytest.raises(RuntimeError, match="--gpuBAMinflate Host") as e:
            infl.host_file(f)
        assert piece in str(e.value), (name, str(e.value))
    assert infl.host_file(b"") == (b"", -1, "OK", 0, [0] * 8)


def many_members(n, seed=9):
    """n members of seven kinds, in an order in which every run of seven holds them all"""
    recs = V.record_stream(40 * n + 4000, seed)
    hand = V._by_hand()
    kinds = [lambda i: V.zmember(recs[40 * i:40 * i + 300 + i % 50], 6), lambda i: V.zmember(recs[40 * i:40 * i + 200], 0), lambda i: V.member(bytes([3, 0]), b""),
             lambda i: V.member(*hand["dyn_runs"]), lambda i: V.zmember(recs[40 * i:40 * i + 900], 1, flush_at=450), lambda i: V.member(*hand["run_dist1"]),
             lambda i: V.member(*hand["dist_equals_produced"])]
    return [kinds[i % 7](i) for i in range(n)]


def zdata(m):
    """the data of a file of one member, by zlib"""
    (d, crc, isize), = V.members_of(m)
    out = zlib.decompressobj(-15).decompress(d)
    assert zlib.crc32(out) == crc and len(out) == isize
    return out


def test_more_members_than_one_sweep(infl):
    """the emulator has 2 CUs: a grid of workgroups_per_cu * 2 workgroups of members_per_workgroup members; and once more with a cap of 2 workgroups"""
    sweep = infl.workgroups_per_cu * 2 * infl.members_per_workgroup
    ms = many_members(sweep + 9)
    for m in ms[:7]:
        assert infl.host_file(m)[0] == zdata(m)
    f = b"".join(ms)
    want = b"".join(zdata(m) for m in ms)
    out, failed, status, n, stats = infl.host_file(f)
    assert (failed, status, n) == (-1, "OK", len(ms)) and out == want
    assert infl.max_workgroups() == 0 and (infl.workgroup, infl.members_per_workgroup, infl.workgroups_per_cu) == (256, 4, 8)
    with Env(STARAMD_INFLATE_MAX_WORKGROUPS=2):
        assert infl.max_workgroups() == 2
        assert infl.host_file(f)[0] == want
        bad = ms[:20] + [V._bad_members()["distance_too_far"][0]] + ms[20:40] + [V._bad_members()["wrong_crc"][0]]
        assert infl.host_file(b"".join(bad))[:3] == (None, 20, "DISTANCE")      # the lowest failing member is reported


def test_exports(infl):
    def exported(path):
        return {l.split()[-1] for l in subprocess.check_output(["nm", "-D", "--defined-only", path], text=True).splitlines() if l.strip()}
    abi = {"staramd_inflate_host_file", "staramd_inflate_free", "staramd_inflate_constant", "staramd_inflate_last_error"}
    assert abi <= exported(emul_lib())
    if os.path.isfile(capi.ENGINE_PATH):
        assert abi <= exported(capi.ENGINE_PATH)
    assert {"sah_set_inflate_device", "sah_inflate_on_device"} <= exported(capi.HOST_PATH)
    assert infl.lds_per_wavefront <= 4096           # several wavefronts per SIMD keep their tables in the CU's LDS


# ---- the tool mode ------------------------------------------------------------------------------------------------------------------------------------

def tool(bam, prefix, more):
    """--runMode inputAlignmentsFromBAM in this process: None, or the error text"""
    try:
        capi.HostRun(["--runMode", "inputAlignmentsFromBAM", "--inputBAMfile", bam, "--outFileNamePrefix", prefix] + list(more)).close()
    except RuntimeError as e:
        return str(e)
    return None


DEDUP = ["--bamRemoveDuplicatesType", "UniqueIdentical"]


def test_tool_mode_dedup_writes_the_hosts_file(infl, work):
    dd = capi.DedupDevice(lib_path=emul_lib())
    dd.install()
    try:
        for name in ("one_of_each", "layout", "empty"):
            bam = D.write_bam(os.path.join(work, name + ".bam"), D.vectors()[name])
            outs = {}
            for tag, more in (("hh", []), ("dh", ["--gpuBAMinflate", "Device"]), ("dd", ["--gpuBAMinflate", "Device", "--gpuBAMdedup", "Device"]), ("hd", ["--gpuBAMinflate", "Host", "--gpuBAMdedup", "Device"])):
                prefix = os.path.join(work, "%s_%s_" % (name, tag))
                assert tool(bam, prefix, DEDUP + more) is None, (name, tag)
                outs[tag] = (bam_parts(prefix + "Processed.out.bam"), open(prefix + "Processed.out.bam", "rb").read())
                log = open(prefix + "Log.out").read()
                where = "Device" if tag[0] == "d" else "Host"
                assert log.count("(--gpuBAMinflate)") == 1 and log.count("--inputBAMfile inflated on the %s (--gpuBAMinflate): " % where) == 1, (name, tag)
                if where == "Device":
                    raw = open(bam, "rb").read()
                    assert "%d members, %d bytes in, %d bytes out\n" % (len(V.members_of(raw)), len(raw), sum(m[2] for m in V.members_of(raw))) in log
            assert outs["hh"] == outs["dh"] == outs["dd"] == outs["hd"], name
    finally:
        capi.DedupDevice.uninstall()


def test_tool_mode_signal_tracks(infl, work):
    sd = capi.SignalDevice(lib_path=emul_lib())
    sd.install()
    try:
        bam = D.write_bam(os.path.join(work, "sig_layout.bam"), D.vectors()["layout"])
        outs = {}
        for tag, more in (("hh", []), ("dh", ["--gpuBAMinflate", "Device"]), ("dd", ["--gpuBAMinflate", "Device", "--gpuSignal", "Device"]), ("hd", ["--gpuSignal", "Device"])):
            prefix = os.path.join(work, "sig_%s_" % tag)
            assert tool(bam, prefix, ["--outWigType", "bedGraph"] + more) is None, tag
            outs[tag] = G.signal_files(prefix)
            assert len(outs[tag]) == 4 and any(outs[tag].values())
        assert outs["hh"] == outs["dh"] == outs["dd"] == outs["hd"]
    finally:
        capi.SignalDevice.uninstall()


def test_device_flag_without_functions(infl, work):
    bam = D.write_bam(os.path.join(work, "clips.bam"), D.vectors()["clips"])
    capi.InflateDevice.uninstall()
    try:
        got = tool(bam, os.path.join(work, "clips_none_"), DEDUP + ["--gpuBAMinflate", "Device"])
        assert "--gpuBAMinflate Device, but no device inflate functions are installed" in got
    finally:
        infl.install()
    assert "EXITING: --gpuBAMinflate takes Host or Device" in tool(bam, os.path.join(work, "clips_bad_"), DEDUP + ["--gpuBAMinflate", "Both"])


def test_malformed_input_fails_on_both_paths(infl, work):
    """every malformed vector: the host path (gzread) fails, the device path fails with the host's text, and neither leaves an output file"""
    for name, (f, member, status) in V.malformed().items():
        bam = os.path.join(work, "bad_%s.bam" % name)
        open(bam, "wb").write(f)
        for tag, more in (("h", []), ("d", ["--gpuBAMinflate", "Device"])):
            prefix = os.path.join(work, "bad_%s_%s_" % (name, tag))
            got = tool(bam, prefix, DEDUP + more)
            assert got is not None and COULD_NOT in got, (name, tag, got)
            assert not os.path.exists(prefix + "Processed.out.bam"), (name, tag)


def test_files_gzread_accepts_and_the_device_does_not(infl, work):
    """gzread never reads BSIZE and takes a file that ends inside a member for a file that ends: the Host path goes on with the bytes it got.  The device
    walks the BSIZE chain and says that the member is cut.  A file that is gzip but not BGZF is a device error whose text names the way out"""
    for name, (f, member, status) in V.lenient().items():
        bam = os.path.join(work, "len_%s.bam" % name)
        open(bam, "wb").write(f)
        assert tool(bam, os.path.join(work, "len_%s_h_" % name), DEDUP) is None, name
        got = tool(bam, os.path.join(work, "len_%s_d_" % name), DEDUP + ["--gpuBAMinflate", "Device"])
        assert got is not None and COULD_NOT in got, (name, got)
    import gzip
    plain = os.path.join(work, "plain.bam")
    open(plain, "wb").write(gzip.compress(b"".join(bam_raw(D.vectors()["clips"]))))
    assert tool(plain, os.path.join(work, "plain_h_"), DEDUP) is None
    got = tool(plain, os.path.join(work, "plain_d_"), DEDUP + ["--gpuBAMinflate", "Device"])
    assert "--gpuBAMinflate Device: " in got and "gzip but not BGZF.  SOLUTION: --gpuBAMinflate Host" in got and not os.path.exists(os.path.join(work, "plain_d_Processed.out.bam"))


def bam_raw(records):
    _, h = V.bam_header_member()
    return [h] + list(records)
