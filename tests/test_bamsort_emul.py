"""k_bamsort.hip (--gpuBAMsort Device, include/star_amd_bamsort.h) compiled for the host by the wave emulator together with k_bgzf.hip: the inflated
output is the records in the order of the host comparator (g, r, order of appending); the compressed bytes are those of the compressor on that stream
(same kernel, same block cut: one segment, every member but the last 0xff00 bytes); budget, download and the front end (capi.HostRun with the emulated
sorter behind sah_set_bamsort_device: Device against Host, --runThreadN 1 against 3, the spill to the host path, the flags).
The GPU tests (tests/test_gpu_bamsort.py) hold the shipped library to the bytes made here, vector by vector."""
import ctypes as C
import os
import random
import struct
import tempfile

import pytest

from util import _map, bam_parts, capi, emul_units_lib, oracle_lib
import test_golden
import test_bgzf_emul as E

IN_MAX = 0xff00
TILE = 32768                    # output bytes per workgroup of k_bamsort_gather, 127 records per LDS chunk
UNMAPPED = (1 << 64) - 1
LEVELS = (0, 1, 6)
_VEC = {}


def emul_lib():
    """the library of the emulated device units (util.emul_units_lib: built once per process)"""
    return emul_units_lib()


def _record(r, i, n):
    """n bytes that name record i and compress like text"""
    return (b"rec%07d:" % i + bytes(r.choice(b"ACGT") for _ in range(max(0, n - 11))))[:n] if n > 1 else bytes([65 + i % 26])[:n]


def _vector(r, lens, keys, cuts=(), slab=None, blocks=None):
    """records of the lengths `lens` with keys[i] = (g, r), appended in len(cuts) + 1 appends that end before the records `cuts`"""
    recs = [_record(r, i, n) for i, n in enumerate(lens)]
    appends, lo = [], 0
    for hi in list(cuts) + [len(lens)]:
        off, ks = 0, []
        for i in range(lo, hi):
            ks.append((keys[i][0], keys[i][1], off, lens[i]))
            off += lens[i]
        appends.append((b"".join(recs[lo:hi]), ks))
        lo = hi
    return {"appends": appends, "env": {"STARAMD_BAMSORT_SLAB_BYTES": slab, "STARAMD_BAMSORT_ROUND_BLOCKS": blocks}}


def vectors():
    """name -> {"appends": [(records, [(g, r, off, len)])], "env": {...}}; the same for the emulator and, in tests/test_gpu_bamsort.py, the MI355X"""
    if _VEC:
        return _VEC
    r = random.Random(20261019)
    rk = lambda n: [(r.randrange(40) << 32 | r.randrange(1 << 20), r.randrange(1 << 33)) for _ in range(n)]
    rl = lambda n: [r.choice([1, 2, 3, 5, 15, 16, 17, 31, 33, 63, 64, 100, 255, 257, 399, 400, r.randint(1, 400)]) for _ in range(n)]
    v = _VEC
    v["empty"] = {"appends": [], "env": {}}
    v["one_byte"] = _vector(r, [1], [(5, 7)])
    v["n65"] = _vector(r, rl(65), rk(65))
    v["n257"] = _vector(r, rl(257), rk(257), cuts=(100,), slab=4096, blocks=2)
    v["n5000"] = _vector(r, [r.randint(1, 400) for _ in range(5000)], rk(5000), cuts=(1700, 1701), blocks=3)       # 30 tiles for the emulator's 8 workgroups, 6 rounds
    v["same_g"] = _vector(r, rl(300), [(77 << 32 | 1234, x) for x in r.sample(range(1 << 40), 300)])
    v["all_equal"] = _vector(r, rl(300), [(3 << 32 | 9, 11)] * 300, cuts=(90, 200), slab=4096)                    # stability, within and across appends
    ks = [(UNMAPPED, r.randrange(1 << 30)) for _ in range(20)] + [(1 << 62 | r.randrange(1 << 40), r.randrange(1 << 30)) for _ in range(20)]
    ks += [((1 << 16) + r.randrange(5) << 32 | (1 << 31) + r.randrange(1000), 1 << 63 | r.randrange(1 << 20)) for _ in range(20)] + rk(40)
    ks += [(UNMAPPED, 1 << 63 | 5), (0, 0), (UNMAPPED - 1, (1 << 64) - 1)]
    r.shuffle(ks)
    v["key_mix"] = _vector(r, rl(len(ks)), ks, cuts=(50,))
    srt = sorted(rk(200))
    v["sorted"] = _vector(r, rl(200), srt)
    v["reverse"] = _vector(r, rl(200), srt[::-1])
    v["cross_block"] = _vector(r, [300] * 250, rk(250))                                      # 0xff00 = 217.6 records
    v["cross_round"] = _vector(r, [301] * 500, rk(500), blocks=2)                            # 2 * 0xff00 = 433.75 records
    v["long_record"] = _vector(r, [100, 70000, 7, 300], [(9, 1), (4, 4), (4, 3), (1, 0)], cuts=(1, 2), slab=4096, blocks=1)     # tiles 1 and 2 hold parts of one record only
    v["slab_exact"] = _vector(r, [256] * 16 + [100, 3], rk(18), cuts=(16,), slab=4096)
    v["total_ff00"] = _vector(r, [256] * 255, rk(255))
    v["total_2ff00_1"] = _vector(r, [256] * 510 + [1], rk(511), cuts=(300,), blocks=1)
    v["many_tiny"] = _vector(r, [r.randint(1, 3) for _ in range(40000)], rk(40000), cuts=(15000,))           # 16000 records per tile: 130 LDS chunks
    # the keys need not tile `records`: the stream is what the keys name.  100 bytes of which one key names 50 (the stream is shorter than the append) ...
    v["gap_tail"] = {"appends": [(_record(r, 0, 100), [(1, 1, 0, 50)])], "env": {}}
    # ... and over several tiles: junk before every record and behind the last, two keys over the same bytes, an empty record, an append no key names
    appends = []
    for cut in (250, 350):
        data, ks = bytearray(), []
        for i in range(cut):
            data += bytes(r.getrandbits(8) for _ in range(r.randint(0, 9)))
            n = r.choice([1, 15, 16, 17, 100, 255, r.randint(1, 300)])
            ks.append((r.randrange(40) << 32, r.randrange(1 << 20), len(data), n))
            data += _record(r, i, n)
        ks += [(5 << 32, 77, ks[3][2], ks[3][3] + ks[4][3] // 2), (6 << 32, 1, len(data), 0), (UNMAPPED, 0, 0, 40)]
        appends.append((bytes(data) + b"tail no key names" * 3, ks))
    appends.insert(1, (b"an append without keys", []))
    v["gaps_overlaps"] = {"appends": appends, "env": {"STARAMD_BAMSORT_SLAB_BYTES": 4096, "STARAMD_BAMSORT_ROUND_BLOCKS": 1}}
    return v


VECTOR_NAMES = list(vectors())


def expected_stream(vec):
    recs, keys = [], []
    for data, ks in vec["appends"]:
        for g, r, off, ln in ks:
            recs.append(data[off:off + ln]); keys.append((g, r))
    order = sorted(range(len(recs)), key=lambda i: (keys[i][0], keys[i][1], i))
    return b"".join(recs[i] for i in order)


class _Env:
    def __init__(self, env):
        self.env = {k: v for k, v in env.items() if v is not None}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in ("STARAMD_BAMSORT_SLAB_BYTES", "STARAMD_BAMSORT_ROUND_BLOCKS")}
        for k in self.old:
            os.environ.pop(k, None)
        os.environ.update({k: str(v) for k, v in self.env.items()})

    def __exit__(self, *a):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def sort_vector(bz, lib_path, vec, level, budget=0):
    """the vector through a BamSortDevice of its own (the two sizes are read from the environment when it is created)"""
    with _Env(vec["env"]):
        bs = capi.BamSortDevice(bz, budget=budget, lib_path=lib_path)
    try:
        for data, ks in vec["appends"]:
            assert bs.append(data, ks)
        out = bs.finish(level)
        return out, bs.stats
    finally:
        bs.close()


@pytest.fixture(scope="module")
def bz():
    b = capi.BgzfDevice(lib_path=emul_lib())
    yield b
    b.close()


def test_vectors_cover_the_cases():
    v = vectors()
    total = lambda k: sum(len(d) for d, _ in v[k]["appends"])
    assert total("total_ff00") == IN_MAX and total("total_2ff00_1") == 2 * IN_MAX + 1
    assert IN_MAX % 300 and (2 * IN_MAX) % 301
    assert len(v["slab_exact"]["appends"][0][0]) == 4096
    assert total("n5000") > 8 * TILE and total("long_record") > 2 * TILE
    assert len(v["many_tiny"]["appends"][0][1]) * TILE // total("many_tiny") > 127
    assert len(expected_stream(v["gap_tail"])) == 50 < total("gap_tail")
    assert TILE < len(expected_stream(v["gaps_overlaps"])) < total("gaps_overlaps") - 500


@pytest.mark.parametrize("name", VECTOR_NAMES)
@pytest.mark.parametrize("level", LEVELS)
def test_vectors(bz, level, name):
    vec = vectors()[name]
    want = expected_stream(vec)
    out, stats = sort_vector(bz, emul_lib(), vec, level)
    ms = E.members(out)
    assert b"".join(x for x, _ in ms) == want
    assert [len(x) for x, _ in ms] == [min(IN_MAX, len(want) - o) for o in range(0, len(want), IN_MAX)]       # every member but the last: 0xff00
    assert all(struct.unpack("<I", m)[0] == IN_MAX for m in _isizes(out)[:-1])
    assert out == bz.compress(level, [want])[0]
    if want:
        assert stats[0] == sum(len(k) for _, k in vec["appends"]) and stats[1] == len(want) and stats[3] == len(out), stats
        blocks = vec["env"].get("STARAMD_BAMSORT_ROUND_BLOCKS") or 8192
        assert stats[2] == -(-len(ms) // blocks), stats


def _after_header(path):
    """the file behind its first member: the BAM header, whose text names the command line"""
    blob = open(path, "rb").read()
    assert E.members(blob[:struct.unpack("<H", blob[16:18])[0] + 1])[0][0][:4] == b"BAM\x01"
    return blob[struct.unpack("<H", blob[16:18])[0] + 1:]


def _isizes(blob):
    p, res = 0, []
    while p < len(blob):
        bsize = struct.unpack("<H", blob[p + 16:p + 18])[0] + 1
        res.append(blob[p + bsize - 4:p + bsize])
        p += bsize
    return res


def test_sorter_is_reusable_after_finish(bz):
    v = vectors()
    bs = capi.BamSortDevice(bz, lib_path=emul_lib())
    try:
        for name in ("n65", "key_mix", "empty", "n65"):
            for data, ks in v[name]["appends"]:
                assert bs.append(data, ks)
            assert b"".join(x for x, _ in E.members(bs.finish(1))) == expected_stream(v[name]), name
    finally:
        bs.close()


def test_budget_and_download(bz):
    r = random.Random(5)
    first, second = bytes(r.getrandbits(8) for _ in range(6000)), bytes(6000)
    bs = capi.BamSortDevice(bz, budget=10000, lib_path=emul_lib())
    try:
        assert bs.append(first, [(1, 2, 0, 6000)]) is True
        assert bs.append(second, [(0, 0, 0, 6000)]) is False
        assert bs.download(0, 6000) == first
        assert bs.append(first[:4000], [(0, 0, 0, 4000)]) is True            # what is left of the budget still takes a smaller one
        assert bs.download(1, 4000) == first[:4000] and bs.download(0, 6000) == first
        assert b"".join(x for x, _ in E.members(bs.finish(1))) == first[:4000] + first
        with pytest.raises(RuntimeError, match="append 0 of 0"):
            bs.download(0, 1)
    finally:
        bs.close()


def test_unknown_level_and_bad_key(bz):
    bs = capi.BamSortDevice(bz, lib_path=emul_lib())
    try:
        assert bs.append(b"abc", [(0, 0, 0, 3)])
        with pytest.raises(RuntimeError, match="compression level 10 is not in -1..9"):
            bs.finish(10)
        with pytest.raises(RuntimeError, match="lies outside"):
            bs.append(b"abc", [(0, 0, 2, 2)])
    finally:
        bs.close()


# ---- the front end -----------------------------------------------------------------------------------------------------------------------------

def run_sorted(info0, prefix, more, bz=None, sorter=True, batch_reads=300):
    """E.run_with_bgzf with --gpuBAMsort: a BamSortDevice of the emulated library (budget: --gpuBAMsortHBM of the run) installed when `sorter`.
    Returns (prefix, sah_bam_sort_counts at the end of the run)"""
    info = dict(info0)
    info["extra"] = list(info.get("extra", [])) + list(more)
    argv = ["--genomeDir", info["idx"], "--readFilesIn"] + info["fastq"] + ["--outFileNamePrefix", prefix] + info["extra"]
    run = capi.HostRun(argv)
    eng = oracle_lib.Oracle(run.genome, run.params)
    bs = None
    try:
        if sorter:
            with _Env({"STARAMD_BAMSORT_SLAB_BYTES": 4096, "STARAMD_BAMSORT_ROUND_BLOCKS": 2}):
                bs = capi.BamSortDevice(bz, budget=run.bamsort_budget(), lib_path=emul_lib())
            run.set_bamsort_device(bs)
        while True:
            b = run.next_batch(batch_reads)
            if b is None:
                break
            run.emit(_map(eng, b).res)
        assert run.next_phase() == 0
        run.finish()
        counts = run.bam_sort_counts()
    finally:
        eng.close()
        run.close()
        if bs is not None:
            bs.close()
    return prefix, counts


BOTH = ["--outSAMtype", "BAM", "Unsorted", "SortedByCoordinate", "--outSAMunmapped", "Within", "KeepPairs"]
SORTED = "Aligned.sortedByCoord.out.bam"


@pytest.fixture(scope="module")
def front_end(bz, built):
    """the runs the front-end tests share: Host, Device with 3 threads and with 1"""
    d = tempfile.mkdtemp(prefix="staramd_bamsort_runs_")
    info = test_golden._tiny_info()
    res = {"dir": d, "info": info}
    res["Host"] = run_sorted(info, os.path.join(d, "host_"), BOTH + ["--runThreadN", "3", "--gpuBAMsort", "Host"], sorter=False)
    res["Device"] = run_sorted(info, os.path.join(d, "dev3_"), BOTH + ["--runThreadN", "3", "--gpuBAMsort", "Device"], bz)
    res["Device1"] = run_sorted(info, os.path.join(d, "dev1_"), BOTH + ["--runThreadN", "1", "--gpuBAMsort", "Device"], bz)
    return res


def test_front_end_device_against_host(front_end):
    (host, hc), (dev, dc) = front_end["Host"], front_end["Device"]
    for f in ("Aligned.out.bam", SORTED):
        assert open(dev + f, "rb").read()[-28:] == E.EOF_MARK
        assert E.same_bam(dev + f, host + f), f
    assert open(dev + SORTED, "rb").read() != open(host + SORTED, "rb").read(), "the records were not laid out and compressed by the device path"
    records = bam_parts(dev + SORTED)[2]
    assert len(records) > 1000
    assert dc[0] == len(records) and dc[1] == sum(len(x) for x in records) and dc[2] >= 2 and dc[3] == 0, dc
    assert hc == [0, 0, 0, 0]
    assert "--gpuBAMsort Device: %d records" % len(records) in open(dev + "Log.out").read()


def test_front_end_bytes_do_not_depend_on_threads(front_end):
    assert _after_header(front_end["Device1"][0] + SORTED) == _after_header(front_end["Device"][0] + SORTED)


def test_front_end_spill(front_end, bz):
    total, appends = front_end["Device"][1][1], front_end["Device"][1][2]
    assert appends >= 2
    budget = total - 1                                            # every append of these runs gets a slab of its own size (slabs of 4096 bytes): all but the last fit
    out, c = run_sorted(front_end["info"], os.path.join(front_end["dir"], "spill_"), BOTH + ["--runThreadN", "3", "--gpuBAMsort", "Device", "--gpuBAMsortHBM", str(budget)], bz)
    assert c[3] == 1 and c[0] == 0 and 1 <= c[2] < appends, c
    assert E.same_bam(out + SORTED, front_end["Host"][0] + SORTED)
    assert open(out + SORTED, "rb").read() != open(front_end["Device"][0] + SORTED, "rb").read()         # the Host path wrote it
    assert "the coordinate sort runs on the host" in open(out + "Log.out").read()


def _argv(info, prefix, more):
    return ["--genomeDir", info["idx"], "--readFilesIn"] + info["fastq"] + ["--outFileNamePrefix", prefix] + more


def test_flag_values(tmp_path, built):
    info = test_golden._tiny_info()
    with pytest.raises(RuntimeError, match="--gpuBAMsort takes Host or Device"):
        capi.HostRun(_argv(info, str(tmp_path / "a_"), ["--outSAMtype", "BAM", "SortedByCoordinate", "--gpuBAMsort", "device"]))
    with pytest.raises(RuntimeError, match="--gpuBAMsort Device orders the records of Aligned.sortedByCoord.out.bam"):
        capi.HostRun(_argv(info, str(tmp_path / "b_"), ["--outSAMtype", "BAM", "Unsorted", "--gpuBAMsort", "Device"]))
    with pytest.raises(RuntimeError, match="--gpuBAMsort Device does not work with --outWigType"):
        capi.HostRun(_argv(info, str(tmp_path / "c_"), ["--outSAMtype", "BAM", "SortedByCoordinate", "--outWigType", "bedGraph", "--gpuBAMsort", "Device"]))


def test_device_without_a_sorter_fails_at_the_first_batch(tmp_path, built):
    with pytest.raises(RuntimeError, match="sah_set_bamsort_device"):
        run_sorted(test_golden._tiny_info(), str(tmp_path / "a_"), ["--outSAMtype", "BAM", "SortedByCoordinate", "--gpuBAMsort", "Device"], sorter=False)


def test_host_is_the_default(front_end, tmp_path):
    out, c = run_sorted(front_end["info"], str(tmp_path / "plain_"), BOTH + ["--runThreadN", "3"], sorter=False)
    assert c == [0, 0, 0, 0]
    assert _after_header(out + SORTED) == _after_header(front_end["Host"][0] + SORTED) and E.same_bam(out + SORTED, front_end["Host"][0] + SORTED)


# ---- the front end's handling of the sorter, with a sorter made of Python callbacks ------------------------------------------------------------

class FakeSorter:
    """a sah_bamsort_fns of Python callbacks for HostRun.set_bamsort_device: append answers append_rc(number of the call), download and finish (with a
    sink) answer the given codes; the calls are counted, and for every finish whether its sink was null"""
    TEXT = "the fake sorter's own words"

    def __init__(self, append_rc=lambda k: 0, download_rc=0, finish_rc=0):
        self.appends, self.downloads, self.finish_sink_null = 0, 0, []
        self._text = C.create_string_buffer(self.TEXT.encode())

        def append(sorter, records, n_bytes, keys, n):
            self.appends += 1
            return append_rc(self.appends)

        def download(sorter, i_append, records):
            self.downloads += 1
            return download_rc

        def finish(sorter, level, sink, user, stats):
            self.finish_sink_null.append(not sink)
            return finish_rc if sink else 0

        self._cb = [C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32)(append),
                    C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_void_p)(download),
                    C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)(finish),
                    C.CFUNCTYPE(C.c_void_p)(lambda: C.addressof(self._text))]

    def fns(self):
        return capi.BamSortFns(*[C.cast(f, C.c_void_p) for f in self._cb]), None


def run_with_fake(prefix, fake, finish=True):
    """the tiny data set with --gpuBAMsort Device and `fake` installed, in batches of 300 reads; finish=False: destroyed after the last batch, without sah_finish"""
    run = capi.HostRun(_argv(test_golden._tiny_info(), prefix, ["--outSAMtype", "BAM", "SortedByCoordinate", "--gpuBAMsort", "Device"]))
    eng = oracle_lib.Oracle(run.genome, run.params)
    try:
        run.set_bamsort_device(fake)
        while True:
            b = run.next_batch(300)
            if b is None:
                break
            run.emit(_map(eng, b).res)
        assert run.next_phase() == 0
        if finish:
            run.finish()
    finally:
        eng.close()
        run.close()


@pytest.mark.parametrize("case", ["append", "download_in_spill", "finish"])
def test_sorter_errors_end_the_run_with_the_sorters_text(case, tmp_path, built):
    fake = {"append": lambda: FakeSorter(append_rc=lambda k: -1),
            "download_in_spill": lambda: FakeSorter(append_rc=lambda k: 1 if k == 2 else 0, download_rc=-1),
            "finish": lambda: FakeSorter(finish_rc=-1)}[case]()
    with pytest.raises(RuntimeError) as e:
        run_with_fake(str(tmp_path / "a_"), fake)
    assert str(e.value) == "EXITING because of fatal ERROR: --gpuBAMsort Device: " + FakeSorter.TEXT
    if case == "append":
        assert fake.appends == 1 and fake.downloads == 0 and fake.finish_sink_null == []
    elif case == "download_in_spill":
        assert fake.appends == 2 and fake.downloads == 1 and fake.finish_sink_null == [True]      # (the run's end leaves the sorter emptied)
    else:
        assert fake.appends >= 2 and fake.finish_sink_null == [False]


def test_run_destroyed_after_appends_empties_the_sorter(tmp_path, built):
    fake = FakeSorter()
    run_with_fake(str(tmp_path / "a_"), fake, finish=False)
    assert fake.appends >= 2 and fake.finish_sink_null == [True]
