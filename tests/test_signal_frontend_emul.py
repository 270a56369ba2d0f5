"""--gpuSignal Device through the front end on the wave emulator: capi.HostRun on the golden tiny_pe set with the emulated sorter and signal functions
behind sah_set_bamsort_device / sah_set_signal_device -- Device against Host (every Signal.* file and the sorted BAM), --runThreadN 1 against 3, the spill
to the host path, the flags, and the tool mode (--runMode inputAlignmentsFromBAM) with and without the device."""
import os
import tempfile

import pytest

from util import _map, capi, oracle_lib
import test_golden
import test_bamsort_emul as S
import test_bgzf_emul as E
import test_signal_emul as G

SORTED = S.SORTED
BASE = ["--outSAMtype", "BAM", "SortedByCoordinate", "--outSAMunmapped", "Within", "KeepPairs"]
WIG = ["--outWigType", "bedGraph"]
DEVICE = ["--gpuBAMcompression", "Device", "--gpuBAMsort", "Device", "--gpuSignal", "Device"]


def run(info0, prefix, more, bz=None, sg=None, batch_reads=300):
    """one alignReads run over the oracle engine; bz: the emulated compressor (its sorter is made here, with the run's budget); sg: the emulated signal functions.
    Returns (prefix, sah_bam_sort_counts, sah_signal_counts)"""
    info = dict(info0)
    argv = ["--genomeDir", info["idx"], "--readFilesIn"] + info["fastq"] + ["--outFileNamePrefix", prefix] + list(info.get("extra", [])) + list(more)
    r = capi.HostRun(argv)
    eng = oracle_lib.Oracle(r.genome, r.params)
    bs = None
    try:
        if bz is not None:
            with S._Env({"STARAMD_BAMSORT_SLAB_BYTES": 4096, "STARAMD_BAMSORT_ROUND_BLOCKS": 2}):
                bs = capi.BamSortDevice(bz, budget=r.bamsort_budget(), lib_path=G.emul_lib())
            r.set_bgzf_device(bz)
            r.set_bamsort_device(bs)
        if sg is not None:
            r.set_signal_device(sg)
        while True:
            b = r.next_batch(batch_reads)
            if b is None:
                break
            r.emit(_map(eng, b).res)
        assert r.next_phase() == 0
        r.finish()
        return prefix, r.bam_sort_counts(), r.signal_counts()
    finally:
        eng.close()
        r.close()
        if bs is not None:
            bs.close()


@pytest.fixture(scope="module")
def bz():
    b = capi.BgzfDevice(lib_path=G.emul_lib())
    yield b
    b.close()


@pytest.fixture(scope="module")
def sg(built):
    return capi.SignalDevice(lib_path=G.emul_lib())


@pytest.fixture(scope="module")
def runs(bz, sg):
    """the runs the tests share: Host / Host, and Device / Device / Device with 3 threads and with 1"""
    d = tempfile.mkdtemp(prefix="staramd_signal_runs_")
    info = test_golden._tiny_info()
    res = {"dir": d, "info": info}
    res["Host"] = run(info, os.path.join(d, "host_"), BASE + WIG + ["--runThreadN", "3"])
    res["Device"] = run(info, os.path.join(d, "dev3_"), BASE + WIG + DEVICE + ["--runThreadN", "3"], bz, sg)
    res["Device1"] = run(info, os.path.join(d, "dev1_"), BASE + WIG + DEVICE + ["--runThreadN", "1"], bz, sg)
    return res


def _same_tracks(a, b, n=4):
    fa, fb = G.signal_files(a), G.signal_files(b)
    assert len(fa) == n and fa == fb, [f for f in fa if fb.get(f) != fa[f]]
    return fa


def test_device_against_host(runs):
    (host, hc, hs), (dev, dc, ds) = runs["Host"], runs["Device"]
    files = _same_tracks(host, dev)
    assert sum(len(x) for x in files.values()) > 10000
    assert E.same_bam(dev + SORTED, host + SORTED)
    assert open(dev + SORTED, "rb").read() != open(host + SORTED, "rb").read(), "the records were not laid out and compressed by the device path"
    assert dc[0] > 1000 and dc[3] == 0 and hc == [0, 0, 0, 0]
    assert ds[0] == 1 and ds[1] == dc[0] and ds[2] > 0 and ds[3] > 0 and hs[0] == 0 and hs[1] == dc[0], (ds, hs)
    log = open(dev + "Log.out").read()
    assert "--gpuSignal Device: %d records" % dc[0] in log and "--gpuSignal" not in open(host + "Log.out").read()


def test_bytes_do_not_depend_on_threads(runs):
    _same_tracks(runs["Device"][0], runs["Device1"][0])
    assert S._after_header(runs["Device1"][0] + SORTED) == S._after_header(runs["Device"][0] + SORTED)


@pytest.mark.parametrize("more", [["--outWigType", "wiggle", "read1_5p", "--outWigStrand", "Unstranded", "--outWigNorm", "None"],
                                  ["--outWigType", "bedGraph", "read2", "--outWigReferencesPrefix", "chr2"]])
def test_other_options(runs, bz, sg, more):
    d, info = runs["dir"], runs["info"]
    tag = "".join(x[:2] for x in more if not x.startswith("--"))
    host = run(info, os.path.join(d, "h%s_" % tag), BASE + more)
    dev = run(info, os.path.join(d, "d%s_" % tag), BASE + more + DEVICE, bz, sg)
    _same_tracks(host[0], dev[0], 2 if "Unstranded" in more else 4)


def test_spill_takes_the_host_path(runs, bz, sg):
    total, appends = runs["Device"][1][1], runs["Device"][1][2]
    assert appends >= 2
    out, c, s = run(runs["info"], os.path.join(runs["dir"], "spill_"), BASE + WIG + DEVICE + ["--runThreadN", "3", "--gpuBAMsortHBM", str(total - 1)], bz, sg)
    assert c[3] == 1 and c[0] == 0, c
    assert s[0] == 0 and s[1] == runs["Device"][1][0], s
    _same_tracks(runs["Host"][0], out)
    assert E.same_bam(out + SORTED, runs["Host"][0] + SORTED)
    log = open(out + "Log.out").read()
    assert "the coordinate sort runs on the host" in log and "--gpuSignal Device: the sorted records are on the host; the signal tracks are computed on the host" in log


def _argv(info, prefix, more):
    return ["--genomeDir", info["idx"], "--readFilesIn"] + info["fastq"] + ["--outFileNamePrefix", prefix] + more


def test_flags(tmp_path, built):
    info = test_golden._tiny_info()
    sortedBam = ["--outSAMtype", "BAM", "SortedByCoordinate"]
    with pytest.raises(RuntimeError, match="--gpuSignal takes Host or Device"):
        capi.HostRun(_argv(info, str(tmp_path / "a_"), sortedBam + WIG + ["--gpuSignal", "device"]))
    with pytest.raises(RuntimeError, match="--gpuSignal Device computes the signal tracks of --outWigType"):
        capi.HostRun(_argv(info, str(tmp_path / "b_"), sortedBam + ["--gpuBAMsort", "Device", "--gpuSignal", "Device"]))
    with pytest.raises(RuntimeError, match="--gpuSignal Device reads the sorted records where --gpuBAMsort Device keeps them"):
        capi.HostRun(_argv(info, str(tmp_path / "c_"), sortedBam + WIG + ["--gpuSignal", "Device"]))
    with pytest.raises(RuntimeError, match="--gpuBAMsort Device does not work with --outWigType: the signal tracks read the sorted records on the host"):
        capi.HostRun(_argv(info, str(tmp_path / "d_"), sortedBam + WIG + ["--gpuBAMsort", "Device", "--gpuSignal", "Host"]))
    for ok in (sortedBam + WIG + ["--gpuSignal", "Host"], sortedBam + WIG + ["--gpuBAMsort", "Device", "--gpuSignal", "Device"]):
        r = capi.HostRun(_argv(info, str(tmp_path / "e_"), ok))
        assert r.signal_on_device() == ("Device" in ok)
        r.close()


def test_device_without_signal_functions_fails(runs, bz, tmp_path):
    with pytest.raises(RuntimeError, match="sah_set_signal_device"):
        run(runs["info"], str(tmp_path / "a_"), BASE + WIG + DEVICE, bz, None)
    assert "sah_set_signal_device" in G.tool_mode(runs["Host"][0] + SORTED, str(tmp_path / "b_"), WIG, device=True)


def test_tool_mode(runs, sg, tmp_path):
    """--runMode inputAlignmentsFromBAM on the run's sorted BAM: with --gpuSignal Device, without it, and the run's own tracks"""
    bam = runs["Host"][0] + SORTED
    sg.install()
    try:
        for k, flags in enumerate((WIG, ["--outWigType", "wiggle", "read1_5p", "--outWigStrand", "Unstranded", "--outWigNorm", "None", "--outWigReferencesPrefix", "chr1"])):
            host = G.tool_mode(bam, str(tmp_path / ("h%d_" % k)), flags)
            dev = G.tool_mode(bam, str(tmp_path / ("d%d_" % k)), flags, device=True)
            assert isinstance(host, dict) and len(host) == (4, 2)[k] and dev == host, k
            if k == 0:
                assert host == G.signal_files(runs["Host"][0])
    finally:
        capi.SignalDevice.uninstall()
