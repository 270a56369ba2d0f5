"""--gpuSignal Device on the MI355X: the shipped library (k_signal.hip in libstaramd.so) gives, on every vector of tests/test_signal_emul.py and every
option combination, the bytes of the host path computed here (writeSignal through the tool mode) -- by the host-records entry and through the sorter;
one run with more occupied tiles than k_signal_tiles has workgroups; the shipped binary on the golden tiny_pe set, Device / Device / Device against
Host / Host.  Every GPU step is a child process under a time limit of its own."""
import os
import pickle
import subprocess
import sys

import pytest

from util import ROOT, bam_parts
import test_bgzf_emul as E
import test_golden
import test_signal_emul as G

pytestmark = pytest.mark.gpu
RUN = os.path.join(ROOT, "tests", "signal_gpu_run.py")
BIN = os.path.join(ROOT, "star_amd", "bin", "star_amd")
SORTED = "Aligned.sortedByCoord.out.bam"


def _child(args, timeout):
    p = subprocess.run([sys.executable, RUN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-4000:]


def test_shipped_library_on_the_vectors(tmp_path, built):
    import signal_gpu_run as R
    dev = tmp_path / "dev"
    dev.mkdir()
    op = str(tmp_path / "out.pkl")
    _child(["lib", str(dev), op], timeout=300)
    got = pickle.load(open(op, "rb"))
    assert got["constants"] == (G.T, G.CH)
    work = str(tmp_path)
    n = 0
    for name in G.VECTOR_NAMES:
        for opt, prefix in R.cases(name):
            want = G.host_expected(work, name, G.wig_flags(*opt, prefix=prefix))
            assert got[("tool", name, opt, prefix)] == want, (name, opt, prefix)
            n += 1
        for opt in R.SORTER_OPTS:
            files, out = got[("sorter", name, opt)]
            assert files == G.host_expected(work, name, G.wig_flags(*opt)), (name, opt)
            assert b"".join(x for x, _ in E.members(out)) == b"".join(G.vectors()[name]), name
    assert n > 100 and G.host_expected(work, "past_end", G.wig_flags("bg", 1, 1, 0)) == G.BUG


def test_more_tiles_than_workgroups(tmp_path, built):
    """test_signal_emul.many_vector(): ~2850 occupied tiles for 8 workgroups per CU"""
    bam = G.write_bam(str(tmp_path / "many.bam"), G.many_vector(), G.MANY_CHROMS)
    flags = G.wig_flags("bg", 1, 1, 0)
    want = G.tool_mode(bam, str(tmp_path / "h_"), flags)
    op = str(tmp_path / "many.pkl")
    _child(["many", bam, str(tmp_path / "d_"), op], timeout=300)
    res = pickle.load(open(op, "rb"))
    assert res["cus"] >= 32, "not the CU count of a GPU"
    tiles = {int(l.split(b"\t")[1]) // G.T for l in want["Signal.UniqueMultiple.str1.out.bg"].splitlines() if l.startswith(b"big")}
    assert len(tiles) > 8 * res["cus"], (len(tiles), res["cus"])
    assert isinstance(want, dict) and res["files"] == want
    assert sum(len(x) for x in want.values()) > 1000000


def _binary(info, prefix, more, timeout=600):
    p = subprocess.run([BIN, "--genomeDir", info["idx"], "--readFilesIn"] + info["fastq"] + ["--outFileNamePrefix", prefix] + list(info.get("extra", [])) + more,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    return prefix


@pytest.mark.parametrize("wig", [["--outWigType", "bedGraph"], ["--outWigType", "wiggle", "read1_5p", "--outWigStrand", "Unstranded", "--outWigNorm", "None"]])
def test_shipped_binary_tiny(tmp_path, wig):
    """the golden data set (needs no reference binary): everything on the device against sort and signal on the host, and the tool mode on the result"""
    info = test_golden._tiny_info()
    base = ["--outSAMtype", "BAM", "SortedByCoordinate", "--outSAMunmapped", "Within", "KeepPairs", "--runThreadN", "4", "--gpuBatchReads", "300"] + wig
    host = _binary(info, str(tmp_path / "host_"), base)
    dev = _binary(info, str(tmp_path / "dev_"), base + ["--gpuBAMcompression", "Device", "--gpuBAMsort", "Device", "--gpuSignal", "Device"])
    want = G.signal_files(host)
    assert len(want) == (2 if "Unstranded" in wig else 4) and sum(len(x) for x in want.values()) > 1000    # (the tracks are not empty)
    assert G.signal_files(dev) == want
    (th, bh, rh), (td, bd, rd) = bam_parts(host + SORTED), bam_parts(dev + SORTED)
    assert rd == rh and bd == bh
    log = open(dev + "Log.out").read()
    assert "--gpuSignal Device: %d records" % len(rd) in log
    p = subprocess.run([BIN, "--runMode", "inputAlignmentsFromBAM", "--inputBAMfile", dev + SORTED, "--outFileNamePrefix", str(tmp_path / "tool_"), "--gpuSignal", "Device"] + wig,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert G.signal_files(str(tmp_path / "tool_")) == want
