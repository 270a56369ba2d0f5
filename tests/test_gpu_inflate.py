"""--gpuBAMinflate Device on the MI355X: the shipped library (k_inflate.hip in libstaramd.so) on every vector of tests/inflate_vectors.py, well-formed and
malformed, with the expectations of the CPU tests (zlib's bytes; the status and the member) -- the malformed ones go to the GPU only behind the bounds
gate of tests/test_inflate_bounds.py --; one file of 3 x (grid cap) + 5 members of seven kinds on a grid so small that the loop turns and every wavefront
meets several kinds; the shipped binary on a tiny sorted BAM, everything on the device against everything on the host.  Every GPU step is a child
process under a time limit of its own."""
import os
import pickle
import subprocess
import sys

import pytest

from util import ROOT, bam_parts
import inflate_vectors as V
import test_inflate_emul as E
import test_signal_emul as G
import test_golden

pytestmark = pytest.mark.gpu
RUN = os.path.join(ROOT, "tests", "inflate_gpu_run.py")
BIN = os.path.join(ROOT, "star_amd", "bin", "star_amd")
SORTED = "Aligned.sortedByCoord.out.bam"


def _child(args, timeout):
    p = subprocess.run([sys.executable, RUN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-4000:]


def test_shipped_library_on_the_vectors(tmp_path, built):
    op = str(tmp_path / "out.pkl")
    _child(["lib", op], timeout=300)
    got = pickle.load(open(op, "rb"))
    assert got["constants"] == (256, 4, 8, 0)
    for name, (f, datas) in V.wellformed().items():
        V.check_wellformed(name, f, datas)
        E.expect_wellformed(got[("well", name)], f, datas, name)
    for name, (f, member, status) in list(V.malformed().items()) + list(V.lenient().items()):
        assert got[("bad", name)] == (None, member, status), (name, got[("bad", name)])
    for name, (f, piece) in V.not_bgzf().items():
        assert piece in got[("not", name)] and "--gpuBAMinflate Host" in got[("not", name)], (name, got[("not", name)])


def test_more_members_than_one_sweep(tmp_path, built):
    """The default cap of 8 workgroups per CU is thousands of members on an MI355X, far above any test file: this run, with STARAMD_INFLATE_MAX_WORKGROUPS=6,
    is the one in which the grid-stride loop turns on the hardware.  24 members a sweep, seven kinds in turn: a wavefront's members are 24 apart, and 24 mod 7
    = 3, so it meets three kinds at least."""
    import inflate_gpu_run as R
    op = str(tmp_path / "sweep.pkl")
    _child(["sweep", op], timeout=300)
    got = pickle.load(open(op, "rb"))
    assert got["cus"] >= 32, "not the CU count of a GPU"
    assert got["cap"] == R.SWEEP_WORKGROUPS * 4 and got["n"] == 3 * got["cap"] + 5
    ms = E.many_members(got["n"])
    want = [E.zdata(m) for m in ms]
    assert len({len(w) for w in want[:7]}) >= 6 and want[2] == b""
    assert got["before"] == want and got["after"] == want
    out, failed, status, n, stats = got["all"]
    assert (failed, status, n) == (-1, "OK", len(ms)) and out == b"".join(want)
    assert stats[3] > 0 and stats[4] > 0


def _binary(args, timeout=600):
    p = subprocess.run([BIN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]


def test_shipped_binary_tiny(tmp_path):
    """the golden data set (needs no reference binary), aligned and sorted; then the tool mode with all of inflate, dedup and compression on the device
    against all on the host, and the signal tracks of --gpuSignal Device with both forms of inflate"""
    info = test_golden._tiny_info()
    al = str(tmp_path / "al_")
    _binary(["--genomeDir", info["idx"], "--readFilesIn"] + list(info["fastq"]) + ["--outFileNamePrefix", al, "--outSAMtype", "BAM", "SortedByCoordinate", "--runThreadN", "4", "--gpuBatchReads", "300"])
    tool = ["--runMode", "inputAlignmentsFromBAM", "--inputBAMfile", al + SORTED, "--runThreadN", "4"]
    outs = {}
    for tag, where in (("host", "Host"), ("dev", "Device")):
        prefix = str(tmp_path / (tag + "_"))
        _binary(tool + ["--outFileNamePrefix", prefix, "--bamRemoveDuplicatesType", "UniqueIdentical", "--gpuBAMinflate", where, "--gpuBAMdedup", where, "--gpuBAMcompression", where], timeout=300)
        outs[tag] = bam_parts(prefix + "Processed.out.bam")
    assert outs["host"] == outs["dev"] and len(outs["dev"][2]) > 100
    raw = open(al + SORTED, "rb").read()
    ms = V.members_of(raw)
    log = open(str(tmp_path / "dev_Log.out")).read()
    assert "--inputBAMfile inflated on the Device (--gpuBAMinflate): %d members, %d bytes in, %d bytes out\n" % (len(ms), len(raw), sum(m[2] for m in ms)) in log
    assert "inflated on the Host (--gpuBAMinflate)" in open(str(tmp_path / "host_Log.out")).read()
    sig = {}
    for tag, where in (("sh", "Host"), ("sd", "Device")):
        prefix = str(tmp_path / (tag + "_"))
        _binary(tool + ["--outFileNamePrefix", prefix, "--outWigType", "bedGraph", "--gpuSignal", "Device", "--gpuBAMinflate", where], timeout=300)
        sig[tag] = G.signal_files(prefix)
    assert sig["sh"] == sig["sd"] and len(sig["sd"]) == 4 and any(sig["sd"].values())
