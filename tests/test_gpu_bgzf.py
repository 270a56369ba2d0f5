"""--gpuBAMcompression Device on the MI355X: the shipped compressor (k_bgzf.hip in libstaramd.so) makes the same bytes as the wave emulator's
build of the same source (tests/test_bgzf_emul.py), alone and from 4 threads at once; a call of three times as many blocks as the kernel has
workgroups equals its blocks compressed one per call; whole runs with the BAM records compressed on the device
decompress to exactly what the Host path and the reference write.  Every GPU step is a child process under a time limit of its own."""
import os
import pickle
import subprocess
import sys

import pytest

from util import ROOT, bam_parts, capi, prepare, refstar
import test_bgzf_emul as E
import test_golden

pytestmark = pytest.mark.gpu
RUN = os.path.join(ROOT, "tests", "bgzf_gpu_run.py")
BIN = os.path.join(ROOT, "star_amd", "bin", "star_amd")


def _child(args, timeout):
    p = subprocess.run([sys.executable, RUN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-4000:]


def test_shipped_library_matches_emulator(tmp_path, built):
    vecs = E.synthetic_vectors()
    vecs["tiny_bam"] = [E.bam_stream(test_golden._tiny_info(), str(tmp_path), "tiny")]
    vp, op = str(tmp_path / "vec.pkl"), str(tmp_path / "out.pkl")
    pickle.dump(vecs, open(vp, "wb"))
    _child(["lib", vp, op], timeout=300)
    got = pickle.load(open(op, "rb"))
    emu = capi.BgzfDevice(lib_path=E.emul_lib())
    try:
        for lv in E.LEVELS:
            for k, segs in vecs.items():
                want = emu.compress(lv, segs)
                E.check(segs, want, lv)
                assert got["single"][(lv, k)] == want, (lv, k)
                for i in range(4):
                    assert got["threads"][(i, lv, k)] == want, (i, lv, k)
    finally:
        emu.close()


def test_more_blocks_than_workgroups(tmp_path, built):
    """the block loop of a workgroup beyond its first trip (LDS, V[] and the scratch slice left by the block before), and the handle's buffers
    growing between calls: every member of the large call equals the same content compressed alone, and inflates to it"""
    op = str(tmp_path / "many.pkl")
    _child(["many", op], timeout=600)
    res = pickle.load(open(op, "rb"))
    print("many: %d workgroups, %d blocks, %.1f MB per call; the large calls took %s s" % (res["grid"], res["nb"], res["bytes"] / 1e6, ", ".join("%.2f" % res[lv][3] for lv in (1, 6, 0))))
    assert res["grid"] >= 64, "not the workgroup count of a GPU"
    E.check_many(res)


EOF_MARK = E.EOF_MARK
CASES = [("pe150_chim", ["--outSAMtype", "BAM", "Unsorted", "--outSAMattributes", "All", "--outSAMunmapped", "Within", "--runThreadN", "3"], 4096),
         ("pe150_indel", ["--outSAMtype", "BAM", "Unsorted", "SortedByCoordinate", "--outSAMunmapped", "Within", "KeepPairs"], 4096),
         ("pe101", ["--quantMode", "TranscriptomeSAM", "--outSAMtype", "BAM", "Unsorted"], 4096),
         ("pe101", ["--outSAMtype", "BAM", "Unsorted", "SortedByCoordinate", "--runThreadN", "4"], 700)]


@pytest.mark.skipif(not refstar.have_ref(), reason="oracle/_ref/STAR not built")
@pytest.mark.parametrize("name,more,batch", CASES)
def test_device_bam_end_to_end(name, more, batch, tmp_path, built):
    info = dict(prepare(name, str(tmp_path), need_ref=False))
    d = os.path.dirname(info["fastq"][0])
    info["extra"] = list(info["extra"]) + more
    rf = list(info["extra"])
    if "--runThreadN" in rf:
        k = rf.index("--runThreadN"); del rf[k:k + 2]
    ref = refstar.align(info["idx"], info["fastq"], os.path.join(d, "ref_"), threads=1, extra=rf)
    out = {}
    for mode in ("Host", "Device"):
        i2 = dict(info)
        i2["extra"] = info["extra"] + ["--gpuBAMcompression", mode]
        ip = os.path.join(d, mode + ".pkl")
        pickle.dump(i2, open(ip, "wb"))
        out[mode] = os.path.join(d, mode + "_")
        _child(["run", ip, out[mode], mode, str(batch)], timeout=600)
    files = [f for f in ("Aligned.out.bam", "Aligned.sortedByCoord.out.bam", "Aligned.toTranscriptome.out.bam") if os.path.exists(ref + f)]
    assert files
    keep = lambda t: [l for l in t.split(b"\n") if not l.startswith((b"@PG", b"@CO"))]
    for f in files:
        dev, host = open(out["Device"] + f, "rb").read(), open(out["Host"] + f, "rb").read()
        assert dev[-28:] == EOF_MARK, f
        assert E.same_bam(out["Device"] + f, out["Host"] + f), f
        (ta, ra, rr), (tb, rb, nr) = bam_parts(ref + f), bam_parts(out["Device"] + f)
        assert ra == rb and len(rr) == len(nr) and rr == nr, f
        assert keep(ta) == keep(tb), f


def test_shipped_binary_device_mode(tmp_path, built):
    """star_amd/bin/star_amd --gpuBAMcompression Device on the golden data set: the decompressed BAM files equal a Host run of the same binary"""
    info = test_golden._tiny_info()
    outs = {}
    for mode in ("Host", "Device"):
        outs[mode] = str(tmp_path / mode) + "_"
        p = subprocess.run([BIN, "--genomeDir", info["idx"], "--readFilesIn"] + info["fastq"] + ["--outFileNamePrefix", outs[mode], "--outSAMtype", "BAM", "Unsorted",
                            "SortedByCoordinate", "--outSAMunmapped", "Within", "--runThreadN", "4", "--gpuBAMcompression", mode],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-3000:]
    for f in ("Aligned.out.bam", "Aligned.sortedByCoord.out.bam"):
        dev, host = open(outs["Device"] + f, "rb").read(), open(outs["Host"] + f, "rb").read()
        assert dev[-28:] == EOF_MARK
        assert E.same_bam(outs["Device"] + f, outs["Host"] + f), f
        assert dev != host
