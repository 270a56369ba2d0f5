"""References added at the mapping stage on the MI355X: the flag sets of tests/test_seq_insert.py with the HIP engine mapping and staramd_seq_insert
(star_amd/csrc/index/seq_core.h on HipBackend) inserting, against the reference binary; the shipped front end with two contexts on the one GPU, and with the
sorted BAM ordered on the device behind the filter.  Reads only oracle/_ref/STAR and what prepare() makes."""
import os
import subprocess

import pytest

import test_seq_insert as T
from util import ROOT, bam_parts, capi, prepare, refstar

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not refstar.have_ref(), reason="oracle/_ref/STAR not built")]
BIN = os.path.join(ROOT, "star_amd", "bin", "star_amd")


def _engine(g, p):
    return capi.Engine(g, p, device=0, max_reads=4096)


@pytest.mark.parametrize("tag", ["none", "keep_only", "keep_all", "keep_all_within"])
def test_added_references_on_the_engine(tag, tmp_path, built):
    info = T.add_references(prepare("se50", str(tmp_path), need_ref=False))
    with capi.device_seq_insertion():
        ref, new = T.run_both(info, tag, T.FLAG_SETS[tag], _engine)
    assert not T.check_sam(ref, new, T.FLAG_SETS[tag])
    assert any(r[2] in (b"spike1", b"spike2", b"copy3") for r in T.records(new))


def test_keep_only_within_paired_on_the_engine(tmp_path, built):
    info = T.add_references(prepare("pe101", str(tmp_path), need_ref=False))
    with capi.device_seq_insertion():
        ref, new = T.run_both(info, "kow", T.FLAG_SETS["keep_only_within"], _engine)
    assert not T.check_sam(ref, new, T.FLAG_SETS["keep_only_within"])


def test_saved_index_on_the_engine(tmp_path, built):
    info = T.add_references(prepare("se50", str(tmp_path), need_ref=False))
    sj = os.path.join(os.path.dirname(info["fastq"][0]), "sj.tab")
    with open(sj, "w") as f:
        f.write("spike1\t401\t600\t+\nchr1\t30001\t30400\t-\n")
    with capi.device_seq_insertion(), capi.device_sjdb_insertion():
        ref, new = T.run_both(info, "save", ["--sjdbFileChrStartEnd", sj, "--sjdbInsertSave", "All"], _engine)
    problems = T.check_sam(ref, new)
    for f in T.INDEX_FILES:
        if open(ref + "_STARgenome/" + f, "rb").read() != open(new + "_STARgenome/" + f, "rb").read():
            problems.append("_STARgenome/%s differs" % f)
    assert not problems, problems


def _binary(info, prefix, more, timeout=300):
    p = subprocess.run([BIN, "--genomeDir", info["idx"], "--readFilesIn"] + info["fastq"] + ["--outFileNamePrefix", prefix, "--genomeFastaFiles", info["extra_fa"]] + list(info.get("extra", [])) + more,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    return prefix


def test_binary_two_contexts(tmp_path, built):
    """the shipped front end installs staramd_seq_insert itself; --gpuDevices 0,0: the insertion runs once, both contexts upload its result"""
    info = T.add_references(prepare("pe101", str(tmp_path), need_ref=False))
    d = os.path.dirname(info["fastq"][0])
    flags = ["--outSAMfilter", "KeepOnlyAddedReferences", "--twopassMode", "Basic"]
    ref = refstar.align(info["idx"], info["fastq"], os.path.join(d, "ref2c_"), threads=1, extra=list(info["extra"]) + ["--genomeFastaFiles", info["extra_fa"]] + flags)
    new = _binary(info, os.path.join(d, "new2c_"), flags + ["--gpuDevices", "0,0"])
    assert not T.check_sam(ref, new)
    log = open(new + "Log.out").read()
    assert "inserting extra sequences into genome indexes" in log and "Finished inserting SA indices" in log


def test_binary_sorted_bam_on_the_device_behind_the_filter(tmp_path, built):
    info = T.add_references(prepare("pe101", str(tmp_path), need_ref=False))
    d = os.path.dirname(info["fastq"][0])
    flags = ["--outSAMtype", "BAM", "SortedByCoordinate", "--outSAMfilter", "KeepAllAddedReferences", "--outSAMunmapped", "Within"]
    ref = refstar.align(info["idx"], info["fastq"], os.path.join(d, "refbs_"), threads=1, extra=list(info["extra"]) + ["--genomeFastaFiles", info["extra_fa"]] + flags)
    new = _binary(info, os.path.join(d, "newbs_"), flags + ["--gpuBAMsort", "Device"])
    (rt, rb, rr), (nt, nb, nr) = bam_parts(ref + "Aligned.sortedByCoord.out.bam"), bam_parts(new + "Aligned.sortedByCoord.out.bam")
    assert rb == nb and b"spike1" in nb and rr == nr and len(nr) > 0
    assert "ordered on the device" in open(new + "Log.out").read()
