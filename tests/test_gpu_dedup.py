"""--gpuBAMdedup Device on the MI355X: the shipped library (k_dedup.hip in libstaramd.so) gives, on every vector of tests/test_dedup_emul.py and every
option set, the bytes and counts of the host path computed here, and the flag words whose digests the reference left in tests/golden/dedup_ref_flags.json
-- with whole hashes and with STARAMD_DEDUP_HASH_BITS=3; `many` and `deep` once more with a grid so small that every loop turns; the shipped binary on the
golden tiny_pe set with every read pair twice: Host, Device, and Device with the device compressor write one file.  Every GPU step is a child process
under a time limit of its own."""
import json
import os
import pickle
import subprocess
import sys

import pytest

from util import ROOT, capi, bam_parts
import test_dedup as T
import test_dedup_emul as D
import test_golden

pytestmark = pytest.mark.gpu
RUN = os.path.join(ROOT, "tests", "dedup_gpu_run.py")
BIN = os.path.join(ROOT, "star_amd", "bin", "star_amd")
SORTED = "Aligned.sortedByCoord.out.bam"


def _child(args, timeout):
    p = subprocess.run([sys.executable, RUN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-4000:]


@pytest.mark.parametrize("bits", ["-", "3"])
def test_shipped_library_on_the_vectors(tmp_path, built, bits):
    op = str(tmp_path / "out.pkl")
    _child(["lib", op, bits], timeout=300)
    got = pickle.load(open(op, "rb"))
    assert got["constants"] == (256, 16, 0)
    golden = json.load(open(T.GOLDEN))
    n = 0
    for name, recs in D.vectors().items():
        for opt in D.options(name):
            want = D.result_of(capi.dedup_host(recs, *opt))
            assert got[(name, opt)] == want, (name, opt, bits)
            if name in D.IN_DOMAIN:
                assert T.flag_digest(D.apply_bits(recs, want[0])) == golden[name][T.opt_tag(opt)], (name, opt)
            n += 1
    assert n > 70


def test_more_classes_and_name_runs_than_one_sweep(tmp_path, built):
    """`many`: 20 000 name runs and ~13 400 classes; `deep`: one class of 5 000 pairs -- on a grid of 8 workgroups.  The assertion that classes and name
    runs exceed workgroups x tile holds only because the child sets STARAMD_DEDUP_MAX_WORKGROUPS=8: the default cap of 16 workgroups per CU x 256
    work-items is about a million items on an MI355X, far above these vectors, so with the default geometry (the test above) no grid-stride loop
    turns; this run is the one in which they do on the hardware."""
    import dedup_gpu_run as R
    op = str(tmp_path / "sweep.pkl")
    _child(["sweep", op], timeout=300)
    got = pickle.load(open(op, "rb"))
    assert got["cus"] >= 32, "not the CU count of a GPU"
    assert got["workgroups"] == R.SWEEP_WORKGROUPS and got["tile"] == 256
    for name in ("many", "deep"):
        for opt in D.OPTION_SETS:
            want = D.result_of(capi.dedup_host(D.vectors()[name], *opt))
            assert got[(name, opt)] == want, (name, opt)
    st = D.expected("many", D.OPTION_SETS[0])[1]
    assert st[3] > got["workgroups"] * got["tile"] and st[2] > got["workgroups"] * got["tile"], (st, got["workgroups"], got["tile"])      # classes, name runs (= pairs)
    assert D.expected("deep", D.OPTION_SETS[0])[1][4] == 2 * 4999


def _binary(args, timeout=600):
    p = subprocess.run([BIN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]


def test_shipped_binary_tiny(tmp_path):
    """the golden data set (needs no reference binary) with every pair twice, the copy under another name: aligned and sorted, then marked three ways"""
    info = test_golden._tiny_info()
    fq = []
    for k, src in enumerate(info["fastq"]):
        lines = open(src).read().splitlines()
        twice = list(lines)
        for i in range(0, len(lines), 4):
            head = lines[i].split()
            nm = head[0][:-2] + "_d" + head[0][-2:] if head[0].endswith(("/1", "/2")) else head[0] + "_d"
            twice += [" ".join([nm] + head[1:])] + lines[i + 1:i + 4]
        fq.append(str(tmp_path / ("twice_%d.fq" % (k + 1))))
        open(fq[-1], "w").write("\n".join(twice) + "\n")
    al = str(tmp_path / "al_")
    _binary(["--genomeDir", info["idx"], "--readFilesIn"] + fq + ["--outFileNamePrefix", al, "--outSAMtype", "BAM", "SortedByCoordinate", "--outSAMunmapped", "Within", "KeepPairs",
             "--runThreadN", "4", "--gpuBatchReads", "300"])
    text, refs, recs = bam_parts(al + SORTED)
    outs = {}
    for tag, more in (("host", ["--gpuBAMdedup", "Host"]), ("dev", ["--gpuBAMdedup", "Device"]), ("devz", ["--gpuBAMdedup", "Device", "--gpuBAMcompression", "Device"])):
        prefix = str(tmp_path / (tag + "_"))
        _binary(["--runMode", "inputAlignmentsFromBAM", "--inputBAMfile", al + SORTED, "--outFileNamePrefix", prefix, "--bamRemoveDuplicatesType", "UniqueIdentical", "--runThreadN", "4"] + more, timeout=300)
        outs[tag] = bam_parts(prefix + "Processed.out.bam")
    assert outs["host"] == outs["dev"] == outs["devz"]
    bits, st = D.restate(recs, True, 0)
    assert outs["dev"] == (text, refs, D.apply_bits(recs, bits))
    assert st[4] > 100 and st[2] > 100, st
    log = open(str(tmp_path / "dev_Log.out")).read()
    assert "on the Device (--gpuBAMdedup): %d records, %d pairs, %d classes, %d records marked, %d unpaired unique records" % (st[0], st[2], st[3], st[4], st[5]) in log
