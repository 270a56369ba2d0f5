"""References added at the mapping stage (--genomeFastaFiles with alignReads, --outSAMfilter KeepOnlyAddedReferences | KeepAllAddedReferences) against
the reference binary, end to end on the CPU: the oracle maps, and the sequences are inserted by the device algorithm on the plain-loop backend
(star_amd/csrc/index/seq_core.h through tests/seq_insert_emul.cpp, installed with capi.device_seq_insertion); the gfx950 leg is
tests/test_gpu_seq_insert.py.  The data sets are prepare()'s se50 (plain index) and pe101 (annotated index).  Every test writes its own extra.fa -- two
spike-ins of about 1 kb with a shared tail of 40 bases, and a sequence that carries 300 bases of chr1, so that reads from there map to both places and
KeepAllAddedReferences has a primary flag to re-set -- and appends reads drawn from the added sequences to the FASTQ.  Compared: the @SQ lines and the
sorted body of Aligned.out.sam, SJ.out.tab, the counters of Log.final.out, and per flag set Unmapped.out.mate*, ReadsPerGene.out.tab, the five index files of
--sjdbInsertSave All, or the inflated sorted BAM."""
import os
import subprocess

import numpy as np
import pytest

from util import ROOT, _rc, _read_fasta, bam_parts, capi, compare_outputs, oracle_lib, prepare, refstar, run_with_engine

pytestmark = pytest.mark.skipif(not refstar.have_ref(), reason="oracle/_ref/STAR not built")
TWIN = os.path.join(ROOT, "oracle", "_build", "libseq_emul.so")
INDEX_FILES = ["sjdbInfo.txt", "sjdbList.out.tab", "Genome", "SA", "SAindex"]
WITHIN = ["--outSAMunmapped", "Within", "--outReadsUnmapped", "Fastx"]


@pytest.fixture(scope="module")
def twin(built):
    subprocess.check_call(["make", "-s", "oracle/_build/libseq_emul.so"], cwd=ROOT)
    return TWIN


def _oracle(g, p):
    return oracle_lib.Oracle(g, p)


def add_references(info, seed=5):
    """extra.fa, spike.gtf and the FASTQ files with reads from the added sequences appended, next to the data set's own files; returns a new info"""
    d = os.path.dirname(info["fastq"][0])
    rng = np.random.default_rng(seed)
    rnd = lambda n: "".join("ACGT"[x] for x in rng.integers(0, 4, n))
    chr1 = _read_fasta(info["fasta"])[0]
    tail = rnd(40)
    at = 20000
    while "N" in chr1[at:at + 300].upper():
        at += 1000
    seqs = [("spike1", rnd(1000) + tail), ("spike2", rnd(880) + tail), ("copy3", rnd(350) + chr1[at:at + 300].upper() + rnd(350))]
    fa = os.path.join(d, "extra.fa")
    with open(fa, "w") as f:
        for n, s in seqs:
            f.write(">%s\n" % n)
            for k in range(0, len(s), 70):
                f.write(s[k:k + 70] + "\n")
    gtf = os.path.join(d, "spike.gtf")                 # the data set's annotation plus one two-exon gene on spike1
    with open(gtf, "w") as f:
        f.write(open(info["gtf"]).read())
        for s, e in ((101, 400), (601, 900)):
            f.write('spike1\tsynth\texon\t%d\t%d\t.\t+\t.\tgene_id "gspike"; transcript_id "tspike";\n' % (s, e))
    L, paired = info["read_len"], info["paired"]
    recs = [[], []]
    k = 0
    for n, s in seqs:
        for _ in range(60):
            if paired:
                fl = int(rng.integers(L + 20, min(len(s), 3 * L)))
                p = int(rng.integers(0, len(s) - fl + 1))
                frag = s[p:p + fl]
                m = [frag[:L], _rc(frag[-L:])]
                if rng.random() < 0.5:
                    m = m[::-1]
            else:
                p = int(rng.integers(0, len(s) - L + 1))
                m = [s[p:p + L] if rng.random() < 0.5 else _rc(s[p:p + L])]
            for im, r in enumerate(m):
                recs[im].append("@x%s_%d\n%s\n+\n%s\n" % (n, k, r, "I" * len(r)))
            k += 1
    # a spliced read over the junction of the spike gene, and a pair of which only one mate lies on an added sequence (the other is random)
    sp = seqs[0][1]
    for j in range(10):
        a = L // 2 - j
        r = sp[400 - a:400] + sp[600:600 + (L - a)]
        if paired:
            recs[0].append("@xsj_%d\n%s\n+\n%s\n" % (j, r, "I" * L)); recs[1].append("@xsj_%d\n%s\n+\n%s\n" % (j, _rc(sp[700:700 + L]), "I" * L))
            recs[0].append("@xhalf_%d\n%s\n+\n%s\n" % (j, sp[50 + j:50 + j + L], "I" * L)); recs[1].append("@xhalf_%d\n%s\n+\n%s\n" % (j, rnd(L), "I" * L))
        else:
            recs[0].append("@xsj_%d\n%s\n+\n%s\n" % (j, r, "I" * L))
    fq = []
    for im, src in enumerate(info["fastq"]):
        dst = os.path.join(d, "reads_plus_%d.fq" % (im + 1))
        with open(dst, "w") as f:
            f.write(open(src).read())
            f.write("".join(recs[im]))
        fq.append(dst)
    out = dict(info)
    out["fastq"] = fq; out["extra_fa"] = fa; out["spike_gtf"] = gtf
    return out


def sq_lines(path):
    return [l for l in open(path, "rb") if l.startswith(b"@SQ")]


def run_both(info, tag, flags, factory):
    """the reference and the front end with `factory` behind it, same flags; returns (reference prefix, our prefix)"""
    d = os.path.dirname(info["fastq"][0])
    flags = ["--genomeFastaFiles", info["extra_fa"]] + list(flags)
    ref = refstar.align(info["idx"], info["fastq"], os.path.join(d, "ref_%s_" % tag), threads=1, extra=list(info["extra"]) + flags)
    mine = dict(info); mine["extra"] = list(info["extra"]) + flags
    new = run_with_engine(mine, os.path.join(d, "new_%s_" % tag), factory)
    return ref, new


def check_sam(ref, new, flags=()):
    problems = compare_outputs(ref, new)
    if sq_lines(ref + "Aligned.out.sam") != sq_lines(new + "Aligned.out.sam"):
        problems.append("@SQ lines differ")
    if not any(b"spike1" in l for l in sq_lines(new + "Aligned.out.sam")):
        problems.append("no @SQ line of an added sequence")
    if "--outReadsUnmapped" in flags:
        for m in (1, 2):
            p = "Unmapped.out.mate%d" % m
            if os.path.exists(ref + p) and open(ref + p, "rb").read() != open(new + p, "rb").read():
                problems.append(p + " differs")
    return problems


def records(prefix):
    return [l.split(b"\t") for l in open(prefix + "Aligned.out.sam", "rb") if not l.startswith(b"@")]


FLAG_SETS = {
    "none": [],
    "keep_only": ["--outSAMfilter", "KeepOnlyAddedReferences"],
    "keep_all": ["--outSAMfilter", "KeepAllAddedReferences"],
    "keep_only_within": ["--outSAMfilter", "KeepOnlyAddedReferences"] + WITHIN,
    "keep_all_within": ["--outSAMfilter", "KeepAllAddedReferences"] + WITHIN,
}


@pytest.mark.parametrize("name", ["se50", "pe101"])
@pytest.mark.parametrize("tag", list(FLAG_SETS))
def test_added_references(name, tag, tmp_path, twin):
    info = add_references(prepare(name, str(tmp_path), need_ref=False))
    with capi.device_seq_insertion(twin, "seq_emul_insert"):
        ref, new = run_both(info, tag, FLAG_SETS[tag], _oracle)
    assert not check_sam(ref, new, FLAG_SETS[tag])
    recs = records(new)
    added = {b"spike1", b"spike2", b"copy3"}
    assert any(r[2] in added for r in recs)
    if tag.startswith("keep"):
        assert all(r[2] in added or (int(r[1]) & 4) for r in recs)
    if tag == "keep_all":                           # reads of the copied 300 bases: one of two alignments survives, as NH:i:1 and primary
        one = [r for r in recs if r[0].startswith(b"xcopy3") and b"NH:i:1" in r and not (int(r[1]) & 256)]
        assert one and [r for r in records(ref) if r[0].startswith(b"xcopy3")]
    if tag == "none":
        assert any(r[0].startswith(b"xcopy3") and b"NH:i:2" in r for r in recs)


def test_two_pass_with_added_references(tmp_path, twin):
    """--twopassMode Basic: the junctions of the 1st pass (the spike gene's among them) are inserted into the index that holds the added sequences;
    --sjdbInsertSave All leaves that index in _STARgenome/, byte for byte the reference's"""
    info = add_references(prepare("pe101", str(tmp_path), need_ref=False))
    with capi.device_seq_insertion(twin, "seq_emul_insert"):
        ref, new = run_both(info, "2p", ["--twopassMode", "Basic", "--sjdbInsertSave", "All"], _oracle)
    problems = check_sam(ref, new)
    for f in INDEX_FILES:
        if open(ref + "_STARgenome/" + f, "rb").read() != open(new + "_STARgenome/" + f, "rb").read():
            problems.append("_STARgenome/%s differs" % f)
    if open(ref + "_STARpass1/SJ.out.tab", "rb").read() != open(new + "_STARpass1/SJ.out.tab", "rb").read():
        problems.append("_STARpass1/SJ.out.tab differs")
    assert not problems, problems
    assert any(l.startswith("spike1\t") for l in open(new + "SJ.out.tab"))


def test_saved_index_with_added_references(tmp_path, twin):
    """--sjdbInsertSave All on a plain index, with a junction ON an added sequence (--sjdbFileChrStartEnd): the five files are the reference's bytes; the
    chromosome tables are those of the NEW index (the reference copies the old ones)"""
    info = add_references(prepare("se50", str(tmp_path), need_ref=False))
    sj = os.path.join(os.path.dirname(info["fastq"][0]), "sj.tab")
    with open(sj, "w") as f:
        f.write("spike1\t401\t600\t+\nchr1\t30001\t30400\t-\n")
    with capi.device_seq_insertion(twin, "seq_emul_insert"):
        ref, new = run_both(info, "save", ["--sjdbFileChrStartEnd", sj, "--sjdbInsertSave", "All"], _oracle)
    problems = check_sam(ref, new)
    for f in INDEX_FILES:
        if open(ref + "_STARgenome/" + f, "rb").read() != open(new + "_STARgenome/" + f, "rb").read():
            problems.append("_STARgenome/%s differs" % f)
    assert not problems, problems
    names = open(new + "_STARgenome/chrName.txt").read().split()
    assert names[-3:] == ["spike1", "spike2", "copy3"]
    starts = [int(x) for x in open(new + "_STARgenome/chrStart.txt").read().split()]
    assert len(starts) == len(names) + 1 and os.path.getsize(new + "_STARgenome/Genome") > starts[-1]
    log = open(new + "Log.out").read()
    assert "inserting extra sequences into genome indexes" in log and "number of new SA indices = " in log and "Finished inserting SA indices" in log


def test_gtf_and_gene_counts_with_added_references(tmp_path, twin):
    """--sjdbGTFfile at the mapping stage with a gene on an added sequence, --quantMode GeneCounts"""
    info = add_references(prepare("se50", str(tmp_path), need_ref=False))
    with capi.device_seq_insertion(twin, "seq_emul_insert"):
        ref, new = run_both(info, "gtf", ["--sjdbGTFfile", info["spike_gtf"], "--quantMode", "GeneCounts"], _oracle)
    problems = check_sam(ref, new)
    if open(ref + "ReadsPerGene.out.tab", "rb").read() != open(new + "ReadsPerGene.out.tab", "rb").read():
        problems.append("ReadsPerGene.out.tab differs")
    assert not problems, problems
    counts = {l.split("\t")[0]: int(l.split("\t")[1]) for l in open(new + "ReadsPerGene.out.tab")}
    assert counts["gspike"] > 0


def test_sorted_bam_keep_all(tmp_path, twin):
    """--outSAMtype BAM SortedByCoordinate with KeepAllAddedReferences: header, reference block and records after inflation"""
    info = add_references(prepare("pe101", str(tmp_path), need_ref=False))
    with capi.device_seq_insertion(twin, "seq_emul_insert"):
        ref, new = run_both(info, "bam", ["--outSAMtype", "BAM", "SortedByCoordinate", "--outSAMfilter", "KeepAllAddedReferences", "--outSAMunmapped", "Within"], _oracle)
    rt, rb, rr = bam_parts(ref + "Aligned.sortedByCoord.out.bam")
    nt, nb, nr = bam_parts(new + "Aligned.sortedByCoord.out.bam")
    assert [l for l in rt.split(b"\n") if l.startswith(b"@SQ")] == [l for l in nt.split(b"\n") if l.startswith(b"@SQ")]
    assert rb == nb and b"spike1" in nb
    assert rr == nr and len(nr) > 0
    assert refstar.final_log_counters(ref + "Log.final.out") == refstar.final_log_counters(new + "Log.final.out")


def test_errors(tmp_path, twin):
    info = add_references(prepare("se50", str(tmp_path), need_ref=False))
    base = ["--genomeDir", info["idx"], "--readFilesIn"] + info["fastq"] + ["--outFileNamePrefix", str(tmp_path / "e_")]
    notfa = str(tmp_path / "not.fa")
    with open(notfa, "w") as f:
        f.write("ACGT\n")
    cases = [(["--outSAMfilter", "KeepOnlyAddedReferences"], "options can only be used if references are added on-the-fly with --genomeFastaFiles"),
             (["--outSAMfilter", "KeepAllAddedReferences"], "options can only be used if references are added on-the-fly with --genomeFastaFiles"),
             (["--genomeFastaFiles", info["extra_fa"], "--outSAMfilter", "KeepSome"], "unknown/unimplemented value for --outSAMfilter: KeepSome"),
             (["--genomeFastaFiles", str(tmp_path / "missing.fa")], "could not open genomeFastaFile: " + str(tmp_path / "missing.fa")),
             (["--genomeFastaFiles", notfa], "is not fasta: the first character is 'A' (65), not '>'"),
             (["--genomeFastaFiles", info["extra_fa"], "--genomeLoad", "LoadAndKeep"], "--genomeFastaFiles at the mapping stage is not compatible with genomeLoad shared memory options")]
    with capi.device_seq_insertion(twin, "seq_emul_insert"):
        for extra, text in cases:
            with pytest.raises(RuntimeError) as e:
                capi.HostRun(base + extra)
            assert text in str(e.value), (extra, str(e.value))
    with pytest.raises(RuntimeError) as e:               # no insertion function installed: there is no host restatement to fall back to
        capi.HostRun(base + ["--genomeFastaFiles", info["extra_fa"]])
    assert "no sequence insertion function is installed (sah_set_seq_insert_fn)" in str(e.value)
    run = capi.HostRun(base + ["--genomeFastaFiles", "-", "--outSAMfilter", "None"])      # the defaults, spelled out
    run.close()
