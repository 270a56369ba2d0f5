"""Writes tests/golden/seq_insert/<case>/: synthetic genomes of a few kb plus extra sequences that the REFERENCE binary (oracle/_ref/STAR) adds at the
mapping stage (--genomeFastaFiles extra.fa).  Kept per case: our inputs genome.fa, extra.fa, annot.gtf, sj_new.tab, sj_old.tab, and for each of two forms

    plain/   a plain index; the mapping run also inserts ONE new junction (sj_new.tab)
    annot/   an index generated with annot.gtf; the mapping run inserts a junction the index already has (sj_old.tab): the junction insertion adds
             nothing, so the saved arrays are the sequence insertion alone, with the junction block moved behind the added text

    <form>/old/{Genome,SA,SAindex,chrStart.txt,genomeParameters.txt}      the index before the run (the reference's genomeGenerate)
    <form>/new/{Genome,SA,SAindex,sjdbInfo.txt,sjdbList.out.tab}          _STARgenome/ of the mapping run with --sjdbInsertSave All

tests/seq_insert_check.cpp and tests/seq_insert_gpu.hip hold the restated insertSeqSA and the product's seqInsertHost (+ sjdbInsertHost) to these
bytes, without the reference being present.

    python tests/golden/make_seq_insert_golden.py     (needs oracle/_ref/STAR; the committed files were made this way and are not rewritten by tests)

Every case: --genomeChrBinNbits 8.
  tails   two added sequences with the same last 40 bases and different lengths, a third that shares 200 bases with a chromosome: the suffixes that
          tie up to their spacer come out in another order than genomeGenerate gives them; one more that begins and ends with the flanks of an
          annotated junction (ties with entries of the junction block).  nSA after the sequence insertion = 0 mod 64
  dups    two identical added sequences, a 200-base poly-A run inside one, a sequence that repeats itself after 150 bases.      nSA = 62 mod 64
          (the number of suffixes is even on both strands together, so 63 mod 64 cannot be had)
  ns      single N every few hundred bases (inside the SAindex prefix of the suffixes in front), an N run, a sequence that begins with N, one that ends with N
  ends    an added poly-A longer than any A run of the genome (insertion point 0) and a poly-T longer than any T run (behind the last old entry)
  cap     a 12 kb chromosome and an added sequence that copies 10 050 of its bases: comparisons stop after 10 000 characters.  Made with
          --runThreadN 1 and 4; kept only if both give the same bytes
"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import refstar  # noqa: E402

OUT = os.path.join(HERE, "seq_insert")
OLD = ["Genome", "SA", "SAindex", "chrStart.txt", "genomeParameters.txt"]
NEW = ["Genome", "SA", "SAindex", "sjdbInfo.txt", "sjdbList.out.tab"]


def _rnd(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def _acgt(seqs):
    return int(sum((np.asarray(s) < 4).sum() for s in seqs))


def _tune(chrs, extra, want):
    """trim the last added sequence until 2 * (number of ACGT) = want mod 64"""
    for _ in range(64):
        if (2 * (_acgt(chrs) + _acgt(extra))) % 64 == want:
            return
        extra[-1] = extra[-1][:-1]
    raise AssertionError("cannot tune")


def _cases():
    rng = np.random.default_rng(20260117)
    out = {}
    # every case: (chromosomes, added sequences, SAindexNbases, overhang, transcripts of annot.gtf, the new junction of the plain form)
    # tails
    g1 = _rnd(rng, 2600); g2 = _rnd(rng, 1500)
    tail = _rnd(rng, 40)
    e1 = np.concatenate([_rnd(rng, 300), tail]); e2 = np.concatenate([_rnd(rng, 520), tail])
    e3 = np.concatenate([_rnd(rng, 150), g1[700:900], _rnd(rng, 167)])
    # a fourth that begins with the donor flank and ends with the acceptor flank of the first annotated junction: its suffixes tie, up to the
    # spacer, with the suffixes of the junction block -- entries that lie behind the insertion point
    e4 = np.concatenate([g1[170:180], _rnd(rng, 120), g1[290:310]])
    chrs, extra = [g1, g2], [e4, e1, e2, e3]
    _tune(chrs, extra, 0)
    out["tails"] = (chrs, extra, 5, 10, [(0, [(101, 180), (301, 390), (601, 700)]), (1, [(201, 280), (451, 520)])], ("chr1", 1001, 1200))
    # dups
    g1 = _rnd(rng, 2200); g2 = _rnd(rng, 900)
    d = _rnd(rng, 400)
    pa = _rnd(rng, 700); pa[250:450] = 0
    unit = _rnd(rng, 150); rep = np.concatenate([unit, unit, unit[:90], _rnd(rng, 45)])
    chrs, extra = [g1, g2], [d, d.copy(), pa, rep]
    _tune(chrs, extra, 62)
    out["dups"] = (chrs, extra, 4, 8, [(0, [(101, 250), (351, 420), (1251, 1300)]), (1, [(51, 140), (301, 380)])], ("chr2", 451, 600))
    # ns
    g = _rnd(rng, 3000)
    for at in range(170, 3000, 290):
        g[at] = 4
    a = _rnd(rng, 900)
    for at in range(140, 900, 210):
        a[at] = 4
    a[500:540] = 4
    b = _rnd(rng, 300); b[0] = 4
    c = _rnd(rng, 280); c[-1] = 4
    out["ns"] = ([g], [a, b, c], 6, 12, [(0, [(201, 260), (431, 500), (701, 760)]), (0, [(1801, 1900), (2001, 2100)])], ("chr1", 1001, 1150))
    # ends: no run of more than 5 equal bases in the random parts, then a 30-A and a 30-T sequence
    g = _rnd(rng, 2500)
    pA = np.concatenate([_rnd(rng, 100), np.zeros(30, np.uint8), _rnd(rng, 100)])
    pT = np.concatenate([_rnd(rng, 80), np.full(30, 3, np.uint8), _rnd(rng, 120)])
    onlyA = np.zeros(45, np.uint8)
    out["ends"] = ([g], [pA, pT, onlyA], 4, 9, [(0, [(101, 200), (401, 480), (901, 1000)])], ("chr1", 1501, 1700))
    # cap
    g = _rnd(rng, 12000)
    e = np.concatenate([_rnd(rng, 60), g[900:10950], _rnd(rng, 75)])
    out["cap"] = ([g], [e], 5, 10, [(0, [(101, 200), (401, 480), (901, 1000)])], ("chr1", 2001, 2300))
    return out


def _fasta(path, seqs, prefix):
    with open(path, "w") as f:
        for i, c in enumerate(seqs):
            f.write(">%s%d\n" % (prefix, i + 1))
            s = "".join("ACGTN"[x] for x in c)
            for k in range(0, len(s), 60):
                f.write(s[k:k + 60] + "\n")


def _write_inputs(d, chrs, extra, transcripts, sjnew):
    _fasta(os.path.join(d, "genome.fa"), chrs, "chr")
    _fasta(os.path.join(d, "extra.fa"), extra, "spike")
    with open(os.path.join(d, "annot.gtf"), "w") as f:
        for t, (ichr, exons) in enumerate(transcripts):
            for (s, e) in exons:
                f.write('chr%d\tsynth\texon\t%d\t%d\t.\t+\t.\tgene_id "g%d"; transcript_id "t%d";\n' % (ichr + 1, s, e, t + 1, t + 1))
    with open(os.path.join(d, "sj_new.tab"), "w") as f:
        f.write("%s\t%d\t%d\t+\n" % sjnew)
    ichr, exons = transcripts[0]
    with open(os.path.join(d, "sj_old.tab"), "w") as f:                  # the first intron of the first transcript
        f.write("chr%d\t%d\t%d\t+\n" % (ichr + 1, exons[0][1] + 1, exons[1][0] - 1))
    with open(os.path.join(d, "reads.fq"), "w") as f:
        s = "".join("ACGT"[x] for x in chrs[0][300:350])
        f.write("@r1\n%s\n+\n%s\n" % (s, "I" * len(s)))


def _map(tmp, form, sj, ov, threads):
    pre = "%s_t%d_" % (form, threads)
    cmd = ["./STAR", "--runMode", "alignReads", "--genomeDir", form, "--readFilesIn", "reads.fq", "--genomeFastaFiles", "extra.fa", "--sjdbFileChrStartEnd", sj,
           "--sjdbInsertSave", "All", "--sjdbOverhang", str(ov), "--runThreadN", str(threads), "--outFileNamePrefix", pre, "--outSAMtype", "None"]
    subprocess.check_call(cmd, cwd=tmp, stdout=subprocess.DEVNULL)
    return os.path.join(tmp, pre + "_STARgenome")


def main():
    if not refstar.have_ref():
        sys.exit("oracle/_ref/STAR is not built")
    total = 0
    shutil.rmtree(OUT, ignore_errors=True)
    for name, (chrs, extra, nb, ov, transcripts, sjnew) in _cases().items():
        dst = os.path.join(OUT, name)
        os.makedirs(dst)
        _write_inputs(dst, chrs, extra, transcripts, sjnew)
        keep = True
        with tempfile.TemporaryDirectory() as tmp:      # relative paths only: the reference copies its command line into genomeParameters.txt
            os.symlink(refstar.REF_BIN, os.path.join(tmp, "STAR"))
            for f in os.listdir(dst):
                shutil.copy(os.path.join(dst, f), tmp)
            for form in ("plain", "annot"):
                os.makedirs(os.path.join(tmp, form))
                cmd = ["./STAR", "--runMode", "genomeGenerate", "--genomeDir", form, "--genomeFastaFiles", "genome.fa", "--genomeSAindexNbases", str(nb),
                       "--genomeChrBinNbits", "8", "--runThreadN", "1", "--outFileNamePrefix", form + "_", "--outTmpDir", form + "_tmp"]
                if form == "annot":
                    cmd += ["--sjdbGTFfile", "annot.gtf", "--sjdbOverhang", str(ov)]
                subprocess.check_call(cmd, cwd=tmp, stdout=subprocess.DEVNULL)
                new = _map(tmp, form, "sj_new.tab" if form == "plain" else "sj_old.tab", ov, 1)
                if name == "cap":
                    new4 = _map(tmp, form, "sj_new.tab" if form == "plain" else "sj_old.tab", ov, 4)
                    same = all(open(os.path.join(new, f), "rb").read() == open(os.path.join(new4, f), "rb").read() for f in NEW)
                    print("cap/%s: --runThreadN 1 and 4 give %s bytes" % (form, "the same" if same else "DIFFERENT"))
                    keep = keep and same
                os.makedirs(os.path.join(dst, form, "old")); os.makedirs(os.path.join(dst, form, "new"))
                for f in OLD:
                    shutil.copy(os.path.join(tmp, form, f), os.path.join(dst, form, "old", f))
                for f in NEW:
                    shutil.copy(os.path.join(new, f), os.path.join(dst, form, "new", f))
                total += sum(os.path.getsize(os.path.join(dst, form, k, f)) for k, fs in (("old", OLD), ("new", NEW)) for f in fs)
        os.remove(os.path.join(dst, "reads.fq"))
        if not keep:
            shutil.rmtree(dst)
            print("case %s dropped" % name)
        else:
            print("case %-6s 2*ACGT = %d (%d mod 64)" % (name, 2 * (_acgt(chrs) + _acgt(extra)), (2 * (_acgt(chrs) + _acgt(extra))) % 64))
    print("tests/golden/seq_insert: %d bytes of reference output" % total)


if __name__ == "__main__":
    main()
