"""Writes tests/golden/tiny_index/<case>/: three synthetic genomes of a few kb, each indexed by the REFERENCE binary (oracle/_ref/STAR) once plain
and once with a small GTF.  Kept per case: our inputs genome.fa and annot.gtf, and of what the reference wrote plain/ and annot/ with Genome, SA,
SAindex, genomeParameters.txt, chrStart.txt (and sjdbList.out.tab in annot/).  oracle/index_routines_check.cpp and tests/index_routines_gpu.hip hold
the restated suffix order, SAindex walk and junction insertion, and the product's buildAll / sjdbInsertHost, to these bytes -- without the
reference being present.

    python tests/golden/make_index_golden.py        (needs oracle/_ref/STAR; the committed files were made this way and are not rewritten by tests)

  tails     four chromosomes whose last 30 bases are the same, padded to 256, the base behind each padding contradicting position order;
            a fifth chromosome with repeats carries the transcripts                       --genomeSAindexNbases 4, --sjdbOverhang 10
  nprefix   single N every few hundred bases (N inside the SAindex prefix of the suffixes in front of it) and an N run        6, 12
  repeats   two chromosomes with repeat families, a 300-base duplicate and poly-A up to a chromosome end; exons cut inside repeats     5, 8
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

OUT = os.path.join(HERE, "tiny_index")
KEEP = ["Genome", "SA", "SAindex", "genomeParameters.txt", "chrStart.txt"]


def _rnd(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def _plant(rng, g, families, copies, length):
    for _ in range(families):
        unit = _rnd(rng, length)
        for _ in range(copies):
            at = int(rng.integers(0, len(g) - length))
            g[at:at + length] = unit
    return g


def _cases():
    rng = np.random.default_rng(20240611)
    out = {}
    # tails
    tail = _rnd(rng, 30)
    chrs = []
    for first in (3, 2, 1, 0):
        c = np.concatenate([_rnd(rng, 120), tail])
        c[0] = first
        chrs.append(c)
    chrs.append(_plant(rng, _rnd(rng, 1200), 2, 3, 60))
    out["tails"] = (chrs, 4, 10, [(4, [(101, 180), (301, 390), (601, 700)]), (4, [(101, 180), (451, 520), (601, 700)]), (4, [(801, 860), (1001, 1100)])])
    # nprefix
    g = _plant(rng, _rnd(rng, 2500), 2, 3, 50).astype(np.uint8)
    for at in range(150, 2500, 270):
        g[at] = 4
    g[1700:1750] = 4
    out["nprefix"] = ([g], 6, 12, [(0, [(201, 260), (431, 500), (701, 760)]), (0, [(901, 960), (1101, 1190)]), (0, [(1801, 1900), (2001, 2100), (2201, 2300)])])
    # repeats
    a = _plant(rng, _rnd(rng, 1800), 3, 4, 80)
    a[1200:1500] = a[200:500]
    a[-35:] = 0
    b = _plant(rng, _rnd(rng, 900), 2, 3, 40)
    b[100:180] = a[300:380]
    out["repeats"] = ([a, b], 5, 8, [(0, [(101, 250), (351, 420), (1251, 1300)]), (0, [(351, 420), (1351, 1420), (1601, 1700)]), (1, [(51, 140), (301, 380), (601, 700)])])
    return out


def _write_inputs(d, chrs, transcripts):
    with open(os.path.join(d, "genome.fa"), "w") as f:
        for i, c in enumerate(chrs):
            f.write(">chr%d\n" % (i + 1))
            s = "".join("ACGTN"[x] for x in c)
            for k in range(0, len(s), 60):
                f.write(s[k:k + 60] + "\n")
    with open(os.path.join(d, "annot.gtf"), "w") as f:
        for t, (ichr, exons) in enumerate(transcripts):
            for (s, e) in exons:
                f.write('chr%d\tsynth\texon\t%d\t%d\t.\t+\t.\tgene_id "g%d"; transcript_id "t%d";\n' % (ichr + 1, s, e, t + 1, t + 1))


def main():
    if not refstar.have_ref():
        sys.exit("oracle/_ref/STAR is not built")
    total = 0
    for name, (chrs, nb, ov, transcripts) in _cases().items():
        dst = os.path.join(OUT, name)
        shutil.rmtree(dst, ignore_errors=True)
        os.makedirs(dst)
        _write_inputs(dst, chrs, transcripts)
        with tempfile.TemporaryDirectory() as tmp:      # relative paths only: the reference copies its command line into genomeParameters.txt
            os.symlink(refstar.REF_BIN, os.path.join(tmp, "STAR"))
            for f in ("genome.fa", "annot.gtf"):
                shutil.copy(os.path.join(dst, f), tmp)
            for kind in ("plain", "annot"):
                os.makedirs(os.path.join(tmp, kind))
                cmd = ["./STAR", "--runMode", "genomeGenerate", "--genomeDir", kind, "--genomeFastaFiles", "genome.fa", "--genomeSAindexNbases", str(nb),
                       "--genomeChrBinNbits", "8", "--runThreadN", "1", "--outFileNamePrefix", kind + "_", "--outTmpDir", kind + "_tmp"]
                if kind == "annot":
                    cmd += ["--sjdbGTFfile", "annot.gtf", "--sjdbOverhang", str(ov)]
                subprocess.check_call(cmd, cwd=tmp, stdout=subprocess.DEVNULL)
                os.makedirs(os.path.join(dst, kind))
                for f in KEEP + (["sjdbList.out.tab"] if kind == "annot" else []):
                    shutil.copy(os.path.join(tmp, kind, f), os.path.join(dst, kind, f))
                    total += os.path.getsize(os.path.join(dst, kind, f))
    print("tests/golden/tiny_index: %d bytes of reference output" % total)


if __name__ == "__main__":
    main()
