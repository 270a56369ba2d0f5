"""Writes tests/golden/dedup_ref_flags.json: per in-domain vector of tests/test_dedup_emul.py and option set, the SHA-256 of the flag words
(flag << 16 | n_cigar_op of every record, in file order) of the Processed.out.bam that the reference binary (oracle/_ref/STAR) wrote.  Recorded
results only; run where the reference is built:  python tests/golden/make_dedup_golden.py"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_dedup as T  # noqa: E402
import test_dedup_emul as D  # noqa: E402


def main():
    work = tempfile.mkdtemp(prefix="staramd_dedup_golden_")
    out = {}
    for name in D.IN_DOMAIN:
        bam = D.write_bam(os.path.join(work, name + ".bam"), D.vectors()[name])
        out[name] = {T.opt_tag(opt): T.flag_digest(T.reference_run(bam, os.path.join(work, "%s_%s_" % (name, T.opt_tag(opt))), opt)[2]) for opt in D.options(name)}
    with open(os.path.join(HERE, "dedup_ref_flags.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
