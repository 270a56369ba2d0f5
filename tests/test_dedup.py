"""--runMode inputAlignmentsFromBAM --bamRemoveDuplicatesType ... on the host path (star_amd/csrc/host/dedup.cpp) through the tool mode: on every vector of
tests/test_dedup_emul.py, both types and --bamRemoveDuplicatesMate2basesN 0 and 3, Processed.out.bam inflates to the input with exactly the flag words
changed that the Python restatement of the rule names, header included.  The in-domain vectors are pinned to the reference: to the digests of the flag
words it wrote (tests/golden/dedup_ref_flags.json, made by tests/golden/make_dedup_golden.py) everywhere, and byte for byte to its own Processed.out.bam
where oracle/_ref/STAR is built."""
import hashlib
import json
import os
import subprocess
import tempfile

import pytest

from util import ROOT, capi, bam_parts, refstar
import test_dedup_emul as D

GOLDEN = os.path.join(ROOT, "tests", "golden", "dedup_ref_flags.json")
LIBC = "the reference leaves the order of equal pairs to qsort of the C library: which pair of equal AS survives is not defined by its code"


def opt_tag(opt):
    return "%s_%d" % (D.TYPES[opt[0]], opt[1])


def flag_digest(records):
    return hashlib.sha256(b"".join(r[16:20] for r in records)).hexdigest()


def reference_run(bam, prefix, opt):
    """the reference's own tool mode on a BAM file: the parts of its Processed.out.bam"""
    subprocess.check_call([refstar.REF_BIN, "--runMode", "inputAlignmentsFromBAM", "--inputBAMfile", bam, "--outFileNamePrefix", prefix, "--bamRemoveDuplicatesType", D.TYPES[opt[0]],
                           "--bamRemoveDuplicatesMate2basesN", str(opt[1]), "--limitBAMsortRAM", "300000000"], stdout=subprocess.DEVNULL, cwd=os.path.dirname(prefix))
    return bam_parts(prefix + "Processed.out.bam")


@pytest.fixture(scope="module")
def work():
    return tempfile.mkdtemp(prefix="staramd_dedup_vec_")


def host_run(work, name, opt):
    bam = os.path.join(work, name + ".bam")
    if not os.path.exists(bam):
        D.write_bam(bam, D.vectors()[name])
    return D.tool_mode(bam, os.path.join(work, "%s_%s_" % (name, opt_tag(opt))), opt)


def only_the_survivor_differs(records, ours, theirs, opt):
    """True when two flag assignments differ only in WHICH pair of a class survives, among pairs whose mate 1 has the AS of the restatement's survivor"""
    v = [D.View(r) for r in records]
    by_name = {}
    for i, x in enumerate(v):
        by_name.setdefault((x.tid, x.name), []).append(i)
    classes = {}
    for ids in by_name.values():
        m1, m2 = sorted(ids, key=lambda i: v[i].flag & 0x80)
        a, b = v[m1], v[m2]
        classes.setdefault((a.tid, a.startS, b.startS, a.flag & ~0x400, b.flag & ~0x400, a.cigarS, b.cigarS, b.bases(opt[1])), []).append((m1, m2))
    for members in classes.values():
        top = max(v[m1].AS for m1, _ in members)
        for bits in (ours, theirs):
            alive = [p for p in members if not bits[p[0]]]
            if len(alive) != 1 or bits[alive[0][1]] or v[alive[0][0]].AS != top or any(bits[p[0]] != bits[p[1]] for p in members):
                return False
    return True


def test_flags_of_the_front_end(built, work):
    bam = D.write_bam(os.path.join(work, "clips_flags.bam"), D.vectors()["clips"])
    base = ["--runMode", "inputAlignmentsFromBAM", "--inputBAMfile", bam, "--outFileNamePrefix", os.path.join(work, "flags_")]
    with pytest.raises(RuntimeError) as e:
        capi.HostRun(base + ["--bamRemoveDuplicatesType", "Identical"])
    assert str(e.value) == "EXITING because of fatal PARAMETERS error: unrecognized option in of --bamRemoveDuplicatesType=Identical\nSOLUTION: use allowed option: - or UniqueIdentical or UniqueIdenticalNotMulti"
    with pytest.raises(RuntimeError) as e:
        capi.HostRun(base + ["--bamRemoveDuplicatesType", "-"])
    assert "only works with --outWigType bedGraph OR --bamRemoveDuplicatesType Identical" in str(e.value) and "not implemented" not in str(e.value)
    with pytest.raises(RuntimeError, match="--gpuBAMdedup takes Host or Device"):
        capi.HostRun(base + ["--bamRemoveDuplicatesType", "UniqueIdentical", "--gpuBAMdedup", "Gpu"])
    # alignReads takes the two flags and ignores them, as the reference does: the run fails on its missing genome, not on them
    with pytest.raises(RuntimeError) as e:
        capi.HostRun(["--genomeDir", os.path.join(work, "no_such_genome"), "--readFilesIn", bam, "--outFileNamePrefix", os.path.join(work, "al_"), "--bamRemoveDuplicatesType", "UniqueIdentical",
                      "--bamRemoveDuplicatesMate2basesN", "3", "--gpuBAMdedup", "Host"])
    assert "bamRemoveDuplicates" not in str(e.value) and "gpuBAMdedup" not in str(e.value)
    # with --outWigType in the same command the tracks are made and the marking is skipped (Parameters.cpp:587-599)
    capi.HostRun(base + ["--bamRemoveDuplicatesType", "UniqueIdentical", "--outWigType", "bedGraph"]).close()
    assert os.path.exists(os.path.join(work, "flags_Signal.Unique.str1.out.bg")) and not os.path.exists(os.path.join(work, "flags_Processed.out.bam"))


@pytest.mark.parametrize("name", D.VECTOR_NAMES)
def test_host_path_equals_the_restatement(built, work, name):
    recs = D.vectors()[name]
    bam = os.path.join(work, name + ".bam")
    if not os.path.exists(bam):
        D.write_bam(bam, recs)
    text, refs, same = bam_parts(bam)
    assert same == recs
    for opt in D.options(name):
        want = D.expected(name, opt)
        got = host_run(work, name, opt)
        assert D.result_of(capi.dedup_host(recs, *opt)) == D.as_result(want), (name, opt)
        if want[0] == "fatal":
            assert got == (D.NH_FATAL if want[1] == 1 else D.AS_FATAL), (name, opt)
            continue
        assert got[0] == text and got[1] == refs, "the header changed"
        assert got[2] == D.apply_bits(recs, want[0]), (name, opt)
        log = open(os.path.join(work, "%s_%s_Log.out" % (name, opt_tag(opt)))).read()
        st = want[1]
        assert "on the Host (--gpuBAMdedup): %d records, %d pairs, %d classes, %d records marked, %d unpaired unique records\n" % (st[0], st[2], st[3], st[4], st[5]) in log
    if name not in ("empty", "no_nh", "no_as", "no_both"):
        assert sum(D.expected(name, D.OPTION_SETS[0])[0]) > 0, "a vector in which nothing is marked shows little"


@pytest.mark.parametrize("name", D.IN_DOMAIN)
def test_golden_digests_of_the_reference(built, work, name):
    """what the reference wrote where it was built, held against the host path everywhere"""
    golden = json.load(open(GOLDEN))[name]
    assert sorted(golden) == sorted(opt_tag(o) for o in D.options(name))
    bad = [opt for opt in D.options(name) if flag_digest(host_run(work, name, opt)[2]) != golden[opt_tag(opt)]]
    assert not bad


@pytest.mark.skipif(not refstar.have_ref(), reason="oracle/_ref/STAR not built")
@pytest.mark.parametrize("name", D.IN_DOMAIN)
def test_reference_byte_for_byte(built, work, name):
    recs = D.vectors()[name]
    tie_only = []
    for opt in D.options(name):
        ours = host_run(work, name, opt)
        ref = reference_run(os.path.join(work, name + ".bam"), os.path.join(work, "%s_ref_%s_" % (name, opt_tag(opt))), opt)
        if ours == ref:
            continue
        bit = lambda parts: [D._u32(r, 16) >> 26 & 1 for r in parts[2]]
        assert name == "ties" and ours[:2] == ref[:2] and D.apply_bits(ref[2], bit(ours)) == ours[2] and only_the_survivor_differs(recs, bit(ours), bit(ref), opt), (name, opt)
        tie_only.append(opt)
    if tie_only:
        pytest.xfail(LIBC + ": %s" % tie_only)
