"""The command-line front end (star_amd/csrc/host/main.cpp): three batch slots (parse / map / post-map on their own threads), the phases of 2-pass and
BySJout (index re-upload, junction whitelist), the second batch of merged mates.  On a box without a GPU the same main.cpp is linked against the oracle
behind the engine's C ABI (oracle/cli_shim.cpp -> oracle/_build/star_amd_oracle_cli, test infrastructure); the GPU twin of this file is the `cli`
tests in test_by_sjout.py / test_config1.py, which run the shipped binary."""
import os
import subprocess
import threading

import pytest

from util import bam_parts, compare_outputs, prepare, refstar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "oracle", "_build", "star_amd_oracle_cli")
pytestmark = pytest.mark.skipif(not refstar.have_ref() or not os.path.exists(CLI), reason="oracle/_ref/STAR or the oracle-backed CLI not built")

CASES = [("pe101", ["--twopassMode", "Basic", "--outFilterType", "BySJout", "--outSAMunmapped", "Within"], 700),
         ("pe76_overlap", ["--peOverlapNbasesMin", "10", "--peOverlapMMp", "0.1", "--chimSegmentMin", "10", "--chimJunctionOverhangMin", "10", "--chimMultimapNmax", "20",
                           "--chimOutType", "WithinBAM", "Junctions", "--outSAMtype", "BAM", "Unsorted", "SortedByCoordinate", "--quantMode", "GeneCounts"], 300),
         ("se50", ["--sjdbGTFfile", "GTF", "--quantMode", "TranscriptomeSAM", "GeneCounts", "--outSAMtype", "BAM", "SortedByCoordinate", "--outWigType", "bedGraph"], 450),
         ("pe150_chim", ["--chimSegmentMin", "15", "--outMultimapperOrder", "Random", "--outReadsUnmapped", "Fastx", "--clip3pNbases", "3", "5"], 5000),
         ("pe101", ["--waspOutputMode", "SAMtag", "--varVCFfile", "VCF", "--outSAMtype", "BAM", "Unsorted", "--twopassMode", "Basic"], 1000)]


# the same runs with one mapper thread per "GPU" (--gpuDevices: two / three oracle-backed contexts fed from the one reader, emitted in input
# order by the one writer, index / whitelist updates fanned out between the phases): still equal to ONE reference run
MULTI = [(CASES[0][0], CASES[0][1], 150, "0,1"), (CASES[1][0], CASES[1][1], 120, "0,1,2"), (CASES[3][0], CASES[3][1], 400, "0,1"), (CASES[4][0], CASES[4][1], 200, "0,1")]


@pytest.mark.parametrize("name,more,batch,devices", MULTI)
def test_cli_pipeline_multi_device(name, more, batch, devices, tmp_path, built):
    run_cli_case(CLI, name, more + ["--gpuDevices", devices], batch, tmp_path)


def run_cli_case(cli, name, more, batch, tmp_path, fastq_hook=None, env=None):
    """one run of a command-line front end (`cli`) against one run of the reference with the same flags: every output file"""
    info = dict(prepare(name, str(tmp_path), need_ref=False))
    d = os.path.dirname(info["fastq"][0])
    if fastq_hook:
        info["fastq"] = fastq_hook(info, d)
    if "VCF" in more:
        from test_wasp import _vcf
        more = [_vcf(info, d) if x == "VCF" else x for x in more]
    more = [info["gtf"] if x == "GTF" else x for x in more]
    cli_only = []
    if "--gpuDevices" in more:
        i = more.index("--gpuDevices"); cli_only = more[i:i + 2]; more = more[:i] + more[i + 2:]
    flags = list(info["extra"]) + more
    rf = list(flags)
    if "--runThreadN" in rf:
        k = rf.index("--runThreadN"); del rf[k:k + 2]
    ref = refstar.align(info["idx"], info["fastq"], os.path.join(d, "ref_"), threads=1, extra=rf)
    new = os.path.join(d, "cli_")
    p = subprocess.run([cli, "--runMode", "alignReads", "--genomeDir", info["idx"], "--readFilesIn"] + info["fastq"] +
                       ["--outFileNamePrefix", new, "--runThreadN", "4", "--gpuBatchReads", str(batch)] + rf + cli_only, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       env=dict(os.environ, **env) if env else None)
    assert p.returncode == 0, p.stderr[-1500:]
    n = 0
    for f in sorted(os.listdir(d)):
        if not f.startswith("ref_") or os.path.isdir(os.path.join(d, f)):
            continue
        g = f[4:]
        if g in ("Log.out", "Log.progress.out", "Log.final.out", "Log.std.out"):
            continue
        pa, pb = os.path.join(d, f), new + g
        assert os.path.exists(pb), g
        if g == "Aligned.out.sam":
            assert refstar.sam_body_sorted(pa) == refstar.sam_body_sorted(pb)
        elif g.endswith(".bam"):
            (ta, ra, rr), (tb, rb, nr) = bam_parts(pa), bam_parts(pb)
            assert ra == rb and (rr == nr if "Random" not in more else sorted(rr) == sorted(nr)), g
        elif g == "Chimeric.out.junction":
            L = lambda p: [l for l in open(p) if not l.startswith("# 2.7.11b")]
            assert L(pa) == L(pb)
        else:
            assert open(pa, "rb").read() == open(pb, "rb").read(), g
        n += 1
    assert n >= 2
    assert refstar.final_log_counters(ref + "Log.final.out") == refstar.final_log_counters(new + "Log.final.out")
    return fast_paths(p.stderr)


def fast_paths(stderr):
    """the front end's count of batches that took a path with a silent fallback behind it (include/star_amd_cli.h fastPaths): output written through a mapping of the
    file, input read in place from mappings of the files, uploads started ahead of their staramd_map_batch call"""
    import re
    m = re.search(r"fast paths: output through a file mapping (\d+) batches, input from file mappings (\d+), uploads prefetched (\d+), kernels begun beside the copy of the results before them (\d+)", stderr)
    assert m, stderr[-800:]
    return {"out_mapped": int(m.group(1)), "in_mapped": int(m.group(2)), "prefetched": int(m.group(3)), "overlapped": int(m.group(4))}


@pytest.mark.parametrize("name,more,batch", CASES)
def test_cli_pipeline(name, more, batch, tmp_path, built):
    run_cli_case(CLI, name, more, batch, tmp_path)


@pytest.mark.parametrize("batch", [700, 333, 5000])
def test_cli_pipeline_sliced_input(batch, tmp_path, built):
    """FastqReader::fill reads a block of a regular file in four slices on threads (positional reads, line ends found per slice); the threshold
    is lowered so that every block of these small inputs takes that path: batches that end inside a slice, a carry, a short last block"""
    run_cli_case(CLI, "pe101", ["--outSAMunmapped", "Within"], batch, tmp_path, env={"STARAMD_READ_SLICE_MIN": "1"})


@pytest.mark.parametrize("kick", ["50", "700"])
def test_cli_pipeline_background_junction_collapse(kick, tmp_path, built):
    """the junction table is collapsed on a thread of its own whenever it passes a threshold (runner.cpp SjBackground); the threshold is lowered so that it happens
    after (almost) every batch of these small inputs, in both passes of a 2-pass run: SJ.out.tab of both passes and everything else still equal to the reference's"""
    run_cli_case(CLI, "pe101", ["--twopassMode", "Basic", "--outSAMunmapped", "Within"], 200, tmp_path, env={"STARAMD_SJ_KICK": kick})


CHIM_WASP = ["--chimSegmentMin", "15", "--chimJunctionOverhangMin", "15", "--chimOutType", "WithinBAM", "--outSAMtype", "BAM", "Unsorted",
             "--waspOutputMode", "SAMtag", "--varVCFfile", "VCF", "--outSAMattributes", "NH", "HI", "AS", "nM", "vA", "vG", "vW"]


def _chimeras_in_runs(info, d):
    """the input re-ordered so that its (few) chimeric reads follow one another in two runs: a chimera in the BAM then inherits its vW from
    a read several places back, across range and batch boundaries"""
    pre = refstar.align(info["idx"], info["fastq"], os.path.join(d, "pre_"), threads=1, extra=list(info["extra"]) + ["--chimSegmentMin", "15", "--chimJunctionOverhangMin", "15"])
    chim = {l.split("\t")[9] for l in open(pre + "Chimeric.out.junction") if not l.startswith("#") and not l.startswith("chr_donorA")}
    assert len(chim) >= 6
    out = []
    for m, f in enumerate(info["fastq"]):
        L = open(f).read().split("\n")
        recs = ["\n".join(L[i:i + 4]) for i in range(0, len(L) - 3, 4)]
        is_chim = [r.split()[0][1:].split("/")[0] in chim for r in recs]
        c = [r for r, x in zip(recs, is_chim) if x]; o = [r for r, x in zip(recs, is_chim) if not x]
        assert len(c) >= 6
        order = o[:21] + c[:len(c) // 2] + o[21:24] + c[len(c) // 2:] + o[24:]
        g = os.path.join(d, "runs_%d.fq" % (m + 1))
        open(g, "w").write("\n".join(order) + "\n")
        out.append(g)
    return out


@pytest.mark.parametrize("batch", [8, 2000])
def test_cli_pipeline_wasp_verdict_on_chimeric_bam_records(batch, tmp_path, built):
    """vW on the BAM records of a chimeric read is the verdict of the nearest earlier read that was not itself a chimera in the BAM
    (ReadAlign_oneRead.cpp:99-103), whatever the batch and thread boundaries in between (the carried value)"""
    run_cli_case(CLI, "pe150_chim", CHIM_WASP, batch, tmp_path, fastq_hook=_chimeras_in_runs)


def test_sam_into_a_named_pipe(tmp_path, built):
    """Aligned.out.sam as a FIFO (mkfifo + a consumer, the way it is piped into samtools): the writer thread must fall back to sequential writes -- a
    positional write on a pipe fails with ESPIPE (runner.cpp SamWriter)"""
    import threading
    info = dict(prepare("pe101", str(tmp_path), need_ref=False))
    d = os.path.dirname(info["fastq"][0])
    flags = list(info["extra"]) + ["--readMapNumber", "400"]
    ref = refstar.align(info["idx"], info["fastq"], os.path.join(d, "ref_"), threads=1, extra=flags)
    new = os.path.join(d, "fifo_")
    os.mkfifo(new + "Aligned.out.sam")
    got = []
    t = threading.Thread(target=lambda: got.append(open(new + "Aligned.out.sam", "rb").read()))
    t.start()
    p = subprocess.run([CLI, "--runMode", "alignReads", "--genomeDir", info["idx"], "--readFilesIn"] + info["fastq"] +
                       ["--outFileNamePrefix", new, "--runThreadN", "4", "--gpuBatchReads", "100"] + flags, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    t.join(timeout=60)
    assert p.returncode == 0, p.stderr[-1500:]
    body = sorted(l for l in got[0].splitlines(keepends=True) if not l.startswith(b"@"))
    assert body == refstar.sam_body_sorted(ref + "Aligned.out.sam")


@pytest.mark.parametrize("name,more,env", [("pe101", [], {"STARAMD_NO_INPUT_MMAP": "1"}), ("pe101", [], {"STARAMD_READ_SLICE_MIN": "4096", "STARAMD_READ_SLICES": "5"}),
                                           ("pe150_indel", ["--outFilterType", "BySJout", "--outSAMunmapped", "Within"], {"STARAMD_READ_SLICE_MIN": "4096"}),
                                           ("se50", ["--twopassMode", "Basic", "--outReadsUnmapped", "Fastx"], {"STARAMD_READ_SLICE_MIN": "2048", "STARAMD_READ_SLICES": "3"}),
                                           ("pe101", ["--outSAMreadID", "Number"], {}), ("pe101", ["--outQSconversionAdd", "-2"], {})])
def test_reader_over_a_mapping_of_the_input_files(name, more, env, tmp_path, built):
    """a regular input file is mapped and a batch is a range of the mapping (reads.cpp fillMapped), line ends looked for in slices on threads (STARAMD_READ_SLICE_MIN lowers
    the size from which a block is sliced); STARAMD_NO_INPUT_MMAP=1 and the options that rewrite the text of a batch (--outSAMreadID Number, --outQSconversionAdd) take
    the copying reader; a held-reads stage (BySJout) and a second pass follow a mapped first one.  Same outputs as the reference either way"""
    fp = run_cli_case(CLI, name, more, 170, tmp_path, env=env)
    # the path under test really ran (a mapped reader that silently falls back to the copying one returns the same bytes)
    copying = "STARAMD_NO_INPUT_MMAP" in env or "--outSAMreadID" in more or "--outQSconversionAdd" in more
    assert (fp["in_mapped"] == 0) if copying else (fp["in_mapped"] >= 2), fp


def _rewrite(info, d, fn, tag):
    out = []
    for m, f in enumerate(info["fastq"]):
        text = open(f, "rb").read()
        g = os.path.join(d, "%s_%d.fq" % (tag, m + 1))
        r = fn(text, m)
        if isinstance(r, list):
            names = []
            for k, part in enumerate(r):
                gk = os.path.join(d, "%s_%d_%d.fq" % (tag, m + 1, k)); open(gk, "wb").write(part); names.append(gk)
            out.append(",".join(names))
        else:
            open(g, "wb").write(r); out.append(g)
    return out


def _records(text):
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return [b"\n".join(lines[i:i + 4]) + b"\n" for i in range(0, len(lines), 4)]


INPUT_SHAPES = {
    "empty_line_ends_the_input": lambda t, m: b"".join(_records(t)[:230]) + b"\n" + b"".join(_records(t)[230:]),       # what follows an empty ID line is not read (both mates cut alike)
    "two_files_per_mate": lambda t, m: [b"".join(_records(t)[:333]), b"".join(_records(t)[333:])],
}


@pytest.mark.parametrize("shape", sorted(INPUT_SHAPES))
@pytest.mark.parametrize("mapped", [True, False])
def test_reader_on_input_shapes(shape, mapped, tmp_path, built):
    """file shapes the reader meets and the reference accepts (it exits on \\r\\n line ends and on a last line without a newline), with the mapped and with the copying reader;
    batches of 100 reads, so that the odd place falls inside a batch"""
    run_cli_case(CLI, "pe101", ["--outSAMunmapped", "Within"], 100, tmp_path, fastq_hook=lambda info, d: _rewrite(info, d, INPUT_SHAPES[shape], shape),
                 env=None if mapped else {"STARAMD_NO_INPUT_MMAP": "1"})


@pytest.mark.parametrize("mapped", [True, False])
def test_regular_file_then_fifo_in_one_list(mapped, tmp_path, built):
    """--readFilesIn a.fq,<fifo>: the first file of a mate is read through its mapping, the second cannot be mapped and takes the copying reader -- the batch that starts the
    second file must not keep the pointer into the first file's mapping (round 4: garbage reads or a fault at exactly this boundary)"""
    info = dict(prepare("pe101", str(tmp_path), need_ref=False))
    d = os.path.dirname(info["fastq"][0])
    parts = _rewrite(info, d, INPUT_SHAPES["two_files_per_mate"], "parts")          # ["m1_0,m1_1", "m2_0,m2_1"]
    ref = refstar.align(info["idx"], parts, os.path.join(d, "ref_"), threads=1, extra=list(info["extra"]))
    fifos, feeders = [], []
    for m, lst in enumerate(parts):
        a, b = lst.split(",")
        f = os.path.join(d, "fifo_%d" % m); os.mkfifo(f); fifos.append(a + "," + f)
        t = threading.Thread(target=lambda src=b, dst=f: open(dst, "wb").write(open(src, "rb").read())); t.start(); feeders.append(t)
    new = os.path.join(d, "cli_")
    p = subprocess.run([CLI, "--runMode", "alignReads", "--genomeDir", info["idx"], "--readFilesIn"] + fifos + ["--outFileNamePrefix", new, "--runThreadN", "4", "--gpuBatchReads", "100"]
                       + list(info["extra"]), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=dict(os.environ, **({} if mapped else {"STARAMD_NO_INPUT_MMAP": "1"})))
    for t in feeders:
        t.join(timeout=60)
    assert p.returncode == 0, p.stderr[-1500:]
    assert refstar.sam_body_sorted(ref + "Aligned.out.sam") == refstar.sam_body_sorted(new + "Aligned.out.sam")
    assert open(ref + "SJ.out.tab", "rb").read() == open(new + "SJ.out.tab", "rb").read()
    fp = fast_paths(p.stderr)
    assert (fp["in_mapped"] >= 2) if mapped else (fp["in_mapped"] == 0), fp


@pytest.mark.parametrize("mode,more", [("2", []), ("2", ["--outSAMtype", "BAM", "Unsorted"]), ("0", []), ("2", ["--twopassMode", "Basic"])])
def test_writer_through_a_mapping_of_the_output_file(mode, more, tmp_path, built):
    """the SAM / unsorted-BAM writer grows the file and copies the batch's text into a mapping of the new part (STARAMD_WRITER_MMAP=2: whatever the size of a batch;
    the default does so from 1 MB per batch); =0: positional writes.  Same bytes either way, and the file ends where the last record ends"""
    fp = run_cli_case(CLI, "pe101", more, 150, tmp_path, env={"STARAMD_WRITER_MMAP": mode, "STARAMD_WRITER_THREADS": "3"})
    # round 4 shipped this test with a writer whose mapping always failed (output opened write-only) and whose fallback produced the same bytes: the count is the test
    assert (fp["out_mapped"] == 0) if mode == "0" else (fp["out_mapped"] >= 2), fp

