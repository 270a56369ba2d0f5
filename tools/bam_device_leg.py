#!/usr/bin/env python3
"""bench.py's BAM leg (the `bam_output` configuration, same argv as bench.py:bam_leg, through capi.run_cli) once with --gpuBAMcompression Host and once
with Device, on the same box.  One JSON line: M pairs/s in the timed region, BAM bytes, device bytes / host bytes, and the split of the device
compression (STARAMD_HOST_TIMING lines of k_bgzf.hip: host staging copy, H2D, kernels, D2H, copy out; summed over the run).
Then the SortedByCoordinate leg of --gpuBAMsort: compression Host + sort Host, compression Device + sort Host, compression Device + sort Device, alternated,
--sort-repeats times each (default 2): M pairs/s in the timed region, finishSeconds (the end of the run: writer drained, sorted BAM written, SJ.out.tab)
and, for the Device sort, the split of staramd_bamsort_finish (its STARAMD_HOST_TIMING line) with the gather kernel's bytes read + written per second.
With --wig (a --sorted-only form) the leg is that of --gpuSignal: Host sort + host signal and Device sort + --gpuSignal Device, both with --outWigType bedGraph,
and beside them the same two forms without --outWigType (they run no signal code): finishSeconds, the signal stage's own time on both sides (the
STARAMD_HOST_TIMING lines of bam_sorted.cpp), the device's split per kernel group and the bytes of the runs (k_signal.hip's line).
  python tools/bam_device_leg.py [--sorted-only [--wig]] [--sort-repeats N] [--reads N ...bench.py flags] [ENV=V ...]     (GPU box)"""
import hashlib, json, os, re, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench


def run_captured(argv):
    """bench._run_cli with this process's stderr (fd 2) going to a file as well: the C++ side prints the timing lines there"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        try:
            t = time.perf_counter()
            rc, rep = bench._run_cli(argv)
            wall = time.perf_counter() - t
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode(errors="replace")
    sys.stderr.write(text[-2000:])
    return rc, rep, wall, text


def split(text):
    keys = ["staging copy", "H2D", "kernels", "D2H", "copy out"]
    tot = {k: 0.0 for k in keys}
    calls = 0
    for line in text.splitlines():
        if "bgzf device:" not in line:
            continue
        calls += 1
        for k in keys:
            m = re.search(re.escape(k) + r" ([0-9.]+) ms", line)
            if m:
                tot[k] += float(m.group(1))
    return dict({k.replace(" ", "_") + "_ms": round(v, 2) for k, v in tot.items()}, calls=calls)


def sort_split(text):
    """the line staramd_bamsort_finish prints: records, MB in and out, rounds, milliseconds per stage; gather_GB_s = (bytes read + bytes written) / gather time"""
    m = re.search(r"bamsort device: (\d+) records, ([0-9.]+) -> ([0-9.]+) MB, (\d+) rounds: sort ([0-9.]+) ms, lengths \+ scan ([0-9.]+) ms, gather ([0-9.]+) ms, deflate ([0-9.]+) ms, D2H ([0-9.]+) ms, sink ([0-9.]+) ms", text)
    if not m:
        return None
    v = [float(x) for x in m.groups()]
    return {"records": int(v[0]), "MB_in": v[1], "MB_out": v[2], "rounds": int(v[3]), "sort_ms": v[4], "lengths_scan_ms": v[5], "gather_ms": v[6], "deflate_ms": v[7], "D2H_ms": v[8],
            "sink_ms": v[9], "gather_GB_s": round(2 * v[1] / max(v[6], 1e-9), 1)}


def signal_split(text):
    """the signal stage of a run: its time on the host's clock (either side) and, on the device, k_signal.hip's line"""
    out = {}
    m = re.search(r"signal stage \((device|host)\): ([0-9.]+) ms", text)
    if m:
        out["side"] = m.group(1); out["stage_ms"] = float(m.group(2))
    m = re.search(r"signal device: (\d+) records, (\d+) pairs, (\d+) tiles, (\d+) runs \(([0-9.]+) MB\): records \+ scan \+ emit ([0-9.]+) ms, sort ([0-9.]+) ms, tiles ([0-9.]+) ms, D2H ([0-9.]+) ms", text)
    if m:
        v = m.groups()
        out.update({"records": int(v[0]), "pairs": int(v[1]), "tiles": int(v[2]), "runs": int(v[3]), "runs_MB": float(v[4]), "records_scan_emit_ms": float(v[5]), "sort_ms": float(v[6]),
                    "tiles_ms": float(v[7]), "D2H_ms": float(v[8])})
    return out or None


def main():
    env = [a for a in sys.argv[1:] if "=" in a and not a.startswith("-")]
    for a in env:
        k, v = a.split("=", 1)
        os.environ[k] = v
    sys.argv = [sys.argv[0]] + [a for a in sys.argv[1:] if a not in env]
    sorted_only = "--sorted-only" in sys.argv
    wig = "--wig" in sys.argv
    repeats = 2
    if "--sort-repeats" in sys.argv:
        k = sys.argv.index("--sort-repeats"); repeats = int(sys.argv[k + 1]); del sys.argv[k:k + 2]
    sys.argv = [a for a in sys.argv if a not in ("--sorted-only", "--wig")]
    args = bench.parse()
    log = lambda s: print("bam_device_leg: " + s, file=sys.stderr, flush=True)
    g, ginfo = bench.build_genome(args, args.genome_mb, log)
    idx = os.path.join(g, "idx")
    nb, w = 6, 2
    n_total = (nb + w) * args.reads
    rd = os.path.join(g, "bamdev_n%d" % n_total)
    os.makedirs(rd, exist_ok=True)
    fq = bench.make_reads(args, g, rd, "reads_r0", n_total, 7000)
    threads = max(4, min(64, bench.effective_cpus()))
    os.environ["STARAMD_HOST_TIMING"] = "1"
    out = {"reads_per_batch": args.reads, "genome_mb": args.genome_mb, "host_threads": threads}
    for name, typ in (() if sorted_only else (("unsorted", ["BAM", "Unsorted"]), ("sorted_by_coordinate", ["BAM", "SortedByCoordinate"]))):
        row = {}
        for mode in ("Host", "Device"):
            prefix = os.path.join(rd, "bam_%s_%s_" % (name, mode))
            argv = ["--runMode", "alignReads", "--genomeDir", idx, "--readFilesIn"] + fq + ["--outFileNamePrefix", prefix, "--runThreadN", str(threads), "--gpuBatchReads",
                    str(args.reads), "--benchWarmupReads", str(w * args.reads), "--readMapNumber", str((nb + w) * args.reads), "--outSAMtype"] + typ + ["--gpuBAMcompression", mode]
            rc, rep, wall, text = run_captured(argv)
            f = prefix + ("Aligned.out.bam" if name == "unsorted" else "Aligned.sortedByCoord.out.bam")
            r = {"exit_code": rc, "Mpairs_s_timed_region": int(rep.timedReads) / max(float(rep.timedWall), 1e-9) / 1e6, "timed_reads": int(rep.timedReads),
                 "whole_run_s": round(wall, 3), "bam_bytes": os.path.getsize(f) if os.path.isfile(f) else None}
            if mode == "Device":
                r["device_compression"] = split(text)
            row[mode] = r
            for q in os.listdir(rd):
                if q.startswith("bam_%s_%s_" % (name, mode)) and q.endswith(".bam"):
                    os.remove(os.path.join(rd, q))
        if row["Host"]["bam_bytes"] and row["Device"]["bam_bytes"]:
            row["device_bytes_over_host_bytes"] = round(row["Device"]["bam_bytes"] / row["Host"]["bam_bytes"], 4)
        out[name] = row
    # --gpuBAMsort: the three forms of the SortedByCoordinate run, alternated
    forms = (("host_host", "Host", "Host", []), ("device_compression", "Device", "Host", []), ("device_compression_and_sort", "Device", "Device", []))
    if wig:
        bg = ["--outWigType", "bedGraph"]
        forms = (("host_host_signal_host", "Host", "Host", bg), ("device_device_signal_device", "Device", "Device", bg + ["--gpuSignal", "Device"]), forms[0], forms[2])
    leg = {f[0]: [] for f in forms}
    for rep_i in range(repeats):
        for tag, comp, srt, more in forms:
            prefix = os.path.join(rd, "bamsort_%s_" % tag)
            argv = ["--runMode", "alignReads", "--genomeDir", idx, "--readFilesIn"] + fq + ["--outFileNamePrefix", prefix, "--runThreadN", str(threads), "--gpuBatchReads",
                    str(args.reads), "--benchWarmupReads", str(w * args.reads), "--readMapNumber", str((nb + w) * args.reads), "--outSAMtype", "BAM", "SortedByCoordinate",
                    "--gpuBAMcompression", comp, "--gpuBAMsort", srt] + more
            rc, rep, wall, text = run_captured(argv)
            f = prefix + "Aligned.sortedByCoord.out.bam"
            r = {"exit_code": rc, "Mpairs_s_timed_region": round(int(rep.timedReads) / max(float(rep.timedWall), 1e-9) / 1e6, 4), "finishSeconds": round(float(rep.finishSeconds), 4),
                 "whole_run_s": round(wall, 3), "bam_bytes": os.path.getsize(f) if os.path.isfile(f) else None}
            if srt == "Device":
                r["finish_split"] = sort_split(text)
            if more:
                r["signal"] = signal_split(text)
                sig = sorted(q for q in os.listdir(rd) if q.startswith("bamsort_%s_Signal." % tag))
                r["signal_bytes"] = sum(os.path.getsize(os.path.join(rd, q)) for q in sig)
                h = hashlib.sha256()
                for q in sig:                                       # the two sides must write the same files
                    h.update(q[len("bamsort_%s_" % tag):].encode() + b"\0" + open(os.path.join(rd, q), "rb").read())
                    os.remove(os.path.join(rd, q))
                r["signal_sha256"] = h.hexdigest()
            leg[tag].append(r)
            if os.path.isfile(f):
                os.remove(f)
    out["sorted_by_coordinate_signal_leg" if wig else "sorted_by_coordinate_sort_leg"] = leg
    print(json.dumps(out))


if __name__ == "__main__":
    main()
