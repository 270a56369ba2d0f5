#!/usr/bin/env python3
"""bench.py's BAM leg (the `bam_output` configuration, same argv as bench.py:bam_leg, through capi.run_cli) once with --gpuBAMcompression Host and once
with Device, on the same box.  One JSON line: M pairs/s in the timed region, BAM bytes, device bytes / host bytes, and the split of the device
compression (STARAMD_HOST_TIMING lines of k_bgzf.hip: host staging copy, H2D, kernels, D2H, copy out; summed over the run).
  python tools/bam_device_leg.py [--reads N ...bench.py flags] [ENV=V ...]     (GPU box)"""
import json, os, re, sys, tempfile, time
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


def main():
    env = [a for a in sys.argv[1:] if "=" in a and not a.startswith("-")]
    for a in env:
        k, v = a.split("=", 1)
        os.environ[k] = v
    sys.argv = [sys.argv[0]] + [a for a in sys.argv[1:] if a not in env]
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
    for name, typ in (("unsorted", ["BAM", "Unsorted"]), ("sorted_by_coordinate", ["BAM", "SortedByCoordinate"])):
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
    print(json.dumps(out))


if __name__ == "__main__":
    main()
