#!/usr/bin/env python3
"""The cost of --genomeFastaFiles at the mapping stage on the 3.1 Gb index bench.py keeps in --workdir (run bench.py first: this tool builds nothing):
the shipped binary maps 1000 pairs with (a) no added references, (b) 92 added sequences of about 1 kb, (c) one of 5 Mb, STARAMD_VERBOSE=1, so that every
stage of staramd_seq_insert (star_amd/csrc/index/seq_core.h: be.stage) and the two PCIe copies print their wall time.  Runs alternate after one unrecorded
run; reported per leg: the stage times, the HIP-event total of the Log.out line, and the wall time of the whole process (index load to the last record:
the mapping itself is 1000 pairs).  The merge's bytes/s: it reads the old packed array and writes the new one once.
    python tools/seq_insert_leg.py [--workdir DIR] [--repeats 2] [--out profiles/seq_insert_leg.json]      (GPU box)"""
import argparse
import glob
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "star_amd", "bin", "star_amd")


def write_fasta(path, lens, seed):
    rng = np.random.default_rng(seed)
    with open(path, "w") as f:
        for i, n in enumerate(lens):
            f.write(">added%d\n" % (i + 1))
            s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes().decode()
            for k in range(0, n, 80):
                f.write(s[k:k + 80] + "\n")


def run(idx, fq, prefix, fasta):
    cmd = [BIN, "--genomeDir", idx, "--readFilesIn"] + fq + ["--outFileNamePrefix", prefix, "--outSAMtype", "None", "--runThreadN", "16"]
    if fasta:
        cmd += ["--genomeFastaFiles", fasta]
    t = time.time()
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=dict(os.environ, STARAMD_VERBOSE="1"), timeout=900)
    wall = time.time() - t
    if p.returncode != 0:
        raise RuntimeError(p.stderr[-2000:])
    stages = {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"staramd index stage (seq: .*?)\s+([0-9.]+) ms", p.stderr)}
    out = {"wall_s": round(wall, 2), "stages_ms": stages}
    m = re.search(r"sequence insertion on the device: ([0-9.]+) ms, (\d+) doubling rounds", open(prefix + "Log.out").read())
    if m:
        out["hip_event_total_ms"] = float(m.group(1)); out["doubling_rounds"] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workdir", default=os.environ.get("STARAMD_BENCH_DIR", "/dev/shm/star_amd_bench"))
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_insert_leg.json"))
    a = ap.parse_args()
    dirs = sorted(glob.glob(os.path.join(a.workdir, "genome_3100mb_*")))
    if not dirs or not os.path.isfile(os.path.join(dirs[-1], "idx", "SA")):
        sys.exit("no 3.1 Gb index under %s: run bench.py first" % a.workdir)
    g = dirs[-1]; idx = os.path.join(g, "idx")
    w = os.path.join(a.workdir, "seq_insert_leg"); os.makedirs(w, exist_ok=True)
    fqs = sorted(glob.glob(os.path.join(g, "**", "*_1.fq"), recursive=True))
    if not fqs:
        sys.exit("no FASTQ of bench.py under " + g)
    fq = []
    for m in (1, 2):
        src = fqs[0][:-5] + "_%d.fq" % m
        dst = os.path.join(w, "r_%d.fq" % m)
        with open(src) as i, open(dst, "w") as o:
            for _ in range(4000):
                o.write(i.readline())
        fq.append(dst)
    legs = {"none": None, "92x1kb": os.path.join(w, "ercc.fa"), "1x5Mb": os.path.join(w, "big.fa")}
    write_fasta(legs["92x1kb"], [int(x) for x in np.random.default_rng(3).integers(500, 2000, 92)], 11)
    write_fasta(legs["1x5Mb"], [5000000], 12)
    sa_bytes = os.path.getsize(os.path.join(idx, "SA"))
    res = {"index": idx, "SA_bytes": sa_bytes, "Genome_bytes": os.path.getsize(os.path.join(idx, "Genome")), "repeats": a.repeats, "legs": {k: [] for k in legs}}
    run(idx, fq, os.path.join(w, "warm_"), legs["92x1kb"])                      # unrecorded
    for r in range(a.repeats):
        for k, fa in legs.items():
            res["legs"][k].append(run(idx, fq, os.path.join(w, "%s_%d_" % (k, r)), fa))
            print(k, r, json.dumps(res["legs"][k][-1]), flush=True)
    for k in ("92x1kb", "1x5Mb"):
        ms = [x["stages_ms"].get("seq: merge") for x in res["legs"][k] if x["stages_ms"].get("seq: merge")]
        if ms:
            res["merge_TBps_" + k] = [round(2 * sa_bytes / (m * 1e-3) / 1e12, 3) for m in ms]
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k.startswith("merge")}))


if __name__ == "__main__":
    main()
