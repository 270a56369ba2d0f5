#!/usr/bin/env python3
"""The duplicate marking of --runMode inputAlignmentsFromBAM --bamRemoveDuplicatesType UniqueIdentical, timed three ways on one box: --gpuBAMdedup Host,
--gpuBAMdedup Device, and the reference binary where oracle/_ref/STAR is built.  Input: the newest Aligned.sortedByCoord.out.bam under bench.py's
workdir when one is there (--workdir, default bench.py's), else a fabricated coordinate-sorted paired-end file of --pairs read pairs (seeded: a third
of the pairs duplicates of another, one class of --deep pairs on one position, 5 % multi-mappers).
Host and Device are alternated, --repeats times each after one unrecorded run of each (first launches load code objects); a difference smaller than
the spread of the repeats is no difference.  Times: the wall time of the tool mode, its stage clocks (STARAMD_HOST_TIMING lines of host/dedup.cpp:
load and inflate, mark, compress and write), the device's own split (k_dedup.hip's line: upload, scan, pairing, classes, survivor, D2H) and
staramd_dedup_result::stats[6..7].  The two paths must write the same file.  One JSON document, to stdout and to --out.
  python tools/dedup_leg.py [--pairs N] [--deep N] [--repeats N] [--out profiles/bam_dedup_device_leg.json]     (GPU box)
With --inflate the two forms of --gpuBAMinflate are alternated instead, --gpuBAMdedup Device in both, on two fabricated files: the one above
(level 1, names in order and one quality string: it compresses about 12 : 1, far more than a real BAM) and one with random names, bases and qualities written at
level 6 (about 4 : 1).  Per run: the tool mode's wall time, `load and inflate`, and for Device its parts -- file read, header walk, H2D, kernel (stream events),
D2H, copy into place, record parse.
  python tools/dedup_leg.py --inflate [--pairs N] [--repeats N] [--out profiles/bam_inflate_device_leg.json]"""
import argparse
import glob
import hashlib
import json
import os
import random
import re
import shutil
import struct
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from star_amd import capi  # noqa: E402

REF_BIN = os.path.join(ROOT, "oracle", "_ref", "STAR")
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def fabricate(path, pairs, deep, seed=1, randomise=False, level=1):
    """a coordinate-sorted paired-end BAM: 2 * pairs unique records + 5 % multi-mappers, 2x76, two chromosomes.  randomise: names, bases and qualities drawn at
    random per record (a pair's mates share the name), as a sequencer's are"""
    r = random.Random(seed)
    chroms = [("chr1", 120000000), ("chr2", 80000000)]
    seqq = bytes([0x12, 0x48] * 19) + b"\x1e" * 76
    if randomise:
        import numpy as np
        g = np.random.default_rng(seed)
        n_rec = 2 * pairs + pairs // 10
        bases = np.array([1, 2, 4, 8], dtype=np.uint8)[g.integers(0, 4, size=(n_rec, 76))]
        packed = (bases[:, 0::2] << 4 | bases[:, 1::2]).astype(np.uint8)
        quals = np.array([37] * 125 + [25, 11, 2], dtype=np.uint8)[g.integers(0, 128, size=(n_rec, 76))]
        rows = np.concatenate([packed, quals], axis=1)
        names = g.integers(0, 10 ** 9, size=pairs + pairs // 10)
    cigs = [struct.pack("<I", 76 << 4), struct.pack("<II", 5 << 4 | 4, 71 << 4), struct.pack("<III", 30 << 4, 900 << 4 | 3, 46 << 4)]
    recs = []

    def one(tid, pos, mpos, flag, name, cig, nh, AS):
        sq = rows[len(recs)].tobytes() if randomise else seqq
        body = struct.pack("<iiIIiiii", tid, pos, 3 << 8 | len(name), flag << 16 | len(cig) // 4, 76, tid, mpos, 0) + name + cig + sq + b"NHC" + bytes([nh]) + b"ASC" + bytes([AS])
        recs.append((tid << 32 | pos, struct.pack("<I", len(body)) + body))

    tmpl = []
    n_tmpl = pairs - pairs // 3 - deep
    for i in range(pairs):
        if i < n_tmpl:
            tid = r.randrange(2)
            p1 = r.randrange(1000, chroms[tid][1] - 2000)
            t = (tid, p1, p1 + r.randrange(0, 500), r.choice(cigs), r.choice(cigs))
            tmpl.append(t)
        elif i < n_tmpl + deep:
            t = (0, 5000000, 5000200, cigs[0], cigs[0])
        else:
            t = tmpl[r.randrange(n_tmpl)]
        name = b"p%09d\0" % (names[i] if randomise else i)
        one(t[0], t[1], t[2], 0x63, name, t[3], 1, r.randrange(40, 150))
        one(t[0], t[2], t[1], 0x93, name, t[4], 1, r.randrange(40, 150))
    for i in range(pairs // 10):
        tid = r.randrange(2)
        one(tid, r.randrange(1000, chroms[tid][1] - 2000), 0, r.choice([0x63, 0x93]), b"m%09d\0" % (names[pairs + i] if randomise else i), cigs[0], 3, 70)
    recs.sort(key=lambda x: x[0])
    text = b"@HD\tVN:1.4\tSO:coordinate\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (c.encode(), n) for c, n in chroms)
    head = b"BAM\1" + struct.pack("<I", len(text)) + text + struct.pack("<I", len(chroms))
    for c, n in chroms:
        head += struct.pack("<I", len(c) + 1) + c.encode() + b"\0" + struct.pack("<I", n)
    data = head + b"".join(x[1] for x in recs)
    with open(path, "wb") as f:
        for o in range(0, len(data), 0xff00):
            chunk = data[o:o + 0xff00]
            c = zlib.compressobj(level, zlib.DEFLATED, -15)
            d = c.compress(chunk) + c.flush()
            f.write(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(d) + 25) + d + struct.pack("<II", zlib.crc32(chunk), len(chunk)))
        f.write(EOF)
    return len(recs), len(data)


def captured(fn):
    """fn() with this process's stderr (fd 2) going to a file as well: the C++ side prints its timing lines there"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        try:
            out = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        return out, f.read().decode(errors="replace")


def tool_run(bam, prefix, mode, threads, inflate=None, digest=True):
    argv = ["--runMode", "inputAlignmentsFromBAM", "--inputBAMfile", bam, "--outFileNamePrefix", prefix, "--bamRemoveDuplicatesType", "UniqueIdentical", "--gpuBAMdedup", mode,
            "--runThreadN", str(threads), "--outBAMcompression", "1"] + (["--gpuBAMinflate", inflate] if inflate else [])

    def go():
        t = time.perf_counter()
        run = capi.HostRun(argv)
        wall = time.perf_counter() - t
        counts = run.dedup_counts()
        run.close()
        return wall, counts

    (wall, counts), text = captured(go)
    row = {"wall_s": round(wall, 4), "records": counts[0], "unique": counts[1], "pairs": counts[2], "classes": counts[3], "marked": counts[4], "unpaired": counts[5]}
    m = re.search(r"dedup stage \((host|device)\): load and inflate ([0-9.]+) ms, mark ([0-9.]+) ms, compress and write ([0-9.]+) ms", text)
    if m:
        row.update(side=m.group(1), load_ms=float(m.group(2)), mark_ms=float(m.group(3)), write_ms=float(m.group(4)))
    m = re.search(r"dedup device: .*: upload ([0-9.]+) ms, scan ([0-9.]+) ms, pairing ([0-9.]+) ms, classes ([0-9.]+) ms, survivor ([0-9.]+) ms, D2H ([0-9.]+) ms", text)
    if m:
        row["device_split_ms"] = dict(zip(("upload", "scan", "pairing", "classes", "survivor", "D2H"), (float(x) for x in m.groups())))
        row["stats_kernels_ms"] = round(counts[6] / 1e6, 3); row["stats_copies_ms"] = round(counts[7] / 1e6, 3)
    m = re.search(r"inflate device: (\d+) members, .*: header walk ([0-9.]+) ms, H2D ([0-9.]+) ms, kernel ([0-9.]+) ms, D2H ([0-9.]+) ms", text)
    if m:
        row["inflate_members"] = int(m.group(1))
        row["inflate_device_ms"] = dict(zip(("header_walk", "H2D", "kernel", "D2H"), (float(x) for x in m.groups()[1:])))
    m = re.search(r"inflate stage \(device\): file read ([0-9.]+) ms, walk \+ device ([0-9.]+) ms, copy into place ([0-9.]+) ms", text)
    if m:
        row["inflate_stage_ms"] = dict(zip(("file_read", "walk_and_device_call", "copy_into_place"), (float(x) for x in m.groups())))
    m = re.search(r"load: inflate ([0-9.]+) ms, header and record parse ([0-9.]+) ms", text)
    if m:
        row["load_split_ms"] = {"inflate": float(m.group(1)), "record_parse": float(m.group(2))}
    if not digest:
        os.remove(prefix + "Processed.out.bam")
        return row
    import gzip
    h = hashlib.sha256()
    with gzip.open(prefix + "Processed.out.bam", "rb") as f:
        for block in iter(lambda: f.read(1 << 24), b""):
            h.update(block)
    row["inflated_sha256"] = h.hexdigest()
    os.remove(prefix + "Processed.out.bam")
    return row


def inflate_leg(args):
    """--inflate: Host and Device forms of --gpuBAMinflate alternated on two fabricated inputs"""
    work = tempfile.mkdtemp(prefix="staramd_inflate_leg_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    out = {"what": "tools/dedup_leg.py --inflate on one MI355X: the tool mode --bamRemoveDuplicatesType UniqueIdentical --gpuBAMdedup Device with --gpuBAMinflate Host and Device alternated "
                   "(%d times each after one unrecorded run of each); --runThreadN %d, --outBAMcompression 1.  load_ms is the stage clock `load and inflate` of host/dedup.cpp; Host is "
                   "gzread on one thread" % (args.repeats, args.threads), "inputs": []}
    dd, infl = capi.DedupDevice(lib_path=args.lib), capi.InflateDevice(lib_path=args.lib)
    dd.install(); infl.install()
    med = lambda xs: sorted(xs)[len(xs) // 2]
    try:
        for tag, randomise, level in (("ordered names, one quality string, level 1", False, 1), ("random names, bases and qualities, level 6", True, 6)):
            bam = os.path.join(work, "fabricated_%d.bam" % level)
            t = time.perf_counter()
            n, raw = fabricate(bam, args.pairs, args.deep, randomise=randomise, level=level)
            entry = {"input": {"source": "fabricated: " + tag, "pairs": args.pairs, "records": n, "inflated_bytes": raw, "bam_bytes": os.path.getsize(bam),
                               "ratio": round(raw / os.path.getsize(bam), 2), "made_in_s": round(time.perf_counter() - t, 1)}}
            for mode in ("Host", "Device"):
                tool_run(bam, os.path.join(work, "warm_%s_" % mode), "Device", args.threads, inflate=mode, digest=False)
            rows = {"Host": [], "Device": []}
            for i in range(args.repeats):
                for mode in ("Host", "Device"):
                    rows[mode].append(tool_run(bam, os.path.join(work, "%s%d_" % (mode, i)), "Device", args.threads, inflate=mode, digest=i == 0))
            entry.update(rows)
            entry["same_file"] = rows["Host"][0]["inflated_sha256"] == rows["Device"][0]["inflated_sha256"]
            entry["summary"] = {m: {"wall_s_median": med([r["wall_s"] for r in rows[m]]), "wall_s_min_max": [min(r["wall_s"] for r in rows[m]), max(r["wall_s"] for r in rows[m])],
                                    "load_ms_median": med([r.get("load_ms", 0) for r in rows[m]]), "load_ms_min_max": [min(r.get("load_ms", 0) for r in rows[m]), max(r.get("load_ms", 0) for r in rows[m])]}
                                for m in rows}
            out["inputs"].append(entry)
            os.remove(bam)
    finally:
        capi.DedupDevice.uninstall(); capi.InflateDevice.uninstall()
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text + "\n")
    print(text)
    shutil.rmtree(work, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inflate", action="store_true", help="alternate --gpuBAMinflate Host and Device instead (two fabricated inputs); default --out profiles/bam_inflate_device_leg.json")
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--deep", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--workdir", default=os.environ.get("STARAMD_BENCH_DIR", "/dev/shm/star_amd_bench" if os.path.isdir("/dev/shm") else "/tmp/star_amd_bench"))
    ap.add_argument("--lib", default=None, help="another library with the ABI of include/star_amd_dedup.h (a rehearsal of this tool without a device; its times mean nothing)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "bam_inflate_device_leg.json" if args.inflate else "bam_dedup_device_leg.json")
    os.environ["STARAMD_HOST_TIMING"] = "1"
    if args.inflate:
        return inflate_leg(args)
    found = sorted(glob.glob(os.path.join(args.workdir, "**", "*Aligned.sortedByCoord.out.bam"), recursive=True), key=os.path.getmtime)
    work = tempfile.mkdtemp(prefix="staramd_dedup_leg_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    out = {"what": "tools/dedup_leg.py on one MI355X: the tool mode --bamRemoveDuplicatesType UniqueIdentical with --gpuBAMdedup Host and Device alternated (%d times each after one unrecorded "
                   "run of each), and the reference binary once; --runThreadN %d, --outBAMcompression 1" % (args.repeats, args.threads)}
    if found:
        bam = found[-1]
        out["input"] = {"source": "bench.py workdir", "file": os.path.basename(bam), "bam_bytes": os.path.getsize(bam)}
    else:
        bam = os.path.join(work, "fabricated.bam")
        t = time.perf_counter()
        n, raw = fabricate(bam, args.pairs, args.deep)
        out["input"] = {"source": "fabricated", "pairs": args.pairs, "records": n, "deep_class_pairs": args.deep, "inflated_bytes": raw, "bam_bytes": os.path.getsize(bam), "made_in_s": round(time.perf_counter() - t, 1)}
    dd = capi.DedupDevice(lib_path=args.lib)
    dd.install()
    try:
        for mode in ("Host", "Device"):
            tool_run(bam, os.path.join(work, "warm_%s_" % mode), mode, args.threads)
        rows = {"Host": [], "Device": []}
        for i in range(args.repeats):
            for mode in ("Host", "Device"):
                rows[mode].append(tool_run(bam, os.path.join(work, "%s%d_" % (mode, i)), mode, args.threads))
    finally:
        capi.DedupDevice.uninstall()
    out.update(rows)
    out["same_file"] = len({r["inflated_sha256"] for rs in rows.values() for r in rs}) == 1
    if os.path.isfile(REF_BIN):
        t = time.perf_counter()
        rc = subprocess.call([REF_BIN, "--runMode", "inputAlignmentsFromBAM", "--inputBAMfile", bam, "--outFileNamePrefix", os.path.join(work, "ref_"), "--bamRemoveDuplicatesType", "UniqueIdentical",
                              "--limitBAMsortRAM", str(max(300000000, 2 * out["input"].get("inflated_bytes", 8 * os.path.getsize(bam)))), "--outBAMcompression", "1"], stdout=subprocess.DEVNULL, cwd=work)
        out["reference"] = {"exit_code": rc, "wall_s": round(time.perf_counter() - t, 3), "note": "single-threaded; its wall time includes inflating and a level-1 deflate of the whole file, like wall_s of the two paths"}
    else:
        out["reference"] = None
    med = lambda xs: sorted(xs)[len(xs) // 2]
    out["summary"] = {m: {"wall_s_median": med([r["wall_s"] for r in rows[m]]), "wall_s_min_max": [min(r["wall_s"] for r in rows[m]), max(r["wall_s"] for r in rows[m])],
                          "mark_ms_median": med([r.get("mark_ms", 0) for r in rows[m]]), "mark_ms_min_max": [min(r.get("mark_ms", 0) for r in rows[m]), max(r.get("mark_ms", 0) for r in rows[m])]} for m in rows}
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text + "\n")
    print(text)
    shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
