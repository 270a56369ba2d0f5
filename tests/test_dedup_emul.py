"""k_dedup.hip (--gpuBAMdedup Device, include/star_amd_dedup.h) compiled for the host by the wave emulator beside k_bgzf.hip, k_bamsort.hip and k_signal.hip:
on every vector below and every option set the bytes and counts it returns are those of the host path (dedupOnHost of host/dedup.cpp, pinned to the
reference in tests/test_dedup.py) -- also with STARAMD_DEDUP_HASH_BITS=3 and =0, where nearly every sorted run holds different names and contents and the
exact-order path decides -- and the tool mode with --gpuBAMdedup Device writes the host's file.  This module also holds the shared vectors (fabricated
records in coordinate order, made by seeded generators), their record builder and a Python restatement of the rule; tests/test_dedup.py
and the GPU tests (tests/test_gpu_dedup.py) use them."""
import ctypes as C
import os
import random
import struct
import subprocess
import tempfile

import pytest

from util import ROOT, capi, bam_parts
import test_signal_emul as G

CHROMS = [("chrA", 200000), ("chrB", 200000), ("chrC", 50000)]
NH_FATAL = "EXITING because of fatal ERROR: SAM tag NH is missing from a read, but it's required for deduplication. \nSOLUTION: re-generate BAM file with NH and AS tags."
AS_FATAL = NH_FATAL.replace("tag NH", "tag AS")
TYPES = {True: "UniqueIdentical", False: "UniqueIdenticalNotMulti"}
OPTION_SETS = [(mm, n) for mm in (True, False) for n in (0, 3)]
_PACK = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}
_EMUL = {}


def emul_lib():
    """k_bgzf.hip + k_bamsort.hip + k_signal.hip + k_dedup.hip + the wave emulator's runtime in a temporary shared library, built once per process by the
    recipe of util.emul_units_lib; oracle/ is only read"""
    if "so" not in _EMUL:
        d = tempfile.mkdtemp(prefix="staramd_dedup_emul_")
        cl = os.environ.get("EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
        hipfl = ["-x", "c++", "-std=c++17", "-O1", "-fPIC", "-Wno-unknown-attributes", "-I", "oracle/wave_emul"]
        jobs = [("star_amd/csrc/engine/%s.hip" % u, hipfl) for u in ("k_bgzf", "k_bamsort", "k_signal", "k_dedup")]
        jobs += [("oracle/wave_emul/emu.cpp", ["-std=c++17", "-O1", "-fPIC", "-D_GNU_SOURCE"]), ("oracle/wave_emul/emu_lds.cpp", ["-std=c++17", "-O1", "-fPIC"])]
        procs, objs = [], []
        for src, fl in jobs:
            o = os.path.join(d, os.path.basename(src) + ".o")
            procs.append(subprocess.Popen([cl] + fl + ["-c", src, "-o", o], cwd=ROOT))
            objs.append(o)
        assert all(p.wait() == 0 for p in procs)
        so = os.path.join(d, "libdedup_units_emul.so")
        subprocess.check_call([cl, "-shared", "-fPIC"] + objs + ["-o", so, "-ldl"], cwd=ROOT)
        _EMUL["so"] = so
    return _EMUL["so"]


# ---- fabricated records ---------------------------------------------------------------------------------------------------------------------------

def attr(tag, val, typ):
    return b"" if val is None else tag + typ.encode() + struct.pack(_PACK[typ], val)


def drec(tid, pos, cigar, flag, name, nh=1, AS=50, nh_typ="C", as_typ="C", seq=None, mtid=None, mpos=-1, pre=b"", post=b"", cut=0):
    """one BAM record with its block_size word.  cigar: [(length, op letter)]; seq: base letters (default: ACGT repeated over the CIGAR's read length);
    nh / AS None = absent; cut: bytes taken off the record's end (block_size says so)"""
    ops = b"".join(struct.pack("<I", n << 4 | "MIDNSHP=X".index(c)) for n, c in cigar)
    if seq is None:
        seq = ("ACGT" * (1 + sum(n for n, c in cigar if c in "MIS=X") // 4))[:sum(n for n, c in cigar if c in "MIS=X")]
    codes = ["=ACMGRSVTWYHKDBN".index(b) for b in seq] + [0]
    packed = bytes(codes[i] << 4 | codes[i + 1] for i in range(0, len(seq), 2))
    nm = name + b"\0"
    body = struct.pack("<iiIIiiii", tid, pos, 3 << 8 | len(nm), flag << 16 | len(cigar), len(seq), tid if mtid is None else mtid, mpos, 0) + nm + ops + packed + b"\x1e" * len(seq)
    body += pre + attr(b"NH", nh, nh_typ) + attr(b"AS", AS, as_typ) + post
    body = body[:len(body) - cut]
    return struct.pack("<I", len(body)) + body


M50 = [(50, "M")]


def pair(name, tid, p1, p2, c1=M50, c2=M50, f1=0x63, f2=0x93, as1=50, as2="same", **kw):
    """the two records of a read pair (mate 1, mate 2) with each other's position; kw1_* / kw2_* go to one mate only, the rest to both"""
    k1 = {k[4:]: v for k, v in kw.items() if k.startswith("kw1_")}
    k2 = {k[4:]: v for k, v in kw.items() if k.startswith("kw2_")}
    both = {k: v for k, v in kw.items() if not k.startswith("kw")}
    return [drec(tid, p1, c1, f1, name, AS=as1, mpos=p2, **dict(both, **k1)), drec(tid, p2, c2, f2, name, AS=as1 if as2 == "same" else as2, mpos=p1, **dict(both, **k2))]


def unmapped(name, flag=0x4d, nh=0):
    return drec(-1, -1, [], flag, name, nh=nh, AS=None, nh_typ="i", seq="ACGTACGTAC")


# ---- the rule, restated (steps 1-5 and what holds outside the domain) -------------------------------------------------------------------

def _u32(r, o):
    return struct.unpack_from("<I", r, o)[0]


def _aux(r, a, lim):
    """{tag: value} of the integer reading of every first occurrence, with every read inside lim (bamAuxInts)"""
    out = {}
    while a + 3 <= lim:
        tag, t = r[a:a + 2], chr(r[a + 2])
        a += 3
        if t in "AcC":
            w = 1
        elif t in "sS":
            w = 2
        elif t in "iIf":
            w = 4
        elif t in "ZH":
            j = a
            while j < lim and r[j] != 0:
                j += 1
            w = j - a + 1
        elif t == "B":
            if a + 5 > lim:
                break
            w = 5 + _u32(r, a + 1) * {"c": 1, "C": 1, "s": 2, "S": 2}.get(chr(r[a]), 4)
        else:
            break
        if tag not in out:
            out[tag] = struct.unpack_from(_PACK[t], r, a)[0] if t in _PACK and a + w <= lim else 0
        a += w
    return out


class View:
    def __init__(self, r):
        lim = min(len(r), 4 + _u32(r, 0))
        self.tid, self.pos, bmn, fnc, self.lseq = struct.unpack_from("<IIIII", r, 4)
        self.flag, ncd, lname = fnc >> 16, fnc & 0xffff, bmn & 0xff
        self.name = r[36:min(36 + lname, lim)]
        cig, self.seq, self.lim, self.r = 36 + lname, 36 + lname + 4 * ncd, lim, r
        n = ncd if self.seq <= lim else ((lim - cig) // 4 if cig < lim else 0)
        w = [_u32(r, cig + 4 * j) for j in range(n)]
        lead = n >= 2 and w[0] & 15 == 4
        trail = n - lead >= 2 and w[-1] & 15 == 4
        self.startS = (self.pos - (w[0] >> 4)) & 0xffffffff if lead else self.pos
        cs = w[lead:n - trail]
        if lead:
            cs[0] = (cs[0] + (w[0] & ~15)) & 0xffffffff
        if trail:
            cs[-1] = (cs[-1] + (w[-1] & ~15)) & 0xffffffff
        self.cigarS = tuple(cs)
        aux = _aux(r, self.seq + (self.lseq + 1) // 2 + self.lseq, lim)
        i32 = lambda v: None if v is None else (v & 0xffffffff) - (1 << 32) if v & 0x80000000 else v & 0xffffffff
        self.nh, self.AS = i32(aux.get(b"NH")), i32(aux.get(b"AS"))

    def bases(self, n):
        nb = min(n, self.lseq)
        idx = [self.lseq - nb + j if self.flag & 0x10 else j for j in range(nb)]
        return tuple((self.r[self.seq + i // 2] >> (0 if i & 1 else 4)) & 15 if self.seq + i // 2 < self.lim else 0 for i in idx)

    def name_key(self):
        return (len(self.name), bytes((b + 128) & 255 for b in self.name))      # the reference compares `char`


def restate(records, mark_multi, n_bases):
    """(final 0x400 bit per record, [records, unique, pairs, classes, marked, unpaired]) or ("fatal", 1 | 2, record)"""
    v = [View(r) for r in records]
    for i, x in enumerate(v):
        if x.nh is None:
            return "fatal", 1, i
    bit = [x.flag >> 10 & 1 for x in v]
    names = {}
    for i, x in enumerate(v):
        if x.nh == 1:
            bit[i] = 0
            names.setdefault((x.tid, x.name), []).append(i)
        elif x.nh > 1 and mark_multi:
            bit[i] = 1
    pairs = []
    for ids in names.values():
        if len(ids) == 2 and (v[ids[0]].flag ^ v[ids[1]].flag) & 0x80:
            pairs.append((ids[1], ids[0]) if v[ids[0]].flag & 0x80 else (ids[0], ids[1]))
    no_as = [m1 for m1, _ in pairs if v[m1].AS is None]
    if no_as:
        return "fatal", 2, min(no_as)
    classes = {}
    for m1, m2 in pairs:
        a, b = v[m1], v[m2]
        classes.setdefault((a.tid, a.startS, b.startS, a.flag & ~0x400, b.flag & ~0x400, a.cigarS, b.cigarS, b.bases(n_bases)), []).append((m1, m2))
    for members in classes.values():
        best = min(members, key=lambda p: (-v[p[0]].AS, v[p[0]].name_key()))
        for p in members:
            if p != best:
                bit[p[0]] = bit[p[1]] = 1
    n_u = sum(len(ids) for ids in names.values())
    return bit, [len(v), n_u, len(pairs), len(classes), sum(bit), n_u - 2 * len(pairs)]


def apply_bits(records, bits):
    out = []
    for r, b in zip(records, bits):
        w = _u32(r, 16)
        out.append(r[:16] + struct.pack("<I", w | 0x400 << 16 if b else w & ~(0x400 << 16)) + r[20:])
    return out


# ---- vectors ------------------------------------------------------------------------------------------------------------------------------------------

BASES_D = range(6)          # one_of_each: a pair of pairs per (mate 2 reverse?, l_seq, d) that differ in the d-th base from mate 2's 5' end alone


def _one_of_each():
    v, k = [], 0

    def trio(tag, base, other):
        """A, its duplicate with a lower AS, and a pair that differs from A in one component alone"""
        return pair(b"A_" + tag, **dict(base, as1=60)) + pair(b"Adup_" + tag, **dict(base, as1=40)) + pair(b"B_" + tag, **dict(base, **other))

    for tag, other in ((b"tid", dict(tid=1)), (b"s1", dict(p1=5001)), (b"s2", dict(p2=5201)), (b"f1", dict(f1=0x61)), (b"f2", dict(f2=0x91)),
                       (b"cw", dict(c1=[(20, "M"), (11, "N"), (30, "M")])), (b"cn", dict(c2=[(24, "M"), (2, "I"), (24, "M")]))):
        base = dict(tid=0, p1=5000 + 1000 * k, p2=5200 + 1000 * k, c1=[(20, "M"), (10, "N"), (30, "M")])
        if "p1" in other:
            other = dict(p1=base["p1"] + 1)
        if "p2" in other:
            other = dict(p2=base["p2"] + 1)
        v += trio(tag, base, other)
        k += 1
    for rev in (0, 1):
        for lseq in (50, 51):
            for d in BASES_D:
                s = ("ACGT" * 13)[:lseq]
                i = lseq - 1 - d if rev else d
                s2 = s[:i] + ("T" if s[i] != "T" else "G") + s[i + 1:]
                fl = dict(f1=0x63, f2=0x93) if rev else dict(f1=0x53, f2=0xa3)
                base = dict(tid=2, p1=1000 + 400 * k, p2=1100 + 400 * k, c1=[(lseq, "M")], c2=[(lseq, "M")], **fl)
                v += pair(b"X_%d" % k, as1=70, kw2_seq=s, **base) + pair(b"Y_%d" % k, as1=30, kw2_seq=s2, **base)
                k += 1
    return v


def one_of_each_marked(n_bases):
    """records that end marked in one_of_each: the seven duplicates, and of the 24 base groups those whose difference lies behind the bases compared"""
    return 2 * (7 + 4 * sum(1 for d in BASES_D if d >= n_bases))


def _clips():
    S = lambda *c: [(int(x[:-1]), x[-1]) for x in c]
    v = pair(b"c1a", 0, 1005, 1300, c1=S("5S", "45M"), as1=60) + pair(b"c1b", 0, 1000, 1300, as1=50)                       # 5S45M at pos + 5 against 50M at pos
    v += pair(b"c2a", 0, 2000, 2300, c1=S("45M", "5S"), as1=60) + pair(b"c2b", 0, 2000, 2300, as1=50)                      # 45M5S against 50M
    v += pair(b"c3a", 0, 3000, 3303, c2=S("3S", "20M", "2I", "22M", "3S"), as1=60) + pair(b"c3b", 0, 3000, 3300, c2=S("23M", "2I", "25M"), as1=50)
    v += pair(b"c4a", 0, 4005, 4300, c1=S("5S", "3I", "42M"), as1=60) + pair(b"c4b", 0, 4000, 4300, c1=S("8I", "42M"), as1=50)      # a leading S before a non-M operation
    v += pair(b"c5a", 1, 2, 300, c1=S("5S", "45M"), as1=60) + pair(b"c5b", 1, 2, 300, c1=S("5S", "45M"), as1=50)           # the clip is longer than pos: startS wraps
    v += pair(b"c5c", 1, 2, 300, c1=S("2S", "48M"), as1=40) + pair(b"c5d", 1, 0, 300, as1=30)
    v += pair(b"c6a", 0, 6005, 6300, c1=S("5S", "45M"), as1=60) + pair(b"c6b", 0, 6005, 6300, as1=50)                      # same pos, different startS: no duplicate
    return v


def _scores():
    v, k = [], 0
    for typ, vals in (("c", (-5, 100, 30)), ("C", (10, 250, 30)), ("s", (-998, -3, -500)), ("S", (10, 60000, 30)), ("i", (-100, 70000, 5)), ("I", (10, 80000, 30))):
        for order in ((1, 0, 2), (0, 1, 2), (0, 2, 1)):                     # the best pair first, in the middle and last in file order
            for j in order:
                v += pair(b"s%d_%d" % (k, j), 0, 1000 + 300 * k, 1100 + 300 * k, as1=vals[j], as_typ=typ)
            k += 1
    v += pair(b"m2big_x", 1, 1000, 1200, as1=10, as2=200) + pair(b"m2big_y", 1, 1000, 1200, as1=20, as2=5)                 # mate 2's AS is never read
    v += pair(b"m2none_x", 1, 2000, 2200, as1=10, as2=None) + pair(b"m2none_y", 1, 2000, 2200, as1=20, as2=None)
    return v


def _ties():
    r = random.Random(5)
    v = pair(b"t_b", 0, 1000, 1200) + pair(b"t_a", 0, 1000, 1200) + pair(b"t_c", 0, 1000, 1200)
    names = [b"z%02d" % i for i in range(39)] + [b"z0"]                                                                    # equal lengths, and a prefix of another
    r.shuffle(names)
    for nm in names:
        v += pair(nm, 0, 3000, 3200, as1=77)
    return v


def _multi():
    v = []
    for i, (nh, typ) in enumerate(((2, "C"), (3, "s"), (70000, "I"), (70000, "i"))):
        for j, fl in enumerate((0x63, 0x463, 0x93, 0x493)):                                                                 # with and without 0x400 in the input
            v.append(drec(0, 1000 + 100 * i + 10 * j, M50, fl, b"mm%d_%d" % (i, j), nh=nh, nh_typ=typ, mpos=1000))
    v += pair(b"u_alone", 0, 5000, 5200, f1=0x463, f2=0x493)                                                                # unique, preset, a class of one: ends clear
    v += pair(b"u_best", 0, 6000, 6200, f1=0x463, f2=0x493, as1=90) + pair(b"u_dup", 0, 6000, 6200, as1=10)                # the preset bit does not part the class
    v += [unmapped(b"un1", 0x4d), unmapped(b"un1", 0x8d), unmapped(b"un2", 0x44d), unmapped(b"un2", 0x48d)]
    return v


def _layout():
    r = random.Random(6)
    v = pair(b"far_a", 0, 1000, 150000, as1=60) + pair(b"far_b", 0, 1000, 150000, as1=40)                                   # mates hundreds of records apart
    for i in range(200):                                                                                                   # chains of overlapping pairs
        v += pair(b"ch%d" % i, 0, 2000 + 100 * i, 2150 + 100 * i, as1=50)
        if i % 5 == 0:
            v += pair(b"ch%d_d" % i, 0, 2000 + 100 * i, 2150 + 100 * i, as1=10 + r.randrange(30))
    v += pair(b"same_a", 1, 7000, 7000, as1=60) + pair(b"same_b", 1, 7000, 7000, as1=40)                                   # both mates on one position
    v += pair(b"left2_a", 1, 9300, 9000, f1=0x53, f2=0xa3, as1=60) + pair(b"left2_b", 1, 9300, 9000, f1=0x53, f2=0xa3, as1=40)      # mate 2 leftmost
    v += [unmapped(b"un%d" % i, fl) for i in range(3) for fl in (0x4d, 0x8d)]
    return v


def _deep():
    """one class of 5 000 pairs with a unique best, next to classes of one"""
    best = 3217
    v = []
    for i in range(5000):
        v += pair(b"deep%05d" % i, 0, 10000, 10200, as1=99 if i == best else 90 - i % 7, as2=1)
    for i in range(100):
        v += pair(b"single%d" % i, 0, 9000 + 17 * i, 10200 + 3 * i, as1=50)
    return v


def _many():
    """20 000 pairs, about a third of them duplicates, over three chromosomes; 2 000 multi-mappers in between.  No two pairs of a class share their AS"""
    r = random.Random(7)
    cig = [M50, [(5, "S"), (45, "M")], [(20, "M"), (300, "N"), (30, "M")], [(25, "M"), (1, "I"), (24, "M")], [(48, "M"), (2, "S")], [(20, "M"), (2, "D"), (30, "M")]]
    tmpl, used, v = [], [], []
    for i in range(13400):
        tid = r.randrange(3)
        p1 = r.randrange(100, (180000, 180000, 40000)[tid])
        fl = r.choice([dict(f1=0x63, f2=0x93), dict(f1=0x53, f2=0xa3)])
        p2 = p1 + r.randrange(0, 400)
        tmpl.append(dict(tid=tid, p1=p1 if fl["f1"] == 0x63 else p2, p2=p2 if fl["f1"] == 0x63 else p1, c1=r.choice(cig), c2=r.choice(cig), **fl))
        used.append(set())
    for i in range(20000):
        t = i if i < len(tmpl) else r.randrange(len(tmpl))
        a = r.randrange(60000)
        while a in used[t]:
            a = r.randrange(60000)
        used[t].add(a)
        v += pair(b"r%d" % i, as1=a, as2=r.randrange(200), as_typ="S", **tmpl[t])
    v += [drec(r.randrange(3), r.randrange(100, 40000), M50, r.choice([0x63, 0x93, 0x463]), b"mm%d" % i, nh=r.choice([2, 3, 7]), mpos=500) for i in range(2000)]
    return v


def _outside():
    S = lambda *c: [(int(x[:-1]), x[-1]) for x in c]
    long_c = [(1, "MI"[j % 2]) for j in range(150)]
    long_d = list(long_c)
    long_d[140] = (2, "M")
    seq50 = "ACGT" * 12 + "AC"
    return {
        "unpaired": pair(b"ok_a", 0, 1000, 1200, as1=60) + pair(b"ok_b", 0, 1000, 1200, as1=40) + pair(b"lone1", 0, 1000, 1200, as1=99)[:1] + pair(b"lone2", 0, 1000, 1200, as1=99)[1:]
                    + pair(b"far", 0, 3000, 3200)[:1] + pair(b"far", 1, 3000, 3200)[1:],                                    # the partner lies on another sequence
        "name_groups": pair(b"g3", 0, 1000, 1200) + pair(b"g3", 0, 1000, 1200)[:1] + pair(b"g4", 0, 2000, 2200) + pair(b"g4", 0, 2000, 2200)
                       + [x for x in pair(b"both1", 0, 3000, 3200, f2=0x63)] + pair(b"ok_a", 0, 1000, 1200, as1=60) + pair(b"ok_b", 0, 1000, 1200, as1=40),
        "empty": [],
        "odd_cigars": pair(b"nc_a", 0, 1000, 1200, c1=[], c2=[], as1=60, seq=seq50) + pair(b"nc_b", 0, 1000, 1200, c1=[], c2=[], as1=40, seq=seq50)
                      + pair(b"ls_a", 0, 2000, 2200, c1=S("50S"), as1=60) + pair(b"ls_b", 0, 2000, 2200, c1=S("50S"), as1=40) + pair(b"ls_c", 0, 2000, 2200, c1=S("49S"), as1=30, kw1_seq=seq50)
                      + pair(b"ss_a", 0, 3000, 3200, c1=S("20S", "30S"), as1=60) + pair(b"ss_b", 0, 2980, 3200, c1=S("50S"), as1=40),
        "low_as": pair(b"lo_a", 0, 1000, 1200, as1=-2000, as_typ="s") + pair(b"lo_b", 0, 1000, 1200, as1=-1500, as_typ="s") + pair(b"lo_c", 0, 1000, 1200, as1=-1000000, as_typ="i"),
        "long_cigar": pair(b"lc_a", 0, 1000, 1200, c1=long_c, as1=60) + pair(b"lc_b", 0, 1000, 1200, c1=long_c, as1=40) + pair(b"lc_c", 0, 1000, 1200, c1=long_d, as1=30),
        # the record's end falls inside the AS value (reads as 0), inside the NH value (NH = 0: untouched), and inside AS's tag of a mate 2 (absent, no error)
        "truncated": pair(b"tr_a", 0, 1000, 1200, as1=60, as_typ="i", kw1_cut=2) + pair(b"tr_b", 0, 1000, 1200, as1=-5, as_typ="c")
                     + pair(b"tr_c", 0, 2000, 2200, nh_typ="i", as1=None, as2=None, kw1_cut=1, f1=0x463) + pair(b"tr_d", 0, 3000, 3200, as1=50, kw2_cut=2) + pair(b"tr_e", 0, 3000, 3200, as1=40),
        "no_nh": pair(b"a", 0, 1000, 1200) + pair(b"b", 0, 2000, 2200, kw2_nh=None) + pair(b"c", 0, 3000, 3200, kw1_nh=None),
        "no_as": pair(b"a", 0, 1000, 1200) + pair(b"b", 0, 2000, 2200, as1=None, as2=7) + pair(b"c", 0, 1500, 2200, as1=None, as2=7),
        "no_both": pair(b"a", 0, 1000, 1200, as1=None, as2=7) + pair(b"b", 0, 2000, 2200, kw1_nh=None),
        "no_as_mate2": pair(b"a", 0, 1000, 1200, as1=60, as2=None) + pair(b"b", 0, 1000, 1200, as1=40, as2=None) + pair(b"lone", 0, 1000, 1200, as1=None)[:1],
    }


IN_DOMAIN = ["one_of_each", "clips", "scores", "ties", "multi", "layout", "deep", "many"]
OUTSIDE = ["unpaired", "name_groups", "empty", "odd_cigars", "low_as", "long_cigar", "truncated", "no_nh", "no_as", "no_both", "no_as_mate2"]
VECTOR_NAMES = IN_DOMAIN + OUTSIDE
_VEC = {}


def vectors():
    """name -> records in coordinate order; the same for the host path, the emulator and, in tests/test_gpu_dedup.py, the MI355X"""
    if not _VEC:
        made = {"one_of_each": _one_of_each(), "clips": _clips(), "scores": _scores(), "ties": _ties(), "multi": _multi(), "layout": _layout(), "deep": _deep(), "many": _many()}
        made.update(_outside())
        for name in VECTOR_NAMES:
            _VEC[name] = G.in_order(made[name])
    return _VEC


def options(name):
    """(markMulti, Mate2basesN) of a vector: both types x {0, 3}; one_of_each also with 1, 2 and 5 bases"""
    return OPTION_SETS + ([(True, n) for n in (1, 2, 5)] if name == "one_of_each" else [])


_WANT = {}


def expected(name, opt):
    """the restatement's answer, computed once"""
    if (name, opt) not in _WANT:
        _WANT[(name, opt)] = restate(vectors()[name], *opt)
    return _WANT[(name, opt)]


def as_result(answer):
    """a restatement answer in the shape of capi.DedupDevice.host_records / capi.dedup_host: (dup bytes or None, fatal, fatalRecord, stats[0..5])"""
    if answer[0] == "fatal":
        return None, answer[1], answer[2], None
    return bytes(answer[0]), 0, 0, answer[1]


def result_of(res):
    dup, fatal, rec, stats = res
    return (None, fatal, rec, None) if fatal else (dup, 0, 0, stats[:6])


def write_bam(path, records):
    return G.write_bam(path, records, CHROMS)


def tool_mode(bam, prefix, opt, device=False, more=()):
    """--runMode inputAlignmentsFromBAM --bamRemoveDuplicatesType in this process (everything happens in sah_create): the parts of Processed.out.bam, or the error text"""
    argv = ["--runMode", "inputAlignmentsFromBAM", "--inputBAMfile", bam, "--outFileNamePrefix", prefix, "--bamRemoveDuplicatesType", TYPES[opt[0]],
            "--bamRemoveDuplicatesMate2basesN", str(opt[1])] + (["--gpuBAMdedup", "Device"] if device else []) + list(more)
    try:
        capi.HostRun(argv).close()
    except RuntimeError as e:
        assert not os.path.exists(prefix + "Processed.out.bam"), "a fatal error leaves a partial file behind"
        return str(e)
    return bam_parts(prefix + "Processed.out.bam")


class HashBits:
    """STARAMD_DEDUP_HASH_BITS for the calls inside"""

    def __init__(self, bits):
        self.bits = bits

    def __enter__(self):
        self.old = os.environ.get("STARAMD_DEDUP_HASH_BITS")
        if self.bits is not None:
            os.environ["STARAMD_DEDUP_HASH_BITS"] = str(self.bits)

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("STARAMD_DEDUP_HASH_BITS", None)
        else:
            os.environ["STARAMD_DEDUP_HASH_BITS"] = self.old


# ---- the tests ------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dd(built):
    d = capi.DedupDevice(lib_path=emul_lib())
    d.install()
    yield d
    capi.DedupDevice.uninstall()


@pytest.fixture(scope="module")
def work():
    return tempfile.mkdtemp(prefix="staramd_dedup_emul_vec_")


def test_vectors_cover_the_cases(dd):
    v = vectors()
    assert list(v) == VECTOR_NAMES
    for name, recs in v.items():
        assert [G.key_of(x) for x in recs] == sorted(G.key_of(x) for x in recs), name
    # more classes and more name runs than a kernel has work-items in one sweep of its grid (the emulator has 2 CUs)
    st = expected("many", (True, 0))[1]
    sweep = dd.workgroup * dd.workgroups_per_cu * 2
    assert st[3] > sweep and st[2] > sweep and st[2] == 20000 and 0.3 < (st[2] - st[3]) / st[2] < 0.36, (st, sweep)
    assert expected("deep", (True, 0))[1][3] == 101


@pytest.mark.parametrize("bits", [None, 3, 0])
@pytest.mark.parametrize("name", VECTOR_NAMES)
def test_device_equals_host(dd, name, bits):
    """dup and stats[0..5] of the emulated kernels against the host path's, with whole and with cut hashes"""
    recs = vectors()[name]
    for opt in options(name):
        want = result_of(capi.dedup_host(recs, *opt))
        with HashBits(bits):
            got = result_of(dd.host_records(recs, *opt))
        assert got == want, (name, opt, bits, got[1:], want[1:], [i for i in range(len(recs)) if got[0] and want[0] and got[0][i] != want[0][i]][:10])
        assert want == as_result(expected(name, opt)), (name, opt)


def test_cut_hashes_reach_the_exact_order_path(dd):
    """With 3 bits a (tid, hash) key has 8 values per sequence: where a sequence holds more unique names than that, different names are sure to meet under
    one key (else the runs with cut hashes would show nothing).  With 0 bits the pairs of one numeric key stay in name order, and in one_of_each that
    order is A_cw, B_cw, Adup_cw (by length first): two contents interleaved under one key"""
    for name in ("layout", "many", "scores", "ties", "one_of_each"):
        per_tid = {}
        for r in vectors()[name]:
            x = View(r)
            if x.nh == 1:
                per_tid.setdefault(x.tid, set()).add(x.name)
        assert max(len(s) for s in per_tid.values()) > 8, name
    trio = sorted((View(r) for r in vectors()["one_of_each"] if View(r).name in (b"A_cw\0", b"B_cw\0", b"Adup_cw\0") and not View(r).flag & 0x80), key=View.name_key)
    assert [x.cigarS == trio[0].cigarS for x in trio] == [True, False, True]
    assert dd.max_workgroups() == 0 and (dd.workgroup, dd.workgroups_per_cu) == (256, 16)


def test_one_of_each_by_hand(built):
    """the vectors whose answer is known by construction: the restatement and the host path's rule both give the counts worked out by hand"""
    for opt in options("one_of_each"):
        bits, st = expected("one_of_each", opt)
        assert st[4] == one_of_each_marked(opt[1]) and st[5] == 0 and st[2] == 7 * 3 + 24 * 2, (opt, st)
        assert capi.dedup_host(vectors()["one_of_each"], *opt)[3][:6] == st, opt
    bits, st = expected("clips", (True, 0))
    assert st[2] == 14 and st[3] == 8 and st[4] == 12
    assert capi.dedup_host(vectors()["clips"], True, 0)[3][:6] == st
    dup = capi.dedup_host(vectors()["ties"], True, 0)[0]
    assert bytes(expected("ties", (True, 0))[0]) == dup
    assert sorted({View(r).name for r, b in zip(vectors()["ties"], dup) if not b}) == [b"t_a\0", b"z0\0"]      # the smallest name of each class survives


def test_tool_mode_on_the_device(dd, work):
    """--gpuBAMdedup Device writes the host's file; once more through the emulated compressor; one Log.out line per run"""
    for name in ("one_of_each", "multi", "layout", "empty", "unpaired"):
        bam = write_bam(os.path.join(work, name + ".bam"), vectors()[name])
        for opt in OPTION_SETS[:1] + OPTION_SETS[3:]:
            want = tool_mode(bam, os.path.join(work, "%s_h%d%d_" % (name, opt[0], opt[1])), opt)
            pd = os.path.join(work, "%s_d%d%d_" % (name, opt[0], opt[1]))
            assert isinstance(want, tuple) and tool_mode(bam, pd, opt, device=True, more=["--runThreadN", "3"]) == want, (name, opt)
            st = expected(name, opt)[1]
            line = "--bamRemoveDuplicatesType %s on the Device (--gpuBAMdedup): %d records, %d pairs, %d classes, %d records marked, %d unpaired unique records\n" % (TYPES[opt[0]], st[0], st[2], st[3], st[4], st[5])
            assert open(pd + "Log.out").read().count(line) == 1
    bz = capi.BgzfDevice(lib_path=emul_lib())
    L = capi.host_lib()
    L.sah_set_bgzf_device_fn.restype = None; L.sah_set_bgzf_device_fn.argtypes = [C.c_void_p, C.c_void_p]
    try:
        L.sah_set_bgzf_device_fn(C.cast(bz.L.staramd_bgzf_compress, C.c_void_p), bz.z)
        bam = os.path.join(work, "layout.bam")
        got = tool_mode(bam, os.path.join(work, "layout_dz_"), OPTION_SETS[0], device=True, more=["--gpuBAMcompression", "Device", "--outBAMcompression", "1"])
        assert got == tool_mode(bam, os.path.join(work, "layout_hz_"), OPTION_SETS[0])
    finally:
        L.sah_set_bgzf_device_fn(None, None)
        bz.close()
    assert "no device BGZF compressor is installed" in tool_mode(bam, os.path.join(work, "layout_nz_"), OPTION_SETS[0], device=True, more=["--gpuBAMcompression", "Device"])


def test_fatal_texts_are_the_hosts(dd, work):
    for name, text in (("no_nh", NH_FATAL), ("no_as", AS_FATAL), ("no_both", NH_FATAL)):
        bam = write_bam(os.path.join(work, name + ".bam"), vectors()[name])
        for bits in (None, 0):
            with HashBits(bits):
                assert tool_mode(bam, os.path.join(work, name + "_d_"), OPTION_SETS[0], device=True) == text
        assert tool_mode(bam, os.path.join(work, name + "_h_"), OPTION_SETS[0]) == text
    assert isinstance(tool_mode(write_bam(os.path.join(work, "nm2.bam"), vectors()["no_as_mate2"]), os.path.join(work, "nm2_d_"), OPTION_SETS[0], device=True), tuple)


def test_exports(dd):
    """the C ABI of include/star_amd_dedup.h in the emulated unit and (where it is built) in the shipped engine library; the host library's hooks"""
    def exported(path):
        return {l.split()[-1] for l in subprocess.check_output(["nm", "-D", "--defined-only", path], text=True).splitlines() if l.strip()}
    abi = {"staramd_dedup_host_records", "staramd_dedup_free", "staramd_dedup_constant", "staramd_dedup_last_error"}
    assert abi <= exported(emul_lib())
    if os.path.isfile(capi.ENGINE_PATH):
        assert abi <= exported(capi.ENGINE_PATH)
    assert {"sah_set_dedup_device", "sah_dedup_on_device", "sah_dedup_counts", "sah_dedup_host_records", "sah_dedup_host_free"} <= exported(capi.HOST_PATH)


def test_device_flag_without_functions(dd, work):
    bam = write_bam(os.path.join(work, "clips.bam"), vectors()["clips"])
    capi.DedupDevice.uninstall()
    try:
        assert "--gpuBAMdedup Device, but no device duplicate-marking functions are installed" in tool_mode(bam, os.path.join(work, "clips_none_"), OPTION_SETS[0], device=True)
    finally:
        dd.install()
    with pytest.raises(RuntimeError, match="record 0 lies outside"):
        dd.host_records([vectors()["clips"][0][:-3]])
    with pytest.raises(RuntimeError, match="sah_dedup_host_records failed"):
        capi.dedup_host([vectors()["clips"][0][:-3]])
