// index_routines_cases.h -- TEST INFRASTRUCTURE: the cases of oracle/index_routines_check.cpp and the comparisons of what the index builder
// (star_amd/csrc/index/index_core.h, sjdb_core.h) leaves with INDEPENDENT RESTATEMENTS of the reference's rules, as templates over the backend
// type.  Included by oracle/index_routines_check.cpp (host compiler, LoopBackend of oracle/loop_backend.h) and by tests/index_routines_gpu.hip
// (hipcc, gfx950, HipBackend): both run the same cases; expected values are computed on the host inside the same program.
//
// Restatements (never the code under test):
//   suffix order     std::sort of the 2N text positions, byte by byte: codes compare as numbers; the first offset where both suffixes hold
//                    code 5 ends the comparison and the smaller position comes first; positions past the text end are padding
//                    (funCompareSuffixes, source/Genome_genomeGenerate.cpp:29-89)
//   rounds           0 if the longest common prefix of two suffixes (stopping at padding) is below 23, else the smallest k with 23 * 2^k above it
//                    (round 0 separates what differs in 23 codes, round k what differs in 23 * 2^k: exact, and held exactly)
//   SAindex          the sequential walk of source/genomeSAindex.cpp:117-176 over EVERY suffix (the reference skips suffixes of the class of
//                    the one before, which write nothing new), classes by a literal funCalcSAiFromSA (source/SuffixArrayFuns.cpp:353-395)
//   insertion        point: linear scan over the old suffix array, full comparison from offset 0, spacer tie rule of compareRefEnds;
//                    order: std::stable_sort by funCompareUintAndSuffixes' rule; merge: the two-pointer loop of source/sjdbBuildIndex.cpp:141-207
//                    with packedSet; SAindex: the walk above over the merged array for values and absent flags, the N marks as the reference's
//                    patch of the old table leaves them (saiPatchedRef: :209-284); tests/golden/tiny_index/nprefix is a case where the two differ
//   primitives       loops, std::stable_sort on the masked key
// L = 14 (the product's default) is not visited: its table has 3.6e8 entries and a sequential walk of that size does not belong in a test of
// seconds; bench.py --full remains its cover.  nSA and 2N are even by construction (two strands), so the sizes "63, 65, 255, 257 ..." are met
// from both sides (62/64/66, 254/256/258 ...) by whole builds and exactly by the stages that take a count (buildSAindex, packArray, compactIf).
#pragma once
#include "../star_amd/csrc/index/index_core.h"
#include "../star_amd/csrc/index/sjdb_core.h"
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

namespace idxchk {
using namespace staridx;

// what a backend reports after a case (HipBackend: its first HIP error); specialised by the harness
template <class BE> struct BackendTraits { static const char *error(BE &) { return nullptr; } };

struct Rng {
    u64 s;
    explicit Rng(u64 seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
    u64 next() { u64 z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    u64 below(u64 n) { return next() % n; }
};

static const char *const CLASSES[] = {
    // text and element-wise pieces
    "text: pads and both strands", "prefixKey: no padding in 23 codes", "prefixKey: padding inside the key", "prefixKey: padding inside the skipped codes",
    "bucketOf: second code padding", "saiClass: all ACGT", "saiClass: non-ACGT at offset 0", "saiClass: non-ACGT inside", "saiClass: L 16",
    // suffix order
    "order: nSA 0", "order: one bucket of one element", "order: rounds 0", "order: rounds 1-2", "order: rounds 3-5", "order: rounds 6 and more", "order: U 2 in the last round",
    "order: padding tie inside 23 codes", "order: padding tie beyond 23 codes", "order: padding tie the continuation contradicts", "order: suffix ends at the text end (rankAt q == n2)",
    "order: 2N a multiple of 256", "order: 2N just below a multiple of 256", "order: 2N just above a multiple of 256", "order: dropped tail non-empty", "order: N run of 600",
    // packing
    "pack: entry across a word boundary", "pack: n a multiple of 64", "pack: n one above a multiple of 64", "pack: n one below a multiple of 64", "pack: width above 32", "pack: width 63", "pack: narrow width",
    // SAindex
    "sai: present entry", "sai: absent before the first present", "sai: absent between", "sai: absent after the last", "sai: N mark", "sai: N at every offset 1..L-1",
    "sai: L 1", "sai: L 2", "sai: L 12 almost all absent", "sai: GstrandBit 32", "sai: GstrandBit 33", "sai: GstrandBit 36", "sai: nSA odd (63, 65)", "sai: first suffix bad (-3)",
    // buildAll
    "build: rc 0 bytes equal", "build: nSA a multiple of 64 (bytes behind the last group)", "build: rc -1", "build: rc -2 SA one byte short", "build: rc -2 SAindex one byte short", "build: rc -3", "build: nSA 0",
    // insertion
    "search: tie at the spacer, + strand", "search: tie at the spacer, - strand", "search: below the first old suffix", "search: above the last old suffix", "search: nSAold 1", "search: nSAold 2", "search: between",
    "insert: new entry at output index 0", "insert: new entry at the last index", "insert: run of 3 or more new entries", "insert: new entry at a multiple of 64", "insert: new entry at 63 mod 64",
    "insert: identical junction texts (offset order)", "insert: junction text with N", "insert: old junction moved, + strand", "insert: old junction moved, - strand", "insert: old junctions, identity numbering",
    "insert: old chromosome entry, - strand shifted", "insert: one radix chunk", "insert: two radix chunks", "insert: three radix chunks", "insert: ten radix chunks",
    "insert: GstrandBit 32", "insert: GstrandBit 33", "insert: GstrandBit 36", "insert: nInd 1 or 2", "insert: zero entry and words behind the array", "insert: new genome text", "insert: SAindex of the merged array",
    "insert: N mark kept where the old table had it, not where a walk would put it",
    // backend primitives
    "prim: forEach", "prim: exclusiveSum in place", "prim: inclusiveMax in place", "prim: readOne", "prim: compactIf none", "prim: compactIf all", "prim: compactIf alternating", "prim: compactIf random",
    "prim: sortPairs bits 0-63 (bit 63 is no sort bit)", "prim: sortPairs bits 0-1", "prim: sortPairs bits 0-bitsFor(4n)",
    "prim: n 1", "prim: n 3000001",
};
// the fixtures the reference wrote: declared when their directory is given (the tests always give it)
static const char *const FIXTURE_CLASSES[] = {
    "fixture: order and SAindex walk against the reference's files", "fixture: insertion restated against the reference's files", "fixture: buildAll against the reference's files", "fixture: sjdbInsertHost against the reference's files",
};

struct Report {
    std::vector<std::pair<std::string, u64>> cls;
    long bad = 0; u64 total = 0, done = 0; int shown = 0;
    std::string cur;
    Report() { for (const char *c : CLASSES) cls.push_back({c, 0}); }
    void declare(const char *c) { cls.push_back({c, 0}); }
    void hit(const char *c, u64 n = 1) {
        for (auto &e : cls) if (e.first == c) { e.second += n; return; }
        fprintf(stderr, "undeclared class '%s'\n", c); exit(2);
    }
    void begin(const std::string &name) { total++; cur = name; }
    void end() { done++; }
    void diff(const char *fmt, ...) {
        bad++;
        if (shown++ >= 40) return;
        char buf[512]; va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
        printf("DIFF [%s] %s\n", cur.c_str(), buf);
    }
    template <class T> void same(const char *what, const std::vector<T> &got, const std::vector<T> &exp) {
        if (got.size() != exp.size()) { diff("%s: %zu entries, expected %zu", what, got.size(), exp.size()); return; }
        for (size_t i = 0; i < got.size(); i++) if (got[i] != exp[i]) { diff("%s[%zu] = %llx, expected %llx", what, i, (unsigned long long)got[i], (unsigned long long)exp[i]); return; }
    }
    void eq(const char *what, u64 got, u64 exp) { if (got != exp) diff("%s = %lld, expected %lld", what, (long long)got, (long long)exp); }
    // one line per class, the case count, the verdict; returns the exit status
    int finish(const char *title) {
        long missing = 0;
        for (auto &e : cls) { printf("  %-78s %llu\n", e.first.c_str(), (unsigned long long)e.second); if (!e.second) missing++; }
        printf("compared %llu of %llu cases\n", (unsigned long long)done, (unsigned long long)total);
        if (missing) printf("%ld classes never occurred\n", missing);
        printf("%s: %ld differences\n", title, bad);
        return (bad || missing || done != total || !total) ? 1 : 0;
    }
};

template <class BE> void checkBackend(BE &be, Report &R) {
    if (const char *e = BackendTraits<BE>::error(be)) {         // the first error ends the process; nothing further is started
        printf("backend error in case [%s]: %s\n", R.cur.c_str(), e); fflush(stdout);
        exit(3);
    }
}
template <class BE, class T> T *up(BE &be, const std::vector<T> &h, u64 extra = 0) {
    T *d = be.template alloc<T>(h.size() + extra);
    if (!h.empty()) be.copyToDevice(d, h.data(), h.size());
    return d;
}
template <class BE, class T> std::vector<T> down(BE &be, const T *d, u64 n) {
    std::vector<T> h(n);
    if (n) be.copyToHost(h.data(), d, n);
    return h;
}

// =====================================================================================================================
// restatements

struct Text {                      // the 2N text; positions outside it are padding
    std::vector<u8> t; u64 n2;
    u8 at(u64 p) const { return p < n2 ? t[p] : (u8)5; }
};
static inline Text textOf(const std::vector<u8> &G) {
    Text T; const u64 N = G.size(); T.n2 = 2 * N; T.t.resize(2 * N);
    for (u64 i = 0; i < N; i++) { u8 c = G[i]; T.t[i] = c; T.t[2 * N - 1 - i] = c < 4 ? (u8)(3 - c) : c; }
    return T;
}
static inline bool suffixLess(const Text &T, u64 a, u64 b) {
    for (u64 k = 0;; k++) {
        u8 ca = T.at(a + k), cb = T.at(b + k);
        if (ca != cb) return ca < cb;
        if (ca == 5) return a < b;
    }
}
static inline u64 lcpToPad(const Text &T, u64 a, u64 b, bool *tie = nullptr) {     // codes in common before a difference or padding in both
    for (u64 k = 0;; k++) {
        u8 ca = T.at(a + k), cb = T.at(b + k);
        if (ca != cb) { if (tie) *tie = false; return k; }
        if (ca == 5) { if (tie) *tie = true; return k; }
    }
}
static inline std::vector<u64> bruteOrder(const Text &T) {
    std::vector<u64> o(T.n2); std::iota(o.begin(), o.end(), 0);
    std::sort(o.begin(), o.end(), [&](u64 a, u64 b) { return suffixLess(T, a, b); });
    return o;
}
static inline u64 saValueRef(u64 pos, u64 N, u32 gsb) { return pos < N ? pos : (pos - N) | (1ull << gsb); }

// funCalcSAiFromSA, literally: the suffix-array value, the genome bytes (padding outside), the strand bit
static inline u64 classRef(const std::vector<u8> &G, u32 gsb, u64 v, int L, int &iL4) {
    const i64 N = (i64)G.size();
    // gSeq when the reference builds the table (Genome_genomeGenerate.cpp:181, :357): the genome, its reverse complement right behind it, padding outside
    auto g = [&](i64 i) -> u8 { return i < 0 || i >= 2 * N ? (u8)5 : i < N ? G[i] : G[2 * N - 1 - i] < 4 ? (u8)(3 - G[2 * N - 1 - i]) : G[2 * N - 1 - i]; };
    const bool dirG = (v >> gsb) == 0; const i64 s = (i64)(v & ~(1ull << gsb));
    iL4 = -1; u64 saind = 0;
    for (int ii = 0; ii < L; ii++) {
        u8 g2 = dirG ? g(s + ii) : g(N - 1 - s - ii);
        if (g2 > 3) { iL4 = ii; saind <<= 2 * (L - ii); return saind; }
        saind = (saind << 2) + (dirG ? g2 : 3 - g2);
    }
    return saind;
}

struct SaiWalk {
    std::vector<u64> e; int bad = 0; u64 start[17];
    u64 present = 0, absBefore = 0, absBetween = 0, absAfter = 0, nMark = 0; u32 offsetsSeen = 0;
};
// genomeSAindexChunk over every suffix; sa = suffix-array values of genome G
static inline SaiWalk saiWalkRef(const std::vector<u8> &G, u32 gsb, const std::vector<u64> &sa, u32 L) {
    SaiWalk W; const u64 nSA = sa.size();
    W.start[0] = 0; for (u32 i = 1; i <= L; i++) W.start[i] = W.start[i - 1] + (1ull << (2 * i));
    for (u32 i = L + 1; i < 17; i++) W.start[i] = 0;
    const u64 absent = 1ull << (gsb + 2), nmask = 1ull << (gsb + 1);
    W.e.assign(W.start[L], 0);
    std::vector<u64> ind0(L, ~0ull);
    for (u64 isa = 0; isa < nSA; isa++) {
        int iL4; const u64 indFull = classRef(G, gsb, sa[isa], (int)L, iL4);
        if (isa == 0 && iL4 >= 0) { W.bad = 1; return W; }           // the reference marks entry start[iL1] - 1 here and never records a prefix again
        if (iL4 > 0) W.offsetsSeen |= 1u << iL4;
        for (u32 iL = 0; iL < L; iL++) {
            const u64 indPref = indFull >> (2 * (L - 1 - iL));
            if ((int)iL == iL4) { for (u32 iL1 = iL; iL1 < L; iL1++) W.e[W.start[iL1] + ind0[iL1]] |= nmask; break; }
            if (indPref > ind0[iL] || isa == 0) {
                W.e[W.start[iL] + indPref] = isa;
                for (u64 ii = ind0[iL] + 1; ii < indPref; ii++) W.e[W.start[iL] + ii] = isa | absent;
                ind0[iL] = indPref;
            }
        }
    }
    for (u32 iL = 0; iL < L; iL++) for (u64 ii = W.start[iL] + ind0[iL] + 1; ii < W.start[iL + 1]; ii++) W.e[ii] = nSA | absent;
    for (u32 iL = 0; iL < L; iL++) {
        bool seen = false;
        for (u64 ii = W.start[iL]; ii < W.start[iL + 1]; ii++) {
            const u64 v = W.e[ii];
            if (v & nmask) W.nMark++;
            if (!(v & absent)) { W.present++; seen = true; }
            else if ((v & (nmask - 1)) == nSA) W.absAfter++;
            else if (!seen) W.absBefore++; else W.absBetween++;
        }
    }
    return W;
}
// The table after a junction insertion.  The reference patches the old table (sjdbBuildIndex.cpp:209-284): values and absent flags as the walk over the
// merged array gives them, but the N marks are (a) those of the old table's present entries, kept (:251), and (b) one per new suffix with a non-ACGT
// code at offset iL inside the prefix, on the previous entry that is not absent, from prefix + "333..." downwards, for every length from iL on (:262-284).
// newPos: text positions (2N text of Gnew) of the new suffixes.  Anchored to the reference's files by the fixtures.
static inline std::vector<u64> saiPatchedRef(const SaiWalk &Wnew, const std::vector<u64> &oldEntries, const Text &Tnew, const std::vector<u64> &newPos, u32 L, u32 gsb, u64 *moved = nullptr) {
    const u64 absent = 1ull << (gsb + 2), nmask = 1ull << (gsb + 1);
    std::vector<u64> e = Wnew.e;
    for (auto &v : e) v &= ~nmask;
    for (u64 i = 0; i < e.size(); i++) if ((oldEntries[i] & nmask) && !(oldEntries[i] & absent)) e[i] |= nmask;
    for (u64 p : newPos) {
        i64 ind1 = 0;
        for (u32 iL = 0; iL < L; iL++) {
            const u8 g = Tnew.at(p + iL);
            ind1 <<= 2;
            if (g > 3) {
                for (u32 iL1 = iL; iL1 < L; iL1++) {
                    ind1 += 3;
                    i64 ind2 = (i64)Wnew.start[iL1] + ind1;
                    for (; ind2 >= 0; ind2--) if ((e[ind2] & absent) == 0) break;
                    if (ind2 >= 0) e[ind2] |= nmask;
                    ind1 <<= 2;
                }
                break;
            } else ind1 += g;
        }
    }
    if (moved) for (u64 i = 0; i < e.size(); i++) if ((e[i] ^ Wnew.e[i]) & nmask) (*moved)++;
    return e;
}
static inline std::vector<u64> packRef(const std::vector<u64> &v, u32 bits, u64 nWords) {
    std::vector<u64> w(nWords, 0);
    for (u64 i = 0; i < v.size(); i++) packedSet(w.data(), i, bits, v[i]);
    return w;
}

// =====================================================================================================================
// genomes

static inline std::vector<u8> rndBases(Rng &r, u64 n) { std::vector<u8> g(n); for (auto &c : g) c = (u8)r.below(4); return g; }
static inline void padTo(std::vector<u8> &g, u64 m) { while (g.size() % m) g.push_back(5); }
static inline void append(std::vector<u8> &g, const std::vector<u8> &x) { g.insert(g.end(), x.begin(), x.end()); }

// =====================================================================================================================
// 1. text, element-wise pieces, suffix order, SAindex and the whole build on one genome

struct GenomeOpts {
    std::vector<u32> Ls;            // SAindex prefix lengths to visit
    std::vector<u32> gsbs;          // GstrandBit values to visit
    bool nRun600 = false;
    u64 truncSA = 0;                // additionally: buildSAindex over the first truncSA suffixes (odd counts)
};

template <class BE> void caseGenome(BE &be, Report &R, const std::string &name, const std::vector<u8> &G, const GenomeOpts &O) {
    R.begin(name);
    const u64 N = G.size(), n2 = 2 * N;
    const Text T = textOf(G);
    // ---- buildText
    u8 *dG = up(be, G);
    u8 *dTraw = be.template alloc<u8>(n2 + 2 * TPAD);
    u8 *dT = buildText(be, dG, N, dTraw);
    {
        std::vector<u8> raw = down(be, dTraw, n2 + 2 * TPAD), exp(n2 + 2 * TPAD, 5);
        std::copy(T.t.begin(), T.t.end(), exp.begin() + TPAD);
        R.same("text", raw, exp);
        R.hit("text: pads and both strands");
    }
    // ---- prefixKey, bucketOf, saiClassFast at every position
    {
        u64 *k0 = be.template alloc<u64>(n2), *k2 = be.template alloc<u64>(n2); u32 *bk = be.template alloc<u32>(n2);
        const u8 *TT = dT;
        be.forEach(n2, [=] IDX_L (u64 p) { k0[p] = prefixKey(TT, p, 0); k2[p] = prefixKey(TT, p, BUCKET_CODES); bk[p] = bucketOf(TT, p); });
        std::vector<u64> g0 = down(be, k0, n2), g2 = down(be, k2, n2); std::vector<u32> gb = down(be, bk, n2);
        for (u64 p = 0; p < n2; p++) {
            u64 f = 0; while (T.at(p + f) != 5) f++;                      // offset of the first padding byte
            for (u32 skip = 0; skip <= 2; skip += 2) {
                u64 key = 0;
                for (u64 k = skip; k < skip + 21; k++) key = key * 8 + (k <= f ? T.at(p + k) : 0);
                if (f < skip + 21) key |= 1ull << 63;
                const u64 got = skip ? g2[p] : g0[p];
                if (got != key) R.diff("prefixKey(%llu, skip %u) = %llx, expected %llx", (unsigned long long)p, skip, (unsigned long long)got, (unsigned long long)key);
            }
            R.hit(f >= 23 ? "prefixKey: no padding in 23 codes" : f < 2 ? "prefixKey: padding inside the skipped codes" : "prefixKey: padding inside the key");
            const u32 b = T.at(p) == 5 ? 30u : (u32)T.at(p) * 6u + T.at(p + 1);
            if (gb[p] != b) R.diff("bucketOf(%llu) = %u, expected %u", (unsigned long long)p, gb[p], b);
            if (T.at(p) != 5 && T.at(p + 1) == 5) R.hit("bucketOf: second code padding");
        }
        be.free(k0); be.free(k2); be.free(bk);
        u32 *cl = be.template alloc<u32>(n2); int *c4 = be.template alloc<int>(n2);
        for (u32 L : {1u, 2u, 7u, 12u, 16u}) {
            be.forEach(n2, [=] IDX_L (u64 p) { int l4; cl[p] = saiClassFast(TT, p, L, l4); c4[p] = l4; });
            std::vector<u32> gc = down(be, cl, n2); std::vector<int> g4 = down(be, c4, n2);
            for (u64 p = 0; p < n2; p++) {
                int e4; const u64 ec = classRef(G, 40, saValueRef(p, N, 40), (int)L, e4);
                if (gc[p] != (u32)ec || g4[p] != e4) R.diff("saiClassFast(%llu, L %u) = %x/%d, expected %llx/%d", (unsigned long long)p, L, gc[p], g4[p], (unsigned long long)ec, e4);
                R.hit(e4 < 0 ? "saiClass: all ACGT" : e4 == 0 ? "saiClass: non-ACGT at offset 0" : "saiClass: non-ACGT inside");
            }
            if (L == 16) R.hit("saiClass: L 16");
        }
        be.free(cl); be.free(c4);
    }
    // ---- suffix order
    const std::vector<u64> ord = bruteOrder(T);
    u64 nSAexp = 0; for (u64 p = 0; p < n2; p++) if (T.t[p] < 4) nSAexp++;
    {
        u64 *dSA = be.template alloc<u64>(n2), *dISA = be.template alloc<u64>(n2);
        u64 rounds = ~0ull;
        const u64 nSA = suffixSort(be, dT, N, dSA, dISA, &rounds);
        std::vector<u64> sa = down(be, dSA, n2), isa = down(be, dISA, n2);
        be.free(dSA); be.free(dISA);
        R.eq("nSA", nSA, nSAexp);
        for (u64 i = 0; i < nSAexp && i < n2; i++) if (sa[i] != ord[i]) { R.diff("SA[%llu] = %llu, expected %llu", (unsigned long long)i, (unsigned long long)sa[i], (unsigned long long)ord[i]); break; }
        {   // the dropped tail: a permutation of exactly the positions that start with N or padding; ISA the inverse everywhere
            std::vector<u8> seen(n2, 0);
            for (u64 i = nSAexp; i < n2; i++) { const u64 p = sa[i]; if (p >= n2 || T.t[p] < 4 || seen[p]) { R.diff("dropped tail: SA[%llu] = %llu", (unsigned long long)i, (unsigned long long)p); break; } seen[p] = 1; }
            for (u64 i = 0; i < n2; i++) if (sa[i] >= n2 || isa[sa[i]] != i) { R.diff("ISA[SA[%llu]] is not %llu", (unsigned long long)i, (unsigned long long)i); break; }
            if (nSAexp < n2) R.hit("order: dropped tail non-empty");
        }
        // rounds from the longest common prefix over adjacent suffixes; padding ties; suffixes that end at the text end
        u64 maxLcp = 0; std::vector<u64> nb(n2, 0);                       // nb[p] = longest common prefix of p with a neighbour in the order
        u64 tieIn = 0, tieOut = 0, tieContra = 0;
        for (u64 i = 0; i + 1 < n2; i++) {
            bool tie; const u64 a = ord[i], b = ord[i + 1], l = lcpToPad(T, a, b, &tie);
            maxLcp = std::max(maxLcp, l); nb[a] = std::max(nb[a], l); nb[b] = std::max(nb[b], l);
            if (tie && l > 0 && T.at(a) < 4) {
                (l < 23 ? tieIn : tieOut)++;
                // what an order that reads on behind the padding (padding as one symbol) would say
                u64 k = l; while (a + k < n2 + 64 && b + k < n2 + 64 && T.at(a + k) == T.at(b + k)) k++;
                if (T.at(a + k) > T.at(b + k)) tieContra++;
            }
        }
        u64 expRounds = 0; while (maxLcp >= 23ull << expRounds) expRounds++;
        R.eq("rounds", rounds, expRounds);
        R.hit(expRounds == 0 ? "order: rounds 0" : expRounds <= 2 ? "order: rounds 1-2" : expRounds <= 5 ? "order: rounds 3-5" : "order: rounds 6 and more");
        if (expRounds) {   // how many positions are still tied when the last round starts
            const u64 h = 23ull << (expRounds - 1); u64 U = 0;
            for (u64 p = 0; p < n2; p++) if (nb[p] >= h) U++;
            if (U == 2) R.hit("order: U 2 in the last round");
        }
        for (u32 k = 0; (23ull << k) <= n2; k++) { const u64 h = 23ull << k, p = n2 - h; if (nb[p] >= h) R.hit("order: suffix ends at the text end (rankAt q == n2)"); }
        if (tieIn) R.hit("order: padding tie inside 23 codes", tieIn);
        if (tieOut) R.hit("order: padding tie beyond 23 codes", tieOut);
        if (tieContra) R.hit("order: padding tie the continuation contradicts", tieContra);
        if (nSAexp == 0) R.hit("order: nSA 0");
        {   u64 cnt[36] = {0}; for (u64 p = 0; p < n2; p++) cnt[T.at(p) == 5 ? 30 : T.at(p) * 6 + T.at(p + 1)]++;
            for (u64 c : cnt) if (c == 1) { R.hit("order: one bucket of one element"); break; } }
        if (n2 % 256 == 0) R.hit("order: 2N a multiple of 256"); else if (n2 % 256 >= 254) R.hit("order: 2N just below a multiple of 256"); else if (n2 % 256 <= 2) R.hit("order: 2N just above a multiple of 256");
        if (O.nRun600) R.hit("order: N run of 600");
    }
    checkBackend(be, R);
    // ---- SAindex over the brute-force order, then the whole build
    std::vector<u64> pos(ord.begin(), ord.begin() + nSAexp);
    for (u32 gsb : O.gsbs) for (u32 L : O.Ls) {
        std::vector<u64> saVal(nSAexp); for (u64 i = 0; i < nSAexp; i++) saVal[i] = saValueRef(pos[i], N, gsb);
        const SaiWalk W = saiWalkRef(G, gsb, saVal, L);
        if (nSAexp) {
            u64 *dPos = up(be, pos); u64 *dU = be.template alloc<u64>(W.start[L]);
            const int bad = buildSAindex(be, dT, dPos, nSAexp, L, gsb, W.start, dU);
            R.eq("buildSAindex return", (u64)bad, (u64)W.bad);
            if (!W.bad) {
                std::vector<u64> got = down(be, dU, W.start[L]);
                for (u32 iL = 0; iL < L; iL++) for (u64 e = W.start[iL]; e < W.start[iL + 1]; e++) if (got[e] != W.e[e]) {
                    R.diff("SAindex gsb %u L %u level %u entry %llu = %llx, expected %llx", gsb, L, iL + 1, (unsigned long long)(e - W.start[iL]), (unsigned long long)got[e], (unsigned long long)W.e[e]); break; }
                if (W.present) R.hit("sai: present entry", W.present);
                if (W.absBefore) R.hit("sai: absent before the first present", W.absBefore);
                if (W.absBetween) R.hit("sai: absent between", W.absBetween);
                if (W.absAfter) R.hit("sai: absent after the last", W.absAfter);
                if (W.nMark) R.hit("sai: N mark", W.nMark);
                if (L >= 3 && W.offsetsSeen == ((1u << L) - 2)) R.hit("sai: N at every offset 1..L-1");
                if (L == 1) R.hit("sai: L 1");
                if (L == 2) R.hit("sai: L 2");
                if (L == 12 && W.present * 100 < W.e.size()) R.hit("sai: L 12 almost all absent");
                R.hit(gsb == 32 ? "sai: GstrandBit 32" : gsb == 33 ? "sai: GstrandBit 33" : "sai: GstrandBit 36");
            } else R.hit("sai: first suffix bad (-3)");
            be.free(dPos); be.free(dU);
            if (O.truncSA && O.truncSA < nSAexp && !W.bad) {           // an odd number of suffixes: the first truncSA of the order
                std::vector<u64> sv(saVal.begin(), saVal.begin() + O.truncSA), pv(pos.begin(), pos.begin() + O.truncSA);
                const SaiWalk W2 = saiWalkRef(G, gsb, sv, L);
                u64 *dP2 = up(be, pv); u64 *dU2 = be.template alloc<u64>(W2.start[L]);
                R.eq("buildSAindex return (truncated)", (u64)buildSAindex(be, dT, dP2, O.truncSA, L, gsb, W2.start, dU2), 0);
                R.same("SAindex over a truncated array", down(be, dU2, W2.start[L]), W2.e);
                R.hit("sai: nSA odd (63, 65)");
                be.free(dP2); be.free(dU2);
            }
        }
        checkBackend(be, R);
        // buildAll: host buffers between guard bytes, exactly as large as needed
        const u32 saBits = gsb + 1, saiBits = gsb + 3;
        const u64 saBytes = packedBytes(nSAexp, saBits), saiBytes = packedBytes(W.start[L], saiBits);
        const u64 GUARD = 64;
        std::vector<u8> hSA(saBytes + 2 * GUARD, 0xC3), hSAi(saiBytes + 2 * GUARD, 0xC3);
        BuildParams P; P.nGenome = N; P.GstrandBit = gsb; P.saIndexNbases = L;
        BuildResult B; memset(&B, 0, sizeof B);
        const int rc = buildAll(be, G.data(), P, hSA.data() + GUARD, saBytes, hSAi.data() + GUARD, saiBytes, B);
        const int rcExp = (nSAexp && W.bad) ? -3 : 0;
        R.eq("buildAll return", (u64)(i64)rc, (u64)(i64)rcExp);
        R.eq("buildAll nSA", B.nSA, nSAexp); R.eq("buildAll nSAbyte", B.nSAbyte, saBytes); R.eq("buildAll nSAi", B.nSAi, W.start[L]); R.eq("buildAll nSAibyte", B.nSAibyte, saiBytes);
        for (u32 i = 0; i < 17; i++) R.eq("buildAll saiStart", B.saiStart[i], W.start[i]);
        auto guardsOk = [&](const std::vector<u8> &b, const char *what) {
            for (u64 i = 0; i < GUARD; i++) if (b[i] != 0xC3 || b[b.size() - 1 - i] != 0xC3) { R.diff("%s: guard bytes overwritten", what); return; } };
        guardsOk(hSA, "SA"); guardsOk(hSAi, "SAindex");
        if (nSAexp) {
            std::vector<u64> w = packRef(saVal, saBits, packedWords(nSAexp, saBits));
            if (memcmp(hSA.data() + GUARD, w.data(), saBytes)) R.diff("buildAll gsb %u L %u: SA bytes differ", gsb, L);
            if (nSAexp % 64 == 0) R.hit("build: nSA a multiple of 64 (bytes behind the last group)");
            if (!W.bad) {
                std::vector<u64> wi = packRef(W.e, saiBits, packedWords(W.start[L], saiBits));
                if (memcmp(hSAi.data() + GUARD, wi.data(), saiBytes)) R.diff("buildAll gsb %u L %u: SAindex bytes differ", gsb, L);
                R.hit("build: rc 0 bytes equal");
            } else R.hit("build: rc -3");
        } else {
            for (u64 i = 0; i < saBytes; i++) if (hSA[GUARD + i] != 0xC3) { R.diff("nSA 0: SA buffer written"); break; }
            R.hit("build: nSA 0");
        }
        checkBackend(be, R);
    }
    be.free(dG); be.free(dTraw);
    checkBackend(be, R);
    R.end();
}

// capacities one byte short, bad arguments
template <class BE> void caseBuildErrors(BE &be, Report &R, const std::vector<u8> &G) {
    R.begin("buildAll: capacities and arguments");
    const u64 N = G.size(), GUARD = 64; const u32 gsb = 32, L = 4;
    BuildParams P; P.nGenome = N; P.GstrandBit = gsb; P.saIndexNbases = L;
    BuildResult B0; memset(&B0, 0, sizeof B0);
    R.eq("sizes only", (u64)(i64)buildAll(be, G.data(), P, (u8 *)nullptr, 0, (u8 *)nullptr, 0, B0), 0);
    u64 nSAexp = 0; for (u8 c : G) if (c < 4) nSAexp += 2;
    R.eq("sizes only: nSAbyte", B0.nSAbyte, packedBytes(nSAexp, gsb + 1)); R.eq("sizes only: nSAibyte", B0.nSAibyte, packedBytes(340, gsb + 3));
    for (int which = 0; which < 2; which++) {
        const u64 capSA = B0.nSAbyte - (which == 0), capSAi = B0.nSAibyte - (which == 1);
        std::vector<u8> hSA(capSA + 2 * GUARD, 0xC3), hSAi(capSAi + 2 * GUARD, 0xC3);
        BuildResult B; memset(&B, 0, sizeof B);
        R.eq("one byte short", (u64)(i64)buildAll(be, G.data(), P, hSA.data() + GUARD, capSA, hSAi.data() + GUARD, capSAi, B), (u64)(i64)-2);
        R.eq("one byte short: nSAbyte", B.nSAbyte, B0.nSAbyte); R.eq("one byte short: nSAibyte", B.nSAibyte, B0.nSAibyte); R.eq("one byte short: nSA", B.nSA, nSAexp);
        for (u8 c : hSA) if (c != 0xC3) { R.diff("one byte short: SA buffer or its guards written"); break; }
        for (u8 c : hSAi) if (c != 0xC3) { R.diff("one byte short: SAindex buffer or its guards written"); break; }
        R.hit(which == 0 ? "build: rc -2 SA one byte short" : "build: rc -2 SAindex one byte short");
    }
    const u32 badArg[3][2] = {{0, 32}, {17, 32}, {4, 61}};
    for (auto &a : badArg) {
        BuildParams Q; Q.nGenome = N; Q.saIndexNbases = a[0]; Q.GstrandBit = a[1];
        BuildResult B; memset(&B, 0, sizeof B);
        R.eq("bad arguments", (u64)(i64)buildAll(be, G.data(), Q, (u8 *)nullptr, 0, (u8 *)nullptr, 0, B), (u64)(i64)-1);
        R.hit("build: rc -1");
    }
    checkBackend(be, R);
    R.end();
}

// =====================================================================================================================
// 2. packArray / packedGetW

template <class BE> void casePack(BE &be, Report &R, u32 bits, u64 n, Rng &rng) {
    R.begin("pack bits " + std::to_string(bits) + " n " + std::to_string(n));
    std::vector<u64> v(n); const u64 mask = (1ull << bits) - 1;
    for (u64 i = 0; i < n; i++) v[i] = i % 5 == 0 ? mask : i % 7 == 0 ? 0 : rng.next() & mask;
    const u64 nW = packedWords(n, bits);
    std::vector<u64> fill(nW, 0x5A5A5A5A5A5A5A5Aull);
    u64 *dV = up(be, v), *dOut = up(be, fill), *dBack = be.template alloc<u64>(n);
    const u64 *vv = dV;
    packArray(be, n, bits, dOut, [=] IDX_L (u64 i) { return vv[i]; });
    const u64 *oo = dOut;
    be.forEach(n, [=] IDX_L (u64 i) { dBack[i] = packedGetW(oo, i, bits); });
    std::vector<u64> got = down(be, dOut, nW), exp = packRef(v, bits, nW);     // the two words behind the groups: zero, as the last 8 bytes of the reference's array
    R.same("packed words", got, exp);
    R.same("packedGetW", down(be, dBack, n), v);
    be.free(dV); be.free(dOut); be.free(dBack);
    if (64 % bits) R.hit("pack: entry across a word boundary");
    R.hit(n % 64 == 0 ? "pack: n a multiple of 64" : n % 64 == 1 ? "pack: n one above a multiple of 64" : "pack: n one below a multiple of 64");
    R.hit(bits == 63 ? "pack: width 63" : bits > 32 ? "pack: width above 32" : "pack: narrow width");
    checkBackend(be, R);
    R.end();
}

// =====================================================================================================================
// 3. junction insertion

struct InsCase {
    std::string name;
    std::vector<u8> Gchr;                 // chromosomes (nGenomeReal bytes)
    u32 Lsj = 0;
    std::vector<std::vector<u8>> oldJ;    // old junction texts, Lsj - 1 codes each
    std::vector<std::vector<u8>> newJ;    // the new table, in its order, Lsj - 1 codes each
    std::vector<int> newIsOld;            // per new-table entry: index into oldJ, or -1
    u32 gsb = 32, L = 4;
    u64 nSAoldUse = 0;                    // search stage only: additionally with the first nSAoldUse old suffixes
};

static inline u8 oldCharRef(const std::vector<u8> &G, u32 gsb, u64 v, u64 k) {      // k-th code of the old suffix with value v (padding outside the genome)
    const i64 N = (i64)G.size(); const i64 s = (i64)(v & ~(1ull << gsb));
    if ((v >> gsb) == 0) { const i64 i = s + (i64)k; return i < N ? G[i] : (u8)5; }
    const i64 i = N - 1 - s - (i64)k; if (i < 0) return 5;
    return G[i] < 4 ? (u8)(3 - G[i]) : G[i];
}
// first old index whose suffix is greater than the query: linear scan, full comparison; a tie at the spacer puts the query behind a + strand
// suffix and in front of a - strand one
static inline u64 searchRef(const std::vector<u8> &G, u32 gsb, const std::vector<u64> &sa, u64 nUse, const u8 *q, int *tie) {
    for (u64 i = 0; i < nUse; i++) {
        for (u64 k = 0;; k++) {
            const u8 a = q[k], b = oldCharRef(G, gsb, sa[i], k);
            if (a < b) return i;
            if (a > b) break;
            if (a == 5) { const bool fwd = (sa[i] >> gsb) == 0; if (tie) *tie |= fwd ? 1 : 2; if (!fwd) return i; break; }
        }
    }
    return nUse;
}

template <class BE> void caseInsert(BE &be, Report &R, const InsCase &C) {
    R.begin(C.name);
    const u32 Lsj = C.Lsj, gsb = C.gsb, saBits = gsb + 1, oldSjdbN = (u32)C.oldJ.size(), sjdbN = (u32)C.newJ.size();
    const u64 nGenomeReal = C.Gchr.size(), nGenomeOld = nGenomeReal + (u64)oldSjdbN * Lsj, nGsj = (u64)sjdbN * Lsj;
    // ---- the old index: chromosomes + old junction block, suffix array by the brute-force order
    std::vector<u8> Gold = C.Gchr;
    for (auto &j : C.oldJ) { append(Gold, j); Gold.push_back(5); }
    const Text Told = textOf(Gold);
    std::vector<u64> ordOld = bruteOrder(Told);
    u64 nSAold = 0; for (u8 c : Told.t) if (c < 4) nSAold++;
    std::vector<u64> saOld(nSAold); for (u64 i = 0; i < nSAold; i++) saOld[i] = saValueRef(ordOld[i], nGenomeOld, gsb);
    const SaiWalk Wold = saiWalkRef(Gold, gsb, saOld, C.L);            // the old table: as generation leaves it
    if (Wold.bad) R.diff("case construction: the old index has a bad first suffix");
    // ---- the new table
    std::vector<u8> Gsj, isOld(sjdbN, 0); std::vector<u32> oldSJind(oldSjdbN, 0); u64 sjNew = 0; bool moved = false, hasN = false;
    for (u32 j = 0; j < sjdbN; j++) {
        append(Gsj, C.newJ[j]); Gsj.push_back(5);
        if (C.newIsOld[j] >= 0) { isOld[j] = 1; oldSJind[C.newIsOld[j]] = j; if ((u32)C.newIsOld[j] != j) moved = true; } else { sjNew++; for (u8 c : C.newJ[j]) if (c == 4) hasN = true; }
    }
    std::vector<u8> Q(2 * nGsj + 1 + 64, 5);                                       // sjdbBuildIndex.cpp:30-39
    for (u64 i = 0; i < nGsj; i++) { Q[i] = Gsj[i]; Q[2 * nGsj - 1 - i] = Gsj[i] < 4 ? (u8)(3 - Gsj[i]) : Gsj[i]; }
    // ---- candidates (:53-99), insertion points, order (funCompareUintAndSuffixes)
    std::vector<u64> off;
    for (u64 isj = 0; isj < 2ull * sjdbN; isj++) {
        const u64 isj1 = isj < sjdbN ? isj : 2ull * sjdbN - 1 - isj;
        for (u32 s = 0; s < Lsj; s++) if (!isOld[isj1] && Q[isj * Lsj + s] <= 3) off.push_back(isj * Lsj + s);
    }
    const u64 nInd = off.size();
    std::vector<u64> ipos(nInd); int ties = 0; u64 below = 0, above = 0, between = 0;
    for (u64 j = 0; j < nInd; j++) { ipos[j] = searchRef(Gold, gsb, saOld, nSAold, &Q[off[j]], &ties); if (ipos[j] == 0) below++; else if (ipos[j] == nSAold) above++; else between++; }
    // ---- device inputs
    std::vector<u8> Graw(nGenomeOld + 2 * SJ_GPAD, 5); std::copy(Gold.begin(), Gold.end(), Graw.begin() + SJ_GPAD);
    u8 *dGraw = up(be, Graw);
    std::vector<u64> saOldW = packRef(saOld, saBits, packedWords(nSAold, saBits));
    u64 *dSAold = up(be, saOldW);
    u64 *dSAiOld = up(be, packRef(Wold.e, gsb + 3, packedWords(Wold.start[C.L], gsb + 3)));
    // ---- the search on its own: sjdbSearchOne per candidate, over the whole old array and over its first nSAoldUse entries
    for (int part = 0; part < 2; part++) {
        const u64 nUse = part ? C.nSAoldUse : nSAold;
        if (!nUse || !nInd) continue;
        u8 *dQ = up(be, Q); u64 *dOff = up(be, off); u64 *dPos = be.template alloc<u64>(nInd);
        const u8 *g = dGraw + SJ_GPAD; const u64 *sw = dSAold; const u8 *qq = dQ; const u64 *oo = dOff;
        be.forEach(nInd, [=] IDX_L (u64 j) {
            auto sa = [=](u64 i) { return packedGetW(sw, i, saBits); };
            dPos[j] = sjdbSearchOne(g, nGenomeOld, gsb, nUse, sa, qq + oo[j]);
        });
        std::vector<u64> got = down(be, dPos, nInd), exp(nInd);
        if (part) for (u64 j = 0; j < nInd; j++) exp[j] = searchRef(Gold, gsb, saOld, nUse, &Q[off[j]], nullptr); else exp = ipos;
        R.same(part ? "insertion point (truncated old array)" : "insertion point", got, exp);
        if (part) R.hit(nUse == 1 ? "search: nSAold 1" : nUse == 2 ? "search: nSAold 2" : "search: between");
        be.free(dQ); be.free(dOff); be.free(dPos);
    }
    if (nSAold == 2) R.hit("search: nSAold 2");
    if (ties & 1) R.hit("search: tie at the spacer, + strand");
    if (ties & 2) R.hit("search: tie at the spacer, - strand");
    if (below) R.hit("search: below the first old suffix", below);
    if (above) R.hit("search: above the last old suffix", above);
    if (between) R.hit("search: between", between);
    checkBackend(be, R);
    // ---- expected order and merge
    std::vector<u64> perm(nInd); std::iota(perm.begin(), perm.end(), 0);
    u64 identical = 0;
    std::stable_sort(perm.begin(), perm.end(), [&](u64 a, u64 b) {
        if (ipos[a] != ipos[b]) return ipos[a] < ipos[b];
        for (u64 k = 0;; k++) {
            const u8 ca = Q[off[a] + k], cb = Q[off[b] + k];
            if (ca != cb) return ca < cb;
            if (ca == 5) { identical++; return off[a] < off[b]; }
        }
    });
    const u64 nSAnew = nSAold + nInd, nGenomeNew = nGenomeReal + nGsj, N2bit = 1ull << gsb, nGsjNew = sjNew * Lsj;
    std::vector<u64> wNew(packedWords(nSAnew + 1, saBits), 0), saNew(nSAnew), newPos;
    u64 at0 = 0, atLast = 0, runs = 0, at64 = 0, at63 = 0, movedPlus = 0, movedMinus = 0, shiftedMinus = 0;
    {
        u64 isj = 0, isa2 = 0, run = 0;
        auto putNew = [&]() {
            u64 ind1 = off[perm[isj]];
            if (ind1 < nGsj) ind1 += nGenomeReal; else ind1 = (ind1 - nGsj) | N2bit;
            if (isa2 == 0) at0++; if (isa2 == nSAnew - 1) atLast++; if (isa2 % 64 == 0) at64++; if (isa2 % 64 == 63) at63++;
            if (++run == 3) runs++;
            newPos.push_back(off[perm[isj]] < nGsj ? off[perm[isj]] + nGenomeReal : nGenomeNew + (off[perm[isj]] - nGsj));
            saNew[isa2] = ind1; packedSet(wNew.data(), isa2, saBits, ind1); ++isa2; ++isj;
        };
        for (u64 isa = 0; isa < nSAold; isa++) {
            while (isj < nInd && isa == ipos[perm[isj]]) putNew();
            run = 0;
            u64 ind1 = saOld[isa];
            if (ind1 & N2bit) {
                u64 ind1s = nGenomeOld - (ind1 & ~N2bit);
                if (ind1s >= nGenomeReal) { const u64 sj1 = (ind1s - nGenomeReal) / Lsj; ind1s += ((u64)oldSJind[sj1] - sj1) * Lsj; ind1 = (nGenomeNew - ind1s) | N2bit; if (oldSJind[sj1] != sj1) movedMinus++; }
                else { ind1 += nGsjNew; if (nGsjNew) shiftedMinus++; }
            } else if (ind1 >= nGenomeReal) { const u64 sj1 = (ind1 - nGenomeReal) / Lsj; ind1 += ((u64)oldSJind[sj1] - sj1) * Lsj; if (oldSJind[sj1] != sj1) movedPlus++; }
            saNew[isa2] = ind1; packedSet(wNew.data(), isa2, saBits, ind1); ++isa2;
        }
        while (isj < nInd) putNew();
        if (isa2 != nSAnew) R.diff("restated merge wrote %llu of %llu entries", (unsigned long long)isa2, (unsigned long long)nSAnew);
    }
    std::vector<u8> Gnew = C.Gchr; append(Gnew, Gsj);
    u64 saiStart[17]; saiStart[0] = 0; for (u32 i = 1; i < 17; i++) saiStart[i] = i <= C.L ? saiStart[i - 1] + (1ull << (2 * i)) : 0;
    // ---- the product
    SjdbParams P; P.nGenomeOld = nGenomeOld; P.nGenomeReal = nGenomeReal; P.nSAold = nSAold; P.GstrandBit = gsb; P.sjdbN = sjdbN; P.sjdbLength = Lsj;
    P.oldSjdbN = oldSjdbN; P.sjNew = sjNew; P.saIndexNbases = C.L;
    SjdbDeviceResult D; memset(&D, 0, sizeof D);
    const u64 padOut = 128;
    R.eq("sjdbInsertDevice return", (u64)(i64)sjdbInsertDevice(be, P, dGraw + SJ_GPAD, dSAold, dSAiOld, Gsj.data(), isOld.data(), oldSJind.data(), saiStart, D, padOut), 0);
    R.eq("nInd", D.nInd, nInd); R.eq("nSAnew", D.nSAnew, nSAnew); R.eq("nGenomeNew", D.nGenomeNew, nGenomeNew); R.eq("saWords", D.saWords, wNew.size());
    R.same("merged suffix array (words, the zero entry and the words behind it)", down(be, D.dSApacked, D.saWords), wNew);
    R.hit("insert: zero entry and words behind the array");
    {
        std::vector<u8> exp(nGenomeNew + 2 * padOut, 5); std::copy(Gnew.begin(), Gnew.end(), exp.begin() + padOut);
        R.same("new genome text", down(be, D.dGnew, nGenomeNew + 2 * padOut), exp);
        R.hit("insert: new genome text");
    }
    {
        const SaiWalk W = saiWalkRef(Gnew, gsb, saNew, C.L);
        R.eq("badFirstSuffix", (u64)D.badFirstSuffix, (u64)W.bad);
        if (!W.bad) {
            const u64 nGW = ((W.start[C.L] + 63) / 64) * (gsb + 3);
            R.eq("saiWords", D.saiWords, packedWords(W.start[C.L], gsb + 3));
            u64 movedMarks = 0;
            const std::vector<u64> ePatched = saiPatchedRef(W, Wold.e, textOf(Gnew), newPos, C.L, gsb, &movedMarks);
            std::vector<u64> got = down(be, D.dSAiPacked, nGW), exp = packRef(ePatched, gsb + 3, nGW);
            if (got != exp) for (u64 e = 0; e < ePatched.size(); e++) if (packedGetW(got.data(), e, gsb + 3) != ePatched[e]) {
                R.diff("SAindex of the merged array: entry %llu = %llx, expected %llx", (unsigned long long)e, (unsigned long long)packedGetW(got.data(), e, gsb + 3), (unsigned long long)ePatched[e]); break; }
            R.same("SAindex of the merged array", got, exp);
            R.hit("insert: SAindex of the merged array");
            if (movedMarks) R.hit("insert: N mark kept where the old table had it, not where a walk would put it", movedMarks);
        }
    }
    be.free(D.dSApacked); be.free(D.dGnew); be.free(D.dSAiPacked); be.free(dGraw); be.free(dSAold); be.free(dSAiOld);
    if (at0) R.hit("insert: new entry at output index 0", at0);
    if (atLast) R.hit("insert: new entry at the last index", atLast);
    if (runs) R.hit("insert: run of 3 or more new entries", runs);
    if (at64) R.hit("insert: new entry at a multiple of 64", at64);
    if (at63) R.hit("insert: new entry at 63 mod 64", at63);
    if (identical) R.hit("insert: identical junction texts (offset order)", identical);
    if (hasN) R.hit("insert: junction text with N");
    if (movedPlus) R.hit("insert: old junction moved, + strand", movedPlus);
    if (movedMinus) R.hit("insert: old junction moved, - strand", movedMinus);
    if (oldSjdbN && !moved) R.hit("insert: old junctions, identity numbering");
    if (shiftedMinus) R.hit("insert: old chromosome entry, - strand shifted", shiftedMinus);
    { const u32 ch = (Lsj + 20) / 21; R.hit(ch == 1 ? "insert: one radix chunk" : ch == 2 ? "insert: two radix chunks" : ch == 3 ? "insert: three radix chunks" : "insert: ten radix chunks"); }
    R.hit(gsb == 32 ? "insert: GstrandBit 32" : gsb == 33 ? "insert: GstrandBit 33" : "insert: GstrandBit 36");
    if (nInd <= 2) R.hit("insert: nInd 1 or 2");
    checkBackend(be, R);
    R.end();
}

// =====================================================================================================================
// 4. backend primitives

template <class BE> void casePrimitives(BE &be, Report &R, u64 n, Rng &rng) {
    const std::string tag = "n " + std::to_string(n);
    const u64 GUARDV = 0xFEEDFACECAFEBEEFull;
    // ---- forEach, readOne
    R.begin("forEach " + tag);
    {
        std::vector<u64> init(n + 2, GUARDV);
        u64 *d = up(be, init); u64 *o = d + 1;
        be.forEach(n, [=] IDX_L (u64 i) { o[i] = i * 2654435761ull + 1; });
        std::vector<u64> got = down(be, d, n + 2), exp(n + 2, GUARDV);
        for (u64 i = 0; i < n; i++) exp[i + 1] = i * 2654435761ull + 1;
        R.same("forEach", got, exp); R.hit("prim: forEach");
        const u64 at[3] = {0, n / 2, n - 1};
        for (u64 i : at) R.eq("readOne", be.readOne(o + i), i * 2654435761ull + 1);
        R.hit("prim: readOne");
        be.free(d);
    }
    checkBackend(be, R); R.end();
    // ---- scans in place
    R.begin("scans " + tag);
    {
        std::vector<u64> a(n + 2, GUARDV), b(n + 2, GUARDV);
        for (u64 i = 1; i <= n; i++) { a[i] = rng.below(1000); b[i] = rng.below(16) == 0 ? rng.below(1ull << 40) : rng.below(100); }
        u64 *da = up(be, a), *db = up(be, b);
        be.exclusiveSum(da + 1, n); be.inclusiveMax(db + 1, n);
        std::vector<u64> ea = a, eb = b; u64 s = 0, m = 0;
        for (u64 i = 1; i <= n; i++) { ea[i] = s; s += a[i]; m = std::max(m, b[i]); eb[i] = m; }
        R.same("exclusiveSum", down(be, da, n + 2), ea); R.hit("prim: exclusiveSum in place");
        R.same("inclusiveMax", down(be, db, n + 2), eb); R.hit("prim: inclusiveMax in place");
        be.free(da); be.free(db);
    }
    checkBackend(be, R); R.end();
    // ---- compactIf
    for (int mode = 0; mode < 4; mode++) {
        R.begin("compactIf mode " + std::to_string(mode) + " " + tag);
        std::vector<u8> f(n);
        for (u64 i = 0; i < n; i++) f[i] = mode == 0 ? 0 : mode == 1 ? 1 : mode == 2 ? (u8)(i & 1) : (u8)(rng.below(3) == 0);
        std::vector<u64> init(n + 2, GUARDV), exp(n + 2, GUARDV); u64 cnt = 0;
        for (u64 i = 0; i < n; i++) if (f[i]) exp[1 + cnt++] = i;
        u8 *df = up(be, f); u64 *d = up(be, init); u64 *o = d + 1; const u8 *ff = df;
        const u64 got = compactIf(be, n, [=] IDX_L (u64 i) { return ff[i] != 0; }, [=] IDX_L (u64 i, u64 k) { o[k] = i; });
        R.eq("compactIf count", got, cnt);
        R.same("compactIf output", down(be, d, n + 2), exp);
        R.hit(mode == 0 ? "prim: compactIf none" : mode == 1 ? "prim: compactIf all" : mode == 2 ? "prim: compactIf alternating" : "prim: compactIf random");
        be.free(df); be.free(d);
        checkBackend(be, R); R.end();
    }
    // ---- sortPairs
    for (int range = 0; range < 3; range++) {
        R.begin("sortPairs range " + std::to_string(range) + " " + tag);
        const int b1 = range == 0 ? 63 : range == 1 ? 1 : (int)bitsFor(4 * n);
        std::vector<u64> k(n), v(n);
        const u64 distinct = n / 7 + 1;
        for (u64 i = 0; i < n; i++) { k[i] = rng.below(distinct) | ((rng.next() & 1) << 63) | (range == 2 ? (rng.below(4) << 40) : 0); v[i] = i; }
        u64 *k0 = up(be, k), *k1 = be.template alloc<u64>(n), *v0 = up(be, v), *v1 = be.template alloc<u64>(n);
        u64 *pk = k0, *pkA = k1, *pv = v0, *pvA = v1;
        be.sortPairs(pk, pkA, pv, pvA, n, 0, b1);
        if (!((pk == k0 && pkA == k1) || (pk == k1 && pkA == k0)) || !((pv == v0 && pvA == v1) || (pv == v1 && pvA == v0))) R.diff("sortPairs: k/kAlt/v/vAlt do not name the buffers handed in");
        const u64 mask = (1ull << b1) - 1;
        std::vector<u64> idx(n); std::iota(idx.begin(), idx.end(), 0);
        std::stable_sort(idx.begin(), idx.end(), [&](u64 a, u64 b) { return (k[a] & mask) < (k[b] & mask); });
        std::vector<u64> ek(n), ev(n); for (u64 i = 0; i < n; i++) { ek[i] = k[idx[i]]; ev[i] = v[idx[i]]; }
        R.same("sortPairs keys (in the buffer k names)", down(be, pk, n), ek);
        R.same("sortPairs values (in the buffer v names)", down(be, pv, n), ev);
        R.hit(range == 0 ? "prim: sortPairs bits 0-63 (bit 63 is no sort bit)" : range == 1 ? "prim: sortPairs bits 0-1" : "prim: sortPairs bits 0-bitsFor(4n)");
        be.free(k0); be.free(k1); be.free(v0); be.free(v1);
        checkBackend(be, R); R.end();
    }
    if (n == 1) R.hit("prim: n 1");
    if (n == 3000001) R.hit("prim: n 3000001");
}

// =====================================================================================================================
// 5. fixtures the reference wrote (tests/golden/tiny_index/<case>/{plain,annot}/...)

static inline bool readAll(const std::string &path, std::vector<u8> &out) {
    FILE *f = fopen(path.c_str(), "rb"); if (!f) return false;
    out.clear(); u8 buf[65536]; size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
    fclose(f); return true;
}
static inline i64 paramOf(const std::vector<u8> &txt, const char *key) {            // "key<white space>value" at a line start ("### GstrandBit 32" included)
    const std::string s(txt.begin(), txt.end()), k(key);
    for (size_t p = 0; (p = s.find(k, p)) != std::string::npos; p += k.size()) {
        if (p && s[p - 1] != '\n' && !(p >= 4 && s.compare(p - 4, 4, "### ") == 0)) continue;
        const char c = s[p + k.size()]; if (c != ' ' && c != '\t') continue;
        return atoll(s.c_str() + p + k.size() + 1);
    }
    return -1;
}

template <class BE> void caseFixture(BE &be, Report &R, const std::string &dir, const std::string &name) {
    R.begin("fixture " + name);
    std::vector<u8> G, SA, SAI, par, chrs, G2, SA2, SAI2, par2, sjl;
    const std::string p = dir + "/" + name + "/plain/", a = dir + "/" + name + "/annot/";
    if (!readAll(p + "Genome", G) || !readAll(p + "SA", SA) || !readAll(p + "SAindex", SAI) || !readAll(p + "genomeParameters.txt", par) || !readAll(p + "chrStart.txt", chrs) ||
        !readAll(a + "Genome", G2) || !readAll(a + "SA", SA2) || !readAll(a + "SAindex", SAI2) || !readAll(a + "genomeParameters.txt", par2) || !readAll(a + "sjdbList.out.tab", sjl)) {
        R.diff("fixture files missing under %s/%s", dir.c_str(), name.c_str()); return;
    }
    const u32 gsb = (u32)paramOf(par, "GstrandBit"), gsb2 = (u32)paramOf(par2, "GstrandBit"), ov = (u32)paramOf(par2, "sjdbOverhang"), Lsj = 2 * ov + 1;
    u64 L; memcpy(&L, SAI.data(), 8);
    const u64 N = G.size(), hdr = 8 * (L + 2);
    u64 nReal = 0; { const std::string s(chrs.begin(), chrs.end()); size_t q = 0; while (q < s.size()) { nReal = strtoull(s.c_str() + q, nullptr, 10); q = s.find('\n', q); if (q == std::string::npos) break; q++; } }
    u32 sjdbN = 0; for (u8 c : sjl) if (c == '\n') sjdbN++;
    if (gsb != gsb2 || nReal != N || G2.size() != N + (u64)sjdbN * Lsj || !sjdbN || L < 1 || L > 16 || memcmp(G.data(), G2.data(), N)) { R.diff("fixture %s: inconsistent files", name.c_str()); return; }
    // ---- plain: brute-force order and the sequential walk against the files' bytes
    const Text T = textOf(G);
    const std::vector<u64> ord = bruteOrder(T);
    u64 nSA = 0; for (u8 c : T.t) if (c < 4) nSA++;
    std::vector<u64> sa(nSA); for (u64 i = 0; i < nSA; i++) sa[i] = saValueRef(ord[i], N, gsb);
    const SaiWalk W = saiWalkRef(G, gsb, sa, (u32)L);
    {
        std::vector<u64> w = packRef(sa, gsb + 1, packedWords(nSA, gsb + 1)), wi = packRef(W.e, gsb + 3, packedWords(W.start[L], gsb + 3));
        R.eq("SA file size", SA.size(), packedBytes(nSA, gsb + 1)); R.eq("SAindex file size", SAI.size(), hdr + packedBytes(W.start[L], gsb + 3));
        if (SA.size() == packedBytes(nSA, gsb + 1) && memcmp(SA.data(), w.data(), SA.size())) R.diff("brute-force order differs from the reference's SA file");
        if (memcmp(SAI.data() + 8, W.start, 8 * (L + 1))) R.diff("SAindex header differs");
        if (SAI.size() == hdr + packedBytes(W.start[L], gsb + 3) && memcmp(SAI.data() + hdr, wi.data(), SAI.size() - hdr)) R.diff("sequential SAindex walk differs from the reference's SAindex file");
        R.hit("fixture: order and SAindex walk against the reference's files");
    }
    // ---- plain: the product
    {
        const u64 GUARD = 64, saB = packedBytes(nSA, gsb + 1), saiB = packedBytes(W.start[L], gsb + 3);
        std::vector<u8> hSA(saB + 2 * GUARD, 0xC3), hSAi(saiB + 2 * GUARD, 0xC3);
        BuildParams P; P.nGenome = N; P.GstrandBit = gsb; P.saIndexNbases = (u32)L; BuildResult B;
        R.eq("buildAll return", (u64)(i64)buildAll(be, G.data(), P, hSA.data() + GUARD, saB, hSAi.data() + GUARD, saiB, B), 0);
        if (SA.size() != saB || memcmp(SA.data(), hSA.data() + GUARD, saB)) R.diff("buildAll: SA differs from the reference's file");
        if (SAI.size() != hdr + saiB || memcmp(SAI.data() + hdr, hSAi.data() + GUARD, saiB)) R.diff("buildAll: SAindex differs from the reference's file");
        R.hit("fixture: buildAll against the reference's files");
    }
    checkBackend(be, R);
    // ---- annotated: insertion from the plain index; Gsj = the junction block of the annotated Genome, nothing old
    {
        const u64 nGsj = (u64)sjdbN * Lsj;
        const u8 *Gsj = G2.data() + N;
        std::vector<u8> Q(2 * nGsj + 65, 5);
        for (u64 i = 0; i < nGsj; i++) { Q[i] = Gsj[i]; Q[2 * nGsj - 1 - i] = Gsj[i] < 4 ? (u8)(3 - Gsj[i]) : Gsj[i]; }
        std::vector<u64> off; for (u64 o = 0; o < 2 * nGsj; o++) if (Q[o] <= 3) off.push_back(o);
        std::vector<u64> ipos(off.size()); for (u64 j = 0; j < off.size(); j++) ipos[j] = searchRef(G, gsb, sa, nSA, &Q[off[j]], nullptr);
        std::vector<u64> perm(off.size()); std::iota(perm.begin(), perm.end(), 0);
        std::stable_sort(perm.begin(), perm.end(), [&](u64 x, u64 y) {
            if (ipos[x] != ipos[y]) return ipos[x] < ipos[y];
            for (u64 k = 0;; k++) { const u8 cx = Q[off[x] + k], cy = Q[off[y] + k]; if (cx != cy) return cx < cy; if (cx == 5) return off[x] < off[y]; }
        });
        const u64 nInd = off.size(), nSAnew = nSA + nInd, N2bit = 1ull << gsb;
        std::vector<u64> saNew, newPos; saNew.reserve(nSAnew);
        u64 isj = 0;
        auto newVal = [&](u64 o) { newPos.push_back(o < nGsj ? o + N : N + nGsj + (o - nGsj)); return o < nGsj ? o + N : (o - nGsj) | N2bit; };
        for (u64 isa = 0; isa < nSA; isa++) {
            while (isj < nInd && ipos[perm[isj]] == isa) saNew.push_back(newVal(off[perm[isj++]]));
            saNew.push_back((sa[isa] & N2bit) ? sa[isa] + nGsj : sa[isa]);
        }
        while (isj < nInd) saNew.push_back(newVal(off[perm[isj++]]));
        const SaiWalk W2 = saiWalkRef(G2, gsb, saNew, (u32)L);
        const std::vector<u64> e2 = saiPatchedRef(W2, W.e, textOf(G2), newPos, (u32)L, gsb);
        std::vector<u64> w = packRef(saNew, gsb + 1, packedWords(nSAnew, gsb + 1)), wi = packRef(e2, gsb + 3, packedWords(W2.start[L], gsb + 3));
        const u64 saB = packedBytes(nSAnew, gsb + 1), saiB = packedBytes(W2.start[L], gsb + 3);
        R.eq("annotated SA file size", SA2.size(), saB); R.eq("annotated SAindex file size", SAI2.size(), hdr + saiB);
        if (SA2.size() == saB && memcmp(SA2.data(), w.data(), saB)) R.diff("restated insertion differs from the reference's annotated SA file");
        if (SAI2.size() == hdr + saiB && memcmp(SAI2.data() + hdr, wi.data(), saiB)) {
            std::vector<u64> fw(packedWords(W2.start[L], gsb + 3), 0); memcpy(fw.data(), SAI2.data() + hdr, saiB);
            for (u32 iL = 0; iL < L; iL++) for (u64 e = W2.start[iL]; e < W2.start[iL + 1]; e++) if (packedGetW(fw.data(), e, gsb + 3) != e2[e])
                R.diff("annotated SAindex level %u entry %llu: the restated patch gives %llx, the reference's file %llx", iL + 1, (unsigned long long)(e - W2.start[iL]),
                       (unsigned long long)e2[e], (unsigned long long)packedGetW(fw.data(), e, gsb + 3));
        }
        R.hit("fixture: insertion restated against the reference's files");
        // the product, host buffers in and out
        const u64 GUARD = 64;
        std::vector<u8> oSA(saB + 2 * GUARD, 0xC3), oSAi(saiB + 2 * GUARD, 0xC3), isOld(sjdbN, 0);
        SjdbParams P; P.nGenomeOld = N; P.nGenomeReal = N; P.nSAold = nSA; P.GstrandBit = gsb; P.sjdbN = sjdbN; P.sjdbLength = Lsj; P.oldSjdbN = 0; P.sjNew = sjdbN; P.saIndexNbases = (u32)L;
        SjdbHostArgs A{G.data(), SA.data(), SA.size(), Gsj, isOld.data(), nullptr, oSA.data() + GUARD, saB, oSAi.data() + GUARD, saiB, SAI.data() + hdr};
        u64 gotInd = 0, gotB = 0, gotBi = 0;
        R.eq("sjdbInsertHost return", (u64)(i64)sjdbInsertHost(be, P, A, gotInd, gotB, gotBi), 0);
        R.eq("sjdbInsertHost nInd", gotInd, nInd); R.eq("sjdbInsertHost SA bytes", gotB, saB); R.eq("sjdbInsertHost SAindex bytes", gotBi, saiB);
        if (SA2.size() != saB || memcmp(SA2.data(), oSA.data() + GUARD, saB)) R.diff("sjdbInsertHost: SA differs from the reference's annotated file");
        if (SAI2.size() != hdr + saiB || memcmp(SAI2.data() + hdr, oSAi.data() + GUARD, saiB)) R.diff("sjdbInsertHost: SAindex differs from the reference's annotated file");
        for (u64 i = 0; i < GUARD; i++) if (oSA[i] != 0xC3 || oSA[oSA.size() - 1 - i] != 0xC3 || oSAi[i] != 0xC3 || oSAi[oSAi.size() - 1 - i] != 0xC3) { R.diff("sjdbInsertHost: guard bytes overwritten"); break; }
        R.hit("fixture: sjdbInsertHost against the reference's files");
    }
    checkBackend(be, R);
    R.end();
}

// =====================================================================================================================
// the case list

static inline std::vector<u8> genomeWithRepeats(Rng &r, u64 n, u32 families, u32 copies, u32 len, u32 nN) {
    std::vector<u8> g = rndBases(r, n);
    for (u32 f = 0; f < families; f++) {
        const std::vector<u8> unit = rndBases(r, len);
        for (u32 c = 0; c < copies; c++) { const u64 at = r.below(n - len); std::copy(unit.begin(), unit.end(), g.begin() + at); if (r.below(2)) g[at + r.below(len)] = (u8)r.below(4); }
    }
    for (u32 i = 0; i < nN; i++) g[r.below(n)] = 4;
    return g;
}

template <class BE> void runGenomeCases(BE &be, Report &R) {
    Rng r(11);
    GenomeOpts small; small.Ls = {1, 2, 3}; small.gsbs = {32};
    auto word = [&](std::initializer_list<int> l) { std::vector<u8> g; for (int c : l) g.push_back((u8)c); return g; };
    // 1, 2, 22, 23, 24 bases
    for (u64 n : {1, 2, 22, 23, 24}) caseGenome(be, R, "random " + std::to_string(n) + " bases", rndBases(r, n), small);
    // 2N around multiples of 256 (CHUNK)
    for (u64 n : {127, 128, 129, 255, 256, 257}) caseGenome(be, R, "2N " + std::to_string(2 * n), rndBases(r, n), small);
    // no ACGT at all; one base among N
    caseGenome(be, R, "all N", std::vector<u8>(40, 4), small);
    { std::vector<u8> g(30, 4); g[11] = 1; caseGenome(be, R, "one base among N", g, small); }
    { std::vector<u8> g(300, 4); g[100] = 2; g[200] = 2; g[201] = 3; caseGenome(be, R, "three bases among N", g, small); }
    // nSA 62 .. 130 (nSA is even: two strands); buildSAindex additionally over the first 63 and 65 suffixes
    for (u64 n : {31, 32, 33, 64}) { GenomeOpts o = small; o.truncSA = n == 32 ? 63 : n == 33 ? 65 : 0; std::vector<u8> g = rndBases(r, n); g.push_back(4); g.push_back(4); caseGenome(be, R, "nSA " + std::to_string(2 * n), g, o); }
    // only C and G: prefix A is absent in front of the first present prefix of every level
    { std::vector<u8> g(200); for (auto &c : g) c = (u8)(1 + r.below(2)); GenomeOpts o; o.Ls = {1, 2, 6}; o.gsbs = {32, 33}; caseGenome(be, R, "C and G only", g, o); }
    // chromosomes padded to 256 whose ends share a tail; what follows the padding contradicts position order (the later chromosome is
    // followed by a smaller base than the earlier one), and so does what precedes the heads on the other strand
    for (u32 tail : {1, 20, 21, 22, 40}) {
        const std::vector<u8> t = rndBases(r, tail); std::vector<u8> g;
        const u8 first[4] = {3, 2, 1, 0};
        for (u32 c = 0; c < 4; c++) { std::vector<u8> chr = rndBases(r, 150 - tail); chr[0] = first[c]; append(chr, t); append(g, chr); padTo(g, 256); }
        GenomeOpts o; o.Ls = {2, 6}; o.gsbs = {32};
        caseGenome(be, R, "shared tail " + std::to_string(tail), g, o);
    }
    // a repeat of the genome's first k bases elsewhere: on the other strand a suffix ends exactly at the text end
    for (u32 k : {23, 46, 100}) {
        std::vector<u8> g = rndBases(r, 700); std::copy(g.begin(), g.begin() + k, g.begin() + 400); g[400 + k] = (u8)((g[k] + 1) & 3);
        GenomeOpts o; o.Ls = {3}; o.gsbs = {32};
        caseGenome(be, R, "head repeated " + std::to_string(k), g, o);
    }
    // runs of period 1, 2 and 7 (many doubling rounds), sized so that the brute-force sort stays cheap
    {
        GenomeOpts o; o.Ls = {2, 8}; o.gsbs = {32};
        std::vector<u8> g = rndBases(r, 300); g.insert(g.end(), 4096, (u8)0); append(g, rndBases(r, 300)); caseGenome(be, R, "period 1 run of 4096", g, o);
        g = rndBases(r, 200); for (u32 i = 0; i < 2000; i++) g.push_back((u8)(i & 1 ? 2 : 1)); append(g, rndBases(r, 200)); caseGenome(be, R, "period 2 run of 2000", g, o);
        g = rndBases(r, 200); const std::vector<u8> u = word({0, 3, 3, 1, 2, 0, 1}); for (u32 i = 0; i < 1500; i++) g.push_back(u[i % 7]); append(g, rndBases(r, 200)); caseGenome(be, R, "period 7 run of 1500", g, o);
        // a reverse palindrome of 46 bases: the position and its twin on the other strand share 46 codes, every other pair fewer, so the last round sorts
        // U = 2 elements (the two strands mirror each other, so U is even and 1 is never met; the smallest bucket or group that is sorted has 2)
        g = rndBases(r, 30); { std::vector<u8> x = rndBases(r, 23); append(g, x); std::reverse(x.begin(), x.end()); for (auto &c : x) c = (u8)(3 - c); append(g, x); } append(g, rndBases(r, 30));
        caseGenome(be, R, "one pair tied in the last round", g, small);
    }
    // an N run of 600
    { std::vector<u8> g = rndBases(r, 500); g.insert(g.end(), 600, (u8)4); append(g, rndBases(r, 500)); GenomeOpts o; o.Ls = {4}; o.gsbs = {32}; o.nRun600 = true; caseGenome(be, R, "N run of 600", g, o); }
    // random genomes with planted repeat families and single N (a non-ACGT code at every offset of some suffix); all widths, all L
    {
        GenomeOpts o; o.Ls = {1, 2, 3, 6, 8}; o.gsbs = {32, 33, 36};
        caseGenome(be, R, "random 3 kb, repeats, N", genomeWithRepeats(r, 3000, 4, 6, 80, 12), o);
        GenomeOpts o2; o2.Ls = {6, 12}; o2.gsbs = {33};
        std::vector<u8> g = genomeWithRepeats(r, 20000, 6, 10, 300, 30); std::copy(g.begin() + 1000, g.begin() + 3000, g.begin() + 12000); padTo(g, 256); append(g, genomeWithRepeats(r, 2000, 2, 4, 60, 3));
        caseGenome(be, R, "random 22 kb, repeat families, 2 kb duplicate", g, o2);
        GenomeOpts o3; o3.Ls = {12}; o3.gsbs = {32};
        caseGenome(be, R, "L 12 on 300 bases", genomeWithRepeats(r, 300, 1, 2, 30, 2), o3);
    }
    // the smallest suffix has N inside the prefix: "AN" with no other A..: -3
    { std::vector<u8> g = word({0, 4, 1, 1, 2, 1, 1, 2, 1}); GenomeOpts o; o.Ls = {2, 5}; o.gsbs = {32}; caseGenome(be, R, "first suffix with N inside the prefix", g, o); }
    caseBuildErrors(be, R, genomeWithRepeats(r, 500, 1, 2, 40, 2));
}

template <class BE> void runPackCases(BE &be, Report &R) {
    Rng r(12);
    for (u32 bits : {33, 34, 35, 36, 40, 63, 3}) for (u64 n : {1, 63, 64, 65, 127, 128, 129}) casePack(be, R, bits, n, r);
}

template <class BE> void runPrimitiveCases(BE &be, Report &R) {
    Rng r(13);
    for (u64 n : {1ull, 2ull, 255ull, 256ull, 257ull, 4095ull, 4096ull, 4097ull, 100003ull, 3000001ull}) casePrimitives(be, R, n, r);
}

template <class BE> void runInsertCases(BE &be, Report &R) {
    Rng r(14);
    auto sub = [](const std::vector<u8> &g, u64 a, u64 n) { return std::vector<u8>(g.begin() + a, g.begin() + a + n); };
    auto revc = [](std::vector<u8> v) { std::reverse(v.begin(), v.end()); for (auto &c : v) if (c < 4) c = (u8)(3 - c); return v; };
    const u32 Ls[5] = {3, 21, 22, 43, 201}, gsbs[3] = {32, 33, 36};
    int n = 0;
    for (u32 Lsj : Ls) for (int variant = 0; variant < 3; variant++, n++) {
        InsCase C; C.Lsj = Lsj; C.gsb = gsbs[n % 3]; C.L = Lsj == 3 ? 2 : variant == 2 ? 6 : 4;
        const u32 J = Lsj - 1;
        // chromosomes: two, padded to 256; a few thousand suffixes
        std::vector<u8> g = genomeWithRepeats(r, 900 + 300 * variant, 2, 4, 50, 3); padTo(g, 256);
        const u64 chr2 = g.size(); append(g, genomeWithRepeats(r, 700, 1, 3, 40, 0)); const u64 end2 = g.size(); padTo(g, 256);
        C.Gchr = g;
        auto junction = [&]() { std::vector<u8> j = sub(g, 10 + r.below(300), J / 2); append(j, sub(g, 400 + r.below(200), J - J / 2)); return j; };       // donor + acceptor flanks
        // old junctions
        const u32 nOld = variant == 0 ? 0 : variant == 1 ? 3 : 7;
        for (u32 i = 0; i < nOld; i++) C.oldJ.push_back(junction());
        // new table: old ones in order; new ones in front, between and behind (variant 2) or behind only (variant 1: identity numbering)
        std::vector<std::vector<u8>> fresh;
        const u32 nNew = variant == 0 ? (Lsj == 3 ? 300 : Lsj == 201 ? 12 : 60) : variant == 1 ? 5 : Lsj == 201 ? 10 : 40;
        for (u32 i = 0; i < nNew; i++) fresh.push_back(junction());
        if (J >= 2) {
            { std::vector<u8> j = junction(); std::vector<u8> t = sub(g, end2 - J / 2, J / 2); std::copy(t.begin(), t.end(), j.end() - J / 2); fresh[0] = j; }                     // ends as chromosome 2 ends: tie, + strand
            { std::vector<u8> j = junction(); std::vector<u8> t = revc(sub(g, chr2, J / 2)); std::copy(t.begin(), t.end(), j.end() - J / 2); fresh[1] = j; }                       // ends as the - strand of chromosome 2's head: tie, - strand
            fresh[2] = fresh[3];                                                                                                                                              // identical texts
            fresh[4][J / 2] = 4;                                                                                                                                              // N inside
            if (nNew > 8) { fresh[5].assign(J, 0); fresh[6].assign(J, 3); fresh[7].assign(J, 3); fresh[7][J - 1] = 2; }                                                        // below and above every old suffix
        }
        u32 io = 0, in = 0;
        if (variant == 2) { for (; in < 3 && in < fresh.size(); in++) { C.newJ.push_back(fresh[in]); C.newIsOld.push_back(-1); } }
        while (io < nOld || in < fresh.size()) {
            if (io < nOld) { C.newJ.push_back(C.oldJ[io]); C.newIsOld.push_back((int)io); io++; }
            if (variant == 2 || io >= nOld) for (u32 k = 0; k < (variant == 2 ? 4u : 1u << 30) && in < fresh.size(); k++, in++) { C.newJ.push_back(fresh[in]); C.newIsOld.push_back(-1); }
        }
        C.nSAoldUse = variant == 0 ? 1 : variant == 1 ? 2 : 17;
        C.name = "insert Lsj " + std::to_string(Lsj) + " variant " + std::to_string(variant);
        caseInsert(be, R, C);
    }
    // old indexes of two suffixes; 1 and 2 junctions
    for (int k = 0; k < 2; k++) {
        InsCase C; C.Lsj = 3; C.gsb = 32; C.L = 1; C.Gchr.assign(40, 4); C.Gchr[17] = 1;
        C.newJ.push_back({(u8)(k ? 0 : 1), 4}); C.newIsOld.push_back(-1);
        if (k) { C.newJ.push_back({3, 3}); C.newIsOld.push_back(-1); }
        C.nSAoldUse = 1; C.name = "insert into two suffixes, " + std::to_string(k + 1) + " junctions";
        caseInsert(be, R, C);
    }
}

template <class BE> void runFixtureCases(BE &be, Report &R, const std::string &dir) {
    for (const char *c : FIXTURE_CLASSES) R.declare(c);
    for (const char *c : {"tails", "nprefix", "repeats"}) caseFixture(be, R, dir, c);
}

} // namespace idxchk
