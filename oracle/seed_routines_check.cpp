// seed_routines_check.cpp -- TEST INFRASTRUCTURE: the seed-search routines of star_amd/csrc/engine/k_seed.hip, one at a time, against the oracle (star_oracle.cpp, the
// line-by-line restatement pinned to the reference) and a brute-force scan, on small adversarial genomes: k_sak_build's key records against a base-by-base construction,
// compareSeqToGenome with and without keys, mmpRunT<u32> and mmpRunT<u64>, seedLookup, nextPiece.  Host build through the wavefront emulator's headers (oracle/wave_emul);
// suffix array and SAindex from the project's own index twin (index_emul.cpp).  Every case is classified from the reference side; a class that never occurred fails the run.
// usage: seed_routines_check [trials] [--dump file]      (--dump: three genomes only; their cases go to `file` for tests/seed_routines_gpu.hip, see seed_routines_cases.h)
#include "k_seed.hip"
#include "star_oracle.cpp"
#include "seed_routines_cases.h"
#include <cstdio>
#include <random>
#include <string>
#include <sys/mman.h>
#include <csignal>
#include <cerrno>
#include <unistd.h>

extern "C" int index_emul_build(const uint8_t *G, uint64_t nGenome, uint32_t GstrandBit, uint32_t saIndexNbases, uint8_t *SA, uint64_t saCap, uint8_t *SAi, uint64_t saiCap, uint64_t *out);

static std::mt19937_64 rng(20240611);
static u32 rnd(u32 n) { return (u32)(rng() % n); }

enum { PADR = 64, ACGT_CAP = 60000 };
// saiNbases and GstrandBit of the three index shapes.  14 (the human default) would make a table of 3.6 * 10^8 entries per genome: 11 is the largest that keeps a genome's
// build at a fraction of a second, and with 4^11 L-mers for < 10^5 suffixes it has what 14 has at full size: mostly absent L-mers, single-suffix entries
static const u32 SHAPES[3][2] = {{4, 32}, {8, 33}, {11, 32}};

struct Gen {
    std::vector<u8> gbuf; u8 *G = nullptr; u64 n = 0; std::vector<u64> cs, cl; int cls = 0;     // cls 0: with N; 1: no non-ACGT code but the padding; 2: as 1, bases C and G only
    u32 P0 = 0, sbit = 0; u64 nSA = 0, nSAi = 0;
    std::vector<u64> SAw, SAiw, pos, inv; std::vector<u8> fwd; std::vector<u16> acgt; std::vector<u8> edge;
    std::vector<SakRec> sak;
    DevIndex X, X0;              // with and without the keys
    Oracle O;
    // the same suffix array with the entry of the genome's first base repeated WIDE_EXTRA times more (still sorted: equal suffixes side by side), so that an interval across
    // the copies has more than 2^32 entries: what mmpRun hands to mmpRunT<u64>.  The copies are words of zero in a mapping that is never touched (forward strand, position 0);
    // entries of the fewest bits the genome allows keep the mapping at 9 GB of address space.  Without keys (their records would be 69 GB that are not zero)
    u64 *wide = nullptr; size_t wideBytes = 0; u64 wideAt = 0, wideHeadWords = 0, wideTailWord = 0, wideWords = 0; u32 wbit = 0;
    DevIndex XW; Oracle OW;
    ~Gen() { if (wide) munmap(wide, wideBytes); }
};
static const u64 WIDE_EXTRA = (1ull << 32) + 12345;
static void packedPut(u64 *words, u64 i, u32 bits, u64 v) { const u64 b = i * bits, w = b >> 6; const u32 sh = (u32)(b & 63); words[w] |= v << sh; if (sh + bits > 64) words[w + 1] |= v >> (64 - sh); }
static inline u8 textAt(const Gen &g, u64 i, u32 k) { const u64 p = g.pos[i]; return g.fwd[i] ? g.G[p + k] : compBase(g.G[(i64)(g.n - 1 - p) - (i64)k]); }

static void makeGenome(Gen &g, int cls) {
    g.cls = cls; g.cs.clear(); g.cl.clear();
    const u32 nChr = 3 + rnd(6); u64 start = 0; std::vector<u32> longChr;
    for (u32 c = 0; c < nChr; c++) {
        const u64 len = (c > 0 && rnd(3) == 0) ? 3 + rnd(43) : 1500 + rnd(5500);
        g.cs.push_back(start); g.cl.push_back(len); if (len >= 1500) longChr.push_back(c);
        start = ((start + len) / 64 + 1) * 64;               // chromosomes start at multiples of the bin; at least one byte of padding behind each
    }
    g.n = start; g.gbuf.assign(g.n + 2 * GPAD, 5); g.G = g.gbuf.data() + GPAD;
    u8 *G = g.G;
    for (u32 c = 0; c < nChr; c++) for (u64 i = 0; i < g.cl[c]; i++) G[g.cs[c] + i] = cls == 2 ? (u8)(1 + rnd(2)) : (u8)rnd(4);
    auto place = [&](u32 len) { const u32 c = longChr[rnd((u32)longChr.size())]; return g.cs[c] + rnd((u32)(g.cl[c] - len)); };
    for (u32 k = 0, nk = 6 + rnd(10); k < nk; k++) {         // tandem and low-complexity stretches
        const u32 len = 20 + rnd(180), per = 1 + rnd(6); const u64 p = place(len);
        for (u32 i = per; i < len; i++) G[p + i] = G[p + i - per];
    }
    for (u32 k = 0, nk = 4 + rnd(6); k < nk; k++) {          // repeat families, longer than saiNbases + 32: exact and 1-5 % diverged copies on either strand, some against chromosome ends
        const u32 len = 50 + rnd(350); const u64 src = place(len);
        std::vector<u8> s(G + src, G + src + len);
        const u32 div = rnd(2) ? 0 : 1 + rnd(5);
        for (u32 m = 0, nm = 2 + rnd(5); m < nm; m++) {
            const u32 c = longChr[rnd((u32)longChr.size())], how = rnd(5);
            u64 d = how == 0 ? g.cs[c] : how == 1 ? g.cs[c] + g.cl[c] - len : how == 2 ? 0 : place(len);
            const bool rc = rnd(2);
            for (u32 i = 0; i < len; i++) { u8 b = rc ? compBase(s[len - 1 - i]) : s[i]; if (div && rnd(100) < div) b = cls == 2 ? (u8)(3 - b) : (u8)((b + 1 + rnd(3)) & 3); G[d + i] = b; }
        }
        for (u32 c = 0; c < nChr; c++) if (g.cl[c] < 46 && rnd(2)) for (u64 i = 0; i < g.cl[c]; i++) G[g.cs[c] + i] = s[i];      // a very short chromosome that is the head of a repeat
    }
    if (cls == 0) {
        for (u32 k = 0, nk = 3 + rnd(5); k < nk; k++) { const u32 len = 1 + rnd(40); const u64 p = place(len); for (u32 i = 0; i < len; i++) G[p + i] = 4; }
        for (u32 k = 0, nk = 10 + rnd(20); k < nk; k++) G[place(1)] = 4;
    }
}

// suffix array, SAindex, key records, the oracle: false when the index twin refuses the genome (its first suffix has a non-ACGT code inside the SAindex prefix)
static long sakDiffs = 0, orderBad = 0, wideRefused = 0; static u64 sakRecords = 0, sakRevNearStart = 0, sakNearPad = 0, sakShortKlen = 0;
static bool buildIndex(Gen &g, u32 shape) {
    g.P0 = SHAPES[shape][0]; g.sbit = SHAPES[shape][1];
    const u32 saBits = g.sbit + 1, saiBits = g.sbit + 3;
    u64 nSAi = 0; for (u32 i = 1; i <= g.P0; i++) nSAi += 1ull << (2 * i);
    g.SAw.assign((2 * g.n * saBits) / 64 + 4, 0); g.SAiw.assign((nSAi * saiBits) / 64 + 4, 0);
    u64 out[5 + 17];
    if (index_emul_build(g.G, g.n, g.sbit, g.P0, (u8 *)g.SAw.data(), g.SAw.size() * 8 - 16, (u8 *)g.SAiw.data(), g.SAiw.size() * 8 - 16, out)) return false;
    g.nSA = out[0]; g.nSAi = out[2];
    DevIndex &X = g.X; memset(&X, 0, sizeof(X));
    X.G = g.G; X.SA = g.SAw.data(); X.SAi = g.SAiw.data(); X.nGenome = g.n; X.nSA = g.nSA;
    for (int i = 0; i < 17; i++) X.saiStart[i] = out[5 + i];
    X.strandBit = g.sbit; X.saBits = saBits; X.saiBits = saiBits; X.saMask = (1ull << saBits) - 1; X.saiMask = (1ull << saiBits) - 1;
    X.strandMask = ~(1ull << g.sbit); X.saiNbit = 1ull << (g.sbit + 1); X.saiAbsentBit = 1ull << (g.sbit + 2); X.saiNbases = g.P0; X.sparseD = 1;
    // the entries decoded; per entry the number of ACGT codes before the first other one, and whether it lies within P0 + 32 of a chromosome's edge or the genome's start
    g.pos.resize(g.nSA); g.fwd.resize(g.nSA); g.acgt.resize(g.nSA); g.edge.assign(g.nSA, 0); g.inv.assign(2 * g.n, ~0ull);
    for (u64 i = 0; i < g.nSA; i++) {
        const u64 v = packedGet(X.SA, i, saBits, X.saMask);
        g.fwd[i] = (v >> g.sbit) == 0; g.pos[i] = v & X.strandMask;
        g.inv[g.fwd[i] ? g.pos[i] : g.n + g.pos[i]] = i;
        u32 k = 0; while (k < ACGT_CAP && textAt(g, i, k) < 4) k++;
        g.acgt[i] = (u16)k;
        const u64 q = g.fwd[i] ? g.pos[i] : g.n - 1 - g.pos[i];             // genome coordinate of the suffix's first base
        for (size_t c = 0; c < g.cs.size(); c++) if (q >= g.cs[c] && q < g.cs[c] + g.cl[c]) g.edge[i] = g.fwd[i] ? (q + g.P0 + 32 > g.cs[c] + g.cl[c]) : (q < g.cs[c] + g.P0 + 32);
    }
    if (g.cls != 0)                                           // guard on the check's own input: suffix order by direct comparison (padding met in both at the same offset: text position decides)
        for (u64 i = 1; i < g.nSA; i++) {
            u32 k = 0; u8 a, b;
            for (;; k++) { a = textAt(g, i - 1, k); b = textAt(g, i, k); if (a != b || a == 5) break; }
            const u64 ta = g.fwd[i - 1] ? g.pos[i - 1] : g.n + g.pos[i - 1], tb = g.fwd[i] ? g.pos[i] : g.n + g.pos[i];
            if (!(a < b || (a == b && ta < tb))) { if (orderBad++ < 5) printf("SUFFIX ORDER entry %llu: code %u then %u at offset %u\n", (unsigned long long)i, a, b, k); }
        }
    // key records: k_sak_build through the emulator's launch over the whole array, against a base-by-base construction
    g.sak.assign(g.nSA + 1, SakRec{0, 0});
    { const DevIndex *Xp = &g.X; u64 *out_ = (u64 *)g.sak.data(); const u64 n1 = g.nSA;                  // (the launch copies what it names)
      hipLaunchKernelGGL(k_sak_build, dim3(std::min<u32>(64, (u32)((n1 + 255) / 256))), dim3(256), 0, 0, Xp, out_, (u64)0, n1); }
    for (u64 i = 0; i < g.nSA; i++) {
        const SakRec r = g.sak[i];
        u32 klen = 32; bool bad = false;
        for (u32 j = 0; j < 32; j++) { const u8 c = textAt(g, i, g.P0 + j); if (c > 3) { klen = j; break; } if (((r.key >> (2 * j)) & 3) != c) bad = true; }       // (the bits behind klen are read by nobody)
        bad |= (r.w0 & X.saMask) != packedGet(X.SA, i, saBits, X.saMask) || (u32)(r.w0 >> 58) != klen || ((r.w0 >> saBits) & ((1ull << (58 - saBits)) - 1)) != 0;
        if (bad && sakDiffs++ < 8) printf("SAK DIFF entry %llu (%s %llu): w0 %016llx key %016llx, klen wanted %u\n", (unsigned long long)i, g.fwd[i] ? "+" : "-", (unsigned long long)g.pos[i], (unsigned long long)r.w0, (unsigned long long)r.key, klen);
        sakRecords++; sakShortKlen += klen < 32;
        if (!g.fwd[i] && g.n - 1 - g.pos[i] < g.P0 + 32) sakRevNearStart++;
        if (g.edge[i]) sakNearPad++;
    }
    g.X.SAK = g.sak.data(); g.X.sakBases = g.P0;
    g.X0 = g.X; g.X0.SAK = nullptr; g.X0.sakBases = 0;
    staramd_genome sg; memset(&sg, 0, sizeof(sg)); staramd_params sp; memset(&sp, 0, sizeof(sp));
    sg.G = g.G; sg.nGenome = g.n; sg.SA = (const u8 *)g.SAw.data(); sg.nSA = g.nSA; sg.SAi = (const u8 *)g.SAiw.data(); sg.nSAi = g.nSAi; sg.GstrandBit = g.sbit; sg.gSAindexNbases = g.P0; sg.gSAsparseD = 1;
    for (int i = 0; i < 17; i++) sg.genomeSAindexStart[i] = out[5 + i];
    sp.seedMultimapNmax = 0xFFFFFFFFu; sp.seedPerReadNmax = 1000;
    g.O.init(&sg, &sp);
    g.wideAt = g.inv[0];
    if (g.wideAt != ~0ull) {
        g.wbit = 16; while ((1ull << g.wbit) <= g.n) g.wbit++;
        const u32 wb = g.wbit + 1; const u64 total = g.nSA + WIDE_EXTRA;
        g.wideWords = total * wb / 64 + 4; g.wideBytes = g.wideWords * 8;
        void *m = mmap(nullptr, g.wideBytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (m == MAP_FAILED) {            // strict overcommit, a limit on address space: nothing the engine did.  The wide trials are left out and the run says so
            if (!wideRefused++) printf("NOTE: %.1f GB of address space for the wide suffix array refused (%s): intervals of more than 2^32 entries are not tried\n", (double)g.wideBytes / 1e9, strerror(errno));
            return true;
        }
        g.wide = (u64 *)m;
        for (u64 i = 0; i < g.nSA; i++) packedPut(g.wide, i <= g.wideAt ? i : i + WIDE_EXTRA, wb, g.pos[i] | (g.fwd[i] ? 0ull : 1ull << g.wbit));
        g.wideHeadWords = ((g.wideAt + 1) * wb + 63) / 64; g.wideTailWord = (g.wideAt + 1 + WIDE_EXTRA) * wb / 64;
        g.XW = g.X0; g.XW.SA = g.wide; g.XW.SAi = nullptr; g.XW.nSA = total; g.XW.strandBit = g.wbit; g.XW.saBits = wb; g.XW.saMask = (1ull << wb) - 1; g.XW.strandMask = ~(1ull << g.wbit);
        sg.SA = (const u8 *)g.wide; sg.nSA = total; sg.SAi = nullptr; sg.nSAi = 0; sg.GstrandBit = g.wbit;
        g.OW.init(&sg, &sp);
    }
    return true;
}

// ---- a read: Lread codes with PADR bytes of anything either side (what lies behind a piece must not count); the oracle gets the same bytes
struct Read { std::vector<u8> b; u8 *R; u32 Lread; };
static void newRead(Read &r, u32 Lread) {
    r.Lread = Lread; r.b.resize(2 * PADR + Lread);
    for (auto &c : r.b) { const u32 x = rnd(16); c = x < 12 ? (u8)(x & 3) : x == 12 ? 4 : x == 13 ? 5 : x == 14 ? (u8)STARAMD_SPACER_BASE : (u8)rnd(4); }
    for (u32 i = 0; i < Lread; i++) r.b[PADR + i] = (u8)rnd(4);
    r.R = r.b.data() + PADR;
}
static void giveRead(Oracle &O, const Read &r) {
    O.R0.assign(r.b.begin(), r.b.end()); O.R1.resize(r.b.size());
    for (size_t i = 0; i < r.b.size(); i++) O.R1[i] = (char)compBase(r.b[i]);
    O.Read1[0] = O.R0.data() + PADR; O.Read1[1] = O.R1.data() + PADR; O.Read1[2] = nullptr; O.Lread = r.Lread;
}
// pc[k]: the piece in scan order as the suffix text sees it (already complemented for a backward scan)
static void layPiece(Read &r, const std::vector<u8> &pc, u32 &S, bool dirR) {
    const u32 n = (u32)pc.size();
    newRead(r, n + rnd(60));
    S = dirR ? rnd(r.Lread - n + 1) : n - 1 + rnd(r.Lread - n + 1);
    for (u32 k = 0; k < n; k++) { if (dirR) r.R[S + k] = pc[k]; else r.R[S - k] = compBase(pc[k]); }
}
static u32 matchLen(const Gen &g, u64 i, const std::vector<u8> &pc, u32 N) { u32 k = 0; while (k < N && pc[k] == textAt(g, i, k)) k++; return k; }

// ---- counters of the case classes (all classified from the reference side)
enum { K_DIFF_IN_KEY, K_END_IN_KEY, K_GENOME_N_IN_KEY, K_READ_N_IN_KEY, K_ALL32, K_L_BELOW, K_L_IN_KEY, K_L_BEHIND, K_N_LE_P0, K_REVERSE, K_EDGE, K_SHORT_BOUND,
       M_FULL_BREAK, M_RUN1, M_RUN_MANY, M_RUN_ALL, M_NOLESS_LEFT, M_NOLESS_RIGHT, M_FROM_LOOKUP, M_ONE_ENTRY, M_TWO_ENTRIES, M_WHOLE_ARRAY, M_U64, W_CASES, W_ACROSS, W_LEFT, W_RIGHT, W_WHOLE,
       S_KIND0, S_KIND1, S_KIND2, S_KIND3, S_SHORT_PIECE, S_HIGH_FWD, S_HIGH_BWD, S_OUTSIDE, S_SEARCHED, Q_PIECES, Q_SPACER, K_CLASSES };
static const char *CLASS_NAME[K_CLASSES] = {"first difference inside the key", "piece ends inside the key", "genome non-ACGT inside the key", "read non-ACGT inside the key", "all 32 key bases agree",
    "L < P0", "P0 <= L < P0+32", "L >= P0+32", "N <= P0", "reverse-strand entry", "entry within P0+32 of a chromosome edge / the genome start", "bound shorter than the key's piece",
    "full match ends the first bisection", "run length 1", "run length > 1", "run = whole interval", "haveLess false on the left", "haveLess false on the right", "interval from seedLookup",
    "interval of one entry", "interval of two entries", "whole array, L = 0", "searches run through mmpRunT<u64>", "intervals of more than 2^32 entries", "... run across the repeated entry", "... run left of it", "... run right of it", "... whole array",
    "lookup kind 0", "lookup kind 1", "lookup kind 2", "lookup kind 3", "piece shorter than the L-mers", "code > 3 in the prefix, forward", "code > 3 in the prefix, backward", "flat index outside the table",
    "lookups followed through the search", "pieces split", "reads with a mate spacer"};
static u64 nClass[K_CLASSES], nMod8[8];

struct Dump { bool on = false; std::vector<u8> reads; std::vector<SrcCmp> cmp; std::vector<SrcMmp> mmp, wide; std::vector<SrcLook> look;
    u32 addRead(const Read &r) { const u32 off = (u32)reads.size() + PADR; reads.insert(reads.end(), r.b.begin(), r.b.end()); while (reads.size() & 7) reads.push_back(5); return off; } };

static long bad = 0;
static u64 shareBy[3][3][3][2];      // index shape, interval from (lookup, chosen, whole array), genome class: dirty / clean
static u64 nCmp = 0, nMmp = 0, nMmpClean = 0, nBruteVsOracleDirty = 0, nBruteVsOracleClean = 0, nLook = 0, nSplit = 0;
#define FAIL(...) do { if (bad++ < 20) { printf(__VA_ARGS__); } } while (0)

// a piece cut from the suffix text of entry e: non-ACGT codes of the genome replaced (a piece holds none), then a base changed, the piece shortened, an N planted
static void cutPiece(const Gen &g, u64 e, std::vector<u8> &pc, u32 &N) {
    const u32 P0 = g.P0, where = rnd(10);
    const u32 Nq = where < 2 ? 1 + rnd(P0) : where < 6 ? P0 + 1 + rnd(31) : P0 + 32 + rnd(70);
    pc.resize(Nq);
    for (u32 k = 0; k < Nq; k++) { u8 c = textAt(g, e, k); pc[k] = c > 3 ? (g.cls == 2 ? (u8)(1 + rnd(2)) : (u8)rnd(4)) : c; }
    if (rnd(10) < 6) { const u32 w = rnd(4), m = w == 0 ? rnd(P0) : w == 3 ? P0 + 32 + rnd(40) : P0 + rnd(32); if (m < Nq) pc[m] = g.cls == 2 ? (u8)(3 - pc[m]) : (u8)((pc[m] + 1 + rnd(3)) & 3); }
    if (rnd(8) == 0) { const u32 j = rnd(3) ? P0 + rnd(32) : P0 + 32 + rnd(30); if (j < Nq) pc[j] = rnd(6) ? 4 : (u8)STARAMD_SPACER_BASE; }
    N = rnd(4) ? Nq : 1 + rnd(Nq);                            // the caller's bound: the piece, or shorter (runEnd compares up to Lmax with the key of the whole piece)
}

static void compareTrial(Gen &g, Dump &D) {
    const u32 P0 = g.P0;
    u64 e = rnd((u32)g.nSA);
    if (rnd(8) == 0) {                                          // an entry next to a chromosome's edge, either strand
        const u32 c = rnd((u32)g.cs.size()); const u64 off = rnd((u32)std::min<u64>(g.cl[c], P0 + 32)), q = rnd(2) ? g.cs[c] + off : g.cs[c] + g.cl[c] - 1 - off;
        const u64 i = g.inv[rnd(2) ? q : g.n + (g.n - 1 - q)]; if (i != ~0ull) e = i;
    }
    std::vector<u8> pc; u32 N, S; cutPiece(g, e, pc, N);
    const u32 Nq = (u32)pc.size();
    u64 iSA = e; if (rnd(5) < 2) { const i64 d = (i64)rnd(7) - 3; if ((i64)e + d >= 0 && (u64)((i64)e + d) < g.nSA) iSA = (u64)((i64)e + d); }       // a neighbour: ties in repeats
    const bool dirR = rnd(2);
    Read r; layPiece(r, pc, S, dirR); giveRead(g.O, r);
    const u32 m = matchLen(g, iSA, pc, N);
    const u32 lw = rnd(5), L = std::min(m, lw == 0 ? 0u : lw == 1 ? rnd(P0 + 1) : lw == 2 ? P0 + rnd(32) : lw == 3 ? P0 + 32 + rnd(20) : m);    // the reference's callers pass a length both are known to share
    bool cO = false, cK = false, c0 = false;
    const u64 lO = g.O.compareSeqToGenome(S, N, L, iSA, dirR, cO);
    SeedCnt cn = {0, 0, 0};
    const QKey qk = makeQKey(g.X, r.R, S, Nq, dirR), q0 = makeQKey(g.X0, r.R, S, Nq, dirR);
    const u32 lK = compareSeqToGenome(g.X, r.R, S, N, L, iSA, dirR, cK, cn, qk), l0 = compareSeqToGenome(g.X0, r.R, S, N, L, iSA, dirR, c0, cn, q0);
    nCmp++;
    if (lO != m) FAIL("ORACLE compare against the scan: %llu / %u\n", (unsigned long long)lO, m);
    if (lK != lO || l0 != lO || (lO < N && (cK != cO || c0 != cO)))
        FAIL("COMPARE DIFF P0 %u entry %llu (%s) S %u N %u Nq %u L %u dirR %d: oracle %llu/%d keys %u/%d no keys %u/%d\n", P0, (unsigned long long)iSA, g.fwd[iSA] ? "+" : "-", S, N, Nq, L, (int)dirR, (unsigned long long)lO, (int)cO, lK, (int)cK, l0, (int)c0);
    // classes
    u32 rn = Nq; for (u32 k = 0; k < Nq; k++) if (pc[k] > 3) { rn = k; break; }
    const u32 gn = g.acgt[iSA];
    if (L >= P0 && L < P0 + 32 && N > P0) {                     // (the calls the key decides or hands on)
        if (m < N && m >= P0 && m < P0 + 32 && m < gn && m < rn) nClass[K_DIFF_IN_KEY]++;
        if (m == N && N < P0 + 32) nClass[K_END_IN_KEY]++;
        if (m == gn && gn >= P0 && gn < P0 + 32 && m < N) nClass[K_GENOME_N_IN_KEY]++;
        if (rn >= P0 && rn < P0 + 32 && rn < N && m >= rn) nClass[K_READ_N_IN_KEY]++;
        if (m >= P0 + 32 && N > P0 + 32) nClass[K_ALL32]++;
        if (N < Nq) nClass[K_SHORT_BOUND]++;
    }
    nClass[L < P0 ? K_L_BELOW : L < P0 + 32 ? K_L_IN_KEY : K_L_BEHIND]++;
    if (N <= P0) nClass[K_N_LE_P0]++;
    if (!g.fwd[iSA]) nClass[K_REVERSE]++;
    if (g.edge[iSA]) nClass[K_EDGE]++;
    if (D.on) { SrcCmp c; c.iSA = iSA; c.rOff = D.addRead(r); c.S = S; c.N = N; c.Nq = Nq; c.L = L; c.dirR = dirR; c.expLen = (u32)lO; c.expComp = lO < N ? (u32)cO : 2u; D.cmp.push_back(c); }
}

static void mmpTrial(Gen &g, Dump &D) {
    const u64 e = rnd((u32)g.nSA);
    std::vector<u8> pc; u32 N, S; cutPiece(g, e, pc, N); pc.resize(N);                 // (here the piece is what the search is given)
    const bool dirR = rnd(2);
    Read r; layPiece(r, pc, S, dirR); giveRead(g.O, r);
    SeedCnt cn = {0, 0, 0};
    u64 first = 0, last = g.nSA - 1; u32 L0 = 0; int how = -1;
    const u32 w = rnd(100);
    if (w < 35) {               // (an interval from the lookup is seldom clean here: with most L-mers absent the entry behind is absent too, and the interval runs to the end of the array)
        const SeedLook k = seedLookup(g.X, r.R, S, N, dirR, cn);
        bool high = false; for (u32 j = 0; j < std::min(N, g.P0); j++) high |= pc[j] > 3;
        if (k.kind != 0 && !high) { first = k.i1; last = k.i2; L0 = k.maxL; how = M_FROM_LOOKUP; }
    }
    if (how < 0 && w < 97) {
        const u64 c = rnd(4) ? e : rnd((u32)g.nSA); const u32 sz = rnd(3);
        const u64 a = sz == 0 ? rnd(3) : sz == 1 ? rnd(40) : rnd(300), b = sz == 0 ? rnd(3) : sz == 1 ? rnd(40) : rnd(300);
        first = c > a ? c - a : 0; last = std::min(g.nSA - 1, c + b);
        how = last == first ? M_ONE_ENTRY : last == first + 1 ? M_TWO_ENTRIES : -2;
    }
    if (how == -1) how = M_WHOLE_ARRAY;
    if (how >= 0) nClass[how]++;
    // the oracle
    u64 Lo = L0, indO[2] = {0, 0};
    const u64 nO = g.O.maxMappableLength(S, N, first, last, dirR, Lo, indO);
    // brute force: the match length of the piece against every entry of the interval, its maximum and the run that reaches it
    u32 Lb = 0; u64 b0 = first, b1 = first;
    for (u64 i = first; i <= last; i++) { const u32 ml = matchLen(g, i, pc, N); if (ml > Lb) { Lb = ml; b0 = b1 = i; } else if (ml == Lb) b1 = i; }
    bool clean = true; for (u64 i = first; i <= last && clean; i++) clean = g.acgt[i] >= Lb + 1;
    const bool agree = Lb == Lo && b0 == indO[0] && b1 == indO[1];
    nMmp++; nMmpClean += clean;
    { const int hk = how == M_FROM_LOOKUP ? 0 : how == M_WHOLE_ARRAY ? 2 : 1; shareBy[g.P0 == 4 ? 0 : g.P0 == 8 ? 1 : 2][hk][g.cls][clean]++; }
    if (!agree) { if (clean) { nBruteVsOracleClean++; FAIL("ORACLE against brute force on a clean case: [%llu, %llu] N %u L0 %u: oracle L %llu [%llu, %llu], scan L %u [%llu, %llu]\n", (unsigned long long)first, (unsigned long long)last, N, L0,
                                      (unsigned long long)Lo, (unsigned long long)indO[0], (unsigned long long)indO[1], Lb, (unsigned long long)b0, (unsigned long long)b1); } else nBruteVsOracleDirty++; }
    // the engine: both index types, with and without keys
    for (int v = 0; v < 4; v++) {
        const DevIndex &X = (v & 1) ? g.X0 : g.X;
        const QKey qk = makeQKey(X, r.R, S, N, dirR);
        u32 L = L0; u64 i0 = ~0ull, i1 = ~0ull;
        const u64 nr = (v & 2) ? mmpRunT<u64>(X, r.R, S, N, first, last, dirR, L, i0, i1, cn, qk) : mmpRunT<u32>(X, r.R, S, N, first, last, dirR, L, i0, i1, cn, qk);
        if (v & 2) nClass[M_U64]++;
        if (L != Lo || i0 != indO[0] || i1 != indO[1] || nr != nO)
            FAIL("MMP DIFF %s %s P0 %u [%llu, %llu] S %u N %u L0 %u dirR %d clean %d: oracle L %llu [%llu, %llu] x%llu, engine L %u [%llu, %llu] x%llu\n", (v & 2) ? "u64" : "u32", (v & 1) ? "no keys" : "keys", g.P0, (unsigned long long)first, (unsigned long long)last,
                 S, N, L0, (int)dirR, (int)clean, (unsigned long long)Lo, (unsigned long long)indO[0], (unsigned long long)indO[1], (unsigned long long)nO, L, (unsigned long long)i0, (unsigned long long)i1, (unsigned long long)nr);
    }
    if (agree) {
        if (Lo == N && last > first + 1 && std::max(b0, first + 1) <= std::min(b1, last - 1)) nClass[M_FULL_BREAK]++;      // an entry strictly inside matches all of the piece: only the loop's break can have found it
        nClass[nO == 1 ? M_RUN1 : M_RUN_MANY]++;
        if (indO[0] == first && indO[1] == last && last > first) nClass[M_RUN_ALL]++;
        if (indO[0] == first && indO[1] < last) nClass[M_NOLESS_LEFT]++;
        if (indO[1] == last && indO[0] > first) nClass[M_NOLESS_RIGHT]++;
    }
    if (D.on) { SrcMmp c; c.first = first; c.last = last; c.exp0 = indO[0]; c.exp1 = indO[1]; c.expNrep = nO; c.rOff = D.addRead(r); c.S = S; c.N = N; c.L = L0; c.dirR = dirR; c.expL = (u32)Lo; D.mmp.push_back(c); }
}

// an interval of more than 2^32 entries: mmpRun's own choice of mmpRunT<u64> and mmpRunT<u64> itself against the oracle on the same array, and the oracle there against the
// scan of the plain array with its indices moved behind the copies (clean cases)
static void wideTrial(Gen &g, Dump &D) {
    if (!g.wide) return;
    const u64 r0 = g.wideAt, W = WIDE_EXTRA;
    const u64 e = rnd(3) ? (u64)std::min<i64>((i64)g.nSA - 1, std::max<i64>(0, (i64)r0 + (i64)rnd(41) - 20)) : rnd((u32)g.nSA);
    std::vector<u8> pc; u32 N, S; cutPiece(g, e, pc, N); pc.resize(N);
    const bool dirR = rnd(2);
    Read r; layPiece(r, pc, S, dirR); giveRead(g.O, r); giveRead(g.OW, r);
    const u32 sz = rnd(5);
    const u64 a = sz == 0 ? 0 : r0 - std::min<u64>(r0, sz == 1 ? rnd(3) : rnd(400)), b = sz == 0 ? g.nSA - 1 : std::min(g.nSA - 1, r0 + (sz == 1 ? rnd(3) : rnd(400)));
    u32 Lb = 0; u64 b0 = a, b1 = a;
    for (u64 i = a; i <= b; i++) { const u32 ml = matchLen(g, i, pc, N); if (ml > Lb) { Lb = ml; b0 = b1 = i; } else if (ml == Lb) b1 = i; }
    bool clean = true; for (u64 i = a; i <= b && clean; i++) clean = g.acgt[i] >= Lb + 1;
    const u64 w0 = b0 <= r0 ? b0 : b0 + W, w1 = b1 >= r0 ? b1 + W : b1;
    u64 Lo = 0, indO[2] = {0, 0};
    const u64 nO = g.OW.maxMappableLength(S, N, a, b + W, dirR, Lo, indO);
    nClass[W_CASES]++; if (sz == 0) nClass[W_WHOLE]++;
    if (clean && (Lo != Lb || indO[0] != w0 || indO[1] != w1)) FAIL("ORACLE on the wide array against the scan: L %llu [%llu, %llu], scan L %u [%llu, %llu]\n", (unsigned long long)Lo, (unsigned long long)indO[0], (unsigned long long)indO[1], Lb, (unsigned long long)w0, (unsigned long long)w1);
    SeedCnt cn = {0, 0, 0}; const QKey qk = makeQKey(g.XW, r.R, S, N, dirR);
    for (int v = 0; v < 2; v++) {
        u32 L = 0; u64 i0 = ~0ull, i1 = ~0ull;
        const u64 nr = v ? mmpRunT<u64>(g.XW, r.R, S, N, a, b + W, dirR, L, i0, i1, cn, qk) : mmpRun(g.XW, r.R, S, N, a, b + W, dirR, L, i0, i1, cn, qk);
        if (L != Lo || i0 != indO[0] || i1 != indO[1] || nr != nO)
            FAIL("WIDE MMP DIFF %s [%llu, %llu] N %u dirR %d clean %d: oracle L %llu [%llu, %llu] x%llu, engine L %u [%llu, %llu] x%llu\n", v ? "mmpRunT<u64>" : "mmpRun", (unsigned long long)a, (unsigned long long)(b + W), N, (int)dirR, (int)clean,
                 (unsigned long long)Lo, (unsigned long long)indO[0], (unsigned long long)indO[1], (unsigned long long)nO, L, (unsigned long long)i0, (unsigned long long)i1, (unsigned long long)nr);
    }
    if (indO[0] <= r0 && indO[1] >= r0 + W) nClass[W_ACROSS]++; else if (indO[1] < r0) nClass[W_LEFT]++; else if (indO[0] > r0 + W) nClass[W_RIGHT]++;
    if (D.on) { SrcMmp c; c.first = a; c.last = b + W; c.exp0 = indO[0]; c.exp1 = indO[1]; c.expNrep = nO; c.rOff = D.addRead(r); c.S = S; c.N = N; c.L = 0; c.dirR = dirR; c.expL = (u32)Lo; D.wide.push_back(c); }
}

// ReadAlign_maxMappableLength2strands.cpp:23-84 up to the interval, base by base on the oracle's arrays (the oracle has it inside maxMappableLength2strands, which goes on into the
// search: lookupTrial below follows that too).  A flat index outside the table: absent -- the reference reads whatever lies there, the engine's rule is the one restated here
struct RefLook { u64 i1, i2; u32 maxL, kind; bool outside; };
static RefLook refLookup(Oracle &O, u64 pieceStart, u64 pieceLength, bool dirR) {
    RefLook k = {0, 0, 0, 0, false};
    const staramd_genome &sg = O.g;
    const u64 Lmax = std::min<u64>(sg.gSAindexNbases, pieceLength);
    u64 ind1 = 0;
    for (u64 ii = 0; ii < Lmax; ii++) { ind1 <<= 2; if (dirR) ind1 += (u64)O.Read1[0][pieceStart + ii]; else ind1 += 3 - (u64)O.Read1[0][pieceStart - ii]; }
    u64 Lind = Lmax, iSA1 = 0, iSA2;
    while (Lind > 0) {
        const u64 flat = sg.genomeSAindexStart[Lind - 1] + ind1;
        if (flat >= sg.nSAi) { k.outside = true; --Lind; ind1 >>= 2; continue; }
        iSA1 = O.SAiAt(flat);
        if ((iSA1 & O.SAiMarkAbsentMaskC) == 0) break;
        --Lind; ind1 >>= 2;
    }
    if (Lind == 0) return k;
    bool iSA2good = true;
    if (sg.genomeSAindexStart[Lind - 1] + ind1 + 1 < sg.genomeSAindexStart[Lind]) {
        iSA2 = O.SAiAt(sg.genomeSAindexStart[Lind - 1] + ind1 + 1);
        if ((iSA2 & O.SAiMarkAbsentMaskC) == 0) iSA2 = (iSA2 & O.SAiMarkNmask) - 1; else { iSA2 = sg.nSA - 1; iSA2good = false; }
    } else { iSA2 = sg.nSA - 1; iSA2good = false; }
    const bool iSA1noN = (iSA1 & O.SAiMarkNmaskC) == 0;
    if (Lind < sg.gSAindexNbases && iSA1noN && iSA2good) { k.i1 = iSA1; k.i2 = iSA2; k.maxL = (u32)Lind; k.kind = 1; }
    else if (iSA1 == iSA2 && iSA1noN && iSA2good) { k.i1 = k.i2 = iSA1; k.maxL = (u32)Lind; k.kind = 2; }
    else { k.i1 = iSA1 & O.SAiMarkNmask; k.i2 = iSA2; k.maxL = (iSA2good && iSA1noN) ? (u32)Lind : 0; k.kind = 3; }
    return k;
}

static void lookupTrial(Gen &g, Dump &D) {
    const u32 P0 = g.P0;
    Read r; newRead(r, 40 + rnd(60));
    if (g.cls == 2 && rnd(2)) for (u32 i = 0; i < r.Lread; i++) r.R[i] = (u8)(1 + rnd(2));
    const bool dirR = rnd(2);
    const u32 len = rnd(3) == 0 ? 1 + rnd(P0) : 1 + rnd(30);
    const u32 S = dirR ? rnd(r.Lread - len + 1) : len - 1 + rnd(r.Lread - len + 1);
    if (rnd(2)) { const u64 e = rnd((u32)g.nSA); for (u32 k = 0; k < len; k++) { const u8 c = textAt(g, e, k); if (c > 3) break; if (dirR) r.R[S + k] = c; else r.R[S - k] = compBase(c); } }      // a prefix the genome has
    bool high = false;
    if (rnd(5) == 0) { const u32 j = rnd(std::min(len, P0)), code = rnd(3) ? 4 : rnd(2) ? 5 : STARAMD_SPACER_BASE; r.R[dirR ? S + j : S - j] = (u8)code; }      // a code above 3 inside the prefix: carries and borrows
    for (u32 j = 0; j < std::min(len, P0); j++) high |= r.R[dirR ? S + j : S - j] > 3;
    giveRead(g.O, r);
    SeedCnt cn = {0, 0, 0};
    const SeedLook k = seedLookup(g.X, r.R, S, len, dirR, cn);
    const RefLook w = refLookup(g.O, S, len, dirR);
    nLook++;
    if (k.i1 != w.i1 || k.i2 != w.i2 || k.maxL != w.maxL || k.kind != w.kind)
        FAIL("LOOKUP DIFF P0 %u S %u len %u dirR %d high %d: want kind %u [%llu, %llu] maxL %u, engine kind %u [%llu, %llu] maxL %u\n", P0, S, len, (int)dirR, (int)high, w.kind, (unsigned long long)w.i1, (unsigned long long)w.i2, w.maxL,
             k.kind, (unsigned long long)k.i1, (unsigned long long)k.i2, k.maxL);
    nClass[S_KIND0 + w.kind]++;
    if (len < P0) nClass[S_SHORT_PIECE]++;
    if (high) nClass[dirR ? S_HIGH_FWD : S_HIGH_BWD]++;
    if (w.outside) nClass[S_OUTSIDE]++;
    if (!high) {             // the whole of one start offset against the oracle's maxMappableLength2strands (with a code above 3 in the prefix the reference's interval may lie anywhere: not followed)
        u64 Nrep = 0, i0 = 0; u32 maxL = 0;
        searchOneDist(g.X, r.R, S, len, dirR, 0, Nrep, i0, maxL, cn);
        g.O.PC.clear(); g.O.nA = 0; g.O.nUM[0] = g.O.nUM[1] = 0; g.O.multNmin = g.O.multNminL = 0; g.O.fatalSeeds = false;
        u64 best = 0; g.O.maxMappableLength2strands(S, len, dirR ? 0 : 1, 0, 0, best, 0);
        nClass[S_SEARCHED]++;
        const bool same = Nrep == 0 ? g.O.PC.empty() : (g.O.PC.size() == 1 && g.O.PC[0].nrep == Nrep && g.O.PC[0].L == maxL && g.O.PC[0].saStart == i0 && best == maxL);
        if (!same) FAIL("SEARCH DIFF P0 %u S %u len %u dirR %d: engine x%llu L %u from %llu, oracle %zu rows x%llu L %llu from %llu\n", P0, S, len, (int)dirR, (unsigned long long)Nrep, maxL, (unsigned long long)i0, g.O.PC.size(),
                        g.O.PC.empty() ? 0ull : (unsigned long long)g.O.PC[0].nrep, g.O.PC.empty() ? 0ull : (unsigned long long)g.O.PC[0].L, g.O.PC.empty() ? 0ull : (unsigned long long)g.O.PC[0].saStart);
    }
    if (D.on) { SrcLook c; c.exp1 = w.i1; c.exp2 = w.i2; c.rOff = D.addRead(r); c.S = S; c.len = len; c.dirR = dirR; c.expMaxL = w.maxL; c.expKind = w.kind; D.look.push_back(c); }
}

// nextPiece against qualitySplit (SequenceFuns.cpp:411-444) base by base: every run of codes <= 3, the mate spacers passed before it
static void splitTrial() {
    Read r; newRead(r, 1 + rnd(120));
    bool spacer = false;
    for (u32 k = 0, nk = rnd(8); k < nk; k++) { const u32 p = rnd(r.Lread), len = rnd(4) ? 1 : 1 + rnd(12); for (u32 i = p; i < p + len && i < r.Lread; i++) { r.R[i] = 4; nMod8[i & 7]++; } }
    if (rnd(2)) { const u32 p = rnd(r.Lread); r.R[p] = STARAMD_SPACER_BASE; nMod8[p & 7]++; spacer = true; }
    if (rnd(16) == 0) for (u32 i = 0; i < r.Lread; i++) r.R[i] = 4;
    u32 iR = 0, iFrag = 0, pS = 0, pL = 0, jR = 0, jFrag = 0;
    for (;;) {
        const bool have = nextPiece(r.R, r.Lread, iR, iFrag, pS, pL);
        while (jR < r.Lread && r.R[jR] > 3) { if (r.R[jR] == STARAMD_SPACER_BASE) jFrag++; jR++; }
        const u32 j1 = jR; while (jR < r.Lread && r.R[jR] <= 3) jR++;
        const bool want = j1 < r.Lread;
        if (have != want || (have && (pS != j1 || pL != jR - j1 || iFrag != jFrag || iR != jR))) { FAIL("SPLIT DIFF Lread %u: piece %u+%u frag %u (%d), base by base %u+%u frag %u (%d)\n", r.Lread, pS, pL, iFrag, (int)have, j1, jR - j1, jFrag, (int)want); break; }
        if (!have) break;
        nClass[Q_PIECES]++;
    }
    nSplit++; nClass[Q_SPACER] += spacer;
}

template <class T> static void put(FILE *f, const T *p, size_t n) { if (n && fwrite(p, sizeof(T), n, f) != n) { perror("seed_routines_check: write"); exit(2); } }

// a genome's trials take a fraction of a second; a search that never ends (a routine that contradicts itself can bisect for ever) is reported, not waited for
static void onAlarm(int) { static const char msg[] = "\na search does not end: 1 differences\n"; (void)!write(1, msg, sizeof(msg) - 1); _exit(1); }

int main(int argc, char **argv) {
    signal(SIGALRM, onAlarm);
    long trials = 120000; const char *dumpPath = nullptr;
    for (int a = 1; a < argc; a++) { if (!strcmp(argv[a], "--dump") && a + 1 < argc) dumpPath = argv[++a]; else trials = atol(argv[a]); }
    const long perGenome = 4000;
    FILE *df = nullptr;
    if (dumpPath) { df = fopen(dumpPath, "wb"); if (!df) { perror(dumpPath); return 2; } const u64 head[2] = {SRC_MAGIC, 3}; put(df, head, 2); trials = 3 * perGenome; }
    long done = 0, nGenomes = 0, refused = 0; bool wideDumped = false;
    for (u32 gi = 0; done < trials; gi++) {
        Gen *gp = new Gen(); Gen &g = *gp;
        fflush(stdout); alarm(60);
        makeGenome(g, gi % 8 == 7 ? 2 : (gi % 8) % 2);                // of 8 genomes: 4 with N, 3 with no non-ACGT code but the padding, 1 of two letters (lookup kind 0)
        if (!buildIndex(g, (u32)(nGenomes % 3))) { refused++; delete gp; if (refused > 1000) { printf("the index twin refuses every genome\n"); return 1; } continue; }
        nGenomes++;
        Dump D; D.on = df != nullptr;
        for (long t = 0; t < perGenome; t++, done++) {
            const u32 k = rnd(10);
            if (k < 4) compareTrial(g, D); else if (k < 8) mmpTrial(g, D); else if (k < 9) lookupTrial(g, D); else splitTrial();
            if (k >= 4 && k < 8 && rnd(4) == 0) lookupTrial(g, D);
            if (rnd(16) == 0) wideTrial(g, D);
        }
        if (df) {
            SrcSet s; memset(&s, 0, sizeof(s));
            s.nGenome = g.n; s.nSA = g.nSA; s.strandBit = g.sbit; s.saiNbases = g.P0; for (int i = 0; i < 17; i++) s.saiStart[i] = g.X.saiStart[i];
            s.gBytes = g.gbuf.size(); s.saWords = g.SAw.size(); s.saiWords = g.SAiw.size(); s.readBytes = D.reads.size(); s.nCmp = D.cmp.size(); s.nMmp = D.mmp.size(); s.nLook = D.look.size();
            s.nWide = (g.wide && !wideDumped) ? D.wide.size() : 0; if (s.nWide) wideDumped = true;          // (one set: the harness needs 9 GB of device memory for it)
            s.wideBit = g.wbit; s.wideExtra = WIDE_EXTRA; s.wideHeadWords = g.wideHeadWords; s.wideTailWord = g.wideTailWord; s.wideWords = g.wideWords;
            put(df, &s, 1); put(df, g.gbuf.data(), g.gbuf.size()); put(df, g.SAw.data(), g.SAw.size()); put(df, g.SAiw.data(), g.SAiw.size()); put(df, g.sak.data(), (size_t)g.nSA);
            put(df, D.reads.data(), D.reads.size()); put(df, D.cmp.data(), D.cmp.size()); put(df, D.mmp.data(), D.mmp.size()); put(df, D.look.data(), D.look.size());
            if (s.nWide) { put(df, g.wide, g.wideHeadWords); put(df, g.wide + g.wideTailWord, g.wideWords - g.wideTailWord); put(df, D.wide.data(), D.wide.size()); }
        }
        delete gp;
    }
    if (df && fclose(df)) { perror(dumpPath); return 2; }
    printf("%ld genomes (%ld refused by the index twin); key records: %llu, %llu short of 32 bases, %llu next to a chromosome's edge, %llu reverse-strand within P0 + 32 of the genome's start: %ld differences; suffix order: %ld out of place\n",
           nGenomes, refused, (unsigned long long)sakRecords, (unsigned long long)sakShortKlen, (unsigned long long)sakNearPad, (unsigned long long)sakRevNearStart, sakDiffs, orderBad);
    long empty = 0;
    for (int c = 0; c < K_CLASSES; c++) {
        if (wideRefused && c >= W_CASES && c <= W_WHOLE) { printf("  %-72s not tried\n", CLASS_NAME[c]); continue; }       // (only where the mapping was refused: see the note above)
        printf("  %-72s %llu\n", CLASS_NAME[c], (unsigned long long)nClass[c]); if (!nClass[c]) empty++;
    }
    printf("  N / spacer positions modulo 8:"); for (int k = 0; k < 8; k++) { printf(" %llu", (unsigned long long)nMod8[k]); if (!nMod8[k]) empty++; } printf("\n");
    if (!sakShortKlen || !sakNearPad || !sakRevNearStart) empty++;
    const double share = nMmp ? (double)nMmpClean / (double)nMmp : 0.0;
    printf("brute force against the oracle: %llu disagreements on clean cases (failures), %llu on the others (no total order there: not failures)\n", (unsigned long long)nBruteVsOracleClean, (unsigned long long)nBruteVsOracleDirty);
    for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) { printf("  clean / all, saiNbases %u, interval %s, genomes with N / without / two letters:", SHAPES[a][0], b == 0 ? "from the lookup" : b == 1 ? "chosen" : "whole array");
        for (int c = 0; c < 3; c++) printf(" %llu/%llu", (unsigned long long)shareBy[a][b][c][1], (unsigned long long)(shareBy[a][b][c][0] + shareBy[a][b][c][1])); printf("\n"); }
    printf("clean share %.4f\n", share);
    if (!dumpPath && share < 0.5) { printf("fewer than half of the search cases are clean\n"); bad++; }
    if (!dumpPath && empty) { printf("%ld case classes never occurred\n", empty); bad += empty; }
    bad += sakDiffs + orderBad;
    printf("%llu compares, %llu searches x 4, %llu lookups, %llu reads split: %ld differences\n", (unsigned long long)nCmp, (unsigned long long)nMmp, (unsigned long long)nLook, (unsigned long long)nSplit, bad);
    return bad ? 1 : 0;
}
