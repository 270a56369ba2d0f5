// window_routines_check.cpp -- TEST INFRASTRUCTURE: the routines of star_amd/csrc/engine/k_window.hip one at a time, and its kernels on batches made by hand, against the oracle
// (star_oracle.cpp, the line-by-line restatement pinned to the reference).  The kernel reads only SA[saStart .. saStart + nrep) of the index, so the check writes the packed array
// itself as lists of (strand, position) it chooses, with the seed tables, chrBin, the junction arrays and the parameter block; the same values go into the oracle's genome.
//   layer 1, each call one emulated wavefront of 64 lanes:
//     createExtendWindowsWithAlign<false> / <true>   against the oracle's, anchor by anchor: return value, nW, the limit flag and the live rows (dead = gStart > gEnd)
//     assignAlignToWindow<false> / <true>            against the oracle's, seed by seed: the whole list (seven fields a row), nwa, lrec, tooMany, the overflow flag, nBlocks
//     sjAlignSplit                                   against the oracle's % and /, offsets around 2^32 included (sjdbOverhang 2^19)
//     ownInsert / ownLookup                          against "flank beats core, then the higher window" per key, over LDS words and over a buffer; tables never above 5/8
//     waveMax64, waveMin32, seedOfLane               against loops over 64 values
//   layer 2: k_windows (first and middle launch), k_windows_big, k_order_hist / _offsets / _scatter with the launch shapes of engine.hip, per read against buildWindows() of the
//     oracle (the first half of stitchPieces), plus structure: places in the pools disjoint and adding up to the cursors, every window reached from one work item, item classes,
//     the order array, pool overflow, guard bytes around every buffer.  The flank-and-cover block of the kernel (owner map / Bloom filter / ownerWave) is reached through this
//     layer alone: moved into a function of its own it compiled to different gfx950 code, so it stays where it is.
// The counters: DC_nWA is the oracle's.  DC_nSAenum and DC_nWindows are not the oracle's C_nSAenum / C_nWindows where a read stops early or travels: the kernel counts a chunk of
// 64 loci when it reads it, ends pass B at too many anchors (the oracle enumerates on), and a read that outgrows the table rows or the seed-list blocks of a launch is counted
// again by the next launch, with the rows it had.  The check traces the oracle's own calls (tracePassA / tracePassB) and derives from them what the launches of each geometry count
// (expectCounters); every batch without a read at the window limit is compared, the number of batches compared is printed and a run without a non-zero comparison fails.
// The window limit: when nW reaches alignWindowsPerReadNmax the reference keeps map bins that point at the overwritten last index, and the oracle's WA[iW] is then indexed outside
// its vector.  A sequence of layer 1 ends with the call that reaches the limit; a read of layer 2 that reaches it is compared in its status bit alone.  Everything below the limit
// is compared in full, and the run fails when fewer than 95 % of the reads are.
// Every case is classified from the reference side and its inputs; the class table is printed and a class that never occurred fails the run.
// usage: window_routines_check [scale] [--dump file]      scale: per cent of the full trial counts (100); --dump: three environments' worth of cases go to `file`
#include "k_window.hip"
#include "star_oracle.cpp"
#include "window_routines_cases.h"
#include <random>
#include <set>
#include <csignal>
#include <unistd.h>

static std::mt19937_64 rng(20250903);
static u32 rnd(u32 n) { return (u32)(rng() % n); }

enum { C_NEW, C_OWNED, C_MERGE_L, C_MERGE_R, C_MERGE_BOTH, C_OTHERCHR_L, C_OTHERCHR_R, C_AT_DIST, C_AT_DIST1, C_BIN0, C_BINLAST, C_OTHER_STRAND, C_ROWS_65, C_ROWS_129, C_MERGE_LATE_TRIP, C_LIMIT, C_TAB_LDS, C_TAB_GLOBAL,
       A_HIT_NOCHANGE, A_MOVE_LEFT, A_MOVE_RIGHT, A_INPLACE, A_DIAG_NOHIT, A_CLAUSE2, A_INS_0, A_INS_MID, A_INS_END, A_LIST_63, A_LIST_64, A_FULL_LREC, A_FULL_ANCHORS, A_COMPACT_1, A_COMPACT_MOST, A_COMPACT_INSERT,
       A_COMPACT_REJECT, A_REJECT_ENTRY, A_BLOCKS_OUT,
       S_TRUE, S_FALSE, S_64BIT, S_OFF_M1, S_OFF_0, S_OFF_P1, S_SJ1_OVH_M1, S_SJ1_OVH, S_END_OVH, S_END_OVH1,
       O_CHAIN_65, O_WRAP, O_SAME_KEY, O_ABSENT, O_KEY_TOP, O_LDS, O_GLOBAL, V_ALLZERO, V_MAX_LANE0, V_MAX_LANE63,
       R_SEEDS_1, R_SEEDS_17, R_SEEDS_64, R_SEEDS_65, R_SEEDS_130, R_UNIQ_SMALLCHR, R_UNIQ_BIGCHR, R_NREP_3, R_NREP_4, R_NREP_64, R_NREP_65, R_NREP_1000, R_FAM_OWNED, R_FAM_SPREAD, R_FAM_SPLIT, R_SHORTCUT_DROP, R_SHORTCUT_HALF, R_MM_BELOW, R_MM_ABOVE,
       R_MATES_ONE, R_MATES_APART, R_D0S0, R_D0S1, R_D1S0, R_D1S1, R_SPLIT_TWO_WIN, R_SPLIT_ONE_NONE, R_GT1024, R_LIMIT, R_TOOMANY, R_EMIT_1, R_EMIT_2, R_EMIT_3, R_EMIT_64, R_EMIT_LATE_ROWS, R_KILLED_WIDE_FLANK,
       R_FLANK_OVER_CORE, R_COVER_BELOW, R_COVER_ABOVE, R_BINS_MAP_LAST, R_BINS_MAP_OFF, B_SHORT_WIN, B_SHORT_WA, B_MID, B_NO_MID, B_TINY, B_MAP_OFF, B_COUNTERS, B_COUNTERS_REPEAT, B_COUNTERS_TOOMANY, N_CLASSES };
static const char *CLASS_NAME[N_CLASSES] = {
    "windows: a new window", "windows: bin inside a window", "windows: left merge", "windows: right merge", "windows: both, the right window killed", "windows: nearest left neighbour on another chromosome",
    "windows: nearest right neighbour on another chromosome", "windows: neighbour exactly winAnchorDistNbins away", "windows: neighbour one bin further", "windows: aBin = 0", "windows: aBin = winBinN - 1",
    "windows: the other strand has a window at the bin", "windows: more than 64 rows", "windows: more than 128 rows", "windows: merge with a window of a second or later trip", "windows: the call that reaches the limit",
    "windows: table in LDS", "windows: table in global memory",
    "list: overlap hit, not longer (no change)", "list: longer seed moved left", "list: longer seed moved right", "list: longer seed in place", "list: same diagonal, other sjA or iFrag (no hit)",
    "list: the second clause of the overlap test alone", "list: insert at rank 0", "list: insert in the middle", "list: insert at the end", "list: 63 rows", "list: 64 rows", "list: full, lrec from one short non-anchor",
    "list: full and all anchors", "list: compaction removes 1 row", "list: compaction removes all but at most 2 rows", "list: compaction, then insert", "list: compaction, then rejection", "list: non-anchor below lrec rejected at entry",
    "list: capBlocks exhausted",
    "split: split", "split: not split", "split: off >= 2^32 (64-bit divide)", "split: off = 2^32 - 1", "split: off = 2^32", "split: off = 2^32 + 1", "split: sj1 = overhang - 1", "split: sj1 = overhang", "split: sj1 + aLength = overhang",
    "split: sj1 + aLength = overhang + 1",
    "owner map: probe of more than 64 slots", "owner map: probe that wraps the table", "owner map: one key from several lanes at once", "owner map: absent key", "owner map: key 2^20 - 1", "owner map: LDS words", "owner map: buffer",
    "wave: all keys zero", "wave: maximum in lane 0", "wave: maximum in lane 63",
    "reads: 1 seed", "reads: 17 seeds", "reads: 64 seeds", "reads: 65 seeds", "reads: 130 seeds", "reads: all seeds of one locus, chromosomes below 0x3FFF", "reads: all seeds of one locus, chromosomes from 0x3FFF",
    "reads: a seed of 3 loci", "reads: of 4", "reads: of 64", "reads: of 65", "reads: of 1000", "reads: family mostly in an owned window", "reads: family spread over new bins", "reads: family with split loci", "reads: shortcut chunk (cnt >= 4, cnt * 16 >= nW) drops an owned locus", "reads: ... holds a split locus with one half owned",
    "reads: seed with nrep > winAnchorMultimapNmax", "reads: multi-locus seed with nrep <= winAnchorMultimapNmax", "reads: both mates in one window", "reads: mates in separate windows", "reads: locus dir 0 strand 0",
    "reads: locus dir 0 strand 1", "reads: locus dir 1 strand 0", "reads: locus dir 1 strand 1", "reads: split locus, halves in two windows", "reads: split locus, one half in no window", "reads: more than 1024 windows",
    "reads: at the window limit (status bit only)", "reads: too many anchors", "reads: window emitted with 1 row", "reads: with 2 rows", "reads: with 3 rows", "reads: with 64 rows", "reads: window with seeds behind table row 64",
    "reads: killed window, winFlankNbins > winAnchorDistNbins", "reads: extents of two windows overlap, winFlankNbins > winAnchorDistNbins", "reads: covered bins within 5/8 of the first launch's slots", "reads: covered bins above 5/8 of the slots",
    "reads: winBinN = 2^19 - 1 (owner map, largest key)", "reads: winBinN = 2^19 (no owner map)", "batches: winCap one short", "batches: waCap one short", "batches: middle launch", "batches: no middle launch",
    "batches: capW 2, capBlocks 2", "batches: owner map off", "batches: DC_nSAenum / DC_nWindows compared", "batches: ... with reads counted again after an overflow",
    "batches: ... with reads that stop at too many anchors"};
static u64 nClass[N_CLASSES];

// ---- environments ----------------------------------------------------------------------------------------------------------------------------------------------------
enum { K_NORMAL, K_BIN19M, K_BIN19, K_BIGOVH, K_WIDE };
struct Env {
    WrsEnv w; int kind; std::vector<u32> chrBin; std::vector<u64> sjD, sjA; std::vector<u64> sa; u64 nSA = 0; std::vector<u64> chrFirstBin;     // first bin of every chromosome, and the end
    Oracle *O = nullptr;
};
static std::vector<Env *> envs; static bool dumping = false;       // dumping: three environments must hold every class
static void packedPut(std::vector<u64> &words, u64 i, u32 bits, u64 v) { const u64 b = i * bits, w = b >> 6; const u32 sh = (u32)(b & 63); if (words.size() < w + 3) words.resize(w + 3, 0); words[w] |= v << sh; if (sh + bits > 64) words[w + 1] |= v >> (64 - sh); }
static u64 realBins(const Env &e) { return e.w.sjGstart >> e.w.P.winBinNbits; }

static Env *makeEnv(int kind, u32 ie) {
    Env *e = new Env(); e->kind = kind; WrsEnv &w = e->w; memset(&w, 0, sizeof(w)); staramd_params &P = w.P;
    P.readNmates = 2;
    static const u32 MM[5] = {0, 1, 3, 50, 200}, SPW[5] = {2, 5, 64, 64, 50}, WPR[8] = {10000, 10000, 10000, 10000, 10000, 50, 50, 4};
    const u32 pk = ie % 4;                             // 0: the engine's defaults; 1: 5 / 2; 2: flanks wider than the anchor distance; 3: anything
    P.winAnchorMultimapNmax = pk == 0 ? 50 : MM[rnd(5)]; P.seedPerWindowNmax = pk == 0 ? 50 : SPW[rnd(5)]; P.alignWindowsPerReadNmax = 10000; (void)WPR;              // (4 and 50 go to two environments below: the share of reads at the limit stays small)
    if (ie == 1) { P.alignWindowsPerReadNmax = 50; P.winAnchorMultimapNmax = 1; } if (ie == 3) { P.alignWindowsPerReadNmax = 4; P.winAnchorMultimapNmax = 3; } if (ie == 5 || ie == 7) { P.seedPerWindowNmax = 64; if (ie == 5) P.winAnchorMultimapNmax = 50; } if (pk == 2) { P.alignWindowsPerReadNmax = 10000; P.seedPerWindowNmax = ie == 2 ? (dumping ? 64 : 5) : 50; P.winAnchorMultimapNmax = 50; }          // (so that no run is without them)
    P.winAnchorDistNbins = pk == 0 ? 9 : pk == 1 ? 5 : pk == 2 ? 2 + rnd(3) : 1 + rnd(9); P.winFlankNbins = pk == 0 ? 4 : pk == 1 ? 2 : pk == 2 ? P.winAnchorDistNbins + 1 + rnd(8) : rnd(6);
    P.winBinNbits = 4 + rnd(5); P.winBinChrNbits = rnd(4);
    u32 nChr = 3 + rnd(7); u64 units = 0; std::vector<u32> chrUnits;
    if (kind == K_BIN19M || kind == K_BIN19) { P.winBinNbits = 0; P.winBinChrNbits = 10; nChr = 4; P.alignWindowsPerReadNmax = 10000; P.winAnchorMultimapNmax = 50; }
    if (kind == K_BIGOVH) { P.winBinNbits = 8; P.winBinChrNbits = 16; }          // (its chrBin stays small: the environment serves sjAlignSplit alone)
    if (kind == K_WIDE) { P.winBinNbits = 4; P.winBinChrNbits = 2; P.alignWindowsPerReadNmax = 10000; P.winAnchorMultimapNmax = 50; P.winAnchorDistNbins = 3; P.winFlankNbins = 1; P.seedPerWindowNmax = 50; }
    for (u32 c = 0; c < nChr; c++) { u32 u = kind == K_WIDE ? 2500 + rnd(500) : (rnd(4) == 0 ? 1 + rnd(3) : 20 + rnd(rnd(3) ? 200 : 3000)) ; if (kind == K_BIN19M || kind == K_BIN19) u = 128; chrUnits.push_back(u); units += u; }
    while (kind == K_NORMAL && ((units << P.winBinChrNbits) << P.winBinNbits) < 8000) { chrUnits[0] += 50; units += 50; }
    if (kind == K_BIN19M || kind == K_BIN19) { const u64 want = kind == K_BIN19M ? (1ull << 19) - 2 : (1ull << 19) - 1; w.nGenome = want; w.sjGstart = want; w.sjdbN = 0; w.sjdbOverhang = 100; w.sjdbLength = 201; }
    else if (kind == K_BIGOVH) { w.sjdbOverhang = 1u << 19; w.sjdbLength = (1u << 20) + 1; w.sjdbN = 4100; w.sjGstart = (units << P.winBinChrNbits) << P.winBinNbits; w.nGenome = w.sjGstart + (u64)w.sjdbN * w.sjdbLength; }
    else { w.sjdbOverhang = 100; w.sjdbLength = 201; w.sjdbN = 20 + rnd(60); w.sjGstart = (units << P.winBinChrNbits) << P.winBinNbits; w.nGenome = w.sjGstart + (u64)w.sjdbN * w.sjdbLength + rnd(50); }
    P.winBinN = (w.nGenome >> P.winBinNbits) + 1;
    w.strandBit = w.nGenome >= (1ull << 32) ? 33 : 32;
    const u32 bigChr = kind == K_NORMAL && (ie % 5 == 4 || (dumping && ie == 2)) ? 1 + rnd(2) : 0;                 // 1: chrBin carries numbers from 0x3FFF; 2: nChrReal itself is that large
    w.nChrReal = bigChr == 2 ? 0x3FFFu + rnd(100) : nChr;
    const u64 nCb = (P.winBinN >> P.winBinChrNbits) + 2; e->chrBin.assign(nCb, (bigChr == 1 ? 0x3FFFu : 0u) + nChr);
    u64 at = 0; for (u32 c = 0; c < nChr; c++) { e->chrFirstBin.push_back(at << P.winBinChrNbits); for (u32 k = 0; k < chrUnits[c] && at < nCb; k++) e->chrBin[at++] = (bigChr == 1 ? 0x3FFFu : 0u) + c; }
    e->chrFirstBin.push_back(std::min<u64>(at << P.winBinChrNbits, w.sjGstart >> P.winBinNbits));
    for (u32 k = 0; k < w.sjdbN; k++) { const u64 lim = w.sjGstart - 2 * (u64)w.sjdbOverhang - 300; const u64 d = w.sjdbOverhang + rng() % (lim - w.sjdbOverhang); e->sjD.push_back(d - w.sjdbOverhang + 0);
        const u32 how = rnd(3); e->sjA.push_back(how == 0 ? std::min<u64>(lim, d + 30 + rnd(200)) : how == 1 ? std::min<u64>(lim, d + ((u64)(1 + rnd(2 * P.winAnchorDistNbins + 2)) << P.winBinNbits)) : rng() % lim); }
    if (e->sjD.empty()) { e->sjD.push_back(0); e->sjA.push_back(0); }
    Oracle *O = new Oracle(); e->O = O;
    memset(&O->g, 0, sizeof(O->g)); O->P = P; O->g.nGenome = w.nGenome; O->g.GstrandBit = w.strandBit; O->g.chrBin = e->chrBin.data(); O->g.chrBinN = nCb; O->g.nChrReal = w.nChrReal;
    O->g.sjGstart = w.sjGstart; O->g.sjdbOverhang = w.sjdbOverhang; O->g.sjdbLength = w.sjdbLength; O->g.sjdbN = w.sjdbN; O->g.sjDstart = e->sjD.data(); O->g.sjAstart = e->sjA.data();
    O->saMask = (1ull << (w.strandBit + 1)) - 1; O->GstrandMask = ~(1ull << w.strandBit);
    if (kind != K_BIGOVH) { O->winBin[0].assign(P.winBinN + 1, 0xFFFF); O->winBin[1].assign(P.winBinN + 1, 0xFFFF); }
    memset(O->cnt, 0, sizeof(O->cnt));
    return e;
}
static u32 envToSet(WrsSet &S, Env *e) {          // (once the reads of the environment are made: its suffix array is complete)
    WrsEnv w = e->w; w.chrBinOff = (u32)S.chrBin.size(); w.chrBinN = (u32)e->chrBin.size(); w.sjOff = (u32)S.sjD.size(); w.saOff = S.sa.size(); e->sa.resize(e->sa.size() + 4, 0); w.saWords = e->sa.size();
    S.chrBin.insert(S.chrBin.end(), e->chrBin.begin(), e->chrBin.end()); S.sjD.insert(S.sjD.end(), e->sjD.begin(), e->sjD.end()); S.sjA.insert(S.sjA.end(), e->sjA.begin(), e->sjA.end()); S.sa.insert(S.sa.end(), e->sa.begin(), e->sa.end());
    S.env.push_back(w); return (u32)S.env.size() - 1;
}

// ---- layer 1: createExtendWindowsWithAlign --------------------------------------------------------------------------------------------------------------------------------
static u64 hashWC(const Oracle &O) {
    u64 h = WRS_HASH0;
    for (u64 j = 0; j < O.nW; j++) { const Win &c = O.WC[j]; if (c.gStart <= c.gEnd) { h = wrsMix(h, c.gStart); h = wrsMix(h, c.gEnd); h = wrsMix(h, c.chr); h = wrsMix(h, c.str); } else h = wrsMix(h, WRS_DEAD); }
    return h;
}
static void createCase(WrsSet &S, Env *e, u32 ie, bool big) {
    Oracle &O = *e->O; const staramd_params &P = O.P; const u64 nb = P.winBinN, dist = P.winAnchorDistNbins;
    std::fill(O.winBin[0].begin(), O.winBin[0].end(), 0xFFFF); std::fill(O.winBin[1].begin(), O.winBin[1].end(), 0xFFFF); O.nW = 0; O.WC.clear(); O.windowsLimit = false;
    WrsCreate c; c.env = ie; c.big = big; c.off = (u32)S.anchor.size(); c.n = 0;
    const u32 scatter = rnd(3) == 0 ? 66 + rnd(3) * 64 : rnd(12), n = scatter + 5 + rnd(40);       // scatter: windows made first (rows of a second and third trip)
    nClass[big ? C_TAB_GLOBAL : C_TAB_LDS]++;
    std::vector<std::pair<u64, u32>> made;           // (bin, strand) of earlier anchors
    for (u32 k = 0; k < n && O.nW < WRS_CAPW - 2; k++) {
        u64 bin; u32 str = rnd(2);
        const u32 how = k < scatter ? 0 : rnd(12);
        const auto recent = [&]() { return made[made.size() - 1 - rnd(std::min<u32>((u32)made.size(), 6))]; };
        if (how == 0 || made.empty()) bin = rng() % nb;
        else if (how <= 2) { const auto m = recent(); const u64 d = rnd(3) == 0 ? 1 + rnd((u32)dist + 3) : dist + rnd(2); bin = how == 1 ? (m.first > d ? m.first - d : 0) : std::min(nb - 1, m.first + d); str = m.second; }
        else if (how == 3) { const auto m = recent(); bin = std::min(nb - 1, m.first + dist + 1 + rnd((u32)dist + 1)); str = m.second; }          // a partner for a bridge
        else if (how == 4 && made.size() >= 2) { const auto a = made[made.size() - 1], b = made[made.size() - 2]; bin = (a.first + b.first) / 2; str = a.second; }     // between the last two
        else if (how == 5) bin = rnd(3) ? 0 : rnd(3);
        else if (how == 6) bin = nb - 1 - (rnd(3) ? 0 : rnd(3));
        else if (how == 7) { const auto m = recent(); bin = m.first; str = m.second ^ 1u; }
        else if (how == 8) { const auto m = recent(); bin = m.first; str = m.second; }
        else if (how == 9) { const u64 f = e->chrFirstBin[rnd((u32)e->chrFirstBin.size())]; bin = std::min(nb - 1, f + rnd(2 * (u32)dist + 2)); bin = bin > dist ? bin - dist : 0; }          // around a chromosome boundary
        else { const auto m = made[rnd((u32)made.size())]; bin = std::min(nb - 1, m.first + rnd(2 * (u32)dist + 4)); bin = bin > dist + 1 ? bin - dist - 1 : 0; str = m.second; }
        if (bin > nb - 1) bin = nb - 1;
        const u64 a1 = (bin << P.winBinNbits) + rnd(1u << P.winBinNbits);
        // classes, from the map before the call
        const uint16_t *wB = O.winBin[str].data(); const u32 chrA = e->chrBin[bin >> P.winBinChrNbits];
        if (wB[bin] != 0xFFFF) nClass[C_OWNED]++;
        else {
            i64 dl = -1, dr = -1; for (u64 d = 1; d <= dist + 1 && d <= bin; d++) if (wB[bin - d] != 0xFFFF) { dl = (i64)d; break; } for (u64 d = 1; d <= dist + 1 && bin + d < nb; d++) if (wB[bin + d] != 0xFFFF) { dr = (i64)d; break; }
            const bool ml = dl > 0 && dl <= (i64)dist && e->chrBin[(bin - dl) >> P.winBinChrNbits] == chrA, mr = dr > 0 && dr <= (i64)dist && e->chrBin[(bin + dr) >> P.winBinChrNbits] == chrA;
            if (dl > 0 && dl <= (i64)dist && !ml) nClass[C_OTHERCHR_L]++; if (dr > 0 && dr <= (i64)dist && !mr) nClass[C_OTHERCHR_R]++;
            if (dl == (i64)dist || dr == (i64)dist) nClass[C_AT_DIST]++; if ((dl == (i64)dist + 1 && dr < 0) || (dr == (i64)dist + 1 && dl < 0)) nClass[C_AT_DIST1]++;
            nClass[ml && mr ? C_MERGE_BOTH : ml ? C_MERGE_L : mr ? C_MERGE_R : C_NEW]++;
            if ((ml && wB[bin - dl] >= 64) || (!ml && mr && wB[bin + dr] >= 64)) nClass[C_MERGE_LATE_TRIP]++;
        }
        if (bin == 0) nClass[C_BIN0]++; if (bin == nb - 1) nClass[C_BINLAST]++; if (O.winBin[str ^ 1u][bin] != 0xFFFF) nClass[C_OTHER_STRAND]++;
        if (O.nW > 64) nClass[C_ROWS_65]++; if (O.nW > 128) nClass[C_ROWS_129]++;
        const int r = O.createExtendWindowsWithAlign(a1, str);
        WrsAnchor a; a.a1 = a1; a.str = str; a.pad = 0; S.anchor.push_back(a);
        WrsCreateOut x; x.ret = (u32)r; x.nW = (u32)O.nW; x.flags = O.windowsLimit ? 1u : 0u; x.pad = 0; x.hash = hashWC(O); S.createExp.push_back(x); c.n++;
        made.push_back({bin, str});
        if (r) { nClass[C_LIMIT]++; break; }
    }
    S.create.push_back(c);
}

// ---- layer 1: assignAlignToWindow ------------------------------------------------------------------------------------------------------------------------------------
static u64 hashWA(const std::vector<WAlign> &W) {
    u64 h = WRS_HASH0;
    for (const WAlign &e : W) { h = wrsMix(h, e.gStart); h = wrsMix(h, (u32)e.nrep); h = wrsMix(h, (u16)e.L); h = wrsMix(h, (u16)e.rStart); h = wrsMix(h, (u64)(i64)(i32)e.sjA); h = wrsMix(h, e.anchor); h = wrsMix(h, e.iFrag); }
    return h;
}
static void assignCase(WrsSet &S, Env *e, u32 ie, bool big) {
    Oracle &O = *e->O; const staramd_params &P = O.P; const u32 Nmax = P.seedPerWindowNmax;
    const u32 nWin = 3, binsPer = 48; if (P.winBinN < nWin * binsPer + 2) return;
    std::fill(O.winBin[0].begin(), O.winBin[0].end(), 0xFFFF); std::fill(O.winBin[1].begin(), O.winBin[1].end(), 0xFFFF);
    for (u32 w = 0; w < nWin; w++) for (u32 b = 0; b < binsPer; b++) O.winBin[0][w * binsPer + b] = (uint16_t)w;
    O.nW = nWin; O.WA.assign(nWin, std::vector<WAlign>()); O.WALrec.assign(nWin, 0); O.tooManyAnchors = false; O.Lread = 120 + rnd(130);
    WrsAssign c; memset(&c, 0, sizeof(c)); c.env = ie; c.big = big; c.Lread = (u32)O.Lread; c.off = (u32)S.seedIn.size(); c.nWin = nWin; c.capBlocks = rnd(5) == 0 ? 1 + rnd(2) : WRS_BLOCKS;
    const u32 flavour = rnd(8);                       // 7: one length, one anchor (a compaction that leaves nearly nothing); 6: a diagonal of its own for every seed (lists that fill up); 0: anything; 1: all anchors (a full list ends the read); 2: no anchors, lengths falling; 3: rising; 4: one window, one diagonal; 5: few anchors, many equal lengths
    const u32 n = 8 + rnd(flavour == 4 ? 60 : 3 * Nmax + 30), span = (binsPer << P.winBinNbits);
    const u32 Lr = (u32)O.Lread; if (span < Lr + 40) return;
    u64 diag[3][3]; for (u32 w = 0; w < nWin; w++) for (u32 d = 0; d < 3; d++) diag[w][d] = ((u64)w * binsPer << P.winBinNbits) + rnd(span - Lr - 2);
    std::set<u32> touched;
    for (u32 k = 0; k < n; k++) {
        WrsSeedIn a; memset(&a, 0, sizeof(a));
        a.iW = flavour == 4 ? 0 : rnd(6) ? 0 : rnd(nWin); a.frag = rnd(8) == 0 ? 1 : 0; a.sjA = rnd(10) == 0 ? (i32)rnd(3) : -1; a.nrep = 1 + rnd(300);
        a.anchor = flavour == 7 ? rnd(40) == 0 : flavour == 6 ? rnd(4) != 0 : flavour == 1 ? 1 : flavour == 2 || flavour == 3 ? 0 : flavour == 5 ? rnd(10) == 0 : rnd(2);
        a.L = flavour == 7 ? 20 + (rnd(30) == 0) : flavour == 2 ? std::max<i32>(5, 60 - (i32)k / 2) : flavour == 3 ? 5 + k / 2 : flavour == 5 ? 20 + rnd(3) : 5 + rnd(50);
        if (a.L > Lr - 1) a.L = Lr - 1;
        a.rStart = rnd(Lr - a.L);
        a.a1 = flavour >= 6 ? ((u64)a.iW * binsPer << P.winBinNbits) + rnd(span - Lr - 2) + a.rStart : diag[a.iW][flavour == 4 ? 0 : rnd(4) ? 0 : rnd(3)] + a.rStart;
        // classes, from the list before the call (the decisions of ReadAlign_assignAlignToWindow.cpp, restated for the table only)
        std::vector<WAlign> &W = O.WA[a.iW]; const u64 lrec0 = O.WALrec[a.iW]; bool blocksOut = false;
        if (!a.anchor && a.L < lrec0) nClass[A_REJECT_ENTRY]++;
        else {
            if (!touched.count(a.iW)) { if (touched.size() >= c.capBlocks) blocksOut = true; else touched.insert(a.iW); }
            if (!blocksOut) {
                u64 iA; bool diagNoHit = false;
                for (iA = 0; iA < W.size(); iA++) { const bool dg = a.a1 + W[iA].rStart == W[iA].gStart + a.rStart, c1 = a.rStart >= W[iA].rStart && a.rStart < W[iA].rStart + W[iA].L, c2 = a.rStart + a.L >= W[iA].rStart && a.rStart + a.L < W[iA].rStart + W[iA].L;
                    if (dg && (c1 || c2) && (a.frag != W[iA].iFrag || W[iA].sjA != (u64)(i64)a.sjA)) diagNoHit = true;
                    if (dg && (c1 || c2) && a.frag == W[iA].iFrag && W[iA].sjA == (u64)(i64)a.sjA) { if (!c1) nClass[A_CLAUSE2]++; break; } }
                if (iA < W.size()) {
                    if (a.L <= W[iA].L) nClass[A_HIT_NOCHANGE]++;
                    else { u64 iA0; for (iA0 = 0; iA0 < W.size(); iA0++) if (iA0 != iA && a.rStart < W[iA0].rStart) break; if (iA0 > iA) --iA0; nClass[iA0 < iA ? A_MOVE_LEFT : iA0 > iA ? A_MOVE_RIGHT : A_INPLACE]++; }
                } else {
                    if (diagNoHit) nClass[A_DIAG_NOHIT]++;
                    u64 size = W.size(), lrec = lrec0; bool out = false;
                    if (size == Nmax) {
                        u32 nShort = 0; lrec = O.Lread + 1; for (const WAlign &x : W) if (x.anchor != 1) lrec = std::min(lrec, x.L); for (const WAlign &x : W) if (x.anchor != 1 && x.L == lrec) nShort++;
                        if (lrec == O.Lread + 1) { nClass[A_FULL_ANCHORS]++; out = true; }
                        else { if (nShort == 1) nClass[A_FULL_LREC]++;
                            if (!a.anchor && a.L < lrec) out = true;
                            else { u64 keep = 0; for (const WAlign &x : W) if (x.anchor == 1 || x.L > lrec) keep++; if (size - keep == 1) nClass[A_COMPACT_1]++; if (keep <= 2 && size > 4) nClass[A_COMPACT_MOST]++;
                                   nClass[a.anchor || a.L > lrec ? A_COMPACT_INSERT : A_COMPACT_REJECT]++; size = keep; } }
                    }
                    if (!out && (a.anchor || a.L > lrec)) {
                        u64 rank = 0, sz = 0; for (const WAlign &x : W) { if (size != W.size() && !(x.anchor == 1 || x.L > lrec)) continue; sz++; }
                        { u64 seen = 0; rank = sz; for (const WAlign &x : W) { if (size != W.size() && !(x.anchor == 1 || x.L > lrec)) continue; if (a.rStart < x.rStart) { rank = seen; break; } seen++; } }
                        nClass[rank == 0 ? A_INS_0 : rank == sz ? A_INS_END : A_INS_MID]++;
                        if (sz + 1 == 63) nClass[A_LIST_63]++; if (sz + 1 == 64) nClass[A_LIST_64]++;
                    }
                }
            }
        }
        WrsAssignOut x; memset(&x, 0, sizeof(x));
        if (blocksOut) { nClass[A_BLOCKS_OUT]++; x.nwa = 0; x.lrec = 0; x.flags = 2; x.nBlocks = (u32)touched.size(); x.hash = WRS_HASH0; }
        else { O.assignAlignToWindow(a.a1, a.L, 0, a.nrep, a.frag, a.rStart, a.anchor != 0, (u64)(i64)a.sjA);
               x.nwa = (u32)W.size(); x.lrec = (u32)O.WALrec[a.iW]; x.flags = O.tooManyAnchors ? 1u : 0u; x.nBlocks = (u32)touched.size(); x.hash = touched.count(a.iW) ? hashWA(W) : WRS_HASH0; }
        S.seedIn.push_back(a); S.assignExp.push_back(x); c.n++;
        if (blocksOut || O.tooManyAnchors) break;
    }
    O.tooManyAnchors = false;
    S.assign.push_back(c);
}

// ---- layer 1: sjAlignSplit, the owner map, the wave helpers ---------------------------------------------------------------------------------------------------------------
static void splitCases(WrsSet &S, Env *e, u32 ie, u32 n) {
    Oracle &O = *e->O; const u64 ovh = e->w.sjdbOverhang, len = e->w.sjdbLength, region = (u64)e->w.sjdbN * len; if (!e->w.sjdbN) return;
    for (u32 k = 0; k < n; k++) {
        WrsSplit c; memset(&c, 0, sizeof(c)); c.env = ie;
        const u32 how = rnd(8); u64 off; u32 L = 5 + rnd(60);
        if (how == 0 && region > (1ull << 32) + 70) { off = (1ull << 32) - 1 + rnd(3); L = rnd(2) ? L : (u32)ovh; }
        else { const u64 isj = rng() % e->w.sjdbN; const u32 h2 = rnd(6); u64 sj1 = h2 == 0 ? ovh - 1 : h2 == 1 ? ovh : h2 <= 3 ? ovh - 1 - rnd((u32)std::min<u64>(ovh - 1, 70)) : rng() % (len - 70);
               const u32 h3 = rnd(4); if (sj1 < ovh && h3 == 0) L = (u32)(ovh - sj1); else if (sj1 < ovh && h3 == 1) L = (u32)(ovh - sj1) + 1; if (L > 60000) L = 60000; if (L == 0) L = 1; off = isj * len + sj1; }
        c.a1 = e->w.sjGstart + off; c.L = L;
        u64 a1D = 0, lD = 0, a1A = 0, lA = 0, isj = 0;
        c.expRet = O.sjAlignSplit(c.a1, L, a1D, lD, a1A, lA, isj) ? 1u : 0u; c.expD = a1D; c.expA = a1A; c.expLD = (u32)lD; c.expLA = (u32)lA; c.expIsj = (u32)isj;
        const u64 sj1 = off % len;
        nClass[c.expRet ? S_TRUE : S_FALSE]++; if (off >> 32) nClass[S_64BIT]++; if (off == (1ull << 32) - 1) nClass[S_OFF_M1]++; if (off == (1ull << 32)) nClass[S_OFF_0]++; if (off == (1ull << 32) + 1) nClass[S_OFF_P1]++;
        if (sj1 == ovh - 1) nClass[S_SJ1_OVH_M1]++; if (sj1 == ovh) nClass[S_SJ1_OVH]++; if (sj1 + L == ovh) nClass[S_END_OVH]++; if (sj1 + L == ovh + 1) nClass[S_END_OVH1]++;
        S.split.push_back(c);
    }
}
static u32 ownHome(u32 key, u32 mask) { return (key * 0x9E3779B1u >> 12) & mask; }
static void ownCase(WrsSet &S) {
    static const u32 SLOTS[5] = {32, 128, 512, 2048, 8192};
    WrsOwn c; memset(&c, 0, sizeof(c)); c.slots = SLOTS[rnd(5)]; c.global = rnd(2); const u32 mask = c.slots - 1, room = c.slots * 5 / 8;
    nClass[c.global ? O_GLOBAL : O_LDS]++;
    std::map<u32, u32> want; std::vector<WrsOwnOp> ins;
    const auto put = [&](u32 key, u32 val) { if (!want.count(key) && want.size() >= room) return; WrsOwnOp o; o.key = key; o.val = val; ins.push_back(o); auto it = want.find(key); if (it == want.end() || it->second < val) want[key] = val; };
    const auto val = [&]() { return (rnd(2) << OWN_BITS) | rnd(1u << OWN_BITS); };
    const u32 flavour = rnd(4);
    if (flavour == 0 && c.slots >= 128) {             // one cluster of more than 64 keys whose home slots lie in the last 8 of the table: the probes wrap
        u32 key = rnd(1u << 20); for (u32 got = 0, tries = 0; got < 66 + rnd(10) && tries < (1u << 21); tries++, key = (key + 1) & 0xFFFFFu) if (ownHome(key, mask) >= c.slots - 8) { put(key, val()); got++; }
    } else if (flavour == 1) { for (u32 k = 0; k < 4; k++) { const u32 key = rnd(1u << 20), m = 2 + rnd(12); for (u32 j = 0; j < m; j++) put(key, val()); nClass[O_SAME_KEY]++; } }
    put((1u << 20) - 1, val()); nClass[O_KEY_TOP]++; if (rnd(2)) put(0, val());
    { const u32 more = rnd(room); for (u32 k = 0; k < more; k++) put(rnd(8) ? rnd(1u << 20) : rnd(64), val()); }
    for (size_t k = ins.size(); k > 1; k--) std::swap(ins[k - 1], ins[rnd((u32)k)]);
    while (ins.size() % 64) { WrsOwnOp o; o.key = 0xFFFFFFFFu; o.val = 0; ins.push_back(o); }
    // the table as a sequential fill leaves it: how far a look-up walks (classes only; the slots a key takes depend on the order, the lengths of the clusters do not)
    std::vector<u32> tab(c.slots, 0); for (const WrsOwnOp &o : ins) if (o.key != 0xFFFFFFFFu) { u32 h = ownHome(o.key, mask); while (tab[h] && tab[h] != o.key + 1) h = (h + 1) & mask; tab[h] = o.key + 1; }
    std::vector<WrsOwnOp> q; for (const auto &kv : want) { WrsOwnOp o; o.key = kv.first; o.val = kv.second & ((1u << OWN_BITS) - 1u); q.push_back(o); }
    for (u32 k = 0, na = 8 + rnd(40); k < na; k++) { u32 key = rnd(1u << 20); if (k < 8 && flavour == 0) for (u32 t = 0; t < (1u << 21) && (want.count(key) || ownHome(key, mask) < c.slots - 8); t++) key = (key + 1) & 0xFFFFFu;
        if (want.count(key)) continue; WrsOwnOp o; o.key = key; o.val = NOWIN; q.push_back(o); nClass[O_ABSENT]++; }
    for (const WrsOwnOp &o : q) { u32 h = ownHome(o.key, mask), steps = 0; bool wrap = false; while (tab[h] && tab[h] != o.key + 1) { if (h == mask) wrap = true; h = (h + 1) & mask; steps++; } if (steps > 64) nClass[O_CHAIN_65]++; if (wrap) nClass[O_WRAP]++; }
    while (q.size() % 64) q.push_back(q[0]);
    c.insOff = (u32)S.ownOp.size(); c.nIns = (u32)ins.size(); S.ownOp.insert(S.ownOp.end(), ins.begin(), ins.end());
    c.qOff = (u32)S.ownOp.size(); c.nQ = (u32)q.size(); S.ownOp.insert(S.ownOp.end(), q.begin(), q.end());
    S.own.push_back(c);
}
static void waveCase(WrsSet &S, u32 k) {
    WrsWave c; memset(&c, 0, sizeof(c)); WrsWaveOut x; memset(&x, 0, sizeof(x));
    const u32 how = k % 5; std::set<u32> used;
    for (u32 l = 0; l < 64; l++) { u32 key = how == 0 ? 0 : rnd(3) == 0 ? 0 : 1 + rnd(how == 4 ? 200 : 0xFFFFFFF0u); while (key && used.count(key)) key++; used.insert(key); c.v64[l] = ((u64)key << 32) | (u32)rng(); c.v32[l] = how == 4 ? rnd(5) : (u32)rng(); }
    if (how == 1) c.v64[0] = (0xFFFFFFFFull << 32) | (u32)rng(); if (how == 2) c.v64[63] = (0xFFFFFFFFull << 32) | (u32)rng(); if (how == 1) c.v32[63] = 0; if (how == 2) c.v32[0] = 0xFFFFFFFFu;
    u32 best = 0; for (u32 l = 1; l < 64; l++) if ((c.v64[l] >> 32) > (c.v64[best] >> 32)) best = l;
    x.max64 = (c.v64[best] >> 32) ? c.v64[best] : 0; x.min32 = c.v32[0]; for (u32 l = 1; l < 64; l++) x.min32 = std::min(x.min32, c.v32[l]);
    if (!(c.v64[best] >> 32)) nClass[V_ALLZERO]++; else if (best == 0) nClass[V_MAX_LANE0]++; else if (best == 63) nClass[V_MAX_LANE63]++;
    for (u32 l = 0; l < 64; l++) { u8 *p = (u8 *)&c.seeds[l]; for (u32 b = 0; b < sizeof(DSeed); b++) p[b] = (u8)rng(); }
    c.src = rnd(64); x.sd = c.seeds[c.src]; memset((u8 *)&x.sd + 20, 0, 4);
    S.wave.push_back(c); S.waveExp.push_back(x);
}

// ---- layer 2: reads ------------------------------------------------------------------------------------------------------------------------------------------------------
static const WrsGeom GEOMS[7] = {
    {128, 128, 16384, 1024, 1024, 65536, 1, 65536},       // the engine's
    {128, 128, 4096, 1024, 1024, 65536, 0, 65536},        // owner map off
    {2, 2, 4096, 3, 3, 4096, 1, 65536},                   // every read with more than 2 windows travels ovfWin -> ovfWin2 -> the table in global memory
    {2, 2, 4096, 0, 0, 4096, 0, 65536},                   // ... without a middle launch, Bloom filter
    {16, 16, 1024, 64, 64, 262144, 1, 16},                // 32 slots, then 8192; a low bar for light reads: heavy reads with window items
    {128, 128, 65536, 1024, 1024, 4096, 1, 65536},
    {128, 128, 4096, 1024, 1024, 16384, 1, 1000}};
struct ReadStats { u64 total = 0, full = 0; } readStats;
// How DC_nSAenum and DC_nWindows come about for one read: the kernel counts a chunk of 64 loci when it reads it, stops pass B at too many anchors, and a read that
// outgrows the table or the seed-list blocks of a launch is counted again by the next launch.  The trace holds, per call of the oracle's two routines in the oracle's order, the
// loci enumerated if the pass stopped in the chunk of that call, so that the expectation of a launch geometry follows from the oracle's own run.
struct Trace { struct ACall { u32 cum, nW; }; struct BCall { u32 cum, iW, tooMany; }; std::vector<ACall> A; std::vector<BCall> B; u64 fullA = 0, fullB = 0, nW = 0, nCov = 0; bool valid = false; };
static std::vector<Trace> traces;          // one per read of S.read
static void locusOf(Oracle &O, const Seed &s, u64 iSA, u64 &aStr, u64 &a1, u64 &aRstart) {
    a1 = O.SAat(iSA); aStr = a1 >> O.g.GstrandBit; a1 &= O.GstrandMask; aRstart = s.rStart;
    if (s.dir == 1 && aStr == 0) { aStr = 1; aRstart = O.Lread - (s.L + aRstart); } else if (s.dir == 0 && aStr == 1) { aRstart = O.Lread - (s.L + aRstart); a1 = O.g.nGenome - (s.L + a1); } else if (s.dir == 1 && aStr == 1) { aStr = 0; a1 = O.g.nGenome - (s.L + a1); }
}
// pass A call by call (ReadAlign_stitchPieces.cpp:41-93 as star_oracle.cpp states it); false: the read reaches the window limit
static bool tracePassA(Oracle &O, Trace &t) {
    const staramd_params &P = O.P; const u32 nbits = P.winBinNbits;
    std::fill(O.winBin[0].begin(), O.winBin[0].end(), 0xFFFF); std::fill(O.winBin[1].begin(), O.winBin[1].end(), 0xFFFF); O.nW = 0; O.WC.clear(); O.windowsLimit = false;
    u64 done = 0;
    for (const Seed &s : O.PC) {
        if (s.nrep > P.winAnchorMultimapNmax) continue;
        for (u64 j = 0; j < s.nrep; j++) {
            const u64 cnt = std::min<u64>(64, s.nrep - j / 64 * 64), chunkEnd = done + j / 64 * 64 + cnt;
            if (j % 64 == 0 && cnt >= 4 && cnt * 16 >= O.nW) {            // the shortcut of the kernel: loci owned when their chunk is read leave the replay
                bool drop = false, half = false;
                for (u64 i = 0; i < cnt; i++) { u64 aStr, a1, aR; locusOf(O, s, s.saStart + j + i, aStr, a1, aR);
                    if (a1 >= O.g.sjGstart) { u64 a1D, lD, a1A, lA, isj; if (!O.sjAlignSplit(a1, s.L, a1D, lD, a1A, lA, isj)) continue; const bool oD = O.winBin[aStr][a1D >> nbits] != 0xFFFF, oA = O.winBin[aStr][a1A >> nbits] != 0xFFFF; if (oD || oA) drop = true; if (oD != oA) half = true; }
                    else if (O.winBin[aStr][a1 >> nbits] != 0xFFFF) drop = true; }
                if (drop) nClass[R_SHORTCUT_DROP]++; if (half) nClass[R_SHORTCUT_HALF]++;
            }
            u64 aStr, a1, aR; locusOf(O, s, s.saStart + j, aStr, a1, aR);
            u64 call[2]; u32 nCall = 0;
            if (a1 >= O.g.sjGstart) { u64 a1D, lD, a1A, lA, isj; if (O.sjAlignSplit(a1, s.L, a1D, lD, a1A, lA, isj)) { call[0] = a1D; call[1] = a1A; nCall = 2; } } else { call[0] = a1; nCall = 1; }
            for (u32 c = 0; c < nCall; c++) { const int r = O.createExtendWindowsWithAlign(call[c], aStr); Trace::ACall x; x.cum = (u32)chunkEnd; x.nW = (u32)O.nW; t.A.push_back(x); if (r) return false; }
        }
        done += s.nrep;
    }
    t.fullA = done; return true;
}
// pass B call by call (:129-185) on the windows createWindows() left, up to too many anchors
static void tracePassB(Oracle &O, Trace &t) {
    const staramd_params &P = O.P; const u32 nbits = P.winBinNbits; u64 done = 0; bool stop = false;
    for (const Seed &s : O.PC) {
        const bool anchor = s.nrep <= P.winAnchorMultimapNmax;
        for (u64 j = 0; j < s.nrep && !stop; j++) {
            const u64 cnt = std::min<u64>(64, s.nrep - j / 64 * 64), chunkEnd = done + j / 64 * 64 + cnt;
            u64 aStr, a1, aR; locusOf(O, s, s.saStart + j, aStr, a1, aR);
            u64 ca[2], cl[2], cr[2], sj = (u64)-1; u32 nCall = 0;
            if (a1 >= O.g.sjGstart) { u64 a1D, lD, a1A, lA, isj; if (O.sjAlignSplit(a1, s.L, a1D, lD, a1A, lA, isj)) { ca[0] = a1D; cl[0] = lD; cr[0] = aR; ca[1] = a1A; cl[1] = lA; cr[1] = aR + lD; sj = isj; nCall = 2; } }
            else { ca[0] = a1; cl[0] = s.L; cr[0] = aR; nCall = 1; }
            for (u32 c = 0; c < nCall && !stop; c++) {
                const u32 iW = O.winBin[aStr][ca[c] >> nbits]; if (iW == 0xFFFF) continue;
                O.assignAlignToWindow(ca[c], cl[c], aStr, s.nrep, s.iFrag, cr[c], anchor, sj);
                Trace::BCall x; x.cum = (u32)chunkEnd; x.iW = iW; x.tooMany = O.tooManyAnchors ? 1u : 0u; t.B.push_back(x); if (O.tooManyAnchors) stop = true;
            }
        }
        done += s.nrep;
    }
    t.fullB = done;
}
// what the launches of a geometry add to the two counters for the read, and the launch that finishes it (0 first, 1 middle, 2 last)
static u32 expectCounters(const Trace &t, const WrsGeom &g, u32 limit, u64 &sa, u64 &win, bool &again, bool &stopped) {
    const u32 caps[3][2] = {{g.capW, g.capBlocks}, {g.capWMid, g.capBlocksMid}, {limit, limit}};
    for (u32 L = 0; L < 3; L++) {
        if (L == 1 && !g.capWMid) continue;
        const u32 capW = caps[L][0], capBlocks = caps[L][1]; bool ovf = false;
        for (const Trace::ACall &c : t.A) if (c.nW > capW) { sa += c.cum; win += capW; ovf = true; break; }
        if (ovf) { again = true; continue; }
        std::set<u32> touched;
        for (const Trace::BCall &c : t.B) {
            if (!touched.count(c.iW)) { if (touched.size() >= capBlocks) { sa += t.fullA + c.cum; win += t.nW; ovf = true; break; } touched.insert(c.iW); }
            if (c.tooMany) { sa += t.fullA + c.cum; win += t.nW; stopped = true; return L; }
        }
        if (ovf) { again = true; continue; }
        sa += t.fullA + t.fullB; win += t.nW; return L;
    }
    return 3;
}

static u64 placeLocus(Env *e, u64 &nSA, u32 dir, u32 str, u64 a1, u32 L) {           // the raw entry that the strand flip of the kernel turns into (str, a1)
    const u32 rawStr = str ^ dir; const u64 raw = rawStr ? e->w.nGenome - L - a1 : a1;
    packedPut(e->sa, nSA, e->w.strandBit + 1, raw | ((u64)rawStr << e->w.strandBit)); return nSA++;
}
static void makeRead(WrsSet &S, Env *e, u32 kindRead) {
    Oracle &O = *e->O; const staramd_params &P = O.P; const u32 nbits = P.winBinNbits; const u64 rb = realBins(*e);
    WrsRead rd; memset(&rd, 0, sizeof(rd)); rd.seedOff = (u32)S.seed.size(); rd.Lread = 100 + rnd(rnd(3) ? 151 : 540);
    static const u32 NS[5] = {1, 17, 64, 65, 130};
    u32 nSeeds = kindRead < 5 ? NS[kindRead] : 2 + rnd(24);
    const bool allUniq = kindRead == 5 || (kindRead < 5 && rnd(3) == 0), wide = kindRead == 6;       // wide: more than 1024 windows (the environment has room for them)
    const bool stack = kindRead == 8;                     // 64 seeds of one locus on 64 diagonals of one site: a list of 64 rows where seedPerWindowNmax allows it, too many anchors where it does not
    const bool many = kindRead == 9;                      // one-locus seeds spread over the genome: more windows than a low alignWindowsPerReadNmax allows
    if (wide) nSeeds = 130; if (stack) nSeeds = 64 - rnd(2); if (many) nSeeds = 60 + rnd(30);
    struct Site { u64 g0; u32 str; };
    std::vector<Site> sites; const u32 nSites = 1 + rnd(4); std::vector<u32> siteSj;        // junctions with a site at one of their ends: a split locus of theirs finds one half owned, the other not
    for (u32 k = 0; k < nSites; k++) { Site s; s.str = rnd(2); const u32 how = rnd(8); u64 bin;
        if (how == 0 && !sites.empty()) bin = (sites.back().g0 >> nbits) + 1 + rnd(2 * P.winAnchorDistNbins + 2), s.str = sites.back().str;        // near the site before: merges and flanks that meet
        else if (how == 1) bin = e->chrFirstBin[rnd((u32)e->chrFirstBin.size())] + rnd(3);
        else if (how == 2 && e->w.sjdbN) { const u32 j = rnd(e->w.sjdbN); siteSj.push_back(j); bin = (rnd(2) ? e->sjD[j] + e->w.sjdbOverhang : e->sjA[j]) >> nbits; }
        else if (how == 3) bin = rnd(2) ? rnd(3) : rb - 1 - rnd(3);
        else bin = rng() % rb;
        if (bin + 3 >= rb) bin = rb > 4 ? rb - 4 : 0; s.g0 = (bin << nbits) + rnd(1u << nbits); sites.push_back(s); }
    std::vector<u32> seedFam; bool sawMulti = false;
    for (u32 k = 0; k < nSeeds; k++) {
        DSeed sd; memset(&sd, 0, sizeof(sd)); sd.dir = (u8)rnd(2); sd.iFrag = (u8)rnd(2); sd.L = (u16)(12 + rnd(40)); sd.rStart = (u16)rnd(rd.Lread - sd.L + 1);
        static const u32 NREP[10] = {2, 3, 4, 5, 3, 4, 64, 65, 200, 1000};
        u32 nrep = allUniq || stack || many || rnd(10) < 7 ? 1 : NREP[rnd(rnd(4) ? 6 : 10)]; if (wide) nrep = 10; if (nrep >= 200 && (sawMulti || rnd(3))) nrep = 3 + rnd(2);
        const u32 fam = nrep == 1 ? rnd(4) == 0 : rnd(3);        // 0: mostly in one window that is already there; 1: spread over new bins; 2: with split loci mixed in
        if (wide || nrep > 5) sawMulti = true;
        sd.nrep = nrep; sd.saStart = e->nSA;
        const Site &st = sites[stack ? 0 : rnd((u32)sites.size())];
        for (u32 j = 0; j < nrep; j++) {
            u32 str = st.str; u64 a1; const u32 aR = str ? rd.Lread - (sd.L + sd.rStart) : sd.rStart;
            const bool sj = !stack && e->w.sjdbN && ((fam == 2 && rnd(3) == 0) || rnd(40) == 0);
            if (stack) a1 = st.g0 + aR + 7u * k;
            else if (sj) { const u64 isj = !siteSj.empty() && rnd(3) ? siteSj[rnd((u32)siteSj.size())] : rnd(e->w.sjdbN), ovh = e->w.sjdbOverhang; const u64 sj1 = rnd(6) ? ovh - 1 - rnd(sd.L - 1u) : ovh + rnd(20); a1 = e->w.sjGstart + isj * e->w.sjdbLength + sj1; str = rnd(2); }
            else if (fam == 1 || wide || many) { a1 = rng() % (e->w.sjGstart - sd.L - 1); str = rnd(2); }
            else if (rnd(4) == 0) { const u64 sh = (u64)rnd(2 * P.winAnchorDistNbins + 4) << nbits; a1 = st.g0 + sh; if (rnd(2) && st.g0 > sh) a1 = st.g0 - sh; }                // some bins away: merges, flanks
            else if (rnd(3)) a1 = st.g0 + aR;                         // on the site's diagonal: overlap hits, replacements
            else a1 = st.g0 + rnd(3u << nbits);
            if (!sj && a1 + sd.L + 1 >= e->w.sjGstart) a1 = e->w.sjGstart - sd.L - 2 - rnd(40);
            placeLocus(e, e->nSA, sd.dir, str, a1, sd.L);
            nClass[sd.dir ? (str ? R_D1S1 : R_D1S0) : (str ? R_D0S1 : R_D0S0)]++;
        }
        if (nrep == 3) nClass[R_NREP_3]++; if (nrep == 4) nClass[R_NREP_4]++; if (nrep == 64) nClass[R_NREP_64]++; if (nrep == 65) nClass[R_NREP_65]++; if (nrep == 1000) nClass[R_NREP_1000]++;
        if (nrep >= 3) nClass[fam == 0 ? R_FAM_OWNED : fam == 1 ? R_FAM_SPREAD : R_FAM_SPLIT]++;
        if (nrep > P.winAnchorMultimapNmax) nClass[R_MM_ABOVE]++; else if (nrep > 1) nClass[R_MM_BELOW]++;
        S.seed.push_back(sd); seedFam.push_back(fam);
    }
    rd.nSeeds = nSeeds;
    if (nSeeds == 1) nClass[R_SEEDS_1]++; if (nSeeds == 17) nClass[R_SEEDS_17]++; if (nSeeds == 64) nClass[R_SEEDS_64]++; if (nSeeds == 65) nClass[R_SEEDS_65]++; if (nSeeds == 130) nClass[R_SEEDS_130]++;
    if (allUniq) { bool bigc = e->w.nChrReal >= 0x3FFFu || e->chrBin[0] >= 0x3FFFu; nClass[bigc ? R_UNIQ_BIGCHR : R_UNIQ_SMALLCHR]++; }
    // ---- the oracle
    O.PC.clear(); for (u32 k = 0; k < nSeeds; k++) { const DSeed &d = S.seed[rd.seedOff + k]; Seed s; s.rStart = d.rStart; s.L = d.L; s.dir = d.dir; s.nrep = d.nrep; s.saStart = d.saStart; s.saEnd = d.saStart + d.nrep - 1; s.iFrag = d.iFrag; O.PC.push_back(s); }
    O.Lread = rd.Lread; O.tooManyAnchors = false; O.windowsLimit = false; O.g.SA = (const uint8_t *)e->sa.data();
    e->sa.resize(e->sa.size() + 2, 0);                     // (SAat reads 8 bytes from the byte an entry starts in)
    O.g.SA = (const uint8_t *)e->sa.data();
    traces.emplace_back(); Trace &tr = traces.back();
    tr.valid = tracePassA(O, tr);
    O.createWindows();
    rd.winOff = (u32)S.win.size(); readStats.total++;
    if (O.windowsLimit) { rd.full = 0; rd.expStatus = STARAMD_ST_WINDOWS_LIMIT; nClass[R_LIMIT]++; S.read.push_back(rd); return; }
    readStats.full++; rd.full = 1;
    // classes from the table before pass B changes nW
    { u64 nCov = 0; bool killed = false, over = false; const u64 nW = O.nW;
      for (u64 j = 0; j < nW; j++) { const Win &c = O.WC[j]; if (c.gStart > c.gEnd) { killed = true; continue; } nCov += c.gEnd - c.gStart + 1; }
      if (P.winFlankNbins > P.winAnchorDistNbins) { if (killed) nClass[R_KILLED_WIDE_FLANK]++;
          for (u64 j = 0; j + 1 < nW && !over; j++) for (u64 k = j + 1; k < nW && !over; k++) { const Win &a = O.WC[j], &b = O.WC[k]; if (a.gStart > a.gEnd || b.gStart > b.gEnd || a.str != b.str) continue; if (a.gStart <= b.gEnd && b.gStart <= a.gEnd) over = true; }
          if (over) nClass[R_FLANK_OVER_CORE]++; }
      tr.nW = nW; tr.nCov = nCov;
      if (nW > 1024) nClass[R_GT1024]++;
      if (e->kind == K_BIN19M && nW) nClass[R_BINS_MAP_LAST]++; if (e->kind == K_BIN19 && nW) nClass[R_BINS_MAP_OFF]++; }
    // split loci: where their halves go (from the map after the flanks)
    for (u32 k = 0; k < nSeeds; k++) { const Seed &s = O.PC[k]; for (u64 i = s.saStart; i <= s.saEnd; i++) { u64 a1 = O.SAat(i), aStr = a1 >> O.g.GstrandBit; a1 &= O.GstrandMask;
        if (s.dir == 1 && aStr == 0) aStr = 1; else if (s.dir == 0 && aStr == 1) a1 = O.g.nGenome - (s.L + a1); else if (s.dir == 1 && aStr == 1) { aStr = 0; a1 = O.g.nGenome - (s.L + a1); }
        if (a1 < O.g.sjGstart) continue; u64 a1D, lD, a1A, lA, isj; if (!O.sjAlignSplit(a1, s.L, a1D, lD, a1A, lA, isj)) continue;
        const uint16_t wD = O.winBin[aStr][a1D >> nbits], wA = O.winBin[aStr][a1A >> nbits];
        if (wD != 0xFFFF && wA != 0xFFFF && wD != wA) nClass[R_SPLIT_TWO_WIN]++; if ((wD == 0xFFFF) != (wA == 0xFFFF)) nClass[R_SPLIT_ONE_NONE]++; } }
    { const u64 nW0 = O.nW; tracePassB(O, tr); O.nW = nW0; O.WA.assign(nW0, std::vector<WAlign>()); O.WALrec.assign(nW0, 0); O.tooManyAnchors = false; }          // (the lists as createWindows() left them)
    O.assignSeeds();
    if (O.tooManyAnchors) { rd.expStatus = STARAMD_ST_TOO_MANY_ANCHORS | STARAMD_ST_NO_GOOD_WINDOW; nClass[R_TOOMANY]++; S.read.push_back(rd); return; }
    bool one = false, apart0 = false, apart1 = false;
    for (u64 iW = 0; iW < O.nW; iW++) {
        const std::vector<WAlign> &W = O.WA[iW]; if (W.empty()) continue;
        WrsWin w; memset(&w, 0, sizeof(w)); w.chr = (u32)O.WC[iW].chr; w.str = (u32)O.WC[iW].str; w.nWA = (u32)W.size(); w.rowOff = (u32)S.row.size();
        for (const WAlign &a : W) { DWA r; memset(&r, 0, sizeof(r)); r.gStart = a.gStart; r.nrep = (u32)a.nrep; r.L = (u16)a.L; r.rStart = (u16)a.rStart; r.sjA = (i32)(i64)a.sjA; r.anchor = (u8)a.anchor; r.iFrag = (u8)a.iFrag; S.row.push_back(r);
                                  w.mates |= a.iFrag == 0 ? 1u : 2u; }
        if (w.mates == 3) one = true; if (w.mates == 1) apart0 = true; if (w.mates == 2) apart1 = true;
        if (w.nWA == 1) nClass[R_EMIT_1]++; if (w.nWA == 2) nClass[R_EMIT_2]++; if (w.nWA == 3) nClass[R_EMIT_3]++; if (w.nWA == 64) nClass[R_EMIT_64]++; if (iW >= 64) nClass[R_EMIT_LATE_ROWS]++;
        rd.expWt = std::max(rd.expWt, w.nWA); rd.expNWin++; S.win.push_back(w);
    }
    if (one) nClass[R_MATES_ONE]++; if (apart0 && apart1) nClass[R_MATES_APART]++;
    S.read.push_back(rd);
}
// the reads of one environment and the batches over them: every geometry over the same reads
static void makeBatches(WrsSet &S, Env *e, u32 nReads, bool dump) {
    Oracle &O = *e->O; const u32 readOff = (u32)S.read.size();
    memset(O.cnt, 0, sizeof(O.cnt));
    const bool roomy = e->kind == K_WIDE;
    for (u32 r = 0; r < nReads; r++) makeRead(S, e, roomy && r < 4 ? 6 : O.P.alignWindowsPerReadNmax == 50 && r % 3 == 0 ? 9 : rnd(O.P.seedPerWindowNmax == 64 ? 3 : 12) == 0 ? 8 : rnd(3) == 0 ? rnd(6) : 7);
    const u32 ie = envToSet(S, e);
    bool anyLimit = false; u32 totWin = 0, totWA = 0;
    for (u32 r = 0; r < nReads; r++) { const WrsRead &rd = S.read[readOff + r]; if (!rd.full) anyLimit = true;
        for (u32 k = 0; k < rd.expNWin; k++) { totWin++; totWA += S.win[rd.winOff + k].nWA; } }
    // (the pools of a batch with reads at the limit: the oracle has no window count for them -- what the kernel can emit at most is the limit itself per read and every locus twice)
    u32 slackWin = 0, slackWA = 0; for (u32 r = 0; r < nReads; r++) { const WrsRead &rd = S.read[readOff + r]; if (rd.full) continue; slackWin += O.P.alignWindowsPerReadNmax; for (u32 k = 0; k < rd.nSeeds; k++) slackWA += 2 * S.seed[rd.seedOff + k].nrep; }
    const u32 nGeom = roomy ? 2 : 7;
    for (u32 gi = 0; gi < nGeom; gi++) {
        if (dump && gi >= 5) continue;
        WrsGeom g = GEOMS[gi]; if (g.capWMid && g.capWMid >= O.P.alignWindowsPerReadNmax) g.capWMid = 0;          // as engine.hip: no middle launch at or above the limit
        WrsBatch b; memset(&b, 0, sizeof(b)); b.env = ie; b.geom = (u32)S.geom.size(); S.geom.push_back(g); b.readOff = readOff; b.nReads = nReads; b.totWin = totWin + slackWin; b.totWA = totWA + slackWA;
        b.cmpCounters = anyLimit ? 0 : 2; b.expWA = totWA;
        bool again = false, stopped = false;
        for (u32 r = 0; r < nReads && !anyLimit; r++) {
            const Trace &t = traces[readOff + r]; const u32 L = expectCounters(t, g, O.P.alignWindowsPerReadNmax, b.expSAenum, b.expWindows, again, stopped);
            // the launch that finishes the read decides the size of its owner map: covered bins against 5/8 of its slots, half a window's worth either side
            const u32 hb = L == 0 ? g.hashBits : L == 1 ? g.hashBitsMid : 0; if (!hb || !g.ownerMap || !t.nW || t.nW > 1024 || O.P.winBinN >= (1u << 19)) continue;
            const u64 slots5 = (u64)(hb / 32) * 5, c8 = t.nCov * 8; if (c8 <= slots5 && c8 + 64 > slots5) nClass[R_COVER_BELOW]++; if (c8 > slots5 && c8 < slots5 + 64) nClass[R_COVER_ABOVE]++;
        }
        if (b.cmpCounters == 2 && b.expWindows) { nClass[B_COUNTERS]++; if (again) nClass[B_COUNTERS_REPEAT]++; if (stopped) nClass[B_COUNTERS_TOOMANY]++; }
        nClass[g.capWMid ? B_MID : B_NO_MID]++; if (g.capW == 2) nClass[B_TINY]++; if (!g.ownerMap) nClass[B_MAP_OFF]++;
        S.batch.push_back(b);
        if (gi == 0 && !anyLimit && totWin > 1 && totWA > 1) { WrsBatch s1 = b; s1.shortPool = 1; s1.cmpCounters = 0; S.batch.push_back(s1); nClass[B_SHORT_WIN]++; WrsBatch s2 = b; s2.shortPool = 2; s2.cmpCounters = 0; S.batch.push_back(s2); nClass[B_SHORT_WA]++; }
    }
}

// a routine that contradicts itself may loop for ever: reported, not waited for
static void onAlarm(int) { static const char msg[] = "\na routine does not end: 1 differences\n"; (void)!write(1, msg, sizeof(msg) - 1); _exit(1); }

int main(int argc, char **argv) {
    signal(SIGALRM, onAlarm); alarm(900);
    long scale = 100; const char *dumpPath = nullptr;
    for (int a = 1; a < argc; a++) { if (!strcmp(argv[a], "--dump") && a + 1 < argc) dumpPath = argv[++a]; else scale = atol(argv[a]); }
    static WrsSet S; dumping = dumpPath != nullptr;
    const u32 nEnv = dumpPath ? 3 : (u32)std::max<long>(4, 8 * scale / 100);            // (a batch is ~0.3 s of the emulator: the environments are few, the routine cases many)
    for (u32 ie = 0; ie < nEnv + 4; ie++) {
        // the last four: winBinN = 2^19 - 1, winBinN = 2^19, the overhang of 2^19 (splits only), room for more than 1024 windows
        const int kind = ie < nEnv ? K_NORMAL : ie == nEnv ? K_BIN19M : ie == nEnv + 1 ? K_BIN19 : ie == nEnv + 2 ? K_BIGOVH : K_WIDE;
        Env *e = makeEnv(kind, ie); envs.push_back(e);
        if (kind == K_BIGOVH) { const u32 id = envToSet(S, e); splitCases(S, e, id, dumpPath ? 3000 : 20000); continue; }
        const u32 lim = e->w.P.alignWindowsPerReadNmax;                // (few reads where nearly every read reaches the limit: the share compared in full stays above 95 %)
        makeBatches(S, e, kind == K_WIDE ? 8 : e->w.P.winAnchorMultimapNmax == 0 ? 8 : kind != K_NORMAL ? 24 : lim == 4 ? 4 : lim == 50 ? 10 : dumpPath ? 60 : 40, dumpPath != nullptr);
        const u32 id = (u32)S.env.size() - 1;
        const u32 nCreate = dumpPath ? 60 : (u32)(60 * scale / 100), nAssign = dumpPath ? 80 : (u32)(110 * scale / 100);
        for (u32 k = 0; k < nCreate * (lim < 10000 ? 3 : 1); k++) createCase(S, e, id, k & 1);
        if (kind == K_NORMAL || kind == K_WIDE) for (u32 k = 0; k < nAssign; k++) assignCase(S, e, id, k & 1);
        splitCases(S, e, id, 300);
    }
    for (u32 k = 0; k < (dumpPath ? 100u : 400u); k++) ownCase(S);
    for (u32 k = 0; k < 500; k++) waveCase(S, k);
    if (dumpPath) { FILE *f = fopen(dumpPath, "wb"); if (!f) { perror(dumpPath); return 2; } wrsWrite(f, S); if (fclose(f)) { perror(dumpPath); return 2; } }
    long bad = wrsRun(S, true);
    long empty = 0; u64 rarest = ~0ull;
    for (int c = 0; c < N_CLASSES; c++) { printf("  %-72s %llu\n", CLASS_NAME[c], (unsigned long long)nClass[c]); if (!nClass[c]) empty++; rarest = std::min<u64>(rarest, nClass[c]); }
    printf("rarest class: %llu cases\n", (unsigned long long)rarest);
    if (empty) { printf("%ld case classes never occurred\n", empty); bad += empty; }
    const double share = readStats.total ? (double)readStats.full / (double)readStats.total : 0.0;
    printf("compared share %.4f\n", share);
    if (share < 0.95) { printf("fewer than 95 %% of the reads are compared in full\n"); bad++; }
    printf("%zu window tables of %zu anchors, %zu seed lists of %zu seeds, %zu splits, %zu owner maps, %zu wave cases, %zu batches over %zu reads: %ld differences\n", S.create.size(), S.anchor.size(), S.assign.size(), S.seedIn.size(),
           S.split.size(), S.own.size(), S.wave.size(), S.batch.size(), S.read.size(), bad);
    return bad ? 1 : 0;
}
