// tail_routines_check.cpp -- TEST INFRASTRUCTURE: the seven kernels behind the stitch walk that every result passes through, one at a time and then as engine.hip runs them, on
// reads, windows, pools and candidate logs made by hand: k_pack_reads, k_stitch_verify, k_stitch_replay, k_stitch_finish (with chimSelectPartner) of k_stitch.hip and k_scan_local,
// k_scan_offsets, k_gather of k_gather.hip.  Where the expected values come from (never from an emulated kernel):
//   output layout and selection     Oracle::emitRead (star_oracle.cpp, the loop mapOneRead ends with) on the same window lists: staramd_read_result, transcripts (iW, exonOffset), exons
//   trBest, per-read limit, no good window     star_oracle.cpp:827-850 (ReadAlign_stitchPieces.cpp:288-348) restated as a loop over the lists (finishExpect)
//   incoming maxScoreMate           star_oracle.cpp:702-706, DESIGN.md 5.4: the maximum of 0 and mm[f] of the windows before; queued iff sens[f] is smaller for some f (verifyExpect)
//   the list of a replayed window   cand_log_ref.h candLogSequential (stitchWindowAligns.cpp:232-303), the LDS arena and then the arena in global memory
//   the partner of resultSelect 2   partnerOverWindows of star_amd/csrc/host/chimeric.cpp:271-299 (ReadAlign_chimericDetectionOld.cpp:45-97) restated over the arrays emitRead gives
//                                   for resultSelect 0 (partnerExpect)
//   k_pack_reads, the scans         their definitions: a loop
// Layers: A packing; B verify; C replay (2 blocks, a small LDS arena, trCap / exCap exactly sufficient and one record short, a window that fits neither arena); D finish over fabricated
// DWinOut and pools; E both scans called directly; F verify -> replay -> finish -> scan_local -> scan_offsets -> gather with the launch shapes of engine.hip, result arrays exactly as
// large as the totals and one record short, and once with CUR_FLAGS set.  Every case is classified from the reference side; the class table is printed, a class that never occurred
// fails the run, and every case made is launched and compared ("compared N of N cases").
// k_pack_reads has no CUR_FLAGS test (it runs at upload, before any pool is used), so the flags class covers the six kernels that have one.
// usage: tail_routines_check [--dump file]
#include "k_stitch.hip"
#include "k_gather.hip"
#include "star_oracle.cpp"
#include "tail_routines_cases.h"
#include <random>
#include <array>
#include <csignal>
#include <unistd.h>
extern thread_local uint32_t ldsReads[];

static std::mt19937_64 rng(20251020);
static u32 rnd(u32 n) { return (u32)(rng() % n); }
#include "cand_log_ref.h"

enum { P_WORDS_1, P_WORDS_13, P_WORDS_64, P_WORDS_65, P_LEN_0, P_LEN_1, P_LEN_FULL_M1, P_LEN_FULL, P_HIGH_BITS, P_READS_70,
       V_NREADS_1, V_NREADS_256, V_NREADS_257, V_NREADS_600, V_NWIN_0, V_NWIN_1, V_NWIN_70, V_STRADDLE, V_SENS_EQ, V_SENS_BELOW1, V_SENS_MAX, V_ONE_MATE, V_NEG_MM, V_REDO, V_REPLAY,
       R_ITEMS_0, R_ITEMS_1, R_ITEMS_3, R_ITEMS_50, R_FIRST_ATTEMPT, R_SECOND_ATTEMPT, R_HARD, R_CAP_EXACT, R_CAP_SHORT, R_CAP_EX_SHORT, R_EMPTY_RESULT, R_MATE_CLAUSE,
       F_SEL0, F_SEL1, F_SEL2, F_RANGE0, F_RANGE1, F_RANGE_LARGE, F_SINGLE_END, F_PAIRED, F_NWIN0_SEEDS, F_NWIN0_NOSEEDS, F_NWIN0_SCRATCH, F_NWIN0_NOGOOD, F_NWIN0_TOOMANY, F_ALL_EMPTY, F_BEST0,
       F_TIE_LATER_SMALLER, F_TIE_LATER_LARGER, F_TIE_EQUAL, F_BEST_BEHIND_EMPTY, F_LIMIT_EXACT, F_LIMIT_BELOW, F_LIMIT_ABOVE, F_LIMIT_FIRST, F_PREFIX_EMPTIES_BEFORE, F_PREFIX_EMPTIES_AFTER, F_PREFIX_CUTS_BEST,
       F_PARTNER_OTHER_WIN, F_PARTNER_RANK, F_PARTNER_NONE, F_PARTNER_STRAND, F_PARTNER_MOTIF0, F_PARTNER_OVERLAP1, F_PARTNER_NO_OVERLAP1, F_PARTNER_CROSS_SHARED, F_PARTNER_SPACER, F_CHIM0_SEL2,
       S_LOCAL_1, S_LOCAL_255, S_LOCAL_256, S_LOCAL_257, S_LOCAL_1000, S_OFF_1, S_OFF_2, S_OFF_1023, S_OFF_1024, S_OFF_1025, S_OFF_2047, S_OFF_2048, S_OFF_2049, S_OFF_5000, S_ZEROS, S_LARGE,
       T_NREADS_1, T_NREADS_256, T_NREADS_257, T_NREADS_700, T_QUEUED, T_NOT_QUEUED_LOG, T_CAP_EXACT, T_CAP_TR_SHORT, T_CAP_EX_SHORT, T_BEST_SECOND_BLOCK, T_PARTNER, T_FLAGS, N_CLASSES };
static const char *CLASS_NAME[N_CLASSES] = {
    "pack: packWords 1", "pack: packWords 13", "pack: packWords 64", "pack: packWords 65 (second trip of the 64 lanes)", "pack: read of length 0", "pack: read of length 1", "pack: read of 8 * packWords - 1 bases",
    "pack: read of 8 * packWords bases", "pack: bytes with bits above the low nibble", "pack: 70 reads",
    "verify: 1 read", "verify: 256 reads", "verify: 257 reads", "verify: 600 reads", "verify: read without windows", "verify: read with 1 window", "verify: read with 70 windows", "verify: windows of a read on both sides of place 256",
    "verify: sens == incoming (not queued by it)", "verify: sens == incoming - 1", "verify: sens INT32_MAX under a positive incoming value", "verify: queued by one mate alone", "verify: negative mm", "verify: window to the redo list",
    "verify: window to the replay list",
    "replay: no item", "replay: 1 item", "replay: 3 items", "replay: 50 items (more than wavefronts)", "replay: fits the LDS arena", "replay: second attempt, arena in global memory", "replay: fits neither arena (OVF_HARD)",
    "replay: pools exactly sufficient", "replay: trCap one short (OVF_TRPOOL)", "replay: exCap one short (OVF_TRPOOL)", "replay: window left without a transcript", "replay: candidate admitted by the maxScoreMate clause alone",
    "finish: resultSelect 0", "finish: resultSelect 1", "finish: resultSelect 2", "finish: outFilterMultimapScoreRange 0", "finish: ... 1", "finish: ... large", "finish: single-end", "finish: paired-end",
    "finish: no window, seeds", "finish: no window, no seeds", "finish: no window, scratch overflow", "finish: no window, no good window already set", "finish: no window, too many anchors", "finish: every window empty", "finish: best score 0",
    "finish: equal head scores, the later gLength smaller", "finish: ... the later gLength larger", "finish: ... equal gLength", "finish: the best window behind empty windows", "finish: nTr + perWindow == perRead", "finish: ... one below",
    "finish: ... above", "finish: the limit at the first window", "finish: the prefix empties a window before the best", "finish: ... after the best", "finish: the prefix shortens the best window",
    "partner: head of another window, below the range", "partner: rank > 0 of the best window, below the range", "partner: none eligible", "partner: strand conflict", "partner: intronMotifs[0] > 0", "partner: runner-up shares a block with the best",
    "partner: runner-up of the best window shares none", "partner: heads of two other windows share a block (not counted)", "partner: segment behind the mate spacer", "finish: resultSelect 2 without chimSegmentMinPositive",
    "scan_local: 1 read", "scan_local: 255", "scan_local: 256", "scan_local: 257", "scan_local: 1000", "scan_offsets: 1 block", "scan_offsets: 2", "scan_offsets: 1023", "scan_offsets: 1024", "scan_offsets: 1025 (chunk 2)",
    "scan_offsets: 2047", "scan_offsets: 2048", "scan_offsets: 2049 (chunk 3)", "scan_offsets: 5000", "scan_offsets: all zero", "scan_offsets: sums above 2^31",
    "tail: 1 read", "tail: 256 reads", "tail: 257 reads", "tail: 700 reads", "tail: window replayed on the way", "tail: window with a log, not queued", "tail: arrays exactly as large as the totals", "tail: one transcript short",
    "tail: one exon short", "tail: trBest of a read behind the first 256", "tail: read with a partner", "tail: CUR_FLAGS set before the launches"};
static u64 nClass[N_CLASSES];
static long refBad = 0;                  // contradictions on the reference side (a restatement against another)

// ---- A --------------------------------------------------------------------------------------------------------------------------------------------------------------------
static void packCase(TrsSet &S, u32 packWords, u32 nReads) {
    TrsPack c; memset(&c, 0, sizeof(c)); c.packWords = packWords; c.nReads = nReads; c.offOff = (u32)S.packOffset.size(); c.baseOff = (u32)S.packBases.size(); c.expOff = (u32)S.packExp.size();
    const u32 full = 8 * packWords; const u32 LEN[10] = {0, 1, 7, 8, 9, 63, 64, 65, full - 1, full};
    nClass[packWords == 1 ? P_WORDS_1 : packWords == 13 ? P_WORDS_13 : packWords == 64 ? P_WORDS_64 : P_WORDS_65]++; if (nReads == 70) nClass[P_READS_70]++;
    u64 at = 0; S.packOffset.push_back(0);
    for (u32 r = 0; r < nReads; r++) {
        u32 L = r < 10 ? LEN[r] : rnd(full + 1); if (nReads == 1) L = LEN[rnd(10)]; if (L > full) L = full;
        if (L == 0) nClass[P_LEN_0]++; if (L == 1) nClass[P_LEN_1]++; if (L == full - 1) nClass[P_LEN_FULL_M1]++; if (L == full) nClass[P_LEN_FULL]++;
        std::vector<u8> b(L); for (u32 j = 0; j < L; j++) { b[j] = (u8)(rnd(3) ? rnd(256) : rnd(5)); if (b[j] > 15) nClass[P_HIGH_BITS]++; }
        // the definition: nibble k of word w is base 8 w + k of the read, 15 behind its end
        for (u32 w = 0; w < packWords; w++) { u32 v = 0; for (u32 k = 0; k < 8; k++) { const u32 j = 8 * w + k; v |= (j < L ? (u32)(b[j] & 15u) : 15u) << (4 * k); } S.packExp.push_back(v); }
        S.packBases.insert(S.packBases.end(), b.begin(), b.end()); at += L; S.packOffset.push_back(at);
    }
    c.nBases = (u32)at; S.pack.push_back(c);
}

// ---- E --------------------------------------------------------------------------------------------------------------------------------------------------------------------
static void scanCase(TrsSet &S, u32 nBlocks, u32 flavour) {          // flavour 0: zeros, 1: small, 2: large (the sums stay below 2^32)
    TrsScan c; memset(&c, 0, sizeof(c)); c.nBlocks = nBlocks; c.totOff = (u32)S.scanTot.size();
    static const u32 NB[9] = {1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 5000}; for (u32 k = 0; k < 9; k++) if (NB[k] == nBlocks) nClass[S_OFF_1 + k]++;
    const u32 lim = 0xFFFFFFFFu / nBlocks; u64 sT = 0, sE = 0; std::vector<u32> v(2 * (size_t)nBlocks);
    for (u32 k = 0; k < 2 * nBlocks; k++) v[k] = flavour == 0 ? 0 : flavour == 1 ? rnd(rnd(4) ? 700 : 2) : lim - rnd(lim / 4 + 1);
    for (u32 k = 0; k < nBlocks; k++) { S.scanExp.push_back((u32)sT); S.scanExp.push_back((u32)sE); sT += v[2 * k]; sE += v[2 * k + 1]; }          // exclusive prefix sums of the pairs
    S.scanExp.push_back((u32)sT); S.scanExp.push_back((u32)sE);
    if (sT >> 32 || sE >> 32) { printf("scan case: a sum does not fit 32 bits\n"); refBad++; }
    if (flavour == 0) nClass[S_ZEROS]++; if (sT >> 31) nClass[S_LARGE]++;
    S.scanTot.insert(S.scanTot.end(), v.begin(), v.end()); S.scan.push_back(c);
}
static TrsBatch newBatch(TrsSet &S, u32 kind, u32 env) {
    TrsBatch b; memset(&b, 0, sizeof(b)); b.kind = kind; b.env = env; b.readOff = (u32)S.read.size(); b.woutOff = (u32)S.wout.size(); b.trOff = (u32)S.tr.size(); b.exOff = (u32)S.ex.size(); b.candOff = S.cand.size();
    b.listOff = (u32)S.list.size(); b.expReadOff = (u32)S.readExp.size(); b.expWoutOff = (u32)S.woutExp.size(); b.expListOff = (u32)S.listExp.size(); b.expWinOff = (u32)S.winExp.size(); b.expRROff = (u32)S.rrExp.size();
    b.expOutTrOff = (u32)S.outTr.size(); b.expOutExOff = (u32)S.outEx.size(); b.expScanOff = (u32)S.scanLocalExp.size(); b.lenOff = (u32)S.readLen.size();
    return b;
}
// the reads' lengths as offsets (nReads + 1), mate1Length beside S.read
static void closeReads(TrsSet &S, TrsBatch &b, const std::vector<u32> &Lread, const std::vector<u32> &len0) {
    b.nReads = (u32)Lread.size(); u64 at = 0; S.readLen.push_back(0); for (u32 r = 0; r < b.nReads; r++) { at += Lread[r]; S.readLen.push_back(at); S.mate1.push_back((u16)len0[r]); }
    while (S.mate1.size() < S.read.size()) S.mate1.push_back(0);
}
static void scanLocalCase(TrsSet &S, u32 nReads) {
    TrsBatch b = newBatch(S, TRS_SCANLOCAL, 0); static const u32 NR[5] = {1, 255, 256, 257, 1000}; for (u32 k = 0; k < 5; k++) if (NR[k] == nReads) nClass[S_LOCAL_1 + k]++;
    std::vector<u32> L(nReads, 0), l0(nReads, 0);
    for (u32 r = 0; r < nReads; r++) { DRead d; memset(&d, 0x5A, sizeof(d)); d.nTr = rnd(5) ? rnd(6) : rnd(3) ? 0 : 3000000 + rnd(1000); d.nEx = d.nTr + rnd(2 * d.nTr + 1); S.read.push_back(d); }
    closeReads(S, b, L, l0);
    // the definition: within every block of 256 reads the exclusive prefix sums, and the block's totals
    std::vector<u32> tb(nReads), eb(nReads), bt(2 * ((nReads + 255) / 256), 0);
    for (u32 r = 0; r < nReads; r++) { const DRead &d = S.read[b.readOff + r]; tb[r] = bt[2 * (r / 256)]; eb[r] = bt[2 * (r / 256) + 1]; bt[2 * (r / 256)] += d.nTr; bt[2 * (r / 256) + 1] += d.nEx; }
    S.scanLocalExp.insert(S.scanLocalExp.end(), tb.begin(), tb.end()); S.scanLocalExp.insert(S.scanLocalExp.end(), eb.begin(), eb.end()); S.scanLocalExp.insert(S.scanLocalExp.end(), bt.begin(), bt.end());
    S.batch.push_back(b);
}

// ---- B --------------------------------------------------------------------------------------------------------------------------------------------------------------------
static void verifyCase(TrsSet &S, u32 nReads) {
    TrsBatch b = newBatch(S, TRS_VERIFY, 0); nClass[nReads == 1 ? V_NREADS_1 : nReads == 256 ? V_NREADS_256 : nReads == 257 ? V_NREADS_257 : V_NREADS_600]++;
    std::vector<u32> L(nReads, 100), l0(nReads, 100), redo, replay; static const u32 NW[5] = {0, 1, 2, 5, 70};
    for (u32 r = 0; r < nReads; r++) {
        DRead d; memset(&d, 0x5A, sizeof(d)); d.nWin = nReads <= 2 ? NW[1 + rnd(4)] : rnd(40) == 0 ? 70 : NW[rnd(4)]; if (nReads > 2 && r == 3) d.nWin = 70; if (nReads > 2 && r == 5) d.nWin = 0;
        if (rnd(4) == 0) for (u32 k = rnd(3); k; k--) { DWinOut o; memset(&o, 0x3C, sizeof(o)); S.wout.push_back(o); S.woutExp.push_back(o); }          // places that belong to no read
        d.winOffset = (u32)S.wout.size() - b.woutOff;
        nClass[d.nWin == 0 ? V_NWIN_0 : d.nWin == 1 ? V_NWIN_1 : d.nWin == 70 ? V_NWIN_70 : V_NWIN_1 + 0]++; if (d.nWin > 1 && d.winOffset < 256 && d.winOffset + d.nWin > 256) nClass[V_STRADDLE]++;
        // star_oracle.cpp:702-706 / DESIGN.md 5.4: the incoming value of a window is the maximum of 0 and mm[f] of the windows before it; queued iff sens[f] is smaller for some f
        i32 M[2] = {0, 0};
        for (u32 k = 0; k < d.nWin; k++) {
            DWinOut o; randomBytes(&o, sizeof(o)); static const i32 MM[6] = {-5, 0, 3, 7, 10, 12};
            for (int f = 0; f < 2; f++) { o.mm[f] = MM[rnd(6)]; const u32 h = rnd(6); o.sens[f] = h == 0 ? M[f] : h == 1 ? M[f] - 1 : h == 2 ? M[f] + 1 : h == 3 ? 0 : INT_MAX; o.minIn[f] = (i32)rnd(3) * 4; }
            o.nCand = rnd(2) ? 0xFFFFFFFFu : rnd(30);
            DWinOut e = o; const bool q0 = o.sens[0] < M[0], q1 = o.sens[1] < M[1];
            for (int f = 0; f < 2; f++) { if (o.sens[f] == M[f] && M[f] > 0) nClass[V_SENS_EQ]++; if (o.sens[f] == M[f] - 1) nClass[V_SENS_BELOW1]++; if (o.mm[f] < 0) nClass[V_NEG_MM]++; }
            if (o.sens[0] == INT_MAX && o.sens[1] == INT_MAX && (M[0] > 0 || M[1] > 0)) nClass[V_SENS_MAX]++; if (q0 != q1) nClass[V_ONE_MATE]++;
            if (q0 || q1) { e.minIn[0] = M[0]; e.minIn[1] = M[1]; const u32 w = (u32)S.wout.size() - b.woutOff; if (o.nCand == 0xFFFFFFFFu) { redo.push_back(w); nClass[V_REDO]++; } else { replay.push_back(w); nClass[V_REPLAY]++; } }
            M[0] = std::max(M[0], o.mm[0]); M[1] = std::max(M[1], o.mm[1]);
            S.wout.push_back(o); S.woutExp.push_back(e);
        }
        S.read.push_back(d);
    }
    closeReads(S, b, L, l0); b.nWout = (u32)S.wout.size() - b.woutOff;
    std::sort(redo.begin(), redo.end()); std::sort(replay.begin(), replay.end()); b.expNRedo = (u32)redo.size(); b.expNReplay = (u32)replay.size();
    S.listExp.insert(S.listExp.end(), redo.begin(), redo.end()); S.listExp.insert(S.listExp.end(), replay.begin(), replay.end());
    S.batch.push_back(b);
}

// ---- transcripts made by hand ---------------------------------------------------------------------------------------------------------------------------------------------
struct Seg { u32 R, L; };
struct ReadShape { u32 Lread, len0; bool paired; };
// motif: 0 none, 1 intronMotifs[1], 2 intronMotifs[2], 3 intronMotifs[0], 4 both
static Tr makeTr(const ReadShape &rs, u32 chr, u32 str, int score, u64 gLength, const std::vector<Seg> &segs, u64 diag, u32 motif) {
    Tr t; memset(&t, 0, sizeof(t)); t.nExons = segs.size();
    for (u32 k = 0; k < segs.size(); k++) {
        t.ex[k][EX_R] = segs[k].R; t.ex[k][EX_L] = segs[k].L; t.ex[k][EX_G] = diag + 5000ull * k + segs[k].R; t.ex[k][EX_iFrag] = rs.paired && segs[k].R > rs.len0 ? 1 : 0; t.ex[k][EX_sjA] = rnd(5) ? (u64)-1 : rnd(100);
        t.shiftSJ[k][0] = rnd(5); t.shiftSJ[k][1] = rnd(5); t.sjAnnot[k] = (uint8_t)rnd(2); t.sjStr[k] = (uint8_t)rnd(3); t.mappedLength += segs[k].L;
    }
    for (u32 k = 0; k + 1 < segs.size(); k++) t.canonSJ[k] = t.ex[k][EX_iFrag] != t.ex[k + 1][EX_iFrag] ? -3 : (int)rnd(6) - 2;
    t.intronMotifs[0] = motif == 3 ? 1 : 0; t.intronMotifs[1] = motif == 1 || motif == 4 ? 2 : 0; t.intronMotifs[2] = motif == 2 || motif == 4 ? 1 : 0; t.sjMotifStrand = (uint8_t)rnd(3);
    const Seg &a = segs[0], &z = segs.back();
    t.iFrag = t.ex[0][EX_iFrag] == t.ex[segs.size() - 1][EX_iFrag] ? (int)t.ex[0][EX_iFrag] : -1;
    t.rStart = a.R; t.rLength = z.R + z.L - a.R; t.roStart = str == 0 ? t.rStart : rs.Lread - t.rStart - t.rLength; t.gStart = t.ex[0][EX_G]; t.gLength = gLength; t.Chr = chr; t.Str = str; t.roStr = str;
    t.nMatch = rnd(200); t.nMM = rnd(10); t.maxScore = score; t.nGap = rnd(3); t.lGap = rnd(1000); t.nDel = rnd(3); t.nIns = rnd(3); t.lDel = rnd(9); t.lIns = rnd(9); t.nUnique = rnd(10); t.nAnchor = rnd(10);
    return t;
}
static std::vector<Seg> randomSegs(const ReadShape &rs, u32 neMax) {
    const u32 ne = 1 + rnd(neMax); std::vector<u32> cut; while (cut.size() < 2 * ne) { const u32 p = rnd(rs.Lread + 1); if (std::find(cut.begin(), cut.end(), p) == cut.end() && !(rs.paired && p == rs.len0)) cut.push_back(p); }
    std::sort(cut.begin(), cut.end()); std::vector<Seg> s; for (u32 k = 0; k < ne; k++) s.push_back(Seg{cut[2 * k], cut[2 * k + 1] - cut[2 * k]}); return s;
}
static void sortBestFirst(std::vector<Tr> &w) { std::stable_sort(w.begin(), w.end(), [](const Tr &a, const Tr &b) { return a.maxScore > b.maxScore || (a.maxScore == b.maxScore && a.gLength < b.gLength); }); }
// the records of one window as the stitch kernels leave them in the pools: Oracle::emitRead on the window alone (exonOffset relative to the window)
static void windowRecords(const std::vector<Tr> &w, std::vector<staramd_transcript> &tr, std::vector<staramd_exon> &ex) {
    tr.clear(); ex.clear(); if (w.empty()) return;
    staramd_params P0; memset(&P0, 0, sizeof(P0)); staramd_read_result rr; memset(&rr, 0, sizeof(rr)); std::vector<std::vector<Tr>> one(1, w); Oracle::emitRead(one, -1, P0, rr, tr, ex);
}

struct FWin { std::vector<Tr> tr; i32 mm[2] = {0, 0}; bool log = false; std::vector<Tr> candTr; std::vector<Cand> cand; };
struct FRead { ReadShape rs; std::vector<FWin> win; u32 status = 0, nSeeds = 5, unmapped = 0; };

// ---- the restatements ---------------------------------------------------------------------------------------------------------------------------------------------------------
struct PartnerExp { int scoreBest = 0, scoreNext = 0; u32 strBest = 0; i32 idx = -1; };
// partnerOverWindows (star_amd/csrc/host/chimeric.cpp:271-299; ReadAlign_chimericDetectionOld.cpp:45-97) over the arrays of resultSelect 0: the head of every other window and the
// other alignments of trBest's own; the runner-up counts only when it shares no block with the best so far
static PartnerExp partnerExpect(const staramd_params &P, const ReadShape &rs, const std::vector<staramd_transcript> &T, const std::vector<staramd_exon> &X, i32 trBest, bool classify) {
    PartnerExp p; const staramd_transcript &m = T[trBest]; const staramd_exon *mx = X.data() + m.exonOffset; i32 best = -1; bool any = false;
    const ChimExtent me = chimExtent(m.Str, mx[0], mx[m.nExons - 1], rs.Lread, rs.len0); const u32 mStr = chimMotifStrand(m.Str, m.intronMotifs, false);
    for (u32 k0 = 0; k0 < T.size();) {
        u32 k1 = k0; while (k1 < T.size() && T[k1].iW == T[k0].iW) k1++;
        const bool bestWindow = (u32)trBest == k0;
        for (u32 k = k0; k < k1; k++) {
            const u32 iWt = k - k0; if (!bestWindow && iWt > 0) break; if (bestWindow && iWt == 0) continue;
            if (T[k].intronMotifs[0] > 0) { if (classify) nClass[F_PARTNER_MOTIF0]++; continue; }
            const staramd_exon *x = X.data() + T[k].exonOffset; const u32 sStr = chimMotifStrand(T[k].Str, T[k].intronMotifs, false);
            if (mStr != 0 && sStr != 0 && mStr != sStr) { if (classify) nClass[F_PARTNER_STRAND]++; continue; }
            const u64 rawS = T[k].Str == 0 ? (u64)x[0].R : rs.Lread - x[T[k].nExons - 1].R - x[T[k].nExons - 1].L; if (classify && rs.paired && rawS > rs.len0) nClass[F_PARTNER_SPACER]++;
            u64 chimOverlap; if (!chimPairEligible(me, chimExtent(T[k].Str, x[0], x[T[k].nExons - 1], rs.Lread, rs.len0), rs.len0, P.chimSegmentMin, P.chimSegmentReadGapMax, chimOverlap)) continue;
            const int chimScore = m.maxScore + T[k].maxScore - (int)chimOverlap; u64 overlap1 = 0;
            if (classify && iWt == 0 && p.scoreBest > 0 && blocksOverlap(X.data() + T[best].exonOffset, (u32)T[best].nExons, x, (u32)T[k].nExons) != 0) nClass[F_PARTNER_CROSS_SHARED]++;          // (:84: only two alignments of one window are compared)
            if (iWt > 0 && p.scoreBest > 0) { overlap1 = blocksOverlap(X.data() + T[best].exonOffset, (u32)T[best].nExons, x, (u32)T[k].nExons); if (classify) nClass[overlap1 ? F_PARTNER_OVERLAP1 : F_PARTNER_NO_OVERLAP1]++; }
            if (chimScore > p.scoreBest) { best = (i32)k; any = true; if (overlap1 == 0) p.scoreNext = p.scoreBest; p.scoreBest = chimScore; p.strBest = sStr; }
            else if (chimScore > p.scoreNext && overlap1 == 0) p.scoreNext = chimScore;
        }
        k0 = k1;
    }
    p.idx = any ? best : -1; return p;
}

struct FinishExp { DRead rd; std::vector<u32> nTr, nEx; staramd_read_result rr; std::vector<staramd_transcript> otr; std::vector<staramd_exon> oex; bool partner = false; };
// what k_stitch_finish and k_gather must make of a read: star_oracle.cpp:827-850 over the lists (trBest with its gLength tie-break, the per-read limit, no good window), then
// Oracle::emitRead for the layout and the selection.  `lists`: the final list of every window (a replayed window: its sequential list).  rr.trOffset / exonOffset start at 0
static FinishExp finishExpect(const staramd_params &P, const FRead &R, const DRead &in, const std::vector<std::vector<Tr>> &lists, bool classify) {
    FinishExp E; E.rd = in; const u32 nWin = (u32)lists.size(); E.nTr.resize(nWin); E.nEx.resize(nWin);
    for (u32 w = 0; w < nWin; w++) { E.nTr[w] = (u32)lists[w].size(); E.nEx[w] = 0; for (const Tr &t : lists[w]) E.nEx[w] += (u32)t.nExons; }
    memset(&E.rr, 0, sizeof(E.rr)); E.rr.trBest = -1; E.rr.status = in.status; E.rr.unmappedLength = in.unmappedLength; E.rr.maxScoreMate[0] = in.maxScoreMate[0]; E.rr.maxScoreMate[1] = in.maxScoreMate[1];
    if (nWin == 0) {
        // star_oracle.cpp:850 with no window at all; a read without seeds was classified before stitchPieces (:898-901), one whose work space overflowed has no result
        if (in.nSeeds > 0 && !(in.status & (STARAMD_ST_SCRATCH_OVERFLOW | STARAMD_ST_NO_GOOD_WINDOW))) E.rd.status |= STARAMD_ST_NO_GOOD_WINDOW;
        if (classify) nClass[in.status & STARAMD_ST_SCRATCH_OVERFLOW ? F_NWIN0_SCRATCH : in.status & STARAMD_ST_NO_GOOD_WINDOW ? F_NWIN0_NOGOOD : in.status & STARAMD_ST_TOO_MANY_ANCHORS ? F_NWIN0_TOOMANY : in.nSeeds ? F_NWIN0_SEEDS : F_NWIN0_NOSEEDS]++;
        E.rr.status = E.rd.status; return E;
    }
    u32 status = in.status; std::vector<std::vector<Tr>> trAll; std::vector<u32> winOf; int bw = -1, bestScore = 0; u64 bestGlen = 0, trN = 0; i32 M[2] = {0, 0}; bool allEmpty = true;
    for (u32 w = 0; w < nWin; w++) {
        const u64 v = trN + P.alignTranscriptsPerWindowNmax;
        if (classify) { if (v == P.alignTranscriptsPerReadNmax) nClass[w == 0 ? F_LIMIT_FIRST : F_LIMIT_EXACT]++; else if (v + 1 == P.alignTranscriptsPerReadNmax) nClass[F_LIMIT_BELOW]++; else if (v > P.alignTranscriptsPerReadNmax) nClass[w == 0 ? F_LIMIT_FIRST : F_LIMIT_ABOVE]++; }
        if (v >= P.alignTranscriptsPerReadNmax) { status |= STARAMD_ST_TR_PER_READ_LIMIT; for (u32 k = w; k < nWin; k++) E.nTr[k] = E.nEx[k] = 0; break; }          // :834; the windows behind it are not walked
        M[0] = std::max(M[0], R.win[w].mm[0]); M[1] = std::max(M[1], R.win[w].mm[1]);                                                                                  // :702 over the leaves of every window walked
        if (lists[w].empty()) continue;
        allEmpty = false; const Tr &h = lists[w][0];
        if (classify && bw >= 0 && h.maxScore == bestScore) nClass[h.gLength < bestGlen ? F_TIE_LATER_SMALLER : h.gLength > bestGlen ? F_TIE_LATER_LARGER : F_TIE_EQUAL]++;
        if (h.maxScore > bestScore || (h.maxScore == bestScore && h.gLength < bestGlen)) { bw = (int)trAll.size(); bestScore = h.maxScore; bestGlen = h.gLength; }   // :843
        trAll.push_back(lists[w]); winOf.push_back(w); trN += lists[w].size();
    }
    if (classify) { if (allEmpty) nClass[F_ALL_EMPTY]++; else if (bestScore == 0) nClass[F_BEST0]++; if (bw >= 0) for (u32 w = 0; w < winOf[bw]; w++) if (lists[w].empty()) { nClass[F_BEST_BEHIND_EMPTY]++; break; } }
    if (bestScore == 0) { status |= STARAMD_ST_NO_GOOD_WINDOW; trAll.clear(); winOf.clear(); bw = -1; }                                                                // :850
    E.rr.status = status; E.rr.maxScoreMate[0] = M[0]; E.rr.maxScoreMate[1] = M[1];
    staramd_params Pe = P;
    if (P.resultSelect && bw >= 0) {
        // the prefix of every window multMapSelect can pick from (ReadAlign_multMapSelect.cpp:26-44, as Oracle::emitRead states it); resultSelect 2 with chimeric detection: and
        // the partner, the prefix of its window reaching up to it (include/star_amd.h)
        const int selMin = trAll[bw][0].maxScore - P.outFilterMultimapScoreRange; std::vector<u32> keep(trAll.size());
        for (u32 o = 0; o < trAll.size(); o++) { u32 n = 0; while (n < trAll[o].size() && trAll[o][n].maxScore >= selMin) n++; keep[o] = n; }
        PartnerExp pe; u32 pOrd = 0, pRank = 0; std::vector<staramd_transcript> t0; std::vector<staramd_exon> x0;
        if (P.resultSelect == 2 && P.chimSegmentMinPositive && P.chimSegmentMin > 0) {
            staramd_params P0 = P; P0.resultSelect = 0; staramd_read_result r0; memset(&r0, 0, sizeof(r0)); r0.trBest = -1; Oracle::emitRead(trAll, bw, P0, r0, t0, x0);
            pe = partnerExpect(P, R.rs, t0, x0, r0.trBest, classify);
            if (pe.idx >= 0) { pOrd = t0[pe.idx].iW; u32 first = 0; while (t0[first].iW != pOrd) first++; pRank = (u32)pe.idx - first;
                if (classify) { if ((int)pOrd != bw && t0[pe.idx].maxScore < selMin) nClass[F_PARTNER_OTHER_WIN]++; if ((int)pOrd == bw && t0[pe.idx].maxScore < selMin) nClass[F_PARTNER_RANK]++; }
                keep[pOrd] = std::max(keep[pOrd], pRank + 1); E.partner = true; }
            else if (classify) nClass[F_PARTNER_NONE]++;
        } else if (classify && P.resultSelect == 2) nClass[F_CHIM0_SEL2]++;
        if (classify) for (u32 o = 0; o < trAll.size(); o++) { if (keep[o] == 0) nClass[(int)o < bw ? F_PREFIX_EMPTIES_BEFORE : F_PREFIX_EMPTIES_AFTER]++; if ((int)o == bw && keep[o] < trAll[o].size()) nClass[F_PREFIX_CUTS_BEST]++; }
        for (u32 o = 0; o < trAll.size(); o++) { const u32 w = winOf[o]; E.nTr[w] = keep[o]; E.nEx[w] = 0; for (u32 k = 0; k < keep[o]; k++) E.nEx[w] += (u32)trAll[o][k].nExons; }
        if (E.partner) {
            // the arrays: the kept prefixes laid out by emitRead (nothing left for it to select)
            std::vector<std::vector<Tr>> cut; int bw2 = -1; u32 idx2 = 0; for (u32 o = 0; o < trAll.size(); o++) { if (!keep[o]) continue; if ((int)o == bw) bw2 = (int)cut.size(); if (o == pOrd) idx2 += pRank; else if (o < pOrd) idx2 += keep[o]; cut.push_back(std::vector<Tr>(trAll[o].begin(), trAll[o].begin() + keep[o])); }
            trAll = cut; bw = bw2; Pe.resultSelect = 0;
            E.rr.status |= STARAMD_ST_CHIM_PARTNER; E.rr.maxScoreMate[0] = pe.scoreBest; E.rr.maxScoreMate[1] = pe.scoreNext; E.rr.unmappedLength = idx2 | (pe.strBest << 30);
            Oracle::emitRead(trAll, bw, Pe, E.rr, E.otr, E.oex);
            // the index must name, in what is returned, the host's partner (iW and exonOffset are those of the arrays it lies in)
            staramd_transcript a = E.otr[idx2], c = t0[pe.idx]; a.iW = c.iW = 0; a.exonOffset = c.exonOffset = 0;
            if (memcmp(&a, &c, sizeof(a)) != 0 || memcmp(E.oex.data() + E.otr[idx2].exonOffset, x0.data() + t0[pe.idx].exonOffset, 32u * c.nExons) != 0) { printf("reference side: the partner's index does not name the host's partner\n"); refBad++; }
        } else { Oracle::emitRead(trAll, bw, Pe, E.rr, E.otr, E.oex); E.rr.maxScoreMate[0] = E.rr.maxScoreMate[1] = 0; }          // the ABI's rule (star_oracle.cpp mapOneRead: 0 under resultSelect)
        u32 sum = 0; for (u32 w = 0; w < nWin; w++) sum += E.nTr[w]; if (sum != E.rr.nTr) { printf("reference side: the prefixes hold %u transcripts, emitRead returned %u\n", sum, E.rr.nTr); refBad++; }
    } else Oracle::emitRead(trAll, bw, Pe, E.rr, E.otr, E.oex);
    if (bestScore == 0 && P.resultSelect) E.rr.maxScoreMate[0] = E.rr.maxScoreMate[1] = 0;
    E.rd.status = E.rr.status & ~(u32)STARAMD_ST_MAPPED_WINDOWS; E.rd.nWt = E.rr.nW; E.rd.nTr = E.rr.nTr; E.rd.nEx = (u32)E.oex.size(); E.rd.bestW = E.rr.trBest >= 0 ? (i32)E.otr[E.rr.trBest].iW : -1;
    E.rd.maxScoreMate[0] = E.rr.maxScoreMate[0]; E.rd.maxScoreMate[1] = E.rr.maxScoreMate[1]; E.rd.unmappedLength = E.rr.unmappedLength;
    return E;
}

// ---- reads made by hand -------------------------------------------------------------------------------------------------------------------------------------------------------
static ReadShape shapeOf(const staramd_params &P) { ReadShape rs; rs.paired = P.readNmates == 2; if (rs.paired) { rs.len0 = 60 + rnd(60); rs.Lread = rs.len0 + 1 + 60 + rnd(60); } else { rs.Lread = 80 + rnd(120); rs.len0 = rs.Lread; } return rs; }
static FWin plainWindow(const ReadShape &rs, const staramd_params &P, u32 nTr, int scoreLo, int scoreSpan, u32 chr) {
    FWin w; const u32 str = rnd(2); static const u64 GL[4] = {100, 200, 300, 70000};
    for (u32 k = 0; k < nTr; k++) w.tr.push_back(makeTr(rs, chr, str, scoreLo + (int)rnd(scoreSpan), GL[rnd(4)], randomSegs(rs, rnd(8) ? 3 : rnd(4) ? 6 : STARAMD_MAX_N_EXONS), 100000 + 7000ull * rnd(50), rnd(6) == 0 ? 1 + rnd(4) : 0));
    sortBestFirst(w.tr); w.mm[0] = rnd(3) ? (i32)rnd(70) : 0; w.mm[1] = rs.paired && rnd(2) ? (i32)rnd(70) : 0; (void)P; return w;
}
// a window with a candidate log: its candidates are transcripts laid out as records, so that the list a replay leaves can go through Oracle::emitRead like any other
static FWin logWindow(const ReadShape &rs, const staramd_params &P, u32 nCand, u32 chr) {
    FWin w; w.log = true; const u32 str = rnd(2), fam = rnd(3); u64 diag[4]; for (int d = 0; d < 4; d++) diag[d] = 200000 + 9000ull * d;
    for (u32 k = 0; k < nCand; k++) {
        std::vector<Seg> segs = randomSegs(rs, rnd(3) ? 2 : CAND_NE_MAX); int score = 0; for (const Seg &s : segs) score += (int)s.L; score = fam == 2 ? 40 + (int)rnd(4) : std::max(1, score - (int)rnd(3));
        Tr t = makeTr(rs, chr, str, score, 100 + rnd(fam == 1 ? 4 : 3000), segs, fam == 0 ? diag[rnd(2)] : 300000 + 11000ull * k, 0);
        if (fam == 0) for (u32 e = 0; e < t.nExons; e++) t.ex[e][EX_G] = diag[rnd(2)] + t.ex[e][EX_R];          // few diagonals: overlaps, removals, blocks
        t.gStart = t.ex[0][EX_G]; w.candTr.push_back(t);
        std::vector<staramd_transcript> tr; std::vector<staramd_exon> ex; windowRecords(std::vector<Tr>(1, t), tr, ex);
        Cand c; memset(&c, 0, sizeof(c)); c.t = tr[0]; c.t.iW = 0xC0DE0000u + k; c.t.exonOffset = 0xE0E0E0E0u; for (u32 e = 0; e < ex.size(); e++) c.ex[e] = ex[e]; w.cand.push_back(c);
        if (t.iFrag >= 0) w.mm[t.iFrag] = std::max(w.mm[t.iFrag], score);
    }
    (void)P; return w;
}
static std::vector<Tr> listOf(const FWin &w, const std::vector<u32> &list) { std::vector<Tr> v; for (u32 id : list) v.push_back(w.candTr[id]); return v; }

static FRead makeRead(const staramd_params &P, u32 scenario) {
    FRead R; R.rs = shapeOf(P); const ReadShape &rs = R.rs; const u32 perWin = P.alignTranscriptsPerWindowNmax; const bool tight = P.alignTranscriptsPerReadNmax < 100;
    R.unmapped = rnd(200); R.nSeeds = 1 + rnd(20);
    const auto nTrOf = [&]() { return 1 + rnd(std::min(perWin, 4u)); };
    if (scenario == 1) { const u32 h = rnd(5); R.nSeeds = h == 1 ? 0 : R.nSeeds; R.status = h == 2 ? STARAMD_ST_SCRATCH_OVERFLOW : h == 3 ? STARAMD_ST_NO_GOOD_WINDOW : h == 4 ? STARAMD_ST_TOO_MANY_ANCHORS : 0; return R; }
    if (scenario == 2) { for (u32 k = 1 + rnd(4); k; k--) R.win.push_back(plainWindow(rs, P, 0, 0, 1, 0)); return R; }
    if (scenario == 3) { for (u32 k = 1 + rnd(3); k; k--) R.win.push_back(plainWindow(rs, P, rnd(3) ? 1 : 0, 0, 1, k)); return R; }
    if (scenario == 4) {          // equal head scores, empty windows in front
        for (u32 k = rnd(3); k; k--) R.win.push_back(plainWindow(rs, P, 0, 0, 1, 0));
        const u32 n = 2 + rnd(3); for (u32 k = 0; k < n; k++) { R.win.push_back(plainWindow(rs, P, nTrOf(), 55, 1, k)); if (rnd(3) == 0) R.win.push_back(plainWindow(rs, P, 0, 0, 1, 0)); }
        return R;
    }
    if (scenario == 5 && P.resultSelect == 2) {          // chimeric layouts: a main segment and others placed around it
        const u32 str = rnd(2), a = rs.paired && rnd(2) ? rs.len0 + 1 + rnd(10) : rnd(10), mainL = 40 + rnd(15), sub = rnd(3) ? rnd(10) : 5 + rnd(2);
        const auto seg1 = [&](u32 r, u32 l) { std::vector<Seg> s; if (r + l > rs.Lread) l = rs.Lread - r; s.push_back(Seg{r, l}); return s; };
        // (read coordinates are those of the transcript's strand: a window on strand 1 covers [R, R + L) of the reversed read, which chimExtent turns round)
        FWin best; best.tr.push_back(makeTr(rs, 1, str, 60, 500, seg1(a, mainL), 400000, sub == 3 ? 1 : 0));
        const u32 pa = a + mainL < rs.Lread - 30 ? a + mainL + rnd(3) : (a > 35 ? a - 35 : 0), pl = 25 + rnd(8);
        const u32 pstr = rnd(4) ? str : str ^ 1u; const u32 par = pstr == str ? pa : (rs.Lread > pa + pl ? rs.Lread - pa - pl : 0);
        if (sub == 1 || sub == 5 || sub == 6) {          // the partner inside the best window, behind a transcript no chimera can use
            best.tr.push_back(makeTr(rs, 1, str, 55 - (int)rnd(3), 600, seg1(a, mainL - 5), 400000, 0));
            best.tr.push_back(makeTr(rs, 1, str, 40, 300, seg1(pa, pl), 410000, 0));
            if (sub == 5) best.tr.push_back(makeTr(rs, 1, str, 38, 300, seg1(pa, pl - 4), 410000, 0));          // same diagonal as the partner: shares its block
            if (sub == 6) best.tr.push_back(makeTr(rs, 1, str, 38, 300, seg1(pa, pl - 4), 420000, 0));          // another diagonal: shares none
        }
        for (u32 k = rnd(2); k; k--) R.win.push_back(plainWindow(rs, P, rnd(2), 20, 10, 7));
        const bool bestFirst = rnd(2); if (bestFirst) R.win.push_back(best);
        if (sub != 1 && sub != 2) { FWin o; o.tr.push_back(makeTr(rs, 2, pstr, sub == 7 ? 59 : 30 + (int)rnd(12), 200, seg1(par, pl), 500000, sub == 3 ? 2 : sub == 4 ? 3 : 0)); if (rnd(2)) o.tr.push_back(makeTr(rs, 2, pstr, 25, 200, seg1(par, pl - 3), 500000, 0)); R.win.push_back(o); }
        if (sub == 2) { FWin o; o.tr.push_back(makeTr(rs, 2, str, 50, 200, seg1(a, mainL - 2), 500000, 0)); R.win.push_back(o); }          // covers what the main segment covers: not eligible
        if (sub == 8) { FWin o; o.tr.push_back(makeTr(rs, 3, pstr, 28 + (int)rnd(12), 250, seg1(par, pl), 600000, 0)); R.win.push_back(o); }
        if (sub == 9) { FWin o; o.tr.push_back(makeTr(rs, 2, pstr, 26 + (int)rnd(16), 250, seg1(par, pl - rnd(3)), 500000, 0)); R.win.push_back(o); }          // a second window on the diagonal of the first
        if (!bestFirst) R.win.push_back(best);
        for (FWin &w : R.win) { sortBestFirst(w.tr); w.mm[0] = (i32)rnd(60); }
        return R;
    }
    // anything: windows of few transcripts, empty ones between them; scores close together (ties) or spread out (prefixes); in the tight environments enough windows to meet the limit
    const u32 nWin = tight ? 2 + rnd(8) : 1 + rnd(6); const bool spread = rnd(2);
    for (u32 k = 0; k < nWin; k++) R.win.push_back(rnd(4) == 0 ? plainWindow(rs, P, 0, 0, 1, 0) : plainWindow(rs, P, tight ? 1 + rnd(perWin) : nTrOf(), spread ? 30 : 54, spread ? 30 : 3, k));
    return R;
}

// one batch of reads into the set, the blocks of the windows in the pools in any order, with what finish (chainKind false: over the pass-0 lists as they are) or the whole tail
// (chainKind true: windows with logs replayed under their true incoming maxScoreMate where verify queues them) must make of it
struct BatchFacts { bool secondBlock = false, partner = false; u32 nQueued = 0; };
static BatchFacts buildBatch(TrsSet &S, TrsBatch &b, const staramd_params &P, const std::vector<FRead> &reads, bool chainKind, bool classify) {
    BatchFacts F; std::vector<u32> L, l0; struct Place { u32 r, w; }; std::vector<Place> places;
    std::vector<std::vector<std::vector<Tr>>> pass0(reads.size()), fin(reads.size());
    u32 extraTr = 0, extraEx = 0; std::vector<u32> replay;
    for (u32 r = 0; r < reads.size(); r++) {
        const FRead &R = reads[r]; DRead d; memset(&d, 0, sizeof(d)); d.status = R.status; d.nSeeds = R.nSeeds; d.seedOffset = rnd(1000); d.unmappedLength = R.unmapped; d.wtOffset = rnd(50); d.pruneBest = (i32)rnd(100); d.bestW = -1;
        if (rnd(5) == 0) { DWinOut o; memset(&o, 0x3C, sizeof(o)); S.wout.push_back(o); }          // a place that belongs to no read
        d.winOffset = (u32)S.wout.size() - b.woutOff; d.nWin = (u32)R.win.size();
        i32 M[2] = {0, 0};
        for (u32 w = 0; w < R.win.size(); w++) {
            const FWin &W = R.win[w]; DWinOut o; memset(&o, 0, sizeof(o)); o.mm[0] = W.mm[0]; o.mm[1] = W.mm[1]; o.sens[0] = o.sens[1] = INT_MAX; o.nCand = 0xFFFFFFFFu; o.pad = 0x77;
            std::vector<Tr> p0 = W.tr, pf = W.tr;
            if (W.log) {
                const i32 zero[2] = {0, 0}; const u32 Nmax = P.alignTranscriptsPerWindowNmax; const i32 range = P.outFilterMultimapScoreRange; const bool chim = P.chimSegmentMinPositive != 0;
                const CandLogResult a = candLogSequential(W.cand, Nmax, range, chim, zero, 0, nullptr), t = candLogSequential(W.cand, Nmax, range, chim, M, 0, nullptr);
                p0 = listOf(W, a.list); pf = listOf(W, t.list); o.sens[0] = a.sens[0]; o.sens[1] = a.sens[1]; o.nCand = (u32)W.cand.size(); o.candOff32 = (u32)((S.cand.size() - b.candOff) / 32u); candLogBytes(W.cand, S.cand);
                const bool queued = o.sens[0] < M[0] || o.sens[1] < M[1]; const u32 wi = (u32)S.wout.size() - b.woutOff;
                if (queued) { replay.push_back(wi); F.nQueued++; extraTr += (u32)pf.size(); for (const Tr &x : pf) extraEx += (u32)x.nExons; if (classify) nClass[T_QUEUED]++; }
                else { if (classify) nClass[T_NOT_QUEUED_LOG]++; if (a.list != t.list) { printf("reference side: a window whose sens is not below the incoming maxScoreMate has another list under it (DESIGN.md 5.4)\n"); refBad++; } }
            }
            M[0] = std::max(M[0], W.mm[0]); M[1] = std::max(M[1], W.mm[1]);
            pass0[r].push_back(p0); fin[r].push_back(chainKind ? pf : p0);
            if (!p0.empty()) { o.nTr = (u32)p0.size(); o.headScore = p0[0].maxScore; o.headGlen = p0[0].gLength; for (const Tr &x : p0) o.nEx += (u32)x.nExons; places.push_back(Place{r, (u32)S.wout.size()}); }
            S.wout.push_back(o);
        }
        S.read.push_back(d); L.push_back(R.rs.Lread); l0.push_back(R.rs.len0);
    }
    closeReads(S, b, L, l0); b.nWout = (u32)S.wout.size() - b.woutOff; b.candBytes = S.cand.size() - b.candOff;
    for (size_t k = places.size(); k > 1; k--) std::swap(places[k - 1], places[rnd((u32)k)]);
    for (const Place &pl : places) {
        DWinOut &o = S.wout[pl.w]; const DRead &d = S.read[b.readOff + pl.r]; const u32 w = pl.w - b.woutOff - d.winOffset;
        std::vector<staramd_transcript> tr; std::vector<staramd_exon> ex; windowRecords(pass0[pl.r][w], tr, ex);
        o.trOffset = (u32)S.tr.size() - b.trOff; o.exOffset = (u32)S.ex.size() - b.exOff; for (staramd_transcript &t : tr) { t.iW = 0xDEAD0000u + pl.r; S.tr.push_back(t); } S.ex.insert(S.ex.end(), ex.begin(), ex.end());
    }
    b.nTrPool = (u32)S.tr.size() - b.trOff; b.nExPool = (u32)S.ex.size() - b.exOff; b.trCap = b.nTrPool + extraTr; b.exCap = b.nExPool + extraEx;
    // ---- expectations
    S.woutExp.insert(S.woutExp.end(), S.wout.begin() + b.woutOff, S.wout.end());
    u32 trAt = 0;
    for (u32 r = 0; r < reads.size(); r++) {
        const DRead d = S.read[b.readOff + r]; FinishExp E = finishExpect(P, reads[r], d, fin[r], classify);
        S.readExp.push_back(E.rd);
        for (u32 w = 0; w < d.nWin; w++) { DWinOut &e = S.woutExp[b.expWoutOff + d.winOffset + w]; e.nTr = E.nTr[w]; e.nEx = E.nEx[w]; }
        E.rr.trOffset = trAt; const u32 exAt = (u32)S.outEx.size() - b.expOutExOff;
        for (staramd_transcript &t : E.otr) { t.exonOffset += exAt; S.outTr.push_back(t); } S.outEx.insert(S.outEx.end(), E.oex.begin(), E.oex.end());
        if (r >= 256 && E.rr.trBest >= 0 && trAt > 0) F.secondBlock = true; if (E.partner) F.partner = true;
        S.rrExp.push_back(E.rr); trAt += E.rr.nTr;
    }
    b.expTrOut = trAt; b.expNOutTr = trAt; b.expNOutEx = (u32)S.outEx.size() - b.expOutExOff; b.outTrCap = b.expNOutTr; b.outExCap = b.expNOutEx;
    std::sort(replay.begin(), replay.end()); b.expNRedo = 0; b.expNReplay = chainKind ? (u32)replay.size() : 0; if (chainKind) S.listExp.insert(S.listExp.end(), replay.begin(), replay.end());
    b.arenaL = 1024; b.arenaG = 2u * (P.alignTranscriptsPerWindowNmax + 2u) * (REC_HDR + 32u * CAND_NE_MAX);
    return F;
}

// ---- C --------------------------------------------------------------------------------------------------------------------------------------------------------------------
static void replayCase(TrsSet &S, u32 env, u32 nItems, bool withHard, u32 shortTr) {
    const staramd_params &P = S.env[env].P; TrsBatch b = newBatch(S, TRS_REPLAY, env); const u32 Nmax = P.alignTranscriptsPerWindowNmax; const i32 range = P.outFilterMultimapScoreRange; const bool chim = P.chimSegmentMinPositive != 0;
    nClass[nItems == 0 ? R_ITEMS_0 : nItems == 1 ? R_ITEMS_1 : nItems == 3 ? R_ITEMS_3 : R_ITEMS_50]++;
    b.arenaL = 1024; b.arenaG = 8192; ReadShape rs; rs.paired = true; rs.len0 = 75; rs.Lread = 151;
    const u32 nWout = nItems + 3; std::vector<u32> listed; for (u32 w = 0; w < nWout; w++) listed.push_back(w); for (size_t k = nWout; k > 1; k--) std::swap(listed[k - 1], listed[rnd((u32)k)]); listed.resize(nItems);
    std::vector<u8> isListed(nWout, 0); for (u32 w : listed) isListed[w] = 1;
    u32 sumT = 0, sumE = 0; std::vector<TrsWinExp> exp(nWout);
    for (u32 w = 0; w < nWout; w++) {
        DWinOut o; randomBytes(&o, sizeof(o)); const bool hard = withHard && isListed[w] && w == listed[0];
        // a window that fits neither arena: more live records than three quarters of the arena in global memory hold (every candidate on a diagonal of its own, none removed)
        const u32 nCand = hard ? 60 : rnd(6) == 0 ? 0 : rnd(3) ? 1 + rnd(3) : 5 + rnd(12);
        FWin W = logWindow(rs, P, nCand, 1); if (hard) for (u32 k = 0; k < nCand; k++) { Cand &c = W.cand[k]; for (u32 e = 0; e < c.t.nExons; e++) c.ex[e].G = 700000 + 13000ull * k + c.ex[e].R; c.t.maxScore = 50; }
        o.minIn[0] = rnd(2) ? 0 : (i32)rnd(140); o.minIn[1] = rnd(2) ? 0 : (i32)rnd(140); o.nCand = nCand; o.candOff32 = (u32)((S.cand.size() - b.candOff) / 32u); candLogBytes(W.cand, S.cand);
        S.wout.push_back(o); if (!isListed[w]) continue;
        // the two attempts of k_stitch_replay: the LDS arena, then the arena in global memory
        CandLogResult res = candLogSequential(W.cand, Nmax, range, chim, o.minIn, b.arenaL, nullptr); const bool second = res.ovf;
        if (second) res = candLogSequential(W.cand, Nmax, range, chim, o.minIn, b.arenaG, nullptr);
        TrsWinExp &e = exp[w]; memset(&e, 0, sizeof(e)); e.w = w; e.hard = res.ovf; e.recOff = S.recExp.size();
        nClass[res.ovf ? R_HARD : second ? R_SECOND_ATTEMPT : R_FIRST_ATTEMPT]++; if (res.sens[0] != INT_MAX || res.sens[1] != INT_MAX) nClass[R_MATE_CLAUSE]++;
        if (res.ovf) continue;
        if (res.list.empty()) nClass[R_EMPTY_RESULT]++;
        u32 eoff = 0; for (u32 id : res.list) { Cand c = W.cand[id]; c.t.exonOffset = eoff; const u8 *p = (const u8 *)&c.t; S.recExp.insert(S.recExp.end(), p, p + REC_HDR); p = (const u8 *)c.ex; S.recExp.insert(S.recExp.end(), p, p + 32u * c.t.nExons); eoff += c.t.nExons; }          // flushWindowImpl: exonOffset relative to the window's block
        e.nTr = (u32)res.list.size(); e.nEx = eoff; if (e.nTr) { e.headScore = W.cand[res.list[0]].t.maxScore; e.headGlen = W.cand[res.list[0]].t.gLength; } sumT += e.nTr; sumE += e.nEx;
    }
    for (u32 w : listed) { S.winExp.push_back(exp[w]); S.list.push_back(w); }
    b.nWout = nWout; b.nList = nItems; b.nWinExp = nItems; b.candBytes = S.cand.size() - b.candOff; b.trCap = sumT; b.exCap = sumE; b.expFlags = 0; for (u32 w : listed) if (exp[w].hard) b.expFlags |= (u32)OVF_HARD;
    if (shortTr == 1 && sumT > 0) { b.trCap = sumT - 1; b.expFlags |= OVF_TRPOOL; nClass[R_CAP_SHORT]++; } else if (shortTr == 2 && sumE > 0) { b.exCap = sumE - 1; b.expFlags |= OVF_TRPOOL; nClass[R_CAP_EX_SHORT]++; } else nClass[R_CAP_EXACT]++;
    std::vector<u32> L, l0; closeReads(S, b, L, l0);
    S.batch.push_back(b);
}

// a routine that contradicts itself may loop for ever: reported, not waited for
static void onAlarm(int) { static const char msg[] = "\na kernel does not end: 1 differences\n"; (void)!write(1, msg, sizeof(msg) - 1); _exit(1); }

int main(int argc, char **argv) {
    signal(SIGALRM, onAlarm); alarm(900);
    const char *dumpPath = nullptr; for (int a = 1; a < argc; a++) if (!strcmp(argv[a], "--dump") && a + 1 < argc) dumpPath = argv[++a];
    static TrsSet S;
    // ---- environments: resultSelect x outFilterMultimapScoreRange x mates, with roomy and tight transcript limits; chimeric detection under resultSelect 2
    for (u32 sel = 0; sel < 3; sel++) for (u32 ir = 0; ir < 3; ir++) for (u32 tight = 0; tight < 2; tight++) {
        TrsEnv e; memset(&e, 0, sizeof(e)); staramd_params &P = e.P; P.resultSelect = sel; P.outFilterMultimapScoreRange = ir == 0 ? 0 : ir == 1 ? 1 : 1000; P.readNmates = 1 + (sel + ir + tight) % 2;
        P.alignTranscriptsPerWindowNmax = tight ? 3 : 100; P.alignTranscriptsPerReadNmax = tight ? 10 : 10000;
        if (sel == 2) { P.chimSegmentMinPositive = 1; P.chimSegmentMin = 12; P.chimSegmentReadGapMax = tight ? 0 : 3; }
        S.env.push_back(e);
    }
    { TrsEnv e = S.env[12]; e.P.chimSegmentMinPositive = 0; S.env.push_back(e); }                                            // resultSelect 2 in the first pass of a two-pass run
    { TrsEnv e = S.env[3]; e.P.alignTranscriptsPerWindowNmax = 5; e.P.alignTranscriptsPerReadNmax = 5; S.env.push_back(e); }      // the limit at the first window
    { TrsEnv e = S.env[14]; e.P.readNmates = 2; S.env.push_back(e); }                                                        // chimeric detection on pairs, range 1
    const u32 nEnv = (u32)S.env.size();
    // ---- A, E
    { static const u32 PW[4] = {1, 13, 64, 65}; for (u32 k = 0; k < 4; k++) { packCase(S, PW[k], 1); packCase(S, PW[k], 1); packCase(S, PW[k], 23); packCase(S, PW[k], 47); packCase(S, PW[k], 70); packCase(S, PW[k], 70); } }
    { static const u32 NB[9] = {1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 5000}; for (u32 k = 0; k < 9; k++) for (u32 f = 0; f < 6; f++) scanCase(S, NB[k], f % 3); }
    { static const u32 NR[5] = {1, 255, 256, 257, 1000}; for (u32 k = 0; k < 5; k++) for (u32 rep = 0; rep < 5; rep++) scanLocalCase(S, NR[k]); }
    // ---- B
    { static const u32 NR[4] = {1, 256, 257, 600}; for (u32 k = 0; k < 4; k++) for (u32 rep = 0; rep < (k == 0 ? 12u : 5u); rep++) verifyCase(S, NR[k]); }
    // ---- C: every item count with and without chimSegmentMinPositive (which admits every candidate), a window that fits neither arena, pools one record short
    { static const u32 NI[4] = {0, 1, 3, 50}; const u32 envs[3] = {2, 14, 3};          // roomy lists, roomy lists under chimSegmentMinPositive, lists of 3
      for (u32 rep = 0; rep < 2; rep++) for (u32 k = 0; k < 4; k++) for (u32 e = 0; e < 3; e++) { replayCase(S, envs[e], NI[k], false, 0); if (NI[k] >= 3) { if (e < 2) replayCase(S, envs[e], NI[k], true, 0); replayCase(S, envs[e], NI[k], false, 1); replayCase(S, envs[e], NI[k], false, 2); } } }
    // ---- D: every environment, every kind of read
    for (u32 ie = 0; ie < nEnv; ie++) {
        const staramd_params &P = S.env[ie].P; TrsBatch b = newBatch(S, TRS_FINISH, ie); std::vector<FRead> reads; const u32 n = 70 + rnd(30);
        for (u32 r = 0; r < n; r++) reads.push_back(makeRead(P, r < 60 ? r % 6 : 0));
        nClass[P.resultSelect == 0 ? F_SEL0 : P.resultSelect == 1 ? F_SEL1 : F_SEL2]++; nClass[P.outFilterMultimapScoreRange == 0 ? F_RANGE0 : P.outFilterMultimapScoreRange == 1 ? F_RANGE1 : F_RANGE_LARGE]++; nClass[P.readNmates == 2 ? F_PAIRED : F_SINGLE_END]++;
        buildBatch(S, b, P, reads, false, true); S.batch.push_back(b);
    }
    // ---- F: the tail as the engine runs it; windows with candidate logs among the reads
    { static const u32 NR[4] = {1, 256, 257, 700};
      for (u32 k = 0; k < 4; k++) for (u32 rep = 0; rep < (k == 0 ? 12u : 5u); rep++) {
          const u32 ie = k == 0 ? (rep * 5 + 1) % nEnv : rep == 0 ? 1 : rep == 1 ? 15 : rep == 2 ? 7 : rep == 3 ? 20 : 14; const staramd_params &P = S.env[ie].P; TrsBatch b = newBatch(S, TRS_TAIL, ie); std::vector<FRead> reads;
          for (u32 r = 0; r < NR[k]; r++) {
              FRead R = makeRead(P, NR[k] == 1 ? (rep % 2 ? 5 : 0) : r % 11 < 6 ? r % 11 : 0);
              if (rnd(NR[k] > 300 ? 6 : 2) == 0 && !R.win.empty()) for (FWin &W : R.win) if (rnd(2)) { const FWin lw = logWindow(R.rs, P, 1 + rnd(P.alignTranscriptsPerWindowNmax < 10 ? 6 : 14), 4); W = lw; }
              reads.push_back(R);
          }
          nClass[T_NREADS_1 + k]++;
          const BatchFacts F = buildBatch(S, b, P, reads, true, true); if (F.secondBlock) nClass[T_BEST_SECOND_BLOCK]++; if (F.partner) nClass[T_PARTNER]++;
          S.batch.push_back(b); nClass[T_CAP_EXACT]++;
          if (b.expNOutTr > 1 && rep < 2) { TrsBatch s1 = b; s1.outTrCap = b.expNOutTr - 1; S.batch.push_back(s1); nClass[T_CAP_TR_SHORT]++; TrsBatch s2 = b; s2.outExCap = b.expNOutEx - 1; S.batch.push_back(s2); nClass[T_CAP_EX_SHORT]++; }
          if (rep < 2) { TrsBatch fl = b; fl.kind = TRS_FLAGS; fl.flags0 = (k + rep) % 2 ? (u32)OVF_WINPOOL : (u32)OVF_TRPOOL; fl.expFlags = fl.flags0; S.batch.push_back(fl); nClass[T_FLAGS]++; }
      } }
    if (dumpPath) { FILE *f = fopen(dumpPath, "wb"); if (!f) { perror(dumpPath); return 2; } trsWrite(f, S); if (fclose(f)) { perror(dumpPath); return 2; } }
    long bad = trsRun(S, true);
    if (refBad) { printf("%ld contradictions on the reference side\n", refBad); bad += refBad; }
    long empty = 0; u64 rarest = ~0ull;
    for (int c = 0; c < N_CLASSES; c++) { printf("  %-72s %llu\n", CLASS_NAME[c], (unsigned long long)nClass[c]); if (!nClass[c]) empty++; rarest = std::min<u64>(rarest, nClass[c]); }
    printf("rarest class: %llu cases\n", (unsigned long long)rarest);
    if (empty) { printf("%ld case classes never occurred\n", empty); bad += empty; }
    printf("%zu pack cases, %zu scans of block totals, %zu batches over %zu reads and %zu windows: %ld differences\n", S.pack.size(), S.scan.size(), S.batch.size(), S.read.size(), S.wout.size(), bad);
    return bad ? 1 : 0;
}
