// stitch_routines_check.cpp -- TEST INFRASTRUCTURE: the wave-cooperative routines of star_amd/csrc/engine/k_stitch.hip, one at a time, each call one emulated wavefront of 64 lanes:
//   coopExtend                                   against extendAlign of oracle/lane_routines_ref.h (the base-by-base restatement of extendAlign.cpp:6-93)
//   coopStitch                                   against stitchAlignToTranscript of the same file (stitchAlignToTranscript.cpp:9-415)
//   coopSjdbFind, coopSjdbHash, sjdbHashFind     against a linear scan of the arrays and binarySearch2, on tables of unique pairs; the hash tables come from the product's own fill
//   replayWindow / recordCandidate (both forms the product instantiates) / recordCandidateImpl<false/true> / compactArena<false/true>
//                                                against a sequential list after stitchWindowAligns.cpp:232-303 (the form of star_oracle.cpp:705-723) over synthetic candidate logs
//   blocksOverlap                                against the oracle's, on random exon lists
// Inputs are steered at the places where a 64-lane restatement of a sequential loop goes wrong: scans, gaps, repeats and lists of more than 64 and more than 128 positions, the
// best position in a second or later trip, equal maxima in two trips, runs of equal starts across chunk boundaries, hash clusters that wrap.  Every case is classified from the
// reference side and its inputs; the class table is printed and a class that never occurred fails the run.  Besides the comparison every call is held to returning the same values
// in all 64 lanes.  Host build through the wavefront emulator's headers (oracle/wave_emul); probes, case records and the comparison: stitch_routines_cases.h.
// usage: stitch_routines_check [scale] [--dump file]      scale: per cent of the full trial counts (100); --dump: the cases go to `file` for tests/stitch_routines_gpu.hip
#include "k_stitch.hip"
#define ExtRes ExtResRef
#include "lane_routines_ref.h"
#undef ExtRes
#include "star_oracle.cpp"
#include "stitch_routines_cases.h"
#include <random>
#include <set>
#include <map>
#include <csignal>
#include <unistd.h>
extern thread_local uint32_t ldsReads[];

static std::mt19937_64 rng(20250117);
static u32 rnd(u32 n) { return (u32)(rng() % n); }
#include "cand_log_ref.h"
static_assert(CAND_NE_MAX == SRS_NE_MAX, "the candidates of cand_log_ref.h fill the record stride of the probes");

// ---- classes -----------------------------------------------------------------------------------------------------------------------------------------------------------
enum { E_SCAN_LE64, E_SCAN_65_128, E_SCAN_GT128, E_LEN_TRIP1, E_LEN_TRIP2, E_LEN_TRIP3, E_BUDGET_LATE, E_SPACER, E_PAD_LOW, E_PAD_HIGH, E_N_READ, E_N_GENOME, E_TOEND_LEN, E_TOEND_FAIL, E_L_NONPOS, E_MATEGAP,
       E_FWD, E_BWD, E_STR0, E_STR1,
       J_RC_OK, J_RC_1, J_RC_2, J_RC_3, J_RC_4, J_RC_5, J_RC_6, J_RC_7, J_RC_8, J_RC_9, J_RC_10, J_KIND_SJA, J_KIND_EQ, J_KIND_DEL, J_KIND_INS, J_KIND_MATE, J_EQGAP_64, J_EQGAP_128, J_LEFT_TRIP2, J_LEFT_EXON_START,
       J_RSCAN_64, J_RSCAN_128, J_JR_TRIP1, J_JR_TRIP2, J_JR_TRIP3, J_TIE_TRIPS, J_JJL_64, J_JJR_64, J_JJL_CAP, J_JJR_CAP, J_MOTIF0, J_MOTIF1, J_MOTIF2, J_MOTIF3, J_MOTIF4, J_MOTIF5, J_MOTIF6, J_FLUSH_LEFT,
       J_ANNOT_M0_SHIFT, J_INS_FLUSH, J_INS_NOFLUSH, J_MATE_E1_OK, J_MATE_E1_FAIL, J_MATE_E2_OK, J_MATE_E2_FAIL, J_HASH, J_BISECT,
       F_PRESENT, F_ABSENT_SAME_START, F_BETWEEN, F_BELOW, F_ABOVE, F_RUN1, F_RUN2, F_RUN63, F_RUN64, F_RUN65, F_RUN200, F_OFFSETS, H_CLUSTER_64, H_CLUSTER_128, H_WRAP, H_MIN_TABLE,
       R_LIST_64, R_LIST_128, R_TAIL, R_REMOVE_TRIP2, R_RANK0_OVER64, R_INSERT_FULL, R_BEHIND_FULL, R_COMPACT_FREES, R_OVF_CLAUSE1, R_OVF_CLAUSE2, R_BIG_NO_OVF, R_FORM_REPLAY, R_FORM_WALK,
       R_FAM_OVERLAP, R_FAM_DISJOINT, R_FAM_NESTED, R_LDS_LIST_64, O_PAIRS, O_NONZERO, N_CLASSES };
static const char *CLASS_NAME[N_CLASSES] = {
    "extend: scan of <= 64 positions", "extend: scan of 65..128 positions", "extend: scan of more than 128 positions", "extend: extendL in the first trip", "extend: extendL in the second trip", "extend: extendL in a later trip",
    "extend: ended by the mismatch budget behind the first trip", "extend: ended by the mate spacer", "extend: ended by code 5 before the genome", "extend: ended by code 5 behind the genome", "extend: non-ACGT code of the read inside the scan",
    "extend: non-ACGT code of the genome inside the scan", "extend: extendToEnd returns a length", "extend: extendToEnd returns -999999999", "extend: (int) L <= 0", "extend: the mate-gap call, L = STARAMD_READ_LEN_MAX",
    "extend: forward", "extend: backward", "extend: strand 0", "extend: strand 1",
    "join: valid score", "join: -1000001", "join: -1000002", "join: -1000003", "join: -1000004", "join: -1000005", "join: -1000006", "join: -1000007", "join: -1000008", "join: -1000009", "join: -1000010",
    "join: annotated by sjA", "join: no gap or equal gap", "join: deletion or junction", "join: insertion", "join: mate join", "join: equal gap of more than 64 bases", "join: equal gap of more than 128 bases",
    "join: left scan stops in a second trip", "join: left scan runs into the start of the exon", "join: right scan of more than 64 positions", "join: right scan of more than 128 positions",
    "join: long right scan, jR in the first trip", "join: long right scan, jR in the second trip", "join: long right scan, jR in a later trip", "join: the same maximum in two trips", "join: jjL >= 64", "join: jjR >= 64",
    "join: jjL at the cap of 256", "join: jjR at the cap of 256", "join: motif 0", "join: motif 1", "join: motif 2", "join: motif 3", "join: motif 4", "join: motif 5", "join: motif 6", "join: non-canonical junction flushed left",
    "join: annotated junction with motif 0 and shifts", "join: insertion with alignInsertionFlushRight", "join: insertion without it", "join: mate join, first extension succeeds", "join: mate join, first extension fails",
    "join: mate join, second extension succeeds", "join: mate join, second extension fails", "join: junction looked up in the hash table", "join: junction looked up by the 64-ary search",
    "look-up: junction present", "look-up: absent pair whose start is present", "look-up: start between two entries", "look-up: start below the first entry", "look-up: start above the last entry",
    "look-up: run of 1 equal start", "look-up: run of 2", "look-up: run of 63", "look-up: run of 64", "look-up: run of 65", "look-up: run of 200", "look-up: (run length, first index mod 64) pairs queried, of 384",
    "hash: probe of more than 64 slots", "hash: probe of more than 128 slots", "hash: probe that wraps past the end of the table", "hash: the 128-slot table",
    "records: decision over a list longer than 64", "records: ... longer than 128", "records: block in the first trip, entries in later trips", "records: removal in a second trip", "records: insert at rank 0 over more than 64 entries",
    "records: insert into a full list", "records: candidate ranked behind a full list", "records: compaction that frees room", "records: overflow, no room after compaction (3584 bytes)", "records: overflow, live set above 3/4 (3584 bytes)",
    "records: large arena of the product, no overflow", "records: replay form", "records: walk form (header and exons in LDS)", "records: family of heavy overlap", "records: family without overlap", "records: nested family on many diagonals",
    "records: list longer than 64 with rank list and arena in LDS", "overlap: exon list pairs", "overlap: pairs with an overlap"};
static u64 nClass[N_CLASSES]; static long refBad = 0;      // refBad: the two reference sides of a look-up disagree
static std::set<u32> offsetsSeen;

// ---- genome, junction sites, environments ----------------------------------------------------------------------------------------------------------------------------------
static const u64 NG = 400000;
struct Site { u64 d, a; u32 repL, repR; };                       // first base of the intron, first base behind it
struct Stretch { u64 p; u32 len, per; };
static std::vector<Site> sites, sitesL, sitesLL, sitesR;        // sitesL / sitesR: with a repeat of 64 bases or more left / right of the junction
static std::vector<Stretch> longStretch;
static u8 *G = nullptr;
static std::vector<DevIndex> Xh;                 // the environments for the reference side (host pointers)
static std::vector<std::vector<u64>> envHashH;

static void makeGenome(SrsSet &S) {
    S.gbuf.assign(NG + 2 * GPAD, 5); G = S.gbuf.data() + GPAD;
    for (u64 i = 0; i < NG; i++) { const u32 x = rnd(1000); G[i] = x < 3 ? 4 : (u8)rnd(4); }
    for (int k = 0; k < 400; k++) { const u64 p = rnd((u32)NG - 400); const u32 len = 5 + rnd(60), per = 1 + rnd(3); for (u32 i = per; i < len; i++) G[p + i] = G[p + i % per]; }
    for (int k = 0; k < 80; k++) { const u32 len = 150 + rnd(650), per = 1 + rnd(6); const u64 p = 3000 + rnd((u32)NG - 8000); for (u32 i = per; i < len; i++) G[p + i] = G[p + i % per]; longStretch.push_back({p, len, per}); }
    static const u8 mot[6][4] = {{2, 3, 0, 2}, {1, 3, 0, 1}, {2, 1, 0, 2}, {1, 3, 2, 1}, {0, 3, 0, 1}, {2, 3, 0, 3}};
    for (int k = 0; k < 3000; k++) {
        Site s; s.d = 3000 + rnd((u32)NG - 12000); s.a = s.d + 21 + rnd(rnd(3) ? 3000 : 400);
        if (rnd(4)) { const u32 m = rnd(6); G[s.d] = mot[m][0]; G[s.d + 1] = mot[m][1]; G[s.a - 2] = mot[m][2]; G[s.a - 1] = mot[m][3]; }
        s.repL = s.repR = 0;
        auto repLen = [&]() { const u32 w = rnd(6); return w < 2 ? 1 + rnd(90) : w == 2 ? 64 + rnd(64) : w == 3 ? 128 + rnd(100) : 256 + rnd(60); };
        const u32 rep = rnd(6);                     // repeats around the junction: the end of exon A = the end of the intron (jjL), the start of the intron = the start of exon B (jjR)
        if (rep == 0 || rep == 2) { const u32 K = repLen(); for (u32 i = 1; i <= K; i++) { if (G[s.a - i] > 3) G[s.a - i] = (u8)rnd(4); G[s.d - i] = G[s.a - i]; } s.repL = K; }
        if (rep == 1 || rep == 2) { const u32 K = repLen(); for (u32 i = 0; i < K; i++) { if (G[s.d + i] > 3) G[s.d + i] = (u8)rnd(4); G[s.a + i] = G[s.d + i]; } s.repR = K; }
        sites.push_back(s); if (s.repL >= 64) sitesL.push_back(s); if (s.repL >= 256) sitesLL.push_back(s); if (s.repR >= 64) sitesR.push_back(s);
    }
}

static void makeEnvs(SrsSet &S, u32 nEnv) {
    for (u32 e = 0; e < nEnv; e++) {
        SrsEnv v; memset(&v, 0, sizeof(v)); staramd_params &P = v.P;
        // scoreStitchSJshift -1: no left scan, the junction scan starts at the end of A (the only way a non-canonical junction is still flushed left)
        P.scoreStitchSJshift = e % 5 < 2 ? -1 : (int)rnd(3); P.alignIntronMin = 21; P.alignIntronMax = e % 3 == 1 ? 500 : 0;
        P.scoreGap = 0; P.scoreGapNoncan = -8; P.scoreGapGCAG = -4; P.scoreGapATAC = -8; P.scoreDelOpen = -2; P.scoreDelBase = -2; P.scoreInsOpen = -2; P.scoreInsBase = -2;
        P.alignInsertionFlushRight = e % 3 == 0; P.sjdbScore = 2; P.alignMatesGapMax = e % 4 == 1 ? 300 : 0; P.alignEndsProtrudeNbasesMax = rnd(5) == 0 ? 10 : 0;
        P.alignSJstitchMismatchNmax[0] = 0; P.alignSJstitchMismatchNmax[1] = -1; P.alignSJstitchMismatchNmax[2] = 0; P.alignSJstitchMismatchNmax[3] = 0;
        if (rnd(4) == 0) for (int k = 0; k < 4; k++) P.alignSJstitchMismatchNmax[k] = (int)rnd(4) - 1;
        if (rnd(2) == 0) for (int k = 0; k < 4; k++) P.alignSJstitchMismatchNmax[k] = -1;
        P.outFilterMismatchNoverLmax = rnd(3) == 0 ? 0.05 : 0.3;
        for (int a = 0; a < 2; a++) for (int b = 0; b < 2; b++) P.alignEndsTypeExt[a][b] = rnd(8) == 0;
        v.sjOff = (u32)S.sjS.size(); v.useHash = e & 1u;
        if (e % 3 != 2) {                           // unique (start, end) pairs, as sjdbPrepare leaves them: sorted, duplicates removed
            std::set<std::pair<u64, u64>> js;
            for (const Site &s : sites) { if (rnd(2)) js.insert({s.d, s.a - 1}); if (rnd(8) == 0) js.insert({s.d, s.a + 5}); if (rnd(8) == 0) { const u32 r = 1 + rnd(3); js.insert({s.d - r, s.a - 1 - r}); } }
            for (int k = 0; k < 60; k++) { const u64 a = rnd((u32)NG); js.insert({a, a + 30 + rnd(500)}); }
            for (const auto &j : js) { S.sjS.push_back(j.first); S.sjE.push_back(j.second); S.sjM.push_back((u8)(rnd(3) ? rnd(7) : 0)); S.sjL.push_back((u8)(rnd(6) ? rnd(4) : rnd(120))); S.sjR.push_back((u8)(rnd(6) ? rnd(4) : rnd(120))); S.sjStr.push_back((u8)rnd(3)); }
            v.sjN = (u32)js.size();
        }
        S.env.push_back(v);
    }
    Xh.resize(nEnv); envHashH.resize(nEnv);
    static std::vector<u32> info; info.resize(S.sjS.size()); for (size_t k = 0; k < info.size(); k++) info[k] = SJ_INFO(S.sjM[k] & 7u, S.sjStr[k] & 3u, S.sjL[k], S.sjR[k]);
    for (u32 e = 0; e < nEnv; e++) {
        const SrsEnv &v = S.env[e]; DevIndex &x = Xh[e]; memset(&x, 0, sizeof(x));
        x.G = G; x.nGenome = NG; x.P = v.P; x.sjdbN = v.sjN;
        if (v.sjN) { x.sjdbStart = S.sjS.data() + v.sjOff; x.sjdbEnd = S.sjE.data() + v.sjOff; x.sjdbMotif = S.sjM.data() + v.sjOff; x.sjdbShiftLeft = S.sjL.data() + v.sjOff; x.sjdbShiftRight = S.sjR.data() + v.sjOff;
                     x.sjdbStrand = S.sjStr.data() + v.sjOff; x.sjdbInfo = info.data() + v.sjOff;
                     if (v.useHash) { const u32 mask = srsHashMask(v.sjN); envHashH[e].assign(2 * ((size_t)mask + 1), 0);
                                      sjdbHashFill(envHashH[e].data(), mask, x.sjdbStart, x.sjdbEnd, x.sjdbMotif, x.sjdbStrand, x.sjdbShiftLeft, x.sjdbShiftRight, v.sjN); x.sjdbHash = envHashH[e].data(); x.sjdbHashMask = mask; } }
    }
}

// ---- a read in the LDS array of this thread (for the reference side) and in the pool (for the probes) ---------------------------------------------------------------------------
static void packRead(SrsSet &S, const std::vector<u8> &r, u32 str, StitchCtx &c, SrsRead &rd) {
    const u32 Lread = (u32)r.size(), nb = (((Lread + 16) / 2 + 8) + 15) & ~15u;
    std::vector<u8> pk(nb, 0xFF);
    for (u32 j = 0; j <= Lread; j++) { const u8 code = j < Lread ? (str == 0 ? r[j] : compBase(r[Lread - 1 - j])) : (u8)15; u8 &b = pk[j >> 1]; b = (j & 1) ? (u8)((b & 0x0F) | (code << 4)) : (u8)((b & 0xF0) | code); }
    memset(ldsReads, 0xCD, 4096); memcpy((u8 *)ldsReads + 64, pk.data(), nb);
    rd.rdOff = (u32)S.packed.size(); S.packed.insert(S.packed.end(), pk.begin(), pk.end());
    rd.Lread = Lread; rd.str = str; rd.len0 = Lread;
    memset(&c, 0, sizeof(c)); c.X = &Xh[rd.env]; c.ldsByte = 64; c.Lread = Lread; c.str = str; c.readLength[0] = Lread; c.mmMaxTotal = rd.mmMaxTotal; gcInit(c.ca); gcInit(c.cb);
}

// what the scan of extendAlign.cpp:58-91 meets, base by base (classes only)
static void classifyExt(const StitchCtx &c, const SrsExt &s) {
    nClass[s.dir > 0 ? E_FWD : E_BWD]++; nClass[s.rd.str ? E_STR1 : E_STR0]++;
    if (s.L == STARAMD_READ_LEN_MAX && s.dir > 0) nClass[E_MATEGAP]++;
    if (s.toEnd) { if (s.expRet && s.exp.maxScore == -999999999) nClass[E_TOEND_FAIL]++; else if (s.expRet) nClass[E_TOEND_LEN]++; return; }
    if ((int)s.L <= 0) { nClass[E_L_NONPOS]++; return; }
    const double thr = fmin(s.pMMmax * (double)(u64)(s.Lprev + s.L), (double)s.nMMmax);
    u32 nMM = 0; bool nR = false, nGn = false; int i, why = 0; u64 at = 0;
    for (i = 0; i < (int)s.L; i++) {
        const u64 gp = s.gStart + (u64)(i64)(s.dir * i); if (gp == (u64)-1) { why = 3; at = gp; break; }
        const u8 gc = G[(i64)gp], rc = RD(c, (u32)((int)s.rStart + s.dir * i));
        if (gc == 5) { why = 3; at = gp; break; } if (rc == STARAMD_SPACER_BASE) { why = 2; break; }
        if (rc > 3 || gc > 3) { nR |= rc > 3; nGn |= gc > 3; continue; }
        if (gc != rc) { if ((double)(u32)(nMM + s.nMMprev) >= thr) { why = 1; break; } nMM++; }
    }
    const u32 scan = (u32)i + (why ? 1u : 0u);
    nClass[scan <= 64 ? E_SCAN_LE64 : scan <= 128 ? E_SCAN_65_128 : E_SCAN_GT128]++;
    if (s.expRet) nClass[s.exp.extendL <= 64 ? E_LEN_TRIP1 : s.exp.extendL <= 128 ? E_LEN_TRIP2 : E_LEN_TRIP3]++;
    if (why == 1 && i >= 64) nClass[E_BUDGET_LATE]++;
    if (why == 2) nClass[E_SPACER]++;
    if (why == 3) nClass[(i64)at < 0 ? E_PAD_LOW : E_PAD_HIGH]++;
    if (nR) nClass[E_N_READ]++; if (nGn) nClass[E_N_GENOME]++;
}

// which branch of stitchAlignToTranscript.cpp a join takes and what its scans meet, base by base (classes only; the comparison is with lane_routines_ref.h)
static void classifyJoin(StitchCtx c, const SrsJoin &s) {
    const DevIndex &X = *c.X; const staramd_params &P = X.P;
    const int rc_ = s.expScore > -1000000 ? 0 : -(s.expScore + 1000000);
    nClass[J_RC_OK + (rc_ <= 10 ? rc_ : 0)]++;
    if (s.h.nExons >= STARAMD_MAX_N_EXONS) return;
    const staramd_exon &eA = s.eA; u32 rBstart = s.rBstart, L = s.L; u64 gBstart = s.gBstart; const u32 rAend = s.rAend; const u64 gAend = s.gAend;
    if (s.sjAB != -1 && eA.sjA == s.sjAB && eA.iFrag == s.iFragB && rBstart == rAend + 1 && gAend + 1 < gBstart) { nClass[J_KIND_SJA]++; return; }
    if (eA.iFrag != s.iFragB) {
        if (!(gBstart + s.ex0R + (i64)P.alignEndsProtrudeNbasesMax >= s.ex0G || s.ex0G < s.ex0R)) return;
        if (P.alignMatesGapMax > 0 && gBstart > eA.G + eA.L + P.alignMatesGapMax) return;
        nClass[J_KIND_MATE]++;
        Hdr h = s.h; ExtResRef e;
        const bool e1 = extendAlign(c, rAend + 1, gAend + 1, 1, 1, STARAMD_READ_LEN_MAX, h.nMatch, h.nMM, c.mmMaxTotal, P.outFilterMismatchNoverLmax, P.alignEndsTypeExt[eA.iFrag][1] != 0, e);
        if (e1) { h.nMatch += e.nMatch; h.nMM += e.nMM; } h.nMatch += L;
        const u32 extlen = P.alignEndsTypeExt[s.iFragB][1] ? STARAMD_READ_LEN_MAX : (u32)(gBstart - s.ex0G + s.ex0R);
        const bool e2 = extendAlign(c, rBstart - 1, gBstart - 1, -1, -1, extlen, h.nMatch, h.nMM, c.mmMaxTotal, P.outFilterMismatchNoverLmax, P.alignEndsTypeExt[s.iFragB][1] != 0, e);
        nClass[e1 ? J_MATE_E1_OK : J_MATE_E1_FAIL]++; nClass[e2 ? J_MATE_E2_OK : J_MATE_E2_FAIL]++;
        return;
    }
    const u64 gBend = gBstart + L - 1; const u32 rBend = rBstart + L - 1;
    if (rBend <= rAend || gBend <= gAend) return;
    if (rBstart <= rAend) { gBstart += rAend - rBstart + 1; rBstart = rAend + 1; L = rBend - rBstart + 1; }
    const int gGap = (int)(gBstart - gAend - 1), rGap = (int)(rBstart - rAend - 1);
    const u64 gBstart1 = gBstart - (u64)(i64)rGap - 1;
    if ((gGap == 0 && rGap == 0) || (gGap > 0 && rGap > 0 && rGap == gGap)) { nClass[J_KIND_EQ]++; if (rGap > 64) nClass[J_EQGAP_64]++; if (rGap > 128) nClass[J_EQGAP_128]++; return; }
    if (rGap > gGap) { nClass[J_KIND_INS]++; nClass[P.alignInsertionFlushRight ? J_INS_FLUSH : J_INS_NOFLUSH]++; return; }
    const u64 Del = (u64)(i64)(gGap - rGap);
    if (Del > P.alignIntronMax && P.alignIntronMax > 0) return;
    nClass[J_KIND_DEL]++;
    int Score1 = 0, jR1 = 1;
    do { jR1--; const u8 rc = RD(c, (u32)((int)rAend + jR1)), gB = G[(i64)(gBstart1 + (i64)jR1)]; if (rc != gB && gB < 4 && rc == G[(i64)(gAend + (i64)jR1)]) Score1 -= 1; } while (Score1 + P.scoreStitchSJshift >= 0 && (int)eA.L + jR1 > 1);
    const int jStart = jR1; const bool byCount = Score1 + P.scoreStitchSJshift < 0;
    if (byCount && jStart <= -64) nClass[J_LEFT_TRIP2]++;
    if (!byCount) nClass[J_LEFT_EXON_START]++;
    const bool isIntron = Del >= P.alignIntronMin; const int jEnd = (int)rBend - (int)rAend;
    int maxScore2 = -999999, jR = 0, jCan = 999; Score1 = 0; std::vector<int> s2;
    for (; jR1 < jEnd || jR1 == jStart; jR1++) {
        const u8 ra = RD(c, (u32)((int)rAend + jR1)), gA = G[(i64)(gAend + (i64)jR1)], gB = G[(i64)(gBstart1 + (i64)jR1)];
        if (ra == gA && ra != gB) Score1 += 1; if (ra != gA && ra == gB) Score1 -= 1;
        int jCan1 = -1, jPen1 = 0;
        if (isIntron) { const u8 d1 = G[(i64)(gAend + (i64)jR1 + 1)], d2 = G[(i64)(gAend + (i64)jR1 + 2)], a1 = G[(i64)(gBstart1 + (i64)jR1 - 1)], a2 = gB;
            if (d1 == 2 && d2 == 3 && a1 == 0 && a2 == 2) jCan1 = 1; else if (d1 == 1 && d2 == 3 && a1 == 0 && a2 == 1) jCan1 = 2; else if (d1 == 2 && d2 == 1 && a1 == 0 && a2 == 2) { jCan1 = 3; jPen1 = P.scoreGapGCAG; }
            else if (d1 == 1 && d2 == 3 && a1 == 2 && a2 == 1) { jCan1 = 4; jPen1 = P.scoreGapGCAG; } else if (d1 == 0 && d2 == 3 && a1 == 0 && a2 == 1) { jCan1 = 5; jPen1 = P.scoreGapATAC; }
            else if (d1 == 2 && d2 == 3 && a1 == 0 && a2 == 3) { jCan1 = 6; jPen1 = P.scoreGapATAC; } else { jCan1 = 0; jPen1 = P.scoreGapNoncan; } }
        s2.push_back(Score1 + jPen1);
        if (maxScore2 < Score1 + jPen1) { maxScore2 = Score1 + jPen1; jR = jR1; jCan = jCan1; }
    }
    const int scanLen = (int)s2.size();
    if (scanLen > 64) { nClass[J_RSCAN_64]++; if (scanLen > 128) nClass[J_RSCAN_128]++; const int trip = (jR - jStart) / 64; nClass[trip == 0 ? J_JR_TRIP1 : trip == 1 ? J_JR_TRIP2 : J_JR_TRIP3]++;
                        int last = -1; for (int k = 0; k < scanLen; k++) if (s2[k] == maxScore2) last = k; if (last / 64 != (jR - jStart) / 64) nClass[J_TIE_TRIPS]++; }
    u32 jjL = 0, jjR = 0;
    for (;;) { if (!(gAend + (i64)jR >= jjL)) break; const u8 x = G[(i64)(gAend - jjL + (i64)jR)]; if (!(x == G[(i64)(gBstart1 - jjL + (i64)jR)] && x < 4 && jjL <= 255)) break; jjL++; }
    for (;;) { if (!(gAend + jjR + (i64)jR + 1 < X.nGenome)) break; const u8 x = G[(i64)(gAend + jjR + (i64)jR + 1)]; if (!(x == G[(i64)(gBstart1 + jjR + (i64)jR + 1)] && x < 4 && jjR <= 255)) break; jjR++; }
    if (jjL >= 64) nClass[J_JJL_64]++; if (jjR >= 64) nClass[J_JJR_64]++; if (jjL == 256) nClass[J_JJL_CAP]++; if (jjR == 256) nClass[J_JJR_CAP]++;
    if (jCan <= 0 && jjL > 0 && (int)eA.L + jR - (int)jjL >= 1) nClass[J_FLUSH_LEFT]++;
    if (X.sjdbN > 0) nClass[X.sjdbHash ? J_HASH : J_BISECT]++;
    if (rc_ == 0) { if (s.expA.canonSJ >= 0 && s.expA.canonSJ <= 6) nClass[J_MOTIF0 + s.expA.canonSJ]++; if (s.expA.sjAnnot && s.expA.canonSJ == 0 && (s.expA.shiftSJ[0] || s.expA.shiftSJ[1])) nClass[J_ANNOT_M0_SHIFT]++; }
}

// ---- joins and extensions: the generator of lane_routines_check.cpp with an unchanging genome, junction tables of unique pairs, pieces, gaps and repeats of up to 350 bases,
// and kinds steered at the return codes and scans that generator met a few times in 40 000 trials
static void joinTrial(SrsSet &S, u32 nExtPerJoin) {
    SrsJoin j; memset(&j, 0, sizeof(j));
    j.rd.env = rnd((u32)S.env.size()); const DevIndex &X = Xh[j.rd.env];
    const bool wide = rnd(3) == 0;
    u32 lenA = wide ? 15 + rnd(340) : 15 + rnd(80), lenB = wide ? 15 + rnd(340) : 15 + rnd(80);
    u64 gA0 = 1000 + rnd((u32)NG - 20000);
    static const int KINDS[18] = {0, 1, 1, 2, 2, 2, 3, 3, 4, 5, 6, 7, 8, 9, 9, 9, 10, 10};
    const int kindGap = KINDS[rnd(18)];      // 0 continuous, 1 small deletion, 2 intron at a site, 3 insertion, 4 equal gap with junk, 5 overlap on the genome, 6 B before the end of A on the genome, 7 deletion inside a long repeat, 8 intron anywhere, 9 / 10 intron at a site with a long repeat left / right of the junction
    u32 between = 0; u64 gB0;
    if (kindGap == 0) gB0 = gA0 + lenA;
    else if (kindGap == 1) gB0 = gA0 + lenA + 1 + rnd(20);
    else if (kindGap == 2) { const Site &s = sites[rnd((u32)sites.size())]; gA0 = s.d - lenA; gB0 = s.a; }
    else if (kindGap == 3) { between = 1 + rnd(wide ? 40 : 12); gB0 = gA0 + lenA + (rnd(2) ? 0 : rnd(wide ? 30 : 10)); }
    else if (kindGap == 4) { between = 1 + rnd(wide ? 300 : 15); gB0 = gA0 + lenA + between; }
    else if (kindGap == 5) gB0 = gA0 + lenA - std::min<u32>(lenA - 1, 1 + rnd(5));
    else if (kindGap == 6) gB0 = gA0 + lenA - std::min<u32>(lenA, lenB + rnd(8));
    else if (kindGap == 7) { const Stretch &t = longStretch[rnd((u32)longStretch.size())]; lenA = 15 + rnd(t.len / 2); lenB = 15 + rnd(t.len / 2); gA0 = t.p + rnd(t.len / 3); gB0 = gA0 + lenA + t.per * (1 + rnd(rnd(2) ? 4 : 30)); }
    else if (kindGap == 9) { const Site &s = rnd(2) ? sitesLL[rnd((u32)sitesLL.size())] : sitesL[rnd((u32)sitesL.size())]; lenA = std::min<u32>(355, s.repL + 10 + rnd(40)); gA0 = s.d - lenA; gB0 = s.a; }
    else if (kindGap == 10) { const Site &s = sitesR[rnd((u32)sitesR.size())]; lenB = std::min<u32>(355, s.repR + 10 + rnd(40)); gA0 = s.d - lenA; gB0 = s.a; }
    else gB0 = gA0 + lenA + 21 + rnd(3000);
    std::vector<u8> r;
    for (u32 i = 0; i < lenA; i++) r.push_back(G[gA0 + i]);
    for (u32 i = 0; i < between; i++) r.push_back(kindGap == 4 && rnd(wide ? 30 : 4) ? G[gA0 + lenA + i] : (u8)rnd(4));
    const u32 rB0 = (u32)r.size();
    for (u32 i = 0; i < lenB; i++) r.push_back(G[gB0 + i]);
    const u32 tail = rnd(20); for (u32 i = 0; i < tail; i++) r.push_back((u8)rnd(4));
    const u32 noise = wide ? 1 + rnd(3) : 3;
    for (auto &b : r) { if (b > 3) b = 4; const u32 x = rnd(100); if (x < noise) b = (u8)rnd(4); else if (x == 3 && rnd(wide ? 4 : 1) == 0) b = 4; }
    const bool otherMate = rnd(5) == 0;
    if (otherMate) r[rB0 - 1] = STARAMD_SPACER_BASE;
    const u32 Lread = (u32)r.size();
    j.rd.mmMaxTotal = rnd(4) == 0 ? 2 : (wide ? 20 : 10);
    StitchCtx c; packRead(S, r, rnd(2), c, j.rd);
    u32 cutA = 5 + rnd(lenA - 5);
    if ((kindGap == 2 || kindGap >= 9) && rnd(3)) cutA = lenA - std::min<u32>(lenA - 5, rnd(12));            // (mostly: seed A reaches the junction, as the seeds of a spliced read do)
    const u32 rAend = cutA - 1; const u64 gAend = gA0 + cutA - 1;
    int shiftB = (int)rnd(12) - 4;
    if ((int)rB0 + shiftB < 1) shiftB = 0;
    if (otherMate) { if (shiftB < 0) shiftB = 0; if (cutA + 1 > rB0) return; }
    u32 rBstart = (u32)((int)rB0 + shiftB); u64 gBstart = (u64)((i64)gB0 + shiftB);
    u32 Lb = 5 + rnd(lenB - 4); if (kindGap == 10 && rnd(4)) Lb = lenB - rnd(5); if (rBstart + Lb > Lread) Lb = Lread - rBstart; if (Lb == 0) return;
    Hdr h; memset(&h, 0, sizeof(h)); h.nExons = 1 + rnd(3); h.nMM = rnd(3); h.nMatch = cutA; h.rStart = 0; h.gStart = gA0; h.tR2 = rAend; h.tG2 = gAend;
    if (rnd(50) == 0) h.nExons = STARAMD_MAX_N_EXONS;
    staramd_exon eA; memset(&eA, 0, sizeof(eA)); eA.G = gA0 + (cutA > 20 && rnd(2) ? cutA - 10 : 0);
    if (kindGap == 9 && rnd(4)) eA.G = gA0;
    else if (rnd(4) == 0 || kindGap == 7) { const u32 l = 1 + rnd(rnd(2) ? 6 : 100); eA.G = gA0 + (cutA > l ? cutA - l : 0); }
    eA.R = (u16)(eA.G - gA0); eA.L = (u16)(cutA - eA.R); eA.iFrag = 0; eA.sjA = -1;
    u32 iFragB = otherMate ? 1 : 0; i32 sjAB = -1;
    if (rnd(8) == 0 && X.sjdbN) { sjAB = (i32)rnd(X.sjdbN); if (rnd(4)) eA.sjA = sjAB; if (rnd(4) && !otherMate) { rBstart = rAend + 1; if (rBstart + Lb > Lread) Lb = Lread - rBstart; if (!Lb) return; } }
    if (rnd(60) == 0 && !otherMate && rBstart > 6) { rBstart = rAend > 8 ? rAend - 3 - rnd(4) : rBstart; Lb = 1 + rnd(3); gBstart = gAend - (rAend - rBstart); }     // B inside A
    j.ex0R = 0; j.ex0G = (otherMate && rnd(10) == 0) ? gBstart + 20 + rnd(100) : gA0;
    j.rAend = rAend; j.gAend = gAend; j.rBstart = rBstart; j.gBstart = gBstart; j.L = Lb; j.iFragB = iFragB; j.sjAB = sjAB; j.h = h; j.eA = eA;
    { Hdr h1 = h; staramd_exon a1 = eA, n1; memset(&n1, 0x5A, sizeof(n1)); bool ad1 = false; StitchCtx c1 = c;
      j.expScore = stitchAlignToTranscript(c1, rAend, gAend, rBstart, gBstart, Lb, iFragB, sjAB, h1, a1, n1, ad1, j.ex0R, j.ex0G);
      j.expAdded = ad1; j.expH = h1; j.expA = a1; j.expN = n1; }
    classifyJoin(c, j);
    S.join.push_back(j);
    for (u32 rep = 0; rep < nExtPerJoin; rep++) {
        SrsExt x; memset(&x, 0, sizeof(x)); x.rd = j.rd;
        const int dir = rep & 1 ? 1 : -1;
        u32 rs = rnd(Lread); u64 gsx = gA0 + rs + (rnd(4) == 0 ? rnd(5) : 0);
        if (rnd(3) == 0) { rs = dir > 0 ? rnd(std::min(Lread, 20u)) : Lread - 1 - rnd(std::min(Lread, 20u)); gsx = rs >= rB0 ? gB0 + (rs - rB0) : gA0 + rs; }      // a start near an end of the read: a long scan
        if (rnd(20) == 0) gsx = dir < 0 ? rnd(rnd(2) ? 12 : 200) : NG - 1 - rnd(rnd(2) ? 12 : 200);                   // near the ends of the genome: padding
        u32 Lx = dir > 0 ? Lread - rs : rs + 1; if (rnd(6) == 0) Lx = rnd(Lx + 1); if (rnd(40) == 0) Lx = (u32)-3;
        if (dir > 0 && rnd(3) == 0) Lx = STARAMD_READ_LEN_MAX;
        const bool toEnd = rnd(6) == 0;
        if (dir > 0 && Lx == STARAMD_READ_LEN_MAX) { bool sp = false; for (u32 i = rs; i < Lread; i++) if (r[i] == STARAMD_SPACER_BASE) sp = true; if (!sp) Lx = Lread - rs; }
        x.rStart = rs; x.dir = dir; x.gStart = gsx; x.L = Lx; x.Lprev = rnd(100); x.nMMprev = rnd(4); x.nMMmax = rnd(3) == 0 ? 2 : (wide ? 10 + rnd(15) : 10); x.pMMmax = rnd(2) ? 0.3 : 0.05; x.toEnd = toEnd;
        ExtResRef e1; StitchCtx d1 = c;
        x.expRet = extendAlign(d1, rs, gsx, dir, dir, Lx, x.Lprev, x.nMMprev, x.nMMmax, x.pMMmax, toEnd, e1) ? 1u : 0u;
        x.exp.maxScore = e1.maxScore; x.exp.extendL = e1.extendL; x.exp.nMatch = e1.nMatch; x.exp.nMM = e1.nMM;
        classifyExt(c, x);
        S.ext.push_back(x);
    }
}

// ---- junction tables of unique pairs and their queries ------------------------------------------------------------------------------------------------------------------------
static const u32 RUNS[6] = {1, 2, 63, 64, 65, 200};
static void makeTable(SrsSet &S, u32 N, bool cover, u32 nSample) {
    SrsTab t; memset(&t, 0, sizeof(t)); t.off = S.tS.size(); t.N = N; t.mask = srsHashMask(N);
    std::vector<u64> xs, ys; std::vector<std::pair<u32, u32>> runs;     // (first index, length)
    u64 cur = 1000 + rnd(1000);
    auto addRun = [&](u32 len) {
        len = std::min<u32>(len, N - (u32)xs.size()); if (!len) return;
        cur += 2 + rnd(50);
        if (rnd(6) == 0) for (u32 k = 0; k < 400000 && sjdbHashSlot(cur, t.mask) + 64u <= t.mask; k++) cur++;       // a start whose slot lies within 64 of the end of the table: the cluster wraps
        u64 e = cur + 30 + rnd(100); runs.push_back({(u32)xs.size(), len});
        for (u32 k = 0; k < len; k++) { xs.push_back(cur); ys.push_back(e); e += 1 + rnd(5); }
    };
    if (cover) for (u32 li = 1; li < 6; li++) for (u32 off = 0; off < 64; off++) { while (xs.size() % 64 != off) addRun(1); addRun(RUNS[li]); }
    const u32 nCover = (u32)xs.size();
    while (xs.size() < N) addRun(rnd(N < 300 ? 3 : 150) == 0 ? RUNS[rnd(6)] : 1);
    for (u32 k = 0; k < N; k++) { S.tS.push_back(xs[k]); S.tE.push_back(ys[k]); S.tInfo.push_back(SJ_INFO(rnd(7), rnd(3), rnd(256), rnd(256))); }
    const u32 it = (u32)S.tab.size(); S.tab.push_back(t);
    // the hash table of this table from the product's fill: for the classes (how far a probe walks, whether it wraps)
    std::vector<u64> hw(2 * ((size_t)t.mask + 1), 0);
    { std::vector<u8> m(N), st(N), sl(N), sr(N); for (u32 k = 0; k < N; k++) { const u32 v = S.tInfo[t.off + k]; m[k] = (u8)SJ_INFO_MOTIF(v); st[k] = (u8)SJ_INFO_STRAND(v); sl[k] = (u8)SJ_INFO_SHL(v); sr[k] = (u8)SJ_INFO_SHR(v); }
      sjdbHashFill(hw.data(), t.mask, xs.data(), ys.data(), m.data(), st.data(), sl.data(), sr.data(), N); }
    auto query = [&](u64 x, u64 y, int cls) {
        SrsFind f; memset(&f, 0, sizeof(f)); f.x = x; f.y = y; f.tab = it; f.expIdx = -1;
        for (u32 k = 0; k < N && xs[k] <= x; k++) if (xs[k] == x && ys[k] == y) { f.expIdx = (i32)k; break; }              // the linear scan
        const int b = binarySearch2(x, y, xs.data(), ys.data(), (int)N);
        if ((b < 0 ? -1 : b) != f.expIdx) { printf("binarySearch2 against the linear scan, table of %u, (%llu, %llu): %d / %d\n", N, (unsigned long long)x, (unsigned long long)y, b, f.expIdx); refBad++; }
        nClass[cls]++; if (t.mask == 127) nClass[H_MIN_TABLE]++;
        u32 h = sjdbHashSlot(x, t.mask), steps = 0; bool wrap = false;
        for (; steps <= t.mask; steps++) { const u32 hh = (h + steps) & t.mask; if (hh < h) wrap = true; if (hw[2 * (size_t)hh] == 0) break; if (f.expIdx >= 0 && (hw[2 * (size_t)hh] >> SJH_START_BITS) == (u64)f.expIdx + 1) break; }
        if (steps > 64) nClass[H_CLUSTER_64]++; if (steps > 128) nClass[H_CLUSTER_128]++; if (wrap) nClass[H_WRAP]++;
        S.find.push_back(f);
    };
    auto queryRunMember = [&](const std::pair<u32, u32> &r, u32 k) {
        for (int li = 0; li < 6; li++) if (r.second == RUNS[li]) { nClass[F_RUN1 + li]++; offsetsSeen.insert((u32)li * 64 + r.first % 64); }
        query(xs[r.first + k], ys[r.first + k], F_PRESENT);
    };
    for (const auto &r : runs) {
        if (N <= 4097) for (u32 k = 0; k < r.second; k++) queryRunMember(r, k);
        else if (r.first < nCover ? (r.second > 1 || rnd(10) == 0) : rnd(r.second > 1 ? 12 : 400) == 0) { queryRunMember(r, 0); queryRunMember(r, r.second - 1); for (u32 k = 0; k < 4 && r.second > 2; k++) queryRunMember(r, rnd(r.second)); if (r.second > 64) { queryRunMember(r, 63); queryRunMember(r, 64); } }
        if (N <= 4097 ? rnd(r.second > 1 ? 2 : 16) == 0 : (r.first < nCover ? rnd(r.second > 1 ? 4 : 40) == 0 : rnd(r.second > 1 ? 12 : 400) == 0)) {
            query(xs[r.first], ys[r.first + r.second - 1] + 7, F_ABSENT_SAME_START); query(xs[r.first], ys[r.first] - 1, F_ABSENT_SAME_START);
            const u32 k = rnd(r.second); if (k + 1 < r.second && ys[r.first + k] + 1 < ys[r.first + k + 1]) query(xs[r.first], ys[r.first + k] + 1, F_ABSENT_SAME_START);
            query(xs[r.first] + 1, ys[r.first], r.first + r.second == N ? F_ABOVE : F_BETWEEN);
        }
    }
    for (u32 k = 0; k < nSample; k++) { const u32 i = rnd(N); query(xs[i], ys[i], F_PRESENT); }
    for (u32 k = 0; k < 10; k++) { query(xs[0] - 1 - rnd(900), ys[0], F_BELOW); query(xs[N - 1] + 1 + rnd(1000), ys[N - 1], F_ABOVE); }
}

// ---- candidate logs and the sequential list -------------------------------------------------------------------------------------------------------------------------------------
// (Cand, asTr, randomBytes, layExons, candLogBytes and the sequential list itself: cand_log_ref.h, shared with oracle/tail_routines_check.cpp)
static void runLogs(SrsSet &S, u32 nLogs) {
    static const u32 NMAX[7] = {1, 3, 63, 64, 65, 100, 130};
    for (u32 il = 0; il < nLogs; il++) {
        const u32 fam = il % 3, Nmax = NMAX[rnd(7)], nCand = 10 + rnd(fam == 0 ? 120 : 420);
        const i32 range = rnd(4) == 0 ? (i32)rnd(6) : 1; const u32 chim = rnd(3) == 0; const i32 minIn[2] = {rnd(2) ? 0 : (i32)rnd(150), rnd(2) ? 0 : (i32)rnd(150)};
        nClass[fam == 0 ? R_FAM_OVERLAP : fam == 1 ? R_FAM_DISJOINT : R_FAM_NESTED]++;
        std::vector<Cand> cand(nCand);
        u64 diag[160]; const u32 nDiag = fam == 0 ? 2 + rnd(2) : 20 + rnd(140); for (u32 d = 0; d < nDiag; d++) diag[d] = 100000 + 1000ull * d + rnd(5);
        const u32 pattern = rnd(4); const i32 S0 = 60 + (i32)rnd(60);
        for (u32 k = 0; k < nCand; k++) {
            Cand &c = cand[k]; randomBytes(&c.t, sizeof(c.t)); memset(c.ex, 0, sizeof(c.ex));
            c.t.iW = k; c.t.iFrag = (i8)((int)rnd(3) - 1); c.t.gLength = 100 + rnd(pattern == 1 ? 8 : 5000); c.t.pad0 = 0; c.t.pad1 = 0;
            if (fam == 0) { layExons(c, 1 + rnd(rnd(3) ? 3 : SRS_NE_MAX), diag, nDiag, 150); c.t.maxScore = (i32)c.t.mappedLength - (i32)rnd(3); }
            else if (fam == 1) {             // never an overlap: a diagonal of its own.  Scores: rising slowly, constant (the genomic length decides), two values, anything (kept by the chimeric switch or dropped by the pre-filter)
                const u64 own = 900000 + 1000ull * k; layExons(c, 1 + rnd(rnd(4) ? 2 : SRS_NE_MAX), &own, 1, 150);
                c.t.maxScore = pattern == 0 ? S0 + (i32)(k / 3) : pattern == 1 ? S0 : pattern == 2 ? S0 - (i32)rnd(2) : 40 + (i32)rnd(100);
                if (pattern == 2 && k > nCand / 2) c.t.maxScore = S0 - 1; }
            else {                           // nested intervals on many diagonals: a longer one covers (removes) a shorter one deep in the list, a shorter one is blocked by a longer one at its head
                const u64 d = diag[rnd(nDiag)]; const u32 a = rnd(60), b = a + 20 + rnd(60), ne = rnd(5) ? 1 : 2;
                staramd_exon &e = c.ex[0]; randomBytes(&e, sizeof(e)); e.R = (u16)a; e.L = (u16)(b - a); e.G = d + a; e.pad0 = e.pad1 = 0; c.t.nExons = (u16)ne; c.t.mappedLength = b - a;
                if (ne == 2) { const u32 m = a + 1 + rnd(b - a - 1); staramd_exon &f = c.ex[1]; randomBytes(&f, sizeof(f)); f.pad0 = f.pad1 = 0; e.L = (u16)(m - a); f.R = (u16)m; f.L = (u16)(b - m); f.G = d + m; }
                c.t.maxScore = pattern == 3 ? 70 + (i32)rnd(3) : (i32)(b - a) - (i32)rnd(2);
                if (pattern != 3 && rnd(3)) c.t.maxScore = 80 - (i32)rnd(2) + (i32)(b - a) / 40; }
        }
        const u64 candOff = S.logPool.size(); candLogBytes(cand, S.logPool);
        // four runs of the log: the product's LDS arena in both forms, the product's large arena in global memory, the wide LDS arena
        for (u32 run = 0; run < 4; run++) {
            SrsLog g; memset(&g, 0, sizeof(g)); g.candOff = candOff; g.nCand = nCand; g.Nmax = Nmax; g.minIn[0] = minIn[0]; g.minIn[1] = minIn[1]; g.range = range; g.chim = chim;
            g.form = run == 0 ? 0u : run == 1 ? 1u : (il + run) & 1u; g.big = run == 2; g.arenaBytes = run < 2 ? 3584u : run == 2 ? 2u * (Nmax + 2u) * (96u + 32u * STARAMD_MAX_N_EXONS) : SRS_ARENA_WIDE;
            nClass[g.form ? R_FORM_WALK : R_FORM_REPLAY]++;
            // stitchWindowAligns.cpp:232-303 one candidate after the other, and the arena's book-keeping (cand_log_ref.h candLogSequential)
            CandLogStats st; const CandLogResult res = candLogSequential(cand, Nmax, range, chim != 0, minIn, g.arenaBytes, &st);
            const std::vector<u32> &list = res.list; const bool ovf = res.ovf;
            nClass[R_LIST_64] += st.list64; if (!g.big) nClass[R_LDS_LIST_64] += st.list64; nClass[R_LIST_128] += st.list128; nClass[R_TAIL] += st.tail; nClass[R_REMOVE_TRIP2] += st.removeTrip2;
            nClass[R_BEHIND_FULL] += st.behindFull; if (run < 2) { nClass[R_OVF_CLAUSE1] += st.ovfClause1; nClass[R_OVF_CLAUSE2] += st.ovfClause2; } nClass[R_COMPACT_FREES] += st.compactFrees;
            nClass[R_RANK0_OVER64] += st.rank0Over64; nClass[R_INSERT_FULL] += st.insertFull;
            g.expOverflow = ovf; g.expN = ovf ? 0 : (u32)list.size(); g.expBest = list.empty() ? 0 : cand[list[0]].t.maxScore; g.expOff = S.logExp.size();
            if (!ovf) S.logExp.insert(S.logExp.end(), list.begin(), list.end());
            if (run == 2 && !ovf) nClass[R_BIG_NO_OVF]++;
            S.log.push_back(g);
        }
    }
}

static void overlapTrials(SrsSet &S, u32 n) {
    for (u32 i = 0; i < n; i++) {
        u64 diag[3]; for (int d = 0; d < 3; d++) diag[d] = 5000 + 300ull * d;
        Cand a, b; memset(&a, 0, sizeof(a)); memset(&b, 0, sizeof(b));
        layExons(a, 1 + rnd(SRS_NE_MAX), diag, 1 + rnd(3), 40 + rnd(200)); layExons(b, 1 + rnd(SRS_NE_MAX), diag, 1 + rnd(3), 40 + rnd(200));
        SrsOvl o; memset(&o, 0, sizeof(o)); o.off1 = (u32)S.ovlEx.size(); o.n1 = a.t.nExons; S.ovlEx.insert(S.ovlEx.end(), a.ex, a.ex + o.n1); o.off2 = (u32)S.ovlEx.size(); o.n2 = b.t.nExons; S.ovlEx.insert(S.ovlEx.end(), b.ex, b.ex + o.n2);
        o.exp = (u32)Oracle::blocksOverlap(asTr(a.ex, o.n1, 0), asTr(b.ex, o.n2, 0));
        nClass[O_PAIRS]++; if (o.exp) nClass[O_NONZERO]++;
        S.ovl.push_back(o);
    }
}

// a routine that contradicts itself may loop for ever: reported, not waited for
static void onAlarm(int) { static const char msg[] = "\na routine does not end: 1 differences\n"; (void)!write(1, msg, sizeof(msg) - 1); _exit(1); }

int main(int argc, char **argv) {
    signal(SIGALRM, onAlarm); alarm(900);
    long scale = 100; const char *dumpPath = nullptr;
    for (int a = 1; a < argc; a++) { if (!strcmp(argv[a], "--dump") && a + 1 < argc) dumpPath = argv[++a]; else scale = atol(argv[a]); }
    if (dumpPath) scale = 25;                         // a few thousand cases per routine
    static SrsSet S;
    makeGenome(S); makeEnvs(S, 36);
    const u32 nJoin = (u32)(22000 * scale / 100);
    for (u32 t = 0; t < nJoin; t++) joinTrial(S, 2);
    static const u32 SIZES[12] = {1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 64 * 64 * 64 + 1};
    for (int k = 0; k < 12; k++) makeTable(S, SIZES[k], SIZES[k] > 4097, SIZES[k] > 4097 ? 1000 : 0);
    nClass[F_OFFSETS] = offsetsSeen.size();
    runLogs(S, (u32)(400 * scale / 100));
    overlapTrials(S, (u32)(20000 * scale / 100));
    if (dumpPath) { FILE *f = fopen(dumpPath, "wb"); if (!f) { perror(dumpPath); return 2; } srsWrite(f, S); if (fclose(f)) { perror(dumpPath); return 2; } }
    long bad = srsRun(S, true) + refBad;
    long empty = 0; u64 rarest = ~0ull;
    for (int c = 0; c < N_CLASSES; c++) { printf("  %-72s %llu\n", CLASS_NAME[c], (unsigned long long)nClass[c]); if (!nClass[c]) empty++; if (c != F_OFFSETS) rarest = std::min<u64>(rarest, nClass[c]); }
    if (nClass[F_OFFSETS] != 384) { printf("runs of equal starts: %llu of the 384 (length, first index mod 64) pairs were queried\n", (unsigned long long)nClass[F_OFFSETS]); empty++; }
    printf("rarest class: %llu cases\n", (unsigned long long)rarest);
    if (empty) { printf("%ld case classes never occurred\n", empty); bad += empty; }
    printf("%zu extensions, %zu joins, %zu look-ups x 3 over %zu tables, %zu exon list pairs, %zu runs of %zu candidate logs: %ld differences\n", S.ext.size(), S.join.size(), S.find.size(), S.tab.size(), S.ovl.size(), S.log.size(), S.log.size() / 4, bad);
    return bad ? 1 : 0;
}
