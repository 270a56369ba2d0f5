// stitch_routines_cases.h -- TEST INFRASTRUCTURE: the cases of oracle/stitch_routines_check.cpp, the probe kernels that run them and the comparison of what the kernels return with
// what the cases expect.  Included behind star_amd/csrc/engine/k_stitch.hip by the CPU check (host build through the wavefront emulator's headers: a launch is emu::launch) and by
// tests/stitch_routines_gpu.hip (hipcc, gfx950), so both run the same probes over the same records.  Every probe gives one wavefront to one case; blocks have 256 lanes, so three of
// four wavefronts work in an LDS slice that does not start at 0, as in the product.  Every lane writes what it holds of the results: they are wave-uniform state for the walk.
// The expected values of a case are the restatement's (oracle/lane_routines_ref.h, a linear scan, the sequential record list of the check), never the emulated routine's.
#pragma once
#include <cstdio>
#include <cstring>
#include <vector>

#define SRS_MAGIC 0x3153524853544954ull
#define SRS_READ_SLICE 1024u          // bytes of a wavefront's LDS slice for the 4-bit packed read (reads of up to 2000 bases)
#define SRS_NE_MAX 6u                 // exons of a synthetic candidate
#define SRS_REC_STRIDE (REC_HDR + 32u * SRS_NE_MAX)
#define SRS_ARENA_WIDE 24576u         // a test-only LDS arena that holds the longest lists: the multi-trip paths of recordCandidateImpl<false> on LDS pointers

struct SrsHead { u64 magic, nGenome, gBytes, nEnv, nSj, packedBytes, nExt, nJoin, nTab, nTabEntries, nFind, logBytes, nLog, nLogExp, nOvl, nOvlExons; };
struct SrsEnv { staramd_params P; u32 sjOff, sjN, useHash, pad; };                  // the junctions of an environment: a slice of the pooled arrays (sjN 0: none)
struct SrsRead { u32 env, rdOff, Lread, str, len0, mmMaxTotal; };                   // rdOff: byte offset of the packed read in the pool (multiple of 16)
struct SrsExt { SrsRead rd; u32 rStart; i32 dir; u64 gStart; u32 L, Lprev, nMMprev, nMMmax; double pMMmax; u32 toEnd, expRet; ExtRes exp; };
struct SrsExtOut { u32 ret; ExtRes e; };
struct SrsJoin { SrsRead rd; u32 rAend, rBstart, L, iFragB; i32 sjAB; u32 ex0R; u64 gAend, gBstart, ex0G; Hdr h; staramd_exon eA; i32 expScore; u32 expAdded; Hdr expH; staramd_exon expA, expN; };
struct SrsJoinOut { i32 score; u32 added; Hdr h; staramd_exon eA, eN; };
struct SrsTab { u64 off, hashOff; u32 N, mask; };                                   // off: into the pooled junction arrays of the tables; hashOff: into the pooled hash words
struct SrsFind { u64 x, y; u32 tab; i32 expIdx; };
struct SrsFindOut { i32 find, hash, one; u32 info; };                               // info: 0xFFFFFFFF when the table has no such junction
// a candidate log and how to run it.  form 0: replayWindow (header and exons as plain pointers into the log); 1: the walk's form of recordCandidate (header in the LDS staging
// slot, exons in the LDS rows of laneSetup).  big / arenaBytes: recordCandidateImpl<true> over an arena in global memory, or <false> over arenaBytes of LDS
struct SrsLog { u64 candOff; u32 nCand, Nmax; i32 minIn[2]; i32 range; u32 chim, form, big, arenaBytes, expN, expOverflow; i32 expBest; u64 expOff; };
struct SrsLogOut { u32 n, overflow; i32 best; u32 ok; };
struct SrsOvl { u32 off1, n1, off2, n2, exp, pad; };

// ---- probes ---------------------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void srsStage(StitchCtx &c, u32 lane, u32 wave, const DevIndex *envX, const u8 *packed, const SrsRead &rd) {
    memset(&c, 0, sizeof(c));
    c.X = envX + rd.env; c.ldsByte = wave * SRS_READ_SLICE; c.Lread = rd.Lread; c.str = rd.str; c.readLength[0] = rd.len0; c.mmMaxTotal = rd.mmMaxTotal;
    gcInit(c.ca); gcInit(c.cb);
    const u32 *src = (const u32 *)(packed + rd.rdOff); const u32 nw = ((rd.Lread + 16u) / 2u + 8u + 3u) / 4u;
    LDS u32 *dst = (LDS u32 *)((LDS u8 *)ldsReads + c.ldsByte);
    for (u32 k = lane; k < nw; k += NLANE) dst[k] = src[k];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
}

extern "C" __global__ void __launch_bounds__(256) k_srs_ext(const DevIndex *envX, const u8 *packed, const SrsExt *cs, u32 n, SrsExtOut *out) {
    const u32 lane = threadIdx.x & 63u, wave = WAVE_INDEX(threadIdx.x >> 6), i = blockIdx.x * 4u + wave;
    if (i >= n) return;
    const SrsExt s = cs[i];
    StitchCtx c; srsStage(c, lane, wave, envX, packed, s.rd);
    SrsExtOut o;
    o.ret = coopExtend(c, lane, s.rStart, s.gStart, s.dir, s.dir, s.L, s.Lprev, s.nMMprev, s.nMMmax, s.pMMmax, s.toEnd != 0, o.e) ? 1u : 0u;
    out[(u64)i * NLANE + lane] = o;
}

extern "C" __global__ void __launch_bounds__(256) k_srs_join(const DevIndex *envX, const u8 *packed, const SrsJoin *cs, u32 n, SrsJoinOut *out) {
    const u32 lane = threadIdx.x & 63u, wave = WAVE_INDEX(threadIdx.x >> 6), i = blockIdx.x * 4u + wave;
    if (i >= n) return;
    const SrsJoin s = cs[i];
    StitchCtx c; srsStage(c, lane, wave, envX, packed, s.rd);
    SrsJoinOut o; memset(&o, 0x5A, sizeof(o));
    o.h = s.h; o.eA = s.eA; bool added = false;
    o.score = coopStitch(c, lane, s.rAend, s.gAend, s.rBstart, s.gBstart, s.L, s.iFragB, s.sjAB, o.h, o.eA, o.eN, added, s.ex0R, s.ex0G);
    o.added = added ? 1u : 0u;
    out[(u64)i * NLANE + lane] = o;
}

extern "C" __global__ void __launch_bounds__(256) k_srs_find(const SrsTab *tabs, const u64 *xs, const u64 *ys, const u64 *hashWords, const SrsFind *cs, u32 n, SrsFindOut *out) {
    const u32 lane = threadIdx.x & 63u, wave = WAVE_INDEX(threadIdx.x >> 6), i = blockIdx.x * 4u + wave;
    if (i >= n) return;
    const SrsFind s = cs[i]; const SrsTab t = tabs[s.tab];
    SrsFindOut o; u32 info = 0xFFFFFFFFu;
    o.find = coopSjdbFind(lane, s.x, s.y, xs + t.off, ys + t.off, t.N);
    o.hash = coopSjdbHash(lane, s.x, s.y, hashWords + t.hashOff, t.mask, info);
    o.info = o.hash >= 0 ? info : 0xFFFFFFFFu;
    int one = -3;
    if (lane == 0) one = sjdbHashFind(hashWords + t.hashOff, t.mask, s.x, s.y);          // the one-lane routine of dev.h: run by one lane (64 walks of a long cluster are 64 times the emulator's time)
    o.one = (i32)first32((u32)one);
    out[(u64)i * NLANE + lane] = o;
}

extern "C" __global__ void __launch_bounds__(256) k_srs_overlap(const staramd_exon *ex, const SrsOvl *cs, u32 n, u32 *out) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const SrsOvl s = cs[i];
    out[i] = blocksOverlap(ex + s.off1, s.n1, ex + s.off2, s.n2);
}

// the decisions of replayWindow around the walk's form of recordCandidate: what finalizeTranscript hands over -- the header in the staging slot, the exon rows of the leaf copy
__device__ static bool srsWalkForm(const staramd_params &P, u32 lane, const DWinOut &o, const u8 *log, WinRec &wr, const LaneMem &m) {
    wr.nWinTr = 0; wr.top = 0; wr.overflow = false; wr.bestScore = 0;
    i32 M[2] = {o.minIn[0], o.minIn[1]};
    const u8 *p = log;
    for (u32 ic = 0; ic < o.nCand; ic++) {
        staramd_transcript t; memcpy(&t, p, REC_HDR);
        const u32 ne = t.nExons;
        staramd_exon x; memset(&x, 0, sizeof(x));
        if (lane < ne) memcpy(&x, p + REC_HDR + 32u * lane, 32);
        LOCKSTEP();                                        // (every lane is done with the rows of the candidate before)
        if (lane == 0) { const u64 *sw = (const u64 *)p; for (u32 i = 0; i < REC_HDR / 8; i++) m.rec[i] = sw[i]; }
        if (lane < ne) ldsPut(&m.LEAF[lane], x);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        p += REC_HDR + 32u * ne;
        const int Score = t.maxScore; const int f = t.iFrag;
        i32 Mf = 0;
        if (f == 0) { M[0] = max(M[0], Score); Mf = M[0]; } else if (f == 1) { M[1] = max(M[1], Score); Mf = M[1]; }
        const bool c1 = Score + P.outFilterMultimapScoreRange >= wr.bestScore || P.chimSegmentMinPositive;
        const bool c2 = f >= 0 && Score + P.outFilterMultimapScoreRange >= Mf;
        if (!(c1 || c2)) continue;
        recordCandidate(P, lane, Score, (u64)t.gLength, (u32)t.mappedLength, ne, m.rec, x, m.LEAF, wr);
        if (wr.overflow) return false;
    }
    return true;
}
template <bool BIG> __device__ static void srsCopyOut(u32 lane, const WinRec &wr, u64 *dst) {
    for (u32 k = 0; k < wr.nWinTr; k++) {
        typename AS<BIG>::trp r = recT<BIG>(wr, k);
        const u32 words = (REC_HDR + 32u * min((u32)r->nExons, SRS_NE_MAX)) / 8u;
        typename AS<BIG>::u64p s = (typename AS<BIG>::u64p)r;
        for (u32 w = lane; w < words; w += NLANE) dst[(u64)k * (SRS_REC_STRIDE / 8u) + w] = s[w];
    }
}
// sliceBytes: LDS of a wavefront (stitchStateBytes of the longest list and the arena of this launch); bigStride: bytes of global arena per case; recs: Nmax records of SRS_REC_STRIDE per case at recOff
extern "C" __global__ void __launch_bounds__(256) k_srs_record(const u8 *logPool, const SrsLog *cs, const u32 *pick, u32 n, u32 sliceBytes, u8 *bigArena, u64 bigStride, SrsLogOut *out, u64 *recs, const u64 *recOff) {
    const u32 lane = threadIdx.x & 63u, wave = WAVE_INDEX(threadIdx.x >> 6), j = blockIdx.x * 4u + wave;
    if (j >= n) return;
    const u32 i = pick[j];
    const SrsLog s = cs[i];
    staramd_params P; memset(&P, 0, sizeof(P));
    P.alignTranscriptsPerWindowNmax = s.Nmax; P.outFilterMultimapScoreRange = s.range; P.chimSegmentMinPositive = (u8)s.chim;
    LaneMem m; laneSetup((LDS u8 *)ldsReads + wave * sliceBytes, 0u, s.Nmax + 1u, m);
    WinRec wr; wr.rank = m.rank; wr.arenaL = m.arena; wr.arenaBytesL = s.big ? 0u : s.arenaBytes; wr.arenaG = bigArena + (u64)j * bigStride; wr.arenaBytesG = s.big ? s.arenaBytes : 0u;
    wr.big = s.big != 0; wr.arenaBytes = s.arenaBytes;
    DWinOut o; memset(&o, 0, sizeof(o)); o.minIn[0] = s.minIn[0]; o.minIn[1] = s.minIn[1]; o.nCand = s.nCand;
    const bool ok = s.form == 0 ? replayWindow(P, lane, o, logPool + s.candOff, wr) : srsWalkForm(P, lane, o, logPool + s.candOff, wr, m);
    SrsLogOut r; r.n = wr.nWinTr; r.overflow = wr.overflow ? 1u : 0u; r.best = wr.bestScore; r.ok = ok ? 1u : 0u;
    out[(u64)i * NLANE + lane] = r;
    if (!wr.overflow) { if (wr.big) srsCopyOut<true>(lane, wr, recs + recOff[i]); else srsCopyOut<false>(lane, wr, recs + recOff[i]); }
}

// ---- the whole set of cases, as the check makes it and the file holds it ------------------------------------------------------------------------------------------------
struct SrsSet {
    SrsHead head; std::vector<u8> gbuf; std::vector<SrsEnv> env; std::vector<u64> sjS, sjE; std::vector<u8> sjM, sjL, sjR, sjStr; std::vector<u8> packed;
    std::vector<SrsExt> ext; std::vector<SrsJoin> join; std::vector<SrsTab> tab; std::vector<u64> tS, tE; std::vector<u32> tInfo; std::vector<SrsFind> find;
    std::vector<u8> logPool; std::vector<SrsLog> log; std::vector<u32> logExp; std::vector<SrsOvl> ovl; std::vector<staramd_exon> ovlEx;
};
template <class T> static void srsPut(FILE *f, const std::vector<T> &v) { if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { perror("stitch routines: write"); exit(2); } }
template <class T> static void srsTake(FILE *f, std::vector<T> &v, size_t n) { v.resize(n); if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "case file: short read\n"); exit(2); } }
static void srsWrite(FILE *f, SrsSet &S) {
    SrsHead &h = S.head; memset(&h, 0, sizeof(h));
    h.magic = SRS_MAGIC; h.gBytes = S.gbuf.size(); h.nGenome = h.gBytes - 2 * GPAD; h.nEnv = S.env.size(); h.nSj = S.sjS.size(); h.packedBytes = S.packed.size(); h.nExt = S.ext.size(); h.nJoin = S.join.size();
    h.nTab = S.tab.size(); h.nTabEntries = S.tS.size(); h.nFind = S.find.size(); h.logBytes = S.logPool.size(); h.nLog = S.log.size(); h.nLogExp = S.logExp.size(); h.nOvl = S.ovl.size(); h.nOvlExons = S.ovlEx.size();
    if (fwrite(&h, sizeof(h), 1, f) != 1) { perror("stitch routines: write"); exit(2); }
    srsPut(f, S.gbuf); srsPut(f, S.env); srsPut(f, S.sjS); srsPut(f, S.sjE); srsPut(f, S.sjM); srsPut(f, S.sjL); srsPut(f, S.sjR); srsPut(f, S.sjStr); srsPut(f, S.packed); srsPut(f, S.ext); srsPut(f, S.join);
    srsPut(f, S.tab); srsPut(f, S.tS); srsPut(f, S.tE); srsPut(f, S.tInfo); srsPut(f, S.find); srsPut(f, S.logPool); srsPut(f, S.log); srsPut(f, S.logExp); srsPut(f, S.ovl); srsPut(f, S.ovlEx);
}
static void srsRead(FILE *f, SrsSet &S) {
    SrsHead &h = S.head;
    if (fread(&h, sizeof(h), 1, f) != 1 || h.magic != SRS_MAGIC) { fprintf(stderr, "not a case file of the stitch routines\n"); exit(2); }
    srsTake(f, S.gbuf, h.gBytes); srsTake(f, S.env, h.nEnv); srsTake(f, S.sjS, h.nSj); srsTake(f, S.sjE, h.nSj); srsTake(f, S.sjM, h.nSj); srsTake(f, S.sjL, h.nSj); srsTake(f, S.sjR, h.nSj); srsTake(f, S.sjStr, h.nSj);
    srsTake(f, S.packed, h.packedBytes); srsTake(f, S.ext, h.nExt); srsTake(f, S.join, h.nJoin); srsTake(f, S.tab, h.nTab); srsTake(f, S.tS, h.nTabEntries); srsTake(f, S.tE, h.nTabEntries); srsTake(f, S.tInfo, h.nTabEntries);
    srsTake(f, S.find, h.nFind); srsTake(f, S.logPool, h.logBytes); srsTake(f, S.log, h.nLog); srsTake(f, S.logExp, h.nLogExp); srsTake(f, S.ovl, h.nOvl); srsTake(f, S.ovlEx, h.nOvlExons);
}

// ---- running a set: device copies (plain copies under the emulator), one launch per routine and arena size, every lane of every case against the expected values ----------------
#define SRS_CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)
template <class T> static T *srsUp(const std::vector<T> &v, size_t extra = 64) {
    T *d = nullptr; const size_t b = v.size() * sizeof(T) + extra;
    SRS_CK(hipMalloc((void **)&d, b)); SRS_CK(hipMemset(d, 0, b)); if (!v.empty()) SRS_CK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
}
template <class T> static std::vector<T> srsDown(const T *d, size_t n) { std::vector<T> v(n); if (n) SRS_CK(hipMemcpy(v.data(), d, n * sizeof(T), hipMemcpyDeviceToHost)); return v; }
#define SRS_FAIL(...) do { if (bad++ < 24) printf(__VA_ARGS__); } while (0)

// the hash table of every table and environment comes from the product's own fill (dev.h sjdbHashFill), on both sides
static u32 srsHashMask(u32 n) { u32 slots = 128; while (slots < 2u * n) slots <<= 1; return slots - 1; }

// cases in parts of 4096: every lane's result comes back (64 records per case)
template <class O, class C, class Launch, class Differs> static void srsChunks(const std::vector<C> &cs, Launch launch, Differs differs) {
    const size_t CH = 4096;
    for (size_t at = 0; at < cs.size(); at += CH) {
        const u32 n = (u32)(cs.size() - at < CH ? cs.size() - at : CH);
        const std::vector<C> part(cs.begin() + at, cs.begin() + at + n);
        C *dC = srsUp(part); O *dO = nullptr; const size_t ob = ((size_t)n * NLANE + 1) * sizeof(O);
        SRS_CK(hipMalloc((void **)&dO, ob)); SRS_CK(hipMemset(dO, 0xEE, ob));
        launch((const C *)dC, n, dO);
        SRS_CK(hipGetLastError()); SRS_CK(hipDeviceSynchronize());
        const std::vector<O> o = srsDown(dO, (size_t)n * NLANE);
        for (u32 i = 0; i < n; i++) for (u32 l = 0; l < NLANE; l++) if (differs((u32)(at + i), l, o[(size_t)i * NLANE + l])) break;
        SRS_CK(hipFree(dC)); SRS_CK(hipFree(dO));
    }
}

static long srsRun(const SrsSet &S, bool quiet = false) {
    long bad = 0;
    // ---- the environments: one DevIndex each
    u8 *dG = srsUp(S.gbuf);
    u64 *dS = srsUp(S.sjS), *dE = srsUp(S.sjE); u8 *dM = srsUp(S.sjM), *dL = srsUp(S.sjL), *dR = srsUp(S.sjR), *dStr = srsUp(S.sjStr);
    std::vector<u32> info(S.sjS.size()); for (size_t k = 0; k < info.size(); k++) info[k] = SJ_INFO(S.sjM[k] & 7u, S.sjStr[k] & 3u, S.sjL[k], S.sjR[k]);
    u32 *dInfo = srsUp(info);
    std::vector<u64> envHash; std::vector<u64> envHashOff(S.env.size(), 0);
    for (size_t e = 0; e < S.env.size(); e++) if (S.env[e].sjN && S.env[e].useHash) {
        const SrsEnv &v = S.env[e]; const u32 mask = srsHashMask(v.sjN);
        envHashOff[e] = envHash.size(); envHash.resize(envHash.size() + 2 * ((size_t)mask + 1), 0);
        sjdbHashFill(envHash.data() + envHashOff[e], mask, S.sjS.data() + v.sjOff, S.sjE.data() + v.sjOff, S.sjM.data() + v.sjOff, S.sjStr.data() + v.sjOff, S.sjL.data() + v.sjOff, S.sjR.data() + v.sjOff, v.sjN);
    }
    u64 *dEnvHash = srsUp(envHash);
    std::vector<DevIndex> X(S.env.size());
    for (size_t e = 0; e < S.env.size(); e++) {
        const SrsEnv &v = S.env[e]; DevIndex &x = X[e]; memset(&x, 0, sizeof(x));
        x.G = dG + GPAD; x.nGenome = S.gbuf.size() - 2 * GPAD; x.P = v.P; x.sjdbN = v.sjN;
        if (v.sjN) { x.sjdbStart = dS + v.sjOff; x.sjdbEnd = dE + v.sjOff; x.sjdbMotif = dM + v.sjOff; x.sjdbShiftLeft = dL + v.sjOff; x.sjdbShiftRight = dR + v.sjOff; x.sjdbStrand = dStr + v.sjOff; x.sjdbInfo = dInfo + v.sjOff;
                     if (v.useHash) { x.sjdbHash = dEnvHash + envHashOff[e]; x.sjdbHashMask = srsHashMask(v.sjN); } }
    }
    DevIndex *dX = srsUp(X); u8 *dPacked = srsUp(S.packed);
    // ---- coopExtend
    srsChunks<SrsExtOut>(S.ext, [&](const SrsExt *dC, u32 n, SrsExtOut *dO) { hipLaunchKernelGGL(k_srs_ext, dim3((n + 3) / 4), dim3(256), 4 * SRS_READ_SLICE, 0, (const DevIndex *)dX, (const u8 *)dPacked, dC, n, dO); },
        [&](u32 i, u32 l, const SrsExtOut &r) { const SrsExt &c = S.ext[i];
            if (r.ret == c.expRet && r.e.maxScore == c.exp.maxScore && r.e.extendL == c.exp.extendL && r.e.nMatch == c.exp.nMatch && r.e.nMM == c.exp.nMM) return false;
            SRS_FAIL("EXTEND DIFF case %u lane %u: dir %d str %u toEnd %u rStart %u L %d Lread %u Lprev %u nMMprev %u nMMmax %u p %.2f: %u/%u score %d/%d len %u/%u nMatch %u/%u nMM %u/%u (routine / restatement)\n", i, l, c.dir, c.rd.str, c.toEnd, c.rStart, (int)c.L,
                     c.rd.Lread, c.Lprev, c.nMMprev, c.nMMmax, c.pMMmax, r.ret, c.expRet, r.e.maxScore, c.exp.maxScore, r.e.extendL, c.exp.extendL, r.e.nMatch, c.exp.nMatch, r.e.nMM, c.exp.nMM);
            return true; });
    // ---- coopStitch: the score; with a valid score the header, the exon it grew and the exon it added, byte for byte
    srsChunks<SrsJoinOut>(S.join, [&](const SrsJoin *dC, u32 n, SrsJoinOut *dO) { hipLaunchKernelGGL(k_srs_join, dim3((n + 3) / 4), dim3(256), 4 * SRS_READ_SLICE, 0, (const DevIndex *)dX, (const u8 *)dPacked, dC, n, dO); },
        [&](u32 i, u32 l, const SrsJoinOut &r) { const SrsJoin &c = S.join[i];
            bool diff = r.score != c.expScore;
            if (!diff && c.expScore > -1000000) diff = memcmp(&r.h, &c.expH, sizeof(Hdr)) != 0 || r.added != c.expAdded || memcmp(&r.eA, &c.expA, 32) != 0 || (c.expAdded && memcmp(&r.eN, &c.expN, 32) != 0);
            if (!diff) return false;
            SRS_FAIL("JOIN DIFF case %u lane %u: str %u rAend %u rBstart %u L %u gap g %lld iFragB %u sjAB %d: score %d/%d added %u/%u eA.L %u/%u canon %d/%d shift %u,%u / %u,%u annot %u/%u sjStr %u/%u nMM %u/%u nMatch %u/%u lGap %u/%u lDel %u/%u lIns %u/%u eN R %u/%u L %u/%u G %llu/%llu (routine / restatement)\n",
                     i, l, c.rd.str, c.rAend, c.rBstart, c.L, (long long)((i64)c.gBstart - (i64)c.gAend - 1), c.iFragB, c.sjAB, r.score, c.expScore, r.added, c.expAdded, r.eA.L, c.expA.L, r.eA.canonSJ, c.expA.canonSJ, r.eA.shiftSJ[0], r.eA.shiftSJ[1], c.expA.shiftSJ[0], c.expA.shiftSJ[1],
                     r.eA.sjAnnot, c.expA.sjAnnot, r.eA.sjStr, c.expA.sjStr, r.h.nMM, c.expH.nMM, r.h.nMatch, c.expH.nMatch, r.h.lGap, c.expH.lGap, r.h.lDel, c.expH.lDel, r.h.lIns, c.expH.lIns, r.eN.R, c.expN.R, r.eN.L, c.expN.L, (unsigned long long)r.eN.G, (unsigned long long)c.expN.G);
            return true; });
    // ---- the junction look-ups
    {
        std::vector<SrsTab> tab = S.tab; std::vector<u64> hw;
        for (SrsTab &t : tab) {
            t.mask = srsHashMask(t.N); t.hashOff = hw.size(); hw.resize(hw.size() + 2 * ((size_t)t.mask + 1), 0);
            std::vector<u8> m(t.N), st(t.N), sl(t.N), sr(t.N);
            for (u32 k = 0; k < t.N; k++) { const u32 v = S.tInfo[t.off + k]; m[k] = (u8)SJ_INFO_MOTIF(v); st[k] = (u8)SJ_INFO_STRAND(v); sl[k] = (u8)SJ_INFO_SHL(v); sr[k] = (u8)SJ_INFO_SHR(v); }
            sjdbHashFill(hw.data() + t.hashOff, t.mask, S.tS.data() + t.off, S.tE.data() + t.off, m.data(), st.data(), sl.data(), sr.data(), t.N);
        }
        SrsTab *dT = srsUp(tab); u64 *dXs = srsUp(S.tS), *dYs = srsUp(S.tE), *dH = srsUp(hw);
        srsChunks<SrsFindOut>(S.find, [&](const SrsFind *dC, u32 n, SrsFindOut *dO) { hipLaunchKernelGGL(k_srs_find, dim3((n + 3) / 4), dim3(256), 0, 0, (const SrsTab *)dT, (const u64 *)dXs, (const u64 *)dYs, (const u64 *)dH, dC, n, dO); },
            [&](u32 i, u32 l, const SrsFindOut &r) { const SrsFind &c = S.find[i];
                const u32 wantInfo = c.expIdx >= 0 ? S.tInfo[S.tab[c.tab].off + (u32)c.expIdx] : 0xFFFFFFFFu;
                if (r.find == c.expIdx && r.hash == c.expIdx && r.one == c.expIdx && r.info == wantInfo) return false;
                SRS_FAIL("LOOK-UP DIFF case %u lane %u: table of %u, (%llu, %llu): coopSjdbFind %d coopSjdbHash %d (info %08x) sjdbHashFind %d, linear scan %d (info %08x)\n", i, l, S.tab[c.tab].N, (unsigned long long)c.x, (unsigned long long)c.y, r.find, r.hash, r.info, r.one, c.expIdx, wantInfo);
                return true; });
        SRS_CK(hipFree(dT)); SRS_CK(hipFree(dXs)); SRS_CK(hipFree(dYs)); SRS_CK(hipFree(dH));
    }
    // ---- blocksOverlap
    {
        const u32 n = (u32)S.ovl.size(); staramd_exon *dEx = srsUp(S.ovlEx); SrsOvl *dC = srsUp(S.ovl); u32 *dO = nullptr; SRS_CK(hipMalloc((void **)&dO, ((size_t)n + 1) * 4)); SRS_CK(hipMemset(dO, 0xEE, ((size_t)n + 1) * 4));
        if (n) hipLaunchKernelGGL(k_srs_overlap, dim3((n + 255) / 256), dim3(256), 0, 0, (const staramd_exon *)dEx, (const SrsOvl *)dC, n, dO);
        SRS_CK(hipGetLastError()); SRS_CK(hipDeviceSynchronize());
        const std::vector<u32> o = srsDown(dO, n);
        for (u32 i = 0; i < n; i++) if (o[i] != S.ovl[i].exp) SRS_FAIL("OVERLAP DIFF case %u: %u, the oracle's %u\n", i, o[i], S.ovl[i].exp);
        SRS_CK(hipFree(dEx)); SRS_CK(hipFree(dC)); SRS_CK(hipFree(dO));
    }
    // ---- the record list: one launch per arena (the LDS of a launch is one size)
    {
        const u32 n = (u32)S.log.size(); u8 *dLog = srsUp(S.logPool); SrsLog *dC = srsUp(S.log);
        std::vector<u64> recOff(n + 1, 0); for (u32 i = 0; i < n; i++) recOff[i + 1] = recOff[i] + (u64)S.log[i].Nmax * (SRS_REC_STRIDE / 8u);
        u64 *dRecOff = srsUp(recOff); u64 *dRecs = nullptr; SRS_CK(hipMalloc((void **)&dRecs, (recOff[n] + 8) * 8)); SRS_CK(hipMemset(dRecs, 0xEE, (recOff[n] + 8) * 8));
        SrsLogOut *dO = nullptr; SRS_CK(hipMalloc((void **)&dO, ((size_t)n * NLANE + 1) * sizeof(SrsLogOut))); SRS_CK(hipMemset(dO, 0xEE, ((size_t)n * NLANE + 1) * sizeof(SrsLogOut)));
        for (u32 pass = 0; pass < 3; pass++) {              // 0: the product's LDS arena and smaller ones; 1: the wide LDS arena; 2: arenas in global memory
            std::vector<u32> pick; u32 arenaL = 0, nmax = 1; u64 bigStride = 0;
            for (u32 i = 0; i < n; i++) { const SrsLog &c = S.log[i]; const u32 p = c.big ? 2u : (c.arenaBytes > 8192u ? 1u : 0u); if (p != pass) continue; pick.push_back(i); nmax = max(nmax, c.Nmax);
                                          if (c.big) bigStride = max(bigStride, (u64)c.arenaBytes); else arenaL = max(arenaL, c.arenaBytes); }
            if (pick.empty()) continue;
            const u32 slice = stitchStateBytes(0u, nmax + 1u, arenaL);
            u32 *dPick = srsUp(pick); u8 *dBig = nullptr; SRS_CK(hipMalloc((void **)&dBig, (size_t)pick.size() * bigStride + 64));
#ifndef STARAMD_WAVE_EMUL
            SRS_CK(hipFuncSetAttribute((const void *)k_srs_record, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(4 * slice)));
#endif
            hipLaunchKernelGGL(k_srs_record, dim3(((u32)pick.size() + 3) / 4), dim3(256), 4 * (size_t)slice, 0, (const u8 *)dLog, (const SrsLog *)dC, (const u32 *)dPick, (u32)pick.size(), slice, dBig, bigStride, dO, dRecs, (const u64 *)dRecOff);
            SRS_CK(hipGetLastError()); SRS_CK(hipDeviceSynchronize());
            SRS_CK(hipFree(dPick)); SRS_CK(hipFree(dBig));
        }
        const std::vector<SrsLogOut> o = srsDown(dO, (size_t)n * NLANE); const std::vector<u64> recs = srsDown(dRecs, (size_t)recOff[n]);
        for (u32 i = 0; i < n; i++) {
            const SrsLog &c = S.log[i]; bool failed = false;
            for (u32 l = 0; l < NLANE && !failed; l++) {
                const SrsLogOut &r = o[(size_t)i * NLANE + l];
                if (r.overflow != c.expOverflow || r.ok != 1u - c.expOverflow || (!c.expOverflow && (r.n != c.expN || r.best != c.expBest))) {
                    failed = true; SRS_FAIL("RECORD LIST DIFF log %u lane %u (form %u, %s arena of %u bytes, list of %u at most, %u candidates): overflow %u/%u, %u/%u records, best score %d/%d (routine / sequential list)\n", i, l, c.form, c.big ? "global" : "LDS", c.arenaBytes, c.Nmax, c.nCand,
                                          r.overflow, c.expOverflow, r.n, c.expN, r.best, c.expBest); }
            }
            if (failed || c.expOverflow) continue;
            std::vector<u64> candAt(c.nCand); { u64 p = c.candOff; for (u32 k = 0; k < c.nCand; k++) { candAt[k] = p; staramd_transcript t; memcpy(&t, S.logPool.data() + p, REC_HDR); p += REC_HDR + 32u * t.nExons; } }
            for (u32 k = 0; k < c.expN; k++) {
                const u8 *want = S.logPool.data() + candAt[S.logExp[c.expOff + k]]; staramd_transcript t; memcpy(&t, want, REC_HDR);
                if (memcmp(&recs[recOff[i] + (u64)k * (SRS_REC_STRIDE / 8u)], want, REC_HDR + 32u * t.nExons) != 0) {
                    staramd_transcript g; memcpy(&g, &recs[recOff[i] + (u64)k * (SRS_REC_STRIDE / 8u)], REC_HDR);
                    SRS_FAIL("RECORD LIST DIFF log %u (form %u, %s arena of %u bytes, list of %u at most): rank %u holds candidate %u (score %d), the sequential list candidate %u (score %d)\n", i, c.form, c.big ? "global" : "LDS", c.arenaBytes, c.Nmax, k, g.iW, g.maxScore, t.iW, t.maxScore);
                    break; }
            }
        }
        SRS_CK(hipFree(dLog)); SRS_CK(hipFree(dC)); SRS_CK(hipFree(dRecOff)); SRS_CK(hipFree(dRecs)); SRS_CK(hipFree(dO));
    }
    SRS_CK(hipFree(dG)); SRS_CK(hipFree(dS)); SRS_CK(hipFree(dE)); SRS_CK(hipFree(dM)); SRS_CK(hipFree(dL)); SRS_CK(hipFree(dR)); SRS_CK(hipFree(dStr)); SRS_CK(hipFree(dInfo)); SRS_CK(hipFree(dEnvHash)); SRS_CK(hipFree(dX)); SRS_CK(hipFree(dPacked));
    if (!quiet) printf("%zu extensions, %zu joins, %zu look-ups x 3 over %zu tables, %zu exon list pairs, %zu candidate logs: %ld differences\n", S.ext.size(), S.join.size(), S.find.size(), S.tab.size(), S.ovl.size(), S.log.size(), bad);
    return bad;
}
