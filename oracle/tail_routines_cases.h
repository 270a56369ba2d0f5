// tail_routines_cases.h -- TEST INFRASTRUCTURE: the cases of oracle/tail_routines_check.cpp, the launches that run them and the comparison of what the kernels left with what the
// cases expect.  Included behind star_amd/csrc/engine/k_stitch.hip and k_gather.hip by the CPU check (host build through the wavefront emulator's headers: a launch is emu::launch)
// and by tests/tail_routines_gpu.hip (hipcc, gfx950), so both run the same launches of k_pack_reads, k_stitch_verify, k_stitch_replay, k_stitch_finish, k_scan_local,
// k_scan_offsets and k_gather over the same records.  Every buffer a kernel may write lies between guard bytes that are verified after each launch and is filled with 0xA5 before
// it, so that "not written" is a comparison like any other.  The expected values of a case are the check's restatements of the oracle's rules, never an emulated kernel's.
#pragma once
#include <cstdio>
#include <cstring>
#include <vector>
#include <chrono>
#include <algorithm>

#define TRS_MAGIC 0x31304c4941545254ull        // "TRTAIL01"
#define TRS_GUARD 4096u                        // guard bytes either side of every buffer
#define TRS_FILL 0xA5
#define TRS_FILL32 0xA5A5A5A5u
#define TRS_REPLAY_BLOCKS 2u                   // k_stitch_replay: 2 blocks of 4 wavefronts, fewer than the longest item list

enum { TRS_VERIFY, TRS_REPLAY, TRS_FINISH, TRS_SCANLOCAL, TRS_TAIL, TRS_FLAGS };
struct TrsHead { u64 magic; u32 szRead, szWout, szTr, szEx, szParams, szBatch, szWinExp, pad; };
struct TrsEnv { staramd_params P; };
struct TrsPack { u32 packWords, nReads, offOff, baseOff, nBases, expOff; };      // offOff: nReads + 1 entries of S.packOffset; expOff: nReads * packWords words of S.packExp
struct TrsScan { u32 nBlocks, totOff, pad0, pad1; };                             // 2 * nBlocks words of S.scanTot; S.scanExp holds, case after case, the 2 * nBlocks bases and the two totals
// what a replayed window must leave: nTr records (header + exon rows, exonOffset relative to the window) at recOff of S.recExp
struct TrsWinExp { u32 w, hard, nTr, nEx; i32 headScore; u32 pad; u64 headGlen, recOff; };
struct TrsBatch {
    u32 kind, env, readOff, nReads, woutOff, nWout, trOff, nTrPool, exOff, nExPool;
    u64 candOff, candBytes;
    u32 listOff, nList;                        // TRS_REPLAY: the replay list as given
    u32 trCap, exCap, arenaL, arenaG, outTrCap, outExCap, flags0, expFlags;
    u32 expReadOff, expWoutOff;                // S.readExp[nReads], S.woutExp[nWout]
    u32 expListOff, expNRedo, expNReplay;      // S.listExp: the redo list sorted, then the replay list sorted
    u32 expWinOff, nWinExp;                    // S.winExp
    u32 expRROff, expOutTrOff, expNOutTr, expOutExOff, expNOutEx;
    u32 expScanOff;                            // S.scanLocalExp: trBase[nReads], exBase[nReads], blockTot[2 * blocks]
    u32 lenOff; u64 expTrOut;                  // lenOff: nReads + 1 entries of S.readLen
};

#define TRS_FIELDS(F) F(env) F(packOffset) F(packBases) F(packExp) F(pack) F(scanTot) F(scanExp) F(scan) F(read) F(readLen) F(mate1) F(wout) F(tr) F(ex) F(cand) F(list) \
                      F(readExp) F(woutExp) F(listExp) F(winExp) F(recExp) F(rrExp) F(outTr) F(outEx) F(scanLocalExp) F(batch)
struct TrsSet {
    std::vector<TrsEnv> env; std::vector<u64> packOffset; std::vector<u8> packBases; std::vector<u32> packExp; std::vector<TrsPack> pack;
    std::vector<u32> scanTot, scanExp; std::vector<TrsScan> scan;
    std::vector<DRead> read; std::vector<u64> readLen; std::vector<u16> mate1; std::vector<DWinOut> wout; std::vector<staramd_transcript> tr; std::vector<staramd_exon> ex; std::vector<u8> cand; std::vector<u32> list;
    std::vector<DRead> readExp; std::vector<DWinOut> woutExp; std::vector<u32> listExp; std::vector<TrsWinExp> winExp; std::vector<u8> recExp; std::vector<staramd_read_result> rrExp;
    std::vector<staramd_transcript> outTr; std::vector<staramd_exon> outEx; std::vector<u32> scanLocalExp; std::vector<TrsBatch> batch;
};
static TrsHead trsHead() { TrsHead h; memset(&h, 0, sizeof(h)); h.magic = TRS_MAGIC; h.szRead = sizeof(DRead); h.szWout = sizeof(DWinOut); h.szTr = sizeof(staramd_transcript); h.szEx = sizeof(staramd_exon);
    h.szParams = sizeof(staramd_params); h.szBatch = sizeof(TrsBatch); h.szWinExp = sizeof(TrsWinExp); return h; }
template <class T> static void trsPut(FILE *f, const std::vector<T> &v) { const u64 n = v.size(); if (fwrite(&n, 8, 1, f) != 1 || (n && fwrite(v.data(), sizeof(T), n, f) != n)) { perror("tail routines: write"); exit(2); } }
template <class T> static void trsTake(FILE *f, std::vector<T> &v) { u64 n = 0; if (fread(&n, 8, 1, f) != 1 || n > (1ull << 32)) { fprintf(stderr, "case file: short read\n"); exit(2); } v.resize(n); if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "case file: short read\n"); exit(2); } }
static void trsWrite(FILE *f, const TrsSet &S) {
    const TrsHead h = trsHead(); if (fwrite(&h, sizeof(h), 1, f) != 1) { perror("tail routines: write"); exit(2); }
#define F(x) trsPut(f, S.x);
    TRS_FIELDS(F)
#undef F
}
static void trsReadFile(FILE *f, TrsSet &S) {
    TrsHead h; const TrsHead want = trsHead(); if (fread(&h, sizeof(h), 1, f) != 1 || memcmp(&h, &want, sizeof(h)) != 0) { fprintf(stderr, "not a case file of the tail routines (magic or record sizes)\n"); exit(2); }
#define F(x) trsTake(f, S.x);
    TRS_FIELDS(F)
#undef F
}

// ---- buffers between guards ---------------------------------------------------------------------------------------------------------------------------------------------
#define TRS_CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)
#define TRS_FAIL(...) do { if (bad++ < 40) printf(__VA_ARGS__); } while (0)
struct TrsBuf { u8 *raw = nullptr; size_t n = 0; const char *name = ""; template <class T> T *as() const { return (T *)(raw + TRS_GUARD); } };
// n bytes of `fill` between two guards of 0xEE; the first srcBytes from src
static TrsBuf trsAlloc(const char *name, size_t n, int fill, const void *src = nullptr, size_t srcBytes = 0) {
    TrsBuf b; b.n = n; b.name = name;
    TRS_CK(hipMalloc((void **)&b.raw, n + 2 * TRS_GUARD)); TRS_CK(hipMemset(b.raw, 0xEE, TRS_GUARD)); TRS_CK(hipMemset(b.raw + TRS_GUARD + n, 0xEE, TRS_GUARD));
    if (n) TRS_CK(hipMemset(b.raw + TRS_GUARD, fill, n));
    if (srcBytes) TRS_CK(hipMemcpy(b.raw + TRS_GUARD, src, srcBytes, hipMemcpyHostToDevice));
    return b;
}
template <class T> static TrsBuf trsUp(const char *name, const std::vector<T> &v, size_t from, size_t count, size_t room = 0) {
    return trsAlloc(name, std::max(count, room) * sizeof(T), TRS_FILL, count ? v.data() + from : nullptr, count * sizeof(T));
}
template <class T> static std::vector<T> trsDown(const TrsBuf &b, size_t n) { std::vector<T> v(n); if (n) TRS_CK(hipMemcpy(v.data(), b.raw + TRS_GUARD, n * sizeof(T), hipMemcpyDeviceToHost)); return v; }
static long trsGuardsBad(const TrsBuf &b) {
    static std::vector<u8> gv(2 * TRS_GUARD); u8 *g = gv.data(); TRS_CK(hipMemcpy(g, b.raw, TRS_GUARD, hipMemcpyDeviceToHost)); TRS_CK(hipMemcpy(g + TRS_GUARD, b.raw + TRS_GUARD + b.n, TRS_GUARD, hipMemcpyDeviceToHost));
    long n = 0; for (u32 k = 0; k < 2 * TRS_GUARD; k++) if (g[k] != 0xEE) n++;
    return n;
}
static void trsFree(TrsBuf &b) { if (b.raw) TRS_CK(hipFree(b.raw)); b.raw = nullptr; }
static bool trsAllFill(const void *p, size_t n) { const u8 *b = (const u8 *)p; for (size_t i = 0; i < n; i++) if (b[i] != TRS_FILL) return false; return true; }
// after a launch: the HIP error state, then every guard
static long trsAfterLaunch(const char *what, u32 ib, const std::vector<TrsBuf *> &all) {
    long bad = 0; TRS_CK(hipGetLastError()); TRS_CK(hipDeviceSynchronize());
    for (const TrsBuf *b : all) { const long gb = trsGuardsBad(*b); if (gb) TRS_FAIL("CASE %u after %s: %ld guard bytes around %s were written\n", ib, what, gb, b->name); }
    return bad;
}

static size_t trsCompared = 0;          // cases launched and compared
// ---- A: k_pack_reads as engine.hip launches it (one block of 64 lanes per read) -------------------------------------------------------------------------------------------
static long trsRunPack(const TrsSet &S, u32 ic) {
    long bad = 0; const TrsPack &c = S.pack[ic];
    TrsBuf bOff = trsUp("readOffset", S.packOffset, c.offOff, c.nReads + 1), bBases = trsUp("bases", S.packBases, c.baseOff, c.nBases, 1);
    TrsBuf bPacked = trsAlloc("packed", ((size_t)c.nReads + 1) * c.packWords * 4, TRS_FILL);          // one row more than reads: it keeps its fill
    DevBatch B; memset(&B, 0, sizeof(B)); B.nReads = c.nReads; B.bases = bBases.as<u8>(); B.readOffset = bOff.as<u64>();
    hipLaunchKernelGGL(k_pack_reads, dim3(c.nReads), dim3(64), 0, 0, B, bPacked.as<u32>(), c.packWords);
    bad += trsAfterLaunch("k_pack_reads", ic, {&bOff, &bBases, &bPacked});
    const std::vector<u32> o = trsDown<u32>(bPacked, ((size_t)c.nReads + 1) * c.packWords);
    for (u32 r = 0; r < c.nReads; r++) for (u32 w = 0; w < c.packWords; w++) if (o[(size_t)r * c.packWords + w] != S.packExp[c.expOff + (size_t)r * c.packWords + w]) {
        TRS_FAIL("PACK DIFF case %u read %u (length %llu) word %u of %u: %08x, wanted %08x\n", ic, r, (unsigned long long)(S.packOffset[c.offOff + r + 1] - S.packOffset[c.offOff + r]), w, c.packWords, o[(size_t)r * c.packWords + w], S.packExp[c.expOff + (size_t)r * c.packWords + w]); break; }
    if (!trsAllFill(o.data() + (size_t)c.nReads * c.packWords, (size_t)c.packWords * 4)) TRS_FAIL("PACK DIFF case %u: the row behind the last read was written\n", ic);
    trsFree(bOff); trsFree(bBases); trsFree(bPacked); trsCompared++;
    return bad;
}

// ---- E: k_scan_offsets on block totals made by hand -----------------------------------------------------------------------------------------------------------------------
// S.scanExp holds, per case and in the order of the cases, 2 * nBlocks bases and the two totals
static long trsRunScan(const TrsSet &S, u32 ic, size_t expOff) {
    long bad = 0; const TrsScan &c = S.scan[ic];
    TrsBuf bTot = trsUp("blockTot", S.scanTot, c.totOff, 2 * (size_t)c.nBlocks), bTotals = trsAlloc("totals", 8, TRS_FILL), bCur = trsAlloc("cursors", CUR_N * 4, 0);
    DevBatch B; memset(&B, 0, sizeof(B)); B.cursors = bCur.as<u32>();
    hipLaunchKernelGGL(k_scan_offsets, dim3(1), dim3(1024), 0, 0, B, bTot.as<u32>(), c.nBlocks, bTotals.as<u32>());
    bad += trsAfterLaunch("k_scan_offsets", ic, {&bTot, &bTotals, &bCur});
    const std::vector<u32> o = trsDown<u32>(bTot, 2 * (size_t)c.nBlocks), t = trsDown<u32>(bTotals, 2);
    for (u32 k = 0; k < 2 * c.nBlocks; k++) if (o[k] != S.scanExp[expOff + k]) { TRS_FAIL("SCAN DIFF case %u (%u blocks): base %u of block %u is %u, wanted %u\n", ic, c.nBlocks, k & 1u, k / 2, o[k], S.scanExp[expOff + k]); break; }
    if (t[0] != S.scanExp[expOff + 2 * c.nBlocks] || t[1] != S.scanExp[expOff + 2 * c.nBlocks + 1]) TRS_FAIL("SCAN DIFF case %u (%u blocks): totals %u %u, wanted %u %u\n", ic, c.nBlocks, t[0], t[1], S.scanExp[expOff + 2 * c.nBlocks], S.scanExp[expOff + 2 * c.nBlocks + 1]);
    trsFree(bTot); trsFree(bTotals); trsFree(bCur); trsCompared++;
    return bad;
}

// ---- B, C, D, E (k_scan_local), F: one batch ------------------------------------------------------------------------------------------------------------------------------
static double trsSecondsBatches[6];
static long trsRunBatch(const TrsSet &S, const TrsBuf &bX, u32 ib) {
    long bad = 0; const auto t0 = std::chrono::steady_clock::now();
    const TrsBatch &b = S.batch[ib]; const staramd_params &P = S.env[b.env].P; const u32 nR = b.nReads, nBlk = (nR + 255u) / 256u;
    const DevIndex *dX = bX.as<DevIndex>() + b.env;
    TrsBuf bReads = trsUp("reads", S.read, b.readOff, nR), bOff = trsUp("readOffset", S.readLen, b.lenOff, nR + 1), bMate = trsUp("mate1Length", S.mate1, b.readOff, nR, 1);
    TrsBuf bWout = trsUp("wout", S.wout, b.woutOff, b.nWout), bTr = trsUp("trPool", S.tr, b.trOff, b.nTrPool, b.trCap), bEx = trsUp("exPool", S.ex, b.exOff, b.nExPool, b.exCap);
    TrsBuf bCand = trsUp("candPool", S.cand, (size_t)b.candOff, (size_t)b.candBytes, 32);
    TrsBuf bRedo = trsAlloc("redoList", (size_t)b.nWout * 4, TRS_FILL), bReplay = trsAlloc("replayList", (size_t)b.nWout * 4, TRS_FILL, b.nList ? S.list.data() + b.listOff : nullptr, (size_t)b.nList * 4);
    TrsBuf bCur = trsAlloc("cursors", CUR_N * 4, 0), bCnt = trsAlloc("counters", DC_N * 8, 0);
    TrsBuf bTrBase = trsAlloc("trBase", (size_t)nR * 4, TRS_FILL), bExBase = trsAlloc("exBase", (size_t)nR * 4, TRS_FILL), bBlockTot = trsAlloc("blockTot", (size_t)nBlk * 8, TRS_FILL), bTotals = trsAlloc("totals", 8, TRS_FILL);
    TrsBuf bOutR = trsAlloc("outReads", (size_t)nR * sizeof(staramd_read_result), TRS_FILL), bOutT = trsAlloc("outTr", (size_t)b.outTrCap * sizeof(staramd_transcript), TRS_FILL), bOutE = trsAlloc("outEx", (size_t)b.outExCap * sizeof(staramd_exon), TRS_FILL);
    TrsBuf bArena = trsAlloc("arena in global memory", (size_t)TRS_REPLAY_BLOCKS * 4 * b.arenaG, TRS_FILL);
    const std::vector<TrsBuf *> all = {&bReads, &bOff, &bMate, &bWout, &bTr, &bEx, &bCand, &bRedo, &bReplay, &bCur, &bCnt, &bTrBase, &bExBase, &bBlockTot, &bTotals, &bOutR, &bOutT, &bOutE, &bArena};
    { std::vector<u32> cur(CUR_N, 0); cur[CUR_TR] = b.nTrPool; cur[CUR_EX] = b.nExPool; cur[CUR_FLAGS] = b.flags0; cur[CUR_ST_REPLAY] = b.nList; TRS_CK(hipMemcpy(bCur.as<u32>(), cur.data(), CUR_N * 4, hipMemcpyHostToDevice)); }
    DevBatch B; memset(&B, 0, sizeof(B));
    B.nReads = nR; B.readOffset = bOff.as<u64>(); B.mate1Length = bMate.as<u16>(); B.reads = bReads.as<DRead>(); B.wout = bWout.as<DWinOut>(); B.winCap = b.nWout;
    B.trPool = bTr.as<staramd_transcript>(); B.trCap = b.trCap; B.exPool = bEx.as<staramd_exon>(); B.exCap = b.exCap; B.redoList = bRedo.as<u32>(); B.replayList = bReplay.as<u32>();
    B.candPool = bCand.as<u8>(); B.cursors = bCur.as<u32>(); B.counters = bCnt.as<u64>();
    const dim3 perRead(nBlk), block(256); const u32 capRank = P.alignTranscriptsPerWindowNmax + 1u;
    const bool chain = b.kind == TRS_TAIL || b.kind == TRS_FLAGS;
    // the launch shapes of engine.hip (the stitch stage behind pass 0, then the gather stage)
    if (b.kind == TRS_VERIFY || chain) { hipLaunchKernelGGL(k_stitch_verify, perRead, block, 0, 0, dX, B); bad += trsAfterLaunch("k_stitch_verify", ib, all); }
    if (b.kind == TRS_REPLAY || chain) {
        hipLaunchKernelGGL(k_stitch_replay, dim3(TRS_REPLAY_BLOCKS), block, 4 * (size_t)stitchStateBytes(0u, capRank, b.arenaL), 0, dX, B, bArena.as<u8>(), 0u, capRank, b.arenaL, b.arenaG, 0u);
        bad += trsAfterLaunch("k_stitch_replay", ib, all);
    }
    if (b.kind == TRS_FINISH || chain) { hipLaunchKernelGGL(k_stitch_finish, perRead, block, 0, 0, dX, B); bad += trsAfterLaunch("k_stitch_finish", ib, all); }
    if (b.kind == TRS_SCANLOCAL || chain) { hipLaunchKernelGGL(k_scan_local, perRead, block, 0, 0, B, bTrBase.as<u32>(), bExBase.as<u32>(), bBlockTot.as<u32>()); bad += trsAfterLaunch("k_scan_local", ib, all); }
    if (chain) {
        hipLaunchKernelGGL(k_scan_offsets, dim3(1), dim3(1024), 0, 0, B, bBlockTot.as<u32>(), nBlk, bTotals.as<u32>()); bad += trsAfterLaunch("k_scan_offsets", ib, all);
        hipLaunchKernelGGL(k_gather, perRead, block, 0, 0, B, (const u32 *)bTrBase.as<u32>(), (const u32 *)bExBase.as<u32>(), (const u32 *)bBlockTot.as<u32>(), bOutR.as<staramd_read_result>(), bOutT.as<staramd_transcript>(), b.outTrCap,
                           bOutE.as<staramd_exon>(), b.outExCap);
        bad += trsAfterLaunch("k_gather", ib, all);
    }
    // ---- what they left
    const std::vector<u32> cur = trsDown<u32>(bCur, CUR_N); const std::vector<u64> cnt = trsDown<u64>(bCnt, DC_N);
    const std::vector<DRead> reads = trsDown<DRead>(bReads, nR); const std::vector<DWinOut> wout = trsDown<DWinOut>(bWout, b.nWout);
    const std::vector<staramd_transcript> tr = trsDown<staramd_transcript>(bTr, b.trCap); const std::vector<staramd_exon> ex = trsDown<staramd_exon>(bEx, b.exCap);
    std::vector<u32> redo = trsDown<u32>(bRedo, b.nWout), replay = trsDown<u32>(bReplay, b.nWout);
    const DRead *readIn = S.read.data() + b.readOff; const DWinOut *woutIn = S.wout.data() + b.woutOff;
    if (cur[CUR_FLAGS] != b.expFlags) TRS_FAIL("CASE %u (kind %u): flags %x, wanted %x\n", ib, b.kind, cur[CUR_FLAGS], b.expFlags);
    const bool poolsAsGiven = b.kind != TRS_REPLAY && b.kind != TRS_TAIL;
    if (poolsAsGiven) {
        if (b.nTrPool && memcmp(tr.data(), S.tr.data() + b.trOff, (size_t)b.nTrPool * sizeof(staramd_transcript)) != 0) TRS_FAIL("CASE %u (kind %u): trPool was changed\n", ib, b.kind);
        if (b.nExPool && memcmp(ex.data(), S.ex.data() + b.exOff, (size_t)b.nExPool * sizeof(staramd_exon)) != 0) TRS_FAIL("CASE %u (kind %u): exPool was changed\n", ib, b.kind);
        if (!trsAllFill(tr.data() + b.nTrPool, (size_t)(b.trCap - b.nTrPool) * sizeof(staramd_transcript)) || !trsAllFill(ex.data() + b.nExPool, (size_t)(b.exCap - b.nExPool) * sizeof(staramd_exon))) TRS_FAIL("CASE %u (kind %u): the pools were written behind their records\n", ib, b.kind);
        if (cur[CUR_TR] != b.nTrPool || cur[CUR_EX] != b.nExPool) TRS_FAIL("CASE %u (kind %u): CUR_TR / CUR_EX %u %u, given %u %u\n", ib, b.kind, cur[CUR_TR], cur[CUR_EX], b.nTrPool, b.nExPool);
    }
    if (b.kind == TRS_VERIFY || b.kind == TRS_TAIL) {
        // the lists as sorted multisets (their order is that of the atomics), the cursors, the counters; behind the lists nothing
        const u32 nRedo = cur[CUR_ST_REDO], nReplay = cur[CUR_ST_REPLAY];
        if (nRedo != b.expNRedo || nReplay != b.expNReplay) TRS_FAIL("VERIFY DIFF case %u: %u windows to walk again and %u to replay, wanted %u and %u\n", ib, nRedo, nReplay, b.expNRedo, b.expNReplay);
        else {
            std::sort(redo.begin(), redo.begin() + nRedo); std::sort(replay.begin(), replay.begin() + nReplay);
            for (u32 k = 0; k < nRedo; k++) if (redo[k] != S.listExp[b.expListOff + k]) { TRS_FAIL("VERIFY DIFF case %u: entry %u of the sorted redo list is window %u, wanted %u\n", ib, k, redo[k], S.listExp[b.expListOff + k]); break; }
            for (u32 k = 0; k < nReplay; k++) if (replay[k] != S.listExp[b.expListOff + b.expNRedo + k]) { TRS_FAIL("VERIFY DIFF case %u: entry %u of the sorted replay list is window %u, wanted %u\n", ib, k, replay[k], S.listExp[b.expListOff + b.expNRedo + k]); break; }
            if (!trsAllFill(redo.data() + nRedo, (size_t)(b.nWout - nRedo) * 4) || !trsAllFill(replay.data() + nReplay, (size_t)(b.nWout - nReplay) * 4)) TRS_FAIL("VERIFY DIFF case %u: a list was written behind its count\n", ib);
        }
        if (cnt[DC_nRedoWin] != b.expNRedo || cnt[DC_nReplayWin] != b.expNReplay) TRS_FAIL("VERIFY DIFF case %u: DC_nRedoWin %llu DC_nReplayWin %llu, wanted %u %u\n", ib, (unsigned long long)cnt[DC_nRedoWin], (unsigned long long)cnt[DC_nReplayWin], b.expNRedo, b.expNReplay);
    }
    if (b.kind == TRS_VERIFY) {
        for (u32 w = 0; w < b.nWout; w++) if (memcmp(&wout[w], &S.woutExp[b.expWoutOff + w], sizeof(DWinOut)) != 0) { const DWinOut &x = wout[w], &y = S.woutExp[b.expWoutOff + w];
            TRS_FAIL("VERIFY DIFF case %u window %u (sens %d %d): minIn %d %d, wanted %d %d%s\n", ib, w, y.sens[0], y.sens[1], x.minIn[0], x.minIn[1], y.minIn[0], y.minIn[1], x.minIn[0] == y.minIn[0] && x.minIn[1] == y.minIn[1] ? " (other bytes differ)" : ""); break; }
        if (nR && memcmp(reads.data(), readIn, (size_t)nR * sizeof(DRead)) != 0) TRS_FAIL("VERIFY DIFF case %u: reads were changed\n", ib);
    }
    if (b.kind == TRS_REPLAY) {
        std::vector<u32> useT(b.trCap, 0), useE(b.exCap, 0); u32 sumT = 0, sumE = 0, nKept = 0; std::vector<u8> listed(b.nWout, 0);
        const bool shortPool = (b.expFlags & OVF_TRPOOL) != 0;
        for (u32 k = 0; k < b.nWinExp; k++) {
            const TrsWinExp &e = S.winExp[b.expWinOff + k]; const DWinOut &o = wout[e.w]; listed[e.w] = 1;
            const bool asGiven = memcmp(&o, &woutIn[e.w], sizeof(DWinOut)) == 0;
            if (e.hard) { if (!asGiven) TRS_FAIL("REPLAY DIFF case %u window %u: fits neither arena and its DWinOut was changed\n", ib, e.w); continue; }
            if (shortPool && asGiven) { nKept++; continue; }                            // (the window that met the end of the pool: which one is up to the atomics)
            DWinOut z = o; z.trOffset = woutIn[e.w].trOffset; z.nTr = woutIn[e.w].nTr; z.exOffset = woutIn[e.w].exOffset; z.nEx = woutIn[e.w].nEx; z.headScore = woutIn[e.w].headScore; z.headGlen = woutIn[e.w].headGlen;
            if (memcmp(&z, &woutIn[e.w], sizeof(DWinOut)) != 0) TRS_FAIL("REPLAY DIFF case %u window %u: mm / sens / minIn / candOff32 / nCand were changed\n", ib, e.w);
            if (o.nTr != e.nTr || o.nEx != e.nEx || o.headScore != (e.nTr ? e.headScore : 0) || o.headGlen != (e.nTr ? e.headGlen : 0)) { TRS_FAIL("REPLAY DIFF case %u window %u: %u transcripts %u exons head %d / %llu, wanted %u %u %d / %llu\n", ib, e.w, o.nTr, o.nEx, o.headScore, (unsigned long long)o.headGlen, e.nTr, e.nEx, e.headScore, (unsigned long long)e.headGlen); continue; }
            if (!e.nTr) { if (o.trOffset || o.exOffset) TRS_FAIL("REPLAY DIFF case %u window %u: empty, offsets %u %u\n", ib, e.w, o.trOffset, o.exOffset); continue; }
            if ((u64)o.trOffset + o.nTr > b.trCap || (u64)o.exOffset + o.nEx > b.exCap) { TRS_FAIL("REPLAY DIFF case %u window %u: block %u + %u / %u + %u outside the pools\n", ib, e.w, o.trOffset, o.nTr, o.exOffset, o.nEx); continue; }
            for (u32 j = 0; j < o.nTr; j++) useT[o.trOffset + j]++; for (u32 j = 0; j < o.nEx; j++) useE[o.exOffset + j]++; sumT += o.nTr; sumE += o.nEx;
            const u8 *p = S.recExp.data() + e.recOff; u32 eoff = 0;
            for (u32 j = 0; j < e.nTr; j++) {
                const staramd_transcript &t = tr[o.trOffset + j]; const u32 ne = ((const staramd_transcript *)p)->nExons;
                if (memcmp(&t, p, REC_HDR) != 0) { TRS_FAIL("REPLAY DIFF case %u window %u rank %u: header differs (score %d, exonOffset %u; wanted %d, %u)\n", ib, e.w, j, t.maxScore, t.exonOffset, ((const staramd_transcript *)p)->maxScore, ((const staramd_transcript *)p)->exonOffset); break; }
                if (memcmp(&ex[o.exOffset + eoff], p + REC_HDR, 32u * ne) != 0) { TRS_FAIL("REPLAY DIFF case %u window %u rank %u: exon rows differ\n", ib, e.w, j); break; }
                p += REC_HDR + 32u * ne; eoff += ne;
            }
        }
        for (u32 w = 0; w < b.nWout; w++) if (!listed[w] && memcmp(&wout[w], &woutIn[w], sizeof(DWinOut)) != 0) { TRS_FAIL("REPLAY DIFF case %u window %u: not on the list and changed\n", ib, w); break; }
        for (u32 k = 0; k < b.trCap; k++) if (useT[k] > 1) { TRS_FAIL("REPLAY DIFF case %u: place %u of trPool belongs to %u windows\n", ib, k, useT[k]); break; }
        for (u32 k = 0; k < b.exCap; k++) if (useE[k] > 1) { TRS_FAIL("REPLAY DIFF case %u: place %u of exPool belongs to %u windows\n", ib, k, useE[k]); break; }
        if (shortPool) { if (!nKept) TRS_FAIL("REPLAY DIFF case %u: the pool is one record short and every window was written\n", ib); }
        else if (cur[CUR_TR] != b.nTrPool + sumT || cur[CUR_EX] != b.nExPool + sumE) TRS_FAIL("REPLAY DIFF case %u: CUR_TR / CUR_EX %u %u, the blocks add up to %u %u\n", ib, cur[CUR_TR], cur[CUR_EX], b.nTrPool + sumT, b.nExPool + sumE);
        // (a wavefront that starts after another has set an overflow flag returns at once, without a ticket: the count is compared where no flag is expected)
        if (!b.expFlags && cur[CUR_ST_TICKETR] != b.nList + TRS_REPLAY_BLOCKS * 4u) TRS_FAIL("REPLAY DIFF case %u: %u tickets drawn, wanted one per item and one per wavefront (%u)\n", ib, cur[CUR_ST_TICKETR], b.nList + TRS_REPLAY_BLOCKS * 4u);
        if (nR && memcmp(reads.data(), readIn, (size_t)nR * sizeof(DRead)) != 0) TRS_FAIL("REPLAY DIFF case %u: reads were changed\n", ib);
    }
    if (b.kind == TRS_FINISH) {
        for (u32 r = 0; r < nR; r++) if (memcmp(&reads[r], &S.readExp[b.expReadOff + r], sizeof(DRead)) != 0) { const DRead &x = reads[r], &y = S.readExp[b.expReadOff + r];
            TRS_FAIL("FINISH DIFF case %u read %u (%u windows, resultSelect %u): status %x nWt %u nTr %u nEx %u bestW %d maxScoreMate %d %d unmappedLength %x; wanted %x %u %u %u %d %d %d %x%s\n", ib, r, x.nWin, P.resultSelect, x.status, x.nWt, x.nTr, x.nEx, x.bestW,
                     x.maxScoreMate[0], x.maxScoreMate[1], x.unmappedLength, y.status, y.nWt, y.nTr, y.nEx, y.bestW, y.maxScoreMate[0], y.maxScoreMate[1], y.unmappedLength, x.winOffset != y.winOffset || x.nWin != y.nWin || x.nSeeds != y.nSeeds ? " (fields of the input differ)" : ""); }
        for (u32 w = 0; w < b.nWout; w++) if (memcmp(&wout[w], &S.woutExp[b.expWoutOff + w], sizeof(DWinOut)) != 0) { const DWinOut &x = wout[w], &y = S.woutExp[b.expWoutOff + w]; TRS_FAIL("FINISH DIFF case %u window %u: nTr %u nEx %u, wanted %u %u%s\n", ib, w, x.nTr, x.nEx, y.nTr, y.nEx, x.nTr == y.nTr && x.nEx == y.nEx ? " (other bytes differ)" : ""); }
    }
    if (b.kind == TRS_FINISH || b.kind == TRS_TAIL) if (cnt[DC_nTrOut] != b.expTrOut) TRS_FAIL("CASE %u: DC_nTrOut %llu, wanted %llu\n", ib, (unsigned long long)cnt[DC_nTrOut], (unsigned long long)b.expTrOut);
    if (b.kind == TRS_SCANLOCAL) {
        const std::vector<u32> tb = trsDown<u32>(bTrBase, nR), eb = trsDown<u32>(bExBase, nR), bt = trsDown<u32>(bBlockTot, 2 * (size_t)nBlk); const u32 *e = S.scanLocalExp.data() + b.expScanOff;
        for (u32 r = 0; r < nR; r++) if (tb[r] != e[r] || eb[r] != e[nR + r]) { TRS_FAIL("SCAN DIFF case %u read %u of %u: bases %u %u, wanted %u %u\n", ib, r, nR, tb[r], eb[r], e[r], e[nR + r]); break; }
        for (u32 k = 0; k < 2 * nBlk; k++) if (bt[k] != e[2 * nR + k]) { TRS_FAIL("SCAN DIFF case %u: total %u of block %u is %u, wanted %u\n", ib, k & 1u, k / 2, bt[k], e[2 * nR + k]); break; }
    }
    if (b.kind == TRS_TAIL) {
        const std::vector<staramd_read_result> rr = trsDown<staramd_read_result>(bOutR, nR); const std::vector<staramd_transcript> ot = trsDown<staramd_transcript>(bOutT, b.outTrCap); const std::vector<staramd_exon> oe = trsDown<staramd_exon>(bOutE, b.outExCap);
        const std::vector<u32> tot = trsDown<u32>(bTotals, 2);
        if (tot[0] != b.expNOutTr || tot[1] != b.expNOutEx) TRS_FAIL("TAIL DIFF case %u: totals %u %u, wanted %u %u\n", ib, tot[0], tot[1], b.expNOutTr, b.expNOutEx);
        u32 eo = 0;
        for (u32 r = 0; r < nR; r++) {
            staramd_read_result y = S.rrExp[b.expRROff + r]; const staramd_read_result &x = rr[r];
            u32 nEx = 0; for (u32 k = 0; k < y.nTr; k++) nEx += S.outTr[b.expOutTrOff + y.trOffset + k].nExons;
            const bool fits = y.nTr > 0 && (u64)y.trOffset + y.nTr <= b.outTrCap && (u64)eo + nEx <= b.outExCap;
            if (!fits) y.trBest = -1;                  // (a read whose block does not fit the arrays: counts and offsets state the need, no record is written and none is named best)
            if (memcmp(&x, &y, sizeof(y)) != 0) TRS_FAIL("TAIL DIFF case %u read %u of %u: status %x nW %u nTr %u trOffset %u trBest %d maxScoreMate %d %d unmappedLength %x; wanted %x %u %u %u %d %d %d %x\n", ib, r, nR, x.status, x.nW, x.nTr, x.trOffset, x.trBest,
                                                         x.maxScoreMate[0], x.maxScoreMate[1], x.unmappedLength, y.status, y.nW, y.nTr, y.trOffset, y.trBest, y.maxScoreMate[0], y.maxScoreMate[1], y.unmappedLength);
            for (u32 k = 0; k < y.nTr && y.trOffset + k < b.outTrCap; k++) { const staramd_transcript &t = ot[y.trOffset + k], &u = S.outTr[b.expOutTrOff + y.trOffset + k];
                if (fits ? memcmp(&t, &u, sizeof(t)) != 0 : !trsAllFill(&t, sizeof(t))) { TRS_FAIL("TAIL DIFF case %u read %u transcript %u: %s (iW %u exonOffset %u score %d; the oracle's %u %u %d)\n", ib, r, k, fits ? "differs" : "written though its read does not fit", t.iW, t.exonOffset, t.maxScore, u.iW, u.exonOffset, u.maxScore); break; } }
            for (u32 k = 0; k < nEx && eo + k < b.outExCap; k++) { const staramd_exon &t = oe[eo + k], &u = S.outEx[b.expOutExOff + eo + k];
                if (fits ? memcmp(&t, &u, sizeof(t)) != 0 : !trsAllFill(&t, sizeof(t))) { TRS_FAIL("TAIL DIFF case %u read %u exon %u: %s\n", ib, r, k, fits ? "differs" : "written though its read does not fit"); break; } }
            eo += nEx;
        }
        if (b.expNOutTr < b.outTrCap && !trsAllFill(ot.data() + b.expNOutTr, (size_t)(b.outTrCap - b.expNOutTr) * sizeof(staramd_transcript))) TRS_FAIL("TAIL DIFF case %u: outTr was written behind the total\n", ib);
        if (b.expNOutEx < b.outExCap && !trsAllFill(oe.data() + b.expNOutEx, (size_t)(b.outExCap - b.expNOutEx) * sizeof(staramd_exon))) TRS_FAIL("TAIL DIFF case %u: outEx was written behind the total\n", ib);
    }
    if (b.kind == TRS_FLAGS) {
        // a pool overflowed earlier: every kernel returns at once, every buffer keeps what it held
        bool kept = (!nR || memcmp(reads.data(), readIn, (size_t)nR * sizeof(DRead)) == 0) && (!b.nWout || memcmp(wout.data(), woutIn, (size_t)b.nWout * sizeof(DWinOut)) == 0) && trsAllFill(redo.data(), (size_t)b.nWout * 4) && trsAllFill(replay.data() + b.nList, (size_t)(b.nWout - b.nList) * 4);
        const TrsBuf *fills[] = {&bTrBase, &bExBase, &bBlockTot, &bTotals, &bOutR, &bOutT, &bOutE};
        for (const TrsBuf *f : fills) { const std::vector<u8> v = trsDown<u8>(*f, f->n); if (!trsAllFill(v.data(), v.size())) { kept = false; TRS_FAIL("FLAGS DIFF case %u: %s was written\n", ib, f->name); } }
        for (u32 k = 0; k < DC_N; k++) if (cnt[k]) kept = false;
        for (u32 k = 0; k < CUR_N; k++) if (cur[k] != (k == CUR_TR ? b.nTrPool : k == CUR_EX ? b.nExPool : k == CUR_FLAGS ? b.flags0 : k == CUR_ST_REPLAY ? b.nList : 0u)) kept = false;
        if (!kept) TRS_FAIL("FLAGS DIFF case %u: CUR_FLAGS was %x before the launches and a buffer, a cursor or a counter was changed\n", ib, b.flags0);
    }
    for (TrsBuf *p : all) trsFree(*p);
    trsCompared++;
    trsSecondsBatches[b.kind] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return bad;
}

static long trsRun(const TrsSet &S, bool quiet = false) {
    long bad = 0; const auto t0 = std::chrono::steady_clock::now();
    std::vector<DevIndex> X(S.env.size()); for (size_t e = 0; e < S.env.size(); e++) { memset(&X[e], 0, sizeof(DevIndex)); X[e].P = S.env[e].P; }
    TrsBuf bX = trsUp("parameters", X, 0, X.size(), 1);
    for (u32 ic = 0; ic < S.pack.size(); ic++) bad += trsRunPack(S, ic);
    { size_t expOff = 0; for (u32 ic = 0; ic < S.scan.size(); ic++) { bad += trsRunScan(S, ic, expOff); expOff += 2 * (size_t)S.scan[ic].nBlocks + 2; } }
    const auto t1 = std::chrono::steady_clock::now();
    for (u32 ib = 0; ib < S.batch.size(); ib++) bad += trsRunBatch(S, bX, ib);
    bad += trsGuardsBad(bX); trsFree(bX);
    printf("seconds: pack and scan cases %.2f; batches: verify %.2f, replay %.2f, finish %.2f, scan %.2f, tail %.2f, flags %.2f\n", std::chrono::duration<double>(t1 - t0).count(), trsSecondsBatches[0], trsSecondsBatches[1], trsSecondsBatches[2],
           trsSecondsBatches[3], trsSecondsBatches[4], trsSecondsBatches[5]);
    const size_t n = S.pack.size() + S.scan.size() + S.batch.size();
    printf("compared %zu of %zu cases\n", trsCompared, n);
    if (trsCompared != n) bad++;
    if (!quiet) printf("%zu pack cases, %zu scans of block totals, %zu batches over %zu reads and %zu windows: %ld differences\n", S.pack.size(), S.scan.size(), S.batch.size(), S.read.size(), S.wout.size(), bad);
    return bad;
}
