// window_routines_cases.h -- TEST INFRASTRUCTURE: the cases of oracle/window_routines_check.cpp, the probe kernels that run them and the comparison of what the kernels return with what
// the cases expect.  Included behind star_amd/csrc/engine/k_window.hip by the CPU check (host build through the wavefront emulator's headers: a launch is emu::launch) and by
// tests/window_routines_gpu.hip (hipcc, gfx950), so both run the same probes and the same launches of k_windows / k_windows_big / k_order_* over the same records.
// Layer 1, one wavefront per case in blocks of 256 lanes (three of four wavefronts work in an LDS slice that does not start at 0, as in the product): createExtendWindowsWithAlign and
// assignAlignToWindow with the table in LDS (<false>) and in global memory (<true>), sjAlignSplit, ownInsert / ownLookup over LDS words and over a buffer, waveMax64 / waveMin32 /
// seedOfLane.  The wave-uniform results are held to being the same in all 64 lanes inside the probe (a ballot against lane 0's value); lane 0 writes them with a hash of the rows.
// Layer 2: a DevBatch made by hand -- fabricated suffix-array entries, seed tables, chrBin, junction arrays -- through the kernels with the launch shapes of engine.hip, every buffer
// between guard words.  The expected values of a case are the oracle's (star_oracle.cpp), never the emulated routine's.
#pragma once
#include <cstdio>
#include <cstring>
#include <vector>
#include <map>
#include <chrono>

#define WRS_MAGIC 0x3130574f444e4957ull        // "WINDOW01"
#define WRS_CAPW 256u                          // table rows of the layer-1 probes (three trips of 64 and more)
#define WRS_HASHBITS 1024u
#define WRS_TAB_WORDS (WRS_CAPW * 8u + WRS_HASHBITS / 32u)
#define WRS_BLOCKS 4u                          // seed-list blocks of an assign case
#define WRS_OWN_SLOTS_MAX 8192u                // slots of the largest owner map (hashBits 262144)
#define WRS_GUARD 32768u                        // guard bytes either side of every buffer: wider than the 64 x 64 words k_order_scatter can be off by when its placement rule is wrong

struct WrsEnv { staramd_params P; u64 nGenome, sjGstart, saOff, saWords; u32 strandBit, sjdbOverhang, sjdbLength, sjdbN, nChrReal, chrBinOff, chrBinN, sjOff; };
struct WrsAnchor { u64 a1; u32 str, pad; };
struct WrsCreate { u32 env, big, off, n; };
struct WrsCreateOut { u32 ret, nW, flags, pad; u64 hash; };                       // flags: winLimit | overflow << 1
struct WrsSeedIn { u64 a1; u32 iW, L, nrep, frag, rStart, anchor; i32 sjA; u32 pad; };
struct WrsAssign { u32 env, big, Lread, off, n, nWin, capBlocks, pad; };
struct WrsAssignOut { u32 nwa, lrec, flags, nBlocks; u64 hash; };                 // flags: tooMany | overflow << 1
struct WrsSplit { u64 a1, expD, expA; u32 env, L, expRet, expLD, expLA, expIsj; };
struct WrsSplitOut { u64 a1D, a1A; u32 ret, lD, lA, isj; };
struct WrsOwn { u32 slots, global, insOff, nIns, qOff, nQ; };                     // nIns, nQ: multiples of 64
struct WrsOwnOp { u32 key, val; };                                                // insert: val = flank << OWN_BITS | window; query: val = the expected answer
struct WrsWave { u64 v64[64]; u32 v32[64]; DSeed seeds[64]; u32 src; u32 pad; };
struct WrsWaveOut { u64 max64; u32 min32, pad; DSeed sd; };
// layer 2
struct WrsGeom { u32 capW, capBlocks, hashBits, capWMid, capBlocksMid, hashBitsMid, ownerMap, lightEst; };
// shortPool: 1 winCap one short, 2 waCap one short.  expSAenum / expWindows: what the launches of the geometry count for the oracle's run of the reads (a chunk of 64 loci
// is counted when it is read, pass B stops at too many anchors, a read that outgrows a launch is counted again by the next)
struct WrsBatch { u32 env, geom, readOff, nReads, shortPool, cmpCounters, totWin, totWA; u64 expSAenum, expWindows, expWA; };
struct WrsRead { u32 seedOff, nSeeds, Lread, full, expStatus, expNWin, expWt, winOff; };                                          // full 0: at the window limit, the status bit only
struct WrsWin { u32 chr, str, nWA, mates, rowOff, pad; };
#define WRS_STATUS_BITS (STARAMD_ST_WINDOWS_LIMIT | STARAMD_ST_TOO_MANY_ANCHORS | STARAMD_ST_NO_GOOD_WINDOW)

__host__ __device__ static inline u64 wrsMix(u64 h, u64 v) { return (h ^ v) * 0x100000001B3ull + (h >> 29); }
#define WRS_HASH0 0xCBF29CE484222325ull
#define WRS_DEAD 0xDEADDEADDEADull

// ---- probes ---------------------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u32 wrsNotUniform(u32 v) { return __ballot(v != first32(v)) != 0 ? 1u : 0u; }
template <bool BIG> __device__ __forceinline__ void wrsSetup(WS<BIG> &s, typename WPtr<BIG>::P tab, DWA *arena, u32 capW, u32 capBlocks, u32 hashBits, u32 Lread) {
    s.hashMask = hashBits - 1u; s.bitmap = tab + capW * 8;
    s.t.coreS = tab; s.t.coreE = tab + capW; s.t.extS = tab + 2 * capW; s.t.extE = tab + 3 * capW;
    s.t.meta = tab + 4 * capW; s.t.blk = tab + 5 * capW; s.t.lrec = tab + 6 * capW; s.t.nwa = tab + 7 * capW;
    s.arena = arena; s.capW = capW; s.capBlocks = capBlocks; s.nW = 0; s.nBlocks = 0; s.Lread = Lread;
    s.tooMany = false; s.winLimit = false; s.overflow = false; s.ownMap = false; s.ownMask = 0;
}
template <bool BIG> __device__ __forceinline__ typename WPtr<BIG>::P wrsTab(u32 *bigTab, u32 i, u32 wave) {
    if constexpr (BIG) return bigTab + (u64)i * WRS_TAB_WORDS;
    else return (typename WPtr<false>::P)ldsTab + wave * WRS_TAB_WORDS;
}

template <bool BIG> __device__ __forceinline__ void wrsCreateBody(const DevIndex *envX, const WrsCreate *cs, const WrsAnchor *an, u32 n, u32 *bigTab, WrsCreateOut *out, u32 *notUniform) {
    const u32 lane = threadIdx.x & 63u, wave = WAVE_INDEX(threadIdx.x >> 6), i = blockIdx.x * 4u + wave;
    if (i >= n) return;
    const WrsCreate c = cs[i]; const DevIndex &X = envX[c.env]; const staramd_params &P = X.P;
    WS<BIG> s; wrsSetup<BIG>(s, wrsTab<BIG>(bigTab, i, wave), nullptr, WRS_CAPW, 0u, WRS_HASHBITS, 0u);
    u32 bad = 0;
    for (u32 k = 0; k < c.n; k++) {
        const WrsAnchor a = an[c.off + k];
        const u32 chr = GLOBAL(u32, X.chrBin)[(u32)(a.a1 >> P.winBinNbits) >> P.winBinChrNbits];
        const int r = createExtendWindowsWithAlign<BIG>(X, s, a.a1, a.str, chr, lane);
        bad |= wrsNotUniform((u32)r) | wrsNotUniform(s.nW) | wrsNotUniform(s.winLimit ? 1u : 0u) | wrsNotUniform(s.overflow ? 1u : 0u);
        rowFence<BIG>();
        if (lane == 0) {
            u64 h = WRS_HASH0;
            for (u32 j = 0; j < s.nW; j++) { const u32 m = s.t.meta[j]; if (m & 1u) { h = wrsMix(h, s.t.coreS[j]); h = wrsMix(h, s.t.coreE[j]); h = wrsMix(h, m >> 2); h = wrsMix(h, (m >> 1) & 1u); } else h = wrsMix(h, WRS_DEAD); }
            WrsCreateOut o; o.ret = (u32)r; o.nW = s.nW; o.flags = (s.winLimit ? 1u : 0u) | (s.overflow ? 2u : 0u); o.pad = 0; o.hash = h; out[c.off + k] = o;
        }
    }
    if (bad && lane == 0) atomicAdd(notUniform, 1u);
}
extern "C" __global__ void __launch_bounds__(256) k_wrs_create(const DevIndex *envX, const WrsCreate *cs, const WrsAnchor *an, u32 n, WrsCreateOut *out, u32 *notUniform) { wrsCreateBody<false>(envX, cs, an, n, nullptr, out, notUniform); }
extern "C" __global__ void __launch_bounds__(256) k_wrs_create_big(const DevIndex *envX, const WrsCreate *cs, const WrsAnchor *an, u32 n, u32 *bigTab, WrsCreateOut *out, u32 *notUniform) { wrsCreateBody<true>(envX, cs, an, n, bigTab, out, notUniform); }

// the seeds of a case go to the windows 0 .. nWin - 1 of a table whose rows the probe sets as the flank block leaves them
template <bool BIG> __device__ __forceinline__ void wrsAssignBody(const DevIndex *envX, const WrsAssign *cs, const WrsSeedIn *sd, u32 n, u32 *bigTab, DWA *arenas, WrsAssignOut *out, u32 *notUniform) {
    const u32 lane = threadIdx.x & 63u, wave = WAVE_INDEX(threadIdx.x >> 6), i = blockIdx.x * 4u + wave;
    if (i >= n) return;
    const WrsAssign c = cs[i]; const DevIndex &X = envX[c.env];
    WS<BIG> s; wrsSetup<BIG>(s, wrsTab<BIG>(bigTab, i, wave), arenas + (u64)i * WRS_BLOCKS * WA_MAX, WRS_CAPW, c.capBlocks, WRS_HASHBITS, c.Lread);
    s.nW = c.nWin;
    if (lane < c.nWin) { s.t.meta[lane] = 1u; s.t.coreS[lane] = s.t.coreE[lane] = s.t.extS[lane] = s.t.extE[lane] = lane; s.t.nwa[lane] = 0; s.t.lrec[lane] = 0; s.t.blk[lane] = NOWIN; }
    rowFence<BIG>();
    u32 bad = 0;
    for (u32 k = 0; k < c.n; k++) {
        const WrsSeedIn a = sd[c.off + k];
        assignAlignToWindow<BIG>(X, s, a.iW, a.a1, a.L, a.nrep, a.frag, a.rStart, a.anchor != 0, a.sjA, lane);
        bad |= wrsNotUniform(s.nBlocks) | wrsNotUniform(s.tooMany ? 1u : 0u) | wrsNotUniform(s.overflow ? 1u : 0u);
        tabFence(); rowFence<BIG>();
        if (lane == 0) {
            WrsAssignOut o; o.nwa = s.t.nwa[a.iW]; o.lrec = s.t.lrec[a.iW]; o.flags = (s.tooMany ? 1u : 0u) | (s.overflow ? 2u : 0u); o.nBlocks = s.nBlocks;
            u64 h = WRS_HASH0; const u32 b = s.t.blk[a.iW];
            if (b != NOWIN) { const DWA *A = s.arena + (u64)b * WA_MAX;
                for (u32 j = 0; j < o.nwa; j++) { const DWA e = A[j]; h = wrsMix(h, e.gStart); h = wrsMix(h, e.nrep); h = wrsMix(h, e.L); h = wrsMix(h, e.rStart); h = wrsMix(h, (u64)(i64)e.sjA); h = wrsMix(h, e.anchor); h = wrsMix(h, e.iFrag); } }
            o.hash = h; out[c.off + k] = o;
        }
        LOCKSTEP();
        if (s.tooMany || s.overflow) break;                      // (wave-uniform, and held to be: the case ends here on the reference side too)
    }
    if (bad && lane == 0) atomicAdd(notUniform, 1u);
}
extern "C" __global__ void __launch_bounds__(256) k_wrs_assign(const DevIndex *envX, const WrsAssign *cs, const WrsSeedIn *sd, u32 n, DWA *arenas, WrsAssignOut *out, u32 *notUniform) { wrsAssignBody<false>(envX, cs, sd, n, nullptr, arenas, out, notUniform); }
extern "C" __global__ void __launch_bounds__(256) k_wrs_assign_big(const DevIndex *envX, const WrsAssign *cs, const WrsSeedIn *sd, u32 n, u32 *bigTab, DWA *arenas, WrsAssignOut *out, u32 *notUniform) { wrsAssignBody<true>(envX, cs, sd, n, bigTab, arenas, out, notUniform); }

extern "C" __global__ void __launch_bounds__(256) k_wrs_split(const DevIndex *envX, const WrsSplit *cs, u32 n, WrsSplitOut *out) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const WrsSplit c = cs[i]; WrsSplitOut o; memset(&o, 0, sizeof(o));
    o.ret = sjAlignSplit(envX[c.env], c.a1, c.L, o.a1D, o.lD, o.a1A, o.lA, o.isj) ? 1u : 0u;
    out[i] = o;
}

// one wavefront per case (blocks of 64 lanes): the LDS form of the owner map in the dynamic LDS of the block, the global form in a buffer.  Lane l inserts entry l of every group
// of 64 with no fence between the groups, as the lanes of the flank block do; then the look-ups, lane l the query l of every group
template <class BP> __device__ __forceinline__ void wrsOwnRun(BP tab, const WrsOwn &c, const WrsOwnOp *ops, u32 *out, u32 lane) {
    for (u32 k = lane; k < c.slots; k += 64) tab[k] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __threadfence_block();
    for (u32 k = lane; k < c.nIns; k += 64) { const WrsOwnOp o = ops[c.insOff + k]; if (o.key != 0xFFFFFFFFu) ownInsert(tab, c.slots - 1u, o.key, o.val); }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __threadfence_block();
    for (u32 k = lane; k < c.nQ; k += 64) out[c.qOff + k] = ownLookup(tab, c.slots - 1u, ops[c.qOff + k].key);
}
extern "C" __global__ void __launch_bounds__(64) k_wrs_own(const WrsOwn *cs, const WrsOwnOp *ops, u32 n, u32 *globalTabs, u32 *out) {
    const u32 lane = threadIdx.x & 63u, i = blockIdx.x;
    if (i >= n) return;
    const WrsOwn c = cs[i];
    if (c.global) wrsOwnRun(globalTabs + (u64)i * WRS_OWN_SLOTS_MAX, c, ops, out, lane);
    else wrsOwnRun((typename WPtr<false>::P)ldsTab, c, ops, out, lane);
}

extern "C" __global__ void __launch_bounds__(256) k_wrs_wave(const WrsWave *cs, u32 n, WrsWaveOut *out) {
    const u32 lane = threadIdx.x & 63u, wave = WAVE_INDEX(threadIdx.x >> 6), i = blockIdx.x * 4u + wave;
    if (i >= n) return;
    WrsWaveOut o; memset(&o, 0, sizeof(o));
    o.max64 = waveMax64(cs[i].v64[lane]); o.min32 = waveMin32(cs[i].v32[lane]); o.sd = seedOfLane(cs[i].seeds[lane], first32(cs[i].src));
    out[(u64)i * 64 + lane] = o;
}

// ---- the whole set of cases, as the check makes it and the file holds it ------------------------------------------------------------------------------------------------
#define WRS_FIELDS(F) F(env) F(chrBin) F(sjD) F(sjA) F(sa) F(anchor) F(create) F(createExp) F(seedIn) F(assign) F(assignExp) F(split) F(own) F(ownOp) F(wave) F(waveExp) \
                      F(geom) F(batch) F(read) F(seed) F(win) F(row)
struct WrsSet {
    std::vector<WrsEnv> env; std::vector<u32> chrBin; std::vector<u64> sjD, sjA, sa;
    std::vector<WrsAnchor> anchor; std::vector<WrsCreate> create; std::vector<WrsCreateOut> createExp;
    std::vector<WrsSeedIn> seedIn; std::vector<WrsAssign> assign; std::vector<WrsAssignOut> assignExp;
    std::vector<WrsSplit> split; std::vector<WrsOwn> own; std::vector<WrsOwnOp> ownOp; std::vector<WrsWave> wave; std::vector<WrsWaveOut> waveExp;
    std::vector<WrsGeom> geom; std::vector<WrsBatch> batch; std::vector<WrsRead> read; std::vector<DSeed> seed; std::vector<WrsWin> win; std::vector<DWA> row;
};
template <class T> static void wrsPut(FILE *f, const std::vector<T> &v) { const u64 n = v.size(); if (fwrite(&n, 8, 1, f) != 1 || (n && fwrite(v.data(), sizeof(T), n, f) != n)) { perror("window routines: write"); exit(2); } }
template <class T> static void wrsTake(FILE *f, std::vector<T> &v) { u64 n = 0; if (fread(&n, 8, 1, f) != 1 || n > (1ull << 32)) { fprintf(stderr, "case file: short read\n"); exit(2); } v.resize(n); if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "case file: short read\n"); exit(2); } }
static void wrsWrite(FILE *f, const WrsSet &S) {
    const u64 magic = WRS_MAGIC; if (fwrite(&magic, 8, 1, f) != 1) { perror("window routines: write"); exit(2); }
#define F(x) wrsPut(f, S.x);
    WRS_FIELDS(F)
#undef F
}
static void wrsReadFile(FILE *f, WrsSet &S) {
    u64 magic = 0; if (fread(&magic, 8, 1, f) != 1 || magic != WRS_MAGIC) { fprintf(stderr, "not a case file of the window routines\n"); exit(2); }
#define F(x) wrsTake(f, S.x);
    WRS_FIELDS(F)
#undef F
}

// ---- running a set --------------------------------------------------------------------------------------------------------------------------------------------------
#define WRS_CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)
#define WRS_FAIL(...) do { if (bad++ < 30) printf(__VA_ARGS__); } while (0)
// a device buffer of n bytes between two guards of WRS_GUARD bytes of 0xEE
struct WrsBuf { u8 *raw = nullptr; size_t n = 0; template <class T> T *as() const { return (T *)(raw + WRS_GUARD); } };
static WrsBuf wrsAlloc(size_t n, int fill, const void *src = nullptr, size_t srcBytes = 0) {
    WrsBuf b; b.n = n;
    WRS_CK(hipMalloc((void **)&b.raw, n + 2 * WRS_GUARD)); WRS_CK(hipMemset(b.raw, 0xEE, WRS_GUARD)); WRS_CK(hipMemset(b.raw + WRS_GUARD + n, 0xEE, WRS_GUARD));
    if (n) WRS_CK(hipMemset(b.raw + WRS_GUARD, fill, n));
    if (srcBytes) WRS_CK(hipMemcpy(b.raw + WRS_GUARD, src, srcBytes, hipMemcpyHostToDevice));
    return b;
}
template <class T> static WrsBuf wrsUp(const std::vector<T> &v, size_t from = 0, size_t count = (size_t)-1) {
    if (count == (size_t)-1) count = v.size() - from;
    return wrsAlloc(count * sizeof(T) + 64, 0, count ? v.data() + from : nullptr, count * sizeof(T));
}
template <class T> static std::vector<T> wrsDown(const WrsBuf &b, size_t n) { std::vector<T> v(n); if (n) WRS_CK(hipMemcpy(v.data(), b.raw + WRS_GUARD, n * sizeof(T), hipMemcpyDeviceToHost)); return v; }
static long wrsGuardsBad(const WrsBuf &b) {
    static std::vector<u8> gv(2 * WRS_GUARD); u8 *g = gv.data(); WRS_CK(hipMemcpy(g, b.raw, WRS_GUARD, hipMemcpyDeviceToHost)); WRS_CK(hipMemcpy(g + WRS_GUARD, b.raw + WRS_GUARD + b.n, WRS_GUARD, hipMemcpyDeviceToHost));
    long n = 0; for (u32 k = 0; k < 2 * WRS_GUARD; k++) if (g[k] != 0xEE) n++;
    return n;
}
static void wrsFree(WrsBuf &b) { if (b.raw) WRS_CK(hipFree(b.raw)); b.raw = nullptr; }

struct WrsDev { WrsBuf sa, chrBin, sjD, sjA, X; };
static void wrsIndexUp(const WrsSet &S, WrsDev &D) {
    D.sa = wrsUp(S.sa); D.chrBin = wrsUp(S.chrBin); D.sjD = wrsUp(S.sjD); D.sjA = wrsUp(S.sjA);
    std::vector<DevIndex> X(S.env.size());
    for (size_t e = 0; e < S.env.size(); e++) {
        const WrsEnv &v = S.env[e]; DevIndex &x = X[e]; memset(&x, 0, sizeof(x));
        x.SA = D.sa.as<u64>() + v.saOff; x.chrBin = D.chrBin.as<u32>() + v.chrBinOff; x.sjDstart = D.sjD.as<u64>() + v.sjOff; x.sjAstart = D.sjA.as<u64>() + v.sjOff;
        x.nGenome = v.nGenome; x.sjGstart = v.sjGstart; x.strandBit = v.strandBit; x.saBits = v.strandBit + 1; x.saMask = (1ull << x.saBits) - 1; x.strandMask = ~(1ull << v.strandBit);
        x.sjdbOverhang = v.sjdbOverhang; x.sjdbLength = v.sjdbLength; x.sjdbN = v.sjdbN; x.nChrReal = v.nChrReal; x.P = v.P;
    }
    D.X = wrsUp(X);
}

static long wrsCountersCompared = 0, wrsCountersNonZero = 0;          // batches whose DC_nSAenum / DC_nWindows were compared, and of those the ones with non-zero expectations
// what a batch leaves behind: everything the kernels wrote, copied back, with the number of guard bytes that were overwritten
struct WrsBatchOut { std::vector<u32> cur; std::vector<u64> cnt; std::vector<DRead> out; std::vector<DWin> win; std::vector<DWA> wa; std::vector<u32> items, order; std::vector<u8> cls; u32 winCap, waCap, orderSlots; };
// one batch through k_windows (first launch), k_windows (middle launch, where the geometry has one), k_windows_big, k_order_hist / _offsets / _scatter
static long wrsLaunchBatch(const WrsSet &S, const WrsDev &D, u32 ib, WrsBatchOut &R) {
    long bad = 0;
    const WrsBatch &b = S.batch[ib]; const WrsGeom &g = S.geom[b.geom]; const WrsEnv &env = S.env[b.env]; const staramd_params &P = env.P;
    const u32 nR = b.nReads;
    const u32 seed0 = S.read[b.readOff].seedOff; u32 nSeedTot = 0;
    std::vector<DRead> reads(nR); std::vector<u64> readOffset(nR + 1, 0);
    for (u32 r = 0; r < nR; r++) { const WrsRead &rd = S.read[b.readOff + r]; memset(&reads[r], 0, sizeof(DRead)); reads[r].seedOffset = rd.seedOff - seed0; reads[r].nSeeds = rd.nSeeds; readOffset[r + 1] = readOffset[r] + rd.Lread; nSeedTot += rd.nSeeds; }
    const u32 winCap = b.shortPool == 1 ? b.totWin - 1 : b.totWin + 7, waCap = b.shortPool == 2 ? b.totWA - 1 : b.totWA + 5;
    const u32 orderSlots = ((winCap + 63u) / 64u) * 64u;
    WrsBuf bReads = wrsUp(reads), bOff = wrsUp(readOffset), bSeeds = wrsUp(S.seed, seed0, nSeedTot);
    WrsBuf bWin = wrsAlloc((size_t)winCap * sizeof(DWin), 0xA5), bWA = wrsAlloc((size_t)waCap * sizeof(DWA), 0xA5), bItems = wrsAlloc((size_t)winCap * 4, 0xA5), bClass = wrsAlloc(winCap, 0xA5);
    WrsBuf bOrder = wrsAlloc((size_t)orderSlots * 4, 0xA5), bHist = wrsAlloc(64 * 4, 0), bOvf = wrsAlloc((size_t)nR * 4, 0xA5), bOvf2 = wrsAlloc((size_t)nR * 4, 0xA5);
    WrsBuf bCur = wrsAlloc(CUR_N * 4, 0), bCnt = wrsAlloc(DC_N * 8, 0);
    const u32 blocks = nR / 4 + 1 < 64 ? nR / 4 + 1 : 64, blocksMid = 4, blocksBig = 1;
    const u32 capWBig = P.alignWindowsPerReadNmax, capBlocksBig = P.alignWindowsPerReadNmax;
    WrsBuf scr = wrsAlloc((size_t)blocks * 4 * winWaveBytes(g.capW, g.capBlocks, 0), 0xA5);
    WrsBuf scrMid = wrsAlloc(g.capWMid ? (size_t)blocksMid * winWaveBytes(g.capWMid, g.capBlocksMid, 0) : 64, 0xA5);
    WrsBuf scrBig = wrsAlloc((size_t)blocksBig * 4 * winWaveBytes(capWBig, capBlocksBig, 1), 0xA5);
    DevBatch B; memset(&B, 0, sizeof(B));
    B.nReads = nR; B.readOffset = bOff.as<u64>(); B.reads = bReads.as<DRead>(); B.seedPool = bSeeds.as<DSeed>(); B.seedCap = nSeedTot;
    B.winPool = bWin.as<DWin>(); B.winCap = winCap; B.waPool = bWA.as<DWA>(); B.waCap = waCap; B.order = bOrder.as<u32>(); B.costHist = bHist.as<u32>(); B.items = bItems.as<u32>(); B.itemClass = bClass.as<u8>();
    B.ovfWin = bOvf.as<u32>(); B.ovfWin2 = bOvf2.as<u32>(); B.cursors = bCur.as<u32>(); B.counters = bCnt.as<u64>();
    const DevIndex *dX = D.X.as<DevIndex>() + b.env;
    const u32 useMid = (g.capWMid ? 1u : 0u) | (g.ownerMap ? 2u : 0u);
    hipLaunchKernelGGL(k_windows, dim3(blocks), dim3(256), 4 * winLdsWords(g.capW, g.hashBits) * sizeof(u32), 0, dX, B, scr.as<u8>(), g.capW, g.capBlocks, 0u, g.lightEst, useMid, g.hashBits);
    if (g.capWMid) hipLaunchKernelGGL(k_windows, dim3(blocksMid), dim3(64), winLdsWords(g.capWMid, g.hashBitsMid) * sizeof(u32), 0, dX, B, scrMid.as<u8>(), g.capWMid, g.capBlocksMid, 2u, g.lightEst, useMid, g.hashBitsMid);
    hipLaunchKernelGGL(k_windows_big, dim3(blocksBig), dim3(256), 0, 0, dX, B, scrBig.as<u8>(), capWBig, capBlocksBig, g.lightEst, useMid);
#ifdef STARAMD_WAVE_EMUL
    const u32 orderBlocks = 3;          // (the emulator makes a fiber per lane: the 1024 blocks of the engine are 262 144 of them per launch)
#else
    const u32 orderBlocks = 1024;
#endif
    hipLaunchKernelGGL(k_order_hist, dim3(orderBlocks), dim3(256), 0, 0, B);
    hipLaunchKernelGGL(k_order_offsets, dim3(1), dim3(1), 0, 0, B);
    hipLaunchKernelGGL(k_order_scatter, dim3(orderBlocks), dim3(256), 0, 0, B);
    WRS_CK(hipGetLastError()); WRS_CK(hipDeviceSynchronize());
    // ---- guards
    { const WrsBuf *all[] = {&bReads, &bOff, &bSeeds, &bWin, &bWA, &bItems, &bClass, &bOrder, &bHist, &bOvf, &bOvf2, &bCur, &bCnt, &scr, &scrMid, &scrBig};
      static const char *nm[] = {"reads", "readOffset", "seedPool", "winPool", "waPool", "items", "itemClass", "order", "costHist", "ovfWin", "ovfWin2", "cursors", "counters", "work space", "work space (middle)", "work space (last)"};
      for (u32 k = 0; k < 16; k++) { const long gb = wrsGuardsBad(*all[k]); if (gb) WRS_FAIL("BATCH %u: %ld guard bytes around %s were written\n", ib, gb, nm[k]); } }
    R.cur = wrsDown<u32>(bCur, CUR_N); R.cnt = wrsDown<u64>(bCnt, DC_N); R.out = wrsDown<DRead>(bReads, nR); R.winCap = winCap; R.waCap = waCap; R.orderSlots = orderSlots;
    R.win = wrsDown<DWin>(bWin, winCap); R.wa = wrsDown<DWA>(bWA, waCap); R.items = wrsDown<u32>(bItems, winCap); R.order = wrsDown<u32>(bOrder, orderSlots); R.cls = wrsDown<u8>(bClass, winCap);
    { WrsBuf *all[] = {&bReads, &bOff, &bSeeds, &bWin, &bWA, &bItems, &bClass, &bOrder, &bHist, &bOvf, &bOvf2, &bCur, &bCnt, &scr, &scrMid, &scrBig}; for (WrsBuf *p : all) wrsFree(*p); }
    return bad;
}

// per read against the oracle's buildWindows(); the places handed out in the pools are disjoint and add up to the cursors
static long wrsCompareReads(const WrsSet &S, u32 ib, const WrsBatchOut &R) {
    long bad = 0; const WrsBatch &b = S.batch[ib]; const u32 nR = b.nReads, nWinOut = R.cur[CUR_WIN], nWAOut = R.cur[CUR_WA];
    const std::vector<DRead> &out = R.out; const std::vector<DWin> &win = R.win; const std::vector<DWA> &wa = R.wa;
    std::vector<u32> winUse(nWinOut, 0), waUse(nWAOut, 0);
    for (u32 r = 0; r < nR; r++) {
        const WrsRead &rd = S.read[b.readOff + r]; const DRead &o = out[r];
        if ((o.status & (rd.full ? WRS_STATUS_BITS : STARAMD_ST_WINDOWS_LIMIT)) != rd.expStatus) WRS_FAIL("BATCH %u read %u: status %x, the oracle's %x\n", ib, r, o.status & WRS_STATUS_BITS, rd.expStatus);
        if (o.status & ~(u32)WRS_STATUS_BITS) WRS_FAIL("BATCH %u read %u: status %x\n", ib, r, o.status);
        if (o.winOffset + o.nWin > nWinOut) { WRS_FAIL("BATCH %u read %u: windows %u + %u of %u\n", ib, r, o.winOffset, o.nWin, nWinOut); continue; }
        u32 nMax = 0; bool okPlaces = true;
        for (u32 k = 0; k < o.nWin; k++) { const DWin &w = win[o.winOffset + k]; winUse[o.winOffset + k]++; if (w.read != r) WRS_FAIL("BATCH %u read %u window %u: belongs to read %u\n", ib, r, k, w.read);
            if ((u64)w.waOffset + w.nWA > nWAOut) { WRS_FAIL("BATCH %u read %u window %u: rows %u + %u of %u\n", ib, r, k, w.waOffset, w.nWA, nWAOut); okPlaces = false; continue; }
            for (u32 j = 0; j < w.nWA; j++) waUse[w.waOffset + j]++; nMax = max(nMax, (u32)w.nWA); }
        if (o.wtOffset != nMax) WRS_FAIL("BATCH %u read %u: wtOffset %u, the largest list has %u rows\n", ib, r, o.wtOffset, nMax);
        if (!rd.full || !okPlaces) continue;
        if (o.nWin != rd.expNWin || o.wtOffset != rd.expWt) { WRS_FAIL("BATCH %u read %u (%u seeds): %u windows with seeds, largest %u; the oracle's %u, %u\n", ib, r, rd.nSeeds, o.nWin, o.wtOffset, rd.expNWin, rd.expWt); continue; }
        for (u32 k = 0; k < o.nWin; k++) {
            const DWin &w = win[o.winOffset + k]; const WrsWin &e = S.win[rd.winOff + k];
            if (w.chr != e.chr || w.str != e.str || w.nWA != e.nWA || w.mates != e.mates) { WRS_FAIL("BATCH %u read %u window %u: chr %u str %u nWA %u mates %u; the oracle's %u %u %u %u\n", ib, r, k, w.chr, w.str, w.nWA, w.mates, e.chr, e.str, e.nWA, e.mates); break; }
            bool rowBad = false;
            for (u32 j = 0; j < e.nWA && !rowBad; j++) { const DWA &x = wa[w.waOffset + j], &y = S.row[e.rowOff + j];
                if (memcmp(&x, &y, sizeof(DWA)) != 0) { rowBad = true; WRS_FAIL("BATCH %u read %u window %u row %u: gStart %llu nrep %u L %u rStart %u sjA %d anchor %u iFrag %u; the oracle's %llu %u %u %u %d %u %u\n", ib, r, k, j,
                    (unsigned long long)x.gStart, x.nrep, x.L, x.rStart, x.sjA, x.anchor, x.iFrag, (unsigned long long)y.gStart, y.nrep, y.L, y.rStart, y.sjA, y.anchor, y.iFrag); } }
            if (rowBad) break;
        }
    }
    // ---- the places handed out are disjoint and add up to the cursors
    for (u32 k = 0; k < nWinOut; k++) if (winUse[k] != 1) { WRS_FAIL("BATCH %u: place %u of winPool belongs to %u reads\n", ib, k, winUse[k]); break; }
    for (u32 k = 0; k < nWAOut; k++) if (waUse[k] != 1) { WRS_FAIL("BATCH %u: place %u of waPool belongs to %u windows\n", ib, k, waUse[k]); break; }
    return bad;
}

// DC_nWA against the oracle's; DC_nSAenum and DC_nWindows against what the launches of the geometry count for the oracle's run (WrsBatch)
static long wrsCompareCounters(const WrsSet &S, u32 ib, const WrsBatchOut &R) {
    long bad = 0; const WrsBatch &b = S.batch[ib]; const std::vector<u64> &cnt = R.cnt;
    if (b.cmpCounters >= 1 && cnt[DC_nWA] != b.expWA) WRS_FAIL("BATCH %u: DC_nWA %llu, the oracle's %llu\n", ib, (unsigned long long)cnt[DC_nWA], (unsigned long long)b.expWA);
    if (b.cmpCounters >= 2) { wrsCountersCompared++; if (b.expWindows && b.expSAenum) wrsCountersNonZero++; }
    if (b.cmpCounters >= 2 && (cnt[DC_nSAenum] != b.expSAenum || cnt[DC_nWindows] != b.expWindows))
        WRS_FAIL("BATCH %u: DC_nSAenum %llu DC_nWindows %llu, the oracle's %llu %llu\n", ib, (unsigned long long)cnt[DC_nSAenum], (unsigned long long)cnt[DC_nWindows], (unsigned long long)b.expSAenum, (unsigned long long)b.expWindows);
    return bad;
}

// work items: every window from exactly one item, item classes; the order array: every item once, padding to a multiple of 64, heaviest class first along the de-interleaved positions
static long wrsCheckItemsAndOrder(const WrsSet &S, u32 ib, const WrsBatchOut &R, u64 *estWraps) {
    long bad = 0; const WrsBatch &b = S.batch[ib]; const WrsGeom &g = S.geom[b.geom]; const u32 nR = b.nReads, nWinOut = R.cur[CUR_WIN], nItems = R.cur[CUR_ITEM], orderSlots = R.orderSlots;
    const std::vector<DRead> &out = R.out; const std::vector<DWin> &win = R.win; const std::vector<u32> &items = R.items, &order = R.order; const std::vector<u8> &cls = R.cls;
    std::vector<u32> reach(nWinOut, 0); std::map<u32, u32> classOf;
    for (u32 k = 0; k < nItems; k++) {
        const u32 it = items[k]; u32 want;
        if (classOf.count(it)) WRS_FAIL("BATCH %u: item %x twice\n", ib, it);
        classOf[it] = cls[k] & 31u;
        if (it & 0x80000000u) {
            const u32 r = it & 0x7FFFFFFFu; if (r >= nR) { WRS_FAIL("BATCH %u: item %u is read %u\n", ib, k, r); continue; }
            u64 est = 0; for (u32 j = 0; j < out[r].nWin; j++) { reach[out[r].winOffset + j]++; est += 1ull << min((u32)win[out[r].winOffset + j].nWA, 20u); }
            if (est >> 32) { if (estWraps) (*estWraps)++; printf("batch %u read %u: est = %llu does not fit 32 bits\n", ib, r, (unsigned long long)est); continue; }
            if (est > g.lightEst) WRS_FAIL("BATCH %u read %u: one item, est %llu above %u\n", ib, r, (unsigned long long)est, g.lightEst);
            want = 0; while (est >> want) want++;
        } else {
            if (it >= nWinOut) { WRS_FAIL("BATCH %u: item %u is window %u of %u\n", ib, k, it, nWinOut); continue; }
            reach[it]++; want = min((u32)win[it].nWA + 1u, 31u);
            const DRead &o = out[win[it].read]; u64 est = 0; for (u32 j = 0; j < o.nWin; j++) est += 1ull << min((u32)win[o.winOffset + j].nWA, 20u);
            if (est <= g.lightEst) WRS_FAIL("BATCH %u window %u: an item of its own, est %llu of its read within %u\n", ib, it, (unsigned long long)est, g.lightEst);
        }
        if (cls[k] != want) WRS_FAIL("BATCH %u item %u (%x): class %u, wanted %u\n", ib, k, it, cls[k], want);
    }
    for (u32 k = 0; k < nWinOut; k++) if (reach[k] != 1) { WRS_FAIL("BATCH %u: window %u is reached from %u items\n", ib, k, reach[k]); break; }
    // ---- order: every item once, padding to a multiple of 64, heaviest class first along the de-interleaved positions
    const u32 G = (nItems + 63u) / 64u, slots = G * 64u; std::map<u32, u32> seen; u32 nPad = 0;
    for (u32 k = 0; k < slots; k++) { if (order[k] == 0xFFFFFFFFu) nPad++; else seen[order[k]]++; }
    if (nPad != slots - nItems || seen.size() != nItems) WRS_FAIL("BATCH %u: order holds %zu items and %u padding words, wanted %u and %u\n", ib, seen.size(), nPad, nItems, slots - nItems);
    for (const auto &kv : seen) if (kv.second != 1 || !classOf.count(kv.first)) { WRS_FAIL("BATCH %u: order holds %x %u times\n", ib, kv.first, kv.second); break; }
    u32 prev = 32;
    for (u32 pos = 0; pos < nItems; pos++) { const u32 it = order[(pos % G) * 64u + pos / G]; if (it == 0xFFFFFFFFu || !classOf.count(it)) { WRS_FAIL("BATCH %u: position %u of the order is empty\n", ib, pos); break; }
        const u32 c = classOf[it]; if (c > prev) { WRS_FAIL("BATCH %u: position %u of the order has class %u behind class %u\n", ib, pos, c, prev); break; } prev = c; }
    for (u32 k = slots; k < orderSlots; k++) if (order[k] != 0xA5A5A5A5u) { WRS_FAIL("BATCH %u: order[%u] behind the padding was written\n", ib, k); break; }
    return bad;
}

static long wrsRunBatch(const WrsSet &S, const WrsDev &D, u32 ib, u64 *estWraps) {
    WrsBatchOut R; long bad = wrsLaunchBatch(S, D, ib, R);
    const WrsBatch &b = S.batch[ib]; const std::vector<u32> &cur = R.cur;
    if (b.shortPool) {
        if (!(cur[CUR_FLAGS] & OVF_WINPOOL)) WRS_FAIL("BATCH %u: %s one short and OVF_WINPOOL is not set (flags %x)\n", ib, b.shortPool == 1 ? "winCap" : "waCap", cur[CUR_FLAGS]);
    } else if (cur[CUR_FLAGS]) WRS_FAIL("BATCH %u: flags %x\n", ib, cur[CUR_FLAGS]);
    else if (cur[CUR_WIN] > R.winCap || cur[CUR_WA] > R.waCap || cur[CUR_ITEM] > R.winCap) WRS_FAIL("BATCH %u: cursors %u %u %u beyond the pools\n", ib, cur[CUR_WIN], cur[CUR_WA], cur[CUR_ITEM]);
    else bad += wrsCompareReads(S, ib, R) + wrsCompareCounters(S, ib, R) + wrsCheckItemsAndOrder(S, ib, R, estWraps);
    return bad;
}

static long wrsRun(const WrsSet &S, bool quiet = false) {
    long bad = 0; const auto t0 = std::chrono::steady_clock::now();
    WrsDev D; wrsIndexUp(S, D);
    const DevIndex *dX = D.X.as<DevIndex>();
    WrsBuf bNU = wrsAlloc(4, 0);
    // ---- createExtendWindowsWithAlign<false> / <true>
    {
        WrsBuf bC = wrsUp(S.create), bA = wrsUp(S.anchor), bO = wrsAlloc(S.anchor.size() * sizeof(WrsCreateOut) + 64, 0xEE), bT = wrsAlloc((size_t)S.create.size() * WRS_TAB_WORDS * 4 + 64, 0xA5);
        std::vector<WrsCreate> lds, big; for (const WrsCreate &c : S.create) (c.big ? big : lds).push_back(c);
        WrsBuf bL = wrsUp(lds), bB = wrsUp(big);
        if (!lds.empty()) hipLaunchKernelGGL(k_wrs_create, dim3(((u32)lds.size() + 3) / 4), dim3(256), 4 * WRS_TAB_WORDS * 4, 0, dX, (const WrsCreate *)bL.as<WrsCreate>(), (const WrsAnchor *)bA.as<WrsAnchor>(), (u32)lds.size(), bO.as<WrsCreateOut>(), bNU.as<u32>());
        if (!big.empty()) hipLaunchKernelGGL(k_wrs_create_big, dim3(((u32)big.size() + 3) / 4), dim3(256), 0, 0, dX, (const WrsCreate *)bB.as<WrsCreate>(), (const WrsAnchor *)bA.as<WrsAnchor>(), (u32)big.size(), bT.as<u32>(), bO.as<WrsCreateOut>(), bNU.as<u32>());
        WRS_CK(hipGetLastError()); WRS_CK(hipDeviceSynchronize());
        const std::vector<WrsCreateOut> o = wrsDown<WrsCreateOut>(bO, S.anchor.size());
        for (size_t i = 0; i < S.create.size(); i++) { const WrsCreate &c = S.create[i];
            for (u32 k = 0; k < c.n; k++) { const WrsCreateOut &x = o[c.off + k], &y = S.createExp[c.off + k];
                if (x.ret != y.ret || x.nW != y.nW || x.flags != y.flags || x.hash != y.hash) { WRS_FAIL("CREATE DIFF case %zu (%s) anchor %u of %u (a1 %llu str %u): ret %u nW %u flags %u rows %016llx; the oracle's %u %u %u %016llx\n", i, c.big ? "global" : "LDS", k, c.n,
                    (unsigned long long)S.anchor[c.off + k].a1, S.anchor[c.off + k].str, x.ret, x.nW, x.flags, (unsigned long long)x.hash, y.ret, y.nW, y.flags, (unsigned long long)y.hash); break; } } }
        bad += wrsGuardsBad(bO) + wrsGuardsBad(bT);
        wrsFree(bC); wrsFree(bA); wrsFree(bO); wrsFree(bT); wrsFree(bL); wrsFree(bB);
    }
    // ---- assignAlignToWindow<false> / <true>
    {
        WrsBuf bS = wrsUp(S.seedIn), bO = wrsAlloc(S.seedIn.size() * sizeof(WrsAssignOut) + 64, 0xEE), bT = wrsAlloc((size_t)S.assign.size() * WRS_TAB_WORDS * 4 + 64, 0xA5);
        WrsBuf bAr = wrsAlloc((size_t)S.assign.size() * WRS_BLOCKS * WA_MAX * sizeof(DWA), 0xA5);
        std::vector<WrsAssign> lds, big; std::vector<u32> idxL, idxB;
        for (size_t i = 0; i < S.assign.size(); i++) { if (S.assign[i].big) { big.push_back(S.assign[i]); idxB.push_back((u32)i); } else { lds.push_back(S.assign[i]); idxL.push_back((u32)i); } }
        WrsBuf bL = wrsUp(lds), bB = wrsUp(big);
        DWA *arL = bAr.as<DWA>(), *arB = bAr.as<DWA>() + (size_t)lds.size() * WRS_BLOCKS * WA_MAX;
        if (!lds.empty()) hipLaunchKernelGGL(k_wrs_assign, dim3(((u32)lds.size() + 3) / 4), dim3(256), 4 * WRS_TAB_WORDS * 4, 0, dX, (const WrsAssign *)bL.as<WrsAssign>(), (const WrsSeedIn *)bS.as<WrsSeedIn>(), (u32)lds.size(), arL, bO.as<WrsAssignOut>(), bNU.as<u32>());
        if (!big.empty()) hipLaunchKernelGGL(k_wrs_assign_big, dim3(((u32)big.size() + 3) / 4), dim3(256), 0, 0, dX, (const WrsAssign *)bB.as<WrsAssign>(), (const WrsSeedIn *)bS.as<WrsSeedIn>(), (u32)big.size(), bT.as<u32>(), arB, bO.as<WrsAssignOut>(), bNU.as<u32>());
        WRS_CK(hipGetLastError()); WRS_CK(hipDeviceSynchronize());
        const std::vector<WrsAssignOut> o = wrsDown<WrsAssignOut>(bO, S.seedIn.size());
        for (size_t i = 0; i < S.assign.size(); i++) { const WrsAssign &c = S.assign[i];
            for (u32 k = 0; k < c.n; k++) { const WrsAssignOut &x = o[c.off + k], &y = S.assignExp[c.off + k]; const WrsSeedIn &a = S.seedIn[c.off + k];
                if (x.nwa != y.nwa || x.lrec != y.lrec || x.flags != y.flags || x.nBlocks != y.nBlocks || x.hash != y.hash) { WRS_FAIL("ASSIGN DIFF case %zu (%s, Nmax %u) seed %u of %u (window %u a1 %llu L %u rStart %u anchor %u frag %u sjA %d): nwa %u lrec %u flags %u blocks %u list %016llx; the oracle's %u %u %u %u %016llx\n",
                    i, c.big ? "global" : "LDS", S.env[c.env].P.seedPerWindowNmax, k, c.n, a.iW, (unsigned long long)a.a1, a.L, a.rStart, a.anchor, a.frag, a.sjA, x.nwa, x.lrec, x.flags, x.nBlocks, (unsigned long long)x.hash, y.nwa, y.lrec, y.flags, y.nBlocks, (unsigned long long)y.hash); break; } } }
        bad += wrsGuardsBad(bO) + wrsGuardsBad(bT) + wrsGuardsBad(bAr);
        wrsFree(bS); wrsFree(bO); wrsFree(bT); wrsFree(bAr); wrsFree(bL); wrsFree(bB);
    }
    // ---- sjAlignSplit
    {
        const u32 n = (u32)S.split.size(); WrsBuf bC = wrsUp(S.split), bO = wrsAlloc((size_t)n * sizeof(WrsSplitOut) + 64, 0xEE);
        if (n) hipLaunchKernelGGL(k_wrs_split, dim3((n + 255) / 256), dim3(256), 0, 0, dX, (const WrsSplit *)bC.as<WrsSplit>(), n, bO.as<WrsSplitOut>());
        WRS_CK(hipGetLastError()); WRS_CK(hipDeviceSynchronize());
        const std::vector<WrsSplitOut> o = wrsDown<WrsSplitOut>(bO, n);
        for (u32 i = 0; i < n; i++) { const WrsSplit &c = S.split[i]; const WrsSplitOut &x = o[i];
            if (x.ret != c.expRet || (c.expRet && (x.a1D != c.expD || x.a1A != c.expA || x.lD != c.expLD || x.lA != c.expLA || x.isj != c.expIsj)))
                WRS_FAIL("SPLIT DIFF case %u (a1 %llu L %u): %u D %llu + %u A %llu + %u junction %u; the oracle's %u D %llu + %u A %llu + %u junction %u\n", i, (unsigned long long)c.a1, c.L, x.ret, (unsigned long long)x.a1D, x.lD, (unsigned long long)x.a1A, x.lA, x.isj,
                         c.expRet, (unsigned long long)c.expD, c.expLD, (unsigned long long)c.expA, c.expLA, c.expIsj); }
        bad += wrsGuardsBad(bO); wrsFree(bC); wrsFree(bO);
    }
    // ---- ownInsert / ownLookup
    {
        const u32 n = (u32)S.own.size(); WrsBuf bC = wrsUp(S.own), bOp = wrsUp(S.ownOp), bO = wrsAlloc(S.ownOp.size() * 4 + 64, 0xEE), bT = wrsAlloc((size_t)n * WRS_OWN_SLOTS_MAX * 4 + 64, 0xA5);
        if (n) hipLaunchKernelGGL(k_wrs_own, dim3(n), dim3(64), WRS_OWN_SLOTS_MAX * 4, 0, (const WrsOwn *)bC.as<WrsOwn>(), (const WrsOwnOp *)bOp.as<WrsOwnOp>(), n, bT.as<u32>(), bO.as<u32>());
        WRS_CK(hipGetLastError()); WRS_CK(hipDeviceSynchronize());
        const std::vector<u32> o = wrsDown<u32>(bO, S.ownOp.size());
        for (u32 i = 0; i < n; i++) { const WrsOwn &c = S.own[i];
            for (u32 k = 0; k < c.nQ; k++) if (o[c.qOff + k] != S.ownOp[c.qOff + k].val) { WRS_FAIL("OWNER MAP DIFF case %u (%u slots, %s) key %u: %x, wanted %x\n", i, c.slots, c.global ? "global" : "LDS", S.ownOp[c.qOff + k].key, o[c.qOff + k], S.ownOp[c.qOff + k].val); break; } }
        bad += wrsGuardsBad(bO) + wrsGuardsBad(bT); wrsFree(bC); wrsFree(bOp); wrsFree(bO); wrsFree(bT);
    }
    // ---- waveMax64, waveMin32, seedOfLane: every lane
    {
        const u32 n = (u32)S.wave.size(); WrsBuf bC = wrsUp(S.wave), bO = wrsAlloc((size_t)n * 64 * sizeof(WrsWaveOut) + 64, 0xEE);
        if (n) hipLaunchKernelGGL(k_wrs_wave, dim3((n + 3) / 4), dim3(256), 0, 0, (const WrsWave *)bC.as<WrsWave>(), n, bO.as<WrsWaveOut>());
        WRS_CK(hipGetLastError()); WRS_CK(hipDeviceSynchronize());
        const std::vector<WrsWaveOut> o = wrsDown<WrsWaveOut>(bO, (size_t)n * 64);
        for (u32 i = 0; i < n; i++) for (u32 l = 0; l < 64; l++) { const WrsWaveOut &x = o[(size_t)i * 64 + l], &y = S.waveExp[i];
            if (x.max64 != y.max64 || x.min32 != y.min32 || memcmp(&x.sd, &y.sd, sizeof(DSeed)) != 0) { WRS_FAIL("WAVE DIFF case %u lane %u: max %016llx min %08x seed row %s; wanted %016llx %08x\n", i, l, (unsigned long long)x.max64, x.min32, memcmp(&x.sd, &y.sd, sizeof(DSeed)) ? "differs" : "equal",
                (unsigned long long)y.max64, y.min32); break; } }
        bad += wrsGuardsBad(bO); wrsFree(bC); wrsFree(bO);
    }
    { const std::vector<u32> nu = wrsDown<u32>(bNU, 1); if (nu[0]) { printf("%u cases in which the 64 lanes do not hold the same wave-uniform values\n", nu[0]); bad += nu[0]; } wrsFree(bNU); }
    // ---- layer 2
    u64 estWraps = 0; const auto t1 = std::chrono::steady_clock::now();
    for (u32 ib = 0; ib < S.batch.size(); ib++) bad += wrsRunBatch(S, D, ib, &estWraps);
    printf("seconds: routines %.1f, batches %.1f\n", std::chrono::duration<double>(t1 - t0).count(), std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count());
    printf("counters compared in %ld of %zu batches, %ld of them with non-zero values\n", wrsCountersCompared, S.batch.size(), wrsCountersNonZero);
    if (!S.batch.empty() && !wrsCountersNonZero) { printf("no batch compared DC_nSAenum and DC_nWindows with non-zero values\n"); bad++; }
    wrsFree(D.sa); wrsFree(D.chrBin); wrsFree(D.sjD); wrsFree(D.sjA); wrsFree(D.X);
    if (!quiet) printf("%zu window tables of %zu anchors, %zu seed lists of %zu seeds, %zu splits, %zu owner maps, %zu wave cases, %zu batches of %zu reads: %ld differences\n", S.create.size(), S.anchor.size(), S.assign.size(), S.seedIn.size(),
                       S.split.size(), S.own.size(), S.wave.size(), S.batch.size(), S.read.size(), bad);
    return bad;
}
