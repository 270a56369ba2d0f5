// k_bamsort.hip -- variable-length byte records ordered under a 128-bit key on the MI355X and compressed in that order (include/star_amd_bamsort.h).
// Self-contained beside k_bgzf.hip (bgzf_resident.h): no engine.hip internals, its own error text, so that the wave emulator can compile the two alone.
//
//   append    records -> a page-locked staging buffer (two, alternating) -> a slab in device memory, on the compressor's stream; the keys, the records'
//             device addresses and lengths stay in host arrays until finish (28 bytes per record)
//   order     record numbers by (g, r, number): rocprim::radix_sort_pairs by r, k_bamsort_pick brings g into that order, radix_sort_pairs by g --
//             both stable, both over the bits the run's keys occupy (g = ~0, the unmapped records, is renumbered to one above the largest other g)
//   offsets   k_bamsort_order: length and address of every record in sorted order; a 64-bit exclusive scan of the lengths = where each record goes
//   rounds    of roundBlocks BGZF blocks: k_bamsort_gather lays the round's part of the sorted stream out in a buffer, the kernels of k_bgzf.hip compress
//             it (one segment cut every 0xff00 bytes), the members come back in one copy on a second stream and go to the sink while the kernels of
//             the next round run.  The kernels of consecutive rounds are ordered on one stream, so one gather buffer serves; the compressed output has two.
//
// k_bamsort_gather is output-centric: a workgroup owns a tile of 32 KiB of the output, every lane 8 aligned 16-byte words of it, each stored once with
// one 16-byte store.  The first record of a tile is found by a bisection over the destination offsets that is the same in every lane; the records of
// the tile are staged through LDS in chunks of 127 (destination offset relative to the tile, source address); a lane finds the record under its word
// by bisection in the chunk and walks on from there: a word inside one record is one unaligned 16-byte load, a word that spans records is put together
// in two 64-bit registers from one such load per record (shifted to its place, cut to its length).  A load may run up to 15 bytes past its record:
// every slab has 16 spare bytes at its end.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <rocprim/rocprim.hpp>
#include <string>
#include <vector>
#include <chrono>
#include <algorithm>
#include <thread>
#include <atomic>
#include "../../../include/star_amd_bamsort.h"
#include "bgzf_resident.h"
#include "bamsort_resident.h"

namespace {

constexpr uint32_t IN_MAX = 0xff00;                 // input bytes per BGZF block (k_bgzf.hip)
constexpr uint32_t NT = 256;                        // work-items per workgroup
constexpr uint32_t WORDS = 8;                       // 16-byte words per lane and tile
constexpr uint32_t TILE = NT * WORDS * 16;          // output bytes per tile
constexpr uint32_t CH = 128;                        // destination offsets per LDS chunk: CH - 1 records and the end of the last one
constexpr uint64_t SLAB_PAD = 16;                   // spare bytes behind every slab (the gather kernel's 16-byte loads)

struct alignas(16) Word16 { uint64_t lo, hi; };

// v cut to its first `take` bytes (1..16), then moved up by `s` bytes (take + s <= 16)
__device__ __forceinline__ Word16 place(Word16 v, uint32_t s, uint32_t take) {
    if (take < 8) { v.hi = 0; v.lo &= (1ull << (8 * take)) - 1; }
    else if (take < 16) v.hi = take == 8 ? 0 : v.hi & ((1ull << (8 * (take - 8))) - 1);
    if (s == 0) return v;
    Word16 o;
    if (s < 8) { o.hi = v.hi << (8 * s) | v.lo >> (64 - 8 * s); o.lo = v.lo << (8 * s); }
    else { o.hi = v.lo << (8 * (s - 8)); o.lo = 0; }
    return o;
}

}  // namespace

__global__ __launch_bounds__(256) void k_bamsort_iota(uint32_t *v, uint32_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * NT) v[i] = (uint32_t)i;
}
// out[i] = g[perm[i]]: the second key in the order of the first pass
__global__ __launch_bounds__(256) void k_bamsort_pick(const uint32_t *perm, const uint64_t *g, uint32_t n, uint64_t *out) {
    for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * NT) out[i] = g[perm[i]];
}
// lengths (64-bit, the scan's input; entry n = 0, so that the scan leaves the total there) and addresses in sorted order
__global__ __launch_bounds__(256) void k_bamsort_order(const uint32_t *perm, const uint32_t *len, const uint64_t *addr, uint32_t n, uint64_t *lenSorted, uint64_t *srcSorted) {
    for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * NT) {
        if (i == n) { lenSorted[i] = 0; continue; }
        const uint32_t p = perm[i];
        lenSorted[i] = len[p]; srcSorted[i] = addr[p];
    }
}

// bytes [start, start + bytes) of the sorted stream into out[0 .. bytes rounded up to 16): dstOff[i] = where sorted record i begins in the stream,
// dstOff[n] = the stream's length; src[i] = its device address.  start is a multiple of 16 and out is 16-byte aligned; grid-stride over the tiles
__global__ __launch_bounds__(256) void k_bamsort_gather(const uint64_t *__restrict__ dstOff, const uint64_t *__restrict__ src, uint64_t n, uint64_t start, uint64_t bytes,
                                                        uint8_t *__restrict__ out) {
    __shared__ int64_t sDst[CH];
    __shared__ uint64_t sSrc[CH];
    const uint32_t tid = threadIdx.x;
    const uint64_t nTiles = (bytes + TILE - 1) / TILE;
#pragma unroll 1
    for (uint64_t tile = blockIdx.x; tile < nTiles; tile += gridDim.x) {
        const uint64_t t0 = start + tile * TILE;
        const int64_t tEnd = (int64_t)min((uint64_t)TILE, bytes - tile * TILE);        // the tile's bytes (the stream ends inside the last one)
        // the last record that begins at or before t0: the same search in every lane
        uint64_t lo = 0, hi = n;                                                         // dstOff[lo] <= t0 (dstOff[0] = 0)
#pragma unroll 1
        while (hi - lo > 1) { const uint64_t mid = lo + (hi - lo) / 2; if (dstOff[mid] <= t0) lo = mid; else hi = mid; }
        Word16 acc[WORDS];
#pragma unroll
        for (uint32_t w = 0; w < WORDS; w++) { acc[w].lo = 0; acc[w].hi = 0; }
#pragma unroll 1
        for (uint64_t base = lo;; base += CH - 1) {
            // records base .. base + CH - 2 and where the last of them ends; past the last record everything begins at the stream's end
            __syncthreads();
            if (tid < CH) {
                const uint64_t i = min(base + tid, n);
                const int64_t d = (int64_t)(dstOff[i] - t0);
                sDst[tid] = d;
                if (i < n && d < tEnd) sSrc[tid] = src[i];
            }
            __syncthreads();
            const int64_t cLo = sDst[0], cHi = sDst[CH - 1];
#pragma unroll
            for (uint32_t w = 0; w < WORDS; w++) {
                const int64_t o = (int64_t)(w * NT + tid) * 16;
                int64_t pos = max(o, cLo);
                const int64_t end = min(min(o + 16, cHi), tEnd);
                if (pos >= end) continue;
                uint32_t a = 0, b = CH - 1;                                               // sDst[a] <= pos < sDst[CH - 1]
#pragma unroll 1
                while (b - a > 1) { const uint32_t m = (a + b) / 2; if (sDst[m] <= pos) a = m; else b = m; }
#pragma unroll 1
                for (uint32_t j = a; pos < end; j++) {
                    const int64_t e = min(sDst[j + 1], end);
                    if (e <= pos) continue;                                               // (an empty record)
                    Word16 v;
                    __builtin_memcpy(&v, (const uint8_t *)sSrc[j] + (pos - sDst[j]), 16);
                    v = place(v, (uint32_t)(pos - o), (uint32_t)(e - pos));
                    acc[w].lo |= v.lo; acc[w].hi |= v.hi;
                    pos = e;
                }
            }
            if (cHi >= tEnd || base + (CH - 1) >= n) break;                               // the tile is full, or no record is left (the caller's bytes never exceed dstOff[n])
        }
#pragma unroll
        for (uint32_t w = 0; w < WORDS; w++) {
            const int64_t o = (int64_t)(w * NT + tid) * 16;
            if (o < tEnd) *(Word16 *)(out + tile * TILE + o) = acc[w];
        }
    }
}

// ---- C ABI --------------------------------------------------------------------------------------------------------------------------------
#define DEV_HOST_PREFIX "BAM sort on the device: "
#define DEV_HOST_ROCPRIM
#include "dev_host.h"

struct staramd_bamsort {
    staramd_bgzf *z = nullptr; int device = 0; hipStream_t st = nullptr, stCopy = nullptr; uint32_t cus = 1;
    uint64_t budget = 0, slabBytes = 256ull << 20, roundBlocks = 8192;
    struct Slab { uint8_t *d; uint64_t cap, used; };
    struct Append { uint8_t *d; uint64_t bytes; };
    std::vector<Slab> slabs; uint64_t allocated = 0;
    std::vector<Append> appends;
    std::vector<uint64_t> g, r, addr; std::vector<uint32_t> len; uint64_t bytes = 0;      // one entry per record, in the order of appending; bytes: the sum of len = the stream's length
    GrowBuf stage[2]; hipEvent_t stageDone[2] = {}; bool stageBusy[2] = {false, false}; uint32_t nextStage = 0;     // page-locked, alternating
    hipEvent_t ev[12] = {};
    BamsortAfterOrder afterOrder = nullptr; void *afterOrderUser = nullptr;              // bamsort_resident.h
};

namespace {
int failBgzf() { g_err = staramd_bgzf_last_error(); return -1; }

uint64_t envBytes(const char *name, uint64_t dflt) { const char *e = getenv(name); const uint64_t v = e ? strtoull(e, nullptr, 10) : 0; return v ? v : dflt; }

void freeSlabs(staramd_bamsort *s) {
    for (auto &sl : s->slabs) (void)hipFree(sl.d);
    s->slabs.clear(); s->appends.clear(); s->allocated = 0; s->bytes = 0;
    std::vector<uint64_t>().swap(s->g); std::vector<uint64_t>().swap(s->r); std::vector<uint64_t>().swap(s->addr); std::vector<uint32_t>().swap(s->len);
}
int waitUploads(staramd_bamsort *s) {
    for (int k = 0; k < 2; k++) if (s->stageBusy[k]) { DH_TRY(hipEventSynchronize(s->stageDone[k])); s->stageBusy[k] = false; }
    return 0;
}

int finishOnDevice(staramd_bamsort *s, int level, int (*sink)(void *, const uint8_t *, uint64_t), void *user, uint64_t stats[8]) {
    typedef std::chrono::steady_clock Clock;
    const uint64_t n64 = s->g.size();
    const uint32_t n = (uint32_t)n64;
    if (s->bytes == 0) return 0;                                                        // no record, or empty ones only: no member
    hipStream_t st = s->st;
    Work wk;
    // ---- order
    uint64_t maxR = 0, maxG = 0; bool anyG = false;
    for (uint32_t i = 0; i < n; i++) { maxR = std::max(maxR, s->r[i]); if (s->g[i] != ~0ull) { maxG = std::max(maxG, s->g[i]); anyG = true; } }
    const uint64_t unmappedG = anyG ? maxG + 1 : 0;
    uint64_t *dG, *dKey, *dKeyAlt, *dAddr, *dLen64, *dSrc; uint32_t *dVal, *dValAlt, *dLen;
    if (wk.dev(dG, n) || wk.dev(dKey, n) || wk.dev(dKeyAlt, n) || wk.dev(dAddr, n) || wk.dev(dLen64, n64 + 1) || wk.dev(dSrc, n) || wk.dev(dVal, n) || wk.dev(dValAlt, n) || wk.dev(dLen, n)) return -1;
    { std::vector<uint64_t> gg(s->g); for (auto &x : gg) if (x == ~0ull) x = unmappedG;
      DH_TRY(hipMemcpyAsync(dG, gg.data(), n64 * 8, hipMemcpyHostToDevice, st)); DH_TRY(hipStreamSynchronize(st)); }
    DH_TRY(hipMemcpyAsync(dKey, s->r.data(), n64 * 8, hipMemcpyHostToDevice, st));
    DH_TRY(hipMemcpyAsync(dAddr, s->addr.data(), n64 * 8, hipMemcpyHostToDevice, st));
    DH_TRY(hipMemcpyAsync(dLen, s->len.data(), n64 * 4, hipMemcpyHostToDevice, st));
    const uint32_t gridN = gridFor(n64, NT, s->cus);
    DH_TRY(hipEventRecord(s->ev[0], st));
    DH_LAUNCH(k_bamsort_iota, dim3(gridN), st, dVal, n);
    PrimSpace prim;
    if (prim.sortPairs(st, dKey, dKeyAlt, dVal, dValAlt, n, bitsOf(maxR))) return -1;
    DH_LAUNCH(k_bamsort_pick, dim3(gridN), st, dVal, dG, n, dKeyAlt);
    std::swap(dKey, dKeyAlt);
    if (prim.sortPairs(st, dKey, dKeyAlt, dVal, dValAlt, n, bitsOf(std::max(maxG, unmappedG)))) return -1;
    DH_TRY(hipEventRecord(s->ev[1], st));
    // ---- where every record goes
    DH_LAUNCH(k_bamsort_order, dim3(gridN), st, dVal, dLen, dAddr, n, dLen64, dSrc);
    if (prim.exclusiveScan(st, dLen64, (size_t)n64 + 1)) return -1;
    const uint64_t *dDst = dLen64;
    DH_TRY(hipEventRecord(s->ev[2], st));
    if (s->afterOrder && s->afterOrder(s->afterOrderUser, st, s->cus, dSrc, dDst, n64)) return fail("the pass over the ordered records reported an error");
    // ---- rounds
    const uint64_t total = s->bytes, nbAll = (total + IN_MAX - 1) / IN_MAX, RB = std::min(s->roundBlocks, nbAll), rounds = (nbAll + RB - 1) / RB;
    const uint64_t roundCap = RB * IN_MAX, outCap = staramd_bgzf_bound(roundCap);
    uint8_t *dRound, *dOut[2], *hOut[2]; uint64_t *dOff[2], *hTot[2], *dBlkOff; uint32_t *dBlkLen, *dBlkLenLast;
    if (wk.dev(dRound, roundCap + 16) || wk.dev(dBlkOff, RB) || wk.dev(dBlkLen, RB) || wk.dev(dBlkLenLast, RB)) return -1;
    for (int k = 0; k < 2; k++) if (wk.dev(dOut[k], outCap) || wk.dev(dOff[k], RB + 1) || wk.host(hOut[k], outCap) || wk.host(hTot[k], 1)) return -1;
    if (bgzfResidentReserve(s->z, RB)) return failBgzf();
    const uint64_t nbLast = nbAll - (rounds - 1) * RB;
    std::vector<uint64_t> blkOff(RB); std::vector<uint32_t> blkLen(RB, IN_MAX), blkLenLast(RB, IN_MAX);
    for (uint64_t b = 0; b < RB; b++) blkOff[b] = b * IN_MAX;
    blkLenLast[nbLast - 1] = (uint32_t)(total - (nbAll - 1) * IN_MAX);
    DH_TRY(hipMemcpyAsync(dBlkOff, blkOff.data(), RB * 8, hipMemcpyHostToDevice, st));
    DH_TRY(hipMemcpyAsync(dBlkLen, blkLen.data(), RB * 4, hipMemcpyHostToDevice, st));
    DH_TRY(hipMemcpyAsync(dBlkLenLast, blkLenLast.data(), RB * 4, hipMemcpyHostToDevice, st));
    DH_TRY(hipStreamSynchronize(st));
    float msSort = 0, msScan = 0, msGather = 0, msDeflate = 0, msD2H = 0; double sSink = 0; uint64_t outBytes = 0;
    (void)hipEventElapsedTime(&msSort, s->ev[0], s->ev[1]); (void)hipEventElapsedTime(&msScan, s->ev[1], s->ev[2]);
    auto launchRound = [&](uint64_t k) -> int {          // events 3 * parity + 3 ..: before the gather, between gather and deflate, after the deflate
        const int p = (int)(k & 1);
        const uint64_t start = k * roundCap, bytes = std::min(roundCap, total - start), nb = k + 1 == rounds ? nbLast : RB;
        const uint64_t nTiles = (bytes + TILE - 1) / TILE;
        DH_TRY(hipEventRecord(s->ev[3 + 3 * p], st));
        DH_LAUNCH(k_bamsort_gather, dim3((uint32_t)std::min<uint64_t>(nTiles, 4ull * s->cus)), st, dDst, (const uint64_t *)dSrc, n64, start, bytes, dRound);
        DH_TRY(hipEventRecord(s->ev[4 + 3 * p], st));
        if (bgzfCompressResident(s->z, dRound, dBlkOff, k + 1 == rounds ? dBlkLenLast : dBlkLen, (uint32_t)nb, level, dOut[p], dOff[p])) return failBgzf();
        DH_TRY(hipMemcpyAsync(hTot[p], dOff[p] + nb, 8, hipMemcpyDeviceToHost, st));
        DH_TRY(hipEventRecord(s->ev[5 + 3 * p], st));
        return 0;
    };
    if (launchRound(0)) return -1;
    for (uint64_t k = 0; k < rounds; k++) {
        const int p = (int)(k & 1);
        if (k + 1 < rounds && launchRound(k + 1)) return -1;
        DH_TRY(hipEventSynchronize(s->ev[5 + 3 * p]));
        const uint64_t got = *hTot[p];
        if (got > outCap) return fail("device output larger than its bound");
        DH_TRY(hipEventRecord(s->ev[9], s->stCopy));
        DH_TRY(hipMemcpyAsync(hOut[p], dOut[p], got, hipMemcpyDeviceToHost, s->stCopy));
        DH_TRY(hipEventRecord(s->ev[10], s->stCopy));
        DH_TRY(hipStreamSynchronize(s->stCopy));
        float a = 0, b = 0, c = 0;
        (void)hipEventElapsedTime(&a, s->ev[3 + 3 * p], s->ev[4 + 3 * p]); (void)hipEventElapsedTime(&b, s->ev[4 + 3 * p], s->ev[5 + 3 * p]); (void)hipEventElapsedTime(&c, s->ev[9], s->ev[10]);
        msGather += a; msDeflate += b; msD2H += c;
        const auto t0 = Clock::now();
        if (sink(user, hOut[p], got)) { (void)hipStreamSynchronize(st); return fail("the sink of the compressed members reported an error"); }
        sSink += std::chrono::duration<double>(Clock::now() - t0).count();
        outBytes += got;
    }
    DH_TRY(hipStreamSynchronize(st));
    if (stats) { stats[0] = n; stats[1] = total; stats[2] = rounds; stats[3] = outBytes; stats[4] = (uint64_t)(msSort * 1e6); stats[5] = (uint64_t)(msGather * 1e6);
                 stats[6] = (uint64_t)(msDeflate * 1e6); stats[7] = (uint64_t)(sSink * 1e9); }
    static const bool timing = getenv("STARAMD_HOST_TIMING") != nullptr;
    if (timing)
        fprintf(stderr, "  bamsort device: %u records, %.1f -> %.1f MB, %llu rounds: sort %.2f ms, lengths + scan %.2f ms, gather %.2f ms, deflate %.2f ms, D2H %.2f ms, sink %.2f ms\n",
                n, total / 1e6, outBytes / 1e6, (unsigned long long)rounds, msSort, msScan, msGather, msDeflate, msD2H, sSink * 1e3);
    return 0;
}
}  // namespace

extern "C" {

const char *staramd_bamsort_last_error(void) { return g_err.c_str(); }

int staramd_bamsort_create(staramd_bamsort **out, staramd_bgzf *z, uint64_t hbmBudgetBytes) {
    *out = nullptr;
    if (!z) return fail("no BGZF compressor to work with");
    staramd_bamsort *s = new staramd_bamsort();
    s->z = z; s->budget = hbmBudgetBytes;
    uint32_t grid = 2;
    bgzfResidentInfo(z, &s->device, &s->st, &grid);
    s->cus = std::max(1u, grid / 2);
    s->slabBytes = envBytes("STARAMD_BAMSORT_SLAB_BYTES", 256ull << 20);
    s->roundBlocks = envBytes("STARAMD_BAMSORT_ROUND_BLOCKS", 8192);
    auto bad = [&](int rc) { staramd_bamsort_destroy(s); return rc; };
    hipError_t e = hipSetDevice(s->device);
    if (e != hipSuccess) return bad(failHip("hipSetDevice", e));
    if ((e = hipStreamCreate(&s->stCopy)) != hipSuccess) return bad(failHip("hipStreamCreate", e));
    for (auto &x : s->stageDone) if ((e = hipEventCreate(&x)) != hipSuccess) return bad(failHip("hipEventCreate", e));
    for (auto &x : s->ev) if ((e = hipEventCreate(&x)) != hipSuccess) return bad(failHip("hipEventCreate", e));
    *out = s;
    return 0;
}

void staramd_bamsort_destroy(staramd_bamsort *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->st) (void)hipStreamSynchronize(s->st);
    if (s->stCopy) (void)hipStreamSynchronize(s->stCopy);
    freeSlabs(s);
    for (auto &b : s->stage) b.release();
    for (auto &x : s->stageDone) if (x) (void)hipEventDestroy(x);
    for (auto &x : s->ev) if (x) (void)hipEventDestroy(x);
    if (s->stCopy) (void)hipStreamDestroy(s->stCopy);
    delete s;
}

int staramd_bamsort_append(staramd_bamsort *s, const uint8_t *records, uint64_t bytes, const staramd_bam_key *keys, uint32_t n) {
    if (!s) return fail("no sorter");
    if (s->g.size() + (uint64_t)n > 0xffffffffull) return fail("more than 2^32 - 1 records");
    for (uint32_t i = 0; i < n; i++) if (keys[i].off > bytes || keys[i].len > bytes - keys[i].off) return fail("record " + std::to_string(i) + " of an append lies outside its " + std::to_string(bytes) + " bytes");
    DH_TRY(hipSetDevice(s->device));
    if (s->budget == 0) { size_t fr = 0, tot = 0; DH_TRY(hipMemGetInfo(&fr, &tot)); s->budget = std::max<uint64_t>(1, fr / 2); }
    // the slab: the last one when the append fits behind what it holds, else a new one within the budget
    staramd_bamsort::Slab *sl = s->slabs.empty() ? nullptr : &s->slabs.back();
    if (!sl || sl->cap - sl->used < bytes) {
        const uint64_t left = s->budget > s->allocated ? s->budget - s->allocated : 0;
        const uint64_t cap = std::max(bytes, std::min(s->slabBytes, left));
        if (cap > left) return 1;
        uint8_t *d = nullptr;
        hipError_t e = hipMalloc((void **)&d, cap + SLAB_PAD);
        if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return 1; }
        if (e != hipSuccess) return failHip("hipMalloc", e);
        s->slabs.push_back({d, cap, 0}); s->allocated += cap;
        sl = &s->slabs.back();
    }
    uint8_t *dst = sl->d + sl->used;
    if (bytes) {
        const uint32_t k = s->nextStage; s->nextStage ^= 1;
        if (s->stageBusy[k]) { DH_TRY(hipEventSynchronize(s->stageDone[k])); s->stageBusy[k] = false; }
        if (s->stage[k].grow(bytes, false)) return -1;
        copyPieces({{s->stage[k].h, records, bytes}}, bytes);           // (a batch's ranges are some MB each)
        DH_TRY(hipMemcpyAsync(dst, s->stage[k].h, bytes, hipMemcpyHostToDevice, s->st));
        DH_TRY(hipEventRecord(s->stageDone[k], s->st));
        s->stageBusy[k] = true;
    }
    sl->used += bytes;
    for (uint32_t i = 0; i < n; i++) s->bytes += keys[i].len;              // the stream is what the keys name: gaps in `records` are left out, bytes under two keys go out twice
    s->appends.push_back({dst, bytes});
    for (uint32_t i = 0; i < n; i++) { s->g.push_back(keys[i].g); s->r.push_back(keys[i].r); s->addr.push_back((uint64_t)(uintptr_t)(dst + keys[i].off)); s->len.push_back(keys[i].len); }
    return 0;
}

int staramd_bamsort_download(staramd_bamsort *s, uint32_t iAppend, uint8_t *records) {
    if (!s) return fail("no sorter");
    if (iAppend >= s->appends.size()) return fail("append " + std::to_string(iAppend) + " of " + std::to_string(s->appends.size()));
    DH_TRY(hipSetDevice(s->device));
    if (waitUploads(s)) return -1;
    const staramd_bamsort::Append &a = s->appends[iAppend];
    if (a.bytes) DH_TRY(hipMemcpy(records, a.d, a.bytes, hipMemcpyDeviceToHost));
    return 0;
}

int staramd_bamsort_finish(staramd_bamsort *s, int level, int (*sink)(void *user, const uint8_t *bytes, uint64_t n), void *user, uint64_t stats[8]) {
    if (!s) return fail("no sorter");
    if (stats) for (int i = 0; i < 8; i++) stats[i] = 0;
    (void)hipSetDevice(s->device);
    int rc = waitUploads(s);
    if (rc == 0 && sink) {
        if ((rc = checkLevel(level)) == 0) {
            bgzfResidentLock(s->z);
            rc = finishOnDevice(s, level, sink, user, stats);
            (void)hipStreamSynchronize(s->st); (void)hipStreamSynchronize(s->stCopy);
            bgzfResidentUnlock(s->z);
        }
    }
    freeSlabs(s);
    s->afterOrder = nullptr; s->afterOrderUser = nullptr;
    return rc;
}

}  // extern "C"

void bamsortSetAfterOrder(staramd_bamsort *s, BamsortAfterOrder fn, void *user) { s->afterOrder = fn; s->afterOrderUser = user; }
