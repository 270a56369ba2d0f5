// k_signal.hip -- the signal tracks of --outWigType on the MI355X, from BAM records in coordinate order that are in device memory (include/star_amd_signal.h).
// Self-contained beside k_bamsort.hip (bamsort_resident.h) and k_bgzf.hip, so that the wave emulator can compile the three alone.
//
//   records   k_signal_records: one lane per record in sorted order.  flag, pos, n_cigar, the NH attribute (the walk of auxInt in host/signal.cpp); the skips
//             (0x400, NH = 0, tid < 0 or unwanted), the mate and strand rules; the number of (tile, span) pairs the record emits -- a span is one contributing
//             M block (or the single position of read1_5p), a tile is T consecutive positions of one chromosome; the normalisation word; the flag
//             "a span reaches chrLength + 1"
//   scan      rocprim::exclusive_scan of the counts = where each record's pairs go
//   emit      k_signal_emit: the same walk, writing key (tid << tileBits | tile) and value (NH, strand, first and last position inside the tile) in record order
//   sort      rocprim::radix_sort_pairs by key over the bits in use: STABLE, so the spans of a tile stay in record order
//   tiles     head flags over the sorted keys + a scan = the occupied tiles and where each begins.  k_signal_tiles: one workgroup per occupied tile, a lane owns
//             P = T / 256 consecutive positions; the tile's spans go through LDS in chunks of CHUNK and are applied one after the other, every lane whose
//             position lies in the span adding (an integer count when NH = 1, 1.0 / NH in double always: one rounding per addition, in record order);
//             then, per track, a boundary wherever the value differs from the position before (always at the tile's first position), as bit masks in LDS;
//             the runs that are not zero are counted (first launch), the counts scanned, and written in order (second launch, same arithmetic).
// T, CHUNK and the workgroups per CU are choices, not measured optima.  1.0 / NH is the IEEE quotient: the engine is compiled without fast-math.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <rocprim/rocprim.hpp>
#include <string>
#include <vector>
#include <algorithm>
#include "../../../include/star_amd_signal.h"
#include "bamsort_resident.h"
#include "../bam_aux.h"

namespace {

constexpr uint32_t NT = 256;                        // work-items per workgroup
constexpr uint32_t LOG_T = 10, T = 1u << LOG_T;     // positions per tile
constexpr uint32_t P = T / NT;                      // consecutive positions per lane
constexpr uint32_t CHUNK = 256;                     // spans per LDS chunk (one load per lane)
constexpr uint32_t WORDS = T / 32;                  // words of a boundary mask
static_assert(P >= 1 && 32 % P == 0 && CHUNK <= NT && WORDS <= NT, "a lane's positions lie in one mask word; a chunk is loaded in one step");

// a span's value word: NH [0, 32), strand [32], first position inside the tile [33, 43), last position inside the tile [43, 53)
__device__ __forceinline__ uint64_t packSpan(uint32_t nh, uint32_t strand, uint32_t first, uint32_t last) { return (uint64_t)nh | (uint64_t)strand << 32 | (uint64_t)first << 33 | (uint64_t)last << 43; }

__device__ __forceinline__ uint32_t ld32(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }      // records lie at arbitrary byte addresses

// the NH attribute of a record of `lim` bytes (auxInt of host/signal.cpp, with every read held inside the record): false = absent
// (the walk itself is bamAuxInts of bam_aux.h, which k_dedup.hip shares)
__device__ bool auxNH(const uint8_t *rec, uint64_t lim, uint64_t a, uint32_t &val) {
    uint32_t none = 0;
    return bamAuxInts(rec, lim, a, 'N', 'H', val, false, 0, 0, none) != 0;
}

struct SigArgs { int32_t type, strand; uint32_t nChr, tileBits; const uint32_t *chrLength, *wanted; };

// One record: the (tile, span) pairs it emits, counted and -- with key != nullptr -- written from key[0], val[0] on.  norm, chrHas, pastEnd: written when not null
__device__ uint64_t walkRecord(const uint8_t *rec, uint64_t len, const SigArgs &A, uint64_t *key, uint64_t *val, uint32_t *norm, uint32_t *chrHas, uint32_t *pastEnd) {
    if (norm) *norm = 0;
    if (len < 36) return 0;
    const uint64_t lim = min(len, (uint64_t)ld32(rec) + 4);
    if (lim < 36) return 0;
    const int32_t tid = (int32_t)ld32(rec + 4);
    if (tid < 0 || (uint32_t)tid >= A.nChr || !A.wanted[tid]) return 0;
    if (chrHas) chrHas[tid] = 1;
    const uint32_t bmn = ld32(rec + 12), fnc = ld32(rec + 16), lseq = ld32(rec + 20), flag = fnc >> 16, nCigar = fnc & 0xffff;
    const uint64_t cigar = 36 + (uint64_t)(bmn & 0xff);
    uint32_t aNH = 1, nh = 0;
    if (auxNH(rec, lim, cigar + 4 * (uint64_t)nCigar + ((uint64_t)lseq + 1) / 2 + lseq, nh)) { aNH = nh; if (norm) *norm = nh; }     // for the normalisation a record without NH is skipped; for the signal it counts as NH = 1
    if ((flag & 0x400) || aNH == 0) return 0;
    uint32_t aG = ld32(rec + 8), iStrand = 0;
    if (A.strand) iStrand = ((flag & 0x10) > 0) == ((flag & 0x80) == 0);
    const uint64_t chrLen = (uint64_t)A.chrLength[tid] + 1;             // one extra base at the end
    uint64_t cnt = 0;
    auto span = [&](uint32_t a, uint32_t n) {                           // positions a .. a + n - 1, n > 0
        if ((uint64_t)a + n > chrLen) { if (pastEnd) *pastEnd = 1; return; }
        const uint32_t last = a + n - 1;
#pragma unroll 1
        for (uint32_t t = a >> LOG_T; t <= last >> LOG_T; t++) {
            const uint32_t t0 = t << LOG_T;
            if (key) { key[cnt] = (uint64_t)(uint32_t)tid << A.tileBits | t; val[cnt] = packSpan(aNH, iStrand, max(a, t0) - t0, min(last - t0, T - 1)); }
            cnt++;
        }
    };
    if (A.type == 1) {
        if (flag & 0x80) return 0;
        if (iStrand == 0) { span(aG, 1); return cnt; }
    }
    const bool contributes = A.type == 0 || (A.type == 2 && (flag & 0x80));
#pragma unroll 1
    for (uint32_t ic = 0; ic < nCigar && cigar + 4 * (uint64_t)ic + 4 <= lim; ic++) {
        const uint32_t c = ld32(rec + cigar + 4 * (uint64_t)ic), op = c & 0xf, n = c >> 4;
        if (op == 2 || op == 3) aG += n;
        else if (op == 0) { if (contributes && n) span(aG, n); aG += n; }
    }
    if (A.type == 1) span(aG - 1, 1);
    return cnt;
}

}  // namespace

// cnt[i] = pairs of sorted record i (cnt[n] = 0, so that the scan leaves the total there); record i = addr[i], dst[i + 1] - dst[i] bytes
__global__ __launch_bounds__(256) void k_signal_records(const uint64_t *__restrict__ addr, const uint64_t *__restrict__ dst, uint64_t n, SigArgs A, uint64_t *__restrict__ cnt,
                                                        uint32_t *__restrict__ norm, uint32_t *__restrict__ chrHas, uint32_t *__restrict__ pastEnd) {
    for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * NT) {
        if (i == n) { cnt[i] = 0; continue; }
        cnt[i] = walkRecord((const uint8_t *)addr[i], dst[i + 1] - dst[i], A, nullptr, nullptr, norm ? norm + i : nullptr, chrHas, pastEnd);
    }
}
// the pairs of record i at off[i] .. (off = the scanned counts)
__global__ __launch_bounds__(256) void k_signal_emit(const uint64_t *__restrict__ addr, const uint64_t *__restrict__ dst, uint64_t n, SigArgs A, const uint64_t *__restrict__ off,
                                                     uint64_t *__restrict__ key, uint64_t *__restrict__ val) {
    for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * NT) {
        const uint64_t o = off[i];
        if (off[i + 1] == o) continue;
        (void)walkRecord((const uint8_t *)addr[i], dst[i + 1] - dst[i], A, key + o, val + o, nullptr, nullptr, nullptr);
    }
}
// head[i] = 1 where a tile begins in the sorted keys (head[n] = 0: the scan leaves the number of tiles there)
__global__ __launch_bounds__(256) void k_signal_heads(const uint64_t *__restrict__ key, uint64_t n, uint64_t *__restrict__ head) {
    for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * NT) head[i] = i < n && (i == 0 || key[i] != key[i - 1]);
}
// start[k] = first pair of occupied tile k; start[number of tiles] = n.  rank = the scanned head flags
__global__ __launch_bounds__(256) void k_signal_tile_starts(const uint64_t *__restrict__ key, const uint64_t *__restrict__ rank, uint64_t n, uint64_t *__restrict__ start) {
    for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * NT) if (i == n || i == 0 || key[i] != key[i - 1]) start[rank[i]] = i;
}

// One workgroup per occupied tile (grid-stride).  fill == 0: runs[] is not touched, nRuns[tile] = the tile's runs.  fill != 0: nRuns is the exclusive scan of
// those counts and the tile's runs are written from runs[nRuns[tile]] on, track by track, in ascending order of position
__global__ __launch_bounds__(256) void k_signal_tiles(const uint64_t *__restrict__ key, const uint64_t *__restrict__ val, const uint64_t *__restrict__ start, uint64_t nTiles,
                                                      uint32_t tileBits, int strand, int fill, uint64_t *__restrict__ nRuns, staramd_signal_run *__restrict__ runs) {
    __shared__ uint64_t sVal[CHUNK];
    __shared__ double sInv[CHUNK];
    __shared__ double sEdge[NT];                    // the value at every lane's last position
    __shared__ uint32_t sBound[WORDS], sStart[WORDS], sPre[WORDS + 1];
    const uint32_t lane = threadIdx.x, p0 = lane * P, w = p0 / 32, sh = p0 % 32;
    const int sigN = strand ? 4 : 2;
#pragma unroll 1
    for (uint64_t tile = blockIdx.x; tile < nTiles; tile += gridDim.x) {
        const uint64_t b = start[tile], e = start[tile + 1], k = key[b];
        const int32_t tid = (int32_t)(k >> tileBits);
        const uint32_t base = (uint32_t)(k & ((1ull << tileBits) - 1)) << LOG_T;
        uint32_t uq0[P], uq1[P]; double mu0[P], mu1[P];
#pragma unroll
        for (uint32_t q = 0; q < P; q++) { uq0[q] = 0; uq1[q] = 0; mu0[q] = 0; mu1[q] = 0; }
#pragma unroll 1
        for (uint64_t c = b; c < e; c += CHUNK) {
            __syncthreads();
            if (lane < CHUNK && c + lane < e) { const uint64_t v = val[c + lane]; sVal[lane] = v; sInv[lane] = 1.0 / (double)(uint32_t)v; }
            __syncthreads();
            const uint32_t m = (uint32_t)min((uint64_t)CHUNK, e - c);
#pragma unroll 1
            for (uint32_t j = 0; j < m; j++) {
                const uint64_t v = sVal[j];
                const uint32_t first = (uint32_t)(v >> 33) & (T - 1), last = (uint32_t)(v >> 43) & (T - 1);
                if (last < p0 || first >= p0 + P) continue;
                const uint32_t one = (uint32_t)v == 1; const double inv = sInv[j];
                if ((v >> 32) & 1) {
#pragma unroll
                    for (uint32_t q = 0; q < P; q++) if (p0 + q >= first && p0 + q <= last) { uq1[q] += one; mu1[q] += inv; }
                } else {
#pragma unroll
                    for (uint32_t q = 0; q < P; q++) if (p0 + q >= first && p0 + q <= last) { uq0[q] += one; mu0[q] += inv; }
                }
            }
        }
        uint64_t outBase = fill ? nRuns[tile] : 0, total = 0;
#pragma unroll 1
        for (int tr = 0; tr < sigN; tr++) {
            double x[P];
#pragma unroll
            for (uint32_t q = 0; q < P; q++) x[q] = tr == 0 ? (double)uq0[q] : tr == 1 ? mu0[q] : tr == 2 ? (double)uq1[q] : mu1[q];
            __syncthreads();
            sEdge[lane] = x[P - 1];
            if (lane < WORDS) { sBound[lane] = 0; sStart[lane] = 0; }
            __syncthreads();
            double prev = lane ? sEdge[lane - 1] : 0.0;
            uint32_t bound = 0, begin = 0;
#pragma unroll
            for (uint32_t q = 0; q < P; q++) {
                if (x[q] != prev || p0 + q == 0) { bound |= 1u << q; if (x[q] != 0) begin |= 1u << q; }
                prev = x[q];
            }
            if (bound) atomicOr(&sBound[w], bound << sh);
            if (begin) atomicOr(&sStart[w], begin << sh);
            __syncthreads();
            if (lane == 0) { uint32_t acc = 0; for (uint32_t i = 0; i < WORDS; i++) { sPre[i] = acc; acc += (uint32_t)__popc(sStart[i]); } sPre[WORDS] = acc; }
            __syncthreads();
            if (fill && begin) {
#pragma unroll
                for (uint32_t q = 0; q < P; q++) {
                    if (!(begin >> q & 1)) continue;
                    const uint32_t bit = sh + q;
                    const uint32_t rank = sPre[w] + (uint32_t)__popc(sStart[w] & ((1u << bit) - 1));
                    uint32_t ww = w, mm = sBound[w] & ~((2u << bit) - 1);                 // the next boundary above this position ends the run
                    while (mm == 0 && ++ww < WORDS) mm = sBound[ww];
                    const uint32_t endp = mm ? ww * 32 + (uint32_t)__ffs((int)mm) - 1 : T;
                    staramd_signal_run r; r.tid = tid; r.track = (uint32_t)tr; r.start = base + p0 + q; r.end = base + endp; r.value = x[q];
                    runs[outBase + total + rank] = r;
                }
            }
            total += sPre[WORDS];
        }
        if (!fill && lane == 0) nRuns[tile] = total;
    }
}

// ---- C ABI --------------------------------------------------------------------------------------------------------------------------------
#define DEV_HOST_PREFIX "signal tracks on the device: "
#define DEV_HOST_ROCPRIM
#include "dev_host.h"

namespace {
void clearResult(staramd_signal_result *r) { memset(r, 0, sizeof(*r)); }
int checkParams(const staramd_signal_params *p, staramd_signal_result *out) {
    if (!p || !out) return fail("no parameters or no result");
    clearResult(out);
    if (p->type < 0 || p->type > 2) return fail("type " + std::to_string(p->type) + " is not 0, 1 or 2");
    if (p->nChr && (!p->chrLength || !p->wanted)) return fail("no chromosome lengths");
    if (p->nChr > 0x7fffffffu) return fail("more than 2^31 - 1 chromosomes");
    out->nChr = p->nChr;
    out->chrHas = (uint8_t *)calloc(std::max<uint32_t>(p->nChr, 1), 1);
    if (!out->chrHas) return fail("no host memory for the result");
    return 0;
}

// the tracks of the n records dAddr[i] (dDst[i + 1] - dDst[i] bytes each) on stream st; out was cleared by checkParams
int signalOnDevice(hipStream_t st, uint32_t cus, const uint64_t *dAddr, const uint64_t *dDst, uint64_t n, const staramd_signal_params *p, staramd_signal_result *out) {
    out->nRecords = n; out->stats[0] = n;
    if (n == 0) return 0;
    Work wk;
    hipEvent_t ev[5];
    for (auto &e : ev) if (wk.event(e)) return -1;
    uint32_t maxLen = 0;
    std::vector<uint32_t> wanted(p->nChr);
    for (uint32_t i = 0; i < p->nChr; i++) { maxLen = std::max(maxLen, p->chrLength[i]); wanted[i] = p->wanted[i] ? 1 : 0; }
    SigArgs A; A.type = p->type; A.strand = p->strand ? 1 : 0; A.nChr = p->nChr; A.tileBits = bitsOf(((uint64_t)maxLen + 1) >> LOG_T);
    uint32_t *dLen, *dWanted, *dNorm = nullptr, *dHas, *dPast; uint64_t *dCnt;
    if (wk.dev(dLen, p->nChr) || wk.dev(dWanted, p->nChr) || wk.dev(dHas, p->nChr) || wk.dev(dPast, 1) || wk.dev(dCnt, n + 1)) return -1;
    if (p->wantNorm && wk.dev(dNorm, n)) return -1;
    DH_TRY(hipMemcpyAsync(dLen, p->chrLength, (uint64_t)p->nChr * 4, hipMemcpyHostToDevice, st));
    DH_TRY(hipMemcpyAsync(dWanted, wanted.data(), (uint64_t)p->nChr * 4, hipMemcpyHostToDevice, st));
    DH_TRY(hipMemsetAsync(dHas, 0, std::max<uint64_t>(p->nChr, 1) * 4, st));
    DH_TRY(hipMemsetAsync(dPast, 0, 4, st));
    A.chrLength = dLen; A.wanted = dWanted;
    PrimSpace prim;
    // ---- records, scan
    DH_TRY(hipEventRecord(ev[0], st));
    DH_LAUNCH(k_signal_records, dim3(gridFor(n, NT, cus)), st, dAddr, dDst, n, A, dCnt, dNorm, dHas, dPast);
    if (prim.exclusiveScan(st, dCnt, n + 1)) return -1;
    uint64_t nPairs = 0; uint32_t past = 0;
    std::vector<uint32_t> has(p->nChr);
    DH_TRY(hipMemcpyAsync(&nPairs, dCnt + n, 8, hipMemcpyDeviceToHost, st));
    DH_TRY(hipMemcpyAsync(&past, dPast, 4, hipMemcpyDeviceToHost, st));
    DH_TRY(hipMemcpyAsync(has.data(), dHas, (uint64_t)p->nChr * 4, hipMemcpyDeviceToHost, st));
    DH_TRY(hipStreamSynchronize(st));
    for (uint32_t i = 0; i < p->nChr; i++) out->chrHas[i] = has[i] ? 1 : 0;
    if (dNorm) {
        out->norm = (uint32_t *)malloc(n * 4);
        if (!out->norm) return fail("no host memory for the result");
        DH_TRY(hipMemcpyAsync(out->norm, dNorm, n * 4, hipMemcpyDeviceToHost, st));
    }
    out->stats[1] = nPairs;
    if (past) { out->pastEnd = 1; DH_TRY(hipStreamSynchronize(st)); return 0; }
    uint64_t nTiles = 0, nRunsTotal = 0;
    float msRec = 0, msSort = 0, msTiles = 0, msBack = 0;
    if (nPairs) {
        // ---- emit, sort
        uint64_t *dKey, *dKeyAlt, *dVal, *dValAlt;
        if (wk.dev(dKey, nPairs + 1) || wk.dev(dKeyAlt, nPairs + 1) || wk.dev(dVal, nPairs + 1) || wk.dev(dValAlt, nPairs + 1)) return -1;
        DH_LAUNCH(k_signal_emit, dim3(gridFor(n, NT, cus)), st, dAddr, dDst, n, A, (const uint64_t *)dCnt, dKey, dVal);
        DH_TRY(hipEventRecord(ev[1], st));
        if (prim.sortPairs(st, dKey, dKeyAlt, dVal, dValAlt, nPairs, A.tileBits + bitsOf(p->nChr ? p->nChr - 1 : 0))) return -1;
        DH_TRY(hipEventRecord(ev[2], st));
        // ---- occupied tiles: the alternate buffers of the sort (whichever they are now: all four have the spare entry) hold head flags / ranks and tile starts
        uint64_t *dRank = dKeyAlt, *dStart = dValAlt;
        DH_LAUNCH(k_signal_heads, dim3(gridFor(nPairs, NT, cus)), st, (const uint64_t *)dKey, nPairs, dRank);
        if (prim.exclusiveScan(st, dRank, nPairs + 1)) return -1;
        DH_LAUNCH(k_signal_tile_starts, dim3(gridFor(nPairs, NT, cus)), st, (const uint64_t *)dKey, (const uint64_t *)dRank, nPairs, dStart);
        DH_TRY(hipMemcpyAsync(&nTiles, dRank + nPairs, 8, hipMemcpyDeviceToHost, st));
        DH_TRY(hipStreamSynchronize(st));
        // ---- tiles: count, scan, fill
        uint64_t *dRuns64 = dRank;                                  // the ranks are done with: nTiles + 1 <= nPairs + 1 counts
        const dim3 gridT((uint32_t)std::min<uint64_t>(nTiles, 8ull * cus));
        DH_TRY(hipMemsetAsync(dRuns64 + nTiles, 0, 8, st));
        DH_LAUNCH(k_signal_tiles, gridT, st, (const uint64_t *)dKey, (const uint64_t *)dVal, (const uint64_t *)dStart, nTiles, A.tileBits, A.strand, 0, dRuns64, (staramd_signal_run *)nullptr);
        if (prim.exclusiveScan(st, dRuns64, nTiles + 1)) return -1;
        DH_TRY(hipMemcpyAsync(&nRunsTotal, dRuns64 + nTiles, 8, hipMemcpyDeviceToHost, st));
        DH_TRY(hipStreamSynchronize(st));
        staramd_signal_run *dRuns = nullptr;
        if (nRunsTotal) {
            if (wk.dev(dRuns, nRunsTotal)) return -1;
            DH_LAUNCH(k_signal_tiles, gridT, st, (const uint64_t *)dKey, (const uint64_t *)dVal, (const uint64_t *)dStart, nTiles, A.tileBits, A.strand, 1, dRuns64, dRuns);
        }
        DH_TRY(hipEventRecord(ev[3], st));
        if (nRunsTotal) {
            out->runs = (staramd_signal_run *)malloc(nRunsTotal * sizeof(staramd_signal_run));
            if (!out->runs) return fail("no host memory for the result");
            DH_TRY(hipMemcpyAsync(out->runs, dRuns, nRunsTotal * sizeof(staramd_signal_run), hipMemcpyDeviceToHost, st));
            out->nRuns = nRunsTotal;
        }
        DH_TRY(hipEventRecord(ev[4], st));
        DH_TRY(hipStreamSynchronize(st));
        (void)hipEventElapsedTime(&msRec, ev[0], ev[1]); (void)hipEventElapsedTime(&msSort, ev[1], ev[2]); (void)hipEventElapsedTime(&msTiles, ev[2], ev[3]); (void)hipEventElapsedTime(&msBack, ev[3], ev[4]);
    } else DH_TRY(hipStreamSynchronize(st));
    out->stats[2] = nTiles; out->stats[3] = nRunsTotal * sizeof(staramd_signal_run);
    out->stats[4] = (uint64_t)(msRec * 1e6); out->stats[5] = (uint64_t)(msSort * 1e6); out->stats[6] = (uint64_t)(msTiles * 1e6); out->stats[7] = (uint64_t)(msBack * 1e6);
    static const bool timing = getenv("STARAMD_HOST_TIMING") != nullptr;
    if (timing)
        fprintf(stderr, "  signal device: %llu records, %llu pairs, %llu tiles, %llu runs (%.1f MB): records + scan + emit %.2f ms, sort %.2f ms, tiles %.2f ms, D2H %.2f ms\n",
                (unsigned long long)n, (unsigned long long)nPairs, (unsigned long long)nTiles, (unsigned long long)nRunsTotal, nRunsTotal * sizeof(staramd_signal_run) / 1e6, msRec, msSort, msTiles, msBack);
    return 0;
}

struct SorterJob { const staramd_signal_params *p; staramd_signal_result *out; bool failed; };
}  // namespace

extern "C" {

const char *staramd_signal_last_error(void) { return g_err.c_str(); }
uint32_t staramd_signal_constant(int which) { return which == 0 ? T : which == 1 ? CHUNK : 0; }

void staramd_signal_free(staramd_signal_result *r) {
    if (!r) return;
    free(r->runs); free(r->norm); free(r->chrHas);
    clearResult(r);
}

int staramd_signal_host_records(int device, const staramd_signal_params *p, const uint8_t *bytes, uint64_t nBytes, const uint64_t *offsets, uint64_t n, staramd_signal_result *out) {
    if (checkParams(p, out)) return -1;
    auto bad = [&](int rc) { staramd_signal_free(out); return rc; };
    std::vector<uint64_t> addr(n), dst(n + 1);
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; i++) {
        uint32_t bs = 0;
        if (offsets[i] > nBytes || nBytes - offsets[i] < 4) return bad(fail("record " + std::to_string(i) + " lies outside the " + std::to_string(nBytes) + " bytes"));
        memcpy(&bs, bytes + offsets[i], 4);
        if (nBytes - offsets[i] - 4 < bs) return bad(fail("record " + std::to_string(i) + " lies outside the " + std::to_string(nBytes) + " bytes"));
        dst[i] = total; total += 4 + (uint64_t)bs;
    }
    dst[n] = total;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return bad(failHip("hipSetDevice", e));
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return bad(failHip("hipGetDeviceProperties", e));
    hipStream_t st = nullptr;
    if ((e = hipStreamCreate(&st)) != hipSuccess) return bad(failHip("hipStreamCreate", e));
    int rc = 0;
    {   Work wk;
        uint8_t *dBytes; uint64_t *dAddr, *dDst;
        rc = wk.dev(dBytes, nBytes + 16) || wk.dev(dAddr, n) || wk.dev(dDst, n + 1) ? -1 : 0;
        if (rc == 0) {
            for (uint64_t i = 0; i < n; i++) addr[i] = (uint64_t)(uintptr_t)(dBytes + offsets[i]);
            auto run = [&]() -> int {
                if (nBytes) DH_TRY(hipMemcpyAsync(dBytes, bytes, nBytes, hipMemcpyHostToDevice, st));
                if (n) DH_TRY(hipMemcpyAsync(dAddr, addr.data(), n * 8, hipMemcpyHostToDevice, st));
                DH_TRY(hipMemcpyAsync(dDst, dst.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
                DH_TRY(hipStreamSynchronize(st));
                return signalOnDevice(st, (uint32_t)std::max(1, prop.multiProcessorCount), dAddr, dDst, n, p, out);
            };
            rc = run();
        }
        (void)hipStreamSynchronize(st);
    }
    (void)hipStreamDestroy(st);
    return rc ? bad(rc) : 0;
}

int staramd_bamsort_finish_signal(staramd_bamsort *s, int level, int (*sink)(void *user, const uint8_t *bytes, uint64_t n), void *user, uint64_t stats[8],
                                  const staramd_signal_params *p, staramd_signal_result *out) {
    if (checkParams(p, out)) return -1;
    if (!s || !sink) { staramd_signal_free(out); return fail("no sorter, or no sink for its members"); }
    SorterJob job{p, out, false};
    bamsortSetAfterOrder(s, [](void *u, hipStream_t st, uint32_t cus, const uint64_t *dAddr, const uint64_t *dDst, uint64_t n) -> int {
        SorterJob *j = (SorterJob *)u;
        const int rc = signalOnDevice(st, cus, dAddr, dDst, n, j->p, j->out);
        if (rc) j->failed = true;
        return rc;
    }, &job);
    const int rc = staramd_bamsort_finish(s, level, sink, user, stats);
    if (rc) { if (!job.failed) g_err = staramd_bamsort_last_error(); staramd_signal_free(out); }
    return rc;
}

}  // extern "C"
