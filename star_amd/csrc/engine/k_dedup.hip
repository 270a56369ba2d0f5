// k_dedup.hip -- duplicate read pairs of a coordinate-sorted BAM marked on the MI355X (include/star_amd_dedup.h; the rule: DESIGN.md 7.6, read through
// ../dedup_rule.h, which host/dedup.cpp shares).  Self-contained beside k_bgzf.hip, k_bamsort.hip and k_signal.hip, so that the wave emulator can compile it alone.
//
//   scan      k_dedup_scan: one lane per record.  Core fields, NH and AS from one attribute walk; kind (unique / multi / untouched) and the bit the record ends
//             with unless a class decides otherwise; startS; 64-bit hashes of the name and of (cigarS, bases).  A scan of the unique flags compacts them
//   pairing   rocprim::radix_sort_pairs by name hash, then by tid: STABLE.  k_dedup_name_heads compares neighbours ON THE NAME BYTES; where two different
//             names share a key the array is merge-sorted by (tid, hash, name) first.  A run of exactly one mate 1 and one mate 2 is a pair (k_dedup_pair_flags)
//   classes   per pair the numeric key tid | startS1 and startS2 | flag1 | flag2 and a content hash; radix passes by hash, low word, high word; k_dedup_class_heads
//             compares neighbours ON THE CONTENT (both cigarS, the bases); the same merge sort where contents collide; a scan numbers the classes
//   survivor  rocprim::inclusive_scan with a segmented operator over (AS of mate 1, then the smaller name): the last pair of a class holds its survivor;
//             k_dedup_mark writes the bytes
// No loop of a lane runs over a class or over the pairs of a position: the merge sort is a binary search per element and level, the survivor a scan.
// One item per work-item in grid-stride loops; NT, the workgroups per CU and the 64 / 32 key bits of the passes are choices, not measured optima.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <rocprim/rocprim.hpp>
#include <string>
#include <vector>
#include <algorithm>
#include "../../../include/star_amd_dedup.h"
#include "../dedup_rule.h"

namespace {

constexpr uint32_t NT = 256;                        // work-items per workgroup
constexpr uint32_t WG_PER_CU = 16;                  // a grid is capped at this many workgroups per CU
constexpr uint64_t TOP = 1ull << 63;
enum : uint8_t { K_UNIQUE = 1, K_MULTI = 2, K_HAS_AS = 16, K_MATE2 = 32 };

// record i = addr[i], dst[i + 1] - dst[i] bytes
struct Recs {
    const uint64_t *addr, *dst;
    __host__ __device__ const uint8_t *at(uint64_t i) const { return (const uint8_t *)addr[i]; }
    __host__ __device__ uint64_t len(uint64_t i) const { return dst[i + 1] - dst[i]; }
};
struct PerRecord { uint8_t *kind, *dup; uint32_t *tid, *startS, *flag; int32_t *as; uint64_t *hN, *hC; };

// order of unique records (values: record numbers): tid, name hash, name
struct NameLess {
    Recs R; const uint32_t *tid; const uint64_t *hN;
    __host__ __device__ int names(uint64_t a, uint64_t b) const { return dedupNameCmp(R.at(a), dedupCore(R.at(a), R.len(a)), R.at(b), dedupCore(R.at(b), R.len(b))); }
    __host__ __device__ bool operator()(uint64_t a, uint64_t b) const {
        if (tid[a] != tid[b]) return tid[a] < tid[b];
        if (hN[a] != hN[b]) return hN[a] < hN[b];
        return names(a, b) < 0;
    }
};
// order of pairs (values: pair numbers): high word, low word, content hash, content
struct ClassLess {
    Recs R; const uint64_t *K2, *K1, *K0, *M1, *M2; uint32_t N;
    __host__ __device__ int content(uint64_t a, uint64_t b) const {
        return dedupContentCmp(R.at(M1[a]), R.len(M1[a]), R.at(M2[a]), R.len(M2[a]), R.at(M1[b]), R.len(M1[b]), R.at(M2[b]), R.len(M2[b]), N);
    }
    __host__ __device__ bool operator()(uint64_t a, uint64_t b) const {
        if (K2[a] != K2[b]) return K2[a] < K2[b];
        if (K1[a] != K1[b]) return K1[a] < K1[b];
        if (K0[a] != K0[b]) return K0[a] < K0[b];
        return content(a, b) < 0;
    }
};
// the survivor so far of a class: elements are head flag << 63 | pair number; a head starts over
struct Survivor {
    Recs R; const int32_t *pas; const uint64_t *M1;
    __host__ __device__ uint64_t operator()(uint64_t a, uint64_t b) const {
        if (b & TOP) return b;
        const uint64_t pa = a & ~TOP, pb = b & ~TOP;
        bool second = pas[pb] > pas[pa];
        if (pas[pb] == pas[pa]) { const uint64_t ra = M1[pa], rb = M1[pb]; second = dedupNameCmp(R.at(rb), dedupCore(R.at(rb), R.len(rb)), R.at(ra), dedupCore(R.at(ra), R.len(ra))) < 0; }
        return (a & TOP) | (second ? pb : pa);
    }
};

}  // namespace

// uflag[i] = 1 for a unique record (uflag[n] = 0: the scan leaves their number there); fatal[0] = the lowest record without NH
__global__ __launch_bounds__(256) void k_dedup_scan(Recs R, uint64_t n, int markMulti, uint32_t N, uint64_t hashMask, PerRecord O, uint64_t *__restrict__ uflag, unsigned long long *__restrict__ fatal) {
    for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * NT) {
        if (i == n) { uflag[i] = 0; continue; }
        const uint8_t *rec = R.at(i);
        const DedupCore c = dedupCore(rec, R.len(i));
        uint32_t nh = 0, as = 0;
        const uint32_t got = c.ok ? bamAuxInts(rec, c.lim, dedupAuxStart(c), 'N', 'H', nh, true, 'A', 'S', as) : 0;
        uint8_t k = 0, d = (uint8_t)(c.flag >> 10 & 1);
        if (!(got & 1)) atomicMin(&fatal[0], (unsigned long long)i);
        else if ((int32_t)nh == 1) { k = K_UNIQUE; d = 0; }
        else if ((int32_t)nh > 1) { k = K_MULTI; if (markMulti) d = 1; }
        if (got & 2) k |= K_HAS_AS;
        if (c.flag & 0x80) k |= K_MATE2;
        O.kind[i] = k; O.dup[i] = d; O.tid[i] = c.tid; O.startS[i] = c.ok ? dedupStartS(rec, c) : 0; O.flag[i] = c.flag; O.as[i] = (int32_t)as;
        const bool u = (k & K_UNIQUE) != 0;
        O.hN[i] = u ? dedupNameHash(rec, c) & hashMask : 0;
        O.hC[i] = u ? dedupContentHash(rec, c, N) : 0;
        uflag[i] = u;
    }
}
// the unique records, in the records' order, with their first sort key
__global__ __launch_bounds__(256) void k_dedup_compact(const uint64_t *__restrict__ uoff, uint64_t n, const uint64_t *__restrict__ hN, uint64_t *__restrict__ U, uint64_t *__restrict__ key) {
    for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * NT) {
        const uint64_t o = uoff[i];
        if (uoff[i + 1] != o) { U[o] = i; key[o] = hN[i]; }
    }
}
// the key of the next radix pass, in the order the values have now
template <class T> __global__ __launch_bounds__(256) void k_dedup_gather(const T *__restrict__ src, const uint64_t *__restrict__ idx, uint64_t n, uint64_t *__restrict__ out) {
    for (uint64_t j = (uint64_t)blockIdx.x * NT + threadIdx.x; j < n; j += (uint64_t)gridDim.x * NT) out[j] = src[idx[j]];
}
// One level of a stable merge sort: blocks of w sorted values each, merged two by two.  An element's place is its rank in its own block plus the number of
// elements of the sibling block that go before it (a binary search; equal elements of the left block go first)
template <class Less> __global__ __launch_bounds__(256) void k_dedup_merge_pass(const uint64_t *__restrict__ in, uint64_t *__restrict__ out, uint64_t n, uint64_t w, Less less) {
    for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * NT) {
        const uint64_t base = i / (2 * w) * (2 * w), mid = min(base + w, n), end = min(base + 2 * w, n), x = in[i];
        const bool left = i < mid;
        uint64_t lo = left ? mid : base, hi = left ? end : mid;
        const uint64_t from = lo;
#pragma unroll 1
        while (lo < hi) {
            const uint64_t m = lo + (hi - lo) / 2, y = in[m];
            const bool before = left ? less(y, x) : !less(x, y);        // y goes before x
            if (before) lo = m + 1; else hi = m;
        }
        out[base + (i - (left ? base : mid)) + (lo - from)] = x;
    }
}
// head[j] = 1 where a (tid, name) begins in the sorted unique records; *dirty = 1 when two different names share (tid, hash): then the order is not exact yet
__global__ __launch_bounds__(256) void k_dedup_name_heads(NameLess L, const uint64_t *__restrict__ U, uint64_t nU, uint8_t *__restrict__ head, uint32_t *__restrict__ dirty) {
    for (uint64_t j = (uint64_t)blockIdx.x * NT + threadIdx.x; j <= nU; j += (uint64_t)gridDim.x * NT) {
        if (j == nU) { head[j] = 1; continue; }                         // (a sentinel: a run ends where the array ends)
        if (j == 0) { head[j] = 1; continue; }
        const uint64_t a = U[j - 1], b = U[j];
        const bool sameTid = L.tid[a] == L.tid[b], same = sameTid && L.names(a, b) == 0;
        head[j] = !same;
        if (sameTid && !same && L.hN[a] == L.hN[b]) *dirty = 1;
    }
}
// pflag[j] = 1 where a pair begins: a run of exactly two records, one of them mate 2 (pflag[nU] = 0)
__global__ __launch_bounds__(256) void k_dedup_pair_flags(const uint64_t *__restrict__ U, uint64_t nU, const uint8_t *__restrict__ head, const uint8_t *__restrict__ kind, uint64_t *__restrict__ pflag) {
    for (uint64_t j = (uint64_t)blockIdx.x * NT + threadIdx.x; j <= nU; j += (uint64_t)gridDim.x * NT) {
        uint64_t f = 0;
        if (j + 1 < nU && head[j] && !head[j + 1] && head[j + 2]) f = ((kind[U[j]] ^ kind[U[j + 1]]) & K_MATE2) != 0;
        pflag[j] = f;
    }
}
struct PairOut { uint64_t *M1, *M2, *K0, *K1, *K2, *V; int32_t *pas; };
// pair p = the scanned flag: its records, its keys, the AS of mate 1; fatal[1] = the lowest mate 1 of a pair without AS
__global__ __launch_bounds__(256) void k_dedup_pairs(const uint64_t *__restrict__ U, uint64_t nU, const uint64_t *__restrict__ poff, PerRecord O, uint64_t hashMask, PairOut Q, unsigned long long *__restrict__ fatal) {
    for (uint64_t j = (uint64_t)blockIdx.x * NT + threadIdx.x; j < nU; j += (uint64_t)gridDim.x * NT) {
        const uint64_t p = poff[j];
        if (poff[j + 1] == p) continue;
        const uint64_t a = U[j], b = U[j + 1], m1 = (O.kind[a] & K_MATE2) ? b : a, m2 = (O.kind[a] & K_MATE2) ? a : b;
        Q.M1[p] = m1; Q.M2[p] = m2; Q.V[p] = p; Q.pas[p] = O.as[m1];
        Q.K0[p] = dedupMix(O.hC[m1], O.hC[m2]) & hashMask;
        Q.K1[p] = dedupKeyLo(O.startS[m2], O.flag[m1], O.flag[m2]);
        Q.K2[p] = dedupKeyHi(O.tid[m1], O.startS[m1]);
        if (!(O.kind[m1] & K_HAS_AS)) atomicMin(&fatal[1], (unsigned long long)m1);
    }
}
// head[j] = 1 where a class begins in the sorted pairs (head[nP] = 0: the scan leaves the number of classes there); *dirty as above, for contents under one hash
__global__ __launch_bounds__(256) void k_dedup_class_heads(ClassLess L, const uint64_t *__restrict__ V, uint64_t nP, uint64_t *__restrict__ head, uint32_t *__restrict__ dirty) {
    for (uint64_t j = (uint64_t)blockIdx.x * NT + threadIdx.x; j <= nP; j += (uint64_t)gridDim.x * NT) {
        if (j == nP) { head[j] = 0; continue; }
        if (j == 0) { head[j] = 1; continue; }
        const uint64_t a = V[j - 1], b = V[j];
        const bool sameNum = L.K2[a] == L.K2[b] && L.K1[a] == L.K1[b], same = sameNum && L.content(a, b) == 0;
        head[j] = !same;
        if (sameNum && !same && L.K0[a] == L.K0[b]) *dirty = 1;
    }
}
__global__ __launch_bounds__(256) void k_dedup_survivor_input(const uint64_t *__restrict__ V, const uint64_t *__restrict__ head, uint64_t nP, uint64_t *__restrict__ E) {
    for (uint64_t j = (uint64_t)blockIdx.x * NT + threadIdx.x; j < nP; j += (uint64_t)gridDim.x * NT) E[j] = (head[j] ? TOP : 0) | V[j];
}
// cls = the exclusive scan of the head flags: pair j is of class cls[j + 1] - 1, and the last of it when the next is a head.  W[class] = its survivor
__global__ __launch_bounds__(256) void k_dedup_winners(const uint64_t *__restrict__ E, const uint64_t *__restrict__ cls, uint64_t nP, uint64_t *__restrict__ W) {
    for (uint64_t j = (uint64_t)blockIdx.x * NT + threadIdx.x; j < nP; j += (uint64_t)gridDim.x * NT)
        if (j + 1 == nP || cls[j + 2] != cls[j + 1]) W[cls[j + 1] - 1] = E[j] & ~TOP;
}
__global__ __launch_bounds__(256) void k_dedup_mark(const uint64_t *__restrict__ V, const uint64_t *__restrict__ cls, const uint64_t *__restrict__ W, const uint64_t *__restrict__ M1, const uint64_t *__restrict__ M2,
                                                    uint64_t nP, uint8_t *__restrict__ dup) {
    for (uint64_t j = (uint64_t)blockIdx.x * NT + threadIdx.x; j < nP; j += (uint64_t)gridDim.x * NT) {
        const uint64_t p = V[j];
        const uint8_t d = W[cls[j + 1] - 1] != p;
        dup[M1[p]] = d; dup[M2[p]] = d;
    }
}

// ---- C ABI --------------------------------------------------------------------------------------------------------------------------------
#define DEV_HOST_PREFIX "duplicate marking on the device: "
#define DEV_HOST_ROCPRIM
#include "dev_host.h"

namespace {
uint32_t envU32(const char *name, uint32_t dflt) { const char *e = getenv(name); return e && *e ? (uint32_t)strtoul(e, nullptr, 10) : dflt; }

struct Geometry {
    uint32_t maxWg;
    uint32_t grid(uint64_t items) const { return (uint32_t)std::min<uint64_t>((items + NT) / NT, maxWg); }
};

template <class Op> int inclusiveScanOp(PrimSpace &prim, hipStream_t st, uint64_t *v, size_t n, Op op) {      // in place
    size_t need = 0;
    DH_TRY(rocprim::inclusive_scan(nullptr, need, v, v, n, op, st));
    if (prim.room(need)) return -1;
    DH_TRY(rocprim::inclusive_scan(prim.tmp, need, v, v, n, op, st));
    return 0;
}
// a, alt: the values and a second array of n; afterwards a names the sorted one
template <class Less> int mergeSort(hipStream_t st, const Geometry &g, uint64_t *&a, uint64_t *&alt, uint64_t n, Less less) {
    for (uint64_t w = 1; w < n; w *= 2) {
        DH_LAUNCH(k_dedup_merge_pass<Less>, dim3(g.grid(n)), st, (const uint64_t *)a, alt, n, w, less);
        std::swap(a, alt);
    }
    return 0;
}
// one stable radix pass of the values by src[value]
template <class T> int passBy(PrimSpace &prim, hipStream_t st, const Geometry &g, const T *src, uint64_t *&key, uint64_t *&keyAlt, uint64_t *&val, uint64_t *&valAlt, uint64_t n, uint32_t bits) {
    if (bits == 0) return 0;
    DH_LAUNCH(k_dedup_gather<T>, dim3(g.grid(n)), st, src, (const uint64_t *)val, n, key);
    return prim.sortPairs(st, key, keyAlt, val, valAlt, n, bits);
}

// dDup: n bytes of the caller's, the final bits when the call returns 0 with out->fatal == 0; msStage: milliseconds of scan, pairing, classes, survivor
int dedupOnDevice(hipStream_t st, uint32_t cus, Recs R, uint64_t n, const staramd_dedup_params *p, uint8_t *dDup, staramd_dedup_result *out, float msStage[4]) {
    const uint32_t hashBits = std::min<uint32_t>(64, envU32("STARAMD_DEDUP_HASH_BITS", 64));
    const uint64_t hashMask = hashBits >= 64 ? ~0ull : (1ull << hashBits) - 1;
    const uint32_t wgEnv = envU32("STARAMD_DEDUP_MAX_WORKGROUPS", 0);
    const Geometry g{wgEnv ? wgEnv : WG_PER_CU * cus};
    const uint32_t N = p->mate2basesN;
    Work wk; PrimSpace prim;
    hipEvent_t ev[5];
    for (auto &e : ev) if (wk.event(e)) return -1;
    // ---- scan
    PerRecord O; O.dup = dDup; uint64_t *dUflag; unsigned long long *dFatal; uint32_t *dDirty;
    if (wk.dev(O.kind, n) || wk.dev(O.tid, n) || wk.dev(O.startS, n) || wk.dev(O.flag, n) || wk.dev(O.as, n) || wk.dev(O.hN, n) || wk.dev(O.hC, n) ||
        wk.dev(dUflag, n + 1) || wk.dev(dFatal, 2) || wk.dev(dDirty, 2)) return -1;
    DH_TRY(hipMemsetAsync(dFatal, 0xff, 16, st));
    DH_TRY(hipMemsetAsync(dDirty, 0, 8, st));
    DH_TRY(hipEventRecord(ev[0], st));
    DH_LAUNCH(k_dedup_scan, dim3(g.grid(n)), st, R, n, p->markMulti ? 1 : 0, N, hashMask, O, dUflag, dFatal);
    if (prim.exclusiveScan(st, dUflag, n + 1)) return -1;
    uint64_t nU = 0, nP = 0, nClasses = 0; unsigned long long fatal[2] = {~0ull, ~0ull}; uint32_t dirty[2] = {0, 0};
    // the counts below are copied into these variables on the stream: no way out of this function, an error's included, leaves such a copy in flight
    struct SyncOnExit { hipStream_t st; ~SyncOnExit() { (void)hipStreamSynchronize(st); } } syncOnExit{st};
    DH_TRY(hipMemcpyAsync(&nU, dUflag + n, 8, hipMemcpyDeviceToHost, st));
    DH_TRY(hipMemcpyAsync(fatal, dFatal, 8, hipMemcpyDeviceToHost, st));
    DH_TRY(hipEventRecord(ev[1], st));
    DH_TRY(hipStreamSynchronize(st));
    out->stats[1] = nU;
    if (fatal[0] != ~0ull) { out->fatal = 1; out->fatalRecord = fatal[0]; return 0; }
    auto stageTimes = [&](int upTo) { for (int i = 0; i < upTo; i++) (void)hipEventElapsedTime(&msStage[i], ev[i], ev[i + 1]); };
    if (nU == 0) { stageTimes(1); return 0; }
    // ---- pairing
    uint64_t *dU, *dUalt, *dKey, *dKeyAlt, *dPflag; uint8_t *dHead;
    if (wk.dev(dU, nU) || wk.dev(dUalt, nU) || wk.dev(dKey, nU) || wk.dev(dKeyAlt, nU) || wk.dev(dPflag, nU + 1) || wk.dev(dHead, nU + 1)) return -1;
    DH_LAUNCH(k_dedup_compact, dim3(g.grid(n)), st, (const uint64_t *)dUflag, n, (const uint64_t *)O.hN, dU, dKey);
    if (hashBits && prim.sortPairs(st, dKey, dKeyAlt, dU, dUalt, nU, hashBits)) return -1;
    if (passBy(prim, st, g, (const uint32_t *)O.tid, dKey, dKeyAlt, dU, dUalt, nU, 32)) return -1;
    const NameLess nameLess{R, O.tid, O.hN};
    DH_LAUNCH(k_dedup_name_heads, dim3(g.grid(nU)), st, nameLess, (const uint64_t *)dU, nU, dHead, dDirty);
    DH_TRY(hipMemcpyAsync(dirty, dDirty, 4, hipMemcpyDeviceToHost, st));
    DH_TRY(hipStreamSynchronize(st));
    if (dirty[0]) {                                                 // two names under one key: exact order first, then the heads again
        if (mergeSort(st, g, dU, dUalt, nU, nameLess)) return -1;
        DH_LAUNCH(k_dedup_name_heads, dim3(g.grid(nU)), st, nameLess, (const uint64_t *)dU, nU, dHead, dDirty);
    }
    DH_LAUNCH(k_dedup_pair_flags, dim3(g.grid(nU)), st, (const uint64_t *)dU, nU, (const uint8_t *)dHead, (const uint8_t *)O.kind, dPflag);
    if (prim.exclusiveScan(st, dPflag, nU + 1)) return -1;
    DH_TRY(hipMemcpyAsync(&nP, dPflag + nU, 8, hipMemcpyDeviceToHost, st));
    DH_TRY(hipEventRecord(ev[2], st));
    DH_TRY(hipStreamSynchronize(st));
    out->stats[2] = nP; out->stats[5] = nU - 2 * nP;
    if (nP == 0) { stageTimes(2); return 0; }
    // ---- classes
    PairOut Q; uint64_t *dValt, *dHeadC, *dE, *dW;
    if (wk.dev(Q.M1, nP) || wk.dev(Q.M2, nP) || wk.dev(Q.K0, nP) || wk.dev(Q.K1, nP) || wk.dev(Q.K2, nP) || wk.dev(Q.V, nP) || wk.dev(Q.pas, nP) ||
        wk.dev(dValt, nP) || wk.dev(dHeadC, nP + 1) || wk.dev(dE, nP) || wk.dev(dW, nP)) return -1;
    DH_LAUNCH(k_dedup_pairs, dim3(g.grid(nU)), st, (const uint64_t *)dU, nU, (const uint64_t *)dPflag, O, hashMask, Q, dFatal);
    uint64_t *dV = Q.V;                                             // the keys of the passes go through dKey / dKeyAlt: nP <= nU
    if (passBy(prim, st, g, (const uint64_t *)Q.K0, dKey, dKeyAlt, dV, dValt, nP, hashBits) || passBy(prim, st, g, (const uint64_t *)Q.K1, dKey, dKeyAlt, dV, dValt, nP, 64) ||
        passBy(prim, st, g, (const uint64_t *)Q.K2, dKey, dKeyAlt, dV, dValt, nP, 64)) return -1;
    const ClassLess classLess{R, Q.K2, Q.K1, Q.K0, Q.M1, Q.M2, N};
    DH_LAUNCH(k_dedup_class_heads, dim3(g.grid(nP)), st, classLess, (const uint64_t *)dV, nP, dHeadC, dDirty + 1);
    DH_TRY(hipMemcpyAsync(dirty + 1, dDirty + 1, 4, hipMemcpyDeviceToHost, st));
    DH_TRY(hipMemcpyAsync(fatal + 1, dFatal + 1, 8, hipMemcpyDeviceToHost, st));
    DH_TRY(hipStreamSynchronize(st));
    if (fatal[1] != ~0ull) { out->fatal = 2; out->fatalRecord = fatal[1]; return 0; }
    if (dirty[1]) {
        if (mergeSort(st, g, dV, dValt, nP, classLess)) return -1;
        DH_LAUNCH(k_dedup_class_heads, dim3(g.grid(nP)), st, classLess, (const uint64_t *)dV, nP, dHeadC, dDirty + 1);
    }
    DH_TRY(hipEventRecord(ev[3], st));
    // ---- survivor
    DH_LAUNCH(k_dedup_survivor_input, dim3(g.grid(nP)), st, (const uint64_t *)dV, (const uint64_t *)dHeadC, nP, dE);
    if (inclusiveScanOp(prim, st, dE, nP, Survivor{R, Q.pas, Q.M1})) return -1;
    if (prim.exclusiveScan(st, dHeadC, nP + 1)) return -1;
    DH_TRY(hipMemcpyAsync(&nClasses, dHeadC + nP, 8, hipMemcpyDeviceToHost, st));
    DH_LAUNCH(k_dedup_winners, dim3(g.grid(nP)), st, (const uint64_t *)dE, (const uint64_t *)dHeadC, nP, dW);
    DH_LAUNCH(k_dedup_mark, dim3(g.grid(nP)), st, (const uint64_t *)dV, (const uint64_t *)dHeadC, (const uint64_t *)dW, (const uint64_t *)Q.M1, (const uint64_t *)Q.M2, nP, O.dup);
    DH_TRY(hipEventRecord(ev[4], st));
    DH_TRY(hipStreamSynchronize(st));
    out->stats[3] = nClasses;
    stageTimes(4);
    return 0;
}
}  // namespace

extern "C" {

const char *staramd_dedup_last_error(void) { return g_err.c_str(); }
uint32_t staramd_dedup_constant(int which) { return which == 0 ? NT : which == 1 ? WG_PER_CU : which == 2 ? envU32("STARAMD_DEDUP_MAX_WORKGROUPS", 0) : 0; }

void staramd_dedup_free(staramd_dedup_result *r) {
    if (!r) return;
    free(r->dup);
    memset(r, 0, sizeof(*r));
}

int staramd_dedup_host_records(int device, const staramd_dedup_params *p, const uint8_t *bytes, uint64_t nBytes, const uint64_t *offsets, uint64_t n, staramd_dedup_result *out) {
    if (!p || !out) return fail("no parameters or no result");
    memset(out, 0, sizeof(*out));
    if (n && (!bytes || !offsets)) return fail("no records");
    std::vector<uint64_t> addr(n), dst(n + 1);
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; i++) {
        uint32_t bs = 0;
        if (offsets[i] > nBytes || nBytes - offsets[i] < 4) return fail("record " + std::to_string(i) + " lies outside the " + std::to_string(nBytes) + " bytes");
        memcpy(&bs, bytes + offsets[i], 4);
        if (nBytes - offsets[i] - 4 < bs) return fail("record " + std::to_string(i) + " lies outside the " + std::to_string(nBytes) + " bytes");
        dst[i] = total; total += 4 + (uint64_t)bs;
    }
    dst[n] = total;
    out->nRecords = n; out->stats[0] = n;
    if (n == 0) return 0;
    out->dup = (uint8_t *)malloc(n);
    if (!out->dup) return fail("no host memory for the result");
    auto bad = [&](int rc) { staramd_dedup_free(out); return rc; };
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return bad(failHip("hipSetDevice", e));
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return bad(failHip("hipGetDeviceProperties", e));
    hipStream_t st = nullptr;
    if ((e = hipStreamCreate(&st)) != hipSuccess) return bad(failHip("hipStreamCreate", e));
    int rc = 0;
    {   Work wk;
        uint8_t *dBytes, *dDup; uint64_t *dAddr, *dDst;
        hipEvent_t ev[4];
        rc = wk.dev(dBytes, nBytes + 16) || wk.dev(dAddr, n) || wk.dev(dDst, n + 1) || wk.dev(dDup, n) || wk.event(ev[0]) || wk.event(ev[1]) || wk.event(ev[2]) || wk.event(ev[3]) ? -1 : 0;
        if (rc == 0) {
            for (uint64_t i = 0; i < n; i++) addr[i] = (uint64_t)(uintptr_t)(dBytes + offsets[i]);
            auto run = [&]() -> int {
                float msStage[4] = {0, 0, 0, 0}, msUp = 0, msAll = 0, msDown = 0;
                DH_TRY(hipEventRecord(ev[0], st));
                DH_TRY(hipMemcpyAsync(dBytes, bytes, nBytes, hipMemcpyHostToDevice, st));
                DH_TRY(hipMemcpyAsync(dAddr, addr.data(), n * 8, hipMemcpyHostToDevice, st));
                DH_TRY(hipMemcpyAsync(dDst, dst.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
                DH_TRY(hipEventRecord(ev[1], st));
                DH_TRY(hipStreamSynchronize(st));
                if (dedupOnDevice(st, (uint32_t)std::max(1, prop.multiProcessorCount), Recs{dAddr, dDst}, n, p, dDup, out, msStage)) return -1;
                DH_TRY(hipEventRecord(ev[2], st));
                if (!out->fatal) DH_TRY(hipMemcpyAsync(out->dup, dDup, n, hipMemcpyDeviceToHost, st));
                DH_TRY(hipEventRecord(ev[3], st));
                DH_TRY(hipStreamSynchronize(st));
                (void)hipEventElapsedTime(&msUp, ev[0], ev[1]); (void)hipEventElapsedTime(&msAll, ev[1], ev[2]); (void)hipEventElapsedTime(&msDown, ev[2], ev[3]);
                out->stats[6] = (uint64_t)(msAll * 1e6); out->stats[7] = (uint64_t)((msUp + msDown) * 1e6);
                if (!out->fatal) { uint64_t marked = 0; for (uint64_t i = 0; i < n; i++) marked += out->dup[i]; out->stats[4] = marked; }
                static const bool timing = getenv("STARAMD_HOST_TIMING") != nullptr;
                if (timing)
                    fprintf(stderr, "  dedup device: %llu records, %llu unique, %llu pairs, %llu classes: upload %.2f ms, scan %.2f ms, pairing %.2f ms, classes %.2f ms, survivor %.2f ms, D2H %.2f ms\n",
                            (unsigned long long)n, (unsigned long long)out->stats[1], (unsigned long long)out->stats[2], (unsigned long long)out->stats[3], msUp, msStage[0], msStage[1], msStage[2], msStage[3], msDown);
                return 0;
            };
            rc = run();
        }
        (void)hipStreamSynchronize(st);
    }
    (void)hipStreamDestroy(st);
    return rc ? bad(rc) : 0;
}

}  // extern "C"
