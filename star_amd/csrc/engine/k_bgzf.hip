// k_bgzf.hip -- BGZF compression of BAM record streams on the MI355X (include/star_amd_bgzf.h).  Self-contained: no engine.hip internals, its
// own error text, so that the wave emulator (oracle/wave_emul) can compile this file alone.
//
// One workgroup (256 work-items) compresses one BGZF block of at most 0xff00 input bytes into a complete gzip member in a 64 KiB slot:
//   stage      the block into LDS; CRC32 as per-lane partial CRCs over the lane's slice, joined by multiplication with x^(8 * bytes after it) mod P
//   candidates (level > 0) for every position the latest earlier position with the same 4-byte hash: the block is walked in chunks of 64 or 32
//              positions, each position reads the hash head of the chunks before its own, then the heads move on by atomicMax (order-independent)
//   parse      every lane parses its own slice of ceil(n / 256) bytes, matches kept inside the slice: greedy on the one candidate (levels 1-3) or the
//              longest of up to 4 candidates along the chain with one step of lazy evaluation (4-9, -1); tokens into the workgroup's global
//              scratch beside the candidates; literal/length and distance histograms by LDS atomicAdd
//   codes      Huffman code lengths (Moffat-Katajainen in place on the frequency-sorted symbols, one lane per tree; limited to 15 / 7 bits by
//              moving codes down until the Kraft sum is one), canonical codes, the run-length coded tree description
//   choose     the smallest of dynamic Huffman (BTYPE 2), fixed Huffman (BTYPE 1) and stored (BTYPE 0); stored always fits a slot
//   emit       exclusive scan of the lanes' token bit lengths, every lane ORs its bits into the zeroed LDS words of the stream
// Nothing that depends on the timing of lanes or workgroups decides a bit of the output: same input and level, same bytes (GPU and emulator).
// Then k_bgzf_scan (exclusive scan of the member sizes) and k_bgzf_compact (slots -> one contiguous output) make one device-to-host copy.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include <mutex>
#include <atomic>
#include <thread>
#include <chrono>
#include <algorithm>
#include "../../../include/star_amd_bgzf.h"
#include "bgzf_resident.h"
#include "crc32_gf2.h"                              // POLY, mulModP, xPow8: shared with k_inflate.hip

namespace {

constexpr uint32_t IN_MAX = 0xff00;                 // input bytes per BGZF block (bgzf.cpp, htslib's BGZF_BLOCK_SIZE)
constexpr uint32_t SLOT = 65536;                    // output bytes per block slot
constexpr uint32_t NT = 256;                        // work-items per workgroup
constexpr uint32_t HASH_BITS = 12;
constexpr uint32_t BUF_WORDS = IN_MAX / 4;          // the block's bytes, later its deflate stream (a Huffman form only when it fits here)
constexpr uint32_t AUX_WORDS = 1u << HASH_BITS;     // hash heads, later histograms / code tables / scan scratch

// aux layout once the candidates are found
constexpr uint32_t A_LITF = 0, A_DISTF = 288, A_SCAN = 320, A_LITP = 576, A_DISTP = 864, A_SYM_L = 896, A_FRQ_L = 1184, A_SYM_D = 1472,
                   A_FRQ_D = 1504, A_BLC_L = 1536, A_NXT_L = 1552, A_BLC_D = 1568, A_NXT_D = 1584, A_RLE = 1600, A_CLF = 1920, A_CLP = 1940,
                   A_SYM_C = 1960, A_FRQ_C = 1980, A_BLC_C = 2000, A_NXT_C = 2016, A_VAR = 2032;
enum { V_DYNBITS, V_FIXBITS, V_HDRBITS, V_HLIT, V_HDIST, V_HCLEN, V_NRLE, V_MD };

__device__ __forceinline__ uint32_t rev(uint32_t code, uint32_t len) { return __builtin_bitreverse32(code) >> (32 - len); }
__device__ __forceinline__ uint32_t log2u(uint32_t x) { return 31 - __clz((int)x); }
// length 3..258 -> symbol 257..285, extra bits, extra value
__device__ __forceinline__ uint32_t lenSym(uint32_t L, uint32_t &eb, uint32_t &ev) {
    if (L <= 10) { eb = 0; ev = 0; return 254 + L; }
    if (L == 258) { eb = 0; ev = 0; return 285; }         // no block gets here while a lane's slice is at most 255 bytes (0xff00 / 256): lengths stop at 255.
                                                        // Kept right for whoever raises the slice; covered at routine level (tests/test_bgzf_routines.py)
    uint32_t l = L - 3, e = log2u(l) - 2;
    eb = e; ev = l & ((1u << e) - 1);
    return 257 + 4 * (e + 1) + ((l >> e) & 3);
}
__device__ __forceinline__ uint32_t lenExtra(uint32_t s) { return (s < 265 || s == 285) ? 0 : (s - 261) / 4; }
// distance 1..32768 -> code 0..29, extra bits, extra value
__device__ __forceinline__ uint32_t distSym(uint32_t D, uint32_t &eb, uint32_t &ev) {
    uint32_t d = D - 1;
    if (d < 4) { eb = 0; ev = 0; return d; }
    uint32_t e = log2u(d) - 1;
    eb = e; ev = d & ((1u << e) - 1);
    return 2 * e + 2 + ((d >> e) & 1);
}
__device__ __forceinline__ uint32_t distExtra(uint32_t c) { return c < 4 ? 0 : (c - 2) / 2; }
__device__ __forceinline__ uint32_t fixedLitLen(uint32_t s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }
// order of the code-length code lengths in the block header (RFC 1951 3.2.7): 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, 5 bits each
__device__ __forceinline__ uint32_t clOrder(uint32_t i) {
    switch (i) {
        case 0: return 16; case 1: return 17; case 2: return 18; case 3: return 0; case 4: return 8; case 5: return 7; case 6: return 9;
        case 7: return 6; case 8: return 10; case 9: return 5; case 10: return 11; case 11: return 4; case 12: return 12; case 13: return 3;
        case 14: return 13; case 15: return 2; case 16: return 14; case 17: return 1; default: return 15;
    }
}

// LSB-first bit writer into LDS words that other lanes may share at the ends of its range (atomicOr into zeroed words)
struct BitW {
    uint32_t *out; uint64_t acc; uint32_t nb, w;
    __device__ void init(uint32_t *o, uint32_t bit) { out = o; acc = 0; nb = bit & 31; w = bit >> 5; }
    __device__ void put(uint32_t v, uint32_t n) {
        acc |= (uint64_t)v << nb; nb += n;
        if (nb >= 32) { atomicOr(&out[w], (uint32_t)acc); w++; acc >>= 32; nb -= 32; }
    }
    __device__ void flush() { if ((uint32_t)acc) atomicOr(&out[w], (uint32_t)acc); }
};

// Huffman code lengths of m >= 2 symbols, one work-item: frq[0..m) ascending frequencies of the symbols sym[0..m) (both LDS).  In-place
// minimum-redundancy code (Moffat & Katajainen 1995), then lengths above maxBits are folded down until the Kraft sum is one, then the lengths
// are handed out again, longest to the least frequent.  Writes len << 16 into pack[sym].
__device__ void huffLengths(uint32_t *A, const uint32_t *sym, uint32_t m, uint32_t maxBits, uint32_t *blc, uint32_t *pack) {
    uint32_t root = 0, leaf = 2;
    A[0] += A[1];
#pragma unroll 1
    for (uint32_t next = 1; next + 1 < m; next++) {
        if (leaf >= m || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = next; } else A[next] = A[leaf++];
        if (leaf >= m || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = next; } else A[next] += A[leaf++];
    }
    A[m - 2] = 0;
#pragma unroll 1
    for (int j = (int)m - 3; j >= 0; j--) A[j] = A[A[j]] + 1;
    int avbl = 1, used = 0, dpth = 0, r = (int)m - 2, nx = (int)m - 1;
    while (avbl > 0) {
        while (r >= 0 && (int)A[r] == dpth) { used++; r--; }
        while (avbl > used) { A[nx--] = (uint32_t)dpth; avbl--; }
        avbl = 2 * used; dpth++; used = 0;
    }
#pragma unroll 1
    for (uint32_t i = 0; i < 16; i++) blc[i] = 0;
#pragma unroll 1
    for (uint32_t i = 0; i < m; i++) blc[min(A[i], maxBits)]++;
    uint32_t total = 0;
#pragma unroll 1
    for (uint32_t i = 1; i <= maxBits; i++) total += blc[i] << (maxBits - i);
    while (total > (1u << maxBits)) {
        blc[maxBits]--;
#pragma unroll 1
        for (uint32_t i = maxBits - 1; i > 0; i--) if (blc[i]) { blc[i]--; blc[i + 1] += 2; break; }
        total--;
    }
    uint32_t i = 0;
#pragma unroll 1
    for (uint32_t len = maxBits; len >= 1; len--)
#pragma unroll 1
        for (uint32_t c = blc[len]; c > 0; c--) pack[sym[i++]] = len << 16;
}
// canonical codes from the lengths in pack[0..nsym) (len << 16): one work-item counts (blc, nxt), then every work-item codes its symbols
__device__ void canonCounts(const uint32_t *pack, uint32_t nsym, uint32_t *blc, uint32_t *nxt) {
#pragma unroll 1
    for (uint32_t i = 0; i < 16; i++) blc[i] = 0;
#pragma unroll 1
    for (uint32_t s = 0; s < nsym; s++) blc[pack[s] >> 16]++;
    uint32_t code = 0; blc[0] = 0;
#pragma unroll 1
    for (uint32_t b = 1; b < 16; b++) { code = (code + blc[b - 1]) << 1; nxt[b] = code; }
}
__device__ void canonCode(uint32_t *pack, uint32_t s, const uint32_t *nxt) {
    const uint32_t L = pack[s] >> 16;
    if (!L) return;
    uint32_t r = 0;
#pragma unroll 1
    for (uint32_t j = 0; j < s; j++) r += (pack[j] >> 16) == L;
    pack[s] = (L << 16) | rev(nxt[L] + r, L);
}
// ranks of the symbols with nonzero frequency by (frequency, symbol): the sorted order the length builder takes
__device__ void rankSym(const uint32_t *f, uint32_t nsym, uint32_t s, uint32_t *sym, uint32_t *frq) {
    const uint32_t fs = f[s];
    if (!fs) return;
    uint32_t r = 0;
#pragma unroll 1
    for (uint32_t j = 0; j < nsym; j++) { const uint32_t fj = f[j]; r += fj && (fj < fs || (fj == fs && j < s)); }
    sym[r] = s; frq[r] = fs;
}

__device__ uint32_t blockScanExcl(uint32_t v, uint32_t *s, uint32_t &total) {
    const uint32_t t = threadIdx.x;
    s[t] = v;
    __syncthreads();
#pragma unroll 1
    for (uint32_t off = 1; off < NT; off <<= 1) {
        const uint32_t x = t >= off ? s[t - off] : 0;
        __syncthreads();
        s[t] += x;
        __syncthreads();
    }
    const uint32_t incl = s[t];
    total = s[NT - 1];
    __syncthreads();
    return incl - v;
}

__device__ __forceinline__ uint32_t matchLen(const uint8_t *b, uint32_t q, uint32_t p, uint32_t maxL) {
    uint32_t L = 0;
    while (L < maxL && b[q + L] == b[p + L]) L++;
    return L;
}

// longest match of position p among its candidates: scr[p] holds (candidate + 1), the candidate's own candidate is the next one back, and so on --
// a hash chain whose links are at least a chunk long.  Up to `depth` of them within 32768, the nearest of the longest; q1 = (its position + 1)
__device__ __forceinline__ uint32_t bestMatch(const uint8_t *b, const uint32_t *scr, uint32_t p, uint32_t maxL, uint32_t depth, uint32_t &q1) {
    uint32_t L = 0, q = scr[p];
#pragma unroll 1
    for (uint32_t d = 0; d < depth && q && p - (q - 1) <= 32768; d++) {
        const uint32_t l = matchLen(b, q - 1, p, maxL);
        if (l > L) { L = l; q1 = q; if (l == maxL) break; }
        q = scr[q - 1];
    }
    return L;
}

__device__ void writeHeader(uint8_t *slot, uint32_t total) {
    uint32_t *w = (uint32_t *)slot;
    w[0] = 0x04088b1fu; w[1] = 0; w[2] = 0x0006ff00u; w[3] = 0x00024342u;       // ID1 ID2 CM FLG | MTIME | XFL OS XLEN | 'B' 'C' SLEN
    slot[16] = (uint8_t)((total - 1) & 0xff); slot[17] = (uint8_t)((total - 1) >> 8);
}
__device__ void writeTrailer(uint8_t *p, uint32_t crc, uint32_t n) {
#pragma unroll 1
    for (int i = 0; i < 4; i++) { p[i] = (uint8_t)(crc >> (8 * i)); p[4 + i] = (uint8_t)(n >> (8 * i)); }
}

}  // namespace

// grid-stride over the blocks; scratch: 2 * IN_MAX words per workgroup (the candidates, which every lane reads along its chains, and the tokens)
// level: 0 stored only; 1 candidates in chunks of 64 positions, greedy parse; 2-3 chunks of 32, greedy; 4-9 and -1 chunks of 32, the longest of up to
// 4 candidates along the chain, lazy parse
__global__ __launch_bounds__(256) void k_bgzf_blocks(const uint8_t *in, const uint64_t *blkOff, const uint32_t *blkLen, uint32_t nBlocks, int level,
                                                     uint32_t *scratchAll, uint8_t *slots, uint32_t *sizes) {
    __shared__ uint32_t buf[BUF_WORDS];
    __shared__ uint32_t aux[AUX_WORDS];
    uint8_t *lb = (uint8_t *)buf;
    const uint32_t tid = threadIdx.x;
    uint32_t *scr = scratchAll + (uint64_t)blockIdx.x * (2 * IN_MAX), *tok = scr + IN_MAX;
    uint32_t *V = aux + A_VAR;
    const bool lazy = level >= 4 || level < 0;
    const uint32_t DEPTH = lazy ? 4 : 1;
    const uint32_t CHUNK = level == 1 ? 64 : 32;            // positions that look up their candidates between two moves of the hash heads: a
                                                            // candidate is at least as far back as the chunk start, so smaller chunks find nearer matches
#pragma unroll 1
    for (uint32_t b = blockIdx.x; b < nBlocks; b += gridDim.x) {
        const uint32_t n = blkLen[b];
        const uint8_t *src = in + blkOff[b];
        uint8_t *slot = slots + (uint64_t)b * SLOT;
#pragma unroll 1
        for (uint32_t i = tid; i < n; i += NT) lb[i] = src[i];
        __syncthreads();
        // ---- CRC32
        const uint32_t S = (n + NT - 1) / NT, s0 = min(n, tid * S), s1 = min(n, s0 + S);
        uint32_t c = 0;
#pragma unroll 1
        for (uint32_t p = s0; p < s1; p++) { c ^= lb[p]; for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ POLY : c >> 1; }
        aux[tid] = c ? mulModP(c, xPow8(n - s1)) : 0;
        __syncthreads();
#pragma unroll 1
        for (uint32_t s = NT / 2; s > 0; s >>= 1) { if (tid < s) aux[tid] ^= aux[tid + s]; __syncthreads(); }
        const uint32_t crc = ~(aux[0] ^ mulModP(0xffffffffu, xPow8(n)));
        __syncthreads();
        bool stored = level == 0;
        if (!stored) {
            // ---- match candidates: hash heads hold (latest position of the chunks before) + 1
#pragma unroll 1
            for (uint32_t i = tid; i < AUX_WORDS; i += NT) aux[i] = 0;
            __syncthreads();
#pragma unroll 1
            for (uint32_t base = 0; base < n; base += CHUNK) {
                const uint32_t p = base + tid;
                uint32_t h = 0; const bool ok = tid < CHUNK && p + 4 <= n;
                if (ok) {
                    const uint32_t v = lb[p] | (uint32_t)lb[p + 1] << 8 | (uint32_t)lb[p + 2] << 16 | (uint32_t)lb[p + 3] << 24;
                    h = (v * 0x9E3779B1u) >> (32 - HASH_BITS);
                }
                if (tid < CHUNK && p < n) scr[p] = ok ? aux[h] : 0;
                __syncthreads();
                if (ok) atomicMax(&aux[h], p + 1);
                __syncthreads();
            }
#pragma unroll 1
            for (uint32_t i = tid; i < A_VAR + 16; i += NT) aux[i] = 0;
            __syncthreads();
            // ---- parse the lane's slice; tokens (literal: byte; match: len << 16 | dist) go to the second half of the scratch, from the slice start
            uint32_t k = 0;
#pragma unroll 1
            for (uint32_t p = s0; p < s1;) {
                uint32_t q = 0, q2 = 0;
                uint32_t L = bestMatch(lb, scr, p, min(258u, s1 - p), DEPTH, q);
                if (L >= 3 && lazy && L < 32 && p + 1 < s1 && bestMatch(lb, scr, p + 1, min(258u, s1 - p - 1), DEPTH, q2) > L) L = 0;
                if (L >= 3) {
                    const uint32_t D = p - (q - 1);
                    uint32_t eb, ev;
                    atomicAdd(&aux[A_LITF + lenSym(L, eb, ev)], 1u);
                    atomicAdd(&aux[A_DISTF + distSym(D, eb, ev)], 1u);
                    tok[s0 + k++] = L << 16 | D;
                    p += L;
                } else {
                    atomicAdd(&aux[A_LITF + lb[p]], 1u);
                    tok[s0 + k++] = lb[p];
                    p++;
                }
            }
            if (tid == 0) atomicAdd(&aux[A_LITF + 256], 1u);       // end of block
            __syncthreads();
            // ---- Huffman trees: distance code of at least two symbols (zlib's inflate takes complete codes only)
            if (tid == 0) {                                         // symbols 0 / 1 get frequency 1 for the tree (bit d of V_MD), 0 for the sizes
                uint32_t nz = 0, mask = 0;
#pragma unroll 1
                for (uint32_t d = 0; d < 30; d++) nz += aux[A_DISTF + d] != 0;
#pragma unroll 1
                for (uint32_t d = 0; d < 2 && nz < 2; d++) if (!aux[A_DISTF + d]) { aux[A_DISTF + d] = 1; mask |= 1u << d; nz++; }
                V[V_MD] = mask;
            }
#pragma unroll 1
            for (uint32_t i = tid; i < 288 + 32; i += NT) { if (i < 288) aux[A_LITP + i] = 0; else aux[A_DISTP + i - 288] = 0; }
            __syncthreads();
            const uint32_t dummyMask = V[V_MD];
            rankSym(aux + A_LITF, 286, tid, aux + A_SYM_L, aux + A_FRQ_L);
            if (tid + NT < 286) rankSym(aux + A_LITF, 286, tid + NT, aux + A_SYM_L, aux + A_FRQ_L);
            if (tid < 30) rankSym(aux + A_DISTF, 30, tid, aux + A_SYM_D, aux + A_FRQ_D);
            __syncthreads();
            if (tid == 0) {
                uint32_t m = 0; for (uint32_t s = 0; s < 286; s++) m += aux[A_LITF + s] != 0;
                huffLengths(aux + A_FRQ_L, aux + A_SYM_L, m, 15, aux + A_BLC_L, aux + A_LITP);
            }
            if (tid == 64) {
                uint32_t m = 0; for (uint32_t s = 0; s < 30; s++) m += aux[A_DISTF + s] != 0;
                huffLengths(aux + A_FRQ_D, aux + A_SYM_D, m, 15, aux + A_BLC_D, aux + A_DISTP);
            }
            __syncthreads();
            // ---- tree description: run-length coded code lengths, code-length code (one work-item)
            if (tid == 0) {
                uint32_t hlit = 286, hdist = 30;
                while (hlit > 257 && !(aux[A_LITP + hlit - 1] >> 16)) hlit--;
                while (hdist > 1 && !(aux[A_DISTP + hdist - 1] >> 16)) hdist--;
                uint32_t *clf = aux + A_CLF, *rle = aux + A_RLE, nr = 0;
#pragma unroll 1
                for (uint32_t i = 0; i < 19; i++) { clf[i] = 0; aux[A_CLP + i] = 0; }
                const uint32_t N = hlit + hdist;
#pragma unroll 1
                for (uint32_t i = 0; i < N;) {
                    const uint32_t v = i < hlit ? aux[A_LITP + i] >> 16 : aux[A_DISTP + i - hlit] >> 16;
                    uint32_t r = 1;
                    while (i + r < N && (i + r < hlit ? aux[A_LITP + i + r] >> 16 : aux[A_DISTP + i + r - hlit] >> 16) == v) r++;
                    i += r;
                    if (v == 0) {
                        while (r >= 11) { const uint32_t t = min(r, 138u); rle[nr++] = 18 | (t - 11) << 8; clf[18]++; r -= t; }
                        if (r >= 3) { rle[nr++] = 17 | (r - 3) << 8; clf[17]++; r = 0; }
                        while (r > 0) { rle[nr++] = 0; clf[0]++; r--; }
                    } else {
                        rle[nr++] = v; clf[v]++; r--;
                        while (r >= 3) { const uint32_t t = min(r, 6u); rle[nr++] = 16 | (t - 3) << 8; clf[16]++; r -= t; }
                        while (r > 0) { rle[nr++] = v; clf[v]++; r--; }
                    }
                }
                uint32_t nz = 0; for (uint32_t s = 0; s < 19; s++) nz += clf[s] != 0;
                if (nz < 2) { if (!clf[0]) clf[0] = 1; else clf[1] = 1; }        // (the header's size comes from rle[], not from these counts)
                uint32_t m = 0;
#pragma unroll 1
                for (uint32_t s = 0; s < 19; s++) if (clf[s]) {      // insertion sort by (frequency, symbol)
                    uint32_t j = m++;
                    while (j > 0 && aux[A_FRQ_C + j - 1] > clf[s]) { aux[A_FRQ_C + j] = aux[A_FRQ_C + j - 1]; aux[A_SYM_C + j] = aux[A_SYM_C + j - 1]; j--; }
                    aux[A_FRQ_C + j] = clf[s]; aux[A_SYM_C + j] = s;
                }
                huffLengths(aux + A_FRQ_C, aux + A_SYM_C, m, 7, aux + A_BLC_C, aux + A_CLP);
                canonCounts(aux + A_CLP, 19, aux + A_BLC_C, aux + A_NXT_C);
#pragma unroll 1
                for (uint32_t s = 0; s < 19; s++) canonCode(aux + A_CLP, s, aux + A_NXT_C);
                uint32_t hclen = 19;
                while (hclen > 4 && !(aux[A_CLP + clOrder(hclen - 1)] >> 16)) hclen--;
                uint32_t hb = 3 + 14 + 3 * hclen;
#pragma unroll 1
                for (uint32_t i = 0; i < nr; i++) { const uint32_t s = rle[i] & 0xff; hb += (aux[A_CLP + s] >> 16) + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0); }
                V[V_HLIT] = hlit; V[V_HDIST] = hdist; V[V_HCLEN] = hclen; V[V_NRLE] = nr; V[V_HDRBITS] = hb;
                V[V_DYNBITS] = hb; V[V_FIXBITS] = 3;
            }
            if (tid == 64) canonCounts(aux + A_DISTP, 30, aux + A_BLC_D, aux + A_NXT_D);
            if (tid == 128) canonCounts(aux + A_LITP, 286, aux + A_BLC_L, aux + A_NXT_L);
            __syncthreads();
            // ---- sizes of the two Huffman forms (dummy distance symbols are not counted: frequency 1 there, no token uses them)
            {
                uint32_t dyn = 0, fix = 0;
#pragma unroll 1
                for (uint32_t s = tid; s < 286; s += NT) {
                    const uint32_t f = aux[A_LITF + s], e = s > 256 ? lenExtra(s) : 0;
                    dyn += f * ((aux[A_LITP + s] >> 16) + e); fix += f * (fixedLitLen(s) + e);
                }
                if (tid < 30) {
                    const uint32_t f = ((dummyMask >> tid) & 1) ? 0 : aux[A_DISTF + tid], e = distExtra(tid);
                    dyn += f * ((aux[A_DISTP + tid] >> 16) + e); fix += f * (5 + e);
                }
                atomicAdd(&V[V_DYNBITS], dyn); atomicAdd(&V[V_FIXBITS], fix);
            }
            __syncthreads();
            const uint32_t dynBits = V[V_DYNBITS], fixBits = V[V_FIXBITS];
            const bool useDyn = dynBits <= fixBits;
            const uint32_t bits = useDyn ? dynBits : fixBits;
            stored = (bits + 7) / 8 >= n + 5 || bits > 32 * BUF_WORDS;   // stored: n + 5 bytes; a Huffman form when smaller and within the LDS buffer
            if (!stored) {
                if (!useDyn) {                                     // the fixed code is the canonical code of these lengths (RFC 1951 3.2.6)
#pragma unroll 1
                    for (uint32_t s = tid; s < 288 + 32; s += NT) { if (s < 288) aux[A_LITP + s] = fixedLitLen(s) << 16; else aux[A_DISTP + s - 288] = 5u << 16; }
                    __syncthreads();
                    if (tid == 0) canonCounts(aux + A_LITP, 288, aux + A_BLC_L, aux + A_NXT_L);
                    if (tid == 64) canonCounts(aux + A_DISTP, 30, aux + A_BLC_D, aux + A_NXT_D);
                    __syncthreads();
                }
#pragma unroll 1
                for (uint32_t s = tid; s < 288; s += NT) canonCode(aux + A_LITP, s, aux + A_NXT_L);
                if (tid < 30) canonCode(aux + A_DISTP, tid, aux + A_NXT_D);
                __syncthreads();
                // ---- bits of the lane's tokens, their offsets
                uint32_t mine = 0;
#pragma unroll 1
                for (uint32_t i = 0; i < k; i++) {
                    const uint32_t t = tok[s0 + i];
                    if (t < 256) { mine += aux[A_LITP + t] >> 16; continue; }
                    uint32_t eb, ev, eb2, ev2;
                    const uint32_t ls = lenSym(t >> 16, eb, ev), ds = distSym(t & 0xffff, eb2, ev2);
                    mine += (aux[A_LITP + ls] >> 16) + eb + (aux[A_DISTP + ds] >> 16) + eb2;
                }
                uint32_t tokTotal;
                const uint32_t hdr = useDyn ? V[V_HDRBITS] : 3;
                const uint32_t at = blockScanExcl(mine, aux + A_SCAN, tokTotal);
#pragma unroll 1
                for (uint32_t i = tid; i < BUF_WORDS; i += NT) buf[i] = 0;
                __syncthreads();
                BitW bw;
                if (tid == 0) {
                    bw.init(buf, 0);
                    bw.put(1, 1); bw.put(useDyn ? 2 : 1, 2);
                    if (useDyn) {
                        bw.put(V[V_HLIT] - 257, 5); bw.put(V[V_HDIST] - 1, 5); bw.put(V[V_HCLEN] - 4, 4);
#pragma unroll 1
                        for (uint32_t i = 0; i < V[V_HCLEN]; i++) bw.put(aux[A_CLP + clOrder(i)] >> 16, 3);
#pragma unroll 1
                        for (uint32_t i = 0; i < V[V_NRLE]; i++) {
                            const uint32_t r = aux[A_RLE + i], s = r & 0xff, cp = aux[A_CLP + s];
                            bw.put(cp & 0xffff, cp >> 16);
                            if (s == 16) bw.put(r >> 8, 2); else if (s == 17) bw.put(r >> 8, 3); else if (s == 18) bw.put(r >> 8, 7);
                        }
                    }
                    bw.flush();
                }
                bw.init(buf, hdr + at);
#pragma unroll 1
                for (uint32_t i = 0; i < k; i++) {
                    const uint32_t t = tok[s0 + i];
                    if (t < 256) { const uint32_t cp = aux[A_LITP + t]; bw.put(cp & 0xffff, cp >> 16); continue; }
                    uint32_t eb, ev, eb2, ev2;
                    const uint32_t ls = lenSym(t >> 16, eb, ev), ds = distSym(t & 0xffff, eb2, ev2);
                    const uint32_t cl = aux[A_LITP + ls], cd = aux[A_DISTP + ds];
                    bw.put(cl & 0xffff, cl >> 16); if (eb) bw.put(ev, eb);
                    bw.put(cd & 0xffff, cd >> 16); if (eb2) bw.put(ev2, eb2);
                }
                bw.flush();
                if (tid == NT - 1) { const uint32_t cp = aux[A_LITP + 256]; bw.init(buf, hdr + tokTotal); bw.put(cp & 0xffff, cp >> 16); bw.flush(); }
                __syncthreads();
                const uint32_t D = (hdr + tokTotal + (aux[A_LITP + 256] >> 16) + 7) / 8;
#pragma unroll 1
                for (uint32_t i = tid; i < D; i += NT) slot[18 + i] = lb[i];
                if (tid == 0) { writeHeader(slot, D + 26); writeTrailer(slot + 18 + D, crc, n); sizes[b] = D + 26; }
            }
        }
        if (stored) {
#pragma unroll 1
            for (uint32_t i = tid; i < n; i += NT) slot[23 + i] = lb[i];
            if (tid == 0) {
                writeHeader(slot, n + 31);
                slot[18] = 1; slot[19] = (uint8_t)n; slot[20] = (uint8_t)(n >> 8); slot[21] = (uint8_t)~n; slot[22] = (uint8_t)(~n >> 8);
                writeTrailer(slot + 23 + n, crc, n);
                sizes[b] = n + 31;
            }
        }
        __syncthreads();
    }
}

// off[i] = sum of sizes[0..i), off[n] = total: one workgroup, every work-item a contiguous run of blocks
__global__ __launch_bounds__(256) void k_bgzf_scan(const uint32_t *sizes, uint32_t n, uint64_t *off) {
    __shared__ uint64_t s[NT];
    const uint32_t t = threadIdx.x, per = (n + NT - 1) / NT, lo = min(n, t * per), hi = min(n, lo + per);
    uint64_t sum = 0;
#pragma unroll 1
    for (uint32_t i = lo; i < hi; i++) sum += sizes[i];
    s[t] = sum;
    __syncthreads();
#pragma unroll 1
    for (uint32_t d = 1; d < NT; d <<= 1) {
        const uint64_t x = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += x;
        __syncthreads();
    }
    uint64_t at = s[t] - sum;
#pragma unroll 1
    for (uint32_t i = lo; i < hi; i++) { off[i] = at; at += sizes[i]; }
    if (t == NT - 1) off[n] = s[NT - 1];
}

__global__ __launch_bounds__(256) void k_bgzf_compact(const uint8_t *slots, const uint32_t *sizes, const uint64_t *off, uint32_t n, uint8_t *out) {
#pragma unroll 1
    for (uint32_t b = blockIdx.x; b < n; b += gridDim.x) {
        const uint8_t *src = slots + (uint64_t)b * SLOT;
        uint8_t *dst = out + off[b];
        const uint32_t sz = sizes[b];
#pragma unroll 1
        for (uint32_t i = threadIdx.x; i < sz; i += NT) dst[i] = src[i];
    }
}

// ---- C ABI --------------------------------------------------------------------------------------------------------------------------------
#define DEV_HOST_PREFIX "BGZF compression on the device: "
#include "dev_host.h"

struct staramd_bgzf {
    int device = 0; hipStream_t st = nullptr; hipEvent_t ev[4] = {};
    uint32_t grid = 1;
    std::mutex mu;
    GrowBuf in, out;        // the segments of a call side by side, and their members
    uint8_t *dSlots = nullptr; uint32_t *dSizes = nullptr, *dBlkLen = nullptr; uint64_t *dOff = nullptr, *dBlkOff = nullptr, *hOff = nullptr; uint64_t capBlk = 0;
    uint32_t *dScratch = nullptr;
};

namespace {
int growBlk(staramd_bgzf *z, uint64_t nb) {
    if (nb <= z->capBlk) return 0;
    nb = std::max<uint64_t>(nb + nb / 4, 64);
    (void)hipFree(z->dSlots); (void)hipFree(z->dSizes); (void)hipFree(z->dBlkLen); (void)hipFree(z->dOff); (void)hipFree(z->dBlkOff); if (z->hOff) (void)hipHostFree(z->hOff);
    z->dSlots = nullptr; z->dSizes = z->dBlkLen = nullptr; z->dOff = z->dBlkOff = z->hOff = nullptr; z->capBlk = 0;
    DH_TRY(hipMalloc((void **)&z->dSlots, nb * SLOT));
    DH_TRY(hipMalloc((void **)&z->dSizes, nb * 4));
    DH_TRY(hipMalloc((void **)&z->dBlkLen, nb * 4));
    DH_TRY(hipMalloc((void **)&z->dBlkOff, nb * 8));
    DH_TRY(hipMalloc((void **)&z->dOff, (nb + 1) * 8));
    DH_TRY(hipHostMalloc((void **)&z->hOff, (nb + 1) * 8, 0));
    z->capBlk = nb;
    return 0;
}
// the three kernels of one call, on the compressor's stream: the one statement of their launch (staramd_bgzf_compress and bgzfCompressResident)
int launchKernels(staramd_bgzf *z, const uint8_t *dIn, const uint64_t *dBlkOff, const uint32_t *dBlkLen, uint32_t nb, int level, uint8_t *dOut, uint64_t *dOff) {
    const uint32_t grid = std::min(nb, z->grid);
    DH_LAUNCH(k_bgzf_blocks, dim3(grid), z->st, dIn, dBlkOff, dBlkLen, nb, level, z->dScratch, z->dSlots, z->dSizes);
    DH_LAUNCH(k_bgzf_scan, dim3(1), z->st, z->dSizes, nb, dOff);
    DH_LAUNCH(k_bgzf_compact, dim3(std::min(nb, 4096u)), z->st, z->dSlots, z->dSizes, dOff, nb, dOut);
    return 0;
}
}  // namespace

// ---- input resident on the device (bgzf_resident.h) ------------------------------------------------------------------------------------------
void bgzfResidentInfo(staramd_bgzf *z, int *device, hipStream_t *stream, uint32_t *grid) { *device = z->device; *stream = z->st; *grid = z->grid; }
void bgzfResidentLock(staramd_bgzf *z) { z->mu.lock(); }
void bgzfResidentUnlock(staramd_bgzf *z) { z->mu.unlock(); }
int bgzfResidentReserve(staramd_bgzf *z, uint64_t nb) {
    DH_TRY(hipSetDevice(z->device));
    return growBlk(z, nb);
}
int bgzfCompressResident(staramd_bgzf *z, const uint8_t *dIn, const uint64_t *dBlkOff, const uint32_t *dBlkLen, uint32_t nb, int level, uint8_t *dOut, uint64_t *dOff) {
    if (checkLevel(level)) return -1;
    if (nb == 0 || nb > z->capBlk) return fail("bgzfCompressResident: " + std::to_string(nb) + " blocks, room reserved for " + std::to_string(z->capBlk));
    return launchKernels(z, dIn, dBlkOff, dBlkLen, nb, level, dOut, dOff);
}

extern "C" {

const char *staramd_bgzf_last_error(void) { return g_err.c_str(); }

uint64_t staramd_bgzf_bound(uint64_t n) { return n + 31 * ((n + IN_MAX - 1) / IN_MAX); }

int staramd_bgzf_create(staramd_bgzf **out, int device, uint64_t initialInputBytes) {
    *out = nullptr;
    staramd_bgzf *z = new staramd_bgzf();
    z->device = device;
    auto bad = [&](int rc) { staramd_bgzf_destroy(z); return rc; };
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return bad(failHip("hipSetDevice", e));
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return bad(failHip("hipGetDeviceProperties", e));
    z->grid = (uint32_t)std::max(1, 2 * prop.multiProcessorCount);          // two 80 KiB workgroups per CU
    if ((e = hipStreamCreate(&z->st)) != hipSuccess) return bad(failHip("hipStreamCreate", e));
    for (auto &x : z->ev) if ((e = hipEventCreate(&x)) != hipSuccess) return bad(failHip("hipEventCreate", e));
    if ((e = hipMalloc((void **)&z->dScratch, (uint64_t)z->grid * IN_MAX * 8)) != hipSuccess) return bad(failHip("hipMalloc", e));
    if (initialInputBytes) {
        const uint64_t nb = (initialInputBytes + IN_MAX - 1) / IN_MAX;
        if (z->in.grow(initialInputBytes) || z->out.grow(staramd_bgzf_bound(initialInputBytes)) || growBlk(z, nb)) return bad(-1);
    }
    *out = z;
    return 0;
}

void staramd_bgzf_destroy(staramd_bgzf *z) {
    if (!z) return;
    (void)hipSetDevice(z->device);
    if (z->st) (void)hipStreamSynchronize(z->st);
    z->in.release(); z->out.release();
    (void)hipFree(z->dSlots); (void)hipFree(z->dSizes); (void)hipFree(z->dBlkLen); (void)hipFree(z->dBlkOff); (void)hipFree(z->dOff); (void)hipFree(z->dScratch);
    if (z->hOff) (void)hipHostFree(z->hOff);
    for (auto &x : z->ev) if (x) (void)hipEventDestroy(x);
    if (z->st) (void)hipStreamDestroy(z->st);
    delete z;
}

int staramd_bgzf_compress(void *zv, int level, uint32_t nSeg, const uint8_t *const *in, const uint64_t *inLen, uint8_t *out, uint64_t outCap, uint64_t *outLen) {
    staramd_bgzf *z = (staramd_bgzf *)zv;
    if (!z) return fail("no compressor");
    if (checkLevel(level)) return -1;
    std::lock_guard<std::mutex> lock(z->mu);
    typedef std::chrono::steady_clock Clock;
    const auto t0 = Clock::now();
    uint64_t total = 0, bound = 0, nb = 0;
    for (uint32_t s = 0; s < nSeg; s++) { total += inLen[s]; bound += staramd_bgzf_bound(inLen[s]); nb += (inLen[s] + IN_MAX - 1) / IN_MAX; }
    if (bound > outCap) return fail("output buffer of " + std::to_string(outCap) + " bytes, " + std::to_string(bound) + " may be needed");
    if (nb == 0) { for (uint32_t s = 0; s < nSeg; s++) outLen[s] = 0; return 0; }
    if (nb > 0xffffffffull) return fail("too many blocks in one call");
    DH_TRY(hipSetDevice(z->device));
    if (z->in.grow(total) || z->out.grow(bound) || growBlk(z, nb)) return -1;
    std::vector<uint64_t> blkOff(nb); std::vector<uint32_t> blkLen(nb);
    std::vector<Piece> ps;
    uint64_t at = 0, ib = 0;
    for (uint32_t s = 0; s < nSeg; s++) {
        ps.push_back({z->in.h + at, in[s], inLen[s]});
        for (uint64_t o = 0; o < inLen[s]; o += IN_MAX) { blkOff[ib] = at + o; blkLen[ib] = (uint32_t)std::min<uint64_t>(IN_MAX, inLen[s] - o); ib++; }
        at += inLen[s];
    }
    copyPieces(ps, total);
    const auto t1 = Clock::now();
    DH_TRY(hipEventRecord(z->ev[0], z->st));
    DH_TRY(hipMemcpyAsync(z->in.d, z->in.h, total, hipMemcpyHostToDevice, z->st));
    DH_TRY(hipMemcpyAsync(z->dBlkOff, blkOff.data(), nb * 8, hipMemcpyHostToDevice, z->st));
    DH_TRY(hipMemcpyAsync(z->dBlkLen, blkLen.data(), nb * 4, hipMemcpyHostToDevice, z->st));
    DH_TRY(hipEventRecord(z->ev[1], z->st));
    if (launchKernels(z, z->in.d, z->dBlkOff, z->dBlkLen, (uint32_t)nb, level, z->out.d, z->dOff)) return -1;
    DH_TRY(hipMemcpyAsync(z->hOff, z->dOff, (nb + 1) * 8, hipMemcpyDeviceToHost, z->st));
    DH_TRY(hipEventRecord(z->ev[2], z->st));
    DH_TRY(hipStreamSynchronize(z->st));
    const uint64_t outTotal = z->hOff[nb];
    if (outTotal > bound) return fail("device output larger than its bound");
    DH_TRY(hipMemcpyAsync(z->out.h, z->out.d, outTotal, hipMemcpyDeviceToHost, z->st));
    DH_TRY(hipEventRecord(z->ev[3], z->st));
    DH_TRY(hipStreamSynchronize(z->st));
    const auto t2 = Clock::now();
    copyPieces({{out, z->out.h, outTotal}}, outTotal);
    ib = 0;
    for (uint32_t s = 0; s < nSeg; s++) {
        const uint64_t k = (inLen[s] + IN_MAX - 1) / IN_MAX;
        outLen[s] = z->hOff[ib + k] - z->hOff[ib];
        ib += k;
    }
    static const bool timing = getenv("STARAMD_HOST_TIMING") != nullptr;
    if (timing) {
        float h2d = 0, ker = 0, d2h = 0;
        (void)hipEventElapsedTime(&h2d, z->ev[0], z->ev[1]); (void)hipEventElapsedTime(&ker, z->ev[1], z->ev[2]); (void)hipEventElapsedTime(&d2h, z->ev[2], z->ev[3]);
        const double ms = 1e3;
        fprintf(stderr, "  bgzf device: %u segments, %llu blocks, %.1f -> %.1f MB: staging copy %.2f ms, H2D %.2f ms, kernels %.2f ms, D2H %.2f ms, copy out %.2f ms\n",
                nSeg, (unsigned long long)nb, total / 1e6, outTotal / 1e6, std::chrono::duration<double>(t1 - t0).count() * ms, h2d, ker, d2h,
                std::chrono::duration<double>(Clock::now() - t2).count() * ms);
    }
    return 0;
}

}  // extern "C"
