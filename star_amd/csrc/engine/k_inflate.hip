// k_inflate.hip -- a BGZF file inflated on the MI355X (include/star_amd_inflate.h; --runMode inputAlignmentsFromBAM --gpuBAMinflate Device).  Self-contained
// beside k_bgzf.hip, k_bamsort.hip, k_signal.hip and k_dedup.hip, so that the wave emulator can compile it alone.
//
// One wavefront inflates one member (a gzip member of at most 64 KiB out), in a grid-stride loop over the member table the host made from the headers.
//   state    the bit reader, the output position and every decoded symbol are the same in all 64 lanes (wave-uniform): every lane decodes every symbol
//   tables   per wavefront in LDS: the code lengths, per tree the count of codes per length, the symbols in canonical order and a table indexed by the next
//            FAST bits for the codes that short (longer ones walk the counts, at most 15 steps); built by the lanes side by side
//   output   straight to global memory: the literal at position p by lane p % 64, byte j of a match by lane j % 64 from out[p - dist + j % dist]
//   check    CRC-32 of the output as per-lane partial CRCs joined by the GF(2) multiply (crc32_gf2.h, shared with k_bgzf.hip), against the trailer
// A match reads bytes that other lanes of the wavefront stored.  The memory pipeline serves the loads and stores of one wavefront in the order of its
// instructions, so the bytes are there; LOCKSTEP() marks each such place (a compiler fence of wavefront scope here, a rendezvous in the emulator).
//
// Malformed input is ordinary input.  No read leaves the member's csize bytes (a bit past the end reads as 0 and, once consumed, ends the decode with a
// status); no write leaves its isize bytes of output; every trip of a loop whose count depends on the data consumes at least one input bit or produces
// at least one output byte -- the trips are counted, and end after at most 8 * csize + isize (tests/inflate_bounds_check.cpp).  The loops that build
// tables are bounded by constants (320 symbols, 15 lengths, 512 entries).  No printf, no assert.
// NT, the workgroups per CU and FAST are choices, not measured optima.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <string>
#include <vector>
#include <algorithm>
#include "../../../include/star_amd_inflate.h"
#include "crc32_gf2.h"

#ifndef LOCKSTEP
#ifdef STARAMD_WAVE_EMUL
#define LOCKSTEP() emu_wave_sync()
#else
#define LOCKSTEP() __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront")
#endif
#endif

namespace {

constexpr uint32_t NT = 256;                        // work-items per workgroup
constexpr uint32_t WAVES = NT / 64;                 // members a workgroup inflates side by side
constexpr uint32_t WG_PER_CU = 8;                   // a grid is capped at this many workgroups per CU
constexpr uint32_t FAST_L = 9, FAST_D = 7;          // bits of the direct tables (literal/length; distance and the code-length code)
constexpr uint32_t MAX_ISIZE = 65536;               // BGZF: a member's output
constexpr uint32_t NO_SYMBOL = 0xffffu;

struct Member { uint64_t in, out; uint32_t csize, isize, crc, pad; };        // the deflate stream file[in .. in + csize), its output out[out .. out + isize)

// a canonical Huffman code as the decoder wants it: cnt[l] codes of length l, the first of them `first[l]`, their symbols sym[off[l] ..) in symbol order;
// fast[next bits] = symbol << 4 | length for the codes of at most `bits` bits, 0 elsewhere
struct Huff { uint16_t *fast, *sym, *cnt, *first, *off; uint32_t bits; };
struct WaveTables {
    uint16_t fastL[1u << FAST_L], fastD[1u << FAST_D], symL[288], symD[32], cntL[16], cntD[16], firstL[16], firstD[16], offL[16], offD[16];
    uint8_t lens[320], clLens[32];                  // literal/length lengths, then the distance lengths; the code-length code's own lengths
    __device__ Huff lit() { return Huff{fastL, symL, cntL, firstL, offL, FAST_L}; }
    __device__ Huff dist() { return Huff{fastD, symD, cntD, firstD, offD, FAST_D}; }       // (the code-length code borrows these while a header is read)
};

// LSB-first reader of in[0 .. csize): `nb` bits wait in acc, idx bytes were taken (bytes past the end as 0)
struct Bits {
    const uint8_t *in; uint32_t csize, idx, nb; uint64_t acc;
    __device__ void refill() {                      // at least 57 bits afterwards
#pragma unroll 1
        while (nb <= 56) { const uint64_t b = idx < csize ? in[idx] : 0; acc |= b << nb; nb += 8; idx++; }
    }
    __device__ uint32_t take(uint32_t n) { const uint32_t v = (uint32_t)(acc & ((1ull << n) - 1)); acc >>= n; nb -= n; return v; }      // n <= 32
    __device__ bool over() const { return (uint64_t)idx * 8 - nb > (uint64_t)csize * 8; }      // a bit past the end was consumed
    __device__ uint32_t bytesUsed() const { return (uint32_t)(((uint64_t)idx * 8 - nb + 7) / 8); }
};

__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint32_t fixedLen(uint32_t s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5; }      // 288..319: the distance code
__device__ __forceinline__ uint32_t codeLenOrder(uint32_t i) {            // RFC 1951 3.2.7
    return i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 7 - (i - 5) / 2 : 8 + (i - 4) / 2;
}

enum { KIND_CODES, KIND_LENS, KIND_DISTS };
// the tables of n code lengths (all lanes call it, with the lengths visible): 0 or a status, the same in every lane
__device__ uint32_t buildHuff(Huff H, const uint8_t *lens, uint32_t n, int kind, uint32_t lane) {
    LOCKSTEP();                                     // every lane is done with the tables these replace
    if (lane < 16) {
        uint32_t c = 0;
#pragma unroll 1
        for (uint32_t s = 0; s < n; s++) c += lens[s] == lane;
        H.cnt[lane] = (uint16_t)c;
    }
#pragma unroll 1
    for (uint32_t i = lane; i < (1u << H.bits); i += 64) H.fast[i] = 0;
    LOCKSTEP();
    int left = 1; uint32_t code = 0, off = 0;
#pragma unroll 1
    for (uint32_t l = 1; l <= 15; l++) {
        const uint32_t c = H.cnt[l];
        left = (left << 1) - (int)c;
        if (left < 0) return STARAMD_INFLATE_OVERSUBSCRIBED;
        if (lane == 0) { H.first[l] = (uint16_t)code; H.off[l] = (uint16_t)off; }
        code = (code + c) << 1; off += c;
    }
    // (zlib's inflate_table: an incomplete set is legal only as no code at all, or one code of one bit, and never for the code-length code)
    if (left > 0 && (kind == KIND_CODES || !(off == 0 || (off == 1 && H.cnt[1] == 1)))) return STARAMD_INFLATE_INCOMPLETE;
    LOCKSTEP();
#pragma unroll 1
    for (uint32_t s = lane; s < n; s += 64) {
        const uint32_t l = lens[s];
        if (!l) continue;
        uint32_t rank = 0;
#pragma unroll 1
        for (uint32_t j = 0; j < s; j++) rank += lens[j] == l;
        H.sym[H.off[l] + rank] = (uint16_t)s;
        if (l <= H.bits) {
            const uint32_t r = __builtin_bitreverse32(H.first[l] + rank) >> (32 - l);
#pragma unroll 1
            for (uint32_t i = r; i < (1u << H.bits); i += 1u << l) H.fast[i] = (uint16_t)(s << 4 | l);
        }
    }
    LOCKSTEP();
    return 0;
}

// the next symbol (its bits taken), or NO_SYMBOL when the next bits are no code (nothing taken).  At least 15 bits wait in the reader
__device__ uint32_t decodeSym(const Huff &H, Bits &B) {
    const uint32_t peek = (uint32_t)B.acc;
    uint32_t e = H.fast[peek & ((1u << H.bits) - 1)];
    if (!(e & 15)) {
        e = NO_SYMBOL << 4;
        int code = 0, first = 0, index = 0;
#pragma unroll 1
        for (uint32_t l = 1; l <= 15; l++) {
            code |= (int)((peek >> (l - 1)) & 1);
            const int c = H.cnt[l];
            if (code - c < first) { e = (uint32_t)H.sym[index + (code - first)] << 4 | l; break; }
            index += c; first += c; first <<= 1; code <<= 1;
        }
    }
    e = uniform(e);
    if (e >> 4 == NO_SYMBOL) return NO_SYMBOL;
    B.take(e & 15);
    return e >> 4;
}

// one member by one wavefront.  status: 0 or STARAMD_INFLATE_*; trips: the turns of the data-dependent loops
__device__ void inflateMember(const uint8_t *in, uint32_t csize, uint8_t *out, uint32_t isize, uint32_t crcWant, WaveTables &T, uint32_t lane, uint32_t &status, uint32_t &trips) {
    Bits B{in, csize, 0, 0, 0};
    uint32_t pos = 0, st = 0, t = 0;
    bool last = false;
#pragma unroll 1
    while (!st && !last) {
        B.refill();
        last = B.take(1) != 0;
        const uint32_t type = B.take(2);
        if (B.over()) { st = STARAMD_INFLATE_INPUT_END; break; }
        t++;                                        // (a trip is counted once the bits it took are known to be the member's own)
        if (type == 3) { st = STARAMD_INFLATE_BLOCK_TYPE; break; }
        if (type == 0) {                            // stored: to the byte boundary, LEN, NLEN, the bytes
            B.take(B.nb & 7);
            const uint32_t h = B.take(32), len = h & 0xffff;
            if (B.over()) { st = STARAMD_INFLATE_INPUT_END; break; }
            if ((len ^ 0xffff) != h >> 16) { st = STARAMD_INFLATE_STORED_LEN; break; }
            const uint32_t p = B.idx - B.nb / 8;
            if (p + len > csize) { st = STARAMD_INFLATE_INPUT_END; break; }
            if (pos + len > isize) { st = STARAMD_INFLATE_OUTPUT_OVER; break; }
#pragma unroll 1
            for (uint32_t j = lane; j < len; j += 64) out[pos + j] = in[p + j];
            pos += len;
            B.idx = p + len; B.nb = 0; B.acc = 0;
            continue;
        }
        uint32_t hlit = 288, hdist = 32;
        LOCKSTEP();                                 // every lane is done with the lengths of the block before
        if (type == 1) {
#pragma unroll 1
            for (uint32_t s = lane; s < 320; s += 64) T.lens[s] = (uint8_t)fixedLen(s);
        } else {
            hlit = B.take(5) + 257; hdist = B.take(5) + 1;
            const uint32_t hclen = B.take(4) + 4;
            if (B.over()) { st = STARAMD_INFLATE_INPUT_END; break; }
            if (hlit > 286 || hdist > 30) { st = STARAMD_INFLATE_TOO_MANY; break; }
#pragma unroll 1
            for (uint32_t i = 0; i < 19; i++) {
                uint32_t v = 0;
                if (i < hclen) {
                    B.refill(); v = B.take(3);
                    if (B.over()) { st = STARAMD_INFLATE_INPUT_END; break; }
                    t++;
                }
                if (lane == 0) T.clLens[codeLenOrder(i)] = (uint8_t)v;
            }
            if (st) break;
            const Huff C = T.dist();
            if ((st = buildHuff(C, T.clLens, 19, KIND_CODES, lane))) break;
            const uint32_t total = hlit + hdist;
            uint32_t n = 0, prev = 0;
#pragma unroll 1
            while (n < total) {
                B.refill();
                const uint32_t s = decodeSym(C, B);
                if (s == NO_SYMBOL) { st = STARAMD_INFLATE_SYMBOL; break; }
                uint32_t rep = 1, val = s;
                if (s == 16) { if (n == 0) { st = STARAMD_INFLATE_REPEAT; break; } val = prev; rep = 3 + B.take(2); }
                else if (s == 17) { val = 0; rep = 3 + B.take(3); }
                else if (s == 18) { val = 0; rep = 11 + B.take(7); }
                if (B.over()) { st = STARAMD_INFLATE_INPUT_END; break; }
                t++;
                if (n + rep > total) { st = STARAMD_INFLATE_REPEAT; break; }
#pragma unroll 1
                for (uint32_t j = lane; j < rep; j += 64) T.lens[n + j] = (uint8_t)val;
                n += rep; prev = val;
            }
            if (st) break;
        }
        LOCKSTEP();                                 // the lengths are written
        if (T.lens[256] == 0) { st = STARAMD_INFLATE_NO_END_CODE; break; }
        const Huff L = T.lit(), D = T.dist();
        if ((st = buildHuff(L, T.lens, hlit, KIND_LENS, lane))) break;
        if ((st = buildHuff(D, T.lens + hlit, hdist, KIND_DISTS, lane))) break;
#pragma unroll 1
        for (;;) {
            B.refill();                             // 57 bits: a length code, its 5 extra bits, a distance code and its 13 are at most 48
            const uint32_t s = decodeSym(L, B);
            if (s == NO_SYMBOL || s >= 286) { st = B.over() ? STARAMD_INFLATE_INPUT_END : STARAMD_INFLATE_SYMBOL; break; }
            if (B.over()) { st = STARAMD_INFLATE_INPUT_END; break; }
            t++;
            if (s < 256) {
                if (pos >= isize) { st = STARAMD_INFLATE_OUTPUT_OVER; break; }
                if (lane == (pos & 63)) out[pos] = (uint8_t)s;
                pos++;
                continue;
            }
            if (s == 256) break;
            uint32_t len;
            if (s < 265) len = s - 254;
            else if (s == 285) len = 258;
            else { const uint32_t e = (s - 261) >> 2; len = ((4 + ((s - 265) & 3)) << e) + 3 + B.take(e); }
            const uint32_t ds = decodeSym(D, B);
            if (ds == NO_SYMBOL || ds >= 30) { st = B.over() ? STARAMD_INFLATE_INPUT_END : STARAMD_INFLATE_SYMBOL; break; }
            uint32_t dist;
            if (ds < 4) dist = ds + 1;
            else { const uint32_t e = (ds >> 1) - 1; dist = ((2 + (ds & 1)) << e) + 1 + B.take(e); }
            if (B.over()) { st = STARAMD_INFLATE_INPUT_END; break; }
            if (dist > pos) { st = STARAMD_INFLATE_DISTANCE; break; }
            if (pos + len > isize) { st = STARAMD_INFLATE_OUTPUT_OVER; break; }
            LOCKSTEP();                             // the source bytes, out[pos - dist .. pos), were stored by other lanes
            const uint8_t *src = out + (pos - dist);
            if (dist >= len) {
#pragma unroll 1
                for (uint32_t j = lane; j < len; j += 64) out[pos + j] = src[j];
            } else {
#pragma unroll 1
                for (uint32_t j = lane; j < len; j += 64) out[pos + j] = src[j % dist];
            }
            pos += len;
        }
    }
    if (!st && pos != isize) st = STARAMD_INFLATE_OUTPUT_SHORT;
    if (!st && B.bytesUsed() != csize) st = STARAMD_INFLATE_STREAM_END;
    if (!st) {
        LOCKSTEP();                                 // the output is read back, every lane a slice of it
        const uint32_t S = (isize + 63) / 64, s0 = min(isize, lane * S), s1 = min(isize, s0 + S);
        uint32_t c = 0;
#pragma unroll 1
        for (uint32_t p = s0; p < s1; p++) { c ^= out[p]; for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ POLY : c >> 1; }
        uint32_t x = c ? mulModP(c, xPow8(isize - s1)) : 0;
#pragma unroll 1
        for (int m = 32; m > 0; m >>= 1) x ^= (uint32_t)__shfl_xor((int)x, m, 64);
        if (uniform(~(x ^ mulModP(0xffffffffu, xPow8(isize)))) != crcWant) st = STARAMD_INFLATE_CRC;
    }
    status = st; trips = t;
}

}  // namespace

// grid-stride over the members, one per wavefront; trips may be null
__global__ __launch_bounds__(256) void k_inflate_members(const uint8_t *__restrict__ file, const Member *__restrict__ tab, uint32_t nMembers, uint8_t *out, uint32_t *__restrict__ status,
                                                         uint32_t *__restrict__ trips) {
    __shared__ WaveTables T[WAVES];
    const uint32_t wave = uniform(threadIdx.x >> 6), lane = threadIdx.x & 63;
#pragma unroll 1
    for (uint32_t m = blockIdx.x * WAVES + wave; m < nMembers; m += gridDim.x * WAVES) {
        const Member mb = tab[m];
        uint32_t st = 0, t = 0;
        inflateMember(file + mb.in, mb.csize, out + mb.out, mb.isize, mb.crc, T[wave], lane, st, t);
        if (lane == 0) { status[m] = st; if (trips) trips[m] = t; }
    }
}

// ---- C ABI --------------------------------------------------------------------------------------------------------------------------------
#define DEV_HOST_PREFIX "BGZF inflation on the device: "
#include "dev_host.h"

namespace {
uint32_t envU32(const char *name, uint32_t dflt) { const char *e = getenv(name); return e && *e ? (uint32_t)strtoul(e, nullptr, 10) : dflt; }
inline uint32_t rd16(const uint8_t *p) { return p[0] | (uint32_t)p[1] << 8; }
inline uint32_t rd32(const uint8_t *p) { return rd16(p) | rd16(p + 2) << 16; }
int notBgzf(uint64_t member, const std::string &why) {
    return fail("member " + std::to_string(member) + " " + why + ": the file is gzip but not BGZF.  SOLUTION: --gpuBAMinflate Host");
}

// The member table of a file: a chain of BSIZE hops.  0; -1 with the error text; or 1 when member tab.size() is cut short or reaches past the file
int walkMembers(const uint8_t *f, uint64_t n, std::vector<Member> &tab, uint64_t &total, uint64_t &nEmpty) {
    uint64_t p = 0;
    total = 0; nEmpty = 0;
    while (p < n) {
        const uint64_t k = tab.size(), left = n - p;
        if (left < 2 || f[p] != 0x1f || f[p + 1] != 0x8b) {
            if (k == 0) return fail("the file does not begin with a gzip member.  SOLUTION: --gpuBAMinflate Host");
            break;                                  // bytes that are no gzip member behind the last one: gzread ignores them
        }
        if (left < 12) return 1;
        if (f[p + 2] != 8) return notBgzf(k, "is not compressed by deflate");
        if ((f[p + 3] & 0x1e) != 0x04) return notBgzf(k, "has no extra field, or a name, a comment or a header CRC");
        const uint32_t xlen = rd16(f + p + 10);
        if (left < 12ull + xlen) return 1;
        uint64_t bsize = 0; bool found = false;
        for (uint32_t x = 0; x + 4 <= xlen;) {
            const uint8_t *sf = f + p + 12 + x;
            const uint32_t slen = rd16(sf + 2);
            if (sf[0] == 'B' && sf[1] == 'C' && slen == 2 && x + 6 <= xlen) { bsize = rd16(sf + 4); found = true; break; }
            x += 4 + slen;
        }
        if (!found) return notBgzf(k, "has no BC subfield");
        const uint64_t size = bsize + 1, hdr = 12ull + xlen;
        if (size > left || size < hdr + 8) return 1;
        Member m;
        m.in = p + hdr; m.csize = (uint32_t)(size - hdr - 8); m.crc = rd32(f + p + size - 8); m.isize = rd32(f + p + size - 4); m.out = total; m.pad = 0;
        if (m.isize > MAX_ISIZE) return notBgzf(k, "declares " + std::to_string(m.isize) + " bytes of output, more than 65536");
        nEmpty += m.isize == 0;
        total += m.isize;
        tab.push_back(m);
        p += size;
    }
    return 0;
}
}  // namespace

extern "C" {

const char *staramd_inflate_last_error(void) { return g_err.c_str(); }
uint32_t staramd_inflate_constant(int which) {
    return which == 0 ? NT : which == 1 ? WAVES : which == 2 ? WG_PER_CU : which == 3 ? envU32("STARAMD_INFLATE_MAX_WORKGROUPS", 0) : which == 4 ? (uint32_t)sizeof(WaveTables) : 0;
}

void staramd_inflate_free(staramd_inflate_result *r) {
    if (!r) return;
    free(r->bytes);
    memset(r, 0, sizeof(*r));
    r->failedMember = -1;
}

int staramd_inflate_host_file(int device, const uint8_t *fileBytes, uint64_t nBytes, staramd_inflate_result *out) {
    if (!out) return fail("no result");
    memset(out, 0, sizeof(*out));
    out->failedMember = -1;
    if (nBytes && !fileBytes) return fail("no file");
    typedef std::chrono::steady_clock Clock;
    const auto t0 = Clock::now();
    std::vector<Member> tab;
    uint64_t total = 0, nEmpty = 0;
    const int w = walkMembers(fileBytes, nBytes, tab, total, nEmpty);
    if (w < 0) return -1;
    const uint64_t n = tab.size();
    out->nMembers = n; out->stats[0] = n; out->stats[1] = nBytes; out->stats[5] = nEmpty;
    if (w == 1) { out->nMembers = n + 1; out->stats[0] = n + 1; out->failedMember = (int64_t)n; out->failedStatus = STARAMD_INFLATE_INPUT_END; return 0; }
    if (n == 0) return 0;
    if (n > 0x7fffffffull) return fail("too many members in one file");
    const double msWalk = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return failHip("hipSetDevice", e);
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return failHip("hipGetDeviceProperties", e);
    hipStream_t st = nullptr;
    if ((e = hipStreamCreate(&st)) != hipSuccess) return failHip("hipStreamCreate", e);
    int rc = 0;
    {   Work wk;
        uint8_t *dFile, *dOut; Member *dTab; uint32_t *dStatus;
        hipEvent_t ev[4];
        std::vector<uint32_t> status(n);
        auto run = [&]() -> int {
            if (wk.dev(dFile, nBytes) || wk.dev(dOut, total) || wk.dev(dTab, n) || wk.dev(dStatus, n)) return -1;
            for (auto &x : ev) if (wk.event(x)) return -1;
            const uint32_t wgEnv = envU32("STARAMD_INFLATE_MAX_WORKGROUPS", 0), maxWg = wgEnv ? wgEnv : WG_PER_CU * (uint32_t)std::max(1, prop.multiProcessorCount);
            const uint32_t grid = (uint32_t)std::min<uint64_t>((n + WAVES - 1) / WAVES, maxWg);
            DH_TRY(hipEventRecord(ev[0], st));
            DH_TRY(hipMemcpyAsync(dFile, fileBytes, nBytes, hipMemcpyHostToDevice, st));
            DH_TRY(hipMemcpyAsync(dTab, tab.data(), n * sizeof(Member), hipMemcpyHostToDevice, st));
            DH_TRY(hipEventRecord(ev[1], st));
            DH_LAUNCH(k_inflate_members, dim3(grid), st, (const uint8_t *)dFile, (const Member *)dTab, (uint32_t)n, dOut, dStatus, (uint32_t *)nullptr);
            DH_TRY(hipEventRecord(ev[2], st));
            DH_TRY(hipMemcpyAsync(status.data(), dStatus, n * 4, hipMemcpyDeviceToHost, st));
            DH_TRY(hipStreamSynchronize(st));
            for (uint64_t i = 0; i < n && out->failedMember < 0; i++) if (status[i]) { out->failedMember = (int64_t)i; out->failedStatus = status[i]; }
            if (out->failedMember < 0 && total) {
                out->bytes = (uint8_t *)malloc(total);
                if (!out->bytes) return fail("no host memory for " + std::to_string(total) + " bytes of output");
                DH_TRY(hipMemcpyAsync(out->bytes, dOut, total, hipMemcpyDeviceToHost, st));
                out->nBytes = total; out->stats[2] = total;
            }
            DH_TRY(hipEventRecord(ev[3], st));
            DH_TRY(hipStreamSynchronize(st));
            float msUp = 0, msKernel = 0, msDown = 0;
            (void)hipEventElapsedTime(&msUp, ev[0], ev[1]); (void)hipEventElapsedTime(&msKernel, ev[1], ev[2]); (void)hipEventElapsedTime(&msDown, ev[2], ev[3]);
            out->stats[3] = (uint64_t)(msKernel * 1e6); out->stats[4] = (uint64_t)((msUp + msDown) * 1e6);
            static const bool timing = getenv("STARAMD_HOST_TIMING") != nullptr;
            if (timing)
                fprintf(stderr, "  inflate device: %llu members, %.1f -> %.1f MB, %u workgroups: header walk %.2f ms, H2D %.2f ms, kernel %.2f ms, D2H %.2f ms\n",
                        (unsigned long long)n, nBytes / 1e6, total / 1e6, grid, msWalk, msUp, msKernel, msDown);
            return 0;
        };
        rc = run();
        (void)hipStreamSynchronize(st);
    }
    (void)hipStreamDestroy(st);
    if (rc) { staramd_inflate_free(out); return rc; }
    return 0;
}

}  // extern "C"
