// crc32_gf2.h -- the arithmetic that joins partial CRC-32s (k_bgzf.hip: of the block a workgroup compresses; k_inflate.hip: of the member a wavefront
// inflated): polynomials over GF(2) modulo P in the reflected bit order of the CRC (bit 31 = x^0).  A lane's CRC of its slice, multiplied by
// x^(8 * bytes after the slice), is its share of the whole; the shares are XORed.  Device code, one copy for both units; internal linkage.
#pragma once
#include <cstdint>

namespace {

constexpr uint32_t POLY = 0xedb88320u;              // CRC-32, reflected

__device__ __forceinline__ uint32_t mulModP(uint32_t a, uint32_t b) {         // a * b mod P, reflected bit order (bit 31 = x^0)
    uint32_t p = 0;
#pragma unroll 1
    for (int i = 0; i < 32; i++) { if (a & (0x80000000u >> i)) p ^= b; b = (b & 1) ? (b >> 1) ^ POLY : b >> 1; }
    return p;
}
__device__ __forceinline__ uint32_t xPow8(uint32_t nBytes) {                   // x^(8 * nBytes) mod P
    uint32_t e = nBytes * 8, p = 0x80000000u, cur = 0x40000000u;
#pragma unroll 1
    for (int k = 0; k < 20; k++) { if ((e >> k) & 1) p = mulModP(cur, p); cur = mulModP(cur, cur); }
    return p;
}

}  // namespace
