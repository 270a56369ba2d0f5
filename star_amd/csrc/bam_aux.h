// bam_aux.h -- the walk over the attributes of one BAM record (bam_aux_get + bam_aux2i), with every read held inside the record.  One statement for the
// device units (k_signal.hip: NH; k_dedup.hip: NH and AS from one walk) and for the host's duplicate marking (host/dedup.cpp).  auxInt of host/signal.cpp
// is the same walk on records the host trusts.
#pragma once
#include <cstdint>
#ifndef BAM_HD
#ifdef __HIPCC__
#define BAM_HD __host__ __device__ inline
#else
#define BAM_HD inline
#endif
#endif
#ifdef __clang__
#define BAM_NO_UNROLL _Pragma("unroll 1")
#else
#define BAM_NO_UNROLL
#endif

BAM_HD uint32_t bamLd32(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }     // records lie at arbitrary byte addresses
BAM_HD uint32_t bamLd16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }

// The integer attributes a0a1 and -- with wantB -- b0b1 of a record of `lim` bytes whose attributes begin at byte a.  Returns bit 0: the first is there,
// bit 1: the second is there; the first occurrence of a tag counts.  A value of a non-integer type, or one that the record's end cuts off, reads as 0.
// The walk ends at the record's end, at an unknown type, and as soon as everything asked for was found.
BAM_HD uint32_t bamAuxInts(const uint8_t *rec, uint64_t lim, uint64_t a, char a0, char a1, uint32_t &valA, bool wantB, char b0, char b1, uint32_t &valB) {
    uint32_t got = 0;
    const uint32_t all = wantB ? 3 : 1;
    BAM_NO_UNROLL
    while (a + 3 <= lim) {
        const uint8_t t = rec[a + 2];
        const bool hitA = !(got & 1) && rec[a] == (uint8_t)a0 && rec[a + 1] == (uint8_t)a1;
        const bool hitB = wantB && !hitA && !(got & 2) && rec[a] == (uint8_t)b0 && rec[a + 1] == (uint8_t)b1;
        a += 3;
        uint64_t w;
        switch (t) {
            case 'A': case 'c': case 'C': w = 1; break;
            case 's': case 'S': w = 2; break;
            case 'i': case 'I': case 'f': w = 4; break;
            case 'Z': case 'H': { uint64_t j = a; while (j < lim && rec[j] != 0) j++; w = j - a + 1; break; }
            case 'B': { if (a + 5 > lim) return got;
                        const uint8_t bt = rec[a]; const uint32_t n = bamLd32(rec + a + 1); w = 5 + (uint64_t)n * (bt == 'c' || bt == 'C' ? 1 : bt == 's' || bt == 'S' ? 2 : 4); break; }
            default: return got;
        }
        if (hitA || hitB) {
            uint32_t val = 0;
            if (a + w <= lim) {
                if (t == 'c') val = (uint32_t)(int32_t)(int8_t)rec[a]; else if (t == 'C') val = rec[a];
                else if (t == 's') val = (uint32_t)(int32_t)(int16_t)bamLd16(rec + a); else if (t == 'S') val = bamLd16(rec + a);
                else if (t == 'i' || t == 'I') val = bamLd32(rec + a);
            }
            if (hitA) { valA = val; got |= 1; } else { valB = val; got |= 2; }
            if (got == all) return got;
        }
        a += w;
    }
    return got;
}
