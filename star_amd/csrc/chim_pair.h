// chim_pair.h -- which two alignments of a read may form a chimera, and with what score: the one statement of that rule, for the host (host/chimeric.cpp, both
// algorithms) and for the device (engine/k_stitch.hip chimSelectPartner), and the one blocksOverlap of the record routines of both stitch kernels and of the host.
//   read-space extent, motif strand   source/ChimericSegment.cpp:5-16 = source/ReadAlign_chimericDetectionOld.cpp:31-43, :50-57, :61-64
//   the pair test                     source/ChimericDetection_chimericDetectionMult.cpp:9-16 = source/ReadAlign_chimericDetectionOld.cpp:66-73
//   blocksOverlap                     source/blocksOverlap.cpp:3-40
// Plain functions over unsigned 64-bit read coordinates: the reference's unsigned arithmetic (differences that wrap) is part of the behaviour.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define CHIM_FN __host__ __device__ inline
#else
#define CHIM_FN inline
#endif

// first and last base an alignment covers in read orientation, mates counted without the spacer between them
struct ChimExtent { uint64_t roS, roE; };
template <class E> CHIM_FN ChimExtent chimExtent(uint32_t Str, const E &first, const E &last, uint64_t Lread, uint64_t len0) {
    ChimExtent x;
    x.roS = Str == 0 ? (uint64_t)first.R : Lread - last.R - last.L;
    x.roE = Str == 0 ? (uint64_t)last.R + last.L - 1 : Lread - first.R - 1;
    if (x.roS > len0) x.roS--;
    if (x.roE > len0) x.roE--;
    return x;
}

// strand the intron motifs of an alignment imply: 0 undefined, 1 that of the RNA, 2 the opposite.  motifs = intronMotifs[3]; both counts positive is "undefined" for
// the multimapping algorithm (bothIsUndefined) and falls through to the comparison for the old one and on the device
template <class M> CHIM_FN uint32_t chimMotifStrand(uint32_t Str, const M &motifs, bool bothIsUndefined) {
    if (motifs[1] == 0 && motifs[2] == 0) return 0u;
    if (bothIsUndefined && motifs[1] > 0 && motifs[2] > 0) return 0u;
    return ((Str == 0) == (motifs[1] > 0)) ? 1u : 2u;
}

// may the two form a chimera: both longer than segmentMin beside what they share, and on different mates or no further apart than segmentReadGapMax.
// overlap: the shared read bases, subtracted from the sum of the two scores
CHIM_FN bool chimPairEligible(const ChimExtent &a, const ChimExtent &b, uint64_t len0, uint64_t segmentMin, uint64_t segmentReadGapMax, uint64_t &overlap) {
    overlap = b.roS > a.roS ? (b.roS > a.roE ? 0 : a.roE - b.roS + 1) : (b.roE < a.roS ? 0 : b.roE - a.roS + 1);
    const bool diffMates = (a.roE < len0 && b.roS >= len0) || (b.roE < len0 && a.roS >= len0);
    return a.roE > segmentMin + a.roS + overlap && b.roE > segmentMin + b.roS + overlap
           && (diffMates || ((a.roE + segmentReadGapMax + 1) >= b.roS && (b.roE + segmentReadGapMax + 1) >= a.roS));
}

// read bases that two exon lists place on the same diagonal (P1 / P2: pointers to exon records, in any address space)
template <class P1, class P2> CHIM_FN uint32_t blocksOverlap(P1 e1, uint32_t n1, P2 e2, uint32_t n2) {
    uint32_t i1 = 0, i2 = 0, nOverlap = 0;
    while (i1 < n1 && i2 < n2) {
        uint64_t rs1 = e1[i1].R, rs2 = e2[i2].R;
        uint64_t re1 = rs1 + e1[i1].L, re2 = rs2 + e2[i2].L;
        uint64_t gs1 = e1[i1].G, gs2 = e2[i2].G;
        if (rs1 >= re2) i2++;
        else if (rs2 >= re1) i1++;
        else if (gs1 - rs1 != gs2 - rs2) { if (re1 >= re2) i2++; if (re2 >= re1) i1++; }
        else { nOverlap += (uint32_t)((re1 < re2 ? re1 : re2) - (rs1 > rs2 ? rs1 : rs2)); if (re1 >= re2) i2++; if (re2 >= re1) i1++; }
    }
    return nOverlap;
}
