// launch_geom.h -- the memory layout that the stitch and window kernels and the host that launches them (engine.hip) have to agree on:
// sizes of the per-wavefront LDS slices and of the per-wavefront work space in HBM.  One statement, called from both sides.
#pragma once
#include "dev.h"

struct Hdr {                               // transcript header + walk position, kept in registers
    u64 gStart, tG2;
    u32 nExons; i32 Score;
    u32 nMatch, nMM, nGap, lGap, nDel, lDel, nIns, lIns, nUnique, nAnchor, rStart, tR2;
};
struct SFrame { Hdr h; u32 iA; u32 pad; staramd_exon eA; };      // one frame of the walk's undo stack

// ---- k_stitch_win / k_stitch_replay: LDS slice of a wavefront = [packed read] [walk state]
// the packed read: ldsWords 32-bit words (4 bits per base), padded to 16 bytes
__host__ __device__ inline u32 stitchReadBytes(u32 ldsWords) { return (ldsWords * 4u + 15u) & ~15u; }
// the read slice that the occupancy queries reckon with, before any batch is known: a 2x101 pair (203 bases with the spacer = 26 words, made odd = 27)
// plus a full 16 bytes of padding, 27 * 4 + 16 -- a little above stitchReadBytes(27) = 112.  The launches use stitchReadBytes of the batch's longest read.
#define STITCH_READ_WORDS_NOMINAL 27u
#define STITCH_READ_BYTES_NOMINAL (STITCH_READ_WORDS_NOMINAL * 4u + 16u)      // = 124
#define REC_HDR_BYTES 96u                  // staging slot for one output record header
// seed list rows (24 B) and compat masks (8 B): as many as the launch walks at most (capDepth - 1 seeds per window), never more than WA_MAX
__host__ __device__ inline u32 waRows(u32 capDepth) { return capDepth == 0 ? (u32)WA_MAX : (capDepth - 1u < (u32)WA_MAX ? capDepth - 1u : (u32)WA_MAX); }
// walk state, in bytes: undo stack, exon rows + leaf copy, rank list, seed list + compat masks, record header (+ arena in the fast path)
__host__ __device__ inline u32 stitchStateBytes(u32 capDepth, u32 capRank, u32 arenaBytes) {
    u32 b = capDepth * (u32)sizeof(SFrame) + 2u * STARAMD_MAX_N_EXONS * 32u + ((capRank * 2u + 31u) & ~31u) + waRows(capDepth) * 32u + REC_HDR_BYTES + arenaBytes;
    return (b + 127u) & ~127u;
}
static_assert(sizeof(SFrame) == 112, "the undo stack of k_stitch_win is laid out in frames of 112 bytes");
static_assert(REC_HDR_BYTES == sizeof(staramd_transcript), "the record header staged in LDS is one staramd_transcript");
static_assert(sizeof(staramd_exon) == 32, "stitchStateBytes: the two exon tables have rows of 32 bytes");
static_assert(sizeof(DWA) == 24, "stitchStateBytes: a seed-list row is 24 bytes of DWA + 8 bytes of compat mask = the 32 of the waRows term");

// ---- k_windows / k_windows_big
#define WBITS 4096u                 // per-read hash bitmap of the bins covered by windows (quick reject of loci outside every window): bits in the first and last launch
// LDS words of a wavefront of k_windows: 8 table columns of capW rows + the bitmap / owner map
__host__ __device__ inline u32 winLdsWords(u32 capW, u32 hashBits) { return capW * 8 + hashBits / 32; }
// per-wave work space in global memory: [table rows + bitmap (big pass only)] [seed-list blocks]
__host__ __device__ inline u64 winWaveBytes(u32 capW, u32 capBlocks, u32 big) {
    u64 b = (u64)capBlocks * WA_MAX * sizeof(DWA);
    if (big) b += (u64)capW * 8 * sizeof(u32) + WBITS / 8;
    return (b + 255) & ~255ull;
}
