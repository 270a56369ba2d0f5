/* star_amd_bamsort.h -- ordering of variable-length byte records under a 128-bit key on the MI355X, and their BGZF compression in that order
 * (star_amd/csrc/engine/k_bamsort.hip, in libstaramd.so).  Made for Aligned.sortedByCoord.out.bam (--gpuBAMsort Device), but it knows nothing of
 * BAM: records are bytes, the order is (g, r, order of appending), exactly the comparator of the host path (CoordSortedBam::sortAndCompress).
 *
 * The records are copied into device memory as they are appended (slabs of STARAMD_BAMSORT_SLAB_BYTES, default 256 MiB; an append goes into one
 * slab as a whole; a larger append gets a slab of its own size).  staramd_bamsort_finish orders the record numbers with two stable radix-sort passes
 * (by r, then by g, over the bit ranges the keys of the run occupy), lays the records out in that order (k_bamsort_gather) and compresses the stream
 * with the kernels of include/star_amd_bgzf.h: ONE segment, cut every 0xff00 bytes, only the last block shorter -- the bytes are those of
 * staramd_bgzf_compress on the same stream.  Rounds of STARAMD_BAMSORT_ROUND_BLOCKS blocks (default 8192); the members of a round come back in one
 * copy and go to `sink` while the kernels of the next round run.  The header block of a BAM file and the EOF marker are not made here.
 * The default budget, the slab size and the round size are choices, not measured optima.
 *
 * One sorter is used from one thread at a time.  Return 0 on success, -1 on error (text in staramd_bamsort_last_error, per calling thread). */
#ifndef STAR_AMD_BAMSORT_H
#define STAR_AMD_BAMSORT_H
#include <stdint.h>
#include "star_amd_bgzf.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct staramd_bamsort staramd_bamsort;
/* off: into `records` of this append.  Unmapped records carry g = ~0 (they sort last) */
typedef struct staramd_bam_key { uint64_t g, r; uint64_t off; uint32_t len; uint32_t reserved; } staramd_bam_key;

/* z's device and stream, and z's kernels at finish (z must outlive the sorter).  hbmBudgetBytes bounds the slabs; 0 = half of what hipMemGetInfo
 * reports free at the first append */
int  staramd_bamsort_create(staramd_bamsort **out, staramd_bgzf *z, uint64_t hbmBudgetBytes);
/* 0 taken; 1 = does not fit the budget and nothing was taken; -1 error.  `records` and `keys` may be reused when the call returns (the copy to
 * the device may still be under way: finish and download wait for it).  More than 2^32 - 1 records in all is an error.
 * Every key must lie inside `records` (off + len <= bytes; otherwise an error, nothing taken); the keys need not tile it.  The ordered stream
 * is made of the bytes the keys name and of nothing else: its length is the sum of the keys' len, bytes of `records` under no key (gaps, a
 * tail) are stored and come back from download but are not written, bytes under two keys are written once per key.  len = 0 is allowed. */
int  staramd_bamsort_append(staramd_bamsort *s, const uint8_t *records, uint64_t bytes, const staramd_bam_key *keys, uint32_t n);
/* the bytes of append number iAppend (0, 1, ... in the order of the calls that returned 0) back to the host: for a caller that goes on without
 * the device after an append answered 1 */
int  staramd_bamsort_download(staramd_bamsort *s, uint32_t iAppend, uint8_t *records);
/* order, lay out, compress at `level` (-1..9 as zlib's), hand the members to sink(user, bytes, n) in order (a nonzero return of sink ends the
 * call with an error).  sink == NULL: nothing is ordered, the records are dropped.  Either way the slabs are freed and the sorter is empty again
 * when the call returns.  stats (may be NULL): [0] records, [1] their bytes (the sum of the keys' len), [2] rounds, [3] compressed bytes, then nanoseconds of [4] the
 * sort, [5] the gather kernel, [6] the deflate kernels, [7] sink */
int  staramd_bamsort_finish(staramd_bamsort *s, int level, int (*sink)(void *user, const uint8_t *bytes, uint64_t n), void *user, uint64_t stats[8]);
void staramd_bamsort_destroy(staramd_bamsort *s);
const char *staramd_bamsort_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
