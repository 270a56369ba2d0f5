/* star_amd_dedup.h -- duplicate read pairs of a coordinate-sorted paired-end BAM marked on the MI355X (star_amd/csrc/engine/k_dedup.hip, in libstaramd.so;
 * --runMode inputAlignmentsFromBAM --bamRemoveDuplicatesType ... --gpuBAMdedup Device).  The rule is the reference's (source/bamRemoveDuplicates.cpp)
 * restated per pair -- DESIGN.md 7.6 -- and star_amd/csrc/host/dedup.cpp is its plain C++ statement; both read a record through star_amd/csrc/dedup_rule.h.
 *
 *   scan      one lane per record: fields, NH and AS from one attribute walk, the record's kind, hashes of its name and of its content; unique records compacted
 *   pairing   stable radix sort of the unique records by (tid, name hash); equal names confirmed on the bytes; one mate 1 + one mate 2 = a pair
 *   classes   stable radix sorts of the pairs by content hash, then by the two words of the numeric key; class heads from the bytes; a scan numbers the classes
 *   survivor  a segmented scan per class over (AS of mate 1, then the smaller name); every other pair of the class is marked
 * Hashes only order records.  Where two different names, or two different contents, meet under one key, the array is put in exact order by a merge sort on
 * the comparisons themselves before heads are taken.  STARAMD_DEDUP_HASH_BITS (0..64, default 64; read at each call) keeps that many bits of both
 * hashes, so that tests reach that path; STARAMD_DEDUP_MAX_WORKGROUPS caps the grid of every kernel (default: 16 per CU), so that tests make the
 * grid-stride loops turn.  The result does not depend on either.
 *
 * Everything of one call is resident: the records, ~60 bytes per record and ~100 bytes per unique record of work arrays.  A file larger than device
 * memory is an error text; processing it chromosome by chromosome is out of scope.
 *
 * Return 0 on success, -1 on error (text in staramd_dedup_last_error, per calling thread).  Device memory that cannot be allocated is an error. */
#ifndef STAR_AMD_DEDUP_H
#define STAR_AMD_DEDUP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct staramd_dedup_params {
    int32_t  markMulti;         /* 1: UniqueIdentical (records with NH > 1 are marked), 0: UniqueIdenticalNotMulti (they keep the bit they have) */
    uint32_t mate2basesN;       /* --bamRemoveDuplicatesMate2basesN */
} staramd_dedup_params;

typedef struct staramd_dedup_result {
    uint8_t *dup; uint64_t nRecords;        /* final value of bit 0x400, one byte per record, in the records' order */
    int32_t fatal; uint64_t fatalRecord;    /* 0 | 1 NH missing | 2 AS missing on mate 1 of a pair; lowest such record (dup is not to be used then) */
    /* [0] records, [1] unique records, [2] pairs, [3] classes, [4] records marked (bytes of dup that are 1), [5] unpaired unique records,
     * [6] nanoseconds on the stream from the end of the upload to the start of the copy back: the kernels, the waits for their counts AND the allocation of
     * the work arrays between the stages (several times the kernels' own time; STARAMD_HOST_TIMING prints the stages alone), [7] nanoseconds of the
     * copies to and from the device */
    uint64_t stats[8];
} staramd_dedup_result;

/* records in host memory: record i is bytes[offsets[i] .. offsets[i] + 4 + its block_size), all inside nBytes (the convention of
 * staramd_signal_host_records).  Uploads them, runs the kernels on `device`; n bytes come back */
int  staramd_dedup_host_records(int device, const staramd_dedup_params *p, const uint8_t *bytes, uint64_t nBytes, const uint64_t *offsets, uint64_t n, staramd_dedup_result *out);
void staramd_dedup_free(staramd_dedup_result *r);
/* sizes the tests aim at: 0 work-items per workgroup (every kernel handles one item per work-item in a grid-stride loop), 1 workgroups per CU a grid
 * is capped at by default, 2 STARAMD_DEDUP_MAX_WORKGROUPS as the next call will read it (0: not set) */
uint32_t staramd_dedup_constant(int which);
const char *staramd_dedup_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
