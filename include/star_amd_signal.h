/* star_amd_signal.h -- read coverage ("signal", --outWigType) on the MI355X from BAM records in coordinate order (star_amd/csrc/engine/k_signal.hip, in
 * libstaramd.so; --gpuSignal Device).  What comes back is not a dense array but RUNS: maximal stretches of one track inside one tile of the genome over
 * which the value is the same and not zero.  The host formatter (signalFromRuns, star_amd/csrc/host/signal.cpp) joins runs that touch across a tile
 * boundary and writes the files of writeSignal, byte for byte.
 *
 * The values are those of the reference's loop (signalFromBAM.cpp:160-200): the Unique tracks are counts; a position of a UniqueMultiple track is the
 * sum of 1.0 / NH in double, added record after record IN THE ORDER OF THE RECORDS, one rounding per addition.  The device keeps that order: every
 * record emits one (tile, span) pair per tile a contributing block touches, in record order; a stable radix sort by tile keeps that order inside a
 * tile; one workgroup per occupied tile applies the tile's spans one after the other, every lane adding to the positions it owns.  No floating-point
 * atomics, no reductions across records.
 *
 * Return 0 on success, -1 on error (text in staramd_signal_last_error, per calling thread).  Work buffers that cannot be allocated are an error. */
#ifndef STAR_AMD_SIGNAL_H
#define STAR_AMD_SIGNAL_H
#include <stdint.h>
#include "star_amd_bamsort.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct staramd_signal_params {
    int32_t  type;              /* --outWigType's second word: 0 every aligned base, 1 read1_5p, 2 read2 */
    int32_t  strand;            /* 1: --outWigStrand Stranded (tracks 2 and 3 exist) */
    uint32_t nChr;
    uint32_t wantNorm;          /* 1: fill staramd_signal_result::norm (--outWigNorm RPM) */
    const uint32_t *chrLength;  /* [nChr] */
    const uint8_t  *wanted;     /* [nChr] 1: the name begins with --outWigReferencesPrefix (the caller's test) */
} staramd_signal_params;

/* positions [start, end) of chromosome tid, 0-based; track: 0 Unique.str1, 1 UniqueMultiple.str1, 2 Unique.str2, 3 UniqueMultiple.str2.
 * In the array the runs of one (tid, track) are in ascending order of start and do not overlap; tid ascends */
typedef struct staramd_signal_run { int32_t tid; uint32_t track; uint32_t start, end; double value; } staramd_signal_run;

typedef struct staramd_signal_result {
    staramd_signal_run *runs; uint64_t nRuns;
    /* one entry per record, in the records' order: NH when the record counts for the normalisation (tid >= 0, wanted reference, NH present), else 0.
     * The sum of 1.0 / NH over it is order-bound as well and is the caller's.  NULL unless wantNorm */
    uint32_t *norm; uint64_t nRecords;
    uint8_t *chrHas; uint32_t nChr;     /* [nChr] 1: a record (a duplicate counts) lies on this wanted chromosome -- the header rule of the wiggle files */
    uint32_t pastEnd;                   /* 1: a contributing block reaches chrLength + 1 or beyond; runs is empty then ("BUG: alignment extends past chromosome") */
    /* [0] records, [1] (tile, span) pairs, [2] occupied tiles, [3] bytes of the runs, then nanoseconds on the stream of [4] the record pass, scan and emit,
     * [5] the sort, [6] the tile passes with their scans, [7] the copies back */
    uint64_t stats[8];
} staramd_signal_result;

/* records in host memory: record i is bytes[offsets[i] .. offsets[i] + 4 + its block_size), all inside nBytes.  Uploads them and runs the kernels on `device` */
int  staramd_signal_host_records(int device, const staramd_signal_params *p, const uint8_t *bytes, uint64_t nBytes, const uint64_t *offsets, uint64_t n, staramd_signal_result *out);
/* staramd_bamsort_finish (same arguments, same bytes to the sink) which, once the order is known and before the rounds free the slabs, also computes
 * the tracks of the records where they lie, on the compressor's stream */
int  staramd_bamsort_finish_signal(staramd_bamsort *s, int level, int (*sink)(void *user, const uint8_t *bytes, uint64_t n), void *user, uint64_t stats[8],
                                   const staramd_signal_params *p, staramd_signal_result *out);
void staramd_signal_free(staramd_signal_result *r);
/* compile-time constants of the kernels, for tests that aim at their edges: 0 positions per tile, 1 spans per LDS chunk */
uint32_t staramd_signal_constant(int which);
const char *staramd_signal_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
