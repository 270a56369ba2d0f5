/* star_amd_inflate.h -- a BGZF file inflated on the MI355X (star_amd/csrc/engine/k_inflate.hip, in libstaramd.so; --runMode inputAlignmentsFromBAM
 * --gpuBAMinflate Device).  BGZF is a chain of independent gzip members of at most 64 KiB, each with its compressed size (BSIZE, in the `BC` extra
 * subfield) and its output size (ISIZE, in the trailer): the host walks the headers, the device inflates the members side by side.
 *
 *   walk      on the host: a chain of BSIZE hops.  A member's gzip header must have FEXTRA and none of FNAME, FCOMMENT, FHCRC; `B` `C` (length 2) is looked
 *             for among the subfields of XLEN, others may stand before or after it.  Every member lies inside the file; the ISIZEs are summed
 *   inflate   one wavefront per member in a grid-stride loop: all of RFC 1951 (stored, fixed and dynamic blocks, any number of them), decode state and
 *             Huffman tables wave-uniform with the tables in LDS, literals and match copies spread over the 64 lanes, output straight to global memory
 *   check     CRC-32 of the member's output as per-lane partial CRCs joined by the GF(2) multiply, against the trailer
 * One status word per member: 0, or a STARAMD_INFLATE_* code.  No read leaves a member's compressed bytes, no write its ISIZE bytes of output, and every
 * trip of the decoder's loops consumes an input bit or produces an output byte, whatever the bytes are.
 *
 * STARAMD_INFLATE_MAX_WORKGROUPS (read at each call) caps the grid (default: 8 workgroups per CU), so that tests make the loop turn; the result does
 * not depend on it.  The file and its output are resident together; what does not fit in device memory is an error text.
 *
 * Return 0 on success, -1 on error (text in staramd_inflate_last_error, per calling thread).  A member that the decoder rejects is NOT an error of the
 * call: it returns 0 with failedMember / failedStatus set and no bytes.  A file that is gzip but not BGZF is an error whose text says so. */
#ifndef STAR_AMD_INFLATE_H
#define STAR_AMD_INFLATE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum {
    STARAMD_INFLATE_OK = 0,
    STARAMD_INFLATE_BLOCK_TYPE = 1,         /* block type 3 */
    STARAMD_INFLATE_STORED_LEN = 2,         /* LEN != ~NLEN */
    STARAMD_INFLATE_OVERSUBSCRIBED = 3,     /* a set of code lengths that claims more codes than there are */
    STARAMD_INFLATE_INCOMPLETE = 4,         /* ... or fewer (but a single distance or literal/length code of one bit, or no distance code, is legal) */
    STARAMD_INFLATE_NO_END_CODE = 5,        /* no code for symbol 256 */
    STARAMD_INFLATE_REPEAT = 6,             /* a repeat with nothing before it, or one that runs past the last code length */
    STARAMD_INFLATE_SYMBOL = 7,             /* literal/length symbols 286 / 287, distance symbols 30 / 31, a code that no symbol has */
    STARAMD_INFLATE_DISTANCE = 8,           /* a distance that reaches before the member's first byte */
    STARAMD_INFLATE_INPUT_END = 9,          /* the input ends inside a symbol or a stored block */
    STARAMD_INFLATE_OUTPUT_OVER = 10,       /* the output would pass ISIZE */
    STARAMD_INFLATE_OUTPUT_SHORT = 11,      /* ... or ends short of it */
    STARAMD_INFLATE_STREAM_END = 12,        /* the deflate stream does not end exactly where the 8-byte trailer begins */
    STARAMD_INFLATE_CRC = 13,               /* the CRC-32 of the output is not the trailer's */
    STARAMD_INFLATE_TOO_MANY = 14,          /* more than 286 literal/length or 30 distance code lengths */
    STARAMD_INFLATE_STATUS_N = 15
};

typedef struct staramd_inflate_result {
    uint8_t *bytes; uint64_t nBytes;        /* the inflated file (malloc'ed; NULL when a member failed or nothing came out) */
    uint64_t nMembers;                      /* members walked, empty ones and the EOF marker included */
    int64_t  failedMember; uint32_t failedStatus;      /* -1 and 0, or the lowest member with a status and that status */
    /* [0] members, [1] input bytes (the file), [2] output bytes, [3] nanoseconds of the kernel, [4] nanoseconds of the copies to and from the device
     * (both from stream events), [5] members that are empty */
    uint64_t stats[8];
} staramd_inflate_result;

/* the whole file in host memory.  Walks the members, uploads, inflates on `device`, brings the bytes back */
int  staramd_inflate_host_file(int device, const uint8_t *fileBytes, uint64_t nBytes, staramd_inflate_result *out);
void staramd_inflate_free(staramd_inflate_result *r);
/* sizes the tests aim at: 0 work-items per workgroup, 1 members a workgroup inflates side by side (one per wavefront), 2 workgroups per CU a grid is capped
 * at by default, 3 STARAMD_INFLATE_MAX_WORKGROUPS as the next call will read it (0: not set), 4 bytes of LDS per wavefront (its tables) */
uint32_t staramd_inflate_constant(int which);
const char *staramd_inflate_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
