/* star_amd_bgzf.h -- BGZF compression of BAM record streams on the MI355X (star_amd/csrc/engine/k_bgzf.hip, in libstaramd.so).
 *
 * Every segment is cut into blocks of 0xff00 input bytes (the last one shorter), exactly as the host path (star_amd/csrc/host/bgzf.cpp) cuts it;
 * every block becomes one complete gzip member (18-byte BGZF header, raw deflate, CRC32, ISIZE).  One workgroup compresses one block; the
 * members of a call are compacted on the device and come back in one copy.  Decompressed content equals the input; the compressed bytes are
 * deterministic (same input and level: same bytes on every run) but differ from zlib's.  The header block of a BAM file and the 28-byte EOF
 * marker are not made here.
 *
 * staramd_bgzf_compress has the signature of the host library's hook (sah_set_bgzf_device_fn, include/star_amd_host.h): install it with the
 * compressor as `user`.  It may be called from several threads; calls are serialised.  Return 0 on success, -1 on error (text in
 * staramd_bgzf_last_error, per calling thread).  Levels -1..9 as zlib's (0 = stored blocks only); any other level is an error. */
#ifndef STAR_AMD_BGZF_H
#define STAR_AMD_BGZF_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct staramd_bgzf staramd_bgzf;
/* own stream, device buffers and page-locked staging buffers for initialInputBytes of input per call (grown on demand) */
int  staramd_bgzf_create(staramd_bgzf **out, int device, uint64_t initialInputBytes);
/* the most output bytes one segment of inputBytes can give */
uint64_t staramd_bgzf_bound(uint64_t inputBytes);
/* z: a staramd_bgzf.  nSeg segments in[s] of inLen[s] bytes; their BGZF members go back to back into out (outCap bytes, at least the sum of
 * staramd_bgzf_bound over the segments), outLen[s] = bytes of segment s.  An empty segment gives no member. */
int  staramd_bgzf_compress(void *z, int level, uint32_t nSeg, const uint8_t *const *in, const uint64_t *inLen,
                           uint8_t *out, uint64_t outCap, uint64_t *outLen);
void staramd_bgzf_destroy(staramd_bgzf *z);
const char *staramd_bgzf_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
