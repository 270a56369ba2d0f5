// bgzf_resident.h -- the BGZF kernels of k_bgzf.hip on input that is in device memory already (k_bamsort.hip lays the sorted records out there).
// Defined in k_bgzf.hip; internal to the engine library.  Errors: -1, text in staramd_bgzf_last_error.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../../include/star_amd_bgzf.h"

// the compressor's device, stream and launch width of k_bgzf_blocks (workgroups)
void bgzfResidentInfo(staramd_bgzf *z, int *device, hipStream_t *stream, uint32_t *grid);
// calls of staramd_bgzf_compress on z wait while it is held (they use the same slots and scratch)
void bgzfResidentLock(staramd_bgzf *z);
void bgzfResidentUnlock(staramd_bgzf *z);
// slots and sizes for up to nb blocks per call.  Frees and reallocates when it has to grow: not while kernels on them are in flight
int bgzfResidentReserve(staramd_bgzf *z, uint64_t nb);
// k_bgzf_blocks, k_bgzf_scan, k_bgzf_compact on z's stream: block b is dIn[dBlkOff[b] .. + dBlkLen[b]); the members go back to back into dOut
// (staramd_bgzf_bound of the input at least), dOff[b] = where member b starts, dOff[nb] = their total.  Returns when the launches are queued.
int bgzfCompressResident(staramd_bgzf *z, const uint8_t *dIn, const uint64_t *dBlkOff, const uint32_t *dBlkLen, uint32_t nb, int level, uint8_t *dOut, uint64_t *dOff);
