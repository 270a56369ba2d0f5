// bamsort_resident.h -- a pass over the records of a sorter where they lie, in sorted order (k_signal.hip computes the signal tracks there).
// Defined in k_bamsort.hip; internal to the engine library.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../../include/star_amd_bamsort.h"

// Called by the next staramd_bamsort_finish with a sink, once, after the order is known and before the rounds (the slabs are freed when finish leaves):
// dAddr[i] = device address of sorted record i, dDst[i] = where it begins in the sorted stream (dDst[n] = the stream's length, so record i has
// dDst[i + 1] - dDst[i] bytes), on stream st of a device with `cus` compute units.  A nonzero return ends finish with an error.  Not called when the
// sorter holds no bytes.  finish forgets fn when it returns.
typedef int (*BamsortAfterOrder)(void *user, hipStream_t st, uint32_t cus, const uint64_t *dAddr, const uint64_t *dDst, uint64_t n);
void bamsortSetAfterOrder(staramd_bamsort *s, BamsortAfterOrder fn, void *user);
