// seed_routines_cases.h -- TEST INFRASTRUCTURE: the case file that oracle/seed_routines_check.cpp writes (--dump) and tests/seed_routines_gpu.hip reads.
// All words little endian.  File = SRC_MAGIC, number of sets, then per set: SrcSet, the genome with its padding (gBytes), the packed suffix array (saWords x 8),
// the packed SAindex (saiWords x 8), the key records the emulator's k_sak_build made (nSA x 16), the reads (readBytes; every read has 64 bytes of its own either
// side), then the cases: nCmp SrcCmp, nMmp SrcMmp, nLook SrcLook.
// Where nWide > 0: a second packed suffix array of (wideBit + 1) bits per entry and wideWords words, in which one entry is repeated wideExtra times more as words of zero --
// the file holds its first wideHeadWords words and the words from wideTailWord on -- and nWide SrcMmp over intervals of more than 2^32 entries of it (no keys).
// One set of a file has them: the array is (2^32 + 12345 + nSA) entries of 17 or 18 bits, 9.1 GB on the device, all of it zero but the head and the tail.
// Expected values are the oracle's (star_oracle.cpp); the CPU check has held them against the engine and a brute-force scan before it writes.
#pragma once
#include <stdint.h>
#define SRC_MAGIC 0x3130545244454553ull       // "SEEDRT01"
struct SrcSet { uint64_t nGenome, nSA, strandBit, saiNbases, saiStart[17], gBytes, saWords, saiWords, readBytes, nCmp, nMmp, nLook,
                nWide, wideBit, wideExtra, wideHeadWords, wideTailWord, wideWords; };
// compareSeqToGenome(S, N, L, iSA, dirR) with a key made for a piece of Nq >= N bases.  expComp: 0 / 1, or 2 where the reference leaves it unset (expLen == N)
struct SrcCmp { uint64_t iSA; uint32_t rOff, S, N, Nq, L, dirR, expLen, expComp; };
// mmpRunT over [first, last] from a common length of L
struct SrcMmp { uint64_t first, last, exp0, exp1, expNrep; uint32_t rOff, S, N, L, dirR, expL; };
struct SrcLook { uint64_t exp1, exp2; uint32_t rOff, S, len, dirR, expMaxL, expKind; };
