// stitch_routines_gpu.hip -- TEST INFRASTRUCTURE: the cases of oracle/stitch_routines_check.cpp as compiled gfx950 code.  Takes k_stitch.hip into its own translation unit and
// runs the probe kernels of oracle/stitch_routines_cases.h over the case file the CPU check wrote (--dump): one wavefront per case in blocks of 256 lanes, the read staged as the
// 4-bit packed copy in dynamic LDS, the genome in device memory with GPAD bytes of code 5 either side; for recordCandidateImpl<false> the rank list and the arena are real LDS,
// for the walk's form of recordCandidate the header slot and the exon rows too.  Every lane's result is held against the expected values of the file, which are the
// restatement's.  A fixed workload that ends by construction: every address comes from the file and lies inside padded arrays, every loop of the routines is bounded by the
// start of the exon, the cap of 255 or the table's mask.  Compile with the product's flags for k_stitch.hip: -O3 -ffp-contract=off -fno-unroll-loops -DSTITCH_WAVES=4.
// usage: stitch_routines_gpu <case file>          last line: "...: <n> differences"
#include "../star_amd/csrc/engine/k_stitch.hip"
#include "../oracle/stitch_routines_cases.h"

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: stitch_routines_gpu <case file>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb"); if (!f) { perror(argv[1]); return 2; }
    static SrsSet S; srsRead(f, S); fclose(f);
    return srsRun(S) ? 1 : 0;
}
