// tail_routines_gpu.hip -- TEST INFRASTRUCTURE: the cases of oracle/tail_routines_check.cpp as compiled gfx950 code.  Takes k_stitch.hip and k_gather.hip into its own translation
// unit and runs the launches of oracle/tail_routines_cases.h over the case file the CPU check wrote (--dump): k_pack_reads one block of 64 lanes per read; k_stitch_verify,
// k_stitch_finish, k_scan_local and k_gather one lane per read in blocks of 256; k_stitch_replay in 2 blocks of 256 with the dynamic LDS of launch depth 0; k_scan_offsets in one
// block of 1024 -- each alone and then in the engine's order.  Everything is compared with the file, whose expected values are the check's restatements of the oracle's rules.
// A fixed workload that ends by construction: every offset comes from the file and lies inside buffers between guard bytes that are verified after every launch; the overflow
// cases (pools and result arrays one record short, a window that fits neither arena) end in the kernels' own bounds tests; every loop of the kernels is bounded by a count of the
// file or by the ticket counter.  Every HIP call is checked and the first error ends the process.
// usage: tail_routines_gpu <case file>          last line: "...: <n> differences"
#include "../star_amd/csrc/engine/k_stitch.hip"
#include "../star_amd/csrc/engine/k_gather.hip"
#include "../oracle/tail_routines_cases.h"

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: tail_routines_gpu <case file>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb"); if (!f) { perror(argv[1]); return 2; }
    static TrsSet S; trsReadFile(f, S); fclose(f);
    return trsRun(S) ? 1 : 0;
}
