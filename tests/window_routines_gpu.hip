// window_routines_gpu.hip -- TEST INFRASTRUCTURE: the cases of oracle/window_routines_check.cpp as compiled gfx950 code.  Takes k_window.hip into its own translation unit and runs
// the probe kernels of oracle/window_routines_cases.h over the case file the CPU check wrote (--dump): one wavefront per case in blocks of 256 lanes for
// createExtendWindowsWithAlign and assignAlignToWindow, the LDS form of the table in the dynamic LDS of the block and the global form in a buffer; the owner map in LDS words and
// in a buffer; sjAlignSplit one lane per case; then the real k_windows (first and middle launch), k_windows_big and k_order_* over the file's batches with the launch shapes of
// engine.hip.  Everything is compared with the file, whose expected values are the oracle's.  A fixed workload that ends by construction: every address comes from the file and
// lies inside buffers between guard bytes that are verified; absent keys are looked up only in owner maps filled to 5/8 at most, which always have an empty slot; every loop of
// the kernels is bounded by a count of the file.
// usage: window_routines_gpu <case file>          last line: "...: <n> differences"
#include "../star_amd/csrc/engine/k_window.hip"
#include "../oracle/window_routines_cases.h"

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: window_routines_gpu <case file>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb"); if (!f) { perror(argv[1]); return 2; }
    static WrsSet S; wrsReadFile(f, S); fclose(f);
    return wrsRun(S) ? 1 : 0;
}
