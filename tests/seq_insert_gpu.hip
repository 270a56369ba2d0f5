// seq_insert_gpu.hip -- TEST INFRASTRUCTURE: the cases of tests/seq_insert_check.cpp as compiled gfx950 code.  The templates of tests/seq_insert_cases.h
// (fabricated cases, the cases of tests/golden/seq_insert, the serial restatement of insertSeqSA computed on the host, comparisons, classes)
// instantiated with the product's HipBackend (star_amd/csrc/index/hip_backend.h).  Every HIP call is checked: the backend keeps its first error, the
// stream is synchronised and the error looked at after every case, and the first one ends the process with a non-zero status before anything
// further is started.  The workload is fixed and ends by construction; the process opens the GPU once.
//
// usage: seq_insert_gpu <golden dir>          last line: "...: <n> differences"
#include "../star_amd/csrc/index/hip_backend.h"
#include "seq_insert_cases.h"
#include <chrono>

namespace idxchk {
template <> struct BackendTraits<HipBackend> {
    static const char *error(HipBackend &be) {
        be.chk(hipStreamSynchronize(be.s), "synchronisation after a case");
        be.chk(hipGetLastError(), "after a case");
        if (be.err == hipSuccess) return nullptr;
        static char buf[256];
        snprintf(buf, sizeof buf, "%s: %s", be.where, hipGetErrorString(be.err));
        return buf;
    }
};
} // namespace idxchk

static double nowSeconds() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char **argv) {
    using namespace seqchk;
    if (argc < 2) { fprintf(stderr, "usage: seq_insert_gpu <golden dir>\n"); return 2; }
    if (hipSetDevice(0) != hipSuccess) { fprintf(stderr, "hipSetDevice failed\n"); return 3; }
    HipBackend be;
    if (hipStreamCreate(&be.s) != hipSuccess) { fprintf(stderr, "hipStreamCreate failed\n"); return 3; }
    SeqReport R;
    double t = nowSeconds();
    auto lap = [&](const char *what) { const double t1 = nowSeconds(); printf("%-40s %.2f s\n", what, t1 - t); fflush(stdout); t = t1; };
    runStrandBitCases(be, R); lap("strand bit check");
    runFabricated(be, R); lap("fabricated insertions");
    runGolden(be, R, argv[1]); lap("cases the reference wrote");
    if (be.tmp) be.chk(hipFree(be.tmp), "hipFree(tmp)");
    be.chk(hipStreamDestroy(be.s), "hipStreamDestroy");
    if (be.err != hipSuccess) { printf("backend error at the end: %s: %s\n", be.where, hipGetErrorString(be.err)); return 3; }
    return R.finish("sequence insertion on gfx950");
}
