// index_routines_gpu.hip -- TEST INFRASTRUCTURE: the cases of oracle/index_routines_check.cpp as compiled gfx950 code.  The templates of
// oracle/index_routines_cases.h (cases from fixed seeds, restatements computed on the host, comparisons, classes) instantiated with the product's
// HipBackend (star_amd/csrc/index/hip_backend.h: k_forEach in slices of 2^31 work-items, rocPRIM radix_sort_pairs through a double_buffer, in-place
// scans, readOne), plus the one case only this backend has: forEach over 2^31 + 300 work-items, i.e. two slices.  Every HIP call is checked: the
// backend keeps its first error, the stream is synchronised and the error looked at after every case, and the first one ends the process with a
// non-zero status before anything further is started.  The workload is fixed and ends by construction; the process opens the GPU once.
//
// usage: index_routines_gpu <fixture dir>          last line: "...: <n> differences"
#include "../star_amd/csrc/index/hip_backend.h"
#include "../star_amd/csrc/index/sjdb_core.h"
#include "../oracle/index_routines_cases.h"
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

static double nowSeconds() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static const char *const HUGE_CLASS = "prim: forEach above one slice (2^31 + 300 work-items)";

// n = 2^31 + 300: the second slice has 300 work-items.  The functor stores its index for the 600 work-items either side of 2^31 (300 of the upper
// 600 do not exist: their slots must stay untouched) and for the last 300, and counts every 2^20-th index: 2049.  A few KB between guard words.
static void caseForEachHuge(HipBackend &be, Report &R) {
    R.begin("forEach 2^31 + 300");
    const u64 mid = 1ull << 31, n = mid + 300, GUARDV = 0xFEEDFACECAFEBEEFull, EMPTY = ~0ull;
    std::vector<u64> init(1 + 1200 + 300 + 1 + 1, EMPTY);
    init.front() = GUARDV; init.back() = GUARDV; init[1 + 1200 + 300] = 0;
    u64 *d = up(be, init); u64 *around = d + 1, *last = around + 1200, *counter = last + 300;
    checkBackend(be, R);
    const double t0 = nowSeconds();
    be.forEach(n, [=] IDX_L (u64 i) {
        if (i + 600 >= mid && i < mid + 600) around[i - (mid - 600)] = i;
        if (i >= n - 300 && i < n) last[i - (n - 300)] = i;
        if ((i & ((1ull << 20) - 1)) == 0) {
#if defined(__HIP_DEVICE_COMPILE__)
            atomicAdd((unsigned long long *)counter, 1ull);
#else
            __atomic_fetch_add(counter, 1ull, __ATOMIC_RELAXED);
#endif
        }
    });
    checkBackend(be, R);
    printf("forEach over 2^31 + 300 work-items: %.1f ms\n", (nowSeconds() - t0) * 1e3);
    std::vector<u64> exp = init;
    for (u64 i = mid - 600; i < n; i++) exp[1 + (i - (mid - 600))] = i;
    for (u64 i = n - 300; i < n; i++) exp[1 + 1200 + (i - (n - 300))] = i;
    exp[1 + 1200 + 300] = 2049;
    R.same("indices either side of 2^31, the last 300, the counter, the guard words", down(be, d, init.size()), exp);
    R.hit(HUGE_CLASS);
    be.free(d);
    checkBackend(be, R);
    R.end();
}
} // namespace idxchk

int main(int argc, char **argv) {
    using namespace idxchk;
    if (argc < 2) { fprintf(stderr, "usage: index_routines_gpu <fixture dir>\n"); return 2; }
    if (hipSetDevice(0) != hipSuccess) { fprintf(stderr, "hipSetDevice failed\n"); return 3; }
    HipBackend be;
    if (hipStreamCreate(&be.s) != hipSuccess) { fprintf(stderr, "hipStreamCreate failed\n"); return 3; }
    Report R;
    R.declare(HUGE_CLASS);
    double t = nowSeconds();
    auto lap = [&](const char *what) { const double t1 = nowSeconds(); printf("%-40s %.2f s\n", what, t1 - t); fflush(stdout); t = t1; };
    runPackCases(be, R); lap("packArray / packedGetW");
    runPrimitiveCases(be, R); lap("backend primitives");
    runGenomeCases(be, R); lap("text, order, SAindex, buildAll");
    runInsertCases(be, R); lap("junction insertion");
    runFixtureCases(be, R, argv[1]); lap("fixtures of the reference");
    caseForEachHuge(be, R); lap("forEach above one slice");
    if (be.tmp) be.chk(hipFree(be.tmp), "hipFree(tmp)");
    be.chk(hipStreamDestroy(be.s), "hipStreamDestroy");
    if (be.err != hipSuccess) { printf("backend error at the end: %s: %s\n", be.where, hipGetErrorString(be.err)); return 3; }
    return R.finish("index routines on gfx950");
}
