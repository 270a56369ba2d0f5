// index_routines_check.cpp -- TEST INFRASTRUCTURE: the passes of the index builder (star_amd/csrc/index/index_core.h: prefixKey, bucketOf, rankAt,
// saiClassFast, compactIf, buildText, suffixSort, packArray, buildSAindex, buildAll; sjdb_core.h: sjdbSearchOne, sjdbInsertDevice, sjdbInsertHost)
// one at a time against independent restatements of the reference's rules, on the plain-loop backend (oracle/loop_backend.h).  The cases, the
// restatements and the comparisons are the templates of oracle/index_routines_cases.h; tests/index_routines_gpu.hip instantiates the same with
// HipBackend.  Cases come from fixed seeds; expected values are computed here on the host.  Every case is classified from the expected side:
// one line per class with its count, "compared X of Y cases", and a last line "...: N differences"; a class that never occurred or a case that
// was not compared fails the run.
//
// usage: index_routines_check [fixture dir]          (tests/golden/tiny_index: the reference's own files hold the restatements and the product)
#include "loop_backend.h"
#include "index_routines_cases.h"

int main(int argc, char **argv) {
    using namespace idxchk;
    LoopBackend be;
    Report R;
    runPackCases(be, R);
    runPrimitiveCases(be, R);
    runGenomeCases(be, R);
    runInsertCases(be, R);
    if (argc > 1) runFixtureCases(be, R, argv[1]);
    return R.finish("index routines on the plain-loop backend");
}
