// seq_insert_check.cpp -- TEST INFRASTRUCTURE: the passes of the sequence insertion (star_amd/csrc/index/seq_core.h) one at a time against a serial
// restatement of the reference's insertSeqSA, on the plain-loop backend (oracle/loop_backend.h).  Cases, restatement and comparisons are the
// templates of tests/seq_insert_cases.h; tests/seq_insert_gpu.hip instantiates the same with HipBackend.  One line per class with its count,
// "compared X of Y cases", and a last line "...: N differences"; a class that never occurred or a case that was not compared fails the run.
//
// usage: seq_insert_check <golden dir>          (tests/golden/seq_insert)
#include "../oracle/loop_backend.h"
#include "seq_insert_cases.h"

int main(int argc, char **argv) {
    using namespace seqchk;
    if (argc < 2) { fprintf(stderr, "usage: seq_insert_check <golden dir>\n"); return 2; }
    LoopBackend be;
    SeqReport R;
    runStrandBitCases(be, R);
    runFabricated(be, R);
    runGolden(be, R, argv[1]);
    return R.finish("sequence insertion on the plain-loop backend");
}
