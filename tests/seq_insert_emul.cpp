// seq_insert_emul.cpp -- TEST INFRASTRUCTURE ONLY.  The sequence insertion of star_amd/csrc/index/seq_core.h on the plain-loop backend
// (oracle/loop_backend.h), with the signature of staramd_seq_insert: the twin behind the CPU tests (tests/test_seq_insert.py installs it through
// capi.device_seq_insertion).  The product is the HIP instantiation in star_amd/csrc/index/index_gpu.hip.
#include "../star_amd/csrc/index/seq_core.h"
#include "../include/star_amd_index.h"
#include "../oracle/loop_backend.h"

using namespace staridx;

extern "C" int seq_emul_insert(int, const staramd_seq_args *a, staramd_seq_result *res) {
    LoopBackend be;
    SeqParams P; P.nG = a->nGenomeReal; P.nG1 = a->nGins; P.nG2 = a->nGenomeOld - a->nGenomeReal; P.nSAold = a->nSAold; P.GstrandBit = a->GstrandBit; P.saIndexNbases = a->gSAindexNbases;
    SeqHostArgs A{a->G, a->SA, a->nSAbyteOld, a->Gins, a->SAout, a->saOutCapacity, a->SAiOut, a->saiOutCapacity};
    SeqDeviceResult R; u64 nb = 0, nbi = 0;
    const int rc = seqInsertHost(be, P, A, R, nb, nbi);
    memset(res, 0, sizeof(*res));
    res->nInd = R.nInd; res->nSAnew = R.nSAnew; res->nSAbyteNew = nb; res->nSAibyte = nbi; res->nCapHits = R.nCapHits; res->doublingRounds = (uint32_t)R.rounds;
    return rc;
}
