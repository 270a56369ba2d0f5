// seed_routines_gpu.hip -- TEST INFRASTRUCTURE: the cases of oracle/seed_routines_check.cpp as compiled gfx950 code.  Takes k_seed.hip into its own translation unit, adds probe
// kernels with one lane per case, reads the case file the CPU check wrote (oracle/seed_routines_cases.h) and holds every result against the expected values in it: k_sak_build's
// records bit for bit against the emulator's, compareSeqToGenome with and without keys, mmpRunT<u32> and mmpRunT<u64> with and without keys, seedLookup, and mmpRun over intervals
// of more than 2^32 entries.  A fixed, terminating workload: every interval and address comes from the file and lies inside the padded arrays.
// usage: seed_routines_gpu <case file>          last line: "...: <n> differences"
#include "../star_amd/csrc/engine/k_seed.hip"
#include "../oracle/seed_routines_cases.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

struct CmpOut { u32 len[2], comp[2]; };                       // [0] keys, [1] no keys
struct MmpOut { u64 i0, i1, nrep; u32 L, pad; };

extern "C" __global__ void __launch_bounds__(256) k_probe_cmp(const DevIndex *Xk, const DevIndex *X0, const u8 *reads, const SrcCmp *cs, u32 n, CmpOut *out) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const SrcCmp c = cs[i]; const u8 *R = reads + c.rOff; SeedCnt cn = {0, 0, 0}; CmpOut o;
    for (u32 v = 0; v < 2; v++) {
        const DevIndex &X = v ? *X0 : *Xk;
        const QKey qk = makeQKey(X, R, c.S, c.Nq, c.dirR != 0);
        bool cr = false;
        o.len[v] = compareSeqToGenome(X, R, c.S, c.N, c.L, c.iSA, c.dirR != 0, cr, cn, qk);
        o.comp[v] = o.len[v] < c.N ? (cr ? 1u : 0u) : 2u;
    }
    out[i] = o;
}
// variants: 0 mmpRunT<u32> keys, 1 mmpRunT<u32> no keys, 2 mmpRunT<u64> keys, 3 mmpRunT<u64> no keys; wide: 0 mmpRun, 1 mmpRunT<u64> on X0 (the array of > 2^32 entries, no keys)
extern "C" __global__ void __launch_bounds__(256) k_probe_mmp(const DevIndex *Xk, const DevIndex *X0, const u8 *reads, const SrcMmp *cs, u32 n, MmpOut *out, u32 wide) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const SrcMmp c = cs[i]; const u8 *R = reads + c.rOff; SeedCnt cn = {0, 0, 0};
    const bool dirR = c.dirR != 0;
    for (u32 v = 0; v < (wide ? 2u : 4u); v++) {
        const DevIndex &X = (wide || (v & 1)) ? *X0 : *Xk;
        const QKey qk = makeQKey(X, R, c.S, c.N, dirR);
        MmpOut o; o.L = c.L; o.i0 = ~0ull; o.i1 = ~0ull; o.pad = 0;
        if (wide) o.nrep = v ? mmpRunT<u64>(X, R, c.S, c.N, c.first, c.last, dirR, o.L, o.i0, o.i1, cn, qk) : mmpRun(X, R, c.S, c.N, c.first, c.last, dirR, o.L, o.i0, o.i1, cn, qk);
        else o.nrep = (v & 2) ? mmpRunT<u64>(X, R, c.S, c.N, c.first, c.last, dirR, o.L, o.i0, o.i1, cn, qk) : mmpRunT<u32>(X, R, c.S, c.N, c.first, c.last, dirR, o.L, o.i0, o.i1, cn, qk);
        out[(u64)i * 4 + v] = o;
    }
}
extern "C" __global__ void __launch_bounds__(256) k_probe_look(const DevIndex *Xk, const u8 *reads, const SrcLook *cs, u32 n, SeedLook *out) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const SrcLook c = cs[i]; SeedCnt cn = {0, 0, 0};
    out[i] = seedLookup(*Xk, reads + c.rOff, c.S, c.len, c.dirR != 0, cn);
}

template <class T> static std::vector<T> take(FILE *f, size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "case file: short read\n"); exit(2); } return v; }
template <class T> static T *up(const std::vector<T> &v, size_t extraBytes = 64) { T *d = nullptr; CK(hipMalloc((void **)&d, v.size() * sizeof(T) + extraBytes)); CK(hipMemset(d, 0, v.size() * sizeof(T) + extraBytes)); if (!v.empty()) CK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice)); return d; }
template <class T> static std::vector<T> down(const T *d, size_t n) { std::vector<T> v(n); if (n) CK(hipMemcpy(v.data(), d, n * sizeof(T), hipMemcpyDeviceToHost)); return v; }

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: seed_routines_gpu <case file>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb"); if (!f) { perror(argv[1]); return 2; }
    const std::vector<u64> head = take<u64>(f, 2);
    if (head[0] != SRC_MAGIC) { fprintf(stderr, "not a case file\n"); return 2; }
    long bad = 0; u64 nRec = 0, nCmp = 0, nMmp = 0, nLook = 0, nWide = 0;
#define FAIL(...) do { if (bad++ < 20) printf(__VA_ARGS__); } while (0)
    for (u64 is = 0; is < head[1]; is++) {
        const SrcSet s = take<SrcSet>(f, 1)[0];
        const std::vector<u8> G = take<u8>(f, s.gBytes); const std::vector<u64> SA = take<u64>(f, s.saWords), SAi = take<u64>(f, s.saiWords);
        const std::vector<SakRec> sakWant = take<SakRec>(f, s.nSA); const std::vector<u8> reads = take<u8>(f, s.readBytes);
        const std::vector<SrcCmp> cmp = take<SrcCmp>(f, s.nCmp); const std::vector<SrcMmp> mmp = take<SrcMmp>(f, s.nMmp); const std::vector<SrcLook> look = take<SrcLook>(f, s.nLook);
        u8 *dG = up(G); u64 *dSA = up(SA), *dSAi = up(SAi); u8 *dReads = up(reads);
        SakRec *dSak = nullptr; CK(hipMalloc((void **)&dSak, (s.nSA + 1) * sizeof(SakRec))); CK(hipMemset(dSak, 0, (s.nSA + 1) * sizeof(SakRec)));
        DevIndex X; memset(&X, 0, sizeof(X));
        X.G = dG + GPAD; X.SA = dSA; X.SAi = dSAi; X.nGenome = s.nGenome; X.nSA = s.nSA;
        for (int i = 0; i < 17; i++) X.saiStart[i] = s.saiStart[i];
        X.strandBit = (u32)s.strandBit; X.saBits = X.strandBit + 1; X.saiBits = X.strandBit + 3; X.saMask = (1ull << X.saBits) - 1; X.saiMask = (1ull << X.saiBits) - 1;
        X.strandMask = ~(1ull << X.strandBit); X.saiNbit = 1ull << (X.strandBit + 1); X.saiAbsentBit = 1ull << (X.strandBit + 2); X.saiNbases = (u32)s.saiNbases; X.sparseD = 1;
        DevIndex *dX0 = nullptr, *dXk = nullptr; CK(hipMalloc((void **)&dX0, sizeof(X))); CK(hipMalloc((void **)&dXk, sizeof(X)));
        CK(hipMemcpy(dX0, &X, sizeof(X), hipMemcpyHostToDevice));
        // key records
        hipLaunchKernelGGL(k_sak_build, dim3((u32)((s.nSA + 255) / 256)), dim3(256), 0, 0, (const DevIndex *)dX0, (u64 *)dSak, (u64)0, s.nSA);
        CK(hipGetLastError()); CK(hipDeviceSynchronize());
        const std::vector<SakRec> sakGot = down(dSak, s.nSA);
        for (u64 i = 0; i < s.nSA; i++) if (sakGot[i].w0 != sakWant[i].w0 || sakGot[i].key != sakWant[i].key) FAIL("SAK DIFF set %llu entry %llu: %016llx %016llx, emulator %016llx %016llx\n", (unsigned long long)is, (unsigned long long)i,
                                                                                                                     (unsigned long long)sakGot[i].w0, (unsigned long long)sakGot[i].key, (unsigned long long)sakWant[i].w0, (unsigned long long)sakWant[i].key);
        nRec += s.nSA;
        X.SAK = dSak; X.sakBases = X.saiNbases; CK(hipMemcpy(dXk, &X, sizeof(X), hipMemcpyHostToDevice));
        // compareSeqToGenome
        { SrcCmp *dC = up(cmp); CmpOut *dO = nullptr; CK(hipMalloc((void **)&dO, (cmp.size() + 1) * sizeof(CmpOut)));
          hipLaunchKernelGGL(k_probe_cmp, dim3((u32)((cmp.size() + 255) / 256 + 1)), dim3(256), 0, 0, (const DevIndex *)dXk, (const DevIndex *)dX0, (const u8 *)dReads, (const SrcCmp *)dC, (u32)cmp.size(), dO);
          CK(hipGetLastError()); CK(hipDeviceSynchronize());
          const std::vector<CmpOut> o = down(dO, cmp.size());
          for (size_t i = 0; i < cmp.size(); i++) for (int v = 0; v < 2; v++) if (o[i].len[v] != cmp[i].expLen || o[i].comp[v] != cmp[i].expComp)
              FAIL("COMPARE DIFF set %llu case %zu %s: %u/%u, oracle %u/%u\n", (unsigned long long)is, i, v ? "no keys" : "keys", o[i].len[v], o[i].comp[v], cmp[i].expLen, cmp[i].expComp);
          nCmp += cmp.size(); CK(hipFree(dC)); CK(hipFree(dO)); }
        // mmpRunT
        { SrcMmp *dC = up(mmp); MmpOut *dO = nullptr; CK(hipMalloc((void **)&dO, (mmp.size() + 1) * 4 * sizeof(MmpOut)));
          hipLaunchKernelGGL(k_probe_mmp, dim3((u32)((mmp.size() + 255) / 256 + 1)), dim3(256), 0, 0, (const DevIndex *)dXk, (const DevIndex *)dX0, (const u8 *)dReads, (const SrcMmp *)dC, (u32)mmp.size(), dO, 0u);
          CK(hipGetLastError()); CK(hipDeviceSynchronize());
          const std::vector<MmpOut> o = down(dO, mmp.size() * 4);
          for (size_t i = 0; i < mmp.size(); i++) for (int v = 0; v < 4; v++) { const MmpOut &r = o[i * 4 + v]; if (r.L != mmp[i].expL || r.i0 != mmp[i].exp0 || r.i1 != mmp[i].exp1 || r.nrep != mmp[i].expNrep)
              FAIL("MMP DIFF set %llu case %zu variant %d: L %u [%llu, %llu], oracle L %u [%llu, %llu]\n", (unsigned long long)is, i, v, r.L, (unsigned long long)r.i0, (unsigned long long)r.i1, mmp[i].expL, (unsigned long long)mmp[i].exp0, (unsigned long long)mmp[i].exp1); }
          nMmp += mmp.size(); CK(hipFree(dC)); CK(hipFree(dO)); }
        // seedLookup
        { SrcLook *dC = up(look); SeedLook *dO = nullptr; CK(hipMalloc((void **)&dO, (look.size() + 1) * sizeof(SeedLook)));
          hipLaunchKernelGGL(k_probe_look, dim3((u32)((look.size() + 255) / 256 + 1)), dim3(256), 0, 0, (const DevIndex *)dXk, (const u8 *)dReads, (const SrcLook *)dC, (u32)look.size(), dO);
          CK(hipGetLastError()); CK(hipDeviceSynchronize());
          const std::vector<SeedLook> o = down(dO, look.size());
          for (size_t i = 0; i < look.size(); i++) if (o[i].i1 != look[i].exp1 || o[i].i2 != look[i].exp2 || o[i].maxL != look[i].expMaxL || o[i].kind != look[i].expKind)
              FAIL("LOOKUP DIFF set %llu case %zu: kind %u [%llu, %llu] maxL %u, wanted kind %u [%llu, %llu] maxL %u\n", (unsigned long long)is, i, o[i].kind, (unsigned long long)o[i].i1, (unsigned long long)o[i].i2, o[i].maxL, look[i].expKind,
                   (unsigned long long)look[i].exp1, (unsigned long long)look[i].exp2, look[i].expMaxL);
          nLook += look.size(); CK(hipFree(dC)); CK(hipFree(dO)); }
        // intervals of more than 2^32 entries (one set of the file): 9.1 GB of device memory, zero but for the head and the tail of the array, freed before the next set
        if (s.nWide) {
            const std::vector<u64> hw = take<u64>(f, s.wideHeadWords), tw = take<u64>(f, s.wideWords - s.wideTailWord); const std::vector<SrcMmp> wide = take<SrcMmp>(f, s.nWide);
            u64 *dW = nullptr; CK(hipMalloc((void **)&dW, (s.wideWords + 8) * 8)); CK(hipMemset(dW, 0, (s.wideWords + 8) * 8));
            CK(hipMemcpy(dW, hw.data(), hw.size() * 8, hipMemcpyHostToDevice)); CK(hipMemcpy(dW + s.wideTailWord, tw.data(), tw.size() * 8, hipMemcpyHostToDevice));
            DevIndex XW = X; XW.SAK = nullptr; XW.sakBases = 0; XW.SA = dW; XW.SAi = nullptr; XW.nSA = s.nSA + s.wideExtra; XW.strandBit = (u32)s.wideBit; XW.saBits = XW.strandBit + 1; XW.saMask = (1ull << XW.saBits) - 1; XW.strandMask = ~(1ull << XW.strandBit);
            DevIndex *dXW = nullptr; CK(hipMalloc((void **)&dXW, sizeof(XW))); CK(hipMemcpy(dXW, &XW, sizeof(XW), hipMemcpyHostToDevice));
            SrcMmp *dC = up(wide); MmpOut *dO = nullptr; CK(hipMalloc((void **)&dO, (wide.size() + 1) * 4 * sizeof(MmpOut)));
            hipLaunchKernelGGL(k_probe_mmp, dim3((u32)((wide.size() + 255) / 256 + 1)), dim3(256), 0, 0, (const DevIndex *)dXW, (const DevIndex *)dXW, (const u8 *)dReads, (const SrcMmp *)dC, (u32)wide.size(), dO, 1u);
            CK(hipGetLastError()); CK(hipDeviceSynchronize());
            const std::vector<MmpOut> o = down(dO, wide.size() * 4);
            for (size_t i = 0; i < wide.size(); i++) for (int v = 0; v < 2; v++) { const MmpOut &r = o[i * 4 + v]; if (r.L != wide[i].expL || r.i0 != wide[i].exp0 || r.i1 != wide[i].exp1 || r.nrep != wide[i].expNrep)
                FAIL("WIDE MMP DIFF set %llu case %zu %s: L %u [%llu, %llu], oracle L %u [%llu, %llu]\n", (unsigned long long)is, i, v ? "mmpRunT<u64>" : "mmpRun", r.L, (unsigned long long)r.i0, (unsigned long long)r.i1, wide[i].expL, (unsigned long long)wide[i].exp0, (unsigned long long)wide[i].exp1); }
            nWide += wide.size(); CK(hipFree(dC)); CK(hipFree(dO)); CK(hipFree(dXW)); CK(hipFree(dW));
        }
        CK(hipFree(dG)); CK(hipFree(dSA)); CK(hipFree(dSAi)); CK(hipFree(dReads)); CK(hipFree(dSak)); CK(hipFree(dX0)); CK(hipFree(dXk));
    }
    fclose(f);
    printf("%llu key records, %llu compares x 2, %llu searches x 4, %llu lookups, %llu searches over more than 2^32 entries x 2: %ld differences\n", (unsigned long long)nRec, (unsigned long long)nCmp, (unsigned long long)nMmp,
           (unsigned long long)nLook, (unsigned long long)nWide, bad);
    return bad ? 1 : 0;
}
