// loop_backend.h -- TEST INFRASTRUCTURE ONLY.  The plain-loop backend of star_amd/csrc/index/index_core.h and sjdb_core.h: what HipBackend
// (star_amd/csrc/index/hip_backend.h) does with kernels and rocPRIM, done with loops and std::stable_sort on the host.  Shared by
// oracle/index_emul.cpp (the twin behind the CPU tests of index generation and junction insertion) and oracle/index_routines_check.cpp.
#pragma once
#include "../star_amd/csrc/index/index_core.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

struct LoopBackend {
    typedef staridx::u64 u64;
    template <class T> T *alloc(u64 n) { return (T *)malloc(std::max<u64>(n * sizeof(T), 16)); }
    void free(void *p) { ::free(p); }
    void stage(const char *) {}
    template <class F> void forEach(u64 n, F f) {
#pragma omp parallel for schedule(static)
        for (u64 i = 0; i < n; i++) f(i);
    }
    void sortPairs(u64 *&k, u64 *&kAlt, u64 *&v, u64 *&vAlt, u64 n, int b0, int b1) {
        u64 mask = (b1 >= 64 ? ~0ull : ((1ull << b1) - 1)) & ~((1ull << b0) - 1);
        std::vector<u64> idx(n);
        std::iota(idx.begin(), idx.end(), 0);
        const u64 *kk = k;
        std::stable_sort(idx.begin(), idx.end(), [=](u64 a, u64 b) { return (kk[a] & mask) < (kk[b] & mask); });
        for (u64 i = 0; i < n; i++) { kAlt[i] = k[idx[i]]; vAlt[i] = v[idx[i]]; }
        std::swap(k, kAlt); std::swap(v, vAlt);
    }
    void exclusiveSum(u64 *a, u64 n) { u64 s = 0; for (u64 i = 0; i < n; i++) { u64 t = a[i]; a[i] = s; s += t; } }
    void inclusiveMax(u64 *a, u64 n) { u64 m = 0; for (u64 i = 0; i < n; i++) { m = std::max(m, a[i]); a[i] = m; } }
    u64 readOne(const u64 *p) { return *p; }
    template <class T> void copyToHost(T *dst, const T *src, u64 n) { memcpy(dst, src, n * sizeof(T)); }
    template <class T> void copyToDevice(T *dst, const T *src, u64 n) { memcpy(dst, src, n * sizeof(T)); }
};
