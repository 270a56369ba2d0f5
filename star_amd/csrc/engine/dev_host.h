// dev_host.h -- the host-side plumbing of the stand-alone device units (k_bgzf.hip, k_bamsort.hip, k_signal.hip), once.  Host code only.  A unit includes
// it below its kernels with DEV_HOST_PREFIX defined (the text its errors begin with), a constant NT (work-items per workgroup: DH_LAUNCH launches with it,
// without dynamic LDS, and checks what the launch reported) and, where it sorts or scans, DEV_HOST_ROCPRIM (after rocprim.hpp).  Everything has internal
// linkage: a unit keeps its own thread-local error text behind its staramd_*_last_error, independent of the others and of engine.hip (the emulator compiles them alone).
#pragma once
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>
#include <thread>
#include <atomic>

namespace {
thread_local std::string g_err;
inline int fail(const std::string &what) { g_err = DEV_HOST_PREFIX + what; return -1; }
inline int failHip(const char *what, hipError_t e) { return fail(std::string(what) + ": " + hipGetErrorString(e)); }
#define DH_TRY(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return failHip(#call, e_); } while (0)
#define DH_LAUNCH(kernel, grid, stream, ...) do { hipLaunchKernelGGL(kernel, grid, dim3(NT), 0, stream, __VA_ARGS__); DH_TRY(hipGetLastError()); } while (0)
inline int checkLevel(int level) { return level < -1 || level > 9 ? fail("compression level " + std::to_string(level) + " is not in -1..9") : 0; }

inline uint32_t bitsOf(uint64_t v) { uint32_t b = 1; while (b < 64 && (v >> b)) b++; return b; }      // bits that v occupies, at least 1: the end bit of a radix sort
// workgroups of nt work-items for a grid-stride loop over `items`: one per nt items (at least one), at most 64 per CU
inline uint32_t gridFor(uint64_t items, uint32_t nt, uint32_t cus) { return (uint32_t)std::min<uint64_t>((items + nt) / nt, 64ull * cus); }

// device arrays, page-locked arrays and events of one call, released when it leaves (an array of 0 elements still gets an address)
struct Work {
    std::vector<void *> d, h; std::vector<hipEvent_t> ev;
    template <class T> int dev(T *&p, uint64_t n) { void *q = nullptr; DH_TRY(hipMalloc(&q, std::max<uint64_t>(n, 1) * sizeof(T))); d.push_back(q); p = (T *)q; return 0; }
    template <class T> int host(T *&p, uint64_t n) { void *q = nullptr; DH_TRY(hipHostMalloc(&q, std::max<uint64_t>(n, 1) * sizeof(T), 0)); h.push_back(q); p = (T *)q; return 0; }
    int event(hipEvent_t &e) { DH_TRY(hipEventCreate(&e)); ev.push_back(e); return 0; }
    ~Work() { for (void *p : d) (void)hipFree(p); for (void *p : h) (void)hipHostFree(p); for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
};

// a device buffer and a page-locked buffer of one size that only grow (to a quarter more than asked, 1 MiB at least); onDevice = false: the page-locked one alone
struct GrowBuf {
    uint8_t *d = nullptr, *h = nullptr; uint64_t cap = 0;
    void release() { if (d) (void)hipFree(d); if (h) (void)hipHostFree(h); d = h = nullptr; cap = 0; }
    int grow(uint64_t bytes, bool onDevice = true) {
        if (bytes <= cap) return 0;
        bytes = std::max<uint64_t>(bytes + bytes / 4, 1u << 20);
        release();
        if (onDevice) DH_TRY(hipMalloc((void **)&d, bytes));
        DH_TRY(hipHostMalloc((void **)&h, bytes, 0));
        cap = bytes;
        return 0;
    }
};

// memcpy of many pieces on up to 8 threads (the staging copies of a batch are a few hundred MB)
struct Piece { uint8_t *dst; const uint8_t *src; uint64_t n; };
inline void copyPieces(const std::vector<Piece> &ps, uint64_t total) {
    const uint64_t CH = 4u << 20;
    std::vector<Piece> cut;
    for (const Piece &p : ps) for (uint64_t o = 0; o < p.n; o += CH) cut.push_back({p.dst + o, p.src + o, std::min(CH, p.n - o)});
    const unsigned W = (unsigned)std::min<uint64_t>(std::min<uint64_t>(8, cut.size()), std::max<uint64_t>(1, total >> 22));
    std::atomic<size_t> next(0);
    auto run = [&] { for (size_t i; (i = next.fetch_add(1)) < cut.size();) memcpy(cut[i].dst, cut[i].src, cut[i].n); };
    std::vector<std::thread> th;
    for (unsigned w = 1; w < W; w++) th.emplace_back(run);
    run();
    for (auto &t : th) t.join();
}

#ifdef DEV_HOST_ROCPRIM
// rocPRIM's temporary storage for the sorts and scans of one call: every primitive is called twice, first for the size it needs and then, once the
// storage has grown to it, for the work.  (index/hip_backend.h keeps wrappers of its own: its errors are sticky, a different design.)
struct PrimSpace {
    void *tmp = nullptr; size_t cap = 0;
    ~PrimSpace() { if (tmp) (void)hipFree(tmp); }
    int room(size_t need) { if (need > cap) { if (tmp) (void)hipFree(tmp); tmp = nullptr; cap = 0; DH_TRY(hipMalloc(&tmp, need)); cap = need; } return 0; }
    // stable, over key bits [0, bits); afterwards the pointers name the sorted arrays and the other two, whichever they were
    template <class K, class V> int sortPairs(hipStream_t st, K *&k, K *&kAlt, V *&v, V *&vAlt, size_t n, uint32_t bits) {
        rocprim::double_buffer<K> dk(k, kAlt); rocprim::double_buffer<V> dv(v, vAlt);
        size_t need = 0;
        DH_TRY(rocprim::radix_sort_pairs(nullptr, need, dk, dv, n, 0u, bits, st));
        if (room(need)) return -1;
        DH_TRY(rocprim::radix_sort_pairs(tmp, need, dk, dv, n, 0u, bits, st));
        k = dk.current(); kAlt = dk.alternate(); v = dv.current(); vAlt = dv.alternate();
        return 0;
    }
    template <class X> int exclusiveScan(hipStream_t st, X *v, size_t n) {      // in place
        size_t need = 0;
        DH_TRY(rocprim::exclusive_scan(nullptr, need, v, v, (X)0, n, rocprim::plus<X>(), st));
        if (room(need)) return -1;
        DH_TRY(rocprim::exclusive_scan(tmp, need, v, v, (X)0, n, rocprim::plus<X>(), st));
        return 0;
    }
};
#endif
}  // namespace
