// cli_run.cpp -- `star_amd`: command-line drop-in for `STAR --runMode alignReads` as a function
// (include/star_amd_cli.h).  Same flags (the subset that reaches the hot path or its outputs; anything else is rejected),
// same genomeDir, same Aligned.out.sam / SJ.out.tab / Log.final.out.  The per-read hot path runs on the MI355X(s) through
// the C ABI of include/star_amd.h; there is no CPU path.
//
// Pipeline (the reference interleaves these per thread, ReadAlignChunk_processChunks.cpp / _mapChunk.cpp):
//   filler, converter FASTQ text -> line table -> numeric batch  (sah_fill_slot, sah_convert_slot)  one thread each, batches numbered in input order
//   mapper threads   one per GPU (--gpuDevices a,b,...): a batch through that GPU's engine context (staramd_map_batch),
//                    plus its merged-mates / WASP re-mapping batches on the same context
//   writer thread    post-map + SAM text on --runThreadN host threads (sah_emit_slot), batches taken in INPUT order whatever
//                    order the GPUs finish in (the order-dependent host state: random multimapper order, vW carry, KeepInputOrder)
// Junction table, Stats and gene counts live in the one host object: nothing to merge inside a process (the reference's
// per-thread tables, outputSJ.cpp:39-83, collapse to one).  Between phases (2-pass, BySJout) every context gets the new
// index / whitelist.
//
// In this file: the hand-off types (Queue, Tokens, ResBuf), generateGenome (--runMode genomeGenerate), Engines (contexts, resident-insertion hook,
// BGZF compressor: set up by create(), released together on every way out), Pipeline (the stage threads as member functions -- filler, converter,
// mapper, writer --, mapInto / mapWaspPieces / mapBatch for one batch on a context, phaseStep between two phases, finish), and staramd_cli_main,
// which reads as that list.
#include <sys/file.h>
#include <fcntl.h>
#include <unistd.h>
#include <cstdio>
#include <ctime>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <map>
#include <array>
#include <algorithm>
#include <chrono>
#include <thread>
#include <mutex>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <string>
#include <memory>
#include "../../../include/star_amd_host.h"
#include "../../../include/star_amd_index.h"
#include "../../../include/star_amd_cli.h"
#include "../../../include/star_amd_async.h"

// the device BGZF compressor (k_bgzf.hip) is in the shipped engine library only: the front ends linked against the oracle / the emulated engine run
// without it, and a run that asks for it there fails at its first batch (sah_set_bgzf_device_fn)
#pragma weak staramd_bgzf_create
#pragma weak staramd_bgzf_compress
#pragma weak staramd_bgzf_destroy
#pragma weak staramd_bgzf_last_error
// likewise the device sorter of Aligned.sortedByCoord.out.bam (k_bamsort.hip, sah_set_bamsort_device)
#pragma weak staramd_bamsort_create
#pragma weak staramd_bamsort_append
#pragma weak staramd_bamsort_download
#pragma weak staramd_bamsort_finish
#pragma weak staramd_bamsort_destroy
#pragma weak staramd_bamsort_last_error
// and the signal tracks on the device (k_signal.hip, sah_set_signal_device)
#pragma weak staramd_signal_host_records
#pragma weak staramd_bamsort_finish_signal
#pragma weak staramd_signal_free
#pragma weak staramd_signal_last_error
// and the duplicate marking on the device (k_dedup.hip, sah_set_dedup_device)
#pragma weak staramd_dedup_host_records
#pragma weak staramd_dedup_free
#pragma weak staramd_dedup_last_error
// and the inflation of the tool mode's input on the device (k_inflate.hip, sah_set_inflate_device)
#pragma weak staramd_inflate_host_file
#pragma weak staramd_inflate_free
#pragma weak staramd_inflate_last_error
// and the insertion of added reference sequences (index_gpu.hip, sah_set_seq_insert_fn): a run with --genomeFastaFiles there ends with the text that says so
#pragma weak staramd_seq_insert

namespace {
typedef std::chrono::steady_clock Clock;
inline double since(Clock::time_point t) { return std::chrono::duration<double>(Clock::now() - t).count(); }

struct Msg { int slot = -1; int n = 0; uint64_t seq = 0; staramd_batch b; bool merged = false; };
struct Queue {                                   // hand-off between two pipeline stages
    std::mutex m; std::condition_variable cv; std::deque<Msg> q; bool closed = false;
    void push(const Msg &x) { { std::lock_guard<std::mutex> l(m); q.push_back(x); } cv.notify_all(); }
    void close() { { std::lock_guard<std::mutex> l(m); closed = true; } cv.notify_all(); }
    bool pop(Msg &x) { std::unique_lock<std::mutex> l(m); cv.wait(l, [&] { return !q.empty() || closed; }); if (q.empty()) return false; x = q.front(); q.pop_front(); return true; }
    void reopen() { std::lock_guard<std::mutex> l(m); closed = false; q.clear(); }      // for the next phase
    bool peek(Msg &x) { std::lock_guard<std::mutex> l(m); if (q.empty()) return false; x = q.front(); return true; }          // what the next pop would hand out, if anything is waiting
};
struct Tokens {                                  // counting semaphore over a small set of buffer indices
    std::mutex m; std::condition_variable cv; std::deque<int> free;
    // the slot that was given back LAST is handed out first: a batch then lands in buffers (line tables, page-locked numeric arrays, result arrays) that were in use a
    // moment ago, and a slot is used for the first time (page faults and hipHostMalloc inside the reader) only when the pipeline really is that deep.  Round-robin order
    // went round all slots whatever the depth: 4.94 / 5.56 M pairs/s against 6.84 / 6.19 with the host stages alone on a GPU box (profiles/r04_host_stages_on_the_gpu_box.txt)
    int take() { std::unique_lock<std::mutex> l(m); cv.wait(l, [&] { return !free.empty(); }); int v = free.back(); free.pop_back(); return v; }
    void give(int v) { { std::lock_guard<std::mutex> l(m); free.push_back(v); } cv.notify_all(); }
};
// result arrays of a batch: page-locked (staramd_pinned_alloc), so that the engine's device-to-host copies are DMA transfers straight into them;
// resize() leaves new elements as they are (the engine overwrites what it reports)
template <class T> struct PinnedAlloc {
    typedef T value_type;
    PinnedAlloc() = default;
    template <class U> PinnedAlloc(const PinnedAlloc<U> &) {}
    // (page-locked memory is a limited resource: when the runtime has none left the array lives in ordinary memory -- the copies are then staged by the
    // runtime, nothing else changes; an exception thrown on a mapper thread would end the process)
    T *allocate(size_t n) {
        void *p = staramd_pinned_alloc((uint64_t)n * sizeof(T));
        if (p) return (T *)p;
        { const size_t bytes = n * sizeof(T); p = malloc(bytes > 0 ? bytes : 1); }
        if (!p) throw std::bad_alloc();
        { std::lock_guard<std::mutex> l(pageableMutex()); pageable().push_back(p); }
        return (T *)p;
    }
    void deallocate(T *p, size_t) {
        {
            std::lock_guard<std::mutex> l(pageableMutex());
            std::vector<void *> &v = pageable();
            for (size_t i = 0; i < v.size(); i++) if (v[i] == (void *)p) { v[i] = v.back(); v.pop_back(); free(p); return; }
        }
        staramd_pinned_free(p);
    }
    static std::vector<void *> &pageable() { static std::vector<void *> v; return v; }
    static std::mutex &pageableMutex() { static std::mutex m; return m; }
    template <class U> void construct(U *p) { ::new ((void *)p) U; }
    template <class U, class... A> void construct(U *p, A &&...a) { ::new ((void *)p) U(std::forward<A>(a)...); }
    template <class U> bool operator==(const PinnedAlloc<U> &) const { return true; }
    template <class U> bool operator!=(const PinnedAlloc<U> &) const { return false; }
};
struct ResBuf {
    std::vector<staramd_read_result, PinnedAlloc<staramd_read_result>> reads; std::vector<staramd_transcript, PinnedAlloc<staramd_transcript>> tr; std::vector<staramd_exon, PinnedAlloc<staramd_exon>> ex; staramd_results res;
    // what the batches of this run have needed per read so far (x 1024): a slot that is used for the first time starts there instead of learning it by an overflow of its own
    // (--chimSegmentMin returns every transcript of every window: 32 per pair, 2 GB of page-locked memory per slot)
    static std::atomic<uint64_t> &seenTr() { static std::atomic<uint64_t> v(0); return v; }
    static std::atomic<uint64_t> &seenEx() { static std::atomic<uint64_t> v(0); return v; }
    static void learn(uint64_t nReads, uint64_t trCount, uint64_t exCount) {
        if (!nReads) return;
        const uint64_t t = trCount * 1024 / nReads + 1, e = exCount * 1024 / nReads + 1;
        for (uint64_t o = seenTr().load(); o < t && !seenTr().compare_exchange_weak(o, t); ) {}
        for (uint64_t o = seenEx().load(); o < e && !seenEx().compare_exchange_weak(o, e); ) {}
    }
    void size(uint64_t nReads) {
        if (reads.size() < nReads) reads.resize(nReads);
        const uint64_t wantTr = std::max<uint64_t>(nReads * 4 + 4096, nReads * seenTr().load() / 1024 * 5 / 4 + 4096);
        if (tr.size() < wantTr) { tr.resize(wantTr); ex.resize(std::max<uint64_t>(tr.size() * 3, nReads * seenEx().load() / 1024 * 5 / 4 + 4096)); }
        memset(&res, 0, sizeof(res));
        point();
    }
    void point() { res.reads = reads.data(); res.tr = tr.data(); res.trCapacity = tr.size(); res.ex = ex.data(); res.exCapacity = ex.size(); }
};

// CLI-level flags that never reach the host library: --gpuDevices a,b,c   --benchWarmupReads N
struct CliFlags { std::vector<int> devices; uint64_t warmupReads = 0; std::vector<char *> rest; };
CliFlags splitFlags(int argc, char **argv) {
    CliFlags f;
    for (int i = 0; i < argc; i++) {
        std::string a = argv[i];
        if (a == "--gpuDevices" && i + 1 < argc) {
            std::string v = argv[++i]; size_t p = 0;
            while (p <= v.size()) { size_t q = v.find(',', p); if (q == std::string::npos) q = v.size(); if (q > p) f.devices.push_back(atoi(v.substr(p, q - p).c_str())); p = q + 1; }
        } else if (a == "--benchWarmupReads" && i + 1 < argc) f.warmupReads = strtoull(argv[++i], nullptr, 10);
        else f.rest.push_back(argv[i]);
    }
    return f;
}

// STARAMD_PIPELINE_LOG=<file>: one line per batch and stage (stage, batch number, start and end in ms since the run's first batch) -- where a batch waited and for what
struct PipeLog {
    std::mutex m; std::vector<std::array<double, 4> > ev; const char *path = getenv("STARAMD_PIPELINE_LOG"); std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double now() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
    void add(int stage, uint64_t seq, double a, double b) { if (!path) return; std::lock_guard<std::mutex> l(m); ev.push_back({(double)stage, (double)seq, a, b}); }
    void dump() {
        if (!path) return;
        FILE *f = fopen(path, "w"); if (!f) return;
        static const char *names[] = {"fill", "convert", "map", "emit"};
        std::sort(ev.begin(), ev.end(), [](const std::array<double, 4> &x, const std::array<double, 4> &y) { return x[2] < y[2]; });
        for (auto &e : ev) fprintf(f, "%-8s %4.0f %10.2f %10.2f %8.2f\n", names[(int)e[0]], e[1], e[2], e[3], e[3] - e[2]);
        fclose(f);
    }
};
// thread CPU of one batch's work on a stage thread (sah_cpu_seconds; the helper threads of a stage count their own).  The host library's CpuScope, restated over
// sah_cpu_add: this file sees the host library through its C interface only
struct StageCpu {
    int stage; timespec t0;
    explicit StageCpu(int st) : stage(st) { clock_gettime(CLOCK_THREAD_CPUTIME_ID, &t0); }
    ~StageCpu() { timespec t1; clock_gettime(CLOCK_THREAD_CPUTIME_ID, &t1); sah_cpu_add(stage, (uint64_t)((t1.tv_sec - t0.tv_sec) * 1000000000ll + (t1.tv_nsec - t0.tv_nsec))); }
};
// fn(d) for every d in [0, n), each on a thread of its own (engine calls that block on their device; no stage counts their CPU)
template <class F> void onEachDevice(size_t n, F fn) { std::vector<std::thread> th; for (size_t d = 0; d < n; d++) th.emplace_back(fn, d); for (auto &t : th) t.join(); }

// One process per GPU on a node: every rank reads the ~30 GB index into host memory before it uploads it, and keeps only ~5 GB of it afterwards
// (sah_engines_ready).  STARAMD_INDEX_LOAD_LOCK=<file> makes the ranks take turns (an advisory file lock from here until the engine contexts hold
// the index), so that the peak is one index + a few GB per rank instead of one index per rank -- which a container limit does not survive.
struct LoadLock {
    int fd = -1; ~LoadLock() { drop(); }
    void take() { if (const char *p = getenv("STARAMD_INDEX_LOAD_LOCK")) { fd = open(p, O_CREAT | O_RDWR, 0666); if (fd >= 0 && flock(fd, LOCK_EX) != 0) { close(fd); fd = -1; } } }
    void drop() { if (fd >= 0) { flock(fd, LOCK_UN); close(fd); fd = -1; } }
};
struct Host { void *h; ~Host() { if (h) sah_destroy(h); } };      // the host object (runner.cpp), released on every way out

// --runMode genomeGenerate: suffix array + SAindex on the device, between the two halves of the host's part
int generateGenome(void *h, const CliFlags &flags) {
    const uint8_t *G; uint64_t nGenome, saCap, saiCap; uint32_t gsb, nb; uint8_t *SA, *SAi;
    if (sah_generate_buffers(h, &G, &nGenome, &gsb, &nb, &SA, &saCap, &SAi, &saiCap)) { fprintf(stderr, "\n%s\n", sah_error(h)); return 104; }
    staramd_index_params ip; memset(&ip, 0, sizeof(ip));
    ip.nGenome = nGenome; ip.GstrandBit = gsb; ip.gSAindexNbases = nb; ip.gSAsparseD = 1;
    staramd_index_result ir;
    auto tg = Clock::now();
    int grc = staramd_index_build(flags.devices.empty() ? sah_device(h) : flags.devices[0], G, &ip, SA, saCap, SAi, saiCap, &ir);
    if (grc) { fprintf(stderr, "\nEXITING because of FATAL ERROR: index build on the MI355X failed: %s\n", staramd_index_last_error()); return 105; }
    double sBuild = since(tg);
    if (sah_generate_finish(h, ir.nSA, ir.nSAbyte, ir.nSAibyte)) { fprintf(stderr, "\n%s\n", sah_error(h)); return 104; }
    fprintf(stderr, "star_amd: genomeGenerate: %llu suffixes, %u doubling rounds, device build %.3f s (%.1f ms on the stream), junction insertion + files %.3f s\n",
            (unsigned long long)ir.nSA, ir.doublingRounds, sBuild, ir.msTotal, since(tg) - sBuild);
    return 0;
}

// ---- what the run holds on the devices: engine contexts, the resident-insertion hook, the BGZF compressor.  Released together, on every way out.
// Every entry of --gpuDevices is an OWNER: a context with an index replica of its own, uploaded concurrently.  Every owner
// gets STARAMD_CONTEXTS_PER_GPU - 1 (default: 1) further contexts that share its resident index (staramd_create_shared: work space and stream of
// their own, no second replica); each context has a mapper thread, so a GPU always has a second batch in flight while the results of one are
// copied out and handed on (the reference: runThreadN workers over one shared genome, STAR.cpp:194-201)
struct Engines {
    void *const h;
    std::vector<int> devices;
    int nOwners = 0, nDev = 0;                      // contexts = mapper threads; context d belongs to owner d % nOwners
    std::vector<staramd_ctx *> ctx, owners;         // index changes go to the owners; the contexts that share an index follow
    staramd_bgzf *bgzf = nullptr;                   // --gpuBAMcompression Device: one compressor on the first device, installed as the host library's hook for the length of the run
    staramd_bamsort *bamsort = nullptr;             // --gpuBAMsort Device: the sorter of Aligned.sortedByCoord.out.bam beside it (it works with the compressor's stream and kernels)
    explicit Engines(void *h) : h(h) {}
    ~Engines() { release(); }
    void release() {
        sah_set_sjdb_resident_fn(nullptr, nullptr);
        for (int d = (int)ctx.size() - 1; d >= 0; d--) if (ctx[d]) { staramd_destroy(ctx[d]); ctx[d] = nullptr; }      // sharers before their owners
        if (bamsort) { sah_set_bamsort_device(nullptr, nullptr); staramd_bamsort_destroy(bamsort); bamsort = nullptr; }
        if (bgzf) { sah_set_bgzf_device_fn(nullptr, nullptr); staramd_bgzf_destroy(bgzf); bgzf = nullptr; }
    }
    // 0, or the exit code of the run
    int create(const CliFlags &flags, uint64_t batchReads, staramd_cli_report &rep) {
        devices = flags.devices;
        if (devices.empty()) devices.push_back(sah_device(h));
        if (devices.size() > STARAMD_CLI_MAX_DEV) { fprintf(stderr, "\nEXITING because of fatal PARAMETERS error: --gpuDevices lists more than %d devices\n", STARAMD_CLI_MAX_DEV); return 104; }
        nOwners = (int)devices.size();
        // engine contexts (= mapper threads) per GPU.  A second context over the same resident index was worth +7 % in round 3, when kernels were slower and the host had 64 threads;
        // with the kernels of round 4 and the 16 CPUs the GPU boxes really give a container, one context is as fast on a quiet box (6.8 M pairs/s either way) and faster on a
        // loaded one (5.7 vs 5.1): the launches of two contexts do not overlap, they stretch each other (profiles/r04_timeline_two_contexts.txt)
        int perGpu = 1; if (const char *e = getenv("STARAMD_CONTEXTS_PER_GPU")) perGpu = std::max(1, atoi(e));
        while (nOwners * perGpu > STARAMD_CLI_MAX_DEV) perGpu--;
        nDev = nOwners * perGpu;
        rep.nDevices = nOwners; rep.nContexts = nDev; rep.genomeLoadSeconds = sah_genome_load_seconds(h);
        // chimeric detection: the partner loop on the device when the engine can (the stand-ins of the CPU tests cannot) -- STARAMD_CHIM_ON_DEVICE=0: every transcript of every
        // window comes back and the loop runs here, as in rounds 1 - 5
        if ((staramd_capabilities() & STARAMD_CAP_CHIM_SELECT) && !(getenv("STARAMD_CHIM_ON_DEVICE") && atoi(getenv("STARAMD_CHIM_ON_DEVICE")) == 0)) { if (sah_chim_select_on_device(h) && getenv("STARAMD_VERBOSE")) fprintf(stderr, "star_amd: partner of chimeric detection chosen on the device (resultSelect 2)\n"); }
        ctx.assign(nDev, nullptr);
        auto tu = Clock::now();
        std::vector<int> rcs(nDev, 0); std::vector<std::string> es(nDev);
        onEachDevice(nOwners, [&](size_t d) { rcs[d] = staramd_create(&ctx[d], devices[d], sah_genome(h), sah_params(h), (uint32_t)batchReads, 0); if (rcs[d]) es[d] = staramd_last_error(); });
        for (int d = nOwners; d < nDev; d++) if (!rcs[d % nOwners]) { rcs[d] = staramd_create_shared(&ctx[d], ctx[d % nOwners], (uint32_t)batchReads, 0); if (rcs[d]) es[d] = staramd_last_error(); }
        for (int d = 0; d < nDev; d++) if (rcs[d]) { fprintf(stderr, "\nEXITING because of FATAL ERROR: cannot initialise the MI355X engine on device %d: %s\n", devices[d % nOwners], es[d].c_str()); return 105; }
        rep.indexUploadSeconds = since(tu);
        const bool sortDev = sah_bamsort_on_device(h) && staramd_bamsort_create && staramd_bamsort_append && staramd_bamsort_download && staramd_bamsort_finish && staramd_bamsort_destroy && staramd_bamsort_last_error;
        if ((sah_bgzf_on_device(h) || sortDev) && staramd_bgzf_create && staramd_bgzf_compress && staramd_bgzf_destroy && staramd_bgzf_last_error) {
            if (staramd_bgzf_create(&bgzf, devices[0], 0)) { fprintf(stderr, "\nEXITING because of FATAL ERROR: cannot initialise the BGZF compressor on device %d: %s\n", devices[0], staramd_bgzf_last_error()); return 105; }
            if (sah_bgzf_on_device(h)) sah_set_bgzf_device_fn(staramd_bgzf_compress, bgzf);
        }
        if (sortDev && bgzf) {
            if (staramd_bamsort_create(&bamsort, bgzf, sah_bamsort_budget(h))) { fprintf(stderr, "\nEXITING because of FATAL ERROR: cannot initialise the BAM sorter on device %d: %s\n", devices[0], staramd_bamsort_last_error()); return 105; }
            static const sah_bamsort_fns fns = {staramd_bamsort_append, staramd_bamsort_download, staramd_bamsort_finish, staramd_bamsort_last_error};
            sah_set_bamsort_device(&fns, bamsort);
        }
        owners.assign(ctx.begin(), ctx.begin() + nOwners);
#ifndef STARAMD_NO_RESIDENT_SJDB
        installResidentInsertion();
#endif
        return 0;
    }
#ifndef STARAMD_NO_RESIDENT_SJDB
    // junction insertion between the passes runs on the arrays resident in HBM, on every owner (no host copy of the new SA unless it is to be saved)
    void installResidentInsertion() {
        // ... provided every device has the room for it (the work space of the insertion is several times the suffix array): asked ONCE, here, because the host copy of
        // the suffix array is released below and nothing could insert without it afterwards.  Without the room: host buffers (staramd_sjdb_insert) + re-upload.
        bool residentFits = true;
        for (int d = 0; d < nOwners; d++) if (!staramd_insert_junctions_fits(ctx[d], (uint64_t)sah_limit_sjdb_insert(h), (uint32_t)sah_sjdb_length(h))) residentFits = false;
        if (!residentFits && (sah_in_pass1(h) || getenv("STARAMD_VERBOSE"))) fprintf(stderr, "star_amd: not enough free device memory to insert junctions into the resident index: the suffix array stays on the host, insertion goes through host buffers\n");
        if (!residentFits || getenv("STARAMD_SJDB_HOST") || getenv("STARAMD_SJDB_NO_RESIDENT")) return;
        sah_set_sjdb_resident_fn([](void *user, const staramd_sjdb_args *a, staramd_sjdb_result *res) -> int {
            std::vector<staramd_ctx *> &cx = *(std::vector<staramd_ctx *> *)user;
            std::vector<int> rcs(cx.size(), 0); std::vector<staramd_sjdb_result> rs(cx.size()); std::vector<std::string> es(cx.size());
            // (the engine keeps its last error per calling thread: the text is taken on the thread that made the call)
            onEachDevice(cx.size(), [&](size_t d) { rcs[d] = staramd_insert_junctions(cx[d], a, d == 0 ? a->SAout : nullptr, a->saOutCapacity, d == 0 ? a->SAiOut : nullptr, a->saiOutCapacity, &rs[d]); if (rcs[d]) es[d] = staramd_last_error(); });
            for (size_t d = 0; d < cx.size(); d++) if (rcs[d]) { fprintf(stderr, "star_amd: junction insertion on device context %zu failed: %s\n", d, es[d].c_str()); return rcs[d]; }
            *res = rs[0];
            return 0;
        }, &owners);
        sah_engines_ready(h);
    }
#endif
};

// ---- the pipeline of one run: filler -> converter -> mappers (one per context) -> writer, batch slots going round.  The stage threads live for one phase
// (mapAllBatches); the buffers, the timing state and the failure live for the run.
struct Pipeline {
    void *const h; const staramd_cli_hooks *const hooks; Engines &eng; const uint64_t batchReads, warmupReads; staramd_cli_report &rep;
    int nSlots;
    std::vector<ResBuf> rb, rbMerged, rbWasp;        // result arrays per slot: the batch, its merged mates, its allele-swapped reads
    std::vector<ResBuf> piecePart;                   // per mapper: one piece of a WASP batch
    std::string failure; std::mutex failM; std::atomic<bool> failed{false};
    void fail(const std::string &s) { std::lock_guard<std::mutex> l(failM); if (failure.empty()) failure = s; failed = true; }
    // ---- timing state
    PipeLog plog;
    std::mutex statM;
    uint64_t nReads = 0; double msDeviceAll = 0;
    bool timedOn, warmupPending;
    Clock::time_point tTimed, t0;
    // warm-up pause: the filler stops after >= warmupReads reads, waits until every batch handed out so far is written
    std::mutex drainM; std::condition_variable drainCv; uint64_t seqParsed = 0, seqEmitted = 0;
    // ---- hand-offs between the stages of a phase
    Tokens slots; Queue filled, parsed;
    std::mutex doneM; std::condition_variable doneCv; std::map<uint64_t, Msg> done; bool mappersClosed = false;      // mapped batches by number: the writer takes them in input order

    Pipeline(void *h, const staramd_cli_hooks *hooks, Engines &eng, uint64_t batchReads, uint64_t warmupReads, staramd_cli_report &rep)
        : h(h), hooks(hooks), eng(eng), batchReads(batchReads), warmupReads(warmupReads), rep(rep), timedOn(warmupReads == 0), warmupPending(warmupReads > 0) {
        // in flight: one batch in each half of the reader, one per mapper, one in the writer, the rest queued between them.  Three more than the stages hold: the reader's time per
        // batch scatters (25 - 80 ms for 400 k pairs on a shared host) around a mean well under the device's 52 ms, and with a queue of one a single slow block left the GPU
        // idle for 25 - 30 ms every few batches (rocprofv3 timeline, profiles/r04_timeline_*.txt)
        int extraSlots = 3; if (const char *e = getenv("STARAMD_EXTRA_SLOTS")) extraSlots = std::max(0, atoi(e));
        nSlots = std::min(24, 2 * eng.nDev + 3 + extraSlots);
        ResBuf::seenTr().store(0); ResBuf::seenEx().store(0);          // (what an earlier run in this process learned -- another data set, other flags -- does not size this one's arrays)
        rb = std::vector<ResBuf>(nSlots); rbMerged = std::vector<ResBuf>(nSlots); rbWasp = std::vector<ResBuf>(nSlots); piecePart = std::vector<ResBuf>(eng.nDev);
        for (auto &r : rb) r.size(batchReads);
        tTimed = t0 = Clock::now();
    }

    // the filler reads the text of batch k+1 and finds its lines (everything that touches the input) while the converter turns the text of batch k into the
    // numeric batch (sah_fill_slot / sah_convert_slot; tools/host_bench.py: the two halves take about the same time, and their sum was the longest
    // stage of the pipeline at the thread budget of an 8-GPU node)
    void filler() {
        uint64_t seq = 0, readsOut = 0;
        for (;;) {
            if (warmupPending && readsOut >= warmupReads) {            // drain, barrier, start the clock
                { std::unique_lock<std::mutex> l(drainM); drainCv.wait(l, [&] { return seqEmitted == seqParsed || failed.load(); }); }
                if (hooks && hooks->warmup_done) hooks->warmup_done(hooks->user);
                std::lock_guard<std::mutex> l(statM);
                warmupPending = false; timedOn = true; tTimed = Clock::now();
                { double z[8]; sah_cpu_seconds(z, 1); }
            }
            Msg m; m.slot = slots.take();
            if (failed.load()) { slots.give(m.slot); break; }
            auto tp = Clock::now();
            { StageCpu sc(0); const double a = plog.now(); m.n = sah_fill_slot(h, m.slot, batchReads); plog.add(0, seq, a, plog.now()); }
            if (m.n < 0) { fail(sah_error(h)); slots.give(m.slot); break; }
            if (m.n == 0) { slots.give(m.slot); break; }
            { std::lock_guard<std::mutex> l(statM); if (timedOn) rep.parseBusy += since(tp); }
            m.seq = seq++; readsOut += (uint64_t)m.n;
            { std::lock_guard<std::mutex> l(drainM); seqParsed = seq; }
            filled.push(m);
        }
        filled.close();
    }
    void converter() {
        Msg m;
        while (filled.pop(m)) {
            auto tp = Clock::now();
            { StageCpu sc(1); const double a = plog.now(); if (!failed.load() && sah_convert_slot(h, m.slot, &m.b) < 0) fail(sah_error(h)); plog.add(1, m.seq, a, plog.now()); }
            if (failed.load()) m.n = 0;                                      // still goes down the pipeline so that the slot and the sequence number are released
            // a slot on its first way down the pipeline gets result arrays of the size the batches before it needed, here, beside the kernels of the batch ahead -- not on
            // the mapper thread between two launches (page-locked memory: ~0.1 s per GB)
            if (m.n > 0 && rb[m.slot].tr.size() < (uint64_t)m.n * ResBuf::seenTr().load() / 1024) rb[m.slot].size((uint64_t)m.n);
            { std::lock_guard<std::mutex> l(statM); if (timedOn && m.n > 0) rep.convertBusy += since(tp); }
            parsed.push(m);
        }
        parsed.close();
    }
    // what one batch cost on its context, summed over the batches mapped for it (the batch, merged mates, WASP pieces)
    struct MapCost { double msDev = 0; float stage[8] = {0}; uint64_t cnt[64] = {0}; };
    // one batch through context d into r, with one retry when the result arrays were too small
    int mapInto(int d, const staramd_batch &bt, ResBuf &r, bool main, MapCost &cost) {
        staramd_ctx *const cx = eng.ctx[d];
        if (r.reads.size() < bt.nReads || r.tr.empty() || r.tr.size() < bt.nReads * ResBuf::seenTr().load() / 1024) r.size(std::max<uint64_t>(bt.nReads, 1024));
        staramd_results &res = r.res;
        int e = staramd_map_batch(cx, &bt, &res);
        if (e == STARAMD_ERR_RESULT_OVERFLOW) {          // more transcripts than the buffers hold -> grow and ask again (the results are resident: the engine copies them, nothing is mapped twice)
            ResBuf::learn(bt.nReads, res.trCount, res.exCount);
            r.tr.resize(res.trCount + res.trCount / 4 + 4096); r.ex.resize(res.exCount + res.exCount / 4 + 4096); r.point();
            e = staramd_map_batch(cx, &bt, &res);
        }
        if (e) return e;
        ResBuf::learn(bt.nReads, res.trCount, res.exCount);
        cost.msDev += res.msTotalDevice;
        if (main) { float s[8] = {0}; int k = staramd_get_timings(cx, s, 8); for (int i = 0; i < k; i++) cost.stage[i] += s[i]; uint64_t c[64] = {0}; int kc = staramd_get_counters(cx, c, 64); for (int i = 0; i < kc; i++) cost.cnt[i] += c[i]; }
        return 0;
    }
    // the nw allele-swapped reads of a batch (can be more than the batch itself: a read over a dense cluster of SNVs has up to 1023 copies) in as many pieces as it
    // takes; every piece is rebased to offset 0 (the engine sizes and uploads a batch by readOffset[nReads]); the results of the pieces are appended to one set
    int mapWaspPieces(int d, const staramd_batch &wb, uint32_t nw, ResBuf &r, MapCost &cost) {
        ResBuf &part = piecePart[d];
        if (r.reads.size() < (size_t)nw) { r.reads.resize((size_t)nw); }
        uint64_t trN = 0, exN = 0; std::vector<uint64_t> off;
        for (uint32_t doneN = 0; doneN < nw; ) {
            staramd_batch piece = wb; piece.nReads = std::min<uint32_t>((uint32_t)batchReads, nw - doneN);
            const uint64_t base = wb.readOffset[doneN];
            off.resize(piece.nReads + 1);
            for (uint32_t k = 0; k <= piece.nReads; k++) off[k] = wb.readOffset[doneN + k] - base;
            piece.bases = wb.bases + base; piece.readOffset = off.data(); piece.mate1Length = wb.mate1Length + doneN; piece.mmMaxTotal = wb.mmMaxTotal + doneN;
            if (int rc = mapInto(d, piece, part, false, cost)) return rc;
            const staramd_results &pr = part.res;
            if (r.tr.size() < trN + pr.trCount) r.tr.resize((trN + pr.trCount) * 3 / 2 + 1024);
            if (r.ex.size() < exN + pr.exCount) r.ex.resize((exN + pr.exCount) * 3 / 2 + 1024);
            for (uint32_t k = 0; k < piece.nReads; k++) { r.reads[doneN + k] = pr.reads[k]; r.reads[doneN + k].trOffset += (uint32_t)trN; }
            for (uint64_t k = 0; k < pr.trCount; k++) { r.tr[trN + k] = pr.tr[k]; r.tr[trN + k].exonOffset += (uint32_t)exN; }
            if (pr.exCount) memcpy(&r.ex[exN], pr.ex, pr.exCount * sizeof(staramd_exon));
            trN += pr.trCount; exN += pr.exCount; doneN += piece.nReads;
        }
        r.point(); r.res.trCount = trN; r.res.exCount = exN;
        return 0;
    }
    // the batch of m, then what is mapped beside it, on context d; the engine's error code (a failure of the host side is reported through fail())
    int mapBatch(int d, Msg &m, MapCost &cost) {
        m.merged = false;
        if (int rc = mapInto(d, m.b, rb[m.slot], true, cost)) return rc;
        staramd_batch mb;                                        // --peOverlapNbasesMin: the overlapping mates of the batch, merged into single reads, are a second batch
        if (sah_merged_slot(h, m.slot, &mb) > 0) { m.merged = true; if (int rc = mapInto(d, mb, rbMerged[m.slot], false, cost)) return rc; }
        staramd_batch wb;                                        // --waspOutputMode: allele-swapped copies of some reads, one more batch
        const int nw = sah_wasp_slot(h, m.slot, &rb[m.slot].res, &wb);
        if (nw > 0) if (int rc = mapWaspPieces(d, wb, (uint32_t)nw, rbWasp[m.slot], cost)) return rc;
        if (sah_wasp_results_slot(h, m.slot, &rb[m.slot].res, nw > 0 ? &rbWasp[m.slot].res : nullptr)) fail(sah_error(h));
        return 0;
    }
    void mapper(int d) {
        Msg m;
        while (parsed.pop(m)) {
            StageCpu sc(2); const double ma = plog.now();
            if (!failed.load()) {
                auto tm = Clock::now(); MapCost cost;
                // the batch that is next in line (if the reader is ahead, as it normally is) starts its upload now, beside the kernels of this one.  Only with ONE
                // mapper: with several, another mapper may pop the batch that was peeked here, and this context would keep a stale upload
                { Msg nx; if (eng.nDev == 1 && parsed.peek(nx) && nx.n > 0) (void)staramd_prefetch_batch(eng.ctx[d], &nx.b); }
                const int rc = mapBatch(d, m, cost);
                if (rc) fail(std::string("EXITING because of FATAL ERROR in the MI355X engine: ") + staramd_last_error());
                std::lock_guard<std::mutex> l(statM);
                msDeviceAll += cost.msDev;
                if (timedOn && !rc) { rep.deviceBusy[d] += since(tm); rep.deviceMs[d] += cost.msDev; for (int i = 0; i < 8; i++) rep.stageMs[i] += cost.stage[i]; for (int i = 0; i < 64; i++) rep.counters[i] += cost.cnt[i]; }
            }
            if (failed.load()) m.n = 0;                              // still goes through the writer so that the slot and the sequence number are released
            plog.add(2, m.seq, ma, plog.now());
            { std::lock_guard<std::mutex> l(doneM); done[m.seq] = m; }
            doneCv.notify_all();
        }
    }
    void writer() {
        uint64_t next = 0;
        for (;;) {
            Msg m;
            {
                std::unique_lock<std::mutex> l(doneM);
                doneCv.wait(l, [&] { return done.count(next) || mappersClosed; });
                auto it = done.find(next);
                if (it == done.end()) { if (mappersClosed) break; continue; }
                m = it->second; done.erase(it);
            }
            next++;
            auto te = Clock::now();
            StageCpu sc(3); const double ea = plog.now();
            if (!failed.load() && m.n > 0 && (m.merged ? sah_emit_slot_merged(h, m.slot, &rb[m.slot].res, &rbMerged[m.slot].res) : sah_emit_slot(h, m.slot, &rb[m.slot].res))) fail(sah_error(h));
            { std::lock_guard<std::mutex> l(statM); if (timedOn && m.n > 0) { rep.emitBusy += since(te); rep.timedReads += (uint64_t)m.n; rep.batches++; } if (m.n > 0) nReads += (uint64_t)m.n; }
            plog.add(3, m.seq, ea, plog.now());
            slots.give(m.slot);
            { std::lock_guard<std::mutex> l(drainM); seqEmitted = next; }
            drainCv.notify_all();
        }
    }
    // one phase: every batch of the input through the four stages
    void mapAllBatches() {
        slots.free.clear(); for (int i = 0; i < nSlots; i++) slots.give(i);
        filled.reopen(); parsed.reopen(); done.clear(); mappersClosed = false;
        { std::lock_guard<std::mutex> l(drainM); seqParsed = seqEmitted = 0; }
        std::thread fillerT([this] { filler(); }), converterT([this] { converter(); }), writerT([this] { writer(); });
        std::vector<std::thread> mappers;
        for (int d = 0; d < eng.nDev; d++) mappers.emplace_back([this, d] { mapper(d); });
        for (auto &t : mappers) t.join();
        { std::lock_guard<std::mutex> l(doneM); mappersClosed = true; }
        doneCv.notify_all();
        drainCv.notify_all();
        fillerT.join(); converterT.join(); writerT.join();
    }
    // between two phases (sah_next_phase): plain run = one phase; --twopassMode Basic adds a 1st pass without SAM, after which the junctions it found
    // are inserted into the index (sjdb_insert.cpp) and every HBM copy is replaced (twoPassRunPass1.cpp:9-96);
    // --outFilterType BySJout adds a 2nd stage over the held reads with the filtered novel junctions as a whitelist (STAR.cpp:203-220).
    // true: the engines are ready for the next phase; false: the run is over (or failed)
    bool phaseStep() {
        if (failed.load()) return false;
        // the phase that follows is known only after sah_next_phase; ranks exchange their tables before it
        if (hooks && hooks->exchange && hooks->exchange(hooks->user, h, 0)) { fail("cross-rank exchange failed"); return false; }
        const int phase = sah_next_phase(h);
        if (phase < 0) { fail(sah_error(h)); return false; }
        if (phase == 0) return false;
        if (phase == 1) {
            const bool inEngine = sah_index_in_engine(h) != 0;       // the insertion ran on the resident arrays: only tables and parameters are new
            std::vector<int> rcs(eng.nOwners, 0); std::vector<std::string> es(eng.nOwners);
            onEachDevice(eng.nOwners, [&](size_t d) {
                rcs[d] = inEngine ? staramd_update_tables(eng.ctx[d], sah_genome(h), sah_params(h)) : staramd_update_index(eng.ctx[d], sah_genome(h), sah_params(h));
                if (rcs[d]) es[d] = staramd_last_error(); });
            for (int d = 0; d < eng.nOwners; d++) if (rcs[d]) fail(std::string("EXITING because of FATAL ERROR: index re-upload failed: ") + es[d]);
            if (failed.load()) return false;
            rep.pass1Seconds = since(t0);
            fprintf(stderr, "star_amd: 1st pass + junction insertion + index re-upload: %.3f s (%llu reads)\n", rep.pass1Seconds, (unsigned long long)nReads);
        } else {
            const uint64_t *ns, *ne; uint64_t nn = sah_novel_junctions(h, &ns, &ne);
            for (int d = 0; d < eng.nOwners; d++) if (staramd_set_novel_junctions(eng.ctx[d], ns, ne, nn, 2)) fail(std::string("EXITING because of FATAL ERROR: ") + staramd_last_error());
            if (failed.load()) return false;
            fprintf(stderr, "star_amd: BySJout stage 1 done (%llu reads so far), %llu novel junctions passed filtering\n", (unsigned long long)nReads, (unsigned long long)nn);
        }
        return true;
    }
    // end of the run: the output files are finished, the report is filled in; the exit code
    int finish() {
        int exitCode = 0;
        if (failed.load()) { fprintf(stderr, "\n%s\n", failure.c_str()); exitCode = 104; }
        else if (hooks && hooks->exchange && hooks->exchange(hooks->user, h, 1)) { fprintf(stderr, "\ncross-rank exchange failed\n"); exitCode = 104; }
        else { const auto tf = Clock::now(); if (sah_finish(h)) { fprintf(stderr, "\n%s\n", sah_error(h)); exitCode = 104; } rep.finishSeconds = since(tf); }
        sah_emit_seconds(h, rep.emitParts);
        plog.dump();
        sah_fast_path_counts(h, rep.fastPaths);
        sah_cpu_seconds(rep.cpuSeconds, 0);
        for (int d = 0; d < eng.nDev; d++) if (eng.ctx[d]) { rep.fastPaths[2] += staramd_prefetch_hits(eng.ctx[d]); rep.fastPaths[3] += staramd_overlapped_batches(eng.ctx[d]); }
        double sec = since(t0);
        rep.reads = nReads; rep.wallMapping = sec; rep.timedWall = since(tTimed);
        if (!exitCode) fprintf(stderr, "star_amd: %llu reads, %.3f s wall in the mapping loop (%.3f s on the device) -> %.3f Mreads/s end to end, %d GPU(s)\n",
                               (unsigned long long)nReads, sec, msDeviceAll / 1e3 / eng.nDev, sec > 0 ? (double)nReads / sec / 1e6 : 0.0, eng.nOwners);
        if (!exitCode) fprintf(stderr, "star_amd: fast paths: output through a file mapping %llu batches, input from file mappings %llu, uploads prefetched %llu, kernels begun beside the copy of the results before them %llu\n",
                               (unsigned long long)rep.fastPaths[0], (unsigned long long)rep.fastPaths[1], (unsigned long long)rep.fastPaths[2], (unsigned long long)rep.fastPaths[3]);
        return exitCode;
    }
};

// --runMode inputAlignmentsFromBAM --bamRemoveDuplicatesType writes Processed.out.bam inside sah_create: with --gpuBAMcompression Device the compressor has to be
// there before it (a run that maps creates its compressor with its engines, Engines::create; the tool mode's other job, --outWigType, writes no BAM and
// gets none).  Released when the tool mode is over
struct ToolBgzf {
    staramd_bgzf *bgzf = nullptr;
    // 0, or the exit code of the run
    int create(const CliFlags &flags) {
        bool tool = false, dev = false, dedup = false, wig = false;
        for (size_t i = 0; i + 1 < flags.rest.size(); i++) {
            const std::string a = flags.rest[i], b = flags.rest[i + 1];
            if (a == "--runMode" && b == "inputAlignmentsFromBAM") tool = true;
            if (a == "--gpuBAMcompression" && b == "Device") dev = true;
            if (a == "--bamRemoveDuplicatesType" && b != "-") dedup = true;
            if (a == "--outWigType" && b != "None") wig = true;
        }
        if (!tool || !dev || !dedup || wig || !(staramd_bgzf_create && staramd_bgzf_compress && staramd_bgzf_destroy && staramd_bgzf_last_error)) return 0;
        const int device = flags.devices.empty() ? 0 : flags.devices[0];
        if (staramd_bgzf_create(&bgzf, device, 0)) { bgzf = nullptr; fprintf(stderr, "\nEXITING because of FATAL ERROR: cannot initialise the BGZF compressor on device %d: %s\n", device, staramd_bgzf_last_error()); return 105; }
        sah_set_bgzf_device_fn(staramd_bgzf_compress, bgzf);
        return 0;
    }
    ~ToolBgzf() { if (bgzf) { sah_set_bgzf_device_fn(nullptr, nullptr); staramd_bgzf_destroy(bgzf); } }
};
}

int staramd_cli_main(int argc, char **argv, const staramd_cli_hooks *hooks, staramd_cli_report *report) {
    staramd_cli_report rep; memset(&rep, 0, sizeof(rep));
    for (int i = 1; i < argc; i++) if (std::string(argv[i]) == "--version") { printf("2.7.11b\n"); return 0; }      // the version whose behaviour is reproduced (Parameters.cpp:340-343)
    CliFlags flags = splitFlags(argc, argv);
    if (!getenv("STARAMD_SJDB_HOST")) sah_set_sjdb_device_fn(staramd_sjdb_insert, flags.devices.empty() ? 0 : flags.devices[0]);   // junction insertion on the device
    if (staramd_seq_insert) sah_set_seq_insert_fn(staramd_seq_insert, flags.devices.empty() ? 0 : flags.devices[0]);      // --genomeFastaFiles at the mapping stage; before sah_create, where the index is loaded
    if (staramd_signal_host_records && staramd_bamsort_finish_signal && staramd_signal_free && staramd_signal_last_error) {      // --gpuSignal Device; before sah_create, where the tool mode runs
        static const sah_signal_fns fns = {staramd_signal_host_records, staramd_bamsort_finish_signal, staramd_signal_free, staramd_signal_last_error};
        sah_set_signal_device(&fns);
    }
    if (staramd_dedup_host_records && staramd_dedup_free && staramd_dedup_last_error) {      // --gpuBAMdedup Device; likewise before sah_create
        static const sah_dedup_fns fns = {staramd_dedup_host_records, staramd_dedup_free, staramd_dedup_last_error};
        sah_set_dedup_device(&fns);
    }
    if (staramd_inflate_host_file && staramd_inflate_free && staramd_inflate_last_error) {      // --gpuBAMinflate Device; likewise
        static const sah_inflate_fns fns = {staramd_inflate_host_file, staramd_inflate_free, staramd_inflate_last_error};
        sah_set_inflate_device(&fns);
    }
    ToolBgzf toolBgzf;
    if (const int rc = toolBgzf.create(flags)) return rc;
    LoadLock loadLock;
    loadLock.take();
    sah_set_batch_alloc(staramd_pinned_alloc, staramd_pinned_free);      // batch arrays in page-locked memory: the uploads are DMA transfers
    char err[4096];
    Host host{sah_create((int)flags.rest.size(), flags.rest.data(), err, sizeof(err))};
    void *const h = host.h;
    if (!h) { fprintf(stderr, "\n%s\n", err); return 104; }
    if (sah_tool_done(h)) return 0;                              // --runMode inputAlignmentsFromBAM: nothing to map
    if (sah_generate_mode(h)) return generateGenome(h, flags);
    Engines eng(h);
    if (const int rc = eng.create(flags, sah_batch_reads(h), rep)) return rc;
    loadLock.drop();
    Pipeline pipe(h, hooks, eng, sah_batch_reads(h), flags.warmupReads, rep);
    do pipe.mapAllBatches(); while (pipe.phaseStep());
    const int exitCode = pipe.finish();
    eng.release();                                               // (the contexts go before the page-locked result arrays of the pipeline)
    if (report) *report = rep;
    return exitCode;
}
