// dedup.cpp -- --runMode inputAlignmentsFromBAM --bamRemoveDuplicatesType UniqueIdentical | UniqueIdenticalNotMulti [--bamRemoveDuplicatesMate2basesN n]:
// duplicate read pairs of a coordinate-sorted paired-end BAM are marked (flag 0x400) and the file is written again as Processed.out.bam.
//   bamRemoveDuplicates     source/bamRemoveDuplicates.cpp:114-271, called from Parameters.cpp:594-599
// The reference walks groups of overlapping pairs; for input in which every unique record has its one partner on its reference sequence the groups do
// not matter and the rule is per pair: key, class, survivor.  dedupOnHost is that rule in plain C++ -- it needs no GPU and is what the
// tests pin to the reference; --gpuBAMdedup Device computes the same bytes on the MI355X (include/star_amd_dedup.h).  Both read a record through
// ../dedup_rule.h, so what a malformed record gives is the same on both paths.
#include "host.h"
#include "../dedup_rule.h"
#include <cstring>
#include <cstdlib>
#include <atomic>

namespace staramd {

static sah_dedup_fns g_dedupFns = {nullptr, nullptr, nullptr};
void setDedupDeviceFns(const sah_dedup_fns *fns) { if (fns) g_dedupFns = *fns; else g_dedupFns = {nullptr, nullptr, nullptr}; }
const sah_dedup_fns *dedupDeviceFns() { return g_dedupFns.host_records && g_dedupFns.free_result && g_dedupFns.last_error ? &g_dedupFns : nullptr; }

namespace {
inline uint32_t rd32(const char *p) { uint32_t v; memcpy(&v, p, 4); return v; }
struct Rec { const uint8_t *p; uint64_t len; DedupCore c; uint32_t startS; int32_t as; bool hasAS, unique; };
struct Pair { uint64_t m1, m2, hi, lo; };
}

bool dedupOnHost(const std::vector<const char *> &recs, bool markMulti, uint32_t N, staramd_dedup_result &out) {
    memset(&out, 0, sizeof(out));
    const uint64_t n = recs.size();
    out.nRecords = n; out.stats[0] = n;
    if (n == 0) return true;
    out.dup = (uint8_t *)calloc(n, 1);
    if (!out.dup) return false;
    // ---- every record: its kind and the bit it ends with unless a class decides otherwise (step 1)
    std::vector<Rec> R(n);
    std::vector<uint64_t> uniq;
    for (uint64_t i = 0; i < n; i++) {
        Rec &r = R[i];
        r.p = (const uint8_t *)recs[i]; r.len = 4 + (uint64_t)rd32(recs[i]);
        r.c = dedupCore(r.p, r.len);
        uint32_t nh = 0, as = 0;
        const uint32_t got = r.c.ok ? bamAuxInts(r.p, r.c.lim, dedupAuxStart(r.c), 'N', 'H', nh, true, 'A', 'S', as) : 0;
        if (!(got & 1)) { if (!out.fatal) { out.fatal = 1; out.fatalRecord = i; } continue; }
        r.hasAS = (got & 2) != 0; r.as = (int32_t)as; r.unique = (int32_t)nh == 1;
        r.startS = dedupStartS(r.p, r.c);
        out.dup[i] = (uint8_t)(r.c.flag >> 10 & 1);
        if (r.unique) { out.dup[i] = 0; uniq.push_back(i); }
        else if ((int32_t)nh > 1 && markMulti) out.dup[i] = 1;
    }
    if (out.fatal) return true;
    out.stats[1] = uniq.size();
    // ---- pairs: the unique records of one reference sequence that share a name, when they are exactly a mate 1 and a mate 2 (step 2)
    auto nameCmp = [&](uint64_t a, uint64_t b) { return dedupNameCmp(R[a].p, R[a].c, R[b].p, R[b].c); };
    std::sort(uniq.begin(), uniq.end(), [&](uint64_t a, uint64_t b) {
        if (R[a].c.tid != R[b].c.tid) return R[a].c.tid < R[b].c.tid;
        const int r = nameCmp(a, b);
        return r ? r < 0 : a < b;
    });
    std::vector<Pair> pairs;
    for (size_t j = 0; j < uniq.size();) {
        size_t e = j + 1;
        while (e < uniq.size() && R[uniq[e]].c.tid == R[uniq[j]].c.tid && nameCmp(uniq[e], uniq[j]) == 0) e++;
        if (e - j == 2 && ((R[uniq[j]].c.flag ^ R[uniq[j + 1]].c.flag) & 0x80)) {
            const uint64_t a = uniq[j], b = uniq[j + 1], m1 = (R[a].c.flag & 0x80) ? b : a, m2 = (R[a].c.flag & 0x80) ? a : b;
            if (!R[m1].hasAS && (!out.fatal || m1 < out.fatalRecord)) { out.fatal = 2; out.fatalRecord = m1; }
            pairs.push_back({m1, m2, dedupKeyHi(R[m1].c.tid, R[m1].startS), dedupKeyLo(R[m2].startS, R[m1].c.flag, R[m2].c.flag)});
        }
        j = e;
    }
    if (out.fatal) return true;
    out.stats[2] = pairs.size(); out.stats[5] = uniq.size() - 2 * pairs.size();
    // ---- classes of equal key (step 3); the survivor of each: the largest AS of mate 1, then the smallest name (step 4); everyone else is marked (step 5)
    auto content = [&](const Pair &a, const Pair &b) { return dedupContentCmp(R[a.m1].p, R[a.m1].len, R[a.m2].p, R[a.m2].len, R[b.m1].p, R[b.m1].len, R[b.m2].p, R[b.m2].len, N); };
    std::sort(pairs.begin(), pairs.end(), [&](const Pair &a, const Pair &b) {
        if (a.hi != b.hi) return a.hi < b.hi;
        if (a.lo != b.lo) return a.lo < b.lo;
        return content(a, b) < 0;
    });
    for (size_t j = 0; j < pairs.size();) {
        size_t e = j + 1, best = j;
        while (e < pairs.size() && pairs[e].hi == pairs[j].hi && pairs[e].lo == pairs[j].lo && content(pairs[e], pairs[j]) == 0) {
            const int32_t x = R[pairs[e].m1].as, y = R[pairs[best].m1].as;
            if (x > y || (x == y && nameCmp(pairs[e].m1, pairs[best].m1) < 0)) best = e;
            e++;
        }
        for (size_t k = j; k < e; k++) if (k != best) out.dup[pairs[k].m1] = out.dup[pairs[k].m2] = 1;
        out.stats[3]++;
        j = e;
    }
    for (uint64_t i = 0; i < n; i++) out.stats[4] += out.dup[i];
    return true;
}

static const char *fatalText(int fatal) {
    return fatal == 1 ? "EXITING because of fatal ERROR: SAM tag NH is missing from a read, but it's required for deduplication. \nSOLUTION: re-generate BAM file with NH and AS tags."
                      : "EXITING because of fatal ERROR: SAM tag AS is missing from a read, but it's required for deduplication. \nSOLUTION: re-generate BAM file with NH and AS tags.";
}

std::string dedupFromBamFile(const RunParams &P, const std::string &bamPath, const std::string &outPath, uint64_t counts[8]) {
    BamFileInMemory bam;
    const auto t0 = std::chrono::steady_clock::now();
    auto msSince = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); };
    std::string err = bam.load(P, bamPath);
    if (!err.empty()) return err;
    const double msLoad = msSince(t0);
    const auto t1 = std::chrono::steady_clock::now();
    const bool markMulti = P.bamRemoveDuplicatesType == "UniqueIdentical";
    const sah_dedup_fns *fns = nullptr;
    staramd_dedup_result res;
    if (P.gpuDedupDevice) {                                         // --gpuBAMdedup Device: the inflated records go to the device as they are; n bytes come back
        if (!(fns = dedupDeviceFns())) return DEDUP_DEVICE_MISSING;
        std::vector<uint64_t> offsets(bam.recs.size());
        for (size_t i = 0; i < bam.recs.size(); i++) offsets[i] = (uint64_t)(bam.recs[i] - bam.d.data());
        const staramd_dedup_params dp = {markMulti ? 1 : 0, P.bamRemoveDuplicatesMate2basesN};
        if (fns->host_records(P.gpuDevice, &dp, (const uint8_t *)bam.d.data(), bam.d.size(), offsets.data(), offsets.size(), &res)) return deviceError("--gpuBAMdedup", fns->last_error());
    } else if (!dedupOnHost(bam.recs, markMulti, P.bamRemoveDuplicatesMate2basesN, res)) return "EXITING because of fatal ERROR: not enough memory for marking duplicates";
    auto release = [&]() { if (fns) fns->free_result(&res); else { free(res.dup); res.dup = nullptr; } };
    if (const int fatal = res.fatal) { release(); return fatalText(fatal); }      // (nothing was written yet: no partial Processed.out.bam)
    for (int i = 0; i < 8; i++) counts[i] = res.stats[i];
    for (size_t i = 0; i < bam.recs.size(); i++) {
        char *w = const_cast<char *>(bam.recs[i]) + 16;
        if (4 + (size_t)rd32(bam.recs[i]) < 20) continue;           // (a record without a flag word)
        uint32_t fnc = rd32(w);
        fnc = res.dup[i] ? fnc | 0x400u << 16 : fnc & ~(0x400u << 16);
        memcpy(w, &fnc, 4);
    }
    release();
    const double msMark = msSince(t1);
    const auto t2 = std::chrono::steady_clock::now();
    // ---- the file: the header as read, then the records in the input's order, BGZF at --outBAMcompression on --runThreadN threads (or through the
    // installed device compressor, --gpuBAMcompression Device), the EOF marker; header block and marker are host-written, as everywhere else
    const bool dev = P.gpuBAMdevice;
    const size_t end = bam.recs.empty() ? bam.headerEnd : (size_t)(bam.recs.back() - bam.d.data()) + 4 + rd32(bam.recs.back());
    if (dev && end > bam.headerEnd && !bgzfDeviceInstalled()) return BGZF_DEVICE_MISSING;
    FILE *f = fopen(outPath.c_str(), "wb");
    if (!f) return "EXITING because of fatal ERROR: could not create output file " + outPath;
    std::atomic<bool> failed(false);                            // (set by the compressing threads too)
    std::string h;
    if (!bgzfCompress(std::string(bam.d.data(), bam.headerEnd), P.outBAMcompression, h) || fwrite(h.data(), 1, h.size(), f) != h.size()) failed = true;
    const size_t T = (size_t)std::max(1, std::min(P.runThreadN, 64)), SLICE = 64 * 0xff00;        // whole BGZF members per slice
    for (size_t base = bam.headerEnd; base < end && !failed && err.empty(); base += SLICE * T) {
        std::vector<std::string> outS(T), raws(T);
        onThreads(T, CPU_NONE, [&](size_t t) {
            const size_t lo = std::min(end, base + t * SLICE), hi = std::min(end, lo + SLICE);
            raws[t].assign(bam.d.data() + lo, hi - lo);
            if (!dev && !bgzfCompress(raws[t], P.outBAMcompression, outS[t])) failed = true;
        });
        if (dev) {
            std::vector<BgzfJob> jobs;
            for (size_t t = 0; t < T; t++) jobs.push_back({&raws[t], &outS[t], P.outBAMcompression});
            err = bgzfCompressDevice(jobs, P.runThreadN);
        }
        for (size_t t = 0; t < T && err.empty(); t++) if (!outS[t].empty() && fwrite(outS[t].data(), 1, outS[t].size(), f) != outS[t].size()) failed = true;
    }
    std::string e; bgzfEof(e);
    if (fwrite(e.data(), 1, e.size(), f) != e.size()) failed = true;
    fclose(f);
    if (failed && err.empty()) err = "EXITING because of fatal ERROR: could not write " + outPath;
    if (!err.empty()) { remove(outPath.c_str()); return err; }
    if (getenv("STARAMD_HOST_TIMING"))
        fprintf(stderr, "  dedup stage (%s): load and inflate %.2f ms, mark %.2f ms, compress and write %.2f ms\n", P.gpuDedupDevice ? "device" : "host", msLoad, msMark, msSince(t2));
    appendLog(P.outFileNamePrefix + "Log.out", "--bamRemoveDuplicatesType %s on the %s (--gpuBAMdedup): %llu records, %llu pairs, %llu classes, %llu records marked, %llu unpaired unique records\n",
              P.bamRemoveDuplicatesType.c_str(), P.gpuDedupDevice ? "Device" : "Host", (unsigned long long)counts[0], (unsigned long long)counts[2], (unsigned long long)counts[3],
              (unsigned long long)counts[4], (unsigned long long)counts[5]);
    return "";
}

} // namespace staramd
