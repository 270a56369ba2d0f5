// bam_sorted.cpp -- CoordSortedBam, the one owner of Aligned.sortedByCoord.out.bam (host.h says what it holds), with the hook of the device sorter
// (--gpuBAMsort Device, include/star_amd_bamsort.h) and appendLog, which the end of a run shares with it.
#include "host.h"
#include <cstdarg>
#include <cstddef>
#include <cstdlib>

namespace staramd {

void appendLog(const std::string &path, const char *fmt, ...) {
    if (FILE *lo = fopen(path.c_str(), "ab")) { va_list ap; va_start(ap, fmt); vfprintf(lo, fmt, ap); va_end(ap); fclose(lo); }
}

static sah_bamsort_fns g_sortFns = sah_bamsort_fns();
static staramd_bamsort *g_sorter = nullptr;
const char *const BAMSORT_DEVICE_MISSING = "EXITING because of fatal PARAMETERS error: --gpuBAMsort Device, but no device sorter is installed (sah_set_bamsort_device)";
void setBamsortDevice(const sah_bamsort_fns *fns, staramd_bamsort *sorter) { g_sortFns = fns ? *fns : sah_bamsort_fns(); g_sorter = fns ? sorter : nullptr; }
bool bamsortDeviceInstalled() { return g_sortFns.append && g_sortFns.download && g_sortFns.finish && g_sortFns.last_error; }
static std::string sorterError() { return deviceError("--gpuBAMsort", g_sortFns.last_error()); }
static_assert(sizeof(BamKey) == 32 && offsetof(BamKey, off) == 16 && offsetof(BamKey, len) == 24, "BamKey is handed to the sorter as staramd_bam_key");

std::string CoordSortedBam::take(const RunParams &P, std::vector<BamKey> &rangeKeys, std::string &raw) {
    if (rangeKeys.empty()) return "";
    const uint32_t chunk = (uint32_t)chunks.size();
    for (BamKey &k : rangeKeys) k.chunk = chunk;
    if (onDevice(P)) {                                          // the records into device memory, only the keys stay here
        const int rc = g_sortFns.append(g_sorter, (const uint8_t *)raw.data(), raw.size(), (const staramd_bam_key *)rangeKeys.data(), (uint32_t)rangeKeys.size());
        if (rc < 0) return sorterError();
        if (rc == 0) { keys.insert(keys.end(), rangeKeys.begin(), rangeKeys.end()); chunks.emplace_back(); appendBytes.push_back(raw.size()); appendsTaken++; return ""; }
        const std::string e = spill(P);                         // it took nothing: this range and the rest of the run go the Host way
        if (!e.empty()) return e;
    }
    keys.insert(keys.end(), rangeKeys.begin(), rangeKeys.end());
    if (P.outBAMunsorted) chunks.emplace_back(raw); else chunks.emplace_back(std::move(raw));
    return "";
}

std::string CoordSortedBam::spill(const RunParams &P) {
    for (size_t i = 0; i < appendBytes.size(); i++) {
        chunks[i].resize(appendBytes[i]);
        if (g_sortFns.download(g_sorter, (uint32_t)i, (uint8_t *)&chunks[i][0])) return sorterError();
    }
    if (g_sortFns.finish(g_sorter, 0, nullptr, nullptr, nullptr)) return sorterError();
    spilled = true;
    appendLog(P.outFileNamePrefix + "Log.out", "--gpuBAMsort Device: the records no longer fit the sorter's budget of device memory after %zu appends; they were brought back and the coordinate sort runs on the host\n", appendBytes.size());
    return "";
}

void CoordSortedBam::abandon(const RunParams &P) { if (onDevice(P) && !appendBytes.empty() && bamsortDeviceInstalled()) (void)g_sortFns.finish(g_sorter, 0, nullptr, nullptr, nullptr); }

static uint64_t nsSince(std::chrono::steady_clock::time_point t0) { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(); }

// --gpuBAMsort Device: ordered, laid out and deflated where the records are; the members come back in order and go to f.  sig (--gpuSignal Device): the
// same finish also computes the tracks where the records lie, after the order is known; the Signal.* files are written from its runs before f is closed
static std::string finishOnDevice(CoordSortedBam &s, const RunParams &P, const GenomeIndex &gi, FILE *f, const sah_signal_fns *sig) {
    int (*put)(void *, const uint8_t *, uint64_t) = [](void *u, const uint8_t *b, uint64_t n) -> int { return fwrite(b, 1, n, (FILE *)u) == n ? 0 : 1; };
    uint64_t st[8] = {0};
    SignalDeviceParams sp; staramd_signal_result sres = staramd_signal_result();
    if (sig) sp.set(P, gi.realChrNames(), gi.realChrLengths());
    const int rc = sig ? sig->finish_signal(g_sorter, P.outBAMcompression, put, f, st, &sp.abi, &sres) : g_sortFns.finish(g_sorter, P.outBAMcompression, put, f, st);
    if (rc) return sig ? deviceError("--gpuSignal", sig->last_error()) : sorterError();
    s.sortCounts[0] = st[0]; s.sortCounts[1] = st[1];
    appendLog(P.outFileNamePrefix + "Log.out", "--gpuBAMsort Device: %llu records, %llu bytes of %zu appends ordered on the device\n", (unsigned long long)st[0], (unsigned long long)st[1], s.appendBytes.size());
    if (!sig) return "";
    const auto t0 = std::chrono::steady_clock::now();
    const std::string werr = signalFromRuns(P, gi.realChrNames(), gi.realChrLengths(), P.outFileNamePrefix + "Signal", sres);
    const uint64_t nsDev = sres.stats[4] + sres.stats[5] + sres.stats[6] + sres.stats[7];
    s.signalCounts[0] = 1; s.signalCounts[1] = sres.stats[0]; s.signalCounts[2] = sres.stats[1]; s.signalCounts[3] = sres.stats[3];
    s.signalCounts[4] = nsDev + nsSince(t0);
    s.signalCounts[5] = sres.stats[4]; s.signalCounts[6] = sres.stats[5]; s.signalCounts[7] = sres.stats[6];
    if (getenv("STARAMD_HOST_TIMING")) fprintf(stderr, "  signal stage (device): %.2f ms, of which on the device %.2f ms; %llu bytes of runs\n", s.signalCounts[4] / 1e6, nsDev / 1e6, (unsigned long long)sres.stats[3]);
    appendLog(P.outFileNamePrefix + "Log.out", "--gpuSignal Device: %llu records, %llu spans in %llu tiles, %llu bytes of runs from the device\n", (unsigned long long)sres.stats[0], (unsigned long long)sres.stats[1], (unsigned long long)sres.stats[2], (unsigned long long)sres.stats[3]);
    sig->free_result(&sres);
    return werr;
}

// the Host way: all records of the run are in memory, ordered once (ord: indices into keys) and compressed on the host threads, slice by slice
static std::string sortAndCompress(const CoordSortedBam &s, const RunParams &P, FILE *f, const std::string &path, std::vector<uint64_t> &ord) {
    const std::vector<BamKey> &K = s.keys;
    ord.resize(K.size());
    for (uint64_t i = 0; i < ord.size(); i++) ord[i] = i;
    std::sort(ord.begin(), ord.end(), [&K](uint64_t a, uint64_t b) { return K[a].g != K[b].g ? K[a].g < K[b].g : K[a].r != K[b].r ? K[a].r < K[b].r : a < b; });
    const uint64_t n = ord.size();
    const uint64_t T = (uint64_t)std::max(1, std::min(P.runThreadN, 64));
    const uint64_t per = std::max<uint64_t>(4096, (n + 4 * T - 1) / (4 * T));          // records per slice; slices are written in order
    bool failed = false;
    const bool dev = P.gpuBAMdevice;                          // --gpuBAMcompression Device: the slices of one round in one hook call
    for (uint64_t base = 0; base < n && !failed; base += per * T) {
        std::vector<std::string> outS(T), raws(dev ? T : 0);
        onThreads(T, CPU_NONE, [&](size_t t) {
            uint64_t lo = std::min(n, base + t * per), hi = std::min(n, lo + per);
            std::string raw;
            for (uint64_t i = lo; i < hi; i++) { const BamKey &k = K[ord[i]]; raw.append(s.chunks[k.chunk], k.off, k.len); }
            if (dev) raws[t].swap(raw);
            else if (!bgzfCompress(raw, P.outBAMcompression, outS[t])) failed = true;
        });
        if (dev) {
            std::vector<BgzfJob> jobs;
            for (uint64_t t = 0; t < T; t++) jobs.push_back({&raws[t], &outS[t], P.outBAMcompression});
            const std::string devErr = bgzfCompressDevice(jobs, P.runThreadN);
            if (!devErr.empty()) return devErr;
        }
        for (uint64_t t = 0; t < T; t++) if (!outS[t].empty() && fwrite(outS[t].data(), 1, outS[t].size(), f) != outS[t].size()) failed = true;
    }
    return failed ? "EXITING because of fatal ERROR: could not write " + path : "";
}

// STAR.cpp:275-283: signal tracks from the sorted alignments
static std::string signalOnHost(CoordSortedBam &s, const RunParams &P, const GenomeIndex &gi, const std::vector<uint64_t> &ord) {
    const uint64_t n = ord.size();
    std::vector<const char *> recs(n);
    for (uint64_t i = 0; i < n; i++) { const BamKey &k = s.keys[ord[i]]; recs[i] = s.chunks[k.chunk].data() + k.off; }
    if (P.gpuSignalDevice)                                  // (the run spilled: its records are here, not on the device)
        appendLog(P.outFileNamePrefix + "Log.out", "--gpuSignal Device: the sorted records are on the host; the signal tracks are computed on the host\n");
    const auto t0 = std::chrono::steady_clock::now();
    const std::string werr = writeSignal(P, gi.realChrNames(), gi.realChrLengths(), P.outFileNamePrefix + "Signal", recs);
    s.signalCounts[1] = n; s.signalCounts[4] = nsSince(t0);
    if (getenv("STARAMD_HOST_TIMING")) fprintf(stderr, "  signal stage (host): %.2f ms\n", s.signalCounts[4] / 1e6);
    return werr;
}

std::string CoordSortedBam::write(const RunParams &P, const GenomeIndex &gi, const std::string &header) {
    const std::string path = P.outFileNamePrefix + "Aligned.sortedByCoord.out.bam";
    const bool toStdout = P.outStd == "BAM_SortedByCoordinate";
    FILE *f = toStdout ? stdout : fopen(path.c_str(), "wb");
    if (!f) return "EXITING because of fatal ERROR: could not create output file " + path;
    const bool device = onDevice(P), sigDevice = device && P.wig.yes && P.gpuSignalDevice;
    const sah_signal_fns *sig = sigDevice ? signalDeviceFns() : nullptr;
    std::string h, err;
    std::vector<uint64_t> ord;
    if (!bgzfCompress(header, P.outBAMcompression, h)) err = "EXITING because of fatal ERROR: BGZF compression failed";
    else {                                                      // the header goes out before a missing hook ends the run, as it always did
        fwrite(h.data(), 1, h.size(), f);
        if (device && !bamsortDeviceInstalled()) err = BAMSORT_DEVICE_MISSING;
        else if (sigDevice && !sig) err = SIGNAL_DEVICE_MISSING;
        else if (!device && P.gpuBAMdevice && !keys.empty() && !bgzfDeviceInstalled()) err = BGZF_DEVICE_MISSING;
    }
    const bool ran = err.empty();                               // (a run that ends on a missing hook keeps its appends: abandon() empties the sorter)
    if (ran) {
        err = device ? finishOnDevice(*this, P, gi, f, sig) : sortAndCompress(*this, P, f, path, ord);
        std::string e; bgzfEof(e); fwrite(e.data(), 1, e.size(), f);
    }
    if (toStdout) fflush(stdout); else fclose(f);
    if (err.empty() && !device && P.wig.yes) err = signalOnHost(*this, P, gi, ord);
    if (ran) { chunks.clear(); keys.clear(); appendBytes.clear(); }
    return err;
}

} // namespace staramd
