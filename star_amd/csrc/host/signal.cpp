// signal.cpp -- --outWigType bedGraph | wiggle [read1_5p | read2], --outWigStrand, --outWigNorm, --outWigReferencesPrefix: read coverage ("signal")
// from the coordinate-sorted alignments, written at the end of an alignReads run as Signal.{Unique,UniqueMultiple}.str{1,2}.out.{bg,wig}.
//   signalFromBAM     source/signalFromBAM.cpp:5-209   (the reference re-reads its sorted BAM; here the sorted records are still in memory)
// --gpuSignal Device: the values are computed on the MI355X (include/star_amd_signal.h) and come back as runs; signalFromRuns writes the same files from them.
#include "host.h"
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <zlib.h>

namespace staramd {

namespace {
inline uint32_t rd32(const char *p) { uint32_t v; memcpy(&v, p, 4); return v; }

// integer value of an attribute of a BAM record (bam_aux_get + bam_aux2i); false when the tag is absent
bool auxInt(const char *rec, const char tag[2], int64_t &val) {
    const uint32_t recSize = rd32(rec), bmn = rd32(rec + 12), fnc = rd32(rec + 16), lseq = rd32(rec + 20);
    const char *a = rec + 36 + (bmn & 0xff) + 4 * (size_t)(fnc & 0xffff) + (lseq + 1) / 2 + lseq, *end = rec + 4 + recSize;
    while (a + 3 <= end) {
        const char t = a[2]; const bool hit = a[0] == tag[0] && a[1] == tag[1];
        a += 3;
        size_t w;
        switch (t) {
            case 'A': case 'c': case 'C': w = 1; break;
            case 's': case 'S': w = 2; break;
            case 'i': case 'I': case 'f': w = 4; break;
            case 'Z': case 'H': w = strlen(a) + 1; break;
            case 'B': { const char bt = a[0]; const uint32_t n = rd32(a + 1); w = 5 + (size_t)n * (bt == 'c' || bt == 'C' ? 1 : bt == 's' || bt == 'S' ? 2 : 4); break; }
            default: return false;
        }
        if (hit) {
            if (t == 'c') val = (int8_t)a[0]; else if (t == 'C') val = (uint8_t)a[0];
            else if (t == 's') { int16_t v; memcpy(&v, a, 2); val = v; } else if (t == 'S') { uint16_t v; memcpy(&v, a, 2); val = v; }
            else if (t == 'i') { int32_t v; memcpy(&v, a, 4); val = v; } else if (t == 'I') { uint32_t v; memcpy(&v, a, 4); val = v; }
            else val = 0;
            return true;
        }
        a += w;
    }
    return false;
}
}

std::string writeSignal(const RunParams &P, const std::vector<std::string> &chrName, const std::vector<uint64_t> &chrLength, const std::string &sigFileName, const std::vector<const char *> &recs) {
    const WigParams &W = P.wig;
    auto wanted = [&](int32_t tid) { return W.referencesPrefix.empty() || chrName[tid].compare(0, W.referencesPrefix.size(), W.referencesPrefix) == 0; };
    double nMult = 0, nUniq = 0;
    if (W.norm == 1) {
        for (const char *rec : recs) {
            const int32_t tid = (int32_t)rd32(rec + 4);
            if (tid < 0 || !wanted(tid)) continue;
            int64_t nh;
            if (auxInt(rec, "NH", nh)) { if ((uint32_t)nh == 1) ++nUniq; else if ((uint32_t)nh > 1) nMult += 1.0 / (uint32_t)nh; }
        }
    }
    const int sigN = W.strand ? 4 : 2;
    double normFactor[4] = {1, 1, 1, 1};
    std::string names[4] = {sigFileName + ".Unique.str1.out", sigFileName + ".UniqueMultiple.str1.out", sigFileName + ".Unique.str2.out", sigFileName + ".UniqueMultiple.str2.out"};
    FILE *out[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int ii = 0; ii < sigN; ii++) {
        names[ii] += W.format == 0 ? ".bg" : ".wig";
        out[ii] = fopen(names[ii].c_str(), "wb");
        if (!out[ii]) { for (int k = 0; k < ii; k++) fclose(out[k]); return "EXITING because of fatal ERROR: could not create output file " + names[ii]; }
    }
    if (W.norm == 1) { normFactor[0] = 1.0e6 / nUniq; normFactor[1] = 1.0e6 / (nUniq + nMult); }
    if (W.strand) { normFactor[2] = normFactor[0]; normFactor[3] = normFactor[1]; }
    const char *numFormat = W.norm == 1 ? "%.5f" : "%g";      // ostream default vs fixed << setprecision(5) (:64-66)
    auto num = [&](FILE *f, double v) { fprintf(f, numFormat, v); };

    int32_t iChr = -999; std::vector<double> sigAll; uint32_t chrLen = 0;
    auto flushChr = [&]() {
        if (iChr == -999) return;
        for (int is = 0; is < sigN; is++) {
            FILE *f = out[is];
            if (W.format == 1) fprintf(f, "variableStep chrom=%s\n", chrName[iChr].c_str());
            double prevSig = 0;
            for (uint32_t ig = 0; ig < chrLen; ig++) {
                const double newSig = sigAll[(size_t)sigN * ig + is];
                if (W.format == 0) {
                    if (newSig != prevSig) {
                        if (prevSig != 0) { fprintf(f, "%u\t", ig); num(f, prevSig * normFactor[is]); fputc('\n', f); }
                        if (newSig != 0) fprintf(f, "%s\t%u\t", chrName[iChr].c_str(), ig);
                        prevSig = newSig;
                    }
                } else if (newSig != 0) { fprintf(f, "%u\t", ig + 1); num(f, newSig * normFactor[is]); fputc('\n', f); }
            }
        }
    };
    for (size_t ir = 0; ir <= recs.size(); ir++) {
        const char *rec = ir < recs.size() ? recs[ir] : nullptr;
        const int32_t tid = rec ? (int32_t)rd32(rec + 4) : -1;
        if (!rec || tid != iChr) {
            flushChr();
            if (!rec) break;
            iChr = tid;
            if (iChr == -1 || !wanted(iChr)) { iChr = -999; continue; }
            chrLen = (uint32_t)chrLength[iChr] + 1;                 // one extra base at the end, always 0
            sigAll.assign((size_t)sigN * chrLen, 0.0);
        }
        if (iChr == -999) continue;
        const uint32_t bmn = rd32(rec + 12), fnc = rd32(rec + 16), flag = fnc >> 16, nCigar = fnc & 0xffff;
        if (flag & 0x400) continue;
        int64_t nh; uint32_t aNH = 1;
        if (auxInt(rec, "NH", nh)) aNH = (uint32_t)nh;
        if (aNH == 0) continue;
        uint32_t aG = rd32(rec + 8), iStrand = 0;
        if (W.strand) iStrand = ((flag & 0x10) > 0) == ((flag & 0x80) == 0);
        if (W.type == 1) {
            if (flag & 0x80) continue;
            if (iStrand == 0) { if (aNH == 1) sigAll[(size_t)aG * sigN + 0 + 2 * iStrand]++; sigAll[(size_t)aG * sigN + 1 + 2 * iStrand] += 1.0 / aNH; continue; }
        }
        const char *cigar = rec + 36 + (bmn & 0xff);
        for (uint32_t ic = 0; ic < nCigar; ic++) {
            const uint32_t c = rd32(cigar + 4 * ic), op = c & 0xf, len = c >> 4;
            if (op == 2 || op == 3) aG += len;
            else if (op == 0) {
                if (W.type == 0 || (W.type == 2 && (flag & 0x80))) {
                    for (uint32_t ig = 0; ig < len; ig++) {
                        if (aG >= chrLen) { for (int k = 0; k < sigN; k++) fclose(out[k]); return "BUG: alignment extends past chromosome in the signal output"; }
                        if (aNH == 1) sigAll[(size_t)aG * sigN + 0 + 2 * iStrand]++;
                        sigAll[(size_t)aG * sigN + 1 + 2 * iStrand] += 1.0 / aNH;
                        aG++;
                    }
                } else aG += len;
            }
        }
        if (W.type == 1) { --aG; if (aNH == 1) sigAll[(size_t)aG * sigN + 0 + 2 * iStrand]++; sigAll[(size_t)aG * sigN + 1 + 2 * iStrand] += 1.0 / aNH; }
    }
    for (int is = 0; is < sigN; is++) fclose(out[is]);
    return "";
}

// ---- --gpuSignal Device: the tracks come back from the device as runs (include/star_amd_signal.h); the functions are installed by the driver
static sah_signal_fns g_signalFns = {nullptr, nullptr, nullptr, nullptr};
void setSignalDeviceFns(const sah_signal_fns *fns) { if (fns) g_signalFns = *fns; else g_signalFns = {nullptr, nullptr, nullptr, nullptr}; }
const sah_signal_fns *signalDeviceFns() { return g_signalFns.host_records && g_signalFns.finish_signal && g_signalFns.free_result && g_signalFns.last_error ? &g_signalFns : nullptr; }

void SignalDeviceParams::set(const RunParams &P, const std::vector<std::string> &chrName, const std::vector<uint64_t> &chrLength) {
    const WigParams &W = P.wig;
    len.resize(chrName.size()); wanted.resize(chrName.size());
    for (size_t i = 0; i < chrName.size(); i++) {
        len[i] = (uint32_t)chrLength[i];
        wanted[i] = W.referencesPrefix.empty() || chrName[i].compare(0, W.referencesPrefix.size(), W.referencesPrefix) == 0;
    }
    abi = {W.type, W.strand ? 1 : 0, (uint32_t)chrName.size(), W.norm == 1, len.data(), wanted.data()};
}

// The files of writeSignal from runs: same names, same formats, same normFactor arithmetic.  A run is joined with the next of its track when they touch and
// hold the same value (a tile boundary of the device must not show in a bedGraph line); wiggle prints every position of a run
std::string signalFromRuns(const RunParams &P, const std::vector<std::string> &chrName, const std::vector<uint64_t> &chrLength, const std::string &sigFileName, const staramd_signal_result &R) {
    const WigParams &W = P.wig;
    double nMult = 0, nUniq = 0;
    if (W.norm == 1 && R.norm) for (uint64_t i = 0; i < R.nRecords; i++) { const uint32_t nh = R.norm[i]; if (nh == 1) ++nUniq; else if (nh > 1) nMult += 1.0 / nh; }      // in the records' order, as writeSignal
    const int sigN = W.strand ? 4 : 2;
    double normFactor[4] = {1, 1, 1, 1};
    std::string names[4] = {sigFileName + ".Unique.str1.out", sigFileName + ".UniqueMultiple.str1.out", sigFileName + ".Unique.str2.out", sigFileName + ".UniqueMultiple.str2.out"};
    FILE *out[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int ii = 0; ii < sigN; ii++) {
        names[ii] += W.format == 0 ? ".bg" : ".wig";
        out[ii] = fopen(names[ii].c_str(), "wb");
        if (!out[ii]) { for (int k = 0; k < ii; k++) fclose(out[k]); return "EXITING because of fatal ERROR: could not create output file " + names[ii]; }
    }
    auto closeAll = [&]() { for (int k = 0; k < sigN; k++) fclose(out[k]); };
    if (R.pastEnd) { closeAll(); return "BUG: alignment extends past chromosome in the signal output"; }
    if (W.norm == 1) { normFactor[0] = 1.0e6 / nUniq; normFactor[1] = 1.0e6 / (nUniq + nMult); }
    if (W.strand) { normFactor[2] = normFactor[0]; normFactor[3] = normFactor[1]; }
    // one line per call, writeSignal's formats put together: "%.5f" under --outWigNorm RPM, "%g" else
    const std::string num = W.norm == 1 ? "%.5f" : "%g", bgLine = "%s\t%u\t%u\t" + num + "\n", wigLine = "%u\t" + num + "\n";
    // a track is a file of its own, so the tracks are written side by side (the runs of one track are in order in the array, whatever lies between them)
    auto writeTrack = [&](int is) {
        FILE *f = out[is];
        const double nf = normFactor[is];
        uint64_t ir = 0;
        for (uint32_t tid = 0; tid < R.nChr && tid < chrName.size() && tid < chrLength.size(); tid++) {
            if (!R.chrHas[tid]) continue;
            const char *chr = chrName[tid].c_str();
            bool pending = false; uint32_t start = 0, end = 0; double value = 0;
            auto flush = [&]() {
                if (!pending) return;
                // (a run that covers the spare base behind the chromosome is never closed by writeSignal's loop over chrLength + 1 positions: the line ends after the start)
                if (end <= chrLength[tid]) fprintf(f, bgLine.c_str(), chr, start, end, value * nf); else fprintf(f, "%s\t%u\t", chr, start);
                pending = false;
            };
            if (W.format == 1) fprintf(f, "variableStep chrom=%s\n", chr);
            for (; ir < R.nRuns && R.runs[ir].tid <= (int32_t)tid; ir++) {
                const staramd_signal_run &r = R.runs[ir];
                if (r.tid != (int32_t)tid || (int)r.track != is || r.value == 0) continue;
                if (W.format == 1) { for (uint32_t ig = r.start; ig < r.end; ig++) fprintf(f, wigLine.c_str(), ig + 1, r.value * nf); continue; }
                if (pending && end == r.start && memcmp(&value, &r.value, 8) == 0) { end = r.end; continue; }
                flush();
                pending = true; start = r.start; end = r.end; value = r.value;
            }
            flush();
        }
    };
    if (P.runThreadN > 1 && R.nRuns > 100000) {
        std::vector<std::thread> th;
        for (int is = 1; is < sigN; is++) th.emplace_back(writeTrack, is);
        writeTrack(0);
        for (auto &t : th) t.join();
    } else for (int is = 0; is < sigN; is++) writeTrack(is);
    closeAll();
    return "";
}

// The input of --runMode inputAlignmentsFromBAM, for both of its jobs (the tracks below, the duplicate marking of dedup.cpp): the file is inflated block by
// block (BGZF = concatenated gzip members) and held in memory; chromosome names and lengths come from its header.
static sah_inflate_fns g_inflateFns = {nullptr, nullptr, nullptr};
void setInflateDeviceFns(const sah_inflate_fns *fns) { if (fns) g_inflateFns = *fns; else g_inflateFns = {nullptr, nullptr, nullptr}; }
const sah_inflate_fns *inflateDeviceFns() { return g_inflateFns.host_file && g_inflateFns.free_result && g_inflateFns.last_error ? &g_inflateFns : nullptr; }

std::string BamFileInMemory::inflateOnHost(const std::string &bamPath, uint64_t &nMembers, uint64_t &nIn) {
    gzFile in = gzopen(bamPath.c_str(), "rb");
    if (!in) return "EXITING because of fatal INPUT error: could not open --inputBAMfile " + bamPath;
    for (;;) {
        const size_t old = d.size(), block = 1u << 24;
        d.resize(old + block);
        int got = gzread(in, d.data() + old, (unsigned)block);
        if (got < 0) { gzclose(in); return "EXITING because of fatal INPUT error: could not decompress --inputBAMfile " + bamPath; }
        d.resize(old + (size_t)got);
        if ((size_t)got < block) break;
    }
    const z_off_t at = gzoffset(in);                            // (compressed bytes read; gzread does not count members)
    nIn = at > 0 ? (uint64_t)at : 0; nMembers = 0;
    gzclose(in);
    return "";
}
// --gpuBAMinflate Device: the file as it is goes to the installed functions, the inflated bytes come back
std::string BamFileInMemory::inflateOnDevice(const RunParams &P, const std::string &bamPath, uint64_t &nMembers, uint64_t &nIn) {
    const sah_inflate_fns *fns = inflateDeviceFns();
    if (!fns) return INFLATE_DEVICE_MISSING;
    const bool timing = getenv("STARAMD_HOST_TIMING") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    auto ms = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    std::vector<uint8_t> file;
    FILE *f = fopen(bamPath.c_str(), "rb");
    if (!f) return "EXITING because of fatal INPUT error: could not open --inputBAMfile " + bamPath;
    for (;;) {
        const size_t old = file.size(), block = 1u << 24;
        file.resize(old + block);
        const size_t got = fread(file.data() + old, 1, block, f);
        file.resize(old + got);
        if (got < block) break;
    }
    const bool readFailed = ferror(f) != 0;
    fclose(f);
    if (readFailed) return "EXITING because of fatal INPUT error: could not read --inputBAMfile " + bamPath;
    const double msRead = ms();
    staramd_inflate_result res;
    if (fns->host_file(P.gpuDevice, file.data(), file.size(), &res)) return deviceError("--gpuBAMinflate", fns->last_error());
    const double msDevice = ms() - msRead;
    nMembers = res.nMembers; nIn = file.size();
    if (res.failedMember >= 0) { fns->free_result(&res); return "EXITING because of fatal INPUT error: could not decompress --inputBAMfile " + bamPath; }
    if (res.nBytes) d.assign((const char *)res.bytes, (const char *)res.bytes + res.nBytes);
    fns->free_result(&res);
    if (timing) fprintf(stderr, "  inflate stage (device): file read %.2f ms, walk + device %.2f ms, copy into place %.2f ms\n", msRead, msDevice, ms() - msRead - msDevice);
    return "";
}

std::string BamFileInMemory::load(const RunParams &P, const std::string &bamPath) {
    uint64_t nMembers = 0, nIn = 0;
    const auto t0 = std::chrono::steady_clock::now();
    const std::string inflErr = P.gpuInflateDevice ? inflateOnDevice(P, bamPath, nMembers, nIn) : inflateOnHost(bamPath, nMembers, nIn);
    if (!inflErr.empty()) return inflErr;
    const double msInflate = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (P.gpuInflateDevice) appendLog(P.outFileNamePrefix + "Log.out", "--inputBAMfile inflated on the Device (--gpuBAMinflate): %llu members, %llu bytes in, %llu bytes out\n", (unsigned long long)nMembers, (unsigned long long)nIn, (unsigned long long)d.size());
    else appendLog(P.outFileNamePrefix + "Log.out", "--inputBAMfile inflated on the Host (--gpuBAMinflate): %llu bytes in, %llu bytes out\n", (unsigned long long)nIn, (unsigned long long)d.size());
    const auto t1 = std::chrono::steady_clock::now();
    struct ParseTime { bool on; double msInflate; std::chrono::steady_clock::time_point t1; ~ParseTime() { if (on) fprintf(stderr, "  load: inflate %.2f ms, header and record parse %.2f ms\n", msInflate, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count()); } }
        parseTime{getenv("STARAMD_HOST_TIMING") != nullptr, msInflate, t1};
    if (d.size() < 12 || memcmp(d.data(), "BAM\1", 4) != 0) return "EXITING because of fatal INPUT error: --inputBAMfile " + bamPath + " is not a BAM file";
    size_t p = 8 + rd32(d.data() + 4);
    if (p + 4 > d.size()) return "EXITING because of fatal INPUT error: truncated BAM header in " + bamPath;
    const uint32_t nRef = rd32(d.data() + p); p += 4;
    for (uint32_t i = 0; i < nRef; i++) {
        if (p + 4 > d.size()) return "EXITING because of fatal INPUT error: truncated BAM header in " + bamPath;
        const uint32_t ln = rd32(d.data() + p); p += 4;
        if (p + ln + 4 > d.size()) return "EXITING because of fatal INPUT error: truncated BAM header in " + bamPath;
        chrName.emplace_back(d.data() + p, ln ? ln - 1 : 0); p += ln;
        chrLength.push_back(rd32(d.data() + p)); p += 4;
    }
    headerEnd = p;
    while (p + 4 <= d.size()) {
        const uint32_t bs = rd32(d.data() + p);
        if (p + 4 + bs > d.size()) break;
        recs.push_back(d.data() + p);
        p += 4 + bs;
    }
    return "";
}

// --runMode inputAlignmentsFromBAM --inputBAMfile x.bam --outWigType ... (Parameters.cpp:585-592): the same tracks from a coordinate-sorted BAM file.
std::string signalFromBamFile(const RunParams &P, const std::string &bamPath, const std::string &sigFileName) {
    BamFileInMemory bam;
    const std::string loadErr = bam.load(P, bamPath);
    if (!loadErr.empty()) return loadErr;
    const std::vector<char> &d = bam.d;
    const std::vector<std::string> &chrName = bam.chrName; const std::vector<uint64_t> &chrLength = bam.chrLength;
    const std::vector<const char *> &recs = bam.recs;
    if (P.gpuSignalDevice) {                                        // --gpuSignal Device: the inflated records go to the device as they are
        const sah_signal_fns *fns = signalDeviceFns();
        if (!fns) return SIGNAL_DEVICE_MISSING;
        std::vector<uint64_t> offsets(recs.size());
        for (size_t i = 0; i < recs.size(); i++) offsets[i] = (uint64_t)(recs[i] - d.data());
        SignalDeviceParams sp; sp.set(P, chrName, chrLength);
        staramd_signal_result res;
        if (fns->host_records(P.gpuDevice, &sp.abi, (const uint8_t *)d.data(), d.size(), offsets.data(), offsets.size(), &res)) return deviceError("--gpuSignal", fns->last_error());
        std::string e = signalFromRuns(P, chrName, chrLength, sigFileName, res);
        fns->free_result(&res);
        return e;
    }
    return writeSignal(P, chrName, chrLength, sigFileName, recs);
}

} // namespace staramd
