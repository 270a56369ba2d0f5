// bgzf.cpp -- BGZF framing of the BAM byte stream (SAM/BAM specification section 4.1; the reference goes through htslib's
// bgzf_write, source/BAMoutput.cpp:60-84).  Every block is an independent gzip member of at most 0xff00 input bytes, so the
// post-map threads compress their own part of a batch and the blocks are simply concatenated in read order.
#include "host.h"
#include <zlib.h>
#include <cstring>
#include <algorithm>
#include <memory>
#include <thread>

namespace staramd {

static const size_t BGZF_INPUT_MAX = 0xff00;

static bool oneBlock(const uint8_t *in, size_t n, int level, std::string &out) {
    uint8_t buf[0x10000 + 64];
    z_stream zs; memset(&zs, 0, sizeof(zs));
    if (deflateInit2(&zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
    zs.next_in = const_cast<uint8_t *>(in); zs.avail_in = (uInt)n;
    zs.next_out = buf + 18; zs.avail_out = sizeof(buf) - 18 - 8;
    int rc = deflate(&zs, Z_FINISH);
    if (rc != Z_STREAM_END) { deflateEnd(&zs); return false; }
    size_t clen = zs.total_out;
    deflateEnd(&zs);
    size_t total = 18 + clen + 8;
    if (total > 0x10000) return false;
    static const uint8_t hdr[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    memcpy(buf, hdr, 16);
    buf[16] = (uint8_t)((total - 1) & 0xff); buf[17] = (uint8_t)((total - 1) >> 8);
    uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), in, (uInt)n), isize = (uint32_t)n;
    memcpy(buf + 18 + clen, &crc, 4); memcpy(buf + 18 + clen + 4, &isize, 4);
    out.append((const char *)buf, total);
    return true;
}

// compress `raw` into BGZF blocks appended to `out`; returns false on a zlib failure
bool bgzfCompress(const std::string &raw, int level, std::string &out) {
    for (size_t off = 0; off < raw.size(); off += BGZF_INPUT_MAX) {
        size_t n = std::min(BGZF_INPUT_MAX, raw.size() - off);
        // level 0 output can exceed the block limit for a full block: fall back to two halves
        if (!oneBlock((const uint8_t *)raw.data() + off, n, level, out)) {
            size_t h = n / 2;
            if (!oneBlock((const uint8_t *)raw.data() + off, h, level, out) || !oneBlock((const uint8_t *)raw.data() + off + h, n - h, level, out)) return false;
        }
    }
    return true;
}

// ---- --gpuBAMcompression Device: the same members cut on the MI355X (include/star_amd_bgzf.h), through a hook the driver installs
static BgzfDeviceFn g_bgzfFn = nullptr;
static void *g_bgzfUser = nullptr;
const char *const BGZF_DEVICE_MISSING = "EXITING because of fatal PARAMETERS error: --gpuBAMcompression Device, but no device BGZF compressor is installed (sah_set_bgzf_device_fn)";
void setBgzfDeviceFn(BgzfDeviceFn fn, void *user) { g_bgzfFn = fn; g_bgzfUser = user; }
bool bgzfDeviceInstalled() { return g_bgzfFn != nullptr; }

std::string bgzfCompressDevice(const std::vector<BgzfJob> &jobs, int threads) {
    if (!g_bgzfFn) return BGZF_DEVICE_MISSING;
    std::vector<int> levels;
    for (const BgzfJob &j : jobs) if (std::find(levels.begin(), levels.end(), j.level) == levels.end()) levels.push_back(j.level);
    for (int level : levels) {
        std::vector<const uint8_t *> in; std::vector<uint64_t> len; std::vector<std::string *> outs;
        uint64_t cap = 0;
        for (const BgzfJob &j : jobs) {
            if (j.level != level || j.in->empty()) continue;
            in.push_back((const uint8_t *)j.in->data()); len.push_back(j.in->size()); outs.push_back(j.out);
            cap += j.in->size() + 31 * ((j.in->size() + BGZF_INPUT_MAX - 1) / BGZF_INPUT_MAX);     // staramd_bgzf_bound
        }
        if (in.empty()) continue;
        // one output buffer per thread, kept between batches (uninitialised: only what the device returns is touched)
        static thread_local std::unique_ptr<uint8_t[]> buf; static thread_local uint64_t bufCap = 0;
        if (bufCap < cap) { bufCap = cap + cap / 4; buf.reset(new uint8_t[bufCap]); }
        std::vector<uint64_t> outLen(in.size()), at(in.size() + 1, 0);
        if (g_bgzfFn(g_bgzfUser, level, (uint32_t)in.size(), in.data(), len.data(), buf.get(), cap, outLen.data()) != 0) return "EXITING because of fatal ERROR: BGZF compression failed";
        for (size_t i = 0; i < in.size(); i++) at[i + 1] = at[i] + outLen[i];
        const char *base = (const char *)buf.get();          // (the helper threads have thread_local buffers of their own)
        overItems((size_t)std::max(1, std::min(threads, 8)), CPU_NONE, outs.size(), [&](size_t i) { outs[i]->append(base + at[i], outLen[i]); });
    }
    return "";
}

// the 28-byte end-of-file marker block
void bgzfEof(std::string &out) {
    static const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    out.append((const char *)eof, 28);
}

} // namespace staramd
