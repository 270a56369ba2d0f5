// inflate_bounds_check.cpp -- TEST INFRASTRUCTURE (tests/test_inflate_bounds.py): k_inflate.hip taken into this translation unit through the wavefront
// emulator's headers and compiled with -fsanitize=address,undefined, as a program of its own.  Every member's compressed bytes and its output lie in heap
// blocks of their exact sizes, so a read past csize or a write past isize is a sanitizer report.
//   usage: inflate_bounds_check <members file> <mutations> <seed>
//   members file (written by the Python test from tests/inflate_vectors.py), per member: u32 csize, isize, crc, expected status, then csize bytes
// Every member of the file runs as it is: the status must be the expected one and, where that is 0, the output zlib's.  Then `mutations` seeded mutations
// of the well-formed members (bit flips, truncations, a member spliced onto another): each must end with a status, or with exactly what zlib makes of
// the same bytes.  Every run's trip count must stay within 8 * csize + isize.  Exit code 0 and "clean" when all of that holds.
#include "../star_amd/csrc/engine/k_inflate.hip"
#include <zlib.h>
#include <random>

namespace {
struct Case { std::vector<uint8_t> in; uint32_t isize, crc, want; };

uint32_t rdU32(FILE *f, bool &ok) { uint8_t b[4]; ok = fread(b, 1, 4, f) == 4; return ok ? rd32(b) : 0; }

// zlib's reading of a raw deflate stream that has to fill exactly isize bytes and end exactly at the end of the input
bool zlibInflates(const std::vector<uint8_t> &in, uint32_t isize, std::vector<uint8_t> &out) {
    z_stream z; memset(&z, 0, sizeof(z));
    if (inflateInit2(&z, -15) != Z_OK) return false;
    out.assign((size_t)isize + 1, 0);
    uint8_t none = 0;
    z.next_in = in.empty() ? &none : const_cast<uint8_t *>(in.data()); z.avail_in = (uInt)in.size();
    z.next_out = out.data(); z.avail_out = (uInt)out.size();
    const int rc = inflate(&z, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && z.total_out == isize && z.avail_in == 0;
    inflateEnd(&z);
    out.resize(isize);
    return ok;
}

struct Run { uint32_t status, trips; std::vector<uint8_t> out; };
// one member through the kernel, with blocks of the exact sizes (new[] of 0 bytes is a block of its own: any access to it is reported)
Run runMember(const std::vector<uint8_t> &in, uint32_t isize, uint32_t crc) {
    uint8_t *dIn = new uint8_t[in.size()], *dOut = new uint8_t[isize];
    if (!in.empty()) memcpy(dIn, in.data(), in.size());
    if (isize) memset(dOut, 0xA5, isize);
    Member *tab = new Member[1];
    tab[0].in = 0; tab[0].out = 0; tab[0].csize = (uint32_t)in.size(); tab[0].isize = isize; tab[0].crc = crc; tab[0].pad = 0;
    uint32_t *status = new uint32_t[1], *trips = new uint32_t[1];
    status[0] = 0xffffffffu; trips[0] = 0xffffffffu;
    hipLaunchKernelGGL(k_inflate_members, dim3(1), dim3(NT), 0, 0, (const uint8_t *)dIn, (const Member *)tab, 1u, dOut, status, trips);
    Run r{status[0], trips[0], std::vector<uint8_t>(dOut, dOut + isize)};
    delete[] dIn; delete[] dOut; delete[] tab; delete[] status; delete[] trips;
    return r;
}
}  // namespace

int main(int argc, char **argv) {
    if (argc != 4) { fprintf(stderr, "usage: inflate_bounds_check <members file> <mutations> <seed>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<Case> cases;
    for (;;) {
        bool ok; Case c;
        const uint32_t csize = rdU32(f, ok);
        if (!ok) break;
        c.isize = rdU32(f, ok); c.crc = rdU32(f, ok); c.want = rdU32(f, ok);
        c.in.resize(csize);
        if (!ok || (csize && fread(c.in.data(), 1, csize, f) != csize)) { fprintf(stderr, "short members file\n"); return 2; }
        cases.push_back(std::move(c));
    }
    fclose(f);
    unsigned long bad = 0, nOk = 0, nRejected = 0, maxTrips = 0;
    auto tripsOk = [&](const Run &r, size_t csize, uint32_t isize, const char *what, size_t i) {
        if (r.trips > maxTrips) maxTrips = r.trips;
        if ((uint64_t)r.trips > 8ull * csize + isize) { fprintf(stderr, "%s %zu: %u trips, more than 8 * %zu + %u\n", what, i, r.trips, csize, isize); bad++; }
    };
    std::vector<size_t> good;
    std::vector<uint8_t> want;
    for (size_t i = 0; i < cases.size(); i++) {
        const Case &c = cases[i];
        const Run r = runMember(c.in, c.isize, c.crc);
        tripsOk(r, c.in.size(), c.isize, "member", i);
        if (r.status != c.want) { fprintf(stderr, "member %zu: status %u, expected %u\n", i, r.status, c.want); bad++; continue; }
        if (c.want == 0) {
            if (!zlibInflates(c.in, c.isize, want) || want != r.out) { fprintf(stderr, "member %zu: not zlib's bytes\n", i); bad++; continue; }
            good.push_back(i); nOk++;
        } else nRejected++;
    }
    if (good.empty()) { fprintf(stderr, "no well-formed member\n"); return 1; }
    const unsigned long nMut = strtoul(argv[2], nullptr, 10);
    std::mt19937_64 rng(strtoull(argv[3], nullptr, 10));
    unsigned long mutOk = 0, mutRejected = 0, kinds[3] = {0, 0, 0};
    for (unsigned long m = 0; m < nMut; m++) {
        const Case &c = cases[good[rng() % good.size()]];
        std::vector<uint8_t> in = c.in;
        uint32_t isize = c.isize;
        const int kind = (int)(rng() % 3);
        kinds[kind]++;
        if (kind == 0 && !in.empty()) {                     // one to four flipped bits
            const int n = 1 + (int)(rng() % 4);
            for (int k = 0; k < n; k++) in[rng() % in.size()] ^= (uint8_t)(1u << (rng() % 8));
        } else if (kind == 1 && !in.empty()) {              // cut short, sometimes with the output size cut too
            in.resize(rng() % in.size());
            if (rng() % 4 == 0) isize = (uint32_t)(rng() % (isize + 1));
        } else {                                            // the start of this member, the rest of another
            const Case &o = cases[good[rng() % good.size()]];
            const size_t a = in.empty() ? 0 : rng() % in.size(), b = o.in.empty() ? 0 : rng() % o.in.size();
            in.resize(a);
            in.insert(in.end(), o.in.begin() + (long)b, o.in.end());
            if (in.size() > 65536) in.resize(65536);
        }
        const Run r = runMember(in, isize, c.crc);
        tripsOk(r, in.size(), isize, "mutation", m);
        if (r.status >= STARAMD_INFLATE_STATUS_N) { fprintf(stderr, "mutation %lu: status %u is no status\n", m, r.status); bad++; continue; }
        if (r.status) { mutRejected++; continue; }
        if (!zlibInflates(in, isize, want) || want != r.out) { fprintf(stderr, "mutation %lu (kind %d): accepted, but zlib does not read these bytes so\n", m, kind); bad++; continue; }
        mutOk++;
    }
    printf("members: %lu inflated, %lu rejected as expected; mutations: %lu flips, %lu cuts, %lu splices: %lu rejected, %lu inflated to zlib's bytes; most trips %lu\n",
           nOk, nRejected, kinds[0], kinds[1], kinds[2], mutRejected, mutOk, maxTrips);
    if (bad) { printf("%lu failures\n", bad); return 1; }
    printf("clean\n");
    return 0;
}
