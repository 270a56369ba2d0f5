// bgzf_routines_check.cpp -- TEST INFRASTRUCTURE: the one-lane routines of k_bgzf.hip behind a C ABI, so that tests/test_bgzf_routines.py can hold them
// to plain Python (RFC 1951's tables, zlib's CRC32, a package-merge optimum).  They sit in an anonymous namespace there, so this file takes k_bgzf.hip
// into its own translation unit; host build through the wavefront emulator's headers (oracle/wave_emul), no GPU.  Nothing here runs a kernel.
#include "../star_amd/csrc/engine/k_bgzf.hip"

extern "C" {

// frq[0..m): ascending frequencies (destroyed), sym[0..m): their symbols, pack[nsym] zeroed by the caller: pack[s] = len << 16 afterwards
void bzr_huff_lengths(uint32_t *frq, const uint32_t *sym, uint32_t m, uint32_t maxBits, uint32_t *pack) {
    uint32_t blc[16];
    huffLengths(frq, sym, m, maxBits, blc, pack);
}
// pack[s] = len << 16 on entry, len << 16 | bit-reversed canonical code afterwards
void bzr_canon(uint32_t *pack, uint32_t nsym) {
    uint32_t blc[16], nxt[16];
    canonCounts(pack, nsym, blc, nxt);
    for (uint32_t s = 0; s < nsym; s++) canonCode(pack, s, nxt);
}
// sym / frq [0..number of nonzero f): the order the length builder takes
void bzr_rank(const uint32_t *f, uint32_t nsym, uint32_t *sym, uint32_t *frq) {
    for (uint32_t s = 0; s < nsym; s++) rankSym(f, nsym, s, sym, frq);
}
uint32_t bzr_len_sym(uint32_t L, uint32_t *eb, uint32_t *ev) { return lenSym(L, *eb, *ev); }
uint32_t bzr_dist_sym(uint32_t D, uint32_t *eb, uint32_t *ev) { return distSym(D, *eb, *ev); }
uint32_t bzr_len_extra(uint32_t s) { return lenExtra(s); }
uint32_t bzr_dist_extra(uint32_t c) { return distExtra(c); }
uint32_t bzr_fixed_lit_len(uint32_t s) { return fixedLitLen(s); }
uint32_t bzr_cl_order(uint32_t i) { return clOrder(i); }
uint32_t bzr_mul_mod_p(uint32_t a, uint32_t b) { return mulModP(a, b); }
uint32_t bzr_x_pow8(uint32_t nBytes) { return xPow8(nBytes); }

}  // extern "C"
