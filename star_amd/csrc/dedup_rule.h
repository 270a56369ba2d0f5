// dedup_rule.h -- what one BAM record gives the duplicate rule of --bamRemoveDuplicatesType (the reference: source/bamRemoveDuplicates.cpp),
// stated once for the host path (host/dedup.cpp) and the device path (engine/k_dedup.hip): the record's fields, its start and its CIGAR with the soft
// clips folded in, the bases of mate 2, the order of names, and hashes of name and content.  The hashes only ORDER records; equality is always taken
// from the comparisons below.  No read leaves the record: `len` bytes are the caller's, the record's own block_size shortens them, and everything that
// would lie behind reads as absent (a CIGAR word that does not fit is no word, a base that does not fit is 0).
#pragma once
#include "bam_aux.h"

struct DedupCore {
    uint64_t lim, cigar, seq;           // bytes of the record that may be read; byte offsets of CIGAR and SEQ
    uint32_t tid, pos, flag, lseq;
    uint32_t nameLen;                   // l_read_name (the NUL counts), cut at the record's end
    uint32_t n, lead, trail;            // CIGAR words that fit; 1: a leading / trailing S is folded into its neighbour
    bool ok;                            // false: not even the fixed fields fit (the record then has no NH either)
};

BAM_HD DedupCore dedupCore(const uint8_t *rec, uint64_t len) {
    DedupCore c; c.ok = false; c.lim = 0; c.cigar = c.seq = 36; c.tid = c.pos = c.flag = c.lseq = c.nameLen = c.n = c.lead = c.trail = 0;
    if (len < 36) return c;
    const uint64_t own = (uint64_t)bamLd32(rec) + 4;
    c.lim = own < len ? own : len;
    if (c.lim < 36) return c;
    c.ok = true;
    const uint32_t bmn = bamLd32(rec + 12), fnc = bamLd32(rec + 16), nCigar = fnc & 0xffff;
    c.tid = bamLd32(rec + 4); c.pos = bamLd32(rec + 8); c.flag = fnc >> 16; c.lseq = bamLd32(rec + 20);
    c.nameLen = bmn & 0xff;
    c.cigar = 36 + (uint64_t)c.nameLen;
    if (36 + (uint64_t)c.nameLen > c.lim) c.nameLen = (uint32_t)(c.lim - 36);
    c.seq = c.cigar + 4 * (uint64_t)nCigar;
    c.n = c.seq <= c.lim ? nCigar : c.cigar < c.lim ? (uint32_t)((c.lim - c.cigar) / 4) : 0;
    // a lone S is left as it is; of "aSbS" only the leading clip has a neighbour left to take it
    c.lead = c.n >= 2 && (bamLd32(rec + c.cigar) & 0xf) == 4;
    c.trail = c.n - c.lead >= 2 && (bamLd32(rec + c.cigar + 4 * (uint64_t)(c.n - 1)) & 0xf) == 4;
    return c;
}
BAM_HD uint64_t dedupAuxStart(const DedupCore &c) { return c.seq + ((uint64_t)c.lseq + 1) / 2 + c.lseq; }
// pos minus a leading clip, in uint32 arithmetic (funStartExtendS)
BAM_HD uint32_t dedupStartS(const uint8_t *rec, const DedupCore &c) { return c.lead ? c.pos - (bamLd32(rec + c.cigar) >> 4) : c.pos; }
// cigarS (funCigarExtendS): m words
BAM_HD uint32_t dedupCigN(const DedupCore &c) { return c.n - c.lead - c.trail; }
BAM_HD uint32_t dedupCigWord(const uint8_t *rec, const DedupCore &c, uint32_t j) {
    uint32_t w = bamLd32(rec + c.cigar + 4 * (uint64_t)(j + c.lead));
    if (j == 0 && c.lead) w += bamLd32(rec + c.cigar) & ~0xfu;
    if (j + 1 == dedupCigN(c) && c.trail) w += bamLd32(rec + c.cigar + 4 * (uint64_t)(c.n - 1)) & ~0xfu;
    return w;
}
// the bases of mate 2 that take part: the first min(N, l_seq) 4-bit codes of a forward record, the last ones of a reverse one
BAM_HD uint32_t dedupBasesN(const DedupCore &c, uint32_t N) { return N < c.lseq ? N : c.lseq; }
BAM_HD uint32_t dedupBase(const uint8_t *rec, const DedupCore &c, uint32_t N, uint32_t j) {
    const uint32_t i = (c.flag & 0x10) ? c.lseq - dedupBasesN(c, N) + j : j;
    const uint64_t at = c.seq + i / 2;
    if (at >= c.lim) return 0;
    return (i & 1) ? rec[at] & 15u : rec[at] >> 4;
}

BAM_HD uint64_t dedupMix(uint64_t h, uint64_t x) { h ^= x; h *= 0x9E3779B97F4A7C15ull; h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32; return h; }
BAM_HD uint64_t dedupNameHash(const uint8_t *rec, const DedupCore &c) {
    uint64_t h = dedupMix(0x6e616d65ull, c.nameLen);
    BAM_NO_UNROLL
    for (uint32_t i = 0; i < c.nameLen; i++) h = dedupMix(h, rec[36 + i]);
    return h;
}
// of cigarS and, for a mate 2, its bases
BAM_HD uint64_t dedupContentHash(const uint8_t *rec, const DedupCore &c, uint32_t N) {
    const uint32_t m = dedupCigN(c);
    uint64_t h = dedupMix(0x63696761ull, m);
    BAM_NO_UNROLL
    for (uint32_t j = 0; j < m; j++) h = dedupMix(h, dedupCigWord(rec, c, j));
    if (c.flag & 0x80) {
        const uint32_t nb = dedupBasesN(c, N);
        h = dedupMix(h, nb);
        BAM_NO_UNROLL
        for (uint32_t j = 0; j < nb; j++) h = dedupMix(h, dedupBase(rec, c, N, j));
    }
    return h;
}

// names: by length, then by bytes as the reference's `char` compares them (funCompareNames)
BAM_HD int dedupNameCmp(const uint8_t *a, const DedupCore &ca, const uint8_t *b, const DedupCore &cb) {
    if (ca.nameLen != cb.nameLen) return ca.nameLen < cb.nameLen ? -1 : 1;
    BAM_NO_UNROLL
    for (uint32_t i = 0; i < ca.nameLen; i++) { const int8_t x = (int8_t)a[36 + i], y = (int8_t)b[36 + i]; if (x != y) return x < y ? -1 : 1; }
    return 0;
}
BAM_HD int dedupCigCmp(const uint8_t *a, const DedupCore &ca, const uint8_t *b, const DedupCore &cb) {
    const uint32_t ma = dedupCigN(ca), mb = dedupCigN(cb);
    if (ma != mb) return ma < mb ? -1 : 1;
    BAM_NO_UNROLL
    for (uint32_t j = 0; j < ma; j++) { const uint32_t x = dedupCigWord(a, ca, j), y = dedupCigWord(b, cb, j); if (x != y) return x < y ? -1 : 1; }
    return 0;
}
BAM_HD int dedupBasesCmp(const uint8_t *a, const DedupCore &ca, const uint8_t *b, const DedupCore &cb, uint32_t N) {
    const uint32_t na = dedupBasesN(ca, N), nb = dedupBasesN(cb, N);
    if (na != nb) return na < nb ? -1 : 1;
    BAM_NO_UNROLL
    for (uint32_t j = 0; j < na; j++) { const uint32_t x = dedupBase(a, ca, N, j), y = dedupBase(b, cb, N, j); if (x != y) return x < y ? -1 : 1; }
    return 0;
}
// the part of a pair's class key that is not a number: cigarS of mate 1, cigarS of mate 2, bases of mate 2
BAM_HD int dedupContentCmp(const uint8_t *a1, uint64_t la1, const uint8_t *a2, uint64_t la2, const uint8_t *b1, uint64_t lb1, const uint8_t *b2, uint64_t lb2, uint32_t N) {
    const DedupCore ca1 = dedupCore(a1, la1), cb1 = dedupCore(b1, lb1);
    int r = dedupCigCmp(a1, ca1, b1, cb1);
    if (r) return r;
    const DedupCore ca2 = dedupCore(a2, la2), cb2 = dedupCore(b2, lb2);
    r = dedupCigCmp(a2, ca2, b2, cb2);
    if (r) return r;
    return dedupBasesCmp(a2, ca2, b2, cb2, N);
}
// the numbers of the key: tid | startS of mate 1, startS of mate 2 | flag of mate 1 | flag of mate 2 (both without 0x400)
BAM_HD uint64_t dedupKeyHi(uint32_t tid, uint32_t startS1) { return (uint64_t)tid << 32 | startS1; }
BAM_HD uint64_t dedupKeyLo(uint32_t startS2, uint32_t flag1, uint32_t flag2) { return (uint64_t)startS2 << 32 | (uint64_t)(flag1 & 0xfbffu) << 16 | (flag2 & 0xfbffu); }
