// seq_core.h -- extra reference sequences (--genomeFastaFiles at the mapping stage) inserted into a finished suffix-array index, as data-parallel
// passes over arrays in HBM.
//
// What it replaces: Genome::insertSequences (source/Genome_insertSequences.cpp:9-33) + insertSeqSA (source/insertSeqSA.cpp:18-319)
//   re-base   :31-51     old entries behind the insertion point move by the inserted length (here: fused into the search and the merge, never a pass
//                        of its own over the old array)
//   work text :53-70     inserted text, its reverse complement, fills and the complement array: the buffer the sort's memcmp walks
//   search    :77-96     insertion point of every suffix of the work text that starts with ACGT, in the re-based OLD suffix array, compared against
//                        the NEW genome text (suffixArraySearch1 with gInsert = nG, compareRefEnds: source/SuffixArrayFuns.cpp:210-351)
//   order     :111-113   (insertion point, bytes of the work text from the offset on -- a plain memcmp of unbounded length that runs through spacers
//                        and fills --, offset)                      (funCompareUintAndSuffixesMemcmp.cpp:7-33, gSuffixLengthMax = -1)
//   merge     :158-199   old and new entries interleaved into the new packed array
//   SAindex   :308       regenerated from the merged array by genomeSAindex: the generation-time builder of index_core.h as it is
// The order is NOT the one genomeGenerate gives the same sequences: suffixes that tie up to their spacer are ordered here by the bytes behind the
// spacer (padding, the next sequence, the fills), there by position.  So the check is a restatement of insertSeqSA, not the from-scratch builder.
//
// Same backend interface as index_core.h / sjdb_core.h: HipBackend is the product, tests/seq_insert_emul.cpp the plain-loop twin for CPU tests.
#pragma once
#include "sjdb_core.h"

namespace staridx {

struct SeqParams {
    u64 nG;                // old chrStart[nChrReal]: end of the chromosomes = start of the old junction block = where the new text goes
    u64 nG1;               // inserted text, padded to chromosome bins (genomeInsertL)
    u64 nG2;               // junction block (old nGenome - nG), moved behind the inserted text
    u64 nSAold;
    u32 GstrandBit, saIndexNbases;
};

enum { SEQ_FILL = 16 };            // GENOME_endFillL (insertSeqSA.cpp:55)
enum { SEQ_SEARCH_N = 10000 };     // the N of suffixArraySearch1 (:84): a comparison stops after this many characters

// insertSeqSA.cpp:21-29: would the grown genome need a wider strand bit than the packed array has?  0 = fits.
// (floor(log2(x)) + 1 is the number of bits of x)
static inline int seqStrandBitCheck(u64 nG, u64 nG1, u32 saWordLength) {
    u32 b = bitsFor(nG + nG1);
    if (b < 32) b = 32;
    return b + 1 > saWordLength ? 1 : 0;
}
static const char *const SEQ_STRANDBIT_ERROR =
    "EXITING because of FATAL ERROR: cannot insert sequence on the fly because of strand GstrandBit problem\n"
    "SOLUTION: please contact STAR author at https://groups.google.com/forum/#!forum/rna-star\n";

// :31-51 one old entry in the coordinates of the new genome
IDX_HD u64 seqRebase(u64 v, u64 nG, u64 nG1, u64 nG2, u64 N2bit) {
    if (v & N2bit) { if ((v & ~N2bit) >= nG2) v += nG1; }
    else if (v >= nG) v += nG1;
    return v;
}

// work text (:53-70).  X = seq1[0]: [0, nG1) inserted text, [nG1, 2 nG1) its reverse complement, SEQ_FILL spacers, [2 nG1 + FILL, 4 nG1 + FILL) the
// complement of the first 2 nG1 bytes (seq1[1]), SEQ_FILL spacers.  SEQ_FILL spacers lie in front of X as well (not part of any comparison).
static inline u64 seqWorkLength(u64 nG1) { return 4 * nG1 + 2 * SEQ_FILL; }
IDX_HD u8 seqWorkChar(const u8 *G1, u64 nG1, u64 i) {
    if (i < nG1) return G1[i];
    if (i < 2 * nG1) return compCode(G1[2 * nG1 - 1 - i]);
    if (i < 2 * nG1 + SEQ_FILL) return 5;
    const u64 k = i - 2 * nG1 - SEQ_FILL;
    if (k < nG1) return compCode(G1[k]);
    if (k < 2 * nG1) return G1[2 * nG1 - 1 - k];           // complement of the reverse complement
    return 5;
}

// compareRefEnds with gInsert = nG (SuffixArrayFuns.cpp:210-219): query and old suffix tie up to a spacer
IDX_HD int seqRefEnds(u64 s, u64 nG, u64 nGenomeNew, bool strG, bool strR) {
    if (strG) return strR ? (s < nG ? 1 : -1) : 1;
    return strR ? -1 : (s < nGenomeNew - nG ? 1 : -1);
}

// suffixArraySearch1(mapGen, seq1, off, 10000, nG, strR, 0, nSAold - 1, 0) (SuffixArrayFuns.cpp:297-351): first old index whose suffix is greater
// than the query.  Gn: NEW genome text (one readable spacer either side is all a comparison can touch: it stops where the query has a spacer, and
// every added sequence ends with one).  sa(i): re-based old entry.  "Smaller than the first" gives 0, "greater than the last" (the reference's -2)
// gives nSAold: it sorts last and lands behind the old array (:187-199).  A comparison that runs SEQ_SEARCH_N characters leaves the result of the
// previous one untouched, and inside the bisection ends the search at the probe (:334-337); *capHit tells.
template <class SAget> IDX_HD u64 seqSearchOne(const u8 *Gn, u64 nGenomeNew, u64 nG, u32 GstrandBit, u64 nSAold, SAget sa, const u8 *q, bool strR, u8 *capHit) {
    int r = 0;
    auto cmp = [&](u64 iSA, u64 L) -> u64 {                    // compareSeqToGenome1 from offset L; returns the new common length
        const u64 v = sa(iSA);
        const bool fwd = (v >> GstrandBit) == 0;
        const u64 s = v & ~(1ull << GstrandBit);
        for (u64 ii = L; ii < SEQ_SEARCH_N; ii++) {
            const u8 a = q[ii], b = fwd ? Gn[s + ii] : compCode(Gn[(i64)(nGenomeNew - 1 - s) - (i64)ii]);
            if (a != b) { r = a > b ? 1 : -1; return ii; }
            if (a == 5) { r = seqRefEnds(s, nG, nGenomeNew, fwd, strR); return ii; }
        }
        return SEQ_SEARCH_N;
    };
    *capHit = 0;
    u64 i1 = 0, i2 = nSAold - 1;
    u64 L1 = cmp(i1, 0);
    if (L1 == SEQ_SEARCH_N) *capHit = 1;
    if (r < 0) return 0;
    u64 L2 = cmp(i2, 0);
    if (L2 == SEQ_SEARCH_N) *capHit = 1;
    if (r > 0) return nSAold;
    u64 L = L1 < L2 ? L1 : L2;
    while (i1 + 1 < i2) {
        const u64 i3 = i1 / 2 + i2 / 2 + (i1 % 2 + i2 % 2) / 2;
        const u64 L3 = cmp(i3, L);
        if (L3 == SEQ_SEARCH_N) { *capHit = 1; return i3; }
        if (r > 0) { i1 = i3; L1 = L3; } else { i2 = i3; L2 = L3; }
        L = L1 < L2 ? L1 : L2;
    }
    return i2;
}

// Rank of every suffix of the token sequence tok[0, n) (tokens >= 1; a suffix that ends at n is smaller than its extensions).  rank[i] in [1, n],
// all different.  Prefix doubling: one token first, then rounds of two stable radix passes on (rank, rank h further on).
template <class BE> u64 *seqRankTokens(BE &be, const u64 *tok, u64 n, u64 maxTok, u64 *roundsOut) {
    u64 *key = be.template alloc<u64>(n), *keyAlt = be.template alloc<u64>(n), *sa = be.template alloc<u64>(n), *saAlt = be.template alloc<u64>(n);
    u64 *rank = be.template alloc<u64>(n), *rankN = be.template alloc<u64>(n);
    { u64 *k = key, *s = sa; be.forEach(n, [=] IDX_L (u64 i) { k[i] = tok[i]; s[i] = i; }); }
    if (n > 1) be.sortPairs(key, keyAlt, sa, saAlt, n, 0, (int)bitsFor(maxTok));
    u64 groups;
    {
        const u64 *k = key, *s = sa; u64 *hd = keyAlt, *rk = rank;
        be.forEach(n, [=] IDX_L (u64 j) { hd[j] = (j == 0 || k[j] != k[j - 1]) ? j : 0; });
        groups = compactIf(be, n, [=] IDX_L (u64 j) { return j == 0 || hd[j] == j; }, [=] IDX_L (u64, u64) {});
        be.inclusiveMax(hd, n);
        be.forEach(n, [=] IDX_L (u64 j) { rk[s[j]] = hd[j] + 1; });
    }
    const int rbits = (int)bitsFor(n + 1);
    u64 h = 1, rounds = 0;
    while (groups < n && h < 2 * n) {                         // (h >= n leaves no two suffixes equal; the bound ends the loop on a backend in an error state, whose counts are 0)
        rounds++;
        { u64 *k = key; const u64 *s = sa, *rk = rank; be.forEach(n, [=] IDX_L (u64 j) { const u64 p = s[j] + h; k[j] = p < n ? rk[p] : 0; }); }
        be.sortPairs(key, keyAlt, sa, saAlt, n, 0, rbits);
        { u64 *k = key; const u64 *s = sa, *rk = rank; be.forEach(n, [=] IDX_L (u64 j) { k[j] = rk[s[j]]; }); }
        be.sortPairs(key, keyAlt, sa, saAlt, n, 0, rbits);
        {
            const u64 *k = key, *s = sa, *rk = rank; u64 *k2 = keyAlt, *hd = saAlt, *rn = rankN;
            be.forEach(n, [=] IDX_L (u64 j) { const u64 p = s[j] + h; k2[j] = p < n ? rk[p] : 0; });
            be.forEach(n, [=] IDX_L (u64 j) { hd[j] = (j == 0 || k[j] != k[j - 1] || k2[j] != k2[j - 1]) ? j : 0; });
            groups = compactIf(be, n, [=] IDX_L (u64 j) { return j == 0 || hd[j] == j; }, [=] IDX_L (u64, u64) {});
            be.inclusiveMax(hd, n);
            be.forEach(n, [=] IDX_L (u64 j) { rn[s[j]] = hd[j] + 1; });
        }
        { u64 *t = rank; rank = rankN; rankN = t; }
        h *= 2;
    }
    be.free(key); be.free(keyAlt); be.free(sa); be.free(saAlt); be.free(rankN);
    if (roundsOut) *roundsOut = rounds;
    return rank;
}

// Rank of the suffixes of the work text X[0, M) that start at off[0 .. nInd) (ascending offsets, each at a code < 4), in PLAIN byte order: a spacer is
// a byte like any other, and a suffix that reaches M is smaller than its extensions (the reference's memcmp would read past its buffer there).
// The padding of an added sequence is a run of up to 2^genomeChrBinNbits spacers, so most of X is spacers.  The text is ranked as TOKENS: every
// code < 5 is a token (code + 1), every maximal run of r spacers ONE token (5 + r).  A suffix that starts outside a run meets runs at their first
// byte only, so comparing tokens is comparing bytes: of two runs the shorter is followed by a byte < 5 (or the end) where the longer goes on.
// The token sequence has about four tokens per added base, whatever the padding.  rankOut[j] are all different.
template <class BE> void seqRankCandidates(BE &be, const u8 *X, u64 M, const u64 *off, u64 nInd, u64 *rankOut, u64 *roundsOut) {
    auto isTok = [=] IDX_L (u64 i) { return X[i] != 5 || i == 0 || X[i - 1] != 5; };
    const u64 nTok = compactIf(be, M, isTok, [=] IDX_L (u64, u64) {});
    u64 *tokPos = be.template alloc<u64>(nTok + 1), *tok = be.template alloc<u64>(nTok);
    compactIf(be, M, isTok, [=] IDX_L (u64 i, u64 t) { tokPos[t] = i; });
    be.forEach(nTok, [=] IDX_L (u64 t) {
        const u64 p = tokPos[t];
        tok[t] = X[p] != 5 ? (u64)X[p] + 1 : 5 + ((t + 1 < nTok ? tokPos[t + 1] : M) - p);
    });
    u64 *rank = seqRankTokens(be, tok, nTok, M + 6, roundsOut);
    be.forEach(nInd, [=] IDX_L (u64 j) {
        const u64 o = off[j];
        u64 lo = 0, hi = nTok;                                   // the token that starts at o
        while (lo + 1 < hi) { const u64 mid = lo + (hi - lo) / 2; if (tokPos[mid] <= o) lo = mid; else hi = mid; }
        rankOut[j] = rank[lo];
    });
    be.free(rank); be.free(tokPos); be.free(tok);
}

struct SeqDeviceResult {
    u64 nInd, nSAnew, nGenomeNew, nCapHits, rounds;
    u64 *dSApacked; u64 saWords;      // new packed suffix array (device), caller frees with be.free
    u8 *dGnew;                        // new genome text with padOut spacer bytes either side (device): dGnew + padOut = base 0
    u64 *dSAiPacked; u64 saiWords;    // new packed SAindex (device)
    int badFirstSuffix;
};

// dGold: old genome text (nG + nG2 bytes), base 0 at dGold.  dSAold: packed old suffix array (whole u64 words readable).
// hG1: the inserted text, nG1 codes: sequences padded with spacers to chromosome bins, as genomeScanFastaFiles lays them out.
template <class BE> int seqInsertDevice(BE &be, const SeqParams &P, const u8 *dGold, const u64 *dSAold, const u8 *hG1, const u64 *saiStart, SeqDeviceResult &R,
                                        u64 padOut = SJ_GPAD) {
    const u64 nG = P.nG, nG1 = P.nG1, nG2 = P.nG2, nSAold = P.nSAold, nGenomeNew = nG + nG1 + nG2;
    const u32 GstrandBit = P.GstrandBit, saBits = P.GstrandBit + 1;
    const u64 N2bit = 1ull << GstrandBit, saMask = saBits >= 64 ? ~0ull : ((1ull << saBits) - 1);
    R.nGenomeNew = nGenomeNew;
    be.stage(nullptr);
    // ---- work text (insertSeqSA.cpp:53-70)
    const u64 M = seqWorkLength(nG1);
    u8 *dG1 = be.template alloc<u8>(nG1 + 1);
    be.copyToDevice(dG1, hG1, nG1);
    u8 *dWraw = be.template alloc<u8>(M + SEQ_FILL);
    u8 *X = dWraw + SEQ_FILL;
    be.forEach(M + SEQ_FILL, [=] IDX_L (u64 i) { dWraw[i] = i < SEQ_FILL ? (u8)5 : seqWorkChar(dG1, nG1, i - SEQ_FILL); });
    // ---- new genome text: chromosomes, added sequences, the moved junction block (Genome_insertSequences.cpp:19-25), spacers either side
    R.dGnew = be.template alloc<u8>(nGenomeNew + 2 * padOut);
    {
        u8 *gn = R.dGnew;
        be.forEach(nGenomeNew + 2 * padOut, [=] IDX_L (u64 i) {
            u8 c = 5;
            if (i >= padOut && i < padOut + nGenomeNew) { const u64 p = i - padOut; c = p < nG ? dGold[p] : p < nG + nG1 ? dG1[p - nG] : dGold[p - nG1]; }
            gn[i] = c;
        });
    }
    const u8 *Gn = R.dGnew + padOut;
    be.stage("seq: work text + genome");
    // ---- candidates: every offset of the forward + reverse-complement text that starts with ACGT, in offset order (:77-96)
    auto isCand = [=] IDX_L (u64 o) { return X[o] < 4; };
    const u64 nInd = compactIf(be, 2 * nG1, isCand, [=] IDX_L (u64, u64) {});
    R.nInd = nInd; R.nSAnew = nSAold + nInd;
    u64 *off = be.template alloc<u64>(nInd + 1), *pos = be.template alloc<u64>(nInd + 1);
    compactIf(be, 2 * nG1, isCand, [=] IDX_L (u64 o, u64 j) { off[j] = o; });
    be.stage("seq: candidates");
    // ---- search (:84) in the old array, entries re-based on the fly
    {
        u8 *hit = be.template alloc<u8>(nInd + 1);
        be.forEach(nInd, [=] IDX_L (u64 j) {
            auto sa = [=](u64 i) { return seqRebase(packedGetW(dSAold, i, saBits) & saMask, nG, nG1, nG2, N2bit); };
            const u64 o = off[j];
            pos[j] = seqSearchOne(Gn, nGenomeNew, nG, GstrandBit, nSAold, sa, X + o, o < nG1, hit + j);
        });
        R.nCapHits = compactIf(be, nInd, [=] IDX_L (u64 j) { return hit[j] != 0; }, [=] IDX_L (u64, u64) {});
        be.free(hit);
    }
    be.stage("seq: search");
    // ---- order (:111-113): (insertion point, byte order of the work text from the offset on, offset).  The suffix ranks are all different, so
    //      the offset never decides; two stable passes, rank first
    R.rounds = 0;
    if (nInd > 1) {
        u64 *key = be.template alloc<u64>(nInd), *keyAlt = be.template alloc<u64>(nInd), *perm = be.template alloc<u64>(nInd), *permAlt = be.template alloc<u64>(nInd);
        seqRankCandidates(be, X, M, off, nInd, key, &R.rounds);
        { u64 *pm = perm; be.forEach(nInd, [=] IDX_L (u64 j) { pm[j] = j; }); }
        be.sortPairs(key, keyAlt, perm, permAlt, nInd, 0, (int)bitsFor(M + 1));
        { u64 *k = key; const u64 *pm = perm; be.forEach(nInd, [=] IDX_L (u64 j) { k[j] = pos[pm[j]]; }); }
        be.sortPairs(key, keyAlt, perm, permAlt, nInd, 0, (int)bitsFor(nSAold + 1));
        { u64 *k = keyAlt; const u64 *pm = perm; be.forEach(nInd, [=] IDX_L (u64 j) { k[j] = off[pm[j]]; }); }
        { const u64 *k = key, *k2 = keyAlt; be.forEach(nInd, [=] IDX_L (u64 j) { pos[j] = k[j]; off[j] = k2[j]; }); }
        be.free(key); be.free(keyAlt); be.free(perm); be.free(permAlt);
    }
    be.stage("seq: order");
    // ---- merge (:158-199), the re-basing of :31-51 fused in: new entry j lands at output index pos[j] + j, old entries fill the rest in order.
    //      The form of sjdb_core.h: a bisection per group of 64 output entries, then ONE THREAD PER OUTPUT WORD, so that the old array streams in
    //      and the new one out through whole cache lines.
    const u64 nSAnew = R.nSAnew;
    R.saWords = packedWords(nSAnew + 1, saBits);
    R.dSApacked = be.template alloc<u64>(R.saWords);
    {
        u64 *out = R.dSApacked; const u64 *ps = pos, *of = off;
        const u64 nGroups = (nSAnew + 1 + 63) / 64;              // one more entry: the 0 the reference writes behind the array (sjdbInsertJunctions.cpp:66-68)
        u64 *jnG = be.template alloc<u64>(nGroups + 1);
        be.forEach(nGroups, [=] IDX_L (u64 g) {
            const u64 o0 = g * 64;
            u64 lo = 0, hi = nInd;                               // first j with pos[j] + j >= o0
            while (lo < hi) { const u64 mid = lo + (hi - lo) / 2; if (ps[mid] + mid < o0) lo = mid + 1; else hi = mid; }
            jnG[g] = lo;
        });
        const u64 nWords = nGroups * saBits;                     // the words of whole groups (packedWords() has two more, zeroed below)
        be.forEach(nWords, [=] IDX_L (u64 w) {
            const u64 bit0 = w * 64;
            u64 e = bit0 / saBits;                               // first entry with bits in this word
            u64 jn = jnG[e >> 6];
            while (jn < nInd && ps[jn] + jn < e) jn++;           // new entries before entry e
            u64 word = 0;
            for (; e * saBits < bit0 + 64; e++) {
                u64 v = 0;
                if (e < nSAnew) {
                    if (jn < nInd && ps[jn] + jn == e) {
                        const u64 f = of[jn++];
                        v = f < nG1 ? f + nG : ((f - nG1 + nG2) | N2bit);                                  // :161-166
                    } else v = seqRebase(packedGetW(dSAold, e - jn, saBits) & saMask, nG, nG1, nG2, N2bit);
                }
                const u64 b = e * saBits;
                word |= b >= bit0 ? (v << (b - bit0)) : (v >> (bit0 - b));
            }
            out[w] = word;
        });
        be.forEach(packedWords(nSAnew + 1, saBits) - nWords, [=] IDX_L (u64 k) { out[nWords + k] = 0; });
        be.free(jnG);
    }
    be.free(pos); be.free(off); be.free(dWraw); be.free(dG1);
    be.stage("seq: merge");
    // ---- SAindex of the merged array: a fresh walk (genomeSAindex, insertSeqSA.cpp:308), every suffix marks
    R.saiWords = packedWords(saiStart[P.saIndexNbases], GstrandBit + 3);
    R.dSAiPacked = be.template alloc<u64>(R.saiWords);
    {
        const u64 N = nGenomeNew;
        u8 *dTraw = be.template alloc<u8>(2 * N + 2 * TPAD);
        u8 *T = buildText(be, Gn, N, dTraw);
        u64 *dSApos = be.template alloc<u64>(nSAnew);
        { const u64 *sp = R.dSApacked; be.forEach(nSAnew, [=] IDX_L (u64 i) { const u64 v = packedGetW(sp, i, saBits); dSApos[i] = (v & N2bit) ? N + (v & ~N2bit) : v; }); }
        const u64 nSAi = saiStart[P.saIndexNbases];
        u64 *dSAiU = be.template alloc<u64>(nSAi);
        be.stage("seq: SAindex text + unpack");
        R.badFirstSuffix = buildSAindex(be, T, dSApos, nSAnew, P.saIndexNbases, GstrandBit, saiStart, dSAiU);
        const u64 *su = dSAiU;
        packArray(be, nSAi, GstrandBit + 3, R.dSAiPacked, [=] IDX_L (u64 i) { return su[i]; });
        be.free(dSAiU); be.free(dSApos); be.free(dTraw);
    }
    be.stage("seq: SAindex build + pack");
    return 0;
}

// host buffers in, host buffers out (include/star_amd_index.h staramd_seq_insert); returns 0, -2 capacity, -3 bad first suffix, -4 GstrandBit
struct SeqHostArgs {
    const u8 *G; const u8 *SA; u64 nSAbyteOld; const u8 *G1;
    u8 *SAout; u64 saCap; u8 *SAiOut; u64 saiCap;
};
template <class BE> int seqInsertHost(BE &be, const SeqParams &P, const SeqHostArgs &A, SeqDeviceResult &R, u64 &nSAbyteNew, u64 &nSAibyte) {
    R = SeqDeviceResult();
    if (seqStrandBitCheck(P.nG, P.nG1, P.GstrandBit + 1)) return -4;
    u64 saiStart[17]; saiStart[0] = 0;
    for (u32 i = 1; i <= P.saIndexNbases; i++) saiStart[i] = saiStart[i - 1] + (1ull << (2 * i));
    const u64 nOld = P.nG + P.nG2;
    be.stage(nullptr);
    u8 *dG = be.template alloc<u8>(nOld + 1);
    be.copyToDevice(dG, A.G, nOld);
    const u64 wOld = (A.nSAbyteOld + 7) / 8 + 2;
    u64 *dSAold = be.template alloc<u64>(wOld);
    { u64 *w = dSAold; be.forEach(3, [=] IDX_L (u64 i) { w[wOld - 1 - i] = 0; }); }
    be.copyToDevice((u8 *)dSAold, A.SA, A.nSAbyteOld);
    be.stage("seq: upload genome + SA");
    seqInsertDevice(be, P, dG, dSAold, A.G1, saiStart, R);
    be.free(dSAold); be.free(dG);
    nSAbyteNew = packedBytes(R.nSAnew, P.GstrandBit + 1); nSAibyte = packedBytes(saiStart[P.saIndexNbases], P.GstrandBit + 3);
    int rc = R.badFirstSuffix ? -3 : 0;
    if (A.saCap < nSAbyteNew || A.saiCap < nSAibyte) rc = -2;
    if (!rc) { be.copyToHost(A.SAout, (const u8 *)R.dSApacked, nSAbyteNew); be.copyToHost(A.SAiOut, (const u8 *)R.dSAiPacked, nSAibyte); }
    be.stage("seq: download SA + SAindex");
    be.free(R.dSApacked); be.free(R.dGnew); be.free(R.dSAiPacked);
    R.dSApacked = nullptr; R.dGnew = nullptr; R.dSAiPacked = nullptr;
    return rc;
}

} // namespace staridx
