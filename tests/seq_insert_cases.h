// seq_insert_cases.h -- TEST INFRASTRUCTURE: the passes of the sequence insertion (star_amd/csrc/index/seq_core.h: seqRebase, seqWorkChar, seqSearchOne,
// seqRankCandidates, seqInsertDevice, seqInsertHost, seqStrandBitCheck) one at a time against a plain, serial restatement of the reference
// (source/insertSeqSA.cpp:18-319, source/SuffixArrayFuns.cpp:210-351, source/funCompareUintAndSuffixesMemcmp.cpp), as templates over a backend:
// tests/seq_insert_check.cpp instantiates them with the plain-loop backend, tests/seq_insert_gpu.hip with HipBackend.  Inputs are fabricated (old
// indexes built by the product's buildAll, which tests/test_index_routines.py holds to the reference) and the cases of tests/golden/seq_insert, whose
// files the reference wrote: the restatement, seqInsertHost, and the chain seqInsertHost -> sjdbInsertHost are held to those bytes.
// Report, Rng, the SAindex walk, packRef, readAll and paramOf are those of oracle/index_routines_cases.h.
#pragma once
#include "../star_amd/csrc/index/seq_core.h"
#include "../oracle/index_routines_cases.h"

namespace seqchk {
using namespace staridx;
using idxchk::Rng; using idxchk::up; using idxchk::down; using idxchk::checkBackend; using idxchk::readAll; using idxchk::paramOf;

static const char *const SEQ_CLASSES[] = {
    "rebase: + strand chromosome entry kept", "rebase: + strand junction entry moved", "rebase: - strand entry below nG2 kept", "rebase: - strand entry moved",
    "work text: all five regions",
    "search: tie at a spacer, query + genome +", "search: tie at a spacer, query + genome -", "search: tie at a spacer, query - genome +", "search: tie at a spacer, query - genome -",
    "search: tie with a + strand entry at or past nG", "search: tie with a - strand entry behind the insertion point", "search: below the first old suffix (0)", "search: above the last old suffix", "search: between",
    "search: stopped at 10000 characters", "order: same insertion point, decided before a spacer", "order: same insertion point, decided behind a spacer",
    "order: ranks of all candidates against memcmp", "order: rounds 1 and more",
    "merge: new entry at output index 0", "merge: new entries behind the last old entry", "merge: run of 3 or more new entries", "merge: nSAnew a multiple of 64", "merge: nSAnew 62 mod 64",
    "merge: zero entry and words behind the array", "merge: GstrandBit 32", "merge: GstrandBit 34", "insert: new genome text", "insert: SAindex of the merged array", "insert: N inside the SAindex prefix of a new suffix",
    "host: rc 0 bytes equal between guards", "host: rc -2 SA one byte short", "host: rc -2 SAindex one byte short", "host: rc -4 GstrandBit",
    "strand bit: fits", "strand bit: does not fit", "strand bit: below 32 counts as 32",
    "golden: restatement against the reference's files (annotated form)", "golden: seqInsertHost against the reference's files (annotated form)",
    "golden: seqInsertHost then sjdbInsertHost against the reference's files (plain form)", "golden: differs from a from-scratch order",
};
struct SeqReport : idxchk::Report {
    SeqReport() { cls.clear(); for (const char *c : SEQ_CLASSES) cls.push_back({c, 0}); }
};

// =====================================================================================================================
// the restatement: insertSeqSA.cpp, line by line, on vectors

struct RefInsert {
    std::vector<u64> rebased, pos, off, saNew;      // pos / off: the sorted list (indArray)
    std::vector<u64> posByOff;                      // 2 nG1 entries, ~0 = no candidate
    std::vector<u8> seqq, Gnew;
    u64 tie[2][2] = {{0, 0}, {0, 0}}, tieMoved[2] = {0, 0}, capHits = 0, atZero = 0, atEnd = 0, between = 0, cmpBefore = 0, cmpBehind = 0, run3 = 0;
    u64 reb[4] = {0, 0, 0, 0};
};

static inline RefInsert refInsert(const std::vector<u8> &Gold, u64 nG, const std::vector<u8> &G1v, const std::vector<u64> &saOld, u32 gsb) {
    RefInsert X;
    const u64 nG1 = G1v.size(), nG2 = Gold.size() - nG, nGenome = nG + nG1 + nG2;
    // Genome_insertSequences.cpp:19-25
    X.Gnew.assign(Gold.begin(), Gold.begin() + nG); X.Gnew.insert(X.Gnew.end(), G1v.begin(), G1v.end()); X.Gnew.insert(X.Gnew.end(), Gold.begin() + nG, Gold.end());
    const i64 PAD = 256;
    std::vector<char> Gp(nGenome + 2 * PAD, 5); memcpy(Gp.data() + PAD, X.Gnew.data(), nGenome);
    char *G = Gp.data() + PAD;
    // :31-51
    const u64 N2bit = 1ull << gsb, strandMask = ~N2bit;
    X.rebased = saOld;
    for (u64 isa = 0; isa < X.rebased.size(); isa++) {
        u64 ind1 = X.rebased[isa];
        if ((ind1 & N2bit) > 0) { if ((ind1 & strandMask) >= nG2) { ind1 += nG1; X.reb[3]++; } else X.reb[2]++; }
        else { if (ind1 >= nG) { ind1 += nG1; X.reb[1]++; } else X.reb[0]++; }
        X.rebased[isa] = ind1;
    }
    // :53-70
    const u64 FILL = 16;
    X.seqq.assign(4 * nG1 + 3 * FILL, 0);
    char *seqq = (char *)X.seqq.data(), *seq1[2] = {seqq + FILL, seqq + 2 * FILL + 2 * nG1};
    memset(seqq, 5, FILL); memset(seqq + 2 * nG1 + FILL, 5, FILL); memset(seqq + 4 * nG1 + 2 * FILL, 5, FILL);
    memcpy(seq1[0], G1v.data(), nG1);
    for (u64 ii = 0; ii < nG1; ii++) seq1[0][2 * nG1 - 1 - ii] = seq1[0][ii] < 4 ? 3 - seq1[0][ii] : seq1[0][ii];
    for (u64 jj = 0; jj < 2 * nG1; jj++) seq1[1][jj] = seq1[0][jj] < 4 ? 3 - seq1[0][jj] : seq1[0][jj];
    // SuffixArrayFuns.cpp:210-351
    const u64 N = 10000, nSA = saOld.size();
    int compRes = 0; bool tied = false, tiedMoved = false; int tieG = 0;
    auto compare1 = [&](u64 S, u64 L, u64 iSA, bool dirR) -> u64 {
        u64 SAstr = X.rebased[iSA];
        const bool dirG = (SAstr >> gsb) == 0;
        SAstr &= strandMask;
        auto refEnds = [&]() {
            tied = true; tieG = dirG ? 0 : 1;
            if (dirG) { tiedMoved = SAstr >= nG; return dirR ? (SAstr < nG ? 1 : -1) : 1; }
            tiedMoved = SAstr < nGenome - nG;
            return dirR ? -1 : (SAstr < nGenome - nG ? 1 : -1);
        };
        if (dirG) {
            char *s = seq1[0] + S + L, *g = G + SAstr + L;
            for (i64 ii = 0; (u64)ii < N - L; ii++) {
                if (s[ii] != g[ii]) { compRes = s[ii] > g[ii] ? 1 : -1; return ii + L; }
                else if (s[ii] == 5) { compRes = refEnds(); return ii + L; }
            }
            return N;
        }
        char *s = seq1[1] + S + L, *g = G + nGenome - 1 - SAstr - L;
        for (i64 ii = 0; (u64)ii < N - L; ii++) {
            if (s[ii] != g[-ii]) {
                char s1 = s[ii], g1 = g[-ii];
                if (s1 < 4) s1 = 3 - s1;
                if (g1 < 4) g1 = 3 - g1;
                compRes = s1 > g1 ? 1 : -1; return ii + L;
            } else if (s[ii] == 5) { compRes = refEnds(); return ii + L; }
        }
        return N;
    };
    auto search1 = [&](u64 S, bool strR, bool &cap) -> u64 {
        u64 i1 = 0, i2 = nSA - 1, L = 0;
        compRes = 0; cap = false;
        u64 L1 = compare1(S, L, i1, strR); if (L1 == N) cap = true;
        if (compRes < 0) return 0;
        u64 L2 = compare1(S, L, i2, strR); if (L2 == N) cap = true;
        if (compRes > 0) return (u64)-2ll;
        L = std::min(L1, L2);
        while (i1 + 1 < i2) {
            const u64 i3 = i1 / 2 + i2 / 2 + (i1 % 2 + i2 % 2) / 2;
            const u64 L3 = compare1(S, L, i3, strR);
            if (L3 == N) { cap = true; return i3; }
            if (compRes > 0) { i1 = i3; L1 = L3; } else if (compRes < 0) { i2 = i3; L2 = L3; }
            L = std::min(L1, L2);
        }
        return i2;
    };
    // :77-96
    X.posByOff.assign(2 * nG1, ~0ull);
    std::vector<std::pair<u64, u64>> ind;
    for (u64 ii = 0; ii < 2 * nG1; ii++) {
        if (seq1[0][ii] > 3) continue;
        bool cap; tied = false;
        const u64 p = search1(ii, ii < nG1, cap);
        // the tie of the LAST comparison that decided is what places the suffix; counting every search in which a tie occurred is enough for the classes
        if (tied) { X.tie[ii < nG1 ? 0 : 1][tieG]++; if (tiedMoved) X.tieMoved[tieG]++; }
        if (cap) X.capHits++;
        if (p == 0) X.atZero++; else if (p == (u64)-2ll) X.atEnd++; else X.between++;
        X.posByOff[ii] = p == (u64)-2ll ? nSA : p;
        ind.push_back({p, ii});
    }
    // :111-113 funCompareUintAndSuffixesMemcmp: memcmp of unbounded length (here: to the end of the buffer), then the offset
    const u64 bufEnd = 4 * nG1 + 2 * FILL;            // from seq1[0]
    std::sort(ind.begin(), ind.end(), [&](const std::pair<u64, u64> &a, const std::pair<u64, u64> &b) {
        if (a.first != b.first) return a.first < b.first;
        if (a.second == b.second) return false;
        const u64 len = bufEnd - std::max(a.second, b.second);
        const int c = memcmp(seq1[0] + a.second, seq1[0] + b.second, len);
        if (c) {
            u64 k = 0; while (seq1[0][a.second + k] == seq1[0][b.second + k]) k++;
            bool behind = false; for (u64 t = 0; t < k; t++) if (seq1[0][a.second + t] == 5) { behind = true; break; }
            if (behind) X.cmpBehind++; else X.cmpBefore++;
            return c < 0;
        }
        return a.second < b.second;
    });
    // :158-199
    const u64 nInd = ind.size();
    ind.push_back({(u64)-999ll, (u64)-999ll});
    auto newVal = [&](u64 ind1) { return ind1 < nG1 ? ind1 + nG : ((ind1 - nG1 + nG2) | N2bit); };
    u64 isa1 = 0;
    for (u64 isa = 0; isa < nSA; isa++) {
        u64 run = 0;
        while (isa == ind[isa1].first) { X.saNew.push_back(newVal(ind[isa1].second)); ++isa1; run++; }
        if (run >= 3) X.run3++;
        X.saNew.push_back(X.rebased[isa]);
    }
    for (; isa1 < nInd; isa1++) X.saNew.push_back(newVal(ind[isa1].second));
    for (u64 j = 0; j < nInd; j++) { X.pos.push_back(ind[j].first == (u64)-2ll ? nSA : ind[j].first); X.off.push_back(ind[j].second); }
    return X;
}

static inline std::vector<u64> unpackBytes(const std::vector<u8> &bytes, u64 n, u32 bits) {
    std::vector<u64> w(bytes.size() / 8 + 3, 0); memcpy(w.data(), bytes.data(), bytes.size());
    std::vector<u64> v(n); for (u64 i = 0; i < n; i++) v[i] = packedGetW(w.data(), i, bits);
    return v;
}

// =====================================================================================================================
// one insertion, pass by pass

struct SeqCase { std::string name; std::vector<u8> Gold; u64 nG; std::vector<u8> G1; std::vector<u8> SAbytes; u64 nSAold; u32 gsb, L; };

template <class BE> RefInsert caseSeqInsert(BE &be, SeqReport &R, const SeqCase &C, std::vector<u8> *saOut = nullptr, std::vector<u8> *saiOut = nullptr) {
    R.begin(C.name);
    const u32 gsb = C.gsb, saBits = gsb + 1; const u64 nG = C.nG, nG1 = C.G1.size(), nG2 = C.Gold.size() - nG, nSAold = C.nSAold, N2bit = 1ull << gsb;
    const std::vector<u64> saOld = unpackBytes(C.SAbytes, nSAold, saBits);
    const RefInsert X = refInsert(C.Gold, nG, C.G1, saOld, gsb);
    const u64 nGenomeNew = X.Gnew.size(), nInd = X.off.size(), nSAnew = nSAold + nInd;
    // ---- re-base
    {
        u64 *d = up(be, saOld);
        be.forEach(nSAold, [=] IDX_L (u64 i) { d[i] = seqRebase(d[i], nG, nG1, nG2, N2bit); });
        R.same("re-based old entries", down(be, d, nSAold), X.rebased);
        be.free(d);
        static const char *const RC[4] = {"rebase: + strand chromosome entry kept", "rebase: + strand junction entry moved", "rebase: - strand entry below nG2 kept", "rebase: - strand entry moved"};
        for (int k = 0; k < 4; k++) if (X.reb[k]) R.hit(RC[k]);
    }
    checkBackend(be, R);
    // ---- work text
    const u64 M = seqWorkLength(nG1);
    u8 *dG1 = up(be, C.G1, 1);
    u8 *dX = be.template alloc<u8>(M);
    be.forEach(M, [=] IDX_L (u64 i) { dX[i] = seqWorkChar(dG1, nG1, i); });
    R.same("work text", down(be, dX, M), std::vector<u8>(X.seqq.begin() + SEQ_FILL, X.seqq.end()));
    R.hit("work text: all five regions");
    checkBackend(be, R);
    // ---- search, every candidate
    {
        std::vector<u8> Gp(nGenomeNew + 2 * SJ_GPAD, 5); memcpy(Gp.data() + SJ_GPAD, X.Gnew.data(), nGenomeNew);
        u8 *dGp = up(be, Gp); const u8 *Gn = dGp + SJ_GPAD;
        std::vector<u64> words(C.SAbytes.size() / 8 + 3, 0); memcpy(words.data(), C.SAbytes.data(), C.SAbytes.size());
        u64 *dSA = up(be, words);
        u64 *dPos = be.template alloc<u64>(2 * nG1); u8 *dHit = be.template alloc<u8>(2 * nG1);
        const u64 saMask = (1ull << saBits) - 1;
        be.forEach(2 * nG1, [=] IDX_L (u64 o) {
            dHit[o] = 0; dPos[o] = ~0ull;
            if (dX[o] > 3) return;
            auto sa = [=](u64 i) { return seqRebase(packedGetW(dSA, i, saBits) & saMask, nG, nG1, nG2, N2bit); };
            dPos[o] = seqSearchOne(Gn, nGenomeNew, nG, gsb, nSAold, sa, dX + o, o < nG1, dHit + o);
        });
        R.same("insertion points", down(be, dPos, 2 * nG1), X.posByOff);
        u64 hits = 0; for (u8 h : down(be, dHit, 2 * nG1)) hits += h;
        R.eq("searches stopped at 10000 characters", hits, X.capHits);
        be.free(dGp); be.free(dSA); be.free(dPos); be.free(dHit);
        static const char *const TC[2][2] = {{"search: tie at a spacer, query + genome +", "search: tie at a spacer, query + genome -"}, {"search: tie at a spacer, query - genome +", "search: tie at a spacer, query - genome -"}};
        for (int a = 0; a < 2; a++) for (int b = 0; b < 2; b++) if (X.tie[a][b]) R.hit(TC[a][b], X.tie[a][b]);
        if (X.tieMoved[0]) R.hit("search: tie with a + strand entry at or past nG", X.tieMoved[0]);
        if (X.tieMoved[1]) R.hit("search: tie with a - strand entry behind the insertion point", X.tieMoved[1]);
        if (X.atZero) R.hit("search: below the first old suffix (0)", X.atZero);
        if (X.atEnd) R.hit("search: above the last old suffix", X.atEnd);
        if (X.between) R.hit("search: between", X.between);
        if (X.capHits) R.hit("search: stopped at 10000 characters", X.capHits);
    }
    checkBackend(be, R);
    // ---- ranks of the candidates (spacer runs as tokens) against a direct sort of their suffixes with memcmp (the shorter of two suffixes that agree to
    //      the end first): the same order, all ranks different
    {
        const u8 *xs = X.seqq.data() + SEQ_FILL;
        std::vector<u64> cand; for (u64 o = 0; o < 2 * nG1; o++) if (xs[o] < 4) cand.push_back(o);
        u64 *dOff = up(be, cand, 1); u64 *dRank = be.template alloc<u64>(cand.size() + 1);
        u64 rounds = 0;
        seqRankCandidates(be, dX, M, dOff, cand.size(), dRank, &rounds);
        const std::vector<u64> got = down(be, dRank, cand.size());
        std::vector<u64> ord(cand.size()); std::iota(ord.begin(), ord.end(), 0);
        std::sort(ord.begin(), ord.end(), [&](u64 a, u64 b) { if (a == b) return false; const u64 oa = cand[a], ob = cand[b]; const int c = memcmp(xs + oa, xs + ob, M - std::max(oa, ob)); return c ? c < 0 : oa > ob; });
        std::vector<u64> byRank(cand.size()); std::iota(byRank.begin(), byRank.end(), 0);
        std::sort(byRank.begin(), byRank.end(), [&](u64 a, u64 b) { return got[a] < got[b]; });
        R.same("candidates in rank order", byRank, ord);
        for (u64 i = 1; i < byRank.size(); i++) if (got[byRank[i]] == got[byRank[i - 1]]) { R.diff("two candidates share rank %llu", (unsigned long long)got[byRank[i]]); break; }
        be.free(dOff); be.free(dRank);
        R.hit("order: ranks of all candidates against memcmp"); if (rounds) R.hit("order: rounds 1 and more");
        if (X.cmpBefore) R.hit("order: same insertion point, decided before a spacer", X.cmpBefore);
        if (X.cmpBehind) R.hit("order: same insertion point, decided behind a spacer", X.cmpBehind);
    }
    be.free(dX); be.free(dG1);
    checkBackend(be, R);
    // ---- the whole insertion on the device arrays
    u64 saiStart[17]; saiStart[0] = 0; for (u32 i = 1; i <= C.L; i++) saiStart[i] = saiStart[i - 1] + (1ull << (2 * i));
    const idxchk::SaiWalk W = idxchk::saiWalkRef(X.Gnew, gsb, X.saNew, C.L);
    {
        u8 *dGold = up(be, C.Gold, 1);
        std::vector<u64> words(C.SAbytes.size() / 8 + 3, 0); memcpy(words.data(), C.SAbytes.data(), C.SAbytes.size());
        u64 *dSA = up(be, words);
        SeqParams P; P.nG = nG; P.nG1 = nG1; P.nG2 = nG2; P.nSAold = nSAold; P.GstrandBit = gsb; P.saIndexNbases = C.L;
        SeqDeviceResult D;
        seqInsertDevice(be, P, dGold, dSA, C.G1.data(), saiStart, D);
        checkBackend(be, R);
        R.eq("nInd", D.nInd, nInd); R.eq("nSAnew", D.nSAnew, nSAnew); R.eq("nGenomeNew", D.nGenomeNew, nGenomeNew); R.eq("nCapHits", D.nCapHits, X.capHits);
        std::vector<u64> expSA = X.saNew; expSA.push_back(0);
        R.eq("saWords", D.saWords, packedWords(nSAnew + 1, saBits));
        R.same("merged suffix array, words", down(be, D.dSApacked, D.saWords), idxchk::packRef(expSA, saBits, packedWords(nSAnew + 1, saBits)));
        std::vector<u8> expG(nGenomeNew + 2 * SJ_GPAD, 5); memcpy(expG.data() + SJ_GPAD, X.Gnew.data(), nGenomeNew);
        R.same("new genome text", down(be, D.dGnew, nGenomeNew + 2 * SJ_GPAD), expG);
        R.eq("bad first suffix", (u64)D.badFirstSuffix, (u64)W.bad);
        if (!W.bad) R.same("SAindex, words", down(be, D.dSAiPacked, D.saiWords), idxchk::packRef(W.e, gsb + 3, packedWords(saiStart[C.L], gsb + 3)));
        be.free(D.dSApacked); be.free(D.dGnew); be.free(D.dSAiPacked); be.free(dGold); be.free(dSA);
        if (nInd && X.pos[0] == 0) R.hit("merge: new entry at output index 0");
        if (nInd && X.pos[nInd - 1] == nSAold) R.hit("merge: new entries behind the last old entry");
        if (X.run3) R.hit("merge: run of 3 or more new entries", X.run3);
        if (nSAnew % 64 == 0) R.hit("merge: nSAnew a multiple of 64");
        if (nSAnew % 64 == 62) R.hit("merge: nSAnew 62 mod 64");
        R.hit("merge: zero entry and words behind the array"); R.hit(gsb == 32 ? "merge: GstrandBit 32" : "merge: GstrandBit 34");
        R.hit("insert: new genome text"); R.hit("insert: SAindex of the merged array");
        for (u64 o : X.off) { bool n = false; const u8 *xs = X.seqq.data() + SEQ_FILL; for (u32 k = 1; k < C.L; k++) { if (xs[o + k] == 5) break; if (xs[o + k] == 4) { n = true; break; } } if (n) { R.hit("insert: N inside the SAindex prefix of a new suffix"); break; } }
    }
    checkBackend(be, R);
    // ---- host buffers in and out, exact capacities between guard bytes
    {
        const u64 GUARD = 64, saB = packedBytes(nSAnew, saBits), saiB = packedBytes(saiStart[C.L], gsb + 3);
        std::vector<u8> oSA(saB + 2 * GUARD, 0xC3), oSAi(saiB + 2 * GUARD, 0xC3);
        SeqParams P; P.nG = nG; P.nG1 = nG1; P.nG2 = nG2; P.nSAold = nSAold; P.GstrandBit = gsb; P.saIndexNbases = C.L;
        SeqHostArgs A{C.Gold.data(), C.SAbytes.data(), C.SAbytes.size(), C.G1.data(), oSA.data() + GUARD, saB, oSAi.data() + GUARD, saiB};
        SeqDeviceResult D; u64 gotB = 0, gotBi = 0;
        R.eq("seqInsertHost return", (u64)(i64)seqInsertHost(be, P, A, D, gotB, gotBi), (u64)(i64)(W.bad ? -3 : 0));
        R.eq("seqInsertHost SA bytes", gotB, saB); R.eq("seqInsertHost SAindex bytes", gotBi, saiB);
        if (!W.bad) {
            std::vector<u64> expSA = X.saNew; expSA.push_back(0);
            const std::vector<u64> w = idxchk::packRef(expSA, saBits, packedWords(nSAnew + 1, saBits)), wi = idxchk::packRef(W.e, gsb + 3, packedWords(saiStart[C.L], gsb + 3));
            if (memcmp(w.data(), oSA.data() + GUARD, saB)) R.diff("seqInsertHost: SA bytes differ from the restatement");
            if (memcmp(wi.data(), oSAi.data() + GUARD, saiB)) R.diff("seqInsertHost: SAindex bytes differ from the restatement");
            for (u64 i = 0; i < GUARD; i++) if (oSA[i] != 0xC3 || oSA[oSA.size() - 1 - i] != 0xC3 || oSAi[i] != 0xC3 || oSAi[oSAi.size() - 1 - i] != 0xC3) { R.diff("seqInsertHost: guard bytes overwritten"); break; }
            R.hit("host: rc 0 bytes equal between guards");
            if (saOut) saOut->assign(oSA.begin() + GUARD, oSA.begin() + GUARD + saB);
            if (saiOut) saiOut->assign(oSAi.begin() + GUARD, oSAi.begin() + GUARD + saiB);
            A.saCap = saB - 1;
            R.eq("seqInsertHost return, SA one byte short", (u64)(i64)seqInsertHost(be, P, A, D, gotB, gotBi), (u64)(i64)-2); R.hit("host: rc -2 SA one byte short");
            A.saCap = saB; A.saiCap = saiB - 1;
            R.eq("seqInsertHost return, SAindex one byte short", (u64)(i64)seqInsertHost(be, P, A, D, gotB, gotBi), (u64)(i64)-2); R.hit("host: rc -2 SAindex one byte short");
            for (u64 i = 0; i < GUARD; i++) if (oSA[i] != 0xC3 || oSA[oSA.size() - 1 - i] != 0xC3 || oSAi[i] != 0xC3 || oSAi[oSAi.size() - 1 - i] != 0xC3) { R.diff("seqInsertHost: guard bytes overwritten by a refused call"); break; }
        }
    }
    checkBackend(be, R);
    R.end();
    return X;
}

// =====================================================================================================================
// fabricated cases: the old index by the product's buildAll (+ a junction block by sjdbInsertHost), gsb 32 and 34

static inline void padChr(std::vector<u8> &g, u64 bin) { const u64 n = g.size(); g.resize(((n + 1) / bin + 1) * bin, 5); }

template <class BE> bool buildOld(BE &be, SeqCase &C, const std::vector<u8> &G, u32 gsb, u32 L) {
    BuildParams P; P.nGenome = G.size(); P.GstrandBit = gsb; P.saIndexNbases = L; BuildResult B;
    if (buildAll(be, G.data(), P, (u8 *)nullptr, 0, (u8 *)nullptr, 0, B)) return false;
    C.SAbytes.assign(B.nSAbyte, 0); std::vector<u8> sai(B.nSAibyte);
    if (buildAll(be, G.data(), P, C.SAbytes.data(), B.nSAbyte, sai.data(), B.nSAibyte, B)) return false;
    C.Gold = G; C.nG = G.size(); C.nSAold = B.nSA; C.gsb = gsb; C.L = L;
    return true;
}

template <class BE> void runFabricated(BE &be, SeqReport &R) {
    Rng rng(77);
    for (int k = 0; k < 4; k++) {
        const u32 gsb = k == 1 ? 34 : 32, L = k == 2 ? 6 : 4; const u64 bin = k == 3 ? 64 : 128;
        std::vector<u8> G;
        for (int c = 0; c < 2; c++) { std::vector<u8> chr = idxchk::rndBases(rng, 300 + rng.below(500)); if (k == 2) chr[100] = 4; padChr(chr, bin); G.insert(G.end(), chr.begin(), chr.end()); }
        SeqCase C; C.name = "fabricated " + std::to_string(k);
        if (!buildOld(be, C, G, gsb, L)) { R.begin(C.name); R.diff("buildAll failed"); continue; }
        // added sequences: a copy of genome bases up to a chromosome end (ties at the spacer, both strands of the query against both of the genome),
        // its reverse complement, a poly-A and a poly-T beyond every run of the genome, two with the same tail, one with N
        std::vector<u8> G1; u64 firstEnd = 0; while (G[firstEnd] != 5) firstEnd++;
        auto add = [&](std::vector<u8> s) { padChr(s, bin); G1.insert(G1.end(), s.begin(), s.end()); };
        std::vector<u8> endCopy(G.begin() + firstEnd - 60, G.begin() + firstEnd); { std::vector<u8> s = idxchk::rndBases(rng, 40); s.insert(s.end(), endCopy.begin(), endCopy.end()); add(s); }
        { std::vector<u8> s(G.begin(), G.begin() + 50); std::vector<u8> rc; for (u64 i = s.size(); i-- > 0;) rc.push_back((u8)(3 - s[i])); std::vector<u8> t = idxchk::rndBases(rng, 30); t.insert(t.end(), rc.begin(), rc.end()); add(t); }
        { std::vector<u8> rc; for (u64 i = endCopy.size(); i-- > 0;) rc.push_back((u8)(3 - endCopy[i])); rc.insert(rc.end(), 25, (u8)(rng.below(4))); add(rc); }
        { std::vector<u8> s(G.begin(), G.begin() + 45); std::vector<u8> t = idxchk::rndBases(rng, 20); s.insert(s.begin(), t.begin(), t.end()); std::vector<u8> u(G.begin(), G.begin() + 45); add(u); add(s); }
        add(std::vector<u8>(40, 0)); add(std::vector<u8>(40, 3));
        const std::vector<u8> tail = idxchk::rndBases(rng, 30);
        for (int t = 0; t < 2; t++) { std::vector<u8> s = idxchk::rndBases(rng, 50 + 37 * t); s.insert(s.end(), tail.begin(), tail.end()); add(s); }
        { std::vector<u8> s = idxchk::rndBases(rng, 90); s[0] = 4; s[45] = 4; s[89] = 4; add(s); }
        C.G1 = G1;
        caseSeqInsert(be, R, C);
    }
}

template <class BE> void runStrandBitCases(BE &be, SeqReport &R) {
    R.begin("strand bit check");
    {   // the host form refuses before it touches an array: numbers alone
        SeqParams P; P.nG = (1ull << 32) - 256; P.nG1 = 256; P.nG2 = 0; P.nSAold = 10; P.GstrandBit = 32; P.saIndexNbases = 4;
        SeqHostArgs A{nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 0};
        SeqDeviceResult D; u64 b = 0, bi = 0;
        R.eq("seqInsertHost return, genome grown to 2^32", (u64)(i64)seqInsertHost(be, P, A, D, b, bi), (u64)(i64)-4); R.hit("host: rc -4 GstrandBit");
        if (!strstr(SEQ_STRANDBIT_ERROR, "cannot insert sequence on the fly because of strand GstrandBit problem")) R.diff("the error text is not the reference's");
    }
    R.eq("3 Gb + 5 Mb in 33 + 1 bits", (u64)seqStrandBitCheck(3100000000ull, 5000000ull, 34), 0); R.hit("strand bit: fits");
    R.eq("2^32 - 256 plus 256 bases in 32 + 1 bits", (u64)seqStrandBitCheck((1ull << 32) - 256, 256, 33), 1);
    R.eq("2^32 - 512 plus 256 bases in 32 + 1 bits", (u64)seqStrandBitCheck((1ull << 32) - 512, 256, 33), 0);
    R.eq("2^33 plus one bin in 33 + 1 bits", (u64)seqStrandBitCheck(1ull << 33, 1ull << 18, 34), 1); R.hit("strand bit: does not fit");
    R.eq("a 4 kb genome in 32 + 1 bits", (u64)seqStrandBitCheck(4096, 768, 33), 0);
    R.eq("a 4 kb genome in a 32-bit word", (u64)seqStrandBitCheck(4096, 768, 32), 1); R.hit("strand bit: below 32 counts as 32");
    R.end();
}

// =====================================================================================================================
// the cases of tests/golden/seq_insert/<case>/{plain,annot}/{old,new}/

static inline std::vector<u8> scanFastaRef(const std::vector<u8> &txt, u64 bin) {      // genomeScanFastaFiles.cpp:35-78 from N = 0
    std::vector<u8> g; u64 N = 0; size_t p = 0;
    while (p < txt.size()) {
        size_t e = p; while (e < txt.size() && txt[e] != '\n') e++;
        if (txt[p] == '>') { if (N > 0) N = ((N + 1) / bin + 1) * bin; g.resize(N, 5); }
        else for (size_t i = p; i < e; i++) { const signed char c = (signed char)txt[i]; if (c < 32) continue; g.push_back(c == 'A' || c == 'a' ? 0 : c == 'C' || c == 'c' ? 1 : c == 'G' || c == 'g' ? 2 : c == 'T' || c == 't' ? 3 : 4); N++; }
        p = e + 1;
    }
    N = ((N + 1) / bin + 1) * bin; g.resize(N, 5);
    return g;
}

template <class BE> void caseGolden(BE &be, SeqReport &R, const std::string &dir, const std::string &name) {
    std::vector<u8> fa;
    if (!readAll(dir + "/" + name + "/extra.fa", fa)) { R.begin("golden " + name); R.diff("no extra.fa under %s/%s", dir.c_str(), name.c_str()); return; }
    const std::vector<u8> G1 = scanFastaRef(fa, 256);
    for (const char *form : {"plain", "annot"}) {
        const std::string o = dir + "/" + name + "/" + form + "/old/", n = dir + "/" + name + "/" + form + "/new/";
        std::vector<u8> G, SA, SAI, par, chrs, G2, SA2, SAI2, info;
        if (!readAll(o + "Genome", G) || !readAll(o + "SA", SA) || !readAll(o + "SAindex", SAI) || !readAll(o + "genomeParameters.txt", par) || !readAll(o + "chrStart.txt", chrs) ||
            !readAll(n + "Genome", G2) || !readAll(n + "SA", SA2) || !readAll(n + "SAindex", SAI2) || !readAll(n + "sjdbInfo.txt", info)) {
            R.begin("golden " + name + "/" + form); R.diff("golden files missing under %s/%s/%s", dir.c_str(), name.c_str(), form); continue;
        }
        const u32 gsb = (u32)paramOf(par, "GstrandBit");
        u64 L; memcpy(&L, SAI.data(), 8);
        const u64 hdr = 8 * (L + 2);
        u64 nG = 0; { const std::string s(chrs.begin(), chrs.end()); size_t q = 0; while (q < s.size()) { nG = strtoull(s.c_str() + q, nullptr, 10); q = s.find('\n', q); if (q == std::string::npos) break; q++; } }
        const u64 sjdbN = strtoull((const char *)std::string(info.begin(), info.end()).c_str(), nullptr, 10);
        u64 ov = 0; { const std::string s(info.begin(), info.end()); ov = strtoull(s.c_str() + s.find_first_of(" \t") + 1, nullptr, 10); }
        const u64 Lsj = 2 * ov + 1;
        SeqCase C; C.name = "golden " + name + "/" + form; C.Gold = G; C.nG = nG; C.G1 = G1; C.SAbytes = SA; C.nSAold = SA.size() * 8 / (gsb + 1); C.gsb = gsb; C.L = (u32)L;
        std::vector<u8> saOut, saiOut;
        const RefInsert X = caseSeqInsert(be, R, C, &saOut, &saiOut);
        R.begin(C.name + " against the reference's bytes");
        const bool annot = std::string(form) == "annot";
        if (G2.size() != nG + G1.size() + sjdbN * Lsj) { R.diff("new Genome has %zu bytes, expected %llu", G2.size(), (unsigned long long)(nG + G1.size() + sjdbN * Lsj)); continue; }
        if (annot) {
            // the junction insertion adds nothing: the saved arrays are the sequence insertion's
            if (G2 != X.Gnew) R.diff("restated new genome text differs from the reference's Genome file");
            std::vector<u64> expSA = X.saNew; expSA.push_back(0);
            const u64 saB = packedBytes(X.saNew.size(), gsb + 1);
            const std::vector<u64> w = idxchk::packRef(expSA, gsb + 1, packedWords(expSA.size(), gsb + 1));
            R.eq("SA file size", SA2.size(), saB);
            if (SA2.size() == saB && memcmp(SA2.data(), w.data(), saB)) {
                const std::vector<u64> f = unpackBytes(SA2, X.saNew.size(), gsb + 1); u64 nd = 0, first = ~0ull;
                for (u64 i = 0; i < f.size(); i++) if (f[i] != X.saNew[i]) { nd++; if (first == ~0ull) first = i; }
                R.diff("restated insertion differs from the reference's SA file in %llu entries, the first at %llu", (unsigned long long)nd, (unsigned long long)first);
            }
            const idxchk::SaiWalk W = idxchk::saiWalkRef(X.Gnew, gsb, X.saNew, (u32)L);
            const std::vector<u64> wi = idxchk::packRef(W.e, gsb + 3, packedWords(W.start[L], gsb + 3));
            const u64 saiB = packedBytes(W.start[L], gsb + 3);
            R.eq("SAindex file size", SAI2.size(), hdr + saiB);
            if (SAI2.size() == hdr + saiB && memcmp(SAI2.data() + hdr, wi.data(), saiB)) R.diff("restated SAindex walk differs from the reference's SAindex file");
            R.hit("golden: restatement against the reference's files (annotated form)");
            if (saOut.size() != SA2.size() || memcmp(saOut.data(), SA2.data(), SA2.size())) R.diff("seqInsertHost: SA differs from the reference's file");
            if (saiOut.size() + hdr != SAI2.size() || memcmp(saiOut.data(), SAI2.data() + hdr, saiOut.size())) R.diff("seqInsertHost: SAindex differs from the reference's file");
            R.hit("golden: seqInsertHost against the reference's files (annotated form)");
        } else {
            // the chain: the junction of sj_new.tab goes into the index the sequence insertion left; Gsj = the junction block of the saved Genome
            const u64 nReal = nG + G1.size(), nSAmid = X.saNew.size();
            if (memcmp(G2.data(), X.Gnew.data(), nReal)) R.diff("restated new genome text differs from the reference's Genome file");
            std::vector<u8> isOld(sjdbN, 0);
            const u64 saiB = saiOut.size();
            u64 nNew = 0; for (u64 i = nReal; i < G2.size(); i++) nNew += G2[i] < 4;
            const u64 saB = packedBytes(nSAmid + 2 * nNew, gsb + 1), GUARD = 64;
            std::vector<u8> oSA(saB + 2 * GUARD, 0xC3), oSAi(saiB + 2 * GUARD, 0xC3);
            SjdbParams P; P.nGenomeOld = nReal; P.nGenomeReal = nReal; P.nSAold = nSAmid; P.GstrandBit = gsb; P.sjdbN = (u32)sjdbN; P.sjdbLength = (u32)Lsj; P.oldSjdbN = 0; P.sjNew = sjdbN; P.saIndexNbases = (u32)L;
            SjdbHostArgs A{X.Gnew.data(), saOut.data(), saOut.size(), G2.data() + nReal, isOld.data(), nullptr, oSA.data() + GUARD, saB, oSAi.data() + GUARD, saiB, saiOut.data()};
            u64 gotInd = 0, gotB = 0, gotBi = 0;
            R.eq("sjdbInsertHost return", (u64)(i64)sjdbInsertHost(be, P, A, gotInd, gotB, gotBi), 0);
            R.eq("sjdbInsertHost nInd", gotInd, 2 * nNew);
            if (SA2.size() != saB || memcmp(SA2.data(), oSA.data() + GUARD, saB)) R.diff("chain: SA differs from the reference's file");
            if (SAI2.size() != hdr + saiB || memcmp(SAI2.data() + hdr, oSAi.data() + GUARD, saiB)) R.diff("chain: SAindex differs from the reference's file");
            R.hit("golden: seqInsertHost then sjdbInsertHost against the reference's files (plain form)");
        }
        checkBackend(be, R);
        // the finding that rules out the from-scratch builder as the check: the same text indexed by buildAll gives another order
        if (annot && name == "tails") {
            SeqCase S;
            if (G2.size() == X.Gnew.size() && buildOld(be, S, std::vector<u8>(X.Gnew.begin(), X.Gnew.begin() + nG + G1.size()), gsb, (u32)L) && X.Gnew.size() == nG + G1.size() + sjdbN * Lsj) {
                // compare the order of the chromosome + added suffixes only (the junction block is not in the from-scratch text)
                const std::vector<u64> scratch = unpackBytes(S.SAbytes, S.nSAold, gsb + 1); std::vector<u64> ours;
                const u64 N2bit = 1ull << gsb, nG2 = sjdbN * Lsj, nReal = nG + G1.size();
                for (u64 v : X.saNew) { if (v & N2bit) { if ((v & ~N2bit) >= nG2) ours.push_back((v - nG2)); } else if (v < nReal) ours.push_back(v); }
                u64 nd = 0; if (ours.size() == scratch.size()) for (u64 i = 0; i < ours.size(); i++) nd += ours[i] != scratch[i];
                printf("tails: %llu of %zu entries differ from the from-scratch order\n", (unsigned long long)nd, ours.size());
                if (ours.size() == scratch.size() && nd) R.hit("golden: differs from a from-scratch order");
            }
        }
        R.end();
    }
}

template <class BE> void runGolden(BE &be, SeqReport &R, const std::string &dir) {
    for (const char *c : {"tails", "dups", "ns", "ends", "cap"}) caseGolden(be, R, dir, c);
}

} // namespace seqchk
