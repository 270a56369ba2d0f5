// cand_log_ref.h -- TEST INFRASTRUCTURE: synthetic candidate logs and the sequential list they must leave, shared by oracle/stitch_routines_check.cpp (replayWindow and
// recordCandidate one call at a time) and oracle/tail_routines_check.cpp (k_stitch_replay over windows made by hand).  Included behind star_oracle.cpp (Tr, Oracle::blocksOverlap)
// and the engine's headers (staramd_transcript, REC_HDR); the including file defines rng / rnd().
//   candLogSequential   stitchWindowAligns.cpp:232-303 one candidate after the other (the form of star_oracle.cpp:705-723, the maxScoreMate pre-filter as in replayWindow), with the
//                       arena's book-keeping (bump pointer, compaction when it hits the end, the two overflow clauses) and, per mate, the smallest Score + range among the
//                       candidates that only the maxScoreMate clause let through (DWinOut::sens)
#pragma once
#include <vector>
#include <algorithm>
#include <climits>

#define CAND_NE_MAX 6u                 // exons of a synthetic candidate
struct Cand { staramd_transcript t; staramd_exon ex[CAND_NE_MAX]; };
static Tr asTr(const staramd_exon *ex, u32 ne, u32 mapped) { Tr t; memset(&t, 0, sizeof(t)); t.nExons = ne; t.mappedLength = mapped; for (u32 k = 0; k < ne; k++) { t.ex[k][EX_R] = ex[k].R; t.ex[k][EX_L] = ex[k].L; t.ex[k][EX_G] = ex[k].G; } return t; }
static void randomBytes(void *p, size_t n) { u8 *b = (u8 *)p; for (size_t i = 0; i < n; i++) b[i] = (u8)rng(); }
// exons on the diagonals diag[] (G - R): ne sorted pieces of the read [0, span)
static void layExons(Cand &c, u32 ne, const u64 *diag, u32 nDiag, u32 span) {
    std::vector<u32> cut; while (cut.size() < 2 * ne) { const u32 p = rnd(span + 1); if (std::find(cut.begin(), cut.end(), p) == cut.end()) cut.push_back(p); } std::sort(cut.begin(), cut.end());
    u32 mapped = 0;
    for (u32 k = 0; k < ne; k++) { staramd_exon &e = c.ex[k]; randomBytes(&e, sizeof(e)); e.R = (u16)cut[2 * k]; e.L = (u16)(cut[2 * k + 1] - cut[2 * k]); e.G = diag[rnd(nDiag)] + e.R; e.pad0 = e.pad1 = 0; mapped += e.L; }
    c.t.nExons = (u16)ne; c.t.mappedLength = mapped;
}
// the bytes of a log as candPool holds them: header, then the exon rows
static void candLogBytes(const std::vector<Cand> &cand, std::vector<u8> &pool) {
    for (const Cand &c : cand) { const u8 *p = (const u8 *)&c.t; pool.insert(pool.end(), p, p + REC_HDR); p = (const u8 *)c.ex; pool.insert(pool.end(), p, p + 32u * c.t.nExons); }
}

// what happened on the way (the classes of the stitch check)
struct CandLogStats { u64 list64 = 0, list128 = 0, tail = 0, removeTrip2 = 0, behindFull = 0, ovfClause1 = 0, ovfClause2 = 0, compactFrees = 0, rank0Over64 = 0, insertFull = 0; };
struct CandLogResult { std::vector<u32> list; bool ovf = false; i32 sens[2] = {INT_MAX, INT_MAX}; };
// arenaBytes 0: no arena (the list alone)
static CandLogResult candLogSequential(const std::vector<Cand> &cand, u32 Nmax, i32 range, bool chim, const i32 minIn[2], u32 arenaBytes, CandLogStats *st) {
    CandLogResult r; std::vector<u32> &list = r.list; i32 M[2] = {minIn[0], minIn[1]}; u32 top = 0; bool &ovf = r.ovf; const u32 nCand = (u32)cand.size();
    for (u32 k = 0; k < nCand && !ovf; k++) {
        const Cand &c = cand[k]; const int Score = c.t.maxScore, f = c.t.iFrag; i32 Mf = 0;
        if (f >= 0) { M[f] = std::max(M[f], Score); Mf = M[f]; }
        const i32 best = list.empty() ? 0 : cand[list[0]].t.maxScore;
        const bool c1 = Score + range >= best || chim, c2 = f >= 0 && Score + range >= Mf;
        if (!(c1 || c2)) continue;
        if (!c1) r.sens[f] = std::min(r.sens[f], Score + range);
        const u32 n0 = (u32)list.size(); if (st) { if (n0 > 64) st->list64++; if (n0 > 128) st->list128++; }
        const Tr tn = asTr(c.ex, c.t.nExons, c.t.mappedLength);
        u32 iTr = 0, orig = 0; bool blocked = false;
        while (iTr < list.size()) {
            const Cand &o = cand[list[iTr]]; const Tr to = asTr(o.ex, o.t.nExons, o.t.mappedLength);
            const u64 nOverlap = Oracle::blocksOverlap(tn, to), uNew = tn.mappedLength - nOverlap, uOld = to.mappedLength - nOverlap;
            if (uNew == 0 && Score < o.t.maxScore) { blocked = true; if (st && orig < 64 && n0 > 64) st->tail++; break; }
            else if (uOld == 0) { list.erase(list.begin() + iTr); if (st && orig >= 64) st->removeTrip2++; }
            else iTr++;
            orig++;
        }
        if (blocked) continue;
        for (iTr = 0; iTr < list.size(); iTr++) if (Score > cand[list[iTr]].t.maxScore || (Score == cand[list[iTr]].t.maxScore && c.t.gLength < cand[list[iTr]].t.gLength)) break;
        if (iTr >= Nmax) { if (st) st->behindFull++; continue; }
        const u32 need = REC_HDR + 32u * c.t.nExons;
        if (arenaBytes && top + need > arenaBytes) {
            u32 live = 0; for (u32 id : list) live += REC_HDR + 32u * cand[id].t.nExons;
            const bool freed = live < top; top = live;
            if (top + need > arenaBytes) { ovf = true; if (st) st->ovfClause1++; break; }
            if (top * 4u > arenaBytes * 3u) { ovf = true; if (st) st->ovfClause2++; break; }
            if (freed && st) st->compactFrees++;
        }
        top += need;
        if (st) { if (iTr == 0 && list.size() > 64) st->rank0Over64++; if (list.size() == Nmax) st->insertFull++; }
        list.insert(list.begin() + iTr, k); if (list.size() > Nmax) list.pop_back();
    }
    return r;
}
