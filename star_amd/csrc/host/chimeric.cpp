// chimeric.cpp -- chimeric alignment detection on the transcripts of all windows (--chimSegmentMin > 0): two alignments of one read that together cover it.
// Host post-map code.  The device returns every recorded transcript of every window for it (resultSelect 0, chimSegmentMinPositive 1: stitchWindowAligns.cpp:247)
// -- or, for chimericDetectionOld on an engine that can (resultSelect 2), runs the partner loop itself and returns its outcome beside the transcripts multMapSelect
// can pick (k_stitch.hip chimSelectPartner).  Which two alignments may pair, and with what score, is stated once for both sides in ../chim_pair.h.
// What restates which lines of the reference:
//   chim_pair.h chimExtent, chimMotifStrand      source/ChimericSegment.cpp:5-16 = source/ReadAlign_chimericDetectionOld.cpp:31-43, :50-57, :61-64
//   chim_pair.h chimPairEligible                 source/ChimericDetection_chimericDetectionMult.cpp:9-16 = ReadAlign_chimericDetectionOld.cpp:66-73
//   chim_pair.h blocksOverlap                    source/blocksOverlap.cpp:3-40
//   cigarP                                       source/ReadAlign_outputTranscriptCIGARp.cpp:4-68
//   bracketJunction                              ReadAlign_chimericDetectionOld.cpp:130-143 = source/ChimericAlign_chimericStitching.cpp:22-33
//   scanJunction                                 ReadAlign_chimericDetectionOld.cpp:143-229 = ChimericAlign_chimericStitching.cpp:35-122
//   shiftToJunction                              ReadAlign_chimericDetectionOld.cpp:231-283 = ChimericAlign_chimericStitching.cpp:125-170
//   chimAlignScore                               source/Transcript_alignScore.cpp:4-58
//   chimericMergedToPair, pushPair               source/ReadAlign_peOverlapMergeMap.cpp:309-368, source/ReadAlign_chimericDetectionPEmerged.cpp:12-32
//   writeJunctionLine                            source/ReadAlign_chimericDetectionOldOutput.cpp:61-71 = source/ChimericAlign_chimericJunctionOutput.cpp:4-23
//   chimericDetectionOld                         source/ReadAlign_chimericDetection.cpp:16-57, ReadAlign_chimericDetectionOld.cpp:7-312, ReadAlign_chimericDetectionOldOutput.cpp:5-16
//   chimericDetectionMult                        ChimericDetection_chimericDetectionMult.cpp:23-138, source/ChimericAlign.cpp:3-32 (chimericCheck), ChimericAlign_chimericStitching.cpp:3-181
#include "host.h"
#include "../chim_pair.h"
#include <algorithm>
#include <cstring>
#include <cmath>

namespace staramd {

namespace {
// the read as the detection sees it.  b / ir: the read that was mapped; nameBatch / nameIr: the pair it was merged from (--peOverlapNbasesMin), when it was
struct ReadView {
    uint64_t Lread, readLength[2];
    const uint8_t *Read1;
    int nMates;
    bool merged;                                   // b holds merged mates: a single-end read as far as the detection goes (ReadAlign_chimericDetectionPEmerged.cpp:12-32)
    const ReadBatch &nb; uint32_t nir;             // where the name and the read group come from: the pair when merged
    const uint32_t *mateStart;                     // merged: where the mates start in the merged read
    uint64_t readLengthOriginal[2], readLengthPair;   // the CIGARp is written against the lengths before clipping (ReadAlign_outputTranscriptCIGARp.cpp:13,25,55)
    const uint8_t *G; int64_t nG;
    uint8_t genome(uint64_t p) const { const int64_t q = (int64_t)p; return q >= 0 && q < nG ? G[q] : 5; }

    ReadView(const RunParams &P, const GenomeIndex &gi, const ReadBatch &b, uint32_t ir, const ReadBatch *nameBatch, uint32_t nameIr, const uint32_t *mateStart_)
        : Lread(b.readOffset[ir + 1] - b.readOffset[ir]), Read1(b.bases.data() + b.readOffset[ir]), nMates(nameBatch ? 1 : (int)P.dev.readNmates), merged(nameBatch != nullptr),
          nb(nameBatch ? *nameBatch : b), nir(nameBatch ? nameIr : ir), mateStart(mateStart_), G(gi.G.data()), nG((int64_t)gi.G.size()) {
        readLength[0] = b.mate1Length[ir]; readLength[1] = nMates == 2 ? Lread - b.mate1Length[ir] - 1 : 0;
        readLengthOriginal[0] = merged ? Lread : (uint64_t)b.seqSpan[0][ir].len; readLengthOriginal[1] = nMates == 2 ? (uint64_t)b.seqSpan[1][ir].len : 0;
        readLengthPair = nMates == 2 ? readLengthOriginal[0] + readLengthOriginal[1] + 1 : readLengthOriginal[0];
    }
};

// one recorded alignment as a candidate segment: where it lies on the read and the strand its intron motifs imply (ChimericSegment)
struct Segment { const staramd_transcript *t; const staramd_exon *ex; ChimExtent ro; uint32_t str; };
Segment makeSegment(const ReadView &rv, const staramd_transcript &t, const staramd_exon *exAll, bool bothMotifsIsUndefined) {
    const staramd_exon *ex = exAll + t.exonOffset;
    return Segment{&t, ex, chimExtent(t.Str, ex[0], ex[t.nExons - 1], rv.Lread, rv.readLength[0]), chimMotifStrand(t.Str, t.intronMotifs, bothMotifsIsUndefined)};
}
void load(ChimTr &c, const Segment &s) { c.t = *s.t; memcpy(c.ex, s.ex, sizeof(staramd_exon) * s.t->nExons); }

inline void appendU(std::string &s, uint64_t v) { char b[24]; int n = 0; do { b[n++] = (char)('0' + v % 10); v /= 10; } while (v); while (n) s.push_back(b[--n]); }
inline void appendI(std::string &s, int v) { if (v < 0) { s.push_back('-'); appendU(s, (uint64_t)(-(int64_t)v)); } else appendU(s, (uint64_t)v); }

std::string cigarP(const ChimTr &c, const ReadView &rv) {
    std::string s;
    const uint64_t *readLength = rv.readLengthOriginal;
    const uint64_t leftMate = rv.nMates > 1 ? c.t.Str : 0;
    const uint32_t ne = c.t.nExons;
    uint64_t trimL = c.ex[0].R - (c.ex[0].R < readLength[leftMate] ? 0 : readLength[leftMate] + 1);
    if (trimL > 0) { appendU(s, trimL); s.push_back('S'); }
    for (uint32_t ii = 0; ii < ne; ii++) {
        if (ii > 0) {
            uint64_t prevEnd = c.ex[ii - 1].G + c.ex[ii - 1].L, gapG = c.ex[ii].G - prevEnd;
            if (c.ex[ii].G >= prevEnd) {
                if (c.ex[ii - 1].canonSJ == -3) {
                    uint64_t s1 = readLength[leftMate] - (c.ex[ii - 1].R + c.ex[ii - 1].L), s2 = c.ex[ii].R - (readLength[leftMate] + 1);
                    if (s1 > 0) { appendU(s, s1); s.push_back('S'); }
                    appendU(s, gapG); s.push_back('p');
                    if (s2 > 0) { appendU(s, s2); s.push_back('S'); }
                } else {
                    uint64_t gapR = (uint64_t)c.ex[ii].R - c.ex[ii - 1].R - c.ex[ii - 1].L;
                    if (gapR > 0) { appendU(s, gapR); s.push_back('I'); }
                    if (c.ex[ii - 1].canonSJ >= 0 || c.ex[ii - 1].sjAnnot == 1) { appendU(s, gapG); s.push_back('N'); }
                    else if (gapG > 0) { appendU(s, gapG); s.push_back('D'); }
                }
            } else { s.push_back('-'); appendU(s, prevEnd - c.ex[ii].G); s.push_back('p'); }
        }
        appendU(s, c.ex[ii].L); s.push_back('M');
    }
    trimL = (c.ex[ne - 1].R < readLength[leftMate] ? readLength[leftMate] : rv.readLengthPair) - c.ex[ne - 1].R - c.ex[ne - 1].L;
    if (trimL > 0) { appendU(s, trimL); s.push_back('S'); }
    return s;
}

// the chimeric junction of two segments in read order: the last genome base before it on either side, the repeat lengths around it, and its motif
// (-1: the mates bracket it, 0: none, 1: GT/AG, 2: CT/AC)
struct ChimJunction { uint64_t J0 = 0, J1 = 0, repeat0 = 0, repeat1 = 0; int motif = 0; };

// mates bracket the junction: it lies somewhere behind segment 0's last block and before segment 1's first
ChimJunction bracketJunction(const ChimTr &t0, const ChimTr &t1, uint32_t e0, uint32_t e1) {
    const staramd_exon &x0 = t0.ex[e0], &x1 = t1.ex[e1];
    ChimJunction j; j.motif = -1;
    j.J0 = t0.t.Str == 1 ? x0.G - 1 : x0.G + x0.L; j.J1 = t1.t.Str == 0 ? x1.G - 1 : x1.G + x1.L;
    return j;
}

// the genome along one segment in read orientation: at(k) = the base k steps from g0 along the walk, complemented on the minus strand (5 outside the genome).
// Offsets are unsigned and wrap as the reference's do: at(jR - 1) at jR = 0 is the base before g0
struct Side {
    const ReadView &rv; uint64_t g0; bool up, comp;
    uint8_t at(uint64_t k) const { const uint8_t b = rv.genome(up ? g0 + k : g0 - k); return comp && b < 4 ? 3 - b : b; }
};
// from genome position g of a segment on strand Str, with the read (forward) or against it
Side walk(const ReadView &rv, uint32_t Str, uint64_t g, bool forward) { return Side{rv, g, (Str == 0) == forward, Str != 0}; }
// block x of a segment on strand Str from its first base in read orientation; shift moves the origin (segment 1 is read at segment 0's offsets)
Side blockSide(const ReadView &rv, uint32_t Str, const staramd_exon &x, uint64_t shift) { return walk(rv, Str, Str == 0 ? x.G + shift : x.G + x.L - 1 - shift, true); }
// how far the two sides agree, up to 100 bases
uint64_t agreeLength(const Side &a, const Side &b) { uint64_t k = 0; while (k < 100 && a.at(k) == b.at(k)) k++; return k; }

// the scan for the chimeric junction inside a mate: every position between the start of segment 0's last block and the end of segment 1's first block is scored by
// which genome the read base agrees with; a GT/AG (CT/AC) pair at the position wins ties.  false = rejected (N in the read, or in the genome with filterGenomicN)
struct JunctionScan { uint64_t roStart0, roStartB, jRbest; int motif; };
bool scanJunction(const ChimParams &C, const ReadView &rv, const ChimTr &t0, const ChimTr &t1, uint32_t e0, uint32_t e1, uint32_t chimStr, JunctionScan &js) {
    const staramd_exon &x0 = t0.ex[e0], &x1 = t1.ex[e1];
    const uint64_t roStart0 = t0.t.Str == 0 ? x0.R : rv.Lread - x0.R - x0.L;
    const uint64_t roStartB = t1.t.Str == 0 ? x1.R : rv.Lread - x1.R - x1.L;
    const Side s0 = blockSide(rv, t0.t.Str, x0, 0), s1 = blockSide(rv, t1.t.Str, x1, roStart0 - roStartB);
    uint64_t jR, jRbest = 0; int jScore = 0, jMotif = 0, jScoreBest = -999999, jScoreJ = 0, chimMotif = 0;
    uint64_t jRmax = roStartB + x1.L;
    jRmax = jRmax > roStart0 ? jRmax - roStart0 - 1 : 0;
    for (jR = 0; jR < jRmax; jR++) {
        if (jR == rv.readLength[0]) jR++;                              // the base between the mates
        const uint8_t bR = rv.Read1[roStart0 + jR], b0 = s0.at(jR), b1 = s1.at(jR);
        if ((C.filterGenomicN && (b0 > 3 || b1 > 3)) || bR > 3) return false;
        const uint8_t b01 = s0.at(jR + 1), b02 = s0.at(jR + 2), b11 = s1.at(jR - 1);
        jMotif = 0;
        if (b01 == 2 && b02 == 3 && b11 == 0 && b1 == 2) { if (chimStr != 2) jMotif = 1; }
        else if (b01 == 1 && b02 == 3 && b11 == 0 && b1 == 1) { if (chimStr != 1) jMotif = 2; }
        if (bR == b0 && bR != b1) jScore++; else if (bR != b0 && bR == b1) jScore--;
        jScoreJ = jMotif == 0 ? jScore + C.scoreJunctionNonGTAG : jScore;
        if (jScoreJ > jScoreBest || (jScoreJ == jScoreBest && jMotif > 0)) { chimMotif = jMotif; jRbest = jR; jScoreBest = jScoreJ; }
    }
    js.roStart0 = roStart0; js.roStartB = roStartB; js.jRbest = jRbest; js.motif = chimMotif;
    return true;
}

// the two blocks next to the junction are cut / extended to meet at it, then the repeat lengths around it: how far the genome behind the junction on one side
// goes on like the genome on the other side
ChimJunction shiftToJunction(const ReadView &rv, ChimTr &t0, ChimTr &t1, uint32_t e0, uint32_t e1, const JunctionScan &js) {
    staramd_exon &x0 = t0.ex[e0], &x1 = t1.ex[e1];
    const uint64_t roStart0 = js.roStart0, roStartB = js.roStartB, jRbest = js.jRbest;
    const uint32_t Str0 = t0.t.Str, Str1 = t1.t.Str;
    ChimJunction j;
    j.motif = js.motif;
    if (Str0 == 1) { x0.R = (uint16_t)(x0.R + x0.L - jRbest - 1); x0.G += x0.L - jRbest - 1; x0.L = (uint16_t)(jRbest + 1); j.J0 = x0.G - 1; }
    else { x0.L = (uint16_t)(jRbest + 1); j.J0 = x0.G + x0.L; }
    if (Str1 == 0) {
        x1.R = (uint16_t)(x1.R + roStart0 + jRbest + 1 - roStartB); x1.G += roStart0 + jRbest + 1 - roStartB;
        x1.L = (uint16_t)(roStartB + x1.L - roStart0 - jRbest - 1); j.J1 = x1.G - 1;
    } else { x1.L = (uint16_t)(roStartB + x1.L - roStart0 - jRbest - 1); j.J1 = x1.G + x1.L; }
    j.repeat1 = agreeLength(walk(rv, Str0, j.J0, true), walk(rv, Str1, Str1 == 0 ? j.J1 + 1 : j.J1 - 1, true));
    j.repeat0 = agreeLength(walk(rv, Str0, Str0 == 0 ? j.J0 - 1 : j.J0 + 1, false), walk(rv, Str1, j.J1, false));
    return j;
}
} // namespace

// score of an alignment recomputed from its blocks (after the junction shift)
int chimAlignScore(const staramd_params &D, const GenomeIndex &gi, const uint8_t *Read1, uint64_t Lread, ChimTr &c) {
    int maxScore = 0; uint32_t nMM = 0;
    c.t.maxScore = 0; c.t.nMM = 0;
    const uint32_t ne = c.t.nExons;
    if (ne == 0) return 0;
    for (uint32_t iex = 0; iex < ne; iex++)
        for (uint32_t ii = 0; ii < c.ex[iex].L; ii++) {
            uint64_t rp = (uint64_t)c.ex[iex].R + ii;
            uint8_t r1 = c.t.roStr == 0 ? Read1[rp] : Read1[Lread - 1 - rp];
            if (c.t.roStr != 0 && r1 < 4) r1 = 3 - r1;
            uint8_t g1 = gi.G[c.ex[iex].G + ii];
            if (r1 > 3 || g1 > 3) continue;
            if (r1 == g1) ++maxScore; else { --maxScore; ++nMM; }
        }
    for (uint32_t iex = 0; iex + 1 < ne; iex++) {
        if (c.ex[iex].sjAnnot == 1) { maxScore += D.sjdbScore; continue; }
        switch (c.ex[iex].canonSJ) {
            case -3: break;
            case -2: maxScore += (int)((int64_t)c.ex[iex + 1].R - c.ex[iex].R - c.ex[iex].L) * D.scoreInsBase + D.scoreInsOpen; break;
            case -1: maxScore += (int)((int64_t)(c.ex[iex + 1].G - c.ex[iex].G) - c.ex[iex].L) * D.scoreDelBase + D.scoreDelOpen; break;
            case 0: maxScore += D.scoreGapNoncan + D.scoreGap; break;
            case 1: case 2: maxScore += D.scoreGap; break;
            case 3: case 4: maxScore += D.scoreGapGCAG + D.scoreGap; break;
            case 5: case 6: maxScore += D.scoreGapATAC + D.scoreGap; break;
        }
    }
    if (D.scoreGenomicLengthLog2scale != 0) {
        unsigned long long gl = std::max(1ULL, (unsigned long long)(c.ex[ne - 1].G + c.ex[ne - 1].L - c.ex[0].G));
        maxScore += int(std::ceil(std::log2((double)gl) * D.scoreGenomicLengthLog2scale - 0.5));
    }
    c.t.maxScore = maxScore; c.t.nMM = nMM;
    return maxScore;
}

namespace {
// ReadAlign::peOverlapChimericSEtoPE: both segments of a chimera of merged mates cut back into the two mates; the shortest one-mate part of either segment (ties:
// the one whose junction lies deeper in its mate) is dropped, so that one mate is chimerically split, not both
void chimericMergedToPair(const ReadView &rv, const ChimTr &se1, const ChimTr &se2, ChimTr tmp[2]) {
    const ReadBatch &nb = rv.nb; const uint32_t nir = rv.nir;
    const uint64_t LreadPE = nb.readOffset[nir + 1] - nb.readOffset[nir];
    const uint64_t readLengthPE[2] = {nb.mate1Length[nir], LreadPE - nb.mate1Length[nir] - 1};
    const uint64_t readLengthOriginalPE[2] = {nb.seqSpan[0][nir].len, nb.seqSpan[1][nir].len};
    mergedAlignToPair(tmp[0], rv.mateStart, se1.t, se1.ex, rv.Lread, readLengthPE, LreadPE);
    mergedAlignToPair(tmp[1], rv.mateStart, se2.t, se2.ex, rv.Lread, readLengthPE, LreadPE);
    uint64_t segLen[2][2] = {{0, 0}, {0, 0}}, segEx[2] = {0, 0}, i1 = 0, i2 = 0, posOfJunctionInRead = 0;
    for (uint64_t ii = 0; ii < 2; ii++) {
        for (uint32_t iex = 0; iex < tmp[ii].t.nExons; iex++) {
            if (tmp[ii].ex[iex].iFrag == tmp[ii].ex[0].iFrag) { segLen[ii][0] += tmp[ii].ex[iex].L; segEx[ii] = iex; } else segLen[ii][1] += tmp[ii].ex[iex].L;
        }
        const uint64_t readLen0 = readLengthOriginalPE[tmp[ii].ex[0].iFrag], readLen1 = readLengthOriginalPE[1 - tmp[ii].ex[0].iFrag];
        for (uint64_t jj = 0; jj < 2; jj++) {
            const uint64_t R = tmp[ii].ex[jj].R;
            const uint64_t cur = R > readLen0 ? readLen0 + readLen1 + 1 - R : R;
            if (segLen[ii][jj] < segLen[i1][i2] || (segLen[ii][jj] == segLen[i1][i2] && cur > posOfJunctionInRead)) { posOfJunctionInRead = cur; i1 = ii; i2 = jj; }
        }
    }
    ChimTr &c = tmp[i1];
    if (i2 == 1) c.t.nExons = (uint16_t)(segEx[i1] + 1);
    else {
        const uint32_t shift = (uint32_t)segEx[i1] + 1, nNew = c.t.nExons - shift;
        for (uint32_t iex = 0; iex < nNew; iex++) c.ex[iex] = c.ex[iex + shift];
        c.t.nExons = (uint16_t)nNew;
    }
}

// the two segments go to the BAM / Chimeric.out.sam writers; those of merged mates are cut back into the pair first.  rescore: both are scored anew from their
// blocks, on the read the records will show (the pair when merged)
void pushPair(std::vector<ChimPair> &bamOut, const RunParams &P, const GenomeIndex &gi, const ReadView &rv, const ChimTr &a0, const ChimTr &a1, bool best,
              const VarOverlap &var0, const VarOverlap &var1, bool rescore) {
    bamOut.push_back(ChimPair{a0, a1, best, var0, var1});
    ChimPair &cp = bamOut.back();
    const uint8_t *Read1 = rv.Read1; uint64_t Lread = rv.Lread;
    if (rv.merged) {
        ChimTr tmp[2];
        chimericMergedToPair(rv, a0, a1, tmp);
        cp.a1 = tmp[0]; cp.a2 = tmp[1];
        Read1 = rv.nb.bases.data() + rv.nb.readOffset[rv.nir]; Lread = rv.nb.readOffset[rv.nir + 1] - rv.nb.readOffset[rv.nir];
    }
    if (rescore) { chimAlignScore(P.dev, gi, Read1, Lread, cp.a1); chimAlignScore(P.dev, gi, Read1, Lread, cp.a2); }
}

// one line of Chimeric.out.junction: 14 columns; the multimapping algorithm adds six, then the read group where the SAM attributes have one
struct MultColumns { uint64_t chimN; int maxPossibleAlignScore, maxNonChimAlignScore, chimScore, chimScoreBest; };
void writeJunctionLine(std::string &out, const RunParams &P, const GenomeIndex &gi, const ReadView &rv, const ChimTr &a0, const ChimTr &a1, const ChimJunction &j, const MultColumns *m) {
    const ChimTr *a[2] = {&a0, &a1}; const uint64_t J[2] = {j.J0, j.J1};
    const uint64_t c[2] = {gi.chrStart[a0.t.Chr], gi.chrStart[a1.t.Chr]};
    for (int k = 0; k < 2; k++) { out += gi.chrName[a[k]->t.Chr]; out.push_back('\t'); appendU(out, J[k] - c[k] + 1); out.push_back('\t'); out.push_back(a[k]->t.Str == 0 ? '+' : '-'); out.push_back('\t'); }
    appendI(out, j.motif); out.push_back('\t'); appendU(out, j.repeat0); out.push_back('\t'); appendU(out, j.repeat1); out.push_back('\t'); out += rv.nb.name(rv.nir);
    for (int k = 0; k < 2; k++) { out.push_back('\t'); appendU(out, a[k]->ex[0].G - c[k] + 1); out.push_back('\t'); out += cigarP(*a[k], rv); }
    if (m) {
        out.push_back('\t'); appendU(out, m->chimN); out.push_back('\t'); appendI(out, m->maxPossibleAlignScore); out.push_back('\t'); appendI(out, m->maxNonChimAlignScore);
        out.push_back('\t'); appendI(out, m->chimScore); out.push_back('\t'); appendI(out, m->chimScoreBest); out += rv.merged ? "\t1" : "\t0";       // PEmerged_bool
    }
    if (P.attrHasRG) { out.push_back('\t'); out += P.outSAMattrRG.at(rv.nb.fileOf(rv.nir)); }   // outSAMattrPresent.RG
    out.push_back('\n');
}

// ---- the steps of chimericDetectionOld ----
// may trBest be the main segment: long enough, chimSegmentMin unmapped bases at one end of the read, no non-canonical junction, one strand (:19-25)
bool mainSegmentOk(const ChimParams &C, const ReadView &rv, const Segment &s) {
    const staramd_transcript &t = *s.t; const staramd_exon &last = s.ex[t.nExons - 1];
    return C.segmentMin > 0 && t.rLength >= C.segmentMin && ((uint64_t)last.R + last.L + C.segmentMin <= rv.Lread || s.ex[0].R >= C.segmentMin)
           && t.intronMotifs[0] == 0 && (t.intronMotifs[1] == 0 || t.intronMotifs[2] == 0);
}

// the best-scoring alignment that may pair with the main segment, and the score of the runner-up that shares no block with it (:45-97): the head of every other
// window and the other alignments of the main segment's own.  k_stitch.hip chimSelectPartner is the same loop over the device's pools
struct Partner { int scoreBest = 0, scoreNext = 0; uint32_t strBest = 0; const staramd_transcript *t = nullptr; };
Partner partnerOverWindows(const ChimParams &C, const ReadView &rv, const ReadAligns &ra, const Segment &mainSeg) {
    Partner p; Segment best{};
    for (uint32_t k0 = 0; k0 < ra.nTr;) {                              // windows: consecutive transcripts with the same iW, best first
        uint32_t k1 = k0;
        while (k1 < ra.nTr && ra.T[k1].iW == ra.T[k0].iW) k1++;
        const bool bestWindow = mainSeg.t == ra.T + k0;
        for (uint32_t k = k0; k < k1; k++) {
            const uint32_t iWt = k - k0;
            if (!bestWindow && iWt > 0) break;
            if (bestWindow && iWt == 0) continue;
            if (ra.T[k].intronMotifs[0] > 0) continue;
            const Segment s = makeSegment(rv, ra.T[k], ra.ex, false);
            if (mainSeg.str != 0 && s.str != 0 && mainSeg.str != s.str) continue;
            uint64_t chimOverlap;
            if (!chimPairEligible(mainSeg.ro, s.ro, rv.readLength[0], C.segmentMin, C.segmentReadGapMax, chimOverlap)) continue;
            const int chimScore = mainSeg.t->maxScore + s.t->maxScore - (int)chimOverlap;
            uint64_t overlap1 = 0;
            if (iWt > 0 && p.scoreBest > 0) overlap1 = blocksOverlap(best.ex, (uint32_t)best.t->nExons, s.ex, (uint32_t)s.t->nExons);
            if (chimScore > p.scoreBest) {
                best = s; p.t = s.t;
                if (overlap1 == 0) p.scoreNext = p.scoreBest;
                p.scoreBest = chimScore;
                p.strBest = s.str;
            } else if (chimScore > p.scoreNext && overlap1 == 0) p.scoreNext = chimScore;
        }
        k0 = k1;
    }
    return p;
}

bool scoreOk(const ChimParams &C, const ReadView &rv, int chimScore) { return chimScore >= C.scoreMin && chimScore + C.scoreDropMax >= (int)(rv.readLength[0] + rv.readLength[1]); }

// a chimera, not a linear alignment: different chromosome or strand, or further apart than an intron / a mate gap may be (:296-309); a junction inside a mate keeps
// its overhangs beside the repeats
bool chimeraOk(const RunParams &P, const ChimTr &t0, const ChimTr &t1, const staramd_exon &x0, const staramd_exon &x1, const ChimJunction &j) {
    if (!(t0.t.Str != t1.t.Str || t0.t.Chr != t1.t.Chr || (t0.t.Str == 0 ? j.J1 - j.J0 + 1ull : j.J0 - j.J1 + 1ull) > (j.motif >= 0 ? P.dev.alignIntronMax : P.dev.alignMatesGapMax))) return false;
    return !(j.motif >= 0 && (x0.L < P.chim.junctionOverhangMin + j.repeat0 || x1.L < P.chim.junctionOverhangMin + j.repeat1));
}
} // namespace

// --chimMultimapNmax 0: the best alignment plus the best-scoring alignment of another window that covers the rest of the read.
// returns true when a chimeric alignment was recorded (Stats::chimericAll); the junction line is appended to `out`
bool chimericDetectionOld(const RunParams &P, const GenomeIndex &gi, const ReadBatch &b, uint32_t ir, const ReadAligns &ra,
                          const staramd_transcript *trBest, uint64_t nTr, const staramd_transcript *trMult0, const staramd_transcript *trMult1, std::string &out,
                          std::vector<ChimPair> *bamOut, const ReadBatch *nameBatch, uint32_t nameIr, const uint32_t *mateStart) {
    const ChimParams &C = P.chim;
    const ReadView rv(P, gi, b, ir, nameBatch, nameIr, mateStart);
    // ---- the main segment
    if (nTr > C.mainSegmentMultNmax && nTr != 2) return false;
    const Segment mainSeg = makeSegment(rv, *trBest, ra.ex, false);
    if (!mainSegmentOk(C, rv, mainSeg)) return false;
    // ---- its partner
    Partner p;
    if (ra.pre) {             // the engine has run the loop on all windows and returned its outcome with the partner (include/star_amd.h, resultSelect 2)
        p.scoreBest = ra.pre->scoreBest; p.scoreNext = ra.pre->scoreNext; p.strBest = ra.pre->strBest;
        if (ra.pre->partner >= 0 && (uint32_t)ra.pre->partner < ra.nTr) p.t = ra.T + ra.pre->partner;
    } else p = partnerOverWindows(C, rv, ra, mainSeg);
    // ---- score gates: high enough, the main segment not multimapping, the chimera unique (:99-116)
    int chimScoreBest = p.scoreBest;
    if (!scoreOk(C, rv, chimScoreBest)) return false;
    if (nTr > C.mainSegmentMultNmax) { if (p.t != trMult0 && p.t != trMult1) return false; }
    const uint32_t chimStr = mainSeg.str == 0 ? p.strBest : mainSeg.str;
    if (p.scoreNext + C.scoreSeparation >= chimScoreBest) return false;
    if (!p.t) return false;                                            // (no partner at all passes the gates above only with settings that make them void)
    // ---- the junction between the two, in read order
    ChimTr trChim[2];
    load(trChim[0], mainSeg); load(trChim[1], makeSegment(rv, *p.t, ra.ex, false));
    auto roStartOf = [&](const ChimTr &c) { return c.t.roStr == 0 ? (uint64_t)c.t.rStart : rv.Lread - c.t.rStart - c.t.rLength; };
    if (roStartOf(trChim[0]) > roStartOf(trChim[1])) std::swap(trChim[0], trChim[1]);
    VarOverlap varOrig[2];
    if (bamOut && P.var && !rv.merged) for (int k = 0; k < 2; k++) P.var->overlap(trChim[k].t, trChim[k].ex, rv.Read1, rv.Lread, gi.chrStart[trChim[k].t.Chr], varOrig[k]);
    const uint32_t e0 = trChim[0].t.Str == 1 ? 0 : trChim[0].t.nExons - 1, e1 = trChim[1].t.Str == 0 ? 0 : trChim[1].t.nExons - 1;
    const staramd_exon &x0 = trChim[0].ex[e0], &x1 = trChim[1].ex[e1];
    ChimJunction j;
    if (x0.iFrag > x1.iFrag) return false;
    else if (x0.iFrag < x1.iFrag) j = bracketJunction(trChim[0], trChim[1], e0, e1);
    else {                                                             // inside one mate: find it, shift the segments to it
        if (!(x0.L >= C.junctionOverhangMin && x1.L >= C.junctionOverhangMin)) return false;
        JunctionScan js;
        if (!scanJunction(C, rv, trChim[0], trChim[1], e0, e1, chimStr, js)) return false;
        if (js.motif == 0) {
            chimScoreBest += 1 + C.scoreJunctionNonGTAG;
            if (!scoreOk(C, rv, chimScoreBest)) return false;
        }
        j = shiftToJunction(rv, trChim[0], trChim[1], e0, e1, js);
    }
    // ---- final test, output
    if (!chimeraOk(P, trChim[0], trChim[1], x0, x1, j)) return false;
    if (bamOut) pushPair(*bamOut, P, gi, rv, trChim[0], trChim[1], true, varOrig[0], varOrig[1], /* rescore: the blocks moved since the alignments were scored */ true);
    if (C.outJunctions) writeJunctionLine(out, P, gi, rv, trChim[0], trChim[1], j, nullptr);
    return true;
}

// --chimMultimapNmax > 0: every pair of recorded alignments of the read (all windows) is a candidate; the junction is located and both sides re-scored for each; the
// pairs within --chimMultimapScoreRange of the best are all reported
bool chimericDetectionMult(const RunParams &P, const GenomeIndex &gi, const ReadBatch &b, uint32_t ir, const ReadAligns &ra, const staramd_transcript *trBest, std::string &out,
                           std::vector<ChimPair> *bamOut, const ReadBatch *nameBatch, uint32_t nameIr, const uint32_t *mateStart) {
    const ChimParams &C = P.chim;
    const ReadView rv(P, gi, b, ir, nameBatch, nameIr, mateStart);
    const int maxNonChimAlignScore = trBest->maxScore;

    // the segments that pass ChimericSegment::segmentCheck, in window order (trAll[iW][iA])
    std::vector<Segment> seg;
    seg.reserve(ra.nTr);
    for (uint32_t k = 0; k < ra.nTr; k++) if (ra.T[k].rLength >= C.segmentMin && ra.T[k].intronMotifs[0] == 0) seg.push_back(makeSegment(rv, ra.T[k], ra.ex, true));
    struct ChimAlign { ChimTr a1, a2; ChimJunction j; int chimScore; VarOverlap var1, var2; };
    std::vector<ChimAlign> chimAligns;
    int chimScoreBest = 0; size_t bestChimAlign = 0;
    const int maxPossibleAlignScore = (int)(rv.readLength[0] + rv.readLength[1]);
    int minScoreToConsider = C.scoreMin;
    if (maxNonChimAlignScore >= minScoreToConsider) minScoreToConsider = maxNonChimAlignScore + 1;
    if (maxPossibleAlignScore - C.scoreDropMax > minScoreToConsider) minScoreToConsider = maxPossibleAlignScore - C.scoreDropMax;

    for (size_t k1 = 0; k1 < seg.size(); k1++) {
        const Segment &s1 = seg[k1];
        for (size_t k2 = k1 + 1; k2 < seg.size(); k2++) {     // later alignments of the same window, then every alignment of the later windows
            const Segment &s2 = seg[k2];
            if (s1.str != 0 && s2.str != 0 && s2.str != s1.str) continue;
            uint64_t chimOverlap;                              // chimericAlignScore
            const int chimScore = chimPairEligible(s1.ro, s2.ro, rv.readLength[0], C.segmentMin, C.segmentReadGapMax, chimOverlap) ? s1.t->maxScore + s2.t->maxScore - (int)chimOverlap : 0;
            if (chimScore < minScoreToConsider) continue;
            const Segment *p1 = &s1, *p2 = &s2;
            if (p1->t->roStart > p2->t->roStart) std::swap(p1, p2);
            const uint32_t ex1 = p1->t->Str == 1 ? 0 : p1->t->nExons - 1, ex2 = p2->t->Str == 0 ? 0 : p2->t->nExons - 1;
            // chimericCheck
            if (!(p1->ex[ex1].iFrag <= p2->ex[ex2].iFrag)) continue;
            if (!(p1->ex[ex1].iFrag < p2->ex[ex2].iFrag || (p1->ex[ex1].L >= C.junctionOverhangMin && p2->ex[ex2].L >= C.junctionOverhangMin))) continue;
            // chimericStitching
            ChimAlign ca;
            load(ca.a1, *p1); load(ca.a2, *p2);
            if (bamOut && P.var && !rv.merged) { P.var->overlap(ca.a1.t, ca.a1.ex, rv.Read1, rv.Lread, gi.chrStart[ca.a1.t.Chr], ca.var1); P.var->overlap(ca.a2.t, ca.a2.ex, rv.Read1, rv.Lread, gi.chrStart[ca.a2.t.Chr], ca.var2); }
            const uint32_t chimStr = std::max(s1.str, s2.str);
            ca.chimScore = chimScore;
            const staramd_exon &x1 = ca.a1.ex[ex1], &x2 = ca.a2.ex[ex2];
            bool alive = true;
            if (x1.iFrag < x2.iFrag) ca.j = bracketJunction(ca.a1, ca.a2, ex1, ex2);
            else {
                JunctionScan js;
                if (!scanJunction(C, rv, ca.a1, ca.a2, ex1, ex2, chimStr, js)) { ca.chimScore = 0; alive = false; }
                else ca.j = shiftToJunction(rv, ca.a1, ca.a2, ex1, ex2, js);
            }
            if (alive) {
                if (ca.j.motif >= 0 && (x1.L < C.junctionOverhangMin || x2.L < C.junctionOverhangMin)) ca.chimScore = 0;   // a linear junction too close to the chimeric one
                else ca.chimScore = chimAlignScore(P.dev, gi, rv.Read1, rv.Lread, ca.a1) + chimAlignScore(P.dev, gi, rv.Read1, rv.Lread, ca.a2) + (ca.j.motif == 0 ? C.scoreJunctionNonGTAG : 0);
            }
            if (ca.chimScore >= minScoreToConsider) {
                chimAligns.push_back(ca);
                if (ca.chimScore > chimScoreBest) {
                    chimScoreBest = ca.chimScore; bestChimAlign = chimAligns.size() - 1;
                    if (chimScoreBest - (int)C.multimapScoreRange > minScoreToConsider) minScoreToConsider = chimScoreBest - (int)C.multimapScoreRange;
                }
            }
        }
    }
    if (chimScoreBest == 0) return false;
    uint64_t chimN = 0;
    for (const ChimAlign &ca : chimAligns) if (ca.chimScore >= minScoreToConsider) ++chimN;
    if (chimN > C.multimapNmax) return false;
    for (size_t i = 0; i < chimAligns.size(); i++) {
        const ChimAlign &ca = chimAligns[i];
        if (ca.chimScore < minScoreToConsider) continue;
        if (bamOut) pushPair(*bamOut, P, gi, rv, ca.a1, ca.a2, i == bestChimAlign, ca.var1, ca.var2, /* rescore: chimericStitching has scored them */ false);
        if (!C.outJunctions) continue;
        const MultColumns m{chimN, maxPossibleAlignScore, maxNonChimAlignScore, ca.chimScore, chimScoreBest};
        writeJunctionLine(out, P, gi, rv, ca.a1, ca.a2, ca.j, &m);
    }
    return chimN > 0;
}

} // namespace staramd
