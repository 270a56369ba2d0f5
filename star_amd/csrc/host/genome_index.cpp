// genome_index.cpp -- parse an unmodified STAR genomeDir.
// Follows Genome::genomeLoad (source/Genome_genomeLoad.cpp:18-467), Genome::chrInfoLoad / chrBinFill
// (source/Genome.cpp:139-215) and Genome::loadSJDB (source/Genome_genomeLoad.cpp:471-521).
#include "host.h"
#include "../index/seq_core.h"
#include <fstream>
#include <sstream>
#include <cmath>
#include <cstring>
#include <chrono>
#include <sys/stat.h>

namespace staramd {

// headroom: capacity beyond the file (address space only, untouched) -- the genome text grows by the inserted junction sequences in a 2-pass run, and a
// vector that has to move for that copies 3 GB on one thread
static bool readFile(const std::string &path, std::vector<uint8_t> &out, size_t extra = 0, size_t headroom = 0) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (headroom) out.reserve((size_t)n + extra + headroom);
    out.assign((size_t)n + extra, 0);
    size_t got = n ? fread(out.data(), 1, (size_t)n, f) : 0;
    fclose(f);
    out.resize((size_t)n + extra);
    return got == (size_t)n;
}

std::string GenomeIndex::load(const std::string &genomeDir) {
    auto t0 = std::chrono::steady_clock::now();
    dir = genomeDir;
    memset(&view, 0, sizeof(view));
    // --- genomeParameters.txt (:33-62): "### GstrandBit N" comment + key/value lines
    uint32_t GstrandBit = 0, gSAindexNbases = 14, gChrBinNbits = 18, gSAsparseD = 1, sjdbOverhang = 0;
    std::string versionGenome;
    {
        std::ifstream pf(dir + "/genomeParameters.txt");
        if (!pf.good()) return "EXITING because of FATAL ERROR: could not open genome file " + dir + "/genomeParameters.txt";
        std::string line;
        while (std::getline(pf, line)) {
            std::istringstream ls(line);
            std::string k;
            ls >> k;
            if (k == "###") { ls >> k; if (k == "GstrandBit") ls >> GstrandBit; continue; }
            if (k == "versionGenome") ls >> versionGenome;
            else if (k == "genomeSAindexNbases") ls >> gSAindexNbases;
            else if (k == "genomeChrBinNbits") ls >> gChrBinNbits;
            else if (k == "genomeSAsparseD") ls >> gSAsparseD;
            else if (k == "sjdbOverhang") ls >> sjdbOverhang;
            else if (k == "genomeType") { std::string v; ls >> v; if (v != "Full") return "EXITING because of FATAL ERROR: the index in " + dir + " was generated with --genomeType " + v + "; only Full genomes are supported by the MI355X engine"; }
            else if (k == "genomeTransformType") { std::string v; ls >> v; if (v != "None") return "EXITING because of FATAL ERROR: the index in " + dir + " is a transformed genome (--genomeTransformType " + v + "); genome transformation is not supported by the MI355X engine"; }
        }
    }
    if (versionGenome != "2.7.4a")       // parametersDefault:2 ; Genome_genomeLoad.cpp:71-83
        return "EXITING because of FATAL ERROR: Genome version: " + versionGenome + " is INCOMPATIBLE with running STAR version: 2.7.11b";
    // --- chrName/Length/Start (Genome.cpp:139-192)
    {
        std::ifstream in(dir + "/chrName.txt");
        if (!in.good()) return "EXITING because of FATAL error, could not open file " + dir + "/chrName.txt";
        std::string l;
        while (std::getline(in, l)) { if (l.empty()) break; chrName.push_back(l); }
    }
    uint32_t nChrReal = (uint32_t)chrName.size();
    chrStart.assign(nChrReal + 1, 0); chrLength.assign(nChrReal, 0);
    {
        std::ifstream in(dir + "/chrLength.txt");
        if (!in.good()) return "EXITING because of FATAL error, could not open file " + dir + "/chrLength.txt";
        for (uint32_t i = 0; i < nChrReal; i++) in >> chrLength[i];
    }
    {
        std::ifstream in(dir + "/chrStart.txt");
        if (!in.good()) return "EXITING because of FATAL error, could not open file " + dir + "/chrStart.txt";
        for (uint32_t i = 0; i <= nChrReal; i++) in >> chrStart[i];
    }
    // --- Genome / SA / SAindex (:139-169, 315-336)
    if (!readFile(dir + "/Genome", G, 0, (size_t)320 << 20)) return "EXITING because of FATAL ERROR: could not open genome file " + dir + "/Genome";
    if (!readFile(dir + "/SA", SA, 8)) return "EXITING because of FATAL ERROR: could not open genome file " + dir + "/SA";
    uint64_t nSAbyte = SA.size() - 8;
    std::vector<uint8_t> sai;
    if (!readFile(dir + "/SAindex", sai, 8)) return "EXITING because of FATAL ERROR: could not open genome file " + dir + "/SAindex";
    uint64_t nb;
    memcpy(&nb, sai.data(), 8);
    if (nb > 16) return "SAindex: unsupported genomeSAindexNbases";
    gSAindexNbases = (uint32_t)nb;
    memcpy(view.genomeSAindexStart, sai.data() + 8, 8 * (nb + 1));
    SAi.assign(sai.begin() + 8 * (nb + 2), sai.end());
    uint64_t nGenome = G.size();
    if (GstrandBit == 0) {       // :149-153
        GstrandBit = (uint32_t)std::floor(std::log((double)nGenome) / std::log(2.0)) + 1;
        if (GstrandBit < 32) GstrandBit = 32;
    }
    view.G = G.data(); view.nGenome = nGenome;
    view.SA = SA.data(); view.nSAbyte = nSAbyte; view.nSA = (nSAbyte * 8) / (GstrandBit + 1);
    view.SAi = SAi.data(); view.nSAibyte = SAi.size() - 8; view.nSAi = view.genomeSAindexStart[nb];
    view.GstrandBit = GstrandBit; view.gSAindexNbases = gSAindexNbases; view.gSAsparseD = gSAsparseD;
    view.gChrBinNbits = gChrBinNbits;
    view.chrStart = chrStart.data(); view.chrLength = chrLength.data(); view.nChrReal = nChrReal;
    insertChrIndFirst = nChrReal;        // Genome_genomeLoad.cpp:246
    // --- chrBinFill (Genome.cpp:209-215)
    uint64_t binBases = 1ull << gChrBinNbits;
    uint64_t chrBinN = chrStart[nChrReal] / binBases + 1;
    chrBin.assign(chrBinN, 0);
    for (uint64_t ii = 0, ichr = 1; ii < chrBinN; ++ii) {
        if (ii * binBases >= chrStart[ichr]) ichr++;
        chrBin[ii] = (uint32_t)(ichr - 1);
    }
    view.chrBin = chrBin.data(); view.chrBinN = chrBinN;
    { struct stat st1; sjdbInfoExists = stat((dir + "/sjdbInfo.txt").c_str(), &st1) == 0; }
    // --- loadSJDB (:471-521)
    view.sjdbOverhang = sjdbOverhang;
    view.sjdbLength = sjdbOverhang == 0 ? 0 : sjdbOverhang * 2 + 1;
    if (nGenome == chrStart[nChrReal]) {
        view.sjdbN = 0; view.sjGstart = chrStart[nChrReal] + 1;
    } else {
        std::ifstream in(dir + "/sjdbInfo.txt");
        if (!in.good()) return "EXITING because of FATAL error, could not open file " + dir + "/sjdbInfo.txt";
        uint64_t n, ov;
        in >> n >> ov;
        view.sjdbN = (uint32_t)n; view.sjdbOverhang = (uint32_t)ov; view.sjdbLength = (uint32_t)(ov * 2 + 1);
        view.sjGstart = chrStart[nChrReal];
        sjDstart.resize(n); sjAstart.resize(n); sjdbStart.resize(n); sjdbEnd.resize(n);
        sjdbMotif.resize(n); sjdbShiftLeft.resize(n); sjdbShiftRight.resize(n); sjdbStrand.resize(n);
        for (uint64_t ii = 0; ii < n; ii++) {
            uint32_t d1, d2, d3, d4;
            in >> sjdbStart[ii] >> sjdbEnd[ii] >> d1 >> d2 >> d3 >> d4;
            sjdbMotif[ii] = (uint8_t)d1; sjdbShiftLeft[ii] = (uint8_t)d2; sjdbShiftRight[ii] = (uint8_t)d3; sjdbStrand[ii] = (uint8_t)d4;
            sjDstart[ii] = sjdbStart[ii] - ov; sjAstart[ii] = sjdbEnd[ii] + 1;
            if (sjdbMotif[ii] == 0) { sjDstart[ii] += sjdbShiftLeft[ii]; sjAstart[ii] += sjdbShiftLeft[ii]; }
        }
        view.sjDstart = sjDstart.data(); view.sjAstart = sjAstart.data(); view.sjdbStart = sjdbStart.data(); view.sjdbEnd = sjdbEnd.data();
        view.sjdbMotif = sjdbMotif.data(); view.sjdbShiftLeft = sjdbShiftLeft.data(); view.sjdbShiftRight = sjdbShiftRight.data(); view.sjdbStrand = sjdbStrand.data();
    }
    loadSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return "";
}

// ---- --genomeFastaFiles at the mapping stage (Genome::insertSequences, source/Genome_insertSequences.cpp:9-33; sizes: Genome_genomeLoad.cpp:244-250)
static SeqInsertFn g_seqInsertFn = nullptr; static int g_seqInsertDevice = 0;
void setSeqInsertFn(SeqInsertFn fn, int device) { g_seqInsertFn = fn; g_seqInsertDevice = device; }

std::string GenomeIndex::insertSequences(const RunParams &P, std::string &log) {
    if (!g_seqInsertFn) return SEQ_INSERT_MISSING;
    const uint32_t nChrOld = view.nChrReal;
    const uint64_t binBases = 1ull << view.gChrBinNbits, nG = chrStart[nChrOld], nGenomeOld = G.size();
    // the added text as genomeScanFastaFiles lays it out behind the last chromosome: nG is a bin boundary, so offsets from 0 are offsets from nG
    std::vector<uint8_t> G1; std::vector<std::string> names; std::vector<uint64_t> starts, lengths;
    {
        const std::string e = scanFastaFiles(P.genomeFastaFiles, binBases, G1, names, starts, lengths);
        if (!e.empty()) return e;
    }
    const uint64_t nG1 = G1.size();
    if (staridx::seqStrandBitCheck(nG, nG1, view.GstrandBit + 1)) return staridx::SEQ_STRANDBIT_ERROR;      // insertSeqSA.cpp:21-29
    log += " ..... inserting extra sequences into genome indexes\n";
    uint64_t nInd = 0;
    for (uint8_t c : G1) nInd += c < 4;
    nInd *= 2;
    const uint32_t wSA = view.GstrandBit + 1;
    const uint64_t nSAnew = view.nSA + nInd;
    std::vector<uint8_t> SAnew(staridx::packedBytes(nSAnew + 1, wSA) + 16, 0), SAiNew(view.nSAibyte + 24, 0);
    staramd_seq_args a; memset(&a, 0, sizeof(a));
    a.G = G.data(); a.nGenomeOld = nGenomeOld; a.nGenomeReal = nG;
    a.SA = SA.data(); a.nSAold = view.nSA; a.nSAbyteOld = view.nSAbyte; a.GstrandBit = view.GstrandBit; a.gSAindexNbases = view.gSAindexNbases;
    a.Gins = G1.data(); a.nGins = nG1;
    a.SAout = SAnew.data(); a.saOutCapacity = SAnew.size(); a.SAiOut = SAiNew.data(); a.saiOutCapacity = SAiNew.size();
    staramd_seq_result r; memset(&r, 0, sizeof(r));
    const int rc = g_seqInsertFn(g_seqInsertDevice, &a, &r);
    if (rc) return "EXITING because of FATAL ERROR: sequence insertion on the MI355X failed (code " + std::to_string(rc) + ")";
    if (r.nInd != nInd || r.nSAibyte != view.nSAibyte) return "EXITING because of FATAL ERROR: sequence insertion on the MI355X returned an index of unexpected size";
    log += "   Finished SA search, number of new SA indices = " + std::to_string(nInd) + "\n   Finished inserting SA indices\n";
    { char t[200]; snprintf(t, sizeof t, "star_amd: sequence insertion on the device: %.1f ms, %u doubling rounds, %llu searches stopped at 10000 characters\n", (double)r.msTotal, r.doublingRounds, (unsigned long long)r.nCapHits); log += t; }
    // the new index: chromosomes, added sequences, the moved junction block (:19-25)
    G.insert(G.begin() + nG, G1.begin(), G1.end());
    SAnew.resize(staridx::packedBytes(nSAnew, wSA) + 8); SA.swap(SAnew);
    SAiNew.resize(view.nSAibyte + 8); SAi.swap(SAiNew);
    chrStart.pop_back();
    for (size_t i = 0; i < names.size(); i++) { chrName.push_back(names[i]); chrStart.push_back(nG + starts[i]); chrLength.push_back(lengths[i]); }
    chrStart.push_back(nG + nG1);
    const uint32_t nChr = (uint32_t)chrName.size();
    view.nChrReal = nChr; view.nSA = nSAnew; view.nSAbyte = staridx::packedBytes(nSAnew, wSA);
    view.sjGstart = view.sjdbN == 0 ? chrStart[nChr] + 1 : chrStart[nChr];
    const uint64_t chrBinN = chrStart[nChr] / binBases + 1;      // chrBinFill (Genome.cpp:209-215)
    chrBin.assign(chrBinN, 0);
    for (uint64_t ii = 0, ichr = 1; ii < chrBinN; ++ii) { if (ii * binBases >= chrStart[ichr]) ichr++; chrBin[ii] = (uint32_t)(ichr - 1); }
    view.chrBinN = chrBinN;
    seqInserted = true;
    refreshView();
    return "";
}

} // namespace staramd
