// runner.cpp -- host run orchestration (the alignReads part of STAR.cpp main(), source/STAR.cpp:58-313)
// and its C interface `sah_*`, used by the CLI (main.cpp) and, through ctypes, by tests/ and bench.py.
// The engine (HIP library behind include/star_amd.h) is NOT linked here: callers pass result buffers in,
// so the same post-map code is exercised with results produced by the HIP engine (product) or,
// in tests only, by the CPU oracle.
//
// In this file: BatchSet (a batch with its merged mates and WASP reads: the main batch and every slot), EmitRange (everything one range of a batch
// produces), SamWriter (the writer thread of Aligned.out.sam / .bam and its two sets of ranges), Runner (the run: init, the batch operations on a
// BatchSet, emitBatch = planEmit / drawRandomOrder / formatRange / compressOnDevice / foldRanges, the phase changes, finish), then the C interface,
// whose batch operations forward to Runner with the set and the error string of the calling stage.  The sorted BAM is CoordSortedBam's (bam_sorted.cpp).
#include "host.h"
#include <unistd.h>
#include <fcntl.h>
#include <atomic>
#include <sys/stat.h>
#include <cerrno>
#include <cstring>
#include <algorithm>
#include <ctime>
#include <memory>
#include <thread>
#include <mutex>
#include <condition_variable>
#include <deque>
#include <array>
#include <random>
#include <chrono>
#include <sys/mman.h>

namespace staramd {

// one batch with what is mapped beside it: the main batch of the one-batch-at-a-time interface (sah_next_batch ...) and every slot of the pipelined one
// (sah_fill_slot ...) are such a set, and each batch operation has one body that takes the set
struct BatchSet {
    ReadBatch batch;
    MergedBatch merged;     // --peOverlapNbasesMin: the merged mates of `batch`, mapped as a second batch
    WaspBatch wasp;         // --waspOutputMode SAMtag: the allele-swapped reads of `batch`, mapped as one more batch
};

// Everything one range of reads of a batch produces (Runner::emitBatch).  A worker thread appends to the members of ITS range for the length of the range, and a
// std::string / std::vector rewrites its size word on every append: two ranges never share a cache line (as neighbouring elements of per-output vectors they did,
// measured 4x per record with 8 threads).  The ranges live in the writer's two sets and keep their capacity between batches: a fresh buffer grows by reallocation
// up to a few hundred KB per range and batch, which glibc serves with mmap / munmap -- page faults on every batch.
struct alignas(64) EmitRange {
    std::string sam;                            // what goes to Aligned.out.sam / .bam: SAM text or BGZF blocks
    std::string raw;                            // BAM: the records, uncompressed
    OutSJ sj; Stats st;
    OutSJ sj1; std::vector<uint32_t> held;      // 1st stage of BySJout: junctions of every read, reads held for the 2nd stage
    GeneCounts gc;                              // --quantMode GeneCounts
    std::vector<BamKey> keys;                   // --outSAMtype BAM SortedByCoordinate
    std::string quantRaw, quantZ; std::vector<QuantPatch> quantPatches;     // --quantMode TranscriptomeSAM: records, their BGZF blocks, where the primary flag goes
    std::string only; bool cut = false;         // KeepPairs with both BAM files: `raw` without the records of the sorted file (what the unsorted one gets)
    std::string chim, chimSam;                  // Chimeric.out.junction lines, Chimeric.out.sam records
    std::string unmapped[2];                    // --outReadsUnmapped Fastx, per mate
    std::string err; double ms = 0;             // error text of the range; time on its worker (STARAMD_HOST_TIMING)
    void reset(bool geneCounts, size_t nGenes) {
        sam.clear(); raw.clear(); sj.data.clear(); st = Stats(); sj1.data.clear(); held.clear(); keys.clear();
        if (geneCounts) gc = GeneCounts(nGenes);
        quantRaw.clear(); quantZ.clear(); quantPatches.clear(); only.clear(); cut = false; chim.clear(); chimSam.clear(); unmapped[0].clear(); unmapped[1].clear();
        err.clear(); ms = 0;
    }
};

// ---- Aligned.out.sam / Aligned.out.bam go to the file on a thread of their own: formatting of batch k+1 overlaps the write of batch k.  Two sets of ranges
// alternate.  The emit side takes a free set, fills ranges[0 .. used) and hands it over; the writer puts out the `sam` of every range, in range order, and frees the set.
struct SamWriter {
    struct Set { std::vector<EmitRange> ranges; uint32_t used = 0; };
    uint64_t mappedWrites = 0;               // batches whose text went out through a mapping of the output file (sah_fast_path_counts)
    double seconds = 0;                      // busy time, whole run
    void start(FILE *out, int runThreadN) {
        samOut = out;
        wantMmap = getenv("STARAMD_WRITER_MMAP") ? atoi(getenv("STARAMD_WRITER_MMAP")) : 1;
        // (follows --runThreadN like every helper count; 8 of 16: the writer is level with the kernels now, 4 copy threads lost 2 % to 8 on one box -- profiles/r06_e2e_session37_*)
        wantW = getenv("STARAMD_WRITER_THREADS") ? (uint32_t)std::max(1, atoi(getenv("STARAMD_WRITER_THREADS"))) : (uint32_t)std::max(1, std::min(8, runThreadN / 2));
        pwriteW = getenv("STARAMD_WRITER_PWRITE_THREADS") ? (uint32_t)std::max(1, atoi(getenv("STARAMD_WRITER_PWRITE_THREADS"))) : 2u;      // (positional writes: 1 = one stream, no contention for the inode lock)
        freeSets = {0, 1};
        thread = std::thread([this] { loop(); });
    }
    Set &takeFree() { std::unique_lock<std::mutex> l(m); cv.wait(l, [&] { return !freeSets.empty(); }); const int k = freeSets.front(); freeSets.pop_front(); return sets[k]; }
    void handOver(Set &s) { { std::lock_guard<std::mutex> l(m); fullSets.push_back((int)(&s - sets)); } cv.notify_all(); }
    void stop() {           // after the sets that were handed over are written
        if (!thread.joinable()) return;
        { std::lock_guard<std::mutex> l(m); stopping = true; }
        cv.notify_all();
        thread.join();
    }
    bool failed() const { return bad.load(); }
    void resumeStream() { if (fd >= 0) { fflush(samOut); fseeko(samOut, (off_t)pos, SEEK_SET); } }      // the batches went out through positional writes: the stream goes on behind them
    ~SamWriter() { stop(); }
private:
    Set sets[2];
    std::mutex m; std::condition_variable cv;
    std::deque<int> freeSets, fullSets; bool stopping = false; std::atomic<bool> bad{false};
    std::thread thread;
    FILE *samOut = nullptr;
    int fd = -1; uint64_t pos = 0;           // positional writes of the SAM / unsorted BAM text (regular file)
    int seekable = -1;                       // -1 not looked at yet, 0 pipe / FIFO / character device (sequential fwrite), 1 regular file
    int wantMmap = 1; uint32_t wantW = 1, pwriteW = 2;      // STARAMD_WRITER_MMAP, _WRITER_THREADS, _WRITER_PWRITE_THREADS
    void loop() {
        for (;;) {
            int k;
            { std::unique_lock<std::mutex> l(m); cv.wait(l, [&] { return !fullSets.empty() || stopping; }); if (fullSets.empty()) return; k = fullSets.front(); fullSets.pop_front(); }
            write(sets[k]);
            { std::lock_guard<std::mutex> l(m); freeSets.push_back(k); }
            cv.notify_all();
        }
    }
    void write(Set &o) {
        CpuScope cpuScope(CPU_WRITE);
        ScopedTimer addTime(&seconds);
        if (seekable < 0 && samOut) {            // a named pipe (mkfifo Aligned.out.sam | samtools ...) or a device has no offsets: pwrite fails with ESPIPE there
            struct stat st; seekable = (samOut != stdout && fstat(fileno(samOut), &st) == 0 && S_ISREG(st.st_mode) && ftello(samOut) >= 0) ? 1 : 0;
        }
        if (!(samOut && seekable == 1 && (o.used > 1 || fd >= 0 || wantMmap >= 2))) {
            for (uint32_t t = 0; t < o.used; t++) {
                const std::string &s = o.ranges[t].sam;
                if (!s.empty() && samOut && fwrite(s.data(), 1, s.size(), samOut) != s.size()) bad = true;
            }
            return;
        }
        // a regular file: the ranges' text buffers go out side by side, each at its own offset (one fwrite stream tops out near
        // 2 GB/s on tmpfs, the SAM text of one GPU runs at about that)
        if (fd < 0) { fflush(samOut); fd = fileno(samOut); pos = (uint64_t)ftello(samOut); }
        std::vector<uint64_t> at(o.used + 1, pos);
        for (uint32_t t = 0; t < o.used; t++) at[t + 1] = at[t] + o.ranges[t].sam.size();
        // write() / pwrite() into ONE file are serialised by the inode lock (tmpfs: 2.9 GB/s from two threads on a box whose tmpfs takes 5.8 / 11.7 / 18.5 GB/s from
        // 1 / 2 / 4 streams into separate files: the SAM writer at 230 MB per batch was the slowest stage of the pipeline there, 80 ms against 52 ms of kernels).  So the
        // file is grown to the batch's end and the new part mapped: the threads copy their ranges into the mapping and take their page faults side by side.
        const uint64_t total = at[o.used] - pos;
        char *map = nullptr; uint64_t mapOff = 0, mapLen = 0;
        // the blocks are reserved before they are written to (posix_fallocate also sets the new size): a full file system is an error return here, not a SIGBUS in a copy
        if (wantMmap && total > 0 && (wantMmap >= 2 || total >= (1u << 20)) && posix_fallocate(fd, (off_t)pos, (off_t)total) == 0) {      // (2: whatever the size -- tests)
            static const uint64_t page = (uint64_t)std::max<long>(sysconf(_SC_PAGESIZE), 4096); mapOff = pos & ~(page - 1); mapLen = at[o.used] - mapOff;
            void *mm = mmap(nullptr, (size_t)mapLen, PROT_READ | PROT_WRITE, MAP_SHARED, fd, (off_t)mapOff);
            if (mm != MAP_FAILED) { map = (char *)mm; mappedWrites++; }
        }
        overItems(map ? wantW : pwriteW, CPU_WRITE, o.used, [&](size_t t) {
            const std::string &s = o.ranges[t].sam;
            const char *p = s.data(); uint64_t left = s.size(), off = at[t];
            if (map) { if (left) memcpy(map + (off - mapOff), p, left); return; }
            while (left && !bad) { ssize_t w = pwrite(fd, p, left, (off_t)off); if (w <= 0) { bad = true; return; } p += w; left -= (uint64_t)w; off += (uint64_t)w; }
        });
        if (map) munmap(map, (size_t)mapLen);
        pos = at[o.used];
    }
};

struct Runner {
    RunParams P;
    GenomeIndex gi;
    FastqReader reader;
    static const int NSLOT = 24;        // batch slots of the pipelined CLI (3 + 2 per GPU are in use: cli_run.cpp)
    BatchSet mainSet, slots[NSLOT];     // pipelined CLI: parse / map / post-map work on different slots
    Variation variation;                      // --varVCFfile
    std::unique_ptr<PostMap> post;
    OutSJ sj;
    Stats stats;
    FILE *samOut = nullptr;
    bool toolDone = false;                          // --runMode inputAlignmentsFromBAM: everything happened in init()
    uint64_t dedupCounts[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // sah_dedup_counts
    bool generateMode = false; GenerateJob genJob;  // --runMode genomeGenerate: FASTA scanned in init(), SA / SAindex built by the caller on the device
    FILE *chimOut = nullptr;                        // Chimeric.out.junction
    FILE *chimSamOut = nullptr;                     // Chimeric.out.sam (--chimOutType SeparateSAMold)
    FILE *unmappedOut[2] = {nullptr, nullptr};      // --outReadsUnmapped Fastx: Unmapped.out.mate1 / mate2
    std::string error;
    // three stages of the pipelined front end run on their own threads; each reports through a string of its own (guarded by errM), and
    // sah_error hands the calling thread a private copy: parseError -- reader (sah_parse_slot), mapError -- mapper threads (sah_wasp_results_slot),
    // `error` -- the emit / control side (one thread at a time)
    std::string parseError, mapError; std::mutex errM;
    SjdbLoci sjdbLoci;                  // junctions known so far (generated genome, --sjdbFileChrStartEnd, 1st pass)
    std::string insertLog;
    bool pass1 = false;
    // --outFilterType BySJout (STAR.cpp:203-220): stage 1 maps everything and holds reads with unannotated junctions, stage 2 maps
    // the held reads again with the filtered novel junctions as a whitelist inside the stitcher
    int bySJoutStage = 0;               // 0 off, 1, 2
    OutSJ sj1;                          // junctions of every read of stage 1 (chunkOutSJ1)
    std::string heldText[2];            // held reads as FASTQ text
    std::vector<uint64_t> novelStart, novelEnd;
    GeneAnnotation genes; GeneCounts geneCounts;      // --quantMode GeneCounts
    TranscriptAnnotation transcripts; FILE *quantOut = nullptr;     // --quantMode TranscriptomeSAM -> Aligned.toTranscriptome.out.bam
    MultOrder multOrder;
    std::mt19937 rngMultOrder; std::uniform_real_distribution<double> rngUniformReal0to1{0.0, 1.0};   // ReadAlign.cpp:11-12 (one stream: iChunk 0)
    CoordSortedBam sorted;              // --outSAMtype BAM SortedByCoordinate: every record, until finish()
    int wireTable = 0;                                // which junction table sah_sj_export / import / clear address: 0 = sj, 1 = sj1
    OutSJ &wire() { if (wireTable != 1) sjBg.drainInto(sj); return wireTable == 1 ? sj1 : sj; }
    // The output junction table grows by one record per junction per read.  Whenever it passes sjKick records it is handed to a thread that collapses it and folds it
    // into what was collapsed before (collapse is a sum / maximum per junction: the order does not matter), so that what is left to sort when the run ends
    // (finish() is inside the timed region of a run; SJ.out.tab needs the collapsed table) is less than sjKick records + the last batch, not everything since the
    // last 4 M-record collapse (ReadAlignChunk_mapChunk.cpp:66-86 collapses when the chunk's buffer is full, for bounded memory; this does the same, off the path)
    struct SjBackground {
        OutSJ folded, work; std::thread th;
        void join() { if (th.joinable()) th.join(); }
        void kick(OutSJ &live) { join(); work.data.swap(live.data); th = std::thread([this] { work.collapse(); folded.mergeFrom(work); work.data.clear(); folded.collapse(); }); }
        void drainInto(OutSJ &live) { join(); if (!folded.data.empty()) { live.mergeFrom(folded); folded.data.clear(); } }
        ~SjBackground() { join(); }
    } sjBg;
    size_t sjKick = 1000000;
    int64_t readMapNumberUser = -1;

    bool init(int argc, char **argv) {
        time(&stats.timeStart);
        error = P.parse(argc, argv);
        if (!error.empty()) return false;
        if (const char *e = getenv("STARAMD_SJ_KICK")) sjKick = (size_t)strtoull(e, nullptr, 10);      // (tests: a few hundred records, so that the background collapse runs on small data)
        {   // createDirectory (streamFuns.cpp:10-35): the directory part of --outFileNamePrefix is made, with its parents, mode S_IRWXU
            const std::string dirPath = P.outFileNamePrefix.substr(0, P.outFileNamePrefix.find_last_of('/') + 1);
            if (!dirPath.empty() && mkdir(dirPath.c_str(), S_IRWXU) == -1 && errno != EEXIST) {
                for (size_t i1 = dirPath.find_first_of('/', 1); i1 < dirPath.size(); i1 = dirPath.find_first_of('/', i1 + 1)) {
                    const std::string d1 = dirPath.substr(0, i1);
                    if (mkdir(d1.c_str(), S_IRWXU) == -1 && errno != EEXIST) {
                        error = "EXITING because of fatal OUTPUT FILE error: could not create output directory: " + d1 + " for --outFileNamePrefix " + P.outFileNamePrefix + "\n ERROR: " + strerror(errno) + "\nSOLUTION: check the path and permissions.\n";
                        return false;
                    }
                }
            }
        }
        if (P.runModeGenerate) {                                    // index generation: no reads; the device stages are run by the caller
            error = genomeGenerateScan(P, gi, genJob);
            generateMode = true;
            return error.empty();
        }
        if (P.runModeFromBAM) {                                     // a tool mode: no index, no reads, no engine
            // Parameters.cpp:587-599: the tracks when --outWigType asks for them, else the duplicate marking
            if (P.wig.yes) error = signalFromBamFile(P, P.inputBAMfile, P.outFileNamePrefix + "Signal");
            else error = dedupFromBamFile(P, P.inputBAMfile, P.outFileNamePrefix + "Processed.out.bam", dedupCounts);
            toolDone = true;
            return error.empty();
        }
        error = gi.load(P.genomeDir);
        if (!error.empty()) return false;
        if (!P.genomeFastaFiles.empty()) {                          // Genome_genomeLoad.cpp:374: references added to the loaded index
            error = gi.insertSequences(P, insertLog);
            if (!error.empty()) return false;
        }
        if (P.sjdbInsertYes()) {
            // sjdbOverhang of the run (Genome_genomeLoad.cpp:113-125) and the run-time directories (Parameters.cpp:817-824,1019-1034)
            uint32_t gov = gi.view.sjdbOverhang;
            if (!P.sjdbOverhangSet && gov > 0) P.sjdbOverhang = gov;
            else if (gi.sjdbInfoExists && P.sjdbOverhangSet && P.sjdbOverhang != gov) {
                error = "EXITING because of fatal PARAMETERS error: present --sjdbOverhang=" + std::to_string(P.sjdbOverhang) + " is not equal to the value at the genome generation step =" + std::to_string(gov) + "\nSOLUTION: \n";
                return false;
            }
            if (P.sjdbOverhang == 0 || P.sjdbOverhang > 500) { error = "EXITING because of fatal PARAMETERS error: pGe.sjdbOverhang <=0 (or > 500) while junctions are inserted on the fly"; return false; }
            gi.view.sjdbOverhang = P.sjdbOverhang; gi.view.sjdbLength = 2 * P.sjdbOverhang + 1;
            P.sjdbInsertOutDir = P.outFileNamePrefix + "_STARgenome/";
            error = makeRunDir(P.sjdbInsertOutDir, P.runDirPermAll);
            if (!error.empty()) return false;
            if (P.twopass) { P.twopassDir = P.outFileNamePrefix + "_STARpass1/"; error = makeRunDir(P.twopassDir, P.runDirPermAll); if (!error.empty()) return false; }
        }
        P.finalize(gi);
        if (P.sjdbInsertPass1()) {                                  // STAR.cpp:147-150: insertion before the (1st) mapping pass
            error = sjdbInsertJunctions(P, gi, sjdbLoci, false, "", insertLog);
            if (!error.empty()) return false;
        }
        error = reader.open(P.readFilesIn, P.readFilesCommand, P.readFilesSAMmates);
        if (!error.empty()) return false;
        if (!P.varVCFfile.empty()) { error = variation.load(P, gi); if (!error.empty()) return false; P.var = &variation; }
        post.reset(new PostMap(P, gi));
        rngMultOrder.seed((unsigned)P.runRNGseed);                  // ReadAlign.cpp:11 (iChunk 0)
        if (P.quantTrSAM) {
            error = transcripts.load(P.sjdbGTFfile.empty() ? P.genomeDir : P.sjdbInsertOutDir);
            if (!error.empty()) return false;
            post->transcripts = &transcripts;
            if (P.quantTrBAMcompression > -2) {
                std::string qp = P.outFileNamePrefix + "Aligned.toTranscriptome.out.bam";
                quantOut = P.outStd == "BAM_Quant" ? stdout : fopen(qp.c_str(), "wb");
                if (!quantOut) { error = "EXITING because of fatal ERROR: could not create output file " + qp; return false; }
                std::string h;
                if (!bgzfCompress(post->quantBamHeader(), P.quantTrBAMcompression, h)) { error = "EXITING because of fatal ERROR: BGZF compression failed"; return false; }
                fwrite(h.data(), 1, h.size(), quantOut);
            }
        }
        if (P.quantGeneCounts) {                                    // Transcriptome.cpp:12-16: a GTF given at the mapping stage wins
            error = genes.load(P.sjdbGTFfile.empty() ? P.genomeDir : P.sjdbInsertOutDir);
            if (!error.empty()) return false;
            geneCounts = GeneCounts(genes.geID.size());
            post->genes = &genes;
        }
        if (P.outFilterBySJout && !P.twopass) { bySJoutStage = 1; P.dev.outFilterBySJoutStage = 1; }
        if (P.twopass) {                                            // twoPassRunPass1.cpp:14-47: no SAM, own read limit
            pass1 = true; post->samOff = true; readMapNumberUser = P.readMapNumber;
            P.dev.chimSegmentMinPositive = 0;                       // twoPassRunPass1.cpp:24 (restored with the index re-upload after the pass)
            if (P.twopass1readsN >= 0) P.readMapNumber = P.readMapNumber < 0 ? P.twopass1readsN : std::min(P.readMapNumber, P.twopass1readsN);
        }
        if (P.chim.segmentMin > 0 && P.chim.outJunctions) {
            std::string cp = P.outFileNamePrefix + "Chimeric.out.junction";
            chimOut = fopen(cp.c_str(), "wb");
            if (!chimOut) { error = "EXITING because of fatal ERROR: could not create output file " + cp; return false; }
            if (P.chim.multimapNmax > 0)                            // column names of the multimapping algorithm's table (ParametersChimeric_initialize.cpp:48-72)
                fputs("chr_donorA\tbrkpt_donorA\tstrand_donorA\tchr_acceptorB\tbrkpt_acceptorB\tstrand_acceptorB\tjunction_type\trepeat_left_lenA\trepeat_right_lenB\tread_name\t"
                      "start_alnA\tcigar_alnA\tstart_alnB\tcigar_alnB\tnum_chim_aln\tmax_poss_aln_score\tnon_chim_aln_score\tthis_chim_aln_score\tbestall_chim_aln_score\tPEmerged_bool\treadgrp\n", chimOut);
        }
        if (P.chim.segmentMin > 0 && P.chim.outSamOld) {            // ParametersChimeric_initialize.cpp:39-42
            std::string cp = P.outFileNamePrefix + "Chimeric.out.sam";
            chimSamOut = fopen(cp.c_str(), "wb");
            if (!chimSamOut) { error = "EXITING because of fatal ERROR: could not create output file " + cp; return false; }
            std::string h = post->samHeader(); fwrite(h.data(), 1, h.size(), chimSamOut);
        }
        if (P.outReadsUnmappedFastx)
            for (uint32_t m = 0; m < P.dev.readNmates; m++) {
                std::string up = P.outFileNamePrefix + "Unmapped.out.mate" + std::to_string(m + 1);
                unmappedOut[m] = fopen(up.c_str(), "wb");
                if (!unmappedOut[m]) { error = "EXITING because of fatal ERROR: could not create output file " + up; return false; }
            }
        if (P.outSAMnone) post->samOff = true;                      // --outSAMtype None
        else if (P.outBAMcoord && !P.outBAMunsorted) {}             // only Aligned.sortedByCoord.out.bam, written at the end of the run
        else {
            std::string samPath = P.outFileNamePrefix + (P.outBAMunsorted ? "Aligned.out.bam" : "Aligned.out.sam");
            // a regular file is opened for reading too: the writer maps the part of the file a batch goes to, and a shared writable mapping needs a descriptor open read-write
            // (a FIFO or a device keeps "wb": opening a FIFO read-write would not wait for its reader)
            struct stat stOut; const bool special = stat(samPath.c_str(), &stOut) == 0 && !S_ISREG(stOut.st_mode);
            samOut = (P.outBAMunsorted ? P.outStd == "BAM_Unsorted" : P.outStd == "SAM") ? stdout : fopen(samPath.c_str(), special ? "wb" : "w+b");
            if (!samOut) { error = "EXITING because of fatal ERROR: could not create output file " + samPath; return false; }
            setvbuf(samOut, nullptr, _IOFBF, 1 << 22);
            std::string h;
            if (P.outBAMunsorted) { if (!bgzfCompress(post->bamHeader(), P.outBAMcompression, h)) { error = "EXITING because of fatal ERROR: BGZF compression failed"; return false; } }
            else h = post->samHeader();
            fwrite(h.data(), 1, h.size(), samOut);
        }
        {   // Log.out and Log.progress.out exist with the reference's first and last lines (pipelines look for the files and for "ALL DONE!"); what the
            // reference logs in between (its parameter dump, timing of its own stages) has no counterpart here
            FILE *lo = fopen((P.outFileNamePrefix + "Log.out").c_str(), "wb");
            if (lo) {
                fprintf(lo, "STAR version=2.7.11b\nstar_amd: MI355X seed-search-and-stitch engine behind STAR's alignReads command line\n##### Command Line:\n%s\n", P.commandLine.c_str());
                fprintf(lo, "Finished loading and checking parameters\nNumber of real (reference) chromosomes= %u\n", gi.view.nChrReal);
                for (uint32_t i = 0; i < gi.view.nChrReal; i++) fprintf(lo, "%u\t%s\t%llu\t%llu\n", i + 1, gi.chrName[i].c_str(), (unsigned long long)gi.chrLength[i], (unsigned long long)gi.chrStart[i]);
                if (!insertLog.empty()) fputs(insertLog.c_str(), lo);
                fclose(lo);
            }
            FILE *lp = fopen((P.outFileNamePrefix + "Log.progress.out").c_str(), "wb");
            if (lp) {
                fputs("           Time    Speed        Read     Read   Mapped   Mapped   Mapped   Mapped Unmapped Unmapped Unmapped Unmapped\n"
                      "                    M/hr      number   length   unique   length   MMrate    multi   multi+       MM    short    other\n", lp);
                fclose(lp);
            }
        }
        writer.start(samOut, P.runThreadN);
        time(&stats.timeStartMap);
        return true;
    }
    // ---- the batch operations of the C interface, one body each.  `s` is the main set or a slot; `sink` is the error string of the stage that calls (see above)
    void report(std::string &sink, const std::string &msg) { std::lock_guard<std::mutex> l(errM); sink = msg; }
    int converted(BatchSet &s, staramd_batch *out) { if (out) *out = s.batch.view(); if (P.mergedMates()) s.merged.build(s.batch, P); return (int)s.batch.n; }
    int parseBatch(BatchSet &s, uint64_t maxReads, staramd_batch *out, std::string &sink) {
        std::string err;
        const bool ok = reader.nextBatch(s.batch, P, maxReads, err);
        if (!err.empty()) { report(sink, err); return -1; }
        return ok ? converted(s, out) : 0;
    }
    int mergedBatch(BatchSet &s, staramd_batch *out) { if (!P.mergedMates() || s.merged.reads.n == 0) return 0; if (out) *out = s.merged.reads.view(); return (int)s.merged.reads.n; }
    int waspBatch(BatchSet &s, const staramd_results *res, staramd_batch *out) {
        if (!P.wasp || pass1) return 0;
        s.wasp.build(P, gi, variation, s.batch, *res);
        if (out) *out = s.wasp.reads.view();
        return (int)s.wasp.reads.n;
    }
    int waspResults(BatchSet &s, const staramd_results *res, const staramd_results *resWasp, std::string &sink) {
        if (!P.wasp || pass1 || s.wasp.reads.n == 0) return 0;
        if (!resWasp) { report(sink, "EXITING because of FATAL ERROR: --waspOutputMode: results of the re-mapped reads are missing"); return -1; }
        s.wasp.finish(P, s.batch, *res, *resWasp);
        return 0;
    }
    bool emitSet(BatchSet &s, const staramd_results *res, const staramd_results *resMerged, bool withMerged = true) {
        return emitBatch(s.batch, res, withMerged && P.mergedMates() ? &s.merged : nullptr, resMerged, P.wasp ? &s.wasp : nullptr);
    }

    // ---- post-map of one batch on --runThreadN host threads: contiguous read ranges, each with an EmitRange of its own (what the reference keeps per
    // ReadAlignChunk), SAM text written in read order.
    // Which outputs the ranges of a batch produce: decided once per batch, read by the range workers, the counting pass and the fold
    struct EmitOutputs {
        bool bamOut;        // BAM records instead of SAM text: a range's records are compressed on its thread, block by block (bgzf.cpp) ...
        bool devBam;        // ... or, --gpuBAMcompression Device, left uncompressed: one hook call per level compresses them after the join
        bool coordKeys;     // --outSAMtype BAM SortedByCoordinate: a sort key per record
        bool stage1;        // 1st stage of --outFilterType BySJout
        bool geneCounts;    // --quantMode GeneCounts (twoPassRunPass1.cpp:24-29: no quantification in the 1st pass)
        bool trSAM;         // --quantMode TranscriptomeSAM (twoPassRunPass1.cpp:24-29)
        bool chim, chimSam; // --chimSegmentMin > 0 (twoPassRunPass1.cpp:24: no chimeric detection in the 1st pass); Chimeric.out.sam
        bool unmapped;      // --outReadsUnmapped Fastx
        bool randomOrder;   // --outMultimapperOrder Random
        bool timing;        // STARAMD_HOST_TIMING
    };
    struct EmitPlan {
        const ReadBatch *bt; const staramd_results *r;
        const MergedBatch *mg; const staramd_results *mgRes;    // --peOverlapNbasesMin: merged mates and their alignments (null: none in this batch)
        const std::vector<int8_t> *waspType;                    // vW per read (null: off)
        EmitOutputs on;
        uint32_t Wk, T, per;                                    // worker threads, ranges, reads per range
        EmitRange *ranges;                                      // T of them, in the writer's set
        int waspEndOfBatch;
        uint32_t lo(uint32_t t) const { return std::min(bt->n, t * per); }
        uint32_t hi(uint32_t t) const { return std::min(bt->n, lo(t) + per); }
    };
    SamWriter writer;
    double tEmitWaitSet = 0, tEmitFormat = 0, tEmitTail = 0;      // seconds, whole run (STARAMD_HOST_TIMING prints them at the end)

    // step 1: what the batch brings, which outputs are on, how it is cut into ranges
    bool planEmit(EmitPlan &pl, const ReadBatch &bt, const staramd_results *r, const MergedBatch *mg, const staramd_results *mgRes, const WaspBatch *wasp) {
        if (P.wasp && !pass1 && !wasp) { error = "EXITING because of FATAL ERROR: --waspOutputMode: the allele-swapped reads of the batch were not mapped (sah_wasp_batch / sah_wasp_results)"; return false; }
        if (mg && (mg->reads.n == 0 || !mgRes)) { if (mg->reads.n > 0) { error = "EXITING because of FATAL ERROR: --peOverlapNbasesMin: the merged mates of the batch were not mapped (sah_merged_batch / sah_emit_merged)"; return false; } mg = nullptr; }
        pl.bt = &bt; pl.r = r; pl.mg = mg; pl.mgRes = mgRes;
        pl.waspType = (wasp && !pass1) ? &wasp->type : nullptr;
        static const bool hostTiming = getenv("STARAMD_HOST_TIMING") != nullptr;
        EmitOutputs &on = pl.on;
        on.bamOut = (P.outBAMunsorted || P.outBAMcoord) && !post->samOff;
        on.coordKeys = on.bamOut && P.outBAMcoord;
        on.stage1 = bySJoutStage == 1;
        on.geneCounts = P.quantGeneCounts && !pass1;
        on.trSAM = P.quantTrSAM && quantOut && !pass1;
        on.devBam = P.gpuBAMdevice && (on.bamOut || on.trSAM);
        on.chim = P.chim.segmentMin > 0 && !pass1;
        on.chimSam = on.chim && chimSamOut;
        on.unmapped = P.outReadsUnmappedFastx && !pass1;
        on.randomOrder = P.outMultimapperRandom;
        on.timing = hostTiming;
        if (on.devBam && !bgzfDeviceInstalled()) { error = BGZF_DEVICE_MISSING; return false; }
        if (on.coordKeys && P.gpuBAMsortDevice && !bamsortDeviceInstalled()) { error = BAMSORT_DEVICE_MISSING; return false; }
        // T contiguous read ranges, formatted by Wk worker threads that take the next range when they are done with one: with as many
        // ranges as threads the section lasts as long as its slowest thread, and on a shared host (the GPU boxes: 16 CPUs of a 256-thread machine) one descheduled
        // thread held the batch for several times the mean (per-thread busy 2.5 - 5.6 ms in a 24 ms section).  Four ranges per thread; gene counting keeps one
        // (a count table per range)
        pl.Wk = (uint32_t)std::max(1, std::min(P.runThreadN, 256));
        pl.T = (P.quantGeneCounts || P.quantTrSAM) ? pl.Wk : std::min<uint32_t>(4 * pl.Wk, 256);
        pl.T = std::max<uint32_t>(1, std::min<uint32_t>(pl.T, bt.n / 256));       // at least 256 reads per range
        pl.per = (bt.n + pl.T - 1) / pl.T;
        return true;
    }
    // where processRange puts what range `e` produces and what it reads besides the batch: the one statement of it, for the counting pass (dry) and the real one
    void wireRange(const EmitPlan &pl, EmitRange &e, bool dry, PostMap::RangeOut &ro, PostMap::RangeIn &ri) {
        const EmitOutputs &on = pl.on;
        ro.sam = (on.bamOut && !dry) ? &e.raw : &e.sam; ro.sj = &e.sj; ro.st = &e.st;
        if (on.stage1) { ro.sj1 = &e.sj1; ro.held = &e.held; }
        if (on.chim) ro.chimJunction = &e.chim;      // (reads whose chimera goes into the BAM are not quantified: the detection has to run in the counting pass too)
        if (on.trSAM) { ro.quantBam = &e.quantRaw; ro.quantPatches = &e.quantPatches; }
        ri.dry = dry; ri.merged = pl.mg; ri.mergedRes = pl.mgRes;
        if (dry) return;                             // the counting pass asks for what decides the number of transcriptomic alignments of a read, nothing else
        if (on.geneCounts) ro.gc = &e.gc;
        if (on.coordKeys) ro.bamKeys = &e.keys;
        if (on.unmapped) ro.unmappedFastx = e.unmapped;
        if (on.chimSam) ro.chimSam = &e.chimSam;
        ri.order = on.randomOrder ? &multOrder : nullptr; ri.waspType = pl.waspType;
    }
    // step 2 (--outMultimapperOrder Random): all draws of the batch, in read order, from the run's one random stream
    void drawRandomOrder(const EmitPlan &pl) {
        // with TranscriptomeSAM the shuffles of a read and its draw of the primary transcriptomic alignment alternate in one random stream: the
        // number of transcriptomic alignments of every read is needed first (it does not depend on the order), so the quantification runs
        // once into throw-away ranges, then all draws of the batch are made in read order, then the batch is formatted for real
        std::vector<uint32_t> nAlignT;
        if (pl.on.trSAM) {
            nAlignT.assign(pl.bt->n, 0);
            overItems(pl.Wk, CPU_EMIT, pl.T, [&](size_t t) {
                EmitRange e0; PostMap::RangeOut ro; PostMap::RangeIn ri;
                wireRange(pl, e0, true, ro, ri);
                post->processRange(*pl.bt, *pl.r, pl.lo((uint32_t)t), pl.hi((uint32_t)t), ro, ri);      // (an error comes back from the real pass)
                for (const QuantPatch &p : e0.quantPatches) nAlignT[p.ir] = p.nAlignT + 1;
            });
        }
        post->drawMultOrder(*pl.bt, *pl.r, [&] { return rngUniformReal0to1(rngMultOrder); }, multOrder, pl.on.trSAM ? &nAlignT : nullptr, pl.mg, pl.mgRes);
    }
    // step 3, on the worker threads: one range through processRange, its BAM records compressed
    void formatRange(EmitPlan &pl, uint32_t t) {
        EmitRange &e = pl.ranges[t];
        ScopedTimer tm(pl.on.timing ? &e.ms : nullptr, 1e3);
        e.reset(pl.on.geneCounts, genes.geID.size());
        const uint32_t lo = pl.lo(t), hi = pl.hi(t);
        PostMap::RangeOut ro; PostMap::RangeIn ri;
        wireRange(pl, e, false, ro, ri);
        if (pl.waspType && hi == pl.bt->n && lo < hi) ro.waspEnd = &pl.waspEndOfBatch;     // (one range ends the batch)
        e.err = post->processRange(*pl.bt, *pl.r, lo, hi, ro, ri);
        if (!pl.on.bamOut) return;
        bool cut = false;
        if (pl.on.coordKeys) for (const BamKey &k : e.keys) if (k.len & 0x80000000u) { cut = true; break; }
        if (cut) {                                           // KeepPairs with both BAM files: records that belong to the sorted one only
            size_t pos = 0;
            for (BamKey &k : e.keys) if (k.len & 0x80000000u) { k.len &= 0x7fffffffu; e.only.append(e.raw, pos, k.off - pos); pos = k.off + k.len; }
            e.only.append(e.raw, pos, std::string::npos);
            e.cut = true;
        }
        if (pl.on.devBam) return;
        const std::string *records = cut ? &e.only : P.outBAMunsorted ? &e.raw : nullptr;
        if (records && e.err.empty() && !bgzfCompress(*records, P.outBAMcompression, e.sam)) e.err = "EXITING because of fatal ERROR: BGZF compression failed";
    }
    // one random number per mapped read, in read order, picks the primary transcriptomic alignment (ReadAlign_quantTranscriptome.cpp:69);
    // the flag is patched into the records (FLAG is the high half of the 5th word) before they are compressed
    void patchQuant(const EmitPlan &pl, EmitRange &e) {
        for (const QuantPatch &qp : e.quantPatches) {
            uint32_t pick = pl.on.randomOrder ? multOrder.quantPick[qp.ir] : (uint32_t)(int)(rngUniformReal0to1(rngMultOrder) * qp.nAlignT);
            for (size_t k = 0; k < qp.recOffset.size(); k++) {
                uint8_t &hi = (uint8_t &)e.quantRaw[qp.recOffset[k] + 19];
                if (qp.recAlign[k] == pick) hi &= (uint8_t)~1u; else hi |= 1u;
            }
        }
    }
    // step 4 (--gpuBAMcompression Device): the BAM records of all ranges through the device hook, before the set goes to the writer
    void compressOnDevice(const EmitPlan &pl) {
        const auto td0 = std::chrono::steady_clock::now();
        std::vector<BgzfJob> jobs;
        if (pl.on.bamOut)
            for (uint32_t t = 0; t < pl.T; t++) {
                EmitRange &e = pl.ranges[t];
                if (e.cut) jobs.push_back({&e.only, &e.sam, P.outBAMcompression});
                else if (P.outBAMunsorted) jobs.push_back({&e.raw, &e.sam, P.outBAMcompression});
            }
        if (pl.on.trSAM) for (uint32_t t = 0; t < pl.T; t++) { EmitRange &e = pl.ranges[t]; patchQuant(pl, e); jobs.push_back({&e.quantRaw, &e.quantZ, P.quantTrBAMcompression}); }
        error = bgzfCompressDevice(jobs, P.runThreadN);
        if (pl.on.timing) fprintf(stderr, "  emit: BAM records of %zu ranges compressed on the device, %.2f ms\n", jobs.size(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - td0).count());
    }
    // step 5, serial and in range order: the ranges into the run's tables and side files
    bool foldRanges(const EmitPlan &pl, std::chrono::steady_clock::time_point te2) {
        const EmitOutputs &on = pl.on;
        EmitRange *const R = pl.ranges; const uint32_t T = pl.T; const ReadBatch &bt = *pl.bt;
        for (uint32_t t = 0; t < T; t++) { sj.mergeFrom(R[t].sj); stats.add(R[t].st); if (on.geneCounts) geneCounts.add(R[t].gc); }
        if (on.timing) fprintf(stderr, "  emit tail: junction records merged %.2f ms (%zu in the table)\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - te2).count(), sj.data.size());
        if (on.trSAM)
            for (uint32_t t = 0; t < T; t++) {
                if (!on.devBam) patchQuant(pl, R[t]);                           // (Device: patched and compressed before the hand-over)
                const std::string &z = R[t].quantZ;
                if ((!on.devBam && !bgzfCompress(R[t].quantRaw, P.quantTrBAMcompression, R[t].quantZ)) || fwrite(z.data(), 1, z.size(), quantOut) != z.size()) { error = "EXITING because of fatal ERROR: could not write Aligned.toTranscriptome.out.bam"; return false; }
            }
        if (on.chim && chimOut) for (uint32_t t = 0; t < T; t++) if (!R[t].chim.empty()) fwrite(R[t].chim.data(), 1, R[t].chim.size(), chimOut);
        if (on.chimSam) for (uint32_t t = 0; t < T; t++) if (!R[t].chimSam.empty()) fwrite(R[t].chimSam.data(), 1, R[t].chimSam.size(), chimSamOut);
        if (on.unmapped) for (uint32_t t = 0; t < T; t++) for (uint32_t m = 0; m < P.dev.readNmates; m++)
            if (!R[t].unmapped[m].empty() && unmappedOut[m]) fwrite(R[t].unmapped[m].data(), 1, R[t].unmapped[m].size(), unmappedOut[m]);
        if (on.coordKeys)                                           // keep the records for the coordinate sort at the end of the run
            for (uint32_t t = 0; t < T; t++) { error = sorted.take(P, R[t].keys, R[t].raw); if (!error.empty()) return false; }
        if (on.stage1) {
            for (uint32_t t = 0; t < T; t++) {
                sj1.mergeFrom(R[t].sj1);
                for (uint32_t ir : R[t].held)                        // held reads, in input order (ReadAlign_outputAlignments.cpp:108-121)
                    for (uint32_t m = 0; m < P.dev.readNmates; m++) {
                        std::string &x = heldText[m];
                        x.push_back('@'); x += bt.name(ir); x += bt.filter[ir] == 'Y' ? " 0:Y:0 " : " 0:N:0 "; x += std::to_string(bt.readIndex(ir)); x.push_back(' '); x += std::to_string(bt.fileOf(ir));
                        if (!bt.extra((int)m, ir).empty()) { x.push_back('\x01'); x += bt.extra((int)m, ir); }
                        x.push_back('\n');
                        x += bt.seq((int)m, ir); x += "\n+\n"; x += bt.qual((int)m, ir); x.push_back('\n');
                    }
            }
            if (sj1.data.size() > 4000000) sj1.collapse();
        }
        if (pl.waspType && !pl.waspType->empty()) post->waspCarry = pl.waspEndOfBatch;
        if (writer.failed()) { error = "EXITING because of fatal ERROR: could not write Aligned.out.sam"; return false; }
        if (sj.data.size() > sjKick) sjBg.kick(sj);      // (bounded memory: ReadAlignChunk_mapChunk.cpp:66-86)
        return true;
    }
    bool emitBatch(const ReadBatch &bt, const staramd_results *r, const MergedBatch *mg = nullptr, const staramd_results *mgRes = nullptr, const WaspBatch *wasp = nullptr) {
        typedef std::chrono::steady_clock Clock;
        auto ms = [](Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        EmitPlan pl;
        if (!planEmit(pl, bt, r, mg, mgRes, wasp)) return false;
        const auto te0 = Clock::now();
        SamWriter::Set &set = writer.takeFree();
        const auto te1 = Clock::now(); tEmitWaitSet += ms(te0, te1) * 1e-3;
        if (set.ranges.size() < pl.T) set.ranges.resize(pl.T);
        set.used = pl.T; pl.ranges = set.ranges.data();
        if (pl.on.randomOrder) drawRandomOrder(pl);
        const double msBefore = ms(te1, Clock::now());
        pl.waspEndOfBatch = post->waspCarry;
        overItems(pl.Wk, CPU_EMIT, pl.T, [&](size_t t) { formatRange(pl, (uint32_t)t); });
        const auto te2 = Clock::now(); tEmitFormat += ms(te1, te2) * 1e-3;
        if (pl.on.timing) {
            double mn = 1e9, mx = 0, sm = 0;
            for (uint32_t t = 0; t < pl.T; t++) { const double x = pl.ranges[t].ms; mn = std::min(mn, x); mx = std::max(mx, x); sm += x; }
            fprintf(stderr, "  emit: %u ranges on %u threads, section %.2f ms, per-range min %.2f / mean %.2f / max %.2f ms\n", pl.T, std::min(pl.Wk, pl.T), ms(te1, te2), mn, sm / pl.T, mx);
        }
        ScopedTimer tail(&tEmitTail, 1.0, te2);
        for (uint32_t t = 0; t < pl.T; t++) if (!pl.ranges[t].err.empty() && error.empty()) error = pl.ranges[t].err;
        if (pl.on.devBam && error.empty()) compressOnDevice(pl);
        if (!error.empty()) set.used = 0;
        writer.handOver(set);
        if (!error.empty() || !foldRanges(pl, te2)) return false;
        if (pl.on.timing) fprintf(stderr, "  emit: before the threads %.2f ms, threads %.2f ms, tail %.2f ms\n", ms(te0, te1) + msBefore, ms(te1, te2) - msBefore, ms(te2, Clock::now()));
        return true;
    }
    // end of the 1st pass (twoPassRunPass1.cpp:75-96): junctions + Log.final.out of the pass into _STARpass1/, insertion of the
    // junctions into the index, reads rewound.  The caller then re-uploads the index (staramd_update_index).
    bool endPass1() {
        if (!pass1) { error = "not in the 1st pass"; return false; }
        static const bool timing = getenv("STARAMD_HOST_TIMING") != nullptr;
        auto T0 = std::chrono::steady_clock::now();
        auto lap = [&](const char *what) { if (timing) { auto t = std::chrono::steady_clock::now(); fprintf(stderr, "  end of pass 1: %-28s %.1f ms\n", what, std::chrono::duration<double, std::milli>(t - T0).count()); T0 = t; } };
        sjBg.drainInto(sj);
        lap("junction table drained");
        error = sj.filterAndWrite(P, gi, P.twopassDir + "SJ.out.tab");
        if (!error.empty()) return false;
        stats.reportFinal(P.twopassDir + "Log.final.out");
        lap("SJ.out.tab + Log.final.out");
        error = sjdbInsertJunctions(P, gi, sjdbLoci, true, P.twopassDir + "SJ.out.tab", insertLog);
        if (!error.empty()) return false;
        lap("sjdbInsertJunctions");
        error = reader.reopen();
        if (!error.empty()) return false;
        time_t t0 = stats.timeStart;
        stats = Stats(); stats.timeStart = t0; time(&stats.timeStartMap);
        sj.data.clear();
        P.readMapNumber = readMapNumberUser; post->samOff = P.outSAMnone; pass1 = false;
        rngMultOrder.seed((unsigned)P.runRNGseed);                  // the 2nd pass runs on fresh ReadAlign objects (twoPassRunPass1.cpp:31-37)
        P.dev.chimSegmentMinPositive = P.chim.segmentMin > 0 ? 1 : 0;
        if (P.outFilterBySJout) { bySJoutStage = 1; P.dev.outFilterBySJoutStage = 1; }
        return true;
    }
    // end of the 1st stage of BySJout (STAR.cpp:203-216, outputSJ.cpp:139-161): whitelist = filtered unannotated junctions of
    // ALL reads of stage 1; the held reads become the input of stage 2.  The caller hands the whitelist to the engine.
    bool endStage1() {
        if (bySJoutStage != 1) { error = "not in the 1st stage of BySJout"; return false; }
        sj1.novelWhitelist(P, novelStart, novelEnd);
        sj1.data.clear(); sj1.data.shrink_to_fit();
        reader.openMemory(std::move(heldText[0]), std::move(heldText[1]), (int)P.dev.readNmates);
        P.readMapNumber = -1;
        bySJoutStage = 2; P.dev.outFilterBySJoutStage = 2;
        return true;
    }
    // what the caller has to do after the last batch of a phase: 0 = finish(); 1 = the index changed (staramd_update_index), map
    // again; 2 = the junction whitelist changed (staramd_set_novel_junctions), map again
    int nextPhase() {
        if (pass1) return endPass1() ? 1 : -1;
        if (bySJoutStage == 1) return endStage1() ? 2 : -1;
        return 0;
    }
    bool finish() {
        // SJ.out.tab (collapse of the junction table, filters, half a million lines) does not depend on the last writes of the alignments:
        // it is produced on a thread of its own while the writer drains (outputSJ.cpp:84,129; STAR.cpp:251)
        std::string sjError;
        std::thread sjThread;
        sjBg.drainInto(sj);
        if (!P.outSJnone) sjThread = std::thread([&] { sjError = sj.filterAndWrite(P, gi, P.outFileNamePrefix + "SJ.out.tab", bySJoutStage == 2); });
        struct Join { std::thread &t; ~Join() { if (t.joinable()) t.join(); } } joinSj{sjThread};
        writer.stop();
        for (FILE *&u : unmappedOut) if (u) { fclose(u); u = nullptr; }
        if (chimSamOut) { fclose(chimSamOut); chimSamOut = nullptr; }
        if (quantOut) { std::string e; bgzfEof(e); fwrite(e.data(), 1, e.size(), quantOut); if (quantOut == stdout) fflush(stdout); else fclose(quantOut); quantOut = nullptr; }
        if (chimOut) {
            if (P.chim.outJunctionFormat == 1)              // Stats::writeLines (Stats.cpp:147-155, STAR.cpp:285)
                fprintf(chimOut, "# 2.7.11b   %s\n# Nreads %llu\tNreadsUnique %llu\tNreadsMulti %llu\n", P.commandLine.c_str(), (unsigned long long)stats.readN,
                        (unsigned long long)stats.mappedReadsU, (unsigned long long)stats.mappedReadsM);
            fclose(chimOut); chimOut = nullptr;
        }
        if (writer.failed()) { error = "EXITING because of fatal ERROR: could not write Aligned.out.sam"; return false; }
        if (samOut) {
            writer.resumeStream();
            if (P.outBAMunsorted) { std::string e; bgzfEof(e); fwrite(e.data(), 1, e.size(), samOut); }
            if (samOut == stdout) fflush(stdout); else fclose(samOut);
            samOut = nullptr;
        }
        if (P.outBAMcoord && !P.outSAMnone) { error = sorted.write(P, gi, post->bamHeader(true)); if (!error.empty()) return false; }
        if (sjThread.joinable()) sjThread.join();
        error = sjError;
        if (!error.empty()) return false;
        stats.reportFinal(P.outFileNamePrefix + "Log.final.out");
        for (const char *f : {"Log.out", "Log.progress.out"}) appendLog(P.outFileNamePrefix + f, "ALL DONE!\n");
        if (P.quantGeneCounts) { error = geneCounts.write(P.outFileNamePrefix + "ReadsPerGene.out.tab", genes, stats); if (!error.empty()) return false; }
        return true;
    }
    ~Runner() {
        writer.stop();
        sorted.abandon(P);      // (a run that ended early leaves the process-wide sorter empty)
        if (getenv("STARAMD_HOST_TIMING")) fprintf(stderr, "  host stages, whole run: writer %.3f s, emit: wait for a text buffer set %.3f s, format on threads %.3f s, serial tail %.3f s\n", writer.seconds, tEmitWaitSet, tEmitFormat, tEmitTail); if (samOut && samOut != stdout) fclose(samOut); if (quantOut == stdout) quantOut = nullptr; for (FILE *u : unmappedOut) if (u) fclose(u); if (chimOut) fclose(chimOut); if (quantOut) fclose(quantOut); }
};

} // namespace staramd

using staramd::Runner;

extern "C" {

void *sah_create(int argc, char **argv, char *errbuf, int errlen) {
    Runner *r = new Runner();
    if (!r->init(argc, argv)) {
        if (errbuf && errlen > 0) { strncpy(errbuf, r->error.c_str(), errlen - 1); errbuf[errlen - 1] = 0; }
        delete r;
        return nullptr;
    }
    return r;
}
const staramd_genome *sah_genome(void *h) { return &((Runner *)h)->gi.view; }
const staramd_params *sah_params(void *h) { return &((Runner *)h)->P.dev; }
uint64_t sah_batch_reads(void *h) { return ((Runner *)h)->P.gpuBatchReads; }
// --runMode genomeGenerate: sah_create has scanned the FASTA files; the caller builds SA + SAindex with staramd_index_build
// (include/star_amd_index.h) into the buffers handed out here, then sah_generate_finish inserts the annotated junctions and writes genomeDir.
// junction insertion (2-pass, --sjdbGTFfile / --sjdbFileChrStartEnd at the mapping stage, genomeGenerate with annotations) on the device:
// fn = staramd_sjdb_insert of the engine library (include/star_amd_index.h); process-wide; NULL restores the host restatement
void sah_set_sjdb_device_fn(int (*fn)(int, const staramd_sjdb_args *, staramd_sjdb_result *), int device) { staramd::setSjdbDeviceFn(fn, device); }
void sah_set_seq_insert_fn(int (*fn)(int, const staramd_seq_args *, staramd_seq_result *), int device) { staramd::setSeqInsertFn(fn, device); }
void sah_set_bgzf_device_fn(staramd::BgzfDeviceFn fn, void *user) { staramd::setBgzfDeviceFn(fn, user); }
// the same on the arrays resident in the engine contexts (staramd_insert_junctions for every context): fn(user, args, result); the front end calls
// sah_engines_ready once its contexts hold the index, and asks sah_index_in_engine after a phase change whether a re-upload is needed at all
void sah_set_sjdb_resident_fn(int (*fn)(void *, const staramd_sjdb_args *, staramd_sjdb_result *), void *user) { staramd::setSjdbResidentFn(fn, user); }
int sah_chim_select_on_device(void *h) {
    Runner *r = (Runner *)h;
    staramd::RunParams &P = r->P;
    // (chimSegmentMinPositive is 0 during the 1st pass of a 2-pass run -- twoPassRunPass1.cpp:24 -- and comes back with the 2nd: the choice is made once, for the run)
    if (!(P.chim.segmentMin > 0 && P.chim.multimapNmax == 0 && !P.mergedMates() && P.dev.resultSelect == 0)) return 0;
    P.dev.resultSelect = 2;
    return 1;
}
void sah_engines_ready(void *h) {
    // every engine context holds the index now, and junction insertion runs on the resident arrays: the host copy of the suffix array (26 GB of a human
    // index, per process -- one process per GPU on a node) is not needed any more.  SAindex and genome stay (small; the SAM writer reads the genome)
    Runner *r = (Runner *)h;
    r->gi.engineHoldsIndex = true;
    // (--sjdbInsertSave All writes the suffix array into _STARgenome, also when no junction was inserted: it stays)
    if (!r->generateMode && !r->P.sjdbInsertSaveAll && !getenv("STARAMD_KEEP_HOST_SA")) { std::vector<uint8_t>().swap(r->gi.SA); r->gi.view.SA = nullptr; }
}
int sah_index_in_engine(void *h) { Runner *r = (Runner *)h; int v = r->gi.indexInEngine ? 1 : 0; r->gi.indexInEngine = false; return v; }
int sah_generate_mode(void *h) { return ((Runner *)h)->generateMode ? 1 : 0; }
int sah_generate_buffers(void *h, const uint8_t **G, uint64_t *nGenome, uint32_t *GstrandBit, uint32_t *saIndexNbases, uint8_t **SA, uint64_t *saCap, uint8_t **SAi, uint64_t *saiCap) {
    Runner *r = (Runner *)h;
    if (!r->generateMode) { r->error = "sah_generate_buffers: not in --runMode genomeGenerate"; return -1; }
    *G = r->gi.G.data(); *nGenome = r->gi.view.nGenome; *GstrandBit = r->genJob.GstrandBit; *saIndexNbases = r->gi.view.gSAindexNbases;
    *SA = r->gi.SA.data(); *saCap = r->gi.SA.size(); *SAi = r->gi.SAi.data(); *saiCap = r->gi.SAi.size();
    return 0;
}
int sah_generate_finish(void *h, uint64_t nSA, uint64_t nSAbyte, uint64_t nSAibyte) {
    Runner *r = (Runner *)h;
    if (!r->generateMode) { r->error = "sah_generate_finish: not in --runMode genomeGenerate"; return -1; }
    if (nSA != r->genJob.nSA || nSAbyte != r->genJob.saBytes || nSAibyte != r->genJob.saiBytes) { r->error = "EXITING because of FATAL problem while generating the suffix array: the device build returned " + std::to_string(nSA) + " indices, expected nSA=" + std::to_string(r->genJob.nSA); return -1; }
    r->error = genomeGenerateFinish(r->P, r->gi, r->genJob, r->sjdbLoci, r->insertLog);
    return r->error.empty() ? 0 : -1;
}
int sah_tool_done(void *h) { return ((Runner *)h)->toolDone ? 1 : 0; }     // 1: the run was a tool mode (--runMode inputAlignmentsFromBAM) and is finished
int sah_device(void *h) { return ((Runner *)h)->P.gpuDevice; }
int sah_bgzf_on_device(void *h) { return ((Runner *)h)->P.gpuBAMdevice ? 1 : 0; }
void sah_set_bamsort_device(const sah_bamsort_fns *fns, staramd_bamsort *sorter) { staramd::setBamsortDevice(fns, sorter); }
void sah_set_signal_device(const sah_signal_fns *fns) { staramd::setSignalDeviceFns(fns); }
int sah_signal_on_device(void *h) { return ((Runner *)h)->P.gpuSignalDevice ? 1 : 0; }
void sah_signal_counts(void *h, uint64_t out[8]) { for (int i = 0; i < 8; i++) out[i] = ((Runner *)h)->sorted.signalCounts[i]; }
void sah_set_dedup_device(const sah_dedup_fns *fns) { staramd::setDedupDeviceFns(fns); }
void sah_set_inflate_device(const sah_inflate_fns *fns) { staramd::setInflateDeviceFns(fns); }
int sah_inflate_on_device(void *h) { return ((Runner *)h)->P.gpuInflateDevice ? 1 : 0; }
int sah_dedup_on_device(void *h) { return ((Runner *)h)->P.gpuDedupDevice ? 1 : 0; }
void sah_dedup_counts(void *h, uint64_t out[8]) { for (int i = 0; i < 8; i++) out[i] = ((Runner *)h)->dedupCounts[i]; }
int sah_dedup_host_records(const staramd_dedup_params *params, const uint8_t *bytes, uint64_t nBytes, const uint64_t *offsets, uint64_t n, staramd_dedup_result *result) {
    std::vector<const char *> recs(n);
    for (uint64_t i = 0; i < n; i++) {
        uint32_t bs = 0;
        if (offsets[i] > nBytes || nBytes - offsets[i] < 4) return -1;
        memcpy(&bs, bytes + offsets[i], 4);
        if (nBytes - offsets[i] - 4 < bs) return -1;
        recs[i] = (const char *)bytes + offsets[i];
    }
    return staramd::dedupOnHost(recs, params->markMulti != 0, params->mate2basesN, *result) ? 0 : -1;
}
void sah_dedup_host_free(staramd_dedup_result *result) { if (result) { free(result->dup); memset(result, 0, sizeof(*result)); } }
int sah_signal_files_from_runs(int argc, char **argv, int nChr, const char *const *chrName, const uint64_t *chrLength, const void *result, char *errbuf, int errlen) {
    staramd::RunParams P;
    std::string e = P.parse(argc, argv);
    if (e.empty()) e = staramd::signalFromRuns(P, std::vector<std::string>(chrName, chrName + nChr), std::vector<uint64_t>(chrLength, chrLength + nChr), P.outFileNamePrefix + "Signal", *(const staramd_signal_result *)result);
    if (errbuf && errlen > 0) { strncpy(errbuf, e.c_str(), errlen - 1); errbuf[errlen - 1] = 0; }
    return e.empty() ? 0 : -1;
}
int sah_bamsort_on_device(void *h) { return ((Runner *)h)->P.gpuBAMsortDevice ? 1 : 0; }
uint64_t sah_bamsort_budget(void *h) { return ((Runner *)h)->P.gpuBAMsortHBM; }
void sah_bam_sort_counts(void *h, uint64_t out[4]) { const staramd::CoordSortedBam &s = ((Runner *)h)->sorted; out[0] = s.sortCounts[0]; out[1] = s.sortCounts[1]; out[2] = s.appendsTaken; out[3] = s.spilled ? 1 : 0; }
double sah_genome_load_seconds(void *h) { return ((Runner *)h)->gi.loadSeconds; }
void sah_cpu_add(int stage, uint64_t ns) { staramd::cpuAdd(stage, ns); }
void sah_cpu_seconds(double out[8], int reset) { for (int i = 0; i < staramd::CPU_NSTAGE; i++) out[i] = (double)staramd::cpuTake(i, reset != 0) * 1e-9; }
void sah_fast_path_counts(void *h, uint64_t out[2]) { Runner *r = (Runner *)h; out[0] = r->writer.mappedWrites; out[1] = r->reader.mappedBatches.load(); }
void sah_emit_seconds(void *h, double out[4]) { Runner *r = (Runner *)h; out[0] = r->tEmitWaitSet; out[1] = r->tEmitFormat; out[2] = r->tEmitTail; out[3] = r->writer.seconds; }
// ---- batch operations.  Every one exists for the main batch (one batch at a time: sah_next_batch, map, sah_emit) and for a slot of the pipelined variant (star_amd CLI:
// FASTQ parsing of batch k+1, the device mapping of batch k and the post-map / SAM writing of batch k-1 overlap; parse and emit are each called from ONE thread, in
// batch order).  Both forward to one member function of Runner with their batch set and the error string of their stage.
int sah_next_batch(void *h, uint64_t maxReads, staramd_batch *out) { Runner *r = (Runner *)h; return r->parseBatch(r->mainSet, maxReads, out, r->error); }
int sah_parse_slot(void *h, int slot, uint64_t maxReads, staramd_batch *out) { Runner *r = (Runner *)h; return r->parseBatch(r->slots[slot], maxReads, out, r->parseError); }
int sah_emit(void *h, const staramd_results *res) { Runner *r = (Runner *)h; return r->emitSet(r->mainSet, res, nullptr) ? 0 : -1; }
// --peOverlapNbasesMin > 0: after sah_next_batch, sah_merged_batch gives the pairs of the batch whose mates overlap, merged into single reads (0 = none);
// map them with the same engine and hand both result sets to sah_emit_merged.  Same for the slots of the pipelined variant.
int sah_merged_batch(void *h, staramd_batch *out) { Runner *r = (Runner *)h; return r->mergedBatch(r->mainSet, out); }
int sah_merged_slot(void *h, int slot, staramd_batch *out) { Runner *r = (Runner *)h; return r->mergedBatch(r->slots[slot], out); }
int sah_emit_merged(void *h, const staramd_results *res, const staramd_results *resMerged) { Runner *r = (Runner *)h; return r->emitSet(r->mainSet, res, resMerged) ? 0 : -1; }
int sah_emit_slot_merged(void *h, int slot, const staramd_results *res, const staramd_results *resMerged) { Runner *r = (Runner *)h; return r->emitSet(r->slots[slot], res, resMerged) ? 0 : -1; }
// (a slot emitted without results of merged mates: the caller found none -- sah_merged_slot -- and nothing is asked of the slot's merged batch)
int sah_emit_slot(void *h, int slot, const staramd_results *res) { Runner *r = (Runner *)h; return r->emitSet(r->slots[slot], res, nullptr, false) ? 0 : -1; }
// --waspOutputMode SAMtag: after mapping a batch, sah_wasp_batch builds from its results the allele-swapped reads that WASP maps again (0 = none, still call
// sah_wasp_results with NULL); map them with the same engine, hand the results to sah_wasp_results, then emit as usual.  *_slot: the pipelined variant, on the mapper threads.
int sah_wasp_batch(void *h, const staramd_results *res, staramd_batch *out) { Runner *r = (Runner *)h; return r->waspBatch(r->mainSet, res, out); }
int sah_wasp_slot(void *h, int slot, const staramd_results *res, staramd_batch *out) { Runner *r = (Runner *)h; return r->waspBatch(r->slots[slot], res, out); }
int sah_wasp_results(void *h, const staramd_results *res, const staramd_results *resWasp) { Runner *r = (Runner *)h; return r->waspResults(r->mainSet, res, resWasp, r->error); }
int sah_wasp_results_slot(void *h, int slot, const staramd_results *res, const staramd_results *resWasp) { Runner *r = (Runner *)h; return r->waspResults(r->slots[slot], res, resWasp, r->mapError); }
// page-locked (or any other) memory for the numeric arrays of the batches; call once, before the first batch is parsed and never with batches alive
void sah_set_batch_alloc(void *(*alloc)(uint64_t), void (*release)(void *)) { staramd::g_batchAllocFn = alloc; staramd::g_batchFreeFn = release; }
int sah_fill_slot(void *h, int slot, uint64_t maxReads) {
    Runner *r = (Runner *)h;
    std::string err;
    bool ok = r->reader.fillBatch(r->slots[slot].batch, r->P, maxReads, err);
    if (!err.empty()) { r->report(r->parseError, err); return -1; }
    return ok ? (int)r->slots[slot].batch.n : 0;
}
int sah_convert_slot(void *h, int slot, staramd_batch *out) {
    Runner *r = (Runner *)h;
    std::string err;
    bool ok = r->reader.convertBatch(r->slots[slot].batch, r->P, err);
    if (!ok || !err.empty()) { r->report(r->parseError, err.empty() ? "convertBatch failed" : err); return -1; }
    return r->converted(r->slots[slot], out);
}
int sah_threads(void *h) { return ((Runner *)h)->P.runThreadN; }
// 2-pass mapping: sah_in_pass1() is 1 after sah_create when --twopassMode Basic was given; map all batches, call sah_pass1_end()
// (junction insertion on the host), re-upload sah_genome()/sah_params() with staramd_update_index(), map all batches again.
int sah_in_pass1(void *h) { return ((Runner *)h)->pass1 ? 1 : 0; }
uint64_t sah_limit_sjdb_insert(void *h) { return (uint64_t)((Runner *)h)->P.limitSjdbInsertNsj; }
uint32_t sah_sjdb_length(void *h) { Runner *r = (Runner *)h; const uint32_t ov = r->gi.view.sjdbOverhang ? r->gi.view.sjdbOverhang : r->P.sjdbOverhang; return 2 * ov + 1; }
int sah_pass1_end(void *h) { return ((Runner *)h)->endPass1() ? 0 : -1; }
// general form (2-pass and/or --outFilterType BySJout): after the last batch call sah_next_phase(): 0 = done, call sah_finish();
// 1 = the index was rewritten: staramd_update_index(sah_genome(), sah_params()) and map every batch again; 2 = the junction
// whitelist was built: staramd_set_novel_junctions(sah_novel_junctions(...), stage 2) and map every batch again; < 0 = error
int sah_next_phase(void *h) { return ((Runner *)h)->nextPhase(); }
uint64_t sah_novel_junctions(void *h, const uint64_t **start, const uint64_t **end) {
    Runner *r = (Runner *)h;
    *start = r->novelStart.data(); *end = r->novelEnd.data();
    return r->novelStart.size();
}
const char *sah_insert_log(void *h) { return ((Runner *)h)->insertLog.c_str(); }
int sah_finish(void *h) { return ((Runner *)h)->finish() ? 0 : -1; }
// ---- end-of-run exchange between ranks (one process per GPU) -------------------------------------
// The reference merges per-thread junction tables and Stats inside one process (outputSJ.cpp:39-83 k-way merge,
// ReadAlignChunk_mapChunk.cpp:124-127 Stats::addStats).  With one process per GPU the same two reductions go over
// RCCL: every rank exports its COLLAPSED table as fixed 32-byte records + 32 counters, rank 0 imports them and then
// runs the unchanged collapse/filter/write.
struct SjWire { uint64_t start; uint32_t gap; uint32_t countUnique, countMultiple; uint16_t overhangLeft, overhangRight; int8_t strand, motif, annot; uint8_t pad[5]; };
static_assert(sizeof(SjWire) == 32, "junction wire record is 32 bytes");

uint64_t sah_sj_export(void *h, void *buf, uint64_t capRecords) {
    Runner *r = (Runner *)h;
    r->wire().collapse();
    uint64_t n = r->wire().data.size();
    if (!buf) return n;
    if (n > capRecords) return (uint64_t)-1;
    SjWire *w = (SjWire *)buf;
    for (uint64_t i = 0; i < n; i++) {
        const staramd::Junction &j = r->wire().data[i];
        SjWire x; memset(&x, 0, sizeof(x));
        x.start = j.start; x.gap = j.gap; x.countUnique = j.countUnique; x.countMultiple = j.countMultiple;
        x.overhangLeft = j.overhangLeft; x.overhangRight = j.overhangRight; x.strand = j.strand; x.motif = j.motif; x.annot = j.annot;
        w[i] = x;
    }
    return n;
}
int sah_sj_import(void *h, const void *buf, uint64_t nRecords) {
    Runner *r = (Runner *)h;
    const SjWire *w = (const SjWire *)buf;
    for (uint64_t i = 0; i < nRecords; i++) {
        staramd::Junction j; j.start = w[i].start; j.gap = w[i].gap; j.strand = w[i].strand; j.motif = w[i].motif; j.annot = w[i].annot;
        j.countUnique = w[i].countUnique; j.countMultiple = w[i].countMultiple; j.overhangLeft = w[i].overhangLeft; j.overhangRight = w[i].overhangRight;
        r->wire().data.push_back(j);
    }
    return 0;
}
void sah_sj_clear(void *h) { ((Runner *)h)->wire().data.clear(); }
// which table the three calls above address: 0 = the output table, 1 = the table of the 1st BySJout stage (all reads' junctions)
void sah_sj_select(void *h, int which) { ((Runner *)h)->wireTable = which; }
int sah_in_stage1(void *h) { return ((Runner *)h)->bySJoutStage == 1 ? 1 : 0; }
// --quantMode GeneCounts across ranks: 7 counters + 3 x nGe gene counts
uint64_t sah_quant_export(void *h, uint64_t *out, uint64_t cap) {
    Runner *r = (Runner *)h;
    if (!r->P.quantGeneCounts) return 0;
    const staramd::GeneCounts &g = r->geneCounts;
    uint64_t nGe = g.gCount[0].size(), n = 7 + 3 * nGe;
    if (!out) return n;
    if (cap < n) return (uint64_t)-1;
    out[0] = g.cMulti; for (int t = 0; t < 3; t++) { out[1 + t] = g.cAmbig[t]; out[4 + t] = g.cNone[t]; for (uint64_t i = 0; i < nGe; i++) out[7 + t * nGe + i] = g.gCount[t][i]; }
    return n;
}
int sah_quant_import_add(void *h, const uint64_t *in, uint64_t n) {
    Runner *r = (Runner *)h;
    staramd::GeneCounts &g = r->geneCounts;
    uint64_t nGe = g.gCount[0].size();
    if (n != 7 + 3 * nGe) return -1;
    g.cMulti += in[0]; for (int t = 0; t < 3; t++) { g.cAmbig[t] += in[1 + t]; g.cNone[t] += in[4 + t]; for (uint64_t i = 0; i < nGe; i++) g.gCount[t][i] += in[7 + t * nGe + i]; }
    return 0;
}
#define SAH_NSTAT 32
// counters as 32 x u64; mappedPortion (double) travels as its bit pattern and is summed by the importer
int sah_stats_export(void *h, uint64_t *out) {
    const staramd::Stats &s = ((Runner *)h)->stats;
    memset(out, 0, SAH_NSTAT * 8);
    uint64_t v[] = {s.readN, s.readBases, s.mappedMismatchesN, s.mappedInsN, s.mappedDelN, s.mappedInsL, s.mappedDelL, s.mappedBases, s.mappedReadsU,
                    s.mappedReadsM, s.unmappedOther, s.unmappedShort, s.unmappedMismatch, s.unmappedMulti, s.unmappedAll, s.chimericAll, s.splicesNsjdb,
                    s.splicesN[0], s.splicesN[1], s.splicesN[2], s.splicesN[3], s.splicesN[4], s.splicesN[5], s.splicesN[6]};
    for (size_t i = 0; i < sizeof(v) / 8; i++) out[i] = v[i];
    memcpy(&out[24], &s.mappedPortion, 8);
    return SAH_NSTAT;
}
int sah_stats_import_add(void *h, const uint64_t *in) {
    staramd::Stats &s = ((Runner *)h)->stats;
    staramd::Stats a;
    a.readN = in[0]; a.readBases = in[1]; a.mappedMismatchesN = in[2]; a.mappedInsN = in[3]; a.mappedDelN = in[4]; a.mappedInsL = in[5]; a.mappedDelL = in[6];
    a.mappedBases = in[7]; a.mappedReadsU = in[8]; a.mappedReadsM = in[9]; a.unmappedOther = in[10]; a.unmappedShort = in[11]; a.unmappedMismatch = in[12];
    a.unmappedMulti = in[13]; a.unmappedAll = in[14]; a.chimericAll = in[15]; a.splicesNsjdb = in[16];
    for (int i = 0; i < 7; i++) a.splicesN[i] = in[17 + i];
    memcpy(&a.mappedPortion, &in[24], 8);
    s.add(a);
    return 0;
}
const char *sah_error(void *h) {
    Runner *r = (Runner *)h;
    static thread_local std::string mine;
    std::lock_guard<std::mutex> l(r->errM);
    if (!r->parseError.empty()) mine = r->parseError; else if (!r->mapError.empty()) mine = r->mapError; else return r->error.c_str();
    return mine.c_str();
}
void sah_destroy(void *h) { delete (Runner *)h; }

}

// struct sizes of the C ABI, so that language bindings can verify their mirrors
extern "C" uint64_t sah_sizeof(int which) {
    switch (which) {
        case 0: return sizeof(staramd_genome);
        case 1: return sizeof(staramd_params);
        case 2: return sizeof(staramd_batch);
        case 3: return sizeof(staramd_read_result);
        case 4: return sizeof(staramd_transcript);
        case 5: return sizeof(staramd_exon);
        case 6: return sizeof(staramd_results);
        default: return 0;
    }
}
