"""ctypes mirror of include/star_amd.h and of the host library's `sah_*` interface.

Python is only plumbing here (tests, bench.py, smoke): the product is the C-ABI library
star_amd/lib/libstaramd.so (hand-written HIP for gfx950) plus the C++ host library
star_amd/lib/libstaramd_host.so.  Loading fails loudly if a library is missing.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")
# STARAMD_ENGINE_LIB=shadow selects the shadow-validation build (tests only; see star_amd/csrc/engine/stitch_scalar.h)
_VARIANT = os.environ.get("STARAMD_ENGINE_LIB", "")
ENGINE_PATH = os.path.join(LIB_DIR, {"shadow": "libstaramd_shadow.so", "profile": "libstaramd_profile.so"}.get(_VARIANT, "libstaramd.so"))
if "/" in _VARIANT:                      # an explicit library path (build experiments)
    ENGINE_PATH = _VARIANT
HOST_PATH = os.path.join(LIB_DIR, "libstaramd_host.so")

u8p = C.POINTER(C.c_uint8)
u16p = C.POINTER(C.c_uint16)
u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)


class Genome(C.Structure):
    _fields_ = [
        ("G", u8p), ("nGenome", C.c_uint64),
        ("SA", u8p), ("nSA", C.c_uint64), ("nSAbyte", C.c_uint64),
        ("SAi", u8p), ("nSAi", C.c_uint64), ("nSAibyte", C.c_uint64),
        ("GstrandBit", C.c_uint32), ("gSAindexNbases", C.c_uint32),
        ("genomeSAindexStart", C.c_uint64 * 17),
        ("gSAsparseD", C.c_uint32), ("gChrBinNbits", C.c_uint32),
        ("chrStart", u64p), ("chrLength", u64p), ("nChrReal", C.c_uint32),
        ("chrBin", u32p), ("chrBinN", C.c_uint64),
        ("sjGstart", C.c_uint64), ("sjdbOverhang", C.c_uint32), ("sjdbLength", C.c_uint32), ("sjdbN", C.c_uint32),
        ("sjDstart", u64p), ("sjAstart", u64p), ("sjdbStart", u64p), ("sjdbEnd", u64p),
        ("sjdbMotif", u8p), ("sjdbShiftLeft", u8p), ("sjdbShiftRight", u8p), ("sjdbStrand", u8p),
    ]


class Params(C.Structure):
    _fields_ = [
        ("readNmates", C.c_uint32),
        ("seedSearchStartLmax", C.c_uint32), ("seedSearchStartLmaxOverLread", C.c_double),
        ("seedSearchLmax", C.c_uint32), ("seedMultimapNmax", C.c_uint32), ("seedPerReadNmax", C.c_uint32),
        ("seedPerWindowNmax", C.c_uint32), ("seedSplitMin", C.c_uint32), ("seedMapMin", C.c_uint32), ("maxNsplit", C.c_uint32),
        ("winAnchorMultimapNmax", C.c_uint32), ("winBinNbits", C.c_uint32), ("winAnchorDistNbins", C.c_uint32),
        ("winFlankNbins", C.c_uint32), ("winBinChrNbits", C.c_uint32), ("winBinN", C.c_uint64),
        ("alignWindowsPerReadNmax", C.c_uint32), ("alignTranscriptsPerWindowNmax", C.c_uint32), ("alignTranscriptsPerReadNmax", C.c_uint32),
        ("alignIntronMin", C.c_uint64), ("alignIntronMax", C.c_uint64), ("alignMatesGapMax", C.c_uint64),
        ("alignSJoverhangMin", C.c_uint32), ("alignSJDBoverhangMin", C.c_uint32),
        ("alignSJstitchMismatchNmax", C.c_int32 * 4),
        ("alignSplicedMateMapLmin", C.c_uint32), ("alignSplicedMateMapLminOverLmate", C.c_double),
        ("alignEndsTypeExt", (C.c_uint8 * 2) * 2),
        ("alignEndsProtrudeNbasesMax", C.c_int32),
        ("alignEndsProtrudeConcordantPair", C.c_uint8), ("alignSoftClipAtReferenceEnds", C.c_uint8),
        ("alignInsertionFlushRight", C.c_uint8), ("outFilterIntronStrandsRemoveInconsistent", C.c_uint8),
        ("outFilterIntronMotifs", C.c_uint8), ("outSAMstrandFieldIntronMotif", C.c_uint8),
        ("chimSegmentMinPositive", C.c_uint8), ("outFilterBySJoutStage", C.c_uint8),
        ("scoreGap", C.c_int32), ("scoreGapNoncan", C.c_int32), ("scoreGapGCAG", C.c_int32), ("scoreGapATAC", C.c_int32),
        ("scoreDelOpen", C.c_int32), ("scoreDelBase", C.c_int32), ("scoreInsOpen", C.c_int32), ("scoreInsBase", C.c_int32),
        ("scoreStitchSJshift", C.c_int32), ("sjdbScore", C.c_int32),
        ("scoreGenomicLengthLog2scale", C.c_double),
        ("outFilterMultimapScoreRange", C.c_int32),
        ("outFilterMismatchNoverLmax", C.c_double),
        ("outFilterMatchNmin", C.c_uint32),
        ("resultSelect", C.c_uint32),
        ("chimSegmentMin", C.c_uint32), ("chimSegmentReadGapMax", C.c_uint32),
    ]


class Batch(C.Structure):
    _fields_ = [("nReads", C.c_uint32), ("bases", u8p), ("readOffset", u64p), ("mate1Length", u16p), ("mmMaxTotal", u16p)]


class ReadResult(C.Structure):
    _fields_ = [("status", C.c_uint32), ("nW", C.c_uint32), ("nTr", C.c_uint32), ("trOffset", C.c_uint32),
                ("trBest", C.c_int32), ("maxScoreMate", C.c_int32 * 2), ("unmappedLength", C.c_uint32)]


class Transcript(C.Structure):
    _fields_ = [("iW", C.c_uint32), ("exonOffset", C.c_uint32), ("nExons", C.c_uint16),
                ("rStart", C.c_uint16), ("rLength", C.c_uint16), ("roStart", C.c_uint16),
                ("Str", C.c_uint8), ("roStr", C.c_uint8), ("iFrag", C.c_int8), ("sjMotifStrand", C.c_uint8),
                ("Chr", C.c_uint32), ("gStart", C.c_uint64), ("gLength", C.c_uint64), ("maxScore", C.c_int32),
                ("nMatch", C.c_uint32), ("nMM", C.c_uint32), ("mappedLength", C.c_uint32),
                ("nGap", C.c_uint32), ("lGap", C.c_uint32), ("nDel", C.c_uint32), ("lDel", C.c_uint32), ("nIns", C.c_uint32), ("lIns", C.c_uint32),
                ("nUnique", C.c_uint16), ("nAnchor", C.c_uint16), ("intronMotifs", C.c_uint16 * 3), ("pad0", C.c_uint16), ("pad1", C.c_uint32)]


class Exon(C.Structure):
    _fields_ = [("G", C.c_uint64), ("R", C.c_uint16), ("L", C.c_uint16), ("sjA", C.c_int32), ("iFrag", C.c_uint8),
                ("canonSJ", C.c_int8), ("sjAnnot", C.c_uint8), ("sjStr", C.c_uint8), ("shiftSJ", C.c_uint16 * 2), ("pad0", C.c_uint32), ("pad1", C.c_uint32)]


class Results(C.Structure):
    _fields_ = [("reads", C.POINTER(ReadResult)),
                ("tr", C.POINTER(Transcript)), ("trCapacity", C.c_uint64), ("trCount", C.c_uint64),
                ("ex", C.POINTER(Exon)), ("exCapacity", C.c_uint64), ("exCount", C.c_uint64),
                ("msSeed", C.c_float), ("msWindows", C.c_float), ("msStitch", C.c_float), ("msTotalDevice", C.c_float)]


class ResultBuffers:
    """Caller-owned result arrays for one batch."""

    def __init__(self, n_reads, tr_cap=None, ex_cap=None):
        tr_cap = tr_cap or max(1024, n_reads * 24)
        ex_cap = ex_cap or tr_cap * 4
        self.reads = (ReadResult * n_reads)()
        self.tr = (Transcript * tr_cap)()
        self.ex = (Exon * ex_cap)()
        self.res = Results()
        self.res.reads = C.cast(self.reads, C.POINTER(ReadResult))
        self.res.tr = C.cast(self.tr, C.POINTER(Transcript)); self.res.trCapacity = tr_cap
        self.res.ex = C.cast(self.ex, C.POINTER(Exon)); self.res.exCapacity = ex_cap

    def as_bytes(self, n_reads):
        """(reads, transcripts, exons) raw bytes of the filled part -- for bit-exact comparisons."""
        r = self.res
        return (bytes(memoryview(self.reads))[:n_reads * C.sizeof(ReadResult)],
                bytes(memoryview(self.tr))[:r.trCount * C.sizeof(Transcript)],
                bytes(memoryview(self.ex))[:r.exCount * C.sizeof(Exon)])


def map_in_pieces(map_one, batch, bufs, max_reads):
    """A batch larger than an engine context takes (e.g. the re-mapping batch of --waspOutputMode, where a read over a dense SNV cluster has hundreds of
    copies): mapped in pieces of at most max_reads reads through map_one(piece, piece_bufs); the results are appended into bufs as if it had been one call."""
    n, done, tr_n, ex_n = batch.nReads, 0, 0, 0
    ro = C.cast(batch.readOffset, C.c_void_p).value; m1 = C.cast(batch.mate1Length, C.c_void_p).value; mm = C.cast(batch.mmMaxTotal, C.c_void_p).value
    while done < n:
        k = min(max_reads, n - done)
        piece = Batch()
        piece.nReads = k; piece.bases = batch.bases
        piece.readOffset = C.cast(ro + 8 * done, type(batch.readOffset)); piece.mate1Length = C.cast(m1 + 2 * done, type(batch.mate1Length)); piece.mmMaxTotal = C.cast(mm + 2 * done, type(batch.mmMaxTotal))
        pb = ResultBuffers(k, tr_cap=max(1024, bufs.res.trCapacity // 2))
        map_one(piece, pb)
        if tr_n + pb.res.trCount > bufs.res.trCapacity or ex_n + pb.res.exCount > bufs.res.exCapacity:
            raise RuntimeError("map_in_pieces: result buffers too small (-3)")
        for i in range(k):
            bufs.reads[done + i] = pb.reads[i]
            bufs.reads[done + i].trOffset += tr_n
        C.memmove(C.byref(bufs.tr, tr_n * C.sizeof(Transcript)), pb.tr, pb.res.trCount * C.sizeof(Transcript))
        for i in range(pb.res.trCount):
            bufs.tr[tr_n + i].exonOffset += ex_n
        C.memmove(C.byref(bufs.ex, ex_n * C.sizeof(Exon)), pb.ex, pb.res.exCount * C.sizeof(Exon))
        tr_n += pb.res.trCount; ex_n += pb.res.exCount; done += k
    bufs.res.trCount = tr_n; bufs.res.exCount = ex_n


def _need(path):
    if not os.path.isfile(path):
        raise RuntimeError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (or `make`) first; "
                           "there is no Python/CPU fallback for the hot path" % path)
    return path


_host = None
_engine = None


def host_lib():
    global _host
    if _host is None:
        L = C.CDLL(_need(HOST_PATH))
        L.sah_create.restype = C.c_void_p
        L.sah_create.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_int]
        L.sah_genome.restype = C.POINTER(Genome); L.sah_genome.argtypes = [C.c_void_p]
        L.sah_params.restype = C.POINTER(Params); L.sah_params.argtypes = [C.c_void_p]
        L.sah_batch_reads.restype = C.c_uint64; L.sah_batch_reads.argtypes = [C.c_void_p]
        L.sah_genome_load_seconds.restype = C.c_double; L.sah_genome_load_seconds.argtypes = [C.c_void_p]
        L.sah_next_batch.restype = C.c_int; L.sah_next_batch.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(Batch)]
        L.sah_emit.restype = C.c_int; L.sah_emit.argtypes = [C.c_void_p, C.POINTER(Results)]
        L.sah_wasp_batch.restype = C.c_int; L.sah_wasp_batch.argtypes = [C.c_void_p, C.POINTER(Results), C.POINTER(Batch)]
        L.sah_wasp_results.restype = C.c_int; L.sah_wasp_results.argtypes = [C.c_void_p, C.POINTER(Results), C.POINTER(Results)]
        L.sah_merged_batch.restype = C.c_int; L.sah_merged_batch.argtypes = [C.c_void_p, C.POINTER(Batch)]
        L.sah_emit_merged.restype = C.c_int; L.sah_emit_merged.argtypes = [C.c_void_p, C.POINTER(Results), C.POINTER(Results)]
        L.sah_finish.restype = C.c_int; L.sah_finish.argtypes = [C.c_void_p]
        L.sah_error.restype = C.c_char_p; L.sah_error.argtypes = [C.c_void_p]
        L.sah_destroy.restype = None; L.sah_destroy.argtypes = [C.c_void_p]
        L.sah_in_pass1.restype = C.c_int; L.sah_in_pass1.argtypes = [C.c_void_p]
        L.sah_pass1_end.restype = C.c_int; L.sah_pass1_end.argtypes = [C.c_void_p]
        L.sah_insert_log.restype = C.c_char_p; L.sah_insert_log.argtypes = [C.c_void_p]
        L.sah_next_phase.restype = C.c_int; L.sah_next_phase.argtypes = [C.c_void_p]
        L.sah_novel_junctions.restype = C.c_uint64; L.sah_novel_junctions.argtypes = [C.c_void_p, C.POINTER(u64p), C.POINTER(u64p)]
        _host = L
    return _host


def engine_lib():
    """The HIP engine.  Raises if the extension has not been built: no fallback."""
    global _engine
    if _engine is None:
        L = C.CDLL(_need(ENGINE_PATH))
        L.staramd_create.restype = C.c_int
        L.staramd_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(Genome), C.POINTER(Params), C.c_uint32, C.c_uint64]
        L.staramd_update_index.restype = C.c_int
        L.staramd_update_index.argtypes = [C.c_void_p, C.POINTER(Genome), C.POINTER(Params)]
        L.staramd_set_novel_junctions.restype = C.c_int
        L.staramd_set_novel_junctions.argtypes = [C.c_void_p, u64p, u64p, C.c_uint64, C.c_uint32]
        L.staramd_map_batch.restype = C.c_int
        L.staramd_map_batch.argtypes = [C.c_void_p, C.POINTER(Batch), C.POINTER(Results)]
        L.staramd_map_resident.restype = C.c_int
        L.staramd_map_resident.argtypes = [C.c_void_p, C.POINTER(Results)]
        L.staramd_destroy.restype = None; L.staramd_destroy.argtypes = [C.c_void_p]
        L.staramd_last_error.restype = C.c_char_p
        L.staramd_get_timings.restype = C.c_int
        L.staramd_get_timings.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int]
        L.staramd_get_counters.restype = C.c_int
        L.staramd_get_counters.argtypes = [C.c_void_p, u64p, C.c_int]
        if hasattr(L, "staramd_launch_count"):
            L.staramd_launch_count.restype = C.c_uint64; L.staramd_launch_count.argtypes = [C.c_void_p]
        # include/star_amd_async.h, staramd_create_shared, staramd_update_tables (tests of call sequences: tests/history_run.py)
        L.staramd_create_shared.restype = C.c_int
        L.staramd_create_shared.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_uint32, C.c_uint64]
        L.staramd_update_tables.restype = C.c_int
        L.staramd_update_tables.argtypes = [C.c_void_p, C.POINTER(Genome), C.POINTER(Params)]
        L.staramd_map_begin.restype = C.c_int; L.staramd_map_begin.argtypes = [C.c_void_p, C.POINTER(Batch)]
        L.staramd_map_wait.restype = C.c_int; L.staramd_map_wait.argtypes = [C.c_void_p]
        L.staramd_map_end.restype = C.c_int; L.staramd_map_end.argtypes = [C.c_void_p, C.POINTER(Results), C.POINTER(Batch)]
        L.staramd_prefetch_batch.restype = C.c_int; L.staramd_prefetch_batch.argtypes = [C.c_void_p, C.POINTER(Batch)]
        L.staramd_prefetch_cancel.restype = C.c_int; L.staramd_prefetch_cancel.argtypes = [C.c_void_p]
        L.staramd_prefetch_hits.restype = C.c_uint64; L.staramd_prefetch_hits.argtypes = [C.c_void_p]
        L.staramd_overlapped_batches.restype = C.c_uint64; L.staramd_overlapped_batches.argtypes = [C.c_void_p]
        _engine = L
    return _engine


class HostRun:
    """One alignReads run on the host side: STAR-style argv in, SAM/SJ/Log files out."""

    def __init__(self, argv):
        L = host_lib()
        args = [b"star_amd"] + [a.encode() if isinstance(a, str) else a for a in argv]
        arr = (C.c_char_p * len(args))(*args)
        err = C.create_string_buffer(4096)
        self.h = L.sah_create(len(args), arr, err, 4096)
        if not self.h:
            raise RuntimeError(err.value.decode())
        self.L = L
        self.genome = L.sah_genome(self.h)
        self.params = L.sah_params(self.h)
        self._bgzf = None
        self._bamsort = None
        self._signal = None

    def set_bgzf_device(self, bz):
        """--gpuBAMcompression Device: BAM records of this run are compressed by `bz` (a BgzfDevice; None uninstalls).  The hook is process-wide
        (sah_set_bgzf_device_fn); close() uninstalls it."""
        L = self.L
        L.sah_set_bgzf_device_fn.restype = None; L.sah_set_bgzf_device_fn.argtypes = [C.c_void_p, C.c_void_p]
        if bz is None:
            L.sah_set_bgzf_device_fn(None, None)
        else:
            L.sah_set_bgzf_device_fn(C.cast(bz.L.staramd_bgzf_compress, C.c_void_p), bz.z)
        self._bgzf = bz

    def set_bamsort_device(self, bs):
        """--gpuBAMsort Device: the records of this run's Aligned.sortedByCoord.out.bam go to `bs` (a BamSortDevice; None uninstalls).  Process-wide
        (sah_set_bamsort_device); close() uninstalls it."""
        L = self.L
        L.sah_set_bamsort_device.restype = None; L.sah_set_bamsort_device.argtypes = [C.c_void_p, C.c_void_p]
        if bs is None:
            L.sah_set_bamsort_device(None, None)
        else:
            fns, s = bs.fns()
            L.sah_set_bamsort_device(C.byref(fns), s)
        self._bamsort = bs

    def set_signal_device(self, sg):
        """--gpuSignal Device: the tracks of --outWigType come from `sg` (a SignalDevice; None uninstalls).  Process-wide (sah_set_signal_device); close()
        uninstalls it.  The tool mode (--runMode inputAlignmentsFromBAM) runs inside HostRun(): use SignalDevice.install() before it."""
        if sg is None:
            SignalDevice.uninstall()
        else:
            sg.install()
        self._signal = sg

    def signal_on_device(self):
        """True: --gpuSignal Device"""
        self.L.sah_signal_on_device.restype = C.c_int; self.L.sah_signal_on_device.argtypes = [C.c_void_p]
        return bool(self.L.sah_signal_on_device(self.h))

    def signal_counts(self):
        """sah_signal_counts: [1 when the device computed the tracks, records, spans, bytes of the runs, ns of the stage, ns of the device's record pass, sort, tile passes]"""
        self.L.sah_signal_counts.restype = None; self.L.sah_signal_counts.argtypes = [C.c_void_p, u64p]
        out = (C.c_uint64 * 8)()
        self.L.sah_signal_counts(self.h, out)
        return list(out)

    def dedup_on_device(self):
        """True: --gpuBAMdedup Device"""
        self.L.sah_dedup_on_device.restype = C.c_int; self.L.sah_dedup_on_device.argtypes = [C.c_void_p]
        return bool(self.L.sah_dedup_on_device(self.h))

    def dedup_counts(self):
        """sah_dedup_counts: [records, unique records, pairs, classes, records marked, unpaired unique records, ns of the device's kernels, ns of its copies]"""
        self.L.sah_dedup_counts.restype = None; self.L.sah_dedup_counts.argtypes = [C.c_void_p, u64p]
        out = (C.c_uint64 * 8)()
        self.L.sah_dedup_counts(self.h, out)
        return list(out)

    def bamsort_budget(self):
        """--gpuBAMsortHBM: what the run's BamSortDevice is to be created with"""
        self.L.sah_bamsort_budget.restype = C.c_uint64; self.L.sah_bamsort_budget.argtypes = [C.c_void_p]
        return self.L.sah_bamsort_budget(self.h)

    def bam_sort_counts(self):
        """sah_bam_sort_counts: [records ordered on the device, their bytes, appends the device took, 1 when the run spilled to the host]"""
        self.L.sah_bam_sort_counts.restype = None; self.L.sah_bam_sort_counts.argtypes = [C.c_void_p, u64p]
        out = (C.c_uint64 * 4)()
        self.L.sah_bam_sort_counts(self.h, out)
        return list(out)

    def next_batch(self, max_reads):
        b = Batch()
        n = self.L.sah_next_batch(self.h, max_reads, C.byref(b))
        if n < 0:
            raise RuntimeError(self.L.sah_error(self.h).decode())
        return b if n > 0 else None

    def merged_batch(self):
        """--peOverlapNbasesMin > 0: the pairs of the current batch whose mates overlap, merged into single reads (None when there are none).
        Map it with the same engine and pass its results to emit() as `merged`."""
        b = Batch()
        n = self.L.sah_merged_batch(self.h, C.byref(b))
        return b if n > 0 else None

    def wasp_batch(self, results):
        """--waspOutputMode SAMtag: the allele-swapped reads built from the results of the current batch (None when there are none); map them with the same
        engine and hand their results to wasp_results() before emit()."""
        b = Batch()
        n = self.L.sah_wasp_batch(self.h, C.byref(results), C.byref(b))
        return b if n > 0 else None

    def wasp_results(self, results, wasp_results):
        if self.L.sah_wasp_results(self.h, C.byref(results), C.byref(wasp_results) if wasp_results is not None else None) != 0:
            raise RuntimeError(self.L.sah_error(self.h).decode())

    def emit(self, results, merged=None):
        rc = self.L.sah_emit(self.h, C.byref(results)) if merged is None else self.L.sah_emit_merged(self.h, C.byref(results), C.byref(merged))
        if rc != 0:
            raise RuntimeError(self.L.sah_error(self.h).decode())

    def in_pass1(self):
        """True while the 1st pass of --twopassMode Basic is running (map every batch, then call pass1_end())."""
        return bool(self.L.sah_in_pass1(self.h))

    def pass1_end(self):
        """Write _STARpass1/, insert the junctions into the host index, rewind the reads; the engine must then be
        given the new index (Engine.update_index(run.genome, run.params))."""
        if self.L.sah_pass1_end(self.h) != 0:
            raise RuntimeError(self.L.sah_error(self.h).decode())

    def next_phase(self):
        """After the last batch: 0 = done (finish()); 1 = the index was rewritten by junction insertion (engine.update_index(run.genome,
        run.params), then map every batch again); 2 = the whitelist of the 2nd BySJout stage was built
        (engine.set_novel_junctions(*run.novel_junctions()), then map every batch again)."""
        r = self.L.sah_next_phase(self.h)
        if r < 0:
            raise RuntimeError(self.L.sah_error(self.h).decode())
        return r

    def novel_junctions(self):
        a, b = u64p(), u64p()
        n = self.L.sah_novel_junctions(self.h, C.byref(a), C.byref(b))
        return a, b, n

    def finish(self):
        if self.L.sah_finish(self.h) != 0:
            raise RuntimeError(self.L.sah_error(self.h).decode())

    def close(self):
        if self.h:
            self.L.sah_destroy(self.h)
            self.h = None
        if self._bgzf is not None:
            self.set_bgzf_device(None)
        if self._bamsort is not None:
            self.set_bamsort_device(None)
        if self._signal is not None:
            self.set_signal_device(None)


class Engine:
    """The MI355X engine context (one per GPU)."""

    def __init__(self, genome_p, params_p, device=0, max_reads=65536, max_bases=None, share_with=None):
        """share_with: another Engine whose resident index this context maps against (staramd_create_shared); genome_p / params_p are then not used"""
        L = engine_lib()
        self.L = L
        self.ctx = C.c_void_p()
        self.max_reads = max_reads
        max_bases = max_bases or max_reads * 660
        if share_with is not None:
            rc = L.staramd_create_shared(C.byref(self.ctx), share_with.ctx, max_reads, max_bases)
        else:
            rc = L.staramd_create(C.byref(self.ctx), device, genome_p, params_p, max_reads, max_bases)
        if rc != 0:
            raise RuntimeError("staramd_create failed (%d): %s" % (rc, L.staramd_last_error().decode()))

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, self.L.staramd_last_error().decode()))

    def update_index(self, genome_p, params_p):
        rc = self.L.staramd_update_index(self.ctx, genome_p, params_p)
        if rc != 0:
            raise RuntimeError("staramd_update_index failed (%d): %s" % (rc, self.L.staramd_last_error().decode()))

    def set_novel_junctions(self, start, end, n, stage=2):
        rc = self.L.staramd_set_novel_junctions(self.ctx, start, end, n, stage)
        if rc != 0:
            raise RuntimeError("staramd_set_novel_junctions failed (%d): %s" % (rc, self.L.staramd_last_error().decode()))

    def map_batch(self, batch, bufs):
        if batch.nReads > self.max_reads:        # more reads than the context was created for: in pieces
            return map_in_pieces(self.map_batch, batch, bufs, self.max_reads)
        rc = self.L.staramd_map_batch(self.ctx, C.byref(batch), C.byref(bufs.res))
        if rc != 0:
            raise RuntimeError("staramd_map_batch failed (%d): %s" % (rc, self.L.staramd_last_error().decode()))

    def map_batch_rc(self, batch, bufs):
        """staramd_map_batch as it is: the return code (STARAMD_ERR_RESULT_OVERFLOW = -3 included), nothing raised, no pieces"""
        return self.L.staramd_map_batch(self.ctx, C.byref(batch), C.byref(bufs.res))

    def update_tables(self, genome_p, params_p):
        self._check(self.L.staramd_update_tables(self.ctx, genome_p, params_p), "staramd_update_tables")

    def map_begin(self, batch):
        self._check(self.L.staramd_map_begin(self.ctx, C.byref(batch)), "staramd_map_begin")

    def map_wait(self):
        self._check(self.L.staramd_map_wait(self.ctx), "staramd_map_wait")

    def map_end_rc(self, bufs, next_batch=None):
        return self.L.staramd_map_end(self.ctx, C.byref(bufs.res), C.byref(next_batch) if next_batch is not None else None)

    def map_end(self, bufs, next_batch=None):
        self._check(self.map_end_rc(bufs, next_batch), "staramd_map_end")

    def prefetch(self, batch):
        self._check(self.L.staramd_prefetch_batch(self.ctx, C.byref(batch)), "staramd_prefetch_batch")

    def prefetch_cancel(self):
        self._check(self.L.staramd_prefetch_cancel(self.ctx), "staramd_prefetch_cancel")

    def prefetch_hits(self):
        return self.L.staramd_prefetch_hits(self.ctx)

    def overlapped_batches(self):
        return self.L.staramd_overlapped_batches(self.ctx)

    def launch_count(self):
        return self.L.staramd_launch_count(self.ctx)

    def map_resident(self, bufs):
        rc = self.L.staramd_map_resident(self.ctx, C.byref(bufs.res))
        if rc != 0:
            raise RuntimeError("staramd_map_resident failed (%d): %s" % (rc, self.L.staramd_last_error().decode()))

    def counters(self, n=40):
        out = (C.c_uint64 * n)()
        k = self.L.staramd_get_counters(self.ctx, out, n)
        return list(out)[:k]

    def timings(self):
        out = (C.c_float * 7)()
        k = self.L.staramd_get_timings(self.ctx, out, 7)
        return dict(zip(["seed", "windows", "order", "stitch_walk", "stitch_redecide", "gather", "total"], list(out)[:k]))

    def close(self):
        if self.ctx:
            self.L.staramd_destroy(self.ctx)
            self.ctx = C.c_void_p()


class BgzfDevice:
    """include/star_amd_bgzf.h: BGZF compression on the MI355X (k_bgzf.hip in libstaramd.so); lib_path: another library with that ABI (the wave
    emulator's build of k_bgzf.hip in the CPU tests)."""

    def __init__(self, device=0, initial_bytes=0, lib_path=None):
        L = C.CDLL(lib_path or _need(ENGINE_PATH))
        L.staramd_bgzf_create.restype = C.c_int
        L.staramd_bgzf_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_uint64]
        L.staramd_bgzf_bound.restype = C.c_uint64; L.staramd_bgzf_bound.argtypes = [C.c_uint64]
        L.staramd_bgzf_compress.restype = C.c_int
        L.staramd_bgzf_compress.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.POINTER(C.c_void_p), u64p, C.c_void_p, C.c_uint64, u64p]
        L.staramd_bgzf_destroy.restype = None; L.staramd_bgzf_destroy.argtypes = [C.c_void_p]
        L.staramd_bgzf_last_error.restype = C.c_char_p
        self.L = L
        self.z = C.c_void_p()
        if L.staramd_bgzf_create(C.byref(self.z), device, initial_bytes) != 0:
            raise RuntimeError("staramd_bgzf_create failed: %s" % L.staramd_bgzf_last_error().decode())

    def compress(self, level, segments):
        """segments: list of bytes -> list of their BGZF members (bytes), one entry per segment"""
        n = len(segments)
        keep = [C.create_string_buffer(bytes(s), len(s)) for s in segments]
        ins = (C.c_void_p * max(n, 1))(*[C.cast(k, C.c_void_p) for k in keep])
        lens = (C.c_uint64 * max(n, 1))(*[len(s) for s in segments])
        cap = sum(self.L.staramd_bgzf_bound(len(s)) for s in segments)
        out = C.create_string_buffer(max(cap, 1))
        out_len = (C.c_uint64 * max(n, 1))()
        if self.L.staramd_bgzf_compress(self.z, level, n, ins, lens, out, cap, out_len) != 0:
            raise RuntimeError("staramd_bgzf_compress failed: %s" % self.L.staramd_bgzf_last_error().decode())
        raw, res, o = out.raw, [], 0
        for i in range(n):
            res.append(raw[o:o + out_len[i]])
            o += out_len[i]
        return res

    def close(self):
        if self.z:
            self.L.staramd_bgzf_destroy(self.z)
            self.z = C.c_void_p()


class BamKey(C.Structure):
    """staramd_bam_key (include/star_amd_bamsort.h)"""
    _fields_ = [("g", C.c_uint64), ("r", C.c_uint64), ("off", C.c_uint64), ("len", C.c_uint32), ("reserved", C.c_uint32)]


BAMSORT_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64)


class BamSortFns(C.Structure):
    """sah_bamsort_fns (include/star_amd_host.h)"""
    _fields_ = [("append", C.c_void_p), ("download", C.c_void_p), ("finish", C.c_void_p), ("last_error", C.c_void_p)]


class BamSortDevice:
    """include/star_amd_bamsort.h: records ordered by (g, r, order of appending) and BGZF-compressed on the MI355X (k_bamsort.hip in libstaramd.so), with
    the stream and kernels of `bz` (a BgzfDevice, which must stay open); lib_path: another library with that ABI -- the one `bz` came from."""

    def __init__(self, bz, budget=0, lib_path=None):
        L = C.CDLL(lib_path or _need(ENGINE_PATH))
        L.staramd_bamsort_create.restype = C.c_int
        L.staramd_bamsort_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_uint64]
        L.staramd_bamsort_append.restype = C.c_int
        L.staramd_bamsort_append.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(BamKey), C.c_uint32]
        L.staramd_bamsort_download.restype = C.c_int
        L.staramd_bamsort_download.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.staramd_bamsort_finish.restype = C.c_int
        L.staramd_bamsort_finish.argtypes = [C.c_void_p, C.c_int, BAMSORT_SINK, C.c_void_p, u64p]
        L.staramd_bamsort_destroy.restype = None; L.staramd_bamsort_destroy.argtypes = [C.c_void_p]
        L.staramd_bamsort_last_error.restype = C.c_char_p
        self.L = L
        self.bz = bz
        self.s = C.c_void_p()
        self.stats = [0] * 8
        if L.staramd_bamsort_create(C.byref(self.s), bz.z, budget) != 0:
            raise RuntimeError("staramd_bamsort_create failed: %s" % L.staramd_bamsort_last_error().decode())

    def append(self, records, keys):
        """records: bytes; keys: (g, r, off, len) per record, off into `records`.  True = taken, False = it does not fit the budget (nothing taken)"""
        buf = C.create_string_buffer(bytes(records), max(len(records), 1))
        ks = (BamKey * max(len(keys), 1))(*[BamKey(g, r, off, ln, 0) for g, r, off, ln in keys])
        rc = self.L.staramd_bamsort_append(self.s, buf, len(records), ks, len(keys))
        if rc < 0:
            raise RuntimeError("staramd_bamsort_append failed: %s" % self.L.staramd_bamsort_last_error().decode())
        return rc == 0

    def download(self, i_append, n_bytes):
        out = C.create_string_buffer(max(n_bytes, 1))
        if self.L.staramd_bamsort_download(self.s, i_append, out) != 0:
            raise RuntimeError("staramd_bamsort_download failed: %s" % self.L.staramd_bamsort_last_error().decode())
        return out.raw[:n_bytes]

    def finish(self, level):
        """the BGZF members of the ordered stream, as bytes; the sorter is empty afterwards.  self.stats: the eight counters of the call"""
        parts = []
        sink = BAMSORT_SINK(lambda user, p, n: parts.append(C.string_at(p, n)) or 0)
        st = (C.c_uint64 * 8)()
        if self.L.staramd_bamsort_finish(self.s, level, sink, None, st) != 0:
            raise RuntimeError("staramd_bamsort_finish failed: %s" % self.L.staramd_bamsort_last_error().decode())
        self.stats = list(st)
        return b"".join(parts)

    def fns(self):
        """(sah_bamsort_fns, sorter) for HostRun.set_bamsort_device"""
        f = BamSortFns(*[C.cast(getattr(self.L, "staramd_bamsort_" + n), C.c_void_p) for n in ("append", "download", "finish", "last_error")])
        return f, self.s

    def close(self):
        if self.s:
            self.L.staramd_bamsort_destroy(self.s)
            self.s = C.c_void_p()


class SignalParams(C.Structure):
    """staramd_signal_params (include/star_amd_signal.h)"""
    _fields_ = [("type", C.c_int32), ("strand", C.c_int32), ("nChr", C.c_uint32), ("wantNorm", C.c_uint32), ("chrLength", C.POINTER(C.c_uint32)), ("wanted", C.POINTER(C.c_uint8))]


class SignalRun(C.Structure):
    """staramd_signal_run"""
    _fields_ = [("tid", C.c_int32), ("track", C.c_uint32), ("start", C.c_uint32), ("end", C.c_uint32), ("value", C.c_double)]


class SignalResult(C.Structure):
    """staramd_signal_result"""
    _fields_ = [("runs", C.POINTER(SignalRun)), ("nRuns", C.c_uint64), ("norm", C.POINTER(C.c_uint32)), ("nRecords", C.c_uint64),
                ("chrHas", C.POINTER(C.c_uint8)), ("nChr", C.c_uint32), ("pastEnd", C.c_uint32), ("stats", C.c_uint64 * 8)]


class SignalFns(C.Structure):
    """sah_signal_fns (include/star_amd_host.h)"""
    _fields_ = [("host_records", C.c_void_p), ("finish_signal", C.c_void_p), ("free_result", C.c_void_p), ("last_error", C.c_void_p)]


class SignalDevice:
    """include/star_amd_signal.h: the tracks of --outWigType from BAM records in coordinate order on the MI355X (k_signal.hip in libstaramd.so); lib_path:
    another library with that ABI (the wave emulator's build in the CPU tests; for sorter_tracks the one the BamSortDevice came from)."""

    def __init__(self, lib_path=None):
        L = C.CDLL(lib_path or _need(ENGINE_PATH))
        L.staramd_signal_host_records.restype = C.c_int
        L.staramd_signal_host_records.argtypes = [C.c_int, C.POINTER(SignalParams), C.c_void_p, C.c_uint64, u64p, C.c_uint64, C.POINTER(SignalResult)]
        L.staramd_bamsort_finish_signal.restype = C.c_int
        L.staramd_bamsort_finish_signal.argtypes = [C.c_void_p, C.c_int, BAMSORT_SINK, C.c_void_p, u64p, C.POINTER(SignalParams), C.POINTER(SignalResult)]
        L.staramd_signal_free.restype = None; L.staramd_signal_free.argtypes = [C.POINTER(SignalResult)]
        L.staramd_signal_constant.restype = C.c_uint32; L.staramd_signal_constant.argtypes = [C.c_int]
        L.staramd_signal_last_error.restype = C.c_char_p
        self.L = L
        self.tile = L.staramd_signal_constant(0)
        self.chunk = L.staramd_signal_constant(1)

    @staticmethod
    def _params(type_, strand, chr_length, wanted, want_norm):
        n = len(chr_length)
        ln = (C.c_uint32 * max(n, 1))(*chr_length)
        wt = (C.c_uint8 * max(n, 1))(*[1 if w else 0 for w in wanted])
        return SignalParams(type_, 1 if strand else 0, n, 1 if want_norm else 0, ln, wt), (ln, wt)

    def _take(self, res):
        """(runs [(tid, track, start, end, value)], norm list or None, chrHas list, pastEnd, stats) of a result, which is freed"""
        try:
            runs = [(r.tid, r.track, r.start, r.end, r.value) for r in (res.runs[i] for i in range(res.nRuns))]
            norm = [res.norm[i] for i in range(res.nRecords)] if res.norm else None
            return runs, norm, [res.chrHas[i] for i in range(res.nChr)], bool(res.pastEnd), list(res.stats)
        finally:
            self.L.staramd_signal_free(C.byref(res))

    def host_records(self, records, type_=0, strand=True, chr_length=(), wanted=None, want_norm=True, device=0):
        """records: list of BAM records (bytes, each with its block_size word) in coordinate order"""
        blob = b"".join(records)
        offs, o = [], 0
        for r in records:
            offs.append(o); o += len(r)
        p, keep = self._params(type_, strand, chr_length, wanted if wanted is not None else [1] * len(chr_length), want_norm)
        res = SignalResult()
        buf = C.create_string_buffer(blob, max(len(blob), 1))
        if self.L.staramd_signal_host_records(device, C.byref(p), buf, len(blob), (C.c_uint64 * max(len(offs), 1))(*offs), len(offs), C.byref(res)) != 0:
            raise RuntimeError("staramd_signal_host_records failed: %s" % self.L.staramd_signal_last_error().decode())
        return self._take(res)

    def sorter_tracks(self, bs, level, type_=0, strand=True, chr_length=(), wanted=None, want_norm=True):
        """staramd_bamsort_finish_signal on the BamSortDevice `bs`: (the BGZF members as bytes, the result as host_records returns it)"""
        parts = []
        sink = BAMSORT_SINK(lambda user, p, n: parts.append(C.string_at(p, n)) or 0)
        st = (C.c_uint64 * 8)()
        p, keep = self._params(type_, strand, chr_length, wanted if wanted is not None else [1] * len(chr_length), want_norm)
        res = SignalResult()
        if self.L.staramd_bamsort_finish_signal(bs.s, level, sink, None, st, C.byref(p), C.byref(res)) != 0:
            raise RuntimeError("staramd_bamsort_finish_signal failed: %s" % self.L.staramd_signal_last_error().decode())
        bs.stats = list(st)
        return b"".join(parts), self._take(res)

    def install(self):
        """sah_set_signal_device with this library's functions (process-wide)"""
        L = host_lib()
        L.sah_set_signal_device.restype = None; L.sah_set_signal_device.argtypes = [C.c_void_p]
        names = ("staramd_signal_host_records", "staramd_bamsort_finish_signal", "staramd_signal_free", "staramd_signal_last_error")
        self._fns = SignalFns(*[C.cast(getattr(self.L, n), C.c_void_p) for n in names])
        L.sah_set_signal_device(C.byref(self._fns))

    @staticmethod
    def uninstall():
        L = host_lib()
        L.sah_set_signal_device.restype = None; L.sah_set_signal_device.argtypes = [C.c_void_p]
        L.sah_set_signal_device(None)


def signal_files_from_runs(argv, chr_names, chr_length, runs, norm, chr_has, past_end=False):
    """the host formatter alone (signalFromRuns of signal.cpp): the Signal.* files of a run with the --outWig* flags in `argv` (and --outFileNamePrefix)
    from runs [(tid, track, start, end, value)], the per-record normalisation words and the has-records flags; returns the error text ("" = none)"""
    L = host_lib()
    L.sah_signal_files_from_runs.restype = C.c_int
    L.sah_signal_files_from_runs.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_char_p), u64p, C.POINTER(SignalResult), C.c_char_p, C.c_int]
    args = [b"star_amd"] + [a.encode() for a in argv]
    names = [n.encode() for n in chr_names]
    rs = (SignalRun * max(len(runs), 1))(*[SignalRun(*r) for r in runs])
    nm = (C.c_uint32 * max(len(norm or []), 1))(*(norm or []))
    ch = (C.c_uint8 * max(len(chr_has), 1))(*chr_has)
    res = SignalResult(rs, len(runs), nm if norm is not None else None, len(norm or []), ch, len(chr_has), 1 if past_end else 0)
    err = C.create_string_buffer(4096)
    L.sah_signal_files_from_runs(len(args), (C.c_char_p * len(args))(*args), len(names), (C.c_char_p * max(len(names), 1))(*names), (C.c_uint64 * max(len(names), 1))(*chr_length), C.byref(res), err, 4096)
    return err.value.decode()


class DedupParams(C.Structure):
    """staramd_dedup_params (include/star_amd_dedup.h)"""
    _fields_ = [("markMulti", C.c_int32), ("mate2basesN", C.c_uint32)]


class DedupResult(C.Structure):
    """staramd_dedup_result"""
    _fields_ = [("dup", C.POINTER(C.c_uint8)), ("nRecords", C.c_uint64), ("fatal", C.c_int32), ("fatalRecord", C.c_uint64), ("stats", C.c_uint64 * 8)]


class DedupFns(C.Structure):
    """sah_dedup_fns (include/star_amd_host.h)"""
    _fields_ = [("host_records", C.c_void_p), ("free_result", C.c_void_p), ("last_error", C.c_void_p)]


class DedupDevice:
    """include/star_amd_dedup.h: the duplicate pairs of --bamRemoveDuplicatesType on the MI355X (k_dedup.hip in libstaramd.so); lib_path: another library
    with that ABI (the wave emulator's build in the CPU tests)."""

    def __init__(self, device=0, lib_path=None):
        L = C.CDLL(lib_path or _need(ENGINE_PATH))
        L.staramd_dedup_host_records.restype = C.c_int
        L.staramd_dedup_host_records.argtypes = [C.c_int, C.POINTER(DedupParams), C.c_void_p, C.c_uint64, u64p, C.c_uint64, C.POINTER(DedupResult)]
        L.staramd_dedup_free.restype = None; L.staramd_dedup_free.argtypes = [C.POINTER(DedupResult)]
        L.staramd_dedup_constant.restype = C.c_uint32; L.staramd_dedup_constant.argtypes = [C.c_int]
        L.staramd_dedup_last_error.restype = C.c_char_p
        self.L = L
        self.device = device
        self.workgroup = L.staramd_dedup_constant(0)
        self.workgroups_per_cu = L.staramd_dedup_constant(1)

    def max_workgroups(self):
        """STARAMD_DEDUP_MAX_WORKGROUPS as the next call will read it (0: not set, the default of workgroups_per_cu per CU holds)"""
        return self.L.staramd_dedup_constant(2)

    def host_records(self, records, mark_multi=True, mate2bases_n=0):
        """records: list of BAM records (bytes, each with its block_size word) in coordinate order.  Returns (dup bytes or None when fatal, fatal, fatalRecord, stats)"""
        dev = self.device
        return _dedup_call(lambda p, buf, n_bytes, offs, n, res: self.L.staramd_dedup_host_records(dev, p, buf, n_bytes, offs, n, res), self.L.staramd_dedup_free,
                           lambda: "staramd_dedup_host_records failed: %s" % self.L.staramd_dedup_last_error().decode(), records, mark_multi, mate2bases_n)

    def install(self):
        """sah_set_dedup_device with this library's functions (process-wide).  The tool mode runs inside HostRun(): install before it"""
        L = host_lib()
        L.sah_set_dedup_device.restype = None; L.sah_set_dedup_device.argtypes = [C.c_void_p]
        names = ("staramd_dedup_host_records", "staramd_dedup_free", "staramd_dedup_last_error")
        self._fns = DedupFns(*[C.cast(getattr(self.L, n), C.c_void_p) for n in names])
        L.sah_set_dedup_device(C.byref(self._fns))

    @staticmethod
    def uninstall():
        L = host_lib()
        L.sah_set_dedup_device.restype = None; L.sah_set_dedup_device.argtypes = [C.c_void_p]
        L.sah_set_dedup_device(None)


def _dedup_call(call, free, error_text, records, mark_multi, mate2bases_n):
    """the records laid out as the two entries of the duplicate marking take them (bytes + offsets), one call, the result as Python values and released"""
    blob = b"".join(records)
    offs, o = [], 0
    for r in records:
        offs.append(o); o += len(r)
    p = DedupParams(1 if mark_multi else 0, mate2bases_n)
    res = DedupResult()
    buf = C.create_string_buffer(blob, max(len(blob), 1))
    if call(C.byref(p), buf, len(blob), (C.c_uint64 * max(len(offs), 1))(*offs), len(offs), C.byref(res)) != 0:
        raise RuntimeError(error_text())
    try:
        dup = C.string_at(res.dup, res.nRecords) if res.dup and not res.fatal else (b"" if not res.fatal else None)
        return dup, res.fatal, res.fatalRecord, list(res.stats)
    finally:
        free(C.byref(res))


def dedup_host(records, mark_multi=True, mate2bases_n=0):
    """the host path's rule alone (dedupOnHost of host/dedup.cpp) on records in memory: what DedupDevice.host_records returns"""
    L = host_lib()
    L.sah_dedup_host_records.restype = C.c_int
    L.sah_dedup_host_records.argtypes = [C.POINTER(DedupParams), C.c_void_p, C.c_uint64, u64p, C.c_uint64, C.POINTER(DedupResult)]
    L.sah_dedup_host_free.restype = None; L.sah_dedup_host_free.argtypes = [C.POINTER(DedupResult)]
    return _dedup_call(L.sah_dedup_host_records, L.sah_dedup_host_free, lambda: "sah_dedup_host_records failed: a record lies outside the bytes, or no memory for the result",
                       records, mark_multi, mate2bases_n)


class InflateResult(C.Structure):
    """staramd_inflate_result (include/star_amd_inflate.h)"""
    _fields_ = [("bytes", C.POINTER(C.c_uint8)), ("nBytes", C.c_uint64), ("nMembers", C.c_uint64), ("failedMember", C.c_int64), ("failedStatus", C.c_uint32),
                ("stats", C.c_uint64 * 8)]


class InflateFns(C.Structure):
    """sah_inflate_fns (include/star_amd_host.h)"""
    _fields_ = [("host_file", C.c_void_p), ("free_result", C.c_void_p), ("last_error", C.c_void_p)]


class InflateDevice:
    """include/star_amd_inflate.h: a BGZF file inflated on the MI355X (k_inflate.hip in libstaramd.so); lib_path: another library with that ABI (the wave
    emulator's build in the CPU tests)."""
    STATUS = ("OK", "BLOCK_TYPE", "STORED_LEN", "OVERSUBSCRIBED", "INCOMPLETE", "NO_END_CODE", "REPEAT", "SYMBOL", "DISTANCE", "INPUT_END", "OUTPUT_OVER",
              "OUTPUT_SHORT", "STREAM_END", "CRC", "TOO_MANY")

    def __init__(self, device=0, lib_path=None):
        L = C.CDLL(lib_path or _need(ENGINE_PATH))
        L.staramd_inflate_host_file.restype = C.c_int
        L.staramd_inflate_host_file.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.POINTER(InflateResult)]
        L.staramd_inflate_free.restype = None; L.staramd_inflate_free.argtypes = [C.POINTER(InflateResult)]
        L.staramd_inflate_constant.restype = C.c_uint32; L.staramd_inflate_constant.argtypes = [C.c_int]
        L.staramd_inflate_last_error.restype = C.c_char_p
        self.L = L
        self.device = device
        self.workgroup = L.staramd_inflate_constant(0)
        self.members_per_workgroup = L.staramd_inflate_constant(1)
        self.workgroups_per_cu = L.staramd_inflate_constant(2)
        self.lds_per_wavefront = L.staramd_inflate_constant(4)

    def max_workgroups(self):
        """STARAMD_INFLATE_MAX_WORKGROUPS as the next call will read it (0: not set, the default of workgroups_per_cu per CU holds)"""
        return self.L.staramd_inflate_constant(3)

    def host_file(self, data):
        """data: the bytes of a BGZF file.  Returns (inflated bytes or None when a member failed, failedMember or -1, the status' name, nMembers, stats)"""
        res = InflateResult()
        buf = C.create_string_buffer(bytes(data), max(len(data), 1))
        if self.L.staramd_inflate_host_file(self.device, buf, len(data), C.byref(res)) != 0:
            raise RuntimeError("staramd_inflate_host_file failed: %s" % self.L.staramd_inflate_last_error().decode())
        try:
            failed = res.failedMember >= 0
            out = None if failed else (C.string_at(res.bytes, res.nBytes) if res.bytes else b"")
            return out, res.failedMember, self.STATUS[res.failedStatus], res.nMembers, list(res.stats)
        finally:
            self.L.staramd_inflate_free(C.byref(res))

    def install(self):
        """sah_set_inflate_device with this library's functions (process-wide).  The tool mode runs inside HostRun(): install before it"""
        L = host_lib()
        L.sah_set_inflate_device.restype = None; L.sah_set_inflate_device.argtypes = [C.c_void_p]
        names = ("staramd_inflate_host_file", "staramd_inflate_free", "staramd_inflate_last_error")
        self._fns = InflateFns(*[C.cast(getattr(self.L, n), C.c_void_p) for n in names])
        L.sah_set_inflate_device(C.byref(self._fns))

    @staticmethod
    def uninstall():
        L = host_lib()
        L.sah_set_inflate_device.restype = None; L.sah_set_inflate_device.argtypes = [C.c_void_p]
        L.sah_set_inflate_device(None)


class device_sjdb_insertion:
    """Context manager: junction insertion (2-pass, --sjdbFileChrStartEnd / --sjdbGTFfile at the mapping stage) of every HostRun created inside
    runs through `fn_lib.fn_name` -- staramd_sjdb_insert of the engine library on a GPU box, or its plain-loop twin in the CPU tests
    (oracle/_build/libindex_emul.so: sjdb_emul_insert) -- instead of the host restatement.  Process-wide switch of the host library."""

    def __init__(self, lib_path=None, fn_name="staramd_sjdb_insert", device=0):
        self.lib = C.CDLL(lib_path or _need(ENGINE_PATH))
        self.fn = C.cast(getattr(self.lib, fn_name), C.c_void_p)
        self.device = device

    def __enter__(self):
        L = host_lib()
        L.sah_set_sjdb_device_fn.restype = None; L.sah_set_sjdb_device_fn.argtypes = [C.c_void_p, C.c_int]
        L.sah_set_sjdb_device_fn(self.fn, self.device)
        return self

    def __exit__(self, *a):
        host_lib().sah_set_sjdb_device_fn(None, 0)
        return False


class device_seq_insertion:
    """Context manager: the sequences that --genomeFastaFiles adds at the mapping stage are inserted, for every HostRun created inside, through
    `fn_lib.fn_name` -- staramd_seq_insert of the engine library on a GPU box, or its plain-loop twin in the CPU tests
    (oracle/_build/libseq_emul.so: seq_emul_insert).  Process-wide switch of the host library; there is no host restatement behind it."""

    def __init__(self, lib_path=None, fn_name="staramd_seq_insert", device=0):
        self.lib = C.CDLL(lib_path or _need(ENGINE_PATH))
        self.fn = C.cast(getattr(self.lib, fn_name), C.c_void_p)
        self.device = device

    def __enter__(self):
        L = host_lib()
        L.sah_set_seq_insert_fn.restype = None; L.sah_set_seq_insert_fn.argtypes = [C.c_void_p, C.c_int]
        L.sah_set_seq_insert_fn(self.fn, self.device)
        return self

    def __exit__(self, *a):
        host_lib().sah_set_seq_insert_fn(None, 0)
        return False


# ---- the command-line front end as a function (include/star_amd_cli.h) ----

class CliHooks(C.Structure):
    _fields_ = [("user", C.c_void_p), ("warmup_done", C.CFUNCTYPE(None, C.c_void_p)), ("exchange", C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int))]


class CliReport(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("wallMapping", C.c_double), ("timedReads", C.c_uint64), ("timedWall", C.c_double),
                ("genomeLoadSeconds", C.c_double), ("indexUploadSeconds", C.c_double), ("nDevices", C.c_int),
                ("deviceBusy", C.c_double * 16), ("deviceMs", C.c_double * 16), ("stageMs", C.c_double * 8), ("counters", C.c_uint64 * 64),
                ("parseBusy", C.c_double), ("emitBusy", C.c_double), ("batches", C.c_uint64), ("pass1Seconds", C.c_double), ("finishSeconds", C.c_double), ("nContexts", C.c_int), ("convertBusy", C.c_double), ("emitParts", C.c_double * 4), ("fastPaths", C.c_uint64 * 4), ("cpuSeconds", C.c_double * 8)]


def run_cli(argv, warmup_done=None, exchange=None, lib_path=None):
    """The whole front end (star_amd/csrc/host/cli_run.cpp) in this process: argv as on the command line; warmup_done() is called when the
    --benchWarmupReads reads are written and the pipeline is empty; exchange(handle, last) at the end of every mapping phase (cross-rank tables).
    Returns (exit code, CliReport)."""
    lib = C.CDLL(lib_path or os.environ.get("STARAMD_CLI_LIB") or _need(os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libstaramd_cli.so")))      # (STARAMD_CLI_LIB: tests of bench.py's plumbing on a box without a GPU)
    lib.staramd_cli_main.restype = C.c_int
    lib.staramd_cli_main.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(CliHooks), C.POINTER(CliReport)]
    args = [b"star_amd"] + [a.encode() for a in argv]
    arr = (C.c_char_p * len(args))(*args)
    hooks = CliHooks()
    WD, EX = CliHooks._fields_[1][1], CliHooks._fields_[2][1]
    wd = WD(lambda u: warmup_done() if warmup_done else None)
    ex = EX(lambda u, h, last: int(exchange(h, last) or 0) if exchange else 0)
    hooks.user = None; hooks.warmup_done = wd; hooks.exchange = ex
    rep = CliReport()
    rc = lib.staramd_cli_main(len(args), arr, C.byref(hooks), C.byref(rep))
    return rc, rep


