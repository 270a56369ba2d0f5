"""One CALL SEQUENCE on an engine context, every result it hands out compared byte for byte with the oracle for the same (index, tables, params, batch).
The results of a batch must depend on those alone, never on what the context did before: an overflow whose results stay resident, a map_begin / map_end
pair, map_resident, new tables / index / whitelist, an owner's update seen by a sharer, grown pools, a prefetched upload.
Test infrastructure (tests/test_engine_call_history.py); a fresh process per scenario, the engine library from STARAMD_ENGINE_LIB (the real one, or the
wavefront emulator's oracle/_build/libstaramd_emul.so).
Usage: python tests/history_run.py <prepared info.pkl> <workdir> <scenario 1..13> <reads per batch> [batch sizes of scenario 12...]      prints OK or the first difference"""
import ctypes as C
import os
import pickle
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from util import capi, oracle_lib  # noqa: E402

OVERFLOW = -3           # STARAMD_ERR_RESULT_OVERFLOW
ST_CHIM_PARTNER = 0x0800


class Fail(Exception):
    pass


def check(cond, what):
    if not cond:
        raise Fail(what)


class OwnBatch:
    """A batch in arrays of its own (the host library reuses its arrays from one next_batch to the next): reads = [(bases, mate1Length, mmMaxTotal)].
    lead: bytes in front of the first read.  view(k): the same arrays from read k on (readOffset[0] > 0: a slice, as the pieces of a WASP batch)."""

    def __init__(self, reads, lead=0):
        self.reads = list(reads)
        n = len(self.reads)
        offs = [lead]
        for r in self.reads:
            offs.append(offs[-1] + len(r[0]))
        self.bases = (C.c_uint8 * max(1, offs[-1]))()
        for r, o in zip(self.reads, offs):
            C.memmove(C.addressof(self.bases) + o, r[0], len(r[0]))
        self.offs = (C.c_uint64 * (n + 1))(*offs)
        self.m1 = (C.c_uint16 * max(1, n))(*[r[1] for r in self.reads])
        self.mm = (C.c_uint16 * max(1, n))(*[r[2] for r in self.reads])
        self.b = self.view(0)

    def view(self, k):
        v = capi.Batch()
        v.nReads = len(self.reads) - k
        v.bases = C.cast(self.bases, capi.u8p)
        v.readOffset = C.cast(C.addressof(self.offs) + 8 * k, capi.u64p)
        v.mate1Length = C.cast(C.addressof(self.m1) + 2 * k, capi.u16p)
        v.mmMaxTotal = C.cast(C.addressof(self.mm) + 2 * k, capi.u16p)
        return v

    def refill(self, other):
        """the arrays of this batch overwritten in place with another batch of the same geometry"""
        check(len(other.reads) == len(self.reads) and list(other.offs) == list(self.offs), "refill: different geometry")
        C.memmove(self.bases, other.bases, C.sizeof(self.bases)); C.memmove(self.m1, other.m1, C.sizeof(self.m1)); C.memmove(self.mm, other.mm, C.sizeof(self.mm))
        self.reads = list(other.reads)

    def n_bases(self):
        return self.offs[len(self.reads)] - self.offs[0]


def load_reads(run, limit):
    """the first `limit` reads of the run, each copied out"""
    out = []
    while len(out) < limit:
        b = run.next_batch(min(4096, limit - len(out)))
        if b is None:
            break
        for i in range(b.nReads):
            lo, hi = b.readOffset[i], b.readOffset[i + 1]
            out.append((C.string_at(C.addressof(b.bases.contents) + lo, hi - lo), b.mate1Length[i], b.mmMaxTotal[i]))
    return out


def first_difference(got, want, n):
    g, w = got.res, want.res
    for i in range(n):
        a, o = got.reads[i], want.reads[i]
        fa = (a.status, a.nW, a.nTr, a.trOffset, a.trBest, a.maxScoreMate[0], a.maxScoreMate[1], a.unmappedLength)
        fo = (o.status, o.nW, o.nTr, o.trOffset, o.trBest, o.maxScoreMate[0], o.maxScoreMate[1], o.unmappedLength)
        if fa != fo:
            return "read %d: engine (status, nW, nTr, trOffset, trBest, maxScoreMate, unmappedLength) %r, oracle %r" % (i, fa, fo)
    if g.trCount != w.trCount or g.exCount != w.exCount:
        return "transcript / exon counts: engine %d / %d, oracle %d / %d" % (g.trCount, g.exCount, w.trCount, w.exCount)
    rg, tg, eg = got.as_bytes(n); ro, to, eo = want.as_bytes(n)
    for name, x, y, size in (("transcript", tg, to, C.sizeof(capi.Transcript)), ("exon", eg, eo, C.sizeof(capi.Exon))):
        if x != y:
            k = next(j for j in range(0, len(x), size) if x[j:j + size] != y[j:j + size]) // size
            rd = max(i for i in range(n) if got.reads[i].trOffset <= k) if name == "transcript" else None
            return "%s record %d differs%s" % (name, k, " (read %d)" % rd if rd is not None else "")
    return None


class Scenario:
    def __init__(self, info, wd, n):
        self.info, self.wd, self.n = info, wd, n
        self.select_all = False
        self.runs = []
        self.engines = []
        self.oracles = []

    def host_run(self, more=(), n_reads=None):
        argv = ["--genomeDir", self.info["idx"], "--readFilesIn"] + self.info["fastq"] + ["--outFileNamePrefix", os.path.join(self.wd, "h%d_" % len(self.runs))] + \
               list(self.info["extra"]) + list(more)
        if n_reads:
            argv += ["--readMapNumber", str(n_reads)]
        r = capi.HostRun(argv)
        self.runs.append(r)
        return r

    def engine(self, run=None, params_p=None, max_reads=None, max_bases=None, share_with=None):
        run = run or self.runs[0]
        e = capi.Engine(run.genome, params_p if params_p is not None else run.params, device=0, max_reads=max_reads or max(64, self.n), max_bases=max_bases, share_with=share_with)
        self.engines.append(e)
        return e

    def oracle(self, run=None, params_p=None):
        run = run or self.runs[0]
        o = oracle_lib.Oracle(run.genome, params_p if params_p is not None else run.params)
        self.oracles.append(o)
        return o

    def room(self, n):
        return capi.ResultBuffers(n, tr_cap=n * (400 if self.select_all else 64))

    def want(self, orc, batch):
        n = batch.nReads if isinstance(batch, capi.Batch) else batch.b.nReads
        bo = self.room(n)
        orc.map_batch(batch if isinstance(batch, capi.Batch) else batch.b, bo)
        return bo

    def expect(self, step, got, want, n):
        d = first_difference(got, want, n)
        if d:
            raise Fail("%s: %s" % (step, d))

    def overflow(self, eng, batch, want, step):
        """the batch mapped into result arrays that are too small: STARAMD_ERR_RESULT_OVERFLOW with the sizes it needs"""
        small = capi.ResultBuffers(batch.nReads, tr_cap=1, ex_cap=1)
        rc = eng.map_batch_rc(batch, small)
        check(rc == OVERFLOW, "%s: staramd_map_batch returned %d, expected the overflow %d" % (step, rc, OVERFLOW))
        check((small.res.trCount, small.res.exCount) == (want.res.trCount, want.res.exCount),
              "%s: the overflow reports %d / %d records, the batch has %d / %d" % (step, small.res.trCount, small.res.exCount, want.res.trCount, want.res.exCount))

    def map(self, eng, batch, step):
        got = self.room(batch.nReads)
        rc = eng.map_batch_rc(batch, got)
        check(rc == 0, "%s: staramd_map_batch returned %d (%s)" % (step, rc, eng.L.staramd_last_error().decode()))
        return got

    def close(self):
        for x in self.engines[::-1] + self.oracles + self.runs:
            x.close()


def batches(pool, n, k):
    """k different batches of n reads each from the pool (from its start again where it ends)"""
    check(len(pool) > n, "the data set has %d reads, batches of %d wanted" % (len(pool), n))
    return [OwnBatch([pool[j % len(pool)] for j in range(i * n, (i + 1) * n)]) for i in range(k)]


def novel_junctions(bufs, n):
    """(start, end) of every unannotated junction in the returned transcripts (first / last intron base, as staramd_set_novel_junctions takes them)"""
    out = set()
    for i in range(n):
        r = bufs.reads[i]
        for t in range(r.trOffset, r.trOffset + r.nTr):
            tr = bufs.tr[t]
            for e in range(tr.exonOffset, tr.exonOffset + tr.nExons - 1):
                ex, nx = bufs.ex[e], bufs.ex[e + 1]
                if ex.canonSJ >= 0 and ex.sjAnnot == 0:
                    out.add((ex.G + ex.L, nx.G - 1))
    return sorted(out)


# ---- the scenarios (tests/test_engine_call_history.py has the table) -------------------------------------------------------------------------------------

def s1_overflow_then_retry(S, pool):
    run = S.host_run(); eng = S.engine(); orc = S.oracle()
    A, = batches(pool, S.n, 1)
    wA = S.want(orc, A)
    S.overflow(eng, A.b, wA, "overflow(A)")
    l0 = eng.launch_count()
    S.expect("retry(A)", S.map(eng, A.b, "retry(A)"), wA, S.n)
    check(eng.launch_count() == l0, "retry(A): the batch was mapped again (launches %d -> %d)" % (l0, eng.launch_count()))


def s2_map_begin_between(S, pool):
    run = S.host_run(); eng = S.engine(); orc = S.oracle()
    A, B = batches(pool, S.n, 2)
    wA, wB = S.want(orc, A), S.want(orc, B)
    S.overflow(eng, A.b, wA, "overflow(A)")
    eng.map_begin(B.b)
    rB = S.room(S.n); eng.map_end(rB)
    S.expect("map_end(B)", rB, wB, S.n)
    S.expect("retry(A) after map_begin(B) / map_end(B)", S.map(eng, A.b, "retry(A)"), wA, S.n)


def s3_map_resident_between(S, pool):
    run = S.host_run(); eng = S.engine(); orc = S.oracle()
    A, = batches(pool, S.n, 1)
    wA = S.want(orc, A)
    S.overflow(eng, A.b, wA, "overflow(A)")
    rR = S.room(S.n); eng.map_resident(rR)
    S.expect("map_resident", rR, wA, S.n)
    l0 = eng.launch_count()
    S.expect("retry(A) after map_resident", S.map(eng, A.b, "retry(A)"), wA, S.n)
    check(eng.launch_count() == l0 + 1, "retry(A) after map_resident: answered from the results of an earlier call (launches %d -> %d)" % (l0, eng.launch_count()))


GAP = ["--scoreGap", "-3"]          # changes scores, not the batch arrays


def s4_update_tables_between(S, pool):
    run = S.host_run(); run2 = S.host_run(GAP)
    eng = S.engine(); orc = S.oracle(); orc2 = S.oracle(run2)
    A, = batches(pool, S.n, 1)
    wA, wA2 = S.want(orc, A), S.want(orc2, A)
    check(first_difference(wA2, wA, S.n) is not None, "%s changes nothing in this batch: the scenario shows nothing" % GAP)
    S.overflow(eng, A.b, wA, "overflow(A)")
    eng.update_tables(run2.genome, run2.params)
    S.expect("retry(A) after update_tables(%s)" % " ".join(GAP), S.map(eng, A.b, "retry(A)"), wA2, S.n)


def s5_novel_junctions_between(S, pool):
    run = S.host_run(["--outFilterType", "BySJout"])
    check(run.params.contents.outFilterBySJoutStage == 1, "--outFilterType BySJout: the parameters are not at stage 1")
    eng = S.engine(); orc = S.oracle(); orc2 = S.oracle()
    A, = batches(pool, S.n, 1)
    wA = S.want(orc, A)
    sj = novel_junctions(wA, S.n)
    keep = sj[::2]                                   # every other novel junction of the batch passes the 2nd stage
    start = (C.c_uint64 * max(1, len(keep)))(*[s for s, e in keep]); end = (C.c_uint64 * max(1, len(keep)))(*[e for s, e in keep])
    orc2.set_novel_junctions(start, end, len(keep), 2)
    wA2 = S.want(orc2, A)
    check(first_difference(wA2, wA, S.n) is not None, "the whitelist (%d of %d novel junctions) changes nothing in this batch" % (len(keep), len(sj)))
    S.overflow(eng, A.b, wA, "overflow(A) at BySJout stage 1")
    eng.set_novel_junctions(start, end, len(keep), 2)
    S.expect("retry(A) after set_novel_junctions(stage 2)", S.map(eng, A.b, "retry(A)"), wA2, S.n)


def s6_update_index_between(S, pool):
    run = S.host_run(); eng = S.engine(); orc = S.oracle()
    A, = batches(pool, S.n, 1)
    wA = S.want(orc, A)
    S.overflow(eng, A.b, wA, "overflow(A)")
    eng.update_index(run.genome, run.params)
    l0 = eng.launch_count()
    S.expect("retry(A) after update_index", S.map(eng, A.b, "retry(A)"), wA, S.n)
    check(eng.launch_count() == l0 + 1, "retry(A) after update_index: answered from the results mapped on the old index (launches %d -> %d)" % (l0, eng.launch_count()))


def s7_batch_edited_in_place(S, pool):
    run = S.host_run(); eng = S.engine(); orc = S.oracle()
    A, = batches(pool, S.n, 1)
    n, mid = S.n, S.n // 2

    def edit_mm():
        for i in (1, mid, n - 2):
            A.mm[i] = 0

    def edit_base():
        o = A.offs[mid] + 17
        A.bases[o] = (A.bases[o] + 1) % 4 if A.bases[o] < 4 else 0

    def edit_mate1():
        A.m1[mid] = A.m1[mid] - 1                     # (within the read: only the mate lengths the thresholds use change)

    for name, edit in (("mmMaxTotal", edit_mm), ("a base of a middle read", edit_base), ("mate1Length", edit_mate1)):
        wA = S.want(orc, A)
        S.overflow(eng, A.b, wA, "overflow(A) before editing %s" % name)
        edit()
        wE = S.want(orc, A)
        l0 = eng.launch_count()
        S.expect("retry(A) after editing %s in place" % name, S.map(eng, A.b, "retry(A)"), wE, n)
        check(eng.launch_count() == l0 + 1, "retry(A) after editing %s in place: answered from the results of the batch before the edit" % name)


def s8_sharer_follows_owner(S, pool):
    run = S.host_run(); run2 = S.host_run(GAP)
    owner = S.engine(); sharer = S.engine(share_with=owner)
    orc = S.oracle(); orc2 = S.oracle(run2)
    A, = batches(pool, S.n, 1)
    wA, wA2 = S.want(orc, A), S.want(orc2, A)
    check(first_difference(wA2, wA, S.n) is not None, "%s changes nothing in this batch" % GAP)
    S.overflow(sharer, A.b, wA, "sharer: overflow(A)")
    owner.update_tables(run2.genome, run2.params)
    S.expect("sharer: retry(A) after the owner's update_tables(%s)" % " ".join(GAP), S.map(sharer, A.b, "retry(A)"), wA2, S.n)
    S.expect("owner: A under the new tables", S.map(owner, A.b, "owner: map(A)"), wA2, S.n)


TINY_POOLS = {"STARAMD_POOL_SLACK": "64", "STARAMD_SEEDS_PER_READ": "1", "STARAMD_WINDOWS_PER_READ": "1", "STARAMD_WA_PER_READ": "1", "STARAMD_TR_PER_READ": "1"}


def s9_grown_pools(S, pool):
    os.environ.update(TINY_POOLS)                    # (read by staramd_create: every pool starts at a few records and grows)
    S.select_all = True
    run = S.host_run(["--gpuResultSelect", "All"]); orc = S.oracle()
    H, = batches(pool, S.n, 1)
    L = OwnBatch([pool[j % len(pool)] for j in range(S.n, S.n + max(2, S.n // 16))])
    wH, wL = S.want(orc, H), S.want(orc, L)
    for order in ((H, wH, "heavy"), (L, wL, "light")), ((L, wL, "light"), (H, wH, "heavy")):
        eng = S.engine()
        for k, (X, wX, name) in enumerate(order):
            l0 = eng.launch_count()
            S.expect("%s batch %s" % (name, "first" if k == 0 else "after the %s one" % order[0][2]), S.map(eng, X.b, name), wX, X.b.nReads)
            if k == 0 and name == "heavy":
                check(eng.launch_count() > l0 + 1, "the heavy batch did not grow a pool (launches %d -> %d): the scenario shows nothing" % (l0, eng.launch_count()))


def s10_prefetch(S, pool):
    run = S.host_run(); eng = S.engine(); orc = S.oracle()
    B, Cb, D = batches(pool, S.n, 3)
    wB, wC, wD = S.want(orc, B), S.want(orc, Cb), S.want(orc, D)
    eng.prefetch(B.b)
    S.expect("map(C) with B prefetched", S.map(eng, Cb.b, "map(C)"), wC, S.n)
    h0 = eng.prefetch_hits()
    S.expect("map(B) after map(C)", S.map(eng, B.b, "map(B)"), wB, S.n)
    check(eng.prefetch_hits() == h0 + 1, "map(B): its prefetched upload was not used (hits %d -> %d)" % (h0, eng.prefetch_hits()))
    eng.prefetch(B.b)
    eng.prefetch_cancel()
    B.refill(D)
    h1 = eng.prefetch_hits()
    S.expect("map(D) in the arrays of a cancelled prefetch of B", S.map(eng, B.b, "map(D)"), wD, S.n)
    check(eng.prefetch_hits() == h1, "map(D): took the cancelled upload of B")


def s11_begin_end(S, pool):
    run = S.host_run(); eng = S.engine(); orc = S.oracle()
    A, B = batches(pool, S.n, 2)
    wA, wB = S.want(orc, A), S.want(orc, B)
    eng.map_begin(A.b)
    rA, rB = S.room(S.n), S.room(S.n)
    o0 = eng.overlapped_batches()
    eng.map_end(rA, B.b)
    check(eng.overlapped_batches() == o0 + 1, "map_end(A, next=B): B was not begun beside the copy of A's results (overlapped %d -> %d)" % (o0, eng.overlapped_batches()))
    eng.map_end(rB)
    S.expect("map_end(A, next=B)", rA, wA, S.n)
    S.expect("map_end(B)", rB, wB, S.n)
    eng.map_begin(A.b)
    small = capi.ResultBuffers(S.n, tr_cap=1, ex_cap=1)
    rc = eng.map_end_rc(small)
    check(rc == OVERFLOW and (small.res.trCount, small.res.exCount) == (wA.res.trCount, wA.res.exCount), "map_end(A) into arrays too small: %d, %d / %d records" % (rc, small.res.trCount, small.res.exCount))
    rA2 = S.room(S.n); eng.map_end(rA2)
    S.expect("map_end(A) again with room", rA2, wA, S.n)
    S.expect("map_batch(A) after it", S.map(eng, A.b, "map(A)"), wA, S.n)


def s12_geometry(S, pool, sizes):
    run = S.host_run()
    top = max(sizes)
    tiled = [pool[i % len(pool)] for i in range(top)]          # (a data set smaller than the largest batch: its reads again)
    big = OwnBatch(tiled)
    eng = S.engine(max_reads=top, max_bases=big.n_bases())     # the largest batch fills the context exactly: maxBatchReads reads, maxBatchBases bases
    orc = S.oracle()
    at = 0
    for k in sizes:
        X = OwnBatch([tiled[(at + i) % top] for i in range(k)]); at += k
        check(k < top or X.n_bases() == big.n_bases(), "the largest batch does not fill maxBatchBases")
        S.expect("%d reads" % k, S.map(eng, X.b, "%d reads" % k), S.want(orc, X), k)
    # a slice: readOffset[0] > 0 at an odd base offset (the pieces of a WASP re-mapping batch)
    sl = OwnBatch(tiled, lead=0 if len(tiled[0][0]) % 2 else 1)
    v = sl.view(1)
    check(v.readOffset[0] % 2 == 1, "the slice does not start at an odd base offset")
    S.expect("slice of %d reads from base %d" % (v.nReads, v.readOffset[0]), S.map(eng, v, "slice"), S.want(orc, v), v.nReads)


def s13_pass1_params(S, pool):
    run = S.host_run()
    A, = batches(pool, S.n, 1)
    for csm, csmp in ((12, 0), (0, 1)):
        p = capi.Params.from_buffer_copy(run.params.contents)
        p.resultSelect = 2; p.chimSegmentMin = csm; p.chimSegmentMinPositive = csmp      # (the 1st pass of a 2-pass chimeric run: runner.cpp sets chimSegmentMinPositive 0, resultSelect stays 2)
        q = capi.Params.from_buffer_copy(p); q.resultSelect = 1
        eng = S.engine(params_p=C.pointer(p)); orc = S.oracle(params_p=C.pointer(q))
        wA = S.want(orc, A)
        got = S.map(eng, A.b, "map(A)")
        step = "resultSelect 2, chimSegmentMin %d, chimSegmentMinPositive %d" % (csm, csmp)
        partners = [i for i in range(S.n) if got.reads[i].status & ST_CHIM_PARTNER]
        check(not partners, "%s: reads %r have STARAMD_ST_CHIM_PARTNER" % (step, partners[:8]))
        S.expect(step + " (oracle under resultSelect 1)", got, wA, S.n)


SCENARIOS = {1: s1_overflow_then_retry, 2: s2_map_begin_between, 3: s3_map_resident_between, 4: s4_update_tables_between, 5: s5_novel_junctions_between,
             6: s6_update_index_between, 7: s7_batch_edited_in_place, 8: s8_sharer_follows_owner, 9: s9_grown_pools, 10: s10_prefetch, 11: s11_begin_end,
             12: s12_geometry, 13: s13_pass1_params}


def main():
    pkl, wd, k, n = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
    sizes = [int(x) for x in sys.argv[5:]]
    info = pickle.load(open(pkl, "rb"))
    S = Scenario(info, wd, n)
    t0 = time.time()
    try:
        r = S.host_run()                          # the reads of the data set, copied out once
        pool = load_reads(r, max([n * 3 + n // 16 + 2] + sizes))
        r.close(); S.runs.clear()
        if k == 12:
            s12_geometry(S, pool, sizes)
        else:
            SCENARIOS[k](S, pool)
        print("OK scenario %d, %.1f s" % (k, time.time() - t0))
    except Fail as e:
        print("DIFF scenario %d (%s): %s" % (k, SCENARIOS[k].__name__, e))
    finally:
        S.close()


main()
