"""The BGZF files that the tests of k_inflate.hip share (tests/test_inflate_emul.py on the wave emulator, tests/test_inflate_bounds.py under the sanitizers,
tests/test_gpu_inflate.py on the MI355X): made here from a bit writer and from real writers, never by the code under test.

    wellformed()   name -> (file bytes, [the data of every member])        every member is held to zlib.decompressobj(-15) and zlib.crc32 by check_wellformed()
    malformed()    name -> (file bytes, failing member, status name)       a BAM header member, the bad member, a good member, the EOF marker
    lenient()      name -> (file bytes, failing member, status name)       files the device rejects and gzread accepts (it never looks at BSIZE, and takes a
                                                                            file that ends early for a file that ends)
    reach(files)   what a set of files gets to: block types, blocks per member, lengths, distances, overlapping copies (a small inflate of its own)
"""
import random
import struct
import zlib

import deflate_inspect as DI

EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
IN_MAX = 0xff00
# a complete code-length code over all 19 symbols: 13 codes of 4 bits, 6 of 5
CL_DEFAULT = [4] * 13 + [5] * 6


class BitW:
    """LSB-first bit writer (RFC 1951 3.1.1); Huffman codes go in most significant bit first"""

    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v, n):
        assert 0 <= v < (1 << n) or n == 0
        self.acc |= v << self.n
        self.n += n

    def code(self, code, length):
        for i in range(length - 1, -1, -1):
            self.put((code >> i) & 1, 1)

    def align(self):
        self.n = (self.n + 7) // 8 * 8

    def raw(self, data):
        assert self.n % 8 == 0
        for b in data:
            self.put(b, 8)

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def stored(bw, data, final, nlen=None):
    bw.put(final, 1); bw.put(0, 2); bw.align()
    bw.put(len(data), 16); bw.put((len(data) ^ 0xffff) if nlen is None else nlen, 16)
    bw.raw(data)


def tokens(bw, toks, lit_lens, dist_lens, eob=True):
    """toks: int = a literal, (length, distance) = a match, ("L", symbol) / ("D", symbol) = that symbol of the literal/length / distance code as it is"""
    lc, dc = DI.canonical_codes(lit_lens), DI.canonical_codes(dist_lens)
    for t in toks:
        if isinstance(t, int):
            bw.code(*lc[t])
        elif t[0] == "L":
            bw.code(*lc[t[1]])
        elif t[0] == "D":
            bw.code(*dc[t[1]])
        else:
            s, eb, ev = DI.len_symbol(t[0])
            bw.code(*lc[s]); bw.put(ev, eb)
            s, eb, ev = DI.dist_symbol(t[1])
            bw.code(*dc[s]); bw.put(ev, eb)
    if eob:
        bw.code(*lc[256])


FIXED_DIST32 = [5] * 32


def fixed(bw, toks, final, eob=True):
    bw.put(final, 1); bw.put(1, 2)
    tokens(bw, toks, DI.FIXED_LIT, FIXED_DIST32, eob)


def dyn_header(bw, final, lit_lens, dist_lens, cl_syms=None, cl_lens=CL_DEFAULT, hclen=19, hlit=None, hdist=None):
    """cl_syms: [(code-length symbol, extra value or None)], default one symbol per length"""
    hlit = len(lit_lens) if hlit is None else hlit
    hdist = len(dist_lens) if hdist is None else hdist
    bw.put(final, 1); bw.put(2, 2); bw.put(hlit - 257, 5); bw.put(hdist - 1, 5); bw.put(hclen - 4, 4)
    for i in range(hclen):
        bw.put(cl_lens[DI.CL_ORDER[i]], 3)
    cc = DI.canonical_codes(cl_lens)
    for s, extra in (cl_syms if cl_syms is not None else [(l, None) for l in list(lit_lens) + list(dist_lens)]):
        bw.code(*cc[s])
        if s >= 16:
            bw.put(extra, {16: 2, 17: 3, 18: 7}[s])


def dynamic(bw, toks, final, lit_lens, dist_lens, eob=True, **kw):
    dyn_header(bw, final, lit_lens, dist_lens, **kw)
    tokens(bw, toks, lit_lens, dist_lens, eob)


def complete_lens(n_symbols, used):
    """code lengths over n_symbols that make a complete code of the symbols in `used` (at least two), as flat as possible"""
    used = sorted(used)
    assert len(used) >= 2
    k = max(1, (len(used) - 1).bit_length())
    short = (1 << k) - len(used)
    lens = [0] * n_symbols
    for i, s in enumerate(used):
        lens[s] = k - 1 if i < short else k
    assert DI.kraft(lens) == 1 << 15
    return lens


def member(deflate, data=None, crc=None, isize=None, extra_before=b"", extra_after=b"", bsize=None):
    """one BGZF member around a raw deflate stream; crc / isize / bsize override what the data says"""
    extra = extra_before + b"BC" + struct.pack("<H", 2) + b"\0\0" + extra_after
    total = 12 + len(extra) + len(deflate) + 8
    assert total <= 65536, total
    extra = extra_before + b"BC" + struct.pack("<HH", 2, (total - 1) if bsize is None else bsize) + extra_after
    crc = zlib.crc32(data) if crc is None else crc
    isize = len(data) if isize is None else isize
    return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", len(extra)) + extra + deflate + struct.pack("<II", crc & 0xffffffff, isize)


def zmember(data, level=6, flush_at=None, **kw):
    z = zlib.compressobj(level, zlib.DEFLATED, -15)
    if flush_at is None:
        d = z.compress(data) + z.flush()
    else:
        d = z.compress(data[:flush_at]) + z.flush(zlib.Z_FULL_FLUSH) + z.compress(data[flush_at:]) + z.flush()
    return member(d, data, **kw)


def record_stream(n_bytes, seed, whole=False):
    """BAM records (the builders of tests/test_dedup_emul.py) side by side, cut to n_bytes -- or, whole: the records that fit into n_bytes, each entire"""
    import test_dedup_emul as D
    r = random.Random(seed)
    out = bytearray()
    i = 0
    while len(out) < n_bytes:
        p = r.randrange(100, 150000)
        for rec in D.pair(b"read%d_%d" % (seed, i), r.randrange(3), p, p + r.randrange(300), as1=r.randrange(200)):
            if whole and len(out) + len(rec) > n_bytes:
                return bytes(out)
            out += rec
        i += 1
    return bytes(out[:n_bytes])


# ---- well-formed ------------------------------------------------------------------------------------------------------------------------------------

def _by_hand():
    """name -> (deflate stream, data).  The data is what the stream was written to mean; check_wellformed() asks zlib"""
    v = {}
    rnd = random.Random(11)
    noise = bytes(rnd.randrange(256) for _ in range(40000))
    bw = BitW(); stored(bw, b"", 1); v["stored_0"] = (bw.bytes(), b"")
    big = (noise * 2)[:65536 - 26 - 5]                      # the largest stored block a BGZF member holds: BSIZE has 16 bits, so 65 535 bytes do not fit
    bw = BitW(); stored(bw, big, 1); v["stored_max"] = (bw.bytes(), big)
    bw = BitW(); fixed(bw, [ord("A")], 1); v["one_byte"] = (bw.bytes(), b"A")
    bw = BitW(); fixed(bw, [1, 2, 3, (258, 3), 9], 1); v["fixed_len258"] = (bw.bytes(), bytes([1, 2, 3] * 87 + [9]))
    bw = BitW(); fixed(bw, [1, 2, 3, (3, 3), 9], 1); v["fixed_len3"] = (bw.bytes(), bytes([1, 2, 3, 1, 2, 3, 9]))
    bw = BitW(); fixed(bw, [7, (258, 1), (258, 1), (70, 1)], 1); v["run_dist1"] = (bw.bytes(), bytes([7] * (1 + 258 + 258 + 70)))
    bw = BitW(); fixed(bw, [ord(c) for c in "abcde"] + [(5, 5), (9, 10)], 1); v["dist_equals_produced"] = (bw.bytes(), b"abcdeabcde" + b"abcdeabcd")
    # 32768 bytes in a stored block, then matches at the largest distance; the second overlaps nothing, the third copies what the first two wrote
    far = noise[:32768]
    bw = BitW(); stored(bw, far, 0); fixed(bw, [(10, 32768), (258, 32768), (100, 268)], 1)
    d = bytearray(far)
    for L, D in ((10, 32768), (258, 32768), (100, 268)):
        for _ in range(L):
            d.append(d[-D])
    v["dist_32768"] = (bw.bytes(), bytes(d))
    # three blocks of three kinds in one member, the stored one empty and not byte-aligned
    lit = complete_lens(257, [65, 66, 256])
    bw = BitW(); fixed(bw, [65, 66], 0); stored(bw, b"", 0); dynamic(bw, [65, 66, 66], 1, lit, [0]); v["three_blocks"] = (bw.bytes(), b"ABABB")
    # HLIT 257: no length code at all, no distance code (HDIST 1, its one length 0)
    lit = complete_lens(257, [0, 255, 256])
    bw = BitW(); dynamic(bw, [0, 255, 255, 0], 1, lit, [0]); v["dyn_hlit257_no_dist"] = (bw.bytes(), bytes([0, 255, 255, 0]))
    # HLIT 286 with a code for symbol 285, and a single distance code of one bit
    lit = complete_lens(286, [97, 256, 260, 285])
    bw = BitW(); dynamic(bw, [97, (258, 1), (6, 1)], 1, lit, [1]); v["dyn_hlit286_one_dist"] = (bw.bytes(), b"a" * 265)
    # a 15-bit code: lengths 1, 2, ... 14, 15, 15 over sixteen symbols, the two longest used
    syms = [256] + list(range(40, 55))
    lit = [0] * 257
    for i, s in enumerate(syms):
        lit[s] = min(i + 1, 15)
    assert DI.kraft(lit) == 1 << 15
    bw = BitW(); dynamic(bw, [54, 53, 40, 54], 1, lit, [0]); v["dyn_15_bits"] = (bw.bytes(), bytes([54, 53, 40, 54]))
    # a run of 138 zeros, and a `16` whose run starts in the literal/length lengths and ends in the distance lengths
    lit = [0] * 260
    lit[0] = 2; lit[200] = 2; lit[256] = 3; lit[257] = 3; lit[258] = 3; lit[259] = 3       # 1/4 + 1/4 + 4/8 = 1
    dist = [3, 3, 3, 3, 3, 3, 3, 3]                                                          # 8/8 = 1
    # 2, 199 zeros (138 + 61), 2, 55 zeros, 3, then ten more 3s as runs of 6 and 5: the first covers symbols 257..259 and distance codes 0..2
    cl = [(2, None), (18, 127), (18, 50), (2, None), (18, 44), (3, None), (16, 3), (16, 2)]
    assert 1 + 138 + 61 + 1 + 55 + 1 + 6 + 5 == 268
    bw = BitW(); dynamic(bw, [0, 200, 200, (4, 2), (3, 7), 0], 1, lit, dist, cl_syms=cl)
    v["dyn_runs"] = (bw.bytes(), bytes([0, 200, 200, 200, 200, 200, 200]) + bytes([0, 200, 200]) + bytes([0]))
    return v


_WELL = {}


def wellformed():
    if _WELL:
        return _WELL
    W = _WELL
    hand = _by_hand()
    for name, (d, data) in hand.items():
        W[name] = (member(d, data) + EOF_MARKER, [data, b""])
    recs = record_stream(3 * IN_MAX + 1234, 1)
    cuts = [recs[o:o + IN_MAX] for o in range(0, len(recs), IN_MAX)]
    for level in (0, 1, 6, 9):
        W["zlib_level%d" % level] = (b"".join(zmember(c, level) for c in cuts) + EOF_MARKER, cuts + [b""])
        W["zlib_level%d_full_flush" % level] = (b"".join(zmember(c, level, flush_at=len(c) // 2) for c in cuts) + EOF_MARKER, cuts + [b""])
    empty = member(bytes([3, 0]), b"")
    W["empty_start_middle_end"] = (empty + zmember(cuts[0][:500]) + empty + empty + zmember(cuts[1][:700]) + empty, [b"", cuts[0][:500], b"", b"", cuts[1][:700], b""])
    W["no_eof_marker"] = (zmember(cuts[0][:3000]), [cuts[0][:3000]])
    W["full_0xff00"] = (zmember(cuts[0]) + EOF_MARKER, [cuts[0], b""])
    big = record_stream(65536, 2)
    W["full_65536"] = (zmember(big) + EOF_MARKER, [big, b""])
    sub = b"XY" + struct.pack("<H", 3) + b"abc"
    W["extra_subfields"] = (zmember(cuts[0][:900], extra_before=sub) + zmember(cuts[0][900:2000], extra_after=sub) + zmember(cuts[0][2000:2100], extra_before=sub, extra_after=sub + sub)
                            + EOF_MARKER, [cuts[0][:900], cuts[0][900:2000], cuts[0][2000:2100], b""])
    W["trailing_bytes"] = (zmember(cuts[0][:100]) + EOF_MARKER + b"\0\0\0not a member", [cuts[0][:100], b""])
    return W


def members_of(file_bytes):
    """[(deflate stream, crc, isize)] by the BSIZE chain; stops where no gzip member begins"""
    out, p = [], 0
    while p + 18 <= len(file_bytes) and file_bytes[p:p + 2] == b"\x1f\x8b":
        xlen = struct.unpack_from("<H", file_bytes, p + 10)[0]
        x, bsize = 0, None
        while x + 4 <= xlen:
            si, slen = file_bytes[p + 12 + x:p + 14 + x], struct.unpack_from("<H", file_bytes, p + 14 + x)[0]
            if si == b"BC" and slen == 2:
                bsize = struct.unpack_from("<H", file_bytes, p + 16 + x)[0]
                break
            x += 4 + slen
        assert bsize is not None
        end = p + bsize + 1
        crc, isize = struct.unpack_from("<II", file_bytes, end - 8)
        out.append((file_bytes[p + 12 + xlen:end - 8], crc, isize))
        p = end
    return out


def check_wellformed(name, file_bytes, datas):
    """the expectation of a well-formed vector comes from zlib alone"""
    ms = members_of(file_bytes)
    assert len(ms) == len(datas), name
    for (d, crc, isize), data in zip(ms, datas):
        z = zlib.decompressobj(-15)
        got = z.decompress(d)
        assert z.eof and z.unused_data == b"" and got == data and zlib.crc32(got) == crc and len(got) == isize, name


# ---- malformed ----------------------------------------------------------------------------------------------------------------------------------

def bam_header_member():
    text = b"@HD\tVN:1.4\tSO:coordinate\n"
    refs = [(b"chrA", 200000), (b"chrB", 200000), (b"chrC", 50000)]
    h = b"BAM\1" + struct.pack("<I", len(text)) + text + struct.pack("<I", len(refs))
    for n, l in refs:
        h += struct.pack("<I", len(n) + 1) + n + b"\0" + struct.pack("<I", l)
    return zmember(h), h


def _bad_members():
    """name -> (member bytes, status name)"""
    B = {}
    F = lambda toks, **kw: _stream(lambda bw: fixed(bw, toks, 1, **kw))
    B["block_type_3"] = (member(bytes([7]), b""), "BLOCK_TYPE")
    bw = BitW(); stored(bw, b"hello", 1, nlen=5 ^ 0xfffe); B["stored_nlen"] = (member(bw.bytes(), b"hello"), "STORED_LEN")
    lit = [0] * 257; lit[0] = 1; lit[1] = 1; lit[256] = 1
    B["lit_oversubscribed"] = (member(_stream(lambda bw: dyn_header(bw, 1, lit, [0])) + b"\0", b""), "OVERSUBSCRIBED")
    lit = [0] * 257; lit[0] = 2; lit[256] = 2
    B["lit_incomplete"] = (member(_stream(lambda bw: dynamic(bw, [0], 1, lit, [0])), b"\0"), "INCOMPLETE")
    lit2 = complete_lens(258, [0, 256, 257])
    B["dist_incomplete"] = (member(_stream(lambda bw: dynamic(bw, [0], 1, lit2, [2, 2])), b"\0"), "INCOMPLETE")
    B["dist_oversubscribed"] = (member(_stream(lambda bw: dynamic(bw, [0], 1, lit2, [1, 1, 1])), b"\0"), "OVERSUBSCRIBED")
    cl_bad = [4] * 12 + [0] + [5] * 6                       # one code of four bits short of complete
    B["codelen_incomplete"] = (member(_stream(lambda bw: dynamic(bw, [0], 1, complete_lens(257, [0, 256]), [0], cl_lens=cl_bad)), b"\0"), "INCOMPLETE")
    cl_over = [4] * 14 + [5] * 5
    B["codelen_oversubscribed"] = (member(_stream(lambda bw: dyn_header(bw, 1, complete_lens(257, [0, 256]), [0], cl_lens=cl_over)) + b"\0", b""), "OVERSUBSCRIBED")
    lit = [0] * 257; lit[0] = 1; lit[1] = 1
    B["no_end_code"] = (member(_stream(lambda bw: dyn_header(bw, 1, lit, [0])) + b"\0", b""), "NO_END_CODE")
    B["repeat_first"] = (member(_stream(lambda bw: dyn_header(bw, 1, [0] * 257, [0], cl_syms=[(16, 0)])) + b"\0\0", b""), "REPEAT")
    B["repeat_past_end"] = (member(_stream(lambda bw: dyn_header(bw, 1, [0] * 257, [0], cl_syms=[(1, None), (18, 127), (18, 127)])) + b"\0\0", b""), "REPEAT")
    B["lit_symbol_286"] = (member(F([65, ("L", 286)], eob=False) + b"\0", b"A"), "SYMBOL")
    B["lit_symbol_287"] = (member(F([65, ("L", 287)], eob=False) + b"\0", b"A"), "SYMBOL")
    B["dist_symbol_30"] = (member(F([65, ("L", 257), ("D", 30)], eob=False) + b"\0", b"A"), "SYMBOL")
    B["dist_symbol_31"] = (member(F([65, ("L", 257), ("D", 31)], eob=False) + b"\0", b"A"), "SYMBOL")
    B["unused_code"] = (member(_stream(lambda bw: (dyn_header(bw, 1, [0] * 256 + [1], [0]), bw.put(1, 1))) + b"\0", b""), "SYMBOL")      # one literal/length code, `0`; the stream sends `1`
    B["no_dist_code_used"] = (member(_stream(lambda bw: dynamic(bw, [0, ("L", 257)], 1, lit2, [0], eob=False)) + b"\0", b"\0"), "SYMBOL")
    B["distance_too_far"] = (member(F([65, (3, 2)]), b"AAAA"), "DISTANCE")
    # 3 header bits, the literal 'a', then five 1 bits of a nine-bit code and nothing more
    bw = BitW(); fixed(bw, [97], 1, eob=False); bw.put(31, 5); assert bw.n == 16
    B["ends_inside_symbol"] = (member(bw.bytes(), b"a"), "INPUT_END")
    bw = BitW(); stored(bw, b"0123456789", 1)
    B["stored_cut"] = (member(bw.bytes()[:-4], b"012345"), "INPUT_END")
    good = b"the same bytes " * 20
    z = zlib.compressobj(6, zlib.DEFLATED, -15); d = z.compress(good) + z.flush()
    B["wrong_crc"] = (member(d, good, crc=zlib.crc32(good) ^ 0x10), "CRC")
    B["isize_one_more"] = (member(d, good, isize=len(good) + 1), "OUTPUT_SHORT")
    B["isize_one_less"] = (member(d, good, isize=len(good) - 1), "OUTPUT_OVER")
    B["stray_byte"] = (member(d + b"\0", good), "STREAM_END")
    B["hlit_287"] = (member(_stream(lambda bw: dyn_header(bw, 1, [], [], cl_syms=[], hlit=287, hdist=1)) + b"\0\0", b""), "TOO_MANY")
    return B


def _stream(write):
    bw = BitW()
    write(bw)
    return bw.bytes()


_BAD = {}


def malformed():
    if not _BAD:
        head, _ = bam_header_member()
        good = zmember(record_stream(2000, 3, whole=True))
        for name, (m, status) in _bad_members().items():
            _BAD[name] = (head + m + good + EOF_MARKER, 1, status)
    return _BAD


def lenient():
    head, _ = bam_header_member()
    good = zmember(record_stream(2000, 3, whole=True))
    whole = head + good + good
    past = head + good + zmember(record_stream(2000, 4, whole=True), bsize=40000)
    return {"cut_inside_member": (whole[:-37], 2, "INPUT_END"), "cut_inside_header": (whole[:len(head) + len(good) + 7], 2, "INPUT_END"), "bsize_past_file": (past, 2, "INPUT_END")}


def not_bgzf():
    """gzip files that are no BGZF: (file bytes, a piece of the error text)"""
    import gzip
    data = record_stream(5000, 5)
    plain = gzip.compress(data)
    named = bytearray(zmember(data[:500])); named[3] |= 8
    other = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", 6) + b"XY" + struct.pack("<H", 2) + b"\0\0" + zmember(data[:500])[18:]
    return {"plain_gzip": (plain, "no extra field"), "with_name": (bytes(named), "a name"), "no_bc_subfield": (other, "no BC subfield"), "not_gzip": (b"BAM\1" + data, "does not begin with a gzip member")}


# ---- what a set of files reaches ------------------------------------------------------------------------------------------------------------------------

class _R:
    def __init__(self, raw):
        self.raw, self.pos = raw + b"\0" * 8, 0

    def get(self, n):
        v = (int.from_bytes(self.raw[self.pos >> 3:(self.pos >> 3) + 8], "little") >> (self.pos & 7)) & ((1 << n) - 1)
        self.pos += n
        return v

    def sym(self, table, maxl):
        v = (int.from_bytes(self.raw[self.pos >> 3:(self.pos >> 3) + 4], "little") >> (self.pos & 7)) & ((1 << maxl) - 1)
        s, l = table[v]
        self.pos += l
        return s


def _table(lengths):
    maxl = max(lengths) if any(lengths) else 1
    t = [None] * (1 << maxl)
    for s, (c, l) in DI.canonical_codes(lengths).items():
        r = int(format(c, "0%db" % l)[::-1], 2)
        for k in range(r, 1 << maxl, 1 << l):
            t[k] = (s, l)
    return t, maxl


def trace(deflate):
    """the classes a well-formed deflate stream reaches, by a plain inflate of its own (its output is not used: zlib gives the expectations)"""
    b, out, got, nblocks = _R(deflate), bytearray(), set(), 0
    while True:
        final, typ = b.get(1), b.get(2)
        nblocks += 1
        got.add(("stored", "fixed", "dynamic")[typ])
        if typ == 0:
            b.pos = (b.pos + 7) & ~7
            n = b.get(16); b.get(16)
            out += deflate[b.pos >> 3:(b.pos >> 3) + n]; b.pos += 8 * n
            if n == 0 and final == 0:
                got.add("stored_empty_inside")
        else:
            if typ == 1:
                ll, dl = list(DI.FIXED_LIT), list(FIXED_DIST32)
            else:
                hlit, hdist, hclen = b.get(5) + 257, b.get(5) + 1, b.get(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[DI.CL_ORDER[i]] = b.get(3)
                ct, cm = _table(cl)
                lens = []
                while len(lens) < hlit + hdist:
                    s = b.sym(ct, cm)
                    if s < 16:
                        lens.append(s)
                    else:
                        r = 3 + b.get(2) if s == 16 else 3 + b.get(3) if s == 17 else 11 + b.get(7)
                        if s == 16 and len(lens) < hlit < len(lens) + r:
                            got.add("repeat_crosses")
                        if s == 18 and r == 138:
                            got.add("run_138")
                        lens += [lens[-1] if s == 16 else 0] * r
                ll, dl = lens[:hlit], lens[hlit:]
                if hlit in (257, 286):
                    got.add("hlit_%d" % hlit)
                if max(ll) == 15:
                    got.add("code_15_bits")
                nd = sum(1 for x in dl if x)
                if nd < 2:
                    got.add("dist_codes_%d" % nd)
            lt, lm = _table(ll)
            dt, dm = _table(dl)
            while True:
                s = b.sym(lt, lm)
                if s < 256:
                    out.append(s)
                elif s == 256:
                    break
                else:
                    eb, base = DI.LEN_TABLE[s - 257]
                    L = base + b.get(eb)
                    eb, base = DI.DIST_TABLE[b.sym(dt, dm)]
                    D = base + b.get(eb)
                    if D == len(out):
                        got.add("dist_equals_produced")
                    if L in (3, 258):
                        got.add("len_%d" % L)
                    if D in (1, 32768):
                        got.add("dist_%d" % D)
                    if D < L:
                        got.add("overlap")
                    for _ in range(L):
                        out.append(out[-D])
        if final:
            break
    if nblocks > 1:
        got.add("several_blocks")
    return got


REACH_WANTED = {"stored", "fixed", "dynamic", "several_blocks", "stored_empty_inside", "len_258", "len_3", "dist_1", "dist_32768", "overlap", "dist_equals_produced", "hlit_257",
                "hlit_286", "dist_codes_0", "dist_codes_1", "code_15_bits", "run_138", "repeat_crosses"}


def reach(files):
    got = set()
    for f in files:
        for d, _, _ in members_of(f):
            got |= trace(d)
    return got
