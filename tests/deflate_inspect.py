"""A small inflate for ONE raw deflate block (RFC 1951) that keeps what zlib hides: the block type, HLIT / HDIST / HCLEN, the three code-length arrays,
the run-length symbols of the tree description, the tokens and the bits consumed -- and the arithmetic that judges an encoder by them: token
histograms, the Huffman optimum and depth of a histogram, the exact length-limited optimum (package-merge), the cost of the tokens under the fixed
code.  All tables are RFC 1951's, written out as data.  inflate_block() checks itself against zlib on every stream it reads, so no test can lean
on a stream it misreads.  Nothing here is shared with k_bgzf.hip."""
import heapq
import zlib

# RFC 1951 3.2.5: length symbols 257..285 -> (extra bits, first length); distance codes 0..29 -> (extra bits, first distance)
LEN_TABLE = [(0, 3), (0, 4), (0, 5), (0, 6), (0, 7), (0, 8), (0, 9), (0, 10), (1, 11), (1, 13), (1, 15), (1, 17), (2, 19), (2, 23), (2, 27), (2, 31),
             (3, 35), (3, 43), (3, 51), (3, 59), (4, 67), (4, 83), (4, 99), (4, 115), (5, 131), (5, 163), (5, 195), (5, 227), (0, 258)]
DIST_TABLE = [(0, 1), (0, 2), (0, 3), (0, 4), (1, 5), (1, 7), (2, 9), (2, 13), (3, 17), (3, 25), (4, 33), (4, 49), (5, 65), (5, 97), (6, 129), (6, 193),
              (7, 257), (7, 385), (8, 513), (8, 769), (9, 1025), (9, 1537), (10, 2049), (10, 3073), (11, 4097), (11, 6145), (12, 8193), (12, 12289),
              (13, 16385), (13, 24577)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]          # 3.2.7
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8                                  # 3.2.6, symbols 0..287
FIXED_DIST = [5] * 30
assert len(LEN_TABLE) == 29 and len(DIST_TABLE) == 30 and len(FIXED_LIT) == 288


def len_symbol(L):
    """length 3..258 -> (symbol, extra bit count, extra value).  Length 258 has a symbol of its own (285); 284 + 31 is never written for it."""
    assert 3 <= L <= 258
    if L == 258:
        return 285, 0, 0
    for i in range(27, -1, -1):
        eb, base = LEN_TABLE[i]
        if L >= base:
            assert L - base < (1 << eb)
            return 257 + i, eb, L - base
    raise AssertionError(L)


def dist_symbol(D):
    """distance 1..32768 -> (code, extra bit count, extra value)"""
    assert 1 <= D <= 32768
    for i in range(29, -1, -1):
        eb, base = DIST_TABLE[i]
        if D >= base:
            assert D - base < (1 << eb)
            return i, eb, D - base
    raise AssertionError(D)


def canonical_codes(lengths):
    """RFC 1951 3.2.2: {symbol: (code, length)} of the nonzero lengths, code as a number whose most significant bit is sent first"""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def kraft(lengths, maxbits=15):
    """sum of 2^(maxbits - len) over the nonzero lengths: 1 << maxbits for a complete code"""
    return sum(1 << (maxbits - l) for l in lengths if l)


class _Decoder:
    def __init__(self, lengths):
        self.maxl = max(lengths) if any(lengths) else 0
        self.table = [None] * (1 << self.maxl)
        assert kraft(lengths, 16) <= 1 << 16, "over-subscribed code"
        for s, (c, l) in canonical_codes(lengths).items():
            r = int(format(c, "0%db" % l)[::-1], 2)                     # the first bit sent is the lowest bit read
            for k in range(r, 1 << self.maxl, 1 << l):
                self.table[k] = (s, l)


class _Bits:
    def __init__(self, raw):
        self.raw, self.pos = bytes(raw) + b"\0" * 4, 0
        self.end = 8 * len(raw)

    def peek(self, n):
        i = self.pos >> 3
        return (int.from_bytes(self.raw[i:i + 4], "little") >> (self.pos & 7)) & ((1 << n) - 1)

    def get(self, n):
        v = self.peek(n)
        self.pos += n
        assert self.pos <= self.end, "read past the end of the stream"
        return v

    def sym(self, dec):
        e = dec.table[self.peek(dec.maxl)] if dec.maxl else None
        assert e is not None, "bits that are no code of an incomplete code"
        self.pos += e[1]
        assert self.pos <= self.end, "read past the end of the stream"
        return e[0]


class Block:
    """btype; n (bytes decoded); data; tokens: int literal or (length, distance); bits: consumed, the 3 header bits included; for BTYPE 2 also
    hlit / hdist / hclen, cl_lens[19], lit_lens[hlit], dist_lens[hdist], rle: [(code-length symbol, repeat count or None)], header_bits."""


def inflate_block(raw):
    """decode `raw`, which must be exactly one final deflate block padded to a byte; asserts agreement with zlib"""
    b, blk = _Bits(raw), Block()
    assert b.get(1) == 1, "BFINAL is not set: more than one block"
    blk.btype = b.get(2)
    assert blk.btype != 3
    out = bytearray()
    blk.tokens, blk.rle = [], []
    blk.hlit = blk.hdist = blk.hclen = None
    blk.cl_lens = blk.lit_lens = blk.dist_lens = None
    if blk.btype == 0:
        b.pos = (b.pos + 7) & ~7
        n, nn = b.get(16), b.get(16)
        assert n ^ nn == 0xffff
        out += raw[b.pos >> 3:(b.pos >> 3) + n]
        assert len(out) == n
        b.pos += 8 * n
        blk.tokens = list(out)
        blk.header_bits = 3
    else:
        if blk.btype == 1:
            blk.lit_lens, blk.dist_lens = list(FIXED_LIT), list(FIXED_DIST)
            blk.header_bits = 3
        else:
            blk.hlit, blk.hdist, blk.hclen = b.get(5) + 257, b.get(5) + 1, b.get(4) + 4
            assert blk.hlit <= 286 and blk.hdist <= 30
            blk.cl_lens = [0] * 19
            for i in range(blk.hclen):
                blk.cl_lens[CL_ORDER[i]] = b.get(3)
            cd, lens = _Decoder(blk.cl_lens), []
            while len(lens) < blk.hlit + blk.hdist:
                s = b.sym(cd)
                if s < 16:
                    lens.append(s); blk.rle.append((s, None))
                elif s == 16:
                    assert lens, "repeat with nothing before it"
                    r = 3 + b.get(2); lens += [lens[-1]] * r; blk.rle.append((16, r))
                elif s == 17:
                    r = 3 + b.get(3); lens += [0] * r; blk.rle.append((17, r))
                else:
                    r = 11 + b.get(7); lens += [0] * r; blk.rle.append((18, r))
            assert len(lens) == blk.hlit + blk.hdist, "a run crosses the end of the lengths"
            blk.lit_lens, blk.dist_lens = lens[:blk.hlit], lens[blk.hlit:]
            assert blk.lit_lens[256], "no code for the end of block"
            blk.header_bits = b.pos
        ld, dd = _Decoder(blk.lit_lens), _Decoder(blk.dist_lens)
        while True:
            s = b.sym(ld)
            if s < 256:
                out.append(s); blk.tokens.append(s)
            elif s == 256:
                break
            else:
                assert s <= 285
                eb, base = LEN_TABLE[s - 257]
                L = base + b.get(eb)
                ds = b.sym(dd)
                assert ds < 30
                eb, base = DIST_TABLE[ds]
                D = base + b.get(eb)
                assert D <= len(out), "distance before the start of the block"
                for _ in range(L):
                    out.append(out[-D])
                blk.tokens.append((L, D))
    blk.bits = b.pos
    assert (blk.bits + 7) // 8 == len(raw), "bytes after the block"
    assert blk.bits == b.end or b.peek(b.end - blk.bits) == 0, "padding bits are not zero"
    blk.data, blk.n = bytes(out), len(out)
    z = zlib.decompressobj(-15)
    assert z.decompress(bytes(raw)) == blk.data and z.eof and z.unused_data == b"", "the inspector and zlib read this stream differently"
    return blk


def histograms(tokens):
    """(literal/length frequencies[286], the end-of-block symbol counted once; distance frequencies[30])"""
    lit, dist = [0] * 286, [0] * 30
    for t in tokens:
        if isinstance(t, tuple):
            lit[len_symbol(t[0])[0]] += 1
            dist[dist_symbol(t[1])[0]] += 1
        else:
            lit[t] += 1
    lit[256] += 1
    return lit, dist


def extra_bits(tokens):
    return sum(len_symbol(t[0])[1] + dist_symbol(t[1])[1] for t in tokens if isinstance(t, tuple))


def token_bits(tokens, lit_lens, dist_lens):
    """bits of the tokens and the end of block under the given code lengths"""
    lit, dist = histograms(tokens)
    assert all(lit_lens[s] for s in range(len(lit)) if lit[s]) and all(dist_lens[s] for s in range(30) if dist[s])
    return sum(f * lit_lens[s] for s, f in enumerate(lit) if f) + sum(f * dist_lens[s] for s, f in enumerate(dist) if f) + extra_bits(tokens)


def fixed_bits(tokens):
    """bits of the whole block in the fixed form (BTYPE 1)"""
    return 3 + token_bits(tokens, FIXED_LIT, FIXED_DIST)


def stored_bytes(n):
    return n + 5


def huffman(freqs):
    """(cost = sum f * len, depth) of a minimum-redundancy code of the nonzero frequencies; among the optimal trees the one of least depth (ties in
    weight go to the shallower subtree), so depth is the smallest that any optimal code needs.  One symbol: a 1-bit code."""
    fs = [f for f in freqs if f]
    if not fs:
        return 0, 0
    if len(fs) == 1:
        return fs[0], 1
    h = [(f, 0) for f in fs]
    heapq.heapify(h)
    cost = 0
    while len(h) > 1:
        (a, da), (b, db) = heapq.heappop(h), heapq.heappop(h)
        cost += a + b
        heapq.heappush(h, (a + b, max(da, db) + 1))
    return cost, h[0][1]


def package_merge(freqs, limit):
    """exact optimum of sum f * len over prefix codes with every length <= limit (Larmore & Hirschberg 1990): {index: length} of the nonzero
    frequencies.  Items are (weight, tuple of leaves); the 2m - 2 cheapest packages of the last level say how often each leaf is taken."""
    leaves = sorted((f, (i,)) for i, f in enumerate(freqs) if f)
    m = len(leaves)
    if m == 1:
        return {leaves[0][1][0]: 1}
    assert m <= 1 << limit
    cur = list(leaves)
    for _ in range(limit - 1):
        pk = [(cur[i][0] + cur[i + 1][0], cur[i][1] + cur[i + 1][1]) for i in range(0, len(cur) - 1, 2)]
        cur = sorted(leaves + pk, key=lambda x: x[0])
    out = dict.fromkeys((l[1][0] for l in leaves), 0)
    for _, ids in cur[:2 * m - 2]:
        for i in ids:
            out[i] += 1
    return out


def check_code_lengths(freqs, lens, limit):
    """Asserts that `lens` is as good a code for `freqs` as the format allows and returns whether the limit pressed (the least deep optimal tree
    is deeper than `limit`).  Always: every used symbol has a code of 1..limit bits, the code is complete (Kraft sum exactly one), no more frequent
    symbol has a longer code.  Optimum depth within the limit: cost equal to the Huffman optimum.  Deeper: cost at least the optimum.  The one
    allowed excess: with fewer than two used symbols, unused symbols 0 / 1 may carry 1-bit codes to make the code complete."""
    lens = list(lens) + [0] * (len(freqs) - len(lens))
    used = [s for s, f in enumerate(freqs) if f]
    dummies = [s for s, l in enumerate(lens) if l and not freqs[s]]
    if dummies:
        assert len(used) < 2 and len(used) + len(dummies) == 2 and all(s < 2 and lens[s] == 1 for s in dummies), (used, dummies)
    assert all(0 < lens[s] <= limit for s in used), "a used symbol without a code, or a code above %d bits" % limit
    if len(used) + len(dummies) >= 2:
        assert kraft(lens, limit) == 1 << limit, "the code is not complete"
    order = sorted(used, key=lambda s: freqs[s])
    for a, b in zip(order, order[1:]):
        assert freqs[a] == freqs[b] or lens[a] >= lens[b], "a more frequent symbol has the longer code"
    cost, (opt, depth) = sum(freqs[s] * lens[s] for s in used), huffman(freqs)
    if depth <= limit:
        assert cost == opt, "cost %d, the Huffman optimum is %d" % (cost, opt)
        return False
    assert cost >= opt
    return True
