"""Every member that k_bgzf.hip (wave emulator build, tests/test_bgzf_emul.py) makes of every vector at every level, taken apart by
tests/deflate_inspect.py and held to DESIGN 7.3:
  codes    the literal/length, distance and code-length codes cost exactly the Huffman optimum of their own histograms (15 / 15 / 7 bits allowing),
           are complete, and HLIT / HDIST / HCLEN and the run-length description are the shortest the documented rule gives
  choice   dynamic, fixed or stored as the rule says, from bit counts recomputed here
  parse    the tokens are the ones a plain sequential restatement of the rule finds (levels 1, 2, 6: one level per row of the kernel's level table)
  reach    the set of branches all vectors x levels reach is asserted, so a vector that stops reaching its branch fails here
The only things shared with the kernel are the hash function and the constants of the rule (chunk sizes, 256 slices, 4096 heads, 32768, 4 candidates and the
lazy cut at 32), taken from DESIGN 7.3.  On this vector set: 10 - 15 s per level on one CPU core, about 70 s for this module (emulator, Python inflate and Python parse)."""
import struct

import pytest

import deflate_inspect as DI
import test_bgzf_emul as E
from test_bgzf_emul import bz  # noqa: F401  (fixture)

IN_MAX = 0xff00
LANES = 256
PARSE_LEVELS = (1, 2, 6)                 # chunks of 64 greedy / chunks of 32 greedy / chunks of 32 lazy: every other level is one of these three
MAX_HEADER_BITS = 17 + 19 * 3 + (286 + 30) * 7      # no tree description is longer: every length as one code-length symbol of 7 bits


def level_rule(level):
    """(chunk, lazy, candidates tried) of a level > 0 or -1, DESIGN 7.3 'Levels'"""
    lazy = level >= 4 or level < 0
    return (64 if level == 1 else 32), lazy, (4 if lazy else 1)


def hash4(d, p):
    return ((int.from_bytes(d[p:p + 4], "little") * 0x9E3779B1) & 0xffffffff) >> 20


def restated_parse(d, level):
    """DESIGN 7.3's parse as one loop over the positions of a block.  -> (tokens, facts)"""
    n = len(d)
    chunk, lazy, tries = level_rule(level)
    S = -(-n // LANES)
    head, cand = {}, [None] * n
    for p in range(n):                                       # the candidate: the latest position with p's hash in the chunks before p's own
        if p and p % chunk == 0:
            for q in range(p - chunk, p):
                if q + 4 <= n:
                    head[hash4(d, q)] = q
        if p + 4 <= n:
            cand[p] = head.get(hash4(d, p))
    facts = set()

    def best(p, end):
        """(length, source) of the longest match among the first `tries` candidates of p -- its candidate, that one's candidate, ... -- that are
        within 32768; the nearest of equally long ones"""
        q, lim, bl, bq = cand[p], min(258, end - p), 0, None
        for _ in range(tries):
            if q is None:
                break
            if p - q > 32768:
                if p - q == 32769:
                    facts.add("candidate 32769 back refused")
                break
            L = 0
            while L < lim and d[q + L] == d[p + L]:
                L += 1
            if L > bl:
                bl, bq = L, q
            q = cand[q]
        return bl, bq
    tokens, p = [], 0
    while p < n:
        end = min(n, (p // S + 1) * S)                       # a match stays inside its lane's slice
        L, q = best(p, end)
        if L >= 3 and lazy and L < 32 and p + 1 < end and best(p + 1, end)[0] > L:
            L = 0
        if L >= 3:
            tokens.append((L, p - q)); p += L
        else:
            tokens.append(d[p]); p += 1
    return tokens, facts


def restated_rle(lens):
    """the tree description of the lengths (literal/length and distance lengths as one sequence): zeros in runs of 11..138 (18), then 3..10 (17),
    else singly; a nonzero length once, then repeats of 3..6 (16), the rest singly"""
    out, i = [], 0
    while i < len(lens):
        v, r = lens[i], 1
        while i + r < len(lens) and lens[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r >= 11:
                t = min(r, 138); out.append((18, t)); r -= t
            if r >= 3:
                out.append((17, r)); r = 0
        else:
            out.append((v, None)); r -= 1
            while r >= 3:
                t = min(r, 6); out.append((16, t)); r -= t
        out += [(v, None)] * r
    return out


def model_lengths(freqs, limit):
    """Code lengths as the kernel's comment states them: Huffman by the two-queue method on the symbols sorted by (frequency, symbol), a leaf before
    a package of the same weight; the lengths handed out longest to the first of that order.  None when the tree is deeper than `limit` (then the
    fold decides, which tests/test_bgzf_routines.py covers)."""
    order = sorted((f, s) for s, f in enumerate(freqs) if f)
    m = len(order)
    assert m >= 2
    w, parent = [f for f, _ in order], [None] * m
    li, pi = 0, m                                            # next leaf, next unused package
    for _ in range(m - 1):
        pick = []
        for _ in range(2):
            if pi >= len(w) or (li < m and w[li] <= w[pi]):
                pick.append(li); li += 1
            else:
                pick.append(pi); pi += 1
        w.append(w[pick[0]] + w[pick[1]])
        parent.append(None)
        parent[pick[0]] = parent[pick[1]] = len(w) - 1
    depth = [0] * len(w)
    for i in range(len(w) - 2, -1, -1):
        depth[i] = depth[parent[i]] + 1
    ds = sorted(depth[:m], reverse=True)
    if ds[0] > limit:
        return None
    lens = [0] * len(freqs)
    for (_, s), l in zip(order, ds):
        lens[s] = l
    return lens


def model_dynamic_bits(tokens):
    """bits of the dynamic form the kernel would make of these tokens, or None where a limit presses"""
    lit, dist = DI.histograms(tokens)
    for s in (0, 1):
        if sum(1 for f in dist if f) < 2 and not dist[s]:
            dist[s] = 1                                      # "distance code of at least two symbols"
    ll, dl = model_lengths(lit, 15), model_lengths(dist, 15)
    if ll is None or dl is None:
        return None
    hlit, hdist = 286, 30
    while hlit > 257 and not ll[hlit - 1]:
        hlit -= 1
    while hdist > 1 and not dl[hdist - 1]:
        hdist -= 1
    rle = restated_rle(ll[:hlit] + dl[:hdist])
    clf = [0] * 19
    for s, _ in rle:
        clf[s] += 1
    if sum(1 for f in clf if f) < 2:
        clf[1 if clf[0] else 0] = 1
    cl = model_lengths(clf, 7)
    if cl is None:
        return None
    hclen = 19
    while hclen > 4 and not cl[DI.CL_ORDER[hclen - 1]]:
        hclen -= 1
    hdr = 17 + 3 * hclen + sum(cl[s] + {16: 2, 17: 3, 18: 7}.get(s, 0) for s, _ in rle)
    return hdr + DI.token_bits(tokens, ll, dl), ll[:hlit], dl[:hdist], cl


def split_members(blob):
    p, out = 0, []
    while p < len(blob):
        bsize = struct.unpack("<H", blob[p + 16:p + 18])[0] + 1
        out.append(blob[p:p + bsize])
        p += bsize
    return out


def check_member(data, member, level, parse=True):
    """every property of one member; -> the set of things this member reached"""
    n = len(data)
    blk = DI.inflate_block(member[18:-8])
    assert blk.data == data
    assert len(member) <= n + 31
    reach = {"BTYPE %d" % blk.btype}
    if level == 0:
        assert blk.btype == 0
        return reach
    tokens, facts = blk.tokens, set()
    if parse or blk.btype == 0:
        tokens, facts = restated_parse(data, level)
        if blk.btype:
            bad = next((i for i, (a, b) in enumerate(zip(tokens, blk.tokens)) if a != b), min(len(tokens), len(blk.tokens)))
            assert tokens == blk.tokens, "token %d: the rule gives %r, the stream has %r" % (bad, tokens[bad:bad + 3], blk.tokens[bad:bad + 3])
    reach |= facts
    lit, dist = DI.histograms(tokens)
    nd = sum(1 for f in dist if f)
    fix = DI.fixed_bits(tokens)
    model = model_dynamic_bits(tokens)
    if blk.btype == 2:
        assert blk.hlit == 257 or blk.lit_lens[-1], "HLIT counts a trailing zero"
        assert blk.hdist == 1 or blk.dist_lens[-1], "HDIST counts a trailing zero"
        assert blk.cl_lens[DI.CL_ORDER[blk.hclen - 1]] or blk.hclen == 4, "HCLEN counts a trailing zero"
        if DI.check_code_lengths(lit, blk.lit_lens, 15):
            reach.add("15-bit limit pressed (literal/length)")
        if DI.check_code_lengths(dist, blk.dist_lens, 15):
            reach.add("15-bit limit pressed (distance)")
        clf = [0] * 19
        for s, _ in blk.rle:
            clf[s] += 1
        if DI.check_code_lengths(clf, blk.cl_lens, 7):
            reach.add("7-bit limit pressed (code-length code)")
        assert blk.rle == restated_rle(blk.lit_lens + blk.dist_lens), "the tree description is not the run-length coding of the rule"
        dyn = blk.header_bits + DI.token_bits(tokens, blk.lit_lens, blk.dist_lens)
        assert dyn == blk.bits
        if model is not None:
            assert (blk.lit_lens, blk.dist_lens, blk.cl_lens, dyn) == (model[1], model[2], model[3], model[0]), "code lengths differ from the stated construction"
        reach.add("distance tree with %s used codes" % ("0" if nd == 0 else "1" if nd == 1 else ">= 2"))
        reach.add("HCLEN %d" % blk.hclen)
        reach |= {"run-length symbol %d" % s for s, _ in blk.rle if s >= 16}
        if (18, 138) in blk.rle:
            reach.add("run-length symbol 18 with 138")
        if max(blk.lit_lens) == 15:
            reach.add("literal/length code of 15 bits")
        if max(blk.cl_lens) == 7:
            reach.add("code-length code of 7 bits")
    else:
        dyn = model[0] if model is not None else None
    # ---- the choice: dynamic if not larger than fixed; stored if that form is not smaller than n + 5 bytes or does not fit the LDS buffer
    if dyn is not None:
        bits = min(dyn, fix)
        want = 0 if ((bits + 7) // 8 >= n + 5 or bits > 8 * IN_MAX) else 2 if dyn <= fix else 1
        assert blk.btype == want, "BTYPE %d emitted; dynamic %d bits, fixed %d bits, stored %d bytes" % (blk.btype, dyn, fix, n + 5)
        if blk.btype:
            assert blk.bits == bits and len(member) == 26 + (bits + 7) // 8
    else:                                                    # a limit pressed and the dynamic form was not emitted: bounds only
        opt = DI.huffman(lit)[0] + DI.huffman(dist)[0] + DI.extra_bits(tokens)
        if blk.btype == 1:
            assert fix <= opt + MAX_HEADER_BITS
        else:
            assert (min(fix, opt + MAX_HEADER_BITS) + 7) // 8 >= n + 5
    if blk.btype:
        if any(isinstance(t, tuple) for t in tokens):
            reach.add("BTYPE %d with matches" % blk.btype)
        if any(isinstance(t, tuple) and t[1] == 32768 for t in tokens):
            reach.add("match at distance 32768")
        if any(isinstance(t, tuple) and t[0] == 255 for t in tokens):
            reach.add("match of length 255")
        assert not any(isinstance(t, tuple) and (t[0] > 255 or t[1] > 32768) for t in tokens)
    return reach


def check_call(bzd, level, segs, outs, parse=True):
    reach = set()
    E.check(segs, outs, level)
    for seg, out in zip(segs, outs):
        assert len(out) <= bzd.L.staramd_bgzf_bound(len(seg))
        ms = split_members(out)
        for i, m in enumerate(ms):
            reach |= check_member(seg[i * IN_MAX:(i + 1) * IN_MAX], m, level, parse)
    return reach


_REACH = {}


@pytest.mark.parametrize("level", E.LEVELS)
def test_streams_of_every_vector(bz, level):  # noqa: F811
    reach = set()
    for name, segs in E.synthetic_vectors().items():
        r = check_call(bz, level, segs, bz.compress(level, segs), parse=level in PARSE_LEVELS)
        _REACH.setdefault(name, set()).update(r)
        reach |= r
    _REACH.setdefault("levels", set()).add(level)


# what all vectors x levels must reach between them
MUST_REACH = ["BTYPE 0", "BTYPE 1", "BTYPE 2", "BTYPE 1 with matches", "BTYPE 2 with matches", "match at distance 32768", "candidate 32769 back refused",
              "match of length 255", "distance tree with 0 used codes", "distance tree with 1 used codes", "distance tree with >= 2 used codes",
              "run-length symbol 16", "run-length symbol 17", "run-length symbol 18", "run-length symbol 18 with 138", "HCLEN 18",
              "7-bit limit pressed (code-length code)", "code-length code of 7 bits", "literal/length code of 15 bits", "HCLEN 19",
              "15-bit limit pressed (literal/length)"]
# what no block reaches, and why
UNREACHABLE = {
    "match of length 256..258 (length symbol 285)": "a match stays inside its lane's slice of ceil(n / 256) <= 255 bytes; lenSym's branch for 258 is covered by "
                                                    "tests/test_bgzf_routines.py::test_length_and_distance_symbols",
    "HCLEN 4": "a block has at least two literal/length codes, so some length 1..15 is sent, and those come after the first four entries of the order",
    "15-bit limit pressed (distance)": "needs 17 or more of the 30 distance codes with Fibonacci-like frequencies; no block found does it.  It is the routine and the limit that "
        "the literal/length tree does press (vector fold_15), and tests/test_bgzf_routines.py runs it on 30-symbol sets",
}


def test_reach(bz):  # noqa: F811
    """coverage is asserted, not hoped for (runs after test_streams_of_every_vector, whose results it collects; alone it computes them itself)"""
    if _REACH.get("levels") != set(E.LEVELS):
        for level in E.LEVELS:
            test_streams_of_every_vector(bz, level)
    reach = set().union(*(v for k, v in _REACH.items() if k != "levels"))
    for name, r in sorted(_REACH.items()):
        if name != "levels":
            print("%-22s %s" % (name, sorted(r)))
    missing = [m for m in MUST_REACH if m not in reach]
    assert not missing, missing
    pressed = sorted(x for x in reach if "limit pressed" in x or "of 15 bits" in x or "of 7 bits" in x or x == "HCLEN 19")
    print("reached besides:", pressed, "HCLEN:", sorted(int(x[6:]) for x in reach if x.startswith("HCLEN")))
    for what, why in UNREACHABLE.items():
        print("not reachable: %s -- %s" % (what, why))
