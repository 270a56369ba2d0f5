"""The one-lane routines of k_bgzf.hip, each against plain Python: the symbol arithmetic against RFC 1951's tables (tests/deflate_inspect.py), the CRC
pieces against zlib.crc32, the code-length builder against the Huffman optimum and -- where 15 / 7 bits press -- against the exact length-limited
optimum (package-merge), the canonical codes against the codes a decoder builds from the same lengths.  Whole blocks do not reach the fold of code
lengths above the limit (tests/test_bgzf_streams.py says what they reach); here it runs on frequency sets built to need it.  Host build of
oracle/bgzf_routines_check.cpp through the wave emulator's headers; no GPU."""
import ctypes as C
import os
import random
import subprocess
import tempfile
import zlib

import pytest

import deflate_inspect as DI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.environ.get("EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="the host clang++ of ROCm is missing")
u32p = C.POINTER(C.c_uint32)
_LIB = {}


def routines_lib():
    """oracle/bgzf_routines_check.cpp in a temporary shared library (built once per process; oracle/ is only read)"""
    if "L" not in _LIB:
        so = os.path.join(tempfile.mkdtemp(prefix="staramd_bgzf_routines_"), "libbgzf_routines.so")
        subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wno-unknown-attributes", "-D_GNU_SOURCE", "-I", "oracle/wave_emul",
                               "oracle/bgzf_routines_check.cpp", "oracle/wave_emul/emu.cpp", "oracle/wave_emul/emu_lds.cpp", "-o", so, "-ldl"], cwd=ROOT)
        L = C.CDLL(so)
        for f in ("bzr_len_extra", "bzr_dist_extra", "bzr_fixed_lit_len", "bzr_cl_order", "bzr_x_pow8"):
            getattr(L, f).restype = C.c_uint32; getattr(L, f).argtypes = [C.c_uint32]
        L.bzr_mul_mod_p.restype = C.c_uint32; L.bzr_mul_mod_p.argtypes = [C.c_uint32, C.c_uint32]
        for f in ("bzr_len_sym", "bzr_dist_sym"):
            getattr(L, f).restype = C.c_uint32; getattr(L, f).argtypes = [C.c_uint32, u32p, u32p]
        L.bzr_huff_lengths.restype = None; L.bzr_huff_lengths.argtypes = [u32p, u32p, C.c_uint32, C.c_uint32, u32p]
        L.bzr_canon.restype = None; L.bzr_canon.argtypes = [u32p, C.c_uint32]
        L.bzr_rank.restype = None; L.bzr_rank.argtypes = [u32p, C.c_uint32, u32p, u32p]
        _LIB["L"] = L
    return _LIB["L"]


@pytest.fixture(scope="module")
def L():
    return routines_lib()


def kernel_lengths(L, freqs, limit):
    """code lengths of the kernel for a frequency array, the way k_bgzf_blocks calls its routines: rankSym of every symbol, then huffLengths"""
    n = len(freqs)
    f = (C.c_uint32 * n)(*freqs)
    sym, frq, pack = (C.c_uint32 * n)(), (C.c_uint32 * n)(), (C.c_uint32 * n)()
    L.bzr_rank(f, n, sym, frq)
    m = sum(1 for x in freqs if x)
    assert m >= 2
    assert [frq[i] for i in range(m)] == sorted(x for x in freqs if x) and sorted(sym[i] for i in range(m)) == [s for s, x in enumerate(freqs) if x]
    assert all((frq[i], sym[i]) < (frq[i + 1], sym[i + 1]) for i in range(m - 1)), "rankSym: not the order (frequency, symbol)"
    L.bzr_huff_lengths(frq, sym, m, limit, pack)
    assert all(not (p & 0xffff) for p in pack)
    return [p >> 16 for p in pack]


def test_length_and_distance_symbols(L):
    eb, ev = C.c_uint32(), C.c_uint32()
    for n in range(3, 259):                 # 258 included: symbol 285, which no block reaches while a lane's slice is at most 255 bytes
        assert (L.bzr_len_sym(n, C.byref(eb), C.byref(ev)), eb.value, ev.value) == DI.len_symbol(n), n
    for d in range(1, 32769):
        assert (L.bzr_dist_sym(d, C.byref(eb), C.byref(ev)), eb.value, ev.value) == DI.dist_symbol(d), d
    for s in range(257, 286):
        assert L.bzr_len_extra(s) == DI.LEN_TABLE[s - 257][0], s
    for c in range(30):
        assert L.bzr_dist_extra(c) == DI.DIST_TABLE[c][0], c
    assert [L.bzr_fixed_lit_len(s) for s in range(288)] == DI.FIXED_LIT
    assert [L.bzr_cl_order(i) for i in range(19)] == DI.CL_ORDER


def _raw(d):
    """the CRC register run over d from 0 with no final complement (what a lane of the kernel keeps), by linearity out of zlib's"""
    return zlib.crc32(d) ^ zlib.crc32(bytes(len(d)))


def test_crc_pieces(L):
    """crc32(A || B) put together the way the kernel joins its lanes' slices: raw(A) * x^(8|B|) + raw(B) + 0xffffffff * x^(8|A || B|), complemented"""
    r = random.Random(7)
    sizes = set(range(0, 300)) | {0xff00, 0xff00 - 1}
    for k in range(1, 16):
        sizes |= {(1 << k) - 1, 1 << k, (1 << k) + 1}
    sizes |= {r.randrange(300, 0xff00) for _ in range(60)}
    big = bytes(r.getrandbits(8) for _ in range(2 * 0xff00))
    assert L.bzr_x_pow8(0) == 0x80000000 and L.bzr_mul_mod_p(0x80000000, 0x12345678) == 0x12345678           # x^0 is the unit
    for nb in sorted(s for s in sizes if s <= 0xff00):
        for na in (0, 1, 255, r.randrange(0, 0xff00 - nb + 1)):
            if na + nb > 0xff00:
                continue
            a, b = big[:na], big[0xff00:0xff00 + nb]
            got = L.bzr_mul_mod_p(_raw(a), L.bzr_x_pow8(nb)) ^ _raw(b) ^ L.bzr_mul_mod_p(0xffffffff, L.bzr_x_pow8(na + nb))
            assert got ^ 0xffffffff == zlib.crc32(a + b), (na, nb)


def _fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


def frequency_sets():
    """(name, frequencies, limit): built to exceed the limit, plus the plain cases"""
    r = random.Random(20261016)
    out = []
    for k in range(17, 41):
        out.append(("fib%d" % k, _fib(k), 15))
    for k in range(9, 20):
        out.append(("fib%d/7" % k, _fib(k), 7))
    for k in (17, 20, 24):                                       # Fibonacci scaled into what one block can hold (total <= 65281), sorted and shuffled
        f = [max(1, x * 65000 // sum(_fib(k))) for x in _fib(k)]
        out.append(("fibscaled%d" % k, f, 15))
        g = f + [0] * (286 - k); r.shuffle(g)
        out.append(("fibscaled%d shuffled" % k, g, 15))
    for base, k in ((2, 16), (2, 30), (3, 20), (2, 19)):
        out.append(("geometric %d^i x %d" % (base, k), [base ** i for i in range(k)], 15))
    for k in (8, 12, 19):
        out.append(("geometric 2^i x %d /7" % k, [2 ** i for i in range(k)], 7))
        out.append(("geometric 3^i x %d /7" % k, [3 ** i for i in range(k)], 7))
    for m in (2, 3, 30, 100, 285, 286):
        out.append(("giant + %d ones" % (m - 1), [65281 - (m - 1)] + [1] * (m - 1), 15))
        out.append(("%d equal" % m, [7] * m, 15))
    for m in (2, 3, 18, 19):
        out.append(("giant + %d ones /7" % (m - 1), [300] + [1] * (m - 1), 7))
        out.append(("%d equal /7" % m, [5] * m, 7))
    out.append(("m = 2", [1, 65280], 15))
    out.append(("m = 2 /7", [1, 1], 7))
    for i in range(20):
        out.append(("m = 286 random %d" % i, [r.randint(1, 65280) for _ in range(286)], 15))
    for i in range(2000):                                        # what a block can hold: total <= 65281
        if i % 2:
            n, limit = r.choice((19, 19, 10, 5)), 7
            m = r.randint(2, n)
            w = [r.random() ** r.choice((1, 4, 12, 40)) for _ in range(m)]
            tot = r.randint(m, 316)
        else:
            n, limit = r.choice((286, 286, 30)), 15
            m = r.randint(2, n)
            w = [r.random() ** r.choice((1, 4, 12, 40)) for _ in range(m)]
            tot = r.randint(m, 65281)
        f = [max(1, int(x * tot / sum(w))) for x in w]
        while sum(f) > max(tot, m):
            f[f.index(max(f))] -= 1
        g = f + [0] * (n - m); r.shuffle(g)
        out.append(("random %d" % i, g, limit))
    return out


def test_code_lengths_against_huffman_and_package_merge(L):
    worst, pressed, n = {15: (1.0, None), 7: (1.0, None)}, {15: 0, 7: 0}, 0
    for name, freqs, limit in frequency_sets():
        lens = kernel_lengths(L, freqs, limit)
        was_pressed = DI.check_code_lengths(freqs, lens, limit)
        used = [s for s, f in enumerate(freqs) if f]
        cost = sum(freqs[s] * lens[s] for s in used)
        pm = DI.package_merge(freqs, limit)
        best = sum(freqs[s] * pm[s] for s in used)
        assert DI.kraft([pm[s] for s in used], limit) <= 1 << limit and max(pm.values()) <= limit, name       # the judge itself
        assert cost >= best, (name, cost, best)
        opt, depth = DI.huffman(freqs)
        assert best >= opt and (best == opt) == (depth <= limit), (name, best, opt, depth)                      # the judge itself, again
        if not was_pressed:
            assert cost == best, (name, cost, best)
        else:
            pressed[limit] += 1
            if cost / best > worst[limit][0]:
                worst[limit] = (cost / best, name)
        n += 1
    print("%d frequency sets; the limit pressed on %d (15 bits) and %d (7 bits); worst cost over the length-limited optimum: %.4f x at 15 bits (%s), %.4f x at 7 bits (%s)"
          % (n, pressed[15], pressed[7], worst[15][0], worst[15][1], worst[7][0], worst[7][1]))
    assert pressed[15] >= 24 and pressed[7] >= 11, pressed          # every Fibonacci set above is deeper than its limit


def test_canonical_codes(L):
    r = random.Random(3)
    cases = [(list(DI.FIXED_LIT), 288), ([5] * 30, 30), ([1, 1] + [0] * 28, 30), ([0, 1, 0, 0, 1] + [0] * 14, 19)]
    for name, freqs, limit in frequency_sets()[::7]:
        cases.append((kernel_lengths(L, freqs, limit), len(freqs)))
    for lens, n in cases:
        pack = (C.c_uint32 * n)(*[l << 16 for l in lens])
        L.bzr_canon(pack, n)
        want = DI.canonical_codes(lens)
        codes = {}
        for s in range(n):
            assert pack[s] >> 16 == lens[s]
            if not lens[s]:
                assert pack[s] == 0
                continue
            sent = format(pack[s] & 0xffff, "0%db" % lens[s])[::-1]         # the kernel keeps the code bit-reversed: its lowest bit is sent first
            assert int(sent, 2) == want[s][0], (s, lens[s])
            codes[s] = sent
        cs = sorted(codes.values())
        assert all(not b.startswith(a) for a, b in zip(cs, cs[1:])), "not prefix-free"
        dec = DI._Decoder(lens)                                              # and the decoder's table reads every code back to its symbol
        for s, sent in codes.items():
            assert dec.table[int(sent[::-1], 2)] == (s, lens[s])
