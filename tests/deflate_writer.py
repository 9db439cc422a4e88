"""A raw-deflate (RFC 1951) bit writer for tests, and a corpus of hand-built edge cases.

The writer puts stored, fixed and dynamic blocks at any bit alignment.  Dynamic headers are written from explicit
code-length arrays and, when asked, from an explicit code-length-code sequence, so that constructs other encoders emit
and zlib's compressor never does (repeats across the literal/distance boundary, incomplete distance trees, 15-bit codes,
length 258 as symbol 284 + 31, ...) can be written on purpose.  Pure Python: nothing here depends on zlib.

Every corpus case records zlib's own verdict, computed by the test that uses it (`reference()`): the expected bytes and
`in_used` of a valid case are zlib's output, never written by hand, and an invalid case must be one zlib rejects.
"""
import zlib

import datagen

LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
         6145, 8193, 12289, 16385, 24577)
DEXT = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


def length_code(n):
    """match length 3..258 -> (symbol, extra value, extra bits), the usual coding (258 = symbol 285)"""
    assert 3 <= n <= 258
    if n == 258:
        return 285, 0, 0
    k = max(i for i in range(28) if LBASE[i] <= n)
    return 257 + k, n - LBASE[k], LEXT[k]


def dist_code(d):
    """distance 1..32768 -> (symbol, extra value, extra bits)"""
    assert 1 <= d <= 32768
    k = max(i for i in range(30) if DBASE[i] <= d)
    return k, d - DBASE[k], DEXT[k]


def canonical(lens):
    """code lengths -> {symbol: (code, length)} (RFC 1951 3.2.2)"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def kraft(lens):
    """sum of 2^(15 - l) over the codes: 1 << 15 for a complete set"""
    return sum(1 << (15 - l) for l in lens if l)


class BitWriter:
    def __init__(self):
        self.acc = 0
        self.n = 0
        self.out = bytearray()
        self.allow_final = True                    # False: every block header says BFINAL = 0 (a case built into a segment)

    @property
    def bitpos(self):
        return 8 * len(self.out) + self.n

    def bits(self, v, k):                          # fields and extra bits: LSB first
        assert 0 <= v < (1 << k) or k == 0
        self.acc |= v << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, k):                          # Huffman codes: MSB first
        self.bits(int(format(c & ((1 << k) - 1), "0%db" % k)[::-1], 2) if k else 0, k)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data

    def copy(self):
        w = BitWriter()
        w.acc, w.n, w.out, w.allow_final = self.acc, self.n, bytearray(self.out), self.allow_final
        return w

    def getvalue(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


# ---- tokens ----
# an int 0..255 is a literal; (length, distance) a match coded the usual way; ("S", lsym, lext, dsym, dext) a match
# coded with these very symbols and extra-bit values; ("L", sym) a lone literal/length symbol; ("B", value, nbits) raw bits

def _tok_fields(t):
    """-> (lsym, lext value, lext bits, dsym or None, dext value, dext bits) or None for raw bits"""
    if isinstance(t, int):
        return t, 0, 0, None, 0, 0
    if t[0] == "S":
        _, ls, le, ds, de = t
        return ls, le, LEXT[ls - 257] if 257 <= ls <= 285 else 0, ds, de, DEXT[ds] if ds < 30 else 0
    if t[0] == "L":
        return t[1], 0, 0, None, 0, 0
    if t[0] == "B":
        return None
    ls, le, lb = length_code(t[0])
    ds, de, db = dist_code(t[1])
    return ls, le, lb, ds, de, db


def used_symbols(tokens):
    ll, d = set(), set()
    for t in tokens:
        f = _tok_fields(t)
        if f is None:
            continue
        ll.add(f[0])
        if f[3] is not None:
            d.add(f[3])
    return ll, d


def _write_tokens(w, tokens, llc, dc):
    for t in tokens:
        f = _tok_fields(t)
        if f is None:
            w.bits(t[1], t[2])
            continue
        ls, le, lb, ds, de, db = f
        w.code(*llc[ls])
        w.bits(le, lb)
        if ds is not None:
            w.code(*dc[ds])
            w.bits(de, db)


def stored(w, data, final=0, nlen=None):
    assert len(data) <= 65535
    w.bits(final if w.allow_final else 0, 1)
    w.bits(0, 2)
    w.align()
    w.bits(len(data), 16)
    w.bits(len(data) ^ 0xffff if nlen is None else nlen, 16)
    w.raw(data)


def sync_flush(w):
    """Z_SYNC_FLUSH marker: an empty stored block, BFINAL = 0"""
    stored(w, b"", 0)


def fixed(w, tokens, final=0, eob=True):
    w.bits(final if w.allow_final else 0, 1)
    w.bits(1, 2)
    llc, dc = canonical(FIXED_LL), canonical(FIXED_D)
    _write_tokens(w, tokens, llc, dc)
    if eob:
        w.code(*llc[256])


def cl_rle(lens):
    """code lengths -> code-length-code sequence [(symbol, extra value)], runs taken across the whole sequence"""
    seq, i = [], 0
    while i < len(lens):
        v = lens[i]
        run = 1
        while i + run < len(lens) and lens[i + run] == v:
            run += 1
        if v == 0 and run >= 3:
            r = min(run, 138)
            seq.append((18, r - 11) if r >= 11 else (17, r - 3))
            i += r
            continue
        seq.append((v, 0))
        i += 1
        run -= 1
        while run >= 3:
            r = min(run, 6)
            seq.append((16, r - 3))
            i += r
            run -= r
    return seq


def cl_lengths(seq):
    """a complete code for the code-length symbols a sequence uses (lengths <= 7)"""
    used = sorted({s for s, _ in seq})
    if len(used) == 1:
        used.append(0 if used[0] else 1)
    m = len(used)
    k = max(1, (m - 1).bit_length())
    short = (1 << k) - m
    lens = [0] * 19
    for i, s in enumerate(used):
        lens[s] = k - 1 if i < short else k
    return lens


def dynamic(w, tokens, ll_lens, d_lens, final=0, hlit=None, hdist=None, cl_seq=None, cl_lens=None, eob=True):
    """a dynamic block from explicit code lengths (ll_lens: literal/length, d_lens: distance); hlit / hdist default to
    the last nonzero length (at least 257 / 1), cl_seq to cl_rle() over both arrays, cl_lens to cl_lengths(cl_seq)"""
    ll_lens = list(ll_lens) + [0] * max(0, 288 - len(ll_lens))
    d_lens = list(d_lens) + [0] * max(0, 32 - len(d_lens))
    if hlit is None:
        hlit = max([257] + [s + 1 for s in range(288) if ll_lens[s]])
    if hdist is None:
        hdist = max([1] + [s + 1 for s in range(32) if d_lens[s]])
    both = ll_lens[:hlit] + d_lens[:hdist]
    if cl_seq is None:
        cl_seq = cl_rle(both)
    if cl_lens is None:
        cl_lens = cl_lengths(cl_seq)
    hclen = max(4, max(i + 1 for i in range(19) if cl_lens[CL_ORDER[i]]))
    w.bits(final if w.allow_final else 0, 1)
    w.bits(2, 2)
    w.bits(hlit - 257, 5)
    w.bits(hdist - 1, 5)
    w.bits(hclen - 4, 4)
    for i in range(hclen):
        w.bits(cl_lens[CL_ORDER[i]], 3)
    clc = canonical(cl_lens)
    for s, x in cl_seq:
        w.code(*clc[s])
        w.bits(x, {16: 2, 17: 3, 18: 7}.get(s, 0))
    llc, dc = canonical(ll_lens), canonical(d_lens)
    _write_tokens(w, tokens, llc, dc)
    if eob:
        w.code(*llc[256])


# ---- code lengths ----

def kraft_complete(n, fixed_lens, need, spare=()):
    """n code lengths: the symbols of fixed_lens get theirs, every symbol of `need` one of the codes left, and the rest of
    the code space goes to `spare` symbols, so that the set is complete.  This is how a test asks for a number of codes at
    each length (the 15-bit codes, a pool of exactly 100 long literals, long length and distance codes, ...)."""
    lens = [0] * n
    for s, l in fixed_lens.items():
        lens[s] = l
    rest = (1 << 15) - kraft(lens)
    assert rest >= 0, "over-subscribed"
    need = [s for s in need if not lens[s]]
    codes = [15 - b for b in range(16) if rest >> b & 1]          # the space left as codes, longest first
    codes = sorted(codes + [1, 1] if 0 in codes else codes)[1 if 0 in codes else 0:]    # (the whole space: two 1-bit codes)
    while len(codes) < len(need):                                  # split the shortest code until every needed symbol has one
        i = next(i for i, l in enumerate(codes) if l < 15)
        l = codes.pop(i)
        codes += [l + 1, l + 1]
        codes.sort()
    spare = [s for s in spare if not lens[s] and s not in need]
    takers = list(need) + spare
    assert len(codes) <= len(takers), "not enough symbols to complete the code"
    for s, l in zip(takers, codes):
        lens[s] = l
    assert kraft(lens) == 1 << 15
    return lens


def huffman_lengths(freq, n, limit=15):
    """length-limited Huffman code lengths for the symbols of freq (dict symbol -> count); two codes at least"""
    import heapq
    f = {s: c for s, c in freq.items() if c}
    while len(f) < 2:
        f[next(s for s in range(n) if s not in f)] = 1
    while True:
        h = [(c, i, (s,)) for i, (s, c) in enumerate(sorted(f.items()))]
        heapq.heapify(h)
        depth = dict.fromkeys(f, 0)
        k = len(h)
        while len(h) > 1:
            a, b = heapq.heappop(h), heapq.heappop(h)
            for s in a[2] + b[2]:
                depth[s] += 1
            heapq.heappush(h, (a[0] + b[0], k, a[2] + b[2]))
            k += 1
        if max(depth.values()) <= limit:
            break
        f = {s: (c + 1) // 2 for s, c in f.items()}
    lens = [0] * n
    for s, d in depth.items():
        lens[s] = d
    return lens


def greedy_parse(data, hist=b"", max_chain=8, max_dist=32768):
    """a simple greedy LZ77 parse (hash of three bytes, a short chain) -> tokens; matches may reach into hist"""
    buf = bytes(hist) + bytes(data)
    h0 = len(hist)
    heads = {}
    for p in range(max(0, h0 - 32768), max(0, h0 - 2)):
        heads.setdefault(buf[p:p + 3], []).append(p)
    toks, i, n = [], h0, len(buf)
    while i < n:
        best, bd = 0, 0
        if i + 3 <= n:
            key = buf[i:i + 3]
            for p in reversed(heads.get(key, [])[-max_chain:]):
                d = i - p
                if d > max_dist:
                    break
                l = 3
                while l < 258 and i + l < n and buf[p + l] == buf[i + l]:
                    l += 1
                if l > best:
                    best, bd = l, d
        step = best if best >= 3 else 1
        for q in range(i, min(i + step, n - 2)):
            heads.setdefault(buf[q:q + 3], []).append(q)
        toks.append((best, bd) if best >= 3 else buf[i])
        i += step
    return toks


def ordinary_block(w, tokens, final=0):
    """a dynamic block with Huffman codes fitted to its tokens (what an ordinary encoder writes)"""
    fl, fd = {}, {}
    for t in tokens:
        ls, _, _, ds, _, _ = _tok_fields(t)
        fl[ls] = fl.get(ls, 0) + 1
        if ds is not None:
            fd[ds] = fd.get(ds, 0) + 1
    fl[256] = 1
    dynamic(w, tokens, huffman_lengths(fl, 286), huffman_lengths(fd, 30), final)


_CONTENT = {}


def content_tokens(n, seed=5):
    """n bytes of text and its greedy parse (cached: embedding a case at several bit phases reuses it)"""
    if (n, seed) not in _CONTENT:
        data = datagen.gen_bytes("text", n, seed)
        _CONTENT[(n, seed)] = (data, greedy_parse(data))
    return _CONTENT[(n, seed)]


def phase_block(w, phase):
    """a fixed block of literals that leaves the writer at bit position = phase (mod 8): header 3 + EOB 7 bits, and each
    literal from 144 on is 9 bits"""
    k = (phase - w.bitpos - 10) % 8
    fixed(w, [0x90 + i for i in range(k)] + [0x41, 0x42])
    return k + 2


# ---- the corpus ----

def _text(n, seed=11):
    return datagen.gen_bytes("text", n, seed)


def _lits(data):
    return list(data)


def _need(tokens):
    ll, d = used_symbols(tokens)
    return sorted(ll | {256}), sorted(d)


def _dyn_with(w, tokens, ll_fixed=None, d_fixed=None, final=0, d_lens=None, **kw):
    """a dynamic block whose codes have the lengths asked for, the rest of each code filled in around them"""
    ll_need, d_need = _need(tokens)
    ll = kraft_complete(286, ll_fixed or {}, ll_need, spare=range(286))
    if d_lens is None:
        d_lens = kraft_complete(30, d_fixed or {}, d_need, spare=range(30))
    dynamic(w, tokens, ll, d_lens, final, **kw)


def _mix(seed, n, extra_syms, every=7, max_dist=32768):
    """text with the literals extra_syms spread through it (each at least twice) and some matches"""
    data = bytearray(_text(n, seed))
    for i, s in enumerate(list(extra_syms) * 2):
        data[(i * every * 13 + 5) % n] = s
    return greedy_parse(bytes(data), max_dist=max_dist)


def _v_dist_single(w):
    """distance tree of one code of length 1 (an incomplete set zlib accepts; zlib writes two codes)"""
    toks = _lits(b"abcdefgh") + [(10, 1), 0x78, (20, 1), (258, 1), 0x79, (3, 1)]
    _dyn_with(w, toks, d_lens=[1], final=1)


def _v_dist_single_far(w):
    """the same with the one code for distance symbol 9 (25..32, three extra bits) at HDIST = 10"""
    toks = _lits(_text(60)) + [("S", 262, 0, 9, 5), 0x7a, ("S", 270, 2, 9, 0), ("S", 285, 0, 9, 7)]
    _dyn_with(w, toks, d_lens=[0] * 9 + [1], final=1)


def _v_no_dist(w):
    """no distance codes at all: HDIST = 1, its length 0 (a block of literals only)"""
    _dyn_with(w, _lits(_text(700, 3)), d_lens=[0], final=1)


def _v_len258_284(w):
    """length 258 written as symbol 284 + extra 31 (zlib decodes it as 258; the usual coding is 285), fixed and dynamic"""
    t = _lits(_text(300, 4))
    fixed(w, t + [("S", 284, 31, 4, 1), 0x21, ("S", 284, 31, 0, 0), ("S", 284, 30, 13, 2)])
    _dyn_with(w, [("S", 284, 31, 10, 7), 0x22, ("S", 284, 31, 1, 0), (258, 3)], final=1)


def _v_rep16_across(w):
    """a repeat (symbol 16) that runs from the literal/length lengths into the distance lengths"""
    toks = _lits(_text(400, 6)) + [(3, 1), (4, 2), (5, 4), (3, 3), 0x55, (5, 1)]
    ll_need, _ = _need(toks)
    ll = kraft_complete(260, {257: 2, 258: 2, 259: 2}, ll_need, spare=range(256))
    d = [2, 2, 2, 2] + [0] * 26                    # codes 0..3 only: distances 1..4
    seq = cl_rle(ll[:257]) + [(2, 0), (16, 3)]        # 257 = 2, then six more: 258, 259 and the four distance lengths
    dynamic(w, toks, ll, d, final=1, hlit=260, hdist=4, cl_seq=seq)


def _v_rep18_across(w):
    """a run of zeros (symbol 18, and 17) from the end of the literal/length lengths into the distance lengths"""
    toks = _lits(_text(500, 7)) + [(3, 9), (4, 12)]
    ll_need, _ = _need(toks)
    ll = kraft_complete(286, {}, ll_need, spare=range(256))       # no length symbol above 258 has a code
    d = [0] * 6 + [1, 1]                             # distance symbols 6 (9..12) and 7 (13..16)
    seq = cl_rle(ll[:271] + d[:8])                   # lengths 259..270 and distances 0..5: one run of 18 zeros
    assert (18, 7) in seq
    dynamic(w, toks, ll, d, final=1, hlit=271, hdist=8, cl_seq=seq)


def _v_len15(w):
    """literal/length and distance codes of every length up to 15 bits"""
    longs = list(range(0xc0, 0xd0))
    ll_fixed = {s: l for s, l in zip(longs, [10, 11, 11, 12, 12, 13, 13, 14, 14, 15, 15, 15, 15, 14, 13, 12])}
    ll_fixed.update({280: 15, 281: 14})
    toks = _mix(8, 3000, longs, max_dist=256) + [("S", 280, 0, 0, 0), ("S", 281, 15, 1, 0)]
    d_lens = list(range(1, 15)) + [15, 15]          # distance symbols 0..15: lengths 1, 2, ..., 14, 15, 15
    toks += [("S", 257, 0, k, 0) for k in range(16)]
    _dyn_with(w, toks, ll_fixed, d_lens=d_lens, final=1)


def _pool_case(nlong):
    """exactly nlong literals with codes longer than the literal root (9 bits): QZK_LPOOL_N = 100 of them fit the pool"""
    def build(w):
        longs = list(range(256 - nlong, 256)) if nlong <= 200 else list(range(0x20)) + list(range(256 - (nlong - 32), 256))
        lens = [10, 11, 12, 13]
        ll_fixed = {s: lens[(s * 7) % 4] for s in longs}
        while kraft(ll_fixed.values()) % 64:       # leave room that codes of at most 9 bits fill exactly
            r = kraft(ll_fixed.values()) % 64
            if r == 32:                            # two 10-bit codes become 11-bit ones
                for s in [s for s in longs if ll_fixed[s] == 10][:2]:
                    ll_fixed[s] = 11
            else:                                  # a code of the lowest unit left one bit shorter (11 bits at least before)
                ll_fixed[next(s for s in longs if 1 << (15 - ll_fixed[s]) == r & -r)] -= 1
        toks = _mix(9 + nlong, 6000, longs, every=3)
        ll_need, _ = _need(toks)
        short = [s for s in ll_need if s not in ll_fixed]
        # the needed short symbols take codes of at most 9 bits: fill with lengths <= 9 for those, the rest spare-long
        ll = kraft_complete(286, ll_fixed, short, spare=[])
        assert all(ll[s] <= 9 for s in short) and sum(1 for s in range(256) if ll[s] > 9) == nlong
        dynamic(w, toks, ll, kraft_complete(30, {}, _need(toks)[1], spare=range(30)), final=1)
    build.__doc__ = "%d literals with codes longer than the 9-bit root" % nlong
    return build


def _v_lit255_long(w):
    """literal 255 with a long code, first in the pool's canonical order, next to END_BLOCK and length symbols with long
    codes (0xff in the pool means 'ask the sorted list in memory')"""
    ll_fixed = {255: 10, 256: 11, 257: 11, 258: 11, 265: 12, 254: 11, 0xfe - 10: 12}
    toks = _mix(10, 2000, [255, 254, 0xf4]) + [(3, 7), (4, 9), (11, 30), 255, (3, 1), 255, 255]
    _dyn_with(w, toks, ll_fixed, final=1)


def _v_long_lensyms(w):
    """length symbols with codes of 10..14 bits (looked up past the root)"""
    ll_fixed = {s: 10 + (s % 5) for s in range(257, 286)}
    toks = _lits(_text(2000, 12))
    for k in range(29):
        toks += [("S", 257 + k, (1 << LEXT[k]) - 1, 3, 0), 0x30 + k % 10]
    _dyn_with(w, toks, ll_fixed, final=1)


def _v_long_dist(w):
    """distance codes longer than the 7-bit distance root: 8..13 bits, every distance symbol in use"""
    pre = _text(33000, 13)
    stored(w, pre[:30000])
    stored(w, pre[30000:])
    d = kraft_complete(30, {29 - k: k + 1 for k in range(7)}, range(23), spare=[])     # 23 codes of 11 and 12 bits
    assert sum(1 for l in d if l > 7) == 23
    toks = []
    for k in range(30):
        toks += [("S", 260 + k % 20, 0, k, (1 << DEXT[k]) - 1 if k % 2 else 0), 0x2e]
    ll_need, _ = _need(toks)
    dynamic(w, toks, kraft_complete(286, {}, ll_need, spare=range(286)), d, final=1)


def _v_empty_dynamic(w):
    """a dynamic block that holds only END_BLOCK, then content"""
    toks = _lits(_text(200, 14))
    ll_need, _ = _need(toks)
    dynamic(w, [], kraft_complete(286, {}, ll_need, spare=range(286)), [1, 1])
    fixed(w, toks, final=1)


def _v_eob_only_code(w):
    """a literal/length code of END_BLOCK alone, length 1 (incomplete; zlib accepts a single 1-bit code), no distances"""
    dynamic(w, [], [0] * 256 + [1], [0])
    fixed(w, _lits(_text(100, 15)) + [(50, 20)], final=1)


def _v_stored_edges(w):
    """stored blocks of 65535 bytes and of 0 bytes with BFINAL (not flush markers), matches back into stored data"""
    big = _text(65535, 16)
    fixed(w, _lits(b"start"))
    stored(w, big)
    fixed(w, [(258, 32768), (100, 32768), 0x41, (3, 1), (258, 30000)])
    stored(w, b"", final=1)


def _v_trailing(w):
    """a BFINAL block followed by bytes that belong to no block: in_used stops at the block's end"""
    fixed(w, greedy_parse(_text(900, 17)), final=1)
    w.align()
    w.raw(b"\x00\x00\xff\xff trailing bytes \x03")


def _v_fixed_all_codes(w):
    """a fixed block that uses every length symbol and every distance symbol (32 KiB of history first)"""
    pre = _text(33000, 18)
    stored(w, pre[:33000])
    toks = []
    for k in range(29):
        toks += [("S", 257 + k, k % (1 << LEXT[k]) if LEXT[k] else 0, k, 0), 0x2c]
    toks += [("S", 257, 0, 29, 8191)]
    fixed(w, toks, final=1)


VALID = {
    "dist_single_code": _v_dist_single,
    "dist_single_code_far": _v_dist_single_far,
    "no_distance_codes": _v_no_dist,
    "len258_as_284_31": _v_len258_284,
    "rep16_across_lit_dist": _v_rep16_across,
    "rep18_across_lit_dist": _v_rep18_across,
    "codes_of_15_bits": _v_len15,
    "pool_100_long_literals": _pool_case(100),
    "pool_101_long_literals": _pool_case(101),
    "pool_220_long_literals": _pool_case(220),
    "literal_255_long": _v_lit255_long,
    "long_length_symbols": _v_long_lensyms,
    "long_distance_codes": _v_long_dist,
    "empty_dynamic_block": _v_empty_dynamic,
    "end_block_only_code": _v_eob_only_code,
    "stored_0_and_65535": _v_stored_edges,
    "bfinal_then_trailing_bytes": _v_trailing,
    "fixed_every_code": _v_fixed_all_codes,
}


# ---- invalid cases ----

def _ordinary_lens(toks):
    ll_need, d_need = _need(toks)
    return kraft_complete(286, {}, ll_need, spare=range(286)), kraft_complete(30, {}, d_need, spare=range(30))


_T = None


def _toks():
    global _T
    if _T is None:
        _T = greedy_parse(_text(600, 21))
    return _T


def _i_hlit(w):
    """HLIT = 287 (more than 286 literal/length codes)"""
    ll, d = _ordinary_lens(_toks())
    dynamic(w, _toks(), ll + [0], d, final=1, hlit=287)


def _i_hdist(w):
    """HDIST = 31 (more than 30 distance codes)"""
    ll, d = _ordinary_lens(_toks())
    dynamic(w, _toks(), ll, d + [0], final=1, hdist=31)


def _i_ll_incomplete(w):
    """a literal/length code with a hole, longest code 10 bits"""
    ll, d = _ordinary_lens(_toks())
    ll[max(range(286), key=lambda s: ll[s])] += 1
    assert kraft(ll) < 1 << 15
    dynamic(w, _toks(), ll, d, final=1)


def _i_ll_oversub(w):
    """an over-subscribed literal/length code"""
    ll, d = _ordinary_lens(_toks())
    ll[next(s for s in range(256) if ll[s] == 0)] = max(ll)
    dynamic(w, _toks(), ll, d, final=1)


def _i_d_oversub(w):
    """an over-subscribed distance code"""
    ll, d = _ordinary_lens(_toks())
    d[next(s for s in range(30) if d[s] == 0)] = 1
    dynamic(w, _toks(), ll, d, final=1)


def _i_d_incomplete(w):
    """an incomplete distance code whose longest code is 2 bits (zlib takes a lone 1-bit code only)"""
    ll, d = _ordinary_lens(_toks())
    dynamic(w, [t for t in _toks() if isinstance(t, int)], ll, [2, 2, 2], final=1)


def _i_cl_incomplete(w):
    """an incomplete code-length code"""
    ll, d = _ordinary_lens(_toks())
    seq = cl_rle(ll + d)
    cl = cl_lengths(seq)
    cl[next(s for s in range(19) if cl[s])] += 1
    dynamic(w, _toks(), ll, d, final=1, hlit=286, hdist=30, cl_seq=seq, cl_lens=cl)


def _i_cl_oversub(w):
    """an over-subscribed code-length code"""
    ll, d = _ordinary_lens(_toks())
    seq = cl_rle(ll + d)
    cl = cl_lengths(seq)
    cl[next(s for s in range(19) if cl[s] == 0)] = 1
    dynamic(w, _toks(), ll, d, final=1, hlit=286, hdist=30, cl_seq=seq, cl_lens=cl)


def _i_rep16_first(w):
    """a repeat of the previous length (symbol 16) as the very first code length: the first six lengths are zero, so a
    decoder that took 'the previous length' to be 0 there would read an otherwise perfect header"""
    ll_need, d_need = _need(_toks())
    ll = kraft_complete(286, {}, ll_need, spare=range(6, 286))
    d = kraft_complete(30, {}, d_need, spare=range(30))
    assert ll[:6] == [0] * 6
    dynamic(w, _toks(), ll, d, final=1, hlit=286, hdist=30, cl_seq=[(16, 3)] + cl_rle(ll[6:] + d))


def _i_rep_past_end(w):
    """a run of zeros (symbol 18) that goes past HLIT + HDIST"""
    ll, d = _ordinary_lens(_toks())
    seq = cl_rle(ll + d)
    covered = lambda q: sum(1 if s < 16 else x + (3 if s < 18 else 11) for s, x in q)
    while covered(seq) > len(ll + d) - 100:
        seq.pop()
    seq.append((18, 127))                              # 138 zeros where fewer than 138 lengths are left
    dynamic(w, _toks(), ll, d, final=1, hlit=286, hdist=30, cl_seq=seq)


def _i_rep16_past_end(w):
    """a repeat (symbol 16) whose count goes past HLIT + HDIST by one"""
    ll, d = _ordinary_lens(_toks())
    d = [5] * 30
    d[0] = d[1] = 4
    seq = cl_rle(ll) + [(4, 0), (4, 0)] + [(5, 0)] + [(16, 3)] * 4 + [(16, 2)]   # 28 lengths of 5 wanted, 1 + 24 + 5 = 30 given
    dynamic(w, _toks(), ll, d, final=1, hlit=286, hdist=30, cl_seq=seq)


def _i_no_eob(w):
    """END_BLOCK with code length 0"""
    ll, d = _ordinary_lens(_toks())
    free = next(s for s in range(256) if ll[s] == 0)
    ll[free], ll[256] = ll[256], 0                  # the same code space, END_BLOCK's code given to an unused literal
    dynamic(w, _toks(), ll, d, final=1, eob=False)
    w.bits(0, 16)


def _i_fixed_sym(sym):
    def build(w):
        fixed(w, _lits(b"hello") + [("L", sym)] + _lits(b"world"), final=1)
    build.__doc__ = "literal/length symbol %d in a fixed block" % sym
    return build


def _i_fixed_dist(dsym):
    def build(w):
        fixed(w, _lits(b"hello world") + [("S", 258, 0, dsym, 0)] + _lits(b"!"), final=1)
    build.__doc__ = "distance symbol %d in a fixed block" % dsym
    return build


def _i_match_no_dist(w):
    """a match in a block whose distance tree is empty"""
    toks = _lits(b"abcdefgh")
    ll_need, _ = _need(toks + [("L", 258)])
    dynamic(w, toks + [("L", 258), ("B", 0, 16)], kraft_complete(286, {}, ll_need, spare=range(286)), [0], final=1, eob=False)


def _i_dist_missing_code(w):
    """the distance tree is one 1-bit code for symbol 0; the stream uses the other bit pattern"""
    toks = _lits(b"abcdefgh") + [(4, 1)]
    ll_need, _ = _need(toks + [("L", 258)])
    ll = kraft_complete(286, {}, ll_need, spare=range(286))
    llc = canonical(ll)
    dynamic(w, toks, ll, [1], eob=False)
    w.code(*llc[258])
    w.bits(1, 1)                                       # distance code '1': no symbol
    w.code(*llc[256])
    fixed(w, _lits(b"xyz"), final=1)


def _i_stored_nlen(w):
    """a stored block whose NLEN is not the complement of LEN"""
    fixed(w, _lits(b"before"))
    stored(w, b"0123456789", final=1, nlen=(10 ^ 0xffff) ^ 0x100)


def _i_btype3(w):
    """block type 3 (reserved)"""
    fixed(w, _lits(b"before"))
    w.bits(1, 1)
    w.bits(3, 2)
    w.bits(0, 16)


def _i_too_far(w):
    """a distance that reaches before the start of the stream"""
    fixed(w, _lits(b"0123456789") + [(5, 11)], final=1)


INVALID = {
    "hlit_287": _i_hlit,
    "hdist_31": _i_hdist,
    "litlen_incomplete": _i_ll_incomplete,
    "litlen_oversubscribed": _i_ll_oversub,
    "dist_oversubscribed": _i_d_oversub,
    "dist_incomplete_2bit": _i_d_incomplete,
    "codelen_code_incomplete": _i_cl_incomplete,
    "codelen_code_oversubscribed": _i_cl_oversub,
    "rep16_first": _i_rep16_first,
    "rep18_past_end": _i_rep_past_end,
    "rep16_past_end": _i_rep16_past_end,
    "end_block_without_code": _i_no_eob,
    "fixed_symbol_286": _i_fixed_sym(286),
    "fixed_symbol_287": _i_fixed_sym(287),
    "fixed_distance_30": _i_fixed_dist(30),
    "fixed_distance_31": _i_fixed_dist(31),
    "match_without_distance_tree": _i_match_no_dist,
    "distance_code_missing": _i_dist_missing_code,
    "stored_nlen_mismatch": _i_stored_nlen,
    "block_type_3": _i_btype3,
    "distance_too_far": _i_too_far,
}


def build_case(fn, prefix=0, phase=None):
    """the stream of one case: alone (prefix = 0), or after `prefix` bytes of ordinary content (a dynamic block of a greedy
    parse) with the case's first block starting at bit `phase` (mod 8).  -> bytes"""
    w = BitWriter()
    if prefix:
        w = _prefix_writer(prefix).copy()
        phase_block(w, phase or 0)
        assert w.bitpos % 8 == (phase or 0) % 8
    fn(w)
    return w.getvalue()


FINAL_ONLY = {"stored_0_and_65535", "bfinal_then_trailing_bytes"}    # their last block must stay the stream's last one
LONE_ONLY = {"distance_too_far"}                                         # valid once there is history before it


def build_member(fn, case_out, nseg=8, where=None):
    """a multi-segment member: nseg segments of seg_out bytes of output each, every one >= 20 KB of ordinary content, the
    case at bit phase k in segment k (only in the segments of `where`, when given; only in the last one for FINAL_ONLY
    cases), stored bytes to fill the segment, a sync-flush marker (no match crosses one), BFINAL in the last segment.
    case_out: the case's output length.  -> (stream, seg_out)"""
    final_only = fn in [VALID.get(k) for k in FINAL_ONLY]
    seg_out = (20480 + 16 + case_out + 4095) // 4096 * 4096
    base = _prefix_writer(20480)
    parts = []
    for k in range(nseg):
        last = k == nseg - 1
        w = base.copy()
        out = 20480 + phase_block(w, k % 8)
        with_case = (where is None or k in where) and (not final_only or last)
        if with_case:
            w.allow_final = last and final_only
            fn(w)
            out += case_out
            w.allow_final = True
            if final_only:
                parts.append(w.getvalue())
                break
        while out < seg_out:
            piece = min(65535, seg_out - out)
            stored(w, bytes((out + i) * 7 & 0xff for i in range(piece)))
            out += piece
        if last:
            stored(w, b"", final=1)
        else:
            sync_flush(w)
        parts.append(w.getvalue())
    return b"".join(parts), seg_out


_PREFIX = {}


def _prefix_writer(n):
    """a writer holding n bytes of ordinary content in one dynamic block (cached; callers copy it)"""
    if n not in _PREFIX:
        w = BitWriter()
        ordinary_block(w, content_tokens(n)[1])
        _PREFIX[n] = w
    return _PREFIX[n]


def reference(comp):
    """zlib's verdict on a raw stream: (ok, bytes, in_used) - in_used counts the bytes up to the end of the BFINAL block"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(comp)
        out += d.flush()
    except zlib.error:
        return False, None, None
    if not d.eof:
        return False, None, None
    return True, out, len(comp) - len(d.unused_data)


def match3_segment(out_len, final=0):
    """a segment of out_len bytes made of one fixed-code block of nothing but length-3 matches (12 bits each: no lane that
    starts off a symbol boundary falls into step), then a sync-flush marker or, with final, BFINAL.  -> bytes"""
    w = BitWriter()
    n3, rest = divmod(out_len - 3, 3)
    fixed(w, [0x61, 0x62, 0x63] + [(3, 3)] * n3 + [0x64] * rest, final=final)
    if not final:
        sync_flush(w)
    return w.getvalue()
