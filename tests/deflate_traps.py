"""Trap inputs for the deflate compressors: small inputs built from zlib 1.2.11's own rules (memLevel 9) so that each one
makes the parse or the Huffman stage take one particular decision, and a reader of raw deflate that shows the decision.

The natural corpora (datagen.KINDS) seldom reach the rules the kernels restate rather than copy: the chain budget, nice
and the speculative compare cap, MAX_DIST for the first and for deeper candidates, NIL at the window origin and after a
slide, skipped insertions at the greedy levels, the lazy evaluation's good / lazy / TOO_FAR rules, the 32767-symbol
block cut, forced distance codes, depth-limited trees and the stored / fixed / dynamic choice.

Every case names the decision it aims at (`check`), evaluated on zlib's own output by tests/test_sim_deflate_traps.py:
a case whose decision zlib does not show is dead and fails that test.  The expected bytes of every case are libz's
(tests/golden/gen_traps.py -> tests/golden/traps.json).  Pure Python + numpy; every random choice is a fixed seed.
"""
import heapq
import zlib

import numpy as np

# zlib 1.2.11 configuration_table: (good, lazy, nice, chain) per level; levels 1-3 are deflate_fast (lazy = max_insert)
CFG = {1: (4, 4, 8, 4), 2: (4, 5, 16, 8), 3: (4, 6, 32, 32), 4: (4, 4, 16, 16), 5: (8, 16, 32, 32),
       6: (8, 16, 128, 128), 7: (8, 32, 128, 256), 8: (32, 128, 258, 1024), 9: (32, 258, 258, 4096)}
MAX_DIST = 32768 - 262
SLIDE_AT = 32768 + MAX_DIST           # fill_window slides once strstart >= wsize + MAX_DIST (and lookahead < 262)
LIT_BUFSIZE = 1 << (9 + 6)            # a block is cut after lit_bufsize - 1 = 32767 symbols
TOO_FAR = 4096
GREEDY, LAZY, ALL = (1, 2, 3), (4, 5, 6, 7, 8, 9), tuple(range(1, 10))


def zhash(b0, b1, b2):
    return ((b0 << 12) ^ (b1 << 6) ^ b2) & 0xffff


def hashes(buf):
    a = np.frombuffer(bytes(buf), np.uint8).astype(np.uint32)
    if len(a) < 3:
        return np.zeros(0, np.uint32)
    return ((a[:-2] << 12) ^ (a[1:-1] << 6) ^ a[2:]) & 0xffff


# ------------------------------------------------------------------------------------------------ raw deflate reader
LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
         6145, 8193, 12289, 16385, 24577)
DEXT = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def _decoder(lens):
    """canonical code -> {(length, code): symbol}"""
    cnt = [0] * 16
    for n in lens:
        cnt[n] += 1
    cnt[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + cnt[b - 1]) << 1
        nxt[b] = code
    tab = {}
    for s, n in enumerate(lens):
        if n:
            tab[(n, nxt[n])] = s
            nxt[n] += 1
    return tab


class Block:
    """one block: btype (0 stored, 1 fixed, 2 dynamic), its first output position, and for fixed / dynamic blocks the
    code lengths (ll, d, cl) and the symbols: (pos, literal byte) or (pos, length, distance), EOB not counted"""
    def __init__(self, btype, final, start):
        self.btype, self.final, self.start = btype, final, start
        self.ll = self.d = self.cl = None
        self.syms = []
        self.stored_len = 0


def read_raw(data):
    """-> (output bytes, [Block]) of a raw deflate stream (any number of blocks; stops after BFINAL or at the end)"""
    pos_bit = [0]
    nbits = len(data) * 8

    def bits(k):
        v = 0
        for i in range(k):
            b = pos_bit[0]
            if b >= nbits:
                raise ValueError("truncated")
            v |= ((data[b >> 3] >> (b & 7)) & 1) << i
            pos_bit[0] = b + 1
        return v

    def sym(tab):
        code = n = 0
        while n < 16:
            code = (code << 1) | bits(1)
            n += 1
            s = tab.get((n, code))
            if s is not None:
                return s
        raise ValueError("bad code")

    out = bytearray()
    blocks = []
    while pos_bit[0] + 3 <= nbits:
        final = bits(1)
        bt = bits(2)
        blk = Block(bt, final, len(out))
        blocks.append(blk)
        if bt == 0:
            pos_bit[0] = (pos_bit[0] + 7) & ~7
            ln = bits(16)
            assert bits(16) == ln ^ 0xffff
            s = pos_bit[0] >> 3
            out += data[s:s + ln]
            pos_bit[0] += 8 * ln
            blk.stored_len = ln
        else:
            if bt == 1:
                ll = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
                dl = [5] * 30
            elif bt == 2:
                hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[CL_ORDER[i]] = bits(3)
                blk.cl = cl
                ct = _decoder(cl)
                seq = []
                while len(seq) < hlit + hdist:
                    c = sym(ct)
                    if c < 16:
                        seq.append(c)
                    elif c == 16:
                        seq += [seq[-1]] * (3 + bits(2))
                    elif c == 17:
                        seq += [0] * (3 + bits(3))
                    else:
                        seq += [0] * (11 + bits(7))
                ll, dl = seq[:hlit] + [0] * (288 - hlit), seq[hlit:] + [0] * (30 - hdist)
            else:
                raise ValueError("btype 3")
            blk.ll, blk.d = ll, dl
            lt, dt = _decoder(ll), _decoder(dl)
            while True:
                s = sym(lt)
                if s < 256:
                    blk.syms.append((len(out), s))
                    out.append(s)
                elif s == 256:
                    break
                else:
                    k = s - 257
                    ln = LBASE[k] + bits(LEXT[k])
                    dc = sym(dt)
                    d = DBASE[dc] + bits(DEXT[dc])
                    blk.syms.append((len(out), ln, d))
                    for _ in range(ln):
                        out.append(out[-d])
        if final:
            break
    return bytes(out), blocks


class Parse:
    """what zlib decided, indexed by input position"""
    def __init__(self, blocks):
        self.blocks = blocks
        self.at = {}
        for b in blocks:
            for s in b.syms:
                self.at[s[0]] = s
        self.coded = [b for b in blocks if b.btype]

    def lit(self, p):
        s = self.at.get(p)
        return s is not None and len(s) == 2

    def match(self, p, ln=None, dist=None):
        s = self.at.get(p)
        return s is not None and len(s) == 3 and (ln is None or s[1] == ln) and (dist is None or s[2] == dist)

    def matches(self):
        return [s for b in self.blocks for s in b.syms if len(s) == 3]

    def types(self):
        return [b.btype for b in self.blocks if not (b.btype == 0 and b.stored_len == 0)]


def unconstrained_depth(freqs):
    """depth of an unlimited Huffman tree over the nonzero frequencies"""
    h = [(f, 0, i) for i, f in enumerate(freqs) if f]
    if len(h) < 2:
        return len(h)
    heapq.heapify(h)
    k = len(freqs)
    while len(h) > 1:
        f1, d1, _ = heapq.heappop(h)
        f2, d2, _ = heapq.heappop(h)
        heapq.heappush(h, (f1 + f2, max(d1, d2) + 1, k))
        k += 1
    return h[0][1]


def block_freqs(blk):
    ll, dd = [0] * 286, [0] * 30
    ll[256] = 1
    for s in blk.syms:
        if len(s) == 2:
            ll[s[1]] += 1
        else:
            n = s[1]
            ll[257 + (28 if n == 258 else max(i for i in range(28) if LBASE[i] <= n))] += 1
            dd[max(i for i in range(30) if DBASE[i] <= s[2])] += 1
    return ll, dd


def zlib_parse(data, level, hw, last=1):
    """zlib's own stream for the case, read back (the liveness checks look at this)"""
    import refcalls as R
    raw = b"".join(R.raw_chunks(data, hw, level, last))
    out, blocks = read_raw(raw)
    assert out == data
    return Parse(blocks)


# ------------------------------------------------------------------------------------------------ input building
class Buf:
    """an input under construction: filler bytes whose 3-grams never repeat (and never meet a planted string's hash),
    planted strings at chosen positions.  The filler's small alphabet keeps its blocks Huffman-coded (not stored), so
    that the symbols at the trap are visible."""
    def __init__(self, seed, alphabet=64):
        self.rng = np.random.RandomState((seed * 2654435761 + 12345) % (1 << 32))     # not the case's own stream
        self.b = bytearray()
        self.alpha = alphabet
        self.seen = set()           # 3-grams present so far
        self.reserved = set()       # hashes that filler must not produce

    def __len__(self):
        return len(self.b)

    def _ok(self, tri):
        return tri not in self.seen and zhash(*tri) not in self.reserved

    def fill(self, n):
        for _ in range(n):
            for _t in range(64):
                c = int(self.rng.randint(self.alpha))
                if len(self.b) < 2 or self._ok((self.b[-2], self.b[-1], c)):
                    break
            else:
                # every follower of these two bytes is taken (hundreds of identical decoys): repeat a 3-gram, never a
                # reserved hash
                for _t in range(256):
                    c = int(self.rng.randint(self.alpha))
                    if zhash(self.b[-2], self.b[-1], c) not in self.reserved:
                        break
            self.b.append(c)
            if len(self.b) >= 3:
                self.seen.add(tuple(self.b[-3:]))
        return self

    def pad_to(self, n):
        return self.fill(n - len(self.b))

    def put(self, s):
        """plant s; the 3-grams it makes are remembered so that filler never repeats them"""
        for c in s:
            self.b.append(c)
            if len(self.b) >= 3:
                self.seen.add(tuple(self.b[-3:]))
        return len(self.b) - len(s)

    def sep(self):
        """one filler byte that also keeps the previous planted string from extending into what follows"""
        return self.fill(1)

    def bytes(self):
        return bytes(self.b)


def same_hash(tri, k):
    """a 3-gram with tri's hash that matches it in 0 bytes (k-th variant: b0's high nibble) or 1 byte"""
    b0, b1, b2 = tri
    if k >= 0:
        return bytes([(b0 & 15) | (((b0 >> 4) + 1 + k) % 16 << 4) if ((b0 >> 4) + 1 + k) % 16 != b0 >> 4 else (b0 ^ 0x80), b1, b2])
    return bytes([b0, b1 ^ 1, b2 ^ 0x40])


# Seeded search: the few cases whose first seed's filler happened to disturb the trap (a repeated 3-gram next to it, a
# parse point moved by a match) take the n-th seed after it.  Found once against libz 1.2.11, fixed here.
SALT = {
    "f1_chain_l1_zero_d3_ph52": 1, "f1_chain_l1_zero_d3_ph53": 1, "f1_chain_l1_zero_d5_ph58": 1,
    "f1_chain_l2_short_d8_ph0": 2, "f1_chain_l3_short_d31_ph0": 3, "f1_chain_l3_short_d33_ph0": 7, "f1_chain_l8_one_d1023_ph0": 1,
    "f1_chain_l8_zero_d1023_ph0": 1, "f2_cascade_l1_ph600": 2, "f2_cascade_l2_ph0": 1, "f2_cascade_l2_ph200": 1,
    "f2_cascade_l2_ph600": 4, "f2_cascade_l3_ph1000": 3, "f3_interior_m4_ph0": 1, "f3_interior_m8_ph45": 1,
    "f3_win_r4_o3_m4": 1, "f3_win_r6_o0_m4": 2, "f3_win_r6_o1_m4": 1, "f3_win_r6_o3_m6": 1, "f3_win_r6_o4_m6": 1,
    "f3_win_r8_o0_m4": 1, "f3_win_r8_o0_m6": 1, "f3_win_r8_o1_m4": 1, "f3_win_r8_o1_m6": 1, "f3_win_r8_o2_m4": 2,
    "f3_win_r8_o3_m4": 2, "f3_win_r8_o4_m4": 1, "f4_clip_l2_a17_far": 6, "f4_clip_l2_a4_near": 1,
    "f4_clip_l9_a3_far": 1, "f4_nice_l9_n257": 1, "f5_exact0_k17": 1, "f5_first_l1_d32506": 1, "f6_maxlazy_l7_p32": 1,
    "f6_stairs_l5_k14_s3": 1, "f6_tie_l5_x0": 1, "f6_tie_l9_x0": 1, "f6_toofar_l6_d4095": 1
}


def _s(seed, name):
    return seed + 7777 * SALT.get(name, 0)


class Case:
    def __init__(self, name, family, levels, data, check, hw=65536, last=(1,), aim=""):
        self.name, self.family, self.levels, self.data = name, family, tuple(levels), bytes(data)
        self.check, self.hw, self.last, self.aim = check, hw, tuple(last), aim

    def __repr__(self):
        return "Case(%s, %d B, levels %s)" % (self.name, len(self.data), self.levels)


def _tail(rng, n, avoid=b""):
    while True:
        t = bytes(rng.randint(0, 256, n).astype(np.uint8))
        if not avoid or t[0] != avoid[0]:
            return t


# ---------------------------------------------------------------- F1 chain budget
def _short_len(i, nice, d):
    """the i-th short decoy's match length: 3 .. min(nice - 1, 11), 3 or 4 for the long chains (they must fit MAX_DIST)"""
    top = min(nice - 1, 11) if d < 2000 else 4
    return 3 + i % (top - 2)


def f1_chain():
    cases = []
    for level in ALL:
        chain = CFG[level][3]
        phases = range(64) if level == 1 else (0,)
        kinds = ("zero",) if level == 1 else ("zero", "one", "short")
        nice = CFG[level][2]
        for kind in kinds:
            for d in (chain - 1, chain, chain + 1):
                if kind == "short" and d == chain - 1 and level in (7, 8):
                    continue            # (no seed found where the short decoys' own matches leave this one alone)
                for ph in phases:
                    seed = _s(1000 * level + 10 * d + ph + (0 if kind == "zero" else 7 if kind == "one" else 13), "f1_chain_l%d_%s_d%d_ph%d" % (level, kind, d, ph))
                    rng = np.random.RandomState(seed)
                    B = Buf(seed)
                    T = bytes([0x21 + (seed % 90), 0x5a, 0x33]) + _tail(rng, 9)
                    th = zhash(*T[:3])
                    B.reserved.add(th)
                    B.fill(8 + ph)
                    real = B.put(T); B.sep()
                    # decoys: newer than the real string, same hash as T's first 3-gram
                    step = 3 if d > 2000 else 4
                    for i in range(d):
                        if kind == "short":
                            k = _short_len(i, nice, d)
                            B.put(T[:k] + bytes([T[k] ^ 0xff]))
                        else:
                            B.put(same_hash(T[:3], i % 14 if kind == "zero" else -1))
                        B.fill(step - 1 if kind != "short" else 1)
                    B.fill(5)
                    P = B.put(T)
                    B.fill(6)
                    data = B.bytes()
                    if P - real > MAX_DIST:
                        raise RuntimeError("chain trap too long")
                    if d < chain:
                        chk = (lambda P, real: lambda z, lv: z.match(P, 12, P - real))(P, real)
                        aim = "real match found as the %d-th candidate" % (d + 1)
                    elif kind == "short":
                        chk = (lambda P, real: lambda z, lv: not z.match(P, 12, P - real))(P, real)
                        aim = "real match beyond the chain budget: not taken (a decoy's or the next position's)"
                    else:
                        chk = (lambda P: lambda z, lv: z.lit(P))(P)
                        aim = "real match beyond the chain budget: literal"
                    cases.append(Case("f1_chain_l%d_%s_d%d_ph%d" % (level, kind, d, ph), "F1", [level], data, chk, aim=aim))
    return cases


# ---------------------------------------------------------------- F2 skipped insertions (greedy levels)
def _stage(B, rng, L, j, avoid_first=True):
    """x: A + u1 ; y: A + u2 (match of exactly L) ; z: A[j:] + u2 + more.  Returns (x, y, z)."""
    A = bytes(rng.randint(0, 256, L).astype(np.uint8))
    u1 = _tail(rng, 6)
    u2 = _tail(rng, 6, avoid=u1)
    x = B.put(A + u1); B.fill(3)
    y = B.put(A + u2); B.fill(3)
    z = B.put(A[j:] + u2 + _tail(rng, 2)); B.fill(3)
    return x, y, z


def f2_insert():
    cases = []
    for level in GREEDY:
        mi = CFG[level][1]
        for L in (mi, mi + 1):
            for j in range(1, L - 1 + 1):
                seed = _s(2000 + 100 * level + 10 * L + j, "f2_ins_l%d_L%d_j%d" % (level, L, j))
                rng = np.random.RandomState(seed)
                B = Buf(seed)
                B.fill(20)
                x, y, z = _stage(B, rng, L, j)
                B.fill(10)
                if L <= mi:
                    chk = (lambda y, z, j: lambda zz, lv: zz.match(y, None) and zz.match(z, None, z - (y + j)))(y, z, j)
                    aim = "interior of a %d-byte match inserted: best candidate inside it" % L
                elif j >= L - 2:
                    chk = (lambda y, z: lambda zz, lv: zz.match(y) and zz.lit(z))(y, z)
                    aim = "interior of a %d-byte match skipped: the only candidate is not in the table" % L
                else:
                    chk = (lambda x, y, z, j: lambda zz, lv: zz.match(y) and zz.match(z, None, z - (x + j)))(x, y, z, j)
                    aim = "interior skipped: the older, shorter candidate"
                cases.append(Case("f2_ins_l%d_L%d_j%d" % (level, L, j), "F2", [level], B.bytes(), chk, aim=aim))
        # a match ending one or two bytes before the end of the chunk (avail - mlen < 3: no insertion)
        for e in (0, 1, 2, 3):
            for L in (mi, mi + 1, 10):
                seed = _s(2500 + 10 * level + e + 100 * L, "f2_end_l%d_L%d_e%d" % (level, L, e))
                rng = np.random.RandomState(seed)
                B = Buf(seed)
                A = bytes(rng.randint(0, 256, L).astype(np.uint8))
                B.fill(30)
                B.put(A); B.fill(40)
                y = B.put(A)
                B.fill(e)
                chk = (lambda y, L: lambda zz, lv: zz.match(y, L))(y, L)
                cases.append(Case("f2_end_l%d_L%d_e%d" % (level, L, e), "F2", [level], B.bytes(), chk,
                                  aim="a %d-byte match ends %d bytes before the chunk end" % (L, e)))
        # many stages packed into one 1024-position window and across its edge (each stage's decision rests on its own
        # match only: the stages share windows, not a dependency chain)
        for ph in (0, 200, 600, 1000):
            seed = _s(2900 + 10 * level + ph, "f2_cascade_l%d_ph%d" % (level, ph))
            rng = np.random.RandomState(seed)
            B = Buf(seed)
            B.fill(ph + 1)
            stages = []
            while len(B) < ph + 1400:
                L = mi + int(rng.randint(2))
                j = 1 + int(rng.randint(L - 1))
                stages.append((L, j) + _stage(B, rng, L, j))

            def chk(zz, lv, stages=stages, mi=mi):
                for L, j, x, y, z in stages:
                    if not zz.match(y):
                        return False
                    if L <= mi and not zz.match(z, None, z - (y + j)):
                        return False
                    if L > mi and not (zz.lit(z) if j >= L - 2 else zz.match(z, None, z - (x + j))):
                        return False
                return True
            cases.append(Case("f2_cascade_l%d_ph%d" % (level, ph), "F2", [level], B.bytes(), chk,
                              aim="%d insertion decisions packed into 1024-position windows" % len(stages)))
    return cases


# ---------------------------------------------------------------- F3 one hash several times in one window
def _key_mates(h, rng):
    """3-grams whose hash differs from h but shares K1's three slot-table keys, one per table"""
    want = [lambda g: g & 255 == h & 255, lambda g: g >> 8 == h >> 8, lambda g: ((g * 40503) >> 12) & 127 == ((h * 40503) >> 12) & 127]
    out = []
    for w in want:
        while True:
            t = tuple(int(v) for v in rng.randint(0, 256, 3))
            g = zhash(*t)
            if g != h and w(g):
                out.append(bytes(t))
                break
    return out


def f3_window():
    cases = []
    for reps in (2, 3, 4, 6, 8):
        for order in range(6):
            for mlen in (4, 6):
                seed = _s(3000 + 100 * reps + 10 * order + mlen, "f3_win_r%d_o%d_m%d" % (reps, order, mlen))
                rng = np.random.RandomState(seed)
                B = Buf(seed)
                G = bytes(rng.randint(0, 256, 3).astype(np.uint8))
                h = zhash(*G)
                mates = _key_mates(h, rng)
                perm = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)][order]
                B.reserved.add(h)
                for m in mates:
                    B.reserved.add(zhash(*m))
                B.fill(5 + order * 7)
                tail = bytes(rng.randint(0, 256, mlen - 3).astype(np.uint8))
                occ = []
                for r in range(reps):
                    occ.append(B.put(G + tail))
                    B.fill(1)
                    for k in perm[:1 + r % 3]:
                        B.put(mates[k]); B.fill(1 + (r + k) % 2)
                B.fill(8)

                def chk(zz, lv, occ=occ, mlen=mlen):
                    return zz.lit(occ[0]) and all(zz.match(occ[i], mlen, occ[i] - occ[i - 1]) for i in range(1, len(occ)))
                cases.append(Case("f3_win_r%d_o%d_m%d" % (reps, order, mlen), "F3", [1], B.bytes(), chk,
                                  aim="a hash %d times in one window between its slot-table mates" % reps))
    # a hash recurring inside the interiors of short (<= 4) and long (> 4) matches
    for mlen in (4, 5, 8):
        for ph in range(0, 64, 9):
            seed = _s(3500 + 100 * mlen + ph, "f3_interior_m%d_ph%d" % (mlen, ph))
            rng = np.random.RandomState(seed)
            B = Buf(seed)
            M = bytes(rng.randint(0, 256, mlen).astype(np.uint8))
            B.fill(10 + ph)
            B.put(M); B.fill(4)
            y = B.put(M); B.fill(2)
            # the 3-gram M[1:4] recurs: its candidates are M's first copy and (if inserted) the interior of the match at y
            z = B.put(M[1:4] + bytes([rng.randint(256)])); B.fill(6)
            inserted = mlen <= 4
            chk = (lambda y, z, ins, mlen: lambda zz, lv: zz.match(y, mlen) and zz.match(z, 3, z - (y + 1) if ins else None)
                   and (ins or zz.at[z][2] != z - (y + 1)))(y, z, inserted, mlen)
            cases.append(Case("f3_interior_m%d_ph%d" % (mlen, ph), "F3", [1], B.bytes(), chk,
                              aim="a string whose newest candidate is a %s match interior" % ("inserted" if inserted else "skipped")))
    return cases


# ---------------------------------------------------------------- F4 nice and cap
def f4_nice():
    cases = []
    for level in ALL:
        nice = CFG[level][2]
        for near in (nice, nice - 1):
            seed = _s(4000 + 10 * level + (near == nice), "f4_nice_l%d_n%d" % (level, near))
            rng = np.random.RandomState(seed)
            B = Buf(seed)
            T = bytes(rng.randint(0, 256, nice + 40).astype(np.uint8))
            full = min(nice + 20, 258)
            B.fill(12)
            far = B.put(T[:full] + bytes([T[full] ^ 0x55])); B.fill(5)
            nr = B.put(T[:near] + bytes([T[near] ^ 0x55])); B.fill(5)
            P = B.put(T[:full + 10]); B.fill(8)
            if near == nice:
                chk = (lambda P, nr, nice: lambda zz, lv: zz.match(P, nice, P - nr))(P, nr, nice)
                aim = "a candidate of exactly nice stops the search"
            else:
                chk = (lambda P, far, full: lambda zz, lv: zz.match(P, full, P - far))(P, far, full)
                aim = "nice - 1 does not stop the search: the longer, older candidate"
            cases.append(Case("f4_nice_l%d_n%d" % (level, near), "F4", [level], B.bytes(), chk, aim=aim))
        # lengths around the speculative compare cap (16) and 258
        for L in (15, 16, 17, 18, 31, 32, 33, 257, 258, 259):
            seed = _s(4100 + 1000 * level + L, "f4_len_l%d_L%d" % (level, L))
            rng = np.random.RandomState(seed)
            B = Buf(seed)
            T = bytes(rng.randint(0, 256, L).astype(np.uint8))
            B.fill(9)
            B.put(T + bytes([rng.randint(256)])); B.fill(7)
            P = B.put(T); B.fill(9)
            chk = (lambda P, L: lambda zz, lv: zz.match(P, min(L, 258)))(P, L)
            cases.append(Case("f4_len_l%d_L%d" % (level, L), "F4", [level], B.bytes(), chk, aim="a match of exactly %d" % L))
        # runs of 258 + 1, 2, 3 bytes after the run's first byte
        for k in (1, 2, 3, 4):
            seed = 4200 + 10 * level + k
            B = Buf(seed)
            B.fill(11)
            r = B.put(bytes([0x41]) * (1 + 258 + k))
            B.fill(6)
            # (the run's interior is not inserted at the greedy levels: a tail of 3 or more matches the run's start)
            chk = (lambda r, k: lambda zz, lv: zz.lit(r) and zz.match(r + 1, 258, 1)
                   and (zz.match(r + 259, k) if k >= 3 else zz.lit(r + 259)))(r, k)
            cases.append(Case("f4_run_l%d_k%d" % (level, k), "F4", [level], B.bytes(), chk, aim="run of 258 + %d" % k))
        # nice clipped by the lookahead at the end of the chunk
        for avail in (3, 4, 5, nice - 1, nice, nice + 1):
            if avail < 3 or avail > 258:
                continue
            for near_full in (True, False):
                seed = _s(4300 + 10 * level + avail + (500 if near_full else 0), "f4_clip_l%d_a%d_%s" % (level, avail, "near" if near_full else "far"))
                rng = np.random.RandomState(seed)
                B = Buf(seed)
                T = bytes(rng.randint(0, 256, avail).astype(np.uint8))
                B.fill(10)
                far = B.put(T + bytes([rng.randint(256)])); B.fill(4)
                nl = avail if near_full else avail - 1
                nr = B.put(T[:nl] + bytes([T[nl] ^ 0x33] if nl < avail else [rng.randint(256)])); B.fill(4)
                P = B.put(T)
                if near_full and nl >= 3:
                    exp = (avail, P - nr)
                elif not near_full and nl >= min(nice, avail):
                    exp = (nl, P - nr)                       # the nearer one already reaches nice
                else:
                    exp = (avail, P - far)
                chk = (lambda P, e: lambda zz, lv: zz.match(P, e[0], e[1]))(P, exp)
                cases.append(Case("f4_clip_l%d_a%d_%s" % (level, avail, "near" if near_full else "far"), "F4", [level], B.bytes(), chk,
                                  aim="nice clipped to the %d bytes left" % avail))
    return cases


# ---------------------------------------------------------------- F5 distances and slides
def f5_dist():
    cases = []
    for level in ALL:
        # a first candidate at MAX_DIST (found) and one byte further (not)
        for dist in (MAX_DIST - 1, MAX_DIST, MAX_DIST + 1):
            seed = _s(5000 + 10 * level + dist - MAX_DIST, "f5_first_l%d_d%d" % (level, dist))
            rng = np.random.RandomState(seed)
            B = Buf(seed)
            T = bytes(rng.randint(0, 256, 12).astype(np.uint8))
            B.reserved.add(zhash(*T[:3]))
            B.fill(20)
            x = B.put(T); B.pad_to(x + dist)
            P = B.put(T); B.fill(8)
            chk = (lambda P, dist: (lambda zz, lv: zz.match(P, 12, dist)) if dist <= MAX_DIST else (lambda zz, lv: zz.lit(P)))(P, dist)
            cases.append(Case("f5_first_l%d_d%d" % (level, dist), "F5", [level], B.bytes(), chk,
                              aim="first candidate at distance %d" % dist))
        # a deeper candidate at MAX_DIST (not found) and MAX_DIST - 1 (found), behind one same-hash decoy
        for dist in (MAX_DIST - 1, MAX_DIST):
            seed = 5100 + 10 * level + dist - MAX_DIST
            rng = np.random.RandomState(seed)
            B = Buf(seed)
            T = bytes(rng.randint(0, 256, 12).astype(np.uint8))
            B.reserved.add(zhash(*T[:3]))
            B.fill(20)
            x = B.put(T); B.pad_to(x + dist - 40)
            B.put(same_hash(T[:3], 0)); B.pad_to(x + dist)
            P = B.put(T); B.fill(8)
            chk = (lambda P, dist: (lambda zz, lv: zz.match(P, 12, dist)) if dist < MAX_DIST else (lambda zz, lv: zz.lit(P)))(P, dist)
            cases.append(Case("f5_deep_l%d_d%d" % (level, dist), "F5", [level], B.bytes(), chk,
                              aim="second candidate at distance %d" % dist))
        # K1's exact0: the table's first candidate at exactly MAX_DIST, a same-hash decoy k bytes back (an earlier lane of
        # the same 64-position window for most k) in front of it - now the MAX_DIST one is second in zlib's chain: not taken
        if level == 1:
            for k in (2, 5, 9, 17, 26, 38, 50, 61):
                seed = _s(5150 + k, "f5_exact0_k%d" % k)
                rng = np.random.RandomState(seed)
                B = Buf(seed)
                T = bytes(rng.randint(0, 256, 12).astype(np.uint8))
                B.reserved.add(zhash(*T[:3]))
                B.fill(20)
                x = B.put(T); B.pad_to(x + MAX_DIST - k)
                B.put(same_hash(T[:3], 0)); B.pad_to(x + MAX_DIST)
                P = B.put(T); B.fill(8)
                chk = (lambda P: lambda zz, lv: zz.lit(P))(P)
                cases.append(Case("f5_exact0_k%d" % k, "F5", [1], B.bytes(), chk,
                                  aim="candidate at MAX_DIST behind a decoy %d back: not taken" % k))
        # NIL: the only candidate at chunk offset 0 (and at 1, found)
        for at in (0, 1):
            seed = 5200 + 10 * level + at
            rng = np.random.RandomState(seed)
            B = Buf(seed)
            T = bytes(rng.randint(0, 256, 10).astype(np.uint8))
            B.reserved.add(zhash(*T[:3]))
            B.fill(at)
            x = B.put(T); B.fill(50)
            P = B.put(T); B.fill(5)
            chk = (lambda P, x: (lambda zz, lv: zz.lit(P)) if x == 0 else (lambda zz, lv: zz.match(P, 10, P - x)))(P, x)
            cases.append(Case("f5_nil_l%d_at%d" % (level, at), "F5", [level], B.bytes(), chk, aim="only candidate at offset %d" % at))
    # the window slide (hw 131072): chunk sizes around 65536 with a candidate found across the slide (U, re-based), and a
    # string T whose only candidate straddles chunk offset 32768 - window position 0 after the slide.  (zlib's NIL at
    # position 0 cannot show on its own there: every parse point after the slide lies more than MAX_DIST past it, so
    # T's literal shows the distance rule; the NIL rule at the origin is f5_nil.)  Then matches straddling the slide.
    for extra in (0, 1, 261, 262, 263):
        for level in (1, 3, 6, 9):
            seed = _s(5300 + extra + 7 * level, "f5_slide_l%d_n%d" % (level, 65536 + extra))
            rng = np.random.RandomState(seed)
            B = Buf(seed)
            T = bytes(rng.randint(0, 256, 14).astype(np.uint8))
            U = bytes(rng.randint(0, 256, 14).astype(np.uint8))
            B.reserved.update((zhash(*T[:3]), zhash(*U[:3])))
            B.fill(32768 - 5)
            x0 = B.put(T)                      # straddles chunk offset 32768
            B.fill(20000)
            u = B.put(U)
            n = 65536 + extra
            B.pad_to(n - 40)
            pt = B.put(T); B.fill(5)
            pu = B.put(U)
            B.pad_to(n)
            data = B.bytes()[:n]

            def chk(zz, lv, pt=pt, pu=pu, u=u):
                return zz.lit(pt) and zz.match(pu, None, pu - u)
            cases.append(Case("f5_slide_l%d_n%d" % (level, n), "F5", [level], data, chk, hw=131072,
                              aim="after the slide: T's candidate %d back is not taken, U's %d back is" % (pt - x0, pu - u)))
    for P0 in (SLIDE_AT - 6, SLIDE_AT - 1, SLIDE_AT, SLIDE_AT + 1, SLIDE_AT + 2):
        for level in (1, 2, 4, 8):
            seed = _s(5400 + P0 - SLIDE_AT + 20 * level, "f5_straddle_l%d_p%d" % (level, P0))
            rng = np.random.RandomState(seed)
            B = Buf(seed)
            T = bytes(rng.randint(0, 256, 20).astype(np.uint8))
            B.reserved.add(zhash(*T[:3]))
            B.fill(40000)
            x = B.put(T + bytes([rng.randint(256)]))
            B.pad_to(P0)
            P = B.put(T)
            B.fill(70000 - len(B))
            chk = (lambda P, x: lambda zz, lv: zz.match(P, 20, P - x))(P, x)
            cases.append(Case("f5_straddle_l%d_p%d" % (level, P0), "F5", [level], B.bytes(), chk, hw=131072,
                              aim="a match from parse point %d across the slide" % P0))
    # candidates on either side of K1's 4 KiB LDS ring's edge
    for dist in (4000, 4030, 4064, 4094, 4095, 4096, 4097, 4098, 4128, 4160, 4200):
        for ph in (0, 17, 41, 63):
            seed = _s(5500 + dist + 1000 * ph, "f5_ring_d%d_ph%d" % (dist, ph))
            rng = np.random.RandomState(seed)
            B = Buf(seed)
            T = bytes(rng.randint(0, 256, 24).astype(np.uint8))
            B.reserved.add(zhash(*T[:3]))
            B.fill(300 + ph)
            x = B.put(T + bytes([rng.randint(256)]))
            B.pad_to(x + dist)
            P = B.put(T); B.fill(30)
            chk = (lambda P, dist: lambda zz, lv: zz.match(P, 24, dist))(P, dist)
            cases.append(Case("f5_ring_d%d_ph%d" % (dist, ph), "F5", [1], B.bytes(), chk, aim="candidate %d back (ring edge)" % dist))
    return cases


# ---------------------------------------------------------------- F6 lazy levels
def f6_lazy():
    cases = []
    for level in LAZY:
        good, lazy, nice, chain = CFG[level]
        # TOO_FAR: a 3-byte match 4096 back is kept, 4097 back is dropped
        for dist in (TOO_FAR - 1, TOO_FAR, TOO_FAR + 1):
            seed = _s(6000 + 10 * level + dist - TOO_FAR, "f6_toofar_l%d_d%d" % (level, dist))
            rng = np.random.RandomState(seed)
            B = Buf(seed)
            T = bytes(rng.randint(0, 256, 3).astype(np.uint8))
            B.reserved.add(zhash(*T))
            B.fill(10)
            x = B.put(T); B.pad_to(x + dist)
            P = B.put(T); B.fill(8)
            chk = (lambda P, dist: (lambda zz, lv: zz.match(P, 3, dist)) if dist <= TOO_FAR else (lambda zz, lv: zz.lit(P)))(P, dist)
            cases.append(Case("f6_toofar_l%d_d%d" % (level, dist), "F6", [level], B.bytes(), chk, aim="3-byte match %d back" % dist))
        # staircases: each next position matches one byte longer
        for k0, steps in sorted({(3, 3), (5, 4), (good - 1, 3), (lazy - 2, 3)}):
            if k0 < 3 or k0 >= lazy or k0 + steps > 250:
                continue
            seed = _s(6100 + 10 * level + k0 + 1000 * steps, "f6_stairs_l%d_k%d_s%d" % (level, k0, steps))
            rng = np.random.RandomState(seed)
            B = Buf(seed)
            S = bytes(rng.randint(0, 256, k0 + 2 * steps + 8).astype(np.uint8))
            B.fill(12)
            for i in range(steps):
                B.put(S[i:i + k0 + i] + bytes([S[i + k0 + i] ^ 0x5a])); B.fill(3)
            P = B.put(S[:k0 + 2 * steps]); B.fill(8)

            def chk(zz, lv, P=P, steps=steps, k0=k0):
                firsts = [q for q in range(P, P + steps) if zz.match(q)]
                return zz.lit(P) and bool(firsts) and zz.at[firsts[0]][1] >= k0 + 1
            cases.append(Case("f6_stairs_l%d_k%d_s%d" % (level, k0, steps), "F6", [level], B.bytes(), chk, aim="lazy steps from length %d" % k0))
        # prev_length at good_match (quarter chain at the next position) and at max_lazy (no search there)
        if good < lazy:
            q = chain >> 2
            for plen, d in ((good, q), (good, q - 1), (good - 1, q)):
                seed = _s(6200 + 10 * level + plen + 3 * d, "f6_good_l%d_p%d_d%d" % (level, plen, d))
                rng = np.random.RandomState(seed)
                B = Buf(seed)
                X = bytes(rng.randint(0, 256, good + 30).astype(np.uint8))
                B.reserved.add(zhash(*X[1:4]))
                B.fill(10)
                B.put(X[:plen] + bytes([X[plen] ^ 0x77])); B.fill(3)                 # P's match: plen bytes
                e2 = B.put(X[1:good + 9] + bytes([X[good + 9] ^ 0x77])); B.fill(3)   # P+1's real match: good + 8 bytes
                for i in range(d):
                    B.put(same_hash(X[1:4], i % 14)); B.fill(2 if d > 300 else 3)
                B.fill(4)
                P = B.put(X[:good + 12]); B.fill(8)
                found = plen < good or d < q
                chk = (lambda P, e2, found, plen: (lambda zz, lv: zz.lit(P) and zz.match(P + 1, None, P + 1 - e2)) if found
                       else (lambda zz, lv: zz.match(P, plen)))(P, e2, found, plen)
                cases.append(Case("f6_good_l%d_p%d_d%d" % (level, plen, d), "F6", [level], B.bytes(), chk,
                                  aim="prev_length %d vs good %d: %d decoys at the next position" % (plen, good, d)))
        if lazy < 258:
            for plen in (lazy, lazy - 1):
                if plen < 3:
                    continue
                seed = _s(6300 + 10 * level + plen, "f6_maxlazy_l%d_p%d" % (level, plen))
                rng = np.random.RandomState(seed)
                B = Buf(seed)
                X = bytes(rng.randint(0, 256, lazy + 40).astype(np.uint8))
                B.fill(10)
                B.put(X[:plen] + bytes([X[plen] ^ 0x77])); B.fill(3)
                e2 = B.put(X[1:plen + 6] + bytes([X[plen + 6] ^ 0x77])); B.fill(3)
                P = B.put(X[:plen + 10]); B.fill(8)
                if plen >= lazy:
                    chk = (lambda P, plen: lambda zz, lv: zz.match(P, plen))(P, plen)
                else:
                    chk = (lambda P, e2: lambda zz, lv: zz.lit(P) and zz.match(P + 1, None, P + 1 - e2))(P, e2)
                cases.append(Case("f6_maxlazy_l%d_p%d" % (level, plen), "F6", [level], B.bytes(), chk,
                                  aim="prev_length %d vs max_lazy %d" % (plen, lazy)))
        # ties: the next position's match of equal length does not replace the held one; one byte longer does
        for extra in (0, 1):
            seed = _s(6400 + 10 * level + extra, "f6_tie_l%d_x%d" % (level, extra))
            rng = np.random.RandomState(seed)
            B = Buf(seed)
            L = min(lazy - 1, 6) if lazy > 4 else 3
            X = bytes(rng.randint(0, 256, L + 20).astype(np.uint8))
            B.fill(10)
            e1 = B.put(X[:L] + bytes([X[L] ^ 0x66])); B.fill(3)
            e2 = B.put(X[1:1 + L + extra] + bytes([X[1 + L + extra] ^ 0x66])); B.fill(3)
            # an equal-length, nearer twin of e1 for the same-length tie inside one search
            t1 = B.put(X[:L] + bytes([X[L] ^ 0x65])); B.fill(3)
            P = B.put(X[:L + 8]); B.fill(8)
            if extra:
                chk = (lambda P, e2: lambda zz, lv: zz.lit(P) and zz.match(P + 1, None, P + 1 - e2))(P, e2)
            else:
                chk = (lambda P, t1, L: lambda zz, lv: zz.match(P, L, P - t1))(P, t1, L)
            cases.append(Case("f6_tie_l%d_x%d" % (level, extra), "F6", [level], B.bytes(), chk,
                              aim="next match %s: ties keep the held, nearest match" % ("longer" if extra else "equal")))
    return cases


# ---------------------------------------------------------------- F7 blocks and trees
def _unique_text(n, alphabet, seed, counts=None):
    """n bytes over the first `alphabet` letters from 'a', no 3-gram twice (so: no match at all)"""
    B = Buf(seed, alphabet)
    B.fill(n)
    return bytes(c + 0x61 if alphabet <= 26 else c for c in B.b)


def f7_blocks():
    cases = []
    # chunks that parse to 32766, 32767 and 32768 symbols (literals only: the block is cut at 32767)
    for ns in (32766, 32767, 32768):
        data = _unique_text(ns, 48, 7000 + ns)
        chk = (lambda ns: lambda zz, lv: sorted(len(b.syms) for b in zz.coded if b.syms)[-1] == min(ns, 32767)
               and sum(len(b.syms) for b in zz.coded) == ns)(ns)
        cases.append(Case("f7_syms_%d" % ns, "F7", ALL, data, chk, aim="%d literal symbols: block cut at 32767" % ns))
    # literal-only blocks that still compress: zlib forces distance codes 0 and 1
    for n, a in ((1200, 14), (5000, 20), (30000, 40)):
        data = _unique_text(n, a, 7100 + n)
        chk = lambda zz, lv: any(b.btype == 2 and not any(len(s) == 3 for s in b.syms) and b.d[:2] == [1, 1] and not any(b.d[2:]) for b in zz.blocks)
        cases.append(Case("f7_nodist_%d_a%d" % (n, a), "F7", ALL, data, chk, aim="no distance code used: two forced"))
    # exactly one distance code in use: code 0 (one run, distance 1) and a code above 1 (distance 7 or 30)
    for dc, span in ((0, 1), (5, 7), (9, 30)):
        seed = 7200 + 10 * dc + span
        rng = np.random.RandomState(seed)
        B = Buf(seed, 20)
        B.fill(3000)
        if dc == 0:
            B.put(b"Z" * 100)
        else:
            pat = bytes(0x30 + int(v) for v in rng.randint(0, 10, span))
            B.put(pat * (3 if span < 10 else 2))
        B.put(b"Y")
        B.fill(2000)
        data = bytes(c + 0x61 if c < 20 else c for c in B.b)

        def chk(zz, lv, dc=dc):
            for b in zz.blocks:
                if b.btype == 2 and any(len(s) == 3 for s in b.syms):
                    used = {max(i for i in range(30) if DBASE[i] <= s[2]) for s in b.syms if len(s) == 3}
                    if used == {dc}:
                        want = {0, 1} if dc < 2 else {0, dc}
                        return {i for i, v in enumerate(b.d) if v} == want and all(b.d[i] == 1 for i in want)
            return False
        cases.append(Case("f7_onedist_c%d" % dc, "F7", ALL, data, chk, aim="one distance code (%d) in use: a second one forced" % dc))
    # exact Fibonacci counts: unconstrained depth above 15 in the distance and literal/length trees (zlib's gen_bitlen
    # overflow repair: 15-bit codes), and above 7 in the code-length tree (7-bit code-length codes)
    for which in ("dist", "len"):
        data = _fib_tree(which, 7340)

        def chk(zz, lv, which=which):
            for b in zz.coded:
                ll, dd = block_freqs(b)
                if b.btype == 2 and which == "dist" and max(b.d) == 15 and unconstrained_depth(dd) > 15:
                    return True
                if b.btype == 2 and which == "len" and max(b.ll) == 15 and unconstrained_depth(ll) > 15:
                    return True
            return False
        cases.append(Case("f7_depth_%s" % which, "F7", ALL, data, chk, aim="unconstrained %s depth above 15: 15-bit codes" % which))
    for seed in (7306, 7313):
        data = _fib_block("len", seed)
        chk = lambda zz, lv: any(b.btype == 2 and max(b.cl) == 7 and _cl_depth(b) > 7 for b in zz.blocks)
        cases.append(Case("f7_cl_deep_s%d" % seed, "F7", ALL, data, chk, hw=131072,
                          aim="unconstrained code-length depth above 7: 7-bit code-length codes"))
    # equal frequencies.  All-equal (the heap's order among equals), and literals at f and 2f: two f leaves merge into a
    # node of 2f, which ties with the 2f leaves in the heap - zlib's tie-break by depth takes the leaf first
    for a, f in ((24, 60), (40, 40), (17, 100)):
        data = _equal_freq([f] * a, 7500 + a)
        chk = (lambda: lambda zz, lv: any(b.btype == 2 and len({v for v in b.ll[:256] if v}) >= 2 for b in zz.blocks))()
        cases.append(Case("f7_equal_a%d_f%d" % (a, f), "F7", ALL, data, chk, aim="%d literals %d times each" % (a, f)))
    for a1, a2, f in ((6, 10, 40), (12, 6, 50), (3, 20, 30)):
        data = _equal_freq([f] * a1 + [2 * f] * a2, 7550 + a1)

        def chk(zz, lv, f=f):
            for b in zz.coded:
                ll, _ = block_freqs(b)
                if b.btype == 2 and ll.count(f) >= 2 and ll.count(2 * f) >= 1:
                    return True
            return False
        cases.append(Case("f7_tie_%dx%d_%dx%d" % (a1, f, a2, 2 * f), "F7", ALL, data, chk,
                          aim="leaves of 2f tie with merged pairs of f leaves: the tie-break by depth"))
    # tiny inputs: stored / fixed / dynamic decided on a few bits
    rng = np.random.RandomState(7600)
    tiny = []
    for i in range(160):
        n = 1 + int(rng.randint(600))
        if i % 4 == 3:                                     # high bytes (9-bit fixed codes): where stored wins
            a, base = 112, 144
        else:
            a = 1 + int(rng.randint(20))
            base = int(rng.randint(0, 256 - a))
        tiny.append(bytes((base + rng.randint(a, size=n)).astype(np.uint8)))
    for i, t in enumerate(tiny):
        cases.append(Case("f7_tiny_%03d" % i, "F7tiny", (1, 2, 6), t, lambda zz, lv: True, aim="block type on a few bits"))
    # blocks that start at byte 32767 / 32769 with the slide inside the block: no stored block for the first (buf == NULL)
    for start, lv in ((32767, (1, 2, 3)), (32769, (1, 2, 3))):
        seed = 7700 + start
        B = Buf(seed, 256)
        B.fill(32767 if start == 32767 else 32764)
        if start == 32769:
            t = B.b[-300:-297]
            B.put(bytes(t)); B.fill(1)                     # one 3-byte match: 32767 symbols cover 32769 bytes
        B.pad_to(100000)
        data = B.bytes()

        def chk(zz, lv, start=start):
            b2 = [b for b in zz.blocks if b.start == start]
            if not b2:
                return False
            return (b2[0].btype != 0) if start == 32767 else (b2[0].btype == 0)
        cases.append(Case("f7_slideblock_s%d" % start, "F7", lv, data, chk, hw=131072,
                          aim="random block from %d across the slide: stored %s" % (start, "ruled out" if start == 32767 else "allowed")))
    return cases


def _equal_freq(counts, seed):
    """literal i exactly counts[i] times, no 3-gram twice (so no match at all)"""
    rng = np.random.RandomState(seed)
    a = len(counts)
    for attempt in range(200):
        left = list(counts)
        out = []
        seen = set()
        ok = True
        for _ in range(sum(counts)):
            cand = [s for s in range(a) if left[s] and (len(out) < 2 or (out[-2], out[-1], s) not in seen)]
            if not cand:
                ok = False
                break
            w = np.array([left[s] for s in cand], float)
            s = cand[int(rng.choice(len(cand), p=w / w.sum()))]
            out.append(s)
            left[s] -= 1
            if len(out) >= 3:
                seen.add(tuple(out[-3:]))
        if ok:
            return bytes(0x41 + s for s in out)
    raise RuntimeError("no equal-frequency text")


def _cl_depth(b):
    """unconstrained depth of the code-length code for the block's lengths (zlib's scan_tree run rules)"""
    nl = max(257, max(i for i, v in enumerate(b.ll) if v) + 1)
    nd = max(1, max([i for i, v in enumerate(b.d) if v] + [0]) + 1)
    freq = [0] * 19
    for seq in (b.ll[:nl], b.d[:nd]):
        i = 0
        prev = -1
        while i < len(seq):
            v = seq[i]
            j = i
            while j < len(seq) and seq[j] == v:
                j += 1
            r = j - i
            if v == 0:
                while r >= 3:
                    k = min(r, 138)
                    freq[18 if k >= 11 else 17] += 1
                    r -= k
                freq[0] += r
            else:
                if v != prev:
                    freq[v] += 1
                    r -= 1
                while r >= 3:
                    freq[16] += 1
                    r -= min(r, 6)
                freq[v] += r
            prev = v
            i = j
    return unconstrained_depth(freq)


def _fib_tree(which, seed):
    """one block whose distance codes ("dist", codes 13-29) or length codes ("len", codes 0-15, with the end-of-block
    code) are used with exact Fibonacci counts 1, 1, 2, .., 1597: an unconstrained depth of 16 or more in that tree.  Between the matches: filler whose
    3-grams never repeat.  A match copies L bytes (4, or the length code's base) from a filler position whose 3-gram
    has not occurred since, at a distance drawn from the code's range, and the byte after the copy makes a 3-gram never
    seen before - so that source is the nearest longest candidate and zlib's match is exactly (L, distance) at every
    level."""
    rng = np.random.RandomState(seed)
    fib = [1, 1]
    while len(fib) < 17:
        fib.append(fib[-1] + fib[-2])
    if which == "dist":         # the most used codes in the middle of the window
        codes = [21, 20, 22, 19, 23, 18, 24, 17, 25, 16, 26, 15, 27, 14, 28, 13, 29]
    else:                       # the end-of-block code (used once) is the chain's other 1
        codes = list(range(16))
    toks = [c for i, c in enumerate(codes) for _ in range(fib[16 - i])]
    toks = [toks[i] for i in rng.permutation(len(toks))]
    if which == "dist":
        toks.sort(key=lambda c: DBASE[c] > 2048)                  # stable: the far ones once there is data that far back
    alpha = 256 if which == "dist" else 40       # few, heavy literals: they join the length codes' chain late
    out = bytearray()
    filler = bytearray()
    last3 = {}

    def push(c, is_filler):
        out.append(c); filler.append(is_filler)
        if len(out) >= 3:
            last3[bytes(out[-3:])] = len(out) - 3

    def fill(n):
        for _ in range(n):
            for _t in range(200):
                c = int(rng.randint(alpha))
                if len(out) < 2 or bytes([out[-2], out[-1], c]) not in last3:
                    break
            else:
                raise RuntimeError("filler stuck")
            push(c, 1)
    fill(2000)
    for c in toks:
        if which == "dist":
            L, lo, hi = 4, DBASE[c], min(DBASE[c] + (1 << DEXT[c]) - 1, MAX_DIST)
        else:
            L, lo, hi = LBASE[c], 64, 4000
        for _t in range(1000):
            d = int(rng.randint(lo, hi + 1))
            s0 = len(out) - d
            if s0 < 1 or d < L or not filler[s0] or last3.get(bytes(out[s0:s0 + 3])) != s0:
                continue
            a, b = out[s0], out[s0 + 1]
            if bytes([out[-2], out[-1], a]) not in last3 and bytes([out[-1], a, b]) not in last3:
                break
        else:
            raise RuntimeError("no source")
        for i in range(L):
            push(out[s0 + i], 0)
        fill(4)
    return bytes(out)


def _fib_block(which, seed):
    """one block's worth of tokens: 3 filler literals, then a match whose distance code ("dist", codes 8-24: stray long matches only add to the
    largest counts) or length code
    ("len", codes 0-16) is drawn with Fibonacci frequencies.  The copy's source is a 3-gram seen once so far, so that
    zlib's nearest longest match is that source (chains permitting)."""
    rng = np.random.RandomState(seed)
    fib = [1, 1]
    while len(fib) < 17:                 # 17 codes, 4180 matches: an unconstrained depth of 16, all in one block
        fib.append(fib[-1] + fib[-2])
    toks = [k for k in range(17) for _ in range(fib[k])]
    toks = [toks[i] for i in rng.permutation(len(toks))]
    B = Buf(seed)
    B.fill(7000)
    out = B.b
    count = {}
    done = 0

    def tally():
        nonlocal done
        for i in range(done, len(out) - 2):
            t = bytes(out[i:i + 3]); count[t] = count.get(t, 0) + 1
        done = max(done, len(out) - 2)
    for k in toks:
        B.fill(3)
        tally()
        if which == "dist":
            c = 8 + k
            ln = 4
            lo, hi = DBASE[c], DBASE[c] + (1 << DEXT[c]) - 1
        else:
            ln = LBASE[k]
            lo, hi = 300, 3000
        for _t in range(40):
            d = int(rng.randint(lo, hi + 1))
            s0 = len(out) - d
            if s0 >= 0 and d >= ln and count.get(bytes(out[s0:s0 + 3]), 0) == 1:
                break
        piece = bytes(out[s0:s0 + ln])
        B.put(piece)
        B.put(bytes([0x80 | int(rng.randint(128))]))
        tally()
    return B.bytes()


def all_cases():
    cs = f1_chain() + f2_insert() + f3_window() + f4_nice() + f5_dist() + f6_lazy() + f7_blocks()
    names = [c.name for c in cs]
    assert len(names) == len(set(names))
    return cs


FAMILIES = ("F1", "F2", "F3", "F4", "F5", "F6", "F7", "F7tiny")


def tiny_types_ok(parses):
    """the tiny inputs as a family: all three block types appear"""
    seen = set()
    for z in parses:
        seen.update(z.types())
    return seen >= {0, 1, 2}
