"""Trap inputs for the LZ4 level-1 compressors (qatzip_amd/csrc/qzk_lz4.h): inputs built so that ONE rule of liblz4 1.9.3's
LZ4_compress_fast / LZ4_compress_fast_continue decides the bytes, each with a check that reads that decision out of
liblz4's own frame.  The deflate side's tests/deflate_traps.py is the model for this file.

A trap is (name, family, data, mode, aim, check):
  mode   "block"  (n <= 65536: LZ4F_compressFrame writes one independent block) or "linked" (n > 65536: linked blocks)
  aim    one line: the decision the trap aims at
  check  predicate over the blocks parse_frame() reads from liblz4's frame: a Blk has .stored, .raw (content bytes),
         .seqs = [(literal length, match length, offset)], .last (last literals) and .at = [(position of the match in
         the frame's content, match length, offset)].  A trap whose check fails on liblz4's output tests nothing.

Everything is built on random filler (numpy's frozen RandomState, fixed seeds): filler never matches itself, so the probe
grid of a search streak is known in advance -

    probe j of a streak from ip sits at ip for j = 0, else at ip + 1 + 32 b (b + 1) + (b + 1) r, t = j - 1, b = t >> 6, r = t & 63

every probed position is inserted, a planted copy is found at the first probe whose four bytes lie inside it AND whose
source word was itself probed, and the backward extension walks to the copy's first byte.  model() restates the parser
serially (table by table, probe by probe); tests/golden/gen_lz4_traps.py holds it against liblz4 on every trap.
"""
import collections
import math
import struct

import numpy as np

MFLIMIT, LASTLIT, MAXBLK = 12, 5, 65536
W0 = 16                                            # QZK_LZ4_W0: probes of a streak's first window
FAMILIES = ("A", "B", "C", "D", "E", "F", "G", "H", "I")


def rnd(n, seed):
    return np.random.RandomState(seed).randint(0, 256, n, dtype=np.uint8).tobytes()


def u32(b, p):
    return b[p] | b[p + 1] << 8 | b[p + 2] << 16 | b[p + 3] << 24


def hash4(v):
    return ((v * 2654435761) & 0xffffffff) >> 19


def hash5(b, p):
    seq = u32(b, p) | b[p + 4] << 32
    return (((seq << 24) & 0xffffffffffffffff) * 889523592379 & 0xffffffffffffffff) >> 52


def grid(ip, count):
    """positions of the first `count` probes of a streak from ip"""
    out = [ip]
    for j in range(1, count):
        t = j - 1; b = t >> 6; r = t & 63
        out.append(ip + 1 + 32 * b * (b + 1) + (b + 1) * r)
    return out


def step_at(j):
    return 1 if j == 0 else (63 + j) >> 6


def probe_at_or_after(ip, pos):
    """(j, position) of the first probe of a streak from ip that sits at or behind pos"""
    if pos <= ip:
        return 0, ip
    b = 0
    while ip + 1 + 32 * (b + 1) * (b + 2) <= pos:
        b += 1
    start = ip + 1 + 32 * b * (b + 1)
    r = max(0, -(-(pos - start) // (b + 1)))
    return 1 + 64 * b + r, start + (b + 1) * r


# ------------------------------------------------------------------------------------------------ the strict reader
Blk = collections.namedtuple("Blk", "stored raw seqs last at")


def parse_block(body, base=0):
    """sequences of one LZ4 block, strictly: the end rules of the format hold or this raises"""
    seqs, at, p, pos = [], [], 0, base
    n = len(body)
    while True:
        tok = body[p]; p += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                x = body[p]; p += 1; lit += x
                if x != 255:
                    break
        p += lit; pos += lit
        assert p <= n
        if p == n:
            assert (tok & 15) == 0, "the last sequence carries literals only"
            return seqs, lit, at
        off = body[p] | body[p + 1] << 8; p += 2
        ml = (tok & 15) + 4
        if (tok & 15) == 15:
            while True:
                x = body[p]; p += 1; ml += x
                if x != 255:
                    break
        assert 0 < off <= pos
        seqs.append((lit, ml, off)); at.append((pos, ml, off)); pos += ml


def parse_frame(frame):
    """blocks of a frame LZ4F_compressFrame wrote (content checksum, no block checksums): -> (FLG, content size, [Blk])"""
    assert frame[:4] == b"\x04\x22\x4d\x18"
    flg = frame[4]
    assert flg >> 6 == 1 and not flg & 0x10 and flg & 4 and not flg & 1
    p = 6; size = None
    if flg & 8:
        size = struct.unpack_from("<Q", frame, p)[0]; p += 8
    p += 1
    blocks, base = [], 0
    while True:
        bh = struct.unpack_from("<I", frame, p)[0]; p += 4
        if bh == 0:
            break
        ln = bh & 0x7fffffff
        body = frame[p:p + ln]; p += ln
        assert len(body) == ln
        if bh >> 31:
            blocks.append(Blk(True, ln, [], ln, []))
            base += ln
        else:
            seqs, last, at = parse_block(body, base if not flg & 0x20 else 0)
            raw = sum(s[0] + s[1] for s in seqs) + last
            blocks.append(Blk(False, raw, seqs, last, at))
            base += raw
    assert p + 4 == len(frame)
    assert size is None or size == base
    return flg, size, blocks


# ------------------------------------------------------------------------------------------------ the serial model
Found = collections.namedtuple("Found", "pos j back how")          # where a sequence's match was met: probe j of its streak


def model(src, cap_rule=True):
    """lz4 1.9.3's fast parser restated serially -> [(stored, seqs, last, founds, fired)] per block.  `founds` says per
    sequence at which probe of its streak (how = "streak") or at the test behind a match (how = "next") it was met and how
    far the backward extension went; `fired` names the capacity check that made the block a stored one (cap = n - 1)."""
    n = len(src)
    linked = n > MAXBLK
    table = {}
    out = []
    for bs in range(0, n, MAXBLK):
        be = min(n, bs + MAXBLK); bn = be - bs
        cap = bn - 1
        seqs, founds, fired = [], [], None
        anchor, op = bs, 0
        H = (lambda p: hash5(src, p)) if linked else (lambda p: hash4(u32(src, p)))
        near = (lambda c, f: c + 65535 >= f) if linked else (lambda c, f: True)
        if bn >= MFLIMIT + 1:
            mfl1 = be - MFLIMIT + 1; matchlimit = be - LASTLIT
            if linked:
                table[H(bs)] = bs
            ip = bs + 1
            while fired is None:
                f, j, hit = ip, 0, None
                while True:
                    st = step_at(j)
                    if f + st > mfl1:
                        break
                    h = H(f); cand = table.get(h, 0); table[h] = f
                    if near(cand, f) and src[cand:cand + 4] == src[f:f + 4]:
                        hit = cand
                        break
                    f += st; j += 1
                if hit is None:
                    break
                mip, match, back = f, hit, 0
                while mip > anchor and match > 0 and src[mip - 1] == src[match - 1]:
                    mip -= 1; match -= 1; back += 1
                lit = mip - anchor
                op += 1
                if op + lit + (2 + 1 + LASTLIT) + lit // 255 > cap:
                    fired = "literals"
                    break
                if lit >= 15:
                    op += (lit - 15) // 255 + 1
                op += lit
                how = "streak"
                while True:
                    op += 2
                    a, b, mc = mip + 4, match + 4, 0
                    while a + mc < matchlimit and src[a + mc] == src[b + mc]:
                        mc += 1
                    if op + (1 + LASTLIT) + (mc + 240) // 255 > cap:
                        fired = "match"
                        break
                    if mc >= 15:
                        op += (mc - 15) // 255 + 1
                    seqs.append((lit, mc + 4, mip - match)); founds.append(Found(mip, j, back, how))
                    mip += mc + 4
                    anchor = mip
                    if mip >= mfl1:
                        break
                    table[H(mip - 2)] = mip - 2
                    h = H(mip); cand = table.get(h, 0); table[h] = mip
                    if near(cand, mip) and src[cand:cand + 4] == src[mip:mip + 4]:
                        op += 1; lit = 0; match = cand; how = "next"; back = 0; j = -1
                        continue
                    break
                if fired or anchor >= mfl1:
                    break
                ip = anchor + 1
        lr = be - anchor
        if fired is None and op + lr + 1 + (lr + 255 - 15) // 255 > cap:
            fired = "last literals"
        out.append((fired is not None, seqs, lr, founds, fired))
    return out


# ------------------------------------------------------------------------------------------------ building blocks
class Buf:
    """random filler with planted copies; plant() keeps the bytes around a copy from agreeing by accident"""

    def __init__(self, n, seed):
        self.b = bytearray(rnd(n, seed))
        self.n = n

    def plant(self, dst, src, ln, guard=True):
        b = self.b
        for i in range(ln):                          # byte by byte: an overlapping copy is a repetition
            b[dst + i] = b[src + i]
        if guard:
            if dst > 0 and src > 0 and b[dst - 1] == b[src - 1]:
                b[dst - 1] ^= 0x55
            if dst + ln < self.n and b[dst + ln] == b[src + ln]:
                b[dst + ln] ^= 0x55
        return self

    def put(self, pos, data):
        self.b[pos:pos + len(data)] = data
        return self

    def ballast(self, ln=160, bs=0):
        """a long copy of the block's bytes 8.. at the far end of the block that starts at bs: the block shrinks whatever else
        happens, and the trap's decision stays visible instead of vanishing in a stored block"""
        dst = min(self.n, bs + MAXBLK) - ln - 40
        self.plant(dst, bs + 8, ln)
        return dst, ln, dst - bs - 8

    def bytes(self):
        return bytes(self.b)


Trap = collections.namedtuple("Trap", "name family data mode aim check")
_TRAPS = []


def trap(name, family, data, aim, check):
    data = bytes(data)
    _TRAPS.append(Trap(name, family, data, "linked" if len(data) > MAXBLK else "block", aim, check))


def first_is(*exp):
    """the block's first sequences are exactly these (literal length, match length, offset)"""
    exp = list(exp)
    return lambda bl: not bl[0].stored and bl[0].seqs[:len(exp)] == exp


def has_at(pos, ml, off, blk=0):
    return lambda bl: not bl[blk].stored and (pos, ml, off) in bl[blk].at


def none_at(lo, hi, blk=0):
    """no match begins in [lo, hi)"""
    return lambda bl: not bl[blk].stored and not any(lo <= a[0] < hi for a in bl[blk].at)


def both(*cs):
    return lambda bl: all(c(bl) for c in cs)


S1 = 4096           # the common size: head (bytes 0..65, every position probed at step 1), filler, planted copies, ballast
S2 = 16384          # where a streak has to reach steps 17-19
M0_AT, M0_LEN = 200, 40


def after_m0(n, seed):
    """filler with a first match M0 (bytes 10..49 again at 200, found by the step-2 grid and walked back to 200): the streak
    behind it starts at 241 with its first window of QZK_LZ4_W0 probes, the register window based at 240"""
    B = Buf(n, seed).plant(M0_AT, 10, M0_LEN)
    return B, M0_AT + M0_LEN, (M0_AT, M0_LEN, M0_AT - 10)


# ------------------------------------------------------------------------------------------------ A: end-of-block rules
def _family_a():
    for n in range(0, 17):
        trap("a_n%d" % n, "A", rnd(n, 100 + n), "n = %d random bytes: below MFLIMIT + 1 nothing is searched; the block is stored" % n,
             (lambda bl: bl == []) if n == 0 else (lambda bl: len(bl) == 1 and bl[0].stored))
    trap("a_eq12", "A", b"\x07" * 12, "12 equal bytes: no search below 13 bytes, stored", lambda bl: bl[0].stored)
    trap("a_eq13", "A", b"\x07" * 13, "13 equal bytes: the one live probe (1 + 1 <= mflimit + 1 = 2) hits position 0; the match stops at n - 5",
         lambda bl: not bl[0].stored and bl[0].seqs == [(1, 7, 1)] and bl[0].last == 5)
    # a last match that starts at n - 12 is taken, one that could only start at n - 11 is not
    for name, d, aim in (("a_last_match_n12", 12, "the probe at n - 12 is live (f + 1 == mflimit + 1): second sequence (3, 7, .)"),
                         ("a_last_match_n11", 11, "a repeat from n - 11 only: its probe is the goto _last_literals, one sequence")):
        n = 96
        B = Buf(n, 11).plant(61, 10, 20)             # M1 ends at 81; the streak behind it probes 82, 83, 84 (= n - 12), 85 is dead
        B.plant(n - d, 40, 8, guard=False)
        B.b[n - d - 1] = B.b[39] ^ 0x55
        if d == 12:
            chk = lambda bl: bl[0].seqs == [(61, 20, 51), (3, 7, 44)] and bl[0].last == 5
        else:
            chk = lambda bl: bl[0].seqs == [(61, 20, 51)] and bl[0].last == 15
        trap(name, "A", B.bytes(), aim, chk)
    # the probe with f + step == mflimit + 1 at step 2, and one byte later; a dead probe before a would-be hit
    g = grid(M0_AT + M0_LEN + 1, 90)
    f80 = g[80]                                      # step 2 there
    assert step_at(80) == 2
    for name, n, at, aim in (("a_can_step2_live", f80 + 2 + 11, f80, "f + 2 == mflimit + 1: the probe is live and hits"),
                             ("a_can_step2_dead", f80 + 2 + 10, f80, "f + 2 == mflimit + 2: the probe is dead, the word under it is never looked up"),
                             ("a_dead_before_hit", f80 + 2 + 10, f80 + 2, "probe 80 is dead; the word under would-be probe 81 of the same window stays unseen")):
        B, e, m0 = after_m0(n, 12)
        B.plant(at, 52, 8, guard=False)
        B.b[at - 1] = B.b[51] ^ 0x55
        if name.endswith("live"):
            chk = lambda bl, at=at, e=e, n=n, m0=m0: bl[0].seqs == [m0, (at - e, 4 + (n - 5) - (at + 4), at - 52)]
        else:
            chk = lambda bl, m0=m0: bl[0].seqs == [m0]
        trap(name, "A", B.bytes(), aim, chk)
    # a match that must stop at n - 5 while the data goes on matching: every residue of maxlen & 3, short and beyond the windows
    for n, base, tag in ((120, 40, "short"), (700, 300, "long")):
        for r in range(4):
            B = Buf(n, 13 + r)
            if base > 65:
                B, e, m0 = after_m0(n, 13 + r)
                dst = e + 3 + r
                B.plant(dst, 4, n - dst)
                exp = [m0, (dst - e, 4 + (n - 5) - (dst + 4), dst - 4)]
            else:
                dst = base + r
                B.plant(dst, 4, n - dst)
                exp = [(dst, 4 + (n - 5) - (dst + 4), dst - 4)]
            trap("a_stop_%s_%d" % (tag, r), "A", B.bytes(),
                 "the copy runs to the block's end, the match stops at n - 5: maxlen & 3 == %d" % (((n - 5) - (dst + 4)) & 3),
                 lambda bl, exp=exp: bl[0].seqs == exp and bl[0].last == 5)
    # the same with the copy ending ONE byte behind n - 5: the byte at the limit agrees, the next one of the same dword differs
    for r in range(4):
        n, dst = 120, 40 + r
        B = Buf(n, 18 + r)
        B.plant(dst, 4, n - 5 - dst + 1)
        trap("a_stop_past_%d" % r, "A", B.bytes(),
             "the copy ends one byte behind n - 5 (maxlen & 3 == %d): the match still stops at n - 5, not at the differing byte" % (((n - 5) - (dst + 4)) & 3),
             lambda bl, exp=[(dst, 4 + (n - 5) - (dst + 4), dst - 4)]: bl[0].seqs == exp and bl[0].last == 5)
    # a sequence that ends exactly at mflimit + 1 (no insert, no further search), and one byte short of it
    for d, name in ((11, "a_ends_at_mfl1"), (12, "a_ends_before_mfl1")):
        n = 400
        B, e, m0 = after_m0(n, 17)
        dst = e + 5; ln = n - d - dst
        B.plant(dst, 4, ln)
        trap(name, "A", B.bytes(), "the second match ends at n - %d: %s" % (d, "the loop ends there" if d == 11 else "position n - 14 is inserted, the streak behind dies at once"),
             lambda bl, exp=[m0, (5, ln, dst - 4)], d=d: bl[0].seqs == exp and bl[0].last == d)


# ------------------------------------------------------------------------------------------------ B: probe grid and acceleration
def _family_b():
    trap("b_probe0_first", "B", Buf(S1, 20).put(0, b"\x21" * 9).put(9, b"\x22").plant(3000, 100, 200).bytes(),
         "probe 0 of the first streak (position 1) meets position 0 through the zeroed table", first_is((1, 8, 1)))
    # hits at chosen probes of the streak behind M0 (ip = 241): lane W0 - 1 of the first window, lane 0 of the second, 63 / 64 / 65
    for j in (0, 1, W0 - 1, W0, W0 + 1, 63, 64, 65, W0 + 63, W0 + 64):
        B, e, m0 = after_m0(S1, 21)
        B.ballast()
        p = grid(e + 1, j + 1)[j]
        ln = 8
        B.plant(p, 52, ln)
        trap("b_probe%d" % j, "B", B.bytes(), "probe %d of the streak behind M0 (position %d, step %d) is the hit" % (j, p, step_at(j)),
             first_is(m0, (p - e, ln, p - 52)))
    # deep in the first streak: steps 2, 3, 17, 18, the copy planted k bytes in front of the probe
    for step, n, r, ks in ((2, S1, 30, (0, 1)), (3, S1, 20, (0, 2)), (17, S2, 12, (0, 16)), (18, S2, 10, (0, 1, 15, 16, 17))):
        b = step - 1
        g = 2 + 32 * b * (b + 1) + step * r
        for k in ks:
            B = Buf(n, 22)
            B.ballast(200)
            B.plant(g - k, 20, 40)
            trap("b_step%d_k%d" % (step, k), "B", B.bytes(),
                 "the probe at %d (step %d) meets a copy planted %d bytes in front of it: first sequence has %d literals" % (g, step, k, g - k),
                 first_is((g - k, 40, g - k - 20)))
    # a repeat between two grid points at step 18 is not seen there
    b = 17; g = 2 + 32 * b * (b + 1) + 18 * 10
    B = Buf(S2, 23)
    bal = B.ballast(200)
    B.plant(g + 1, 20, 20)                            # 9975..9994: the probes at 9974 and 9992 both read a byte outside it
    trap("b_between_grid_step18", "B", B.bytes(), "20 repeated bytes between the probes at %d and %d: no match there" % (g, g + 18),
         first_is((bal[0], bal[1], bal[2])))
    # a hit on the last lane of a window with a suspect lane before it: probes 77 and 78 read the same word, probe 79 hits
    B, e, m0 = after_m0(S1, 24)
    B.ballast()
    g = grid(e + 1, 81)
    assert g[78] - g[77] == 2 and g[79] - g[78] == 2
    w = bytes(B.b[g[77]:g[77] + 2])
    B.put(g[77], w * 3)                               # period 2 over probes 77 and 78: 78 is suspect, and it is a hit on 77
    trap("b_suspect_hit_before_last_lane", "B", B.bytes(), "probes 77 and 78 (step 2) share a word: the replay makes 78 the hit, offset 2",
         both(first_is(m0), lambda bl, p=g[78], e=e: bl[0].seqs[1][2] == 2 and bl[0].seqs[1][0] <= p - e))
    B = after_m0(S1, 25)[0]; B.ballast()
    w1, w2 = _same_hash_pair(7)
    B.put(g[70], w1).put(g[74], w2)                   # same hash, different words: lane of 74 is suspect, no hit
    B.plant(g[79], 52, 8)
    trap("b_last_lane_hit_after_suspect", "B", B.bytes(), "probe 79 = lane 63 of its window hits; lane 58 before it is a suspect that misses",
         first_is(m0, (g[79] - e, 8, g[79] - 52)))


# ------------------------------------------------------------------------------------------------ word pairs by brute force
def _same_hash_pair(seed, same_hash=True):
    """two different 4-byte words with the same 13-bit hash (or: different hashes on the same key h & 1023)"""
    rs = np.random.RandomState(seed)
    w1 = rs.randint(0, 256, 4, dtype=np.uint8).tobytes()
    h1 = hash4(u32(w1, 0))
    while True:
        w2 = rs.randint(0, 256, 4, dtype=np.uint8).tobytes()
        h2 = hash4(u32(w2, 0))
        if w2 != w1 and ((h2 == h1) if same_hash else (h2 != h1 and (h2 & 1023) == (h1 & 1023))):
            return w1, w2


def _fifth_byte_pair(seed):
    """four bytes and two different fifth bytes.  hash5 multiplies the fifth byte into the top eight of its twelve bits by an
    odd constant, so two strings with equal first four bytes NEVER share a bucket (asserted here for all 256 fifth bytes):
    a hash5 collision with equal first four bytes does not exist, and there is no trap for it"""
    w = rnd(4, seed)
    assert len({hash5(w + bytes([c]), 0) for c in range(256)}) == 256
    return w + b"\x00", w + b"\x01"


# ------------------------------------------------------------------------------------------------ C: backward extension
def _family_c():
    # the register path (the streak behind M0, F holds mip): the copy's source lies around a probe of the step-18 grid at 9974,
    # so only ONE of its words is in the table and the probes before it miss: back = k, stopped by a differing byte
    sg = 2 + 32 * 17 * 18 + 18 * 10
    m0_at = 12000
    jm, pm = probe_at_or_after(1, m0_at)
    for k in (0, 1, 15, 16, 17):
        B = Buf(S2, 30)
        B.ballast(200)
        B.plant(pm, 10, M0_LEN)
        e = pm + M0_LEN
        dst = e + 3
        B.plant(dst, sg - k, k + 24)
        trap("c_regs_back%d" % k, "C", B.bytes(),
             "only the word at %d is in the table: the probe at %d hits and walks %d bytes back (sixteen out of the registers)" % (sg, dst + k, k),
             first_is((pm, M0_LEN, pm - 10), (3, k + 24, dst - (sg - k))))
    # stopped by the anchor: the bytes before the anchor agree too, the literal length becomes 0
    for k in (1, 16, 17):
        B = Buf(S2, 31)
        B.ballast(200)
        B.plant(pm, 10, M0_LEN)
        e = pm + M0_LEN
        B.b[sg - k - 1] = B.b[e - 1]                  # "could go on": the byte in front of the source is M0's last byte
        B.plant(e, sg - k, k + 24, guard=False)
        B.b[e + k + 24] = B.b[sg + 24] ^ 0x55
        trap("c_anchor_back%d" % k, "C", B.bytes(),
             "the walk back from %d stops at the anchor after %d bytes although the bytes before agree: literal length 0" % (e + k, k),
             first_is((pm, M0_LEN, pm - 10), (0, k + 24, e - (sg - k))))
    # the memory loop (first streak, mip far outside F): source on the step-18 grid, copy met by the step-19 grid
    g19 = 2 + 32 * 18 * 19 + 19 * 20
    for k in (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200):
        B = Buf(S2, 32)
        B.ballast(200)
        B.plant(g19 - k, sg - k, k + 30)
        trap("c_mem_back%d" % k, "C", B.bytes(),
             "the step-19 probe at %d is the first whose source word (%d, step-18 grid) was inserted: %d bytes back, literal run %d" % (g19, sg, k, g19 - k),
             first_is((g19 - k, k + 30, g19 - sg)))
    # stopped by position 0: the candidate is the block's first word, reached through the zeroed table (position 0 is never inserted)
    B, e, m0 = after_m0(S1, 33)
    B.ballast()
    p = e + 9
    B.plant(p, 0, 24)
    trap("c_pos0", "C", B.bytes(), "bytes 0..23 again at %d: candidate 0 out of an empty slot, no walk back below position 0" % p,
         first_is(m0, (9, 24, p)))


# ------------------------------------------------------------------------------------------------ D: collisions inside one window
def _family_d():
    for per in (1, 2, 3, 4, 5, 6, 7, 8):
        # right behind a match: the W0-wide window; every lane is suspect, the replay finds the candidate among earlier lanes
        B, e, m0 = after_m0(S1, 40 + per)
        B.ballast()
        q, ln = e + 2, 300
        pat = bytes(B.b[q:q + per])
        if per > 1 and len(set(pat)) == 1:
            pat = bytes([pat[0] ^ 1]) + pat[1:]
        B.put(q, (pat * (ln // per + 1))[:ln])
        B.b[q - 1] = pat[-1] ^ 0x55; B.b[q + ln] = pat[ln % per] ^ 0x55
        trap("d_period%d_w0" % per, "D", B.bytes(),
             "period %d from %d on: the probe at %d finds the one at %d among the lanes of its own window" % (per, q, q + per, q),
             first_is(m0, (2 + per, ln - per, per)))
        # deep in the first streak (step 7, 64-wide windows): the first two probes with the same word are lcm(7, per) apart
        b = 6; g = 2 + 32 * b * (b + 1) + 7 * 20
        B = Buf(S1, 50 + per)
        B.ballast()
        q, ln = g - 3, 600
        pat = bytes(B.b[q:q + per])
        if per > 1 and len(set(pat)) == 1:
            pat = bytes([pat[0] ^ 1]) + pat[1:]
        B.put(q, (pat * (ln // per + 1))[:ln])
        B.b[q - 1] = pat[-1] ^ 0x55; B.b[q + ln] = pat[ln % per] ^ 0x55
        off = 7 * per // math.gcd(7, per)
        trap("d_period%d_deep" % per, "D", B.bytes(),
             "period %d met by probes 7 apart: the first repeat of a probed word is %d bytes on, walked back to %d" % (per, off, q + off),
             first_is((q + off, ln - off, off)))
    for split in (False, True):
        tag = "split" if split else "one_window"
        for same_hash in (True, False):
            w1, w2 = _same_hash_pair(60 + same_hash, same_hash)
            for third in (1, 2):
                B, e, m0 = after_m0(S1, 62)
                B.ballast()
                p1, p2, p3 = e + 3, (e + 21 if split else e + 9), e + 41
                B.put(p1, w1).put(p2, w2).put(p3, (w1, w2)[third - 1])
                kept = third == 2 or not same_hash
                name = "d_%s_%s_third%d" % ("hash" if same_hash else "key", tag, third)
                aim = ("%s and %s %s (lanes of %s); word %d again at %d: %s"
                       % (w1.hex(), w2.hex(), "share a hash" if same_hash else "share h & 1023 but not the hash",
                          "two windows" if split else "the first window", third, p3,
                          "the table kept its position" if kept else "the later word took its slot, no match"))
                if kept:
                    chk = both(first_is(m0), lambda bl, p3=p3, src=(p1, p2)[third - 1]: any(a[0] == p3 and a[2] == p3 - src for a in bl[0].at))
                else:
                    chk = both(first_is(m0), none_at(e, e + 120))
                trap(name, "D", B.bytes(), aim, chk)


# ------------------------------------------------------------------------------------------------ E: which positions get inserted
def _family_e():
    # the hit lane is inserted, the lanes behind it are not
    for which in ("hit", "after"):
        B, e, m0 = after_m0(S1, 70)
        B.ballast()
        d1 = e + 4
        B.plant(d1, 52, 12)                           # probe 3 of the first window hits; lanes 4.. read positions inside the match
        t = 600
        jt, pt = probe_at_or_after(d1 + 12 + 1, t)
        if which == "hit":
            B.plant(pt, d1, 8, guard=False)           # the word of the hit position again: the table holds d1, not 52
            B.b[pt - 1] = B.b[51] ^ 0x33; B.b[pt + 8] ^= 0x77
            chk = has_at(pt, 8, pt - d1)
            aim = "the word at the hit position %d comes back at %d: the hit lane was inserted, offset %d (not %d)" % (d1, pt, pt - d1, pt - 52)
        else:
            B.plant(pt, d1 + 2, 8, guard=False)       # a word only a lane BEHIND the hit read: the table still holds 54
            B.b[pt - 1] = B.b[53] ^ 0x33; B.b[pt + 8] ^= 0x77
            chk = has_at(pt, 8, pt - 54)
            aim = "the word at %d, read by a lane behind the hit lane, comes back at %d: not inserted, offset %d (not %d)" % (d1 + 2, pt, pt - 54, pt - d1 - 2)
        trap("e_lane_%s_hit" % which, "E", B.bytes(), aim, both(first_is(m0, (4, 12, d1 - 52)), chk))
    # chains of zero-literal sequences through the test behind a match
    B, e, m0 = after_m0(S1, 71)
    B.ballast()
    p = e + 6
    srcs = (20, 44, 8, 30, 56)
    exp = [m0]
    for i, s in enumerate(srcs):
        B.plant(p, s, 8, guard=False)
        exp.append((6 if i == 0 else 0, 8, p - s))
        p += 8
    trap("e_chain5", "E", B.bytes(), "five copies back to back: four sequences without literals, each met by the test at mip",
         lambda bl, exp=exp: bl[0].seqs[:len(exp)] == exp)
    # the candidate of the test at mip is the position mip - 2 inserted just before it
    B, e, m0 = after_m0(S1, 72)
    B.ballast()
    p = e + 6
    B.plant(p, 20, 10, guard=False)                    # ends at mip = p + 10 with the bytes (a, b)
    a, b = B.b[p + 8], B.b[p + 9]
    if B.b[30] == a:
        B.b[30] ^= 0x55
    B.put(p + 10, bytes([a, b]) * 6)
    B.b[p + 22] = a ^ 0x55
    trap("e_mip2_is_candidate", "E", B.bytes(), "period 2 behind a match: the test at mip finds mip - 2, inserted an instruction earlier: (0, 12, 2)",
         first_is(m0, (6, 10, p - 20), (0, 12, 2)))
    # mip - 2 is inserted although no probe read it: its word comes back later
    B, e, m0 = after_m0(S1, 73)
    B.ballast()
    d1 = e + 4
    B.plant(d1, 20, 16)
    mip = d1 + 16
    jt, pt = probe_at_or_after(mip + 1, 700)
    B.plant(pt, mip - 2, 8, guard=False)
    B.b[pt - 1] = B.b[mip - 3] ^ 0x33
    trap("e_mip2_inserted", "E", B.bytes(), "the word at mip - 2 = %d (two match bytes, two new ones) is in the table: met again at %d" % (mip - 2, pt),
         both(first_is(m0, (4, 16, d1 - 20)), lambda bl, pt=pt, o=pt - (mip - 2): any(a[0] == pt and a[2] == o for a in bl[0].at)))
    _epoch_frames()


EPOCH_WORDS = (b"\xc3\x5a\x17\xe9", b"\x0b\xd4\x66\x91", b"\x7e\x21\xf8\x3c")


def _epoch_frames():
    """e_epoch_plant leaves the three EPOCH_WORDS in the table at positions 30, 34 and 38; e_epoch_probe<k> has word k at 50
    only and other bytes at 30..41.  Alone each is an ordinary frame.  As frames of ONE wave of the pull kernel a whole turn of
    its 16-bit epoch apart (tests/test_sim_lz4_traps.py), a probe frame meets the plant frame's entry under its own epoch
    again unless the table was cleared at the wrap - and would then write a match that liblz4 never saw.  (Three probe
    frames with a word each: a probe frame overwrites the entry of its own word, whatever its epoch.)"""
    B = Buf(S1, 75)
    B.ballast()
    for k, w in enumerate(EPOCH_WORDS):
        B.put(30 + 4 * k, w)
    trap("e_epoch_plant", "E", B.bytes(), "the words %s at 30, 34, 38 only: inserted, never met" % " ".join(w.hex() for w in EPOCH_WORDS),
         none_at(0, 3000))
    for k, w in enumerate(EPOCH_WORDS):
        B = Buf(S1, 76 + k)
        B.ballast()
        B.put(50, w)
        assert not any(x in bytes(B.b[26:46]) for x in EPOCH_WORDS)
        trap("e_epoch_probe%d" % (k + 1), "E", B.bytes(),
             "the word %s at 50 only: no match there (a stale entry of the plant frame would say %d)" % (w.hex(), 30 + 4 * k), none_at(0, 3000))


# ------------------------------------------------------------------------------------------------ F: length codes and capacities
def _family_f():
    for lit in (14, 15, 16, 127, 128, 129, 269, 270, 271, 300, 525, 780, 1035):
        B = Buf(S1, 80)
        B.ballast()
        B.plant(lit, 2, 10)
        trap("f_lit%d" % lit, "F", B.bytes(), "first literal run of exactly %d bytes" % lit, first_is((lit, 10, lit - 2)))
    for lit in (127, 128, 129, 140, 300):
        B, e, m0 = after_m0(S1, 81)
        B.ballast()
        B.plant(e + lit, 52, 12)
        trap("f_lit%d_behind_match" % lit, "F", B.bytes(),
             "a literal run of %d behind a match (QZK_L4C_LITMAX: out of the register window up to 128, memory to memory above)" % lit,
             first_is(m0, (lit, 12, e + lit - 52)))
    for mc in [14, 15, 16, 269, 270, 271] + list(range(225, 246)):
        B, e, m0 = after_m0(S1, 82)
        B.ballast()
        B.plant(e + 3, 52, mc + 4)
        trap("f_mc%d" % mc, "F", B.bytes(), "match count %d behind a match (input side from F, candidate side from C, the rest from memory)" % mc,
             first_is(m0, (3, mc + 4, e + 3 - 52)))
    for mc in (14, 15, 16, 269, 270, 271, 524, 525):
        B = Buf(S1, 83)
        B.ballast()
        B.plant(2048, 20, mc + 4)
        trap("f_mc%d_deep" % mc, "F", B.bytes(), "match count %d deep in a streak (neither window holds it)" % mc, first_is((2048, mc + 4, 2028)))
    B = Buf(S2, 84)
    B.plant(9000, 300, 6000)
    trap("f_match6000", "F", B.bytes(), "a match of 6000 bytes", first_is((9000, 6000, 8700)))
    for per in (1, 2, 3):
        pat = rnd(per, 85 + per) if per > 1 else b"\x5a"
        data = (pat * (S1 // per + 1))[:S1]
        trap("f_whole_block_off%d" % per, "F", data, "the whole block is one match at offset %d" % per,
             lambda bl, per=per: bl[0].seqs == [(per, S1 - 5 - per, per)] and bl[0].last == 5)
    # many short sequences in a row: the staged output crosses 256 at every phase; a long literal run right behind a partial flush
    for seed, gap in ((90, 0), (91, 0), (92, 200), (93, 131)):
        rs = np.random.RandomState(seed)
        B = Buf(S1, seed)
        p, nseq, gap_at = 80, 0, 90
        exp = []
        last_end = None
        while p < S1 - 400:
            lit = int(rs.randint(0, 4)) if nseq else 80
            if gap and nseq == gap_at:
                lit = gap
            ml = int(rs.randint(4, 9)); s = int(rs.randint(1, 60 - ml))
            p += lit if nseq else 0
            B.plant(p, s, ml, guard=False)
            # the copy must end where it is planted to end, and the literals in front of it must not extend it backwards
            if B.b[p + ml] == B.b[s + ml]:
                B.b[p + ml] ^= 0x55
            nseq += 1; p += ml
        data = B.bytes()
        trap("f_short_seqs_%d%s" % (seed, "_gap%d" % gap if gap else ""), "F", data,
             "hundreds of sequences of 4-8 match bytes and 0-3 literals%s" % (", one literal run of %d among them" % gap if gap else ""),
             lambda bl, gap=gap: len(bl[0].seqs) > 300 and (not gap or any(s[0] >= gap for s in bl[0].seqs[1:])))


# ------------------------------------------------------------------------------------------------ G: the shrink limit
# seeds found by tests/golden/gen_lz4_traps.py --search (shrink_input below, liblz4's unconstrained block size): n -> {delta: seed}
SHRINK_SEEDS = {256: {-2: 5, -1: 4, 0: 3, 1: 73}, 1000: {-2: 2, -1: 50, 0: 7, 1: 17}, 4096: {-2: 127, -1: 6, 0: 48, 1: 2},
                65536: {-2: 1666, -1: 1085, 0: 5149, 1: 2091}}


def shrink_input(n, seed):
    """random bytes with 1-8 planted repeats of 5-8 bytes"""
    rs = np.random.RandomState(seed)
    b = bytearray(rs.randint(0, 256, n, dtype=np.uint8).tobytes())
    for _ in range(int(rs.randint(1, 9)) * max(1, n // 1024)):
        ln = int(rs.randint(5, 9))
        a = int(rs.randint(0, n - 2 * ln))
        d = int(rs.randint(a + ln, n - ln))
        b[d:d + ln] = b[a:a + ln]
    return bytes(b)


def _family_g():
    for n in sorted(SHRINK_SEEDS):
        for delta, seed in sorted(SHRINK_SEEDS[n].items()):
            trap("g_n%d_%+d" % (n, delta), "G", shrink_input(n, seed),
                 "unconstrained block size n%+d: %s" % (delta, "fits n - 1, compressed" if delta < 0 else "does not fit, stored"),
                 (lambda bl: not bl[0].stored and len(bl[0].seqs) > 0) if delta < 0 else (lambda bl: bl[0].stored))
    # each of the three capacity checks as the one that fires (model() names it; liblz4's frame only shows the stored block)
    B = Buf(S1, 95).plant(4072, 20, 20)
    trap("g_cap_literals", "G", B.bytes(), "4072 literals in front of the only match: the literal-run check gives up", lambda bl: bl[0].stored)
    B = Buf(S1, 96).plant(4071, 20, 24)
    trap("g_cap_match", "G", B.bytes(), "4071 literals: the run still fits, the match's length bytes and last literals do not", lambda bl: bl[0].stored)
    B = Buf(S1, 97).plant(2000, 20, 4)
    trap("g_cap_last_literals", "G", B.bytes(), "one match of four bytes saves one byte: the last-literals check gives up", lambda bl: bl[0].stored)
    B = Buf(S1, 97).plant(2000, 20, 40)
    trap("g_cap_none", "G", B.bytes(), "the same with a match of 40: every check passes", first_is((2000, 40, 1980)))


G_FIRED = {"g_cap_literals": "literals", "g_cap_match": "match", "g_cap_last_literals": "last literals", "g_cap_none": None}


# ------------------------------------------------------------------------------------------------ H: 16-bit positions
H_SEED = 0          # filler of 64 KB without a single accidental match (set by the search of gen_lz4_traps.py)


def _family_h():
    n = MAXBLK
    for name, s_at, d_at in (("h_cand_above_32767", 40000, 50000), ("h_cand_above_65000", 65050, 65300)):
        B = Buf(n, H_SEED)
        B.plant(30000, 8, 400)                          # the block shrinks; the streak behind it starts at 30401
        ps = probe_at_or_after(30401, s_at)[1]          # source word and copy both sit on that streak's grid
        pd = probe_at_or_after(30401, d_at)[1]
        B.plant(pd, ps, 120)
        trap(name, "H", B.bytes(), "a candidate at %d, met from %d: positions above %d in 16-bit entries" % (ps, pd, 32767 if ps < 65000 else 65000),
             has_at(pd, 120, pd - ps))
    B = Buf(n, H_SEED)
    B.plant(3000, 2000, 59000)                          # one long match: few probes, the words of bytes 1.. stay in the table
    B.plant(65480, 1, n - 65480)
    trap("h_word_at_1_recurs_at_65480", "H", B.bytes(), "bytes 1..56 again from 65480 to the block's end: offset 65479, the count stops at n - 5",
         lambda bl: not bl[0].stored and bl[0].at[-1] == (65480, 65531 - 65480, 65479) and bl[0].last == 5)


# ------------------------------------------------------------------------------------------------ I: linked frames
I_SEED = 0          # filler for the linked traps (likewise free of accidental matches over its first 139264 bytes)


def _family_i():
    n = MAXBLK + 8192
    # an offset of exactly 65535 is taken, 65536 is refused: inside the second block, and right behind a block border.  The block
    # between source and copy is one long match (no probes: the 4096-entry table keeps the source word)
    for where, cur, n_ in (("inside", MAXBLK + 3000, n), ("border", 2 * MAXBLK + 2, 2 * MAXBLK + 4096)):
        for dist in (65535, 65536):
            B = Buf(n_, I_SEED)
            bs = (cur // MAXBLK) * MAXBLK
            B.ballast(300, bs)
            s = cur - dist
            sb = (s // MAXBLK) * MAXBLK
            # s must be a probe: a match M ends three bytes in front of it; the same in front of cur
            for q in (s, cur):
                if q - (q // MAXBLK) * MAXBLK > 60:
                    B.plant(q - 3 - 40, (q // MAXBLK) * MAXBLK + 10, 40)
            B.plant(s + 600, s + 300, sb + MAXBLK - 40 - (s + 600))
            B.plant(cur, s, 8)
            blk = cur // MAXBLK
            trap("i_dist%d_%s" % (dist, where), "I", B.bytes(),
                 "the probe at %d meets the word of %d, %d back: %s" % (cur, s, dist, "taken" if dist == 65535 else "refused"),
                 has_at(cur, 8, 65535, blk) if dist == 65535 else none_at(cur - 2, cur + 20, blk))
    # a candidate in the previous block; the walk back stops at the block's start although the bytes before agree
    B = Buf(n, I_SEED)
    B.ballast(300, MAXBLK)
    ps = probe_at_or_after(1, 65000)[1]
    j2, cur = probe_at_or_after(MAXBLK + 1, MAXBLK + 5)
    k = cur - MAXBLK
    B.plant(MAXBLK - 6, ps - k - 6, 6 + k + 30)
    trap("i_back_stops_at_block_start", "I", B.bytes(),
         "the copy straddles the border: block 2's probe at %d walks back %d bytes to the block's first byte, no further" % (cur, k),
         lambda bl, k=k, ps=ps: not bl[1].stored and bl[1].seqs[0] == (0, k + 30, MAXBLK - (ps - k)))
    # a match that would run past the block's end - 5
    B = Buf(2 * MAXBLK + 4096, I_SEED)
    ps = probe_at_or_after(MAXBLK + 1, MAXBLK + 100)[1]
    cur = probe_at_or_after(MAXBLK + 1, 2 * MAXBLK - 800)[1]
    B.plant(cur, ps, 1200)
    trap("i_match_stops_at_block_end", "I", B.bytes(), "a copy of 1200 bytes from %d on crosses the border: the match stops 5 bytes short of it" % cur,
         lambda bl, cur=cur, ps=ps: not bl[1].stored and bl[1].at[-1] == (cur, 2 * MAXBLK - 5 - cur, cur - ps) and bl[1].last == 5)
    # a last block of 1 .. 12 bytes (13: the first that is searched)
    for tail in (1, 4, 11, 12, 13):
        B = Buf(MAXBLK + tail, I_SEED)
        B.plant(60000, 8, 400)
        B.plant(MAXBLK, 100, tail, guard=False)
        trap("i_last_block_%d" % tail, "I", B.bytes(), "a last block of %d bytes (bytes 100.. again): stored, nothing is searched below 13" % tail,
             lambda bl, tail=tail: len(bl) == 2 and bl[1].raw == tail and bl[1].stored and not bl[0].stored)
    # four bytes shared, the fifth not: different buckets of hash5, so lz4 finds no match
    a5, b5 = _fifth_byte_pair(9)
    B = Buf(n, I_SEED)
    B.ballast(300, MAXBLK)
    p1 = probe_at_or_after(MAXBLK + 1, MAXBLK + 20)[1]
    p2 = probe_at_or_after(MAXBLK + 1, MAXBLK + 40)[1]
    B.put(p1, a5).put(p2, b5)
    B.b[p1 - 1] = 1; B.b[p2 - 1] = 2
    trap("i_fifth_byte_differs", "I", B.bytes(), "four bytes agree, the fifth puts them in different buckets: no match",
         none_at(MAXBLK, MAXBLK + 100, 1))


_BUILT = None


def all_traps():
    """every trap, in a fixed order (built once per process)"""
    global _BUILT
    if _BUILT is None:
        del _TRAPS[:]
        for fam in (_family_a, _family_b, _family_c, _family_d, _family_e, _family_f, _family_g, _family_h, _family_i):
            fam()
        names = [t.name for t in _TRAPS]
        assert len(set(names)) == len(names)
        _BUILT = list(_TRAPS)
    return _BUILT


def by_size(traps):
    """block traps grouped by their size: equal-size traps are the frames of one call"""
    groups = collections.OrderedDict()
    for t in traps:
        if t.mode == "block":
            groups.setdefault(len(t.data), []).append(t)
    return groups
