"""Trap inputs for the LZ4-HC kernels (qatzip_amd/csrc/qzk_lz4hc.h): inputs built so that ONE rule of liblz4 1.9.3's
LZ4HC_compress_hashChain (compression levels 3-8) decides the bytes, each with a check that reads that decision out of
liblz4's own frame and, where the frame cannot show it, out of the trace of model().  tests/lz4_traps.py (the level-1
compressors) is the model for this file; its strict reader and its filler are used here, not copied.

A trap is (name, family, data, levels, aim, check):
  levels the compression levels it runs at
  aim    one line: the decision the trap aims at
  check  check(blocks, trace, level): blocks are what lz4_traps.parse_frame() reads from liblz4's frame at that level (a Blk
         has .stored, .raw, .seqs = [(literal length, match length, offset)], .last and .at = [(position in the frame's
         content, match length, offset)]); trace is model()'s.  A trap whose check fails on liblz4's output tests nothing.

model(src, level) restates lz4hc.c 1.9.3 serially - LZ4HC_Insert, LZ4HC_InsertAndGetWiderMatch (prefix mode, no pattern
analysis, no chain swap), LZ4HC_compress_hashChain with limitedOutput, and LZ4F_compressFrame's block loop - and returns the
frame with a Trace: per decision label (LABELS) how often it fired and, for the rarer ones, at which search positions.
tests/golden/gen_lz4hc_traps.py holds the model's bytes equal to liblz4's on every trap at every level; after that the trace
may be trusted.

Families: A chains and the first candidate, B attempts, C the search, D the parse state machine, E the encoder and the
ends, F geometry.  A, B, E and F are planted by hand on random filler.  The state machine's branches (D) and the search's
stop reasons (part of C) come from a seeded search over small-alphabet inputs with overlapping copies (sm_input()): per label
the smallest input whose trace holds it, kept here as its seed (SM_SEEDS, printed by gen_lz4hc_traps.py --search).
"""
import collections
import struct

import numpy as np

from lz4_traps import Buf, rnd, u32

MFLIMIT, LASTLIT, MAXBLK, MINMATCH, OPTIMAL_ML, MAXD = 12, 5, 65536, 4, 18, 65535
LEVELS = (3, 4, 5, 6, 7, 8)
FAMILIES = ("A", "B", "C", "D", "E", "F")


def attempts_of(level):
    """lz4hc.c clTable, the hash-chain levels"""
    return {3: 4, 4: 8, 5: 16, 6: 32, 7: 64, 8: 128}[level]


def hash_hc(v):
    return ((v * 2654435761) & 0xffffffff) >> 17


# two words with equal hash_hc and different bytes (found once by the seeded search of gen_lz4hc_traps.py --pairs):
# COLLIDE differ in their bytes 2 and 3 (a candidate that fails the 16-bit pre-check of a first search), COLLIDE_LOW agree in
# bytes 2 and 3 (it passes the pre-check and fails the word compare), COLLIDE_SHIFT are abcd / bcde: the words of two
# neighbouring positions of the five bytes abcde
COLLIDE = (bytes.fromhex("426d37f8"), bytes.fromhex("80f92a5e"))
COLLIDE_LOW = (bytes.fromhex("0000a85c"), bytes.fromhex("c22aa85c"))
COLLIDE_SHIFT = bytes.fromhex("9be3b0e501")


# ------------------------------------------------------------------------------------------------ the serial model
# label -> the decision (the lines are qzk_lz4hc.h's).  Every label is fired by a live trap, but those of UNREACHABLE.
LABELS = collections.OrderedDict((
    # A / B / C: LZ4HC_InsertAndGetWiderMatch
    ("first.none", "the hash table's slot is empty: no candidate (line 133)"),
    ("first.below", "the slot's position lies below lowestMatchIndex - farther than 65535, or under the window: no candidate (line 133)"),
    ("first.at65535", "the first candidate is exactly 65535 back and is tried (line 133)"),
    ("walk.end_attempts", "the attempts ran out with a candidate still in reach (loop 135-145)"),
    ("walk.end_below", "the walk ended at a chain entry below 65535 that leads under lowestMatchIndex (line 143)"),
    ("walk.end_capped", "the walk ended at a capped chain entry (65535) (line 143)"),
    ("try.pre16_fail", "a candidate failed the 16-bit pre-check (line 138): it cost an attempt"),
    ("try.word_fail", "a candidate passed the pre-check and failed the word compare (line 138): a collision, or a shorter match"),
    ("try.longer", "a candidate beat `longest` (line 141)"),
    ("try.equal", "a candidate equalled `longest`: the earlier one stays (line 141)"),
    ("try.shorter", "a candidate stayed below `longest` (line 141)"),
    ("back.mismatch", "the backward extension stopped at a differing byte"),
    ("back.ilow", "the backward extension stopped at iLowLimit"),
    ("back.prefix", "the backward extension stopped at the frame's first byte (m - back == 0)"),
    ("count.limit", "the forward count ran into matchlimit"),
    # D: LZ4HC_compress_hashChain
    ("s2.search", "line 200: the second search"),
    ("s2.nosearch", "line 200 else: ip + ml beyond mflimit, no second search"),
    ("s2.same", "line 203: no better match, ML1 is encoded"),
    ("restore.yes", "line 207: ML1 was skipped and ML2 starts inside ML0: ML0 comes back"),
    ("restore.no", "line 207: not restored (nothing was skipped, or ML2 starts behind ML0)"),
    ("small.d0", "line 208: start2 == ip, ML1 removed"),
    ("small.d1", "line 208: start2 == ip + 1, ML1 removed"),
    ("small.d2", "line 208: start2 == ip + 2, ML1 removed"),
    ("small.d3plus", "line 208: start2 - ip >= 3, on to the third search"),
    ("opt.out", "line 212: start2 - ip >= OPTIMAL_ML, no correction"),
    ("opt.ml_gt18", "line 214: ml above OPTIMAL_ML, cut to it"),
    ("opt.ml_le18", "line 214: ml at most OPTIMAL_ML"),
    ("opt.clamp2", "line 215: the second clamp, ML2 is left four bytes"),
    ("opt.corr_pos", "line 217: correction > 0, ML2 starts later"),
    ("opt.corr_nonpos", "line 217: correction <= 0, ML2 stays"),
    ("s3.search", "line 219: the third search"),
    ("s3.nosearch", "line 219 else: start2 + ml2 beyond mflimit, no third search"),
    ("s3.same_trim", "line 222-223: no better match, ML1 cut where ML2 starts"),
    ("s3.same_notrim", "line 222: no better match, ML1 whole"),
    ("s3.nospace", "line 229: ML3 starts before ip + ml + 3"),
    ("s3.seq1_now", "line 230: ML3 starts at or behind ML1's end: ML1 is written, ML3 becomes ML1"),
    ("s3.cut", "line 231: ML2 starts inside ML1 and is cut"),
    ("s3.nocut", "line 231: ML2 starts at ML1's end"),
    ("s3.ml2_dead", "line 234: the cut leaves ML2 below MINMATCH, ML3 takes its place"),
    ("s3.ml2_alive", "line 234: ML2 survives the cut"),
    ("s3.replace", "line 241: ML3 replaces ML2, search again"),
    ("asc.overlap", "line 245: three ascending matches, ML2 starts inside ML1"),
    ("asc.nooverlap", "line 245: three ascending matches, ML2 starts at or behind ML1's end"),
    ("asc.opt", "line 246 true (lines 247-250): OPTIMAL_ML shortening of the first of three ascending matches"),
    ("asc.plain", "line 251: ML1 ends where ML2 starts"),
    # E: LZ4HC_encodeSequence and the last literals
    ("fit.literals", "line 155: the literal run does not fit"),
    ("fit.match", "line 166: the match length does not fit"),
    ("fit.last", "line 262: the last literals do not fit"),
))

# Labels no input fires, each with its argument from lz4hc.c (at most three may stand here: tests/test_sim_lz4hc_traps.py).
#
# asc.opt.  Every way to the "three ascending matches" code goes through _Search3's own correction (lz4hc.c: the block under
# `if ((start2 - ip) < OPTIMAL_ML)`), the jumps back from "ML3 replaces ML2" and from "ML2 becomes ML1" included.  Behind it,
# with d = start2 - ip < 18: without the second clamp new_ml = min(ml, 18); then either correction > 0 and start2 = ip +
# min(ml, 18), or correction <= 0, which says start2 - ip >= min(ml, 18) > d only if ml <= d, that is start2 >= ip + ml.
# All three fail `start2 < ip + ml && start2 - ip < 18`.  With the second clamp new_ml = d + ml2 - 4 and correction = ml2 - 4,
# at least 1 since ml2 > 4 whenever a second match exists; ml2 becomes exactly 4 and start2 + 4 = the old start2 + ml2.  The
# third search then runs from start2 + ml2 - 3 = start2 + 1 with iLowLimit = start2, so start3 is start2 or start2 + 1,
# while the ascending case needs start3 >= ip + ml + 3 > start2 + 3.  So line 229 takes every such case and line 246 is never
# true.  The seeded search (gen_lz4hc_traps.py --search 15000: 30000 inputs of sm_input(), each at levels 3 and 8) never reached it.
UNREACHABLE = ("asc.opt",)

BULK = ("first.none", "try.longer", "s2.search", "s2.same", "restore.no")   # counted, positions not kept


class Trace:
    def __init__(self):
        self.count = collections.Counter()
        self.where = collections.defaultdict(set)       # label -> search positions (frame coordinates), but for BULK
        self.blocks = []                                # per block: (stored, [(position, literals, match length, offset)], last literals)
        self.backs = collections.defaultdict(list)      # search position -> lengths of the backward extensions made there

    def hit(self, label, pos):
        assert label in LABELS, label
        self.count[label] += 1
        if label not in BULK:
            self.where[label].add(pos)

    def __contains__(self, label):
        return self.count[label] > 0

    def at(self, label, pos):
        return pos in self.where[label]

    def labels(self):
        return sorted(self.count)


def xxh32(b, seed=0):
    P1, P2, P3, P4, P5, M = 2654435761, 2246822519, 3266489917, 668265263, 374761393, 0xffffffff
    rot = lambda x, r: ((x << r) | (x >> (32 - r))) & M
    n, p = len(b), 0
    if n >= 16:
        v = [(seed + P1 + P2) & M, (seed + P2) & M, seed, (seed - P1) & M]
        words = struct.unpack_from("<%dI" % (n // 16 * 4), b, 0)
        for i, w in enumerate(words):
            k = i & 3
            v[k] = (rot((v[k] + w * P2) & M, 13) * P1) & M
        p = n // 16 * 16
        h = (rot(v[0], 1) + rot(v[1], 7) + rot(v[2], 12) + rot(v[3], 18)) & M
    else:
        h = (seed + P5) & M
    h = (h + n) & M
    while p + 4 <= n:
        h = (rot((h + u32(b, p) * P3) & M, 17) * P4) & M; p += 4
    while p < n:
        h = (rot((h + b[p] * P5) & M, 11) * P1) & M; p += 1
    h ^= h >> 15; h = (h * P2) & M; h ^= h >> 13; h = (h * P3) & M; h ^= h >> 16
    return h


class _HC:
    """LZ4HC_CCtx_internal after LZ4HC_init_internal on a fresh state: the frame's first byte has index 65536, dictLimit =
    lowLimit = 65536, the tables are zero"""

    def __init__(self, src):
        self.src = src
        self.hash = [0] * 32768
        self.chain = [0] * 65536
        self.next = 65536
        self.low = 65536

    def insert(self, target):
        """LZ4HC_Insert: every index below target"""
        src, hasht, chain = self.src, self.hash, self.chain
        idx = self.next
        while idx < target:
            p = idx - 65536
            h = hash_hc(src[p] | src[p + 1] << 8 | src[p + 2] << 16 | src[p + 3] << 24)
            delta = idx - hasht[h]
            chain[idx & 0xffff] = MAXD if delta > MAXD else delta
            hasht[h] = idx
            idx += 1
        self.next = target                                          # (as the source has it: unconditionally)

    def wider(self, ip, ilow, ihigh, longest, attempts, T):
        """LZ4HC_InsertAndGetWiderMatch(ip, iLowLimit, iHighLimit, longest) -> (longest, matchpos, startpos); positions are
        the frame's, matchpos / startpos None when `longest` was not beaten"""
        src = self.src
        ipi = ip + 65536
        lowest = self.low if self.low + 65536 > ipi else ipi - MAXD
        look = ip - ilow
        pattern = src[ip:ip + 4]
        mpos = spos = None
        self.insert(ipi)
        mi = self.hash[hash_hc(u32(src, ip))]
        if mi < lowest:
            T.hit("first.none" if mi == 0 else "first.below", ip)
            return longest, mpos, spos
        if ipi - mi == MAXD:
            T.hit("first.at65535", ip)
        nd = 0
        while mi >= lowest and attempts > 0:
            attempts -= 1
            m = mi - 65536
            a, b = ilow + longest - 1, m - look + longest - 1
            if src[a:a + 2] == src[b:b + 2]:
                if src[m:m + 4] == pattern:
                    back = 0
                    if look:
                        lim = min(look, m)                          # max(iMin - ip, mMin - match), mMin the frame's first byte
                        while back < lim and src[ip - back - 1] == src[m - back - 1]:
                            back += 1
                        T.backs[ip].append(back)
                        T.hit("back.ilow" if back == look else "back.prefix" if back == m else "back.mismatch", ip)
                    f = 0
                    x, y = ip + 4, m + 4
                    while x + f < ihigh and src[x + f] == src[y + f]:
                        f += 1
                    if x + f == ihigh:
                        T.hit("count.limit", ip)
                    ml = MINMATCH + f + back
                    if ml > longest:
                        longest, mpos, spos = ml, m - back, ip - back
                        T.hit("try.longer", ip)
                    else:
                        T.hit("try.equal" if ml == longest else "try.shorter", ip)
                else:
                    T.hit("try.word_fail", ip)
            else:
                T.hit("try.pre16_fail", ip)
            nd = self.chain[mi & 0xffff]
            mi -= nd
        if mi >= lowest:
            T.hit("walk.end_attempts", ip)
        else:
            T.hit("walk.end_capped" if nd == MAXD else "walk.end_below", ip)
        return longest, mpos, spos


class _Overflow(Exception):
    pass


def _hash_chain(hc, bs, be, cap, attempts, T):
    """LZ4HC_compress_hashChain of src[bs:be) with limitedOutput into cap bytes (cap None: notLimited) -> (block or None when
    it does not fit, [(position, literals, match length, offset)], last literals)"""
    src = hc.src
    out = bytearray()
    seqs = []
    st = {"ip": bs, "anchor": bs}

    def encode(ml, ref):
        ip, anchor = st["ip"], st["anchor"]
        length = ip - anchor
        token_at = len(out); out.append(0)
        if cap is not None and len(out) + length // 255 + length + (2 + 1 + LASTLIT) > cap:
            T.hit("fit.literals", ip)
            raise _Overflow
        if length >= 15:
            tok = 15 << 4; ln = length - 15
            while ln >= 255:
                out.append(255); ln -= 255
            out.append(ln)
        else:
            tok = length << 4
        out.extend(src[anchor:ip])
        off = ip - ref
        assert 0 < off <= MAXD
        out.append(off & 255); out.append(off >> 8)
        ln = ml - MINMATCH
        if cap is not None and len(out) + ln // 255 + (1 + LASTLIT) > cap:
            T.hit("fit.match", ip)
            raise _Overflow
        if ln >= 15:
            tok += 15; ln -= 15
            while ln >= 255:
                out.append(255); ln -= 255
            out.append(ln)
        else:
            tok += ln
        out[token_at] = tok
        seqs.append((ip, length, ml, off))
        st["ip"] = st["anchor"] = ip + ml

    try:
        if be - bs >= MFLIMIT + 1:
            mflimit, matchlimit = be - MFLIMIT, be - LASTLIT
            while st["ip"] <= mflimit:
                ip = st["ip"]
                ml, ref, _ = hc.wider(ip, ip, matchlimit, MINMATCH - 1, attempts, T)
                if ml < MINMATCH:
                    st["ip"] = ip + 1
                    continue
                start0, ref0, ml0 = ip, ref, ml
                state = "search2"
                while state != "main":
                    if state == "search2":
                        if ip + ml <= mflimit:
                            T.hit("s2.search", ip)
                            ml2, r2, s2 = hc.wider(ip + ml - 2, ip, matchlimit, ml, attempts, T)
                            if ml2 > ml:
                                ref2, start2 = r2, s2
                        else:
                            T.hit("s2.nosearch", ip)
                            ml2 = ml
                        if ml2 == ml:
                            T.hit("s2.same", ip)
                            st["ip"] = ip
                            encode(ml, ref)
                            state = "main"
                            continue
                        if start0 < ip and start2 < ip + ml0:
                            T.hit("restore.yes", ip)
                            ip, ref, ml = start0, ref0, ml0
                        else:
                            T.hit("restore.no", ip)
                        if start2 - ip < 3:
                            T.hit("small.d%d" % (start2 - ip), ip)
                            ml, ip, ref = ml2, start2, ref2
                            continue
                        T.hit("small.d3plus", ip)
                        state = "search3"
                    # _Search3
                    if start2 - ip < OPTIMAL_ML:
                        new_ml = ml
                        if new_ml > OPTIMAL_ML:
                            T.hit("opt.ml_gt18", ip)
                            new_ml = OPTIMAL_ML
                        else:
                            T.hit("opt.ml_le18", ip)
                        if ip + new_ml > start2 + ml2 - MINMATCH:
                            T.hit("opt.clamp2", ip)
                            new_ml = (start2 - ip) + ml2 - MINMATCH
                        correction = new_ml - (start2 - ip)
                        if correction > 0:
                            T.hit("opt.corr_pos", ip)
                            start2 += correction; ref2 += correction; ml2 -= correction
                        else:
                            T.hit("opt.corr_nonpos", ip)
                    else:
                        T.hit("opt.out", ip)
                    if start2 + ml2 <= mflimit:
                        T.hit("s3.search", ip)
                        ml3, r3, s3 = hc.wider(start2 + ml2 - 3, start2, matchlimit, ml2, attempts, T)
                        if ml3 > ml2:
                            ref3, start3 = r3, s3
                    else:
                        T.hit("s3.nosearch", ip)
                        ml3 = ml2
                    if ml3 == ml2:
                        if start2 < ip + ml:
                            T.hit("s3.same_trim", ip)
                            ml = start2 - ip
                        else:
                            T.hit("s3.same_notrim", ip)
                        st["ip"] = ip
                        encode(ml, ref)
                        st["ip"] = start2
                        encode(ml2, ref2)
                        state = "main"
                        continue
                    if start3 < ip + ml + 3:
                        T.hit("s3.nospace", ip)
                        if start3 >= ip + ml:
                            T.hit("s3.seq1_now", ip)
                            if start2 < ip + ml:
                                T.hit("s3.cut", ip)
                                correction = ip + ml - start2
                                start2 += correction; ref2 += correction; ml2 -= correction
                                if ml2 < MINMATCH:
                                    T.hit("s3.ml2_dead", ip)
                                    start2, ref2, ml2 = start3, ref3, ml3
                                else:
                                    T.hit("s3.ml2_alive", ip)
                            else:
                                T.hit("s3.nocut", ip)
                            st["ip"] = ip
                            encode(ml, ref)
                            ip, ref, ml = start3, ref3, ml3
                            start0, ref0, ml0 = start2, ref2, ml2
                            state = "search2"
                            continue
                        T.hit("s3.replace", ip)
                        start2, ref2, ml2 = start3, ref3, ml3
                        state = "search3"
                        continue
                    if start2 < ip + ml:
                        T.hit("asc.overlap", ip)
                        if start2 - ip < OPTIMAL_ML:
                            T.hit("asc.opt", ip)
                            if ml > OPTIMAL_ML:
                                ml = OPTIMAL_ML
                            if ip + ml > start2 + ml2 - MINMATCH:
                                ml = (start2 - ip) + ml2 - MINMATCH
                            correction = ml - (start2 - ip)
                            if correction > 0:
                                start2 += correction; ref2 += correction; ml2 -= correction
                        else:
                            T.hit("asc.plain", ip)
                            ml = start2 - ip
                    else:
                        T.hit("asc.nooverlap", ip)
                    st["ip"] = ip
                    encode(ml, ref)
                    ip, ref, ml = start2, ref2, ml2
                    start2, ref2, ml2 = start3, ref3, ml3
                    state = "search3"
        lr = be - st["anchor"]
        if cap is not None and len(out) + 1 + (lr + 255 - 15) // 255 + lr > cap:
            T.hit("fit.last", st["anchor"])
            raise _Overflow
    except _Overflow:
        return None, seqs, None
    if lr >= 15:
        out.append(15 << 4); acc = lr - 15
        while acc >= 255:
            out.append(255); acc -= 255
        out.append(acc)
    else:
        out.append(lr << 4)
    out.extend(src[st["anchor"]:be])
    return bytes(out), seqs, lr


def model(src, level, limited=True):
    """LZ4F_compressFrame(contentChecksum, contentSize, 64 KB blocks, autoFlush, compressionLevel = level) -> (frame, Trace).
    One hash-chain state for the whole frame above 64 KB (linked blocks: every block continues the tables of the one before,
    whether that one was stored or not); a block is stored when it does not fit n - 1 bytes.  limited=False: every block is
    compressed whatever its size (notLimited) - what a block would have come to."""
    src = bytes(src)
    n = len(src)
    attempts = attempts_of(level)
    T = Trace()
    flg = (1 << 6) | ((1 << 5) if n <= MAXBLK else 0) | ((1 << 3) if n else 0) | (1 << 2)
    desc = bytes([flg, 4 << 4]) + (struct.pack("<Q", n) if n else b"")
    out = bytearray(b"\x04\x22\x4d\x18" + desc + bytes([(xxh32(desc) >> 8) & 0xff]))
    hc = _HC(src)
    for bs in range(0, n, MAXBLK):
        be = min(n, bs + MAXBLK)
        blk, seqs, last = _hash_chain(hc, bs, be, (be - bs - 1) if limited else None, attempts, T)
        T.blocks.append((blk is None, seqs, last))
        if blk is None:
            out += struct.pack("<I", (be - bs) | 0x80000000) + src[bs:be]
        else:
            out += struct.pack("<I", len(blk)) + blk
    out += struct.pack("<II", 0, xxh32(src))
    return bytes(out), T


# ------------------------------------------------------------------------------------------------ building blocks
Trap = collections.namedtuple("Trap", "name family data levels aim check")
_TRAPS = []


def trap(name, family, data, levels, aim, check):
    _TRAPS.append(Trap(name, family, bytes(data), tuple(levels), aim, check))


def has_at(pos, ml, off, blk=0):
    return lambda bl, tr, lvl: not bl[blk].stored and (pos, ml, off) in bl[blk].at


def none_at(lo, hi, blk=0):
    """no match begins in [lo, hi)"""
    return lambda bl, tr, lvl: not bl[blk].stored and not any(lo <= a[0] < hi for a in bl[blk].at)


def fired(label, pos=None):
    return lambda bl, tr, lvl: (label in tr) if pos is None else tr.at(label, pos)


def both(*cs):
    return lambda bl, tr, lvl: all(c(bl, tr, lvl) for c in cs)


S1 = 4096                   # the size class of the hand-built block traps
SM_SIZES = (256, 1024)      # the size classes of the searched ones
NL1 = 2 * MAXBLK            # linked: block 1 reaches 65535 back into block 0
NL2 = 2 * MAXBLK + 4096     # linked: a short block 2 behind two whole ones
LINKED_LEVELS = (3, 8)


def linked(n, seed, blk):
    """filler of n bytes whose block blk shrinks whatever else happens (a long copy of its own first bytes at its far end: a
    stored block would hide the trap's decision)"""
    B = Buf(n, seed)
    B.ballast(160 if min(n, (blk + 1) * MAXBLK) - blk * MAXBLK <= S1 else 700, blk * MAXBLK)
    return B


def scrub(B, at):
    """The hash has 15 bits: in 64 KB of filler every word has a few positions with its hash and other bytes in front of
    it, each one a candidate that costs an attempt.  This takes them away for the word at `at`: every earlier position with
    that hash and another word gets a byte changed, so that the chain of `at` holds what the trap planted and nothing else."""
    b = B.b
    want = bytes(b[at:at + 4])
    h = hash_hc(u32(want, 0))
    for _ in range(64):
        a = np.frombuffer(bytes(b[:at + 3]), np.uint8).astype(np.uint32)
        words = a[:-3] | a[1:-2] << 8 | a[2:-1] << 16 | a[3:] << 24
        hit = [int(p) for p in np.nonzero((words * np.uint32(2654435761)) >> 17 == h)[0] if bytes(b[p:p + 4]) != want]
        if not hit:
            return B
        for p in hit:
            b[p] ^= 0x40 >> (_ % 6)
    raise AssertionError("scrub does not end")


# ------------------------------------------------------------------------------------------------ A: chains and the first candidate
def _family_a():
    # (That the last three positions of a frame are never inserted shows in no frame: nothing can match a word that ends
    # behind the input.  What can go wrong there is the read itself, and the sanitizer program of
    # tests/test_sim_lz4hc_traps.py, with every input in a buffer of exactly its size, is the check for it.)
    cur = MAXBLK + 3000
    for dist in (65534, 65535, 65536):
        B = scrub(linked(NL1, 200, 1).plant(cur, cur - dist, 12), cur)
        if dist <= MAXD:
            chk = has_at(cur, 12, dist, 1)
            if dist == MAXD:
                chk = both(chk, fired("first.at65535", cur))
        else:
            chk = both(none_at(cur - 3, cur + 12, 1), fired("first.below", cur))
        trap("a_only_copy_at_%d" % dist, "A", B.bytes(), LINKED_LEVELS,
             "the only earlier copy of 12 bytes lies %d back: %s" % (dist, "taken with that offset" if dist <= MAXD else "not taken"), chk)
    cur = MAXBLK + 6000
    B = scrub(linked(NL1, 201, 1).plant(cur - 65535, cur - 70000, 12).plant(cur, cur - 65535, 12), cur)
    trap("a_copies_at_65535_and_70000", "A", B.bytes(), LINKED_LEVELS, "copies 65535 and 70000 back: the one at 65535 is the first candidate",
         both(has_at(cur, 12, 65535, 1), fired("first.at65535", cur)))
    B = linked(NL1, 202, 1)
    B.put(cur, COLLIDE[0]).plant(cur - 70000, cur, 12)
    scrub(B, cur).put(cur - 65535, COLLIDE[1])
    trap("a_collision_at_65535", "A", B.bytes(), LINKED_LEVELS,
         "the copy lies 70000 back, the word 65535 back has the hash and other bytes: it costs an attempt, its chain entry leads below the window",
         both(none_at(cur - 3, cur + 12, 1), fired("first.at65535", cur), fired("try.pre16_fail", cur), fired("walk.end_below", cur)))
    cur = 2 * MAXBLK + 3000
    B = scrub(linked(NL2, 203, 2).plant(cur, 60000, 12), cur)
    trap("a_copy_only_in_block0_from_block2", "A", B.bytes(), LINKED_LEVELS, "block 2's string has its only copy in block 0, below block 2's window: no match",
         both(none_at(cur - 3, cur + 12, 2), fired("first.below", cur)))
    B = scrub(linked(NL2, 204, 2).plant(70000, 60000, 12).plant(cur, 70000, 12), cur)
    trap("a_predecessor_below_window", "A", B.bytes(), LINKED_LEVELS,
         "the candidate at 70000 has a predecessor of its own at 60000, below block 2's window start: taken, and the walk ends there",
         both(has_at(cur, 12, cur - 70000, 2), fired("walk.end_below", cur)))
    cur = MAXBLK + 3000
    B = scrub(linked(NL1, 205, 1).plant(MAXBLK + 1500, MAXBLK + 500, 12).plant(cur, MAXBLK + 500, 12), cur)
    trap("a_capped_entry_mid_walk", "A", B.bytes(), LINKED_LEVELS, "two candidates, the second one's chain entry is capped (no predecessor): the walk ends at it",
         both(has_at(cur, 12, 1500, 1), fired("walk.end_capped", cur)))
    B = scrub(linked(NL1, 206, 1).plant(cur, MAXBLK - 2, 12), cur)
    trap("a_word_straddles_block_border", "A", B.bytes(), LINKED_LEVELS,
         "the four bytes at 65534 straddle the border of blocks 0 and 1: inserted by block 1's first search and found from it", has_at(cur, 12, 3002, 1))
    # the 64 positions of one trip of the chain kernel: 1024 .. 1087
    for k in (2, 3):
        B = Buf(S1, 210 + k); B.ballast()
        for i in range(1, k):
            B.plant(1030 + 10 * i, 1030, 8)
        B.plant(2000, 1030, 8)
        last = 1030 + 10 * (k - 1)
        trap("a_trip_same_word_%d_times" % k, "A", B.bytes(), LEVELS, "the same word %d times inside one trip (1024..1087), met again at 2000: the nearest one" % k,
             both(has_at(1040, 8, 10), has_at(last, 8, 10), has_at(2000, 8, 2000 - last)))
    B = Buf(S1, 213); B.ballast()
    B.put(1060, b"\x5a" * 200); B.b[1059] = 0x11; B.b[1260] = 0x22
    trap("a_one_byte_run", "A", B.bytes(), LEVELS, "a run of one byte over three trips: every lane carries the same hash at distance 1, across 1087 / 1088 too",
         has_at(1061, 199, 1))
    for per in (2, 3, 63, 64, 65):
        B = Buf(S1, 220 + per); B.ballast()
        pat = bytes(B.b[1060:1060 + per])
        B.put(1060, (pat * (400 // per + 1))[:400])
        B.b[1059] = pat[-1] ^ 0x55; B.b[1460] = pat[400 % per] ^ 0x55
        trap("a_period_%d" % per, "A", B.bytes(), LEVELS, "period %d from 1060 on: position %d finds 1060" % (per, 1060 + per), has_at(1060 + per, 400 - per, per))
    B = Buf(S1, 230); B.ballast()
    B.put(1087, COLLIDE_SHIFT).put(1100, COLLIDE_SHIFT)
    B.plant(2000, 1088, 8).plant(2100, 1101, 8)
    trap("a_collision_in_a_trip_and_across_trips", "A", B.bytes(), LEVELS,
         "abcde with hash(abcd) == hash(bcde) at 1087 (lanes 63 / 0 of two trips) and at 1100 (lanes 12 / 13 of one): the chains hold both words in order",
         both(has_at(1100, 5, 13), has_at(2000, 8, 912), has_at(2100, 8, 999), fired("try.pre16_fail", 2000)))


# ------------------------------------------------------------------------------------------------ B: attempts
def _attempt_trap(k, seed):
    """cur = 3000 holds W T (24 bytes).  Its k-th candidate, the farthest, is the only whole copy.  The k - 1 nearer ones,
    16 bytes apart, hold W T[0:4] and then another byte: the nearest gives a match of 8, the others fail the 16-bit
    pre-check.  Each also holds T[2:6] on its own: the word of the second search behind a match of 8, so that search burns
    its attempts as well and cannot make good what the first one missed."""
    B = Buf(S1, seed); B.ballast()
    cur = 3000
    W, T = rnd(4, seed + 1000), rnd(20, seed + 2000)
    far = cur - 16 * (k - 1) - 32
    B.put(cur, W + T).put(far, W + T)
    B.b[cur + 24] = B.b[far + 24] ^ 0x55
    for i in range(1, k):
        f = cur - 16 * i
        B.put(f, W + T[:4] + bytes([T[4] ^ (1 + i % 200)]))
        B.put(f + 10, T[2:6])
        B.b[f + 14] = T[6] ^ (1 + i % 200)
        B.b[f + 9] = T[1] ^ (1 + i % 200)
        B.b[f + 15] = (0x80 + i) & 255
    B.b[far - 1] = B.b[cur - 1] ^ 0x55
    for at in range(cur, cur + 21):                      # every search around cur spends its attempts on what is planted
        scrub(B, at)
    return B.bytes(), cur, cur - far


def _family_b():
    for lvl in LEVELS:
        a = attempts_of(lvl)
        for k in (a, a + 1):
            data, cur, off = _attempt_trap(k, 300 + k)
            chk = lambda bl, tr, L, k=k, cur=cur, off=off: (
                (cur, 24, off) in bl[0].at if attempts_of(L) >= k else
                ((cur, 8, 16) in bl[0].at and (cur + 8, 16, off) in bl[0].at and tr.at("walk.end_attempts", cur) and tr.at("walk.end_attempts", cur + 6)))
            trap("b_long_candidate_is_number_%d" % k, "B", data, LEVELS,
                 "the only whole copy is candidate %d: levels with at least %d attempts take it, the others write 8 + 16" % (k, k), chk)
    for tag, pair, label in (("pre16", COLLIDE, "try.pre16_fail"), ("word", COLLIDE_LOW, "try.word_fail")):
        B = Buf(S1, 340); B.ballast()
        cur = 3000
        T = rnd(20, 341)
        B.put(cur, pair[0] + T).put(2000, pair[0] + T)
        B.b[cur + 24] = B.b[2024] ^ 0x55; B.b[cur - 1] = B.b[1999] ^ 0x55
        scrub(B, cur); scrub(B, cur + 1)
        for i in range(1, 5):
            B.put(cur - 16 * i, pair[1])
        chk = lambda bl, tr, L, cur=cur, label=label: (
            (cur, 24, 1000) in bl[0].at if attempts_of(L) >= 5 else ((cur + 1, 23, 1000) in bl[0].at and tr.at("walk.end_attempts", cur))) and tr.at(label, cur)
        trap("b_colliding_candidates_%s" % tag, "B", B.bytes(), LEVELS,
             "four words with the hash and other bytes (they fail the %s) in front of the copy: level 3 spends its attempts on them" %
             ("16-bit pre-check" if tag == "pre16" else "word compare"), chk)


# ------------------------------------------------------------------------------------------------ C: the search
def _family_c():
    # a candidate as long as `longest` passes the 16-bit pre-check only if the byte behind the match agrees too: two
    # candidates are equal where matchlimit cuts both.  30 bytes at 3000, at 3500 and as the block's last 30
    B = Buf(S1, 400).plant(1000, 8, 160).plant(3500, 3000, 30)
    B.plant(S1 - 30, 3000, 30)
    scrub(B, S1 - 30)
    trap("c_equal_lengths_first_met_stays", "C", B.bytes(), LEVELS, "two candidates that both run into matchlimit, 25 bytes each: the nearer one, met first, stays",
         both(has_at(S1 - 30, 25, S1 - 30 - 3500), fired("try.equal", S1 - 30)))
    B = Buf(S1, 401); B.ballast()
    B.plant(1500, 500, 12).plant(2500, 500, 13)
    trap("c_farther_one_byte_longer", "C", B.bytes(), LEVELS, "the farther candidate is one byte longer: it wins", has_at(2500, 13, 2000))
    for ln in (255, 256, 257, 259, 260, 261):
        B = Buf(S1, 402); B.ballast()
        B.plant(2000, 500, ln)
        trap("c_forward_%d" % ln, "C", B.bytes(), LEVELS, "a match of exactly %d bytes (the wave compare takes 256 a trip)" % ln, has_at(2000, ln, 1500))
    # backward extension of 63, 64, 65 bytes in the second search: ML1 = 80 bytes of A = a[0:j] + b[0:80 - j] at 2000, and the
    # 120 bytes of b from 2000 + j on; the search at 2000 + 78 meets b and walks back to 2000 + j
    for back in (63, 64, 65):
        j = 78 - back
        B = Buf(S1, 410 + back); B.ballast()
        B.plant(1000 + j, 600, 80 - j)
        B.plant(2000, 1000, 80)
        B.plant(2000 + j, 600, 120)
        trap("c_back_%d" % back, "C", B.bytes(), LEVELS,
             "the second search at 2078 meets a longer match and walks %d bytes back to %d, stopped by a differing byte" % (back, 2000 + j),
             both(lambda bl, tr, L, back=back: back in tr.backs[2078], fired("back.mismatch", 2078), has_at(2000, 18, 1000),
                  has_at(2018, 102 + j, 1400 + j)))


# ------------------------------------------------------------------------------------------------ C / D: the searched inputs
def sm_input(seed, n):
    """n bytes over a small alphabet with overlapping planted copies and a few stretches of random bytes"""
    rs = np.random.RandomState(seed)
    k = int(rs.randint(2, 7))
    b = bytearray(rs.randint(0, k, n, dtype=np.uint8).tobytes())
    for _ in range(int(rs.randint(0, 4))):
        ln = int(rs.randint(4, 40)); a = int(rs.randint(0, n - ln))
        b[a:a + ln] = rs.randint(0, 256, ln, dtype=np.uint8).tobytes()
    for _ in range(int(rs.randint(0, 14))):
        ln = int(rs.randint(5, min(100, n // 3)))
        a = int(rs.randint(0, n - 2 * ln)); d = int(rs.randint(a + 1, n - ln))
        for i in range(ln):
            b[d + i] = b[a + i]
        if rs.randint(0, 2):
            b[d + int(rs.randint(0, ln))] ^= 1          # a copy with one byte changed: two matches that overlap a third
    return bytes(b)


# label -> (size class, seed): the smallest input of the search (gen_lz4hc_traps.py --search) whose trace holds the label at
# every level 3-8
SM_SEEDS = {
    "try.word_fail": (256, 2124),
    "try.equal": (256, 0),
    "try.shorter": (256, 1),
    "back.ilow": (256, 2),
    "back.prefix": (256, 2),
    "s2.search": (256, 0),
    "s2.nosearch": (256, 0),
    "s2.same": (256, 0),
    "restore.yes": (256, 13),
    "restore.no": (256, 2),
    "small.d1": (256, 2),
    "small.d2": (256, 2),
    "small.d3plus": (256, 2),
    "opt.out": (256, 14),
    "opt.ml_gt18": (256, 3),
    "opt.ml_le18": (256, 2),
    "opt.clamp2": (256, 3004),
    "opt.corr_pos": (256, 2),
    "opt.corr_nonpos": (256, 21),
    "s3.search": (256, 2),
    "s3.nosearch": (256, 39),
    "s3.same_trim": (256, 3),
    "s3.same_notrim": (256, 2),
    "s3.nospace": (256, 2),
    "s3.seq1_now": (256, 2),
    "s3.cut": (256, 101),
    "s3.nocut": (256, 2),
    "s3.ml2_dead": (1024, 1342),
    "s3.ml2_alive": (256, 101),
    "s3.replace": (256, 422),
    "asc.overlap": (256, 597),
    "asc.nooverlap": (256, 23),
    "asc.plain": (256, 597),
}
SM_FAMILY = {"try.shorter": "C", "back.ilow": "C", "back.prefix": "C", "back.mismatch": "C"}


def _family_sm():
    by_input = collections.OrderedDict()
    for label in LABELS:
        if label in SM_SEEDS:
            by_input.setdefault(SM_SEEDS[label], []).append(label)
    for (n, seed), labels in by_input.items():
        fam = "C" if all(x in SM_FAMILY for x in labels) else "D"
        trap("%s_searched_%d_%d" % (fam.lower(), n, seed), fam, sm_input(seed, n), LEVELS, "fires " + ", ".join(labels),
             lambda bl, tr, L, labels=labels: not bl[0].stored and all(x in tr for x in labels))


# ------------------------------------------------------------------------------------------------ E: the encoder and the ends
def _family_e():
    for lit in (14, 15, 269, 270):
        B = Buf(S1, 500); B.ballast()
        B.plant(lit, 0, 10)
        trap("e_literals_%d" % lit, "E", B.bytes(), LEVELS, "a first literal run of exactly %d bytes" % lit,
             lambda bl, tr, L, lit=lit: bl[0].seqs[0] == (lit, 10, lit))
    for ml in (18, 19, 273, 274):
        B = Buf(S1, 501); B.ballast()
        B.plant(2000, 500, ml)
        trap("e_match_%d" % ml, "E", B.bytes(), LEVELS, "a match of exactly %d bytes" % ml, has_at(2000, ml, 1500))
    for last in (14, 15, 270):
        B = Buf(S1, 502)
        B.plant(1000, 8, 160)
        B.plant(S1 - last - 20, 300, 20, guard=False)
        B.b[S1 - last - 21] = B.b[299] ^ 0x55; B.b[S1 - last] = B.b[320] ^ 0x55
        trap("e_last_literals_%d" % last, "E", B.bytes(), LEVELS, "%d last literals" % last,
             lambda bl, tr, L, last=last: not bl[0].stored and bl[0].last == last and bl[0].at[-1] == (S1 - last - 20, 20, S1 - last - 320))
    for n in range(0, 14):
        trap("e_n%d" % n, "E", rnd(n, 510 + n), LEVELS, "%d random bytes: %s" % (n, "no block" if n == 0 else "stored"),
             (lambda bl, tr, L: bl == []) if n == 0 else (lambda bl, tr, L: len(bl) == 1 and bl[0].stored))
    trap("e_13_equal_bytes", "E", b"\x07" * 13, LEVELS, "13 equal bytes: position 1 is searched, the match stops at n - 5",
         lambda bl, tr, L: not bl[0].stored and bl[0].seqs == [(1, 7, 1)] and bl[0].last == 5)
    for d in (12, 11):
        n = 96
        B = Buf(n, 520).plant(61, 10, 20)
        B.plant(n - d, 40, 8, guard=False)
        B.b[n - d - 1] = B.b[39] ^ 0x55
        if d == 12:
            chk = lambda bl, tr, L: bl[0].seqs == [(61, 20, 51), (3, 7, 44)] and bl[0].last == 5
        else:
            chk = lambda bl, tr, L: bl[0].seqs == [(61, 20, 51)] and bl[0].last == 15
        trap("e_last_match_at_end_minus_%d" % d, "E", B.bytes(), LEVELS,
             "a repeat from be - %d on: %s" % (d, "searched (ip == mflimit) and taken" if d == 12 else "behind mflimit, never searched"), chk)
    n, dst = 120, 40
    B = Buf(n, 521).plant(dst, 4, n - dst)
    trap("e_match_stops_five_short", "E", B.bytes(), LEVELS, "the copy runs to the block's end: the match stops at be - 5",
         both(lambda bl, tr, L: bl[0].seqs == [(40, 75, 36)] and bl[0].last == 5, fired("count.limit", 40)))
    # the three "does not fit" exits, each on a block that would come to n bytes exactly (stored), with a twin that comes to
    # n - 1 (kept).  Sizes: a sequence costs 1 + ext(lit) + lit + 2 + ext'(ml - 4), the end 1 + ext(last) + last.
    #   last literals: one match of m bytes at 2000: n - m + 4 + 8 + 9 + 1 -> m = 22 gives n, m = 23 gives n - 1
    #   match:        matches of mA at 2000 and of 10 at n - 15: n - mA - 10 + 7 + 8 + 9 -> mA = 14 gives n; the second
    #                 sequence's literal run passes its check by one byte, the match check fails by one
    #   literals:     the second literal run is 8 * 255 + 5 bytes (its length / 255 is what its extension bytes are): mA = 13
    #                 at 2023 gives n and the run's check fails by one; mA = 14 at 2022 gives n - 1
    for name, plants, label in (("last", ((2000, 22),), "fit.last"), ("last_twin", ((2000, 23),), None),
                                ("match", ((2000, 14), (S1 - 15, 10)), "fit.match"), ("match_twin", ((2000, 15), (S1 - 15, 10)), None),
                                ("literals", ((2023, 13), (S1 - 15, 10)), "fit.literals"), ("literals_twin", ((2022, 14), (S1 - 15, 10)), None)):
        B = Buf(S1, 530)
        for i, (at, ml) in enumerate(plants):
            B.plant(at, 100 + 40 * i, ml, guard=False)
            B.b[at - 1] = B.b[100 + 40 * i - 1] ^ 0x55
            if at + ml < S1 - LASTLIT:
                B.b[at + ml] = B.b[100 + 40 * i + ml] ^ 0x55
        data = B.bytes()
        if label:
            chk = lambda bl, tr, L, label=label, data=data: (bl[0].stored and label in tr and
                                                             model(data, L, limited=False)[1].blocks[0][0] is False and
                                                             len(model(data, L, limited=False)[0]) == 15 + 4 + S1 + 8)
            aim = "the block would come to n bytes exactly; %s gives up and it is stored" % LABELS[label]
        else:
            chk = lambda bl, tr, L, plants=plants: (not bl[0].stored and [a[:2] for a in bl[0].at] == [tuple(p) for p in plants] and
                                                    sum(1 + (s[0] >= 15) + max(0, s[0] - 15) // 255 + s[0] + 2 + (s[1] >= 19) for s in bl[0].seqs) +
                                                    1 + (bl[0].last >= 15) + max(0, bl[0].last - 15) // 255 + bl[0].last == S1 - 1)
            aim = "the twin: the block comes to n - 1 bytes and is kept"
        trap("e_does_not_fit_%s" % name, "E", data, LEVELS, aim, chk)


# ------------------------------------------------------------------------------------------------ F: geometry
def _family_f():
    for n, what in ((2 * MAXBLK + 1, "the last block holds one byte"), (MAXBLK + 12, "a last block of 12 bytes: stored, nothing searched"),
                    (MAXBLK + 13, "a last block of 13 bytes (bytes 30000.. again): the first size that is searched")):
        B = Buf(n, 600)
        B.plant(60000, 8, 700)
        if n > 2 * MAXBLK:
            B.plant(MAXBLK + 60000, MAXBLK + 8, 700)
        tail = n % MAXBLK
        B.plant(n - tail, 30000, tail, guard=False)
        if tail == 13:
            chk = lambda bl, tr, L: len(bl) == 2 and not bl[0].stored and not bl[1].stored and bl[1].seqs == [(0, 8, MAXBLK - 30000)] and bl[1].last == 5
        else:
            chk = lambda bl, tr, L, tail=tail, n=n: len(bl) == (n + MAXBLK - 1) // MAXBLK and bl[-1].stored and bl[-1].raw == tail and not bl[0].stored
        trap("f_frame_of_%d" % n, "F", B.bytes(), LINKED_LEVELS, what, chk)
    # the farthest a block can reach: block 2's first byte matches 65535 back, block 1's second byte (block 1's first byte,
    # the window's start, is 65536 away from block 2's first: no position of block 2 reaches it)
    B = scrub(linked(NL2, 601, 2).plant(2 * MAXBLK, MAXBLK + 1, 12), 2 * MAXBLK)
    trap("f_block2_first_byte_reaches_65535_back", "F", B.bytes(), LINKED_LEVELS,
         "block 2's first twelve bytes are block 1's bytes 1..12: offset 65535, the lowest position its window offers",
         both(lambda bl, tr, L: not bl[2].stored and bl[2].seqs[0] == (0, 12, 65535), fired("first.at65535", 2 * MAXBLK)))


_BUILT = None


def all_traps():
    """every trap, in a fixed order (built once per process)"""
    global _BUILT
    if _BUILT is None:
        del _TRAPS[:]
        for fam in (_family_a, _family_b, _family_c, _family_sm, _family_e, _family_f):
            fam()
        names = [t.name for t in _TRAPS]
        assert len(set(names)) == len(names)
        for t in _TRAPS:
            assert len(t.data) <= S1 or len(t.data) > MAXBLK, t.name
        _BUILT = list(_TRAPS)
    return _BUILT


def is_linked(t):
    return len(t.data) > MAXBLK


def by_size(traps):
    """block traps grouped by their size: equal-size traps are the frames of one call"""
    groups = collections.OrderedDict()
    for t in traps:
        if not is_linked(t):
            groups.setdefault(len(t.data), []).append(t)
    return groups
