"""LZ4 blocks built sequence by sequence, each with the bytes it must decode to - the matrix of tests/test_sim_lz4_sequences.py
and tests/test_gpu_lz4_sequences.py.  A case chooses literal lengths, offsets and match lengths so that ONE edge of the frame
decoder (qatzip_amd/csrc/qzk_lz4.h: qzk_l4_stage / qzk_l4_window / qzk_l4_slow / qzk_lz4_dblock) or of the copy engine
(qzk_lz_batch.h) is met, and carries the edge in its name.  The model output is made here, by a byte-by-byte LZ77 copy; what
liblz4 1.9.3 answers to every frame is recorded in tests/golden/lz4_sequences/index.json (tests/golden/gen_lz4_sequences.py,
which also holds the model against liblz4's bytes).

Every case comes in two wrappings: "wave" - its block alone in a small frame, the one-wave kernel's work - and "blocks" - the
same block behind a stored block of BIG random bytes in a frame of independent blocks, which is a candidate of the
wave-per-block route.  Cases with history across blocks stand in a linked frame and have the wave wrapping only.

class   strict          the block obeys the format's end rules, or is malformed: the decoder agrees with liblz4
        lenient_end     end-rule violations liblz4 refuses and this decoder accepts: status 0 and the model's bytes
        strict_offset0  offset 0: liblz4 1.9.3 copies from undefined memory, this decoder refuses
"""
import hashlib
import random
import struct

import datagen
import lz4_frame_writer as W

# ---------------------------------------------------------------- the decoder's constants the edges are derived from
RING = 1024             # QZK_L4_RING: bytes of the stream the LDS ring holds
HALF = 512              # the ring's refill
QUEUE = 128             # QZK_L4_Q
WAVE = 64               # lanes: a window's starts, a batch's sequences
RB_LIM = 3072           # QZK_RB_LIM: output bytes of one batch
RB_LITMAX = 992         # QZK_RB_LITMAX: literal-span bytes of one batch
RB_COOP = 32            # QZK_RB_COOP: window copies from here on are the whole wave's
RB_LITCOOP = 64         # QZK_RB_LITCOOP
CAND = 65571            # QZK_LZ4_CAND: frames above it are candidates of the block route
BIG = 66000             # the stored block in front of a blocks-route case
PHASE = 5               # the output's 16-byte phase the matrix is laid out for (the tests' decode() default)
END = 12                # closing literals of a block that obeys every end rule wherever its last match stands
MAXFRAME = 140000

STRICT, LENIENT, OFFSET0 = "strict", "lenient_end", "strict_offset0"
CLASSES = (STRICT, LENIENT, OFFSET0)


def stream(n, seed):
    """n bytes no two stretches of which are alike: SHA-256 in counter mode"""
    out = bytearray()
    k = 0
    while len(out) < n:
        out += hashlib.sha256(b"lz4seq %d %d" % (seed, k)).digest()
        k += 1
    return bytes(out[:n])


def big_block(block_id=5):
    """the stored block in front of a blocks-route case (no more than the frame's BD maximum)"""
    return datagen.gen_bytes("rand", BIG, 3)[:W.BLOCK_MAX[block_id]]


class Block:
    """one block in the making: .body its bytes, .out what it decodes to (history included in .hist bytes in front)"""

    def __init__(self, seed, history=b""):
        self.body = bytearray()
        self.out = bytearray(history)
        self.hist = len(history)
        self.records = []                                           # (literal offset in the stream, literals, match length, offset)
        self._lits = stream(1 << 17, seed)
        self._at = 0
        self.valid = True                                           # the model could follow every offset

    def _take(self, n):
        assert self._at + n <= len(self._lits)
        self._at += n
        return self._lits[self._at - n:self._at]

    @property
    def pos(self):
        return len(self.body)

    @property
    def produced(self):
        return len(self.out) - self.hist

    @staticmethod
    def _ext(r):
        out = bytearray()
        while r >= 255:
            out.append(255); r -= 255
        out.append(r)
        return out

    def seq(self, lit, off, ml):
        """lit literals, then ml >= 4 bytes from off back"""
        m = ml - 4
        self.body.append((min(lit, 15) << 4) | min(m, 15))
        if lit >= 15:
            self.body += self._ext(lit - 15)
        lo = self.pos
        ls = self._take(lit)
        self.body += ls
        self.out += ls
        self.body += struct.pack("<H", off)
        if m >= 15:
            self.body += self._ext(m - 15)
        self.records.append((lo, lit, ml, off))
        if off == 0 or off > len(self.out):
            self.valid = False
            return self
        for _ in range(ml):                                         # the reference: one byte at a time
            self.out.append(self.out[-off])
        return self

    def end(self, lit=END):
        self.body.append(min(lit, 15) << 4)
        if lit >= 15:
            self.body += self._ext(lit - 15)
        lo = self.pos
        ls = self._take(lit)
        self.body += ls
        self.out += ls
        self.records.append((lo, lit, 0, 1))
        return self

    @staticmethod
    def lit_for_size(size, ml_ext=0):
        """the literal count of a sequence that takes `size` stream bytes (token, extensions, literals, offset, ml_ext bytes)"""
        for lit in range(max(size - 3 - ml_ext - 1 - size // 255 - 1, 0), size):
            if 1 + (len(Block._ext(lit - 15)) if lit >= 15 else 0) + lit + 2 + ml_ext == size:
                return lit
        return None

    def pad_to(self, target):
        """plain sequences until the next token stands at stream offset `target`"""
        while self.pos != target:
            gap = target - self.pos
            assert gap >= 3, (self.pos, target)
            size = 200 if gap > 300 else gap
            if self.lit_for_size(size) is None or (size != gap and gap - size < 3):
                size = 9
            lit = self.lit_for_size(size)
            self.seq(lit, min(len(self.out) + lit, 1 + lit % 9), 4 + lit % 5)
        return self

    def model(self):
        return bytes(self.out[self.hist:]) if self.valid else None


def batches(records, phase=PHASE):
    """the batches qzk_lz4_dblock makes of a block of fewer than 64 records (every record is queued before the first batch):
    [(first record, count, obase, wstart)]; count 0: the record goes the direct way"""
    assert len(records) < WAVE
    out, i, obase, hd = [], 0, 0, phase
    while i < len(records):
        sh = (phase + obase) & 15
        tot, fit, span0 = 0, 0, records[i][0]
        for lo, lit, ml, _ in records[i:]:
            if tot + lit + ml > RB_LIM or lo + lit - span0 > RB_LITMAX:
                break
            tot += lit + ml; fit += 1
        if fit == 0:
            out.append((i, 0, obase, obase))
            obase += records[i][1] + records[i][2]
            hd = (phase + obase) & 15
            i += 1
            continue
        out.append((i, fit, obase, obase - sh + hd))
        if (sh + tot) >> 4:
            hd = 0
        obase += tot
        i += fit
    return out


def nmem_of(records, k, phase=PHASE):
    """bytes record k's match takes from before the window of its batch (qzk_rb_batch's nmem); None on the direct way"""
    for first, cnt, obase, wstart in batches(records, phase):
        if first <= k < first + max(cnt, 1):
            if cnt == 0:
                return None
            my_m = obase + sum(r[1] + r[2] for r in records[first:k]) + records[k][1]
            gap = my_m - wstart
            _, _, ml, off = records[k]
            return min(ml, off - gap) if off > gap else 0
    raise AssertionError(k)


class Case:
    def __init__(self, name, cls, body, model, cap_delta=0, pre=(), independent=True, block_id=5, stored=False, path=None, room=8192):
        self.name, self.cls, self.body, self.model = name, cls, bytes(body), model
        self.cap_delta = cap_delta                                  # the capacity offered, relative to what the frame decodes to
        self.pre = list(pre)                                        # blocks in front: (body, stored, what it decodes to)
        self.independent, self.block_id, self.stored, self.path = independent, block_id, stored, path
        self.room = room                                            # the capacity offered to a block the model cannot follow

    def _content(self, head):
        if self.model is None:
            return None
        return head + b"".join(p[2] for p in self.pre) + self.model

    def wrappings(self):
        return ("wave", "blocks") if self.independent else ("wave",)

    def frame(self, wrapping):
        blocks = [(p[0], p[1]) for p in self.pre] + [(self.body, self.stored)]
        if wrapping == "blocks":
            assert self.independent
            blocks.insert(0, (big_block(self.block_id), True))
        fr = W.frame(blocks, block_id=self.block_id, independent=self.independent)
        assert len(fr) <= MAXFRAME, (self.name, len(fr))
        if wrapping == "wave" and self.independent and not self.pre:
            assert len(fr) <= CAND, (self.name, len(fr))
        if wrapping == "blocks":
            assert len(fr) > CAND
        return fr

    def content(self, wrapping):
        """what the frame decodes to, or None where the model cannot follow it"""
        return self._content(big_block(self.block_id) if wrapping == "blocks" else b"")

    def cap(self, wrapping):
        c = self.content(wrapping)
        if c is None:                                               # room for whatever a decoder makes of it
            return (len(big_block(self.block_id)) if wrapping == "blocks" else 0) + sum(len(p[2]) for p in self.pre) + self.room
        return len(c) + self.cap_delta


def cases():
    """the matrix: a list of Case, names unique"""
    out = []
    seed = [1000]

    def nb(first_lit=24):
        """a new block; first_lit: a first sequence, so that there is something to match from"""
        seed[0] += 1
        b = Block(seed[0])
        if first_lit:
            b.seq(first_lit, 7, 6)
        return b

    def add(name, b, cls=STRICT, **kw):
        out.append(Case(name, cls, b.body, b.model(), **kw))

    # ------------------------------------------------------------ token parsing (qzk_l4_window / qzk_l4_slow)
    for ln in (0, 14, 15):
        for mn in (0, 14, 15):
            add("tok_litnib%d_mlnib%d" % (ln, mn), nb().seq(ln, 9, mn + 4).end())
    for tag, v in (("ext0", 15), ("ext254", 15 + 254), ("ext255_0", 270), ("ext255_255_3", 15 + 255 + 255 + 3)):
        add("tok_lit_" + tag, nb().seq(v, 11, 8).end())
        add("tok_ml_" + tag, nb().seq(3, 11, v + 4).end())
    add("tok_both_ext_269_273", nb().seq(269, 200, 273).end())
    add("tok_both_ext_270_274", nb().seq(270, 201, 274).end())
    add("tok_both_ext_300_600", nb().seq(300, 17, 600).end())
    add("tok_both_ext_800_1000_then_short", nb().seq(800, 700, 1000).seq(1, 3, 4).end())
    for nseq in (WAVE - 2, WAVE - 1, WAVE, WAVE + 1, QUEUE - 1, QUEUE, QUEUE + 1, 200, 450):
        b = nb(16)                                                  # 3-byte sequences: 21-22 starts in a 64-byte window
        for k in range(nseq - 2):
            b.seq(0, 1 + (5 * k) % 16, 4 + k % 3)
        add("tok_min_seqs_%d_records" % nseq, b.end())
    b = nb(16)
    for k in range(150):                                            # 3- and 4-byte sequences: every lane gets to be a start
        b.seq(k % 2, 1 + (7 * k) % 13, 4 + k % 11)
    add("tok_min_seqs_mixed_152_records", b.end())
    for at in (60, 61, 62, 63, 64, 65, 127, 128):                   # a sequence with both extensions that begins on lane `at` % 64
        b = nb(0).seq(at - 4, 5, 4)
        assert b.pos == at
        add("tok_start_at_%d" % at, b.seq(40, 33, 50).seq(2, 1, 4).end())

    # ------------------------------------------------------------ ring staging (qzk_l4_stage)
    # the probe: token t, literal extension t+1, 20 literals, offset t+22 / t+23, match extension t+24
    for edge in (HALF, RING, RING + HALF):
        for what, d in (("tok_ext", 1), ("tok", 0), ("lits", 2), ("off_lo_hi", 23), ("off", 22), ("off_mlext", 24), ("mlext", 25)):
            b = nb().pad_to(edge - d)
            add("ring_%d_%s" % (edge, what), b.seq(20, 19, 26).seq(1, 2, 5).end())
    for edge in (HALF, RING, RING + HALF, 2 * RING):                # minimum sequences across the edge, every phase of 3
        for d in (0, 1, 2):
            b = nb().pad_to(edge - 30 - d)
            for k in range(20):
                b.seq(0, 1 + k % 7, 4)
            add("ring_%d_min_seqs_phase%d" % (edge, d), b.end())
    # a literal run from lane 0 of the first window that ends around `filled` (1024 there), and around the first refill
    for q in (HALF - 3, HALF, RING - 4, RING - 3, RING - 2, RING - 1, RING, RING + 1, RING + 2):
        b = nb(0)
        lit = Block.lit_for_size(q + 2)                             # the run ends at q, the offset behind it
        b.seq(lit, 100, 9)
        assert b.records[0][0] + lit == q
        add("ring_litrun_ends_%d" % q, b.seq(2, 5, 4).end())
    for lit in (HALF + 1, RING, RING + 1, RING + HALF, RING + HALF + 1, 2 * RING + 7, 3000):
        add("ring_lit_%d" % lit, nb().seq(lit, 50, 8).end())
        add("ring_lit_%d_then_short" % lit, nb().seq(lit, 50, 8).seq(0, 1, 4).seq(1, 2, 4).end())
    for at in (RING + HALF - 1, RING + HALF, RING + HALF + 1, 2 * RING, 2 * RING + HALF - 1, 2 * RING + HALF):
        b = nb(0)                                                   # the sequence behind a long run begins exactly at `at`
        b.seq(Block.lit_for_size(at), 77, 4)
        assert b.pos == at
        add("ring_restage_next_at_%d" % at, b.seq(17, 9, 21).seq(0, 1, 4).end())

    # ------------------------------------------------------------ batch fitting (qzk_lz4_dblock)
    for total in (RB_LIM - 1, RB_LIM, RB_LIM + 1):
        b = nb(0)
        for k in range(WAVE):
            b.seq(8, 3 + k % 6, 40 + (k == 5) * (total - RB_LIM))
        assert b.produced == total
        add("fit_64_seqs_%d_bytes" % total, b.end())
    for span in (RB_LITMAX - 1, RB_LITMAX, RB_LITMAX + 1):
        b = nb(0)
        longer = span - (63 * 15 + 12)
        for k in range(WAVE):
            b.seq(13 if k >= WAVE - longer else 12, 2 + k % 9, 4 + k % 5)
        assert b.records[63][0] + b.records[63][1] - b.records[0][0] == span
        add("fit_64_seqs_span_%d" % span, b.end())
    add("fit_one_lit_%d_batch" % RB_LITMAX, nb().seq(RB_LITMAX, 40, 10).end())
    for lit in [RB_LITMAX + 1] + list(range(1000, 1008)) + [4000]:
        add("direct_lit_%d" % lit, nb().seq(lit, 40, 10).seq(3, 2, 4).end())
    add("direct_lit_1003_first", nb(0).seq(1003, 1003, 5).end())
    for ml in (RB_LIM - 1, RB_LIM, RB_LIM + 1, 5000):
        add("direct_match_%d" % ml, nb().seq(0, 13, ml).seq(3, 2, 4).end())
    add("fit_lit_plus_match_%d" % RB_LIM, nb().seq(72, 13, RB_LIM - 72).end())
    add("direct_lit_plus_match_%d" % (RB_LIM + 1), nb().seq(72, 13, RB_LIM + 1 - 72).end())
    for d in (1, 2, 3, 5, 7, 8, 63, 64, 65, 200):
        add("direct_match_dist%d" % d, nb(0).seq(220, 9, 4).seq(5, d, 3300 + d).seq(1, 1, 4).end())
    add("direct_match_dist_all_produced", nb(0).seq(100, 100, 3500).end())
    add("direct_match_dist_all_produced_behind_batch", nb().seq(50, 24 + 6 + 50, 3400).end())
    add("direct_match_dist_above_produced", nb(0).seq(100, 101, 3500).end())
    add("direct_match_dist_above_produced_behind_batch", nb().seq(50, 24 + 6 + 50 + 1, 3400).end())
    add("direct_match_offset0", nb().seq(5, 0, 3500).end(), OFFSET0)
    add("direct_lit_offset0", nb().seq(1200, 0, 8).end(), OFFSET0)

    # ------------------------------------------------------------ the match copy (qzk_rb_batch)
    # a first sequence of 3060 bytes fills a batch; the probe stands in the second, 10 literals behind the window's start
    def full_batch():
        """one sequence of RB_LIM - 12 bytes: whatever follows stands in the second batch"""
        return nb(0).seq(900, 300, RB_LIM - 12 - 900)

    def second_batch(nmem, ml):
        b = full_batch()
        obase = b.produced
        gap = ((PHASE + obase) & 15) + 10
        b.seq(10, gap + nmem, ml).end()
        assert nmem_of(b.records, 1) == nmem, (nmem, ml, nmem_of(b.records, 1))
        return b
    for nmem in (1, 2, 3, 4, 7, 8, 16, 17, 24, 25, 32, 33, 40, 41, 64, 65, 520):
        if nmem >= 4:
            add("mem_%d_whole_match" % nmem, second_batch(nmem, nmem))
        add("mem_%d_then_window" % nmem, second_batch(nmem, nmem + 9))
    add("mem_8_then_window_300", second_batch(8, 308))
    add("mem_33_then_window_31", second_batch(33, 64))
    b = full_batch()                                   # every lane of the second batch its own part from memory
    for k in range(40):
        b.seq(2, 40 + 11 * k, 4 + k)
    add("mem_40_lanes", b.end())
    add("mem_all_produced", full_batch().seq(10, RB_LIM - 12 + 10, 8).end())
    for d in (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 63, 64, 65):
        b = nb(0)
        for ln in (4, 7, 8, 9, 31, RB_COOP, RB_COOP + 1, 300):
            b.seq(d + 2, d, ln)
        add("win_dist%d_len_4_7_8_9_31_32_33_300" % d, b.end())
        b = full_batch()                               # the same behind a full batch: the window begins inside a row
        for ln in (4, 9, 31, RB_COOP + 1):
            b.seq(d + 2, d, ln)
        add("win2_dist%d_len_4_9_31_33" % d, b.end())
    for depth in (2, 8, 63):
        b = nb(0).seq(9, 4, 6)
        for k in range(depth - 1):                                  # the source: the tail of the match before and this literal
            b.seq(1, 2 + k % 4, 4 + k % 9)
        add("chain_depth%d" % depth, b.end())
        b = nb(0).seq(9, 4, 40)
        for k in range(depth - 1):                                  # long and short copies in turn, each from the one before
            ml = (40, 5, 33, 12)[k % 4]
            b.seq(1, ml + 1 if k % 3 == 0 else 3 + k % 5, ml)
        add("chain_depth%d_coop_and_lane" % depth, b.end())
    # the match before stands at [m, m + first); 20 literals; then `second` bytes whose source ends one byte into it / begins
    # at its last byte
    for first, second in ((40, 6), (6, 40), (6, 6), (40, 40), (6, 31), (33, 31)):
        b = nb(64).seq(2, 5, first)
        add("chain_src_ends_1_into_%d_read_by_%d" % (first, second), b.seq(20, first + 20 + second - 1, second).end())
        b = nb(64).seq(2, 5, first)
        add("chain_src_begins_at_last_of_%d_read_by_%d" % (first, second), b.seq(20, 21, second).end())
    for tag, mk in (("lane", lambda: nb().seq(5, 19, 20)), ("coop", lambda: nb().seq(5, 99, 100)),
                    ("direct", lambda: nb().seq(3999, 3999, 4000)), ("mem", lambda: full_batch().seq(10, 49, 50))):
        add("overlap_own_dest_by_1_" + tag, mk().end())

    # ------------------------------------------------------------ output placement: capacity
    def paths():
        return (("batch", nb().seq(30, 11, 70).seq(3, 40, 9).end(), False),
                ("direct_lit", nb().seq(1300, 11, 7).end(), False),
                ("direct_match", nb().seq(4, 9, 3600).end(), False),
                ("stored", None, True))
    for tag, b, stored in paths():
        for d in (0, 1, -1, -17):
            name = "cap_%s_%s" % (tag, "exact" if d == 0 else "plus%d" % d if d > 0 else "minus%d" % -d)
            if stored:
                data = stream(1000, 77)
                out.append(Case(name, STRICT, data, data, cap_delta=d, stored=True, path=tag if d == 0 else None))
            else:
                out.append(Case(name, STRICT, b.body, b.model(), cap_delta=d, path=tag if d == 0 else None))

    # ------------------------------------------------------------ history: linked frames, and the same blocks independent
    first64 = stream(BIG, 501)
    first1k = stream(1000, 502)
    for tag, first, lit, reach in (("1", first1k, 10, 1), ("33", first1k, 10, 33), ("65535", first64, 0, 65535),
                                   ("all_produced", first1k, 10, 1000), ("65535_lit", first64, 35, 65535 - 35)):
        for indep in (False, True):
            seed[0] += 1
            b = Block(seed[0], first if not indep else b"")
            b.seq(lit, lit + reach, 20).seq(2, 9, 5).end()
            add("hist_%s_reach_%s" % ("independent" if indep else "linked", tag), b, pre=[(first, True, first)], independent=indep)
    seed[0] += 1
    b = Block(seed[0], first1k).seq(10, 1011, 20).end()
    add("hist_linked_reach_above_produced", b, pre=[(first1k, True, first1k)], independent=False)
    seed[0] += 1
    b = Block(seed[0], first1k).seq(900, 700, 2100).seq(10, 3000 + 10 + 500, 600).seq(1200, 1200 + 3610 + 999, 3100).end()
    add("hist_linked_batch_mem_and_direct_match_into_first", b, pre=[(first1k, True, first1k)], independent=False)
    pre_c = nb().seq(40, 7, 80).end()
    seed[0] += 1
    b = Block(seed[0], pre_c.model()).seq(0, 30, 40).seq(3, 160, 12).end()
    add("hist_linked_compressed_first_lit0", b, pre=[(bytes(pre_c.body), False, pre_c.model())], independent=False)

    # ------------------------------------------------------------ malformed
    add("bad_offset_above_produced_by_1", nb(0).seq(20, 21, 8).end())
    add("bad_offset_above_produced_by_1_later", nb().seq(20, 24 + 6 + 20 + 1, 8).end())
    add("bad_offset_above_produced_by_1_second_batch", full_batch().seq(10, RB_LIM - 12 + 10 + 1, 8).end())
    add("offset0", nb().seq(5, 0, 8).end(), OFFSET0)
    add("offset0_first", nb(0).seq(5, 0, 8).end(), OFFSET0)
    add("offset0_slow_reader", nb().seq(300, 0, 8).end(), OFFSET0)
    b = nb()
    base = b.pos                                                    # token, 255, 30, 300 literals, offset, 255, 255, 71, closing
    whole = b.seq(300, 100, 600).end().body
    for tag, cut in (("lit_ext", base + 2), ("literals", base + 3 + 150), ("offset", base + 3 + 300 + 1), ("ml_ext", base + 3 + 300 + 2 + 2),
                     ("behind_match", base + 3 + 300 + 2 + 3)):
        out.append(Case("bad_cut_in_" + tag, STRICT, whole[:cut], None))
    b = nb()
    base = b.pos                                                    # token, 5 literals, offset, 11, closing
    small = b.seq(5, 3, 30).end().body
    for tag, cut in (("literals", base + 1 + 2), ("offset", base + 1 + 5 + 1), ("ml_ext", base + 1 + 5 + 2), ("behind_match", base + 1 + 5 + 3)):
        out.append(Case("bad_short_cut_in_" + tag, STRICT, small[:cut], None))
    out.append(Case("bad_lit_len_beyond_block", STRICT, bytes(nb().seq(5, 3, 8).body) + b"\xf0\x40" + stream(30, 9), None))
    out.append(Case("bad_one_byte_0x10", STRICT, b"\x10", None))
    out.append(Case("bad_one_byte_0x00", LENIENT, b"\x00", b""))

    # ------------------------------------------------------------ the end rules liblz4 enforces and this decoder does not
    for n in (0, 1, 2, 3, 4):
        add("end_closing_literals_%d" % n, nb().seq(5, 3, 30).end(n), LENIENT)
    add("end_closing_literals_5", nb().seq(5, 3, 30).end(5))
    add("end_ml_ext_in_last_5", nb().seq(5, 3, 30).seq(2, 9, 19 + 40).end(3), LENIENT)
    add("end_last_match_4_closing_5", nb().seq(5, 3, 30).seq(0, 2, 4).end(5), LENIENT)
    b = nb(0).seq(500, 400, 65536 - 500 - 4)
    add("end_bd4_full_block_closing_4", b.end(4), LENIENT, block_id=4)
    b = nb(0).seq(500, 400, 65536 - 500 - 5)
    add("end_bd4_full_block_closing_5", b.end(5), block_id=4)
    b = nb(0).seq(500, 400, 65536 - 500 - 12)
    add("end_bd4_full_block_closing_12", b.end(12), block_id=4)
    b = nb(0).seq(500, 400, 65537 - 500 - 12)
    over = b.end(12).body
    # (with room for more than a whole block liblz4 decodes in place and names the failure ERROR_GENERIC; with less room than
    # the BD maximum "does not fit" is as true an answer as "bad data", and the one-wave kernel gives the first)
    out.append(Case("bad_bd4_block_decodes_to_65537_room_70000", STRICT, over, None, block_id=4, room=70000))
    add("bad_bd4_offset_above_produced_by_1_room_70000", nb(0).seq(20, 21, 8).end(), block_id=4, room=70000)

    names = [c.name for c in out]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return out


def expect(case, wrapping, rec):
    """what a decoder of this project must answer to the case, from its class and liblz4's recorded verdict `rec`:
    ("ok", the bytes) - status 0, the whole frame used, exactly these bytes; ("short",) - status -2; ("refuse",) - any error"""
    if case.cls == OFFSET0:
        return ("refuse",)
    if case.cls == LENIENT:
        return ("ok", case.content(wrapping))
    if rec["liblz4"] == "OK":
        return ("ok", case.content(wrapping))
    if case.model is not None and case.cap_delta < 0:
        assert rec["liblz4"] == "incomplete"
        return ("short",)
    return ("refuse",)


def check(case, wrapping, rec, frame, status, in_used, out_len, out, where):
    """one result against expect()"""
    want = expect(case, wrapping, rec)
    if want[0] == "ok":
        assert status == 0 and in_used == len(frame) and out_len == len(want[1]), (case.name, where, status, in_used, out_len, len(want[1]))
        if out != want[1]:
            at = next(i for i in range(len(out)) if out[i] != want[1][i])
            raise AssertionError((case.name, where, "first wrong byte at", at - (len(want[1]) - len(case.model)), "of the block's output"))
    elif want[0] == "short":
        assert status == -2, (case.name, where, status)
    else:
        assert status != 0, (case.name, where, "accepted")


def representatives():
    """one small case per path, for the sixteen output phases"""
    return [c for c in cases() if c.path]


# ---------------------------------------------------------------- random mode: blocks of the strict shape
_LITS = (0, 0, 1, 2, 3, 7, 8, 14, 15, 16, 31, 63, 64, 65, 269, 270, 271, 511, 513, 993, 1024, 1030)
_MLS = (4, 4, 5, 7, 8, 9, 18, 19, 20, 31, 32, 33, 64, 273, 274, 300, 3073)
_OFFS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 200, 1000)


def random_block(rng):
    """a valid block that obeys the end rules: triples drawn from the edge values above -> Block"""
    b = Block(rng.randrange(1 << 30))
    b.seq(rng.choice((1, 9, 24, 300)), 1, 4)
    style = rng.randrange(4)
    for _ in range(rng.choice((1, 3, 20, 70, 140))):
        if b.produced > 50000 or b.pos > 40000:
            break
        lit = rng.choice(_LITS) if style != 1 else rng.choice((0, 0, 1, 2))
        ml = rng.choice(_MLS) if style != 1 else rng.choice((4, 4, 5, 9))
        off = rng.choice(_OFFS) if rng.randrange(4) else rng.randrange(1, b.produced + lit + 1)
        b.seq(lit, min(off, b.produced + lit), ml)
    return b.end(rng.choice((5, 12, 13, 40)) if b.records[-1][2] >= 12 else END)


def random_cases(n, seed):
    rng = random.Random(seed)
    out = []
    for i in range(n):
        b = random_block(rng)
        out.append(Case("random_%d" % i, STRICT, b.body, b.model()))
    return out
