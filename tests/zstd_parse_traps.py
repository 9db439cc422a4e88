"""Trap inputs for Kzp, the hash-chain lazy parse of zstd sessions (qatzip_amd/csrc/qzk_zstd_parse.h): inputs built so that
ONE rule of that header's comment decides the records, each with a check that reads the decision out of the answer of
model() and of its trace.  No library has this parse, so the authority is model(): P1, P2 and P3 restated serially from the
header's comment and, for the history, from RFC 8878 3.1.1.5.  It imports nothing from the emulator and calls no kernel; the
strict reader (tests/zstd_full_format.py) and libzstd, which resolve the repeat codes of the frames on their own, cross-check
its records from outside (tests/test_sim_zstd_parse_traps.py).  tests/lz4hc_traps.py is the model for this file; its filler
and Buf are used here, not copied.

A trap is (name, family, data, hw_buff_sz, mini_match, depth, aim, check):
  aim    one line: the decision the trap aims at
  check  check(seqs, trace): seqs = [(literal length, match length, offset)] and the Trace of model(data, hw_buff_sz,
         mini_match, depth).  A trap whose check fails on the model tests nothing.

model(chunk, hw_buff_sz, mini_match, depth, mingain=10, lazy2=64, hshift=2) -> (chain, res, seqs, literals, trace): the
chain distances of P1, the {length, distance} of P2, the records and literals of P3, and per decision label (LABELS) how
often it fired and, for the rarer ones, at which positions.  The three constants follow a build with other -D values.
P2 is walked in the wave's order (64 positions a trip, one candidate per lane a round, the capped ones in lane order) only
so that the trace can see the run table, which changes no answer.  tests/golden/gen_zstd_parse_traps.py holds chain, results,
records and literals equal to the emulator's on every trap; after that the trace may be trusted.

Families: A chains (P1), B the walk and its depth (P2), C lengths and the run table (P2), D the lazy evaluation (P3), E the
ends, F geometry.  A, B, C, E, F and part of D are planted by hand on random filler.  The corners of P3's state machine come
from a seeded search over small-alphabet inputs with overlapping copies (sm_input()): per label the smallest input whose
trace holds it, kept as its seed (SM_SEEDS, printed by gen_zstd_parse_traps.py --search).

Labels and their traps, as trap_table() prints them: label, then the traps whose check asks for it.  Every label is asked
for by the check of at least one trap or stands in UNREACHABLE with its argument (below, at UNREACHABLE), and the seeded
search must not have found it; tests/test_sim_zstd_parse_traps.py holds this list to trap_table() and enforces the rule.
  p1.head            a_trip_same_word_2_times, a_trip_same_word_3_times, a_period_63, a_period_64, a_period_65, f_chunk_of_2048, f_chunk_of_4096, f_chunk_of_8192, f_chunk_of_16384, f_chunk_of_32768, f_chunk_of_65536
  p1.lane            a_trip_same_word_2_times, a_trip_same_word_3_times, a_period_1, a_period_2, a_period_3
  p1.collision       a_collision_mm3_narrower, a_collision_mm3_as_is, a_collision_mm4_narrower
  p1.tail            e_last_match_leaves_0_mm3, e_chunk_of_3_mm3, e_last_match_leaves_0_mm4, e_chunk_of_4_mm4
  p1.mm3_fourth      a_three_bytes_then_another_mm3
  p1.width.1024      c_equal_lengths_nearer_stays
  p1.width.2048      f_chunk_of_2048
  p1.width.4096      f_chunk_of_4096
  p1.width.8192      f_chunk_of_8192
  p1.width.16384     f_chunk_of_16384
  p1.width.32768     f_chunk_of_32768
  p1.width.65536     f_chunk_of_65536
  p1.width.131072    f_offsets_65535_and_65536
  p2.end_depth       b_whole_copy_is_candidate_2_depth_1, b_whole_copy_is_candidate_3_depth_2, b_whole_copy_is_candidate_5_depth_4, b_whole_copy_is_candidate_17_depth_16, b_whole_copy_is_candidate_64_depth_63, b_whole_copy_is_candidate_65_depth_64, b_whole_copy_is_candidate_257_depth_256
  p2.end_chain       d_backwards_to_p_equals_off
  p2.end_reach       c_match_reaches_the_end, f_one_match_from_1_to_the_end, f_the_largest_offset_taken
  p2.mm_fail         a_collision_mm4_narrower
  p2.longer          c_farther_one_byte_longer
  p2.equal           b_whole_copy_is_candidate_4_depth_4, b_whole_copy_is_candidate_16_depth_16, b_whole_copy_is_candidate_63_depth_63, b_whole_copy_is_candidate_64_depth_64, b_whole_copy_is_candidate_256_depth_256, c_equal_lengths_nearer_stays
  p2.shorter         c_farther_one_byte_shorter
  p2.len31           c_length_31
  p2.len32           c_length_32
  p2.len33           c_length_33
  p2.cap_guard       c_capped_candidate_cannot_pass
  p2.run_miss        c_run_table_slot_of_two_distances
  p2.run_hit         a_period_1, a_period_2, a_period_3, a_period_63, a_period_64, a_period_65, c_run_table_slot_of_two_distances
  p2.run_replace     c_run_table_slot_of_two_distances
  p2.run_again       c_run_table_slot_of_two_distances
  p2.run_before      c_run_table_entry_of_a_later_lane
  p2.run_past        c_run_table_slot_of_two_distances
  p2.run_at_end      UNREACHABLE
  stored.refused_9   d_gain_9_mm3, d_gain_9_mm4, d_searched_256_0_mm3_depth4
  stored.taken_10    a_collision_mm3_narrower, a_collision_mm3_as_is, a_collision_mm4_as_is, a_three_bytes_then_another_mm3, d_gain_10_mm3, d_gain_10_mm4, d_searched_256_0_mm3_depth4
  stored.rep1.ll1    d_repeat_behind_a_changed_byte, d_searched_256_0_mm3_depth4
  stored.rep2.ll1    d_searched_256_0_mm3_depth64
  stored.rep3.ll1    d_searched_256_1_mm3_depth4
  stored.rep1.ll0    d_searched_256_2_mm3_depth4
  stored.rep2.ll0    d_searched_256_2_mm3_depth4
  stored.rep3.ll0    d_stored_match_is_rep1_less_1, d_searched_256_1_mm3_depth4
  rep.skip_zero      d_rep1_is_1, d_searched_256_0_mm3_depth4
  rep.skip_beyond    d_searched_256_0_mm3_depth4
  rep.skip_same      d_repeat_behind_a_changed_byte, d_searched_256_0_mm3_depth4, f_one_match_from_1_to_the_end
  rep.only           d_searched_256_3_mm3_depth64
  rep.beats          d_rep1_less_1_beats_a_longer_match, d_repeat_is_priced_as_one, d_searched_256_2_mm3_depth4
  rep.loses          d_searched_256_2_mm3_depth4
  rep.tie_lower      d_tie_goes_to_the_lower_offset_value, d_searched_256_10_mm3_depth4
  rep.tie_stays      d_searched_256_16_mm3_depth64
  la1.stay_4         d_ahead_1_gains_4, d_searched_256_2_mm3_depth4
  la1.move_5         d_ahead_1_gains_5, d_searched_256_11_mm3_depth4
  la2.stay_7         d_ahead_2_gains_7, d_searched_256_10_mm3_depth64
  la2.move_8         d_ahead_2_gains_8, d_searched_256_5_mm3_depth64
  la2.untried        d_ahead_2_at_depth_63, d_searched_256_0_mm3_depth4
  la2.tried          d_ahead_2_at_depth_64, d_searched_256_0_mm3_depth64
  la.restart2        d_look_ahead_restarts_three_times, d_searched_256_2_mm3_depth64
  la.restart3        d_look_ahead_restarts_three_times, d_searched_256_245_mm4_depth16
  la.cut_by_end      d_searched_256_0_mm4_depth64, e_match_in_the_last_3_bytes, e_match_in_the_last_4_bytes
  back.anchor        d_backwards_to_the_anchor, d_searched_256_2_mm3_depth4
  back.mismatch      d_look_ahead_restarts_three_times, d_searched_256_0_mm3_depth4
  back.at_off        d_backwards_to_p_equals_off, d_searched_256_0_mm3_depth4
  back.none_rep      d_repeat_behind_a_changed_byte, d_searched_256_0_mm3_depth4
  back.rep_front     UNREACHABLE
  back.ov_changed    UNREACHABLE
  push.keep.ll1      d_repeat_behind_a_changed_byte, d_searched_256_0_mm3_depth4
  push.swap.ll1      d_searched_256_2_mm3_depth4
  push.swap.ll0      d_searched_256_2_mm3_depth4
  push.rot.ll1       d_searched_256_0_mm3_depth4
  push.rot.ll0       d_rep1_less_1_beats_a_longer_match, d_stored_match_is_rep1_less_1, d_searched_256_0_mm3_depth4
  end.match_at_end   c_match_reaches_the_end, d_searched_256_0_mm3_depth4, e_last_match_leaves_0_mm3, e_match_in_the_last_3_bytes, e_last_match_leaves_0_mm4, e_match_in_the_last_4_bytes, f_one_match_from_1_to_the_end, f_the_largest_offset_taken
  end.tail           d_searched_256_3_mm4_depth16, e_last_match_leaves_1_mm3, e_last_match_leaves_2_mm3, e_last_match_leaves_1_mm4, e_last_match_leaves_2_mm4, e_last_match_leaves_3_mm4
  end.short_chunk    e_chunk_of_1_mm3, e_chunk_of_2_mm3, e_chunk_of_1_mm4, e_chunk_of_2_mm4, e_chunk_of_3_mm4
"""
import collections

import numpy as np

from lz4_traps import Buf, rnd

FAMILIES = ("A", "B", "C", "D", "E", "F")
LANECAP, RUNBITS = 32, 8
HWS = (1024, 2048, 4096, 8192, 16384, 32768, 65536, 131072)
DEPTHS = (1, 2, 4, 16, 63, 64, 256)

# label -> the decision (the lines are qzk_zstd_parse.h's)
LABELS = collections.OrderedDict((
    # P1
    ("p1.head", "the predecessor comes from the head table (an earlier trip of 64 positions)"),
    ("p1.lane", "the predecessor is a lane of the same trip: the nearest earlier lane with the hash"),
    ("p1.collision", "the predecessor has the hash and other bytes"),
    ("p1.tail", "a position in the last mini_match - 1 bytes: no hash, chain 0"),
    ("p1.mm3_fourth", "mini_match 3: the predecessor agrees in three bytes and differs in the fourth"),
    ("p1.width.1024", "hw_buff_sz 1024: a head table of 1024 >> QZK_ZP_HSHIFT entries"),
    ("p1.width.2048", "hw_buff_sz 2048"), ("p1.width.4096", "hw_buff_sz 4096"), ("p1.width.8192", "hw_buff_sz 8192"),
    ("p1.width.16384", "hw_buff_sz 16384"), ("p1.width.32768", "hw_buff_sz 32768"), ("p1.width.65536", "hw_buff_sz 65536"),
    ("p1.width.131072", "hw_buff_sz 131072"),
    # P2
    ("p2.end_depth", "the walk ended at `hops >= depth` with the chain going on"),
    ("p2.end_chain", "the walk ended at the chain's end (nd == 0)"),
    ("p2.end_reach", "the walk ended because the match reaches the chunk's end (best == maxlen)"),
    ("p2.mm_fail", "a candidate failed the mini_match-byte compare: it cost a hop"),
    ("p2.longer", "a candidate beat `best`"),
    ("p2.equal", "a candidate equalled `best`: the nearer one stays"),
    ("p2.shorter", "a candidate stayed below `best`"),
    ("p2.len31", "a candidate of exactly 31 bytes: below the lane's cap"),
    ("p2.len32", "a candidate of exactly 32 bytes: at the cap, finished by the wave with a count of 0"),
    ("p2.len33", "a candidate of exactly 33 bytes"),
    ("p2.cap_guard", "a capped candidate that cannot pass `best` (the byte behind best differs): not counted by the wave"),
    ("p2.run_miss", "the run table has another distance or nothing in the slot: counted and stored"),
    ("p2.run_hit", "the run table holds {d, p0, e} with p0 <= p < e: the length is e - p"),
    ("p2.run_replace", "an entry of another distance is replaced"),
    ("p2.run_again", "a distance whose entry was replaced is asked for again: counted again"),
    ("p2.run_before", "the slot holds the distance with p0 > p (a later lane stored it a round earlier): counted"),
    ("p2.run_past", "the slot holds the distance with e < p: counted"),
    ("p2.run_at_end", "the slot holds the distance with e == p"),
    # P3
    ("stored.refused_9", "the stored match has a gain of QZK_ZP_MINGAIN - 1: no candidate"),
    ("stored.taken_10", "the stored match has a gain of exactly QZK_ZP_MINGAIN: a candidate"),
    ("stored.rep1.ll1", "the stored match's distance is rep1 with literals in front (offset value 1)"),
    ("stored.rep2.ll1", "... rep2 with literals (2)"), ("stored.rep3.ll1", "... rep3 with literals (3)"),
    ("stored.rep1.ll0", "... rep2 without literals (offset value 1)"), ("stored.rep2.ll0", "... rep3 without literals (2)"),
    ("stored.rep3.ll0", "... rep1 - 1 without literals (3)"),
    ("rep.skip_zero", "rep1 - 1 with rep1 == 1: offset 0, skipped"),
    ("rep.skip_beyond", "a repeat offset beyond p: skipped"),
    ("rep.skip_same", "a repeat offset equal to the candidate held: skipped"),
    ("rep.only", "a repeat candidate with no other candidate"),
    ("rep.beats", "a repeat candidate with a higher gain than the one held"),
    ("rep.loses", "a repeat candidate with a lower gain"),
    ("rep.tie_lower", "equal gains, the repeat has the lower offset value: it wins"),
    ("rep.tie_stays", "equal gains, the one held has the lower offset value: it stays"),
    ("la1.stay_4", "the candidate at p + 1 gains exactly 4 more: not moved"),
    ("la1.move_5", "the candidate at p + 1 gains exactly 5 more: moved"),
    ("la2.stay_7", "the candidate at p + 2 gains exactly 7 more: not moved"),
    ("la2.move_8", "the candidate at p + 2 gains exactly 8 more: moved"),
    ("la2.untried", "depth below QZK_ZP_LAZY2: p + 2 is not looked at"),
    ("la2.tried", "depth from QZK_ZP_LAZY2 on: p + 2 is looked at"),
    ("la.restart2", "the look-ahead moved twice in a row"),
    ("la.restart3", "the look-ahead moved three times in a row"),
    ("la.cut_by_end", "p + a + mini_match > n: the look-ahead stops at the chunk's end"),
    ("back.anchor", "the backward extension reached the anchor: ll == 0"),
    ("back.mismatch", "the backward extension stopped at a differing byte"),
    ("back.at_off", "the backward extension stopped at p == off"),
    ("back.none_rep", "a repeat with literals in front: no backward extension"),
    ("back.rep_front", "a repeat whose byte in front also matches"),
    ("back.ov_changed", "the extension used up the literals and the offset value changed"),
    ("push.keep.ll1", "offset value 1 with literals: the history stays"),
    ("push.swap.ll1", "offset value 2 with literals: rep1 and rep2 swap"),
    ("push.swap.ll0", "offset value 1 without literals: rep1 and rep2 swap"),
    ("push.rot.ll1", "offset value 3 or above with literals: the history moves down"),
    ("push.rot.ll0", "offset value 2 or above without literals: the history moves down"),
    ("end.match_at_end", "the last match ends at the chunk's end"),
    ("end.tail", "the last match leaves 1 .. mini_match - 1 bytes: literals, never searched"),
    ("end.short_chunk", "a chunk shorter than mini_match: literals only"),
))

# Labels no input fires, each with its argument from the header's rules.  The search of gen_zstd_parse_traps.py --search
# (20000 inputs of sm_input() per size, each under the four (mini_match, depth) of SM_MODES) never reached one of them.
#
# p2.run_at_end.  An entry {d, p0, e} says that the bytes at distance d agree from p0 to e and, unless e is the chunk's end,
# differ at e.  A candidate at distance d from position e reaches the run table only after its first mini_match bytes
# compared equal, which in[e] != in[e - d] forbids; e == n is no position.  So `pj < run_e` is only ever false with e < pj.
#
# back.rep_front.  Let the chosen repeat have offset o at p, literals in front, and in[p - 1] == in[p - 1 - o].  Forward
# lengths are maximal, so o matches ml + 1 bytes from p - 1.  If p - 1 > anchor the three repeat offsets at p - 1 are those
# of p (the history moves only at a record), so o was a candidate there with 4 more gain: the parse point p - 1 held a
# candidate of at least that gain, a move to p needs MORE than 4 above it (first margin), and a move from p - 2 to p needs
# more than 7 above a candidate that the look-ahead by 1 had already left for p - 1 (its gain there is 11 above).  If
# p - 1 == anchor, then o == rep1 is ruled out because rep1 is the offset of the record that ended at the anchor, whose
# match is maximal: in[anchor] != in[anchor - rep1]; and rep2 / rep3 are candidates at the anchor too (offset values 1 / 2
# with no literals, one lower than at p), again with at least 4 more gain.  (It follows that the kernel's `c.ov > 3` in front
# of the backward extension saves the compare and decides nothing: a build that extends repeats too gives the same records
# on every trap.)
#
# back.ov_changed.  A match that is no repeat at p (literals in front: o is none of rep1 .. rep3) gets another offset value
# with no literals only if o == rep1 - 1, and only if the extension reached the anchor: o matches from the anchor on, k
# bytes more.  The anchor is always a parse point, and there rep1 - 1 was a candidate with offset value 3 and a gain of
# 4 (ml + k) - 1.  Every move of the look-ahead raises the gain strictly, so the candidate finally taken has more than that,
# but it has 4 ml - floor(log2(o + 3)), which is less.  (The anchor 0 is never reached: the extension needs p > o >= 1.)
UNREACHABLE = ("p2.run_at_end", "back.rep_front", "back.ov_changed")

BULK = ("p2.mm_fail", "p2.longer", "p2.shorter", "la2.untried", "la2.tried")         # counted, positions not kept


class Trace:
    def __init__(self):
        self.count = collections.Counter()
        self.where = collections.defaultdict(set)       # label -> positions, but for BULK

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
        return sorted(k for k, v in self.count.items() if v)


# ------------------------------------------------------------------------------------------------ the serial model
def hash_of(b, p, mm, hbits):
    """the hash of the mini_match bytes at p: Knuth's multiplier on the little-endian word, the fourth byte shifted out for
    mini_match 3 (header: "the same hash of mini_match bytes")"""
    v = b[p] | b[p + 1] << 8 | b[p + 2] << 16 | ((b[p + 3] << 24) if mm == 4 else 0)
    if mm == 3:
        v <<= 8
    return ((v * 2654435761) & 0xffffffff) >> (32 - hbits)


def _count(a, p, q, limit):
    """common prefix of a[p:] and a[q:], at most limit bytes (numpy: the only use of it in the model)"""
    k = 0
    step = 64
    while k < limit:
        w = min(step, limit - k)
        ne = np.flatnonzero(a[p + k:p + k + w] != a[q + k:q + k + w])
        if len(ne):
            return k + int(ne[0])
        k += w
        step *= 8
    return limit


def hb(v):
    return v.bit_length() - 1


def p1_chain(b, hw_buff_sz, mm, hshift=2, T=None):
    """P1: per position the distance to the nearest earlier position with the same hash of mm bytes, 0 for none"""
    n = len(b)
    hbits = hw_buff_sz.bit_length() - 1 - hshift
    chain = [0] * n
    last = {}
    for p in range(n):
        if p + mm > n:
            if T:
                T.hit("p1.tail", p)
            continue
        h = hash_of(b, p, mm, hbits)
        q = last.get(h)
        if q is not None:
            chain[p] = p - q
            if T:
                T.hit("p1.lane" if q >= p - p % 64 else "p1.head", p)
                if b[q:q + mm] != b[p:p + mm]:
                    T.hit("p1.collision", p)
                elif mm == 3 and p + 4 <= n and b[q + 3] != b[p + 3]:
                    T.hit("p1.mm3_fourth", p)
        last[h] = p
    return chain


def p2_search(b, chain, mm, depth, T):
    """P2: per position the longest match of at least mm bytes among the first `depth` candidates of its chain, the nearer
    among equals; a walk ends early only where the match reaches the chunk's end"""
    n = len(b)
    a = np.frombuffer(b, np.uint8) if n else np.zeros(0, np.uint8)
    res = [(0, 0)] * n
    run = {}                                            # slot -> (d, p0, e): the trace's own, no answer depends on it
    gone = set()                                        # distances whose entry was replaced
    for P0 in range(0, n, 64):
        lanes = []
        for p in range(P0, min(P0 + 64, n)):
            if p + mm <= n and chain[p]:
                lanes.append({"p": p, "cur": p - chain[p], "best": 0, "bd": 0, "hops": 0, "max": n - p})
        active = lanes
        while active:
            nxt = []
            for L in active:                            # ascending lanes: the order in which the wave finishes capped ones
                p, cur, best, maxlen = L["p"], L["cur"], L["best"], L["max"]
                nd = chain[cur]
                ln = 0
                if b[cur:cur + mm] == b[p:p + mm]:
                    lim = min(maxlen, LANECAP)
                    ln = _count(a, p, cur, lim)
                    if ln >= LANECAP and ln < maxlen:
                        if best < LANECAP or b[cur + best] == b[p + best]:
                            d = p - cur
                            slot = ((d * 2654435761) & 0xffffffff) >> (32 - RUNBITS)
                            ent = run.get(slot)
                            if ent and ent[0] == d and ent[1] <= p < ent[2]:
                                T.hit("p2.run_hit", p)
                                ln = ent[2] - p
                                assert maxlen > 8192 or ln == _count(a, p, cur, maxlen)      # the table changes no answer
                            else:
                                if ent and ent[0] == d:
                                    T.hit("p2.run_before" if ent[1] > p else "p2.run_at_end" if ent[2] == p else "p2.run_past", p)
                                else:
                                    T.hit("p2.run_miss", p)
                                    if ent:
                                        T.hit("p2.run_replace", p)
                                        gone.add(ent[0])
                                    if d in gone:
                                        T.hit("p2.run_again", p)
                                        gone.discard(d)
                                ln = LANECAP + _count(a, p + LANECAP, cur + LANECAP, maxlen - LANECAP)
                                run[slot] = (d, p, p + ln)
                        else:
                            T.hit("p2.cap_guard", p)
                            ln = -LANECAP               # (not its true length: no length label)
                    if ln in (31, 32, 33):
                        T.hit("p2.len%d" % ln, p)
                    ln = abs(ln)
                else:
                    T.hit("p2.mm_fail", p)
                if ln >= mm:
                    if ln > best:
                        T.hit("p2.longer", p)
                        best = L["best"] = ln
                        L["bd"] = p - cur
                    else:
                        T.hit("p2.equal" if ln == best else "p2.shorter", p)
                L["hops"] += 1
                if best == maxlen:
                    T.hit("p2.end_reach", p)
                elif nd == 0:
                    T.hit("p2.end_chain", p)
                elif L["hops"] >= depth:
                    T.hit("p2.end_depth", p)
                else:
                    L["cur"] = cur - nd
                    nxt.append(L)
            active = nxt
        for L in lanes:
            res[L["p"]] = (L["best"], L["bd"])
    return res


def offset_value(off, ll, r):
    """RFC 8878 3.1.1.5: the repeat codes with and without literals in front; the lowest one that names the offset"""
    cands = (r[0], r[1], r[2]) if ll else (r[1], r[2], r[0] - 1)
    for k in range(3):
        if off == cands[k]:
            return k + 1
    return off + 3


def p3_lazy(b, res, mm, depth, mingain, lazy2, T):
    """P3: the lazy evaluation -> (records, literals)"""
    n = len(b)
    a = np.frombuffer(b, np.uint8) if n else np.zeros(0, np.uint8)
    r = [1, 4, 8]
    seqs, lits = [], bytearray()

    def best_at(p, ll, trace):
        """(ml, off, ov, gain) or None"""
        hit = T.hit if trace else (lambda *_: None)
        c = None
        sl, sd = res[p]
        if sl >= mm:
            ov = offset_value(sd, ll, r)
            gain = 4 * sl - hb(ov)
            if ov <= 3:
                hit("stored.rep%d.ll%d" % (ov, 1 if ll else 0), p)
            if gain == mingain - 1:
                hit("stored.refused_9", p)
            if gain == mingain:
                hit("stored.taken_10", p)
            if gain >= mingain:
                c = (sl, sd, ov, gain)
        cands = (r[0], r[1], r[2]) if ll else (r[1], r[2], r[0] - 1)
        for off in cands:
            if off == 0:
                hit("rep.skip_zero", p)
                continue
            if off > p:
                hit("rep.skip_beyond", p)
                continue
            if c and off == c[1]:
                hit("rep.skip_same", p)
                continue
            if b[p:p + mm] != b[p - off:p - off + mm]:
                continue
            ml = _count(a, p, p - off, n - p)
            ov = offset_value(off, ll, r)
            gain = 4 * ml - hb(ov)
            if c is None:
                hit("rep.only", p)
                c = (ml, off, ov, gain)
            elif gain > c[3]:
                hit("rep.beats", p)
                c = (ml, off, ov, gain)
            elif gain < c[3]:
                hit("rep.loses", p)
            elif ov < c[2]:
                hit("rep.tie_lower", p)
                c = (ml, off, ov, gain)
            else:
                hit("rep.tie_stays", p)
        return c

    p = anchor = 0
    if n < mm:
        T.hit("end.short_chunk", 0)
    while p + mm <= n:
        c = best_at(p, p > anchor, True)
        if c is None:
            p += 1
            continue
        moves = 0
        while True:
            moved = False
            T.hit("la2.tried" if depth >= lazy2 else "la2.untried", p)
            for step in ((1, 2) if depth >= lazy2 else (1,)):
                if p + step + mm > n:
                    T.hit("la.cut_by_end", p)
                    break
                c2 = best_at(p + step, True, True)
                margin = 4 if step == 1 else 7
                if c2:
                    if c2[3] == c[3] + margin:
                        T.hit("la1.stay_4" if step == 1 else "la2.stay_7", p)
                    if c2[3] == c[3] + margin + 1:
                        T.hit("la1.move_5" if step == 1 else "la2.move_8", p)
                    if c2[3] > c[3] + margin:
                        c = c2
                        p += step
                        moved = True
                        break
            if not moved:
                break
            moves += 1
            if moves in (2, 3):
                T.hit("la.restart%d" % moves, p)
        ml, off, ov, gain = c
        if ov > 3:
            while p > anchor and p > off and b[p - 1] == b[p - 1 - off]:
                p -= 1
                ml += 1
            if p == anchor:
                if ml > c[0]:
                    T.hit("back.anchor", p)
            elif p == off:
                T.hit("back.at_off", p)
            else:
                T.hit("back.mismatch", p)
        elif p > anchor:
            T.hit("back.none_rep", p)
            if p > off and b[p - 1] == b[p - 1 - off]:
                T.hit("back.rep_front", p)
        ll = p - anchor
        ov2 = offset_value(off, ll != 0, r)
        if ov2 != ov:
            T.hit("back.ov_changed", p)
        ov = ov2
        lits += b[anchor:p]
        seqs.append((ll, ml, off))
        # the history (RFC 8878 3.1.1.5): a repeat code moves its offset to the front, a new offset pushes the others down
        if ll and ov == 1:
            T.hit("push.keep.ll1", p)
        elif (ll and ov == 2) or (not ll and ov == 1):
            T.hit("push.swap.ll1" if ll else "push.swap.ll0", p)
            r[0], r[1] = off, r[0]
        else:
            T.hit("push.rot.ll1" if ll else "push.rot.ll0", p)
            r[0], r[1], r[2] = off, r[0], r[1]
        p += ml
        anchor = p
        if p == n:
            T.hit("end.match_at_end", p)
        elif n - p < mm:
            T.hit("end.tail", p)
    lits += b[anchor:]
    return seqs, bytes(lits)


def model(chunk, hw_buff_sz, mini_match, depth, mingain=10, lazy2=64, hshift=2):
    """-> (chain, res, seqs, literals, trace) of one chunk of at most hw_buff_sz bytes"""
    b = bytes(chunk)
    assert len(b) <= hw_buff_sz and hw_buff_sz in HWS and mini_match in (3, 4) and 1 <= depth <= 256
    T = Trace()
    T.hit("p1.width.%d" % hw_buff_sz, 0)
    chain = p1_chain(b, hw_buff_sz, mini_match, hshift, T)
    res = p2_search(b, chain, mini_match, depth, T)
    seqs, lits = p3_lazy(b, res, mini_match, depth, mingain, lazy2, T)
    return chain, res, seqs, lits, T


# ------------------------------------------------------------------------------------------------ building blocks
Trap = collections.namedtuple("Trap", "name family data hw_buff_sz mini_match depth aim check")
_TRAPS = []
ASKS = collections.OrderedDict()                        # trap name -> the labels its check asks for


def trap(name, family, data, hw, mm, depth, aim, check):
    data = bytes(data)
    assert len(data) <= hw
    ASKS[name] = tuple(check.labels)
    _TRAPS.append(Trap(name, family, data, hw, mm, depth, aim, check))


def _chk(fn, labels=()):
    fn.labels = tuple(labels)
    return fn


def starts(seqs):
    """[(position, match length, offset)] of the records"""
    out, p = [], 0
    for ll, ml, off in seqs:
        p += ll
        out.append((p, ml, off))
        p += ml
    return out


def has_at(pos, ml, off):
    return _chk(lambda seqs, tr: (pos, ml, off) in starts(seqs))


def has_rec(pos, ll, ml, off):
    """a record with exactly ll literals in front"""
    return _chk(lambda seqs, tr: any(s == (pos, ml, off) and q[0] == ll for s, q in zip(starts(seqs), seqs)))


def none_at(lo, hi):
    """no match begins in [lo, hi)"""
    return _chk(lambda seqs, tr: not any(lo <= s[0] < hi for s in starts(seqs)))


def fired(label, pos=None):
    assert label in LABELS, label
    return _chk((lambda seqs, tr: label in tr) if pos is None else (lambda seqs, tr: tr.at(label, pos)), (label,))


def both(*cs):
    return _chk(lambda seqs, tr: all(c(seqs, tr) for c in cs), [x for c in cs for x in c.labels])


def colliding_words(mm, same_bits, other_bits, seed):
    """two words of mm bytes (in four) with one hash at same_bits and two at other_bits"""
    rs = np.random.RandomState(seed)
    seen = {}
    while True:
        w = rs.randint(0, 256, 4, dtype=np.uint8).tobytes()
        h = hash_of(w, 0, mm, same_bits)
        for o in seen.get(h, []):
            if o[:mm] != w[:mm] and hash_of(o, 0, mm, other_bits) != hash_of(w, 0, mm, other_bits) and not set(o) & set(w):
                return o[:mm], w[:mm]
        seen.setdefault(h, []).append(w)


def colliding_distances(lo, hi):
    """two distances in [lo, hi) whose run-table slots collide"""
    seen = {}
    for d in range(lo, hi):
        s = ((d * 2654435761) & 0xffffffff) >> (32 - RUNBITS)
        if s in seen and d - seen[s] > 60:
            return seen[s], d
        seen.setdefault(s, d)
    raise AssertionError


K1, S4 = 1024, 4096


def ballast(B, at=780, ln=200):
    """a long copy of the chunk's bytes 8.. far from the trap: the block shrinks whatever else happens, and the trap's decision
    stays visible in the frame instead of vanishing in a raw block"""
    return B.plant(at, 8, ln)
CI = (K1, 4, 16)            # hw_buff_sz, mini_match, depth of the 1024-byte traps that also run as the chunks of one call


# ------------------------------------------------------------------------------------------------ A: chains
def _family_a():
    # the 64 positions of one trip of the chain kernel: 1024 .. 1087
    for k in (2, 3):
        B = Buf(S4, 210 + k)
        for i in range(1, k):
            B.plant(1030 + 10 * i, 1030, 8)
        last = 1030 + 10 * (k - 1)
        B.plant(2000, 1030, 8)
        trap("a_trip_same_word_%d_times" % k, "A", B.bytes(), S4, 4, 4, "the same word %d times inside one trip (1024..1087), met again at 2000: the nearest one" % k,
             both(has_at(1040, 8, 10), has_at(last, 8, 10), has_at(2000, 8, 2000 - last), fired("p1.lane", 1040), fired("p1.lane", last),
                  fired("p1.head", 2000)))
    for per, mm in ((1, 3), (2, 3), (3, 4), (63, 4), (64, 4), (65, 4)):
        B = Buf(S4, 220 + per)
        pat = bytes(B.b[1060:1060 + per])
        B.put(1060, (pat * (400 // per + 1))[:400])
        B.b[1059] = pat[-1] ^ 0x55; B.b[1460] = pat[400 % per] ^ 0x55
        trap("a_period_%d" % per, "A", B.bytes(), S4, mm, 4, "period %d from 1060 on over seven trips: position %d finds 1060" % (per, 1060 + per),
             both(has_at(1060 + per, 400 - per, per), fired("p1.lane" if per < 28 else "p1.head", 1060 + per), fired("p2.run_hit")))
    # a colliding word between a word and its only copy, depth 1: it costs the one hop.  The copy is mini_match bytes and no
    # more, so no later position finds it and nothing extends back over it
    for mm in (3, 4):
        for tag, bits in (("narrower", (8, 9)), ("as_is", (7, 8))):
            w1, w2 = colliding_words(mm, bits[0], bits[1], 40 + mm)
            B = ballast(Buf(K1, 240 + mm))
            src, dst = (500, 503) if mm == 3 else (420, 500)        # offset 3 / 80: a gain of exactly 10
            mid = 502 if mm == 3 else 460
            if mm == 3:
                B.put(src - 8, w2)
            else:
                B.put(mid, w2)
            B.put(src, w1); B.put(dst, w1)
            B.b[dst + mm] = B.b[src + mm] ^ 0x55; B.b[src - 1] = B.b[dst - 1] ^ 0x55
            if mm == 3:
                # three bytes pay only from 4 back or less (and 1 and 4 are repeat offsets of a fresh history): the colliding
                # word cannot stand between.  It stands in front: no trap of the hop, one of the collision at the source
                chk = both(has_at(dst, 3, 3), fired("p1.collision", src), fired("stored.taken_10", dst))
                aim = "a colliding word 8 in front of a word, its copy 3 behind: the word's chain leads to the other bytes, the copy's to the word"
            elif tag == "narrower":
                chk = both(none_at(dst - 3, dst + mm), fired("p1.collision", dst), fired("p2.mm_fail"))
                aim = "a word with the same 8 hash bits (not 9) between a word and its copy, depth 1: the hop is spent, no match"
            else:
                chk = both(has_at(dst, 4, 80), fired("stored.taken_10", dst))
                aim = "a word with the same 7 hash bits (not 8) between a word and its copy, depth 1: no collision at 8 bits, the copy is found"
            trap("a_collision_mm%d_%s" % (mm, tag), "A", B.bytes(), K1, mm, 1, aim, chk)
    w = rnd(5, 250)
    for mm in (3, 4):
        B = ballast(Buf(K1, 251))
        B.put(500, w[:3] + w[:3] + bytes([w[0] ^ 0x55]))
        B.b[499] = w[2] ^ 0x2a
        trap("a_three_bytes_then_another_mm%d" % mm, "A", B.bytes(), K1, mm, 16,
             "abcabcX: mini_match 3 finds abc 3 back (gain 10) whatever the fourth byte, mini_match 4 finds nothing",
             both(has_at(503, 3, 3), fired("p1.mm3_fourth", 503), fired("stored.taken_10", 503)) if mm == 3 else none_at(496, 512))


# ------------------------------------------------------------------------------------------------ B: the walk and its depth
def _attempt_trap(k, seed):
    """cur holds W T (4 + 20 bytes).  Its k-th candidate, the farthest, is the only whole copy.  The k - 1 nearer ones, 12
    bytes apart, hold W T[0:4] and then another byte: 8 bytes each, the nearest stays.  Every position of W T[0:4] has the
    same k candidates, so a walk of fewer than k hops leaves 8 bytes from 12 back and 16 from the far copy"""
    B = Buf(S4, seed)
    cur = 3700
    W, T = rnd(4, seed + 1000), rnd(20, seed + 2000)
    far = cur - 12 * (k - 1) - 24
    B.put(cur, W + T).put(far, W + T)
    B.b[cur + 24] = B.b[far + 24] ^ 0x55
    for i in range(1, k):
        f = cur - 12 * i
        B.put(f, W + T[:4] + bytes([T[4] ^ (1 + i % 200), (i * 7) & 255, 0x80 | (i & 127), (i * 13 + 5) & 255]))
    B.b[far - 1] = B.b[cur - 1] ^ 0x55
    return B.bytes(), cur, cur - far


def _family_b():
    for depth in DEPTHS:
        for k in (depth, depth + 1):
            data, cur, off = _attempt_trap(k, 300 + k)
            if k <= depth:
                chk = both(has_at(cur, 24, off), *([fired("p2.equal", cur)] if k >= 3 else []))
            else:
                chk = both(has_at(cur, 8, 12), has_at(cur + 8, 16, off), fired("p2.end_depth", cur))
            trap("b_whole_copy_is_candidate_%d_depth_%d" % (k, depth), "B", data, S4, 4, depth,
                 "the only whole copy is candidate %d: %s" % (k, "taken" if k <= depth else "out of reach, 8 + 16 bytes"), chk)


# ------------------------------------------------------------------------------------------------ C: lengths and the run table
def _flush(B):
    """three unrelated matches between 470 and 560: what was a repeat offset before them is none behind them, so the search's
    choice is the parse's"""
    return B.plant(470, 30, 8).plant(500, 50, 8).plant(530, 70, 8)


def _family_c():
    for ln in (31, 32, 33, 287, 288, 289):
        B = Buf(K1, 400 + ln)
        B.plant(600, 100, ln)
        lab = [fired("p2.len%d" % ln, 600)] if ln < 34 else []
        trap("c_length_%d" % ln, "C", B.bytes(), *CI, "a match of exactly %d bytes (a lane counts 32, the wave 256 a trip)" % ln,
             both(has_at(600, ln, 500), *lab))
    B = _flush(Buf(K1, 410).plant(400, 100, 12)).plant(700, 100, 12)
    trap("c_equal_lengths_nearer_stays", "C", B.bytes(), *CI, "two candidates of 12 bytes: the nearer one stays", both(has_at(700, 12, 300), fired("p2.equal", 700), fired("p1.width.1024")))
    B = _flush(Buf(K1, 411).plant(400, 100, 12)).plant(700, 100, 13)
    trap("c_farther_one_byte_longer", "C", B.bytes(), *CI, "the farther candidate is one byte longer: it wins", both(has_at(700, 13, 600), fired("p2.longer")))
    B = _flush(Buf(K1, 422).plant(400, 100, 13)).plant(700, 400, 13)
    B.b[112] ^= 0x55
    trap("c_farther_one_byte_shorter", "C", B.bytes(), *CI, "the farther candidate is one byte shorter: the nearer stays", both(has_at(700, 13, 300), fired("p2.shorter")))
    B = _flush(Buf(K1, 413).plant(400, 100, 50)).plant(700, 400, 50)
    B.b[135] ^= 0x55
    trap("c_capped_candidate_cannot_pass", "C", B.bytes(), *CI,
         "best is 50; the next candidate agrees in 35 bytes: capped at 32, the byte behind best differs, the wave does not count it",
         both(has_at(700, 50, 300), fired("p2.cap_guard", 700)))
    B = Buf(K1, 414)
    B.plant(K1 - 50, 100, 50, guard=False); B.b[K1 - 51] = B.b[99] ^ 0x55
    trap("c_match_reaches_the_end", "C", B.bytes(), *CI, "the first candidate reaches the chunk's end: the walk stops",
         both(has_at(K1 - 50, 50, K1 - 150), fired("p2.end_reach", K1 - 50), fired("end.match_at_end", K1)))
    d1, d2 = colliding_distances(300, 900)
    B = Buf(S4, 415)
    B.plant(1500, 1500 - d1, 40).plant(2000, 2000 - d2, 40).plant(2500, 2500 - d1, 40).plant(2600, 2600 - d1, 40)
    trap("c_run_table_slot_of_two_distances", "C", B.bytes(), 32768, 4, 16,
         "matches of 40 at distances %d, %d, %d, %d: one slot, replaced, asked for again, and found with its end behind" % (d1, d2, d1, d1),
         both(has_at(1500, 40, d1), has_at(2000, 40, d2), has_at(2500, 40, d1), has_at(2600, 40, d1), fired("p2.run_miss", 1500), fired("p2.run_hit", 1501),
              fired("p2.run_replace", 2000), fired("p2.run_again", 2500), fired("p2.run_past", 2600)))
    # lane 0 of the trip 2048 .. 2111 reaches distance 900 in its second round, lane 63 in its first: the entry of 900 is
    # lane 63's, p0 = 2111, when lane 0 asks - and lane 0's match ends at 2081
    B = Buf(S4, 416)
    B.plant(2048, 1148, 33).plant(2111, 1211, 40)
    B.put(2020, bytes(B.b[2048:2052])); B.b[2024] = B.b[2052] ^ 0x55; B.b[2019] = B.b[2047] ^ 0x2a
    trap("c_run_table_entry_of_a_later_lane", "C", B.bytes(), 32768, 4, 16,
         "the slot holds the distance from a later position of the trip: not a hit, counted: 33 bytes, not 103",
         both(has_at(2048, 33, 900), has_at(2111, 40, 900), fired("p2.run_before", 2048)))


# ------------------------------------------------------------------------------------------------ D: the lazy evaluation, by hand
def _family_d():
    for mm, cases in ((3, ((3, True), (5, False))), (4, ((124, True), (125, False)))):
        for off, taken in cases:
            B = ballast(Buf(K1, 500 + off))
            B.plant(600, 600 - off, mm)
            trap("d_gain_%d_mm%d" % (10 if taken else 9, mm), "D", B.bytes(), K1, mm, 16,
                 "%d bytes from %d back: a gain of %d, %s" % (mm, off, 10 if taken else 9, "taken" if taken else "literals"),
                 both(has_at(600, mm, off), fired("stored.taken_10", 600)) if taken else both(none_at(598, 600 + mm), fired("stored.refused_9", 600)))
    B = Buf(K1, 510).plant(600, 100, 40)
    B.b[620] ^= 0x55
    trap("d_repeat_behind_a_changed_byte", "D", B.bytes(), *CI, "a copy with one byte changed: the second half has one literal and rep1",
         both(has_rec(600, 600, 20, 500), has_rec(621, 1, 19, 500), fired("stored.rep1.ll1", 621), fired("push.keep.ll1", 621), fired("back.none_rep", 621),
              fired("rep.skip_same", 621)))
    B = Buf(K1, 511).plant(600, 100, 20).plant(620, 121, 19)
    B.plant(30, 620, 20)
    trap("d_rep1_less_1_beats_a_longer_match", "D", B.bytes(), *CI,
         "a copy with one byte dropped, and its 19 bytes with the next one again 590 back: the search keeps those 20 (gain 71), the parse takes rep1 - 1 (75)",
         both(has_at(600, 20, 500), has_rec(620, 0, 19, 499), fired("rep.beats", 620), fired("push.rot.ll0", 620)))
    B = Buf(K1, 512).plant(600, 100, 20).plant(620, 121, 19)
    trap("d_stored_match_is_rep1_less_1", "D", B.bytes(), *CI, "a copy with one byte dropped: the stored match's distance is rep1 - 1, offset value 3",
         both(has_rec(620, 0, 19, 499), fired("stored.rep3.ll0", 620), fired("push.rot.ll0", 620)))
    B = Buf(K1, 513)
    B.put(600, bytes([B.b[600]]) * 40)
    B.plant(640, 100, 12)
    B.b[599] = B.b[600] ^ 0x55
    trap("d_rep1_is_1", "D", B.bytes(), *CI, "a run of one byte, then a copy at once: rep1 - 1 is 0 and no offset",
         both(has_rec(601, 601, 39, 1), has_rec(640, 0, 12, 540), fired("rep.skip_zero", 640)))
    B = Buf(K1, 514).plant(600, 100, 20)
    B.plant(621, 121, 9)
    B.plant(21, 621, 10)
    trap("d_repeat_is_priced_as_one", "D", B.bytes(), *CI,
         "rep1 gives 9 bytes (gain 36), the stored match 10 bytes from 600 back (gain 31): the repeat wins only at its own price",
         both(has_rec(621, 1, 9, 500), fired("rep.beats", 621)))
    B = Buf(K1, 515).plant(600, 100, 20)
    B.plant(621, 121, 9)
    B.plant(601, 621, 10)
    trap("d_tie_goes_to_the_lower_offset_value", "D", B.bytes(), *CI,
         "rep1 gives 9 bytes (gain 36), the stored match 10 bytes from 20 back (gain 40 - 4): a tie, the repeat has the lower offset value",
         both(has_rec(621, 1, 9, 500), fired("rep.tie_lower", 621)))
    # the look-ahead: 8 bytes at p from o1 back, more from p + 1 (p + 2) on from o2 back
    p = 900
    for name, a, l2, o1, o2, depth, want, lab, aim in (
            ("d_ahead_1_gains_4", 1, 9, 700, 600, 16, 0, "la1.stay_4", "9 bytes at p + 1, as far: 4 more, stays"),
            ("d_ahead_1_gains_5", 1, 10, 100, 600, 16, 1, "la1.move_5", "10 bytes at p + 1, three bits farther: 5 more, moves"),
            ("d_ahead_2_gains_7", 2, 10, 400, 700, 64, 0, "la2.stay_7", "10 bytes at p + 2, one bit farther: 7 more, stays"),
            ("d_ahead_2_gains_8", 2, 10, 700, 600, 64, 2, "la2.move_8", "10 bytes at p + 2, as far: 8 more, moves"),
            ("d_ahead_2_at_depth_63", 2, 10, 700, 600, 63, 0, "la2.untried", "the same input at depth 63: p + 2 is not looked at"),
            ("d_ahead_2_at_depth_64", 2, 10, 700, 600, 64, 2, "la2.tried", "... and at depth 64 it is")):
        B = Buf(K1, 520)
        B.plant(p - o1, p, 8).plant(p + a - o2, p + a, l2)
        chk = has_at(p, 8, o1) if want == 0 else has_at(p + a, l2, o2)
        trap(name, "D", B.bytes(), K1, 4, depth, aim, both(chk, fired(lab, p) if lab[4:] not in ("untried", "tried") else fired(lab)))
    B = Buf(K1, 521)
    B.plant(p - 600, p, 8).plant(p + 1 - 650, p + 1, 10).plant(p + 2 - 700, p + 2, 12).plant(p + 3 - 750, p + 3, 14)
    trap("d_look_ahead_restarts_three_times", "D", B.bytes(), *CI, "8, 10, 12, 14 bytes at p .. p + 3, each 8 more than the one before: the last one",
         both(has_at(p + 3, 14, 750), fired("la.restart2", p + 2), fired("la.restart3", p + 3), fired("back.mismatch", p + 3)))
    x = rnd(20, 522)
    B = Buf(K1, 523).put(0, x + x)
    B.b[40] = x[0] ^ 0x55
    trap("d_backwards_to_p_equals_off", "D", B.bytes(), *CI, "the chunk's first 20 bytes twice: the match at 20 has nothing in front of its source",
         both(has_rec(20, 20, 20, 20), fired("back.at_off", 20), fired("p2.end_chain", 20)))
    # the match begins one byte late for the search (the word at 599 has a colliding word in front, depth 1) and is extended
    # back to the anchor, the end of the match before
    w1, w2 = colliding_words(4, 8, 9, 44)
    B = Buf(K1, 524)
    B.put(100, w1); B.plant(580, 60, 19); B.put(560, w2); B.plant(599, 100, 16)
    trap("d_backwards_to_the_anchor", "D", B.bytes(), K1, 4, 1, "a match found one byte late is extended back to the end of the match before: no literals",
         both(has_rec(599, 0, 16, 499), fired("back.anchor", 599)))


# ------------------------------------------------------------------------------------------------ D: the searched inputs
from lz4hc_traps import sm_input  # noqa: E402  (small alphabet, overlapping copies, a few stretches of random bytes)

SM_SIZES = (256, 1024)
SM_MODES = ((3, 4), (4, 16), (3, 64), (4, 64))          # (mini_match, depth) the search runs every input at
# label -> (size, seed, mini_match, depth): the smallest input of the search whose trace holds the label
SM_SEEDS = {
    "stored.refused_9": (256, 0, 3, 4),
    "stored.taken_10": (256, 0, 3, 4),
    "stored.rep1.ll1": (256, 0, 3, 4),
    "stored.rep2.ll1": (256, 0, 3, 64),
    "stored.rep3.ll1": (256, 1, 3, 4),
    "stored.rep1.ll0": (256, 2, 3, 4),
    "stored.rep2.ll0": (256, 2, 3, 4),
    "stored.rep3.ll0": (256, 1, 3, 4),
    "rep.skip_zero": (256, 0, 3, 4),
    "rep.skip_beyond": (256, 0, 3, 4),
    "rep.skip_same": (256, 0, 3, 4),
    "rep.only": (256, 3, 3, 64),
    "rep.beats": (256, 2, 3, 4),
    "rep.loses": (256, 2, 3, 4),
    "rep.tie_lower": (256, 10, 3, 4),
    "rep.tie_stays": (256, 16, 3, 64),
    "la1.stay_4": (256, 2, 3, 4),
    "la1.move_5": (256, 11, 3, 4),
    "la2.stay_7": (256, 10, 3, 64),
    "la2.move_8": (256, 5, 3, 64),
    "la2.untried": (256, 0, 3, 4),
    "la2.tried": (256, 0, 3, 64),
    "la.restart2": (256, 2, 3, 64),
    "la.restart3": (256, 245, 4, 16),
    "la.cut_by_end": (256, 0, 4, 64),
    "back.anchor": (256, 2, 3, 4),
    "back.mismatch": (256, 0, 3, 4),
    "back.at_off": (256, 0, 3, 4),
    "back.none_rep": (256, 0, 3, 4),
    "push.keep.ll1": (256, 0, 3, 4),
    "push.swap.ll1": (256, 2, 3, 4),
    "push.swap.ll0": (256, 2, 3, 4),
    "push.rot.ll1": (256, 0, 3, 4),
    "push.rot.ll0": (256, 0, 3, 4),
    "end.match_at_end": (256, 0, 3, 4),
    "end.tail": (256, 3, 4, 16),
}


def _family_sm():
    by_input = collections.OrderedDict()
    for label in LABELS:
        if label in SM_SEEDS:
            by_input.setdefault(SM_SEEDS[label], []).append(label)
    for (n, seed, mm, depth), labels in by_input.items():
        trap("d_searched_%d_%d_mm%d_depth%d" % (n, seed, mm, depth), "D", sm_input(seed, n), K1, mm, depth, "fires " + ", ".join(labels),
             both(*[fired(x) for x in labels]))


# ------------------------------------------------------------------------------------------------ E: the ends
def _family_e():
    for mm in (3, 4):
        for left in range(0, mm):
            B = Buf(K1, 600 + left)
            B.plant(K1 - left - 20, 100, 20, guard=False)
            B.b[K1 - left - 21] = B.b[99] ^ 0x55
            if left:
                B.b[K1 - left] = B.b[120] ^ 0x55
            trap("e_last_match_leaves_%d_mm%d" % (left, mm), "E", B.bytes(), K1, mm, 16, "the last match ends %d bytes before the chunk's end" % left,
                 both(has_at(K1 - left - 20, 20, K1 - left - 120), fired("end.tail" if left else "end.match_at_end", K1 - left),
                      *([fired("p1.tail", K1 - 1)] if left == 0 else [])))
        for n in range(1, mm + 1):
            trap("e_chunk_of_%d_mm%d" % (n, mm), "E", b"\x07" * n, K1, mm, 4, "%d equal bytes" % n,
                 both(_chk(lambda seqs, tr: seqs == []), fired("end.short_chunk", 0) if n < mm else fired("p1.tail", n - 1)))
        unit = rnd(mm + 1, 610 + mm)
        B = ballast(Buf(K1, 611), 700)
        B.put(K1 - 2 * mm - 1, unit + unit[:mm])
        B.b[K1 - 2 * mm - 2] = unit[mm] ^ 0x55
        if mm == 3:
            chk = both(has_at(K1 - 3, 3, 4), fired("la.cut_by_end", K1 - 3), fired("end.match_at_end", K1))
        else:
            chk = both(has_at(K1 - 4, 4, 5), fired("la.cut_by_end", K1 - 4), fired("end.match_at_end", K1))
        trap("e_match_in_the_last_%d_bytes" % mm, "E", B.bytes(), K1, mm, 64, "the last %d bytes repeat %d back: found, and nothing to look ahead to" % (mm, mm + 1), chk)


# ------------------------------------------------------------------------------------------------ F: geometry
def _family_f():
    depths = {2048: 16, 4096: 63, 8192: 256, 16384: 64, 32768: 16, 65536: 64}
    for hw in HWS[1:7]:
        mm = 3 if hw in (2048, 8192, 32768) else 4
        B = Buf(hw, 700 + hw // 1024).plant(hw - 300, 200, 20)
        trap("f_chunk_of_%d" % hw, "F", B.bytes(), hw, mm, depths[hw], "hw_buff_sz %d: the head table's width; a copy from %d back" % (hw, hw - 500),
             both(has_at(hw - 300, 20, hw - 500), fired("p1.width.%d" % hw), fired("p1.head", hw - 300)))
    n = 131072
    B = Buf(n, 710).plant(70000, 70000 - 65535, 12).plant(100000, 100000 - 65536, 12)
    trap("f_offsets_65535_and_65536", "F", B.bytes(), n, 4, 4, "copies from 65535 and from 65536 back: both taken (the default parse ends at 65535)",
         both(has_at(70000, 12, 65535), has_at(100000, 12, 65536), fired("p1.width.131072")))
    # an offset of 131071 would need a match at position 131071, the chunk's last byte; the last position with mini_match
    # bytes behind it is n - mini_match, and its farthest source is position 0
    trap("f_one_match_from_1_to_the_end", "F", b"A" * n, n, 3, 4, "131072 equal bytes: one literal and one match of 131071 bytes, every walk one hop long",
         both(_chk(lambda seqs, tr: seqs == [(1, n - 1, 1)]), fired("p2.end_reach", 1), fired("p2.end_reach", n - 3), fired("rep.skip_same", 1),
              fired("end.match_at_end", n)))
    B = ballast(Buf(n, 712), 60000, 300)
    B.plant(n - 12, 0, 12, guard=False); B.b[n - 13] = 0x11
    trap("f_the_largest_offset_taken", "F", B.bytes(), n, 4, 16, "the chunk's last 12 bytes are its first 12: offset 131060 (the largest of all, 131072 - mini_match, pays for no match of mini_match bytes)",
         both(has_at(n - 12, 12, n - 12), fired("end.match_at_end", n), fired("p2.end_reach", n - 12)))


_BUILT = None


def all_traps():
    """every trap, in a fixed order (built once per process)"""
    global _BUILT
    if _BUILT is None:
        del _TRAPS[:]
        ASKS.clear()
        for fam in (_family_a, _family_b, _family_c, _family_d, _family_sm, _family_e, _family_f):
            fam()
        names = [t.name for t in _TRAPS]
        assert len(set(names)) == len(names)
        _BUILT = list(_TRAPS)
    return _BUILT


def independent_traps():
    """the 1024-byte traps with the mini_match and depth of CI: the chunks of one call at hw_buff_sz 1024"""
    return [t for t in all_traps() if (len(t.data), t.hw_buff_sz, t.mini_match, t.depth) == (K1,) + CI]


def label_traps():
    """label -> the traps whose check asks for it"""
    all_traps()
    out = collections.OrderedDict((lab, []) for lab in LABELS)
    for name, labs in ASKS.items():
        for lab in labs:
            if name not in out[lab]:
                out[lab].append(name)
    return out


def trap_table():
    return "\n".join("  %-18s %s" % (lab, ", ".join(names) if names else "UNREACHABLE" if lab in UNREACHABLE else "-") for lab, names in label_traps().items())
