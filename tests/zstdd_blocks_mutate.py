"""Corrupted many-block zstd frames for the decoder's block route (tests/test_sim_zstdd_blocks_corrupt.py,
tests/test_gpu_zstd_dec_blocks_corrupt.py): tests/zstdd_mutate.py's mutants - a mutant is (base name, position, value), none
is stored, nothing is random - over the frames of tests/golden/zstd_dec_blocks/, each decoded under route `blocks` with the
host walk's count, under route `blocks` with the base's count (the stale hint) and by stage E.

Bases: every case of the index that decodes (sim[0] == 0) and the refusals with status -1, -2, -3 and -4; the three r_count_*
cases (a wrong count over a good frame) are none.  The frames of at most EXHAUSTIVE_MAX bytes come first, then the larger
ones, each in the index's order.  out_cap is the case's cap plus 64 for a good frame and the case's cap for a refusal (of
r_out_cap_short and r_eout_then_bits the cap is the refusal).

Positions.  A frame of at most EXHAUSTIVE_MAX bytes is flipped whole.  Of a larger frame a whole decode here, twice on the
emulator's block route and once in the strict reader costs 15 to 130 ms, so the positions are bounded by this rule:
  - the frame header and the checksum field, every byte;
  - of every block the first byte of its header: Last_Block, Block_Type and the low bits of Block_Size - what makes the
    caller's count stale;
  - of the KEPT blocks all that Base.flip_positions takes of a large frame - the header and the BLOCK_HEAD bytes behind it,
    SIDE bytes each side of every section edge - and the block's last SIDE bytes (a sequence bit stream is read from its
    tail: that byte decides underrun); the six substitutions on every FIELDS byte of the frame header and of the kept blocks.
  KEPT is
  - of a frame of at most HEAVY_MIN bytes: blocks 0 and 1 (the one that sets tables and the first that may inherit) and the
    last block the header walk reaches (of r_cut_in_block_17 the one that is cut);
  - of a larger frame: that last block alone - with every block before it good, the refusal there is the latest in stream
    order and every earlier descriptor is decoded in full;
  - of s_between_treeless and s_between_repeat: the first block with sequences behind the first run of Raw, RLE and
    sequence-less blocks - the first that inherits over a gap - the block just before it, and the last block.
The total is derived from the bases and asserted; nothing is sampled."""
import collections
import concurrent.futures
import json
import multiprocessing
import os
import subprocess
import time

import zstd_ref
import zstdd_blocks_sim as B
import zstdd_mutate as M
import zstdd_sim as D

HEAVY_MIN = 6000
NEIGHBOURS = ("n_text_9000_L1", "h_reach_first_byte", "h_repeat_each")      # and tests/golden/zstd_dec/'s ONE_BLOCK
ONE_BLOCK = "a_text_3073_L1"
BASE_STATUSES = (0, D.EDATA, D.EOUT, D.ETRUNC, D.ECKSUM)
SCRATCH_SLICE = 2000


class BlockBase(M.Base):
    def __init__(self, e):
        frame = B.frame_bytes(e)
        M.Base.__init__(self, e["name"], frame, e["cap"], len(frame) <= M.EXHAUSTIVE_MAX)
        self.cap = e["cap"] + 64 if e["sim"][0] == 0 else e["cap"]
        self.nblocks = e["nblocks"]                 # the base's count: the stale hint of its mutants
        self.between = e["group"] == "s"
        self._pos = None

    def blocks(self):
        """[(header's position, end of the block)] by the block headers alone, as far as they lie in the frame"""
        f, n, out = self.frame, len(self.frame), []
        pos = self.sections[0][2]
        while pos + 3 <= n:
            bh = f[pos] | f[pos + 1] << 8 | f[pos + 2] << 16
            end = min(n, pos + 3 + (1 if (bh >> 1) & 3 == 1 else bh >> 3))
            out.append((pos, end))
            if bh & 1 or (bh >> 1) & 3 == 3 or end == n:
                break
            pos = end
        return out

    def kept(self):
        blocks = self.blocks()
        last = len(blocks) - 1
        if self.between:
            with_seq = set(sum(1 for p, _ in blocks if p < a) - 1 for name, a, _ in self.sections if name == "modes")
            gap = next(k for k in range(1, last) if k not in with_seq)
            heir = next(k for k in range(gap, last) if k in with_seq)
            return {heir - 1, heir, last}
        return {last} if len(self.frame) > HEAVY_MIN else {0, 1, last}

    def _positions(self):
        """-> (flip positions, substitution positions)"""
        if self._pos is None:
            n, blocks, kept = len(self.frame), self.blocks(), self.kept()
            starts = [p for p, _ in blocks]
            flips, fields = set(p for p, _ in blocks), set()
            for k in kept:
                flips.update(range(max(blocks[k][0] + 3, blocks[k][1] - M.SIDE), blocks[k][1]))
            for name, a, b in self.sections:
                k = sum(1 for p in starts if p <= a) - 1
                if name in ("frame_header", "checksum"):
                    flips.update(range(a, b))
                elif k not in kept:
                    continue
                elif name == "block_header":
                    flips.update(range(a, min(n, a + 3 + M.BLOCK_HEAD)))
                elif name not in M.OUTSIDE_A_BLOCK:
                    for edge in (a, b):
                        flips.update(range(max(0, edge - M.SIDE), min(n, edge + M.SIDE)))
                if name in M.FIELDS:
                    fields.update(range(a, b))
            self._pos = sorted(flips), sorted(fields)
        return self._pos

    def flip_positions(self):
        return list(range(len(self.frame))) if self.exhaustive else self._positions()[0]

    def field_positions(self):
        return M.Base.field_positions(self) if self.exhaustive else self._positions()[1]


def bases():
    cases = [e for e in B.index()["cases"] if e["sim"][0] in BASE_STATUSES]
    out = [BlockBase(e) for e in cases]
    assert not [b.name for b in out if b.name.startswith("r_count_")] and len(out) == len(B.index()["cases"]) - 3
    return [b for b in out if b.exhaustive] + [b for b in out if not b.exhaustive]


def base_by_name():
    return {b.name: b for b in bases()}


def neighbours():
    """good frames that go between the mutants, multi-block ones and one of one block: [(frame, content, sha256, count)]"""
    by = {e["name"]: e for e in B.index()["cases"]}
    out = [(B.frame_bytes(by[n]), by[n]["cap"], by[n]["sha256"], by[n]["nblocks"]) for n in NEIGHBOURS]
    one = next(e for e in D.index()["frames"] if e["name"] == ONE_BLOCK)
    return out + [(D.frame_bytes(one), one["content"], one["sha256"], 1)]


_BASES = None


def _base(name):
    global _BASES
    if _BASES is None:
        _BASES = base_by_name()
    return _BASES[name]


def _triples(res):
    return [(int(r["status"]), int(r["in_used"]), int(r["out_len"])) for r in res]


def decode_call(call, good, counts, route, scratch_cap=0):
    """one call [(frame, cap, tag)] -> (violations, [(triple, output)], fail_blk, routed); route None: stage E"""
    comp, segs, out_size = D.layout([c[0] for c in call], [c[1] for c in call])
    if route is None:
        rc, res, out, _ = D.decode(comp, segs, out_size)
        info = {"fail_blk": [-1] * len(call), "routed": 0}
    else:
        rc, res, out, info = B.decode(comp, segs, out_size, counts, route, scratch_cap)
    bad = []
    if rc != 0:
        bad.append("guard bytes were written (rc %d) under route %s" % (rc, route))
    got = [(r, out[int(s["out_off"]):int(s["out_off"]) + r[2]]) for s, r in zip(segs, _triples(res))]
    for (m, cap, tag), (r, o) in zip(call, got):
        if tag is None:
            g = next(g for g in good if g[0] is m)
            if r != (0, len(m), g[1]) or M.sha(o) != g[2]:
                bad.append("a good neighbour came out as %r under route %s" % (r, route))
    return bad, got, info["fail_blk"], info["routed"]


def judge(base, m, r, out, with_lib):
    """zstdd_mutate.judge; a refusal's out_cap is its case's cap and the strict reader has none, so EOUT for a frame the
    strict reader accepts is no violation where that frame's content is longer than out_cap"""
    bad, cls, sv = M.judge(base, m, r, out, with_lib)
    if r[0] == D.EOUT and sv == "ok" and len(M.strict(m)[1]) > base.cap:
        bad = [b for b in bad if b != "the decoder refuses (%d) what the strict reader accepts" % D.EOUT]
    return bad, cls, sv


def owes_ehint(m, hint, cap):
    """include/qzamd_zstd_blocks.h: "a frame that takes it with a wrong count answers QZD_ZSTD_EHINT".  The count is wrong by
    the headers alone: behind a frame header that is not refused (a skippable frame has no block), the walk over the block
    headers meets `hint` blocks and none of them is the last, or it ends with another number.  A walk that stops before that
    on a header that is refused or cut leaves the answer to the blocks, which is stage E's.  This is the document's
    sentence written out, independent of Plan's code"""
    n = len(m)
    if n < 4:
        return False
    magic = int.from_bytes(m[:4], "little")
    if magic & 0xfffffff0 == 0x184D2A50:
        return n >= 8 and int.from_bytes(m[4:8], "little") <= n - 8
    if magic != 0xFD2FB528 or n < 5 or m[4] & 0x0b:
        return False
    single, flag = (m[4] >> 5) & 1, m[4] >> 6
    fb = (single, 2, 4, 8)[flag]
    pos = 5 + (0 if single else 1) + fb
    if n < pos or (not single and 10 + (m[5] >> 3) > 31):
        return False
    content = int.from_bytes(m[pos - fb:pos], "little") + (256 if fb == 2 else 0)
    if content > 0xffffffff or (fb and content > cap):
        return False
    window = content if single else (1 << (10 + (m[5] >> 3))) + ((1 << (10 + (m[5] >> 3))) >> 3) * (m[5] & 7)
    for b in range(hint):
        if n - pos < 3:
            return False
        bh = int.from_bytes(m[pos:pos + 3], "little")
        kind, size = (bh >> 1) & 3, bh >> 3
        if kind == 3 or size > min(window, 131072) or n - pos - 3 < (1 if kind == 1 else size):
            return False
        pos += 3 + (1 if kind == 1 else size)
        if bh & 1:
            return b + 1 != hint
    return True


def sweep_slice(job):
    """mutants start .. stop - 1 of one base, in calls between good frames, by stage E and (a), (b), (c) -> (records, violations,
    classes); a record: (base, pos, value, own count, (a)'s triple, (b)'s triple, class or None, sha of an accepted output or
    None, the earliest refused block under (a) or (b) or -1, accepted with other bytes than the base's content)"""
    name, start, stop, with_lib = job
    base, good, G = _base(name), neighbours(), B.group()
    data0 = M.strict(base.frame)[1]
    records, violations, classes = [], [], collections.Counter()
    items = ((base.mutant(p, v), base.cap, (p, v)) for p, v in list(base.recipes())[start:stop])
    for call in M.calls(items, good, G):
        assert call[0][2] is None and call[-1][2] is None and all(c[2] is None for c in call[::G])
        gcount = [next(g[3] for g in good if g[0] is c[0]) if c[2] is None else None for c in call]
        own = [B.walk_count(c[0]) if n is None else n for c, n in zip(call, gcount)]
        stale = [base.nblocks if n is None else n for n in gcount]
        where = "%s: in the call that begins with %r: " % (name, [c[2] for c in call if c[2]][:1])
        badE, gotE, _, _ = decode_call(call, good, None, None)
        badA, gotA, fbA, routedA = decode_call(call, good, own, "blocks")
        badB, gotB, fbB, routedB = decode_call(call, good, stale, "blocks")
        violations += [where + b for b in badE + badA + badB]
        if routedA != sum(1 for n in own if n) or routedB != len(call):
            violations.append(where + "%d and %d frames of %d took the block route" % (routedA, routedB, len(call)))
        gotC = gotA
        if base.exhaustive:
            badC, gotC, _, _ = decode_call(call, good, own, "auto")
            violations += [where + b for b in badC]
        for k, (m, cap, tag) in enumerate(call):
            if tag is None:
                continue
            what = "%s byte %d = 0x%02x: " % (name, tag[0], tag[1])
            (r, o), e, b, c = gotA[k], gotE[k], gotB[k], gotC[k]
            if (r, o) != e:
                violations.append(what + "route blocks with the count %d gives %r, stage E %r%s" % (own[k], r, e[0], " - other bytes" if r == e[0] else ""))
            if c != (r, o):
                violations.append(what + "route auto gives %r, route blocks %r" % (c[0], r))
            if (b[0][0] == B.EHINT) != owes_ehint(m, base.nblocks, cap):
                violations.append(what + "route blocks with the stale count %d gives %r, and EHINT is %s" % (base.nblocks, b[0], "not owed" if b[0][0] == B.EHINT else "owed"))
            if b[0] == (B.EHINT, 0, 0):
                if own[k] == base.nblocks:
                    violations.append(what + "EHINT for the count %d, which is the host walk's" % own[k])
            elif b != e:
                violations.append(what + "route blocks with the stale count %d gives %r, stage E %r" % (base.nblocks, b[0], e[0]))
            if own[k] == base.nblocks and b != (r, o):
                violations.append(what + "the same count %d, but %r and then %r" % (own[k], r, b[0]))
            bad, cls, sv = judge(base, m, r, o, with_lib)
            violations += [what + x for x in bad]
            if cls:
                classes[cls] += 1
            records.append((name, tag[0], tag[1], own[k], r, b[0], cls, M.sha(o) if r[0] == 0 else None, max(fbA[k], fbB[k]), r[0] == 0 and o != data0))
    return records, violations, classes


def run(only=None, with_lib=None, progress=False):
    """the whole sweep on the emulator, as zstdd_mutate.run -> {"total", "expected", "seconds", "violations", "classes",
    "per_base", "with_lib", "records" (sweep_slice has their fields)}"""
    t0 = time.time()
    with_lib = zstd_ref.available() if with_lib is None else with_lib
    D.build_so()
    B.build_so()
    res = {"total": 0, "expected": 0, "violations": [], "classes": collections.Counter(), "per_base": {}, "records": [], "with_lib": with_lib}
    jobs = []
    for base in map(_base, [b.name for b in bases()]):
        if only is not None and base.name not in only:
            continue
        n = base.count()
        res["expected"] += n
        res["per_base"][base.name] = 0
        jobs += [(base.name, a, min(n, a + M.SLICE), with_lib) for a in range(0, n, M.SLICE)]
    workers = min(M.WORKERS, os.cpu_count() or 1)
    pool = multiprocessing.get_context("fork").Pool(workers) if workers > 1 else None
    try:
        for job, (records, violations, classes) in zip(jobs, pool.imap(sweep_slice, jobs) if pool else map(sweep_slice, jobs)):
            res["records"] += records
            res["violations"] += violations
            res["classes"].update(classes)
            res["total"] += len(records)
            res["per_base"][job[0]] += len(records)
            if progress and job[2] == _base(job[0]).count():
                print("%-28s %6d mutants, %4.0f s so far" % (job[0], res["per_base"][job[0]], time.time() - t0), flush=True)
    finally:
        if pool:
            pool.terminate()
    res["seconds"] = time.time() - t0
    return res


def scratch_slice(sweep):
    """the exhaustive bases' first SCRATCH_SLICE mutants under (a) with a scratch cap that holds one frame a round ->
    violations: a guard, a neighbour, or an answer that is not the sweep's"""
    violations, good, G, done = [], neighbours(), B.group(), 0
    records = [r for r in sweep["records"] if _base(r[0]).exhaustive][:SCRATCH_SLICE]
    items = ((_base(r[0]).mutant(r[1], r[2]), _base(r[0]).cap, r) for r in records)
    for call in M.calls(items, good, G):
        counts = [next(g[3] for g in good if g[0] is c[0]) if c[2] is None else c[2][3] for c in call]
        comp, segs, out_size = D.layout([c[0] for c in call], [c[1] for c in call])
        rc, res, out, info = B.decode(comp, segs, out_size, counts, "blocks", scratch_cap=1)
        if rc != 0 or info["rounds"] != len(call):
            violations.append("guard rc %d, %d rounds for %d frames" % (rc, info["rounds"], len(call)))
        for (m, cap, tag), s, r in zip(call, segs, _triples(res)):
            o = out[int(s["out_off"]):int(s["out_off"]) + r[2]]
            if tag is None:
                g = next(g for g in good if g[0] is m)
                if r != (0, len(m), g[1]) or M.sha(o) != g[2]:
                    violations.append("a good neighbour came out as %r" % (r,))
                continue
            done += 1
            if r != tag[4] or (r[0] == 0 and M.sha(o) != tag[7]):
                violations.append("%s byte %d = 0x%02x: %r a frame a round, %r in the sweep" % (tag[0], tag[1], tag[2], r, tag[4]))
    return done, violations


# (200 accepted outputs, each with its SHA: tests/golden/zstd_dec_blocks/ stays under the 300,000 bytes its index test allows)
SAMPLE_PER_KIND, SAMPLE_ACCEPTED_MAX, SAMPLE_LATER_MAX = 8, 200, 500


def gpu_sample(sweep):
    """in sweep order: per base and (status under (a), EHINT or not under (b)) the first SAMPLE_PER_KIND mutants, every routed
    mutant accepted with other bytes than the base's content up to SAMPLE_ACCEPTED_MAX, every mutant whose earliest refused
    block is not block 0 up to SAMPLE_LATER_MAX -> ["base|pos|value|count|status|in_used|out_len|sha or -"]: the mutant with
    its own count and (a)'s answer, and behind it, where the base's count is another, with that count and (b)'s answer"""
    seen, accepted, later, out = collections.Counter(), 0, 0, []
    for name, pos, value, own, r, rb, cls, digest, fb, other in sweep["records"]:
        kind = (name, r[0], rb[0] == B.EHINT)
        take = False
        if seen[kind] < SAMPLE_PER_KIND:
            seen[kind] += 1
            take = True
        if other and own and accepted < SAMPLE_ACCEPTED_MAX:
            accepted += 1
            take = True
        if fb > 0 and later < SAMPLE_LATER_MAX:
            later += 1
            take = True
        if not take:
            continue
        sha = digest or "-"
        out.append("%s|%d|%d|%d|%d|%d|%d|%s" % (name, pos, value, own, r[0], r[1], r[2], sha))
        stale = _base(name).nblocks
        if stale != own:
            out.append("%s|%d|%d|%d|%d|%d|%d|%s" % (name, pos, value, stale, rb[0], rb[1], rb[2], sha if rb[0] == 0 else "-"))
    return out


def parse_sample(lines):
    """-> [(base name, pos, value, count, (status, in_used, out_len), sha or None, own)]; own: the line has the mutant's
    own count - the line behind it with the same mutant has the base's"""
    out = []
    for ln in lines:
        name, pos, value, count, st, used, olen, digest = ln.split("|")
        row = (name, int(pos), int(value))
        own = not out or out[-1][:3] != row
        out.append(row + (int(count), (int(st), int(used), int(olen)), None if digest == "-" else digest, own))
    return out


def sample():
    with open(os.path.join(B.GOLDEN, "corrupt_sample.json")) as f:
        return json.load(f)["sample"]


def sanitizer_run(tmp, lines):
    """tests/sim/sim_zstdd_blocks.cpp as a program of its own (`recipe` mode), built with -fsanitize=address,undefined: every
    line of the sample under route `blocks` with its count, every mutant under route `frame`, each in an allocation of exactly
    its size; the answers must be the sample's.  Nothing is loaded into python."""
    exe = os.path.join(tmp, "sim_zstdd_blocks_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSIM_ZSTDDB_MAIN",
                           "-I", B.SIMDIR, "-Wno-unused-function", "-o", exe, B.SRC])
    by = base_by_name()
    want = collections.OrderedDict()
    for row in parse_sample(lines):
        want.setdefault(row[0], []).append(row)

    def one(arg):
        k, (name, rows), route = arg
        b = by[name]
        rows = [r for r in rows if route == "blocks" or r[6]]
        fbase, frec = os.path.join(tmp, "base%d_%s.zst" % (k, route)), os.path.join(tmp, "recipe%d_%s.txt" % (k, route))
        with open(fbase, "wb") as f:
            f.write(b.frame)
        with open(frec, "w") as f:
            f.write("".join("%d %d %d\n" % r[1:4] for r in rows))
        r = subprocess.run([exe, "recipe", fbase, frec, str(b.cap), route], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and "0 failures" in r.stdout, (name, route, r.stdout[-2000:] + r.stderr[-4000:])
        got = [tuple(int(x) for x in ln.split()) for ln in r.stdout.splitlines() if ln and ln[0].isdigit()]
        assert got == [r[1:4] + r[4] for r in rows], (name, route, [(g, w) for g, w in zip(got, rows) if g[3:] != w[4]][:5])
        return len(rows)

    jobs = [(k, item, route) for k, item in enumerate(want.items()) for route in ("blocks", "frame")]
    with concurrent.futures.ThreadPoolExecutor(min(M.WORKERS, os.cpu_count() or 1)) as ex:
        return sum(ex.map(one, jobs))
