"""Corrupted zstd frames for the decoder's tests (tests/test_sim_zstdd_corrupt.py, tests/test_gpu_zstdd_corrupt.py,
tests/golden/gen_zstd_dec_corrupt.py): which bytes of which committed frame are changed to what, in one fixed order, and
how mutants are put into calls between good frames.  Nothing here is random and no mutant is stored: a mutant is
(base name, position, value)."""
import collections
import hashlib
import json
import multiprocessing
import os
import re
import subprocess
import time

import zstd_format
import zstd_full_format as ZF
import zstd_ref
import zstdd_sim as D

HAND = os.path.join(D.HERE, "golden", "zstd_dec_corrupt")
EXHAUSTIVE_MAX = 1536               # committed frames of groups a, b, c up to this size are flipped whole
LARGE = ("c_edge_fibonacci", "a_text_70001_L3_cs", "a_text_300000_L19_cs")
BLOCK_HEAD, SIDE = 64, 16           # of a larger frame: the first bytes of every block, the bytes each side of a boundary
SUBSTITUTES = 6                     # 0x00, 0xFF, 0x7F, 0x80, v + 1, v - 1
FIELDS = ("frame_header", "block_header", "literals_header", "tree_header", "tree_weights", "jump_table", "sequence_count",
          "modes", "ll_description", "of_description", "ml_description", "ll_rle_code", "of_rle_code", "ml_rle_code")
OUTSIDE_A_BLOCK = ("frame_header", "block_header", "raw_block", "rle_block", "checksum", "skippable_data")
STATUSES = (D.EDATA, D.EOUT, D.ETRUNC, D.ECKSUM, D.EUNSUP)
NEIGHBOURS = ("a_text_3073_L1", "c_edge_two", "c_window_fcs", "c_edge_rle", "b_records_70001_mm3_c1")
CALL_SEGMENTS, CALL_BYTES = 512, 24 << 20
GROUP = 4                           # QZK_ZD_G, the frames a wave of stage E takes (the emulator test holds it against the build)


def hand_index():
    with open(os.path.join(HAND, "index.json")) as f:
        return json.load(f)


def hand_bytes(entry):
    with open(os.path.join(HAND, entry["file"]), "rb") as f:
        return f.read()


class Base:
    def __init__(self, name, frame, content, exhaustive):
        self.name, self.frame, self.content, self.exhaustive = name, frame, content, exhaustive
        self.cap = content + 64
        self._sections = None

    @property
    def sections(self):
        """the strict reader's (name, start, end) - of a refused frame, what it read before it refused"""
        if self._sections is None:
            try:
                self._sections = ZF.decode_frame(self.frame)[0]["sections"]
            except zstd_format.FormatError as e:
                self._sections = getattr(e, "sections", [])
        return self._sections

    def flip_positions(self):
        n = len(self.frame)
        if self.exhaustive:
            return list(range(n))
        keep = set()
        for name, a, b in self.sections:
            if name == "frame_header":
                keep.update(range(a, b))
            elif name == "block_header":
                keep.update(range(a, min(n, a + 3 + BLOCK_HEAD)))
            elif name not in OUTSIDE_A_BLOCK:
                for edge in (a, b):
                    keep.update(range(max(0, edge - SIDE), min(n, edge + SIDE)))
        return sorted(keep)

    def field_positions(self):
        return sorted(set(p for name, a, b in self.sections if name in FIELDS for p in range(a, b)))

    def count(self):
        return 8 * len(self.flip_positions()) + SUBSTITUTES * len(self.field_positions())

    def recipes(self):
        """(position, value) of every mutant, in sweep order: the flips by position and bit, then the substitutions"""
        f = self.frame
        for p in self.flip_positions():
            for bit in range(8):
                yield p, f[p] ^ (1 << bit)
        for p in self.field_positions():
            for v in (0x00, 0xFF, 0x7F, 0x80, (f[p] + 1) & 255, (f[p] - 1) & 255):
                yield p, v

    def mutant(self, pos, value):
        m = bytearray(self.frame)
        m[pos] = value
        return bytes(m)


def bases():
    """the hand-built frames, every committed frame of groups a, b, c up to EXHAUSTIVE_MAX bytes, and LARGE"""
    out = [Base("hand:" + e["name"], hand_bytes(e), e["content"], True) for e in hand_index()["frames"]]
    for e in D.index()["frames"]:
        if e["group"] in "abc" and e["size"] <= EXHAUSTIVE_MAX:
            out.append(Base(e["name"], D.frame_bytes(e), e["content"], True))
        elif e["name"] in LARGE:
            out.append(Base(e["name"], D.frame_bytes(e), e["content"], False))
    assert len([b for b in out if not b.exhaustive]) == len(LARGE)
    return out


def base_by_name():
    return {b.name: b for b in bases()}


def neighbours():
    """good committed frames that go between the mutants: [(frame, content, sha256)]"""
    by = {e["name"]: e for e in D.index()["frames"]}
    return [(D.frame_bytes(by[n]), by[n]["content"], by[n]["sha256"]) for n in NEIGHBOURS]


def calls(items, good, group, extra_front=None):
    """items: (frame, cap, tag) one after the other -> calls of at most CALL_SEGMENTS segments and CALL_BYTES of out_cap, each
    a list of (frame, cap, tag) with a good frame (tag None) at the front, at the back and at every multiple of `group`;
    extra_front: one more good frame for the front of the first call"""
    cur, size, k, first = [], 0, 0, True

    def neighbour():
        nonlocal k
        g = good[k % len(good)]
        k += 1
        return (g[0], g[1], None)

    def close():
        if len(cur) % group == 0 or cur[-1][2] is not None:
            cur.append(neighbour())
        return cur

    for it in items:
        if cur and (len(cur) + 3 > CALL_SEGMENTS or size + it[1] > CALL_BYTES):
            yield close()
            cur, size = [], 0
        if first and extra_front is not None:
            cur.append((extra_front[0], extra_front[1], None))
            size += extra_front[1]
            while len(cur) % group:
                cur.append(neighbour())
        first = False
        if len(cur) % group == 0:
            cur.append(neighbour())
        cur.append(it)
        size += it[1]
    if cur:
        yield close()


def strict(frame):
    """the strict reader's answer: ("ok", data, end) or (its message, None, 0)"""
    try:
        info, end = ZF.decode_frame(frame)
        return "ok", info["data"], end
    except zstd_format.FormatError as e:
        return str(e), None, 0


def klass(message):
    """a class of strictness: the strict reader's message with its numbers removed"""
    return re.sub(r"\d+", "N", message)


def sha(b):
    return hashlib.sha256(b).hexdigest()


def libzstd(frame, cap):
    """ZSTD_decompress's answer: ("ok", data) or (its error's name, None)"""
    try:
        return "ok", zstd_ref.decompress(frame, cap)
    except ValueError as e:
        return str(e).split(": ", 1)[1], None


def judge(base, m, r, out, with_lib):
    """one mutant's decode against rules 2 and 3 -> ([violations], class of rule 4 or None, the strict reader's verdict)"""
    st, used, olen = r
    sv, sdata, send = strict(m)
    bad, cls = [], None
    if st == 0:
        if sv != "ok":
            bad.append("the decoder accepts what the strict reader refuses (%s)" % sv)
        elif (used, olen) != (send, len(sdata)) or out != sdata:
            bad.append("accepted with other bytes than the strict reader's: %r against (%d, %d)" % (r, send, len(sdata)))
        if with_lib:
            lv, ldata = libzstd(m[:used], base.cap)         # the frame as the decoder took it: in_used bytes
            if lv != "ok":
                bad.append("the decoder accepts what libzstd refuses (%s)" % lv)
            elif ldata != out:
                bad.append("accepted with other bytes than libzstd's")
    else:
        if sv == "ok":
            bad.append("the decoder refuses (%d) what the strict reader accepts" % st)
        if st not in STATUSES:
            bad.append("status %d is not documented" % st)
        # include/qzamd_device.h: in_used / out_len of a failed frame are 0 - of a checksum mismatch they are the frame's
        if st == D.ECKSUM:
            if sv != "content checksum mismatch" or not (0 < used <= len(m) and olen <= base.cap):
                bad.append("a checksum refusal with %r, the strict reader: %s" % (r, sv))
        elif (used, olen) != (0, 0):
            bad.append("a refusal with in_used %d, out_len %d" % (used, olen))
        if with_lib and libzstd(m, base.cap)[0] == "ok":
            cls = klass(sv)
    return bad, cls, sv


SLICE, WORKERS = 384, 8              # mutants per job of the sweep; processes at most (the emulator and both readers are serial code)
_BASES = None


def _base(name):
    global _BASES
    if _BASES is None:
        _BASES = base_by_name()
    return _BASES[name]


def sweep_slice(job):
    """mutants start .. stop - 1 of one base, in calls between good frames -> (records, violations, classes)"""
    name, start, stop, with_lib = job
    base, good, G = _base(name), neighbours(), D.group()
    assert G == GROUP
    data0 = strict(base.frame)[1]
    records, violations, classes = [], [], collections.Counter()
    items = ((base.mutant(p, v), base.cap, (p, v)) for p, v in list(base.recipes())[start:stop])
    for call in calls(items, good, G):
        comp, segs, out_size = D.layout([c[0] for c in call], [c[1] for c in call])
        rc, rs, out, _ = D.decode(comp, segs, out_size)
        if rc != 0:
            violations.append("%s: guard bytes were written (rc %d) in the call that begins with %r" % (name, rc, [c[2] for c in call if c[2]][:1]))
        assert call[0][2] is None and call[-1][2] is None and all(c[2] is None for c in call[::G])
        for (m, cap, tag), s, r in zip(call, segs, rs):
            r = (int(r["status"]), int(r["in_used"]), int(r["out_len"]))
            o = out[int(s["out_off"]):int(s["out_off"]) + r[2]]
            if tag is None:
                g = next(g for g in good if g[0] is m)
                if r != (0, len(m), g[1]) or sha(o) != g[2]:
                    violations.append("%s: a good neighbour came out as %r" % (name, r))
                continue
            bad, cls, sv = judge(base, m, r, o, with_lib)
            violations += ["%s byte %d = 0x%02x: %s" % (name, tag[0], tag[1], b) for b in bad]
            if cls:
                classes[cls] += 1
            records.append((name, tag[0], tag[1], r, cls, sha(o) if r[0] == 0 and o != data0 else None))
    return records, violations, classes


def run(only=None, with_lib=None, progress=False):
    """the whole sweep on the emulator, in jobs of SLICE mutants over up to WORKERS processes; the order of what comes back
    is the sweep's -> {"total", "expected", "seconds", "violations": [text], "classes": {class: count}, "per_base": {name:
    count}, "with_lib", "records": [(base, pos, value, (status, in_used, out_len), class or None, sha of an accepted output
    that is not the base's content or None)]}"""
    t0 = time.time()
    with_lib = zstd_ref.available() if with_lib is None else with_lib
    D.build_so()
    res = {"total": 0, "expected": 0, "violations": [], "classes": collections.Counter(), "per_base": {}, "records": [], "with_lib": with_lib}
    jobs = []
    for name, base in ((b.name, b) for b in map(_base, [b.name for b in bases()])):
        if only is not None and name not in only:
            continue
        n = base.count()
        res["expected"] += n
        res["per_base"][name] = 0
        jobs += [(name, a, min(n, a + SLICE), with_lib) for a in range(0, n, SLICE)]
    workers = min(WORKERS, os.cpu_count() or 1)
    pool = multiprocessing.get_context("fork").Pool(workers) if workers > 1 else None
    try:
        for job, (records, violations, classes) in zip(jobs, pool.imap(sweep_slice, jobs) if pool else map(sweep_slice, jobs)):
            res["records"] += records
            res["violations"] += violations
            res["classes"].update(classes)
            res["total"] += len(records)
            res["per_base"][job[0]] += len(records)
            if progress and job[2] == _base(job[0]).count():
                print("%-40s %6d mutants, %4.0f s so far" % (job[0], res["per_base"][job[0]], time.time() - t0), flush=True)
    finally:
        if pool:
            pool.terminate()
    res["seconds"] = time.time() - t0
    return res


SAMPLE_PER_CLASS, SAMPLE_ACCEPTED_MAX = 8, 2000


def gpu_sample(sweep):
    """per base and class of rule 4 the first SAMPLE_PER_CLASS mutants in sweep order, and every mutant the decoder accepts
    with other bytes than the base's content, up to SAMPLE_ACCEPTED_MAX -> ["base|pos|value|status|in_used|out_len|sha or -"]"""
    seen, taken, out = collections.Counter(), 0, []
    for name, pos, value, r, cls, digest in sweep["records"]:
        if digest is not None and taken < SAMPLE_ACCEPTED_MAX:
            taken += 1
        elif cls is not None and seen[(name, cls)] < SAMPLE_PER_CLASS:
            seen[(name, cls)] += 1
            digest = None
        else:
            continue
        out.append("%s|%d|%d|%d|%d|%d|%s" % (name, pos, value, r[0], r[1], r[2], digest or "-"))
    return out


def parse_sample(lines):
    """-> [(base name, pos, value, (status, in_used, out_len), sha or None)]"""
    out = []
    for ln in lines:
        name, pos, value, st, used, olen, digest = ln.split("|")
        out.append((name, int(pos), int(value), (int(st), int(used), int(olen)), None if digest == "-" else digest))
    return out


def sanitizer_run(tmp, sample):
    """tests/sim/sim_zstdd.cpp as a program of its own, built with -fsanitize=address,undefined: every hand-built frame as it is
    and every mutant of the sample, each in an allocation of exactly its size; the answers must be the sample's.  Nothing is
    loaded into python."""
    exe = os.path.join(tmp, "sim_zstdd_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DSIM_ZSTDD_MAIN", "-I", D.SIMDIR, "-Wno-unused-function", "-o", exe, os.path.join(D.SIMDIR, "sim_zstdd.cpp")])
    by = base_by_name()
    want = collections.OrderedDict()
    for e in hand_index()["frames"]:
        b = by["hand:" + e["name"]]
        want.setdefault(b.name, []).append((0, b.frame[0], tuple(e["sim"])))
    for name, pos, value, r, _ in parse_sample(sample):
        want.setdefault(name, []).append((pos, value, r))
    ran = 0
    for k, (name, rows) in enumerate(want.items()):
        b = by[name]
        fbase, frec = os.path.join(tmp, "base%d.zst" % k), os.path.join(tmp, "recipe%d.txt" % k)
        with open(fbase, "wb") as f:
            f.write(b.frame)
        with open(frec, "w") as f:
            f.write("".join("%d %d\n" % (p, v) for p, v, _ in rows))
        r = subprocess.run([exe, "recipe", fbase, frec, str(b.cap)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "0 failures" in r.stdout, (name, r.stdout[-2000:] + r.stderr[-4000:])
        got = [tuple(int(x) for x in ln.split()) for ln in r.stdout.splitlines() if ln and ln[0].isdigit()]
        assert got == [(p, v) + tuple(rr) for p, v, rr in rows], (name, [(g, w) for g, w in zip(got, rows) if g[2:] != tuple(w[2])][:5])
        ran += len(rows)
    return ran
