#!/usr/bin/env python3
"""Writes tests/golden/zstd_dec_blocks/: multi-block frames for the block route of the zstd decoder
(qatzip_amd/csrc/qzk_zstdd_blocks.h), and index.json - per case the frame's file, the out_cap and the block count the decoder
is given, the pinned {status, in_used, out_len}, the output's SHA-256, the strict reader's verdict
(tests/zstd_full_format.py) and libzstd's.  Run where libzstd loads; the frames are committed because a GPU box may have
none.  A Window_Descriptor of 1 KB makes the block maximum 1 KB, so 40 KB of input are 40 blocks.

    (n) libzstd's own frames with ZSTD_c_windowLog 10: natural Repeat_Mode and Treeless chains
    (s) a frame of (n) with Raw, RLE, empty and sequence-less blocks put between a block that defines a Huffman tree or a
        sequence table and the block that uses it
    (h) hand-built blocks (raw literals; RLE_Mode, Predefined and Repeat_Mode tables): every form a repeat offset takes at a
        block's first sequence, deltas that add up over blocks, each table repeated on its own, no trailing literals
    (r) refusals, and frames given with a wrong block count

Every case is decoded on the emulator under route `blocks` and under route `frame`; the two must agree, and with the strict
reader.  A refusal libzstd accepts is kept only under "libzstd_accepts" with the reason.
"""
import ctypes as C
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import zstd_format as fmt  # noqa: E402
import zstd_full_format as zf  # noqa: E402
import zstd_ref  # noqa: E402
import zstd_sim  # noqa: E402

OUT = os.path.join(HERE, "zstd_dec_blocks")
MAGIC = bytes.fromhex("28b52ffd")


# ---------------------------------------------------------------- writing frames and blocks by hand
def frame(blocks, content=None, checksum=None, window_byte=0x00):
    """blocks: [(type, payload, size)] -> a frame behind a Window_Descriptor (1 KB by default).  content: a 4-byte
    Frame_Content_Size; checksum: the four bytes to append (Content_Checksum_Flag set)"""
    fhd = (0x80 if content is not None else 0) | (0x04 if checksum is not None else 0)
    out = bytearray(MAGIC) + bytes([fhd, window_byte])
    if content is not None:
        out += content.to_bytes(4, "little")
    for i, (btype, payload, size) in enumerate(blocks):
        last = 1 if i == len(blocks) - 1 else 0
        out += (size << 3 | btype << 1 | last).to_bytes(3, "little") + payload
    if checksum is not None:
        out += checksum
    return bytes(out)


def raw(data):
    return (0, bytes(data), len(data))


def rle(byte, n):
    return (1, bytes([byte]), n)


def back_bits(fields):
    """[(value, bits)] in the order the decoder reads them -> the stream, read from its end, with its end mark"""
    acc, pos = 0, 0
    for v, nb in reversed(fields):
        assert 0 <= v < (1 << nb) or nb == 0 and v == 0
        acc |= v << pos
        pos += nb
    acc |= 1 << pos
    return acc.to_bytes(pos // 8 + 1, "little")


TABLES = {"ll": (fmt.LL_TABLE, 6), "of": (fmt.OF_TABLE, 5), "ml": (fmt.ML_TABLE, 6)}


def _states(table, codes):
    """the states an FSE decoder passes through when it yields `codes`: the last one is any state of its symbol, and each
    earlier one the state of its symbol whose range holds the next"""
    st = [None] * len(codes)
    st[-1] = next(u for u, e in enumerate(table) if e[0] == codes[-1])
    for i in range(len(codes) - 2, -1, -1):
        st[i] = next(u for u, (s, nb, base) in enumerate(table) if s == codes[i] and base <= st[i + 1] < base + (1 << nb))
    return st


def compressed(lits, seqs, ll=("rle",), of=("rle",), ml=("rle",), nseq=None, drop_bits=0):
    """a Compressed block: raw literals, then seqs = [(literal length, match length, offset value)].  Per table ("rle",): RLE_Mode -
    every sequence of the block has the same code -, ("predefined",), or ("repeat", "rle" | "predefined"): Repeat_Mode of a table
    of that kind.  nseq: the count the header claims; drop_bits: that many fields fewer at the stream's low end (what the
    decoder reads last)."""
    n = len(lits)
    assert n < 4096
    body = bytearray(((n << 4) | 0x04).to_bytes(2, "little")) + bytes(lits)     # Raw_Literals_Block, 12-bit size
    count = len(seqs) if nseq is None else nseq
    assert count < 128
    body.append(count)
    if not count:
        return (2, bytes(body), len(body))
    lcodes = [fmt.ll_code(s[0]) for s in seqs]
    mcodes = [fmt.ml_code(s[1]) for s in seqs]
    ocodes = [s[2].bit_length() - 1 for s in seqs]
    modes, descr, kinds = 0, bytearray(), []
    for k, (spec, codes) in enumerate(((ll, lcodes), (of, ocodes), (ml, mcodes))):
        mode = {"predefined": 0, "rle": 1, "repeat": 3}[spec[0]]
        modes |= mode << (6 - 2 * k)
        kind = spec[1] if spec[0] == "repeat" else spec[0]
        kinds.append(kind)
        if kind == "rle":
            assert len(set(codes)) == 1, "an RLE table has one code"
            if spec[0] == "rle":
                descr.append(codes[0])
    body.append(modes)
    body += descr
    fields = []
    sts = []
    for k, (name, codes) in enumerate((("ll", lcodes), ("of", ocodes), ("ml", mcodes))):
        sts.append(_states(TABLES[name][0], codes) if kinds[k] == "predefined" else None)
    for k, name in enumerate(("ll", "of", "ml")):                   # the initial states: LL, OF, ML
        if sts[k]:
            fields.append((sts[k][0], TABLES[name][1]))
    for i, (l, m, ov) in enumerate(seqs):
        fields.append((ov - (1 << ocodes[i]), ocodes[i]))
        fields.append((m - fmt.ML_BASE[mcodes[i]], fmt.ML_BITS[mcodes[i]]))
        fields.append((l - fmt.LL_BASE[lcodes[i]], fmt.LL_BITS[lcodes[i]]))
        if i + 1 < len(seqs):
            for k, name in ((0, "ll"), (2, "ml"), (1, "of")):      # the updates: LL, ML, OF
                if sts[k]:
                    s, nb, base = TABLES[name][0][sts[k][i]]
                    fields.append((sts[k][i + 1] - base, nb))
    if drop_bits:
        fields = fields[:-drop_bits]
    body += back_bits(fields)
    return (2, bytes(body), len(body))


def replay(blocks):
    """what the hand-built blocks decode to, by the strict reader"""
    return zf.decode_frame(frame(blocks))[0]["data"]


def walk_blocks(fr):
    """[{off, type, size, last, lit (literals type of a Compressed block), nseq, modes}] from the headers"""
    h = zf.frame_header(fr)
    pos, out = h["header_size"], []
    while True:
        bh = int.from_bytes(fr[pos:pos + 3], "little")
        b = {"off": pos, "type": (bh >> 1) & 3, "size": bh >> 3, "last": bh & 1}
        body = fr[pos + 3:pos + 3 + (1 if b["type"] == 1 else b["size"])]
        if b["type"] == 2:
            t, f = body[0] & 3, (body[0] >> 2) & 3
            if t < 2:
                hs = 1 if not f & 1 else 2 if f == 1 else 3
                n = int.from_bytes(body[:hs], "little") >> (3 if hs == 1 else 4)
                lend = hs + (n if t == 0 else 1)
            else:
                hs, bits = (3, 10) if f < 2 else (4, 14) if f == 2 else (5, 18)
                lend = hs + (int.from_bytes(body[:hs], "little") >> (4 + bits))
            q = body[lend:]
            if q[0] < 128:
                nseq, qp = q[0], 1
            elif q[0] < 255:
                nseq, qp = ((q[0] - 128) << 8) + q[1], 2
            else:
                nseq, qp = q[1] + (q[2] << 8) + 0x7f00, 3
            b.update(lit=t, nseq=nseq, modes=q[qp] if nseq else 0)
        b["raw"] = (b["type"], bytes(body), b["size"])
        out.append(b)
        pos += 3 + len(body)
        if b["last"]:
            return out


def stitched(frames, window_byte=0x38):
    """frames of this project's writer, one per chunk, none of which uses a repeat offset (the writer's default): their blocks
    as ONE frame behind a Window_Descriptor (128 KB by default) and a 4-byte Frame_Content_Size - a many-block frame where
    libzstd does not load"""
    blocks, total = [], 0
    for fr in frames:
        total += zf.frame_header(fr)["content_size"]
        blocks += [b["raw"] for b in walk_blocks(fr)]
    return frame(blocks, content=total, window_byte=window_byte)


class _Buf(C.Structure):
    _fields_ = [("p", C.c_void_p), ("size", C.c_size_t), ("pos", C.c_size_t)]


def libzstd_frame(src, level, checksum, window_log=10):
    L = zstd_ref.lib()
    L.ZSTD_createCCtx.restype = C.c_void_p
    L.ZSTD_freeCCtx.argtypes = [C.c_void_p]
    L.ZSTD_CCtx_setParameter.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.ZSTD_CCtx_setParameter.restype = C.c_size_t
    L.ZSTD_compress2.restype = C.c_size_t
    L.ZSTD_compress2.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
    cctx = L.ZSTD_createCCtx()
    try:
        assert not L.ZSTD_isError(L.ZSTD_CCtx_setParameter(cctx, 100, level))       # ZSTD_c_compressionLevel
        assert not L.ZSTD_isError(L.ZSTD_CCtx_setParameter(cctx, 101, window_log))  # ZSTD_c_windowLog
        assert not L.ZSTD_isError(L.ZSTD_CCtx_setParameter(cctx, 201, checksum))    # ZSTD_c_checksumFlag
        cap = L.ZSTD_compressBound(len(src)) + 64
        dst = C.create_string_buffer(cap)
        r = L.ZSTD_compress2(cctx, dst, cap, bytes(src), len(src))
        assert not L.ZSTD_isError(r)
        return dst.raw[:r]
    finally:
        L.ZSTD_freeCCtx(cctx)


def verdict(fr, cap):
    try:
        zstd_ref.decompress(fr, cap)
        return "ok"
    except ValueError as e:
        return str(e).split(": ", 1)[1]


def reader(fr):
    """-> ("ok", data, blocks) or (the strict reader's message, None, None)"""
    try:
        info, end = zf.decode_frame(fr)
        assert end == len(fr)
        return "ok", info["data"], info["blocks"]
    except fmt.FormatError as e:
        return str(e), None, None


def random_chain(rng, nblocks, text):
    """a frame's blocks behind a Raw block of 40 bytes: Compressed blocks of two sequences whose LL / OF / ML modes are drawn
    from Predefined, RLE_Mode and - once a table is set - Repeat_Mode, with now and then a Raw, an RLE or a sequence-less
    block among them: the chains in which a table is inherited over blocks that set, repeat or put back the others"""
    blocks = [raw(text[:40])]
    kind = [None, None, None]                                       # per table: what a Repeat would repeat
    code = [None, None, None]                                       # ... and the value an RLE table stands for
    at = 40
    while len(blocks) < nblocks:
        c = int(rng.integers(0, 10))
        if c == 0:
            blocks.append(raw(text[at:at + 5]))
        elif c == 1:
            blocks.append(rle(0x61 + len(blocks) % 20, 4))
        elif c == 2:
            blocks.append(compressed(text[at:at + 6], []))
        else:
            spec, vals = [], []
            for k in range(3):
                m = ("predefined", "rle", "repeat")[int(rng.integers(0, 3 if kind[k] else 2))]
                if m == "repeat":
                    spec.append(("repeat", kind[k]))
                else:
                    spec.append((m,))
                    kind[k] = m
                    if m == "rle":
                        code[k] = (int(rng.integers(1, 6)), int(rng.integers(8, 12)), int(rng.integers(3, 9)))[k]
                if kind[k] == "rle":
                    vals.append([code[k], code[k] if k != 1 else 8 + (code[k] + 1) % 4])     # (an OF code is three more bits)
                else:
                    vals.append([(int(rng.integers(0, 6)), int(rng.integers(4, 14)), int(rng.integers(3, 12)))[k] for _ in range(2)])
            seqs = [(vals[0][i], vals[2][i], vals[1][i]) for i in range(2)]
            blocks.append(compressed(text[at:at + 12], seqs, ll=spec[0], of=spec[1], ml=spec[2]))
        at = 40 + (at + 13) % 500
    return blocks


def predefined_put_back(k, text):
    """block A sets the three tables in RLE_Mode; block B puts table k back to Predefined and repeats the other two - it
    defines nothing that block C inherits from a block -; block C repeats all three: table k of B, the others of A"""
    rep = ("repeat", "rle")
    a = compressed(text[40:60], [(3, 4, 8), (3, 4, 9)])
    spec = [rep, rep, rep]
    spec[k] = ("predefined",)
    seqs = [[3, 4, 8], [3, 4, 9]]
    seqs[0][(0, 2, 1)[k]] = (2, 21, 5)[k]                          # a value only the predefined table of k can give
    b = compressed(text[60:80], [tuple(q) for q in seqs], ll=spec[0], of=spec[1], ml=spec[2])
    spec[k] = ("repeat", "predefined")
    seqs[1][(0, 2, 1)[k]] = (5, 30, 6)[k]
    c = compressed(text[80:100], [tuple(q) for q in seqs], ll=spec[0], of=spec[1], ml=spec[2])
    return [raw(text[:40]), a, b, raw(b"--"), c, raw(b"z")]


HISTORY = [(10, 4, 5 + 3), (5, 3, 7 + 3), (3, 5, 9 + 3)]                # leaves the repeat offsets 9, 7, 5


def hand_cases():
    """-> [(name, blocks, what)] of frames that decode"""
    text = zstd_sim.make_input("text", 600, 4)
    first = compressed(text[:40], HISTORY, of=("rle",), ll=("predefined",), ml=("predefined",))
    cases = []
    for ov in (1, 2, 3):
        for l in (0, 6):
            # the block's first sequence takes its distance from the history that crosses the boundary; the second one
            # uses what the first left behind
            blk = compressed(text[100:100 + l + 9], [(l, 4, ov), (l and 2, 3, ov)], ll=("predefined",), ml=("predefined",))
            tail = compressed(text[200:205], [(2, 3, 1)])
            cases.append(("h_rep%d_%s" % (ov, "ll0" if l == 0 else "ll6"), [first, blk, tail, raw(b"end")],
                          "offset value %d with literal length %d as a block's first sequence, behind the history 9, 7, 5" % (ov, l)))
    # rep0 - 1 block after block: 9 -> 8 -> 7 -> 6, a Raw block and an empty one in between
    minus = compressed(b"", [(0, 3, 3)])
    cases.append(("h_minus_chain", [first, minus, minus, raw(b""), rle(0x41, 7), minus, compressed(b"xy", [(1, 4, 1)]), raw(b"z")],
                  "three blocks that only apply rep0 - 1, a Raw, an empty and an RLE block among them: the deltas add up to 3"))
    # each table repeated on its own, of an RLE table and of a predefined one
    b0 = compressed(text[:30], [(6, 5, 8), (3, 6, 9)], ll=("predefined",), of=("predefined",), ml=("predefined",))
    b1 = compressed(text[30:50], [(2, 4, 8), (2, 4, 9)], ll=("repeat", "predefined"), of=("rle",), ml=("rle",))
    b2 = compressed(text[50:70], [(3, 4, 10), (3, 7, 11)], ll=("rle",), of=("repeat", "rle"), ml=("predefined",))
    b3 = compressed(text[70:90], [(3, 5, 2), (3, 9, 1)], ll=("repeat", "rle"), of=("predefined",), ml=("repeat", "predefined"))
    b4 = compressed(text[90:120], [(5, 6, 12), (5, 6, 20)], ll=("rle",), of=("repeat", "predefined"), ml=("rle",))
    b5 = compressed(text[120:140], [(1, 6, 4), (2, 6, 4)], ll=("predefined",), of=("rle",), ml=("repeat", "rle"))
    b6 = compressed(text[140:160], [(1, 6, 5), (1, 6, 6)], ll=("repeat", "predefined"), of=("repeat", "rle"), ml=("repeat", "rle"))
    cases.append(("h_repeat_each", [b0, b1, raw(b"--"), b2, b3, rle(0x2e, 5), b4, compressed(b"lits only", []), b5, raw(b""), b6],
                  "Repeat_Mode for LL, OF and ML on their own, of an RLE table and of a predefined one, Raw, RLE, empty and "
                  "sequence-less blocks between the definition and its use (every block that sets a predefined table here also "
                  "sets another table its user inherits, or its user inherits nothing else: h_predefined_put_back_* are the other case)"))
    # a table put back to Predefined by a block that defines nothing else the user inherits, the user's other tables from a
    # still earlier block: the pass over that earlier block must not leave ITS table in the place of the predefined one
    for k, name in enumerate(("ll", "of", "ml")):
        cases.append(("h_predefined_put_back_%s" % name, predefined_put_back(k, text),
                      "%s set in RLE_Mode with the others, put back to Predefined by a block that repeats the others, then all three repeated" % name.upper()))
    # no trailing literals: the sequences take every literal - in the middle and as the frame's last block
    full = compressed(text[300:310], [(4, 5, 6), (6, 3, 1)], ll=("predefined",), of=("predefined",), ml=("predefined",))
    cases.append(("h_no_trailing", [raw(text[:16]), full, full, compressed(text[320:324], [(4, 8, 24)])],
                  "blocks whose sequences take all their literals: the blocks' last records are no-ops"))
    # a distance that reaches the frame's first byte from the third block: only the position in the frame allows it
    cases.append(("h_reach_first_byte", [raw(text[:10]), rle(0x30, 6), compressed(text[20:24], [(4, 30, 20 + 3)])],
                  "distance 20 at position 16 + 4 of the frame: allowed by the frame's position, not by the block's"))
    # 70 small blocks in a frame: more than a wave of Fix, and a count that is no multiple of the group
    many = [first] + [compressed(text[i:i + 3], [(1, 3, 1 if i % 3 else 2)]) if i % 5 else raw(text[i:i + 7]) for i in range(1, 70)]
    cases.append(("h_70_blocks", many, "70 blocks of a few bytes each"))
    return cases


def main():
    assert zstd_ref.available(), "libzstd is needed to generate"
    import zstdd_blocks_sim as B
    import zstdd_sim as D
    os.makedirs(OUT, exist_ok=True)
    for f in os.listdir(OUT):
        os.remove(os.path.join(OUT, f))
    cases, accepted = [], []
    files = {}

    def add(name, group, fr, what, cap=None, nblocks=None, want=None, file_of=None):
        """one case: the frame (or the committed file of another case), the cap and the count the decoder gets"""
        msg, data, blocks = reader(fr)
        if cap is None:
            assert data is not None, (name, msg)
            cap = len(data)
        if nblocks is None:
            nblocks = B.walk_count(fr)
            assert nblocks, name
        fname = file_of or name + ".zst"
        if fname not in files:
            files[fname] = fr
            with open(os.path.join(OUT, fname), "wb") as f:
                f.write(fr)
        assert files[fname] == fr
        info = {}
        rb, ob = B.decode_frames([fr], [cap], nblocks=[nblocks], route="blocks", gap=32, info=info)
        ra, oa = D.decode_frames([fr], [cap], gap=32)
        assert info["routed"] == 1, name
        e = {"name": name, "group": group, "file": fname, "size": len(fr), "what": what, "cap": cap, "nblocks": nblocks,
             "sim": list(rb[0]), "reader": msg, "libzstd": verdict(fr, cap)}
        if rb[0][0] == B.EHINT:
            assert want == B.EHINT, (name, rb)
        else:
            assert rb == ra and ob == oa, (name, rb, ra)                # the two routes
            assert want is None or rb[0][0] == want, (name, rb, want)
            if rb[0][0] == 0:
                assert msg == "ok" and ob[0] == data and rb[0] == (0, len(fr), len(data)), (name, rb, msg)
                assert e["libzstd"] == "ok" and zstd_ref.decompress(fr, cap) == data, name
                e.update(sha256=hashlib.sha256(data).hexdigest(), blocks=blocks, tally=zf.decode_frame(fr)[0]["tally"])
            elif rb[0][0] in (D.EDATA, D.ETRUNC, D.ECKSUM):
                assert msg != "ok", (name, rb)                         # (EOUT is about cap, which the reader does not know)
                if e["libzstd"] == "ok":
                    accepted.append(name)
            else:
                assert e["libzstd"] != "ok", name
        cases.append(e)
        return e

    # ---- (n)
    nat = {}
    for kind, n, level, checksum in (("text", 40000, 3, 1), ("records", 40000, 19, 0), ("silesia", 70001, 3, 0), ("lzmix", 30000, 19, 1),
                                     ("text", 9000, 1, 0), ("rand", 5000, 1, 0)):
        src = zstd_sim.make_input(kind, n, 11)
        fr = libzstd_frame(src, level, checksum)
        name = "n_%s_%d_L%d%s" % (kind, n, level, "_cs" if checksum else "")
        e = add(name, "n", fr, "ZSTD_compress2, windowLog 10, level %d, checksum %d over zstd_sim.make_input(%r, %d, 11)" % (level, checksum, kind, n))
        assert zf.decode_frame(fr)[0]["data"] == src and e["blocks"] >= n // 1024
        nat[name] = fr
    union = set(t for e in cases for t in e["tally"])
    for t in ["lit:treeless", "block:raw"] + ["%s:%s" % (a, m) for a in ("ll", "of", "ml") for m in ("predefined", "fse", "repeat")]:
        assert t in union, t
    assert any(e["blocks"] > 64 and e["blocks"] % B.group() for e in cases)
    # ---- (s): blocks put between a definition and its use
    filler = [raw(b"between"), rle(0x5f, 9), raw(b""), compressed(b"no sequences here", [])]
    for tag, bname in (("treeless", "n_text_40000_L3_cs"), ("repeat", "n_records_40000_L19")):
        blks = walk_blocks(nat[bname])
        spliced, at = [], []
        for i, b in enumerate(blks):
            uses = b["type"] == 2 and (b["lit"] == 3 or (b["nseq"] and any(((b["modes"] >> s) & 3) == 3 for s in (6, 4, 2))))
            if uses and len(at) < 6:
                spliced += filler[len(at) % 2:]
                at.append(i)
            spliced.append(b["raw"])
        assert len(at) == 6
        if tag == "treeless":
            assert all(blks[i]["lit"] == 3 for i in at)
        else:
            assert all(any(blks[i]["modes"] >> s & 3 == 3 for i in at) for s in (6, 4, 2))
        data = replay(spliced)
        add("s_between_" + tag, "s", frame(spliced, checksum=(zf.xxh64(data) & 0xffffffff).to_bytes(4, "little")),
            "%s with Raw, RLE, empty and sequence-less blocks in front of blocks %s, which use %s" %
            (bname, at, "Treeless literals" if tag == "treeless" else "Repeat_Mode"))
    # ---- (h)
    hand = {}
    for name, blocks, what in hand_cases():
        data = replay(blocks)
        fr = frame(blocks, content=len(data), checksum=(zf.xxh64(data) & 0xffffffff).to_bytes(4, "little"))
        add(name, "h", fr, what)
        hand[name] = (blocks, data)
    tallies = set(t for e in cases if e["group"] == "h" for t in e["tally"])
    for t in ["rep:%d:%s" % (c, l) for c in (1, 2, 3) for l in ("ll>0", "ll0")]:
        assert t in tallies, t
    # ---- (r)
    text = zstd_sim.make_input("text", 600, 4)
    first = hand["h_minus_chain"][0][0]
    minus = compressed(b"", [(0, 3, 3)])
    one = compressed(text[:8], [(8, 3, 1 + 3)])                           # leaves rep0 = 1
    add("r_symbolic_0", "r", frame([one, raw(b"ab"), minus, raw(b"c")]), "rep0 is 1 when a block's first sequence applies rep0 - 1", cap=64, want=D.EDATA)
    add("r_symbolic_0_two_steps", "r", frame([compressed(text[:8], [(8, 3, 2 + 3)]), minus, minus, raw(b"c")]),
        "rep0 is 2 and two blocks in a row apply rep0 - 1: the second one reaches 0", cap=64, want=D.EDATA)
    add("r_repeat_nothing", "r", frame([raw(b"abcdefgh"), compressed(b"xy", [(2, 3, 4)], ll=("repeat", "rle")), raw(b"c")]),
        "Repeat_Mode for LL in the frame's first Compressed block", cap=64, want=D.EDATA)
    treeless = (2, bytes([0x43, 0x40, 0x00]) + b"\x01" + b"\x00", 5)          # four literals in a one-byte stream, no sequences
    add("r_treeless_nothing", "r", frame([raw(b"abcdefgh"), treeless, raw(b"c")]), "Treeless literals with no tree before them", cap=64, want=D.EDATA)
    over = compressed(b"ab", [(5, 3, 4)])                                 # takes five literals of two
    add("r_earliest_wins", "r", frame([first, over, raw(b"ok"), compressed(b"xy", [(2, 3, 4)])])[:-4],
        "block 1 takes more literals than it has (malformed), block 3 is cut (truncated): the first one is the answer", cap=256, nblocks=4, want=D.EDATA)
    add("r_later_cut_alone", "r", frame([first, raw(b"ok"), raw(b"ok"), compressed(b"xy", [(2, 3, 4)])])[:-4],
        "the same frame without the malformed block: truncated", cap=256, nblocks=4, want=D.ETRUNC)
    # one block: 12 sequences of 1 + 4 bytes behind 20 bytes; the cap ends inside record 3, the stream after record 9
    # (the cap holds the 20 bytes and the block's 14 literals: a block whose literals alone pass out_cap is malformed at its header)
    seqs = [(1, 4, 8 + (i % 4)) for i in range(12)]
    lits = text[:14]
    blocks = [raw(text[100:120]), compressed(lits, seqs[:10], nseq=12), raw(b"c")]
    add("r_eout_then_bits", "r", frame(blocks), "EOUT at record 3 (out_cap 20 + 3 * 5 + 2), the bit stream ends at record 10: EOUT", cap=37, want=D.EOUT)
    add("r_bits_alone", "r", frame(blocks), "the same frame with room: the bit stream's end is the answer", cap=400, want=D.EDATA, file_of="r_eout_then_bits.zst")
    blocks = [raw(text[100:120]), compressed(lits, seqs[:3], nseq=12), raw(b"c")]
    add("r_bits_then_eout", "r", frame(blocks), "the bit stream ends at record 3, out_cap would end at record 10: malformed", cap=20 + 10 * 5 + 3, want=D.EDATA)
    add("r_distance_global", "r", frame([raw(text[:10]), rle(0x30, 6), compressed(text[20:24], [(4, 30, 21 + 3)])]),
        "h_reach_first_byte with distance 21: one byte in front of the frame", cap=64, want=D.EDATA)
    base = nat["n_records_40000_L19"]
    k = walk_blocks(base)[17]
    add("r_cut_in_block_17", "r", base[:k["off"] + 3 + k["size"] // 2], "n_records_40000_L19 cut inside block 17", cap=40000, nblocks=len(walk_blocks(base)),
        want=D.ETRUNC)
    blocks, data = hand["h_repeat_each"]
    add("r_content_one_more", "r", frame(blocks, content=len(data) + 1), "h_repeat_each with a content size one above", cap=len(data) + 1, want=D.EDATA)
    add("r_content_one_less", "r", frame(blocks, content=len(data) - 1), "h_repeat_each with a content size one below", cap=len(data), want=D.EDATA)
    good = frame(blocks, content=len(data), checksum=(zf.xxh64(data) & 0xffffffff).to_bytes(4, "little"))
    add("r_checksum_missing", "r", good[:-4], "h_repeat_each without its four checksum bytes", cap=len(data), nblocks=len(blocks), want=D.ETRUNC)
    add("r_checksum_wrong", "r", good[:-1] + bytes([good[-1] ^ 0x80]), "h_repeat_each, last checksum byte changed", cap=len(data), want=D.ECKSUM)
    add("r_out_cap_short", "r", nat["n_text_9000_L1"], "n_text_9000_L1 with an out_cap one below the content", cap=8999, want=D.EOUT, file_of="n_text_9000_L1.zst")
    n = len(walk_blocks(nat["n_text_9000_L1"]))
    for hint in (n - 1, n + 1, 1):
        add("r_count_%d_for_%d" % (hint, n), "r", nat["n_text_9000_L1"], "n_text_9000_L1 given with %d blocks" % hint, cap=9000, nblocks=hint, want=B.EHINT,
            file_of="n_text_9000_L1.zst")
    reasons = {"r_symbolic_0": "libzstd makes a repeat offset of 0 an offset of 1 (ZSTD_decodeSequence: offset += !offset)",
               "r_symbolic_0_two_steps": "as r_symbolic_0",
               "r_bits_alone": "ZSTD_decompressSequences only checks that the stream is not left unfinished: read past its beginning it gives "
                               "zeros (RFC 8878, 4.1: the stream must be used up exactly)"}
    assert sorted(accepted) == sorted(a for a in reasons if a in accepted) and all(a in reasons for a in accepted), accepted
    with open(os.path.join(OUT, "index.json"), "w") as f:
        json.dump({"libzstd": zstd_ref.version(), "group": B.group(), "libzstd_accepts": [{"name": a, "reason": reasons[a]} for a in sorted(accepted)],
                   "cases": cases}, f, indent=1)
    print("%d cases, %d files, %d bytes; libzstd accepts %s" % (len(cases), len(files), sum(len(v) for v in files.values()), accepted))


if __name__ == "__main__":
    main()
