"""A strict reader of whole RFC 8878 frames without dictionaries - the scope of a zstd decode session ("Zstd
sessions", decoding) - written from the RFC on top of zstd_format's bit readers and table builders: the model the device
decoder (qatzip_amd/csrc/qzk_zstdd.h) is compared with, frame by frame.  Beside the data it returns a tally of the format
features a frame uses, which tests/golden/gen_zstd_dec.py records and tests/test_sim_zstdd.py checks for coverage.

Everything the RFC or the scope forbids raises FormatError; Truncated (a FormatError) where the input merely ends early."""
from zstd_format import (FormatError, BackBits, fse_table, read_ncount, read_weights_fse, huffman_table, huffman_stream,
                         LL_TABLE, OF_TABLE, ML_TABLE, LL_BASE, ML_BASE, LL_BITS, ML_BITS, MAX_BLOCK)

MAGIC = 0xFD2FB528
M64 = (1 << 64) - 1
P1, P2, P3, P4, P5 = (0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5)


class Truncated(FormatError):
    pass


def _rotl(v, r):
    return ((v << r) | (v >> (64 - r))) & M64


def _round(acc, v):
    return (_rotl((acc + v * P2) & M64, 31) * P1) & M64


def xxh64(data, seed=0):
    """XXH64 from its specification (xxhash_spec.md)"""
    n, p = len(data), 0
    if n >= 32:
        a = [(seed + P1 + P2) & M64, (seed + P2) & M64, seed, (seed - P1) & M64]
        while p + 32 <= n:
            for i in range(4):
                a[i] = _round(a[i], int.from_bytes(data[p + 8 * i:p + 8 * i + 8], "little"))
            p += 32
        h = (_rotl(a[0], 1) + _rotl(a[1], 7) + _rotl(a[2], 12) + _rotl(a[3], 18)) & M64
        for v in a:
            h = ((h ^ _round(0, v)) * P1 + P4) & M64
    else:
        h = (seed + P5) & M64
    h = (h + n) & M64
    while p + 8 <= n:
        h = (_rotl(h ^ _round(0, int.from_bytes(data[p:p + 8], "little")), 27) * P1 + P4) & M64
        p += 8
    if p + 4 <= n:
        h = (_rotl(h ^ (int.from_bytes(data[p:p + 4], "little") * P1 & M64), 23) * P2 + P3) & M64
        p += 4
    while p < n:
        h = (_rotl(h ^ (data[p] * P5 & M64), 11) * P1) & M64
        p += 1
    h ^= h >> 33
    h = h * P2 & M64
    h ^= h >> 29
    h = h * P3 & M64
    return h ^ (h >> 32)


MODE_NAMES = ("predefined", "rle", "fse", "repeat")


class _Frame:
    """what a frame keeps across its blocks"""

    def __init__(self):
        self.huf = None                    # (table, maxbits)
        self.tabs = {"LL": None, "OF": None, "ML": None}
        self.rep = [1, 4, 8]
        self.tally = set()
        self.sections = []                 # (name, start, end) in the frame's bytes
        self.lit_types = []                # the literals type of every Compressed block so far
        self.tkind = {"LL": None, "OF": None, "ML": None}     # what each table was last set from
        self.nseq0_since = {"LL": False, "OF": False, "ML": False}


def _literals(blk, F, at=0):
    """-> (literals, bytes used); at: where blk begins in the frame (for the sections)"""
    if not blk:
        raise FormatError("a block without a literals section")
    t, fmt = blk[0] & 3, (blk[0] >> 2) & 3
    F.lit_types.append(("raw", "rle", "huffman", "treeless")[t])
    if t < 2:
        hs = 1 if not fmt & 1 else 2 if fmt == 1 else 3
        if len(blk) < hs:
            raise FormatError("the literals header is cut")
        n = int.from_bytes(blk[:hs], "little") >> (3 if hs == 1 else 4)
        if n > MAX_BLOCK:
            raise FormatError("%d literals" % n)
        if t == 0:
            if len(blk) < hs + n:
                raise FormatError("raw literals are cut by the block's end")
            F.tally.add("lit:raw")
            F.sections += [("literals_header", at, at + hs), ("raw_literals", at + hs, at + hs + n)]
            return bytes(blk[hs:hs + n]), hs + n
        if len(blk) < hs + 1:
            raise FormatError("the RLE literal is missing")
        F.tally.add("lit:rle")
        F.sections += [("literals_header", at, at + hs), ("rle_literal", at + hs, at + hs + 1)]
        return bytes(blk[hs:hs + 1]) * n, hs + 1
    hs, bits, streams = ((3, 10, 1), (3, 10, 4), (4, 14, 4), (5, 18, 4))[fmt]
    if len(blk) < hs:
        raise FormatError("the literals header is cut")
    v = int.from_bytes(blk[:hs], "little") >> 4
    n, csz = v & ((1 << bits) - 1), v >> bits
    if n > MAX_BLOCK:
        raise FormatError("%d literals" % n)
    if len(blk) < hs + csz:
        raise FormatError("compressed literals are cut by the block's end")
    body = blk[hs:hs + csz]
    F.sections.append(("literals_header", at, at + hs))
    at += hs
    if t == 3:
        if F.huf is None:
            raise FormatError("treeless literals without a previous tree")
        F.tally.add("lit:treeless")
        if F.lit_types[-3:] == ["huffman", "raw", "treeless"]:
            F.tally.add("lit:treeless<raw<huffman")
        dsz = 0
    else:
        if not body:
            raise FormatError("the tree description is missing")
        hb = body[0]
        if hb >= 128:
            nw = hb - 127
            dsz = 1 + (nw + 1) // 2
            if len(body) < dsz:
                raise FormatError("the weights are cut")
            weights = [(body[1 + i // 2] >> 4) if i % 2 == 0 else (body[1 + i // 2] & 15) for i in range(nw)]
            F.tally.add("weights:direct")
            if nw == 128:
                F.tally.add("weights:direct128")
            F.sections += [("tree_header", at, at + 1), ("tree_weights", at + 1, at + dsz)]
        else:
            if hb == 0 or len(body) < 1 + hb:
                raise FormatError("the compressed weights are cut")
            weights = read_weights_fse(body[1:1 + hb], F.tally)
            dsz = 1 + hb
            F.sections += [("tree_header", at, at + 1), ("tree_weights", at + 1, at + dsz)]
            F.tally.add("weights:fse")
        F.huf = huffman_table(weights)
        F.tally.add("lit:huffman")
    table, maxbits = F.huf
    F.tally.add("hufbits:%d" % maxbits)
    rest = body[dsz:]
    at += dsz
    if streams == 1:
        lits = huffman_stream(rest, table, maxbits, n)
        F.sections.append(("stream1", at, at + len(rest)))
        if n == 1:
            F.tally.add("lit:1stream:1")
    else:
        F.tally.add("lit:4streams%d" % bits)
        if len(rest) < 6:
            raise FormatError("the jump table is cut")
        s1, s2, s3 = (int.from_bytes(rest[2 * i:2 * i + 2], "little") for i in range(3))
        rest = rest[6:]
        if s1 + s2 + s3 >= len(rest):
            raise FormatError("the jump table runs past the literals section")
        seg = (n + 3) // 4
        if n < 3 * seg:
            raise FormatError("%d literals in four streams" % n)
        cuts = [0, s1, s1 + s2, s1 + s2 + s3, len(rest)]
        counts = [seg, seg, seg, n - 3 * seg]
        if counts[3] < 2:
            F.tally.add("lit:stream4:%d" % counts[3])
        F.sections.append(("jump_table", at, at + 6))
        F.sections += [("stream%d" % (i + 1), at + 6 + cuts[i], at + 6 + cuts[i + 1]) for i in range(4)]
        lits = b"".join(huffman_stream(rest[cuts[i]:cuts[i + 1]], table, maxbits, counts[i]) for i in range(4))
    return lits, hs + csz


_SEQ = {"LL": (LL_TABLE, 6, 35, 9), "OF": (OF_TABLE, 5, 31, 8), "ML": (ML_TABLE, 6, 52, 9)}


def _seq_table(mode, name, blk, pos, F, at):
    predefined, plog, maxcode, maxlog = _SEQ[name]
    F.tally.add("%s:%s" % (name.lower(), MODE_NAMES[mode]))
    start = pos
    if mode == 3:
        if F.tabs[name] is not None and F.nseq0_since[name]:
            F.tally.add("repeat<nseq0<%s" % F.tkind[name])
    else:
        F.tkind[name] = MODE_NAMES[mode]
    F.nseq0_since[name] = False
    if mode == 0:
        F.tabs[name] = (predefined, plog)
    elif mode == 1:
        if pos >= len(blk):
            raise FormatError("an RLE table's code is missing")
        if blk[pos] > maxcode:
            raise FormatError("FSE symbol %d out of range for %s" % (blk[pos], name))
        F.tabs[name] = ([(blk[pos], 0, 0)], 0)
        pos += 1
    elif mode == 2:
        norm, log, used = read_ncount(blk[pos:], maxlog, maxcode + 1, F.tally)
        F.tabs[name] = (fse_table(norm, log), log)
        F.tally.add("tablelog:%s:%d" % (name.lower(), log))
        pos += used
    elif F.tabs[name] is None:
        raise FormatError("%s repeats a table that was never set" % name)
    if pos > start:
        F.sections.append(("%s_%s" % (name.lower(), "rle_code" if mode == 1 else "description"), at + start, at + pos))
    return pos


def _sequences(blk, F, produced, nlits, at=0):
    """-> [(literal length, match length, distance)], repeat offsets resolved; at: where blk begins in the frame"""
    if not blk:
        raise FormatError("a block without a sequences section")
    b0 = blk[0]
    if b0 < 128:
        n, pos = b0, 1
    elif b0 < 255:
        if len(blk) < 2:
            raise FormatError("the sequence count is cut")
        n, pos = ((b0 - 128) << 8) + blk[1], 2
    else:
        if len(blk) < 3:
            raise FormatError("the sequence count is cut")
        n, pos = blk[1] + (blk[2] << 8) + 0x7f00, 3
    if n == 0:
        if len(blk) != 1:
            raise FormatError("bytes behind an empty sequences section")
        F.tally.add("nseq0")
        F.sections.append(("sequence_count", at, at + 1))
        for k in F.nseq0_since:
            F.nseq0_since[k] = True
        return []
    if pos >= len(blk):
        raise FormatError("the modes byte is missing")
    modes = blk[pos]
    F.sections += [("sequence_count", at, at + pos), ("modes", at + pos, at + pos + 1)]
    pos += 1
    if modes & 3:
        raise FormatError("reserved bits in the modes byte")
    had = all(F.tabs[k] is not None for k in ("LL", "OF", "ML"))
    for shift, name in ((6, "LL"), (4, "OF"), (2, "ML")):
        if (modes >> shift) & 3 == 3 and not had:
            raise FormatError("%s repeats a table that was never set" % name)
        pos = _seq_table((modes >> shift) & 3, name, blk, pos, F, at)
    (llt, lllog), (oft, oflog), (mlt, mllog) = F.tabs["LL"], F.tabs["OF"], F.tabs["ML"]
    F.sections.append(("bitstream", at + pos, at + len(blk)))
    bits = BackBits(blk[pos:])
    sl, so, sm = bits.read(lllog), bits.read(oflog), bits.read(mllog)
    seqs, rep, used = [], F.rep, 0
    for i in range(n):
        lc, oc, mc = llt[sl][0], oft[so][0], mlt[sm][0]
        if lc > 35 or oc > 31 or mc > 52:
            raise FormatError("a sequence code out of range")
        ov = (1 << oc) + bits.read(oc)
        ml = ML_BASE[mc] + bits.read(ML_BITS[mc])
        ll = LL_BASE[lc] + bits.read(LL_BITS[lc])
        if oc > 16:
            F.tally.add("ofcode>16")
        if lc == 35:
            F.tally.add("llcode35")
        if ov > 3:
            off = ov - 3
            rep = [off, rep[0], rep[1]]
        else:
            F.tally.add("rep:%d:%s" % (ov, "ll0" if ll == 0 else "ll>0"))
            idx = ov - 1 + (1 if ll == 0 else 0)
            if idx:
                off = rep[idx] if idx < 3 else rep[0] - 1
                if off == 0:
                    raise FormatError("a repeat offset of 0")
                rep = [off, rep[0], rep[2] if idx == 1 else rep[1]]
            else:
                off = rep[0]
        used += ll
        if used > nlits:
            raise FormatError("a sequence takes more literals than the section holds")
        produced += ll
        if off > produced:
            raise FormatError("offset %d with %d bytes produced" % (off, produced))
        if off == produced:
            F.tally.add("offset:all-produced")
        if i == 0 and (ll, ml, off) == (1, 3, 1):
            F.tally.add("seq0:ll1:ml3:off1")
        produced += ml
        seqs.append((ll, ml, off))
        if i + 1 < n:
            sl = llt[sl][2] + bits.read(llt[sl][1])
            sm = mlt[sm][2] + bits.read(mlt[sm][1])
            so = oft[so][2] + bits.read(oft[so][1])
    bits.done()
    F.rep = rep
    return seqs


def frame_header(buf, pos=0):
    """-> dict(header_size, window or None, content_size or None, checksum, single, fcs_bytes) of the zstd frame at buf[pos:]"""
    if len(buf) - pos < 5:
        raise Truncated("the frame header is cut")
    fhd = buf[pos + 4]
    if fhd & 0x08:
        raise FormatError("reserved bit in the frame header descriptor")
    if fhd & 0x03:
        raise FormatError("a dictionary id")
    single, flag = bool(fhd & 0x20), fhd >> 6
    fb = (1 if single else 0, 2, 4, 8)[flag]
    hs = 5 + (0 if single else 1) + fb
    if len(buf) - pos < hs:
        raise Truncated("the frame header is cut")
    p = pos + 5
    window = None
    if not single:
        wlog = 10 + (buf[p] >> 3)
        if wlog > 31:                                               # libzstd's ZSTD_WINDOWLOG_MAX
            raise FormatError("a window log of %d" % wlog)
        window = (1 << wlog) + ((1 << wlog) >> 3) * (buf[p] & 7)
        p += 1
    content = None
    if fb:
        content = int.from_bytes(buf[p:p + fb], "little") + (256 if fb == 2 else 0)
    return {"header_size": hs, "window": window, "content_size": content, "checksum": bool(fhd & 4), "single": single, "fcs_bytes": fb}


def decode_frame(buf, pos=0):
    """the frame at buf[pos:] -> (info, where the next one begins).  info: "data", "size", "content_size" (or None), "blocks",
    "tally" (a sorted list), "skippable", "sections" ([(name, start, end)] in the order met, positions from the frame's start) """
    F = _Frame()
    try:
        return _decode_frame(bytes(buf), pos, F)
    except FormatError as e:
        e.sections = F.sections             # what was read before the refusal
        raise


def _decode_frame(buf, pos, F):
    start = pos
    if len(buf) - pos < 4:
        raise Truncated("no magic")
    magic = int.from_bytes(buf[pos:pos + 4], "little")
    if magic & 0xFFFFFFF0 == 0x184D2A50:
        if len(buf) - pos < 8:
            raise Truncated("a skippable frame's size is cut")
        sz = int.from_bytes(buf[pos + 4:pos + 8], "little")
        if len(buf) - pos < 8 + sz:
            raise Truncated("a skippable frame is cut")
        return {"data": b"", "size": 8 + sz, "content_size": 0, "blocks": 0, "tally": ["skippable"], "skippable": True,
                "sections": [("frame_header", 0, 8), ("skippable_data", 8, 8 + sz)]}, pos + 8 + sz
    if magic != MAGIC:
        raise FormatError("no zstd magic")
    h = frame_header(buf, pos)
    F.tally.add("fcs:%d" % h["fcs_bytes"])
    F.tally.add("single" if h["single"] else "window")
    if h["window"] is not None and h["content_size"] is not None:
        F.tally.add("window+fcs")
    if h["checksum"]:
        F.tally.add("checksum")
    window = h["window"] if h["window"] is not None else h["content_size"]
    bmax = min(window, MAX_BLOCK)
    if not h["single"] and buf[pos + 5] & 7:
        F.tally.add("window:mantissa")
    if h["content_size"] in (255, 256, 65791, 65792):
        F.tally.add("content:%d" % h["content_size"])
    F.sections.append(("frame_header", 0, h["header_size"]))
    pos += h["header_size"]
    out = bytearray()
    nblocks = 0
    while True:
        if len(buf) - pos < 3:
            raise Truncated("a block header is cut")
        bh = int.from_bytes(buf[pos:pos + 3], "little")
        pos += 3
        last, btype, bsz = bh & 1, (bh >> 1) & 3, bh >> 3
        nblocks += 1
        F.sections.append(("block_header", pos - 3 - start, pos - start))
        if btype == 3:
            raise FormatError("block type 3")
        if bsz > bmax:
            raise FormatError("a block of %d with a maximum of %d" % (bsz, bmax))
        if btype == 0:
            if len(buf) - pos < bsz:
                raise Truncated("a Raw block is cut")
            out += buf[pos:pos + bsz]
            F.sections.append(("raw_block", pos - start, pos - start + bsz))
            pos += bsz
            F.tally.add("block:raw")
            if last and bsz == 0:
                F.tally.add("block:raw:empty-last")
            if h["window"] is not None and bsz == bmax < MAX_BLOCK:
                F.tally.add("block:at-window")
        elif btype == 1:
            if len(buf) - pos < 1:
                raise Truncated("an RLE block is cut")
            out += buf[pos:pos + 1] * bsz
            F.sections.append(("rle_block", pos - start, pos - start + 1))
            pos += 1
            F.tally.add("block:rle")
            if bsz in (1, MAX_BLOCK):
                F.tally.add("block:rle:%s" % ("1" if bsz == 1 else "max"))
        else:
            if len(buf) - pos < bsz:
                raise Truncated("a Compressed block is cut")
            blk = buf[pos:pos + bsz]
            pos += bsz
            F.tally.add("block:compressed")
            lits, used = _literals(blk, F, pos - bsz - start)
            before = len(out)
            seqs = _sequences(blk[used:], F, before, len(lits), pos - bsz - start + used)
            lp = 0
            for ll, ml, off in seqs:
                out += lits[lp:lp + ll]
                lp += ll
                if off >= ml:
                    out += out[len(out) - off:len(out) - off + ml]
                else:
                    pat = bytes(out[len(out) - off:])
                    out += (pat * (ml // off + 1))[:ml]
            out += lits[lp:]
            if len(out) - before > bmax:
                raise FormatError("a block of %d bytes with a maximum of %d" % (len(out) - before, bmax))
            if len(out) - before == MAX_BLOCK:
                F.tally.add("block:compressed:max")
        if h["content_size"] is not None and len(out) > h["content_size"]:
            raise FormatError("output beyond the content size")
        if last:
            break
    if h["content_size"] is not None and len(out) != h["content_size"]:
        raise FormatError("content size %d, %d bytes decoded" % (h["content_size"], len(out)))
    if h["checksum"]:
        if len(buf) - pos < 4:
            raise Truncated("the content checksum is cut")
        if int.from_bytes(buf[pos:pos + 4], "little") != xxh64(bytes(out)) & 0xFFFFFFFF:
            raise FormatError("content checksum mismatch")
        F.sections.append(("checksum", pos - start, pos - start + 4))
        pos += 4
    return {"data": bytes(out), "size": pos - start, "content_size": h["content_size"], "blocks": nblocks,
            "tally": sorted(F.tally), "skippable": False, "sections": F.sections}, pos


def decode_frames(stream):
    stream = bytes(stream)
    pos, frames = 0, []
    while pos < len(stream):
        info, pos = decode_frame(stream, pos)
        frames.append(info)
    return frames


def decode(stream):
    return b"".join(f["data"] for f in decode_frames(stream))
