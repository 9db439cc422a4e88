"""An independent strict reader of the zstd subset a zstd session writes ("Zstd sessions"), written from
RFC 8878 and not from the kernel: what the tests decode the compressor's frames with.

    frame  := 28 B5 2F FD | descriptor: Single_Segment, nothing else | Frame_Content_Size in the smallest of 1, 2, 4 bytes |
              ONE block, Last_Block set: Raw (the whole content) or Compressed (smaller than the content)
    block  := literals section (Raw, RLE or Compressed; the smallest size format; Compressed: a Huffman code of at most 11
              bits, one stream up to 1023 literals and four above) | sequences section (each of LL, OF, ML Predefined or
              RLE; no repeat offsets)

Everything outside the subset or the RFC raises FormatError."""


class FormatError(ValueError):
    pass


MAGIC = b"\x28\xb5\x2f\xfd"
MAX_BLOCK = 131072
HUF_MAX_BITS = 11

LL_NORM = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
OF_NORM = [1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1]
ML_NORM = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]


def _bases(bits, first):
    out, b = [], first
    for k in bits:
        out.append(b)
        b += 1 << k
    return out


LL_BASE = _bases(LL_BITS, 0)
ML_BASE = _bases(ML_BITS, 3)
assert LL_BASE[16:26] == [16, 18, 20, 22, 24, 28, 32, 40, 48, 64] and LL_BASE[35] == 65536
assert ML_BASE[32:44] == [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131] and ML_BASE[52] == 65539


def ll_code(ll):
    return max(c for c in range(36) if LL_BASE[c] <= ll)


def ml_code(ml):
    return max(c for c in range(53) if ML_BASE[c] <= ml)


class BackBits:
    """a stream read from its end: the highest set bit of the last byte is the end mark"""

    def __init__(self, data):
        if len(data) == 0 or data[-1] == 0:
            raise FormatError("a stream without its end mark")
        self.d = bytes(data)
        self.n = 8 * (len(data) - 1) + data[-1].bit_length() - 1       # the bits below the end mark

    def _bits(self, hi, k):
        """bits hi - k .. hi - 1 of the stream as a little-endian number (a window of bytes: a long stream costs no more)"""
        lo = hi - k
        return (int.from_bytes(self.d[lo >> 3:(hi + 7) >> 3], "little") >> (lo & 7)) & ((1 << k) - 1)

    def read(self, k):
        if k > self.n:
            raise FormatError("a stream is read past its beginning")
        self.n -= k
        return self._bits(self.n + k, k)

    def peek_padded(self, k):
        """the next k bits, zeros where the stream has no more"""
        if k <= self.n:
            return self._bits(self.n, k)
        return self._bits(self.n, self.n) << (k - self.n)

    def done(self):
        if self.n:
            raise FormatError("%d bits left over in a stream" % self.n)


def fse_table(norm, log):
    """RFC 8878, 4.1.1: -> [(symbol, bits, baseline)] per state"""
    size = 1 << log
    if sum(abs(n) for n in norm) != size:
        raise FormatError("a distribution does not add up to its table")
    sym = [None] * size
    high = size - 1
    for s, n in enumerate(norm):
        if n == -1:
            sym[high] = s
            high -= 1
    pos, step = 0, (size >> 1) + (size >> 3) + 3
    for s, n in enumerate(norm):
        for _ in range(max(n, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    if pos != 0:
        raise FormatError("a distribution does not fill its table")
    nxt = [abs(n) for n in norm]
    table = []
    for u in range(size):
        s = sym[u]
        x = nxt[s]
        nxt[s] += 1
        nb = log - (x.bit_length() - 1)
        table.append((s, nb, (x << nb) - size))
    return table


LL_TABLE = fse_table(LL_NORM, 6)
OF_TABLE = fse_table(OF_NORM, 5)
ML_TABLE = fse_table(ML_NORM, 6)


def read_ncount(data, max_log, max_symbols, notes=None):
    """an FSE table description -> (distribution, accuracy log, bytes used); notes (a set) <- "ncount:..." tags of its shape"""
    v = int.from_bytes(data, "little")
    avail = 8 * len(data)
    log = 5 + (v & 15)
    pos = 4
    if log > max_log:
        raise FormatError("accuracy log %d above %d" % (log, max_log))
    remaining, threshold, nbits = (1 << log) + 1, 1 << log, log + 1
    norm, prev0 = [], False
    while remaining > 1:
        if prev0:
            run = 1
            while True:
                r = (v >> pos) & 3
                pos += 2
                norm += [0] * r
                run += r
                if r != 3:
                    break
            if notes is not None:
                notes.add("ncount:zrun:%d" % run)
        if len(norm) >= max_symbols:
            raise FormatError("a distribution with more than %d symbols" % max_symbols)
        mx = (2 * threshold - 1) - remaining
        if ((v >> pos) & (threshold - 1)) < mx:
            count = (v >> pos) & (threshold - 1)
            pos += nbits - 1
        else:
            count = (v >> pos) & (2 * threshold - 1)
            if count >= threshold:
                count -= mx
            pos += nbits
        count -= 1
        remaining -= abs(count)
        if remaining < 1:
            raise FormatError("a distribution above its table's size")
        norm.append(count)
        prev0 = count == 0
        while remaining < threshold:
            nbits -= 1
            threshold >>= 1
        if pos > avail:
            raise FormatError("a distribution is cut by its field's end")
    if notes is not None:
        notes.add("ncount:lastbits:%d" % ((pos - 1) % 8 + 1))
        if -1 in norm:
            notes.add("ncount:lessthan1")
    return norm, log, (pos + 7) // 8


def read_weights_fse(data, notes=None):
    """FSE-compressed Huffman weights (4.2.1.2): two states taking turns until the stream is used up"""
    norm, log, used = read_ncount(data, 6, 13, notes)
    if notes is not None:
        notes.add("wlog:%d" % log)
    table = fse_table(norm, log)
    bits = BackBits(data[used:])
    st = [bits.read(log), bits.read(log)]
    out, k = [], 0
    while True:
        s, nb, base = table[st[k]]
        out.append(s)
        if nb > bits.n:
            out.append(table[st[k ^ 1]][0])
            break
        st[k] = base + bits.read(nb)
        if st[k] >= len(table):
            raise FormatError("FSE state %d out of range" % st[k])
        k ^= 1
        if len(out) > 255:
            raise FormatError("more than 255 weights")
    if len(out) > 255:                                              # (the last two come without another look at the count)
        raise FormatError("more than 255 weights")
    bits.done()
    return out


def huffman_table(weights):
    """the listed weights (the last one follows from them) -> (lookup by the next `maxbits` bits: (symbol, length), maxbits)"""
    total = sum((1 << (w - 1)) for w in weights if w)
    if total == 0:
        raise FormatError("a Huffman tree without weights")
    maxbits = total.bit_length()
    rest = (1 << maxbits) - total
    if rest & (rest - 1):
        raise FormatError("Huffman weights do not add up to a power of two")
    if maxbits > HUF_MAX_BITS:
        raise FormatError("a Huffman code of %d bits" % maxbits)
    weights = list(weights) + [rest.bit_length()]
    if any(w > maxbits for w in weights):
        raise FormatError("a Huffman weight above the tree's height")
    if weights.count(1) < 2:                                        # libzstd's HUF_readStats: rankStats[1] < 2
        raise FormatError("a Huffman tree without two symbols of weight 1")
    table = []
    for w in range(1, maxbits + 1):
        for s, ws in enumerate(weights):
            if ws == w:
                table += [(s, maxbits + 1 - w)] * (1 << (w - 1))
    assert len(table) == 1 << maxbits
    return table, maxbits


def huffman_stream(data, table, maxbits, count):
    bits = BackBits(data)
    out = bytearray()
    for _ in range(count):
        s, ln = table[bits.peek_padded(maxbits)]
        if ln > bits.n:
            raise FormatError("a Huffman stream ends inside a code")
        bits.n -= ln
        out.append(s)
    bits.done()
    return bytes(out)


def read_literals(blk):
    """-> (literals, bytes used, info)"""
    if not blk:
        raise FormatError("a block without a literals section")
    t, fmt = blk[0] & 3, (blk[0] >> 2) & 3
    if t == 3:
        raise FormatError("treeless literals are outside the subset")
    if t < 2:
        if not blk[0] & 4:                                          # one bit of size format: bit 3 belongs to the size
            hs, n = 1, blk[0] >> 3
        elif fmt == 1:
            hs, n = 2, int.from_bytes(blk[:2], "little") >> 4
            if n < 32:
                raise FormatError("wrong size format: %d literals fit one byte" % n)
        else:
            hs, n = 3, int.from_bytes(blk[:3], "little") >> 4
            if n < 4096:
                raise FormatError("wrong size format: %d literals fit two bytes" % n)
        if len(blk) < hs:
            raise FormatError("the literals header is cut")
        if n > MAX_BLOCK:
            raise FormatError("%d literals" % n)
        if t == 0:
            if len(blk) < hs + n:
                raise FormatError("raw literals are cut by the block's end")
            return bytes(blk[hs:hs + n]), hs + n, {"type": "raw", "regen": n, "size": hs + n}
        if len(blk) < hs + 1:
            raise FormatError("the RLE literal is missing")
        return bytes(blk[hs:hs + 1]) * n, hs + 1, {"type": "rle", "regen": n, "size": hs + 1}
    if fmt == 0:
        hs, bits, streams = 3, 10, 1
    elif fmt == 1:
        raise FormatError("four streams in the 10-bit size format are outside the subset")
    elif fmt == 2:
        hs, bits, streams = 4, 14, 4
    else:
        hs, bits, streams = 5, 18, 4
    if len(blk) < hs:
        raise FormatError("the literals header is cut")
    v = int.from_bytes(blk[:hs], "little") >> 4
    n, csz = v & ((1 << bits) - 1), v >> bits
    if (fmt == 0 and n > 1023) or (fmt == 2 and not 1024 <= n <= 16383) or (fmt == 3 and n < 16384):
        raise FormatError("wrong size format %d for %d literals" % (fmt, n))
    if n > MAX_BLOCK:
        raise FormatError("%d literals" % n)
    if len(blk) < hs + csz or csz == 0:
        raise FormatError("compressed literals are cut by the block's end")
    body = blk[hs:hs + csz]
    hb = body[0]
    if hb >= 128:
        nw = hb - 127
        dsz = 1 + (nw + 1) // 2
        if len(body) < dsz:
            raise FormatError("the weights are cut")
        weights = []
        for i in range(nw):
            b = body[1 + i // 2]
            weights.append(b >> 4 if i % 2 == 0 else b & 15)
        if nw % 2 and body[dsz - 1] & 15:
            raise FormatError("a weight behind the last one")
        desc = "direct"
    else:
        if hb == 0 or len(body) < 1 + hb:
            raise FormatError("the compressed weights are cut")
        weights = read_weights_fse(body[1:1 + hb])
        dsz = 1 + hb
        desc = "fse"
    table, maxbits = huffman_table(weights)
    rest = body[dsz:]
    if streams == 1:
        lits = huffman_stream(rest, table, maxbits, n)
    else:
        if len(rest) < 6:
            raise FormatError("the jump table is cut")
        s1, s2, s3 = (int.from_bytes(rest[2 * i:2 * i + 2], "little") for i in range(3))
        rest = rest[6:]
        if s1 + s2 + s3 >= len(rest):
            raise FormatError("the jump table runs past the literals section")
        seg = (n + 3) // 4
        cuts = [0, s1, s1 + s2, s1 + s2 + s3, len(rest)]
        counts = [seg, seg, seg, n - 3 * seg]
        lits = b"".join(huffman_stream(rest[cuts[i]:cuts[i + 1]], table, maxbits, counts[i]) for i in range(4))
    return lits, hs + csz, {"type": "compressed", "regen": n, "size": hs + csz, "streams": streams, "description": desc,
                            "description_size": dsz, "maxbits": maxbits}


def _seq_table(mode, name, predefined, maxcode, blk, pos):
    if mode == 0:
        return predefined, pos, 6 if name != "OF" else 5
    if mode == 1:
        if pos >= len(blk):
            raise FormatError("an RLE table's code is missing")
        if blk[pos] > maxcode:
            raise FormatError("FSE symbol %d out of range for %s" % (blk[pos], name))
        return [(blk[pos], 0, 0)], pos + 1, 0
    raise FormatError("%s mode %d is outside the subset" % (name, mode))


def read_sequences(blk):
    """-> ([(literal length, match length, offset)], info)"""
    if not blk:
        raise FormatError("a block without a sequences section")
    b0 = blk[0]
    if b0 < 128:
        n, pos = b0, 1
    elif b0 < 255:
        if len(blk) < 2:
            raise FormatError("the sequence count is cut")
        n, pos = ((b0 - 128) << 8) + blk[1], 2
        if n < 128:
            raise FormatError("wrong size format: %d sequences fit one byte" % n)
    else:
        if len(blk) < 3:
            raise FormatError("the sequence count is cut")
        n, pos = blk[1] + (blk[2] << 8) + 0x7f00, 3
    if n == 0:
        if len(blk) != 1:
            raise FormatError("bytes behind an empty sequences section")
        return [], {"count": 0, "size": 1, "modes": None}
    if pos >= len(blk):
        raise FormatError("the modes byte is missing")
    modes = blk[pos]
    pos += 1
    if modes & 3:
        raise FormatError("reserved bits in the modes byte")
    llt, pos, lllog = _seq_table(modes >> 6, "LL", LL_TABLE, 35, blk, pos)
    oft, pos, oflog = _seq_table((modes >> 4) & 3, "OF", OF_TABLE, 31, blk, pos)
    mlt, pos, mllog = _seq_table((modes >> 2) & 3, "ML", ML_TABLE, 52, blk, pos)
    bits = BackBits(blk[pos:])
    sl, so, sm = bits.read(lllog), bits.read(oflog), bits.read(mllog)
    seqs = []
    for i in range(n):
        lc, oc, mc = llt[sl][0], oft[so][0], mlt[sm][0]
        ov = (1 << oc) + bits.read(oc)
        ml = ML_BASE[mc] + bits.read(ML_BITS[mc])
        ll = LL_BASE[lc] + bits.read(LL_BITS[lc])
        if ov <= 3:
            raise FormatError("a repeat offset is outside the subset")
        seqs.append((ll, ml, ov - 3))
        if i + 1 < n:
            sl = llt[sl][2] + bits.read(llt[sl][1])
            sm = mlt[sm][2] + bits.read(mlt[sm][1])
            so = oft[so][2] + bits.read(oft[so][1])
            if sl >= len(llt) or sm >= len(mlt) or so >= len(oft):
                raise FormatError("FSE state out of range")
    bits.done()
    return seqs, {"count": n, "size": len(blk), "modes": (modes >> 6, (modes >> 4) & 3, (modes >> 2) & 3)}


def decode_frame(buf, pos=0):
    """the frame at buf[pos:] -> (info, where the next one begins).  info: "data", "sequences" (None for a Raw block),
    "size", "content_size", "header_size", "block" ("raw" / "compressed"), "literals" and "seq" (the sections' infos)"""
    start = pos
    if buf[pos:pos + 4] != MAGIC:
        raise FormatError("no zstd magic")
    if pos + 5 > len(buf):
        raise FormatError("the frame header is cut")
    fhd = buf[pos + 4]
    if fhd & 0x08:
        raise FormatError("reserved bit in the frame header descriptor")
    if fhd & 0x10:
        raise FormatError("unused bit set in the frame header descriptor")
    if not fhd & 0x20:
        raise FormatError("a frame without Single_Segment is outside the subset")
    if fhd & 0x04:
        raise FormatError("a content checksum is outside the subset")
    if fhd & 0x03:
        raise FormatError("a dictionary id is outside the subset")
    flag = fhd >> 6
    if flag == 3:
        raise FormatError("an 8-byte content size is outside the subset")
    fb = (1, 2, 4)[flag]
    pos += 5
    if pos + fb + 3 > len(buf):
        raise FormatError("the frame header is cut")
    content = int.from_bytes(buf[pos:pos + fb], "little") + (256 if flag == 1 else 0)
    if flag == 2 and content < 65792:
        raise FormatError("wrong size format: a content size of %d fits a smaller field" % content)
    if content == 0 or content > MAX_BLOCK:
        raise FormatError("content size %d" % content)
    pos += fb
    bh = int.from_bytes(buf[pos:pos + 3], "little")
    pos += 3
    if not bh & 1:
        raise FormatError("more than one block is outside the subset")
    btype, bsz = (bh >> 1) & 3, bh >> 3
    if pos + bsz > len(buf):
        raise FormatError("the block runs past the stream")
    info = {"content_size": content, "header_size": 5 + fb, "literals": None, "seq": None}
    if btype == 0:
        if bsz != content:
            raise FormatError("content size %d, Raw block of %d" % (content, bsz))
        info.update(block="raw", data=bytes(buf[pos:pos + bsz]), sequences=None)
    elif btype == 2:
        if bsz >= content:
            raise FormatError("a Compressed block of %d bytes for %d" % (bsz, content))
        blk = bytes(buf[pos:pos + bsz])
        lits, used, linfo = read_literals(blk)
        seqs, sinfo = read_sequences(blk[used:])
        out = bytearray()
        lp = 0
        for ll, ml, off in seqs:
            if lp + ll > len(lits):
                raise FormatError("a sequence takes more literals than the section holds")
            out += lits[lp:lp + ll]
            lp += ll
            if off > len(out):
                raise FormatError("offset %d with %d bytes produced" % (off, len(out)))
            if off >= ml:
                out += out[len(out) - off:len(out) - off + ml]
            else:
                for _ in range(ml):
                    out.append(out[-off])
        out += lits[lp:]
        if len(out) != content:
            raise FormatError("content size %d, %d bytes decoded" % (content, len(out)))
        info.update(block="compressed", data=bytes(out), sequences=seqs, literals=linfo, seq=sinfo)
    else:
        raise FormatError("block type %d is outside the subset" % btype)
    pos += bsz
    info["size"] = pos - start
    return info, pos


def decode_frames(stream):
    """-> [info per frame]"""
    stream = bytes(stream)
    pos, frames = 0, []
    while pos < len(stream):
        info, pos = decode_frame(stream, pos)
        frames.append(info)
    return frames


def decode(stream, hw_buff_sz=None):
    """the data of a stream of frames; with hw_buff_sz, every frame but the last must hold exactly that much"""
    frames = decode_frames(stream)
    if hw_buff_sz is not None:
        for i, f in enumerate(frames):
            if f["content_size"] > hw_buff_sz or (i + 1 < len(frames) and f["content_size"] != hw_buff_sz):
                raise FormatError("frame %d holds %d bytes (hw_buff_sz %d)" % (i, f["content_size"], hw_buff_sz))
    return b"".join(f["data"] for f in frames)


def bound(n, hw_buff_sz):
    """qzMaxCompressedLength of a zstd session: per chunk of c bytes the Raw block, 4 + 1 + 4 + 3 + c"""
    full, rest = divmod(n, hw_buff_sz)
    return full * (hw_buff_sz + 12) + (rest + 12 if rest else 0)
