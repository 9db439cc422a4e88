"""An independent reader of LZ4s streams, written from the format section of INTEGRATION.md ("LZ4s sessions") and not from
the kernel: what the tests decode the compressor's output with.

    block    := u32le size, then `size` bytes of sequences
    sequence := token | [lit-len bytes] | literals | ( end of block | u16le offset | [match-len bytes] )

The reader is strict: everything the format does not allow raises FormatError."""
import struct


class FormatError(ValueError):
    pass


def _ext(blk, pos, v):
    """the 15 rule: add the following bytes until one is below 255"""
    while True:
        if pos >= len(blk):
            raise FormatError("a length byte is cut by the block's end")
        s = blk[pos]
        pos += 1
        v += s
        if s != 255:
            return v, pos


def decode_block(blk, mini_match):
    """one block's sequences -> (bytes, {"sequences", "matches", "shortest_match", "longest_offset", "longest_literals",
    "longest_match"}); shortest_match is None without a match"""
    if mini_match not in (3, 4):
        raise ValueError("mini_match is 3 or 4")
    out = bytearray()
    st = {"sequences": 0, "matches": 0, "shortest_match": None, "longest_offset": 0, "longest_literals": 0, "longest_match": 0}
    pos = 0
    while pos < len(blk):
        token = blk[pos]
        pos += 1
        L = token >> 4
        if L == 15:
            L, pos = _ext(blk, pos, L)
        if L > 65535:
            raise FormatError("literal length %d above 65535" % L)
        if pos + L > len(blk):
            raise FormatError("literals are cut by the block's end")
        out += blk[pos:pos + L]
        pos += L
        st["sequences"] += 1
        st["longest_literals"] = max(st["longest_literals"], L)
        if pos == len(blk):
            if token & 15:
                raise FormatError("a match code without an offset at the block's end")
            if L == 0:
                raise FormatError("trailing empty sequence")
            break
        if pos + 2 > len(blk):
            raise FormatError("the offset is cut by the block's end")
        offset = blk[pos] | blk[pos + 1] << 8
        pos += 2
        M = token & 15
        if M == 15:
            M, pos = _ext(blk, pos, M)
        if M == 0:
            if offset:
                raise FormatError("offset %d on a sequence without a match" % offset)
            if L == 0:
                raise FormatError("empty sequence")
            continue
        ml = M + mini_match - 1
        if ml > 65535:
            raise FormatError("match length %d above 65535" % ml)
        if offset == 0 or offset > len(out):
            raise FormatError("offset %d with %d bytes produced" % (offset, len(out)))
        st["matches"] += 1
        st["shortest_match"] = ml if st["shortest_match"] is None else min(st["shortest_match"], ml)
        st["longest_match"] = max(st["longest_match"], ml)
        st["longest_offset"] = max(st["longest_offset"], offset)
        if offset >= ml:
            out += out[len(out) - offset:len(out) - offset + ml]
        else:
            for _ in range(ml):
                out.append(out[-offset])
    return bytes(out), st


def split(stream):
    """the blocks of a stream, each with its size word"""
    pos, blocks = 0, []
    while pos < len(stream):
        if pos + 4 > len(stream):
            raise FormatError("a size word is cut by the stream's end")
        size = struct.unpack_from("<I", stream, pos)[0]
        if pos + 4 + size > len(stream):
            raise FormatError("size word %d runs past the stream" % size)
        blocks.append(stream[pos:pos + 4 + size])
        pos += 4 + size
    return blocks


def decode_stats(stream, mini_match, hw_buff_sz):
    """-> (bytes, [per-block statistics])"""
    out, stats = [], []
    blocks = split(bytes(stream))
    for i, b in enumerate(blocks):
        data, st = decode_block(b[4:], mini_match)
        if len(data) == 0:
            raise FormatError("block %d is empty" % i)
        if len(data) > hw_buff_sz or (i + 1 < len(blocks) and len(data) != hw_buff_sz):
            raise FormatError("block %d decodes to %d bytes (hw_buff_sz %d)" % (i, len(data), hw_buff_sz))
        out.append(data)
        stats.append(st)
    return b"".join(out), stats


def decode(stream, mini_match, hw_buff_sz):
    return decode_stats(stream, mini_match, hw_buff_sz)[0]


def bound(n, hw_buff_sz):
    """qzMaxCompressedLength of an LZ4s session: the sum over the call's chunks of 4 + c + c/255 + 4*ceil(c/65535) + 16"""
    total = 0
    pos = 0
    while pos < n:
        c = min(hw_buff_sz, n - pos)
        total += 4 + c + c // 255 + 4 * ((c + 65534) // 65535) + 16
        pos += c
    return total
