"""A small writer of LZ4 frames (lz4_Frame_format.md) for tests: the header with any FLG / BD / content size / dictID, block
words, stored or given block bodies, block checksums, end mark, content checksum - every part can be left out or damaged.
It plays the role tests/deflate_writer.py plays for deflate.  XXH32 comes from the oracle (oracle_lib.lib().qzo_xxh32)."""
import struct

import oracle_lib

MAGIC = 0x184D2204
BLOCK_MAX = {4: 1 << 16, 5: 1 << 18, 6: 1 << 20, 7: 1 << 22}


def xxh32(b):
    b = bytes(b)
    return oracle_lib.lib().qzo_xxh32(b, len(b), 0)


def header(block_id=4, independent=True, block_checksum=False, content_size=None, content_checksum=False, dict_id=None,
           flg=None, bd=None):
    """magic, FLG, BD, the optional fields and the header checksum.  flg / bd, when given, are written as they are"""
    if flg is None:
        flg = 0x40 | (0x20 if independent else 0) | (0x10 if block_checksum else 0) | (0x08 if content_size is not None else 0) | \
              (0x04 if content_checksum else 0) | (0x01 if dict_id is not None else 0)
    if bd is None:
        bd = block_id << 4
    desc = bytes([flg, bd])
    if flg & 0x08:
        desc += struct.pack("<Q", content_size or 0)
    if flg & 0x01:
        desc += struct.pack("<I", dict_id or 0)
    return struct.pack("<I", MAGIC) + desc + bytes([(xxh32(desc) >> 8) & 0xff])


def block(body, stored=False, checksum=False, checksum_xor=0):
    """block word, body and - if asked for - XXH32 of the body as it stands in the frame (xor checksum_xor: a damaged one)"""
    out = struct.pack("<I", len(body) | (0x80000000 if stored else 0)) + bytes(body)
    if checksum:
        out += struct.pack("<I", xxh32(body) ^ checksum_xor)
    return out


def frame(blocks, content=None, end_mark=True, **hdr):
    """blocks: [(body, stored)] or ready-made bytes from block().  content: the decoded bytes - needed for the content
    checksum when content_checksum=True.  Block checksums follow hdr's block_checksum"""
    bc = bool(hdr.get("block_checksum"))
    out = [header(**hdr)]
    for b in blocks:
        out.append(bytes(b) if isinstance(b, (bytes, bytearray)) else block(b[0], b[1], bc))
    if end_mark:
        out.append(struct.pack("<I", 0))
    if hdr.get("content_checksum"):
        out.append(struct.pack("<I", xxh32(content)))
    return b"".join(out)


def literals_block(data):
    """data as ONE compressed block: a single sequence of literals only (what a block's last sequence is)"""
    n = len(data)
    out = bytearray()
    if n < 15:
        out.append(n << 4)
    else:
        out.append(0xf0)
        r = n - 15
        while r >= 255:
            out.append(255); r -= 255
        out.append(r)
    return bytes(out) + bytes(data)


def sequences_block(seqs, last_literals):
    """a compressed block of sequences [(literals, offset, match length >= 4)] and its closing literals (>= 5 bytes for a
    block liblz4 accepts behind a match)"""
    out = bytearray()
    for lits, off, ml in seqs:
        m = ml - 4
        out.append((min(len(lits), 15) << 4) | min(m, 15))
        if len(lits) >= 15:
            r = len(lits) - 15
            while r >= 255:
                out.append(255); r -= 255
            out.append(r)
        out += lits
        out += struct.pack("<H", off)
        if m >= 15:
            r = m - 15
            while r >= 255:
                out.append(255); r -= 255
            out.append(r)
    return bytes(out) + literals_block(last_literals)


def blocks_of(fr):
    """[(word, body offset, body length)] of a frame, and the position behind its end mark"""
    flg = fr[4]
    pos = 7 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0)
    out = []
    while True:
        w = struct.unpack_from("<I", fr, pos)[0]
        pos += 4
        if w == 0:
            return out, pos
        ln = w & 0x7fffffff
        out.append((w, pos, ln))
        pos += ln + (4 if flg & 0x10 else 0)
