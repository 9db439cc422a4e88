#!/usr/bin/env python3
"""Writes tests/golden/zstd_dec/: the frames the zstd decoder is tested on, and index.json - per frame the recipe, the
content's SHA-256, the feature tally of tests/zstd_full_format.py, libzstd's verdict and (where the emulator build of the
decoder is at hand) the decoder's {status, in_used, out_len}.  Run where libzstd loads (written with 1.4.8); the frames are
committed because a GPU box may have no libzstd.

    (a) seventeen libzstd frames: ZSTD_compress2 / ZSTD_compressStream2 over zstd_sim.make_input(kind, n, 11)
    (b) ZSTD_compressSequences on the LZ4s parse (the reference's utils/qzstd.c:251)
    (c) features libzstd did not produce in (a): this project's writer through the emulator, and hand-built headers
    (d) refusals: one frame per cause, each the smallest edit of a frame of (a)-(c) that the strict reader answers with
        that cause - found by trying single-bit edits in the frame's first bytes - and that libzstd refuses too.  A cause
        libzstd accepts is dropped and listed under "dropped" in the index: today "block_above_max" (ZSTD_decompress 1.4.8
        does not compare a block with the window in its one-shot path).
"""
import ctypes as C
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import zstd_format  # noqa: E402
import zstd_full_format as zf  # noqa: E402
import zstd_ref  # noqa: E402
import zstd_sim  # noqa: E402

OUT = os.path.join(HERE, "zstd_dec")
MAX_FILE = 141019

LIBZSTD = [  # kind, n, level, checksum, stream
    ("text", 3073, 1, 0, 0), ("text", 70001, 1, 0, 0), ("text", 70001, 3, 1, 0), ("text", 300000, 19, 1, 0),
    ("records", 262144, 1, 0, 0), ("records", 140000, 19, 0, 0), ("silesia", 300000, 3, 1, 0), ("silesia", 140000, 19, 0, 0),
    ("lzmix", 200000, 3, 0, 1), ("lzmix", 140000, 19, 1, 1), ("runs", 70001, 1, 0, 0), ("mod200", 70001, 3, 0, 0),
    ("rand", 70001, 1, 1, 0), ("allA", 140000, 3, 0, 0), ("allA", 300000, 1, 1, 1), ("text", 140000, -5, 0, 0),
    ("silesia", 300000, 6, 0, 1),
]
# what the union of the tallies of (a) must hold (tests/test_sim_zstdd.py asserts it of the committed index)
REQUIRED_A = (["block:raw", "block:rle", "block:compressed", "lit:raw", "lit:huffman", "lit:treeless", "lit:4streams10",
               "hufbits:7", "hufbits:9", "hufbits:10", "ofcode>16", "fcs:0", "fcs:2", "fcs:4", "checksum", "window"]
              + ["%s:%s" % (t, m) for t in ("ll", "of", "ml") for m in ("predefined", "fse", "repeat")]
              + ["rep:%d:%s" % (c, l) for c in (1, 2, 3) for l in ("ll>0", "ll0")])
REQUIRED_C = ["lit:rle", "weights:direct", "hufbits:11", "ll:rle", "of:rle", "ml:rle", "fcs:1", "nseq0", "llcode35",
              "skippable", "fcs:8", "window+fcs"]


class _Buf(C.Structure):
    _fields_ = [("p", C.c_void_p), ("size", C.c_size_t), ("pos", C.c_size_t)]


def libzstd_frame(src, level, checksum, stream):
    L = zstd_ref.lib()
    L.ZSTD_createCCtx.restype = C.c_void_p
    L.ZSTD_freeCCtx.argtypes = [C.c_void_p]
    L.ZSTD_CCtx_setParameter.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.ZSTD_CCtx_setParameter.restype = C.c_size_t
    L.ZSTD_compress2.restype = C.c_size_t
    L.ZSTD_compress2.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
    L.ZSTD_compressStream2.restype = C.c_size_t
    L.ZSTD_compressStream2.argtypes = [C.c_void_p, C.POINTER(_Buf), C.POINTER(_Buf), C.c_int]
    cctx = L.ZSTD_createCCtx()
    try:
        assert not L.ZSTD_isError(L.ZSTD_CCtx_setParameter(cctx, 100, level))       # ZSTD_c_compressionLevel
        assert not L.ZSTD_isError(L.ZSTD_CCtx_setParameter(cctx, 201, checksum))    # ZSTD_c_checksumFlag
        cap = L.ZSTD_compressBound(len(src)) + 64
        dst = C.create_string_buffer(cap)
        if not stream:
            r = L.ZSTD_compress2(cctx, dst, cap, bytes(src), len(src))
            assert not L.ZSTD_isError(r)
            return dst.raw[:r]
        keep = C.create_string_buffer(bytes(src), len(src))
        ob = _Buf(C.addressof(dst), cap, 0)
        half = len(src) // 2
        for end, op in ((half, 1), (len(src), 2)):                                   # ZSTD_e_flush at half, then ZSTD_e_end
            ib = _Buf(C.addressof(keep), end, 0 if op == 1 else half)
            while True:
                r = L.ZSTD_compressStream2(cctx, C.byref(ob), C.byref(ib), op)
                assert not L.ZSTD_isError(r)
                if r == 0 and ib.pos == ib.size:
                    break
        return dst.raw[:ob.pos]
    finally:
        L.ZSTD_freeCCtx(cctx)


def verdict(frame, cap):
    """libzstd's answer to ONE frame: "ok" or its error's name"""
    try:
        zstd_ref.decompress(frame, cap)
        return "ok"
    except ValueError as e:
        return str(e).split(": ", 1)[1]


def reheader(frame, single, fcs_bytes):
    """the same blocks behind another frame header: Window_Descriptor instead of Single_Segment, another width of
    Frame_Content_Size"""
    h = zf.frame_header(frame)
    content = h["content_size"]
    assert content is not None
    fhd = (frame[4] & 0x04) | (0x20 if single else 0) | ({1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes] << 6)
    out = bytearray(frame[:4]) + bytes([fhd])
    if not single:
        wlog = max(10, (max(content, 1) - 1).bit_length())
        out.append((wlog - 10) << 3)
    out += (content - (256 if fcs_bytes == 2 else 0)).to_bytes(fcs_bytes, "little")
    return bytes(out) + frame[h["header_size"]:]


# (d): cause -> a part of the strict reader's message
CAUSES = {
    "treeless_without_tree": "treeless literals without", "repeat_without_table": "repeats a table that was never set",
    "weights_not_power_of_two": "do not add up to a power of two", "huffman_code_above_11": "a Huffman code of",
    "accuracy_log": "accuracy log",
    "symbol_out_of_range": "out of range for", "no_end_mark": "without its end mark", "bits_left_over": "bits left over",
    "read_past_beginning": "read past its beginning", "huffman_ends_inside_code": "ends inside a code",
    "jump_table": "jump table runs past", "literals_overconsumed": "takes more literals", "repeat_offset_0": "a repeat offset of 0",
    "offset_beyond": "bytes produced", "block_type_3": "block type 3", "reserved_descriptor_bit": "reserved bit in the frame header",
    "fse_description_cut": "cut by its field's end", "fse_too_many_symbols": "a distribution with more than",
}
# causes of the issue's list that no frame can show: read_ncount's largest value of a count is exactly what is left of the
# table (RFC 8878, 4.1.1: the field's width follows the remaining points), so a distribution can neither overshoot nor miss
# its table - the checks stay in the reader and in the kernel, nothing reaches them
UNREACHABLE = ["fse_overshoot", "fse_does_not_fill"]


def hand_block(block):
    """a Single_Segment frame of one Compressed block (Frame_Content_Size 64: the block is refused before it matters)"""
    return bytes.fromhex("28b52ffd2040") + (len(block) << 3 | 5).to_bytes(3, "little") + block


def search_edits(bases, found):
    """single-bit edits of the first bytes of each base frame, each assigned to the first cause still open that the strict
    reader names and libzstd refuses too"""
    for bname, frame, cap in bases:
        for pos in range(5, min(len(frame), 700)):
            if all(c in found for c in CAUSES):
                return
            for bit in range(8):
                m = bytearray(frame)
                m[pos] ^= 1 << bit
                try:
                    zf.decode_frame(bytes(m))
                    continue
                except zstd_format.FormatError as e:
                    msg = str(e)
                for cause, part in CAUSES.items():
                    if cause not in found and part in msg:
                        v = verdict(bytes(m), cap)
                        if v != "ok":
                            found[cause] = (bytes(m), "%s with bit %d of byte %d flipped" % (bname, bit, pos), v, msg)
                        break


def main():
    assert zstd_ref.available(), "libzstd is needed to generate"
    os.makedirs(OUT, exist_ok=True)
    for f in os.listdir(OUT):
        os.remove(os.path.join(OUT, f))
    entries = []

    def add(name, group, frame, recipe, data, wanted=None, lib_verdict=None, reader=None):
        assert len(frame) <= MAX_FILE, (name, len(frame))
        e = {"name": name, "group": group, "file": name + ".zst", "size": len(frame), "recipe": recipe}
        if group != "d":
            info, end = zf.decode_frame(frame)
            assert end == len(frame) and info["data"] == data, name
            e.update(content=len(data), sha256=hashlib.sha256(data).hexdigest(), tally=info["tally"],
                     has_content=info["content_size"] is not None,
                     libzstd=verdict(frame, len(data)) if not info["skippable"] else "ok")
            assert e["libzstd"] == "ok", (name, e["libzstd"])
        else:
            e.update(cause=wanted, libzstd=lib_verdict, reader=reader, content=len(data))
        with open(os.path.join(OUT, e["file"]), "wb") as f:
            f.write(frame)
        entries.append(e)
        return e

    # ---- (a)
    by = {}
    for kind, n, level, checksum, stream in LIBZSTD:
        src = zstd_sim.make_input(kind, n, 11)
        fr = libzstd_frame(src, level, checksum, stream)
        name = "a_%s_%d_L%s%s%s" % (kind, n, str(level).replace("-", "m"), "_cs" if checksum else "", "_st" if stream else "")
        add(name, "a", fr, {"kind": kind, "n": n, "seed": 11, "level": level, "checksum": checksum, "stream": stream}, src)
        by[name] = (fr, src)
    union = set(t for e in entries for t in e["tally"])
    missing = [t for t in REQUIRED_A if t not in union]
    assert not missing, "the libzstd frames no longer hold: %s" % missing
    # ---- (b)
    for kind in ("text", "records"):
        for mm in (3, 4):
            src = zstd_sim.make_input(kind, 70001, 11)
            chunks = zstd_sim.expected_sequences(src, 65536, mm)
            for ci, seqs in enumerate(chunks):
                piece = src[ci * 65536:(ci + 1) * 65536]
                fr = zstd_ref.compress_sequences(piece, seqs)
                assert fr is not None
                add("b_%s_70001_mm%d_c%d" % (kind, mm, ci), "b", fr,
                    {"kind": kind, "n": 70001, "seed": 11, "mini_match": mm, "chunk": ci, "hw_buff_sz": 65536}, piece)
    # ---- (c)
    for edge in ("rle", "two", "fibonacci", "count0", "ml3", "count1", "huf1024", "huf16384", "count128", "count7f00"):
        rc, stream, lens = zstd_sim.encode([zstd_sim.EDGES[edge]])
        assert rc == 0
        add("c_edge_%s" % edge, "c", stream, {"writer": "zstd_sim.encode", "edge": edge}, zstd_sim.rebuild(zstd_sim.EDGES[edge]))
    src = zstd_sim.make_input("merged", 73000, 8)
    stream, lens = zstd_sim.compress(src, 131072, 3)
    add("c_merged", "c", stream, {"writer": "zstd_sim.compress", "kind": "merged", "n": 73000, "seed": 8, "hw_buff_sz": 131072, "mini_match": 3}, src)
    add("c_skippable", "c", (0x184D2A53).to_bytes(4, "little") + (11).to_bytes(4, "little") + b"user data!!", {"hand": "skippable frame, magic 0x184D2A53, 11 bytes"}, b"")
    small, small_src = by["a_text_3073_L1"]
    add("c_fcs8", "c", reheader(small, True, 8), {"hand": "a_text_3073_L1 with an 8-byte Frame_Content_Size"}, small_src)
    add("c_window_fcs", "c", reheader(small, False, 2), {"hand": "a_text_3073_L1 with a Window_Descriptor and a 2-byte Frame_Content_Size"}, small_src)
    union_c = set(t for e in entries for t in e["tally"])
    missing = [t for t in REQUIRED_C if t not in union_c]
    assert not missing, "(c) lacks: %s" % missing
    # ---- (d)
    found, dropped = {}, []
    cs_frame, cs_src = by["a_text_70001_L3_cs"]

    def explicit(cause, frame, how, cap, part=None):
        try:
            zf.decode_frame(frame)
            raise AssertionError("the strict reader accepts " + cause)
        except zstd_format.FormatError as e:
            msg = str(e)
        assert part is None or part in msg, (cause, msg)
        v = verdict(frame, cap)
        if v == "ok":
            dropped.append({"cause": cause, "how": how, "reason": "libzstd accepts it"})
        else:
            found[cause] = (frame, how, v, msg)

    explicit("dictionary_id", small[:4] + bytes([small[4] | 1, 5]) + small[5:], "a_text_3073_L1 with Dictionary_ID_Flag 1 and id 5", 3073)
    explicit("reserved_descriptor_bit", small[:4] + bytes([small[4] | 8]) + small[5:], "a_text_3073_L1 with descriptor bit 3 set", 3073)
    h = zf.frame_header(small)
    hs = h["header_size"]
    explicit("block_type_3", small[:hs] + bytes([small[hs] | 6]) + small[hs + 1:], "a_text_3073_L1, first block's type 3", 3073)
    big = bytes(range(256)) * 8
    explicit("block_above_max", bytes.fromhex("28b52ffd") + bytes([0x00, 0x00]) + (len(big) << 3 | 1).to_bytes(3, "little") + big,
             "a Raw block of 2048 bytes behind a Window_Descriptor of 1 KB", len(big))
    fcs = int.from_bytes(small[5:7], "little")
    explicit("output_beyond_content", small[:5] + (fcs - 1).to_bytes(2, "little") + small[7:], "a_text_3073_L1, content size one less", 3073)
    explicit("output_short_of_content", small[:5] + (fcs + 1).to_bytes(2, "little") + small[7:], "a_text_3073_L1, content size one more", 3074)
    explicit("checksum", cs_frame[:-1] + bytes([cs_frame[-1] ^ 1]), "a_text_70001_L3_cs, last checksum byte changed", 70001)
    explicit("cut_last_byte", small[:-1], "a_text_3073_L1 without its last byte", 3073)
    explicit("cut_in_header", small[:6], "a_text_3073_L1, six bytes", 3073)
    explicit("cut_checksum", cs_frame[:-2], "a_text_70001_L3_cs without two bytes of its checksum", 70001)
    # hand-built blocks: no literals (00), then one sequence with every table in RLE_Mode (modes 0x54; the LL, OF, ML codes) and
    # the stream of its extra bits
    explicit("repeat_offset_0", hand_block(bytes.fromhex("00015400010003")), "hand-built: LL code 0, OF code 1 with extra bit 1 (offset value 3, "
             "literal length 0: rep[0] - 1 = 0), ML code 0", 64, CAUSES["repeat_offset_0"])
    explicit("literals_overconsumed", hand_block(bytes.fromhex("00015405020004")), "hand-built: no literals, one sequence of literal length 5", 64,
             CAUSES["literals_overconsumed"])
    explicit("symbol_out_of_range", hand_block(bytes.fromhex("00015424020004")), "hand-built: RLE_Mode literal length code 36", 64, CAUSES["symbol_out_of_range"])
    explicit("repeat_without_table", hand_block(bytes.fromhex("0001d4020004")), "hand-built: Repeat_Mode for LL in a frame's first block", 64,
             CAUSES["repeat_without_table"])
    explicit("huffman_code_above_11", hand_block(bytes.fromhex("42c00080c00100")), "hand-built: four Huffman literals, direct weights, one weight of 12", 64,
             CAUSES["huffman_code_above_11"])
    # what the corruption sweep found (tests/test_sim_zstdd_corrupt.py): a direct weight of c_edge_two changed from 1 to 3, 5 or
    # 9 - the implied symbol gets the same weight, two one-bit codes and no symbol of weight 1, which HUF_readStats refuses
    with open(os.path.join(OUT, "c_edge_two.zst"), "rb") as f:
        two = f.read()
    assert two[17] == 0x01
    for w in (3, 5, 9):
        explicit("huffman_no_weight_1_w%d" % w, two[:17] + bytes([w]) + two[18:], "c_edge_two with byte 17, among its direct weights, 0x%02x instead of 0x01" % w,
                 900, "without two symbols of weight 1")
    bases = [("a_text_3073_L1", small, 3073)]
    for e in list(entries):
        if e["name"] in ("c_edge_two", "c_edge_fibonacci", "c_edge_ml3", "c_edge_huf1024", "c_edge_count128", "b_text_70001_mm3_c1", "b_records_70001_mm4_c1"):
            with open(os.path.join(OUT, e["file"]), "rb") as f:
                bases.append((e["name"], f.read(), e["content"]))
    search_edits(bases, found)
    for cause in UNREACHABLE:
        dropped.append({"cause": cause, "how": "-", "reason": "no frame can show it: a count's largest value is what is left of the table"})
    for cause in CAUSES:
        if cause not in found:
            dropped.append({"cause": cause, "how": "single-bit edits of %s" % ", ".join(b[0] for b in bases), "reason": "no edit gives it"})
    for cause, (frame, how, v, msg) in sorted(found.items()):
        add("d_" + cause, "d", frame, {"edit": how}, b"\0" * 3100 if "70001" not in how else b"\0" * 70100, wanted=cause, lib_verdict=v, reader=msg)
    # ---- the decoder's own answers on the emulator, pinned for the GPU tests
    try:
        import zstdd_sim
        for e in entries:
            with open(os.path.join(OUT, e["file"]), "rb") as f:
                fr = f.read()
            cap = e["content"] if e["group"] != "d" else e["content"]
            res, out = zstdd_sim.decode_frames([fr], [cap])
            e["sim"] = list(res[0])
            if e["group"] != "d":
                assert res[0] == (0, len(fr), e["content"]) and hashlib.sha256(out[0]).hexdigest() == e["sha256"], (e["name"], res[0])
            else:
                assert res[0][0] != 0, e["name"]
    except ImportError:
        print("no emulator harness: the index carries no 'sim' results")
    with open(os.path.join(OUT, "index.json"), "w") as f:
        json.dump({"libzstd": zstd_ref.version(), "required_a": REQUIRED_A, "required_c": REQUIRED_C, "dropped": dropped, "frames": entries}, f, indent=1)
    total = sum(e["size"] for e in entries)
    print("%d frames, %d bytes, largest %d; refusals: %s; dropped: %s" % (len(entries), total, max(e["size"] for e in entries),
                                                                        sorted(found), [d["cause"] for d in dropped]))


if __name__ == "__main__":
    main()
