#!/usr/bin/env python3
"""Writes tests/golden/zstd_dec_corrupt/: hand-built frames from tests/zstd_hand_writer.py - the corners of RFC 8878 that no
compressor at hand produces - and index.json: per frame the recipe, the content's SHA-256, the feature tally of
tests/zstd_full_format.py, libzstd's verdict and the decoder's {status, in_used, out_len} on the emulator; the classes of
strictness the corruption sweep sees (tests/test_sim_zstdd_corrupt.py) and the sample of mutants the GPU test runs
(tests/test_gpu_zstdd_corrupt.py).  Run where libzstd loads (written with 1.4.8).

A frame is "ok" when the strict reader, libzstd and the decoder agree on its bytes, and a "refusal" when the decoder and the
strict reader refuse it; libzstd's verdict on a refusal is recorded, not required."""
import collections
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import zstd_format  # noqa: E402
import zstd_full_format as zf  # noqa: E402
import zstd_hand_writer as W  # noqa: E402
import zstd_ref  # noqa: E402

OUT = os.path.join(HERE, "zstd_dec_corrupt")
MAXBLK = 131072
# what the union of the tallies must hold (tests/test_sim_zstdd_corrupt.py asserts it of the committed index)
REQUIRED = (["hufbits:2", "hufbits:3", "hufbits:4", "hufbits:8", "weights:direct128", "wlog:5", "wlog:6", "lit:stream4:0",
             "lit:stream4:1", "lit:1stream:1", "lit:treeless<raw<huffman", "tablelog:ll:5", "tablelog:ll:9", "tablelog:ml:5", "tablelog:ml:9", "tablelog:of:5",
             "tablelog:of:8", "ncount:lessthan1", "ncount:zrun:1", "ncount:zrun:3", "ncount:zrun:4", "ncount:zrun:7", "ncount:lastbits:8",
             "ncount:lastbits:1", "repeat<nseq0<rle", "repeat<nseq0<predefined", "repeat<nseq0<fse", "block:raw:empty-last",
             "block:rle:1", "block:rle:max", "block:compressed:max", "block:at-window", "window:mantissa", "content:255",
             "content:256", "content:65791", "content:65792", "seq0:ll1:ml3:off1", "offset:all-produced"])
REQUIRED_REFUSALS = ["compressed_max_plus_1", "window_block_plus_1", "offset_all_produced_plus_1", "repeat3_ll0_rep1_later_block",
                     "huffman_no_weight_1_w3", "huffman_no_weight_1_w5", "huffman_no_weight_1_w9"]


def execute(parts, history=b""):
    """what blocks of (literals, [(ll, ml, Offset_Value)]) regenerate, repeat offsets by RFC 8878, 3.1.1.5"""
    out, rep = bytearray(history), [1, 4, 8]
    for lits, seqs in parts:
        lp = 0
        for ll, ml, ov in seqs:
            out += lits[lp:lp + ll]
            lp += ll
            if ov > 3:
                rep = [ov - 3, rep[0], rep[1]]
            else:
                i = ov - 1 + (ll == 0)
                if i == 1:
                    rep = [rep[1], rep[0], rep[2]]
                elif i == 2:
                    rep = [rep[2], rep[0], rep[1]]
                elif i == 3:
                    rep = [rep[0] - 1, rep[0], rep[1]]
            for _ in range(ml):
                out.append(out[-rep[0]])
        out += lits[lp:]
    return bytes(out)


def cblock(lit_section, seq_section, last=True):
    return W.block("compressed", lit_section + seq_section, last)


def small_frame(blocks, content):
    """Single_Segment where every block fits the content (the window, then); else a Window_Descriptor of 1 KB and a 4-byte
    Frame_Content_Size: a tiny Compressed block is larger than what it regenerates"""
    if max(len(b) - 3 for b in blocks) <= content:
        return W.frame(blocks, content)
    return W.frame(blocks, content, fcs_bytes=4, window_byte=0x00)


def huf_frame(weights, lits, tree, streams=1, seqs=None):
    """one Compressed block: Huffman literals of the listed weights (the last one is implied) and one or no sequence"""
    allw = list(weights) + [W.last_weight(weights)]
    seqs = [] if seqs is None else seqs
    data = execute([(lits, seqs)])
    return small_frame([cblock(W.literals("huffman", lits, allw, tree, streams), W.sequences(seqs))], len(data)), data


def spread(nsym, n):
    return bytes((i * 7) % nsym for i in range(n))


def find_ncount(want_lastbits):
    """the first LL distribution (three counts, accuracy 5 to 7) whose description ends with that many bits in its last byte"""
    for log in (5, 6, 7):
        size = 1 << log
        for a in range(1, size - 1):
            for b in range(1, size - a):
                norm = [a, b, size - a - b]
                if (W.ncount(norm, log)[1] - 1) % 8 + 1 == want_lastbits:
                    return norm, log
    raise AssertionError(want_lastbits)


def hand_frames():
    """-> [(name, frame, data or None for a refusal, content for out_cap, recipe)]"""
    F = []

    def ok(name, frame, data, recipe):
        F.append((name, frame, data, len(data), recipe))

    def bad(name, frame, content, recipe):
        F.append((name, frame, None, content, recipe))

    # ---- Huffman and literals
    for bits, w in ((2, [2, 1]), (3, [3, 2, 1]), (4, [4, 3, 2, 1]), (8, [8, 7, 6, 5, 4, 3, 2, 1])):
        lits = spread(len(w) + 1, 40)
        fr, data = huf_frame(w, lits, W.tree_direct(w), seqs=[(30, 5, 9)])
        ok("huf_%dbit" % bits, fr, data, "direct weights %s and the implied one, 40 literals in one stream, one match of 5 at offset 6" % w)
    w = [1] * 128
    lits = bytes(range(129)) + bytes([128]) * 20
    fr, data = huf_frame(w, lits, W.tree_direct(w))
    ok("weights_direct_128", fr, data, "128 direct weights of 1 (header byte 255), the implied 129th symbol has weight 8; no sequences")
    w = [1, 1, 2, 3, 4]
    for log, norm in ((5, [8, 8, 8, 4, 4]), (6, [16, 16, 16, 8, 8])):
        fr, data = huf_frame(w, spread(6, 30), W.tree_fse(w, norm, log), seqs=[(10, 4, 7)])
        ok("weights_fse_log%d" % log, fr, data, "weights %s FSE-coded with counts %s at accuracy %d" % (w, norm, log))
    w = [3, 2, 1]
    for n in (6, 7):
        fr, data = huf_frame(w, spread(4, n), W.tree_direct(w), streams=4)
        ok("four_streams_%d" % n, fr, data, "%d literals in four streams: the fourth holds %s" % (n, "only its end mark" if n == 6 else "one literal"))
    fr, data = huf_frame(w, b"\x02", W.tree_direct(w))
    ok("one_stream_1", fr, data, "one literal in one stream")
    allw = w + [W.last_weight(w)]
    parts = [(spread(4, 12), [(8, 4, 6)]), (b"wxyz", [(2, 3, 1)]), (spread(4, 9)[::-1], [(5, 6, 20)])]
    blocks = [cblock(W.literals("huffman", parts[0][0], allw, W.tree_direct(w)), W.sequences(parts[0][1]), False),
              cblock(W.literals("raw", parts[1][0]), W.sequences(parts[1][1]), False),
              cblock(W.literals("treeless", parts[2][0], allw), W.sequences(parts[2][1]), True)]
    data = execute(parts)
    ok("treeless_after_raw_after_huffman", W.frame(blocks, len(data)), data, "three Compressed blocks: Huffman, Raw, Treeless literals")
    # ---- sequence tables
    seqs = [(2, 4, 5), (1, 3, 6), (0, 5, 4), (2, 3, 7), (1, 4, 5), (0, 3, 1)]        # LL codes 0-2, ML codes 0-2, OF codes 0, 2
    lits = b"abcdefgh"
    data = execute([(lits, seqs)])

    def table_frame(name, ll, of, ml, recipe, use=seqs):
        d = execute([(lits, use)])
        ok(name, small_frame([cblock(W.literals("raw", lits), W.sequences(use, ll, of, ml))], len(d)), d, recipe)

    table_frame("tables_log_smallest", ("fse", [16, 8, 8], 5), ("fse", [8, 8, 16], 5), ("fse", [8, 8, 16], 5),
                "FSE_Compressed tables at accuracy 5 / 5 / 5")
    table_frame("tables_log_largest", ("fse", [256, 128, 128], 9), ("fse", [64, 64, 128], 8), ("fse", [128, 128, 256], 9),
                "FSE_Compressed tables at accuracy 9 / 8 / 9")
    table_frame("table_less_than_1", ("fse", [16, 8, 7, -1], 5), ("fse", [-1, 7, 24], 5), ("predefined",),
                "LL and OF descriptions with a 'less than 1' probability")
    runs = [(6, 6, 4), (0, 3, 4), (2, 4, 4), (11, 3, 4), (22, 5, 4), (0, 3, 4)]      # LL codes 6, 0, 2, 11, 19, 0
    big = bytes(range(65, 65 + 42))
    d = execute([(big, runs)])
    ok("table_zero_runs", W.frame([cblock(W.literals("raw", big), W.sequences(
        runs, ("fse", [8, 0, 8, 0, 0, 0, 4, 0, 0, 0, 0, 4, 0, 0, 0, 0, 0, 0, 0, 8], 5), ("rle", 2), ("predefined",)))], len(d)), d,
       "an LL description with zero-probability runs of 1, 3, 4 and 7 symbols")
    for lastbits, tag in ((8, "byte_boundary"), (1, "one_bit")):
        norm, log = find_ncount(lastbits)
        table_frame("table_ends_%s" % tag, ("fse", norm, log), ("predefined",), ("predefined",),
                    "an LL description %s at accuracy %d: %d bits in its last byte" % (norm, log, lastbits))
    specs = {"rle": [("rle", 1), ("rle", 2), ("rle", 1)], "predefined": [("predefined",)] * 3,
             "fse": [("fse", [16, 8, 8], 5), ("fse", [8, 8, 16], 5), ("fse", [8, 8, 16], 5)]}
    again = {"rle": [("repeat", 1), ("repeat", 2), ("repeat", 1)], "predefined": [("repeat",) + W.PREDEFINED[k] for k in ("LL", "OF", "ML")],
             "fse": [("repeat",) + s[1:] for s in specs["fse"]]}
    for kind in ("rle", "predefined", "fse"):
        use = [(1, 4, 4), (1, 4, 5), (1, 4, 6)] if kind == "rle" else seqs
        parts = [(lits, use), (b"--", []), (lits, use)]
        blocks = [cblock(W.literals("raw", lits), W.sequences(use, *specs[kind]), False),
                  cblock(W.literals("raw", b"--"), W.sequences([]), False),
                  cblock(W.literals("raw", lits), W.sequences(use, *again[kind]), True)]
        d = execute(parts)
        ok("repeat_after_%s" % kind, W.frame(blocks, len(d)), d, "Repeat_Mode for LL, OF and ML after %s tables, a block without sequences in between" % kind)
    # ---- blocks and frames
    ok("empty_raw_last", W.frame([W.block("raw", b"abc"), W.block("raw", b"", True)], 3), b"abc", "a Raw block of 3 bytes, then an empty Raw last block")
    ok("rle_block_1", W.frame([W.block("rle", b"Q", True, 1)], 1), b"Q", "an RLE block of 1 byte")
    ok("rle_block_max", W.frame([W.block("rle", b"Q", True, MAXBLK)], MAXBLK), b"Q" * MAXBLK, "an RLE block of Block_Maximum_Size")
    for extra, name in ((0, "compressed_max"), (1, "compressed_max_plus_1")):
        s = [(1, MAXBLK - 1 + extra, 4)]
        fr = W.frame([cblock(W.literals("rle", b"A", regen=1), W.sequences(s))], MAXBLK + extra)
        if extra:
            bad(name, fr, MAXBLK + 1, "a Compressed block that regenerates Block_Maximum_Size + 1: one literal and a match of 131072 at offset 1")
        else:
            ok(name, fr, b"A" * MAXBLK, "a Compressed block that regenerates exactly Block_Maximum_Size: one literal and a match of 131071 at offset 1")
    body = bytes(i * 31 & 255 for i in range(1153))
    ok("window_block", W.frame([W.block("raw", body[:1152], True)], window_byte=0x01), body[:1152],
       "Window_Descriptor 0x01 (1 KB + 1/8: 1152 bytes) and a Raw block of 1152")
    bad("window_block_plus_1", W.frame([W.block("raw", body, True)], window_byte=0x01), 1153, "Window_Descriptor 0x01 (1152 bytes) and a Raw block of 1153")
    for n in (255, 256, 65791, 65792):
        ok("content_%d" % n, W.frame([W.block("rle", b"c", True, n)], n), b"c" * n, "Frame_Content_Size %d in its smallest field, one RLE block" % n)
    s = [(1, 3, 4)]
    ok("match3_offset1_first", small_frame([cblock(W.literals("raw", b"m"), W.sequences(s))], 4), execute([(b"m", s)]),
       "a block's first sequence: literal length 1, a match of 3 at offset 1")
    s = [(4, 4, 7)]
    ok("offset_all_produced", small_frame([cblock(W.literals("raw", b"abcd"), W.sequences(s))], 8), execute([(b"abcd", s)]), "an offset equal to the 4 bytes produced so far")
    bad("offset_all_produced_plus_1", small_frame([cblock(W.literals("raw", b"abcd"), W.sequences([(4, 4, 8)]))], 8), 8, "an offset of 5 with 4 bytes produced")
    blocks = [cblock(W.literals("raw", b"m"), W.sequences([(1, 3, 4)]), False), cblock(W.literals("raw", b""), W.sequences([(0, 3, 3)]), True)]
    bad("repeat3_ll0_rep1_later_block", small_frame(blocks, 7), 7, "block 1 leaves the first repeat offset at 1; block 2 begins with repeat code 3 and literal length 0: offset 0")
    # ---- the finding: a tree of two one-bit codes without a symbol of weight 1
    for wt in (3, 5, 9):
        lits = bytes([0, 1] * 20)
        tree = W.tree_direct([wt])
        codes = {0: (0, 1), 1: (1, 1)}
        body = tree + W.huffman_stream(codes, lits)
        sec = (2 | 0 << 2 | len(lits) << 4 | len(body) << 14).to_bytes(3, "little") + body
        bad("huffman_no_weight_1_w%d" % wt, small_frame([cblock(sec, W.sequences([]))], len(lits)), len(lits),
            "one direct weight of %d: the implied symbol gets %d too, two one-bit codes and no symbol of weight 1 (libzstd's HUF_readStats refuses it)" % (wt, wt))
    return F


def verdict(frame, cap):
    try:
        return "ok", zstd_ref.decompress(frame, cap)
    except ValueError as e:
        return str(e).split(": ", 1)[1], None


def main():
    assert zstd_ref.available(), "libzstd is needed to generate"
    import zstdd_sim
    os.makedirs(OUT, exist_ok=True)
    for f in os.listdir(OUT):
        os.remove(os.path.join(OUT, f))
    entries = []
    for name, frame, data, content, recipe in hand_frames():
        e = {"name": name, "file": name + ".zst", "size": len(frame), "recipe": recipe, "kind": "ok" if data is not None else "refusal",
             "content": content}
        lib, lib_data = verdict(frame, content + 64)
        res, outs = zstdd_sim.decode_frames([frame], [content + 64])
        e["libzstd"], e["sim"] = lib, list(res[0])
        try:
            info, end = zf.decode_frame(frame)
            assert data is not None, "the strict reader accepts the refusal " + name
            assert end == len(frame) and info["data"] == data, name
            assert lib == "ok" and lib_data == data, (name, lib)
            assert res[0] == (0, len(frame), len(data)) and outs[0] == data, (name, res[0])
            e.update(sha256=hashlib.sha256(data).hexdigest(), tally=info["tally"])
        except zstd_format.FormatError as ex:
            assert data is None, (name, str(ex))
            assert res[0][0] != 0 and res[0][1:] == (0, 0), (name, res[0])
            e["reader"] = str(ex)
        with open(os.path.join(OUT, e["file"]), "wb") as f:
            f.write(frame)
        entries.append(e)
    union = set(t for e in entries for t in e.get("tally", []))
    assert not [t for t in REQUIRED if t not in union], [t for t in REQUIRED if t not in union]
    assert not [n for n in REQUIRED_REFUSALS if n not in [e["name"] for e in entries if e["kind"] == "refusal"]]
    index = {"libzstd": zstd_ref.version(), "required": REQUIRED, "required_refusals": REQUIRED_REFUSALS, "frames": entries}
    with open(os.path.join(OUT, "index.json"), "w") as f:
        json.dump(index, f, indent=1)
    # ---- the sweep's classes of strictness and the GPU sample, from the frames just written
    import zstdd_mutate as S
    sweep = S.run(progress=True)
    kinds = collections.Counter(v.split(": ", 1)[1] for v in sweep["violations"])
    assert not sweep["violations"], (sorted(kinds.items()), sweep["violations"][:10])
    index["classes"] = sorted(sweep["classes"])
    sample = S.gpu_sample(sweep)
    with tempfile.TemporaryDirectory() as tmp:
        S.sanitizer_run(tmp, sample)                       # a mutant enters the sample only if the sanitizer build ran it clean
    index["sample"] = sample
    with open(os.path.join(OUT, "index.json"), "w") as f:
        json.dump(index, f, indent=1)
    print("%d frames, %d bytes; %d mutants in %.0f s; %d classes; %d sampled" % (
        len(entries), sum(e["size"] for e in entries), sweep["total"], sweep["seconds"], len(index["classes"]), len(sample)))


if __name__ == "__main__":
    main()
