"""The zstd kernel (qatzip_amd/csrc/qzk_zstd.h: K4s's parse with the record emitter, then the entropy stage) on the CPU SIMT
emulator.  Every frame is read by the strict reader of tests/zstd_format.py and, where libzstd loads, by ZSTD_decompress
(tests/zstd_ref.py); where it does not, the pinned index - made where it did - carries that check.

Left as the issue words them but not reachable, each replaced by the nearest thing that is:
  * "b'A' * 131072 ... all three modes RLE": the LZ4s parse gives (1, 65535, 1), (0, 65532, 1), (0, 4, 1) - the sequences are
    the LZ4s session's by contract, so only the offsets share a code; asserted: matches of 65535, OF in RLE_Mode, a frame
    under 64 bytes;
  * a Raw literals section of 0 bytes: a frame's first match needs a byte to copy, so records without literals are refused;
  * a literal length of 131071: with its match of three it needs 131074 bytes of content, above 128 KB - refused; 131069, the
    longest that fits, is coded."""
import hashlib

import pytest

import lz4s_format
import lz4s_sim
import zstd_format as Z
import zstd_ref
import zstd_sim as S

KINDS = ("text", "records", "silesia", "lzmix", "runs", "mod200", "rand", "allA")
SIZES = (1, 2, 3, 4, 5, 12, 13, 63, 64, 65, 4095, 65535, 65536)


def _read(stream, src, hw):
    """both readers; -> the strict reader's frames"""
    frames = Z.decode_frames(stream)
    assert b"".join(f["data"] for f in frames) == src
    for i, f in enumerate(frames):
        assert f["content_size"] == min(hw, len(src) - i * hw)
        assert f["size"] <= f["content_size"] + 12
    zstd_ref.check(stream, src)
    return frames


@pytest.mark.parametrize("mm", (3, 4))
@pytest.mark.parametrize("kind", KINDS)
def test_round_trip(kind, mm):
    for n in SIZES:
        src = S.make_input(kind, n, 11)
        got, lens = S.compress(src, 65536, mm)
        frames = _read(got, src, 65536)
        assert [f["size"] for f in frames] == lens and sum(lens) == len(got)


@pytest.mark.parametrize("dist", (65535, 65536))
def test_far_offsets(dist):
    src = lz4s_sim.far_input(dist)
    got, _ = S.compress(src, 131072, 3)
    f = _read(got, src, 131072)[0]
    assert f["block"] == "compressed"
    offs = [o for _, _, o in f["sequences"]]
    assert max(offs) <= 65535
    if dist == 65535:
        assert 65535 in offs
    assert f["sequences"] == S.expected_sequences(src, 131072, 3)[0]


def test_merged_literal_length_takes_code_35():
    src = S.merged_input()
    got, _ = S.compress(src, 131072, 3)
    f = _read(got, src, 131072)[0]
    assert f["block"] == "compressed"
    assert max(ll for ll, _, _ in f["sequences"]) > 65535
    assert Z.ll_code(max(ll for ll, _, _ in f["sequences"])) == 35
    assert f["sequences"] == S.expected_sequences(src, 131072, 3)[0]


def test_all_a():
    src = b"A" * 131072
    got, _ = S.compress(src, 131072, 3)
    f = _read(got, src, 131072)[0]
    assert max(ml for _, ml, _ in f["sequences"]) == 65535
    assert f["seq"]["modes"][1] == 1 and all(o == 1 for _, _, o in f["sequences"])
    assert len(got) < 64


def _pinned_inputs():
    for c in S.index()["cases"]:
        yield c, S.make_input(c["kind"], c["n"], c["seed"])


def test_pin_and_same_sequences():
    """the emulator reproduces every pinned case, and the reader's sequence list is what decLz4Block's rule yields from the
    LZ4s session's stream for the same input (frames whose block is Raw have none to compare)"""
    cases = S.index()["cases"]
    assert len(cases) >= 20
    compared = 0
    for c, src in _pinned_inputs():
        assert hashlib.sha256(src).hexdigest() == c["in_sha"]
        got, _ = S.compress(src, c["hw_buff_sz"], c["mini_match"])
        assert (len(got), hashlib.sha256(got).hexdigest()) == (c["out_len"], c["out_sha"]), c
        frames = _read(got, src, c["hw_buff_sz"])
        want = S.expected_sequences(src, c["hw_buff_sz"], c["mini_match"])
        assert len(want) == len(frames)
        for f, w in zip(frames, want):
            if f["block"] == "compressed":
                assert f["sequences"] == w, c
                compared += 1
    assert compared >= 20


def test_chunks_are_independent():
    src = S.make_input("silesia", 5 * 16384 - 100, 3)
    whole, lens = S.compress(src, 16384, 3)
    parts = [S.compress(src[i:i + 16384], 16384, 3)[0] for i in range(0, len(src), 16384)]
    assert len(parts) == 5 and b"".join(parts) == whole and [len(p) for p in parts] == lens
    assert S.compress(src, 16384, 3, waves=1)[0] == whole
    src = S.make_input("lzmix", 8 * 4096, 4)
    assert S.compress(src, 4096, 4, waves=1)[0] == S.compress(src, 4096, 4, waves=8)[0]


# ---------------------------------------------------------------- the entropy stage alone
@pytest.fixture(scope="module")
def edges():
    """every edge frame through sim_zstd_encode once: name -> (frame, the reader's info, the stream)"""
    out = {}
    names = sorted(S.EDGES)
    rc, stream, lens = S.encode([S.EDGES[k] for k in names])
    assert rc == 0
    pos = 0
    for k, ln in zip(names, lens):
        one = stream[pos:pos + ln]
        pos += ln
        f, end = Z.decode_frame(one)
        assert end == ln
        data = S.rebuild(S.EDGES[k])
        assert f["data"] == data and f["content_size"] == S.EDGES[k][0], k
        zstd_ref.check(one, data)
        assert ln <= len(data) + 12
        out[k] = (S.EDGES[k], f, one)
    return out


def test_edges_keep_their_records(edges):
    for k, (frame, f, _) in edges.items():
        assert f["block"] == "compressed", k
        assert f["sequences"] == frame[1], k


def test_edges_one_frame_alone_gives_the_same_bytes(edges):
    for k in ("count128", "huf1024", "top129"):
        rc, stream, _ = S.encode([S.EDGES[k]])
        assert rc == 0 and stream == edges[k][2]


def test_sequence_count_forms(edges):
    for k, n in (("count0", 0), ("count1", 1), ("count127", 127), ("count128", 128), ("count7eff", 0x7eff), ("count7f00", 0x7f00)):
        assert edges[k][1]["seq"]["count"] == n
    # every record of many() has the same three codes
    assert edges["count128"][1]["seq"]["modes"] == (1, 1, 1)


def test_literals_types_and_size_formats(edges):
    def lit(k):
        return edges[k][1]["literals"]
    for k, n, hs in (("raw31", 31, 1), ("raw32", 32, 2), ("raw4095", 4095, 2), ("raw4096", 4096, 3)):
        assert lit(k)["type"] == "raw" and lit(k)["regen"] == n and lit(k)["size"] == n + hs
    for k, streams in (("huf1023", 1), ("huf1024", 4), ("huf16383", 4), ("huf16384", 4)):
        assert lit(k)["type"] == "compressed" and lit(k)["streams"] == streams and lit(k)["size"] < lit(k)["regen"]
    assert lit("rle")["type"] == "rle" and lit("rle")["size"] == 3
    assert lit("two")["type"] == "compressed" and lit("two")["maxbits"] == 1
    assert lit("uniform256")["type"] == "raw"
    assert lit("fibonacci")["type"] == "compressed" and lit("fibonacci")["maxbits"] == 11
    for k, d in (("top127", "direct"), ("top128", "direct"), ("top129", "fse"), ("top255", "fse")):
        assert lit(k)["type"] == "compressed" and lit(k)["description"] == d, k


def test_length_and_offset_codes(edges):
    for k, ml in (("ml3", 3), ("ml4", 4), ("ml34", 34), ("ml35", 35), ("ml65535", 65535)):
        assert edges[k][1]["sequences"][0][1] == ml
    assert [Z.ml_code(m) for m in (3, 4, 34, 35, 65535)] == [0, 1, 31, 32, 51]
    for k, ll in (("ll15", 15), ("ll16", 16), ("ll63", 63), ("ll64", 64), ("ll65535", 65535), ("ll65536", 65536), ("ll131069", 131069)):
        assert edges[k][1]["sequences"][0][0] == ll
    assert [Z.ll_code(v) for v in (15, 16, 63, 64, 65535, 65536, 131069)] == [15, 16, 24, 25, 34, 35, 35]
    assert edges["off1"][1]["sequences"][0][2] == 1 and edges["off5"][1]["sequences"][0][2] == 5
    assert edges["ll65535"][1]["sequences"][0][2] == 65535


@pytest.mark.parametrize("name", sorted(S.REFUSED))
def test_refusals(name):
    frame, want = S.REFUSED[name]
    rc, stream, _ = S.encode([frame])
    assert rc == want and stream == b""


def test_a_refused_frame_refuses_the_call():
    rc, stream, _ = S.encode([S.EDGES["count1"], S.REFUSED["match2"][0], S.EDGES["rle"]])
    assert rc == S.ERR_DATA and stream == b""


# ---------------------------------------------------------------- the reader
def _frame(block, content, btype=2):
    fhd, fcs = (0x20, bytes([content])) if content < 256 else (0x60, (content - 256).to_bytes(2, "little"))
    return Z.MAGIC + bytes([fhd]) + fcs + (1 | btype << 1 | len(block) << 3).to_bytes(3, "little") + block


def test_reader_is_strict(edges):
    """one hand-built bad frame per rule of the reader's list"""
    def bad(buf, word):
        with pytest.raises(Z.FormatError, match=word):
            Z.decode_frame(bytes(buf))
    lits = bytes([5 << 3]) + b"abcde"                               # five Raw literals
    # one sequence (5, 30, 2), all three tables RLE: LL code 5, OF code 2 (value 5 = 4 + 1), ML code 27; the stream holds the
    # offset's two extra bits (01) and the end mark: 0b101
    seqs = bytes([1, 0x54, 5, 2, 27, 0b101])
    good = _frame(lits + seqs, 35)
    f, _ = Z.decode_frame(good)
    assert f["data"] == b"abcde" + b"de" * 15 and f["sequences"] == [(5, 30, 2)]
    zstd_ref.check(good, f["data"])
    b = bytearray(good); b[4] |= 0x08; bad(b, "reserved bit")
    bad(_frame(lits + bytes([1, 0x55, 5, 2, 27, 0b101]), 35), "reserved bits in the modes")
    bad(_frame(bytes([0 | 1 << 2 | 5 << 4, 0]) + b"abcde" + seqs, 35), "wrong size format")
    bad(Z.MAGIC + bytes([0xa0]) + (35).to_bytes(4, "little") + good[6:], "wrong size format")
    bad(_frame(lits + bytes([0x80, 1, 0x54, 5, 2, 27, 0b101]), 35), "wrong size format")
    # Huffman: weights 1, 1, 1 (sum 3, then an implied one to 4 - fine) against 2, 1, 1, 1 (sum 5: 3 missing to 8)
    hdr = lambda n, c: (2 | n << 4 | c << 14).to_bytes(3, "little")
    bad(_frame(hdr(4, 4) + bytes([127 + 4, 0x21, 0x11, 0x01]) + seqs, 35), "power of two")
    # twelve bits: weights 12, 11, 10 ... 1 and the implied last 1
    w = [12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1]
    packed = bytes(w[i] << 4 | w[i + 1] for i in range(0, 12, 2))
    bad(_frame(hdr(4, 8) + bytes([127 + 12]) + packed + b"\x01" + seqs, 35), "12 bits")
    # a stream without its end mark, and one with bits left over
    bad(_frame(lits + bytes([1, 0x54, 5, 2, 27, 0]), 35), "end mark")
    bad(_frame(lits + bytes([1, 0x54, 5, 2, 27, 0b1101]), 35), "left over")
    huf = edges["two"][2]
    f2 = edges["two"][1]
    cut = bytearray(huf); cut[f2["header_size"] + 3 + f2["literals"]["size"] - 1] = 0
    bad(cut, "end mark")
    # an FSE symbol past its table
    bad(_frame(lits + bytes([1, 0x54, 36, 2, 27, 0b101]), 35), "out of range")
    bad(_frame(lits + bytes([1, 0x54, 5, 2, 53, 0b101]), 35), "out of range")
    # an offset beyond the produced bytes: OF code 3, value 8 + 0 = offset 5 ... + 1 = offset 6 with 5 bytes there
    bad(_frame(lits + bytes([1, 0x54, 5, 3, 27, 0b1001]), 35), "bytes produced")
    # content size disagreement
    bad(_frame(lits + seqs, 36), "content size")
    bad(_frame(b"abc", 4, btype=0), "content size")
    # outside the subset
    bad(_frame(lits + bytes([1, 0x94, 5, 2, 27, 0b101]), 35), "outside the subset")
    bad(_frame(lits + bytes([1, 0x54, 5, 1, 27, 0b11]), 35), "repeat offset")
    bad(_frame(bytes([3]) + seqs, 35), "treeless")
    b = bytearray(good); b[4] |= 0x04; bad(b, "checksum")
    b = bytearray(good); b[6] &= 0xfe; bad(b, "more than one block")


# ---------------------------------------------------------------- ratio
def test_ratio():
    idx = S.index()
    for r in idx["ratio"]:
        src = S.make_input(r["kind"], r["n"], r["seed"])
        assert hashlib.sha256(src).hexdigest() == r["in_sha"]
        got, lens = S.compress(src, 65536, 3)
        frames = Z.decode_frames(got)
        print(r["kind"], "zstd", len(got), "lz4s", r["lz4s_len"], "libzstd level 1", r["libzstd_level1"], "compressSequences",
              r["libzstd_compress_sequences"], "ratio", r["ratio"])
        assert all(ln <= 65536 + 12 for ln in lens)
        assert len(got) < len(src)
        assert len(got) == r["zstd_len"]
        for f in frames:
            lt = f["literals"]
            if lt and lt["type"] == "compressed":
                raw = lt["regen"] + (1 if lt["regen"] < 32 else 2 if lt["regen"] < 4096 else 3)
                assert lt["size"] <= raw
                if r["kind"] == "text":
                    assert lt["size"] < lt["regen"]
        if r["kind"] == "text":
            assert any(f["literals"] and f["literals"]["type"] == "compressed" for f in frames)
        base = r["libzstd_compress_sequences"] or r["libzstd_level1"]
        assert len(got) / base <= r["cap"]
        lz4s, _ = lz4s_sim.compress(src, 65536, 3)
        assert len(lz4s) == r["lz4s_len"]


# ---------------------------------------------------------------- the host side under a sanitizer
def test_host_side_under_sanitizers(tmp_path):
    """tests/sim/sim_zstd.cpp as a program of its own (SIM_ZSTD_MAIN): the bound, the frame descriptions of encode_frames and
    the scan over frame lengths - qzd_zstd_host.h, the lines the device layer runs - on the edge list, built with
    -fsanitize=address,undefined.  A stand-alone program: nothing here is loaded into python."""
    import os
    import subprocess
    exe = str(tmp_path / "sim_zstd_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DSIM_ZSTD_MAIN", "-I", S.SIMDIR, "-Wno-unused-function", "-o", exe, os.path.join(S.SIMDIR, "sim_zstd.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr
