"""The LZ4s kernel (qatzip_amd/csrc/qzk_lz4s.h) on the CPU SIMT emulator: every stream is read back by the independent
reader tests/lz4s_format.py, which is strict about everything the format does not allow.  The -m gpu twin is
tests/test_gpu_lz4s.py, which must reproduce the pinned streams of tests/golden/lz4s/index.json byte for byte.

The emulator driver (tests/sim/sim_lz4s.cpp) fills the slots with a pattern and fails the call when a block passes
4 + c + c/255 + 4*ceil(c/65535) + 16 or a byte behind it is touched, so every case here checks the bound as well."""
import hashlib
import json
import os

import pytest

import lz4s_format as F
import lz4s_sim
import refcalls

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "lz4s", "index.json")) as f:
    INDEX = json.load(f)

SIZES = (1, 2, 3, 4, 5, 12, 13, 63, 64, 65, 4095, 65535, 65536)
KINDS = ("text", "records", "silesia", "lzmix", "runs", "mod200", "rand", "allA")


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def roundtrip(src, hw, mm, waves=0):
    got, lens = lz4s_sim.compress(src, hw, mm, waves)
    data, stats = F.decode_stats(got, mm, hw)
    assert data == src
    assert sum(lens) == len(got) and len(stats) == (len(src) + hw - 1) // hw
    assert len(got) <= F.bound(len(src), hw)
    for st in stats:
        assert st["longest_offset"] <= 65535 and st["longest_literals"] <= 65535 and st["longest_match"] <= 65535
        assert st["shortest_match"] is None or st["shortest_match"] >= mm
    return got, stats


@pytest.mark.parametrize("mm", (3, 4))
@pytest.mark.parametrize("kind", KINDS)
def test_sizes_round_trip(kind, mm):
    for n in SIZES:
        src = lz4s_sim.make_input(kind, n, 3)
        roundtrip(src, 65536, mm)


@pytest.mark.parametrize("mm", (3, 4))
def test_four_blocks_the_last_of_one_byte(mm):
    src = lz4s_sim.make_input("text", 3073, 3)
    got, stats = roundtrip(src, 1024, mm)
    blocks = F.split(got)
    assert len(blocks) == 4 and blocks[3] == b"\x02\x00\x00\x00\x10" + src[-1:]


@pytest.mark.parametrize("mm", (3, 4))
def test_window(mm):
    """nothing farther back than 65535 is taken, with hw_buff_sz above 64 KB.  The check is carried by the two far_input
    layouts, where the table still holds the far candidates when their copies arrive: exactly 65535 back (taken: the reader
    sees that offset) and exactly 65536 back (not taken).  window_input is the layout with 70000 random bytes in front; its
    sources are gone from the table before their copies arrive, so it only round-trips (lz4s_sim.window_input)."""
    roundtrip(lz4s_sim.window_input(), 131072, mm)
    _, st = roundtrip(lz4s_sim.far_input(65535), 131072, mm)
    assert st[0]["longest_offset"] == 65535
    got, st = roundtrip(lz4s_sim.far_input(65536), 131072, mm)
    assert st[0]["longest_offset"] < 65535
    assert len(got) > 3000                                          # (the second copy went out as literals)


@pytest.mark.parametrize("mm", (3, 4))
def test_split_rules(mm):
    """a literal run above 65535 goes on in sequences without a match, a match above 65535 in further matches"""
    got, st = roundtrip(lz4s_sim.make_input("rand", 131072, 3), 131072, mm)
    # (random bytes do hold the odd match: 2^17 positions meet a candidate with their 12-bit hash each, one in 2^20 of which
    # agrees in four bytes)
    assert st[0]["matches"] <= 2 and st[0]["sequences"] >= 3 and st[0]["longest_literals"] == 65535
    assert len(got) <= 4 + 131072 + 2 * (1 + 257 + 2) + 1 + 2 * st[0]["matches"]   # two full runs, two literals, the block's end
    got, st = roundtrip(b"A" * 131072, 131072, mm)
    assert st[0]["longest_match"] == 65535 and st[0]["matches"] == 3 and st[0]["sequences"] == 3
    assert len(got) <= 4 + 2 + 2 * (3 + 257) + 3


@pytest.mark.parametrize("mm", (3, 4))
def test_derived_sizes(mm):
    """64 KB of one byte: a literal, then one match of 65535 bytes with 257 length bytes - with the size word and room for one
    more sequence at most 280 bytes.  Random bytes stay inside the bound (checked by roundtrip for every case)."""
    got, st = roundtrip(b"A" * 65536, 65536, mm)
    assert len(got) <= 280
    assert st[0]["sequences"] == 1 and st[0]["longest_match"] == 65535 and st[0]["longest_offset"] == 1
    for n in (1, 255, 65535, 65536):
        got, _ = roundtrip(lz4s_sim.make_input("rand", n, 9), 65536, mm)
        assert len(got) <= 4 + n + n // 255 + 4 * ((n + 65534) // 65535) + 16


def test_shortest_matches():
    """mini_match 4: nothing shorter than 4 (roundtrip checks it for every case); mini_match 3: matches of exactly 3 appear
    on text, so the three-byte search is really there"""
    src = lz4s_sim.make_input("text", 65536, 3)
    _, st4 = roundtrip(src, 65536, 4)
    assert st4[0]["shortest_match"] == 4
    _, st3 = roundtrip(src, 65536, 3)
    assert st3[0]["shortest_match"] == 3


@pytest.mark.parametrize("mm", (3, 4))
def test_chunks_are_independent(mm):
    """five chunks in one launch = the five one-chunk streams; and the same bytes from 1 wave and from 8"""
    src = lz4s_sim.make_input("silesia", 4 * 16384 + 5000, 3)
    whole, _ = lz4s_sim.compress(src, 16384, mm)
    parts = b"".join(lz4s_sim.compress(src[i:i + 16384], 16384, mm)[0] for i in range(0, len(src), 16384))
    assert whole == parts
    assert lz4s_sim.compress(src, 16384, mm, waves=1)[0] == whole
    assert lz4s_sim.compress(src, 16384, mm, waves=8)[0] == whole
    assert F.decode(whole, mm, 16384) == src


@pytest.mark.parametrize("r", INDEX["ratio"], ids=lambda r: r["kind"])
def test_ratio_gate(r):
    """at 64 KB chunks and mini_match 3 the LZ4s stream is at most 1.10 times the sum of liblz4 1.9.3's level-1 block bodies
    for the same chunks.  The bodies' sizes are recorded in the index (made where the library is installed) and checked
    against the library where it is here."""
    src = lz4s_sim.make_input(r["kind"], r["n"], r["seed"])
    assert _sha(src) == r["in_sha"]
    if refcalls.lz4_pinned():
        assert sum(len(refcalls.lz4_compress_block(src[i:i + 65536], 65536 + 300)) for i in range(0, r["n"], 65536)) == r["lz4_bodies"]
    got, _ = roundtrip(src, 65536, 3)
    print("%s: LZ4s %d bytes, liblz4 bodies %d, ratio %.4f" % (r["kind"], len(got), r["lz4_bodies"], len(got) / r["lz4_bodies"]))
    assert len(got) <= 1.10 * r["lz4_bodies"]
    assert len(got) == r["lz4s_len"]


def test_ratio_gate_covers_the_four_corpora():
    assert sorted(r["kind"] for r in INDEX["ratio"]) == ["lzmix", "records", "silesia", "text"]
    assert all(r["n"] == 262144 for r in INDEX["ratio"])


def test_pin():
    """the emulator reproduces every pinned stream (the GPU test does the same with the GPU build)"""
    assert len(INDEX["cases"]) >= 20
    for c in INDEX["cases"]:
        src = lz4s_sim.make_input(c["kind"], c["n"], c["seed"])
        assert _sha(src) == c["in_sha"], c
        got, _ = lz4s_sim.compress(src, c["hw_buff_sz"], c["mini_match"])
        assert (len(got), _sha(got)) == (c["out_len"], c["out_sha"]), c
        assert F.decode(got, c["mini_match"], c["hw_buff_sz"]) == src


def test_reader_is_strict():
    """the reader refuses what the format does not allow (so that its acceptance above means something)"""
    def blk(body):
        return len(body).to_bytes(4, "little") + body
    good = blk(b"\x22ab" + b"\x02\x00" + b"\x10c")                  # "ab", a match of 4 (M 2, mini_match 3) from 2 back, "c"
    assert F.decode(good, 3, 65536) == b"ababab" + b"c"
    for bad in (good[:-1],                                          # the size word runs past the stream
                blk(b"\x30ab"),                                     # literals cut by the block's end
                blk(b"\x22ab\x02"),                                 # offset cut
                blk(b"\x22ab\x00\x00\x10c"),                        # offset 0 on a match
                blk(b"\x22ab\x03\x00\x10c"),                        # offset beyond the produced bytes
                blk(b"\x20ab\x01\x00\x10c"),                        # non-zero offset without a match
                blk(b"\x22ab\x02\x00\x00"),                         # trailing empty sequence
                blk(b"\xf0" + b"\xff" * 256 + b"\xf1" + b"x" * 65536),   # 65536 literals in one sequence
                blk(b"\x1fa\x01\x00" + b"\xff" * 256 + b"\xf0"),    # a match of 65537
                ):
        with pytest.raises(F.FormatError):
            F.decode(bad, 3, 65536)
    with pytest.raises(F.FormatError):                              # a block other than the last that is not hw_buff_sz bytes
        F.decode(blk(b"\x10a") + blk(b"\x10b"), 3, 1024)
