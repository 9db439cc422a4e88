"""The hash-chain lazy parse of zstd sessions (include/qzamd_zstd_parse.h, qatzip_amd/csrc/qzk_zstd_parse.h) on the CPU SIMT
emulator, through the host plan the device layer runs (qzd_zstd_parse_host.h).  Every frame is read by the strict reader of
whole frames (tests/zstd_full_format.py) and, where libzstd loads, by ZSTD_decompress; the sequence list the reader returns,
repeat offsets resolved, is checked record by record against the input."""
import functools
import hashlib
import subprocess

import pytest

import zstd_parse_sim as P
import zstd_parse_traps as T
import zstd_seq_sim as Q
import zstd_sim as S

EDGES = P.edge_cases()


def _sha(b):
    return hashlib.sha256(b).hexdigest()


@functools.lru_cache(maxsize=None)
def _edge(name, flags=3):
    """an edge case through the emulator and both readers, once: (stream, per-frame lengths, the reader's frames)"""
    src, hw, mm, depth = EDGES[name]
    got, lens = P.compress(src, hw, mm, flags, depth)
    frames = Q.read(got, src, hw)
    assert [f["size"] for f in frames] == lens and sum(lens) == len(got)
    return got, lens, frames


@functools.lru_cache(maxsize=None)
def _ratio_run(kind, depth):
    r = [r for r in S.index()["ratio"] if r["kind"] == kind][0]
    src = S.make_input(r["kind"], r["n"], r["seed"])
    got, lens = P.compress(src, 65536, 3, 3, depth)
    return src, got, Q.read(got, src, 65536)


def _check_frames(src, hw, mm, frames):
    """every sequence of every compressed frame: ml >= mm, 1 <= off <= its position, source bytes equal to target bytes"""
    n = 0
    for i, f in enumerate(frames):
        if "block:compressed" in f["tally"]:
            P.check_sequences(src[i * hw:(i + 1) * hw], f["sequences"], mm)
            n += len(f["sequences"])
    return n


# ---------------------------------------------------------------- 1. every frame decodes, every sequence holds
@pytest.mark.parametrize("name", sorted(EDGES))
def test_edge_frames_decode_and_their_sequences_hold(name):
    src, hw, mm, depth = EDGES[name]
    _, _, frames = _edge(name)
    nseq = _check_frames(src, hw, mm, frames)
    assert nseq > 0 or name == "random"


# ---------------------------------------------------------------- 2. the search finds the longest match
@pytest.mark.parametrize("mm", (3, 4))
@pytest.mark.parametrize("name", sorted(P.small_inputs()))
def test_search_is_the_longest_match(name, mm):
    b = P.small_inputs()[name]
    assert len(b) == 4096
    chain, res = P.search(b, 4096, mm, 256)
    want = P.brute_longest(b, mm)
    # the chain: every link points at the nearest earlier position of the chunk with the same hash of mm bytes (the serial
    # model's P1, tests/zstd_parse_traps.py), at this head-table width and at the widest
    assert chain == T.p1_chain(b, 4096, mm)
    wide, wres = P.search(b, 131072, mm, 256)
    assert wide == T.p1_chain(b, 131072, mm)
    whops = [0] * len(b)
    for p, d in enumerate(wide):
        assert 0 <= d <= p and (d == 0 or d >= chain[p] > 0)       # fewer collisions: never nearer than the narrow table's
        whops[p] = whops[p - d] + 1 if d else 0
    assert all(wres[p] == want[p] for p in range(len(b)) if whops[p] <= 256)
    hops = [0] * len(b)
    for p, d in enumerate(chain):
        assert 0 <= d <= p
        hops[p] = hops[p - d] + 1 if d else 0
    checked = 0
    for p in range(len(b)):
        # a chain no longer than the depth is walked to its end; one that is longer only where the walk may stop early:
        # the match reaches the chunk's end, and nothing nearer is as long
        if hops[p] <= 256 or (res[p][0] and p + res[p][0] == len(b)):
            assert res[p] == want[p], (name, mm, p, res[p], want[p], hops[p])
            checked += 1
        else:
            assert res[p][0] <= want[p][0]
        if res[p][0]:
            assert res[p][0] >= mm and 1 <= res[p][1] <= p and P.match_len(b, p, p - res[p][1]) == res[p][0]
    print(name, mm, "positions checked against brute force:", checked, "longest chain:", max(hops))
    assert checked >= (4096 if name in ("text", "rand", "period3", "period200") else 2048)
    # depth 1: the verdict of the chain's first candidate alone
    chain1, res1 = P.search(b, 4096, mm, 1)
    assert chain1 == chain
    for p, d in enumerate(chain):
        k = P.match_len(b, p, p - d) if d else 0
        assert res1[p] == ((k, d) if k >= mm else (0, 0)), (name, mm, p)


def test_search_reaches_past_65535_and_to_the_chunks_end():
    b = P.far_repeat()
    _, res = P.search(b, 131072, 3, 16)
    assert res[70000] == (60000, 70000)
    assert res[100000] == (30000, 70000)
    _, res = P.search(b"A" * 131072, 131072, 3, 4)
    assert res[0] == (0, 0) and res[1] == (131071, 1) and res[131069] == (3, 1) and res[131070] == (0, 0)


# ---------------------------------------------------------------- 3. the sequence flags do not change the sequences
@pytest.mark.parametrize("name", ("overlap", "rep_ll0", "late3", "depth16", "far"))
def test_flags_do_not_change_the_sequences(name):
    """"far": an offset of 70000 through the entropy stage under flags 0, 1, 2 and 3"""
    src, hw, mm, depth = EDGES[name]
    first = None
    for flags in (0, 1, 2, 3):
        stream, lens = P.compress(src, hw, mm, flags, depth)
        pos = 0
        per_chunk = []
        for i, ln in enumerate(lens):
            chunk = src[i * hw:(i + 1) * hw]
            frame, seqs, lits = P.records(chunk, hw, mm, depth, flags)
            assert frame == stream[pos:pos + ln]
            pos += ln
            P.check_sequences(chunk, seqs, mm, lits)
            # the frame is what the entropy stage alone makes of these records and literals
            rc, alone, _ = Q.encode([(len(chunk), seqs, lits)], flags)
            assert rc == 0 and alone == frame, (name, flags, i)
            per_chunk.append((seqs, lits))
        if first is None:
            first = per_chunk
        assert per_chunk == first, (name, flags)


# ---------------------------------------------------------------- 4. depth 0 is the default parse
def test_depth_0_is_the_default_parse():
    cases = [c for c in Q.index()["cases"] if c["n"] == 70001 and c["mini_match"] == 3 and c["kind"] in ("text", "lzmix", "runs")]
    assert len(cases) >= 5 and set(c["flags"] for c in cases) == {1, 2, 3}
    for c in cases:
        src = S.make_input(c["kind"], c["n"], c["seed"])
        if c["flags"] == 3:
            P.compress(src, c["hw_buff_sz"], c["mini_match"], 3, 16)       # a depth, and then 0
        got, _ = P.compress(src, c["hw_buff_sz"], c["mini_match"], c["flags"], 0)
        assert (len(got), _sha(got)) == (c["out_len"], c["out_sha"]), c
    c = S.index()["cases"][0]
    src = S.make_input(c["kind"], c["n"], c["seed"])
    got, _ = P.compress(src, c["hw_buff_sz"], c["mini_match"], 0, 0)
    assert (len(got), _sha(got)) == (c["out_len"], c["out_sha"])


# ---------------------------------------------------------------- 5. edge cases
def test_the_far_match_is_taken():
    """the second half repeats the first at distance 70000: out of the default parse's reach (65535), so the new frame must
    be less than 0.6 of the default frame under the same flags"""
    src, hw, mm, depth = EDGES["far"]
    got, _, frames = _edge("far")
    default, _ = Q.compress(src, hw, mm, 3)
    print("far: depth %d %d bytes, default %d bytes, ratio %.4f" % (depth, len(got), len(default), len(got) / len(default)))
    assert len(got) < 0.6 * len(default)
    assert (60000, 70000) in [(ml, off) for _, ml, off in frames[0]["sequences"]]
    assert all(off <= 65535 for _, _, off in Q.read(default, src, hw)[0]["sequences"])


def test_all_one_byte_is_one_match_to_the_chunks_end():
    _, _, frames = _edge("all_one")
    assert frames[0]["sequences"] == [(1, 131071, 1)] and frames[0]["size"] < 40


def test_random_bytes_are_raw_blocks():
    _, lens, frames = _edge("random")
    assert all("block:raw" in f["tally"] for f in frames) and lens == [4096 + 10, 904 + 10]


def test_short_last_chunks():
    for name, tail in (("tail1", 1), ("tail2", 2), ("tail3", 3), ("hw1024_3073", 1)):
        _, lens, frames = _edge(name)
        assert frames[-1]["content_size"] == tail and lens[-1] == tail + 9 and "block:raw" in frames[-1]["tally"]


@pytest.mark.parametrize("mm", (3, 4))
def test_a_match_in_the_last_mini_match_bytes(mm):
    src = EDGES["late%d" % mm][0]
    _, _, frames = _edge("late%d" % mm)
    seqs = frames[0]["sequences"]
    assert "block:compressed" in frames[0]["tally"] and seqs[-1][1:] == (mm, mm + 1)
    assert sum(ll + ml for ll, ml, _ in seqs) == len(src) == 1500 + 2 * mm + 1


def test_overlapping_matches():
    _, _, frames = _edge("overlap")
    seqs = frames[0]["sequences"]
    assert any(off == 1 and ml >= 290 for _, ml, off in seqs) and any(off == 5 and ml >= 390 for _, ml, off in seqs)


def test_repeat_offset_hits():
    """one byte changed in a copy: the match behind the changed byte has ll == 1 and the offset of the match before it
    (rep1); one byte dropped: ll == 0 and that offset less 1 (the third repeat code of ll == 0)"""
    _, _, frames = _edge("rep_ll_gt0")
    assert "rep:1:ll>0" in frames[0]["tally"]
    seqs = frames[0]["sequences"]
    assert any(a[2] == b[2] == 700 and b[0] == 1 for a, b in zip(seqs, seqs[1:]))
    _, _, frames = _edge("rep_ll0")
    assert "rep:3:ll0" in frames[0]["tally"]
    seqs = frames[0]["sequences"]
    assert any(a[2] == 700 and b[2] == 699 and b[0] == 0 for a, b in zip(seqs, seqs[1:]))
    # without the flag the same sequences, no repeat code
    src, hw, mm, depth = EDGES["rep_ll0"]
    f1 = Q.read(P.compress(src, hw, mm, 1, depth)[0], src, hw)[0]
    assert f1["sequences"] == seqs and not [t for t in f1["tally"] if t.startswith("rep:")]


def test_depths():
    sizes = [len(_edge("depth%d" % d)[0]) for d in P.DEPTHS]
    print("lzmix 20000 bytes, depths", P.DEPTHS, sizes)
    assert len(set(_sha(_edge("depth%d" % d)[0]) for d in P.DEPTHS)) >= 3
    assert sizes[-1] < sizes[0]


def test_rounds_do_not_change_the_bytes():
    """the host plan: a round holds what the budget allows, 4096 chunks at most; a call cut into rounds of 3 chunks, or of
    1, gives the bytes of a call in one round"""
    assert P.round_chunks(1024, 5000) == 4096 and P.round_chunks(1024, 7) == 7
    for hw in (1024, 4096, 65536, 131072):
        r = P.round_chunks(hw, 1 << 20)
        assert 1 <= r <= 4096 and r * P.chunk_bytes(hw) <= 4 << 30 and (r == 4096 or (r + 1) * P.chunk_bytes(hw) > 4 << 30)
        assert P.chunk_bytes(hw) <= 21 * hw + 1024
    src = S.make_input("silesia", 10 * 1024 + 100, 4)
    whole, lens = P.compress(src, 1024, 3, 3, 16)
    assert len(lens) == 11
    assert P.compress(src, 1024, 3, 3, 16, round_cap=3) == (whole, lens) == P.compress(src, 1024, 3, 3, 16, round_cap=1)
    parts = [P.compress(src[i:i + 1024], 1024, 3, 3, 16)[0] for i in range(0, len(src), 1024)]
    assert b"".join(parts) == whole


def test_refusals():
    src = b"abc" * 1000
    for kw in (dict(depth=257), dict(depth=0xffffffff), dict(flags=4), dict(hw_buff_sz=512), dict(hw_buff_sz=262144), dict(mini_match=5)):
        assert P.run(src, **kw)[0] == -2, kw


# ---------------------------------------------------------------- 6. pins
def test_pinned_edges():
    idx = P.index()["edges"]
    assert sorted(idx) == sorted(EDGES)
    for name, c in idx.items():
        src, hw, mm, depth = EDGES[name]
        assert (hw, mm, depth, _sha(src)) == (c["hw_buff_sz"], c["mini_match"], c["depth"], c["in_sha"]), name
        got = _edge(name)[0]
        assert (len(got), _sha(got)) == (c["out_len"], c["out_sha"]), name


def test_pinned_kinds():
    cases = P.index()["cases"]
    assert [c["kind"] for c in cases] == list(P.KINDS)
    for c in cases:
        assert (c["n"], c["hw_buff_sz"], c["mini_match"], c["depth"], c["flags"]) == (70001, 65536, 3, 16, 3)
        src = S.make_input(c["kind"], c["n"], c["seed"])
        assert _sha(src) == c["in_sha"]
        got, lens = P.compress(src, 65536, 3, 3, 16)
        assert (len(got), _sha(got)) == (c["out_len"], c["out_sha"]), c
        _check_frames(src, 65536, 3, Q.read(got, src, 65536))


# ---------------------------------------------------------------- 7. ratio
@pytest.mark.parametrize("kind", ("text", "records", "silesia", "lzmix"))
def test_ratio(kind):
    """against libzstd's ZSTD_compress on each 64 KB chunk alone (recorded by the generator from the library, never from this
    code); level 3 is zstd's default"""
    r = [r for r in P.index()["ratio"] if r["kind"] == kind][0]
    default = [x for x in Q.index()["ratio"] if x["kind"] == kind][0]["zstd_seq_len"]
    assert r["default_flags3"] == default and sorted(r["depths"]) == ["16", "4", "64"]
    for depth in P.RATIO_DEPTHS:
        src, got, frames = _ratio_run(kind, depth)
        assert _sha(src) == r["in_sha"]
        d = r["depths"][str(depth)]
        ratio = len(got) / r["libzstd_compress"]["3"]
        print(kind, "depth", depth, len(got), "default", default, "libzstd 1/3/9", r["libzstd_compress"], "ratio to level 3 %.4f" % ratio)
        assert len(got) == d["len"]
        assert d["cap"] == round(d["ratio"] + 0.02, 4) and ratio <= d["cap"]
        assert _check_frames(src, 65536, 3, frames) > 0
    if kind != "records":                                           # records: recorded only, the default already beats libzstd
        assert len(_ratio_run(kind, 64)[1]) < default


def test_no_offset_above_131071_at_128_kb_chunks():
    r = S.index()["ratio"][0]
    src = S.make_input(r["kind"], r["n"], r["seed"])
    got, _ = P.compress(src, 131072, 3, 3, 16)
    frames = Q.read(got, src, 131072)
    offs = [off for f in frames for _, _, off in f["sequences"]]
    assert _check_frames(src, 131072, 3, frames) == len(offs) > 0 and max(offs) <= 131071
    print("128 KB chunks: largest offset", max(offs), "offsets above 65535:", sum(1 for o in offs if o > 65535))
    assert max(off for _, _, off in _edge("far")[2][0]["sequences"]) <= 131071
    assert max(off for _, _, off in _edge("hw131072")[2][0]["sequences"]) <= 131071


# ---------------------------------------------------------------- the driver and the host plan under a sanitizer
def test_driver_under_sanitizers(tmp_path):
    """tests/sim/sim_zstd_parse.cpp as a program of its own (SIM_ZSTD_PARSE_MAIN): chunks of every kind through the rounds of
    the host plan under every flag, the refusals, the plan's bounds - built with -fsanitize=address,undefined.  A stand-alone
    program: nothing here is loaded into python."""
    exe = str(tmp_path / "sim_zstd_parse_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DSIM_ZSTD_PARSE_MAIN", "-I", S.SIMDIR, "-Wno-unused-function", "-o", exe, P.SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr
