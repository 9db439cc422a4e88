"""A plain writer of zstd frames from explicit parts, written from RFC 8878 for the tests of the decoder: every choice a
compressor would make is an argument here - the literals mode and size format, the Huffman weights (direct or as an FSE
description), the number of streams, the normalised counts and accuracy log of each sequence table, the mode of each table,
the sequences as (literal length, match length, Offset_Value).  Nothing is validated: a frame the RFC forbids can be written
on purpose.  It shares no code with the kernels, the emulator or the readers; only the RFC's constant tables are imported."""
from zstd_format import LL_NORM, OF_NORM, ML_NORM, LL_BITS, ML_BITS, LL_BASE, ML_BASE

MAGIC = b"\x28\xb5\x2f\xfd"
PREDEFINED = {"LL": (LL_NORM, 6), "OF": (OF_NORM, 5), "ML": (ML_NORM, 6)}


def back_bits(fields):
    """(value, width) in the order a decoder reads them -> the bytes of a backward stream with its end mark"""
    v = 1
    for val, n in fields:
        assert 0 <= val < (1 << n) or (n == 0 and val == 0), (val, n)
        v = (v << n) | val
    return v.to_bytes((v.bit_length() + 7) // 8, "little")


# ---------------------------------------------------------------- FSE

def fse_states(norm, log):
    """4.1.1 -> per state (symbol, bits, baseline)"""
    size = 1 << log
    cells, high = [None] * size, size - 1
    for s, c in enumerate(norm):
        if c == -1:
            cells[high] = s
            high -= 1
    pos, step = 0, (size >> 1) + (size >> 3) + 3
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            cells[pos] = s
            pos = (pos + step) % size
            while pos > high:
                pos = (pos + step) % size
    seen = [abs(c) for c in norm]
    states = []
    for s in cells:
        x = seen[s]
        seen[s] += 1
        nb = log - (x.bit_length() - 1)
        states.append((s, nb, (x << nb) - size))
    return states


def fse_chain(states, symbols, want_bits_last=False):
    """the states a decoder passes through to give `symbols`, and the bits it reads between them: -> (first state,
    [(value, width)] one per transition).  The last state is the lowest one of its symbol (with want_bits_last: the lowest
    that reads at least one bit)"""
    last = [i for i, (s, nb, _) in enumerate(states) if s == symbols[-1] and (nb or not want_bits_last)][0]
    chain, trans = [last], []
    for sym in reversed(symbols[:-1]):
        nxt = chain[0]
        st = [i for i, (s, nb, base) in enumerate(states) if s == sym and base <= nxt < base + (1 << nb)][0]
        trans.insert(0, (nxt - states[st][2], states[st][1]))
        chain.insert(0, st)
    return chain[0], trans


def ncount(norm, log):
    """4.1.1: the description of a distribution (trailing zero counts are not written)"""
    v, pos = log - 5, 4
    remaining, threshold, nbits = (1 << log) + 1, 1 << log, log + 1
    i, prev0 = 0, False
    while remaining > 1:
        if prev0:
            z = 0
            while norm[i + z] == 0:
                z += 1
            i += z
            while z >= 3:
                v |= 3 << pos
                pos += 2
                z -= 3
            v |= z << pos
            pos += 2
        x = norm[i] + 1
        mx = 2 * threshold - 1 - remaining
        if x < mx:
            v |= x << pos
            pos += nbits - 1
        else:
            v |= (x if x < threshold else x + mx) << pos
            pos += nbits
        remaining -= abs(norm[i])
        prev0 = norm[i] == 0
        i += 1
        while remaining < threshold:
            nbits -= 1
            threshold >>= 1
    return v.to_bytes((pos + 7) // 8, "little"), pos


# ---------------------------------------------------------------- Huffman

def last_weight(weights):
    total = sum(1 << (w - 1) for w in weights if w)
    rest = (1 << total.bit_length()) - total
    return rest.bit_length()


def huffman_codes(weights):
    """all weights, the last one included -> ({symbol: (code, length)}, the longest code)"""
    maxbits = sum(1 << (w - 1) for w in weights if w).bit_length() - 1
    codes, at = {}, 0
    for w in range(1, maxbits + 1):
        for s, ws in enumerate(weights):
            if ws == w:
                codes[s] = (at >> (w - 1), maxbits + 1 - w)
                at += 1 << (w - 1)
    return codes, maxbits


def huffman_stream(codes, lits):
    return back_bits([codes[b] for b in lits])


def tree_direct(weights):
    """the listed weights (without the last) as 4-bit fields behind the header byte 127 + count"""
    w = list(weights) + [0] * (len(weights) & 1)
    return bytes([127 + len(weights)]) + bytes(w[i] << 4 | w[i + 1] for i in range(0, len(w), 2))


def tree_fse(weights, norm, log):
    """the listed weights through two FSE states that take turns (4.2.1.2)"""
    states = fse_states(norm, log)
    n = len(weights)
    assert n >= 2
    a, b = list(weights[0::2]), list(weights[1::2])
    # the state that gives the last but one weight must ask for bits it does not get: that ends the stream
    fa, ta = fse_chain(states, a, want_bits_last=(n - 2) % 2 == 0)
    fb, tb = fse_chain(states, b, want_bits_last=(n - 2) % 2 == 1)
    fields = [(fa, log), (fb, log)]
    for i in range(max(len(ta), len(tb))):
        fields += ta[i:i + 1] + tb[i:i + 1]
    desc, _ = ncount(norm, log)
    body = desc + back_bits(fields)
    assert len(body) < 128
    return bytes([len(body)]) + body


# ---------------------------------------------------------------- sections, blocks, frames

def literals(mode, lits=b"", weights=None, tree=None, streams=1, fmt=None, regen=None):
    """mode "raw" | "rle" | "huffman" | "treeless".  weights: ALL weights by symbol (the codes); tree: the tree description's
    bytes (tree_direct / tree_fse; None for treeless); fmt: the Size_Format, else the smallest that holds the sizes"""
    n = len(lits) if regen is None else regen
    if mode in ("raw", "rle"):
        t = 0 if mode == "raw" else 1
        if fmt is None:
            fmt = 0 if n < 32 else 1 if n < 4096 else 3
        if fmt == 0:
            head = bytes([t | n << 3])
        else:
            head = (t | fmt << 2 | n << 4).to_bytes(2 if fmt == 1 else 3, "little")
        return head + (bytes(lits) if mode == "raw" else bytes(lits[:1]))
    codes, _ = huffman_codes(weights)
    if streams == 1:
        body = huffman_stream(codes, lits)
    else:
        seg = (n + 3) // 4
        parts = [huffman_stream(codes, lits[i * seg:(i + 1) * seg]) for i in range(4)]
        body = b"".join(len(p).to_bytes(2, "little") for p in parts[:3]) + b"".join(parts)
    body = (tree or b"") + body
    if fmt is None:
        fmt = 0 if streams == 1 else 1 if max(n, len(body)) < 1024 else 2 if max(n, len(body)) < 16384 else 3
    bits = (10, 10, 14, 18)[fmt]
    t = 2 if mode == "huffman" else 3
    head = (t | fmt << 2 | n << 4 | len(body) << (4 + bits)).to_bytes((3, 3, 4, 5)[fmt], "little")
    return head + body


def _code(value, bases):
    return max(c for c in range(len(bases)) if bases[c] <= value)


def sequences(seqs, ll=("predefined",), of=("predefined",), ml=("predefined",), count_form=None):
    """seqs: [(literal length, match length, Offset_Value)] - the value as written: 1-3 repeat codes, else offset + 3.
    A table: ("predefined",) | ("rle", code) | ("fse", norm, log) | ("repeat", norm, log) with the table that is in force
    (log 0 and norm None after RLE_Mode: ("repeat", code))"""
    n = len(seqs)
    if count_form is None:
        count_form = 1 if n < 128 else 2 if n < 0x7f00 else 3
    head = bytes([n]) if count_form == 1 else bytes([128 + (n >> 8), n & 255]) if count_form == 2 else b"\xff" + (n - 0x7f00).to_bytes(2, "little")
    if n == 0:
        return head
    lc = [_code(s[0], LL_BASE) for s in seqs]
    mc = [_code(s[1], ML_BASE) for s in seqs]
    oc = [s[2].bit_length() - 1 for s in seqs]
    modes, descs, chains = 0, b"", []
    for shift, name, spec, codes in ((6, "LL", ll, lc), (4, "OF", of, oc), (2, "ML", ml, mc)):
        kind = spec[0]
        modes |= {"predefined": 0, "rle": 1, "fse": 2, "repeat": 3}[kind] << shift
        if kind == "rle" or (kind == "repeat" and len(spec) == 2):
            if kind == "rle":
                descs += bytes([spec[1]])
            chains.append((0, 0, [(0, 0)] * (n - 1)))
            continue
        norm, log = PREDEFINED[name] if kind == "predefined" else spec[1:3]
        if kind == "fse":
            descs += ncount(norm, log)[0]
        first, trans = fse_chain(fse_states(norm, log), codes)
        chains.append((first, log, trans))
    (fl, lllog, tl), (fo, oflog, to), (fm, mllog, tm) = chains
    fields = [(fl, lllog), (fo, oflog), (fm, mllog)]
    for i, (llen, mlen, ov) in enumerate(seqs):
        fields += [(ov - (1 << oc[i]), oc[i]), (mlen - ML_BASE[mc[i]], ML_BITS[mc[i]]), (llen - LL_BASE[lc[i]], LL_BITS[lc[i]])]
        if i + 1 < n:
            fields += [tl[i], tm[i], to[i]]
    return head + bytes([modes]) + descs + back_bits(fields)


def block(btype, payload, last=False, size=None):
    """btype "raw" | "rle" | "compressed"; size: Block_Size where it is not the payload's length (an RLE block)"""
    t = {"raw": 0, "rle": 1, "compressed": 2}[btype]
    bs = len(payload) if size is None else size
    return ((1 if last else 0) | t << 1 | bs << 3).to_bytes(3, "little") + bytes(payload)


def frame(blocks, content=None, fcs_bytes=None, window_byte=None, checksum=None):
    """window_byte None: Single_Segment (content needed).  fcs_bytes: 0, 1, 2, 4, 8, else the smallest for content.
    checksum: the 4 bytes behind the last block"""
    single = window_byte is None
    if fcs_bytes is None:
        fcs_bytes = 0 if content is None else (1 if single and content < 256 else 2 if 256 <= content < 65792 else 4)
    fhd = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes] << 6 | (0x20 if single else 0) | (4 if checksum is not None else 0)
    out = MAGIC + bytes([fhd]) + (b"" if single else bytes([window_byte]))
    if fcs_bytes:
        out += (content - (256 if fcs_bytes == 2 else 0)).to_bytes(fcs_bytes, "little")
    return out + b"".join(blocks) + (checksum or b"")
