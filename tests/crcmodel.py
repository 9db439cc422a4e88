"""The Rocksoft model of a CRC, bit by bit in pure Python: the reference of the programmable-CRC tests (qzk_crcn_kernel,
qzd_crcn_ranges, the Crc64 calls and the CRCs of the metadata records).

A config is (width, polynomial, initial_value, reflect_in, reflect_out, xor_out) - the fields of QzCrc64Config_T /
QzCrc32Config_T (include/qatzip.h) in front of which stands the width.  CATALOGUE holds nine published algorithms with
their check values, the CRC of b"123456789" (Greg Cook's catalogue of parametrised CRC algorithms)."""


def _reflect(v, bits):
    r = 0
    for _ in range(bits):
        r = (r << 1) | (v & 1)
        v >>= 1
    return r


def register(cfg, data, reg=None):
    """the raw register after `data`, from `reg` (None: the config's initial value)"""
    width, poly, init, refin, _, _ = cfg
    top, mask = 1 << (width - 1), (1 << width) - 1
    reg = init if reg is None else reg
    for b in data:
        if refin:
            b = _reflect(b, 8)
        reg ^= b << (width - 8)
        for _ in range(8):
            reg = ((reg << 1) ^ poly) & mask if reg & top else (reg << 1) & mask
    return reg


def finalise(cfg, reg):
    width, _, _, _, refout, xorout = cfg
    return (_reflect(reg, width) if refout else reg) ^ xorout


def unfinalise(cfg, crc):
    width, _, _, _, refout, xorout = cfg
    v = crc ^ xorout
    return _reflect(v, width) if refout else v


def crc(cfg, data, start=None):
    """CRC of `data`; start = the finalised CRC of the bytes before it (zlib's crc32(crc, buf) chaining), None = none"""
    return finalise(cfg, register(cfg, data, None if start is None else unfinalise(cfg, start)))


def empty(cfg):
    """the CRC of the empty message: what a chain starts from"""
    return finalise(cfg, cfg[2])


CRC64_ECMA = (64, 0x42F0E1EBA9EA3693, 0, 0, 0, 0)
CRC64_XZ = (64, 0x42F0E1EBA9EA3693, 0xFFFFFFFFFFFFFFFF, 1, 1, 0xFFFFFFFFFFFFFFFF)
CRC64_GO_ISO = (64, 0x1B, 0xFFFFFFFFFFFFFFFF, 1, 1, 0xFFFFFFFFFFFFFFFF)
CRC64_WE = (64, 0x42F0E1EBA9EA3693, 0xFFFFFFFFFFFFFFFF, 0, 0, 0xFFFFFFFFFFFFFFFF)
CRC32_ISO_HDLC = (32, 0x04C11DB7, 0xFFFFFFFF, 1, 1, 0xFFFFFFFF)
CRC32_BZIP2 = (32, 0x04C11DB7, 0xFFFFFFFF, 0, 0, 0xFFFFFFFF)
CRC32C = (32, 0x1EDC6F41, 0xFFFFFFFF, 1, 1, 0xFFFFFFFF)
CRC32_MPEG2 = (32, 0x04C11DB7, 0xFFFFFFFF, 0, 0, 0)
CRC32_CKSUM = (32, 0x04C11DB7, 0, 0, 0, 0xFFFFFFFF)

CATALOGUE = {
    "CRC-64/ECMA-182": (CRC64_ECMA, 0x6C40DF5F0B497347),
    "CRC-64/XZ": (CRC64_XZ, 0x995DC9BBDF1939FA),
    "CRC-64/GO-ISO": (CRC64_GO_ISO, 0xB90956C775A41001),
    "CRC-64/WE": (CRC64_WE, 0x62EC59E3F1A4F00A),
    "CRC-32/ISO-HDLC": (CRC32_ISO_HDLC, 0xCBF43926),
    "CRC-32/BZIP2": (CRC32_BZIP2, 0xFC891918),
    "CRC-32C": (CRC32C, 0xE3069283),
    "CRC-32/MPEG-2": (CRC32_MPEG2, 0x0376E6E7),
    "CRC-32/CKSUM": (CRC32_CKSUM, 0x765E7680),
}


def _table(cfg):
    width, poly = cfg[0], cfg[1]
    top, mask = 1 << (width - 1), (1 << width) - 1
    tab = []
    for b in range(256):
        r = b << (width - 8)
        for _ in range(8):
            r = ((r << 1) ^ poly) & mask if r & top else (r << 1) & mask
        tab.append(r)
    return tab


_TABLES = {}
_REV8 = [_reflect(b, 8) for b in range(256)]


def crc_fast(cfg, data, start=None):
    """crc() a byte at a time through a table (the same model; the tests check it against the bitwise one): for the long
    buffers of the GPU tests"""
    key = cfg[:2]
    if key not in _TABLES:
        _TABLES[key] = _table(cfg)
    tab = _TABLES[key]
    width, _, init, refin, _, _ = cfg
    sh, mask = width - 8, (1 << width) - 1
    reg = init if start is None else unfinalise(cfg, start)
    if refin:
        rev = _REV8
        for b in data:
            reg = tab[(reg >> sh) ^ rev[b]] ^ ((reg << 8) & mask)
    else:
        for b in data:
            reg = tab[(reg >> sh) ^ b] ^ ((reg << 8) & mask)
    return finalise(cfg, reg)


def crc_many(cfg, pieces):
    """[crc(cfg, p) for p in pieces], for the many equal-sized blocks of the GPU tests: the table-driven byte step of
    crc_fast taken by all pieces at once (numpy), a piece dropping out when it ends.  A few pieces go through crc_fast."""
    if len(pieces) < 8:
        return [crc_fast(cfg, p) for p in pieces]
    import numpy as np
    key = cfg[:2]
    if key not in _TABLES:
        _TABLES[key] = _table(cfg)
    width, _, init, refin, _, _ = cfg
    tab = np.array(_TABLES[key], np.uint64)
    rev = np.array(_REV8, np.uint64)
    lens = np.array([len(p) for p in pieces])
    data = np.zeros((len(pieces), max(int(lens.max()), 1)), np.uint64)
    for i, p in enumerate(pieces):
        data[i, :len(p)] = np.frombuffer(p, np.uint8)
    if refin:
        data = rev[data]
    sh, mask = np.uint64(width - 8), np.uint64((1 << width) - 1)
    reg = np.full(len(pieces), init, np.uint64)
    for i in range(int(lens.max())):
        nxt = tab[(reg >> sh) ^ data[:, i]] ^ ((reg << np.uint64(8)) & mask)
        reg = np.where(lens > i, nxt, reg)
    return [finalise(cfg, int(r)) for r in reg]
