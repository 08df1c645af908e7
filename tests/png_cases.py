"""A small PNG writer (numpy + stdlib zlib / binascii) and the streams the PNG tests share.

The writer exists because the tests need what Pillow never writes: a chosen filter type in every row (Pillow never picks
Average), IDAT chunks split at chosen bytes, a chosen deflate level and strategy (stored, fixed and dynamic blocks), non-zero
padding bits, short palettes and indices past them.  Expected frames come from the pixel array that went in, under the layout
include/scannertools_hip.h states -- never from the code under test.
"""
import binascii
import struct
import zlib

import numpy as np

SIG = b"\x89PNG\r\n\x1a\n"
SAMPLES = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}   # colour type -> samples per pixel


def chunk(typ, data=b"", crc=None):
    data = bytes(data)
    c = binascii.crc32(typ + data) & 0xFFFFFFFF if crc is None else crc
    return struct.pack(">I", len(data)) + typ + data + struct.pack(">I", c)


def ihdr(w, h, depth, ct, interlace=0, compression=0, filt=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ct, compression, filt, interlace))


def scanlines(pixels, ct, depth, pad=0):
    """(h, rowbytes) uint8 unfiltered scanlines of a pixel array: (h, w) samples or indices for colour types 0 and 3,
    (h, w, 2 / 3 / 4) for 4 / 2 / 6.  Sub-byte samples are packed from the most significant bit down; the unused low bits of
    a row's last byte are taken from ``pad``."""
    px = np.asarray(pixels)
    h, w = px.shape[:2]
    if depth == 8:
        return np.ascontiguousarray(px.reshape(h, w * SAMPLES[ct]).astype(np.uint8))
    per = 8 // depth
    rb = (w + per - 1) // per
    full = np.zeros((h, rb * per), np.int64)
    full[:, :w] = px
    rows = np.zeros((h, rb), np.int64)
    for k in range(per):
        rows |= full[:, k::per] << (8 - depth * (k + 1))
    used = w * depth - (rb - 1) * 8           # bits of the last byte that hold samples
    if used < 8:
        rows[:, -1] |= pad & ((1 << (8 - used)) - 1)
    return rows.astype(np.uint8)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(rows, bpp, filters):
    """The h x (1 + rowbytes) filtered bytes of unfiltered scanlines, row y under filter type filters[y]."""
    rows = np.asarray(rows, np.uint8)
    h, rb = rows.shape
    out = np.zeros((h, 1 + rb), np.uint8)
    prev = np.zeros(rb, np.int64)
    for y in range(h):
        cur = rows[y].astype(np.int64)
        a = np.zeros(rb, np.int64)
        c = np.zeros(rb, np.int64)
        if rb > bpp:
            a[bpp:] = cur[:-bpp]
            c[bpp:] = prev[:-bpp]
        ft = int(filters[y])
        pred = {0: 0, 1: a, 2: prev, 3: (a + prev) >> 1, 4: _paeth(a, prev, c)}[ft]
        out[y, 0] = ft
        out[y, 1:] = (cur - pred) & 255
        prev = cur
    return out


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15):
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    return co.compress(bytes(data)) + co.flush()


def filter_bpp(ct, depth):
    return 1 if depth < 8 else SAMPLES[ct]


def write_png(pixels, ct, depth=8, filters=0, palette=None, trns=None, splits=None, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, pad=0,
              before_idat=(), after_idat=(), zdata=None):
    """A PNG stream.  filters: one type for every row or a sequence of h types.  palette: (k, 3) uint8.  trns: the tRNS
    chunk's bytes.  splits: byte positions at which the zlib stream is cut into IDAT chunks (equal positions give empty ones).
    before_idat / after_idat: further chunks (bytes).  zdata: the zlib stream to store instead of the picture's own."""
    px = np.asarray(pixels)
    h, w = px.shape[:2]
    if np.isscalar(filters):
        filters = [filters] * h
    raw = filter_rows(scanlines(px, ct, depth, pad), filter_bpp(ct, depth), filters)
    z = deflate(raw.tobytes(), level, strategy) if zdata is None else bytes(zdata)
    out = SIG + ihdr(w, h, depth, ct)
    if palette is not None:
        out += chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes())
    if trns is not None:
        out += chunk(b"tRNS", bytes(trns))
    for c in before_idat:
        out += c
    cuts = [0] + sorted(splits or []) + [len(z)]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        out += chunk(b"IDAT", z[lo:hi])
    for c in after_idat:
        out += c
    return out + chunk(b"IEND")


def expected(pixels, ct, depth=8, palette=None, trns=None):
    """The frame the layout table gives for a pixel array."""
    px = np.asarray(pixels)
    h, w = px.shape[:2]
    if ct == 0:
        return (px.astype(np.int64) * {1: 255, 2: 85, 4: 17, 8: 1}[depth]).astype(np.uint8).reshape(h, w, 1)   # tRNS ignored
    if ct == 2:
        px = px.astype(np.uint8)
        if trns is None:
            return px
        key = np.array([trns[1], trns[3], trns[5]], np.uint8)
        alpha = np.where((px == key).all(axis=2), 0, 255).astype(np.uint8)
        return np.concatenate([px, alpha[..., None]], axis=2)
    if ct == 3:
        table = np.zeros((256, 4), np.uint8)
        table[:, 3] = 255
        pal = np.asarray(palette, np.uint8)
        table[:len(pal), :3] = pal
        if trns is not None:
            table[:len(trns), 3] = np.frombuffer(bytes(trns), np.uint8)
        out = table[px.astype(np.int64)]
        return np.ascontiguousarray(out if trns is not None else out[..., :3])
    if ct == 4:
        px = px.astype(np.uint8)
        return np.ascontiguousarray(px[..., [0, 0, 0, 1]])
    return px.astype(np.uint8)


# ---- the shared cases: name -> (stream, expected frame) -----------------------------------------------------------------------
CT_OF_BPP = {1: 0, 2: 4, 3: 2, 4: 6}   # a depth-8 colour type for each bytes-per-pixel value
BAND_ROWS = (0, 63, 64, 65, 127, 128)
PAIR_FILTERS = [f for a in range(5) for b in range(5) for f in (a, b)]   # every ordered pair of filter types, consecutively


def picture(rng, h, w, ct, depth=8, lo=0, hi=None):
    hi = (1 << depth) if hi is None else hi
    shape = (h, w) if SAMPLES[ct] == 1 else (h, w, SAMPLES[ct])
    return rng.integers(lo, hi, shape)


def _smooth(rng, h, w, s):
    """A picture the filters act on in earnest: gradients plus a little noise."""
    y, x = np.mgrid[0:h, 0:w]
    base = (3 * x + 5 * y)[..., None] + 40 * np.arange(s)
    return ((base + rng.integers(0, 6, (h, w, s))) & 255).reshape((h, w) if s == 1 else (h, w, s))


_CACHE = {}


def cases():
    """Every case of the CPU twin's tests, built once: {name: (stream, expected)}."""
    if _CACHE:
        return _CACHE
    rng = np.random.default_rng(20260)
    out = {}

    def add(name, px, ct, depth=8, **kw):
        assert name not in out
        out[name] = (write_png(px, ct, depth, **kw), expected(px, ct, depth, kw.get("palette"), kw.get("trns")))

    # geometry: heights x widths x bytes per pixel, a random filter type in every row
    for h in (1, 2, 63, 64, 65, 129):
        for w in (1, 2, 3, 63, 64, 65, 131):
            for bpp in (1, 2, 3, 4):
                ct = CT_OF_BPP[bpp]
                add("geom_%dx%d_bpp%d" % (h, w, bpp), _smooth(rng, h, w, bpp), ct, filters=rng.integers(0, 5, h))
    # every filter type in row 0 and at every position relative to a 64-row band
    for ft in range(5):
        for bpp in (1, 3, 4):
            filters = rng.integers(0, 5, 130)
            filters[list(BAND_ROWS)] = ft
            add("band_f%d_bpp%d" % (ft, bpp), _smooth(rng, 130, 37, bpp), CT_OF_BPP[bpp], filters=filters)
    # all 25 ordered pairs of consecutive filter types
    for bpp in (1, 2, 3, 4):
        add("pairs_bpp%d" % bpp, picture(rng, len(PAIR_FILTERS), 21, CT_OF_BPP[bpp]), CT_OF_BPP[bpp], filters=PAIR_FILTERS)
    # arithmetic: Paeth's ties (few distinct values, so pa = pb, pb = pc and all three equal occur), Average sums past 255
    add("paeth_ties_rgb", rng.choice([0, 1, 2, 3, 4, 6, 100, 103], (40, 33, 3)), 2, filters=4)
    add("paeth_ties_gray", rng.choice([7, 8, 9, 10, 13], (40, 70)), 0, filters=4)
    add("paeth_flat", np.full((9, 20, 4), 77), 6, filters=4)
    add("average_carry", picture(rng, 40, 33, 2, lo=200, hi=256), 2, filters=3)
    add("average_carry_gray", picture(rng, 70, 90, 0, lo=128, hi=256), 0, filters=3)
    # packing: widths that end inside a byte, padding bits set
    for depth in (1, 2, 4):
        for w in (1, 3, 5, 7, 9):
            f = rng.integers(0, 5, 5)
            add("bits_gray_d%d_w%d" % (depth, w), picture(rng, 5, w, 0, depth), 0, depth, filters=f, pad=0xFF)
            pal = rng.integers(0, 256, (1 << depth, 3))
            add("bits_pal_d%d_w%d" % (depth, w), picture(rng, 5, w, 3, depth), 3, depth, filters=f, pad=0xAB, palette=pal)
    # palettes: short ones, indices past them, short tRNS; colour keys
    add("pal8_full", picture(rng, 20, 31, 3), 3, palette=rng.integers(0, 256, (256, 3)), filters=rng.integers(0, 5, 20))
    add("pal8_short_past", picture(rng, 20, 31, 3), 3, palette=rng.integers(0, 256, (100, 3)))
    add("pal4_short_past", picture(rng, 11, 13, 3, 4), 3, 4, palette=rng.integers(0, 256, (5, 3)), pad=0x0F)
    add("pal8_trns_short", picture(rng, 20, 31, 3, lo=0, hi=64), 3, palette=rng.integers(0, 256, (64, 3)), trns=bytes(range(0, 200, 10)))
    add("pal8_trns_past", picture(rng, 9, 17, 3), 3, palette=rng.integers(0, 256, (30, 3)), trns=bytes([0, 128, 255, 7]), filters=2)
    add("pal2_trns", picture(rng, 9, 17, 3, 2), 3, 2, palette=rng.integers(0, 256, (4, 3)), trns=bytes([0, 99]), filters=1)
    rgb = rng.choice([10, 20], (30, 29, 3))
    add("rgb_key_hit", rgb, 2, trns=bytes([0, 10, 0, 20, 0, 10]), filters=rng.integers(0, 5, 30))
    add("rgb_key_miss", rgb, 2, trns=bytes([0, 11, 0, 20, 0, 10]), filters=4)
    add("gray_trns_ignored", picture(rng, 12, 14, 0), 0, trns=bytes([0, 5]))
    add("gray4_trns_ignored", picture(rng, 12, 15, 0, 4), 0, 4, trns=bytes([0, 5]))
    add("gray_alpha", _smooth(rng, 70, 45, 2), 4, filters=rng.integers(0, 5, 70))
    _CACHE.update(out)
    return _CACHE


# ---- streams the parser and the inflater must refuse: (name, stream, status, a piece of the message) -------------------------
ST_ERR_INVALID, ST_ERR_UNSUPPORTED = 1, 4


def small_valid(**kw):
    rng = np.random.default_rng(7)
    return write_png(_smooth(rng, 6, 9, 3), 2, filters=[0, 1, 2, 3, 4, 1], **kw)


def _raw_stream(chunks):
    return SIG + b"".join(chunks)


def malformed():
    rng = np.random.default_rng(11)
    px = _smooth(rng, 6, 9, 3)
    raw = filter_rows(scanlines(px, 2, 8), 3, [0, 1, 2, 3, 4, 1])
    z = deflate(raw.tobytes())
    idat, iend = chunk(b"IDAT", z), chunk(b"IEND")
    hdr = ihdr(9, 6, 8, 2)
    pal = chunk(b"PLTE", bytes(range(12)))
    out = []

    def add(name, stream, status, piece):
        out.append((name, bytes(stream), status, piece))

    add("bad_signature", b"\x89PNG\r\n\x1a\r" + hdr + idat + iend, ST_ERR_INVALID, "signature")
    add("jpeg_bytes", b"\xff\xd8\xff\xe0" + bytes(40), ST_ERR_INVALID, "signature")
    add("empty", b"", ST_ERR_INVALID, "signature")
    add("sixteen_bit", _raw_stream([ihdr(9, 6, 16, 2), idat, iend]), ST_ERR_UNSUPPORTED, "16-bit")
    add("adam7", _raw_stream([ihdr(9, 6, 8, 2, interlace=1), idat, iend]), ST_ERR_UNSUPPORTED, "Adam7")
    add("too_wide", _raw_stream([ihdr(65536, 1, 8, 0), idat, iend]), ST_ERR_UNSUPPORTED, "65535")
    add("bad_interlace", _raw_stream([ihdr(9, 6, 8, 2, interlace=2), idat, iend]), ST_ERR_INVALID, "interlace")
    add("bad_depth", _raw_stream([ihdr(9, 6, 4, 2), idat, iend]), ST_ERR_INVALID, "bit depth")
    add("bad_colour_type", _raw_stream([ihdr(9, 6, 8, 5), idat, iend]), ST_ERR_INVALID, "colour type")
    add("bad_compression", _raw_stream([ihdr(9, 6, 8, 2, compression=1), idat, iend]), ST_ERR_INVALID, "compression method")
    add("bad_filter_method", _raw_stream([ihdr(9, 6, 8, 2, filt=1), idat, iend]), ST_ERR_INVALID, "filter method")
    add("zero_width", _raw_stream([ihdr(0, 6, 8, 2), idat, iend]), ST_ERR_INVALID, "size")
    add("ihdr_short", _raw_stream([chunk(b"IHDR", bytes(12)), idat, iend]), ST_ERR_INVALID, "IHDR of 12")
    add("no_ihdr", _raw_stream([idat, iend]), ST_ERR_INVALID, "not IHDR")
    add("second_ihdr", _raw_stream([hdr, hdr, idat, iend]), ST_ERR_INVALID, "second IHDR")
    add("no_idat", _raw_stream([hdr, iend]), ST_ERR_INVALID, "no IDAT")
    add("no_iend", _raw_stream([hdr, idat]), ST_ERR_INVALID, "no IEND")
    add("plte_after_idat", _raw_stream([hdr, idat, pal, iend]), ST_ERR_INVALID, "PLTE after IDAT")
    add("plte_bad_length", _raw_stream([hdr, chunk(b"PLTE", bytes(10)), idat, iend]), ST_ERR_INVALID, "PLTE of 10")
    add("plte_twice", _raw_stream([hdr, pal, pal, idat, iend]), ST_ERR_INVALID, "second PLTE")
    add("plte_in_gray", _raw_stream([ihdr(9, 6, 8, 0), pal, idat, iend]), ST_ERR_INVALID, "PLTE in a gray")
    add("palette_without_plte", _raw_stream([ihdr(9, 6, 8, 3), idat, iend]), ST_ERR_INVALID, "without PLTE")
    add("trns_before_plte", _raw_stream([ihdr(9, 6, 8, 3), chunk(b"tRNS", b"\x01"), pal, idat, iend]), ST_ERR_INVALID, "tRNS before PLTE")
    add("trns_after_idat", _raw_stream([hdr, idat, chunk(b"tRNS", bytes(6)), iend]), ST_ERR_INVALID, "tRNS after IDAT")
    add("trns_longer_than_palette", _raw_stream([ihdr(9, 6, 8, 3), pal, chunk(b"tRNS", bytes(5)), idat, iend]), ST_ERR_INVALID, "tRNS of 5")
    add("trns_bad_length_rgb", _raw_stream([hdr, chunk(b"tRNS", bytes(2)), idat, iend]), ST_ERR_INVALID, "tRNS of 2")
    add("trns_with_alpha", _raw_stream([ihdr(9, 6, 8, 6), chunk(b"tRNS", bytes(2)), idat, iend]), ST_ERR_INVALID, "alpha channel")
    add("idat_not_consecutive", _raw_stream([hdr, chunk(b"IDAT", z[:10]), chunk(b"tEXt", b"k\0v"), chunk(b"IDAT", z[10:]), iend]), ST_ERR_INVALID,
        "not consecutive")
    add("unknown_critical", _raw_stream([hdr, chunk(b"ABCD", b"xyz"), idat, iend]), ST_ERR_INVALID, "critical chunk ABCD")
    add("bad_chunk_type", _raw_stream([hdr, chunk(b"a1cd", b""), idat, iend]), ST_ERR_INVALID, "chunk type")
    add("chunk_runs_past_end", _raw_stream([hdr, struct.pack(">I", 1000) + b"IDAT" + z]), ST_ERR_INVALID, "runs past the end")
    add("iend_with_data", _raw_stream([hdr, idat, chunk(b"IEND", b"x")]), ST_ERR_INVALID, "IEND of 1")
    for name, chunks in (("IHDR", [chunk(b"IHDR", hdr[8:21], crc=1), idat, iend]), ("IDAT", [hdr, chunk(b"IDAT", z, crc=2), iend]),
                         ("IEND", [hdr, idat, chunk(b"IEND", crc=3)]), ("PLTE", [hdr, chunk(b"PLTE", bytes(12), crc=4), idat, iend]),
                         ("tRNS", [hdr, chunk(b"tRNS", bytes(6), crc=5), idat, iend])):
        add("bad_crc_" + name, _raw_stream(chunks), ST_ERR_INVALID, "chunk %s fails its CRC-32" % name)
    # the data: lengths, filter types, and what the inflater refuses
    add("too_few_rows", write_png(px, 2, zdata=deflate(raw[:5].tobytes())), ST_ERR_INVALID, "inflated length 140")
    add("too_many_rows", write_png(px, 2, zdata=deflate(raw.tobytes() + bytes(28))), ST_ERR_INVALID, "more output than")
    add("one_byte_more", write_png(px, 2, zdata=deflate(raw.tobytes() + b"\0")), ST_ERR_INVALID, "more output than")
    bad = raw.copy()
    bad[3, 0] = 5
    add("filter_type_5", write_png(px, 2, zdata=deflate(bad.tobytes())), ST_ERR_INVALID, "row 3 has filter type 5")
    add("adler", write_png(px, 2, zdata=z[:-1] + bytes([z[-1] ^ 0x55])), ST_ERR_INVALID, "Adler-32 mismatch")
    add("zlib_truncated", write_png(px, 2, zdata=z[:len(z) // 2]), ST_ERR_INVALID, "truncated input")
    add("zlib_no_data", write_png(px, 2, zdata=b""), ST_ERR_INVALID, "truncated input")
    add("zlib_bad_method", write_png(px, 2, zdata=b"\x79\x9b" + z[2:]), ST_ERR_INVALID, "compression method")
    add("zlib_dictionary", write_png(px, 2, zdata=b"\x78\xbb" + z[2:]), ST_ERR_INVALID, "preset dictionary")
    add("zlib_fcheck", write_png(px, 2, zdata=b"\x78\x9d" + z[2:]), ST_ERR_INVALID, "FCHECK")
    add("block_type_3", write_png(px, 2, zdata=b"\x78\x9c\x07"), ST_ERR_INVALID, "block type 3")
    add("stored_nlen", write_png(px, 2, zdata=b"\x78\x9c\x01\x05\x00\x05\x00abcde"), ST_ERR_INVALID, "LEN/NLEN")
    return out
