"""CPU: the host side of the PNG decoder -- the library's own inflater against Python's zlib, the container parser on every
refusal and malformation, the CPU twin of the kernels (st_png_decode_host) against the frames the pixel arrays give under the
layout table, against Pillow's golden frames and against Pillow reading the hand-written streams; the proto field; the
stand-alone sanitizer run of the host sources."""
import ctypes
import io
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import png_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = 1, 4


@pytest.fixture(scope="module")
def hip():
    from scannertools_amd import hip
    return hip


def _inflate(hip, z, size):
    """(status, message or data) of st_zlib_inflate into exactly `size` bytes."""
    from scannertools_amd._native import StError
    try:
        return 0, hip.zlib_inflate(z, size)
    except StError as e:
        return e.status, str(e)


# ---- the inflater --------------------------------------------------------------------------------------------------------------
def _mixed_input(rng):
    """Runs, repeats at distances 1, 2, 258, 32767 and 32768, and noise, in a random order, behind 33 000 bytes to reach back into."""
    out = bytearray(rng.integers(0, 256, 2000).astype(np.uint8).tobytes() * 17)[:33000]
    for _ in range(int(rng.integers(4, 12))):
        kind = int(rng.integers(0, 3))
        if kind == 0:
            out += bytes([int(rng.integers(0, 256))]) * int(rng.integers(1, 700))
        elif kind == 1:
            d = int(rng.choice([1, 2, 258, 32767, 32768]))
            for _ in range(int(rng.integers(3, 600))):
                out.append(out[-d])
        else:
            out += rng.integers(0, int(rng.choice([2, 16, 256])), int(rng.integers(1, 900))).astype(np.uint8).tobytes()
    return bytes(out)


def test_inflater_equals_zlib_on_200_inputs_at_every_level_and_strategy(hip):
    rng = np.random.default_rng(1950)
    strategies = [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED]
    seen = set()
    for i in range(200):
        data = _mixed_input(rng)
        level, strategy = i % 10, strategies[(i // 10) % 5]
        seen.add((level, strategy))
        z = pc.deflate(data, level, strategy)
        assert zlib.decompress(z) == data
        st, got = _inflate(hip, z, len(data))
        assert st == 0 and got == data, (i, level, strategy, got if st else "")
    assert len(seen) == 50


def test_inflater_block_kinds_flushes_and_long_stored_streams(hip):
    rng = np.random.default_rng(3)
    text = bytes(rng.integers(97, 101, 5000).astype(np.uint8))
    # fixed blocks need compressible data; the first bits of the deflate data tell the block type
    assert (pc.deflate(text, 6, zlib.Z_FIXED)[2] >> 1) & 3 == 1 and (pc.deflate(text, 6)[2] >> 1) & 3 == 2 and (pc.deflate(text, 0)[2] >> 1) & 3 == 0
    for flush in (zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH):
        co = zlib.compressobj(6)
        z = b""
        for k in range(0, len(text), 700):
            z += co.compress(text[k:k + 700]) + co.flush(flush) + co.flush(flush)   # empty stored blocks in mid-stream
        z += co.flush()
        assert _inflate(hip, z, len(text)) == (0, text)
    big = rng.integers(0, 256, 200000).astype(np.uint8).tobytes()   # level 0: four stored blocks
    assert _inflate(hip, zlib.compress(big, 0), len(big)) == (0, big)
    assert _inflate(hip, zlib.compress(b"", 6), 0) == (0, b"")
    for wbits in (9, 12, 15):
        assert _inflate(hip, pc.deflate(text, 6, wbits=wbits), len(text)) == (0, text)


def test_inflater_never_writes_past_the_buffer(hip):
    from scannertools_amd import _native
    rng = np.random.default_rng(4)
    data = bytes(rng.integers(97, 100, 3000).astype(np.uint8)) + bytes(500)
    for level in (0, 1, 6):
        z = zlib.compress(data, level)
        assert _inflate(hip, z, len(data)) == (0, data)                    # exactly large enough
        st, msg = _inflate(hip, z, len(data) - 1)                          # one byte short
        assert st == INVALID and "more output than the buffer holds" in msg
        buf = np.full(len(data) + 64, 0xA5, np.uint8)
        produced, m = ctypes.c_size_t(0), ctypes.create_string_buffer(160)
        assert _native.lib().st_zlib_inflate(z, len(z), buf.ctypes.data, len(data) - 1, ctypes.byref(produced), m, 160) == INVALID
        assert (buf[len(data) - 1:] == 0xA5).all()


class _Bits:
    """Deflate's bit order: fields from the least significant bit up, Huffman codes from their most significant bit."""

    def __init__(self):
        self.v, self.n = 0, 0

    def bits(self, value, count):
        self.v |= value << self.n
        self.n += count
        return self

    def code(self, value, count):
        for k in range(count - 1, -1, -1):
            self.bits((value >> k) & 1, 1)
        return self

    def fixed_lit(self, s):
        if s < 144:
            return self.code(0x30 + s, 8)
        if s < 256:
            return self.code(0x190 + s - 144, 9)
        return self.code(s - 256, 7) if s < 280 else self.code(0xC0 + s - 280, 8)

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def _canonical(lens):
    """{symbol: (code, length)} of a list of code lengths (RFC 1951 3.2.2)."""
    out, code = {}, 0
    for length in range(1, 16):
        for s, ln in enumerate(lens):
            if ln == length:
                out[s] = (code, length)
                code += 1
        code <<= 1
    return out


def _dynamic(litlens, distlens, symbols, cl_lens=None):
    """One final dynamic block: the code lengths are written one by one with a code length code of sixteen 4-bit codes (or
    cl_lens), then `symbols`: ('l', s) a literal/length symbol, ('d', s) a distance symbol, ('x', value, bits) extra bits."""
    b = _Bits().bits(1, 1).bits(2, 2).bits(len(litlens) - 257, 5).bits(len(distlens) - 1, 5).bits(15, 4)
    cl = [4] * 16 + [0, 0, 0] if cl_lens is None else cl_lens
    for s in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15):
        b.bits(cl[s], 3)
    clc = _canonical(cl)
    for ln in list(litlens) + list(distlens):
        if ln in clc:                       # (a malformed cl_lens is refused before the lengths are read)
            b.code(*clc[ln])
    lit, dist = _canonical(litlens), _canonical(distlens)
    for sym in symbols:
        if sym[0] == "x":
            b.bits(sym[1], sym[2])
        else:
            b.code(*(lit if sym[0] == "l" else dist)[sym[1]])
    return b.bytes()


def _zl(deflate_bytes, data=b""):
    return b"\x78\x9c" + deflate_bytes + zlib.adler32(data).to_bytes(4, "big")


def _litlens(spec):
    lens = [0] * 258
    for s, ln in spec.items():
        lens[s] = ln
    return lens


def test_inflater_hand_built_streams_it_must_accept(hip):
    # RFC 1951 allows a single distance code of length 1: 'a', then length 3 at distance 1
    z = _zl(_dynamic(_litlens({97: 1, 256: 2, 257: 2}), [1], [("l", 97), ("l", 257), ("d", 0), ("l", 256)]), b"aaaa")
    assert zlib.decompress(z) == b"aaaa" and _inflate(hip, z, 4) == (0, b"aaaa")
    # a block without any distance code, literals only
    z = _zl(_dynamic(_litlens({97: 1, 98: 2, 256: 2}), [0], [("l", 97), ("l", 98), ("l", 256)]), b"ab")
    assert zlib.decompress(z) == b"ab" and _inflate(hip, z, 2) == (0, b"ab")
    # the farthest and longest match there is: 32 768 stored bytes, then length 258 at distance 32 768 in a fixed block
    data = np.random.default_rng(5).integers(0, 256, 32768).astype(np.uint8).tobytes()
    stored = b"\x00" + (32768).to_bytes(2, "little") + (32768 ^ 0xFFFF).to_bytes(2, "little") + data
    fixed = _Bits().bits(1, 1).bits(1, 2).fixed_lit(285).code(29, 5).bits(32768 - 24577, 13).fixed_lit(256).bytes()
    z = _zl(stored + fixed, data + data[:258])
    assert zlib.decompress(z) == data + data[:258] and _inflate(hip, z, 32768 + 258) == (0, data + data[:258])
    # codes longer than the lookahead table: lengths 1 .. 14 and two of 15
    lens = _litlens({256: 1, 77: 14, 78: 15, 79: 15})
    for k in range(12):
        lens[65 + k] = k + 2
    text = bytes(range(65, 80)) * 3
    z = _zl(_dynamic(lens, [0], [("l", c) for c in text] + [("l", 256)]), text)
    assert zlib.decompress(z) == text and _inflate(hip, z, len(text)) == (0, text)


MALFORMED_DEFLATE = [
    ("block type 3", _Bits().bits(1, 1).bits(3, 2).bytes(), "block type 3"),
    ("stored LEN / NLEN", b"\x01\x05\x00\x05\x00abcde", "LEN/NLEN mismatch"),
    ("over-subscribed code length codes", _dynamic(_litlens({256: 1}), [0], [], cl_lens=[1] * 19), "over-subscribed code length"),
    ("incomplete code length codes", _dynamic(_litlens({256: 1}), [0], [], cl_lens=[1] + [0] * 18), "incomplete code length"),
    ("over-subscribed literals", _dynamic(_litlens({97: 1, 98: 1, 256: 1}), [0], [("l", 256)]), "over-subscribed literal/length"),
    ("incomplete literals", _dynamic(_litlens({97: 1, 256: 2}), [0], [("l", 256)]), "incomplete literal/length"),
    ("no end-of-block code", _dynamic(_litlens({97: 1, 98: 1}), [0], [("l", 97)]), "incomplete literal/length"),
    ("over-subscribed distances", _dynamic(_litlens({97: 1, 256: 1}), [1, 1, 1], [("l", 256)]), "over-subscribed distance"),
    ("incomplete distances", _dynamic(_litlens({97: 1, 256: 1}), [2, 2], [("l", 256)]), "incomplete distance"),
    ("length symbol 286", _Bits().bits(1, 1).bits(1, 2).fixed_lit(97).fixed_lit(286).bytes() + b"\0\0", "invalid length symbol 286"),
    ("length symbol 287", _Bits().bits(1, 1).bits(1, 2).fixed_lit(97).fixed_lit(287).bytes() + b"\0\0", "invalid length symbol 287"),
    ("distance symbol 30", _Bits().bits(1, 1).bits(1, 2).fixed_lit(97).fixed_lit(257).code(30, 5).bytes() + b"\0\0", "invalid distance symbol 30"),
    ("distance symbol 31", _Bits().bits(1, 1).bits(1, 2).fixed_lit(97).fixed_lit(257).code(31, 5).bytes() + b"\0\0", "invalid distance symbol 31"),
    ("distance before the start", _Bits().bits(1, 1).bits(1, 2).fixed_lit(97).fixed_lit(257).code(1, 5).fixed_lit(256).bytes(),
     "distance 2 reaches before the start of the output (1 bytes so far)"),
    ("repeat without a previous length", _Bits().bits(1, 1).bits(2, 2).bits(0, 5).bits(0, 5).bits(0, 4).bits(1, 3).bits(0, 3).bits(0, 3).bits(1, 3)
     .code(1, 1).bits(0, 2).bytes() + b"\0\0\0", "no previous length"),
]


@pytest.mark.parametrize("name,deflate_bytes,piece", MALFORMED_DEFLATE, ids=[m[0].replace(" ", "_") for m in MALFORMED_DEFLATE])
def test_inflater_names_each_malformation(hip, name, deflate_bytes, piece):
    z = _zl(deflate_bytes + bytes(4))
    with pytest.raises(zlib.error):
        zlib.decompress(z)                                # the hand-built stream is malformed for zlib too
    st, msg = _inflate(hip, z, 1000)
    assert st == INVALID and piece in msg, msg


def test_inflater_zlib_header_trailer_and_truncation(hip):
    data = bytes(np.random.default_rng(6).integers(97, 101, 600).astype(np.uint8))
    for level in (0, 6):
        z = zlib.compress(data, level)
        for cut in range(len(z)):                          # every truncation, header and trailer included
            st, msg = _inflate(hip, z[:cut], len(data))
            assert st == INVALID and "truncated input" in msg, (cut, msg)
    z = zlib.compress(data, 6)
    for bad, piece in ((b"\x79\x9b" + z[2:], "compression method 9"), (b"\x88\x98" + z[2:], "exceeds 32 KiB"), (b"\x78\x9d" + z[2:], "FCHECK"),
                       (b"\x78\xbb" + z[2:], "preset dictionary"), (z[:-1] + bytes([z[-1] ^ 1]), "Adler-32 mismatch"),
                       (z[:-4] + bytes([z[-4] ^ 0x80]) + z[-3:], "Adler-32 mismatch")):
        st, msg = _inflate(hip, bad, len(data))
        assert st == INVALID and piece in msg, msg


# ---- the container -----------------------------------------------------------------------------------------------------------------
def _decode(hip, stream):
    from scannertools_amd._native import StError
    try:
        return 0, hip.png_decode_host(stream)
    except StError as e:
        return e.status, str(e)


MALFORMED = pc.malformed()


@pytest.mark.parametrize("name,stream,status,piece", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_parser_refuses_with_status_and_message(hip, name, stream, status, piece):
    from scannertools_amd import _native
    st, msg = _decode(hip, stream)
    assert st == status and piece in msg, msg
    info = _native.PngInfo()
    raw = np.zeros(1 << 12, np.uint8)
    assert _native.lib().st_png_filtered(stream, len(stream), raw.ctypes.data, raw.size, ctypes.byref(info)) == status
    assert piece in info.message.decode()


def test_malformed_corpus_covers_the_issue_list():
    names = {m[0] for m in MALFORMED}
    assert {"sixteen_bit", "adam7", "bad_crc_IHDR", "bad_crc_PLTE", "bad_crc_tRNS", "bad_crc_IDAT", "bad_crc_IEND", "plte_after_idat",
            "trns_before_plte", "trns_after_idat", "idat_not_consecutive", "too_few_rows", "one_byte_more", "filter_type_5"} <= names
    assert {m[2] for m in MALFORMED} == {INVALID, UNSUPPORTED}


def test_probe_reports_the_decoded_shape_and_reads_no_further_than_the_first_idat(hip):
    rng = np.random.default_rng(8)
    s = pc.write_png(rng.integers(0, 4, (6, 9)), 3, 2, palette=rng.integers(0, 256, (4, 3)), trns=bytes([1, 2]))
    assert hip.probe_png(s) == {"h": 6, "w": 9, "channels": 4, "color_type": 3, "bit_depth": 2, "interlace": 0, "palette_entries": 4, "trns_entries": 2}
    cut = s[:-12]                                          # nothing behind the first IDAT is read: the IEND chunk is missing
    assert hip.probe_png(cut)["channels"] == 4
    assert _decode(hip, cut)[0] == INVALID
    assert hip.probe_png(pc.small_valid()) == {"h": 6, "w": 9, "channels": 3, "color_type": 2, "bit_depth": 8, "interlace": 0, "palette_entries": 0,
                                               "trns_entries": 0}


def test_every_truncation_of_a_valid_stream_is_refused(hip):
    s = pc.small_valid()
    assert _decode(hip, s)[0] == 0
    for cut in range(len(s)):
        st, msg = _decode(hip, s[:cut])
        assert st == INVALID and msg, cut


def test_idat_split_at_every_byte_and_empty_idats(hip):
    whole = pc.small_valid()
    st, want = _decode(hip, whole)
    assert st == 0
    z_len = int.from_bytes(whole[whole.index(b"IDAT") - 4:whole.index(b"IDAT")], "big")
    for level, strategy in ((6, zlib.Z_DEFAULT_STRATEGY), (0, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED)):
        n = z_len if (level, strategy) == (6, zlib.Z_DEFAULT_STRATEGY) else len(pc.deflate(bytes(1), level, strategy)) + 60
        for cut in range(0, n + 1):                         # inside the zlib header, the blocks and the Adler-32 trailer
            st, got = _decode(hip, pc.small_valid(splits=[cut], level=level, strategy=strategy))
            assert st == 0 and (got == want).all(), (level, cut)
    for splits in ([0, 0, 0], [1, 1, 2, 2, 2], [5, 5, 9, z_len, z_len], list(range(1, z_len))):
        st, got = _decode(hip, pc.small_valid(splits=[min(c, z_len) for c in splits]))
        assert st == 0 and (got == want).all(), splits


def test_ancillary_chunks_are_skipped_and_an_apng_decodes_to_its_default_image(hip):
    st, want = _decode(hip, pc.small_valid())
    gama = pc.chunk(b"gAMA", (45455).to_bytes(4, "big"))
    junk = pc.chunk(b"iCCP", b"not a profile", crc=123)        # unchecked: its CRC is not looked at
    actl = pc.chunk(b"acTL", (2).to_bytes(4, "big") + bytes(4))
    fctl = pc.chunk(b"fcTL", bytes(26))
    fdat = pc.chunk(b"fdAT", bytes(4) + b"garbage")
    for before, after in (([gama, junk], [pc.chunk(b"tEXt", b"a\0b")]), ([actl, fctl], [fctl, fdat, fdat])):
        st, got = _decode(hip, pc.small_valid(before_idat=before, after_idat=after))
        assert st == 0 and (got == want).all()


# ---- the CPU twin ------------------------------------------------------------------------------------------------------------------
def test_case_list_covers_the_geometry_the_issue_names():
    names = set(pc.cases())
    for h in (1, 2, 63, 64, 65, 129):
        for w in (1, 2, 3, 63, 64, 65, 131):
            for bpp in (1, 2, 3, 4):
                assert "geom_%dx%d_bpp%d" % (h, w, bpp) in names
    assert {(a, b) for a, b in zip(pc.PAIR_FILTERS[:-1], pc.PAIR_FILTERS[1:])} == {(a, b) for a in range(5) for b in range(5)}
    assert set(pc.BAND_ROWS) == {0, 63, 64, 65, 127, 128}


def test_cpu_twin_equals_the_expected_frames(hip):
    for name, (stream, want) in pc.cases().items():
        got = hip.png_decode_host(stream)
        assert got.shape == want.shape and (got == want).all(), name


def test_stage_one_returns_the_writers_filtered_rows(hip):
    rng = np.random.default_rng(9)
    for ct, depth in ((0, 1), (0, 8), (2, 8), (3, 4), (4, 8), (6, 8)):
        px = pc.picture(rng, 70, 13, ct, depth)
        filters = rng.integers(0, 5, 70)
        raw = pc.filter_rows(pc.scanlines(px, ct, depth), pc.filter_bpp(ct, depth), filters)
        s = pc.write_png(px, ct, depth, filters=filters, palette=rng.integers(0, 256, (16, 3)) if ct == 3 else None)
        got = hip.png_filtered(s)
        assert got.shape == raw.shape and (got == raw).all() and (got[:, 0] == filters).all()


def test_paeth_data_meets_every_tie_and_average_sums_pass_255():
    """The arithmetic cases do what they are there for: computed from the pixel arrays, not from the code under test."""
    for name, bpp in (("paeth_ties_rgb", 3), ("paeth_ties_gray", 1)):
        px = pc.cases()[name][1].astype(np.int64)
        rows = px.reshape(px.shape[0], -1)
        a, b, c = rows[1:, :-bpp], rows[1:, bpp:] * 0 + rows[:-1, bpp:], rows[:-1, :-bpp]
        p = a + b - c
        pa, pb, pc_ = np.abs(p - a), np.abs(p - b), np.abs(p - c)
        # (pa = pb with a != b forces pc = 0, so that tie shows only where a = b; the other two choose between different bytes)
        assert ((pa == pb) & (pa <= pc_)).any() and ((pb == pc_) & (pb < pa) & (b != c)).any()
        assert ((pa == pb) & (pb == pc_)).any() and ((pa == pc_) & (pa <= pb) & (a != c)).any()
    for name, bpp in (("average_carry", 3), ("average_carry_gray", 1)):
        rows = pc.cases()[name][1].astype(np.int64)
        rows = rows.reshape(rows.shape[0], -1)
        assert ((rows[1:, :-bpp] + rows[:-1, bpp:]) > 255).any()


def test_pillow_reads_the_hand_written_streams_to_the_same_frames():
    """Arbitrates the writer and the layout table against libpng; skipped only where Pillow is missing."""
    Image = pytest.importorskip("PIL.Image")
    for name, (stream, want) in pc.cases().items():
        im = Image.open(io.BytesIO(stream))
        got = np.asarray(im.convert({1: "L", 3: "RGB", 4: "RGBA"}[want.shape[2]])).reshape(want.shape)
        assert (got == want).all(), name


def test_cpu_twin_equals_pillows_golden_frames(hip):
    path = os.path.join(ROOT, "tests", "golden", "png_golden.npz")
    gold = np.load(path)
    names = [str(c) for c in gold["cases"]]
    assert os.path.getsize(path) < 1 << 20 and len(names) == 48
    kinds = set()
    for name in names:
        stream = gold[name + "__png"].tobytes()
        info = hip.probe_png(stream)
        kinds.add((info["color_type"], info["bit_depth"], info["trns_entries"] > 0))
        got = hip.png_decode_host(stream)
        assert got.shape == gold[name + "__img"].shape and (got == gold[name + "__img"]).all(), name
    assert kinds >= {(0, 1, False), (0, 8, False), (0, 8, True), (2, 8, False), (2, 8, True), (4, 8, False), (6, 8, False)} | {
        (3, d, t) for d in (1, 2, 4, 8) for t in (False, True)}


# ---- proto, ABI -----------------------------------------------------------------------------------------------------------------
def test_png_field_bytes_both_ways():
    from scannertools_amd import _proto
    assert _proto.image_decoder_args(png="DECODE") == b"\x28\x01" == _proto.image_decoder_args(png="decode") == _proto.image_decoder_args(png=1)
    assert _proto.image_decoder_args(png="REFUSE") == b"\x28\x00" and _proto.image_decoder_args(png=7) == b"\x28\x07"
    assert _proto.image_decoder_args() == b"" and _proto.image_decoder_args("JPEG", "gpu", "subsequence", 2) == b"\x08\x01\x10\x01\x18\x01\x20\x02"
    assert _proto.image_decoder_args("ANY", png="DECODE") == b"\x08\x02\x28\x01"
    assert _proto.image_decoder_args("PNG", None, None, None, "DECODE") == b"\x08\x00\x28\x01"
    assert _proto.parse_image_decoder_args(b"\x08\x00\x28\x01") == {"image_type": "PNG", "png": "DECODE"}
    assert _proto.parse_image_decoder_args(b"\x28\x00") == {"png": "REFUSE"} and _proto.parse_image_decoder_args(b"\x28\x07") == {"png": 7}
    assert _proto.parse_image_decoder_args(b"\x08\x01\x10\x01") == {"image_type": "JPEG", "entropy": "GPU"}
    with pytest.raises(ValueError):
        _proto.image_decoder_args(png="maybe")


def test_no_new_timing_slot_and_no_new_abi_version():
    from scannertools_amd import _native
    assert _native.K_COUNT == 19 and _native.lib().st_abi_version() == 1
    header = open(os.path.join(ROOT, "include", "scannertools_hip.h")).read()
    assert "ST_K_COUNT = 19" in header
    for sym in ("st_png_probe", "st_zlib_inflate", "st_png_filtered", "st_png_decode_host", "st_png_decode_batch"):
        assert sym in _native.SIGNATURES and sym + "(" in header


# ---- the host sources under the sanitizers: a stand-alone program, never loaded into Python ----------------------------------------
def test_host_sources_are_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "png_host_check")
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "scannertools_amd", "csrc"), os.path.join(ROOT, "scripts", "png_host_check.cpp"),
                    os.path.join(ROOT, "scannertools_amd", "csrc", "st_png_host.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "png_host_corpus.bin")], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    last = res.stdout.strip().splitlines()[-1]
    assert last.startswith("png_host_check: ") and last.endswith(" 0 failures") and int(last.split()[1]) >= 50 and int(last.split()[3]) >= 3000
