"""No GPU: the PNG encoder's definition (tests/ref_png_encode_np.py) against independent decoders -- zlib's inflater, zlib.crc32,
zlib.adler32, the library's PNG decoder and Pillow --, st_png_encode_host against the definition byte for byte, its size against
zlib's Z_RLE, the code construction on synthetic histograms, the argument message, the registration, the refusals and the
engine's row check.  DESIGN.md 4.18."""
import math
import os
import zlib

import numpy as np
import pytest

import ref_png_encode_np as ref
from png_encode_cases import CASES, FILTERS, PICTURES, RUN_LENGTHS, SMALL_PICTURES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# st_png_encode_host's IDAT payload against zlib's Z_RLE stream of the same filtered bytes, as measured (DESIGN.md 4.18 has every
# figure).  Frames of at least one piece (32 768 filtered bytes): the worst ratio over PICTURES is 1.0041 (sheet_160x200x3),
# asserted rounded up to the next half per cent.  Frames below a piece: a fixed cost of some tens of bytes per stream -- the worst
# over SMALL_PICTURES is 37 bytes (gradient_average: 486 against 449), asserted rounded up to the next multiple of 8 --, which is
# 0.4 % of a 64 x 64 photo but 70 % of a 75-byte gradient, so no ratio is claimed there.
SIZE_RATIO = 1.005
SMALL_EXCESS_BYTES = 40


@pytest.fixture(scope="module")
def streams():
    """Per case the definition's stream and the host twin's: computed once, never changed."""
    from scannertools_amd.hip import png_encode_host
    return {name: (ref.encode(fr, flt), png_encode_host(fr, flt)) for name, (fr, flt) in CASES.items()}


def _idat(stream):
    return b"".join(d for t, d, _ in ref.chunks(stream) if t == b"IDAT")


def test_the_definition_holds_against_independent_decoders(streams):
    from scannertools_amd.hip import png_decode_host
    try:
        import io
        from PIL import Image
    except ImportError:
        Image = None
    for name, (fr, flt) in CASES.items():
        want, _ = streams[name]
        chunks = ref.chunks(want)
        pieces = -(-fr.shape[0] * (1 + fr.shape[1] * fr.shape[2]) // ref.PIECE)
        assert [t for t, _, _ in chunks] == [b"IHDR"] + [b"IDAT"] * (pieces + 1) + [b"IEND"], name
        assert all(zlib.crc32(t + d) & 0xFFFFFFFF == crc for t, d, crc in chunks), name
        raw = ref.filter_rows(fr, flt).tobytes()
        data = _idat(want)
        assert data[:2] == b"\x78\x01" and zlib.decompress(data) == raw, name
        assert int.from_bytes(data[-4:], "big") == zlib.adler32(raw) & 0xFFFFFFFF, name
        if flt != "adaptive":
            assert (ref.filter_rows(fr, flt)[:, 0] == FILTERS.index(flt)).all()
        back = png_decode_host(want)
        assert back.shape == fr.shape and np.array_equal(back, fr), name
        if Image is not None:
            pil = np.asarray(Image.open(io.BytesIO(want)))
            assert np.array_equal(pil.reshape(fr.shape), fr), name


def test_the_host_twin_writes_the_definitions_bytes(streams):
    from scannertools_amd.hip import png_encode_bound
    for name, (fr, _) in CASES.items():
        want, got = streams[name]
        assert got == want, (name, len(got), len(want))
        assert len(got) <= png_encode_bound(*fr.shape), name
    # the bound is reached: noise stores every piece
    fr, _ = CASES["noise_90x130x3"]
    assert len(streams["noise_90x130x3"][1]) == png_encode_bound(*fr.shape)


def test_the_cases_are_what_they_claim(streams):
    """Stored beside coded pieces, the 15-bit limit, every run length, a run across every piece boundary."""
    def kinds(name):   # per piece: is its first block a stored one?
        out = []
        for k, (t, d, _) in enumerate(c for c in ref.chunks(streams[name][0])[1:-2]):
            out.append((((d[2] if k == 0 else d[0]) >> 1) & 3) == 0)
        return out
    assert kinds("mixed") == [True, False, True]
    assert kinds("noise_90x130x3") == [True, True]
    assert kinds("zeros_128x1023x1") == [False] * 4
    raw = ref.filter_rows(*CASES["fibonacci"]).tobytes()
    _, counts, ll, cl, _, _ = ref.piece_tables(raw)
    assert max(ll) == 15 and max(cl) <= 7 and sorted(c for c in counts if c) == [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181, 6765, 10946]
    toks = ref.tokens(ref.filter_rows(*CASES["runs"]).tobytes())
    assert {n for _, n in toks} == {0, 3, 257, 258} and len(RUN_LENGTHS) == 11
    # R = 262: a literal, a match of 258 and three literals; R = 518: a literal, two matches of 258 and one literal
    assert ref.tokens(bytes([5] * 262)) == [(5, 0), (0, 258), (0, 3)] and ref.tokens(bytes([5] * 261)) == [(5, 0), (0, 258), (5, 0), (5, 0)]
    assert ref.tokens(bytes([5] * 518)) == [(5, 0), (0, 258), (0, 258), (5, 0)] and ref.tokens(bytes([5] * 4)) == [(5, 0), (0, 3)]
    assert ref.tokens(bytes([5] * 3)) == [(5, 0)] * 3
    for name, size in (("7x4680x1_32767", 32767), ("128x255x1_32768", 32768), ("33x992x1_32769", 32769), ("zeros_128x1023x1", 131072)):
        assert ref.filter_rows(*CASES[name]).size == size


def test_size_against_zlib_rle(streams):
    """The IDAT payload against zlib.compressobj(6, DEFLATED, 15, 8, Z_RLE) fed the same filtered bytes with a full flush every
    32 768: at most SIZE_RATIO on every picture of a piece or more, at most SMALL_EXCESS_BYTES more than it on every smaller
    picture, and no piece anywhere longer than its stored form."""
    assert not set(PICTURES) & set(SMALL_PICTURES)
    for name in PICTURES + SMALL_PICTURES:
        fr, flt = CASES[name]
        raw = ref.filter_rows(fr, flt).tobytes()
        assert (len(raw) >= ref.PIECE - 1) == (name in PICTURES), name
        co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
        yard = b"".join(co.compress(raw[at:at + ref.PIECE]) + co.flush(zlib.Z_FULL_FLUSH) for at in range(0, len(raw), ref.PIECE)) + co.flush()
        payload = len(_idat(streams[name][1]))
        print("%-22s filtered %6d  payload %6d  Z_RLE %6d  %+4d  ratio %.4f" % (name, len(raw), payload, len(yard), payload - len(yard), payload / len(yard)))
        if name in PICTURES:
            assert payload <= SIZE_RATIO * len(yard), (name, payload, len(yard))
        else:
            assert payload <= len(yard) + SMALL_EXCESS_BYTES, (name, payload, len(yard))
    for name, (fr, flt) in CASES.items():
        raw_len = ref.filter_rows(fr, flt).size
        for k, (t, d, _) in enumerate(ref.chunks(streams[name][1])[1:-2]):
            piece = min(ref.PIECE, raw_len - k * ref.PIECE)
            assert len(d) - (2 if k == 0 else 0) <= 5 + piece, (name, k)


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


@pytest.mark.parametrize("name,counts,limit", [
    ("one_symbol", [0] * 40 + [17] + [0] * 245, 15),
    ("one_symbol_first", [9] + [0] * 18, 7),
    ("two_symbols", [0, 0, 5, 0, 0, 0, 1000000] + [0] * 279, 15),
    ("all_286_equal", [3] * 286, 15),
    ("fibonacci_20", _fib(20) + [0] * 266, 15),
    ("fibonacci_30", _fib(30) + [0] * 256, 15),
    ("fibonacci_19_limit_7", _fib(19), 7),
    ("fibonacci_19_reversed_limit_7", _fib(19)[::-1], 7),
    ("none", [0] * 19, 7),
])
def test_code_construction_on_synthetic_histograms(name, counts, limit):
    from fractions import Fraction
    from scannertools_amd.hip import png_huff_limited
    got = png_huff_limited(counts, limit).tolist()
    assert max(got) <= limit
    assert sum(Fraction(1, 2 ** v) for v in got if v) == 1, got
    assert all(v > 0 for c, v in zip(counts, got) if c)
    assert sum(1 for v in got if v) == max(2, sum(1 for c in counts if c))
    assert got == ref.huff_lengths(counts, limit)
    # a more frequent symbol never has the longer code
    used = [(c, v) for c, v in zip(counts, got) if c]
    assert all(va <= vb for ca, va in used for cb, vb in used if ca > cb)
    if name == "fibonacci_20":
        assert max(got) == 15          # 19 deep without the limit
    if name == "all_286_equal":
        assert sorted(set(got)) == [8, 9]


def test_code_construction_refusals():
    from scannertools_amd.hip import StError, png_huff_limited
    for counts, limit in (([1], 15), ([1] * 287, 15), ([1] * 19, 4), ([1, 2], 0), ([1, 2], 16), ([2 ** 31, 2 ** 31], 15)):
        with pytest.raises(StError):
            png_huff_limited(counts, limit)


def test_argument_message_round_trips_and_absent_fields_change_nothing():
    from scannertools_amd import _proto
    old = _proto.image_encoder_args(90, "4:2:2", "none", True)
    assert _proto.image_encoder_args(90, "4:2:2", "none", True, "jpeg", "adaptive") == old == _proto.image_encoder_args(90, "4:2:2", 1, 1, 0, 0)
    assert _proto.image_encoder_args() == _proto.image_encoder_args(format="JPEG") and b"" == _proto.image_encoder_args(0, "")[0:0]
    assert "format" not in _proto.parse_image_encoder_args(old) and "png_filter" not in _proto.parse_image_encoder_args(old)
    png = _proto.image_encoder_args(90, "4:2:2", "none", True, "png", "paeth")
    assert png == old + bytes([5 << 3, 1, 6 << 3, 5])
    assert _proto.parse_image_encoder_args(png) == {"quality": 90, "subsampling": "4:2:2", "restart": "NONE", "optimize": True, "format": "PNG", "png_filter": "PAETH"}
    for k, name in enumerate(("adaptive", "none", "sub", "up", "average", "paeth")):
        msg = _proto.image_encoder_args(format="png", png_filter=name)
        assert _proto.parse_image_encoder_args(msg).get("png_filter", "ADAPTIVE") == name.upper() and msg == _proto.image_encoder_args(format=1, png_filter=k)
    assert _proto.parse_image_encoder_args(_proto.image_encoder_args(format=7, png_filter=-1))["format"] == 7
    assert _proto.parse_image_encoder_args(_proto.image_encoder_args(format=7, png_filter=-1))["png_filter"] == -1
    for bad in ({"format": "gif"}, {"png_filter": "best"}, {"format": None}, {"png_filter": True}, {"format": 1.0}):
        with pytest.raises(ValueError):
            _proto.image_encoder_args(**bad)
    text = open(os.path.join(ROOT, "scannertools_amd", "scanner_kernels", "scannertools_imgproc_amd.proto")).read()
    assert "message ImageEncoderArgsWithFormat {" in text and "Format format = 5;" in text and "PngFilter png_filter = 6;" in text


def test_registration_and_validation():
    """The op is registered as before, once per device; unknown enum values fail validate() with the value in the message, on
    both devices, with no GPU context needed."""
    import re
    from scannertools_amd import _proto, engine
    from scannertools_amd.engine import Client, DeviceType, NamedStream, NamedVideoStream, PerfParams, _CppMultiOpNode
    regs = [r for r in engine.registered_kernels() if r[0] == "ImageEncoder"]
    assert len(regs) == 2 and len({r[1] for r in regs}) == 2
    sc = Client()
    sc.ingest_frames("v", np.zeros((2, 8, 8, 3), np.uint8))
    frame = sc.io.Input([NamedVideoStream(sc, "v")])
    for dev in (DeviceType.CPU, DeviceType.GPU):
        for args, words in ((_proto.image_encoder_args(format=2), "ImageEncoder: format 2 is not supported (JPEG or PNG)"),
                            (_proto.image_encoder_args(format=-1), "ImageEncoder: format -1 is not supported (JPEG or PNG)"),
                            (_proto.image_encoder_args(format="png", png_filter=6), "ImageEncoder: png_filter 6 is not supported"),
                            (_proto.image_encoder_args(png_filter=-2), "ImageEncoder: png_filter -2 is not supported"),
                            (_proto.image_encoder_args(quality=101, format="png"), "ImageEncoder: quality 101 is outside 1..100")):
            with pytest.raises(RuntimeError, match=re.escape(words)):
                sc.run(sc.io.Output(_CppMultiOpNode(sc, "ImageEncoder", [frame], dev, None, args), [NamedStream(sc, "o")]), PerfParams.estimate())
    with pytest.raises(ValueError, match="format must be one of"):
        sc.ops.ImageEncoder(frame=frame, format="gif")


def test_host_refusals_and_their_words():
    from scannertools_amd import _native
    from scannertools_amd.hip import StError, png_encode_bound, png_encode_host, png_filter
    import ctypes
    L = _native.lib()
    msg = ctypes.create_string_buffer(160)
    for (h, w, c, f), words in (((8, 8, 2, 5), "2 channel(s) cannot be written (1: gray, 3: R, G, B, 4: R, G, B, A)"),
                                ((8, 8, 5, 5), "5 channel(s) cannot be written"),
                                ((0, 8, 3, 5), "frame size 8x0 is outside 1..65535"),
                                ((8, 65536, 3, 5), "frame size 65536x8 is outside 1..65535"),
                                ((8, 8, 3, 6), "filter 6 is not supported (ST_PNG_FILTER_NONE = 0 .. ST_PNG_FILTER_PAETH = 4, ST_PNG_FILTER_ADAPTIVE = 5)"),
                                ((8, 8, 3, -1), "filter -1 is not supported")):
        assert L.st_png_encode_check(h, w, c, f, msg, 160) == 1 and words in msg.value.decode(), (words, msg.value)
        size = ctypes.c_size_t(77)
        buf = np.full(64, 0xA5, np.uint8)
        assert L.st_png_encode_host(buf.ctypes.data, h, w, c, f, buf.ctypes.data, 64, ctypes.byref(size)) == 1
        assert size.value == 77 and (buf == 0xA5).all()
    assert L.st_png_encode_check(8, 8, 3, 5, msg, 160) == 0 and msg.value == b""
    assert L.st_png_encode_bound(8, 8, 2) == -1 and L.st_png_encode_bound(65535, 65535, 4) > 4 * 65535 * 65535
    with pytest.raises(StError, match="2 channel"):
        png_encode_host(np.zeros((4, 4, 2), np.uint8))
    with pytest.raises(StError, match="outside 1..65535"):
        png_encode_bound(0, 4, 3)
    with pytest.raises(ValueError, match="png filter must be one of"):
        png_encode_host(np.zeros((4, 4, 3), np.uint8), "best")
    assert [png_filter(n) for n in FILTERS] == [0, 1, 2, 3, 4, 5] and png_filter(3) == 3
    # a buffer too small: refused, nothing written; a null buffer: the size alone
    fr = np.zeros((4, 4, 3), np.uint8)
    size, buf = ctypes.c_size_t(0), np.full(200, 0xA5, np.uint8)
    assert L.st_png_encode_host(fr.ctypes.data, 4, 4, 3, 5, None, 0, ctypes.byref(size)) == 0 and size.value == len(png_encode_host(fr))
    assert L.st_png_encode_host(fr.ctypes.data, 4, 4, 3, 5, buf.ctypes.data, size.value - 1, ctypes.byref(size)) == 1 and (buf == 0xA5).all()
    assert 2 * (1 + 2 * 3) + 68 + 17 == png_encode_bound(2, 2, 3) and math.ceil(6220800 / 32768) == 190


def test_the_engines_row_check_widens_only_under_png():
    from scannertools_amd.engine import Client, NamedVideoStream
    sc = Client()
    sc.ingest_frames("gray", np.zeros((3, 6, 5, 1), np.uint8))
    sc.ingest_frames("two", np.zeros((3, 6, 5, 2), np.uint8))
    gray, two = sc.io.Input([NamedVideoStream(sc, "gray")]), sc.io.Input([NamedVideoStream(sc, "two")])
    with pytest.raises(ValueError, match=r"ImageEncoder: row 0 is \(6, 5, 1\) uint8, not an \(h, w, 3\) uint8 frame"):
        sc.ops.ImageEncoder(frame=gray).rows([0, 1])
    with pytest.raises(ValueError, match=r"ImageEncoder: row 0 is \(6, 5, 1\) uint8, not an \(h, w, 3\) uint8 frame"):
        sc.ops.ImageEncoder(frame=gray, format="jpeg", png_filter="paeth").rows([0, 1])
    with pytest.raises(ValueError, match=r"ImageEncoder: row 1 is \(6, 5, 2\) uint8, not an \(h, w, 1 \| 3 \| 4\) uint8 frame"):
        sc.ops.ImageEncoder(frame=two, format="png").rows([1])
    assert sc.ops.ImageEncoder(frame=gray, format="png").png and not sc.ops.ImageEncoder(frame=gray).png
