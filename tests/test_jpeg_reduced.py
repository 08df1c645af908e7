"""CPU: ImageDecoder at scale 1/2, 1/4 and 1/8.  The definition (tests/ref_jpeg_reduced_np.py, libjpeg's scaled decoding restated)
against Pillow's golden frames (tests/golden/jpeg_reduced_golden.npz) and live Pillow; the library's host functions
st_jpeg_scaled_size / st_jpeg_scaled_geometry against the definition's sizes; the ImageDecoderArgs.scale_denom field; the
front end's refusals."""
import ctypes
import hashlib
import io
import json
import os
import types

import numpy as np
import pytest

import ref_jpeg_np as ref
import ref_jpeg_reduced_np as red

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD_PATH = os.path.join(ROOT, "tests", "golden", "jpeg_reduced_golden.npz")
GOLD = np.load(GOLD_PATH)
CASES = [str(c) for c in GOLD["cases"]]                       # "<stream>/<d>": Pillow's frame
REF_ONLY = [str(c) for c in GOLD["restatement_only"]]         # "<stream>/<d>": the restatement's frame, Pillow cannot be asked
ST_ERR_INVALID, ST_ERR_UNSUPPORTED = 1, 4
SAMPLINGS = {"444": (1, 1), "422": (2, 1), "420": (2, 2), "gray": (1, 1)}


def _jpg(name):
    return GOLD[name + "__jpg"].tobytes()


def _same(name, d, got):
    """got equals the golden frame of (name, d), stored whole or as its SHA-256."""
    key = "%s__d%d" % (name, d)
    if key in GOLD.files:
        return got.shape == GOLD[key].shape and np.array_equal(got, GOLD[key])
    return got.shape == tuple(GOLD[key + "_shape"]) and hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == str(GOLD[key + "_sha"])


@pytest.fixture(scope="module")
def L():
    from scannertools_amd import _native
    return _native.lib()


def test_golden_file_holds_the_cases_the_scale_is_held_to():
    assert os.path.getsize(GOLD_PATH) < 400 * 1000
    cells, sizes = set(), set()
    for c in CASES:
        name, d = c.rsplit("/", 1)
        cfg = json.loads(str(GOLD[name + "__cfg"]))
        cells.add((name.split("_")[1], int(d), cfg["quality"], "restart_marker_rows" in cfg))
        sizes.add((cfg["w"], cfg["h"], int(d)))
    for samp in SAMPLINGS:
        for d in (2, 4, 8):
            assert {(samp, d, 30, True), (samp, d, 30, False), (samp, d, 95, True), (samp, d, 95, False)} <= cells, (samp, d)
    for w, h in ((8, 8), (16, 16), (17, 33), (37, 53), (64, 128), (128, 256), (100, 131)):
        assert {(w, h, 2), (w, h, 4), (w, h, 8)} <= sizes, (w, h)
    assert {(40, 3, 2), (3, 40, 2)} <= sizes
    # a side below the denominator (or below 4, where draft() settles on a smaller one): the restatement is the only reference
    assert {c.split("_")[0] for c in REF_ONLY} == {"40x3", "3x40", "1x1", "7x9"}
    assert 8 * len(REF_ONLY) <= len(REF_ONLY) + len(CASES)


def test_restatement_equals_every_golden_frame():
    """Byte for byte, Pillow's frames and (trivially, they are its own) the restatement-only ones."""
    parsed = {}
    for c in CASES + REF_ONLY:
        name, d = c.rsplit("/", 1)
        if name not in parsed:
            parsed[name] = ref.parse(_jpg(name))
        got = red.decode_parsed(parsed[name], int(d))
        s = parsed[name]
        assert got.shape[:2] == red.scaled_size(s["h"], s["w"], int(d)) and got.dtype == np.uint8, c
        assert _same(name, int(d), got), c


def _encode(Image, arr, **kw):
    buf = io.BytesIO()
    Image.fromarray(arr, "RGB" if arr.ndim == 3 else "L").save(buf, "JPEG", **kw)
    return buf.getvalue()


def test_restatement_equals_live_pillow():
    """A seeded sweep: 12 sizes x 4 samplings x 2 qualities x 3 denominators.  Where Pillow's draft() hands out the denominator
    asked for, the restatement equals it byte for byte.  Frames with a side below the denominator (1 x 1; 7 x 9 at 1/8) cannot
    be asked for: there the restatement is its own and only reference, and no more than one case in eight may be such."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(11)
    backed = alone = 0
    for w, h in ((8, 8), (9, 16), (16, 9), (31, 33), (50, 20), (23, 41), (64, 48), (33, 17), (72, 56), (40, 24), (7, 9), (1, 1)):
        for sname, sub in (("444", "4:4:4"), ("422", "4:2:2"), ("420", "4:2:0"), ("gray", None)):
            for q, extra in ((30, dict(restart_marker_rows=1)), (95, dict())):
                arr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
                arr[: h // 2] = (arr[: h // 2].astype(int) // 8 + np.linspace(40, 200, w)[None, :, None]).astype(np.uint8)   # half smooth
                kw = dict(extra, quality=q)
                if sub is None:
                    arr = arr[..., 0]
                else:
                    kw["subsampling"] = sub
                jpg = _encode(Image, arr, **kw)
                parsed = ref.parse(jpg)
                for d in (2, 4, 8):
                    got = red.decode_parsed(parsed, d)
                    assert got.shape[:2] == (-(-h // d), -(-w // d))
                    im = Image.open(io.BytesIO(jpg))
                    im.draft(im.mode, (max(1, w // d), max(1, h // d)))
                    if im.decoderconfig[:1] != (d,):
                        assert min(w, h) < d, (w, h, sname, q, d)
                        alone += 1
                        continue
                    assert im.size == (got.shape[1], got.shape[0]), (w, h, sname, q, d)
                    want = np.asarray(im)
                    want = want if want.ndim == 3 else want[..., None]
                    assert np.array_equal(got, want), (w, h, sname, q, d, int(np.abs(got.astype(int) - want).max()))
                    backed += 1
    assert backed + alone == 288 and 8 * alone <= backed + alone, (backed, alone)


def test_scaled_size(L):
    oh, ow = ctypes.c_int(-1), ctypes.c_int(-1)
    for h, w in ((1, 1), (7, 9), (8, 8), (17, 33), (1080, 1920), (65535, 65535)):
        for d in (1, 2, 4, 8):
            assert L.st_jpeg_scaled_size(h, w, d, ctypes.byref(oh), ctypes.byref(ow)) == 0
            assert (oh.value, ow.value) == red.scaled_size(h, w, d) == (-(-h // d), -(-w // d))
    oh.value = ow.value = -1
    for h, w, d in ((8, 8, 0), (8, 8, 3), (8, 8, 16), (8, 8, -2), (0, 8, 2), (8, 0, 2), (65536, 8, 2), (8, 65536, 2), (-1, 8, 1)):
        assert L.st_jpeg_scaled_size(h, w, d, ctypes.byref(oh), ctypes.byref(ow)) == ST_ERR_INVALID, (h, w, d)
    assert (oh.value, ow.value) == (-1, -1)
    assert L.st_jpeg_scaled_size(8, 8, 2, None, ctypes.byref(ow)) == ST_ERR_INVALID
    from scannertools_amd import hip
    assert hip.jpeg_scaled_size(1080, 1920, 8) == (135, 240) and hip.jpeg_scaled_size(17, 33, 2) == (9, 17)
    for bad in (0, 3, 16, "2", None, True):
        with pytest.raises(ValueError, match="scale"):
            hip.jpeg_scaled_size(8, 8, bad)
    with pytest.raises(ValueError):
        hip.jpeg_scaled_size(0, 8, 2)


def test_scaled_geometry_equals_the_restatement(L):
    """All twelve sampling x denominator cells (and denominator 1), on sizes where every ceil differs; then the table of the
    contract itself; then the refusals."""
    from scannertools_amd import _native, hip
    seen = set()
    for c in CASES + REF_ONLY:
        name, _ = c.rsplit("/", 1)
        if name in seen:
            continue
        seen.add(name)
        jpg, cfg, samp = _jpg(name), json.loads(str(GOLD[name + "__cfg"])), name.split("_")[1]
        H, V = SAMPLINGS[samp]
        comps = [(1, 1)] if samp == "gray" else [(H, V), (1, 1), (1, 1)]
        for d in (1, 2, 4, 8):
            want = red.geometry(cfg["h"], cfg["w"], comps, d)
            got = hip.jpeg_scaled_geometry(jpg, d)
            assert got == {"S": [g["S"] for g in want], "dw": [g["dw"] for g in want], "dh": [g["dh"] for g in want]}, (name, d)
            m = 8 // d
            assert got["S"][0] == m and (samp == "gray" or got["S"][1] == got["S"][2] == (2 * m if samp == "420" and d > 1 else m)), (name, d)
            if d > 1:
                assert all(g["fv"] == 1 for g in want) and [g["fh"] for g in want][1:] == ([2, 2] if samp == "422" else [1, 1][:len(comps) - 1])
    assert {n.split("_")[1] for n in seen} == set(SAMPLINGS)
    # refusals: a bad denominator names itself, a stream the probe refuses keeps the probe's status and message
    jpg = _jpg("16x16_420_q30" if "16x16_420_q30__jpg" in GOLD.files else "16x16_420_q30_rst")
    S, dw, dh, info = (ctypes.c_int * 3)(), (ctypes.c_int * 3)(), (ctypes.c_int * 3)(), _native.JpegInfo()
    for d in (0, 3, 16, -1):
        assert L.st_jpeg_scaled_geometry(jpg, len(jpg), d, S, dw, dh, ctypes.byref(info)) == ST_ERR_INVALID and (b"scale_denom %d" % d) in info.message
        with pytest.raises(hip.StError, match="scale_denom"):
            hip.jpeg_scaled_geometry(jpg, d)
    assert L.st_jpeg_scaled_geometry(jpg, len(jpg), 2, None, dw, dh, None) == ST_ERR_INVALID
    assert L.st_jpeg_scaled_geometry(jpg, len(jpg), 2, S, dw, dh, None) == 0 and list(S) == [4, 8, 8] and list(dw) == [8, 8, 8]
    assert L.st_jpeg_scaled_geometry(jpg[:100], 100, 2, S, dw, dh, ctypes.byref(info)) == ST_ERR_INVALID and info.message
    probe = _native.JpegInfo()
    assert L.st_jpeg_probe(jpg[:100], 100, ctypes.byref(probe)) == ST_ERR_INVALID and probe.message == info.message
    prog = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_golden.npz"))["progressive__jpg"].tobytes()
    assert L.st_jpeg_scaled_geometry(prog, len(prog), 4, S, dw, dh, ctypes.byref(info)) == ST_ERR_UNSUPPORTED and b"progressive" in info.message


def test_image_decoder_args_scale_denom_field():
    from scannertools_amd import _proto
    assert _proto.image_decoder_args() == b"" and _proto.image_decoder_args(scale_denom=None) == b""
    assert _proto.image_decoder_args(scale_denom=0) == b""                                  # proto3 does not write a zero
    for d in (1, 2, 4, 8):
        assert _proto.image_decoder_args(scale_denom=d) == bytes([0x20, d]) == _proto.encode([(4, "int32", d)])   # as protoc writes it
        assert _proto.parse_image_decoder_args(_proto.image_decoder_args(scale_denom=d)) == {"scale_denom": d}
    assert _proto.image_decoder_args("JPEG", "gpu", "subsequence", 4) == b"\x08\x01\x10\x01\x18\x01\x20\x04"
    assert _proto.image_decoder_args("JPEG", "gpu", "subsequence") == b"\x08\x01\x10\x01\x18\x01"       # positional calls mean what they meant
    assert _proto.parse_image_decoder_args(b"\x08\x01\x10\x01\x18\x01\x20\x04") == {"image_type": "JPEG", "entropy": "GPU", "split": "SUBSEQUENCE", "scale_denom": 4}
    assert _proto.parse_image_decoder_args(b"\x08\x01") == {"image_type": "JPEG"}                        # an absent field stays absent: 1
    # a bad value stays a number, a negative one included (an int32 is ten bytes on the wire)
    assert _proto.parse_image_decoder_args(_proto.image_decoder_args(scale_denom=3)) == {"scale_denom": 3}
    assert _proto.image_decoder_args(scale_denom=-2) == b"\x20\xfe" + b"\xff" * 8 + b"\x01"
    assert _proto.parse_image_decoder_args(_proto.image_decoder_args(scale_denom=-2)) == {"scale_denom": -2}
    proto = open(os.path.join(ROOT, "scannertools_amd", "scanner_kernels", "scannertools_imgproc_amd.proto")).read()
    assert "int32 scale_denom = 4;" in proto
    src = open(os.path.join(ROOT, "scannertools_amd", "scanner_kernels", "image_decoder_kernel_hip.cpp")).read()
    assert "st_jpeg_decode_batch_scaled" in src and "f.number == 4" in src


def test_front_end_names_and_value_error():
    from scannertools_amd import _native, engine, hip
    for sym in ("st_jpeg_scaled_size", "st_jpeg_scaled_geometry", "st_jpeg_decode_batch_scaled"):
        assert sym in _native.SIGNATURES and hasattr(_native.lib(), sym)
    assert hip.JPEG_SCALES == (1, 2, 4, 8)
    jpg = _jpg(CASES[0].rsplit("/", 1)[0])
    for bad in (3, 0, 16, -2, "2", None, 2.5, True):
        with pytest.raises(ValueError, match="scale must be one of 1, 2, 4, 8"):
            hip.HipContext.decode_jpeg(None, [jpg], scale=bad)                  # refused before the context is touched
    ops = types.SimpleNamespace(sc=None)
    assert engine._Ops.ImageDecoder(ops, img=None, args={"entropy": "gpu", "scale_denom": 8}).args == b"\x10\x01\x20\x08"
    assert engine._Ops.ImageDecoder(ops, img=None, args={"scale_denom": 3}).args == b"\x20\x03"     # the kernel's validate() refuses it
    assert _native.source_hash() and "st_jpeg_reduced.hip" in open(os.path.join(ROOT, "scannertools_amd", "csrc", "Makefile")).read()
