"""CPU: the ImageDecoder op's definition (tests/ref_jpeg_np.py) against Pillow's golden frames, and the host stage of the
library (st_jpeg_probe / st_jpeg_coefficients: marker parser + Huffman decoder) against the definition, on well-formed,
refused, truncated and corrupted streams."""
import ctypes
import io
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import ref_jpeg_np as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_golden.npz"))
CASES = [str(c) for c in GOLD["cases"]]
REFUSED = [str(c) for c in GOLD["refused"]]
SAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}


def _jpg(name):
    return GOLD[name + "__jpg"].tobytes()


@pytest.fixture(scope="module")
def L():
    from scannertools_amd import _native
    return _native.lib()


@pytest.fixture(scope="module")
def ref_coefficients():
    """The definition's coefficients and tables of every golden case, computed once."""
    return {name: ref.coefficients(_jpg(name)) for name in CASES}


def _coefficients(L, data, cap=None, extra=0):
    """(status, message, coef, quant, info) of st_jpeg_coefficients into a buffer of `cap` (+ `extra` guard) values."""
    from scannertools_amd import _native
    info = _native.JpegInfo()
    n = (1 << 16) if cap is None else cap
    coef = np.full(n + extra, 12345, np.int16)
    quant = np.zeros((3, 64), np.uint16)
    st = L.st_jpeg_coefficients(data, len(data), coef.ctypes.data, n, quant.ctypes.data, ctypes.byref(info))
    return st, info.message.decode(), coef, quant, info


def test_golden_file_holds_the_cases_the_op_is_held_to():
    assert len(CASES) >= 140 and len(REFUSED) == 6 and len(GOLD["batch"]) == 33
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "jpeg_golden.npz")) < 1 << 20
    sizes = {(json.loads(str(GOLD[c + "__cfg"]))["w"], json.loads(str(GOLD[c + "__cfg"]))["h"]) for c in CASES}
    assert {(1, 1), (3, 3), (2, 5), (8, 8), (17, 13), (5, 40), (40, 5), (16, 16), (33, 65), (37, 53), (136, 248), (200, 328), (131, 77)} <= sizes


def test_definition_equals_pillow_golden_frames():
    for name in CASES:
        got, want = ref.decode(_jpg(name)), GOLD[name + "__img"]
        assert got.shape == want.shape and got.dtype == np.uint8, name
        assert np.array_equal(got, want), (name, int(np.abs(got.astype(int) - want).max()))


def test_definition_equals_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    for w, h in ((1, 1), (2, 2), (3, 7), (9, 16), (16, 9), (31, 33), (50, 20)):
        for kw in (dict(quality=50, subsampling="4:2:0"), dict(quality=88, subsampling="4:2:2", optimize=True),
                   dict(quality=97, subsampling="4:4:4", restart_marker_blocks=2), dict(quality=12, subsampling="4:2:0", restart_marker_rows=1)):
            arr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            arr[h // 2:] = (arr[h // 2:] // 8) * 8 + 3          # a flatter half
            buf = io.BytesIO()
            Image.fromarray(arr).save(buf, "JPEG", **kw)
            want = np.asarray(Image.open(io.BytesIO(buf.getvalue())))
            assert np.array_equal(ref.decode(buf.getvalue()), want), (w, h, kw)
        buf = io.BytesIO()
        Image.fromarray(rng.integers(0, 256, (h, w), dtype=np.uint8)).save(buf, "JPEG", quality=70)
        assert np.array_equal(ref.decode(buf.getvalue())[..., 0], np.asarray(Image.open(io.BytesIO(buf.getvalue())))), (w, h)


def test_probe_reports_shape_and_sampling(L):
    from scannertools_amd import _native
    from scannertools_amd.hip import probe_jpeg
    for name in CASES:
        cfg, img = json.loads(str(GOLD[name + "__cfg"])), GOLD[name + "__img"]
        info = _native.JpegInfo()
        data = _jpg(name)
        assert L.st_jpeg_probe(data, len(data), ctypes.byref(info)) == _native.ST_OK, (name, info.message)
        assert info.message == b""
        assert (info.h, info.w, info.channels) == img.shape == (cfg["h"], cfg["w"], img.shape[2]), name
        assert (info.h_samp, info.v_samp) == (SAMPLING[cfg["subsampling"]] if img.shape[2] == 3 else (1, 1)), name
        mcux = -(-cfg["w"] // (8 * info.h_samp))
        want_ri = cfg.get("restart_marker_blocks", 0) or (mcux * cfg["restart_marker_rows"] if "restart_marker_rows" in cfg else 0)
        assert info.restart_interval == want_ri, name
    assert probe_jpeg(_jpg("17x13_smooth_q30_422")) == {"h": 13, "w": 17, "channels": 3, "h_samp": 2, "v_samp": 1, "restart_interval": 0}
    assert L.st_jpeg_probe(_jpg(CASES[0]), 10, None) == _native.ST_ERR_INVALID


def test_coefficients_equal_the_definition(L, ref_coefficients):
    from scannertools_amd import _native
    from scannertools_amd.hip import jpeg_coefficients
    for name in CASES:
        want_c, want_q = ref_coefficients[name]
        st, msg, coef, quant, info = _coefficients(L, _jpg(name), cap=want_c.size, extra=64)
        assert st == _native.ST_OK, (name, msg)
        assert np.array_equal(coef[:want_c.size], want_c), name
        assert (coef[want_c.size:] == 12345).all(), name                      # nothing past the stream's own blocks
        assert np.array_equal(quant[:info.channels], want_q), name
    c, q = jpeg_coefficients(_jpg("33x65_noise_q100_420_rst3"))
    assert np.array_equal(c, ref_coefficients["33x65_noise_q100_420_rst3"][0]) and q.shape == (3, 64)


def test_refused_streams_return_their_status_and_name_the_cause(L):
    from scannertools_amd import _native
    from scannertools_amd.hip import StError, probe_jpeg
    for name in REFUSED:
        data, status, cause = _jpg(name), int(GOLD[name + "__status"]), str(GOLD[name + "__cause"])
        st, msg, coef, _, _ = _coefficients(L, data)
        assert st == status and cause in msg, (name, st, msg)
        assert (coef == 12345).all() or name == "truncated_scan", name
        if name != "truncated_scan":                                           # its markers are whole: the scan fails, not the probe
            info = _native.JpegInfo()
            assert L.st_jpeg_probe(data, len(data), ctypes.byref(info)) == status and cause.encode() in info.message, name
            with pytest.raises(StError, match=cause):
                probe_jpeg(data)
    assert L.st_jpeg_coefficients(None, 0, None, 0, None, None) == _native.ST_ERR_INVALID


def _patched(data, old, new):
    assert data.count(old) == 1
    return data.replace(old, new)


def test_other_stream_kinds_are_refused_by_name(L):
    """Marker-level variants made by editing a golden stream: what the format allows and this decoder declines."""
    from scannertools_amd import _native
    base = _jpg("16x16_smooth_q75_444")
    sof = base.index(b"\xff\xc0")
    dqt = base.index(b"\xff\xdb")
    variants = {
        "extended": base[:sof + 1] + b"\xc1" + base[sof + 2:],
        "lossless": base[:sof + 1] + b"\xc3" + base[sof + 2:],
        "arithmetic": base[:sof + 1] + b"\xc9" + base[sof + 2:],
        "12-bit": base[:sof + 1] + b"\xc1" + base[sof + 2:sof + 4] + b"\x0c" + base[sof + 5:],
        "16-bit quantisation": base[:dqt + 4] + bytes([0x10 | base[dqt + 4]]) + base[dqt + 5:],
        "sampling": base[:sof + 11] + b"\x41" + base[sof + 12:],               # luma 4x1
        "Adobe": base[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + base[base.index(b"\xff\xdb"):],   # transform 0, no JFIF
        "multiple scans": _patched(base, b"\xff\xda\x00\x0c\x03", b"\xff\xda\x00\x08\x01")[:base.index(b"\xff\xda") + 7]
                          + base[base.index(b"\xff\xda") + 11:],   # a scan of the first component alone
    }
    for cause, data in variants.items():
        st, msg, _, _, _ = _coefficients(L, data)
        assert st == _native.ST_ERR_UNSUPPORTED and cause in msg, (cause, st, msg)
    # fill bytes before a marker and an unknown APPn / COM are skipped
    filled = base[:dqt] + b"\xff\xff\xff" + base[dqt:sof] + b"\xff\xfe\x00\x05abc" + b"\xff\xe5\x00\x04zz" + base[sof:]
    st, msg, coef, _, _ = _coefficients(L, filled)
    assert st == _native.ST_OK and np.array_equal(coef[:3 * 4 * 64], ref.coefficients(base)[0]), msg


def test_truncated_and_corrupted_streams_return_a_status(L, ref_coefficients):
    from scannertools_amd import _native
    ok = (_native.ST_OK, _native.ST_ERR_INVALID, _native.ST_ERR_UNSUPPORTED)
    for name in ("3x3_noise_q75_444", "17x13_smooth_q90_422_rstrow"):   # the second has a restart marker
        data = _jpg(name)
        need = ref_coefficients[name][0].size
        for cut in range(len(data)):
            st, msg, coef, _, _ = _coefficients(L, data[:cut], cap=need, extra=64)
            assert st in ok and (coef[need:] == 12345).all(), (name, cut)
            assert st != _native.ST_OK or cut >= len(data) - 2, (name, cut, msg)    # only the EOI marker may be missing
            assert st == _native.ST_OK or msg, (name, cut)
    name = "17x13_noise_q90_422_rstrow"
    data, need = bytearray(_jpg(name)), ref_coefficients[name][0].size
    rng = np.random.default_rng(11)
    statuses = set()
    for _ in range(2000):
        pos, val = int(rng.integers(2, len(data))), int(rng.integers(0, 256))
        old, data[pos] = data[pos], val
        st, msg, coef, _, _ = _coefficients(L, bytes(data), cap=need, extra=64)
        data[pos] = old
        assert st in ok and (coef[need:] == 12345).all(), (pos, val)
        statuses.add(st)
    assert _native.ST_OK in statuses and _native.ST_ERR_INVALID in statuses


def test_coefficient_cap_is_honoured(L, ref_coefficients):
    from scannertools_amd import _native
    name = "33x65_smooth_q75_444"
    need = ref_coefficients[name][0].size
    st, msg, coef, _, _ = _coefficients(L, _jpg(name), cap=need - 1, extra=need)
    assert st == _native.ST_ERR_INVALID and "coef holds" in msg and (coef == 12345).all()
    st, _, coef, _, _ = _coefficients(L, _jpg(name), cap=need, extra=64)
    assert st == _native.ST_OK and (coef[need:] == 12345).all()


def test_host_parser_under_address_and_ub_sanitizers(tmp_path):
    """st_jpeg_parse.cpp on its own, built with -fsanitize=address,undefined and driven from a child process over every golden
    and refused stream, every prefix of two streams and seeded corruptions (the pattern of
    test_host.py::test_op_library_under_address_and_ub_sanitizers; host code only)."""
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not asan or not os.path.isabs(asan) or shutil.which("g++") is None:
        pytest.skip("no libasan / g++")
    lib = tmp_path / "libst_jpeg_parse_asan.so"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "scannertools_amd", "csrc", "st_jpeg_parse.cpp"), "-o", str(lib)])
    script = r'''
import ctypes, numpy as np
G = np.load(%r)
L = ctypes.CDLL(%r)
class Info(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int) for k in ("h", "w", "channels", "h_samp", "v_samp", "restart_interval")] + [("message", ctypes.c_char * 160)]
L.st_jpeg_coefficients.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.POINTER(Info)]
L.st_jpeg_probe.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(Info)]
def run(data, cap):
    info, quant = Info(), np.zeros(192, np.uint16)
    coef = np.zeros(max(cap, 1), np.int16)          # exactly cap values: one write past it is the sanitizer's to see
    L.st_jpeg_probe(data, len(data), ctypes.byref(info))
    return L.st_jpeg_coefficients(data, len(data), coef.ctypes.data, cap, quant.ctypes.data, ctypes.byref(info))
def need(name):
    h, w, c = G[name + "__img"].shape
    return 64 * 3 * (-(-w // 16) * 2) * (-(-h // 16) * 2)
for name in G["cases"]:
    assert run(G[name + "__jpg"].tobytes(), need(str(name))) == 0, name
for name in G["refused"]:
    assert run(G[name + "__jpg"].tobytes(), 1 << 16) != 0, name
rng = np.random.default_rng(5)
for name in ("3x3_noise_q75_444", "17x13_noise_q100_420_rst3", "5x40_smooth_q95_420_opt"):
    data = G[name + "__jpg"].tobytes()
    for cut in range(len(data)):
        run(data[:cut], need(name))
    buf = bytearray(data)
    for _ in range(1500):
        pos = int(rng.integers(0, len(buf)))
        old, buf[pos] = buf[pos], int(rng.integers(0, 256))
        run(bytes(buf), need(name))
        buf[pos] = old
print("sanitized run ok")
''' % (os.path.join(ROOT, "tests", "golden", "jpeg_golden.npz"), str(lib))
    preload = " ".join(p for p in (asan, os.environ.get("LD_PRELOAD", "")) if p)
    env = dict(os.environ, LD_PRELOAD=preload, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0")
    p = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "sanitized run ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr, p.stderr[-4000:]


def test_image_decoder_args_round_trip():
    from scannertools_amd import _proto
    assert _proto.image_decoder_args(None) == b"" and _proto.parse_image_decoder_args(b"") == {}
    assert _proto.image_decoder_args("JPEG") == b"\x08\x01" == _proto.encode([(1, "int32", 1)])      # as protoc writes it
    assert _proto.image_decoder_args("ANY") == b"\x08\x02"
    assert _proto.image_decoder_args("PNG") == b"\x08\x00"          # written explicitly: the kernel must be able to see it
    for name in ("PNG", "JPEG", "ANY"):
        assert _proto.parse_image_decoder_args(_proto.image_decoder_args(name)) == {"image_type": name}
    assert _proto.parse_image_decoder_args(_proto.image_decoder_args(7)) == {"image_type": 7}
    proto = open(os.path.join(ROOT, "scannertools_amd", "scanner_kernels", "scannertools_imgproc_amd.proto")).read()
    assert "message ImageDecoderArgs" in proto and "PNG = 0;" in proto and "JPEG = 1;" in proto and "ANY = 2;" in proto


def test_op_and_front_end_names_exist():
    from scannertools_amd import _native, engine, hip
    ops = {(name, dev) for name, dev, _, _ in engine.registered_kernels()}
    assert {("ImageDecoder", 0), ("ImageDecoder", 1)} <= ops
    assert all(can_batch and kind == 1 for name, _, kind, can_batch in engine.registered_kernels() if name == "ImageDecoder")
    info = engine.op_info("ImageDecoder")
    assert info["input_names"] == ["img"] and info["output_names"] == ["frame"] and info["frame_output"]
    assert callable(hip.HipContext.decode_jpeg) and callable(hip.probe_jpeg) and callable(hip.jpeg_coefficients)
    assert callable(engine._Ops.ImageDecoder)
    assert _native.KERNEL_NAMES[_native.K_JPEG] == "jpeg"
    for sym in ("st_jpeg_probe", "st_jpeg_coefficients", "st_jpeg_decode_batch"):
        assert sym in _native.SIGNATURES and hasattr(_native.lib(), sym)


def test_engine_names_the_row_of_a_stream_it_cannot_decode():
    """Rows are probed on the host before a kernel instance exists: no GPU is needed to be told which row is wrong."""
    from scannertools_amd.engine import Client, DeviceType, NamedStream, PerfParams
    good = [_jpg(n) for n in GOLD["batch"][:3]]
    for bad, what in ((_jpg("progressive"), "row 2: progressive"), (_jpg("32x24_batch_444")[:40], "row 2: truncated"),
                      (_jpg("16x16_smooth_q75_444"), "row 2 changes shape")):
        sc = Client()
        sc.ingest_rows("jpgs", good[:2] + [bad] + good[2:])
        img = sc.io.Input([NamedStream(sc, "jpgs")])
        with pytest.raises(ValueError, match=what):
            sc.run(sc.io.Output(sc.ops.ImageDecoder(img=img, device=DeviceType.CPU, batch=4), [NamedStream(sc, "o")]), PerfParams.estimate())
