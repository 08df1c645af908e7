"""CPU: the host side of the ImageEncoder op (quantisation tables, stream header, size bound, argument checks, registration,
argument messages) against the streams Pillow wrote (tests/golden/jpeg_encode_golden.npz), and the numpy restatement of
libjpeg's forward path (tests/ref_jpeg_encode_np.py) against the coefficients in those streams."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import ref_jpeg_encode_np as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD_PATH = os.path.join(ROOT, "tests", "golden", "jpeg_encode_golden.npz")
GOLD = np.load(GOLD_PATH)
CASES = [str(c) for c in GOLD["cases"]]
BATCH = [str(c) for c in GOLD["batch"]]
SAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
ST_ERR_INVALID, ST_ERR_UNSUPPORTED = 1, 4
ENTRY_POINTS = ["st_jpeg_quant_tables", "st_jpeg_encode_header", "st_jpeg_encode_bound", "st_jpeg_encode_batch", "st_jpeg_encode_fetch"]


def _cfg(name):
    return json.loads(str(GOLD[name + "__cfg"]))


def _jpg(name):
    return GOLD[name + "__jpg"].tobytes()


def _header_end(jpg):
    """Index one past the SOS segment."""
    sos = jpg.index(b"\xff\xda")
    return sos + 2 + int.from_bytes(jpg[sos + 2:sos + 4], "big")


def test_golden_file_holds_the_cases_the_op_is_held_to():
    assert len(CASES) >= 150 and len(BATCH) == 33
    assert os.path.getsize(GOLD_PATH) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "jpeg_golden.npz"))
    cfgs = [_cfg(c) for c in CASES]
    shapes = {(c["h"], c["w"]) for c in cfgs}
    assert {(1, 1), (8, 8), (7, 17), (17, 7), (65, 33), (33, 65), (34, 40), (40, 34), (24, 9), (9, 24), (80, 24), (152, 16), (9, 200), (8, 360), (24, 32)} <= shapes
    for shape in shapes - {(24, 32)}:
        assert {c["subsampling"] for c in cfgs if (c["h"], c["w"]) == shape} == set(SAMPLING), shape
    assert {c["quality"] for c in cfgs} == {1, 50, 95, 100} and {c["content"] for c in cfgs} == {"noise", "flat", "checker", "ramp"}
    # intervals of more than 64 and more than 128 blocks: the entropy kernel's wave then makes several passes
    blocks = {-(-c["w"] // (8 * SAMPLING[c["subsampling"]][0])) * (SAMPLING[c["subsampling"]][0] * SAMPLING[c["subsampling"]][1] + 2) for c in cfgs}
    assert {75, 78, 92, 135, 138} <= blocks
    # ten intervals, so that RST7 is followed by RST0
    from scannertools_amd.hip import probe_jpeg
    for shape, sub in (((80, 24), "4:4:4"), ((152, 16), "4:2:0")):
        name = [n for n, c in zip(CASES, cfgs) if (c["h"], c["w"]) == shape and c["subsampling"] == sub][0]
        markers = re.findall(rb"\xff[\xd0-\xd7]", _jpg(name)[629:])   # 0xFF in the scan's data is always followed by 0x00
        assert markers == [bytes([0xFF, 0xD0 + k % 8]) for k in range(9)], name
    for name in CASES:
        info, c = probe_jpeg(_jpg(name)), _cfg(name)
        assert (info["h"], info["w"], info["channels"]) == (c["h"], c["w"], 3)
        assert (info["h_samp"], info["v_samp"]) == SAMPLING[c["subsampling"]]
        assert info["restart_interval"] == -(-c["w"] // (8 * info["h_samp"]))   # one MCU row


def test_quant_tables_equal_the_golden_streams():
    from scannertools_amd.hip import jpeg_coefficients, jpeg_quant_tables
    seen = set()
    for name in CASES:
        q = _cfg(name)["quality"]
        _, quant = jpeg_coefficients(_jpg(name))
        luma, chroma = jpeg_quant_tables(q)
        assert np.array_equal(luma, quant[0]) and np.array_equal(chroma, quant[1]) and np.array_equal(chroma, quant[2]), name
        seen.add(q)
    assert seen == {1, 50, 95, 100}
    assert jpeg_quant_tables(100)[0].max() == 1 and jpeg_quant_tables(1)[1].max() == 255


def test_header_equals_the_golden_streams():
    from scannertools_amd.hip import jpeg_encode_header
    for name in CASES:
        c, jpg = _cfg(name), _jpg(name)
        got = jpeg_encode_header(c["h"], c["w"], c["quality"], c["subsampling"])
        assert got == jpg[:_header_end(jpg)], name
        assert len(got) == 629


def test_bound_covers_every_golden_stream_and_the_stated_worst_case():
    from scannertools_amd.hip import jpeg_encode_bound
    for name in CASES:
        c = _cfg(name)
        assert jpeg_encode_bound(c["h"], c["w"], c["subsampling"]) >= len(_jpg(name)), name
    # 16 x 16: one MCU of six blocks at 4:2:0, two of four at 4:2:2, four of three at 4:4:4; 1660 bits of codes per block are
    # under 208 bytes, every byte stuffed 416; 629 bytes of header, an RST marker between MCU rows, EOI
    assert jpeg_encode_bound(16, 16, "4:2:0") >= 629 + 6 * 416 + 2
    assert jpeg_encode_bound(16, 16, "4:2:2") >= 629 + 8 * 416 + 2 + 2
    assert jpeg_encode_bound(16, 16, "4:4:4") >= 629 + 12 * 416 + 2 + 2
    assert (22 + 63 * 26 + 7) // 8 <= 208
    # and it is not a wild guess either: below twice the stated figure
    assert jpeg_encode_bound(16, 16, "4:2:0") <= 2 * (629 + 6 * 416 + 2)


def test_numpy_restatement_equals_the_golden_coefficients():
    from scannertools_amd.hip import jpeg_coefficients
    for name in CASES:
        c = _cfg(name)
        want, quant = jpeg_coefficients(_jpg(name))
        hs, vs = SAMPLING[c["subsampling"]]
        got = ref.coefficients(GOLD[c["img"]], quant[0], quant[1], hs, vs)
        assert got.shape == want.shape, name
        assert np.array_equal(got, want), (name, int(np.count_nonzero(got != want)))


def test_numpy_restatement_equals_the_golden_streams():
    """Header from the library, scan from the restatement's own entropy coder (tables read from the header's DHT segments):
    the whole stream, byte for byte."""
    from scannertools_amd.hip import jpeg_encode_header, jpeg_quant_tables
    for name in CASES:
        c, jpg = _cfg(name), _jpg(name)
        hs, vs = SAMPLING[c["subsampling"]]
        header = jpeg_encode_header(c["h"], c["w"], c["quality"], c["subsampling"])
        coef = ref.coefficients(GOLD[c["img"]], *jpeg_quant_tables(c["quality"]), hs, vs)
        assert header + ref.scan(coef, c["h"], c["w"], hs, vs, header) == jpg, name


def test_registration():
    from scannertools_amd import engine
    regs = [r for r in engine.registered_kernels() if r[0] == "ImageEncoder"]
    assert sorted(dev for _, dev, _, _ in regs) == [0, 1]
    assert all(kind == 1 and can_batch for _, _, kind, can_batch in regs)
    info = engine.op_info("ImageEncoder")
    assert info["input_names"] == ["frame"] and info["output_names"] == ["img"] and not info["frame_output"]
    assert info["inputs"] == 1 and info["outputs"] == 1 and info["stencil"] == [0] and not info["unbounded_state"]


def test_symbols_are_declared_bound_and_exported():
    from scannertools_amd import _native
    header = open(os.path.join(ROOT, "include", "scannertools_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = ctypes.CDLL(_native.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _native.SIGNATURES and hasattr(L, name), name
    assert "st_jpeg_enc.hip" in open(os.path.join(ROOT, "scannertools_amd", "csrc", "Makefile")).read()
    assert _native.K_COUNT == 19 and _native.lib().st_abi_version() == 1   # no new timing slot, no new ABI version
    proto = open(os.path.join(ROOT, "scannertools_amd", "scanner_kernels", "scannertools_imgproc_amd.proto")).read()
    assert re.search(r"message ImageEncoderArgs \{\s*int32 quality = 1;\s*string subsampling = 2;\s*\}", proto)


def test_argument_message_round_trips():
    from scannertools_amd import _proto
    assert _proto.image_encoder_args() == b"" and _proto.parse_image_encoder_args(b"") == {}
    assert _proto.image_encoder_args(95, "4:2:0") == b"\x08\x5f\x12\x054:2:0"
    for q, s in ((1, "4:4:4"), (100, "4:2:2"), (75, ""), (0, "4:2:0"), (-3, "nonsense")):
        want = {k: v for k, v in (("quality", q), ("subsampling", s)) if v}
        assert _proto.parse_image_encoder_args(_proto.image_encoder_args(q, s)) == want


def test_host_entry_points_refuse_bad_arguments():
    from scannertools_amd import _native
    from scannertools_amd.hip import StError, jpeg_encode_bound, jpeg_encode_header, jpeg_quant_tables, jpeg_sampling
    L = _native.lib()
    buf, size = ctypes.create_string_buffer(1024), ctypes.c_size_t()
    q = (ctypes.c_uint16 * 64)()
    for quality in (0, -1, 101):
        assert L.st_jpeg_quant_tables(quality, q, q) == ST_ERR_INVALID
        assert L.st_jpeg_encode_header(8, 8, quality, 2, 2, buf, 1024, ctypes.byref(size)) == ST_ERR_INVALID
        with pytest.raises(StError, match="quality"):
            jpeg_quant_tables(quality)
    assert L.st_jpeg_quant_tables(50, None, q) == ST_ERR_INVALID
    for hs, vs in ((1, 2), (4, 1), (2, 4), (0, 0), (3, 3)):
        assert L.st_jpeg_encode_header(8, 8, 50, hs, vs, buf, 1024, ctypes.byref(size)) == ST_ERR_UNSUPPORTED
        assert L.st_jpeg_encode_bound(8, 8, hs, vs) == -1
    for name in ("4:1:1", "4:4:0", "420", "", None, (2, 2)):
        with pytest.raises(ValueError, match="subsampling"):
            jpeg_sampling(name)
    with pytest.raises(ValueError, match="subsampling"):
        jpeg_encode_header(8, 8, 50, "4:1:1")
    for h, w in ((0, 8), (8, 0), (65536, 8), (8, 65536), (-1, -1)):
        assert L.st_jpeg_encode_header(h, w, 50, 2, 2, buf, 1024, ctypes.byref(size)) == ST_ERR_INVALID
        assert L.st_jpeg_encode_bound(h, w, 2, 2) == -1
        with pytest.raises(StError, match="65535"):
            jpeg_encode_bound(h, w)
    # a buffer that is too small: the size is reported, nothing is written
    small = ctypes.create_string_buffer(b"\x55" * 100, 100)
    assert L.st_jpeg_encode_header(8, 8, 50, 2, 2, small, 100, ctypes.byref(size)) == ST_ERR_INVALID and size.value == 629
    assert small.raw == b"\x55" * 100
    assert L.st_jpeg_encode_header(8, 8, 50, 2, 2, None, 0, ctypes.byref(size)) == ST_ERR_INVALID
    assert L.st_jpeg_encode_header(65535, 65535, 100, 1, 1, buf, 1024, None) == 0
    assert jpeg_encode_bound(65535, 65535, "4:4:4") > 65535 * 65535


def test_batch_entry_point_names_the_cause_before_it_needs_a_context():
    """Without a GPU no context exists; a null context is refused first.  What the call says about its own arguments is in
    tests/test_jpeg_encode_gpu.py; here: the shared check that words those messages."""
    from scannertools_amd import _native
    L = _native.lib()
    assert L.st_jpeg_encode_batch(None, None, 1, 8, 8, 50, 2, 2) == ST_ERR_INVALID
    assert L.st_jpeg_encode_fetch(None, None, None, 0) == ST_ERR_INVALID


def _run_op(sc, mk):
    from scannertools_amd.engine import NamedStream, PerfParams
    return sc.run(sc.io.Output(mk(), [NamedStream(sc, "o")]), PerfParams.estimate())


def test_validate_refuses_bad_arguments_without_a_gpu_context():
    """The kernel class checks its arguments before it opens a context, so the cause is named with or without a GPU."""
    from scannertools_amd import _proto
    from scannertools_amd.engine import Client, DeviceType, NamedVideoStream, _CppMultiOpNode
    sc = Client()
    sc.ingest_frames("v", np.zeros((2, 8, 8, 3), np.uint8))
    frame = sc.io.Input([NamedVideoStream(sc, "v")])
    for dev in (DeviceType.CPU, DeviceType.GPU):
        for kw, cause in ((dict(quality=101), "quality 101 is outside 1..100"), (dict(quality=-5), "quality -5 is outside 1..100"),
                          (dict(subsampling="4:1:1"), 'subsampling "4:1:1" is not supported'), (dict(subsampling="420"), "is not supported")):
            with pytest.raises(RuntimeError, match=re.escape(cause)):
                _run_op(sc, lambda: sc.ops.ImageEncoder(frame=frame, device=dev, **kw))
        with pytest.raises(RuntimeError, match="could not parse ImageEncoderArgs"):
            _run_op(sc, lambda: _CppMultiOpNode(sc, "ImageEncoder", [frame], dev, None, b"\x12\x7f4"))   # a truncated string field
    assert _proto.image_encoder_args(0, "") == b""   # ... and the defaults (95, 4:2:0) are accepted: see the GPU tests
    import torch
    if not torch.cuda.is_available():   # valid arguments without a GPU: a loud failure, no fallback
        with pytest.raises(RuntimeError, match="st_ctx_create"):
            _run_op(sc, lambda: sc.ops.ImageEncoder(frame=frame))
