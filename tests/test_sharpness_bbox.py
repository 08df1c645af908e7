"""SharpnessBBoxCPP / SharpnessBBox without a GPU: the ``bboxes`` element writer and parser, refusal of invalid boxes and
malformed bytes at the Python layer, the C ABI symbols and op registrations, and the reference definition (oracle.resize_u8
of the crop, then tests/ref_frame_stats_np.py) on cases with a known answer."""
import ctypes
import os
import re
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_frame_stats_np as R  # noqa: E402
from util import random_frames  # noqa: E402

SYMBOLS = ["st_bbox_moments_u8c3_batch", "st_bbox_moments_u8c3_strided", "st_bbox_sharpness_u8c3_batch",
           "st_bbox_sharpness_u8c3_strided"]


def definition(frame, box, kind):
    """The contract: the crop as an image of its own, resized to 200 x 200 by the oracle, then the frame statistic."""
    import oracle
    x1, y1, x2, y2 = box
    return R.stat(oracle.resize_u8(np.ascontiguousarray(frame[y1:y2, x1:x2]), 200, 200), kind)


# ---- the bboxes element ---------------------------------------------------------------------------------------------------
def test_byte_layout_by_hand():
    from scannertools_amd import types
    got = types.write_bboxes([(1.5, 2.0, 30.25, 40.0)])
    msg = b"".join(bytes([tag]) + struct.pack("<f", v) for tag, v in ((0x0d, 1.5), (0x15, 2.0), (0x1d, 30.25), (0x25, 40.0)))
    assert len(msg) == 20
    assert got == struct.pack("<Q", 1) + struct.pack("<Q", 20) + msg
    assert types.write_bboxes([]) == struct.pack("<Q", 0)


def test_round_trip():
    from scannertools_amd import _proto, types
    assert types.bboxes(types.write_bboxes([])) == []
    assert types.bboxes(None) is None
    boxes = [(1.5, 2.0, 30.25, 40.0), (0.0, 7.0, 9.0, 11.0), (-0.5, 0.0, 3.0, 0.75), (1e6, 2e6, 3e6, 4e6)]
    back = types.bboxes(types.write_bboxes(boxes))
    assert [tuple(b) for b in back] == [tuple(float(np.float32(v)) for v in b) for b in boxes]
    assert back[0].x1 == 1.5 and back[0].y2 == 40.0
    # an absent coordinate is 0, and 0 is left out of the bytes
    assert types.bbox_message((0.0, 7.0, 9.0, 11.0)) == b"".join(bytes([t]) + struct.pack("<f", v) for t, v in ((0x15, 7.0), (0x1d, 9.0), (0x25, 11.0)))
    assert tuple(types.bboxes(struct.pack("<QQ", 1, 0))[0]) == (0.0, 0.0, 0.0, 0.0)
    # fields after y2 (score = 5 as a float, a varint, a string, a fixed64) are skipped by wire type
    extra = _proto.encode([(5, "float", 0.9), (6, "int32", 3), (8, "string", "face")]) + bytes([9 << 3 | 1]) + b"\x01" * 8
    elem = types.write_bboxes([types.bbox_message((4.0, 5.0, 6.0, 7.0), extra), (1.0, 2.0, 3.0, 4.0)])
    assert [tuple(b) for b in types.bboxes(elem)] == [(4.0, 5.0, 6.0, 7.0), (1.0, 2.0, 3.0, 4.0)]
    # truncation toward zero, as (int)bbox.x1()
    t = types.truncate_bboxes([(-0.5, 0.99, 3.99, 2.5), (1.0, 2.0, 3.0, 4.0)], 10, 10)
    assert t.dtype == np.int32 and t.tolist() == [[0, 0, 3, 2], [1, 2, 3, 4]]
    assert types.truncate_bboxes([], 10, 10).shape == (0, 4)


def test_sharpness_bbox_reader():
    from scannertools_amd import types
    assert types.sharpness_bbox(b"") == ()
    assert types.sharpness_bbox(struct.pack("3f", 1.5, 2.5, 0.0)) == (1.5, 2.5, 0.0)
    assert types.sharpness_bbox(None) is None
    with pytest.raises(ValueError):
        types.sharpness_bbox(b"\x00" * 5)


@pytest.mark.parametrize("cut", ["count", "length", "message", "inside_field", "over_long", "count_too_large", "not_a_float"])
def test_malformed_bytes_are_refused(cut):
    from scannertools_amd import types
    good = types.write_bboxes([(1.0, 2.0, 3.0, 4.0), (5.0, 6.0, 7.0, 8.0)])
    bad = {"count": good[:5], "length": good[:8 + 4], "message": good[:8 + 8 + 7], "over_long": good + b"\x00",
           "inside_field": struct.pack("<QQ", 1, 3) + b"\x0d\x00\x00",
           "count_too_large": struct.pack("<Q", 3) + good[8:],
           "not_a_float": struct.pack("<QQ", 1, 2) + b"\x08\x05"}[cut]   # x1 as a varint
    with pytest.raises(ValueError):
        types.bboxes(bad)
    from scannertools_amd import frame_stats
    with pytest.raises(ValueError, match="row 1"):
        frame_stats.bbox_records("SharpnessBBoxCPP", list(np.zeros((2, 8, 8, 3), np.uint8)), [types.write_bboxes([]), bad])


INVALID = {"x_empty": (3, 1, 3, 4), "y_empty": (1, 4, 3, 4), "x_reversed": (5, 1, 2, 4), "y_reversed": (1, 6, 3, 2),
           "negative_x": (-1.0, 0, 3, 4), "negative_y": (0, -2.5, 3, 4), "past_right": (0, 0, 9, 4), "past_bottom": (0, 0, 4, 7),
           "nan": (float("nan"), 0, 3, 4), "inf": (0, 0, float("inf"), 4), "minus_inf": (float("-inf"), 0, 3, 4),
           "beyond_int32": (0, 0, 3e9, 4), "below_int32": (-3e9, 0, 3, 4)}


@pytest.mark.parametrize("why", sorted(INVALID))
def test_invalid_boxes_are_refused_without_a_gpu(why):
    """h = 6, w = 8.  Every kind of invalid box is a ValueError naming row and box from the Python op, the engine's C++ op node
    and the shared checker, before anything touches the GPU (this test runs where there is none)."""
    from scannertools_amd import engine, frame_stats, types
    from scannertools_amd.engine import Client, NamedStream, NamedVideoStream, PerfParams
    frames = random_frames(3, 3, 6, 8)
    rows = [types.write_bboxes([(0, 0, 8, 6)]), types.write_bboxes([]), types.write_bboxes([(1, 1, 2, 2), INVALID[why]])]
    with pytest.raises(ValueError, match="box 1"):
        types.truncate_bboxes(types.bboxes(rows[2]), 6, 8)
    with pytest.raises(ValueError, match="row 2: box 1"):
        frame_stats.bbox_records("SharpnessBBox", list(frames), rows)
    with pytest.raises(ValueError, match="box 1"):
        frame_stats.sharpness_bbox(None, frames[2], rows[2])
    sc = Client()
    sc.ingest_frames("v", frames)
    sc.ingest_rows("b", rows)
    frame, boxes = sc.io.Input([NamedVideoStream(sc, "v")]), sc.io.Input([NamedStream(sc, "b")])
    for node in (sc.ops.SharpnessBBoxCPP(frame=frame, bboxes=boxes), sc.ops.SharpnessBBox(frame=frame, bboxes=boxes)):
        with pytest.raises(ValueError, match="row 2: box 1"):
            sc.run(sc.io.Output(node, [NamedStream(sc, "o")]), PerfParams.estimate(), cache_mode=engine.CacheMode.Overwrite)


def test_the_largest_coordinates_that_fit_are_not_the_problem():
    """A coordinate just inside int32 is refused for being outside the frame, not for its size; the frame's own corner passes."""
    from scannertools_amd import types
    assert types.truncate_bboxes([(0, 0, 8.9, 6.9)], 6, 8).tolist() == [[0, 0, 8, 6]]
    with pytest.raises(ValueError, match="not inside"):
        types.truncate_bboxes([(0, 0, 2147483520.0, 4)], 6, 8)
    with pytest.raises(ValueError, match="int32"):
        types.truncate_bboxes([(0, 0, 2147483648.0, 4)], 6, 8)


# ---- C ABI and registrations ------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    from scannertools_amd import _native
    header = open(os.path.join(ROOT, "include", "scannertools_hip.h")).read()
    L = ctypes.CDLL(_native.LIB_PATH)
    for s in SYMBOLS:
        assert re.search(r"\bint %s\(st_ctx\* ctx," % s, header), s
        assert s in _native.SIGNATURES and hasattr(L, s), s
    assert re.search(r"#define ST_BBOX_SIDE 200\b", header) and _native.BBOX_SIDE == 200


def test_registrations():
    from scannertools_amd import engine, frame_stats
    regs = {(name, dev): (kind, cb) for name, dev, kind, cb in engine.registered_kernels()}
    for dev in (0, 1):
        assert regs[("SharpnessBBoxCPP", dev)] == (1, True)          # BatchedKernel with .batch(), on CPU and GPU
    info = engine.op_info("SharpnessBBoxCPP")
    assert info["inputs"] == 2 and info["outputs"] == 1 and not info["frame_output"]
    assert info["input_names"] == ["frame", "bboxes"] and info["output_names"] == ["sharpness_bbox"]   # imgproc.cpp:272-276
    sc = engine.Client()
    assert callable(sc.ops.SharpnessBBoxCPP) and callable(sc.ops.SharpnessBBox) and callable(sc.ingest_rows)
    for fn in ("sharpness_bbox", "compute_sharpness_bbox", "compute_sharpness_bbox_cpp"):
        assert callable(getattr(frame_stats, fn))


def test_malformed_imgproc_args_fail_kernel_creation():
    from scannertools_amd import engine, types
    from scannertools_amd.engine import Client, NamedStream, NamedVideoStream, PerfParams
    sc = Client()
    sc.ingest_frames("v", np.zeros((1, 8, 8, 3), np.uint8))
    sc.ingest_rows("b", [types.write_bboxes([(0, 0, 4, 4)])])
    node = sc.ops.SharpnessBBoxCPP(frame=sc.io.Input([NamedVideoStream(sc, "v")]), bboxes=sc.io.Input([NamedStream(sc, "b")]))
    node.args = b"\x08"                      # a truncated varint
    with pytest.raises(RuntimeError, match="could not parse ImgProcArgs"):
        sc.run(sc.io.Output(node, [NamedStream(sc, "o")]), PerfParams.estimate(), cache_mode=engine.CacheMode.Overwrite)


def test_ingested_rows_are_a_stream():
    from scannertools_amd import types
    from scannertools_amd.engine import Client, NamedStream
    sc = Client()
    rows = [types.write_bboxes([(0, 0, 4, 4)]), types.write_bboxes([])]
    sc.ingest_rows("b", rows, reader=types.bboxes)
    s = NamedStream(sc, "b")
    assert s.len() == 2 and [[tuple(b) for b in r] for r in s.load()] == [[(0.0, 0.0, 4.0, 4.0)], []]
    assert sc.io.Input([s]).rows([1, 0]) == [rows[1], rows[0]]


# ---- the definition on cases with a known answer ----------------------------------------------------------------------------
def test_constant_frame_gives_zero_for_every_box():
    f = np.empty((450, 470, 3), np.uint8)
    f[:] = (200, 30, 90)
    for box in [(0, 0, 470, 450), (3, 5, 203, 205), (10, 20, 410, 420), (7, 9, 8, 10), (0, 0, 199, 201), (50, 1, 450, 201)]:
        for kind in ("SharpnessCPP", "Sharpness"):
            assert definition(f, box, kind) == 0.0


def test_a_200_box_is_the_statistic_of_the_crop():
    f = random_frames(5, 1, 260, 300)[0]
    for x1, y1 in [(0, 0), (100, 60), (37, 11)]:
        crop = f[y1:y1 + 200, x1:x1 + 200]
        for kind in ("SharpnessCPP", "Sharpness"):
            assert definition(f, (x1, y1, x1 + 200, y1 + 200), kind) == R.stat(crop, kind)
    # the crop is isolated: pixels around it do not enter (the Python op's behaviour, which both ops take here)
    g = f.copy()
    g[:60] = 255 - g[:60]
    g[:, :100] = 255 - g[:, :100]
    assert definition(g, (100, 60, 300, 260), "Sharpness") == definition(f, (100, 60, 300, 260), "Sharpness")


def test_a_400_box_is_the_statistic_of_its_rounded_cell_means():
    f = random_frames(6, 1, 430, 440)[0]
    x1, y1 = 21, 13
    c = f[y1:y1 + 400, x1:x1 + 400].astype(np.int64)
    mean = ((c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    for kind in ("SharpnessCPP", "Sharpness"):
        assert definition(f, (x1, y1, x1 + 400, y1 + 400), kind) == R.stat(mean, kind)


def test_noise_box_does_not_fit_32_bits():
    """The figure the issue quotes: on a 200 x 200 box of uniform noise the sum of L^2 per channel is 4.3 - 4.4e9, above 2^32."""
    m = R.moments(random_frames(8, 1, 200, 200)[0], False, True)
    assert all(4.2e9 < q < 4.5e9 and q > 2 ** 32 for q in m[5:8])
