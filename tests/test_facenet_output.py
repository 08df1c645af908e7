"""FacenetOutput without a GPU: the numpy restatement (tests/ref_facenet_output_np.py) against the
library's geometry and against answers worked out by hand, the element reader and writer, registration and symbols, and
the validate() refusals, which come before a context is opened."""
import struct

import numpy as np
import pytest

import ref_facenet_output_np as ref
from scannertools_amd import _native, _proto, engine, types
from scannertools_amd.hip import facenet_geometry

F = np.float32


def test_geometry_is_the_library_geometry_plus_the_ceil_rule():
    for scale in (0.05, 0.25, 0.5, 0.73, 1.0, 1.37, 1.5, 2.0):
        for h in (1, 7, 8, 9, 48, 67, 96, 184, 1080):
            for w in (1, 8, 53, 64, 93, 192, 320, 1920):
                nh, nw, gh, gw = ref.geometry(h, w, scale)
                if min(nh, nw) < 1:
                    with pytest.raises(_native.StError):
                        facenet_geometry(h, w, scale)
                    continue
                assert facenet_geometry(h, w, scale) == (nh, nw), (h, w, scale)
                assert nh % 8 == 0 and nw % 8 == 0 and (gh, gw) == (nh // 8, nw // 8)
    # the shapes the GPU tests use, and 1080p at scale 0.5
    assert ref.geometry(67, 93, 0.73)[2:] == (6, 9) and ref.geometry(96, 192, 1.0)[2:] == (12, 24)
    assert ref.geometry(48, 64, 1.5)[2:] == (9, 12) and ref.geometry(184, 320, 1.0)[2:] == (23, 40)
    assert ref.geometry(1080, 1920, 0.5) == (544, 960, 68, 120)


def _single_cell_map(gw, gh, t, xi, yi, conf, adj=(0.0, 0.0, 0.0, 0.0)):
    m = np.zeros((125, gw, gh), F)
    m[:25] = -100.0                       # sigmoid 3.8e-44: below every threshold used here
    m[t, xi, yi] = conf
    for k in range(4):
        m[25 + 25 * k + t, xi, yi] = adj[k]
    return m


def test_known_answers_for_a_single_cell():
    T = np.zeros((25, 4), F)
    T[4] = (-3, -4, 4, 3)                 # tw = th = 8
    T[20] = (0, 0, 15, 7)                 # tw = 16, th = 8
    # a 32 x 16 frame at scale 0.5: network input 16 x 8, grid 2 x 1
    assert ref.geometry(16, 32, 0.5) == (8, 16, 1, 2)
    rows, idx, score = ref.decode(_single_cell_map(2, 1, 4, 1, 0, 0.0), 16, 32, 0.5, T, 0.5)
    # logit 0: e = 1, score = 0.5, and 0.5 < 0.5 is false.  x = 7, y = -1; x = 7 / 16 * 32 = 14, bw = 8 / 16 * 32 = 16,
    # y = -1 / 8 * 16 = -2, bh = 8 / 8 * 16 = 16; x1 = (14 - 8) / 32, y1 = (-2 - 8) / 16, x2 = 22 / 32, y2 = 6 / 16
    assert idx.tolist() == [1] and rows.tolist() == [[0.1875, -0.625, 0.6875, 0.375, 0.5]]     # candidate (t 4, xi 1, yi 0)
    assert score.shape == (30,) and score[1] == 0.5 and (np.delete(score, 1) < 1e-40).all()
    assert len(ref.decode(_single_cell_map(2, 1, 4, 1, 0, 0.0), 16, 32, 0.5, T, np.nextafter(F(0.5), F(1)))[0]) == 0
    # dcx = 0.25 moves the centre by tw / 4 = 2 network pixels = 4 frame pixels; dcy = -0.5 by -4 network = -8 frame pixels
    rows, _, _ = ref.decode(_single_cell_map(2, 1, 4, 1, 0, 0.0, (0.25, -0.5, 0.0, 0.0)), 16, 32, 0.5, T, 0.5)
    assert rows.tolist() == [[0.3125, -1.125, 0.8125, -0.125, 0.5]]
    # template 20 is candidate block 10 of the 15-template list: index 10 * 2 + 0; dcw = ln 2 doubles the width up to rounding
    rows, idx, _ = ref.decode(_single_cell_map(2, 1, 20, 0, 0, 30.0, (0.0, 0.0, np.log(2.0), 0.0)), 16, 32, 0.5, T, 0.5)
    assert idx.tolist() == [20] and rows[0, 4] == 1.0                          # 1 + e^-30 rounds to 1 in float64
    np.testing.assert_allclose(rows[0, :4], [(-2 - 32) / 32, (-2 - 8) / 16, (-2 + 32) / 32, (-2 + 8) / 16], rtol=1e-6)
    # scale above 1: templates 18 .. 24 are not looked at; an invalid template never is
    assert len(ref.decode(_single_cell_map(1, 1, 20, 0, 0, 30.0), 4, 4, 2.0, T, 0.5)[0]) == 0
    assert len(ref.decode(_single_cell_map(1, 1, 4, 0, 0, 30.0), 4, 4, 2.0, T, 0.5)[0]) == 1
    assert len(ref.decode(_single_cell_map(2, 1, 3, 0, 0, 30.0), 16, 32, 0.5, T, 0.5)[0]) == 0
    # drops: a NaN adjustment; a NaN logit passes the threshold test (as `confidence < threshold_` lets it) and keeps a NaN score
    assert len(ref.decode(_single_cell_map(2, 1, 4, 0, 0, 30.0, (np.nan, 0, 0, 0)), 16, 32, 0.5, T, 0.5)[0]) == 0
    rows, _, _ = ref.decode(_single_cell_map(2, 1, 4, 0, 0, np.nan), 16, 32, 0.5, T, 0.5)
    assert len(rows) == 1 and np.isnan(rows[0, 4]) and not np.isnan(rows[0, :4]).any()
    # the exponential is the rounded float64 one
    v = F(0.3)
    assert ref.exp32(v) == F(np.exp(np.float64(v)))


def test_known_answers_of_the_suppression():
    a, b, c = (0, 0, 1, 1), (0, 0, .5, .5), (2, 2, 3, 3)
    rows = lambda *bs: np.asarray([box + (s,) for box, s in bs], F)
    # b lies inside a: a covers all of b's area (1 >= 0.1), c is disjoint (0)
    assert ref.nms(rows((a, .9), (b, .8), (c, .7))).tolist() == [0, 2]
    # b first: it covers a quarter of a's area -- suppressed at 0.1, kept at 0.3; the denominator is the area of the box under test
    assert ref.nms(rows((a, .8), (b, .9), (c, .7)), 0.1).tolist() == [1, 2]
    assert ref.nms(rows((a, .8), (b, .9), (c, .7)), 0.3).tolist() == [1, 0, 2]
    # equal scores: ascending index; identical boxes: the first survives
    assert ref.nms(rows((c, .5), (a, .5), (a, .5), (b, .5))).tolist() == [0, 1]
    # a zero-area box: 0 / 0 is not below the overlap, so any kept box suppresses it, itself included when it comes first
    z = (5, 5, 5, 6)
    assert ref.nms(rows((a, .9), (z, .8))).tolist() == [0]
    assert ref.nms(rows((z, .9), (a, .8))).tolist() == [0, 1]
    # offset 1, the pixel formula: a box half a unit away now "touches"
    d = (1.5, 0, 2.5, 1)
    assert ref.nms(rows((a, .9), (d, .8)), 0.1, 0.0).tolist() == [0, 1]
    assert ref.nms(rows((a, .9), (d, .8)), 0.1, 1.0).tolist() == [0]          # (1 - 1.5 + 1) * (1 - 0 + 1) / (2 * 2) = 0.25
    # a NaN coordinate in the box under test: its area is NaN, it falls to the first kept box
    n = (np.nan, 0, 1, 1)
    assert ref.nms(rows((c, .9), (n, .8))).tolist() == [0]
    assert ref.nms(np.zeros((0, 5), F)).tolist() == []


def test_scored_bboxes_round_trip():
    rows = np.asarray([[0.25, -0.5, 0.75, 1.5, 0.9], [0.0, 0.125, 0.5, 0.0, 0.5], [0.1, 0.2, 0.3, 0.4, 0.0], [-0.0, 0, 0, 0, 0]], F)
    buf = types.write_scored_bboxes(rows)
    f = lambda v: struct.pack("<f", v)
    first = b"\x0d" + f(0.25) + b"\x15" + f(-0.5) + b"\x1d" + f(0.75) + b"\x25" + f(1.5) + b"\x2d" + f(F(0.9))
    second = b"\x15" + f(0.125) + b"\x1d" + f(0.5) + b"\x2d" + f(0.5)        # x1 = 0 and y2 = 0 are left out
    assert buf.startswith(struct.pack("<Q", 4) + struct.pack("<Q", 25) + first + struct.pack("<Q", 15) + second)
    assert buf.endswith(struct.pack("<Q", 0))                                  # the all-zero box is an empty message
    back = types.scored_bboxes(buf)
    assert back.dtype == F and back.shape == (4, 5)
    np.testing.assert_array_equal(back, rows)
    # the coordinate reader sees the same boxes; the plain writer and reader keep their behaviour
    assert [tuple(b) for b in types.bboxes(buf)] == [tuple(float(v) for v in r[:4]) for r in rows]
    plain = types.write_bboxes([(1, 2, 3, 4)])
    assert types.scored_bboxes(plain).tolist() == [[1, 2, 3, 4, 0]] and types.bboxes(plain) == [types.BBox(1, 2, 3, 4)]
    # no boxes: the 8-byte count
    assert types.write_scored_bboxes(np.zeros((0, 5))) == struct.pack("<Q", 0)
    assert types.scored_bboxes(struct.pack("<Q", 0)).shape == (0, 5) and types.scored_bboxes(None) is None
    with pytest.raises(ValueError):
        types.scored_bboxes(buf[:-1])                                          # ends inside a length
    with pytest.raises(ValueError):
        types.scored_bboxes(struct.pack("<Q", 1) + struct.pack("<Q", 2) + b"\x28\x01")   # score as a varint


def test_registration_and_symbols():
    regs = {(name, dev): (kind, cb) for name, dev, kind, cb in engine.registered_kernels("caffe")}
    assert regs[("FacenetOutput", 0)] == (1, True) and regs[("FacenetOutput", 1)] == (1, True)   # CPU and GPU, Batched, .batch()
    assert "FacenetOutput" not in {n for n, _, _, _ in engine.registered_kernels()}             # not in the imgproc library
    info = engine.op_info("FacenetOutput")
    assert not info["frame_output"] and info["output_names"] == ["bboxes"]
    assert info["input_names"] == ["facenet_output", "original_frame_info"]
    L = _native.lib()
    for sym in ("st_facenet_output_batch", "st_facenet_output_fetch", "st_bbox_nms_f32"):
        assert sym in _native.SIGNATURES and hasattr(L, sym), sym
    assert _native.K_COUNT == 19 and _native.K_CPM2_NMS == 15 and L.st_abi_version() == 1


def _run_error(make_node):
    from scannertools_amd.engine import Client, NamedStream, NamedVideoStream, PerfParams
    sc = Client()
    sc.ingest_frames("maps", np.zeros((2, 125, 1, 1), F))
    sc.ingest_frames("v", np.zeros((2, 8, 8, 3), np.uint8))
    maps = sc.io.Input([NamedVideoStream(sc, "maps")])
    info = sc.ops.InfoFromFrame(frame=sc.io.Input([NamedVideoStream(sc, "v")]))
    with pytest.raises(RuntimeError) as e:
        sc.run(sc.io.Output(make_node(sc, maps, info), [NamedStream(sc, "o")]), PerfParams.estimate())
    return str(e.value)


@pytest.mark.parametrize("device", [0, 1])
def test_validate_refusals_name_the_cause(tmp_path, device):
    """Every refusal comes before the context is opened, so it is reached with or without a GPU, on both registrations."""
    from scannertools_amd.engine import _CppMultiOpNode
    good = tmp_path / "templates.bin"
    good.write_bytes(ref.templates().tobytes())
    short = tmp_path / "short.bin"
    short.write_bytes(ref.templates().tobytes()[:399])
    op = lambda **kw: (lambda sc, maps, info: sc.ops.FacenetOutput(facenet_output=maps, original_frame_info=info, device=device, batch=2, **kw))
    assert "scale must be positive" in _run_error(op(scale=0.0, threshold=0.5, templates_path=str(good)))
    assert "scale must be positive" in _run_error(op(scale=-1.0, threshold=0.5, templates_path=str(good)))
    assert "threshold must be a finite number" in _run_error(op(scale=1.0, threshold=float("nan"), templates_path=str(good)))
    assert "Could not find template file." in _run_error(op(scale=1.0, threshold=0.5, templates_path=str(tmp_path / "none.bin")))
    assert "Could not find template file." in _run_error(op(scale=1.0, threshold=0.5, templates_path=""))
    assert "Template file not correct." in _run_error(op(scale=1.0, threshold=0.5, templates_path=str(short)))
    for bad in (b"\x0a\x05abc", b"\x1d\x00\x00", b"\x0a\x02\x0a\x7f" + _proto.encode([(3, "float", 1.0)])):   # truncated field, truncated float, malformed caffe_args
        msg = _run_error(lambda sc, maps, info: _CppMultiOpNode(sc, "FacenetOutput", [maps, info], device, 2, bad))
        assert "Could not parse FacenetArgs" in msg
