"""FacenetInput and CaffeInput without a GPU: the host-only entry points against the numpy
restatement (tests/ref_net_input_np.py), the contracts' known answers, the restatement against the float64 definition,
registration, the proto writers and the validate() refusals that need no device."""
import struct

import numpy as np
import pytest

import ref_net_input_np as ref
from scannertools_amd import _native, _proto, engine
from scannertools_amd.hip import caffe_input_axis, facenet_geometry

SCALES = (0.05, 0.1, 0.25, 0.33, 0.5, 0.73, 0.999, 1.0, 1.37, 2.0, 3.3, 8.0)
# the axis pairs the contract names: downscales and equal sizes, none with an empty window
PAIRS = [(1920, 224), (1920, 227), (1920, 300), (1920, 960), (1280, 368), (1080, 224), (1080, 227), (1080, 300), (640, 224),
         (480, 224), (100, 33), (97, 29), (53, 20), (37, 16), (33, 11), (31, 7), (64, 64), (41, 41)]


# ---- host-only entry points ---------------------------------------------------------------------
def test_facenet_geometry_matches_the_restatement():
    for scale in SCALES:
        for h in range(1, 131):
            for w in (1, 2, 7, 8, 9, 53, 64, 100, 130, h):
                want = ref.facenet_geometry(h, w, scale)
                if min(want) < 1:
                    with pytest.raises(_native.StError):
                        facenet_geometry(h, w, scale)
                else:
                    assert facenet_geometry(h, w, scale) == want, (h, w, scale)
    assert facenet_geometry(37, 53, 1.0) == (40, 56) and facenet_geometry(48, 64, 0.5) == (24, 32)
    assert facenet_geometry(1, 1, 1.0) == (8, 8) and facenet_geometry(1080, 1920, 0.5) == (544, 960)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(_native.StError):
            facenet_geometry(8, 8, bad)


def test_caffe_axis_matches_the_restatement_and_empty_windows_agree():
    empty = set()
    for n_in in range(1, 131):
        for n_out in range(1, 131):
            st, begin, first, count = caffe_input_axis(n_in, n_out)
            rb, rf, rc, contiguous = ref.caffe_axis(n_in, n_out)
            assert contiguous, (n_in, n_out)                       # members are always consecutive taps
            np.testing.assert_array_equal(begin, rb)
            np.testing.assert_array_equal(first, rf)
            np.testing.assert_array_equal(count, rc)
            assert (st == _native.ST_ERR_UNSUPPORTED) == bool((rc == 0).any()), (n_in, n_out)
            if (rc == 0).any():
                empty.add((n_in, n_out))
    assert empty and all(n_out > n_in for n_in, n_out in empty)   # no downscale or equal size has an empty window
    assert (16, 24) in empty and (20, 30) in empty and (16, 32) not in empty
    assert int((ref.caffe_axis(16, 24)[2] == 0).sum()) == 10 and int((ref.caffe_axis(20, 30)[2] == 0).sum()) == 14
    L = _native.lib()
    assert L.st_caffe_input_axis(0, 4, None, None, None) == _native.ST_ERR_INVALID


@pytest.mark.parametrize("n_in,n_out", PAIRS + [(16, 32)])
def test_caffe_axis_named_pairs(n_in, n_out):
    st, begin, first, count = caffe_input_axis(n_in, n_out)
    rb, rf, rc, contiguous = ref.caffe_axis(n_in, n_out)
    assert st == _native.ST_OK and contiguous and (count > 0).all()
    np.testing.assert_array_equal(begin, rb)
    np.testing.assert_array_equal(first, rf)
    np.testing.assert_array_equal(count, rc)
    start = begin + first
    assert start.min() >= 0 and (np.diff(start) >= 0).all() and (start + count - 1).max() <= n_in   # n_in itself: the clamp
    if n_in == n_out:          # ratio 1: the mean of samples x and x + 1 (the reference's half-pixel quirk)
        np.testing.assert_array_equal(start, np.arange(n_out))
        assert (count == 2).all()
    if n_in == 2 * n_out:      # 2:1: three taps 2x .. 2x + 2
        np.testing.assert_array_equal(start, 2 * np.arange(n_out))
        assert (count == 3).all()
    if (n_in, n_out) == (1920, 224):
        assert set(count) == {8, 9}
    if (n_in, n_out) == (1080, 224):
        assert set(count) == {4, 5}
    if (n_in, n_out) == (16, 32):
        assert (start + count - 1).max() == 16                      # the last window reaches index n_in


# ---- known answers of the restatement -----------------------------------------------------------
def test_caffe_known_answers():
    zero = (0.0, 0.0, 0.0)
    fr = np.random.default_rng(1).integers(0, 256, (2, 6, 5, 3), dtype=np.uint8)
    same = ref.caffe_input(fr, 6, 5, zero)                          # ratio 1: (v[x] + v[x + 1]) / 2 per axis, edge replicated
    p = np.pad(fr.astype(np.float64), ((0, 0), (0, 1), (0, 1), (0, 0)), mode="edge")
    want = (p[:, :-1, :-1] + p[:, :-1, 1:] + p[:, 1:, :-1] + p[:, 1:, 1:]) / 4
    np.testing.assert_array_equal(same, want[..., ::-1].transpose(0, 3, 1, 2).astype(np.float32))   # quarters are exact
    # constant frames: 200 gives 200.0 .. 200.00005 (fl(1 / m) lies above 1 / m for m = 3, 5, 6, 7, 9); 255 gives exactly 255.0
    # through the clamp where the windows hold up to 6 members.  With 9 members (240 -> 28, as 1920 -> 224) the running sum
    # passes 128, where float32 steps by 2^-16, and can end one step BELOW 255: 254.99998, which no clamp repairs.
    for h, w, nh, nw, exact255 in ((37, 53, 16, 20, True), (48, 64, 24, 32, True), (97, 100, 29, 33, True), (64, 64, 64, 64, True),
                                   (135, 240, 28, 28, False)):
        c200 = ref.caffe_input(np.full((1, h, w, 3), 200, np.uint8), nh, nw, zero)
        assert c200.min() >= 200.0 and c200.max() <= np.float32(200.00005)
        c255 = ref.caffe_input(np.full((1, h, w, 3), 255, np.uint8), nh, nw, zero)
        assert c255.max() == 255.0 and c255.min() == (255.0 if exact255 else np.nextafter(np.float32(255), np.float32(0)))
    # channel flip and mean order: plane c is input channel 2 - c minus mean_colors[c]
    fr = np.zeros((1, 8, 8, 3), np.uint8)
    fr[..., 0], fr[..., 1], fr[..., 2] = 10, 20, 40                 # R, G, B
    out = ref.caffe_input(fr, 4, 4, (1.0, 2.0, 4.0))
    assert [float(out[0, c, 0, 0]) for c in range(3)] == [39.0, 18.0, 6.0]
    outn = ref.caffe_input(fr, 4, 4, (1.0, 2.0, 4.0), normalize=True)
    np.testing.assert_array_equal(outn, out / np.float32(255.0))   # a division


def test_facenet_known_answers():
    rs = np.zeros((1, 8, 16, 3), np.uint8)                          # a resized frame: net_h 8, net_w 16
    rs[0, 2, 5] = (10, 20, 40)
    out = ref.facenet_from_resized(rs, (1.5, 2.5, 4.5))
    assert out.shape == (1, 3, 16, 8) and out.dtype == np.float32
    assert [float(out[0, c, 5, 2]) for c in range(3)] == [8.5, 17.5, 35.5]      # no flip; [c][x][y]
    assert float(out[0, 0, 2, 5]) == -1.5
    m = (104.00699, 116.66877, 122.67892)
    np.testing.assert_array_equal(ref.facenet_from_resized(rs, m)[0, :, 0, 0], -np.asarray(m, np.float32))


@pytest.mark.parametrize("h,w,nh,nw", [(37, 53, 16, 20), (97, 100, 29, 33), (180, 200, 21, 23), (48, 64, 24, 32), (31, 33, 7, 11),
                                       (64, 64, 64, 64), (16, 16, 32, 32)])
@pytest.mark.parametrize("normalize", [False, True])
def test_restatement_within_the_derived_bound_of_the_definition(h, w, nh, nw, normalize):
    fr = np.random.default_rng(h * w).integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    mean = (104.00699, 116.66877, 122.67892)
    a, b = ref.caffe_input(fr, nh, nw, mean, normalize), ref.caffe_input64(fr, nh, nw, mean, normalize)
    assert a.dtype == np.float32 and a.shape == (2, 3, nh, nw)
    err = float(np.abs(a.astype(np.float64) - b).max())
    bound = ref.caffe_bound(h, w, nh, nw, mean, normalize)
    print("max |f32 - f64| = %.3g, bound %.3g" % (err, bound))
    assert err <= bound


# ---- layers above the C ABI ----------------------------------------------------------------------
def test_registration_and_symbols():
    regs = {(name, dev): (kind, cb) for name, dev, kind, cb in engine.registered_kernels("caffe")}
    for op in ("FacenetInput", "CaffeInput"):
        assert regs[(op, 0)] == (1, True) and regs[(op, 1)] == (1, True)    # DeviceType CPU = 0 and GPU = 1, Batched, .batch()
        assert (op, 0) not in {(n, d) for n, d, _, _ in engine.registered_kernels()}   # not in the imgproc library
    fi, ci = engine.op_info("FacenetInput"), engine.op_info("CaffeInput")
    assert fi["frame_output"] and fi["output_names"] == ["facenet_input"] and fi["input_names"] == ["frame"]
    assert ci["frame_output"] and ci["output_names"] == ["caffe_frame"] and ci["input_names"] == ["frame"]
    L = _native.lib()
    for sym in ("st_facenet_geometry", "st_facenet_input_batch", "st_caffe_input_axis", "st_caffe_input_batch"):
        assert sym in _native.SIGNATURES and hasattr(L, sym)
    assert _native.K_NET_INPUT == 18 and _native.K_COUNT == 19 and _native.KERNEL_NAMES[_native.K_NET_INPUT] == "net_input"


def test_proto_writers_match_the_wire_format():
    f = lambda v: struct.pack("<f", v)
    mean = (1.5, -2.0, 0.0)
    packed = b"\x3a\x0c" + f(1.5) + f(-2.0) + f(0.0)               # field 7, length-delimited, 12 bytes
    unpacked = b"\x3d" + f(1.5) + b"\x3d" + f(-2.0) + b"\x3d" + f(0.0)   # field 7, fixed32, three times (zero included)
    assert _proto.net_descriptor(mean_colors=mean) == packed
    assert _proto.net_descriptor(mean_colors=mean, packed=False) == unpacked
    # NetDescriptor{input_width: 300 (5), input_height: 200 (6), mean_colors (7), normalize (11)}
    nd = b"\x28\xac\x02\x30\xc8\x01" + packed + b"\x58\x01"
    assert _proto.net_descriptor(300, 200, mean, True) == nd
    assert _proto.caffe_input_args(300, 200, mean, True) == b"\x0a" + bytes([len(nd)]) + nd
    assert _proto.caffe_input_args(300, 200, mean, True, batch_size=4) == b"\x0a" + bytes([len(nd)]) + nd + b"\x10\x04"
    # input_width -1: a ten-byte varint
    assert _proto.net_descriptor(-1, 0, ()) == b"\x28" + b"\xff" * 9 + b"\x01"
    # FacenetArgs{caffe_args (1){net_descriptor (1)}, templates_path (2), scale (3), threshold (4)}
    ca = b"\x0a" + bytes([len(packed)]) + packed
    assert _proto.facenet_args(0.5, mean) == b"\x0a" + bytes([len(ca)]) + ca + b"\x1d" + f(0.5)
    assert _proto.facenet_args(0.5, mean, "t", 0.25) == b"\x0a" + bytes([len(ca)]) + ca + b"\x12\x01t" + b"\x1d" + f(0.5) + b"\x25" + f(0.25)
    assert _proto.facenet_args(0.0, ()) == b""


def _run_error(make_op):
    from scannertools_amd.engine import Client, NamedStream, NamedVideoStream, PerfParams
    sc = Client()
    sc.ingest_frames("v", np.zeros((2, 8, 8, 3), np.uint8))
    frame = sc.io.Input([NamedVideoStream(sc, "v")])
    with pytest.raises(RuntimeError) as e:
        sc.run(sc.io.Output(make_op(sc, frame), [NamedStream(sc, "o")]), PerfParams.estimate())
    return str(e.value)


@pytest.mark.parametrize("packed", [True, False])
def test_validate_refusals_name_the_cause(packed):
    """Argument checks come before the context is opened, so they are reached with or without a GPU."""
    from scannertools_amd.engine import _CppOpNode
    m3 = (1.0, 2.0, 3.0)
    assert "scale must be positive" in _run_error(lambda sc, fr: sc.ops.FacenetInput(frame=fr, scale=0.0, mean_colors=m3, packed=packed))
    assert "scale must be positive" in _run_error(lambda sc, fr: sc.ops.FacenetInput(frame=fr, scale=-0.5, mean_colors=m3, packed=packed))
    msg = _run_error(lambda sc, fr: sc.ops.FacenetInput(frame=fr, scale=0.5, mean_colors=(1.0, 2.0), packed=packed))
    assert "mean_colors must hold 3 values, got 2" in msg
    msg = _run_error(lambda sc, fr: sc.ops.CaffeInput(frame=fr, input_width=4, input_height=4, mean_colors=(1.0, 2.0, 3.0, 4.0), packed=packed))
    assert "mean_colors must hold 3 values, got 4" in msg
    assert "must be positive" in _run_error(lambda sc, fr: sc.ops.CaffeInput(frame=fr, input_width=4, input_height=0, mean_colors=m3, packed=packed))
    for op, what in (("FacenetInput", "Could not parse FacenetArgs"), ("CaffeInput", "Could not parse CaffeInputArgs")):
        assert what in _run_error(lambda sc, fr: _CppOpNode(sc, op, fr, None, None, None, b"\x0a\x7f\x01"))          # truncated
        assert what in _run_error(lambda sc, fr: _CppOpNode(sc, op, fr, None, None, None, b"\x0a\x03\x0a\x05\x01"))  # bad nesting
    # a packed mean_colors payload that is not a whole number of floats
    bad_nd = b"\x3a\x05" + b"\x00" * 5
    bad = _proto.message(1, bad_nd)
    assert "Could not parse CaffeInputArgs" in _run_error(lambda sc, fr: _CppOpNode(sc, "CaffeInput", fr, None, None, None, bad))
