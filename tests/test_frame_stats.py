"""Frame statistics without a GPU: the definitions (tests/ref_frame_stats_np.py) against the oracle, explicit loops, known
answers and numpy; the ContrastCPP deviation bound; the op registrations, argument errors and the absence of a CPU fallback."""
import os
import pickle
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_frame_stats_np as R  # noqa: E402
from util import random_frames, texture_stream  # noqa: E402

# ContrastCPP's float32 running sum (old/cpp_ops/imgproc.cpp:113-121) against the exactly rounded standard deviation this
# build returns: relative differences measured on seeded natural-like and uniform-noise frames (seeds 7 and 11 below) were at
# most 1.53e-3 at 1080p and 7.63e-3 at 4K (the drift grows with the number of terms).  The bounds below are those, rounded
# up; DESIGN.md quotes the same figures.
CONTRAST_CPP_BOUND = {(1080, 1920): 2e-3, (2160, 3840): 1e-2}


def test_luma_is_the_oracle_rgb2yuv_y_over_the_whole_cube():
    import oracle
    cube = np.arange(1 << 24, dtype=np.uint32)
    img = np.stack([(cube >> 16) & 255, (cube >> 8) & 255, cube & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    assert (R.luma(img) == oracle.cvt_color(img, 83)[..., 0]).all()   # 83 = COLOR_RGB2YUV


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (37, 53)])
def test_laplacian_is_the_reflect101_loop(shape):
    f = np.random.default_rng(sum(shape)).integers(0, 256, shape + (3,), dtype=np.uint8)
    assert (R.laplacian(f) == R.laplacian_loop(f)).all()


def test_known_answers():
    const = np.empty((9, 11, 3), np.uint8)
    const[:] = (200, 30, 90)
    y = int(R.luma(const[:1, :1])[0, 0])
    assert R.stat(const, "Brightness") == y and R.stat(const, "BrightnessCPP") == np.float32(y)
    for k in ("Contrast", "ContrastCPP", "Sharpness", "SharpnessCPP"):
        assert R.stat(const, k) == 0.0
    # 0/255 checkerboard: every interior value is +-1020
    yy, xx = np.mgrid[:8, :10]
    board = np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[..., None], 3, axis=2)
    L = R.laplacian(board)
    assert (np.abs(L[1:-1, 1:-1]) == 1020).all()
    # one bright pixel (value 255 in every channel) in the interior of a black 5x5 frame: L = -1020 there, +255 at its four
    # neighbours, 0 elsewhere, per channel
    dot = np.zeros((5, 5, 3), np.uint8)
    dot[2, 2] = 255
    N = 25
    s, q = -1020 + 4 * 255, 1020 ** 2 + 4 * 255 ** 2
    assert R.moments(dot)[2:] == [s] * 3 + [q] * 3
    var = q / N - (s / N) ** 2
    assert abs(float(R.stat(dot, "SharpnessCPP")) - var) <= 1e-6 * var
    assert abs(float(R.stat(dot, "Sharpness")) - var) <= 1e-12 * var   # pooled: the three channels are equal


@pytest.mark.parametrize("kind", ["Brightness", "Contrast", "Sharpness"])
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (3, 5), (61, 83), (120, 160)])
def test_python_op_definitions_match_numpy(kind, shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    frames = [rng.integers(0, 256, shape + (3,), dtype=np.uint8)]
    if min(shape) > 8:
        frames.append(texture_stream(3, 1, shape[0], shape[1], margin=2)[0][0])
    for f in frames:
        ours, ref = float(R.stat(f, kind)), float(R.numpy_python_op(f, kind))
        assert abs(ours - ref) <= 1e-12 * abs(ref) + 1e-300, (ours, ref)


@pytest.mark.parametrize("h,w", sorted(CONTRAST_CPP_BOUND))
def test_contrast_cpp_deviation_is_bounded(h, w):
    frames = [f for seed in (7, 11) for f in list(texture_stream(seed, 2, h, w)[0]) + list(random_frames(seed + 1, 1, h, w))]
    for f in frames:
        exact, ref = float(R.stat(f, "ContrastCPP")), float(R.contrast_cpp_reference_float32(f))
        assert abs(ref - exact) <= CONTRAST_CPP_BOUND[(h, w)] * exact, (ref, exact)


# ---- op library and front-ends ----------------------------------------------------------------------------------------------
CPP_OPS = {"BrightnessCPP": "brightness", "ContrastCPP": "contrast", "SharpnessCPP": "sharpness"}


def test_registrations():
    from scannertools_amd import engine
    regs = {(name, dev): (kind, cb) for name, dev, kind, cb in engine.registered_kernels()}
    for op, col in CPP_OPS.items():
        for dev in (0, 1):
            assert regs[(op, dev)] == (1, True)          # BatchedKernel with .batch(), on CPU and GPU
        info = engine.op_info(op)
        assert info["inputs"] == 1 and info["outputs"] == 1 and not info["frame_output"]
        assert info["output_names"] == [col]             # old/cpp_ops/imgproc.cpp:245-270
    from scannertools_amd import frame_stats
    sc = engine.Client()
    for name in list(CPP_OPS) + ["Brightness", "Contrast", "Sharpness"]:
        assert callable(getattr(sc.ops, name))
    for fn in ("compute_brightness", "compute_brightness_cpp", "compute_contrast", "compute_contrast_cpp", "compute_sharpness",
               "compute_sharpness_cpp", "brightness", "contrast", "sharpness"):
        assert callable(getattr(frame_stats, fn))


def test_readers():
    import struct
    from scannertools_amd import types
    assert types.frame_stat(struct.pack("f", 1.5)) == 1.5 and types.frame_stat(None) is None
    v = types.pickled(pickle.dumps(np.float64(2.25)))
    assert v == 2.25 and isinstance(v, np.float64)


def _graph(frames):
    from scannertools_amd.engine import Client, NamedVideoStream
    sc = Client()
    sc.ingest_frames("v", frames)
    return sc, sc.io.Input([NamedVideoStream(sc, "v")])


def test_malformed_imgproc_args_fail_kernel_creation():
    from scannertools_amd import engine
    from scannertools_amd.engine import NamedStream, PerfParams
    sc, frame = _graph(np.zeros((2, 8, 8, 3), np.uint8))
    for op in CPP_OPS:
        node = getattr(sc.ops, op)(frame=frame)
        node.args = b"\x08"                      # a truncated varint
        with pytest.raises(RuntimeError, match="could not parse ImgProcArgs"):
            sc.run(sc.io.Output(node, [NamedStream(sc, "o")]), PerfParams.estimate(), cache_mode=engine.CacheMode.Overwrite)


@pytest.mark.parametrize("bad", [np.zeros((2, 8, 8, 4), np.uint8), np.zeros((2, 8, 8, 3), np.float32), np.zeros((2, 8, 8, 1), np.uint8)])
def test_frames_must_be_u8_with_three_channels(bad):
    from scannertools_amd import engine
    from scannertools_amd.engine import NamedStream, PerfParams
    sc, frame = _graph(bad)
    for op in list(CPP_OPS) + ["Brightness", "Contrast", "Sharpness"]:
        with pytest.raises(ValueError, match="not \\(h, w, 3\\) uint8"):
            sc.run(sc.io.Output(getattr(sc.ops, op)(frame=frame), [NamedStream(sc, "o")]), PerfParams.estimate(),
                   cache_mode=engine.CacheMode.Overwrite)


def test_no_gpu_means_runtime_error_not_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from scannertools_amd import engine
    from scannertools_amd.engine import DeviceType, NamedStream, PerfParams
    sc, frame = _graph(random_frames(1, 2, 8, 8))
    nodes = [getattr(sc.ops, op)(frame=frame, device=dev) for op in CPP_OPS for dev in (DeviceType.CPU, DeviceType.GPU)]
    nodes += [getattr(sc.ops, op)(frame=frame) for op in ("Brightness", "Contrast", "Sharpness")]
    for node in nodes:
        with pytest.raises(RuntimeError):
            sc.run(sc.io.Output(node, [NamedStream(sc, "o")]), PerfParams.estimate(), cache_mode=engine.CacheMode.Overwrite)


def test_definitions_against_opencv_golden():
    """tests/golden/frame_stats_opencv_<version>.npz (made by tests/golden/make_frame_stats_golden.py where cv2 exists) pins
    the definitions against real OpenCV; skipped while no such file is committed."""
    import glob
    paths = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "frame_stats_opencv_*.npz")))
    if not paths:
        pytest.skip("no frame-statistics OpenCV dump committed (run tests/golden/make_frame_stats_golden.py where cv2 exists)")
    for path in paths:
        g = np.load(path)
        i = 0
        while "frame_%d" % i in g:
            f = g["frame_%d" % i]
            m = R.moments(f)
            assert (R.luma(f) == g["y_%d" % i]).all()
            assert list(g["lap_sum_%d" % i]) == m[2:5] and list(g["lap_sq_%d" % i]) == m[5:8]
            assert R.stat(f, "BrightnessCPP") == g["brightness_cpp_%d" % i]
            assert R.stat(f, "SharpnessCPP") == g["sharpness_cpp_%d" % i]
            for k in ("Brightness", "Contrast", "Sharpness"):
                ref = float(g["%s_%d" % (k.lower(), i)])
                assert abs(float(R.stat(f, k)) - ref) <= 1e-12 * abs(ref) + 1e-12
            i += 1
