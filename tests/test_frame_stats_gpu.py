"""Frame statistics on the MI355X: moments bit for bit against the exact integer definitions (tests/ref_frame_stats_np.py),
the six statistics against the restated formulas and numpy, batch / launch-split independence, both kernel classes and the
Python ops through the engine, and invalid calls."""
import ctypes
import os
import pickle
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_frame_stats_np as R  # noqa: E402
from util import random_frames, texture_stream  # noqa: E402

pytestmark = pytest.mark.gpu

GEOMS = [(1080, 1920, 8), (2160, 3840, 2), (1920, 1080, 2), (479, 853, 3), (1079, 1919, 2), (1, 1, 5), (1, 7, 4), (7, 1, 4),
         (3, 5, 3)]


def _frames(h, w, n, seed):
    if h >= 16 and w >= 16:
        return np.concatenate([texture_stream(seed, n - 1, h, w, margin=2)[0], random_frames(seed, 1, h, w)]) if n > 1 else \
            random_frames(seed, 1, h, w)
    return random_frames(seed, n, h, w)


def _special(h, w):
    yy, xx = np.mgrid[:h, :w]
    board = np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[..., None], 3, axis=2)
    return np.stack([np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8), board])


@pytest.mark.parametrize("h,w,n", GEOMS)
def test_moments_are_exact(hip_ctx, h, w, n):
    frames = np.concatenate([_frames(h, w, n, h + w), _special(h, w)])
    d = torch.from_numpy(frames).cuda()
    got = hip_ctx.frame_moments(d).cpu().numpy()
    ref = np.array([R.moments(f) for f in frames], np.int64)
    assert (got == ref).all()
    # the batch entry point (one buffer per frame, each at its own alignment) agrees with the strided one
    pad = [torch.zeros(3 * h * w + 16, dtype=torch.uint8, device="cuda") for _ in frames]
    views = []
    for i, f in enumerate(frames):
        off = (5 * i + 1) % 16
        pad[i][off:off + 3 * h * w] = torch.from_numpy(f.reshape(-1)).cuda()
        views.append(pad[i][off:off + 3 * h * w].view(h, w, 3))
    assert (hip_ctx.frame_moments(views).cpu().numpy() == ref).all()
    # the work masks compute their own moments, equal to the full call's, and leave the others 0
    lum = hip_ctx.frame_moments(d, luma=True, laplacian=False).cpu().numpy()
    lap = hip_ctx.frame_moments(d, luma=False, laplacian=True).cpu().numpy()
    assert (lum[:, :2] == ref[:, :2]).all() and (lum[:, 2:] == 0).all()
    assert (lap[:, 2:] == ref[:, 2:]).all() and (lap[:, :2] == 0).all()


@pytest.mark.parametrize("h,w", [(1080, 1920), (479, 853), (3, 5), (1, 1)])
def test_six_statistics(hip_ctx, h, w):
    frames = np.concatenate([_frames(h, w, 3, 5), _special(h, w)])
    d = torch.from_numpy(frames).cuda()
    for kind in R.KINDS:
        got = hip_ctx.frame_stats(d, kind).cpu().numpy()
        ref = np.array([R.stat(f, kind) for f in frames])
        if kind.endswith("CPP"):
            assert got.dtype == np.float32 and (got.view(np.uint32) == ref.astype(np.float32).view(np.uint32)).all(), kind
        else:
            assert got.dtype == np.float64 and (got == ref.astype(np.float64)).all(), kind
            npy = np.array([R.numpy_python_op(f, kind) for f in frames])
            assert (np.abs(got - npy) <= 1e-12 * np.abs(npy) + 1e-12).all(), kind


def test_result_does_not_depend_on_the_batch(hip_ctx):
    h, w = 37, 53
    frames = random_frames(9, 257, h, w)
    d = torch.from_numpy(frames).cuda()
    full = hip_ctx.frame_moments(d).cpu().numpy()
    for n in (1, 33):
        for s in range(0, 257, n):
            assert (hip_ctx.frame_moments(d[s:s + n]).cpu().numpy() == full[s:s + n]).all()
    assert (full[[0, 100, 256]] == np.array([R.moments(frames[i]) for i in (0, 100, 256)])).all()


def _tiny(i, h=2, w=3):
    """Frame i of the long call: bytes derived from the frame index (re-derived here, not shared with other files)."""
    k = np.arange(h * w * 3, dtype=np.int64)
    return ((i * 7 + k * 13 + (i >> 8) * 31 + (i >> 16) * 101) % 256).astype(np.uint8).reshape(h, w, 3)


def test_more_than_65535_frames_in_one_call(hip_ctx):
    n = 65538
    frames = np.stack([_tiny(i) for i in range(n)])
    d = torch.from_numpy(frames).cuda()
    whole = hip_ctx.frame_moments(d).cpu().numpy()
    parts = np.concatenate([hip_ctx.frame_moments(d[s:s + 65535]).cpu().numpy() for s in range(0, n, 65535)])
    assert (whole == parts).all()
    for i in (0, 65534, 65535, 65536, 65537):
        assert list(whole[i]) == R.moments(frames[i]), i
    lst = [d[i] for i in range(n)]
    assert (hip_ctx.frame_moments(lst).cpu().numpy() == whole).all()


def _engine_run(op, frames, device, batch):
    from scannertools_amd.engine import CacheMode, Client, NamedStream, NamedVideoStream, PerfParams
    sc = Client()
    sc.ingest_frames("v", frames)
    frame = sc.io.Input([NamedVideoStream(sc, "v")])
    node = getattr(sc.ops, op)(frame=frame, device=device, batch=batch)
    out = NamedStream(sc, "o")
    sc.run(sc.io.Output(node, [out]), PerfParams.estimate(), cache_mode=CacheMode.Overwrite)
    return sc, list(out.load())


@pytest.mark.parametrize("op", ["BrightnessCPP", "ContrastCPP", "SharpnessCPP"])
def test_kernel_classes(op, hip_ctx):
    from scannertools_amd.engine import Client, DeviceType
    frames = _frames(120, 160, 13, 21)
    ref = [R.stat(f, op) for f in frames]
    before = Client().live_buffers()
    for device in (DeviceType.GPU, DeviceType.CPU):
        for batch in (1, 5, 13):
            sc, rows = _engine_run(op, frames, device, batch)
            assert all(isinstance(v, float) for v in rows)
            assert (np.array(rows, np.float32).view(np.uint32) == np.array(ref, np.float32).view(np.uint32)).all(), (device, batch)
            assert sc.live_buffers() == before


@pytest.mark.parametrize("op", ["Brightness", "Contrast", "Sharpness"])
def test_python_ops(op):
    from scannertools_amd.engine import CacheMode, Client, NamedStream, NamedVideoStream, PerfParams
    from scannertools_amd import frame_stats
    frames = _frames(90, 70, 4, 3)
    sc = Client()
    sc.ingest_frames("v", frames)
    frame = sc.io.Input([NamedVideoStream(sc, "v")])
    out = NamedStream(sc, "o")
    sc.run(sc.io.Output(getattr(sc.ops, op)(frame=frame), [out]), PerfParams.estimate(), cache_mode=CacheMode.Overwrite)
    got = list(out.load())
    for f, v in zip(frames, got):
        ref = R.numpy_python_op(f, op)
        assert isinstance(v, np.float64) and abs(v - ref) <= 1e-12 * abs(ref) + 1e-12
    one = pickle.loads(getattr(frame_stats, op.lower())(None, frames[0]))
    assert isinstance(one, np.float64) and one == got[0]


def test_runners_end_to_end():
    from scannertools_amd.engine import Client
    from scannertools_amd import frame_stats
    frames = texture_stream(4, 3, 1080, 1920)[0]
    sc = Client()
    sc.ingest_frames("clip", frames)
    (b,) = frame_stats.compute_brightness_cpp(sc, ["clip"], batch=3)
    (c,) = frame_stats.compute_contrast(sc, ["clip"])
    (s,) = frame_stats.compute_sharpness(sc, ["clip"])
    assert list(b.load()) == [float(R.stat(f, "BrightnessCPP")) for f in frames]
    assert list(c.load()) == [R.stat(f, "Contrast") for f in frames]
    assert list(s.load()) == [R.stat(f, "Sharpness") for f in frames]


def test_invalid_calls_raise_and_leave_the_context_usable(hip_ctx):
    from scannertools_amd import _native
    from scannertools_amd.hip import StError
    L, h = _native.lib(), hip_ctx._h
    hip_ctx._bind()
    m = torch.zeros((2, 8), dtype=torch.int64, device="cuda")
    fr = torch.zeros((2, 4, 4, 3), dtype=torch.uint8, device="cuda")
    vp = ctypes.c_void_p
    bad = [L.st_frame_moments_u8c3_strided(h, vp(fr.data_ptr()), 48, 2, 4, 4, 0, vp(m.data_ptr())),      # empty mask
           L.st_frame_moments_u8c3_strided(h, vp(fr.data_ptr()), 48, 2, 4, 4, 4, vp(m.data_ptr())),      # unknown bit
           L.st_frame_moments_u8c3_strided(h, vp(fr.data_ptr()), 48, 2, 0, 4, 3, vp(m.data_ptr())),      # h = 0
           L.st_frame_moments_u8c3_strided(h, vp(fr.data_ptr()), 47, 2, 4, 4, 3, vp(m.data_ptr())),      # stride too small
           L.st_frame_moments_u8c3_strided(h, vp(fr.data_ptr()), 48, 2, 4, 4, 3, None),                  # no output
           L.st_frame_moments_u8c3_strided(h, vp(fr.data_ptr()), 3 << 20, 1, 1, 1 << 20, 3, vp(m.data_ptr())),  # row too wide
           L.st_frame_stats_finish(h, vp(m.data_ptr()), 2, 4, 4, 6, vp(m.data_ptr())),                   # unknown kind
           L.st_frame_stats_finish(h, vp(m.data_ptr()), 2, 4, -1, 0, vp(m.data_ptr()))]
    assert bad[:5] + bad[6:] == [_native.ST_ERR_INVALID] * 7 and bad[5] == _native.ST_ERR_UNSUPPORTED
    with pytest.raises(StError):
        hip_ctx.frame_moments(fr, luma=False, laplacian=False)
    with pytest.raises(ValueError):
        hip_ctx.frame_stats(fr, 9)
    f = random_frames(2, 2, 4, 4)
    got = hip_ctx.frame_moments(torch.from_numpy(f).cuda()).cpu().numpy()
    assert (got == np.array([R.moments(x) for x in f])).all()
