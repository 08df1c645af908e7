"""Montage on the MI355X, bit-exact against an oracle montage composed here from oracle.resize_u8 tiles on a zero canvas:
the ABI entry (down / up scaling, the copy and 2 x 2 paths, odd widths, bytes outside the tiles untouched), both kernel
classes at several batch sizes, the ShotBoundaries -> keyframes -> Montage pipeline and a geometry change mid-stream."""
import ctypes
import math

import numpy as np
import pytest
import torch

import oracle
from scannertools_amd import _proto, engine
from scannertools_amd.engine import CacheMode, Client, DeviceType, NamedStream, NamedVideoStream, PerfParams
from util import random_frames

pytestmark = pytest.mark.gpu


def tile_height(h, w, target_width):
    return int(target_width / (1.0 * w) * h)


def oracle_montage(frames, num_frames, target_width, frames_per_row):
    h, w = frames[0].shape[:2]
    th = tile_height(h, w, target_width)
    mh = int(float(math.ceil(num_frames / (1.0 * frames_per_row))) * th)
    canvas = np.zeros((mh, frames_per_row * target_width, 3), np.uint8)
    for k, f in enumerate(frames):
        x, y = k % frames_per_row, k // frames_per_row
        canvas[th * y:th * (y + 1), target_width * x:target_width * (x + 1)] = oracle.resize_u8(f, target_width, th)
    return canvas


@pytest.mark.parametrize("h,w,tw,n,fpr", [(1080, 1920, 240, 5, 3),   # downscale
                                          (48, 64, 200, 3, 2),       # upscale
                                          (90, 120, 120, 4, 3),      # equal size: copy
                                          (96, 128, 64, 5, 2),       # exact half: the 2 x 2 mean
                                          (37, 53, 19, 7, 3),        # 3 * 19 = 57 bytes per tile row
                                          (61, 83, 33, 5, 4), (50, 70, 35, 3, 3)])
def test_abi_tiles_match_oracle_and_leave_the_rest(hip_ctx, h, w, tw, n, fpr):
    frames = random_frames(h + w + tw, n, h, w)
    th = tile_height(h, w, tw)
    first = 1                                       # tiles 1 .. n of a canvas with room for n + 2
    rows = (first + n + 1) // fpr + 1
    canvas = torch.full((rows * th, fpr * tw + 5, 3), 0xA5, dtype=torch.uint8, device="cuda")  # wider than the tiles
    hip_ctx.montage(torch.from_numpy(frames).cuda(), canvas, tw, th, fpr, first_slot=first)
    torch.cuda.synchronize()
    got = canvas.cpu().numpy()
    want = np.full(got.shape, 0xA5, np.uint8)
    for i in range(n):
        s = first + i
        x, y = s % fpr, s // fpr
        want[th * y:th * (y + 1), tw * x:tw * (x + 1)] = oracle.resize_u8(frames[i], tw, th)
    np.testing.assert_array_equal(got, want)


def test_abi_equals_resize(hip_ctx):
    """The tile bits are st_resize_u8_batch's, path for path."""
    for (h, w, tw) in [(1080, 1920, 240), (96, 128, 64), (90, 120, 120), (48, 64, 200)]:
        frames = torch.from_numpy(random_frames(h * w, 3, h, w)).cuda()
        th = tile_height(h, w, tw)
        canvas = torch.zeros((th, 3 * tw, 3), dtype=torch.uint8, device="cuda")
        hip_ctx.montage(frames, canvas, tw, th, 3)
        ref = hip_ctx.resize(frames, tw, th)
        torch.cuda.synchronize()
        for i in range(3):
            assert torch.equal(canvas[:, tw * i:tw * (i + 1)], ref[i])


def _montage_rows(device, frames, num_frames, tw, fpr, batch):
    sc = Client()
    sc.ingest_frames("in", frames)
    m = sc.ops.Montage(frame=sc.io.Input([NamedVideoStream(sc, "in")]), num_frames=num_frames, target_width=tw,
                       frames_per_row=fpr, device=device, batch=batch)
    out = NamedStream(sc, "out")
    sc.run(sc.io.Output(m, [out]), PerfParams.estimate(), cache_mode=CacheMode.Overwrite)
    return list(out.load())


@pytest.mark.parametrize("device", [DeviceType.CPU, DeviceType.GPU])
def test_kernel_classes_batch_sizes(device):
    frames = random_frames(13, 13, 120, 160)
    want = oracle_montage(frames, 13, 60, 4)          # 4 rows of tiles, the last one 3/4 black
    L = engine._imgproc()
    before = (L.stshim_live_buffers(0), L.stshim_live_buffers(1))
    for batch in (1, 5, 13):
        rows = _montage_rows(device, frames, 13, 60, 4, batch)
        assert len(rows) == 13
        assert all(r.shape == want.shape and r.dtype == np.uint8 for r in rows)
        np.testing.assert_array_equal(rows[-1], want)
    assert (L.stshim_live_buffers(0), L.stshim_live_buffers(1)) == before


@pytest.mark.parametrize("device", [DeviceType.CPU, DeviceType.GPU])
def test_short_stream_hands_over_no_canvas(device):
    """Fewer frames than num_frames: every row is a placeholder, and the unfinished canvas is freed."""
    L = engine._imgproc()
    before = (L.stshim_live_buffers(0), L.stshim_live_buffers(1))
    rows = _montage_rows(device, random_frames(3, 5, 40, 60), 8, 30, 4, 2)
    assert len(rows) == 5 and all(r.shape == (40, 120, 3) for r in rows)
    assert (L.stshim_live_buffers(0), L.stshim_live_buffers(1)) == before


def test_last_row_alone_runs_the_whole_stream():
    frames = random_frames(7, 9, 64, 96)
    sc = Client()
    sc.ingest_frames("in", frames)
    m = sc.ops.Montage(frame=sc.io.Input([NamedVideoStream(sc, "in")]), num_frames=9, target_width=48, frames_per_row=4,
                       device=DeviceType.GPU, batch=4)
    got = m.rows([8])[0]
    np.testing.assert_array_equal(got, oracle_montage(frames, 9, 48, 4))


@pytest.mark.parametrize("device", [DeviceType.CPU, DeviceType.GPU])
def test_shot_keyframe_montage_pipeline(device):
    """Histogram -> ShotBoundaries -> Gather(keyframes) -> Montage: a contact sheet of the shots of a clip with known cuts."""
    rng = np.random.default_rng(1)
    n, h, w = 300, 480, 640
    cuts = [41, 120, 199, 260]
    frames = np.empty((n, h, w, 3), np.uint8)
    base = rng.integers(0, 256, (h, w, 3))
    for i in range(n):
        if i in cuts:
            base = rng.integers(0, 256, (h, w, 3))
        frames[i] = np.clip(base + rng.integers(-3, 4, (h, w, 3)), 0, 255)
    sc = Client()
    sc.ingest_frames("clip", frames)
    frame = sc.io.Input([NamedVideoStream(sc, "clip")])
    hist = sc.ops.Histogram(frame=frame, device=device, batch=64)
    bounds = NamedStream(sc, "bounds")
    sc.run(sc.io.Output(sc.ops.ShotBoundaries(histograms=hist), [bounds]), PerfParams.estimate())
    found = next(bounds.load(rows=[0]))
    assert found == cuts
    keyframes = [0] + found
    m = sc.ops.Montage(frame=sc.streams.Gather(frame, [keyframes]), num_frames=len(keyframes), target_width=160,
                       frames_per_row=3, device=device, batch=8)
    out = NamedStream(sc, "sheet")
    sc.run(sc.io.Output(m, [out]), PerfParams.estimate())
    sheet = list(out.load())[-1]
    assert sheet.shape == (2 * 120, 480, 3)
    np.testing.assert_array_equal(sheet, oracle_montage([frames[k] for k in keyframes], len(keyframes), 160, 3))


@pytest.mark.parametrize("device", [DeviceType.CPU, DeviceType.GPU])
def test_geometry_change_resets_the_canvas(device):
    """Two streams of different frame sizes through one kernel instance: the second montage is that of the second
    stream alone (new_frame_info -> reset discards the first stream's partial canvas)."""
    L = engine._imgproc()
    a = random_frames(21, 3, 60, 80)
    b = random_frames(22, 5, 90, 100)
    args = _proto.encode([(1, "int64", 5), (4, "int32", 50), (6, "int32", 2)])
    err = ctypes.create_string_buffer(512)
    k = L.stshim_kernel_create(b"Montage", device, 0, args, len(args), err, 512)
    assert k, err.value
    try:
        results = []
        for fr in (a, b):
            if device == DeviceType.GPU:
                keep = [torch.from_numpy(f).cuda() for f in fr]
                ptrs = [t.data_ptr() for t in keep]
                torch.cuda.synchronize()
            else:
                keep = [np.ascontiguousarray(f) for f in fr]
                ptrs = [f.ctypes.data for f in keep]
            res = L.stshim_run_frames(k, (ctypes.c_void_p * len(ptrs))(*ptrs), len(ptrs), fr.shape[1], fr.shape[2], 3, 0, 2,
                                      (ctypes.c_int * 1)(0), 1, err, 512)
            assert res and not err.value, err.value
            try:
                results.append(engine._CppOpNode._fetch(L, res, L.stshim_outputs_count(res) - 1))
            finally:
                L.stshim_outputs_free(res)
        np.testing.assert_array_equal(results[1], oracle_montage(b, 5, 50, 2))
    finally:
        L.stshim_kernel_destroy(k)
