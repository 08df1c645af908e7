"""SharpnessBBoxCPP / SharpnessBBox on the MI355X.  The expected value of every test comes from code that is not under test:
``oracle.resize_u8`` of the contiguous crop to 200 x 200, then tests/ref_frame_stats_np.py (exact integer moments and the
restated finishing formulas).  All comparisons are exact; the float64 statistic is also compared with numpy's own variance
at the 1e-12 relative bound of tests/test_frame_stats_gpu.py."""
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


def resized(frame, box):
    import oracle
    x1, y1, x2, y2 = box
    return oracle.resize_u8(np.ascontiguousarray(frame[y1:y2, x1:x2]), 200, 200)


def ref_moments(frames, recs):
    return np.array([R.moments(resized(frames[f], (x1, y1, x2, y2)), False, True) for f, x1, y1, x2, y2 in recs], np.int64).reshape(-1, 8)


def special(h, w):
    yy, xx = np.mgrid[:h, :w]
    board = np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[..., None], 3, axis=2)
    return [np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8), board]


def misaligned(frames):
    """Every frame in a buffer of its own, each at its own byte offset."""
    views, keep = [], []
    for i, f in enumerate(frames):
        h, w = f.shape[:2]
        buf = torch.zeros(3 * h * w + 16, dtype=torch.uint8, device="cuda")
        off = (5 * i + 1) % 16
        buf[off:off + 3 * h * w] = torch.from_numpy(np.ascontiguousarray(f).reshape(-1)).cuda()
        keep.append(buf)
        views.append(buf[off:off + 3 * h * w].view(h, w, 3))
    return views, keep


def box_list(h, w):
    """(x1, y1, x2, y2) boxes of an h x w frame (h, w >= 420): every shape and position the contract names."""
    b = [(40, 50, 240, 250),                      # 200 x 200: copy
         (30, 10, 430, 410),                      # 400 x 400: the 2 x 2 reroute
         (8, 9, 408, 209), (8, 9, 208, 409),      # 400 x 200 and 200 x 400: one axis exactly 2 x
         (5, 6, 6, 7), (5, 6, 6, 13), (5, 6, 12, 7), (9, 2, 12, 7),   # 1 x 1, 1 x 7 (w x h), 7 x 1, 3 x 5: up-scaling
         (11, 3, 210, 204),                       # 199 x 201
         (0, 0, w, h),                            # the whole frame
         # touching each edge and each corner
         (0, 100, 150, 300), (w - 150, 100, w, 300), (100, 0, 300, 150), (100, h - 150, 300, h),
         (0, 0, 200, 200), (w - 200, 0, w, 200), (0, h - 200, 200, h), (w - 200, h - 200, w, h),
         (0, 0, 400, 400), (w - 400, h - 400, w, h), (w - 1, h - 1, w, h), (0, 0, 1, 1),
         # two overlapping boxes, and the same box twice
         (60, 60, 360, 300), (200, 150, 420, 420), (60, 60, 360, 300)]
    # 3 * x1 mod 16 takes every value 0 .. 15 (3 is a unit modulo 16), on the copy path, the 2 x 2 path and the linear path
    assert sorted((3 * x) % 16 for x in range(16)) == list(range(16))
    for x in range(16):
        b += [(x, 7, x + 200, 207), (x, 3, x + 400, 403), (x, 1, x + 333, 278)]
    return b


def check_both_layouts(ctx, frames, recs):
    recs = np.asarray(recs, np.int64).reshape(-1, 5)
    ref = ref_moments(frames, recs)
    assert (ref[:, :2] == 0).all()
    got = ctx.bbox_moments(torch.from_numpy(np.stack(frames)).cuda(), recs).cpu().numpy()
    bad = np.flatnonzero((got != ref).any(axis=1))
    assert bad.size == 0, ("one tensor", recs[bad[:5]].tolist(), got[bad[:5]].tolist(), ref[bad[:5]].tolist())
    views, keep = misaligned(frames)
    got = ctx.bbox_moments(views, recs).cpu().numpy()
    bad = np.flatnonzero((got != ref).any(axis=1))
    assert bad.size == 0, ("misaligned list", recs[bad[:5]].tolist(), got[bad[:5]].tolist(), ref[bad[:5]].tolist())
    return ref


def test_moments_bit_for_bit_1080p(hip_ctx):
    h, w = 1080, 1920
    tex = list(texture_stream(3, 2, h, w)[0])
    noise = list(random_frames(4, 2, h, w))
    frames = [tex[0], noise[0]] + special(h, w) + [tex[1], noise[1]]     # frame 5 (tex[1]) gets no box
    boxes = box_list(h, w)
    recs = [(f,) + b for f in (0, 1) for b in boxes]
    recs += [(f,) + b for f in (2, 3, 4) for b in boxes[:25] + boxes[25::7]]
    recs += [(6,) + b for b in boxes[:4]]
    assert not any(r[0] == 5 for r in recs)
    ref = check_both_layouts(hip_ctx, frames, recs)
    # noise does not fit a 32-bit record: the sum of squares of a 200 x 200 noise box is above 2^32
    assert ref[len(boxes), 5:].min() > 2 ** 32
    # constant frames give 0
    assert (ref[[i for i, r in enumerate(recs) if r[0] in (2, 3)]] == 0).all()


@pytest.mark.parametrize("h,w", [(2160, 3840), (1920, 1080)])
def test_moments_bit_for_bit_whole_frame_4k_and_portrait(hip_ctx, h, w):
    frames = [texture_stream(h, 1, h, w)[0][0], random_frames(w, 1, h, w)[0]] + special(h, w)[2:]
    recs = [(f,) + b for f in range(3) for b in [(0, 0, w, h), (w - 200, h - 200, w, h), (1, 1, w - 1, h - 1), (w - 401, 0, w - 1, 400)]]
    check_both_layouts(hip_ctx, frames, recs)


def test_300_boxes_in_one_frame_and_frames_without_boxes(hip_ctx):
    h, w = 480, 640
    frames = list(texture_stream(11, 3, h, w)[0]) + list(random_frames(12, 2, h, w))
    rng = np.random.default_rng(13)
    recs = []
    for _ in range(300):
        x1, y1 = int(rng.integers(0, w - 1)), int(rng.integers(0, h - 1))
        recs.append((3, x1, y1, int(rng.integers(x1 + 1, w + 1)), int(rng.integers(y1 + 1, h + 1))))
    recs += [(0, 0, 0, 200, 200), (4, 1, 2, 401, 402)]          # frames 1 and 2 have no box, between frames that have
    check_both_layouts(hip_ctx, frames, recs)


def test_a_call_without_boxes_is_empty(hip_ctx):
    d = torch.from_numpy(random_frames(1, 3, 32, 48)).cuda()
    for fr in (d, list(d.unbind(0))):
        got = hip_ctx.bbox_moments(fr, np.zeros((0, 5), np.int64))
        assert got.shape == (0, 8) and got.dtype == torch.int64
        for kind, dt in (("SharpnessCPP", torch.float32), ("Sharpness", torch.float64)):
            v = hip_ctx.bbox_sharpness(fr, [], kind)
            assert v.shape == (0,) and v.dtype == dt
    # the C ABI: m = 0 is a successful no-op, whatever the other pointers are
    from scannertools_amd import _native
    hip_ctx._bind()
    assert _native.lib().st_bbox_moments_u8c3_strided(hip_ctx._h, ctypes.c_void_p(d.data_ptr()), 3 * 32 * 48, 3, 32, 48, None, 0, None) == 0


def test_both_statistics_bit_for_bit(hip_ctx):
    h, w = 1080, 1920
    frames = [texture_stream(5, 1, h, w)[0][0], random_frames(6, 1, h, w)[0]] + special(h, w)
    boxes = box_list(h, w)
    recs = np.array([(f,) + b for f in range(5) for b in boxes[:25] + boxes[25::5]], np.int64)
    d = torch.from_numpy(np.stack(frames)).cuda()
    imgs = [resized(frames[f], (x1, y1, x2, y2)) for f, x1, y1, x2, y2 in recs]
    m = hip_ctx.bbox_moments(d, recs)
    for kind, dt, bits in (("SharpnessCPP", np.float32, np.uint32), ("Sharpness", np.float64, np.uint64)):
        got = hip_ctx.bbox_sharpness(d, recs, kind).cpu().numpy()
        ref = np.array([R.stat(i, kind) for i in imgs], dt)
        assert got.dtype == dt and (got.view(bits) == ref.view(bits)).all(), kind
        # the existing finishing entry point over the moments records gives the same bits as the fused launch
        from scannertools_amd import _native
        out = torch.empty(len(recs), dtype=torch.float32 if dt == np.float32 else torch.float64, device="cuda")
        hip_ctx._check(_native.lib().st_frame_stats_finish(hip_ctx._h, ctypes.c_void_p(m.data_ptr()), len(recs), 200, 200,
                                                          _native.FS_KINDS[kind], ctypes.c_void_p(out.data_ptr())))
        assert (out.cpu().numpy().view(bits) == ref.view(bits)).all(), kind
        if kind == "Sharpness":
            npy = np.array([R.laplacian(i).astype(np.float64).var() for i in imgs])
            assert (np.abs(got - npy) <= 1e-12 * np.abs(npy)).all()


def test_same_bits_as_the_existing_path_composed_by_hand(hip_ctx):
    h, w = 1080, 1920
    frames = [texture_stream(7, 1, h, w)[0][0], random_frames(8, 1, h, w)[0]]
    boxes = box_list(h, w)[:25] + [(3, 1, 336, 278), (14, 7, 214, 207), (9, 3, 409, 403)]
    recs = np.array([(f,) + b for f in range(2) for b in boxes], np.int64)
    d = torch.from_numpy(np.stack(frames)).cuda()
    got = hip_ctx.bbox_moments(d, recs).cpu().numpy()
    for i, (f, x1, y1, x2, y2) in enumerate(recs):
        crop = d[f, y1:y2, x1:x2].contiguous()
        img = hip_ctx.resize([crop], 200, 200)
        by_hand = hip_ctx.frame_moments(img, luma=False).cpu().numpy()[0]
        assert (got[i] == by_hand).all(), (recs[i].tolist(), got[i].tolist(), by_hand.tolist())


def test_result_does_not_depend_on_the_call(hip_ctx):
    h, w = 48, 64
    n = 257
    frames = random_frames(9, n, h, w)
    rng = np.random.default_rng(10)
    recs = []
    for f in range(n):
        for _ in range(2):
            x1, y1 = int(rng.integers(0, w - 1)), int(rng.integers(0, h - 1))
            recs.append((f, x1, y1, int(rng.integers(x1 + 1, w + 1)), int(rng.integers(y1 + 1, h + 1))))
    recs = np.array(recs, np.int64)
    d = torch.from_numpy(frames).cuda()
    full = hip_ctx.bbox_moments(d, recs).cpu().numpy()
    for i in (0, 1, 200, 513):
        assert (full[i] == ref_moments(frames, recs[i:i + 1])[0]).all()
    for nb in (1, 33):
        for s in range(0, n, nb):
            sub = recs[2 * s:2 * (s + nb)].copy()
            sub[:, 0] -= s
            assert (hip_ctx.bbox_moments(d[s:s + nb], sub).cpu().numpy() == full[2 * s:2 * (s + nb)]).all(), (nb, s)
    assert (hip_ctx.bbox_moments(d, recs[::-1].copy()).cpu().numpy() == full[::-1]).all()
    for kind in ("SharpnessCPP", "Sharpness"):
        v = hip_ctx.bbox_sharpness(d, recs, kind).cpu().numpy()
        assert (hip_ctx.bbox_sharpness(d, recs[::-1].copy(), kind).cpu().numpy() == v[::-1]).all()


def _tiny(i, h=4, w=5):
    """Frame i of the long call: bytes derived from the frame index (re-derived here, not shared with other files)."""
    k = np.arange(h * w * 3, dtype=np.int64)
    return ((i * 7 + k * 13 + (i >> 8) * 31 + (i >> 16) * 101) % 256).astype(np.uint8).reshape(h, w, 3)


def test_more_than_65535_boxes_in_one_call(hip_ctx):
    m, h, w = 65538, 4, 5
    nf = 1024
    frames = np.stack([_tiny(i) for i in range(nf)])
    i = np.arange(m)
    x1, y1 = i % 4, (i // 4) % 3
    recs = np.stack([i % nf, x1, y1, x1 + 1 + (i // 12) % (w - x1), y1 + 1 + (i // 60) % (h - y1)], axis=1).astype(np.int64)
    assert (recs[:, 3] <= w).all() and (recs[:, 4] <= h).all()
    d = torch.from_numpy(frames).cuda()
    whole = hip_ctx.bbox_moments(d, recs).cpu().numpy()
    parts = np.concatenate([hip_ctx.bbox_moments(d, recs[:65535]).cpu().numpy(), hip_ctx.bbox_moments(d, recs[65535:]).cpu().numpy()])
    assert (whole == parts).all()
    for k in (0, 65534, 65535, 65536, 65537):
        assert (whole[k] == ref_moments(frames, recs[k:k + 1])[0]).all(), k
    assert (hip_ctx.bbox_moments([d[k] for k in range(nf)], recs).cpu().numpy() == whole).all()


# ---- the ops through the engine -------------------------------------------------------------------------------------------
def _clip():
    from scannertools_amd import types
    h, w = 120, 160
    frames = np.concatenate([texture_stream(21, 12, h, w, margin=2)[0], random_frames(21, 1, h, w)])
    rng = np.random.default_rng(22)
    boxes = []
    for i in range(13):
        row = []
        for _ in range(i % 5):                                  # 0 .. 4 boxes per frame
            x1, y1 = float(rng.uniform(0, w - 2)), float(rng.uniform(0, h - 2))
            row.append((x1, y1, float(rng.uniform(int(x1) + 1, w)), float(rng.uniform(int(y1) + 1, h))))
        boxes.append(row)
    boxes[6] = [(0.0, 0.0, 160.0, 120.0), (-0.5, -0.25, 100.9, 100.9), (30.0, 10.0, 130.0, 110.0)]   # whole frame, a negative fraction
    rows = [types.write_bboxes(r) for r in boxes]
    trunc = [types.truncate_bboxes(types.bboxes(r), h, w).tolist() for r in rows]
    return frames, rows, trunc


def _graph(frames, rows):
    from scannertools_amd.engine import Client, NamedStream, NamedVideoStream
    sc = Client()
    sc.ingest_frames("v", frames)
    sc.ingest_rows("b", rows)
    return sc, sc.io.Input([NamedVideoStream(sc, "v")]), sc.io.Input([NamedStream(sc, "b")])


def test_kernel_classes(hip_ctx):
    from scannertools_amd import types
    from scannertools_amd.engine import CacheMode, Client, DeviceType, NamedStream, PerfParams
    frames, rows, trunc = _clip()
    ref = [np.array([R.stat(resized(f, b), "SharpnessCPP") for b in t], np.float32) for f, t in zip(frames, trunc)]
    before = Client().live_buffers()
    for device in (DeviceType.GPU, DeviceType.CPU):
        for batch in (1, 8):
            sc, frame, boxes = _graph(frames, rows)
            out = NamedStream(sc, "o")
            sc.run(sc.io.Output(sc.ops.SharpnessBBoxCPP(frame=frame, bboxes=boxes, device=device, batch=batch), [out]),
                   PerfParams.estimate(), cache_mode=CacheMode.Overwrite)
            raw = sc._tables["o"][0]
            assert [len(e) for e in raw] == [4 * len(t) for t in trunc], (device, batch)
            got = list(out.load())
            for g, r in zip(got, ref):
                assert isinstance(g, tuple) and len(g) == len(r)
                assert (np.array(g, np.float32).view(np.uint32) == r.view(np.uint32)).all(), (device, batch)
            assert types.sharpness_bbox(raw[0]) == ()
            assert sc.live_buffers() == before


def test_python_op(hip_ctx):
    from scannertools_amd import frame_stats
    from scannertools_amd.engine import CacheMode, Client, NamedStream, PerfParams
    frames, rows, trunc = _clip()
    before = Client().live_buffers()
    sc, frame, boxes = _graph(frames, rows)
    out = NamedStream(sc, "o")
    sc.run(sc.io.Output(sc.ops.SharpnessBBox(frame=frame, bboxes=boxes), [out]), PerfParams.estimate(), cache_mode=CacheMode.Overwrite)
    got = list(out.load())
    for f, t, g in zip(frames, trunc, got):
        assert isinstance(g, list) and len(g) == len(t) and all(isinstance(v, np.float64) for v in g)
        assert g == [R.stat(resized(f, b), "Sharpness") for b in t]
    one = pickle.loads(frame_stats.sharpness_bbox(None, frames[6], rows[6]))
    assert one == got[6]
    assert sc.live_buffers() == before


def test_runners_end_to_end(hip_ctx):
    from scannertools_amd import frame_stats
    from scannertools_amd.engine import Client, NamedStream
    frames, rows, trunc = _clip()
    sc = Client()
    sc.ingest_frames("a", frames)
    sc.ingest_frames("b", frames[::-1].copy())
    sc.ingest_rows("a_boxes", rows)
    sc.ingest_rows("b_boxes", rows[::-1])
    cpp = frame_stats.compute_sharpness_bbox_cpp(sc, ["a", "b"], ["a_boxes", NamedStream(sc, "b_boxes")], batch=8)
    py = frame_stats.compute_sharpness_bbox(sc, ["a", "b"], ["a_boxes", "b_boxes"])
    assert len(cpp) == 2 and len(py) == 2
    ref_cpp = [tuple(float(R.stat(resized(f, b), "SharpnessCPP")) for b in t) for f, t in zip(frames, trunc)]
    ref_py = [[R.stat(resized(f, b), "Sharpness") for b in t] for f, t in zip(frames, trunc)]
    assert list(cpp[0].load()) == ref_cpp and list(cpp[1].load()) == ref_cpp[::-1]
    assert list(py[0].load()) == ref_py and list(py[1].load()) == ref_py[::-1]
    # the stored rows are what the readers read
    assert [frame_stats.reader_bbox_cpp(e) for e in sc._tables["a_sharpness_bbox_cpp"][0]] == ref_cpp
    assert [frame_stats.reader(e) for e in sc._tables["a_sharpness_bbox"][0]] == ref_py


# ---- invalid input launches nothing ---------------------------------------------------------------------------------------
def test_invalid_boxes_fail_by_name_and_leave_the_context_usable(hip_ctx):
    from scannertools_amd import _native, types
    from scannertools_amd.engine import CacheMode, DeviceType, NamedStream, PerfParams
    from scannertools_amd.hip import StError  # noqa: F401
    frames = random_frames(31, 4, 60, 80)
    d = torch.from_numpy(frames).cuda()
    L, hh, vp = _native.lib(), hip_ctx._h, ctypes.c_void_p
    hip_ctx._bind()
    sentinel = torch.full((3, 8), -7, dtype=torch.int64, device="cuda")
    K = _native.K_FRAME_STATS
    hip_ctx.timing_enable([K])
    hip_ctx.timing_reset()
    good = [0, 0, 0, 80, 60]
    for bad in ([4, 0, 0, 8, 8], [-1, 0, 0, 8, 8], [1, 5, 0, 5, 8], [1, 0, 9, 8, 9], [1, -1, 0, 8, 8], [1, 0, -1, 8, 8], [1, 0, 0, 81, 8],
                [1, 0, 0, 8, 61], [1, 9, 0, 3, 8]):
        rec = np.array([good, bad, good], np.int32)
        st = L.st_bbox_moments_u8c3_strided(hh, vp(d.data_ptr()), 3 * 60 * 80, 4, 60, 80, rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 3,
                                            vp(sentinel.data_ptr()))
        assert st == _native.ST_ERR_INVALID, bad
        assert b"box 1" in L.st_ctx_last_error(hh)
        tab = (vp * 4)(*[d[i].data_ptr() for i in range(4)])
        st = L.st_bbox_sharpness_u8c3_batch(hh, tab, 4, 60, 80, rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 3, 2, vp(sentinel.data_ptr()))
        assert st == _native.ST_ERR_INVALID, bad
        with pytest.raises(ValueError, match="box 1"):
            hip_ctx.bbox_moments(d, rec)
    rec = np.array([good], np.int32)
    bp = rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    assert L.st_bbox_sharpness_u8c3_strided(hh, vp(d.data_ptr()), 3 * 60 * 80, 4, 60, 80, bp, 1, 0, vp(sentinel.data_ptr())) == _native.ST_ERR_INVALID
    assert L.st_bbox_moments_u8c3_strided(hh, vp(d.data_ptr()), 3 * 60 * 80 - 1, 4, 60, 80, bp, 1, vp(sentinel.data_ptr())) == _native.ST_ERR_INVALID
    assert L.st_bbox_moments_u8c3_strided(hh, vp(d.data_ptr()), 3 * 60 * 80, 4, 60, 80, bp, 1, None) == _native.ST_ERR_INVALID
    assert L.st_bbox_moments_u8c3_strided(hh, vp(d.data_ptr()), 3 * 60 * 80, 4, 60, 80, None, 1, vp(sentinel.data_ptr())) == _native.ST_ERR_INVALID
    hip_ctx.sync()
    # nothing was launched and nothing was written
    assert hip_ctx.timing_read(K)[0] == 0
    assert (sentinel.cpu().numpy() == -7).all()
    hip_ctx.timing_enable([])

    # the ops: row k of the stream is named, before a kernel instance exists
    rows = [types.write_bboxes([(0, 0, 80, 60)]), types.write_bboxes([]), types.write_bboxes([(1, 1, 9, 9), (70, 50, 81, 60)]),
            types.write_bboxes([(2, 2, 4, 4)])]
    for device in (DeviceType.GPU, DeviceType.CPU):
        sc, frame, boxes = _graph(frames, rows)
        with pytest.raises(ValueError, match="row 2: box 1"):
            sc.run(sc.io.Output(sc.ops.SharpnessBBoxCPP(frame=frame, bboxes=boxes, device=device, batch=4), [NamedStream(sc, "o")]),
                   PerfParams.estimate(), cache_mode=CacheMode.Overwrite)
    sc, frame, boxes = _graph(frames, rows[:2] + [rows[3][:-3], rows[3]])
    for node in (sc.ops.SharpnessBBoxCPP(frame=frame, bboxes=boxes, device=DeviceType.GPU), sc.ops.SharpnessBBox(frame=frame, bboxes=boxes)):
        with pytest.raises(ValueError, match="row 2"):
            sc.run(sc.io.Output(node, [NamedStream(sc, "o")]), PerfParams.estimate(), cache_mode=CacheMode.Overwrite)

    # the context works afterwards
    recs = np.array([[3, 5, 6, 75, 56], [0, 0, 0, 80, 60]], np.int64)
    assert (hip_ctx.bbox_moments(d, recs).cpu().numpy() == ref_moments(frames, recs)).all()
