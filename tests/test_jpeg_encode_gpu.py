"""GPU: st_jpeg_encode_batch / st_jpeg_encode_fetch and the ImageEncoder kernel classes against the streams Pillow wrote
(tests/golden/jpeg_encode_golden.npz, the only thing this file reads): byte for byte."""
import ctypes
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_encode_golden.npz"))
CASES = [str(c) for c in GOLD["cases"]]
BATCH = [str(c) for c in GOLD["batch"]]
ST_ERR_INVALID, ST_ERR_UNSUPPORTED = 1, 4


def _cfg(name):
    return json.loads(str(GOLD[name + "__cfg"]))


def _jpg(name):
    return GOLD[name + "__jpg"].tobytes()


def _img(name):
    return GOLD[_cfg(name)["img"]]


def _first_difference(a, b):
    n = min(len(a), len(b))
    d = np.nonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))[0]
    return (len(a), len(b), int(d[0]) if len(d) else n)


@pytest.fixture(scope="module")
def batch_singles(hip_ctx):
    """The 33 pictures of one shape, each encoded in a call of its own: computed once, never changed."""
    import torch
    return [hip_ctx.encode_jpeg(torch.from_numpy(_img(n)[None]).cuda())[0] for n in BATCH]


def test_every_golden_case_is_byte_identical(hip_ctx):
    """1x1 up to 152x16, all three samplings, qualities 1 / 50 / 95 / 100, noise / flat / checker / ramp: edge columns and rows,
    padding blocks, both row replications, ZRL, EOB-only blocks, categories 11 and 10, stuffed bytes, RST7 -> RST0."""
    import torch
    for name in CASES:
        c = _cfg(name)
        (got,) = hip_ctx.encode_jpeg(torch.from_numpy(_img(name)[None]).cuda(), c["quality"], c["subsampling"])
        want = _jpg(name)
        assert got == want, (name,) + _first_difference(got, want)


def test_batch_equals_singles_and_golden(hip_ctx, batch_singles):
    import torch
    frames = torch.from_numpy(np.stack([_img(n) for n in BATCH])).cuda()
    got = hip_ctx.encode_jpeg(frames)
    assert len(got) == 33
    for i, n in enumerate(BATCH):
        assert got[i] == batch_singles[i] == _jpg(n), (n,) + _first_difference(got[i], _jpg(n))
    # frames handed as separate buffers at odd addresses, one of them several times
    buf = torch.zeros((4, 24 * 32 * 3 + 5), dtype=torch.uint8, device="cuda")
    views = []
    for k in range(4):
        v = buf[k, k + 1:k + 1 + 24 * 32 * 3].view(24, 32, 3)
        v.copy_(frames[k])
        views.append(v)
    assert views[1].data_ptr() % 4 != views[2].data_ptr() % 4
    got = hip_ctx.encode_jpeg([views[0], views[3], views[3], views[1], views[3], views[2]])
    assert got == [batch_singles[i] for i in (0, 3, 3, 1, 3, 2)]
    assert hip_ctx.encode_jpeg([]) == []


def test_consecutive_calls_do_not_leak_tables(hip_ctx):
    import torch
    names = ["17x7_noise_q1_420", "17x7_noise_q100_420", "17x7_noise_q50_444", "17x7_noise_q95_422", "17x7_noise_q1_420"]
    frame = torch.from_numpy(_img(names[0])[None]).cuda()
    for name in names + names[::-1]:
        c = _cfg(name)
        assert hip_ctx.encode_jpeg(frame, c["quality"], c["subsampling"])[0] == _jpg(name), name


def test_more_frames_than_one_grid_dimension(hip_ctx):
    """65 537 frames of 8 x 8 in one call, two pictures alternating: every stream is that of its frame."""
    import torch
    n = 65537
    pics = torch.from_numpy(np.stack([_img("8x8_noise_q95_420"), _img("8x8_ramp_q50_420")])).cuda()
    want = [_jpg("8x8_noise_q95_420"), hip_ctx.encode_jpeg(pics[1:2], 95, "4:2:0")[0]]
    assert hip_ctx.encode_jpeg(pics[0:1], 95, "4:2:0")[0] == want[0] and want[0] != want[1]
    got = hip_ctx.encode_jpeg([pics[i & 1] for i in range(n)], 95, "4:2:0")
    assert len(got) == n
    wrong = [i for i in range(n) if got[i] != want[i & 1]]
    assert not wrong, (len(wrong), wrong[:5])
    hip_ctx.release_workspace()


def test_refusals_name_their_cause_before_anything_is_launched(hip_ctx):
    import torch
    from scannertools_amd import _native
    L, hh, vp = _native.lib(), hip_ctx._h, ctypes.c_void_p
    hip_ctx._bind()
    frame = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    tab = (vp * 2)(frame.data_ptr(), frame.data_ptr())
    sizes = (ctypes.c_size_t * 2)()
    hip_ctx.timing_enable(list(range(_native.K_COUNT)))
    hip_ctx.timing_reset()

    def refused(status, cause, *args):
        assert L.st_jpeg_encode_batch(hh, *args) == status, args
        msg = L.st_ctx_last_error(hh).decode()
        assert cause in msg, (args, msg)
        # a refused call leaves nothing to fetch
        assert L.st_jpeg_encode_fetch(hh, None, sizes, 0) == ST_ERR_INVALID and "no st_jpeg_encode_batch call" in L.st_ctx_last_error(hh).decode()

    for q in (0, -1, 101):
        refused(ST_ERR_INVALID, "quality %d is outside 1..100" % q, tab, 2, 8, 8, q, 2, 2)
    for hs, vs in ((1, 2), (4, 1), (2, 4), (0, 0)):
        refused(ST_ERR_UNSUPPORTED, "luma sampling %dx%d is not supported" % (hs, vs), tab, 2, 8, 8, 50, hs, vs)
    for h, w in ((0, 8), (8, 0), (65536, 8), (8, 65536)):
        refused(ST_ERR_INVALID, "frame size %dx%d is outside 1..65535" % (w, h), tab, 2, h, w, 50, 2, 2)
    refused(ST_ERR_INVALID, "n = -1 is negative", tab, -1, 8, 8, 50, 2, 2)
    refused(ST_ERR_INVALID, "null frame table", None, 2, 8, 8, 50, 2, 2)
    refused(ST_ERR_INVALID, "frame 1 is a null pointer", (vp * 2)(frame.data_ptr(), None), 2, 8, 8, 50, 2, 2)
    assert sum(hip_ctx.timing_read(k)[0] for k in range(_native.K_COUNT)) == 0          # nothing was launched
    # n = 0 succeeds and does nothing; its fetch hands over nothing
    assert L.st_jpeg_encode_batch(hh, None, 0, 8, 8, 50, 2, 2) == 0 and L.st_jpeg_encode_fetch(hh, None, None, 0) == 0
    assert sum(hip_ctx.timing_read(k)[0] for k in range(_native.K_COUNT)) == 0
    # a fetch into buffers that are too small reports the sizes and copies nothing
    assert L.st_jpeg_encode_batch(hh, tab, 2, 8, 8, 50, 2, 2) == 0
    small = np.full((2, 16), 0x5A, np.uint8)
    bufs = (vp * 2)(small[0].ctypes.data, small[1].ctypes.data)
    assert L.st_jpeg_encode_fetch(hh, bufs, sizes, 16) == ST_ERR_INVALID and "the buffers hold 16" in L.st_ctx_last_error(hh).decode()
    assert sizes[0] == sizes[1] > 629 and (small == 0x5A).all()
    hip_ctx.timing_enable([])


def test_only_the_jpeg_slot_counts_launches(hip_ctx):
    import torch
    from scannertools_amd import _native
    hip_ctx.timing_enable(list(range(_native.K_COUNT)))
    hip_ctx.timing_reset()
    frames = torch.from_numpy(np.stack([_img(n) for n in BATCH[:5]])).cuda()
    assert hip_ctx.encode_jpeg(frames) == [_jpg(n) for n in BATCH[:5]]
    counts = [hip_ctx.timing_read(k)[0] for k in range(_native.K_COUNT)]
    assert counts[_native.K_JPEG] == 4 and sum(counts) == 4, counts     # transform, entropy, layout, pack
    hip_ctx.timing_enable([])


def _client_with_batch():
    from scannertools_amd.engine import Client, NamedVideoStream
    sc = Client()
    sc.ingest_frames("pics", np.stack([_img(n) for n in BATCH]))
    return sc, sc.io.Input([NamedVideoStream(sc, "pics")])


def test_kernel_classes_write_the_golden_streams():
    from scannertools_amd import engine
    from scannertools_amd.engine import CacheMode, DeviceType, NamedStream, PerfParams
    L = engine._imgproc()
    before = (L.stshim_live_buffers(0), L.stshim_live_buffers(1))
    for device in (DeviceType.GPU, DeviceType.CPU):
        sc, frame = _client_with_batch()
        out = NamedStream(sc, "jpgs")
        sc.run(sc.io.Output(sc.ops.ImageEncoder(frame=frame, device=device, batch=8), [out]), PerfParams.estimate(), cache_mode=CacheMode.Overwrite)
        rows = list(out.load())
        assert len(rows) == 33                                    # executes of 8, 8, 8, 8 and 1 rows
        for n, r in zip(BATCH, rows):
            assert bytes(r) == _jpg(n), (device, n)
    # other arguments: the defaults spelled out as an empty message, and another quality and sampling
    sc, frame = _client_with_batch()
    a, b = NamedStream(sc, "a"), NamedStream(sc, "b")
    sc.run([sc.io.Output(sc.ops.ImageEncoder(frame=frame, quality=0, subsampling="", device=DeviceType.GPU, batch=33), [a]),
            sc.io.Output(sc.ops.ImageEncoder(frame=frame, quality=50, subsampling="4:4:4", device=DeviceType.GPU, batch=5), [b])],
           PerfParams.estimate(), cache_mode=CacheMode.Overwrite)
    assert [bytes(r) for r in a.load()] == [_jpg(n) for n in BATCH]
    from scannertools_amd.hip import probe_jpeg
    for r in b.load():
        info = probe_jpeg(r)
        assert (info["h"], info["w"], info["h_samp"], info["v_samp"], info["restart_interval"]) == (24, 32, 1, 1, 4)
    assert (L.stshim_live_buffers(0), L.stshim_live_buffers(1)) == before


def test_frames_that_are_not_u8c3_are_refused_by_name():
    """Before any kernel instance exists: the kernel class could only abort."""
    from scannertools_amd.engine import Client, DeviceType, NamedVideoStream
    sc = Client()
    sc.ingest_frames("gray", np.zeros((2, 8, 8, 1), np.uint8))
    sc.ingest_frames("float", np.zeros((2, 8, 8, 3), np.float32))
    for stream, what in (("gray", "(8, 8, 1) uint8"), ("float", "(8, 8, 3) float32")):
        frame = sc.io.Input([NamedVideoStream(sc, stream)])
        with pytest.raises(ValueError, match="ImageEncoder: row 0 is .*not an \\(h, w, 3\\) uint8 frame") as e:
            sc.ops.ImageEncoder(frame=frame, device=DeviceType.GPU, batch=2).rows([0, 1])
        assert what in str(e.value)


def test_round_trip_through_the_decoder_in_a_graph():
    """ImageEncoder -> ImageDecoder: the frames are what Pillow decodes its own streams to."""
    from scannertools_amd.engine import CacheMode, DeviceType, NamedStream, PerfParams
    sc, frame = _client_with_batch()
    img = sc.ops.ImageEncoder(frame=frame, device=DeviceType.GPU, batch=16)
    out = NamedStream(sc, "decoded")
    sc.run(sc.io.Output(sc.ops.ImageDecoder(img=img, device=DeviceType.GPU, batch=16), [out]), PerfParams.estimate(), cache_mode=CacheMode.Overwrite)
    rows = list(out.load())
    assert len(rows) == 33
    for n, r in zip(BATCH, rows):
        want = GOLD[n + "__dec"]
        assert r.dtype == np.uint8 and r.shape == want.shape and np.array_equal(r, want), n


def test_montage_feeds_the_encoder():
    from scannertools_amd.engine import Client, DeviceType, NamedVideoStream
    from scannertools_amd.hip import probe_jpeg
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (13, 60, 80, 3), dtype=np.uint8)
    sc = Client()
    sc.ingest_frames("in", frames)
    m = sc.ops.Montage(frame=sc.io.Input([NamedVideoStream(sc, "in")]), num_frames=13, target_width=40, frames_per_row=4,
                       device=DeviceType.GPU, batch=13)
    rows = sc.ops.ImageEncoder(frame=m, device=DeviceType.GPU, batch=1).rows([12])     # the one row that carries the canvas
    want = m.rows([12])[0]
    assert len(rows) == 1
    info = probe_jpeg(rows[0])
    assert (info["h"], info["w"], info["channels"]) == want.shape == (120, 160, 3)
    assert (info["h_samp"], info["v_samp"], info["restart_interval"]) == (2, 2, 10)
