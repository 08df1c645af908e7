"""GPU: st_png_encode_batch and the ImageEncoder kernel classes with format = PNG.  Everywhere the device's streams equal
st_png_encode_host's byte for byte (which tests/test_png_encode.py ties to the restatement and to zlib); round trips go through
the library's own PNG decoder.  Launch counts: DESIGN.md 4.18."""
import ctypes
import zlib

import numpy as np
import pytest

import ref_png_encode_np as ref
from png_encode_cases import CASES, FILTERS, noise, photo, sheet

pytestmark = pytest.mark.gpu

ST_ERR_INVALID = 1
PNG_LAUNCHES = 4   # filter, deflate, layout, pack


def _host(frame, flt):
    from scannertools_amd.hip import png_encode_host
    return png_encode_host(frame, flt)


def _dev(ctx, frames, flt="adaptive"):
    import torch
    if isinstance(frames, np.ndarray):
        frames = torch.from_numpy(frames).cuda()
    return ctx.encode_png(frames, flt)


def _why(name, got, want):
    n = min(len(got), len(want))
    d = np.nonzero(np.frombuffer(got[:n], np.uint8) != np.frombuffer(want[:n], np.uint8))[0]
    return (name, len(got), len(want), int(d[0]) if len(d) else n)


@pytest.fixture(scope="module")
def host_streams():
    """st_png_encode_host of every case: computed once, never changed."""
    return {name: _host(fr, flt) for name, (fr, flt) in CASES.items()}


def test_every_case_equals_the_host_twin(hip_ctx, host_streams):
    """Geometry (1 x 1 at 1, 3, 4 channels, 1 x 5, 5 x 1, 3 x 7 x 3, 17 x 21 x 4, 33 x 65 x 3, 64 x 64 x 3), filtered sizes of 32 767,
    32 768 and 32 769 bytes, four zero pieces with a run across every boundary, every run length around 3 and around the multiples of
    258, all-zero and all-255 frames, noise (stored pieces), stored beside coded pieces, Fibonacci counts (the 15-bit limit), every
    filter on a gradient, on noise and on a sheet."""
    for name, (fr, flt) in CASES.items():
        (got,) = _dev(hip_ctx, fr[None], flt)
        assert got == host_streams[name], _why(name, got, host_streams[name])
    assert len(CASES) >= 40


def test_batch_equals_singles(hip_ctx):
    """n = 1, 3, 33 with mixed content (stored, coded and flat frames side by side), the same frame pointer repeated, frames at odd
    addresses."""
    import torch
    h, w, c = 40, 37, 3
    kinds = [photo(h, w, c, 11), noise(h, w, c, 12), np.zeros((h, w, c), np.uint8), sheet(h, w, c, 13), np.full((h, w, c), 255, np.uint8)]
    singles = [_host(k, "adaptive") for k in kinds]
    for n in (1, 3, 33):
        order = [(5 * i + i // 5) % 5 for i in range(n)]
        got = _dev(hip_ctx, np.stack([kinds[i] for i in order]))
        assert got == [singles[i] for i in order], n
    dev = [torch.from_numpy(k).cuda() for k in kinds]
    order = (1, 1, 0, 1, 4, 4, 2, 1)
    assert hip_ctx.encode_png([dev[i] for i in order]) == [singles[i] for i in order]
    buf = torch.zeros((5, h * w * c + 8), dtype=torch.uint8, device="cuda")
    views = []
    for k in range(5):
        v = buf[k, k + 1:k + 1 + h * w * c].view(h, w, c)
        v.copy_(dev[k])
        views.append(v)
    assert len({v.data_ptr() % 4 for v in views}) == 4
    assert hip_ctx.encode_png(views) == singles
    assert hip_ctx.encode_png([]) == []


def test_fetch_writes_nothing_around_its_buffers(hip_ctx):
    """Guard bytes around the host buffers of st_png_encode_fetch; a capacity too small is refused with nothing written."""
    import torch
    from scannertools_amd import _native
    L, hh = _native.lib(), hip_ctx._h
    hip_ctx._bind()
    frames = torch.from_numpy(np.stack([photo(20, 30, 4, 3), noise(20, 30, 4, 4)])).cuda()
    want = hip_ctx.encode_png(frames)
    sizes = (ctypes.c_size_t * 2)()
    assert L.st_png_encode_fetch(hh, None, sizes, 0) == 0 and list(sizes) == [len(s) for s in want]
    most, guard = max(sizes), 32
    store = np.full((2, guard + most + guard), 0xA5, np.uint8)
    bufs = (ctypes.c_void_p * 2)(*[store[i].ctypes.data + guard for i in range(2)])
    assert L.st_png_encode_fetch(hh, bufs, sizes, most - 1) == ST_ERR_INVALID and (store == 0xA5).all()
    assert "the buffers hold" in L.st_ctx_last_error(hh).decode()
    assert L.st_png_encode_fetch(hh, bufs, sizes, most) == 0
    for i in range(2):
        assert store[i, guard:guard + sizes[i]].tobytes() == want[i]
        assert (store[i, :guard] == 0xA5).all() and (store[i, guard + sizes[i]:] == 0xA5).all()


def test_more_frames_than_one_grid_dimension(hip_ctx):
    """65 537 frames of 2 x 2 x 3 in one call, two pictures alternating."""
    import torch
    n = 65537
    pics = np.stack([noise(2, 2, 3, 21), np.full((2, 2, 3), 9, np.uint8)])
    want = [_host(pics[0], "adaptive"), _host(pics[1], "adaptive")]
    dev = torch.from_numpy(pics).cuda()
    got = hip_ctx.encode_png([dev[i & 1] for i in range(n)])
    assert len(got) == n
    wrong = [i for i in range(n) if got[i] != want[i & 1]]
    assert not wrong, (len(wrong), wrong[:5])
    hip_ctx.release_workspace()


def test_two_calls_of_different_shapes_back_to_back(hip_ctx):
    import torch
    a, b = photo(50, 700, 1, 31), sheet(9, 11, 4, 32)
    da, db = torch.from_numpy(a[None]).cuda(), torch.from_numpy(np.stack([b, b[::-1].copy()])).cuda()
    for _ in range(2):
        assert hip_ctx.encode_png(da, "paeth") == [_host(a, "paeth")]
        assert hip_ctx.encode_png(db, "up") == [_host(b, "up"), _host(b[::-1], "up")]


def test_refusals_come_before_any_launch_and_keep_the_last_streams(hip_ctx):
    import torch
    from scannertools_amd import _native
    L, hh, vp = _native.lib(), hip_ctx._h, ctypes.c_void_p
    hip_ctx._bind()
    frame = torch.from_numpy(photo(8, 8, 3, 41)).cuda()
    (want,) = hip_ctx.encode_png(frame[None])
    tab = (vp * 2)(frame.data_ptr(), frame.data_ptr())
    holed = (vp * 2)(frame.data_ptr(), None)
    hip_ctx.timing_enable(list(range(_native.K_COUNT)))
    hip_ctx.timing_reset()
    refusals = [((tab, 0, 8, 8, 3, 5), "png_encode: n = 0 (at least one frame)"),
                ((tab, -3, 8, 8, 3, 5), "png_encode: n = -3 (at least one frame)"),
                ((tab, 2, 8, 8, 2, 5), "png_encode: 2 channel(s) cannot be written"),
                ((tab, 2, 8, 8, 0, 5), "png_encode: 0 channel(s) cannot be written"),
                ((tab, 2, 0, 8, 3, 5), "png_encode: frame size 8x0 is outside 1..65535"),
                ((tab, 2, 8, 65536, 3, 5), "png_encode: frame size 65536x8 is outside 1..65535"),
                ((tab, 2, 8, 8, 3, 6), "png_encode: filter 6 is not supported"),
                ((tab, 2, 8, 8, 3, -1), "png_encode: filter -1 is not supported"),
                ((None, 2, 8, 8, 3, 5), "png_encode: null frame table"),
                ((holed, 2, 8, 8, 3, 5), "png_encode: frame 1 is a null pointer")]
    sizes = (ctypes.c_size_t * 1)()
    for (t, n, h, w, c, f), words in refusals:
        assert L.st_png_encode_batch(hh, t, n, h, w, c, f) == ST_ERR_INVALID, words
        msg = L.st_ctx_last_error(hh).decode()
        assert words in msg, (words, msg)
        # the previous call's stream is still there
        assert L.st_png_encode_fetch(hh, None, sizes, 0) == 0 and sizes[0] == len(want)
        buf = np.zeros(len(want), np.uint8)
        assert L.st_png_encode_fetch(hh, (vp * 1)(buf.ctypes.data), sizes, len(want)) == 0 and buf.tobytes() == want
    assert sum(hip_ctx.timing_read(k)[0] for k in range(_native.K_COUNT)) == 0   # nothing was launched
    hip_ctx.timing_enable([])
    with pytest.raises(ValueError, match="png filter must be one of"):
        hip_ctx.encode_png(frame[None], "best")
    # a context that never encoded has nothing to fetch
    from scannertools_amd.hip import HipContext
    with HipContext(0) as fresh:
        assert L.st_png_encode_fetch(fresh._h, None, sizes, 0) == ST_ERR_INVALID
        assert "no st_png_encode_batch call" in L.st_ctx_last_error(fresh._h).decode()


def test_launch_count(hip_ctx):
    """Four launches a call, whatever its size and filter; only the jpeg slot counts."""
    import torch
    from scannertools_amd import _native
    hip_ctx.timing_enable(list(range(_native.K_COUNT)))
    for frames, flt in ((photo(5, 5, 1)[None], "adaptive"), (np.stack([noise(90, 130, 3)] * 3), "none"), (np.zeros((2, 128, 1023, 1), np.uint8), "sub")):
        hip_ctx.timing_reset()
        hip_ctx.encode_png(torch.from_numpy(frames).cuda(), flt)
        counts = [hip_ctx.timing_read(k)[0] for k in range(_native.K_COUNT)]
        assert counts[_native.K_JPEG] == PNG_LAUNCHES and sum(counts) == PNG_LAUNCHES, counts
    hip_ctx.timing_enable([])


def test_a_1080p_frame_decodes_back_exactly(hip_ctx):
    """1080 x 1920 x 3: 190 pieces.  Decoded by the library's PNG decoder on the device and inflated by zlib."""
    import torch
    frame = sheet(1080, 1920, 3, 51)
    (got,) = hip_ctx.encode_png(torch.from_numpy(frame[None]).cuda())
    assert got == _host(frame, "adaptive")
    back = hip_ctx.decode_png([got]).cpu().numpy()[0]
    assert back.shape == frame.shape and np.array_equal(back, frame)
    chunks = ref.chunks(got)
    assert [t for t, _, _ in chunks] == [b"IHDR"] + [b"IDAT"] * 191 + [b"IEND"]
    assert all(zlib.crc32(t + d) & 0xFFFFFFFF == crc for t, d, crc in chunks)
    raw = zlib.decompress(b"".join(d for t, d, _ in chunks if t == b"IDAT"))
    assert len(raw) == 1080 * (1 + 1920 * 3)


def _client(frames):
    from scannertools_amd.engine import Client, NamedVideoStream
    sc = Client()
    sc.ingest_frames("pics", frames)
    return sc, sc.io.Input([NamedVideoStream(sc, "pics")])


def test_kernel_classes_write_the_host_twins_streams():
    from scannertools_amd import engine
    from scannertools_amd.engine import CacheMode, DeviceType, NamedStream, PerfParams
    L = engine._imgproc()
    before = (L.stshim_live_buffers(0), L.stshim_live_buffers(1))
    frames = np.stack([photo(40, 34, 3, 61), noise(40, 34, 3, 62), np.zeros((40, 34, 3), np.uint8), sheet(40, 34, 3, 63)] * 3)
    for device in (DeviceType.GPU, DeviceType.CPU):
        for flt in ("adaptive", "paeth"):
            sc, frame = _client(frames)
            out = NamedStream(sc, "png")
            sc.run(sc.io.Output(sc.ops.ImageEncoder(frame=frame, format="png", png_filter=flt, device=device, batch=5), [out]),
                   PerfParams.estimate(), cache_mode=CacheMode.Overwrite)
            rows = list(out.load())
            assert len(rows) == 12                                  # executes of 5, 5 and 2 rows
            for fr, r in zip(frames, rows):
                assert bytes(r) == _host(fr, flt), (device, flt)
    assert (L.stshim_live_buffers(0), L.stshim_live_buffers(1)) == before


@pytest.mark.parametrize("channels", [1, 3, 4])
def test_round_trip_through_the_decoder_in_a_graph(channels):
    """ImageEncoder(format=png) -> ImageDecoder(png = DECODE) returns the input frames exactly."""
    from scannertools_amd.engine import CacheMode, DeviceType, NamedStream, PerfParams
    frames = np.stack([photo(33, 65, channels, 70 + i) if i % 3 else sheet(33, 65, channels, 70 + i) for i in range(9)])
    sc, frame = _client(frames)
    img = sc.ops.ImageEncoder(frame=frame, format="png", device=DeviceType.GPU, batch=4)
    out = NamedStream(sc, "decoded")
    sc.run(sc.io.Output(sc.ops.ImageDecoder(img=img, device=DeviceType.GPU, batch=4, args={"png": "decode"}), [out]), PerfParams.estimate(),
           cache_mode=CacheMode.Overwrite)
    rows = list(out.load())
    assert len(rows) == 9
    for fr, r in zip(frames, rows):
        assert r.dtype == np.uint8 and r.shape == fr.shape and np.array_equal(r, fr)


def test_montage_sheets_are_written_losslessly():
    """Montage -> ImageEncoder(format=png): zlib and a plain unfilter give the sheet the Montage op emits."""
    from scannertools_amd.engine import CacheMode, DeviceType, NamedStream, PerfParams
    frames = np.stack([photo(48, 64, 3, 80 + i) for i in range(8)])
    sc, frame = _client(frames)
    kw = dict(frame=frame, num_frames=8, target_width=32, frames_per_row=4, device=DeviceType.GPU, batch=4)
    sheets, pngs = NamedStream(sc, "sheets"), NamedStream(sc, "pngs")
    sc.run([sc.io.Output(sc.ops.Montage(**kw), [sheets]),
            sc.io.Output(sc.ops.ImageEncoder(frame=sc.ops.Montage(**kw), format="png", device=DeviceType.GPU, batch=4), [pngs])],
           PerfParams.estimate(), cache_mode=CacheMode.Overwrite)
    want, got = [r for r in sheets.load()], [bytes(r) for r in pngs.load()]
    assert len(want) == len(got) == 8 and np.asarray(want[7]).any()   # the last row carries the sheet, the others zeros of its shape
    for s, g in zip(want, got):
        s = np.asarray(s)
        assert s.shape == (48, 128, 3)
        chunks = ref.chunks(g)
        raw = zlib.decompress(b"".join(d for t, d, _ in chunks if t == b"IDAT"))
        assert np.array_equal(ref.unfilter(raw, *s.shape), s) and g == _host(s, "adaptive")
