"""GPU: st_jpeg_decode_batch and the ImageDecoder kernel classes against Pillow's golden frames
(tests/golden/jpeg_golden.npz, the only thing this file reads): byte for byte."""
import ctypes
import os

import numpy as np
import pytest

from util import env_threads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_golden.npz"))
CASES = [str(c) for c in GOLD["cases"]]
BATCH = [str(c) for c in GOLD["batch"]]


def _jpg(name):
    return GOLD[name + "__jpg"].tobytes()


def _img(name):
    return GOLD[name + "__img"]


def test_every_golden_case_is_byte_exact(hip_ctx):
    """Includes 1x1, 3x3 and 2x5 (replication instead of the fancy filter), odd widths (byte stores), widths that are a
    multiple of 4 (dword stores) and of 16 (16-byte stores), restart intervals, optimised tables and one-component streams."""
    from scannertools_amd import _native
    hip_ctx.timing_enable([_native.K_JPEG])
    hip_ctx.timing_reset()
    for name in CASES:
        got = hip_ctx.decode_jpeg([_jpg(name)]).cpu().numpy()
        want = _img(name)
        assert got.shape == (1,) + want.shape, name
        assert np.array_equal(got[0], want), (name, int(np.abs(got[0].astype(int) - want).max()), int((got[0] != want).sum()))
    launches, _ = hip_ctx.timing_read(_native.K_JPEG)
    assert launches == len(CASES)          # one bracket (IDCT + colour launch) per sub-batch
    hip_ctx.timing_enable([])


def test_store_width_does_not_change_a_byte(hip_ctx):
    """The same streams into frames that start on a 16-byte boundary, on a 4-byte one and on an odd byte: the 16-byte,
    dword and byte store paths of the colour kernel."""
    import torch
    for name in ("48x24_vec_444", "48x24_vec_422", "48x24_vec_420", "48x24_vec_gray", "136x248_420", "32x24_batch_444"):
        want = _img(name)
        nbytes = want.size
        for offset in (0, 4, 1):
            buf = torch.full((nbytes + 64,), 0x5A, dtype=torch.uint8, device=hip_ctx.device)
            out = buf[offset:offset + nbytes].view((1,) + want.shape)
            hip_ctx.decode_jpeg([_jpg(name)], out=out)
            host = buf.cpu().numpy()
            assert np.array_equal(host[offset:offset + nbytes].reshape(want.shape), want), (name, offset)
            assert (host[:offset] == 0x5A).all() and (host[offset + nbytes:] == 0x5A).all(), (name, offset)


def test_batches_equal_singles_at_any_thread_count(hip_ctx):
    singles = [hip_ctx.decode_jpeg([_jpg(n)]).cpu().numpy()[0] for n in BATCH]
    for n, want in zip(BATCH, singles):
        assert np.array_equal(want, _img(n)), n
    for count in (1, 8, 33):
        results = {}
        for threads in (16, 1, 3):           # 1: one stream per sub-batch, the two page-locked slots alternate 33 times
            with env_threads("ST_JPEG_THREADS", threads):
                results[threads] = hip_ctx.decode_jpeg([_jpg(n) for n in BATCH[:count]]).cpu().numpy()
        assert np.array_equal(results[16], np.stack(singles[:count])), count
        assert np.array_equal(results[1], results[16]) and np.array_equal(results[3], results[16]), count


def test_mixed_subsampling_in_one_call(hip_ctx):
    names = BATCH[:3] + ["32x24_batch_444"] + BATCH[3:5]
    for threads in (16, 2):
        with env_threads("ST_JPEG_THREADS", threads):
            got = hip_ctx.decode_jpeg([_jpg(n) for n in names]).cpu().numpy()
        for i, n in enumerate(names):
            assert np.array_equal(got[i], _img(n)), (threads, n)


def test_bad_stream_fails_the_call_and_writes_nothing(hip_ctx):
    import torch
    from scannertools_amd import _native
    from scannertools_amd.hip import StError
    L, hh, vp = _native.lib(), hip_ctx._h, ctypes.c_void_p
    hip_ctx._bind()
    good = [_jpg(n) for n in BATCH[:4]]
    scan = good[0].index(b"\xff\xda")
    bad_streams = [(_jpg("progressive"), _native.ST_ERR_UNSUPPORTED, b"progressive"),
                   (_jpg("random_bytes"), _native.ST_ERR_INVALID, b"not a JPEG"),
                   (b"", _native.ST_ERR_INVALID, b"empty"),
                   (_jpg("48x24_vec_420"), _native.ST_ERR_INVALID, b"stream 2 is 48x24"),            # another shape
                   (_jpg("32x24_batch_444")[:200], _native.ST_ERR_INVALID, b"stream 2"),           # cut inside the tables
                   (good[1][:scan + (len(good[1]) - scan) // 2], _native.ST_ERR_INVALID, b"scan")]  # cut inside the scan
    with env_threads("ST_JPEG_THREADS", 16):
        for bad, status, cause in bad_streams:
            streams = good[:2] + [bad] + good[2:]
            n = len(streams)
            out = torch.full((n, 24, 32, 3), 0xA5, dtype=torch.uint8, device=hip_ctx.device)
            keep = [ctypes.create_string_buffer(s, len(s)) for s in streams]
            bufs = (vp * n)(*[ctypes.addressof(k) for k in keep])
            sizes = (ctypes.c_size_t * n)(*[len(s) for s in streams])
            to = (vp * n)(*[out[i].data_ptr() for i in range(n)])
            st = L.st_jpeg_decode_batch(hh, bufs, sizes, n, 24, 32, 3, to)
            msg = L.st_ctx_last_error(hh)
            assert st == status and cause in msg and b"stream 2" in msg, (st, msg)
            hip_ctx.sync()
            assert (out.cpu().numpy() == 0xA5).all(), msg
            with pytest.raises(StError, match="stream 2"):
                hip_ctx.decode_jpeg(streams)
        # bad arguments
        n = 1
        keep = ctypes.create_string_buffer(good[0], len(good[0]))
        bufs, sizes = (vp * 1)(ctypes.addressof(keep)), (ctypes.c_size_t * 1)(len(good[0]))
        out = torch.full((1, 24, 32, 3), 0xA5, dtype=torch.uint8, device=hip_ctx.device)
        to = (vp * 1)(out.data_ptr())
        assert L.st_jpeg_decode_batch(hh, bufs, sizes, 1, 24, 32, 1, to) == _native.ST_ERR_INVALID       # channels differ
        assert L.st_jpeg_decode_batch(hh, bufs, sizes, 1, 24, 32, 2, to) == _native.ST_ERR_INVALID
        assert L.st_jpeg_decode_batch(hh, bufs, sizes, 1, 32, 24, 3, to) == _native.ST_ERR_INVALID       # h and w swapped
        assert L.st_jpeg_decode_batch(hh, None, sizes, 1, 24, 32, 3, to) == _native.ST_ERR_INVALID
        assert L.st_jpeg_decode_batch(hh, bufs, sizes, 1, 24, 32, 3, (vp * 1)(None)) == _native.ST_ERR_INVALID
        assert L.st_jpeg_decode_batch(hh, bufs, sizes, 0, 24, 32, 3, to) == _native.ST_OK
        hip_ctx.sync()
        assert (out.cpu().numpy() == 0xA5).all()
    # the context works afterwards
    got = hip_ctx.decode_jpeg(good).cpu().numpy()
    assert all(np.array_equal(got[i], _img(BATCH[i])) for i in range(4))
    assert hip_ctx.decode_jpeg([]).shape[0] == 0


def test_corrupt_scan_in_a_later_sub_batch_fails_the_call_and_both_decoders_slots_survive(hip_ctx):
    """Seven 16 x 16 streams on two threads are four sub-batches, so both page-locked slots are refilled; stream 5 (the third
    sub-batch, slot 0's second filling) has whole markers and a scan cut in the middle, which shows only while a worker
    decodes it.  The context then decodes the good streams: the slots' events and busy flags survive a failed call.  The same
    with PNG streams afterwards: the two decoders' slots are separate."""
    import png_cases as pc
    from scannertools_amd import _native, hip
    from scannertools_amd.hip import StError
    names = [c for c in CASES if c.startswith("16x16_") and "gray" not in c][:7]
    good = [_jpg(n) for n in names]
    scan = good[5].index(b"\xff\xda")
    bad = good[5][:scan + (len(good[5]) - scan) // 2]
    assert len(good) == 7 and hip.probe_jpeg(bad) == hip.probe_jpeg(good[5])             # header parsing passes
    with env_threads("ST_JPEG_THREADS", 2):
        with pytest.raises(StError, match="jpeg: stream 5: ") as e:
            hip_ctx.decode_jpeg(good[:5] + [bad] + good[6:])
        assert e.value.status == _native.ST_ERR_INVALID and "scan" in str(e.value)
        got = hip_ctx.decode_jpeg(good).cpu().numpy()
    assert all(np.array_equal(got[i], _img(n)) for i, n in enumerate(names))
    rng = np.random.default_rng(13)
    pxs = [pc.picture(rng, 12, 11, 6) for _ in range(7)]
    pngs = [pc.write_png(p, 6) for p in pxs]
    z = pc.deflate(pc.filter_rows(pc.scanlines(pxs[5], 6, 8), 4, [1] * 12).tobytes())
    with env_threads("ST_PNG_THREADS", 2):
        with pytest.raises(StError, match="png: stream 5: png: zlib: Adler-32 mismatch") as e:
            hip_ctx.decode_png(pngs[:5] + [pc.write_png(pxs[5], 6, zdata=z[:-1] + bytes([z[-1] ^ 1]))] + pngs[6:])
        assert e.value.status == _native.ST_ERR_INVALID
        got = hip_ctx.decode_png(pngs).cpu().numpy()
    assert all(np.array_equal(got[i], pc.expected(p, 6, 8)) for i, p in enumerate(pxs))


def _run_decoder(device, names, batch, args=None):
    from scannertools_amd.engine import CacheMode, Client, NamedStream, PerfParams
    sc = Client()
    sc.ingest_rows("jpgs", [_jpg(n) for n in names])
    img = sc.io.Input([NamedStream(sc, "jpgs")])
    out = NamedStream(sc, "frames")
    sc.run(sc.io.Output(sc.ops.ImageDecoder(img=img, device=device, batch=batch, args=args), [out]), PerfParams.estimate(),
           cache_mode=CacheMode.Overwrite)
    return list(out.load())


def test_kernel_classes_decode_the_golden_frames():
    from scannertools_amd.engine import DeviceType
    for device in (DeviceType.GPU, DeviceType.CPU):
        frames = _run_decoder(device, BATCH[:9], 4)                        # executes of 4, 4 and 1 rows
        assert len(frames) == 9
        for n, f in zip(BATCH, frames):
            assert f.dtype == np.uint8 and np.array_equal(f, _img(n)), (device, n)
        for name, args in (("37x53_smooth_q95_420_opt", {"image_type": "JPEG"}), ("33x65_gray_q60", None), ("131x77_420_rst5", b"\x08\x01")):
            (f,) = _run_decoder(device, [name], 1, args)
            assert np.array_equal(f, _img(name)), (device, name)


def test_image_decoder_feeds_histogram():
    from scannertools_amd.engine import CacheMode, Client, DeviceType, NamedStream, NamedVideoStream, PerfParams
    names = BATCH[:6]
    sc = Client()
    sc.ingest_rows("jpgs", [_jpg(n) for n in names])
    sc.ingest_frames("golden", np.stack([_img(n) for n in names]))
    frame = sc.ops.ImageDecoder(img=sc.io.Input([NamedStream(sc, "jpgs")]), device=DeviceType.GPU, batch=4)
    a, b = NamedStream(sc, "hist_decoded"), NamedStream(sc, "hist_golden")
    sc.run([sc.io.Output(sc.ops.Histogram(frame=frame, device=DeviceType.GPU, batch=4), [a]),
            sc.io.Output(sc.ops.Histogram(frame=sc.io.Input([NamedVideoStream(sc, "golden")]), device=DeviceType.GPU, batch=4), [b])],
           PerfParams.estimate(), cache_mode=CacheMode.Overwrite)
    got, want = list(a.load()), list(b.load())
    assert len(got) == 6
    for i, n in enumerate(names):
        assert np.array_equal(np.stack(got[i]), np.stack(want[i])), n
        ref = np.stack([np.bincount(_img(n)[..., c].reshape(-1) >> 4, minlength=16) for c in range(3)])
        assert np.array_equal(np.stack(got[i]), ref), n


def test_png_and_any_fail_validation():
    from scannertools_amd.engine import DeviceType
    for device in (DeviceType.GPU, DeviceType.CPU):
        for image_type in ("PNG", "ANY"):
            with pytest.raises(RuntimeError, match="image_type %s is not supported" % image_type):
                _run_decoder(device, BATCH[:2], 2, {"image_type": image_type})
        with pytest.raises(RuntimeError, match="could not parse ImageDecoderArgs"):
            _run_decoder(device, BATCH[:2], 2, b"\x08")


def test_shape_change_inside_a_batch_is_reported():
    from scannertools_amd.engine import DeviceType
    for device in (DeviceType.GPU, DeviceType.CPU):
        with pytest.raises(ValueError, match="row 2 changes shape inside a batch"):
            _run_decoder(device, BATCH[:2] + ["48x24_vec_420"] + BATCH[2:4], 8)
        with pytest.raises(ValueError, match="row 1: progressive"):
            _run_decoder(device, BATCH[:1] + ["progressive"], 8)
