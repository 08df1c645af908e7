"""GPU: st_png_decode_batch (HipContext.decode_png) and the ImageDecoder kernel classes with png = DECODE.  Frames must be
EQUAL -- PNG is lossless -- to the frames the pixel arrays give under the layout table (tests/png_cases.py) and to the CPU
twin's (st_png_decode_host)."""
import ctypes
import os

import numpy as np
import pytest

import png_cases as pc
from util import env_threads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = 1, 4


def _four_channel_streams(n, h=33, w=29, seed=1):
    """n streams of four colour types that all decode to (h, w, 4): RGBA, gray + alpha, palette + tRNS, RGB + colour key."""
    rng = np.random.default_rng(seed)
    streams, frames = [], []
    for i in range(n):
        filters = rng.integers(0, 5, h)
        kind = i % 4
        if kind == 0:
            px, kw = pc.picture(rng, h, w, 6), dict(ct=6)
        elif kind == 1:
            px, kw = pc.picture(rng, h, w, 4), dict(ct=4)
        elif kind == 2:
            px, kw = pc.picture(rng, h, w, 3, 4), dict(ct=3, depth=4, palette=rng.integers(0, 256, (13, 3)), trns=bytes(rng.integers(0, 256, 7).astype(np.uint8)))
        else:
            px, kw = rng.choice([5, 250], (h, w, 3)), dict(ct=2, trns=bytes([0, 5, 0, 250, 0, 5]))
        ct, depth = kw.pop("ct"), kw.pop("depth", 8)
        streams.append(pc.write_png(px, ct, depth, filters=filters, level=int(rng.integers(0, 10)), **kw))
        frames.append(pc.expected(px, ct, depth, kw.get("palette"), kw.get("trns")))
    return streams, np.stack(frames)


def test_every_case_of_the_cpu_file_is_equal(hip_ctx):
    """Every geometry, filter position, filter pair, tie, packing and palette case, grouped by decoded shape so that streams
    of different colour types and depths share calls; against the expected frames and against the CPU twin."""
    from scannertools_amd import hip
    groups = {}
    for name, (stream, want) in pc.cases().items():
        groups.setdefault(want.shape, []).append(name)
    assert len(groups) > 60
    for shape, names in groups.items():
        got = hip_ctx.decode_png([pc.cases()[n][0] for n in names]).cpu().numpy()
        assert got.shape == (len(names),) + shape
        for k, n in enumerate(names):
            assert np.array_equal(got[k], pc.cases()[n][1]), (n, int((got[k] != pc.cases()[n][1]).sum()))
            assert np.array_equal(got[k], hip.png_decode_host(pc.cases()[n][0])), n
    for name in ("geom_129x131_bpp3", "geom_65x1_bpp1", "pairs_bpp4", "bits_pal_d1_w9"):    # and alone
        assert np.array_equal(hip_ctx.decode_png([pc.cases()[name][0]]).cpu().numpy()[0], pc.cases()[name][1]), name


def test_pillows_golden_streams_are_equal(hip_ctx):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "png_golden.npz"))
    for name in [str(c) for c in gold["cases"]]:
        got = hip_ctx.decode_png([gold[name + "__png"].tobytes()]).cpu().numpy()[0]
        assert got.shape == gold[name + "__img"].shape and np.array_equal(got, gold[name + "__img"]), name


@pytest.mark.parametrize("n", [1, 17, 70])
def test_calls_of_1_17_and_70_mixed_streams(hip_ctx, n):
    """17 exceeds the default thread count: two sub-batches; 70: five, both page-locked slots refilled."""
    from scannertools_amd import _native
    streams, want = _four_channel_streams(n, seed=n)
    hip_ctx.timing_enable(list(range(_native.K_COUNT)))
    hip_ctx.timing_reset()
    with env_threads("ST_PNG_THREADS", 16):                                  # the default, whatever this machine has
        got = hip_ctx.decode_png(streams).cpu().numpy()
    counts = [hip_ctx.timing_read(k)[0] for k in range(_native.K_COUNT)]
    hip_ctx.timing_enable([])
    assert np.array_equal(got, want), [k for k in range(n) if not np.array_equal(got[k], want[k])]
    # per sub-batch of 16 an unfilter launch, and an expansion launch where one of its frames needs it (every kind but RGBA, i % 4 == 0)
    launches = sum(1 + any(i % 4 for i in range(s, min(s + 16, n))) for s in range(0, n, 16))
    assert launches == {1: 1, 17: 3, 70: 10}[n]
    assert counts[_native.K_JPEG] == launches and sum(counts) == launches, counts


def test_output_frames_at_odd_addresses(hip_ctx):
    import torch
    rng = np.random.default_rng(2)
    px = pc.picture(rng, 70, 37, 2)
    direct = [pc.write_png(px, 2, filters=rng.integers(0, 5, 70))] * 3          # written by the unfilter kernel itself
    expanded, want4 = _four_channel_streams(3, 70, 37, seed=3)                   # written by the expansion kernel
    for streams, want in ((direct, np.stack([px.astype(np.uint8)] * 3)), (expanded, want4)):
        nbytes = want.size
        for off in (1, 2, 3, 5, 16):
            flat = torch.full((nbytes + 64,), 0xCD, dtype=torch.uint8, device="cuda")
            out = flat[off:off + nbytes].view(want.shape)
            assert out.data_ptr() % 16 == off % 16
            hip_ctx.decode_png(streams, out=out)
            host = flat.cpu().numpy()
            assert np.array_equal(host[off:off + nbytes].reshape(want.shape), want), off
            assert (host[:off] == 0xCD).all() and (host[off + nbytes:] == 0xCD).all(), off     # not a byte outside the frames


def test_a_65_row_frame_of_20000_rgba_pixels(hip_ctx):
    """The kernel has no row-length threshold; this is the widest row the issue names: 80 000 bytes, 5000 pieces per row, a
    second band of one row whose upper row is carried from the first."""
    rng = np.random.default_rng(4)
    px = (rng.integers(0, 256, (65, 20000, 4)) & 0xF8).astype(np.uint8)
    got = hip_ctx.decode_png([pc.write_png(px, 6, filters=[4, 3, 1, 2, 0] * 13, level=1)]).cpu().numpy()[0]
    assert np.array_equal(got, px), int((got != px).sum())


def test_a_1080p_rgb_frame(hip_ctx):
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:1080, 0:1920]
    px = (((x + 2 * y)[..., None] // np.array([3, 5, 7]) + rng.integers(0, 8, (1080, 1920, 3))) & 255).astype(np.uint8)
    got = hip_ctx.decode_png([pc.write_png(px, 2, filters=rng.integers(0, 5, 1080), level=1)]).cpu().numpy()[0]
    assert np.array_equal(got, px), int((got != px).sum())


def test_refusals_leave_the_outputs_unwritten_and_launch_nothing(hip_ctx):
    import torch
    from scannertools_amd import _native
    from scannertools_amd.hip import StError
    good = [pc.small_valid(), pc.small_valid(level=0)]                       # 6 x 9 x 3, the shape of the malformed streams' IHDR
    rgba = pc.write_png(pc.picture(np.random.default_rng(7), 6, 9, 6), 6)
    wide = pc.write_png(pc.picture(np.random.default_rng(7), 6, 10, 2), 2)
    hip_ctx.timing_enable(list(range(_native.K_COUNT)))
    hip_ctx.timing_reset()
    out = torch.full((3, 6, 9, 3), 0xCD, dtype=torch.uint8, device="cuda")
    for name, stream, status, piece in pc.malformed():
        with pytest.raises(StError) as e:
            hip_ctx.decode_png(good + [stream], out=out)
        assert e.value.status == status and "png: stream 2: " in str(e.value) and piece in str(e.value), (name, str(e.value))
    for stream, piece in ((rgba, "stream 1 is 9x6 with 4 channel(s), the call decodes 9x6 with 3"), (wide, "stream 1 is 10x6 with 3 channel(s)")):
        with pytest.raises(StError) as e:
            hip_ctx.decode_png([good[0], stream, good[1]], out=out)
        assert e.value.status == INVALID and piece in str(e.value)
    # (corrupt data shows only while inflating: a call of one sub-batch then writes and launches nothing either)
    assert sum(hip_ctx.timing_read(k)[0] for k in range(_native.K_COUNT)) == 0
    assert (out.cpu().numpy() == 0xCD).all()
    hip_ctx.decode_png(good + [good[0]], out=out)
    assert hip_ctx.timing_read(_native.K_JPEG)[0] == 1                        # the context still works: one unfilter launch
    assert np.array_equal(out.cpu().numpy()[2], hip_ctx.decode_png(good[:1]).cpu().numpy()[0])
    hip_ctx.timing_enable([])


def test_corrupt_data_in_a_later_sub_batch_fails_the_call_and_names_the_stream(hip_ctx):
    from scannertools_amd.hip import StError
    streams, _ = _four_channel_streams(40, 12, 11, seed=8)
    rng = np.random.default_rng(9)
    px = pc.picture(rng, 12, 11, 6)
    raw = pc.filter_rows(pc.scanlines(px, 6, 8), 4, [1] * 12)
    z = pc.deflate(raw.tobytes())
    streams[37] = pc.write_png(px, 6, zdata=z[:-1] + bytes([z[-1] ^ 1]))
    with pytest.raises(StError, match="png: stream 37: png: zlib: Adler-32 mismatch"):
        hip_ctx.decode_png(streams)


# ---- the kernel classes through the stand-in engine -----------------------------------------------------------------------------------
def _run_decoder(device, rows, batch, args):
    from scannertools_amd.engine import CacheMode, Client, NamedStream, PerfParams
    sc = Client()
    sc.ingest_rows("imgs", rows)
    img = sc.io.Input([NamedStream(sc, "imgs")])
    out = NamedStream(sc, "frames")
    sc.run(sc.io.Output(sc.ops.ImageDecoder(img=img, device=device, batch=batch, args=args), [out]), PerfParams.estimate(),
           cache_mode=CacheMode.Overwrite)
    return list(out.load())


def _devices():
    from scannertools_amd.engine import DeviceType
    return (DeviceType.GPU, DeviceType.CPU)


def test_kernel_classes_decode_png_rows_for_every_image_type():
    streams, want = _four_channel_streams(9, seed=10)
    for device in _devices():
        for args in ({"png": "DECODE", "image_type": "PNG"}, {"png": "DECODE", "image_type": "ANY"}, {"png": "DECODE"}, b"\x28\x01"):
            frames = _run_decoder(device, streams, 4, args)                  # executes of 4, 4 and 1 rows
            assert len(frames) == 9
            for k, f in enumerate(frames):
                f = np.asarray(f.cpu() if hasattr(f, "cpu") else f)
                assert f.dtype == np.uint8 and f.shape == (33, 29, 4) and np.array_equal(f, want[k]), (device, args, k)


def test_kernel_classes_mix_jpeg_and_png_rows_in_one_execute(hip_ctx):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_golden.npz"))
    batch = [str(c) for c in gold["batch"]][:4]
    jpgs = [gold[n + "__jpg"].tobytes() for n in batch]
    own = hip_ctx.decode_jpeg(jpgs).cpu().numpy()                             # the JPEG library's own frames (= Pillow's golden ones)
    assert all(np.array_equal(own[k], gold[n + "__img"]) for k, n in enumerate(batch))
    h, w, c = own.shape[1:]
    assert c == 3
    rng = np.random.default_rng(11)
    pxs = [pc.picture(rng, h, w, 2) for _ in range(3)]
    pal = rng.integers(0, 256, (16, 3))
    idx = pc.picture(rng, h, w, 3, 4)
    pngs = [pc.write_png(p, 2, filters=rng.integers(0, 5, h)) for p in pxs] + [pc.write_png(idx, 3, 4, palette=pal, filters=2)]
    png_want = [p.astype(np.uint8) for p in pxs] + [pc.expected(idx, 3, 4, pal)]
    rows = [jpgs[0], pngs[0], pngs[1], jpgs[1], jpgs[2], pngs[2], pngs[3], jpgs[3]]
    want = [own[0], png_want[0], png_want[1], own[1], own[2], png_want[2], png_want[3], own[3]]
    for device in _devices():
        for args in ({"png": "DECODE"}, {"png": "DECODE", "image_type": "ANY", "entropy": "auto"}, {"png": "DECODE", "entropy": "gpu", "split": "subsequence"}):
            frames = _run_decoder(device, rows, 8, args)                      # ONE execute() with both kinds of row
            for k, f in enumerate(frames):
                f = np.asarray(f.cpu() if hasattr(f, "cpu") else f)
                assert np.array_equal(f, want[k]), (device, args, k)
        # JPEG rows alone still go the JPEG way, scaled too
        frames = _run_decoder(device, jpgs, 4, {"png": "DECODE", "scale_denom": 2})
        half = hip_ctx.decode_jpeg(jpgs, scale=2).cpu().numpy()
        for k, f in enumerate(frames):
            assert np.array_equal(np.asarray(f.cpu() if hasattr(f, "cpu") else f), half[k])


def test_kernel_classes_fatal_cases_and_validation():
    gold = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_golden.npz"))
    batch = [str(c) for c in gold["batch"]][:2]
    jpgs = [gold[n + "__jpg"].tobytes() for n in batch]
    h, w = gold[batch[0] + "__img"].shape[:2]
    rng = np.random.default_rng(12)
    png = pc.write_png(pc.picture(rng, h, w, 2), 2)
    other = pc.write_png(pc.picture(rng, h, w + 1, 2), 2)
    rgba = pc.write_png(pc.picture(rng, h, w, 6), 6)
    sixteen = next(m[1] for m in pc.malformed() if m[0] == "sixteen_bit")
    for device in _devices():
        with pytest.raises(ValueError, match="row 1: png: not a PNG stream"):          # image_type PNG: a JPEG row is fatal
            _run_decoder(device, [png, jpgs[0]], 2, {"png": "DECODE", "image_type": "PNG"})
        with pytest.raises(ValueError, match="row 0: "):                                # image_type JPEG: a PNG row is no JPEG
            _run_decoder(device, [png, jpgs[0]], 2, {"png": "DECODE", "image_type": "JPEG"})
        with pytest.raises(ValueError, match="row 1: a PNG row cannot be decoded at scale_denom 2"):
            _run_decoder(device, [jpgs[0], png], 2, {"png": "DECODE", "scale_denom": 2})
        with pytest.raises(ValueError, match="row 1: png: 16-bit samples are not supported"):
            _run_decoder(device, [png, sixteen], 2, {"png": "DECODE"})
        with pytest.raises(ValueError, match="row 2 changes shape inside a batch"):
            _run_decoder(device, [png, jpgs[0], other], 4, {"png": "DECODE"})
        with pytest.raises(ValueError, match="row 1 changes shape inside a batch"):
            _run_decoder(device, [png, rgba], 4, {"png": "DECODE"})
        with pytest.raises(RuntimeError, match="invalid png 2"):
            _run_decoder(device, jpgs[:1], 1, b"\x28\x02")
        # without the field nothing changes: PNG / ANY fail validate(), a PNG row is not a JPEG
        for image_type in ("PNG", "ANY"):
            with pytest.raises(RuntimeError, match="image_type %s is not supported" % image_type):
                _run_decoder(device, jpgs, 2, {"image_type": image_type})
            with pytest.raises(RuntimeError, match="image_type %s is not supported" % image_type):
                _run_decoder(device, jpgs, 2, {"image_type": image_type, "png": "REFUSE"})
        with pytest.raises(ValueError, match="row 0: "):
            _run_decoder(device, [png], 1, None)
