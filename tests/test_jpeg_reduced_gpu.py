"""GPU: ImageDecoder at scale 1/2, 1/4 and 1/8 (st_jpeg_decode_batch_scaled, decode_jpeg(scale=), ImageDecoderArgs.scale_denom)
against Pillow's golden frames, byte for byte, on all three entropy paths.  Reads tests/golden/jpeg_reduced_golden.npz only;
the frames of its "restatement_only" list (a side shorter than the denominator: 1 x 1, 7 x 9 at 1/8, 40 x 3 and 3 x 40 at
1/4 and 1/8) are tests/ref_jpeg_reduced_np.py's, which Pillow cannot be asked for.
Not covered: a reduced frame above 2 097 152 pixels, where the colour kernel's grid strides (it needs a 16-megapixel source)."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from util import env_threads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_reduced_golden.npz"))
CASES = [(str(c).rsplit("/", 1)[0], int(str(c).rsplit("/", 1)[1])) for c in list(GOLD["cases"]) + list(GOLD["restatement_only"])]
SUBPIXEL = [(n, d) for n, d in CASES if n.startswith(("1x1_", "7x9_"))]
STREAMS = sorted({n for n, _ in CASES})


def _jpg(name):
    return GOLD[name + "__jpg"].tobytes()


def _stream(prefix):
    """The one stream whose name starts with `prefix` (a name may end in _rst)."""
    (name,) = [n for n in STREAMS if n == prefix or n == prefix + "_rst"]
    return name


def _same(name, d, got):
    key = "%s__d%d" % (name, d)
    if key in GOLD.files:
        return got.shape == GOLD[key].shape and np.array_equal(got, GOLD[key])
    return got.shape == tuple(GOLD[key + "_shape"]) and hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == str(GOLD[key + "_sha"])


@pytest.mark.parametrize("mode", ["host", "gpu", "subsequence"])
def test_every_golden_case_is_byte_exact(hip_ctx, mode):
    """Every sampling x denominator at 8 x 8 .. 128 x 256: partial MCUs, reduced widths that take the 16-, 4- and 1-pixel
    lanes, replication at 4:2:2 (40 x 3, 3 x 40, and everything at 1/8), DC-only columns (quality 30).  "gpu": the streams
    with restart intervals, one lane per interval; "subsequence": every stream."""
    kw = {"host": dict(), "gpu": dict(entropy="gpu"), "subsequence": dict(entropy="gpu", split="subsequence")}[mode]
    ran = 0
    for name, d in CASES:
        if mode == "gpu" and not name.endswith("_rst"):
            continue
        got = hip_ctx.decode_jpeg([_jpg(name)], scale=d, **kw).cpu().numpy()
        assert got.shape[0] == 1 and _same(name, d, got[0]), (mode, name, d)
        ran += 1
    assert ran == (len(CASES) if mode != "gpu" else sum(n.endswith("_rst") for n, _ in CASES)) and ran >= 90


def test_subpixel_frames(hip_ctx):
    """1 x 1 at every denominator and 7 x 9 at 1/8: one output pixel or row from a partial block.  The restatement is the only
    reference for these."""
    assert {(n.split("_")[0], d) for n, d in SUBPIXEL} >= {("1x1", 2), ("1x1", 4), ("1x1", 8), ("7x9", 8)}
    for name, d in SUBPIXEL:
        for kw in (dict(), dict(entropy="auto", split="subsequence")):
            got = hip_ctx.decode_jpeg([_jpg(name)], scale=d, **kw).cpu().numpy()
            assert _same(name, d, got[0]), (name, d, kw)


def test_mixed_subsampling_in_one_call(hip_ctx):
    """4:4:4, 4:2:2 and 4:2:0 of one shape in one call: at 1/8 the luma and the 4:4:4 / 4:2:2 chroma are 1 x 1 blocks while
    the 4:2:0 chroma is 2 x 2, so both inverse DCT kernels run over one sub-batch."""
    names = [_stream("37x53_%s_q%d" % (s, q)) for s, q in (("420", 95), ("444", 30), ("422", 95), ("420", 30), ("444", 95))]
    for d in (2, 4, 8):
        for threads in (16, 2):
            with env_threads("ST_JPEG_THREADS", threads):
                got = hip_ctx.decode_jpeg([_jpg(n) for n in names], scale=d).cpu().numpy()
            for i, n in enumerate(names):
                assert _same(n, d, got[i]), (d, threads, n)
        got = hip_ctx.decode_jpeg([_jpg(n) for n in names], scale=d, entropy="gpu", split="subsequence").cpu().numpy()
        assert all(_same(n, d, got[i]) for i, n in enumerate(names)), d


def test_seventy_tiny_frames(hip_ctx):
    """70 frames of 8 x 8 and of 17 x 33: blockIdx.y runs over the frames of a launch; one thread makes 70 sub-batches of one
    frame each through the two alternating slots, three make 24."""
    for size in ("8x8", "17x33"):
        pool = [n for n in STREAMS if n.startswith(size + "_") and "_gray_" not in n]
        names = [pool[i % len(pool)] for i in range(70)]
        for d in (2, 8):
            for threads in (16, 1, 3):
                with env_threads("ST_JPEG_THREADS", threads):
                    got = hip_ctx.decode_jpeg([_jpg(n) for n in names], scale=d).cpu().numpy()
                assert all(_same(n, d, got[i]) for i, n in enumerate(names)), (size, d, threads)
            got = hip_ctx.decode_jpeg([_jpg(n) for n in names], scale=d, entropy="auto", split="subsequence").cpu().numpy()
            assert all(_same(n, d, got[i]) for i, n in enumerate(names)), (size, d)


def test_store_width_does_not_change_a_byte(hip_ctx):
    """Frames that start on a 16-byte boundary, on a 4-byte one and on an odd byte: reduced widths of 64, 32 and 16 pixels
    would take the 16-pixel lanes, and take the 4- and 1-pixel ones instead.  Nothing is written outside the frame."""
    import torch
    for name in (_stream("128x256_420_q95"), _stream("128x256_422_q30"), _stream("64x128_444_q95"), _stream("128x256_gray_q30")):
        for d in (2, 4, 8):
            want = hip_ctx.decode_jpeg([_jpg(name)], scale=d).cpu().numpy()[0]
            assert _same(name, d, want) and want.shape[1] % 4 == 0, (name, d)
            nbytes = want.size
            for offset in (0, 4, 1):
                buf = torch.full((nbytes + 64,), 0x5A, dtype=torch.uint8, device=hip_ctx.device)
                out = buf[offset:offset + nbytes].view((1,) + want.shape)
                hip_ctx.decode_jpeg([_jpg(name)], out=out, scale=d)
                host = buf.cpu().numpy()
                assert np.array_equal(host[offset:offset + nbytes].reshape(want.shape), want), (name, d, offset)
                assert (host[:offset] == 0x5A).all() and (host[offset + nbytes:] == 0x5A).all(), (name, d, offset)


def test_scale_one_is_the_call_without_the_argument(hip_ctx):
    for name in (_stream("100x131_420_q95"), _stream("37x53_422_q30"), _stream("64x128_gray_q95"), _stream("17x33_444_q30")):
        for kw in (dict(), dict(entropy="auto"), dict(entropy="gpu", split="subsequence")):
            a = hip_ctx.decode_jpeg([_jpg(name)], **kw).cpu().numpy()
            b = hip_ctx.decode_jpeg([_jpg(name)], scale=1, **kw).cpu().numpy()
            assert a.shape == b.shape and np.array_equal(a, b), (name, kw)


def test_bad_denominator_and_entropy_are_refused_before_anything_is_written(hip_ctx):
    import torch
    from scannertools_amd import _native
    L, hh, vp = _native.lib(), hip_ctx._h, ctypes.c_void_p
    hip_ctx._bind()
    name = _stream("16x16_420_q95")
    jpg = _jpg(name)
    keep = ctypes.create_string_buffer(jpg, len(jpg))
    bufs, sizes = (vp * 1)(ctypes.addressof(keep)), (ctypes.c_size_t * 1)(len(jpg))
    out = torch.full((1, 16, 16, 3), 0xA5, dtype=torch.uint8, device=hip_ctx.device)
    to = (vp * 1)(out.data_ptr())
    for d in (0, 3, 16, -4):
        assert L.st_jpeg_decode_batch_scaled(hh, bufs, sizes, 1, 16, 16, 3, d, 0, None, to) == _native.ST_ERR_INVALID
        assert (b"scale_denom %d" % d) in L.st_ctx_last_error(hh)
    for e in (3, -1):
        assert L.st_jpeg_decode_batch_scaled(hh, bufs, sizes, 1, 16, 16, 3, 2, e, None, to) == _native.ST_ERR_INVALID
        assert (b"entropy %d" % e) in L.st_ctx_last_error(hh)
    # the refusals of the call it stands for: another shape, and at the interval path a stream without restart intervals
    assert L.st_jpeg_decode_batch_scaled(hh, bufs, sizes, 1, 16, 32, 3, 2, 0, None, to) == _native.ST_ERR_INVALID
    assert b"stream 0 is 16x16" in L.st_ctx_last_error(hh)
    if not name.endswith("_rst"):
        assert L.st_jpeg_decode_batch_scaled(hh, bufs, sizes, 1, 16, 16, 3, 2, 1, None, to) == _native.ST_ERR_UNSUPPORTED
        assert b"no restart intervals" in L.st_ctx_last_error(hh)
    hip_ctx.sync()
    assert (out.cpu().numpy() == 0xA5).all()
    # with denominator 1 it is the call it stands for; with 2 it writes the first 8 x 8 x 3 bytes only
    assert L.st_jpeg_decode_batch_scaled(hh, bufs, sizes, 1, 16, 16, 3, 1, 0, None, to) == _native.ST_OK
    hip_ctx.sync()
    assert np.array_equal(out.cpu().numpy(), hip_ctx.decode_jpeg([jpg]).cpu().numpy())
    out.fill_(0xA5)
    assert L.st_jpeg_decode_batch_scaled(hh, bufs, sizes, 1, 16, 16, 3, 2, 2, None, to) == _native.ST_OK
    hip_ctx.sync()
    host = out.cpu().numpy().reshape(-1)
    assert _same(name, 2, host[:192].reshape(8, 8, 3)) and (host[192:] == 0xA5).all()


def _run_decoder(device, names, batch, args):
    from scannertools_amd.engine import CacheMode, Client, NamedStream, PerfParams
    sc = Client()
    sc.ingest_rows("jpgs", [_jpg(n) for n in names])
    img = sc.io.Input([NamedStream(sc, "jpgs")])
    out = NamedStream(sc, "frames")
    sc.run(sc.io.Output(sc.ops.ImageDecoder(img=img, device=device, batch=batch, args=args), [out]), PerfParams.estimate(),
           cache_mode=CacheMode.Overwrite)
    return list(out.load())


def test_kernel_classes_write_the_reduced_frames():
    """ImageDecoderArgs.scale_denom through both registrations: the output frame's FrameInfo carries the reduced shape."""
    from scannertools_amd.engine import DeviceType
    pool = [n for n in STREAMS if n.startswith("37x53_") and "_gray_" not in n]
    rst = [n for n in pool if n.endswith("_rst")]
    for device in (DeviceType.GPU, DeviceType.CPU):
        for d in (2, 8):
            frames = _run_decoder(device, pool, 4, {"scale_denom": d})                 # executes of 4 and 2 rows
            assert len(frames) == len(pool) == 6
            for n, f in zip(pool, frames):
                assert f.dtype == np.uint8 and f.shape == (-(-53 // d), -(-37 // d), 3) and _same(n, d, f), (device, d, n)
            for args in ({"scale_denom": d, "entropy": "auto", "split": "subsequence"}, bytes([0x10, 0x02, 0x20, d])):
                frames = _run_decoder(device, pool, 8, args)
                assert all(_same(n, d, f) for n, f in zip(pool, frames)), (device, d, args)
            frames = _run_decoder(device, rst, 8, {"scale_denom": d, "entropy": "gpu"})
            assert len(rst) >= 2 and all(_same(n, d, f) for n, f in zip(rst, frames)), (device, d)
        gray = _stream("100x131_gray_q95")
        (f,) = _run_decoder(device, [gray], 1, {"image_type": "JPEG", "scale_denom": 4})
        assert f.shape == (33, 25, 1) and _same(gray, 4, f), device
        # 0 and 1 are full size; anything else fails validate()
        (a,), (b,), (c,) = (_run_decoder(device, [gray], 1, args) for args in (None, {"scale_denom": 1}, b"\x20\x00"))
        assert a.shape == (131, 100, 1) and np.array_equal(a, b) and np.array_equal(a, c)
        for bad in (3, 16, -2):
            with pytest.raises(RuntimeError, match="invalid scale_denom %d" % bad):
                _run_decoder(device, [gray], 1, {"scale_denom": bad})
