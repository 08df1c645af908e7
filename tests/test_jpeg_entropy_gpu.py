"""GPU: st_jpeg_decode_batch_gpu (k_jpeg_entropy_dec: the Huffman decoder on the device, one lane per restart interval) and the
ImageDecoder kernel classes with ImageDecoderArgs.entropy, against Pillow's golden frames and the numpy definition
(tests/ref_jpeg_np.py): byte for byte.  Reads tests/golden/jpeg_restart_golden.npz, jpeg_golden.npz and jpeg_encode_golden.npz."""
import ctypes
import json
import os

import numpy as np
import pytest

import ref_jpeg_np as ref
from util import env_threads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_golden.npz"))
ENC = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_encode_golden.npz"))
RST = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_restart_golden.npz"))
RST_CASES = [str(c) for c in RST["cases"]]
GOOD = [str(c) for c in RST["good"]]
MIXED = [str(c) for c in RST["mixed"]]
CORRUPT = [str(c) for c in RST["corrupt"]]
ENC_BATCH = [str(c) for c in ENC["batch"]]
TINY = ["8x8_noise_q100_420_rst3", "8x8_smooth_q100_420_rst3", "8x8_noise_q90_422_rstrow", "8x8_smooth_q90_422_rstrow"]   # of jpeg_golden.npz


def _rjpg(name):
    return RST[name + "__jpg"].tobytes()


def _rimg(name):
    key = name + "__img"
    return RST[key] if key in RST.files else RST[str(RST[name + "__same_as"]) + "__img"]


def _has_dri(jpg):
    sos = jpg.index(b"\xff\xda")
    return jpg.find(b"\xff\xdd\x00\x04", 0, sos) >= 0


GOLD_DRI = [str(c) for c in GOLD["cases"] if _has_dri(GOLD[str(c) + "__jpg"].tobytes())]


def test_new_golden_cases_are_byte_exact_and_one_bracket_each(hip_ctx):
    """262 intervals over five workgroups with RSTn wrapping 32 times, per-frame optimised tables, a one-component scan,
    intervals that span MCU rows with a short last one, 130 row intervals, fill bytes in front of markers."""
    from scannertools_amd import _native
    hip_ctx.timing_enable([_native.K_JPEG])
    hip_ctx.timing_reset()
    for name in RST_CASES:
        got = hip_ctx.decode_jpeg([_rjpg(name)], entropy="gpu").cpu().numpy()
        want = _rimg(name)
        assert got.shape == (1,) + want.shape, name
        assert np.array_equal(got[0], want), (name, int((got[0] != want).sum()))
    launches, _ = hip_ctx.timing_read(_native.K_JPEG)
    assert launches == len(RST_CASES)          # one bracket (entropy + IDCT + colour launch) per sub-batch
    hip_ctx.timing_enable([])


def test_every_dri_case_of_the_decoder_golden_file(hip_ctx):
    assert len(GOLD_DRI) == 42
    for name in GOLD_DRI:
        got = hip_ctx.decode_jpeg([GOLD[name + "__jpg"].tobytes()], entropy="gpu").cpu().numpy()
        want = GOLD[name + "__img"]
        assert got.shape == (1,) + want.shape and np.array_equal(got[0], want), name


def test_encoder_streams_equal_the_definition(hip_ctx):
    """Every stream of jpeg_encode_golden.npz (one restart interval per MCU row), the streams of one shape in one call."""
    names = [k[:-5] for k in ENC.files if k.endswith("__jpg")]
    assert len(names) == 167
    want = {n: ref.decode(ENC[n + "__jpg"].tobytes()) for n in names}
    by_shape = {}
    for n in names:
        by_shape.setdefault(want[n].shape, []).append(n)
    for shape, group in by_shape.items():
        got = hip_ctx.decode_jpeg([ENC[n + "__jpg"].tobytes() for n in group], entropy="gpu").cpu().numpy()
        for i, n in enumerate(group):
            assert np.array_equal(got[i], want[n]), (n, shape)


def test_batches_equal_singles(hip_ctx):
    streams = [ENC[n + "__jpg"].tobytes() for n in ENC_BATCH]
    singles = [hip_ctx.decode_jpeg([s], entropy="gpu").cpu().numpy()[0] for s in streams]
    for n, got in zip(ENC_BATCH, singles):
        assert np.array_equal(got, ENC[n + "__dec"]), n
    for count in (1, 8, 33):
        for threads in (16, 3):
            with env_threads("ST_JPEG_THREADS", threads):
                got = hip_ctx.decode_jpeg(streams[:count], entropy="gpu").cpu().numpy()
            assert np.array_equal(got, np.stack(singles[:count])), (count, threads)


def test_mixed_sampling_and_mixed_tables_in_one_call(hip_ctx):
    got = hip_ctx.decode_jpeg([GOLD[n + "__jpg"].tobytes() for n in TINY], entropy="gpu").cpu().numpy()      # 4:2:0 and 4:2:2
    for i, n in enumerate(TINY):
        assert np.array_equal(got[i], GOLD[n + "__img"]), n
    names = [MIXED[0], GOOD[0], MIXED[1], MIXED[1], MIXED[0], GOOD[1], MIXED[1]]         # standard and optimised tables alternate
    for threads in (16, 2):
        with env_threads("ST_JPEG_THREADS", threads):
            got = hip_ctx.decode_jpeg([_rjpg(n) for n in names], entropy="gpu").cpu().numpy()
        for i, n in enumerate(names):
            assert np.array_equal(got[i], _rimg(n)), (threads, i, n)


def test_store_width_does_not_change_a_byte(hip_ctx):
    """Frames that start on a 16-byte boundary, on a 4-byte one and on an odd byte; the bytes around them stay."""
    import torch
    for name in ("32x24_mixed_std", "131x61_420_rst5", "40x24_gray_rst2", "16x1040_422_rstrow_fill"):
        want = _rimg(name)
        nbytes = want.size
        for offset in (0, 4, 1):
            buf = torch.full((nbytes + 64,), 0x5A, dtype=torch.uint8, device=hip_ctx.device)
            out = buf[offset:offset + nbytes].view((1,) + want.shape)
            hip_ctx.decode_jpeg([_rjpg(name)], out=out, entropy="gpu")
            host = buf.cpu().numpy()
            assert np.array_equal(host[offset:offset + nbytes].reshape(want.shape), want), (name, offset)
            assert (host[:offset] == 0x5A).all() and (host[offset + nbytes:] == 0x5A).all(), (name, offset)


def test_one_launch_past_a_grid_dimension(hip_ctx):
    """65 537 streams in one call: one entropy launch with the frames on grid.x, 65 537 workgroups wide (its stride over the
    frames is NOT taken: the launch caps grid.x at 2^20 frames), the dense kernels, frames on grid.y, in two launches.  The stride
    over a frame's groups of intervals (grid.y) is what tests/test_jpeg_large_gpu.py reaches."""
    n = 65537
    streams = [GOLD[t + "__jpg"].tobytes() for t in TINY]
    frames = np.stack([GOLD[t + "__img"] for t in TINY])
    got = hip_ctx.decode_jpeg([streams[i & 3] for i in range(n)], entropy="gpu").cpu().numpy()
    assert got.shape == (n, 8, 8, 3)
    assert np.array_equal(got[:65536].reshape(16384, 4, 8, 8, 3), np.broadcast_to(frames, (16384, 4, 8, 8, 3)))
    assert np.array_equal(got[65536], frames[0])


def test_auto_falls_back_to_the_host_and_gpu_names_the_stream(hip_ctx):
    import torch
    from scannertools_amd import _native
    from scannertools_amd.hip import StError
    streams = [_rjpg(GOOD[0]), _rjpg(GOOD[1]), GOLD["32x24_batch00__jpg"].tobytes(), _rjpg(GOOD[2])]       # stream 2 has no DRI
    host = hip_ctx.decode_jpeg(streams).cpu().numpy()
    assert np.array_equal(hip_ctx.decode_jpeg(streams, entropy="auto").cpu().numpy(), host)
    assert np.array_equal(host[2], GOLD["32x24_batch00__img"]) and np.array_equal(host[3], _rimg(GOOD[2]))
    out = torch.full((4, 24, 32, 3), 0xA5, dtype=torch.uint8, device=hip_ctx.device)
    with pytest.raises(StError, match="stream 2: no restart intervals") as e:
        hip_ctx.decode_jpeg(streams, out=out, entropy="gpu")
    assert e.value.status == _native.ST_ERR_UNSUPPORTED
    hip_ctx.sync()
    assert (out.cpu().numpy() == 0xA5).all()
    # with restart intervals everywhere "auto" is the device path: same frames
    good = [_rjpg(n) for n in GOOD]
    assert np.array_equal(hip_ctx.decode_jpeg(good, entropy="auto").cpu().numpy(), np.stack([_rimg(n) for n in GOOD]))
    with pytest.raises(ValueError, match="entropy must be one of"):
        hip_ctx.decode_jpeg(good, entropy="device")


def test_corrupt_interval_fails_the_call_and_writes_nothing(hip_ctx):
    """The stored corrupt variants (every marker present, the second half of one interval's bytes gone) between four good
    streams.  tests/test_jpeg_entropy.py runs the same bytes through the same core under the sanitizers first: the kernel
    stops at the end of the interval's bytes and reports it."""
    import torch
    from scannertools_amd import _native
    from scannertools_amd.hip import StError
    L, hh, vp = _native.lib(), hip_ctx._h, ctypes.c_void_p
    hip_ctx._bind()
    good = [_rjpg(n) for n in GOOD]
    for name in CORRUPT:
        k = int(RST[name + "__interval"])
        streams = good[:2] + [_rjpg(name)] + good[2:]
        n = len(streams)
        out = torch.full((n, 24, 32, 3), 0xA5, dtype=torch.uint8, device=hip_ctx.device)
        keep = [ctypes.create_string_buffer(s, len(s)) for s in streams]
        bufs = (vp * n)(*[ctypes.addressof(b) for b in keep])
        sizes = (ctypes.c_size_t * n)(*[len(s) for s in streams])
        to = (vp * n)(*[out[i].data_ptr() for i in range(n)])
        st = L.st_jpeg_decode_batch_gpu(hh, bufs, sizes, n, 24, 32, 3, to)
        msg = L.st_ctx_last_error(hh)
        assert st == _native.ST_ERR_INVALID and b"stream 2" in msg and b"restart interval %d of 4" % k in msg, (name, st, msg)
        hip_ctx.sync()
        assert (out.cpu().numpy() == 0xA5).all(), (name, msg)
        with pytest.raises(StError, match="stream 2: corrupt scan: restart interval %d" % k):
            hip_ctx.decode_jpeg(streams, entropy="gpu")
        # the context decodes the good streams afterwards
        got = hip_ctx.decode_jpeg(good, entropy="gpu").cpu().numpy()
        assert all(np.array_equal(got[i], _rimg(GOOD[i])) for i in range(4)), name
    # a truncated scan and a wrong RSTn are found by the host's interval scan: nothing is launched
    bad_rst = bytearray(good[1])
    at = good[1].index(b"\xff\xd1")
    bad_rst[at + 1] = 0xD5
    scan = good[1].index(b"\xff\xda")
    for bad, cause in ((good[1][:scan + (len(good[1]) - scan) // 2], b"truncated or corrupt scan"), (bytes(bad_rst), b"no RST1 marker")):
        streams = good[:2] + [bad] + good[2:]
        out = torch.full((5, 24, 32, 3), 0xA5, dtype=torch.uint8, device=hip_ctx.device)
        keep = [ctypes.create_string_buffer(s, len(s)) for s in streams]
        bufs = (vp * 5)(*[ctypes.addressof(b) for b in keep])
        sizes = (ctypes.c_size_t * 5)(*[len(s) for s in streams])
        to = (vp * 5)(*[out[i].data_ptr() for i in range(5)])
        st = L.st_jpeg_decode_batch_gpu(hh, bufs, sizes, 5, 24, 32, 3, to)
        msg = L.st_ctx_last_error(hh)
        assert st == _native.ST_ERR_INVALID and b"stream 2" in msg and cause in msg, (st, msg)
        hip_ctx.sync()
        assert (out.cpu().numpy() == 0xA5).all(), msg
    assert L.st_jpeg_decode_batch_gpu(hh, None, None, 0, 24, 32, 3, None) == _native.ST_OK
    assert L.st_jpeg_decode_batch_gpu(hh, None, None, 1, 24, 32, 3, None) == _native.ST_ERR_INVALID


def _run_decoder(device, streams, batch, args):
    from scannertools_amd.engine import CacheMode, Client, NamedStream, PerfParams
    sc = Client()
    sc.ingest_rows("jpgs", streams)
    img = sc.io.Input([NamedStream(sc, "jpgs")])
    out = NamedStream(sc, "frames")
    sc.run(sc.io.Output(sc.ops.ImageDecoder(img=img, device=device, batch=batch, args=args), [out]), PerfParams.estimate(),
           cache_mode=CacheMode.Overwrite)
    return list(out.load())


def test_kernel_classes_honour_the_entropy_field():
    from scannertools_amd.engine import DeviceType
    names = GOOD + MIXED
    for device in (DeviceType.GPU, DeviceType.CPU):
        for args in ({"entropy": "gpu"}, {"entropy": "auto"}, b"\x08\x01\x10\x01"):
            frames = _run_decoder(device, [_rjpg(n) for n in names], 4, args)               # executes of 4 and 2 rows
            assert len(frames) == 6
            for n, f in zip(names, frames):
                assert f.dtype == np.uint8 and np.array_equal(f, _rimg(n)), (device, args, n)
        # AUTO with a row that has no restart intervals takes the host path for that execute(); GPU refuses the row by name
        streams = [_rjpg(GOOD[0]), GOLD["32x24_batch00__jpg"].tobytes(), _rjpg(GOOD[1])]
        frames = _run_decoder(device, streams, 8, {"entropy": "auto"})
        assert np.array_equal(frames[1], GOLD["32x24_batch00__img"]) and np.array_equal(frames[2], _rimg(GOOD[1])), device
        with pytest.raises(ValueError, match="row 1: no restart intervals"):
            _run_decoder(device, streams, 8, {"entropy": "gpu"})
        with pytest.raises(RuntimeError, match="invalid entropy 7"):
            _run_decoder(device, streams, 8, b"\x10\x07")


def test_encoder_feeds_the_device_decoder_in_one_graph():
    """ImageEncoder -> ImageDecoder(entropy = gpu): the frames are the definition's decode of the streams the encoder writes."""
    from scannertools_amd.engine import CacheMode, Client, DeviceType, NamedStream, NamedVideoStream, PerfParams
    want = [ref.decode(ENC[n + "__jpg"].tobytes()) for n in ENC_BATCH]
    for device in (DeviceType.GPU, DeviceType.CPU):
        sc = Client()
        sc.ingest_frames("pics", np.stack([ENC[json.loads(str(ENC[n + "__cfg"]))["img"]] for n in ENC_BATCH]))
        frame = sc.io.Input([NamedVideoStream(sc, "pics")])
        img = sc.ops.ImageEncoder(frame=frame, device=DeviceType.GPU, batch=16)
        out = NamedStream(sc, "decoded")
        sc.run(sc.io.Output(sc.ops.ImageDecoder(img=img, device=device, batch=16, args={"entropy": "gpu"}), [out]), PerfParams.estimate(),
               cache_mode=CacheMode.Overwrite)
        rows = list(out.load())
        assert len(rows) == 33
        for n, r, w in zip(ENC_BATCH, rows, want):
            assert r.dtype == np.uint8 and np.array_equal(r, w), (device, n)
