"""GPU: st_jpeg_decode_batch_gpu_split (the kernels of st_jpeg_subseq.hip: the Huffman decoder on the device with one lane per
subsequence, for streams with or without restart intervals) and the ImageDecoder kernel classes with ImageDecoderArgs.split,
against Pillow's golden frames and the host path: byte for byte.  Reads tests/golden/jpeg_subsequence_golden.npz,
jpeg_golden.npz, jpeg_restart_golden.npz and jpeg_encode_golden.npz."""
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
SUB = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_subsequence_golden.npz"))
SUB_CASES = [str(c) for c in SUB["cases"]]
SUB_GOOD = [str(c) for c in SUB["good"]]
SUB_CORRUPT = [str(c) for c in SUB["corrupt"]]
RST_CASES = [str(c) for c in RST["cases"]]
RST_GOOD = [str(c) for c in RST["good"]]
RST_MIXED = [str(c) for c in RST["mixed"]]
BATCH = [str(c) for c in GOLD["batch"]]
ENC_BATCH = [str(c) for c in ENC["batch"]]
TINY = ["8x8_noise_q30_422", "8x8_smooth_q95_420_opt", "8x8_noise_q5_420", "8x8_smooth_q75_444"]            # of jpeg_golden.npz, no DRI
TINY_MIXED = ["8x8_noise_q30_422", "8x8_noise_q100_420_rst3", "8x8_smooth_q95_420_opt", "8x8_smooth_q90_422_rstrow", "8x8_noise_q5_420",
              "8x8_smooth_q100_420_rst3", "8x8_noise_q90_422_rstrow"]
OPTS = ((8, 0), (16, 0), (0, 1))             # (subseq_bytes, max_rounds); the last one is the fallback


def _has_dri(jpg):
    sos = jpg.index(b"\xff\xda")
    return jpg.find(b"\xff\xdd\x00\x04", 0, sos) >= 0


GOLD_PLAIN = [str(c) for c in GOLD["cases"] if not _has_dri(GOLD[str(c) + "__jpg"].tobytes())]


def _rimg(name):
    key = name + "__img"
    return RST[key] if key in RST.files else RST[str(RST[name + "__same_as"]) + "__img"]


def _split(hip_ctx, streams, shape, opts, fill=0xA5):
    """(status, message, (n, h, w, c) frames) of st_jpeg_decode_batch_gpu_split with the options (subseq_bytes, max_rounds)."""
    import torch
    from scannertools_amd import _native
    L, vp = _native.lib(), ctypes.c_void_p
    hip_ctx._bind()
    n = len(streams)
    out = torch.full((n,) + tuple(shape), fill, dtype=torch.uint8, device=hip_ctx.device)
    keep = [ctypes.create_string_buffer(s, len(s)) for s in streams]
    bufs = (vp * n)(*[ctypes.addressof(b) for b in keep])
    sizes = (ctypes.c_size_t * n)(*[len(s) for s in streams])
    to = (vp * n)(*[out[i].data_ptr() for i in range(n)])
    o = _native.JpegSplitOpts(*opts)
    st = L.st_jpeg_decode_batch_gpu_split(hip_ctx._h, bufs, sizes, n, shape[0], shape[1], shape[2], to, ctypes.byref(o))
    msg = L.st_ctx_last_error(hip_ctx._h) if st else b""
    hip_ctx.sync()
    return st, msg, out.cpu().numpy()


def test_frames_without_restart_intervals_at_the_default_size(hip_ctx):
    """Every stream without DRI of jpeg_golden.npz and every stream of the new file, the streams of one shape in one call."""
    assert len(GOLD_PLAIN) == 130
    by_shape = {}
    for G, names in ((GOLD, GOLD_PLAIN), (SUB, SUB_CASES)):
        for n in names:
            by_shape.setdefault(G[n + "__img"].shape, []).append((G[n + "__jpg"].tobytes(), G[n + "__img"], n))
    assert len(by_shape) > 10
    for shape, group in by_shape.items():
        got = hip_ctx.decode_jpeg([g[0] for g in group], entropy="gpu", split="subsequence").cpu().numpy()
        assert got.shape == (len(group),) + shape
        for i, (_, want, n) in enumerate(group):
            assert np.array_equal(got[i], want), (n, int((got[i] != want).sum()))
        assert 1 <= hip_ctx.last_jpeg_rounds() <= 64, shape


def test_small_subsequences_and_the_fallback(hip_ctx):
    """8 and 16 bytes per lane, and one round launch with the interval decoder behind it: 200x328_422 is 2 408 lanes of 8 bytes in
    38 workgroups.  Each result is the host path's; with DRI it is the interval kernel's too."""
    from scannertools_amd import _native
    cases = [(GOLD, "200x328_422"), (SUB, "203x213_noise_420"), (SUB, "61x45_gray"), (GOLD, "8x8_gray_q60")]
    cases += [(GOLD, n) for n in TINY] + [(RST, n) for n in RST_CASES]
    for G, name in cases:
        jpg = G[name + "__jpg"].tobytes()
        host = hip_ctx.decode_jpeg([jpg]).cpu().numpy()
        assert np.array_equal(host[0], _rimg(name) if G is RST else G[name + "__img"]), name
        if _has_dri(jpg):
            assert np.array_equal(hip_ctx.decode_jpeg([jpg], entropy="gpu", split="interval").cpu().numpy(), host), name
        for opts in OPTS:
            st, msg, got = _split(hip_ctx, [jpg], host.shape[1:], opts)
            assert st == _native.ST_OK, (name, opts, msg)
            assert np.array_equal(got, host), (name, opts, int((got != host).sum()))


def test_batches_equal_singles(hip_ctx):
    streams = [GOLD[n + "__jpg"].tobytes() for n in BATCH]
    assert len(streams) == 33 and not any(_has_dri(s) for s in streams)
    singles = [hip_ctx.decode_jpeg([s], entropy="gpu", split="subsequence").cpu().numpy()[0] for s in streams]
    for n, got in zip(BATCH, singles):
        assert np.array_equal(got, GOLD[n + "__img"]), n
    for count in (1, 8, 33):
        for threads in (16, 3):
            with env_threads("ST_JPEG_THREADS", threads):
                got = hip_ctx.decode_jpeg(streams[:count], entropy="auto", split="subsequence").cpu().numpy()
            assert np.array_equal(got, np.stack(singles[:count])), (count, threads)


def test_mixed_streams_in_one_call(hip_ctx):
    """With and without DRI, 4:2:0 and 4:2:2, standard and optimised tables, in one call."""
    for threads in (16, 2):
        with env_threads("ST_JPEG_THREADS", threads):
            got = hip_ctx.decode_jpeg([GOLD[n + "__jpg"].tobytes() for n in TINY_MIXED], entropy="gpu", split="subsequence").cpu().numpy()
        for i, n in enumerate(TINY_MIXED):
            assert np.array_equal(got[i], GOLD[n + "__img"]), (threads, n)
    names = [(RST, RST_MIXED[0]), (SUB, SUB_GOOD[0]), (RST, RST_MIXED[1]), (GOLD, BATCH[0]), (RST, RST_GOOD[1]), (SUB, SUB_GOOD[2]), (RST, RST_MIXED[1])]
    for subseq_bytes in (None, 8):
        got = hip_ctx.decode_jpeg([G[n + "__jpg"].tobytes() for G, n in names], entropy="gpu", split="subsequence", subseq_bytes=subseq_bytes).cpu().numpy()
        for i, (G, n) in enumerate(names):
            assert np.array_equal(got[i], _rimg(n) if G is RST else G[n + "__img"]), (subseq_bytes, i, n)


def test_store_width_does_not_change_a_byte(hip_ctx):
    """Frames that start on a 16-byte boundary, on a 4-byte one and on an odd byte; the bytes around them stay."""
    import torch
    for name in ("32x24_good0", "61x45_gray", "97x75_420_opt", "264x40_422_rstrow4"):
        want = SUB[name + "__img"]
        nbytes = want.size
        for offset in (0, 4, 1):
            buf = torch.full((nbytes + 64,), 0x5A, dtype=torch.uint8, device=hip_ctx.device)
            out = buf[offset:offset + nbytes].view((1,) + want.shape)
            hip_ctx.decode_jpeg([SUB[name + "__jpg"].tobytes()], out=out, entropy="gpu", split="subsequence")
            host = buf.cpu().numpy()
            assert np.array_equal(host[offset:offset + nbytes].reshape(want.shape), want), (name, offset)
            assert (host[:offset] == 0x5A).all() and (host[offset + nbytes:] == 0x5A).all(), (name, offset)


def test_one_call_past_a_grid_dimension(hip_ctx):
    """65 537 tiny streams without DRI in one call: more frames than one grid.y holds, so the dense kernels (frames on grid.y) run
    in two launches, of 65 535 and 2 frames.  The subsequence kernels take frames on grid.x, here 65 537 workgroups wide: their
    `f += gridDim.x` stride is NOT taken (lane_grid() caps grid.x at 2^20 frames), and no frame has more than one group of lanes.
    The strides over groups and segments (grid.y) are what tests/test_jpeg_large_gpu.py reaches."""
    n = 65537
    streams = [GOLD[t + "__jpg"].tobytes() for t in TINY]
    frames = np.stack([GOLD[t + "__img"] for t in TINY])
    got = hip_ctx.decode_jpeg([streams[i & 3] for i in range(n)], entropy="gpu", split="subsequence").cpu().numpy()
    assert got.shape == (n, 8, 8, 3)
    assert np.array_equal(got[:65536].reshape(16384, 4, 8, 8, 3), np.broadcast_to(frames, (16384, 4, 8, 8, 3)))
    assert np.array_equal(got[65536], frames[0])


def test_a_corrupt_scan_fails_the_call_and_writes_nothing(hip_ctx):
    """The stored corrupt variants (every marker present, a quarter of the scan's bytes gone) and a truncated scan, each as stream
    2 between good streams.  tests/test_jpeg_subsequence.py runs the same bytes through the same core under the sanitizers first."""
    from scannertools_amd import _native
    from scannertools_amd.hip import StError
    good = [SUB[n + "__jpg"].tobytes() for n in SUB_GOOD]
    want = np.stack([SUB[n + "__img"] for n in SUB_GOOD])
    scan = good[1].index(b"\xff\xda") + 14
    bads = [SUB[n + "__jpg"].tobytes() for n in SUB_CORRUPT] + [good[1][:scan + (len(good[1]) - scan) // 2]]
    causes = (b"bad DC code", b"bad AC code", b"a run leaves the block", b"the data ends inside the interval")
    for bad in bads:
        streams = good[:2] + [bad] + good[2:]
        for opts in ((0, 0), (8, 0), (0, 1)):
            st, msg, out = _split(hip_ctx, streams, (24, 32, 3), opts)
            assert st == _native.ST_ERR_INVALID and b"stream 2: corrupt scan: the scan: " in msg and any(c in msg for c in causes), (opts, st, msg)
            assert (out == 0xA5).all(), (opts, msg)
        with pytest.raises(StError, match="stream 2: corrupt scan: the scan"):
            hip_ctx.decode_jpeg(streams, entropy="gpu", split="subsequence")
        # the context decodes the good streams afterwards
        assert np.array_equal(hip_ctx.decode_jpeg(good, entropy="gpu", split="subsequence").cpu().numpy(), want)
    # with DRI the message names the interval
    rgood = [RST[n + "__jpg"].tobytes() for n in RST_GOOD]
    for name in RST["corrupt"]:
        k = int(RST[str(name) + "__interval"])
        st, msg, out = _split(hip_ctx, rgood[:2] + [RST[str(name) + "__jpg"].tobytes()] + rgood[2:], (24, 32, 3), (0, 0))
        assert st == _native.ST_ERR_INVALID and b"stream 2" in msg and b"restart interval %d of 4" % k in msg and (out == 0xA5).all(), (name, st, msg)
    L = _native.lib()
    assert L.st_jpeg_decode_batch_gpu_split(hip_ctx._h, None, None, 0, 24, 32, 3, None, None) == _native.ST_OK
    assert L.st_jpeg_decode_batch_gpu_split(hip_ctx._h, None, None, 1, 24, 32, 3, None, None) == _native.ST_ERR_INVALID
    st, msg, _ = _split(hip_ctx, good, (24, 32, 3), (12, 0))
    assert st == _native.ST_ERR_INVALID and b"subseq_bytes" in msg


def _run_decoder(device, streams, batch, args):
    from scannertools_amd.engine import CacheMode, Client, NamedStream, PerfParams
    sc = Client()
    sc.ingest_rows("jpgs", streams)
    img = sc.io.Input([NamedStream(sc, "jpgs")])
    out = NamedStream(sc, "frames")
    sc.run(sc.io.Output(sc.ops.ImageDecoder(img=img, device=device, batch=batch, args=args), [out]), PerfParams.estimate(),
           cache_mode=CacheMode.Overwrite)
    return list(out.load())


def test_kernel_classes_honour_the_split_field():
    from scannertools_amd.engine import DeviceType
    rows = [(RST, RST_GOOD[0]), (SUB, SUB_GOOD[0]), (RST, RST_MIXED[1]), (GOLD, BATCH[3]), (SUB, SUB_GOOD[3]), (RST, RST_GOOD[2])]
    streams = [G[n + "__jpg"].tobytes() for G, n in rows]
    for device in (DeviceType.GPU, DeviceType.CPU):
        for args in ({"entropy": "gpu", "split": "subsequence"}, {"entropy": "auto", "split": "subsequence"}, b"\x08\x01\x10\x01\x18\x01"):
            frames = _run_decoder(device, streams, 4, args)                                  # executes of 4 and 2 rows
            assert len(frames) == 6
            for (G, n), f in zip(rows, frames):
                assert f.dtype == np.uint8 and np.array_equal(f, _rimg(n) if G is RST else G[n + "__img"]), (device, args, n)
        with pytest.raises(ValueError, match="row 1: no restart intervals"):                # by interval the row is still refused
            _run_decoder(device, streams, 8, {"entropy": "gpu", "split": "interval"})
        for args in (b"\x18\x01", b"\x10\x00\x18\x01"):
            with pytest.raises(RuntimeError, match="split = SUBSEQUENCE.*entropy"):
                _run_decoder(device, streams, 8, args)
        with pytest.raises(RuntimeError, match="invalid split 7"):
            _run_decoder(device, streams, 8, b"\x18\x07")


def test_encoder_feeds_the_subsequence_decoder_in_one_graph():
    """ImageEncoder -> ImageDecoder(entropy = gpu, split = subsequence): the definition's decode of the streams the encoder writes."""
    from scannertools_amd.engine import CacheMode, Client, DeviceType, NamedStream, NamedVideoStream, PerfParams
    want = [ref.decode(ENC[n + "__jpg"].tobytes()) for n in ENC_BATCH]
    for device in (DeviceType.GPU, DeviceType.CPU):
        sc = Client()
        sc.ingest_frames("pics", np.stack([ENC[json.loads(str(ENC[n + "__cfg"]))["img"]] for n in ENC_BATCH]))
        frame = sc.io.Input([NamedVideoStream(sc, "pics")])
        img = sc.ops.ImageEncoder(frame=frame, device=DeviceType.GPU, batch=16)
        out = NamedStream(sc, "decoded")
        sc.run(sc.io.Output(sc.ops.ImageDecoder(img=img, device=device, batch=16, args={"entropy": "gpu", "split": "subsequence"}), [out]),
               PerfParams.estimate(), cache_mode=CacheMode.Overwrite)
        rows = list(out.load())
        assert len(rows) == 33
        for n, r, w in zip(ENC_BATCH, rows, want):
            assert r.dtype == np.uint8 and np.array_equal(r, w), (device, n)
