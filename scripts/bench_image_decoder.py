"""ImageDecoder on the MI355X: 1080p 4:2:0 baseline JPEG streams at quality 75 and 90, batches of 1, 8 and 32.
Prints one JSON line.

Needs Pillow to make the streams (seeded synthetic frames) and as the yardstick: Pillow's full decode (libjpeg-turbo at its
defaults, what cv::imdecode calls) on a thread pool stands in for the reference's cv::imdecode pool.  Per quality:
  (a) kernel time of the two kernels per frame from the library's events (st_ctx_timing_*, ST_K_JPEG brackets both launches
      of a sub-batch) and the share of 8 TB/s it is in the as-built byte model (coefficients in, planes out and in again,
      frames out); per-kernel durations come from a trace run, see below;
  (b) the host stage alone (st_jpeg_coefficients: markers + Huffman decoding) in frames/s on 1, 4 and 16 threads;
  (c) st_jpeg_decode_batch end to end (streams in host memory -> frames in device memory, synchronised) in frames/s at
      ST_JPEG_THREADS = 1, 4 and 16, beside Pillow's full decode of the same streams on as many threads.
The first frame of every quality is compared with Pillow byte for byte before anything is timed.

    python scripts/bench_image_decoder.py [--rounds 5]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_image_decoder.py --trace

--trace makes three calls per quality and batch and times nothing: the kernel statistics of the trace then hold k_jpeg_idct
and k_jpeg_color over known work.

    python scripts/bench_image_decoder.py --entropy gpu [--rounds 5]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_image_decoder.py --entropy gpu --trace

--entropy gpu measures st_jpeg_decode_batch_gpu (the Huffman decoder on the device, one lane per restart interval) over the
same pictures re-encoded with one restart interval per MCU row (restart_marker_rows=1), at batches of 32 and 256: frames/s
end to end (synchronised), kernel ms per frame from the library's events (one ST_K_JPEG bracket per sub-batch: the upload,
the entropy launch, the wait for its status word and the two dense launches), and the bytes uploaded per frame.  Beside
it, in the same run, st_jpeg_decode_batch of the same streams at ST_JPEG_THREADS=16: the baseline.  With --trace it makes
three device-path calls per quality and batch, so that the trace's statistics give k_jpeg_entropy_dec's share.

    python scripts/bench_image_decoder.py --split subsequence [--rounds 3]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_image_decoder.py --split subsequence --trace

--split subsequence measures st_jpeg_decode_batch_gpu_split (one lane per subsequence of the entropy-coded bytes) in calls of 1,
8, 32 and 256 frames, frames/s end to end (synchronised) as the median and range of three medians of --rounds calls: (a) on
the streams as Pillow writes them by default (no DRI) beside st_jpeg_decode_batch at ST_JPEG_THREADS=16, (b) on the same pictures
with one restart interval per MCU row beside st_jpeg_decode_batch_gpu (one lane per interval) and the host path.  It reports the
round launches per call and the lanes per frame.  With --trace it makes three subsequence calls per quality, kind of stream and
call size and times nothing.

    python scripts/bench_image_decoder.py --scale 1 2 4 8 [--rounds 3]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_image_decoder.py --scale 1 2 4 8 --trace

--scale measures decode_jpeg(scale=d) (st_jpeg_decode_batch_scaled: libjpeg's scaled decoding, frames of ceil(1080 / d) x
ceil(1920 / d)) for every denominator given, in one process, on the quality-75 pictures with one restart interval per MCU row:
calls of 32 and 256 frames on the host path (ST_JPEG_THREADS=16) and on the interval path, frames/s end to end (synchronised) as
the median and range of three medians of --rounds calls, and the ST_K_JPEG bracket per frame.  Denominator 1 is the yardstick:
code the scale does not touch.  With 4 among them it also times decode + Resize to the 1/4 size beside decode(scale=4), for the
reader only (the two do not produce the same pixels).  With --trace it makes three calls per denominator, path and call size.

    python scripts/bench_image_decoder.py --png [--rounds 3]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_image_decoder.py --png --trace

--png measures decode_png (st_png_decode_batch: inflate on ST_PNG_THREADS=16 host threads, filter reconstruction and expansion
in HIP kernels) on the same 1080p pictures stored as RGB PNG at deflate levels 1 and 6, the rows' filter types cycling through
Sub, Up, Average and Paeth, written by the writer of tests/png_cases.py (Pillow need not be there).  Calls of 1, 8, 32 and 256
streams: frames/s end to end (synchronised), the wall time of a call, the wall time of inflating the call's streams alone on 16
host threads (st_zlib_inflate), and the ST_K_JPEG kernel time of the call from the library's events.  Beside it, in the same
run, Pillow's full decode of the same streams on 16 threads -- or, where Pillow is missing, zlib.decompress plus the library's
CPU twin (st_png_decode_host) on 16 threads; "yardstick" in the output says which.  And the inflater alone on one thread in MB/s
of output against zlib.decompress on the same streams.  With --trace it makes three calls per level and call size.
"""
import argparse
import ctypes
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

H, W = 1080, 1920
BATCHES = (1, 8, 32)
THREADS = (1, 4, 16)
DISTINCT = 8
# as-built byte model per frame (two launches): 4:2:0 has 1.5 samples per pixel on the block-padded planes (1088 rows)
BLOCKS = (W // 16) * ((H + 15) // 16) * 6
MODEL_BYTES = BLOCKS * 128 + 2 * BLOCKS * 64 + H * W * 3


def picture(i):
    rng = np.random.default_rng(100 + i)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    ph = rng.uniform(0, 6.28, 6)
    img = np.stack([127 + 100 * np.sin(x / 37 + ph[0]) * np.cos(y / 23 + ph[1]), 127 + 100 * np.sin((x + y) / 51 + ph[2]) * np.cos(y / 9 + ph[3]),
                    127 + 100 * np.cos(x / 13 + ph[4]) * np.sin((x - y) / 29 + ph[5])], axis=-1)
    return np.clip(img + rng.normal(0, 12, img.shape), 0, 255).astype(np.uint8)   # sensor-like noise: a few hundred KB at q75


def make_streams(Image, quality):
    out = []
    for i in range(DISTINCT):
        img = picture(i)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", quality=quality, subsampling="4:2:0")
        out.append(buf.getvalue())
    return out


def rate(fn, frames, rounds):
    fn()
    times = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return frames / statistics.median(times)


GPU_BATCHES = (32, 256)


def entropy_gpu(args, Image):
    import torch
    from scannertools_amd import _native
    from scannertools_amd.hip import HipContext, jpeg_restart_intervals
    os.environ["ST_JPEG_THREADS"] = "16"
    ctx = HipContext(0)
    result = {"bench": "image_decoder_entropy_gpu", "h": H, "w": W, "sampling": "4:2:0", "restart": "one interval per MCU row",
              "host_threads": 16, "qualities": {}}
    out = torch.empty((max(GPU_BATCHES), H, W, 3), dtype=torch.uint8, device=ctx.device)
    for quality in (75, 90):
        streams = []
        for s in make_streams(Image, quality):
            buf = io.BytesIO()
            Image.open(io.BytesIO(s)).save(buf, "JPEG", quality=quality, subsampling="4:2:0", restart_marker_rows=1)
            streams.append(buf.getvalue())
        for entropy in ("gpu", "host"):
            got = ctx.decode_jpeg(streams[:1], entropy=entropy).cpu().numpy()[0]
            assert np.array_equal(got, np.asarray(Image.open(io.BytesIO(streams[0])))), "decode differs from Pillow (%s)" % entropy
        tables = [jpeg_restart_intervals(s) for s in streams]
        # what one frame adds to a sub-batch's upload: its entropy-coded bytes (padded), interval table, frame record and header
        upload = statistics.mean(((int(t[-1, 1]) - int(t[0, 0]) + 16 + 15) & ~15) + 8 * len(t) + 96 + 512 for t in tables)
        q = {"stream_bytes": int(statistics.mean(len(s) for s in streams)), "intervals_per_frame": len(tables[0]),
             "upload_bytes_per_frame": int(upload), "coefficient_bytes_per_frame": BLOCKS * 128}

        def call(n, entropy):
            ctx.decode_jpeg([streams[i % DISTINCT] for i in range(n)], out=out[:n], entropy=entropy)
            ctx.sync()

        if args.trace:
            for n in GPU_BATCHES:
                for _ in range(3):
                    call(n, "gpu")
            continue
        for entropy in ("gpu", "host"):
            fps, kms = {}, {}
            for n in GPU_BATCHES:
                runs = [rate(lambda: call(n, entropy), n, args.rounds) for _ in range(3)]     # three medians: the run-to-run range
                fps["batch%d" % n] = {"median": round(statistics.median(runs), 1), "min": round(min(runs), 1), "max": round(max(runs), 1)}
            ctx.timing_enable([_native.K_JPEG])
            for n in GPU_BATCHES:
                call(n, entropy)
                ctx.timing_reset()
                for _ in range(args.rounds):
                    call(n, entropy)
                launches, ms = ctx.timing_read(_native.K_JPEG)
                kms["batch%d" % n] = {"ms_per_frame": round(ms / (args.rounds * n), 4), "brackets_per_call": launches / args.rounds}
            ctx.timing_enable([])
            q[entropy + "_fps"], q[entropy + "_bracket"] = fps, kms
        result["qualities"]["q%d" % quality] = q
    ctx.close()
    print(json.dumps(result))


SPLIT_BATCHES = (1, 8, 32, 256)


def split_subsequence(args, Image):
    import torch
    from scannertools_amd.hip import HipContext
    os.environ["ST_JPEG_THREADS"] = "16"
    ctx = HipContext(0)
    result = {"bench": "image_decoder_split_subsequence", "h": H, "w": W, "sampling": "4:2:0", "host_threads": 16, "subseq_bytes": args.subseq_bytes or 128,
              "calls_per_median": args.rounds, "qualities": {}}
    out = torch.empty((max(SPLIT_BATCHES), H, W, 3), dtype=torch.uint8, device=ctx.device)
    for quality in (75, 90):
        plain = make_streams(Image, quality)
        rows = []
        for s in plain:
            buf = io.BytesIO()
            Image.open(io.BytesIO(s)).save(buf, "JPEG", quality=quality, subsampling="4:2:0", restart_marker_rows=1)
            rows.append(buf.getvalue())
        q = {}
        for kind, streams, paths in (("no_dri", plain, ("subsequence", "host")), ("restart_rows", rows, ("subsequence", "interval", "host"))):

            def call(n, path):
                batch = [streams[i % DISTINCT] for i in range(n)]
                if path == "host":
                    ctx.decode_jpeg(batch, out=out[:n])
                elif path == "interval":
                    ctx.decode_jpeg(batch, out=out[:n], entropy="gpu")
                else:
                    ctx.decode_jpeg(batch, out=out[:n], entropy="gpu", split="subsequence", subseq_bytes=args.subseq_bytes)
                ctx.sync()

            want = np.asarray(Image.open(io.BytesIO(streams[0])))
            for path in paths:
                call(1, path)
                assert np.array_equal(out[0].cpu().numpy(), want), "decode differs from Pillow (%s, %s)" % (kind, path)
            k = {"stream_bytes": int(statistics.mean(len(s) for s in streams)),
                 "lanes_per_frame": int(statistics.mean(-(-(len(s) - s.index(b"\xff\xda")) // (args.subseq_bytes or 128)) for s in streams))}
            if args.trace:
                for n in SPLIT_BATCHES:
                    for _ in range(3):
                        call(n, "subsequence")
                q[kind] = k
                continue
            for path in paths:
                fps = {}
                for n in SPLIT_BATCHES:
                    runs = [rate(lambda: call(n, path), n, args.rounds) for _ in range(3)]     # three medians: the run-to-run range
                    fps["batch%d" % n] = {"median": round(statistics.median(runs), 1), "min": round(min(runs), 1), "max": round(max(runs), 1)}
                    if path == "subsequence":
                        fps["batch%d" % n]["round_launches"] = ctx.last_jpeg_rounds()
                k[path + "_fps"] = fps
            q[kind] = k
        result["qualities"]["q%d" % quality] = q
    ctx.close()
    print(json.dumps(result))


def scaled(args, Image):
    import torch
    from scannertools_amd import _native
    from scannertools_amd.hip import HipContext, jpeg_scaled_size
    os.environ["ST_JPEG_THREADS"] = "16"
    ctx = HipContext(0)
    quality = 75
    result = {"bench": "image_decoder_scale", "h": H, "w": W, "sampling": "4:2:0", "quality": quality, "restart": "one interval per MCU row",
              "host_threads": 16, "calls_per_median": args.rounds, "scales": {}}
    streams = []
    for s in make_streams(Image, quality):
        buf = io.BytesIO()
        Image.open(io.BytesIO(s)).save(buf, "JPEG", quality=quality, subsampling="4:2:0", restart_marker_rows=1)
        streams.append(buf.getvalue())
    result["stream_bytes"] = int(statistics.mean(len(s) for s in streams))
    paths = (("host", dict()), ("interval", dict(entropy="gpu")))
    for d in args.scale:
        oh, ow = jpeg_scaled_size(H, W, d)
        out = torch.empty((max(GPU_BATCHES), oh, ow, 3), dtype=torch.uint8, device=ctx.device)
        im = Image.open(io.BytesIO(streams[0]))
        if d > 1:
            im.draft("RGB", (W // d, H // d))
        want = np.asarray(im)
        assert want.shape == (oh, ow, 3)

        def call(n, kw):
            ctx.decode_jpeg([streams[i % DISTINCT] for i in range(n)], out=out[:n], scale=d, **kw)
            ctx.sync()

        r = {"frame": [oh, ow, 3]}
        for path, kw in paths:
            call(1, kw)
            assert np.array_equal(out[0].cpu().numpy(), want), "decode at 1/%d differs from Pillow (%s)" % (d, path)
            if args.trace:
                for n in GPU_BATCHES:
                    for _ in range(3):
                        call(n, kw)
                continue
            fps, kms = {}, {}
            for n in GPU_BATCHES:
                runs = [rate(lambda: call(n, kw), n, args.rounds) for _ in range(3)]     # three medians: the run-to-run range
                fps["batch%d" % n] = {"median": round(statistics.median(runs), 1), "min": round(min(runs), 1), "max": round(max(runs), 1)}
            ctx.timing_enable([_native.K_JPEG])
            for n in GPU_BATCHES:
                call(n, kw)
                ctx.timing_reset()
                for _ in range(args.rounds):
                    call(n, kw)
                _, ms = ctx.timing_read(_native.K_JPEG)
                kms["batch%d" % n] = round(ms / (args.rounds * n), 4)
            ctx.timing_enable([])
            r[path + "_fps"], r[path + "_bracket_ms_per_frame"] = fps, kms
        if d == 4 and not args.trace:
            # what a pipeline without the scale does for the same size: the full decode, then Resize
            full = torch.empty((32, H, W, 3), dtype=torch.uint8, device=ctx.device)
            small = torch.empty((32, oh, ow, 3), dtype=torch.uint8, device=ctx.device)

            def decode_resize():
                ctx.decode_jpeg([streams[i % DISTINCT] for i in range(32)], out=full)
                ctx.resize(full, ow, oh, out=small)
                ctx.sync()

            runs = [rate(decode_resize, 32, args.rounds) for _ in range(3)]
            r["decode_then_resize_host_fps_batch32"] = {"median": round(statistics.median(runs), 1), "min": round(min(runs), 1), "max": round(max(runs), 1)}
        result["scales"]["1/%d" % d] = r
        del out
    ctx.close()
    print(json.dumps(result))


PNG_BATCHES = (1, 8, 32, 256)


def png(args):
    import zlib
    import torch
    from scannertools_amd import _native
    from scannertools_amd.hip import HipContext, png_decode_host, zlib_inflate
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import png_cases as pc
    try:
        from PIL import Image
    except ImportError:
        Image = None
    os.environ["ST_PNG_THREADS"] = "16"
    ctx = HipContext(0)
    L = _native.lib()
    result = {"bench": "image_decoder_png", "h": H, "w": W, "colour_type": "RGB 8", "filters": "Sub, Up, Average, Paeth by row", "host_threads": 16,
              "calls_per_median": args.rounds, "yardstick": "Pillow on 16 threads" if Image else "zlib.decompress + st_png_decode_host on 16 threads",
              "levels": {}}
    pictures = [picture(i) for i in range(DISTINCT)]
    raws = [pc.filter_rows(pc.scanlines(p, 2, 8), 3, [1 + y % 4 for y in range(H)]).tobytes() for p in pictures]
    out = torch.empty((max(PNG_BATCHES), H, W, 3), dtype=torch.uint8, device=ctx.device)
    sink = [np.empty(len(raws[0]), np.uint8) for _ in range(16)]
    for level in (1, 6):
        zs = [pc.deflate(r, level) for r in raws]
        streams = [pc.write_png(p, 2, zdata=z) for p, z in zip(pictures, zs)]
        assert np.array_equal(ctx.decode_png(streams[:1]).cpu().numpy()[0], pictures[0]), "decode differs from the picture"
        r = {"stream_bytes": int(statistics.mean(len(s) for s in streams)), "inflated_bytes": len(raws[0])}

        def call(n):
            ctx.decode_png([streams[i % DISTINCT] for i in range(n)], out=out[:n])
            ctx.sync()

        if args.trace:
            for n in PNG_BATCHES:
                for _ in range(3):
                    call(n)
            result["levels"]["z%d" % level] = r
            continue
        # the inflater alone, one thread, against zlib on the same streams
        t0 = time.perf_counter()
        for z, raw in zip(zs, raws):
            assert zlib_inflate(z, len(raw)) == raw
        ours = time.perf_counter() - t0
        t0 = time.perf_counter()
        for z in zs:
            zlib.decompress(z)
        theirs = time.perf_counter() - t0
        mb = sum(len(x) for x in raws) / 1e6
        r["inflate_one_thread_MBps"] = {"st_zlib_inflate": round(mb / ours, 1), "zlib_decompress": round(mb / theirs, 1), "ratio": round(theirs / ours, 3)}

        def inflate_only(i):
            z, buf = zs[i % DISTINCT], sink[i % 16]
            assert L.st_zlib_inflate(z, len(z), buf.ctypes.data, buf.size, None, None, 0) == 0

        def yardstick(i):
            if Image:
                Image.open(io.BytesIO(streams[i % DISTINCT])).load()
            else:
                zlib.decompress(zs[i % DISTINCT])
                png_decode_host(streams[i % DISTINCT])

        calls = {}
        with ThreadPoolExecutor(16) as pool:
            for n in PNG_BATCHES:
                c = {"fps": round(rate(lambda: call(n), n, args.rounds), 1)}
                c["call_ms"] = round(1e3 * n / c["fps"], 2)
                c["inflate_alone_ms"] = round(1e3 * n / rate(lambda: list(pool.map(inflate_only, range(n))), n, args.rounds), 2)
                c["yardstick_fps"] = round(rate(lambda: list(pool.map(yardstick, range(n))), n, args.rounds), 1)
                calls["batch%d" % n] = c
        ctx.timing_enable([_native.K_JPEG])
        for n in PNG_BATCHES:
            call(n)
            ctx.timing_reset()
            for _ in range(args.rounds):
                call(n)
            launches, ms = ctx.timing_read(_native.K_JPEG)
            calls["batch%d" % n]["kernel_ms"] = round(ms / args.rounds, 3)
            calls["batch%d" % n]["launches"] = launches / args.rounds
        ctx.timing_enable([])
        r["calls"] = calls
        result["levels"]["z%d" % level] = r
    ctx.close()
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--entropy", choices=("host", "gpu"), default="host", help="gpu: measure st_jpeg_decode_batch_gpu beside the host path")
    ap.add_argument("--split", choices=("interval", "subsequence"), default="interval",
                    help="subsequence: measure st_jpeg_decode_batch_gpu_split beside the interval kernel and the host path")
    ap.add_argument("--subseq-bytes", type=int, default=None, help="with --split subsequence: bytes per lane (default: the library's)")
    ap.add_argument("--scale", type=int, nargs="+", choices=(1, 2, 4, 8), default=None,
                    help="measure decode_jpeg(scale=d) for each denominator given, on the host path and the interval path")
    ap.add_argument("--png", action="store_true", help="measure decode_png on 1080p RGB PNG streams at deflate levels 1 and 6")
    args = ap.parse_args()
    if args.png:
        return png(args)
    try:
        from PIL import Image
    except ImportError:
        sys.exit("bench_image_decoder.py needs Pillow to make its 1080p streams and as its yardstick")
    if args.scale:
        return scaled(args, Image)
    if args.split == "subsequence":
        return split_subsequence(args, Image)
    if args.entropy == "gpu":
        return entropy_gpu(args, Image)
    import torch
    from scannertools_amd import _native
    from scannertools_amd.hip import HipContext
    L = _native.lib()
    ctx = HipContext(0)
    result = {"bench": "image_decoder", "h": H, "w": W, "sampling": "4:2:0", "model_bytes_per_frame": MODEL_BYTES, "qualities": {}}
    for quality in (75, 90):
        streams = make_streams(Image, quality)
        got = ctx.decode_jpeg(streams[:1]).cpu().numpy()[0]
        assert np.array_equal(got, np.asarray(Image.open(io.BytesIO(streams[0])))), "decode differs from Pillow"
        q = {"stream_bytes": int(statistics.mean(len(s) for s in streams))}
        outs = {n: torch.empty((n, H, W, 3), dtype=torch.uint8, device=ctx.device) for n in BATCHES}

        def gpu_call(n):
            ctx.decode_jpeg([streams[i % DISTINCT] for i in range(n)], out=outs[n])
            ctx.sync()

        if args.trace:
            os.environ["ST_JPEG_THREADS"] = "16"
            for n in BATCHES:
                for _ in range(3):
                    gpu_call(n)
            continue
        # (b) the host stage alone
        coefs = [np.empty(BLOCKS * 64, np.int16) for _ in range(32)]

        def host_stage(i):
            s = streams[i % DISTINCT]
            assert L.st_jpeg_coefficients(s, len(s), coefs[i].ctypes.data, coefs[i].size, None, None) == 0

        def pillow(i):
            Image.open(io.BytesIO(streams[i % DISTINCT])).load()

        q["host_stage_fps"], q["pillow_fps"], q["decode_batch_fps"], q["kernel_ms_per_frame"] = {}, {}, {}, {}
        for t in THREADS:
            with ThreadPoolExecutor(t) as pool:
                q["host_stage_fps"][t] = round(rate(lambda: list(pool.map(host_stage, range(32))), 32, args.rounds), 1)
                q["pillow_fps"][t] = round(rate(lambda: list(pool.map(pillow, range(32))), 32, args.rounds), 1)
            # (c) end to end, (a) kernel time from the library's events
            os.environ["ST_JPEG_THREADS"] = str(t)
            for n in BATCHES:
                q["decode_batch_fps"]["threads%d_batch%d" % (t, n)] = round(rate(lambda: gpu_call(n), n, args.rounds), 1)
        os.environ["ST_JPEG_THREADS"] = "16"
        ctx.timing_enable([_native.K_JPEG])
        for n in BATCHES:
            gpu_call(n)
            ctx.timing_reset()
            for _ in range(args.rounds):
                gpu_call(n)
            launches, ms = ctx.timing_read(_native.K_JPEG)
            per_frame = ms / (args.rounds * n)
            q["kernel_ms_per_frame"]["batch%d" % n] = round(per_frame, 4)
            q["kernel_share_of_8TBps_batch%d" % n] = round(MODEL_BYTES / (per_frame * 1e-3) / 8e12, 3)
        ctx.timing_enable([])
        result["qualities"]["q%d" % quality] = q
    ctx.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
