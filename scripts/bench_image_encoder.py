"""ImageEncoder on the MI355X: resident 1080p frames to baseline JPEG streams at quality 95, 4:2:0, batches of 32 and 256.
Prints one JSON line.

Needs Pillow as the yardstick: Pillow (libjpeg-turbo) encoding the same frames from host memory on a pool of 16 threads is
the only baseline there is -- the op has no predecessor.  Per batch size, after a warm-up call, over --rounds repetitions:
  (a) frames/s of the whole call, st_jpeg_encode_batch + st_jpeg_encode_fetch into host buffers (median, and the range);
  (b) the four kernels' time per frame from the library's events (ST_K_JPEG brackets each launch);
  (c) the bytes per frame that cross to the host (the streams), beside the 6.2 MB of a raw frame;
  (d) Pillow's frames/s on 16 threads, host frames in, bytes out.
The first stream is compared with Pillow's byte for byte before anything is timed.  The frames are synthetic (seeded smooth
structure plus sensor-like noise), eight distinct ones repeated.

    python scripts/bench_image_encoder.py [--rounds 7] [--restart row|none|both] [--optimize off|on|both]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_image_encoder.py --trace [--restart none]

--trace makes three calls per batch size and times nothing: the kernel statistics of the trace then hold the four kernels'
shares (k_jpeg_fdct, k_jpeg_entropy, k_jpeg_layout, k_jpeg_pack) over known work.

--restart row (the default) measures streams with one restart interval per MCU row and prints what it always printed; none
measures streams without restart markers (five launches: k_jpeg_fdct, k_jpeg_entropy<false>, k_jpeg_ff_count, k_jpeg_layout<false>,
k_jpeg_pack_bits; Pillow then encodes without markers too); both measures the two in ONE run on the same frames, their timed
calls alternating, so that the difference between them can be set against the spread between repeats of the run.  The figures
of "none" go under "batches_norst".

--optimize off (the default) changes nothing; on measures the calls with per-frame optimised Huffman tables
(st_jpeg_encode_batch_opt(..., optimize = 1): k_jpeg_sym_stats and k_jpeg_opt_tables between the transform and the entropy coder;
Pillow then saves with optimize=True too); both measures the two settings in ONE run on the same frames, their timed calls
alternating like those of --restart both, so that "off" is the unchanged path measured beside "on".  The figures with optimised
tables go under "batches_opt" / "batches_norst_opt": frames/s, kernel ms per frame and stream bytes per frame as for the others.

--format png measures the lossless PNG output instead (st_png_encode_batch + st_png_encode_fetch) on two kinds of
resident 1080p RGB frames: the noisy frames above ("photo") and Montage-like sheets, the same pictures at quarter size tiled 2 x 2
inside flat borders ("sheet").  Per kind and batch size: frames/s of the whole call, the four kernels' ms per frame from the
library's events, stream bytes per frame, and in the same run Pillow's save(format="PNG") on 16 threads at its default and at
compress_level=1.  The first stream of each kind is decoded back with the library's own decoder before anything is timed.  With
--trace it makes three calls per kind and batch size for a rocprofv3 --kernel-trace --stats run of its own (k_png_filter,
k_png_deflate, k_png_enc_layout, k_png_enc_pack).
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
QUALITY, SUBSAMPLING = 95, "4:2:0"
BATCHES = (32, 256)
DISTINCT = 8
THREADS = 16


def make_frames():
    out = []
    for i in range(DISTINCT):
        rng = np.random.default_rng(100 + i)
        y, x = np.mgrid[0:H, 0:W].astype(np.float32)
        ph = rng.uniform(0, 6.28, 6)
        img = np.stack([127 + 100 * np.sin(x / 37 + ph[0]) * np.cos(y / 23 + ph[1]), 127 + 100 * np.sin((x + y) / 51 + ph[2]) * np.cos(y / 9 + ph[3]),
                        127 + 100 * np.cos(x / 13 + ph[4]) * np.sin((x - y) / 29 + ph[5])], axis=-1)
        out.append(np.clip(img + rng.normal(0, 12, img.shape), 0, 255).astype(np.uint8))
    return out


def make_sheets(host):
    """Montage-like: four quarter-size pictures in a 2 x 2 grid with flat borders and gutters"""
    out = []
    for i in range(DISTINCT):
        sheet = np.zeros((H, W, 3), np.uint8)
        th, tw = H // 2 - 60, W // 2 - 80
        for k in range(4):
            tile = host[(i + k) % DISTINCT][::2, ::2][:th, :tw]
            y0, x0 = 40 + (k // 2) * (H // 2), 60 + (k % 2) * (W // 2)
            sheet[y0:y0 + th, x0:x0 + tw] = tile
        out.append(sheet)
    return out


def main_png(args):
    from PIL import Image
    import torch
    from scannertools_amd import _native
    from scannertools_amd.hip import HipContext, png_encode_bound
    L = _native.lib()
    ctx = HipContext(0)
    photos = make_frames()
    kinds = {"photo": photos, "sheet": make_sheets(photos)}
    bound = png_encode_bound(H, W, 3)
    result = {"bench": "image_encoder_png", "h": H, "w": W, "filter": "adaptive", "raw_frame_bytes": H * W * 3, "bound_bytes": bound,
              "rounds": args.rounds}
    ctx._bind()
    for kind, host in kinds.items():
        dev = [torch.from_numpy(f).cuda() for f in host]
        (first,) = ctx.encode_png([dev[0]])
        assert np.array_equal(ctx.decode_png([first]).cpu().numpy()[0], host[0]), "the stream does not decode back to the frame"
        result[kind] = {}

        def pillow(i, level):
            buf = io.BytesIO()
            Image.fromarray(host[i % DISTINCT]).save(buf, "PNG", **({} if level is None else {"compress_level": level}))
            return len(buf.getvalue())

        for n in BATCHES:
            tab = (ctypes.c_void_p * n)(*[dev[i % DISTINCT].data_ptr() for i in range(n)])
            sizes = (ctypes.c_size_t * n)()
            store = np.empty((n, bound), np.uint8)   # pages are touched only where written
            bufs = (ctypes.c_void_p * n)(*[store[i].ctypes.data for i in range(n)])

            def call():
                ctx._check(L.st_png_encode_batch(ctx._h, tab, n, H, W, 3, 5))
                ctx._check(L.st_png_encode_fetch(ctx._h, bufs, sizes, bound))

            if args.trace:
                for _ in range(3):
                    call()
                continue
            call()   # warm-up: workspace, stream buffer and staging grow here
            b = {"stream_bytes_per_frame": int(statistics.mean(sizes))}
            t = []
            for _ in range(args.rounds):
                t0 = time.perf_counter()
                call()
                t.append(time.perf_counter() - t0)
            b.update({"fps_median": round(n / statistics.median(t), 1), "fps_min": round(n / max(t), 1), "fps_max": round(n / min(t), 1)})
            ctx.timing_enable([_native.K_JPEG])
            ctx.timing_reset()
            for _ in range(args.rounds):
                call()
            launches, ms = ctx.timing_read(_native.K_JPEG)
            ctx.timing_enable([])
            b["kernel_ms_per_frame"] = round(ms / (args.rounds * n), 4)
            b["kernel_launches_per_call"] = launches // args.rounds
            with ThreadPoolExecutor(THREADS) as pool:
                for level, key in ((None, "pillow_default"), (1, "pillow_level1")):
                    t, got = [], []
                    for _ in range(2):
                        t0 = time.perf_counter()
                        got = list(pool.map(lambda i: pillow(i, level), range(n)))
                        t.append(time.perf_counter() - t0)
                    b[key + "_%d_threads_fps" % THREADS] = round(n / min(t), 1)
                    b[key + "_bytes_per_frame"] = int(statistics.mean(got))
            result[kind]["batch%d" % n] = b
            del store
        del dev
        ctx.release_workspace()
    ctx.close()
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--format", choices=("jpeg", "png"), default="jpeg")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--restart", choices=("row", "none", "both"), default="row")
    ap.add_argument("--optimize", choices=("off", "on", "both"), default="off")
    args = ap.parse_args()
    try:
        from PIL import Image
    except ImportError:
        sys.exit("bench_image_encoder.py needs Pillow as its yardstick")
    if args.format == "png":
        return main_png(args)
    import torch
    from scannertools_amd import _native
    from scannertools_amd.hip import HipContext, jpeg_encode_bound
    L = _native.lib()
    ctx = HipContext(0)
    host = make_frames()
    dev = [torch.from_numpy(f).cuda() for f in host]

    # a mode is (restart, optimised tables); without --optimize the modes and their keys are what they always were
    modes = [(r, o) for r in (("row", "none") if args.restart == "both" else (args.restart,))
             for o in {"off": (False,), "on": (True,), "both": (False, True)}[args.optimize]]
    if any(o for _, o in modes):
        from PIL import ImageFile
        ImageFile.MAXBLOCK = max(ImageFile.MAXBLOCK, 1 << 24)   # optimize=True saves need the whole stream in one block

    def pillow(i, mode=("row", False)):
        buf = io.BytesIO()
        kw = {"restart_marker_rows": 1} if mode[0] == "row" else {}
        if mode[1]:
            kw["optimize"] = True
        Image.fromarray(host[i % DISTINCT]).save(buf, "JPEG", quality=QUALITY, subsampling=SUBSAMPLING, **kw)
        return buf.getvalue()

    for mode in modes:
        assert ctx.encode_jpeg([dev[0]], QUALITY, SUBSAMPLING, restart=mode[0], optimize=mode[1])[0] == pillow(0, mode), \
            "the stream differs from Pillow's (restart=%s, optimize=%s)" % mode
    result = {"bench": "image_encoder", "h": H, "w": W, "quality": QUALITY, "sampling": SUBSAMPLING, "raw_frame_bytes": H * W * 3,
              "bound_bytes": jpeg_encode_bound(H, W, SUBSAMPLING), "rounds": args.rounds}
    keys = {("row", False): "batches", ("none", False): "batches_norst", ("row", True): "batches_opt", ("none", True): "batches_norst_opt"}
    for mode in modes:
        result[keys[mode]] = {}
    ctx._bind()
    for n in BATCHES:
        tab = (ctypes.c_void_p * n)(*[dev[i % DISTINCT].data_ptr() for i in range(n)])
        sizes = (ctypes.c_size_t * n)()
        store = np.empty((n, 1 << 22), np.uint8)   # no 1080p stream of these frames reaches 4 MiB; pages are touched only where written
        bufs = (ctypes.c_void_p * n)(*[store[i].ctypes.data for i in range(n)])

        def call(mode):
            if mode[1]:
                ctx._check(L.st_jpeg_encode_batch_opt(ctx._h, tab, n, H, W, QUALITY, 2, 2, 0 if mode[0] == "row" else 1, 1))
            elif mode[0] == "row":
                ctx._check(L.st_jpeg_encode_batch(ctx._h, tab, n, H, W, QUALITY, 2, 2))
            else:
                ctx._check(L.st_jpeg_encode_batch_rst(ctx._h, tab, n, H, W, QUALITY, 2, 2, 1))
            ctx._check(L.st_jpeg_encode_fetch(ctx._h, bufs, sizes, store.shape[1]))

        if args.trace:
            for mode in modes:
                for _ in range(3):
                    call(mode)
            continue
        times, stream_bytes = {m: [] for m in modes}, {}
        for mode in modes:
            call(mode)   # warm-up: workspace, stream buffer and staging grow here
            stream_bytes[mode] = int(statistics.mean(sizes))
        for _ in range(args.rounds):   # the modes' timed calls alternate
            for mode in modes:
                t0 = time.perf_counter()
                call(mode)
                times[mode].append(time.perf_counter() - t0)
        for mode in modes:
            t = times[mode]
            b = {"fps_median": round(n / statistics.median(t), 1), "fps_min": round(n / max(t), 1), "fps_max": round(n / min(t), 1),
                 "stream_bytes_per_frame": stream_bytes[mode]}
            ctx.timing_enable([_native.K_JPEG])
            ctx.timing_reset()
            for _ in range(args.rounds):
                call(mode)
            launches, ms = ctx.timing_read(_native.K_JPEG)
            ctx.timing_enable([])
            b["kernel_ms_per_frame"] = round(ms / (args.rounds * n), 4)
            b["kernel_launches_per_call"] = launches // args.rounds
            with ThreadPoolExecutor(THREADS) as pool:
                list(pool.map(lambda i: pillow(i, mode), range(n)))
                t = []
                for _ in range(max(3, args.rounds // 2)):
                    t0 = time.perf_counter()
                    list(pool.map(lambda i: pillow(i, mode), range(n)))
                    t.append(time.perf_counter() - t0)
            b["pillow_%d_threads_fps_median" % THREADS] = round(n / statistics.median(t), 1)
            b["pillow_fps_min"], b["pillow_fps_max"] = round(n / max(t), 1), round(n / min(t), 1)
            result[keys[mode]]["batch%d" % n] = b
        del store
    ctx.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
