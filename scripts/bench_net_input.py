"""FacenetInput and CaffeInput kernel time on device-resident 1080p frames at batch 1 / 8 / 32: FacenetInput at scales 0.5
and 1.0, CaffeInput to 224 x 224 and 300 x 300.  Prints one JSON line.  Time is the library's own event pair around each
launch (ST_K_NET_INPUT; median over the repetitions), so it holds the kernel and not the Python call.  Every op is set
against its byte model -- 3 h w bytes read plus 12 net_h net_w written -- as a share of 8 TB/s, and against two yardsticks
measured in the same run on the same frames, each in its own byte model: st_cpm2_input_batch (3 h w + 12 net_h net_w at its
own geometry) and st_resize_u8_batch INTER_LINEAR to the same size (3 h w + 3 net_h net_w).

    python scripts/bench_net_input.py [--batch 1,8,32] [--reps 20]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from scannertools_amd import _native
from scannertools_amd.hip import HipContext, cpm2_geometry, facenet_geometry

H, W = 1080, 1920
PEAK = 8e12   # bytes per second
MEAN = (104.00699, 116.66877, 122.67892)


def kernel_ms(ctx, kernel_id, call, reps):
    """Median per-call kernel time in ms of `call`, from the library's events for `kernel_id`."""
    ctx.timing_enable([kernel_id])
    try:
        for _ in range(3):
            call()
        samples = []
        for _ in range(reps):
            ctx.timing_reset()
            call()
            launches, ms = ctx.timing_read(kernel_id)
            assert launches == 1, launches
            samples.append(ms)
    finally:
        ctx.timing_enable([])
    return statistics.median(samples)


def row(name, n, ms, bytes_per_frame, **extra):
    bps = n * bytes_per_frame / (ms * 1e-3)
    return dict(op=name, batch=n, kernel_ms=round(ms, 4), bytes_per_frame=bytes_per_frame, TBps=round(bps / 1e12, 3),
                share_of_8TBps=round(bps / PEAK, 3), **extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="1,8,32")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    ctx = HipContext(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    results = []
    for n in [int(x) for x in a.batch.split(",")]:
        frames = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
        for scale in (0.5, 1.0):
            nh, nw = facenet_geometry(H, W, scale)
            out = torch.empty((n, 3, nw, nh), dtype=torch.float32, device="cuda")
            ms = kernel_ms(ctx, _native.K_NET_INPUT, lambda: ctx.facenet_input(frames, scale, MEAN, out=out), a.reps)
            r = row("FacenetInput", n, ms, 3 * H * W + 12 * nh * nw, scale=scale, net=[nh, nw])
            _, _, ch, cw = cpm2_geometry(H, W, scale)
            cout = torch.empty((n, 3, ch, cw), dtype=torch.float32, device="cuda")
            cms = kernel_ms(ctx, _native.K_CPM2_INPUT, lambda: ctx.cpm2_input(frames, scale, out=cout), a.reps)
            c = row("CPM2Input", n, cms, 3 * H * W + 12 * ch * cw, scale=scale, net=[ch, cw])
            rout = torch.empty((n, nh, nw, 3), dtype=torch.uint8, device="cuda")
            rms = kernel_ms(ctx, _native.K_RESIZE, lambda: ctx.resize(frames, nw, nh, out=rout), a.reps)
            rr = row("Resize INTER_LINEAR", n, rms, 3 * H * W + 3 * nh * nw, net=[nh, nw])
            r["bytes_per_s_vs_cpm2_input"] = round(r["TBps"] / c["TBps"], 3) if c["TBps"] else None
            results += [r, c, rr]
            del out, cout, rout
        for side in (224, 300):
            out = torch.empty((n, 3, side, side), dtype=torch.float32, device="cuda")
            ms = kernel_ms(ctx, _native.K_NET_INPUT, lambda: ctx.caffe_input(frames, side, side, MEAN, out=out), a.reps)
            r = row("CaffeInput", n, ms, 3 * H * W + 12 * side * side, net=[side, side])
            r["source_read_once_ms_at_8TBps"] = round(n * 3 * H * W / PEAK * 1e3, 4)
            rout = torch.empty((n, side, side, 3), dtype=torch.uint8, device="cuda")
            rms = kernel_ms(ctx, _native.K_RESIZE, lambda: ctx.resize(frames, side, side, out=rout), a.reps)
            results += [r, row("Resize INTER_LINEAR", n, rms, 3 * H * W + 3 * side * side, net=[side, side])]
            del out, rout
        del frames
    print(json.dumps({"bench": "net_input", "frame": [H, W], "timing": "library events per launch, median of %d" % a.reps,
                      "results": results}))
    ctx.close()


if __name__ == "__main__":
    main()
