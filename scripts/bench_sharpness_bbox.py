"""SharpnessBBox on the MI355X: the fused entry point against the same results composed from the older entry points.
Prints one JSON line.

Resident 1080p frames at batch 1, 8 and 32 with 1, 4 and 16 boxes per frame; box sides drawn (seeded) from {64, 200, 400, 720}
plus the whole frame.  Per cell:
  (a) one st_bbox_sharpness_u8c3_strided call for all boxes of all frames (HipContext.bbox_sharpness, kind SharpnessCPP);
  (b) per box: a crop copy into a dense buffer (torch), st_resize_u8_batch to 200 x 200, st_frame_moments_u8c3_batch
      (Laplacian only) and st_frame_stats_finish, every buffer allocated beforehand.  None of these is touched by the
      SharpnessBBox change, so (b) is what the same result cost before it.
Both are warmed up, then timed with device events around windows of repeated calls, the two sides alternating; the figure is
the median window divided by its calls.  The results of (a) and (b) are compared bit for bit before anything is timed.

    python scripts/bench_sharpness_bbox.py [--rounds 5]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_sharpness_bbox.py --trace

--trace makes three calls per side and cell and times nothing: under rocprofv3 the kernel statistics then hold, over the same
work on both sides, k_bbox_moments for (a) and the copy, resize, moments and finishing kernels for (b).  A kernel-trace
duration leaves out launch gaps and host time, which are most of (b); the event figures include them.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

H, W = 1080, 1920
SIDES = (64, 200, 400, 720)


def draw_boxes(rng, n, per_frame):
    recs = []
    for f in range(n):
        for _ in range(per_frame):
            k = int(rng.integers(0, len(SIDES) + 1))
            if k == len(SIDES):
                recs.append((f, 0, 0, W, H))
                continue
            s = SIDES[k]
            x1, y1 = int(rng.integers(0, W - s + 1)), int(rng.integers(0, H - s + 1))
            recs.append((f, x1, y1, x1 + s, y1 + s))
    return np.array(recs, np.int64)


class Composed:
    """(b): the older entry points, one box at a time, with every buffer allocated beforehand."""

    def __init__(self, ctx, frames, recs):
        from scannertools_amd import _native
        self.ctx, self.frames, self.recs = ctx, frames, recs
        self.crops = [torch.empty((y2 - y1, x2 - x1, 3), dtype=torch.uint8, device="cuda") for _, x1, y1, x2, y2 in recs]
        self.img = torch.empty((1, 200, 200, 3), dtype=torch.uint8, device="cuda")
        self.mom = torch.empty((1, 8), dtype=torch.int64, device="cuda")
        self.out = torch.empty(len(recs), dtype=torch.float32, device="cuda")
        self.finish = _native.lib().st_frame_stats_finish
        self.kind = _native.FS_KINDS["SharpnessCPP"]

    def __call__(self):
        ctx = self.ctx
        for i, (f, x1, y1, x2, y2) in enumerate(self.recs):
            self.crops[i].copy_(self.frames[f, y1:y2, x1:x2])
            ctx.resize([self.crops[i]], 200, 200, out=self.img)
            ctx.frame_moments(self.img, luma=False, laplacian=True, out=self.mom)
            ctx._check(self.finish(ctx._h, ctypes.c_void_p(self.mom.data_ptr()), 1, 200, 200, self.kind,
                                   ctypes.c_void_p(self.out.data_ptr() + 4 * i)))
        return self.out


def window_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace", action="store_true", help="three calls per side and cell, no timing (for rocprofv3)")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.ensure_built()
    from scannertools_amd.hip import HipContext
    assert torch.cuda.is_available(), "bench_sharpness_bbox needs a GPU"
    gen = torch.Generator(device="cuda").manual_seed(0)
    frames = torch.randint(0, 256, (32, H, W, 3), dtype=torch.uint8, device="cuda", generator=gen)
    rng = np.random.default_rng(0)
    cells = []
    with HipContext(0) as ctx:
        for n in (1, 8, 32):
            for per in (1, 4, 16):
                recs = draw_boxes(rng, n, per)
                d = frames[:n]
                new = lambda: ctx.bbox_sharpness(d, recs, "SharpnessCPP")   # noqa: E731
                old = Composed(ctx, d, recs.tolist())
                va, vb = new().cpu().numpy(), old().cpu().numpy().copy()
                assert (va.view(np.uint32) == vb.view(np.uint32)).all(), "fused and composed results differ"
                if a.trace:
                    for _ in range(3):
                        new()
                        old()
                    torch.cuda.synchronize()
                    cells.append({"batch": n, "boxes_per_frame": per, "boxes": len(recs)})
                    continue
                for _ in range(3):
                    new()
                    old()
                torch.cuda.synchronize()
                # windows of about 50 ms each
                ca = max(5, min(2000, int(50.0 / max(window_ms(new, 5), 1e-3))))
                cb = max(3, min(500, int(50.0 / max(window_ms(old, 3), 1e-3))))
                ta, tb = [], []
                for _ in range(a.rounds):
                    ta.append(window_ms(new, ca))
                    tb.append(window_ms(old, cb))
                ma, mb = statistics.median(ta), statistics.median(tb)
                cells.append({"batch": n, "boxes_per_frame": per, "boxes": len(recs), "fused_us": round(ma * 1e3, 1),
                              "composed_us": round(mb * 1e3, 1), "composed_over_fused": round(mb / ma, 2),
                              "fused_us_min_max": [round(min(ta) * 1e3, 1), round(max(ta) * 1e3, 1)],
                              "composed_us_min_max": [round(min(tb) * 1e3, 1), round(max(tb) * 1e3, 1)],
                              "calls_per_window": [ca, cb]})
    print(json.dumps({"frame": [H, W], "rounds": a.rounds, "trace": a.trace, "cells": cells}))


if __name__ == "__main__":
    main()
