"""FacenetOutput on the MI355X: kernel time of st_facenet_output_batch from the library's own events, beside the byte model
and the numpy restatement on the host.  Prints one JSON line.

1080p frames at scale 0.5 (network input 960 x 544, grid 120 x 68, 122 400 candidates per frame), batch 1, 8 and 32, on maps
drawn (seeded) so that about 0, 100 and 5 000 candidates per frame pass the threshold 0.5.  Per cell:
  kernel_us_per_frame   the decode, sort + suppression and pack launches (timing slot cpm2_nms), median over the rounds of
                        the sum over a window of calls, per call and frame;
  call_us_per_frame     the whole call as the host sees it (both copies to the host and the synchronisations included);
  model_us_per_frame    15 * G * 4 bytes -- the valid confidence planes, all that a frame without survivors has to read -- at
                        8 TB/s;
  numpy_ms_per_frame    tests/ref_facenet_output_np.py on one frame on the host.
The first frame of every cell is compared with the restatement bit for bit before anything is timed.

    python scripts/bench_facenet_output.py [--rounds 5] [--calls 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

H, W, SCALE, THRESHOLD = 1080, 1920, 0.5, 0.5
# logit bias -> expected survivors of 122 400 normal(bias, 1) logits above 0
BIASES = {"0": -30.0, "100": -3.15, "5000": -1.74}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.ensure_built()
    import ref_facenet_output_np as ref
    from scannertools_amd import _native
    from scannertools_amd.hip import HipContext
    assert torch.cuda.is_available(), "bench_facenet_output needs a GPU"
    _, _, gh, gw = ref.geometry(H, W, SCALE)
    G = gw * gh
    T = ref.templates()
    cells = []
    with HipContext(0) as ctx:
        for label, bias in BIASES.items():
            maps = np.stack([ref.make_map(1000 + i, gw, gh, bias) for i in range(32)])
            t0 = time.perf_counter()
            survivors, _, _ = ref.decode(maps[0], H, W, SCALE, T, THRESHOLD)
            want = survivors[ref.nms(survivors)]
            numpy_ms = (time.perf_counter() - t0) * 1e3
            dev = torch.from_numpy(maps).cuda()
            for n in (1, 8, 32):
                d = dev[:n]
                got = ctx.facenet_output(d, H, W, SCALE, T, THRESHOLD)
                assert got[0].shape == want.shape and (got[0].view(np.uint32) == want.view(np.uint32)).all(), "library and restatement differ"
                ctx.timing_enable([_native.K_CPM2_NMS])
                kernel, wall = [], []
                for _ in range(a.rounds):
                    ctx.timing_reset()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.calls):
                        ctx.facenet_output(d, H, W, SCALE, T, THRESHOLD)
                    wall.append((time.perf_counter() - t0) / a.calls)
                    kernel.append(ctx.timing_read(_native.K_CPM2_NMS)[1] / a.calls)
                ctx.timing_enable([])
                cells.append({"survivors_target": label, "survivors_frame0": int(len(survivors)), "kept_frame0": int(len(want)),
                              "kept_mean": round(float(np.mean([len(r) for r in got])), 1), "batch": n,
                              "kernel_us_per_frame": round(statistics.median(kernel) * 1e3 / n, 2),
                              "kernel_us_min_max": [round(min(kernel) * 1e3 / n, 2), round(max(kernel) * 1e3 / n, 2)],
                              "call_us_per_frame": round(statistics.median(wall) * 1e6 / n, 1),
                              "model_us_per_frame": round(15 * G * 4 / 8e12 * 1e6, 3),
                              "numpy_ms_per_frame": round(numpy_ms, 2)})
    print(json.dumps({"frame": [H, W], "scale": SCALE, "grid": [gw, gh], "candidates": 15 * G, "threshold": THRESHOLD,
                      "rounds": a.rounds, "calls": a.calls, "cells": cells}))


if __name__ == "__main__":
    main()
