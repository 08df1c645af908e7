"""Frame statistics throughput (BrightnessCPP / ContrastCPP / SharpnessCPP and their Python twins) on the MI355X.  Prints one
JSON line.

1. The moments kernel on device-resident 1080p frames at batch 1, 32 and 256, through both entry points (strided stream and
   per-frame pointer table), luma + Laplacian: frames/s from the host clock around repeated calls that end in a device
   synchronise, and kernel time from the library's dispatch events (st_ctx_timing_*, ST_K_FRAME_STATS).  Algorithmic bytes per
   call: 6 220 800 per frame plus the halo rows the bands re-read (two rows of 5 760 B per band boundary); the fraction is of
   8 TB/s.
2. The three C++ ops through the GPU kernel class (device frames) and the staged CPU kernel class (host frames uploaded),
   batch 32: frames/s from the engine's execute() time.

    python scripts/bench_frame_stats.py [--reps 20]
"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

H, W = 1080, 1920
FRAME_BYTES = 3 * H * W
PEAK = 8.0e12


def halo_bytes(ctx_num_cus, n):
    """Bytes the bands re-read above and below themselves (the band plan of st_framestats.hip: fm_band_rows)."""
    target = 4 * ctx_num_cus
    rows = max(4, -(-n * H // target))
    rows = min(rows, (510 * 6144) // (3 * W), H)
    bands = -(-H // rows)
    return n * (2 * (bands - 1)) * 3 * W


def bench_moments(ctx, frames, n, entry, reps):
    from scannertools_amd import _native
    d = frames[:n]
    arg = list(d.unbind(0)) if entry == "batch" else d
    out = torch.empty((n, 8), dtype=torch.int64, device="cuda")
    for _ in range(3):
        ctx.frame_moments(arg, out=out)
    torch.cuda.synchronize()
    ctx.timing_enable([_native.K_FRAME_STATS])
    ctx.timing_reset()
    t0 = time.perf_counter()
    for _ in range(reps):
        ctx.frame_moments(arg, out=out)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / reps
    launches, ms = ctx.timing_read(_native.K_FRAME_STATS)
    ctx.timing_enable([])
    kern = ms / 1e3 / reps
    algo = n * FRAME_BYTES + halo_bytes(256, n)
    return {"entry": entry, "batch": n, "frames_per_s": round(n / wall, 1), "call_us": round(wall * 1e6, 1),
            "kernel_us": round(kern * 1e6, 1), "launches_per_call": launches / reps,
            "kernel_TBps": round(algo / kern / 1e12, 3), "fraction_of_8TBps": round(algo / kern / PEAK, 3)}


def bench_op(op, device, frames_np, frames_dev, batch, n):
    from scannertools_amd import engine
    from scannertools_amd.engine import DeviceType
    L = engine._imgproc()
    err = ctypes.create_string_buffer(512)
    k = L.stshim_kernel_create(op.encode(), device, 0, b"", 0, err, 512)
    if not k:
        raise RuntimeError(err.value.decode())
    try:
        if device == DeviceType.GPU:
            ptrs = [frames_dev[i % frames_dev.shape[0]].data_ptr() for i in range(n)]
        else:
            ptrs = [frames_np[i % frames_np.shape[0]].ctypes.data for i in range(n)]
        best = None
        for rep in range(3):
            torch.cuda.synchronize()
            res = L.stshim_run_frames(k, (ctypes.c_void_p * n)(*ptrs), n, H, W, 3, 0, batch, (ctypes.c_int * 1)(0), 1, err, 512)
            secs = L.stshim_last_execute_seconds()
            if not res or err.value:
                raise RuntimeError(err.value.decode())
            L.stshim_outputs_free(res)
            if rep:
                best = secs if best is None else min(best, secs)
    finally:
        L.stshim_kernel_destroy(k)
    return {"op": op, "device": "GPU" if device == DeviceType.GPU else "CPU (staged)", "batch": batch, "frames": n,
            "frames_per_s": round(n / best, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.ensure_built()
    from scannertools_amd.engine import DeviceType
    from scannertools_amd.hip import HipContext
    assert torch.cuda.is_available(), "bench_frame_stats needs a GPU"
    gen = torch.Generator(device="cuda").manual_seed(0)
    frames = torch.randint(0, 256, (256, H, W, 3), dtype=torch.uint8, device="cuda", generator=gen)
    res = {"moments": [], "ops": []}
    with HipContext(0) as ctx:
        for entry in ("strided", "batch"):
            for n in (1, 32, 256):
                res["moments"].append(bench_moments(ctx, frames, n, entry, a.reps))
    host = frames[:32].cpu().numpy()
    for op in ("BrightnessCPP", "ContrastCPP", "SharpnessCPP"):
        res["ops"].append(bench_op(op, DeviceType.GPU, host, frames, 32, 256))
        res["ops"].append(bench_op(op, DeviceType.CPU, host, frames, 32, 64))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
