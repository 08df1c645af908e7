"""Montage throughput through the GPU kernel class (MontageKernelHIP, run by the op library's engine) on device-resident
1080p frames -> target_width 240 (135-row tiles), 8 per row, for num_frames 64 / 1000 at batch 1 / 32.  Prints one JSON
line.  Time is the host clock around every execute() -- each ends in a device synchronise -- summed by the engine.
Bandwidth counts what the resize must move per frame: about two source rows per output row read (270 x 5760 B) and the
tile written (97 200 B).

    python scripts/bench_montage.py [--frames 64,1000] [--batch 1,32] [--reps 3]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from scannertools_amd import _proto, engine
from scannertools_amd.engine import DeviceType

H, W, TW, FPR = 1080, 1920, 240, 8
TH = int(TW / (1.0 * W) * H)
BYTES_PER_FRAME = 2 * TH * W * 3 + TH * TW * 3   # 270 x 5760 B read + 97 200 B written


def run_once(L, frames, num_frames, batch):
    args = _proto.encode([(1, "int64", num_frames), (4, "int32", TW), (6, "int32", FPR)])
    err = ctypes.create_string_buffer(512)
    k = L.stshim_kernel_create(b"Montage", DeviceType.GPU, 0, args, len(args), err, 512)
    if not k:
        raise RuntimeError(err.value.decode())
    try:
        ptrs = [frames[i % frames.shape[0]].data_ptr() for i in range(num_frames)]
        torch.cuda.synchronize()
        res = L.stshim_run_frames(k, (ctypes.c_void_p * num_frames)(*ptrs), num_frames, H, W, 3, 0, batch,
                                  (ctypes.c_int * 1)(0), 1, err, 512)
        secs = L.stshim_last_execute_seconds()
        if not res or err.value:
            raise RuntimeError(err.value.decode())
        L.stshim_outputs_free(res)
    finally:
        L.stshim_kernel_destroy(k)
    return secs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="64,1000")
    ap.add_argument("--batch", default="1,32")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    L = engine._imgproc()
    g = torch.Generator(device="cuda").manual_seed(0)
    # 64 distinct frames; longer streams cycle through them (the kernel reads every frame anyway)
    frames = torch.randint(0, 256, (64, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    results = []
    for nf in [int(x) for x in a.frames.split(",")]:
        for b in [int(x) for x in a.batch.split(",")]:
            run_once(L, frames, nf, b)   # warm-up: first allocations, code object load
            best = min(run_once(L, frames, nf, b) for _ in range(a.reps))
            results.append({"num_frames": nf, "batch": b, "seconds": round(best, 6),
                            "frames_per_s": round(nf / best, 1), "achieved_GBps": round(nf * BYTES_PER_FRAME / best / 1e9, 1)})
    print(json.dumps({"bench": "montage", "frame": [H, W], "target_width": TW, "tile_height": TH, "frames_per_row": FPR,
                      "bytes_per_frame": BYTES_PER_FRAME, "timing": "host clock around execute(), best of %d" % a.reps,
                      "results": results}))


if __name__ == "__main__":
    main()
