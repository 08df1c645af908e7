"""The Caffe op's forward pass on the MI355X: VGG-16 and bvlc_googlenet topologies at 224 x 224 with random weights (written to a
temporary directory), batches of 1, 8 and 32.  Prints a table and one JSON line.

Per network and batch, from the library's ST_K_CONV dispatch events (scannertools_caffe_time_net: one warm-up pass, then `reps`
passes timed whole and `reps` passes timed layer by layer):
  frames/s        batch / median kernel time of a whole pass, with the scatter (max - min) / median over the passes
  InnerProduct    the layers' median kernel time next to the time of reading the same weight bytes ONCE at the rate of the
                  project's streaming-read micro-benchmark (scripts/ubench/stream_read.hip, compiled and run here: the best
                  non-temporal rate over 64 frames = 398 MB, the size of VGG-16's fc6)
  convolutions    the MFMA convolutions' FLOP / their median kernel time, next to the pose network's 121 TFLOP/s (DESIGN.md
                  section 4.9); the direct kernel's layers (GoogLeNet's 7 x 7 / 2) separately

    python scripts/bench_caffe_net.py [--reps 7] [--runs 2] [--nets vgg16,googlenet]
"""
import argparse
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

POSE_TFLOPS = 121.0


def stream_rate(tmp):
    """GB/s of scripts/ubench/stream_read.hip reading 64 frames (398 MB) once: the best of its workgroup counts, non-temporal."""
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ubench", "stream_read.hip")
    exe = os.path.join(tmp, "stream_read")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", src, "-o", exe])
    out = subprocess.check_output([exe], text=True, timeout=120)
    rates = [float(m.group(1)) for m in re.finditer(r"frames\s+64\s+wg\s+\d+\s+nt 1 :\s+[\d.]+ us per launch\s+(\d+) GB/s", out)]
    return max(rates)


def time_net(L, prototxt, caffemodel, n, reps):
    total = (ctypes.c_double * reps)()
    steps = (ctypes.c_double * 512)()
    names = ctypes.create_string_buffer(1 << 16)
    err = ctypes.create_string_buffer(1024)
    ns = L.scannertools_caffe_time_net(prototxt.encode(), caffemodel.encode(), b"prob", 0, n, reps, total, steps, 512, names, 1 << 16, err, 1024)
    if ns < 0:
        raise RuntimeError(err.value.decode())
    return list(total), dict(zip(names.value.decode().split("\n")[:ns], list(steps)[:ns]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--nets", default="vgg16,googlenet")
    args = ap.parse_args()
    import __graft_entry__ as g
    g.ensure_built()
    from scannertools_amd import caffe_net, engine
    L = engine._caffe()
    L.scannertools_caffe_time_net.restype = ctypes.c_int
    L.scannertools_caffe_time_net.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                              ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.c_char_p,
                                              ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    result = {"reps": args.reps, "runs": args.runs, "nets": {}}
    with tempfile.TemporaryDirectory() as tmp:
        result["stream_read_GBps"] = stream_rate(tmp)
        for name in args.nets.split(","):
            net, _ = getattr(caffe_net, name)(seed=1)
            prototxt, caffemodel = net.write(tmp)
            convs = {l["name"]: l for l in net.layers if l["type"] == "Convolution"}
            fcs = {l["name"]: l for l in net.layers if l["type"] == "InnerProduct"}
            rows = []
            for run in range(args.runs):
                for n in (1, 8, 32):
                    total, steps = time_net(L, prototxt, caffemodel, n, args.reps)
                    med = statistics.median(total)
                    mfma_flop = mfma_ms = direct_flop = direct_ms = 0.0
                    for cname, l in convs.items():
                        p = l["convolution_param"]
                        k, s, pad, grp = p["kernel_size"], p.get("stride", 1), p.get("pad", 0), p.get("group", 1)
                        cin = net.shapes[l["bottom"][0]][0]
                        co, oh, ow = net.shapes[l["top"][0]]
                        flop = 2.0 * n * co * oh * ow * (cin // grp) * k * k
                        if s == 1 and k % 2 and k <= 7 and 2 * pad + 1 == k and grp == 1:
                            mfma_flop += flop
                            mfma_ms += steps[cname]
                        else:
                            direct_flop += flop
                            direct_ms += steps[cname]
                    ip = {}
                    for fname, l in fcs.items():
                        nbytes = net.weights[fname][0].size * 4
                        floor_ms = nbytes / (result["stream_read_GBps"] * 1e9) * 1e3
                        ip[fname] = {"weight_MB": round(nbytes / 1e6, 1), "ms": round(steps[fname], 4), "stream_once_ms": round(floor_ms, 4),
                                     "ratio": round(steps[fname] / floor_ms, 2)}
                    rows.append({"run": run, "batch": n, "pass_ms_median": round(med, 3), "scatter": round((max(total) - min(total)) / med, 4),
                                 "frames_per_s": round(n / med * 1e3, 1), "mfma_conv_TFLOPs": round(mfma_flop / mfma_ms / 1e9, 1),
                                 "mfma_conv_share_of_pose_rate": round(mfma_flop / mfma_ms / 1e9 / POSE_TFLOPS, 3),
                                 "mfma_conv_ms": round(mfma_ms, 3),
                                 "direct_conv_TFLOPs": round(direct_flop / direct_ms / 1e9, 2) if direct_ms else None,
                                 "direct_conv_ms": round(direct_ms, 3), "inner_product": ip,
                                 "other_ms": round(sum(steps.values()) - mfma_ms - direct_ms - sum(v["ms"] for v in ip.values()), 3)})
                    r = rows[-1]
                    print("%-9s run %d batch %2d: %8.1f frames/s (pass %.3f ms, scatter %.1f %%)  MFMA conv %.1f TFLOP/s (%.2f of pose)  direct conv %s ms  "
                          "InnerProduct %s" % (name, run, n, r["frames_per_s"], r["pass_ms_median"], 100 * r["scatter"], r["mfma_conv_TFLOPs"],
                                               r["mfma_conv_share_of_pose_rate"], r["direct_conv_ms"],
                                               ", ".join("%s %.3f ms = %.2f x stream" % (k, v["ms"], v["ratio"]) for k, v in ip.items())), flush=True)
            result["nets"][name] = rows
            os.remove(caffemodel)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
