"""CPU: host logic (ShotBoundaries, wire readers, sharding) and the C-ABI surface."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "shot_golden.npz"))
CASES = sorted({k.rsplit("__", 1)[0] for k in GOLD.files})


# ---- ShotBoundaries (product) vs the reference's golden outputs: bit-exact ----------------------
@pytest.mark.parametrize("case", CASES)
def test_shot_boundaries_matches_reference_golden(case):
    from scannertools_amd.shot_detection import shot_boundaries
    h = GOLD[case + "__hist"]
    frames = [[np.array(h[i, j]) for j in range(3)] for i in range(len(h))]   # wire format of types.histograms
    res = shot_boundaries(None, frames)
    assert len(res) == len(h)
    assert res[0] == GOLD[case + "__bounds"].tolist()
    assert all(r is None for r in res[1:])                                     # shot_detection.py:28


def test_shot_boundaries_contract_and_constants():
    import scannertools_amd as sa
    assert sa.WINDOW_SIZE == 500 and sa.BOUNDARY_BATCH == 10000000
    one = [[np.zeros(16, np.int32)] * 3]
    assert sa.shot_boundaries(None, one) == [[]]
    with pytest.raises(ValueError):
        sa.shot_boundaries(None, [np.zeros((2, 16), np.int32)] * 4)


def _outlier_boundaries_loop(diffs):
    """Per-window evaluation of the outlier rule (what shot_detection.py:21-26 does row by row):
    the cross-check of the product's strided, vectorised evaluation."""
    W, n = 500, len(diffs)
    out = []
    for i in range(1, n):
        window = diffs[max(i - W, 0):min(i + W, n)]
        if diffs[i] - np.mean(window) > 2.5 * np.std(window):
            out.append(i)
    return out


def test_vectorised_window_statistics_equal_the_reference_loop():
    from scannertools_amd.shot_detection import outlier_boundaries
    rng = np.random.default_rng(0)
    for trial in range(25):
        n = int(rng.integers(1, 3500)) if trial < 22 else (999, 1000, 1001)[trial - 22]
        d = np.abs(rng.standard_normal(n)) * float(rng.integers(1, 1000)) / 3.0
        if n > 5:
            d[rng.integers(0, n, 5)] *= 50
        d[0] = 0
        assert outlier_boundaries(d) == _outlier_boundaries_loop(d), (trial, n)
    assert outlier_boundaries(np.zeros(0)) == [] and outlier_boundaries(np.zeros(1)) == []


def test_histogram_diffs_is_chebyshev_mean():
    from scipy.spatial import distance
    from scannertools_amd.shot_detection import histogram_diffs
    h = np.random.default_rng(0).integers(0, 5000, (40, 3, 16)).astype(np.int32)
    ref = [0.0] + [np.mean([distance.chebyshev(h[i - 1][j], h[i][j]) for j in range(3)]) for i in range(1, 40)]
    np.testing.assert_array_equal(histogram_diffs(h), np.array(ref))


def test_wire_readers():
    from scannertools_amd import types
    h = np.arange(48, dtype=np.int32)
    parts = types.histograms(h.tobytes())
    assert len(parts) == 3 and all(p.dtype == np.int32 and p.shape == (16,) for p in parts)
    np.testing.assert_array_equal(np.concatenate(parts), h)
    assert types.histograms(None) is None
    f = np.arange(2 * 3 * 2, dtype=np.float32)
    assert types.flow(f.tobytes(), 2, 3).shape == (2, 3, 2) and types.flow(None, 2, 3) is None


# ---- sharding -----------------------------------------------------------------------------------
def test_shard_ranges_cover_and_halo():
    from scannertools_amd.sharding import flow_shard, local_pairs, shard_range
    for n in (0, 1, 7, 10000, 10001):
        for world in (1, 2, 3, 8):
            rs = [shard_range(n, r, world) for r in range(world)]
            assert rs[0][0] == 0 and rs[-1][1] == n
            assert all(rs[i][1] == rs[i + 1][0] for i in range(world - 1))
            assert max(e - s for s, e in rs) - min(e - s for s, e in rs) <= 1
    rows, frames = flow_shard(10000, 3, 8)
    assert rows == (3750, 5000) and frames == (3750, 5001)          # one halo frame
    rows, frames = flow_shard(10000, 7, 8)
    assert frames == (8750, 10000)                                   # last shard: edge clamp, no halo
    p = local_pairs(rows, frames, 10000)
    assert p[0].tolist() == [0, 1] and p[-1].tolist() == [1249, 1249]  # last row pairs the last frame with itself
    rows, frames = flow_shard(100, 1, 4, stencil=(-1, 0))
    assert rows == (25, 50) and frames == (24, 50)


def test_two_rank_gloo_shot_pipeline(tmp_path):
    """world_size 2 over gloo on CPU: shard -> gather on rank 0 -> ShotBoundaries == single-process."""
    out = str(tmp_path / "b.npy")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29571")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29571", os.path.join(ROOT, "tests", "_dist_worker.py"), out, "1000"]
    subprocess.run(cmd, check=True, env=env, timeout=300, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    assert np.load(out).tolist() == GOLD["s0_n1000_b16__bounds"].tolist()


def test_bench_starts_its_own_ranks(tmp_path):
    """`python bench.py --gpus 2` must start two ranks itself (the parent never touches the GPU) and
    relay rank 0's line; exercised on CPU with --dry-run (gloo rendezvous, barriers and the
    max-over-ranks reduction around a dummy step).  A WORLD_SIZE that contradicts --gpus is an error."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run", "--steps", "3"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["dry_run"] is True and line["steps"] == 3
    assert line["ms_per_step"] >= 2.0                 # the slower rank (2 ms per dummy step) sets the time
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run"],
                         env=dict(env, WORLD_SIZE="1"), capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "WORLD_SIZE" in bad.stderr


def test_bench_dump_outputs(tmp_path):
    """bench.py --dump-outputs: the whole output when it fits, otherwise the first / last pairs' fields, a seeded choice of
    further pairs and flow vectors at seeded positions over all pairs; float32, within the budget, the same every run."""
    import torch
    import bench
    g = torch.Generator().manual_seed(0)
    hist = torch.randint(0, 1 << 21, (4, 3, 256), dtype=torch.int32, generator=g)
    small = torch.randn((4, 30, 40, 2), generator=g)
    d = bench.dump_outputs(torch, str(tmp_path / "small"), small, hist)
    assert d["files"] == {"histogram": [4, 3, 256], "flow": [4, 30, 40, 2]}
    np.testing.assert_array_equal(np.load(tmp_path / "small" / "flow.npy"), small.numpy())
    h_got = np.load(tmp_path / "small" / "histogram.npy")
    assert h_got.dtype == np.float32 and np.array_equal(h_got.astype(np.int64), hist.numpy())

    B, h, w = 40, 480, 640                        # 98 MB of flow: over the budget, so sampled
    big = torch.randn((B, h, w, 2), generator=g)
    runs = [bench.dump_outputs(torch, str(tmp_path / ("big%d" % i)), big, hist) for i in range(2)]
    assert {k: v for k, v in runs[0].items() if k != "dir"} == {k: v for k, v in runs[1].items() if k != "dir"}
    d = runs[0]
    assert set(d["files"]) == {"histogram", "flow_pairs", "flow_points"}
    assert sum(os.path.getsize(tmp_path / "big0" / f) for f in os.listdir(tmp_path / "big0")) <= 64 * 1000 * 1000
    pairs = d["flow_pairs"]
    assert pairs[0] == 0 and pairs[-1] == B - 1 and 2 < len(pairs) < B and pairs == sorted(set(pairs))
    fp = np.load(tmp_path / "big0" / "flow_pairs.npy")
    assert fp.dtype == np.float32 and np.array_equal(fp, big[pairs].numpy())
    pts = np.load(tmp_path / "big0" / "flow_points.npy")
    assert pts.dtype == np.float32 and pts.shape == (bench.DUMP_POINTS, 2)
    where = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(B * h * w, size=bench.DUMP_POINTS, replace=False))
    assert np.array_equal(pts, big.reshape(-1, 2).numpy()[where])
    for name in d["files"]:
        assert np.array_equal(np.load(tmp_path / "big0" / (name + ".npy")), np.load(tmp_path / "big1" / (name + ".npy")))


def test_bench_rejects_steps_below_one():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run", "--steps", "0"],
                       env=_clean_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr


def _clean_env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}


def _check_eight_rank_line(line):
    assert line["n_gpus"] == 8 and line["dry_run"] is True
    assert line["rccl_world_size"] == 8 and line["distinct_devices"] == 8 and len(line["devices"]) == 8
    assert len(line["ms_per_step_by_rank"]) == 8
    assert line["ms_per_step"] >= max(line["ms_per_step_by_rank"]) * 0.999   # the slowest rank sets the time
    assert line["ms_per_step_by_rank"][7] >= 8.0                             # rank r sleeps r + 1 ms per dummy step


def test_bench_eight_ranks_both_launchers():
    """The line the driver reads at N = 8, from both ways of starting the ranks (bench.py's own spawn and
    torch.distributed.run as the driver does it), on CPU with --dry-run: eight gloo ranks, the collective's own
    count of ranks, one device entry per rank, every rank's time, max over ranks as the step time."""
    import json
    import socket
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--dry-run", "--steps", "2"],
                       env=_clean_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    _check_eight_rank_line(json.loads(lines[0]))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "8", "--dry-run", "--steps", "2"],
                       env=_clean_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    _check_eight_rank_line(json.loads(lines[0]))


def test_shot_pipeline_eight_ranks():
    """Config 3's sharding at the size BASELINE.json names (8 ranks): contiguous shards, halo-free histograms, gather on
    rank 0, one ShotBoundaries pass over the whole stream (dry run: numpy bincount stands in for the kernel)."""
    import json
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "shot_pipeline.py"), "--gpus", "8", "--dry-run",
                        "--frames", "2003", "--height", "16", "--width", "24", "--cuts", "5"],
                       env=_clean_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert line["n_gpus"] == 8 and line["frames"] == 2003 and line["planted_found"] is True
    # ... and at BASELINE config 3's own size: 10 000 frames = 1 250 per rank, the per-rank table on rank 0's stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "shot_pipeline.py"), "--gpus", "8", "--dry-run",
                        "--frames", "10000", "--height", "16", "--width", "24", "--cuts", "8"],
                       env=_clean_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert line["frames"] == 10000 and line["planted_found"] is True
    assert [t["frames"] for t in line["ranks"]] == [1250] * 8 and len({t["device"] for t in line["ranks"]}) == 8
    assert "8 rank(s)" in r.stderr and r.stderr.count("1250") >= 8
    from scannertools_amd.sharding import flow_shard
    for rk in range(8):     # the OpticalFlow shards of the same stream: 1 250 rows + 1 halo frame (none behind the last)
        rows, frames = flow_shard(10000, rk, 8)
        assert rows == (1250 * rk, 1250 * (rk + 1)) and frames == (1250 * rk, min(10000, 1250 * (rk + 1) + 1))


def test_shot_pipeline_starts_its_own_ranks():
    """scripts/shot_pipeline.py --gpus 2 --dry-run: two gloo ranks, CPU histograms of a tiny stream
    (numpy bincount standing in for the kernel in the dry run only), gather on rank 0, ShotBoundaries."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "shot_pipeline.py"), "--gpus", "2", "--dry-run",
                        "--frames", "1200", "--height", "24", "--width", "32", "--cuts", "3"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert line["n_gpus"] == 2 and line["frames"] == 1200 and line["planted_found"] is True


def test_spawn_ranks_fails_fast_and_times_out(tmp_path, capfd):
    """A rank that dies at once takes the others down with it (they would otherwise wait in the rendezvous for torch's
    own timeout); a job that never finishes ends at the overall timeout; rank 0's output is relayed only on success."""
    import time
    from scannertools_amd.sharding import spawn_ranks
    script = tmp_path / "w.py"
    script.write_text("import os, sys, time\nr = int(os.environ['RANK'])\nmode = sys.argv[1]\n"
                      "print('hello from', r, flush=True)\n"
                      "if mode == 'die' and r == 1: sys.exit(7)\n"
                      "if mode != 'ok': time.sleep(60)\n")
    t0 = time.monotonic()
    assert spawn_ranks(str(script), ["die"], 3) == 1
    assert time.monotonic() - t0 < 20
    out, err = capfd.readouterr()
    assert "rank 1 exited with code 7" in err and "hello from 0" not in out
    t0 = time.monotonic()
    assert spawn_ranks(str(script), ["hang"], 2, timeout=1.0, grace=2.0) == 1
    assert time.monotonic() - t0 < 20
    assert "no result within" in capfd.readouterr().err
    assert spawn_ranks(str(script), ["ok"], 2) == 0
    assert "hello from 0" in capfd.readouterr().out


# ---- C ABI --------------------------------------------------------------------------------------
def _header_functions():
    src = open(os.path.join(ROOT, "include", "scannertools_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(st_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from scannertools_amd import _native
    assert os.path.exists(_native.LIB_PATH), "run __graft_entry__.build() first"
    L = ctypes.CDLL(_native.LIB_PATH)
    names = _header_functions()
    assert len(names) >= 25
    for n in names:
        assert hasattr(L, n), "header declares %s but the library does not export it" % n
    # and the Python binding covers the same set
    assert sorted(_native.SIGNATURES) == names


def test_library_matches_the_tree():
    """st_build_info: the library was made from exactly the sources of this tree (the Makefile hashes them into it), and
    __graft_entry__.ensure_built() -- what conftest, smoke() and bench.py call first -- therefore leaves it alone."""
    from scannertools_amd import _native
    info = _native.build_info()
    assert set(info) == {"src", "host", "at"}
    assert info["src"] == _native.source_hash(), "libscannertools_hip.so was built from other sources: run make"
    out = subprocess.check_output(["make", "-s", "--no-print-directory", "-C", os.path.join(ROOT, "scannertools_amd", "csrc"), "srchash"], text=True)
    assert out.strip() == info["src"]


def test_native_libraries_are_never_committed():
    """A checkout must compile what it tests (round-5 verdict, item 4): every native library build() makes, and the objects
    behind them, are git-ignored, so no checkout carries a library built from other sources or on another machine."""
    import fnmatch
    import __graft_entry__ as g
    ign = [ln.strip() for ln in open(os.path.join(ROOT, ".gitignore")) if ln.strip() and not ln.startswith("#")]
    assert "*.so" in ign and "*.o" in ign
    for path in g.NATIVE + [g.BUILD_RECORD]:
        rel = os.path.relpath(path, ROOT)
        assert any(fnmatch.fnmatch(rel, p) or fnmatch.fnmatch(os.path.basename(rel), p) for p in ign), rel


def test_abi_host_only_entry_points():
    from scannertools_amd import _native
    import oracle
    L = _native.lib()
    assert L.st_abi_version() == 1
    assert L.st_status_string(0) == b"ok" and b"unsupported" in L.st_status_string(4)
    p = _native.default_params()
    assert (p.num_levels, p.pyr_scale, p.fast_pyramids, p.win_size, p.num_iters, p.poly_n, p.poly_sigma, p.flags) == \
        (3, 0.5, 0, 15, 3, 5, 1.2, 0)                      # optical_flow_kernel_cpu.cpp:16
    from scannertools_amd.hip import fb_level_geom, fb_levels
    for h, w in ((1080, 1920), (2160, 3840), (480, 640), (203, 317), (48, 64)):
        assert fb_levels(h, w) == oracle.fb_levels(h, w)
        for k in range(fb_levels(h, w) + 1):
            assert fb_level_geom(h, w, k) == oracle.fb_level_geom(h, w, k)
    with pytest.raises(TypeError):
        _native.default_params(nonsense=1)


def test_no_gpu_means_loud_failure_not_fallback():
    """Without a GPU nothing computes: context creation reports an error, the front-end raises."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from scannertools_amd import _native
    from scannertools_amd.hip import HipContext
    h = ctypes.c_void_p()
    assert _native.lib().st_ctx_create(0, ctypes.byref(h)) != 0 and not h.value
    with pytest.raises(RuntimeError):
        HipContext(0)


def test_product_never_imports_the_oracle():
    for root, _, files in os.walk(os.path.join(ROOT, "scannertools_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                txt = open(os.path.join(root, f)).read()
                assert not re.search(r"^\s*(import|from)\s+oracle\b", txt, flags=re.M), f
                assert "liboracle" not in txt and "oracle.c" not in txt.replace("oracle/oracle.c", ""), f


# ---- Scanner op library ---------------------------------------------------------------------------
def test_imgproc_library_registrations():
    from scannertools_amd import engine
    regs = engine.registered_kernels()
    ops = {(name, dev) for name, dev, _, _ in regs}
    assert {("Histogram", 0), ("Histogram", 1), ("OpticalFlow", 0), ("OpticalFlow", 1),
            ("FlowHistogram", 0), ("FlowHistogram", 1), ("Blur", 0), ("Blur", 1),
            ("Resize", 0), ("Resize", 1), ("ConvertColor", 0), ("ConvertColor", 1)} <= ops
    for name, dev, kind, can_batch in regs:
        assert can_batch                                           # .batch() as in histogram_kernel_cpu.cpp:54-57
        assert kind == (3 if name == "OpticalFlow" else 1)         # StenciledBatched / Batched
    assert engine.op_info("OpticalFlow")["stencil"] == [0, 1]      # optical_flow_kernel_cpu.cpp:51-54
    assert engine.op_info("OpticalFlow")["frame_output"] and not engine.op_info("Histogram")["frame_output"]
    assert not engine.op_info("FlowHistogram")["frame_output"]     # flow_histogram_kernel_cpu.cpp:62
    assert engine.op_info("Blur")["frame_output"]                  # blur_kernel_cpu.cpp:96
    assert engine.op_info("NoSuchOp") is None


def test_proto_writer_matches_wire_format():
    """BlurArgs{kernel_size: 3, sigma: 0.1} as protoc would serialise it."""
    from scannertools_amd import _proto
    import struct
    assert _proto.encode([(1, "int32", 3), (2, "float", 0.1)]) == b"\x08\x03\x15" + struct.pack("<f", 0.1)
    assert _proto.encode([(1, "int32", 0), (2, "float", 0.0)]) == b""       # proto3 omits defaults
    assert _proto.encode([(1, "int32", 300), (5, "string", "INTER_LINEAR")]) == b"\x08\xac\x02\x2a\x0cINTER_LINEAR"


def test_engine_reports_missing_gpu_cleanly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from scannertools_amd.engine import Client, DeviceType, NamedStream, NamedVideoStream, PerfParams
    sc = Client()
    sc.ingest_frames("v", np.zeros((2, 8, 8, 3), np.uint8))
    frame = sc.io.Input([NamedVideoStream(sc, "v")])
    hist = sc.ops.Histogram(frame=frame, device=DeviceType.CPU)
    with pytest.raises(RuntimeError, match="st_ctx_create"):
        sc.run(sc.io.Output(hist, [NamedStream(sc, "o")]), PerfParams.estimate())


def test_op_library_under_address_and_ub_sanitizers(tmp_path):
    """The Scanner-side host code (kernel classes, argument parsing, shim registries and the failure
    path of kernel creation without a GPU) built with -fsanitize=address,undefined and driven through
    the Python engine in a child process.  (GPU code cannot run under ASan on this pool.)"""
    import shutil
    import subprocess
    import sys
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the failure path is not taken")
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not asan or not os.path.isabs(asan) or shutil.which("g++") is None:
        pytest.skip("no libasan / g++")
    from scannertools_amd import _native
    _native.build()
    lib = tmp_path / "libscannertools_imgproc.so"
    kdir = os.path.join(ROOT, "scannertools_amd", "scanner_kernels")
    srcs = [os.path.join(kdir, f) for f in sorted(os.listdir(kdir)) if f.endswith(".cpp")]
    flags = ["-O1", "-std=c++17", "-fPIC", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
             "-I" + os.path.join(ROOT, "scanner_shim"), "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
             "-D__HIP_PLATFORM_AMD__"]
    srcs.append(os.path.join(ROOT, "scanner_shim", "shim.cpp"))
    objs, procs = [], []
    for src in srcs:  # one compiler process per translation unit
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        objs.append(obj)
        procs.append(subprocess.Popen(["g++"] + flags + ["-c", src, "-o", obj]))
    assert all(pr.wait() == 0 for pr in procs)
    subprocess.check_call(["g++", "-shared", "-fsanitize=address,undefined", "-o", str(lib)] + objs +
                          ["-L" + os.path.dirname(_native.LIB_PATH), "-lscannertools_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.dirname(_native.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"])
    script = r'''
import sys
sys.path.insert(0, %r)
import numpy as np
from scannertools_amd import engine
engine.IMGPROC_LIB = %r
from scannertools_amd.engine import Client, DeviceType, NamedStream, NamedVideoStream, PerfParams
assert len(engine.registered_kernels()) >= 12
assert engine.op_info("Resize")["frame_output"] and engine.op_info("NoSuchOp") is None
sc = Client()
sc.ingest_frames("v", np.zeros((2, 8, 8, 3), np.uint8))
frame = sc.io.Input([NamedVideoStream(sc, "v")])
errors = []
for mk in (lambda: sc.ops.Histogram(frame=frame), lambda: sc.ops.Blur(frame=frame, kernel_size=3, sigma=0.1),
           lambda: sc.ops.Resize(frame=frame, width=4, height=4, interpolation="INTER_AREA"),
           lambda: sc.ops.ConvertColor(frame=frame, conversion="COLOR_RGB2GRAY"),
           lambda: sc.ops.OpticalFlow(frame=frame, device=DeviceType.GPU), lambda: sc.ops.FlowHistogram(flow=frame),
           lambda: sc.ops.Blur(frame=frame, kernel_size=0),
           lambda: sc.ops.OpenPose(frame=frame, model_directory="/nonexistent", compute_hands=True),
           lambda: sc.ops.OpenPose(frame=frame, model_directory="/nonexistent", pose_num_scales=3, pose_scale_gap=0.2)):
    try:
        sc.run(sc.io.Output(mk(), [NamedStream(sc, "o")]), PerfParams.estimate())
    except RuntimeError as e:
        errors.append(str(e))
assert len(errors) == 9, errors
assert any("hand and face networks" in e for e in errors)
assert any("Could not parse BlurArgs" in e for e in errors)
# the caffemodel reader of the CPM2 kernel class on well-formed, truncated and random bytes
import ctypes, os, tempfile
from scannertools_amd import _proto
L = ctypes.CDLL(%r)
L.scannertools_caffe_check_model.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
err = ctypes.create_string_buffer(256)
layer = _proto.message(100, _proto.message(1, b"conv1_1") + _proto.message(7, _proto.message(5, np.zeros(64 * 27, "<f4").tobytes())) +
                       _proto.message(7, _proto.message(5, np.zeros(64, "<f4").tobytes())))
rng = np.random.default_rng(1)
overflow = b"\xa2\x06" + b"\xff" * 9 + b"\x01" + b"\x00"  # field 100, a length of 2**64 - 1: `i + len` wraps
for blob in (layer, layer[:len(layer) // 2], layer[:7], b"", rng.integers(0, 256, 5000, dtype=np.uint8).tobytes(), layer * 3 + b"\xff",
             overflow, layer + overflow, b"\x09\x00", b"\x0d\x00\x00"):
    with tempfile.NamedTemporaryFile(delete=False) as fh:
        fh.write(blob)
    assert L.scannertools_caffe_check_model(fh.name.encode(), err, 256) == -1 and err.value
    os.unlink(fh.name)
assert L.scannertools_caffe_check_model(None, err, 256) == -1
assert L.scannertools_caffe_check_model(tempfile.gettempdir().encode(), err, 256) == -1 and b"cannot read" in err.value  # a directory
print("sanitized run ok")
''' % (ROOT, str(lib), str(lib))
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0")
    p = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "sanitized run ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr, p.stderr[-4000:]
