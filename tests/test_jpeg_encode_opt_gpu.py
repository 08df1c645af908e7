"""GPU: st_jpeg_encode_batch_opt(..., optimize = 1) and the ImageEncoder kernel classes with optimize against the streams Pillow
wrote with optimize=True (tests/golden/jpeg_encode_opt_golden.npz), byte for byte in both restart modes; the device's symbol
counts and DHT segments against their host twins; the launch counts of DESIGN.md 4.16c; and the default paths beside it all, so
that the per-frame tables and headers do not leak into the cached ones."""
import ctypes
import json
import os

import numpy as np
import pytest

from jpeg_encode_opt_cases import CASES, SAMPLING, case_name, picture, sha256

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_encode_opt_golden.npz"))
GOLD_ROW = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_encode_golden.npz"))
GOLD_NONE = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_encode_norst_golden.npz"))
ST_ERR_INVALID = 1
# transform, symbol statistics, table construction, entropy coding, [0xFF count of the rows' owned bytes,] layout, pack
OPT_LAUNCHES = {"row": 6, "none": 7}
DEFAULT_LAUNCHES = {"row": 4, "none": 5}


def _cfg(c):
    return json.loads(str(GOLD[case_name(c) + "__cfg"]))


def _is_golden(c, got):
    cfg = _cfg(c)
    return (len(got), sha256(got)) == (cfg["jpg_len"], cfg["jpg_sha"])


def _why(c, got):
    """What to show when a stream differs: the lengths, and the first differing byte where the file holds the stream."""
    name, cfg = case_name(c), _cfg(c)
    if name + "__jpg" not in GOLD.files:
        return (name, len(got), cfg["jpg_len"])
    want = GOLD[name + "__jpg"].tobytes()
    n = min(len(got), len(want))
    d = np.nonzero(np.frombuffer(got[:n], np.uint8) != np.frombuffer(want[:n], np.uint8))[0]
    return (name, len(got), len(want), int(d[0]) if len(d) else n)


def _pic(c):
    return picture(c["kind"], c["h"], c["w"], c["seed"])


def _encode(ctx, c, frames=None, **kw):
    import torch
    frames = torch.from_numpy(_pic(c)[None]).cuda() if frames is None else frames
    return ctx.encode_jpeg(frames, c["quality"], c["subsampling"], restart=c["restart"], optimize=True, **kw)


def _used(tag, restart=None):
    return [c for c in CASES if tag in c["uses"] and restart in (None, c["restart"])]


def test_every_golden_case_is_byte_identical(hip_ctx):
    """The grid (both restart modes, three samplings, five qualities, four contents, five sizes), codes of more than 16 bits before
    the limiting, tables of one symbol, rows of 6 / 8 / 12 bits at every phase, rows that own no byte, bytes of three rows' bits,
    padding in an earlier row's byte.  The geometry cases have a test of their own."""
    done = 0
    for c in CASES:
        if {"tall", "wide"} & set(c["uses"]):
            continue
        (got,) = _encode(hip_ctx, c)
        assert _is_golden(c, got), _why(c, got)
        done += 1
    assert done == len(CASES) - 8 == 264


def test_geometry_thresholds(hip_ctx):
    """258 MCU rows, flat and noise (the sum over the rows above takes a second turn; flat: 257 rows of 6 bits); 198 and 132 blocks in
    a row (the statistics and entropy waves take several chunks)."""
    for c in _used("tall") + _used("wide"):
        (got,) = _encode(hip_ctx, c)
        assert _is_golden(c, got), _why(c, got)


@pytest.fixture(scope="module")
def batch_singles(hip_ctx):
    """Per restart mode the four pictures of 40 x 34 (flat, smooth, noise, two-level; quality 75, 4:2:0), each encoded in a call of
    its own: computed once, never changed."""
    return {r: [_encode(hip_ctx, c)[0] for c in _used("batch", r)] for r in ("row", "none")}


def test_batch_equals_singles_and_golden(hip_ctx, batch_singles):
    """One call mixes frames whose tables differ; frames at odd addresses; the same frame several times."""
    import torch
    for restart in ("row", "none"):
        cases, singles = _used("batch", restart), batch_singles[restart]
        assert [c["kind"] for c in cases] == ["flat", "smooth", "noise", "twolevel"]
        for c, s in zip(cases, singles):
            assert _is_golden(c, s), _why(c, s)
        frames = torch.from_numpy(np.stack([_pic(c) for c in cases])).cuda()
        assert _encode(hip_ctx, cases[0], frames) == singles
        buf = torch.zeros((4, 40 * 34 * 3 + 5), dtype=torch.uint8, device="cuda")
        views = []
        for k in range(4):
            v = buf[k, k + 1:k + 1 + 40 * 34 * 3].view(40, 34, 3)
            v.copy_(frames[k])
            views.append(v)
        assert views[1].data_ptr() % 4 != views[2].data_ptr() % 4
        order = (0, 3, 3, 1, 3, 2, 0, 2)
        assert _encode(hip_ctx, cases[0], [views[i] for i in order]) == [singles[i] for i in order]
        assert hip_ctx.encode_jpeg([], restart=restart, optimize=True) == []


def test_six_bit_rows_beside_noise_in_one_call(hip_ctx):
    """64 x 8 at 4:4:4: a flat frame (rows of 6 bits, a chroma DC table of two symbols) between noise frames, in both modes: every
    frame is coded with its own tables and its scan joined from its own rows."""
    import torch
    for restart in ("row", "none"):
        flat = next(c for c in _used("short_rows", restart) if (c["h"], c["kind"]) == (64, "flat"))
        (noise,) = _used("mixed", restart)
        assert (flat["quality"], flat["subsampling"]) == (noise["quality"], noise["subsampling"])
        order = (noise, flat, flat, noise, flat)
        got = _encode(hip_ctx, flat, torch.from_numpy(np.stack([_pic(c) for c in order])).cuda())
        for c, g in zip(order, got):
            assert _is_golden(c, g), (restart,) + _why(c, g)


def test_optimize_on_and_off_alternate_on_one_context(hip_ctx):
    """The same picture, quality and sampling with and without optimize, in both restart modes, in turn on one context: each call
    Pillow's bytes for its setting -- the per-frame tables and header do not reach the cached ones, nor the other way round."""
    import torch
    for row, none in zip(_used("batch", "row"), _used("batch", "none")):
        frame = torch.from_numpy(_pic(row)[None]).cuda()
        case = {"row": row, "none": none}
        plain = {r: GOLD[case_name(c) + "__plain"].tobytes() for r, c in case.items()}
        for restart, opt in (("row", True), ("row", False), ("none", True), ("none", False), ("row", True), ("none", False), ("none", True), ("row", False)):
            (got,) = hip_ctx.encode_jpeg(frame, 75, "4:2:0", restart=restart, optimize=opt)
            if opt:
                assert _is_golden(case[restart], got), (restart,) + _why(case[restart], got)
                assert len(got) < len(plain[restart]) and got[:177] == plain[restart][:177]
            else:
                assert got == plain[restart], (case_name(case[restart]), restart)
        # and the defaults are still restart "row" without optimize
        assert hip_ctx.encode_jpeg(frame, 75, "4:2:0")[0] == plain["row"]
    # a case of the fixtures of the default paths after all that
    name = "8x360_noise_q50_422"
    cfg = json.loads(str(GOLD_NONE[name + "__cfg"]))
    frame = torch.from_numpy(GOLD_NONE[cfg["img"]][None]).cuda()
    assert hip_ctx.encode_jpeg(frame, 50, "4:2:2", restart="none")[0] == GOLD_NONE[name + "__jpg"].tobytes()
    assert hip_ctx.encode_jpeg(frame, 50, "4:2:2")[0] == GOLD_ROW[name + "__jpg"].tobytes()


def test_device_statistics_and_tables_equal_their_host_twins(hip_ctx):
    """st_jpeg_encode_fetch_stats against st_jpeg_symbol_stats over the coefficients the host decoder reads from the stream, and
    the four DHT segments the device placed in the header against st_jpeg_optimal_dht of those counts -- for a batch of four, the
    frames with codes beyond 16 bits, 6-bit rows, a one-symbol table, and a row of 198 blocks."""
    import torch
    from scannertools_amd.hip import jpeg_coefficients, jpeg_optimal_dht, jpeg_symbol_stats
    picks = [_used("batch", r) for r in ("row", "none")]
    picks += [[c] for c in CASES if case_name(c) in ("256x256_noise30_q100_444_none", "256x256_noise30_q95_444_row", "512x8_flat0_q90_444_none",
                                                     "512x8_gray6_q90_444_none", "8x528_noise33_q75_444_row", "8x528_smooth34_q95_420_none")]
    assert len(picks) == 8
    for cases in picks:
        c = cases[0]
        got = _encode(hip_ctx, c, torch.from_numpy(np.stack([_pic(k) for k in cases])).cuda())
        stats = hip_ctx.last_jpeg_symbol_stats(len(cases))
        assert stats.shape == (len(cases), 4, 256)
        for k, g, s in zip(cases, got, stats):
            assert _is_golden(k, g), _why(k, g)
            coef, _ = jpeg_coefficients(g)
            want = jpeg_symbol_stats(coef, k["h"], k["w"], k["subsampling"], k["restart"])
            assert (s == want).all(), (case_name(k), np.argwhere(s != want)[:4].tolist())
            at = 177
            for t in range(4):
                seg, _ = jpeg_optimal_dht(s[t], t)
                assert g[at:at + len(seg)] == seg, (case_name(k), t)
                at += len(seg)
            assert g[at:at + 2] == (b"\xff\xdd" if k["restart"] == "row" else b"\xff\xda")
    # nothing to fetch after a call without optimize, or after a refused one
    from scannertools_amd import _native
    hip_ctx.encode_jpeg(torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda"))
    out = np.zeros(1024, np.uint64)
    assert _native.lib().st_jpeg_encode_fetch_stats(hip_ctx._h, out.ctypes.data, 1024) == ST_ERR_INVALID
    assert "no st_jpeg_encode_batch_opt call" in _native.lib().st_ctx_last_error(hip_ctx._h).decode()


def test_more_frames_than_one_grid_dimension(hip_ctx):
    """65 537 frames of 8 x 8 in one call, two pictures alternating, without restart markers: every stream is that of its frame."""
    import torch
    n = 65537
    c = next(k for k in CASES if (k["h"], k["w"], k["kind"], k["restart"]) == (8, 8, "noise", "none"))
    pic = _pic(c)
    pics = torch.from_numpy(np.stack([pic, pic[::-1, ::-1].copy()])).cuda()
    want = [_encode(hip_ctx, c, pics[0:1])[0], _encode(hip_ctx, c, pics[1:2])[0]]
    assert _is_golden(c, want[0]) and want[0] != want[1]
    got = _encode(hip_ctx, c, [pics[i & 1] for i in range(n)])
    assert len(got) == n
    wrong = [i for i in range(n) if got[i] != want[i & 1]]
    assert not wrong, (len(wrong), wrong[:5])
    hip_ctx.release_workspace()


def test_a_bad_optimize_is_refused_before_anything_is_launched(hip_ctx):
    import torch
    from scannertools_amd import _native
    L, hh, vp = _native.lib(), hip_ctx._h, ctypes.c_void_p
    hip_ctx._bind()
    frame = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    tab = (vp * 2)(frame.data_ptr(), frame.data_ptr())
    sizes = (ctypes.c_size_t * 2)()
    assert L.st_jpeg_encode_batch_opt(hh, tab, 2, 8, 8, 50, 2, 2, 1, 1) == 0          # something to fetch, which a refusal takes away
    hip_ctx.timing_enable(list(range(_native.K_COUNT)))
    hip_ctx.timing_reset()
    for bad in (2, -1, 77):
        for restart in (0, 1):
            assert L.st_jpeg_encode_batch_opt(hh, tab, 2, 8, 8, 50, 2, 2, restart, bad) == ST_ERR_INVALID
            msg = L.st_ctx_last_error(hh).decode()
            assert "jpeg_encode: optimize %d is not supported (0 or 1)" % bad in msg, msg
            assert L.st_jpeg_encode_fetch(hh, None, sizes, 0) == ST_ERR_INVALID and "no st_jpeg_encode_batch call" in L.st_ctx_last_error(hh).decode()
    # the other refusals are the default path's, with its messages, and come first
    assert L.st_jpeg_encode_batch_opt(hh, tab, 2, 8, 8, 50, 2, 2, 5, 7) == ST_ERR_INVALID and "restart 5 is not supported" in L.st_ctx_last_error(hh).decode()
    assert L.st_jpeg_encode_batch_opt(hh, tab, 2, 8, 8, 0, 2, 2, 1, 1) == ST_ERR_INVALID and "quality 0 is outside 1..100" in L.st_ctx_last_error(hh).decode()
    assert L.st_jpeg_encode_batch_opt(hh, None, 2, 8, 8, 50, 2, 2, 1, 1) == ST_ERR_INVALID and "null frame table" in L.st_ctx_last_error(hh).decode()
    assert sum(hip_ctx.timing_read(k)[0] for k in range(_native.K_COUNT)) == 0          # nothing was launched
    hip_ctx.timing_enable([])
    with pytest.raises(ValueError, match="optimize 2 is not supported"):
        hip_ctx.encode_jpeg(frame[None], optimize=2)


def test_launch_counts(hip_ctx, batch_singles):
    """Six launches with restart markers, seven without; four and five with optimize off, through the new entry point too.  Only
    the jpeg slot counts."""
    import torch
    from scannertools_amd import _native
    L, vp = _native.lib(), ctypes.c_void_p
    cases = _used("batch", "row")
    frames = torch.from_numpy(np.stack([_pic(c) for c in cases])).cuda()
    tab = (vp * 4)(*[frames[i].data_ptr() for i in range(4)])
    hip_ctx.timing_enable(list(range(_native.K_COUNT)))
    for restart, opt in (("row", True), ("none", True), ("row", False), ("none", False), ("none", True), ("row", True)):
        hip_ctx.timing_reset()
        got = hip_ctx.encode_jpeg(frames, 75, "4:2:0", restart=restart, optimize=opt)
        counts = [hip_ctx.timing_read(k)[0] for k in range(_native.K_COUNT)]
        want = (OPT_LAUNCHES if opt else DEFAULT_LAUNCHES)[restart]
        assert counts[_native.K_JPEG] == want and sum(counts) == want, (restart, opt, counts)
        if opt:
            assert got == batch_singles[restart]
        else:   # optimize = 0 through the new entry point is st_jpeg_encode_batch_rst: the same launches, the same bytes
            hip_ctx.timing_reset()
            assert L.st_jpeg_encode_batch_opt(hip_ctx._h, tab, 4, 40, 34, 75, 2, 2, {"row": 0, "none": 1}[restart], 0) == 0
            counts = [hip_ctx.timing_read(k)[0] for k in range(_native.K_COUNT)]
            assert counts[_native.K_JPEG] == want and sum(counts) == want, (restart, counts)
            sizes = (ctypes.c_size_t * 4)()
            assert L.st_jpeg_encode_fetch(hip_ctx._h, None, sizes, 0) == 0 and list(sizes) == [len(g) for g in got]
    hip_ctx.timing_enable([])


def _client(restart):
    from scannertools_amd.engine import Client, NamedVideoStream
    sc = Client()
    cases = _used("batch", restart)
    sc.ingest_frames("pics", np.stack([_pic(c) for c in cases] * 3))   # 12 rows: the four pictures three times
    return sc, sc.io.Input([NamedVideoStream(sc, "pics")]), cases * 3


def test_kernel_classes_write_the_golden_streams():
    from scannertools_amd import engine
    from scannertools_amd.engine import CacheMode, DeviceType, NamedStream, PerfParams
    L = engine._imgproc()
    before = (L.stshim_live_buffers(0), L.stshim_live_buffers(1))
    for device in (DeviceType.GPU, DeviceType.CPU):
        for restart in ("row", "none"):
            sc, frame, cases = _client(restart)
            opt, plain = NamedStream(sc, "opt"), NamedStream(sc, "plain")
            sc.run([sc.io.Output(sc.ops.ImageEncoder(frame=frame, quality=75, restart=restart, optimize=True, device=device, batch=5), [opt]),
                    sc.io.Output(sc.ops.ImageEncoder(frame=frame, quality=75, restart=restart, device=device, batch=5), [plain])],
                   PerfParams.estimate(), cache_mode=CacheMode.Overwrite)
            rows, plain_rows = list(opt.load()), list(plain.load())
            assert len(rows) == 12 == len(plain_rows)                # executes of 5, 5 and 2 rows
            for c, r, p in zip(cases, rows, plain_rows):
                assert _is_golden(c, bytes(r)), (device, restart) + _why(c, bytes(r))
                assert len(bytes(r)) < len(bytes(p)) and bytes(p)[:177] == bytes(r)[:177]
    assert (L.stshim_live_buffers(0), L.stshim_live_buffers(1)) == before


@pytest.mark.parametrize("restart,decoder_args", [("row", None), ("none", None), ("row", {"entropy": "gpu", "split": "subsequence"}),
                                                  ("none", {"entropy": "gpu", "split": "subsequence"}), ("row", {"entropy": "gpu", "split": "interval"})],
                         ids=["row_host", "none_host", "row_subsequence", "none_subsequence", "row_interval"])
def test_round_trip_through_the_decoder_in_a_graph(restart, decoder_args):
    """ImageEncoder(optimize=True) -> ImageDecoder: the frames are what Pillow decodes its own optimize=True streams to, on the
    decoder's host entropy path, by subsequence on the device, and by restart interval on the device where the stream has them."""
    from scannertools_amd.engine import CacheMode, DeviceType, NamedStream, PerfParams
    sc, frame, cases = _client(restart)
    img = sc.ops.ImageEncoder(frame=frame, quality=75, restart=restart, optimize=True, device=DeviceType.GPU, batch=8)
    out = NamedStream(sc, "decoded")
    sc.run(sc.io.Output(sc.ops.ImageDecoder(img=img, device=DeviceType.GPU, batch=8, args=decoder_args), [out]), PerfParams.estimate(),
           cache_mode=CacheMode.Overwrite)
    rows = list(out.load())
    assert len(rows) == 12
    for c, r in zip(cases, rows):
        want = GOLD[case_name(c) + "__dec"]
        assert r.dtype == np.uint8 and r.shape == want.shape and np.array_equal(r, want), case_name(c)
