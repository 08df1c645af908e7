"""GPU: st_jpeg_encode_batch_rst(..., ST_JPEG_RESTART_NONE) and the ImageEncoder kernel classes with restart = NONE against the
streams Pillow wrote at its defaults (tests/golden/jpeg_encode_norst_golden.npz): no DRI, no RSTn, byte for byte.  The default
mode beside it against tests/golden/jpeg_encode_golden.npz, so that neither leaks into the other."""
import ctypes
import json
import os

import numpy as np
import pytest

import ref_jpeg_encode_norst_np as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_encode_norst_golden.npz"))
GOLD_ROW = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_encode_golden.npz"))
CASES = [str(c) for c in GOLD["cases"]]
BATCH = [str(c) for c in GOLD["batch"]]
SAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
ST_ERR_INVALID = 1
# transform, entropy coding per MCU row, 0xFF count of the rows' owned bytes, layout, pack
NORST_LAUNCHES = 5


def _cfg(name):
    return json.loads(str(GOLD[name + "__cfg"]))


def _jpg(name):
    return GOLD[name + "__jpg"].tobytes()


def _img(name):
    return GOLD[_cfg(name)["img"]]


def _first_difference(a, b):
    n = min(len(a), len(b))
    d = np.nonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))[0]
    return (len(a), len(b), int(d[0]) if len(d) else n)


@pytest.fixture(scope="module")
def batch_singles(hip_ctx):
    """The 33 pictures of one shape, each encoded in a call of its own: computed once, never changed."""
    import torch
    return [hip_ctx.encode_jpeg(torch.from_numpy(_img(n)[None]).cuda(), restart="none")[0] for n in BATCH]


def test_every_golden_case_is_byte_identical(hip_ctx):
    """The common shapes at all three samplings (edge and padding blocks whose DC differences run on from row to row), rows of
    more than 64 and 128 blocks, rows of 14 / 20 / 32 bits at every phase of the bit offset, 0xFF bytes made of two rows' bits,
    scans that end aligned, padded, and padded to 0xFF."""
    import torch
    for name in CASES:
        c = _cfg(name)
        (got,) = hip_ctx.encode_jpeg(torch.from_numpy(_img(name)[None]).cuda(), c["quality"], c["subsampling"], restart="none")
        want = _jpg(name)
        assert got == want, (name,) + _first_difference(got, want)


def test_batch_equals_singles_and_golden(hip_ctx, batch_singles):
    import torch
    frames = torch.from_numpy(np.stack([_img(n) for n in BATCH])).cuda()
    got = hip_ctx.encode_jpeg(frames, restart="none")
    assert len(got) == 33
    for i, n in enumerate(BATCH):
        assert got[i] == batch_singles[i] == _jpg(n), (n,) + _first_difference(got[i], _jpg(n))
    # frames handed as separate buffers at odd addresses, one of them several times
    buf = torch.zeros((4, 24 * 32 * 3 + 5), dtype=torch.uint8, device="cuda")
    views = []
    for k in range(4):
        v = buf[k, k + 1:k + 1 + 24 * 32 * 3].view(24, 32, 3)
        v.copy_(frames[k])
        views.append(v)
    assert views[1].data_ptr() % 4 != views[2].data_ptr() % 4
    got = hip_ctx.encode_jpeg([views[0], views[3], views[3], views[1], views[3], views[2]], restart="none")
    assert got == [batch_singles[i] for i in (0, 3, 3, 1, 3, 2)]
    assert hip_ctx.encode_jpeg([], restart="none") == []


def test_alternating_modes_do_not_share_a_header(hip_ctx):
    """The same shape, quality and sampling with restart "row" and "none" in turn on one context: each its own golden bytes
    (the cached header and tables are keyed by the mode too)."""
    import torch
    both = [n for n in CASES if n in set(str(c) for c in GOLD_ROW["cases"])]
    names = BATCH[:2]
    for sub in SAMPLING:   # per sampling the two largest shapes that both files hold
        by_shape = {(_cfg(n)["h"], _cfg(n)["w"]): n for n in both if _cfg(n)["subsampling"] == sub and not n.startswith("24x32")}
        names = [by_shape[s] for s in sorted(by_shape, key=lambda s: s[0] * s[1])[-2:]] + names
    assert len(names) == 8 and len({(_cfg(n)["h"], _cfg(n)["w"]) for n in names}) >= 4
    for name in names:
        c = _cfg(name)
        assert json.loads(str(GOLD_ROW[name + "__cfg"])) == c and np.array_equal(GOLD_ROW[c["img"]], _img(name))
        frame = torch.from_numpy(_img(name)[None]).cuda()
        for restart in ("row", "none", "none", "row", "none", "row"):
            (got,) = hip_ctx.encode_jpeg(frame, c["quality"], c["subsampling"], restart=restart)
            want = _jpg(name) if restart == "none" else GOLD_ROW[name + "__jpg"].tobytes()
            assert got == want, (name, restart) + _first_difference(got, want)
        assert len(_jpg(name)) < len(GOLD_ROW[name + "__jpg"])
    # and the default is still "row"
    assert hip_ctx.encode_jpeg(frame, c["quality"], c["subsampling"])[0] == GOLD_ROW[names[-1] + "__jpg"].tobytes()


def test_shortest_rows_beside_noise_in_one_call(hip_ctx):
    """120 x 8 in one flat colour (rows of 14 / 20 / 32 bits) in a batch with noise frames of the same shape, whose streams
    the restatement gives: every frame's scan starts from its own first row."""
    import torch
    from scannertools_amd.hip import jpeg_encode_header, jpeg_quant_tables
    rng = np.random.default_rng(77)
    noise = [rng.integers(0, 256, (120, 8, 3), dtype=np.uint8) for _ in range(2)]
    for sub, (hs, vs) in SAMPLING.items():
        name = "120x8_flat_q95_" + sub.replace(":", "")
        flat = _img(name)
        header = jpeg_encode_header(120, 8, 95, sub, restart="none")
        want = [header + ref.scan_norst(ref.coefficients(a, *jpeg_quant_tables(95), hs, vs), 120, 8, hs, vs, header)[0] for a in noise]
        frames = torch.from_numpy(np.stack([noise[0], flat, flat, noise[1], flat])).cuda()
        got = hip_ctx.encode_jpeg(frames, 95, sub, restart="none")
        assert got == [want[0], _jpg(name), _jpg(name), want[1], _jpg(name)], sub


def test_more_frames_than_one_grid_dimension(hip_ctx):
    """65 537 frames of 8 x 8 in one call, two pictures alternating: every stream is that of its frame."""
    import torch
    n = 65537
    name = "8x8_noise_q50_420"
    pic = _img(name)
    pics = torch.from_numpy(np.stack([pic, pic[::-1, ::-1].copy()])).cuda()
    want = [_jpg(name), hip_ctx.encode_jpeg(pics[1:2], 50, "4:2:0", restart="none")[0]]
    assert hip_ctx.encode_jpeg(pics[0:1], 50, "4:2:0", restart="none")[0] == want[0] and want[0] != want[1]
    got = hip_ctx.encode_jpeg([pics[i & 1] for i in range(n)], 50, "4:2:0", restart="none")
    assert len(got) == n
    wrong = [i for i in range(n) if got[i] != want[i & 1]]
    assert not wrong, (len(wrong), wrong[:5])
    hip_ctx.release_workspace()


def test_a_bad_restart_is_refused_before_anything_is_launched(hip_ctx):
    import torch
    from scannertools_amd import _native
    L, hh, vp = _native.lib(), hip_ctx._h, ctypes.c_void_p
    hip_ctx._bind()
    frame = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    tab = (vp * 2)(frame.data_ptr(), frame.data_ptr())
    sizes = (ctypes.c_size_t * 2)()
    assert L.st_jpeg_encode_batch_rst(hh, tab, 2, 8, 8, 50, 2, 2, 1) == 0          # something to fetch, which a refusal takes away
    hip_ctx.timing_enable(list(range(_native.K_COUNT)))
    hip_ctx.timing_reset()
    for bad in (2, -1, 77):
        assert L.st_jpeg_encode_batch_rst(hh, tab, 2, 8, 8, 50, 2, 2, bad) == ST_ERR_INVALID
        msg = L.st_ctx_last_error(hh).decode()
        assert "jpeg_encode: restart %d is not supported" % bad in msg, msg
        assert L.st_jpeg_encode_fetch(hh, None, sizes, 0) == ST_ERR_INVALID and "no st_jpeg_encode_batch call" in L.st_ctx_last_error(hh).decode()
    # the other refusals are the default mode's, with its messages
    assert L.st_jpeg_encode_batch_rst(hh, tab, 2, 8, 8, 0, 2, 2, 1) == ST_ERR_INVALID and "quality 0 is outside 1..100" in L.st_ctx_last_error(hh).decode()
    assert L.st_jpeg_encode_batch_rst(hh, None, 2, 8, 8, 50, 2, 2, 1) == ST_ERR_INVALID and "null frame table" in L.st_ctx_last_error(hh).decode()
    assert sum(hip_ctx.timing_read(k)[0] for k in range(_native.K_COUNT)) == 0          # nothing was launched
    hip_ctx.timing_enable([])
    with pytest.raises(ValueError, match="restart 'rows' is not supported"):
        hip_ctx.encode_jpeg(frame[None], restart="rows")


def test_launch_counts_of_both_modes(hip_ctx):
    import torch
    from scannertools_amd import _native
    frames = torch.from_numpy(np.stack([_img(n) for n in BATCH[:5]])).cuda()
    hip_ctx.timing_enable(list(range(_native.K_COUNT)))
    for restart, launches, gold in (("row", 4, GOLD_ROW), ("none", NORST_LAUNCHES, GOLD), ("row", 4, GOLD_ROW)):
        hip_ctx.timing_reset()
        kw = {} if restart == "row" else {"restart": restart}     # the default path, called as it was before
        assert hip_ctx.encode_jpeg(frames, **kw) == [gold[n + "__jpg"].tobytes() for n in BATCH[:5]]
        counts = [hip_ctx.timing_read(k)[0] for k in range(_native.K_COUNT)]
        assert counts[_native.K_JPEG] == launches and sum(counts) == launches, (restart, counts)
    hip_ctx.timing_enable([])


def _client_with_batch():
    from scannertools_amd.engine import Client, NamedVideoStream
    sc = Client()
    sc.ingest_frames("pics", np.stack([_img(n) for n in BATCH]))
    return sc, sc.io.Input([NamedVideoStream(sc, "pics")])


def test_kernel_classes_write_the_golden_streams():
    from scannertools_amd import engine
    from scannertools_amd.engine import CacheMode, DeviceType, NamedStream, PerfParams
    L = engine._imgproc()
    before = (L.stshim_live_buffers(0), L.stshim_live_buffers(1))
    for device in (DeviceType.GPU, DeviceType.CPU):
        sc, frame = _client_with_batch()
        none, row = NamedStream(sc, "none"), NamedStream(sc, "row")
        sc.run([sc.io.Output(sc.ops.ImageEncoder(frame=frame, restart="none", device=device, batch=8), [none]),
                sc.io.Output(sc.ops.ImageEncoder(frame=frame, device=device, batch=8), [row])],
               PerfParams.estimate(), cache_mode=CacheMode.Overwrite)
        rows = list(none.load())
        assert len(rows) == 33                                    # executes of 8, 8, 8, 8 and 1 rows
        for n, r in zip(BATCH, rows):
            assert bytes(r) == _jpg(n), (device, n)
        assert [bytes(r) for r in row.load()] == [GOLD_ROW[n + "__jpg"].tobytes() for n in BATCH]
    assert (L.stshim_live_buffers(0), L.stshim_live_buffers(1)) == before


@pytest.mark.parametrize("decoder_args", [None, {"entropy": "gpu", "split": "subsequence"}], ids=["host_entropy", "gpu_subsequence"])
def test_round_trip_through_the_decoder_in_a_graph(decoder_args):
    """ImageEncoder(restart="none") -> ImageDecoder: the frames are what Pillow decodes its own streams to.  With the decoder's
    entropy="gpu", split="subsequence" nothing between the two ops has a marker, and both Huffman coders run on the device."""
    from scannertools_amd.engine import CacheMode, DeviceType, NamedStream, PerfParams
    sc, frame = _client_with_batch()
    img = sc.ops.ImageEncoder(frame=frame, restart="none", device=DeviceType.GPU, batch=16)
    out = NamedStream(sc, "decoded")
    sc.run(sc.io.Output(sc.ops.ImageDecoder(img=img, device=DeviceType.GPU, batch=16, args=decoder_args), [out]), PerfParams.estimate(),
           cache_mode=CacheMode.Overwrite)
    rows = list(out.load())
    assert len(rows) == 33
    for n, r in zip(BATCH, rows):
        want = GOLD[n + "__dec"]
        assert r.dtype == np.uint8 and r.shape == want.shape and np.array_equal(r, want), n
