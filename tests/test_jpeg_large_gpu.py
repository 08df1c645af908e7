"""GPU: the JPEG encoder and every path of the decoder at the frame sizes where their launch geometry changes, byte for byte
against Pillow's streams and frames (tests/golden/jpeg_large_golden.npz).  The small fixtures of the other JPEG modules stop at
19 MCU rows, 138 blocks per row, 2408 lanes and a handful of segments; here: more than 256 MCU rows (k_jpeg_ff_count's sum takes
a second turn), rows of 65 500 pixels (384 chunks of k_jpeg_entropy, thousands of steps of k_jpeg_pack_bits), more than 2 097 152
pixels in k_jpeg_color<1> (its grid strides), more than 64 MiB of coefficients in one st_jpeg_decode_batch call (the sub-batches
are cut by bytes), more than 65 536 restart intervals, lanes and subsequences and more than 1024 segments (the grid.y strides of
k_jpeg_entropy_dec, k_jsq_round, k_jsq_write and k_jsq_scan), and the workload's 1080 x 1920.

The pictures are rebuilt from their recipes (tests/jpeg_large_cases.py).  Where the file holds only a stream's length and
SHA-256, those are compared, and on a mismatch the restatement is run to name the first wrong byte.  A decoded frame is compared
with ref_jpeg_np.decode of the stream, whose SHA-256 must be the one Pillow's frame had; tests/test_jpeg_large.py pins both
restatements to Pillow on the CPU and asserts that every case crosses the threshold it is here for.  No test uses a corrupt
stream or provokes a fault."""
import json
import os

import numpy as np
import pytest

import jpeg_large_cases as lc
import ref_jpeg_encode_norst_np as ref_norst
import ref_jpeg_encode_np as ref_row
import ref_jpeg_np
from util import env_threads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_large_golden.npz"))
CASES = [str(c) for c in GOLD["cases"]]


def _cfg(name):
    return json.loads(str(GOLD[name + "__cfg"]))


def _by_use(use, restart=None):
    return [n for n in CASES if use in _cfg(n)["uses"] and restart in (None, _cfg(n)["restart"])]


def _picture(name):
    c = _cfg(name)
    return lc.picture(c["kind"], c["h"], c["w"], c["seed"], c["channels"])


def _restate(arr, quality, subsampling, restart):
    """The stream the restatement writes for a picture: the library's header and tables, the restatement's coefficients and scan."""
    from scannertools_amd.hip import jpeg_encode_header, jpeg_quant_tables
    h, w = arr.shape[:2]
    hs, vs = lc.SAMPLING[subsampling]
    header = jpeg_encode_header(h, w, quality, subsampling, restart=restart)
    coef = ref_row.coefficients(arr, *jpeg_quant_tables(quality), hs, vs)
    if restart == "none":
        return header + ref_norst.scan_norst(coef, h, w, hs, vs, header)[0]
    return header + ref_row.scan(coef, h, w, hs, vs, header)


def _first_difference(a, b):
    n = min(len(a), len(b))
    d = np.nonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))[0]
    return (len(a), len(b), int(d[0]) if len(d) else n)


def _assert_stream(name, got, arr=None):
    """got is Pillow's stream of the case.  The failure names the lengths and the first differing byte; where the file holds only
    the stream's hash, the restatement (which test_jpeg_large.py holds to that hash) is run for them."""
    if name + "__jpg" in GOLD.files:
        want = GOLD[name + "__jpg"].tobytes()
        assert got == want, (name,) + _first_difference(got, want)
    elif len(got) != int(GOLD[name + "__jpg_len"]) or lc.sha256(got) != str(GOLD[name + "__jpg_sha256"]):
        c = _cfg(name)
        want = _restate(_picture(name) if arr is None else arr, c["quality"], c["subsampling"], c["restart"])
        assert lc.sha256(want) == str(GOLD[name + "__jpg_sha256"]), (name, "the restatement does not write the stream Pillow wrote")
        assert got == want, (name,) + _first_difference(got, want)


def _encode(hip_ctx, name, arr=None):
    import torch
    c = _cfg(name)
    arr = _picture(name) if arr is None else arr
    (got,) = hip_ctx.encode_jpeg(torch.from_numpy(arr[None]).cuda(), c["quality"], c["subsampling"], restart=c["restart"])
    return got


_DECODED = {}


def _decoded(name, jpg=None):
    """ref_jpeg_np.decode of a case's stream, computed once and never changed; the frame has the hash Pillow's frame had."""
    if name not in _DECODED:
        frame = ref_jpeg_np.decode(GOLD[name + "__jpg"].tobytes() if jpg is None else jpg)
        if name + "__dec_sha256" in GOLD.files:
            assert lc.sha256(frame.tobytes()) == str(GOLD[name + "__dec_sha256"]), name
        frame.setflags(write=False)
        _DECODED[name] = frame
    return _DECODED[name]


def _decode_paths(jpg):
    """The keyword sets of decode_jpeg a stream is decoded with: host entropy, one lane per restart interval where there are
    any, one lane per subsequence at the default size and at 8 bytes."""
    sos = jpg.index(b"\xff\xda")
    paths = [dict(), dict(entropy="gpu", split="subsequence"), dict(entropy="gpu", split="subsequence", subseq_bytes=8)]
    if jpg.find(b"\xff\xdd\x00\x04", 0, sos) >= 0:
        paths.insert(1, dict(entropy="gpu", split="interval"))
    return paths


def _assert_frames(got, want, what):
    import torch
    want = torch.from_numpy(np.array(want)).to(got.device)   # (a copy: the shared expectation is read-only)
    if got.shape != want.shape or not torch.equal(got, want):
        assert got.shape == want.shape, what
        bad = torch.nonzero((got != want).reshape(got.shape[0], -1))
        n, at = int(bad[0, 0]), int(bad[0, 1])
        c = got.shape[3]
        raise AssertionError((what, "wrong bytes: %d" % len(bad), "first: frame %d, y %d, x %d" % (n, at // c // got.shape[2], at // c % got.shape[2])))


# ---- encoder ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("restart", ["none", "row"])
def test_tall_frames(hip_ctx, restart):
    """258 and 261 MCU rows: k_jpeg_ff_count's sum over the rows above takes a second turn of its 256 threads, k_jpeg_layout,
    k_jpeg_pack and k_jpeg_pack_bits index past row 255.  130 rows: all four waves of the sum in one turn.  300 rows of 14 /
    20 / 32 bits in one flat colour: a sum of many tiny lengths."""
    names = _by_use("tall", restart)
    assert len(names) == (7 if restart == "none" else 6)
    for name in names:
        _assert_stream(name, _encode(hip_ctx, name))


@pytest.mark.parametrize("restart", ["none", "row"])
def test_two_tall_frames_in_one_call(hip_ctx, restart):
    """Two pictures of one tall shape in one call, and swapped: a frame's sum over the rows above starts at its own first row."""
    import torch
    seconds = _by_use("tall_pair", restart)
    assert len(seconds) == 2
    for second in seconds:
        c = _cfg(second)
        (first,) = [n for n in _by_use("tall", restart) if (_cfg(n)["h"], _cfg(n)["w"], _cfg(n)["quality"]) == (c["h"], c["w"], c["quality"])]
        pair = (first, second)
        a, b = _picture(pair[0]), _picture(pair[1])
        for order in ((0, 1), (1, 0), (0, 0, 1)):
            frames = torch.from_numpy(np.stack([(a, b)[i] for i in order])).cuda()
            got = hip_ctx.encode_jpeg(frames, c["quality"], c["subsampling"], restart=restart)
            assert len(got) == len(order)
            for k, i in enumerate(order):
                _assert_stream(pair[i], got[k], (a, b)[i])


@pytest.mark.parametrize("restart", ["none", "row"])
def test_wide_frames(hip_ctx, restart):
    """65 500 pixels, the widest frame libjpeg writes: 8 rows of noise at quality 100 and 4:4:4 (the longest row in bits, 384
    chunks of 64 blocks, more than 8000 steps of 256 bytes in k_jpeg_pack_bits), 16 rows at 4:2:0, 9 smooth rows at 4:2:2 (a second
    MCU row, of padding blocks)."""
    names = _by_use("wide", restart)
    assert len(names) == 3
    for name in names:
        _assert_stream(name, _encode(hip_ctx, name))


@pytest.mark.parametrize("restart", ["none", "row"])
def test_workload_frame(hip_ctx, restart):
    """1080 x 1920 at 4:2:0 and quality 95: 68 MCU rows (two waves of the sum), 12 chunks per row."""
    (name,) = _by_use("workload", restart)
    _assert_stream(name, _encode(hip_ctx, name))


def test_a_frame_wider_than_libjpeg_writes(hip_ctx):
    """8 x 65 535: the format's 16-bit fields hold it and the library accepts it, libjpeg refuses every dimension above 65 500.
    libjpeg cannot arbitrate here: the stream is compared with the restatement alone (which tests/test_jpeg_large.py holds to
    Pillow up to 65 500), and the decoder's frame with ref_jpeg_np.decode of that stream."""
    import torch
    from scannertools_amd.hip import probe_jpeg
    arr = lc.picture("noise", 8, 65535, 40)
    frame = torch.from_numpy(arr[None]).cuda()
    for restart in ("none", "row"):
        want = _restate(arr, 50, "4:4:4", restart)
        (got,) = hip_ctx.encode_jpeg(frame, 50, "4:4:4", restart=restart)
        assert got == want, (restart,) + _first_difference(got, want)
    info = probe_jpeg(got)
    assert (info["h"], info["w"], info["restart_interval"]) == (8, 65535, 8192)
    frame = ref_jpeg_np.decode(got)
    for kw in _decode_paths(got):
        _assert_frames(hip_ctx.decode_jpeg([got], **kw), frame[None], kw)


# ---- decoder ---------------------------------------------------------------------------------------------------------------

def test_color_kernel_strides_over_its_grid(hip_ctx):
    """1449 x 1451 at 4:2:0 and at 4:2:2: the odd width selects k_jpeg_color<1>, one pixel per thread, and the frame has more
    pixels than the kernel's largest grid (8192 workgroups of 256) has threads."""
    names = _by_use("color_stride")
    assert len(names) == 2
    for name in names:
        jpg = GOLD[name + "__jpg"].tobytes()
        for kw in _decode_paths(jpg):
            _assert_frames(hip_ctx.decode_jpeg([jpg], **kw), _decoded(name)[None], (name, kw))


def test_color_kernel_strides_at_an_odd_address(hip_ctx):
    """1448 x 1452 (a width of 4 k) written at an address one byte off: k_jpeg_color<1> again, and the bytes around the frame stay."""
    import torch
    (name,) = _by_use("color_stride_offset")
    jpg, want = GOLD[name + "__jpg"].tobytes(), _decoded(name)
    nbytes = want.size
    for kw in _decode_paths(jpg):
        for offset in (1, 0):
            buf = torch.full((nbytes + 64,), 0x5A, dtype=torch.uint8, device=hip_ctx.device)
            out = buf[offset:offset + nbytes].view((1,) + want.shape)
            assert out.data_ptr() % 4 == offset
            hip_ctx.decode_jpeg([jpg], out=out, **kw)
            _assert_frames(out, want[None], (name, kw, offset))
            assert bool((buf[:offset] == 0x5A).all()) and bool((buf[offset + nbytes:] == 0x5A).all()), (name, kw, offset)


def test_sub_batches_cut_by_bytes(hip_ctx):
    """Seven streams of 12.7 MB of coefficients each in one call, two pictures in an order without a period.
    st_jpeg_decode_batch cuts a sub-batch where its coefficients would pass 64 MiB (kSlotCoefBytes): with 16 threads after the
    fifth stream (two sub-batches, the second into the device buffers the first used); with 2 threads the cut by count comes
    first (four sub-batches, the page-locked slots handed back).  The launches are counted: one timed region per sub-batch.
    The device paths (st_jpeg_decode_batch_gpu, ..._gpu_split) cut at 2 GiB (kGpuCoefBytes), which this call stays under: they
    take it as one sub-batch, and must give the same frames."""
    from scannertools_amd import _native
    names = _by_use("byte_cut")
    streams = [GOLD[names[i] + "__jpg"].tobytes() for i in lc.BYTE_CUT_ORDER]
    want = np.stack([_decoded(names[i]) for i in lc.BYTE_CUT_ORDER])
    hip_ctx.timing_enable(list(range(_native.K_COUNT)))
    try:
        for threads, sub_batches in ((16, 2), (2, 4)):
            for kw, regions in ((dict(), sub_batches), (dict(entropy="gpu", split="interval"), 1), (dict(entropy="gpu", split="subsequence"), 1)):
                hip_ctx.timing_reset()
                with env_threads("ST_JPEG_THREADS", threads):
                    got = hip_ctx.decode_jpeg(streams, **kw)
                _assert_frames(got, want, (threads, kw))
                counts = [hip_ctx.timing_read(k)[0] for k in range(_native.K_COUNT)]
                assert counts[_native.K_JPEG] == regions and sum(counts) == regions, (threads, kw, counts)
                del got
    finally:
        hip_ctx.timing_enable([])
        hip_ctx.release_workspace()


def _options(hip_ctx, jpg, want, name):
    for kw in _decode_paths(jpg) + [dict(entropy="gpu", split="subsequence", max_rounds=1), dict(entropy="gpu", split="subsequence", subseq_bytes=8, max_rounds=1)]:
        _assert_frames(hip_ctx.decode_jpeg([jpg], **kw), want[None], (name, kw))


def test_more_than_65536_restart_intervals(hip_ctx):
    """2056 x 2056, one component, a restart interval per block: 66 049 intervals are 1033 groups of 64 lanes, past grid.y =
    1024 of k_jpeg_entropy_dec; by subsequence they are 66 049 segments of one lane each, past the 1024 of k_jsq_scan and, as
    lanes, of k_jsq_round and k_jsq_write; lane_at() searches 66 049 segments."""
    (name,) = _by_use("many_intervals")
    _options(hip_ctx, GOLD[name + "__jpg"].tobytes(), _decoded(name), name)


def test_more_than_1024_segments_of_three_components(hip_ctx):
    """520 x 520 at 4:2:0, a restart interval per MCU: 1089 segments of six blocks."""
    (name,) = _by_use("many_segments")
    _options(hip_ctx, GOLD[name + "__jpg"].tobytes(), _decoded(name), name)


def test_more_than_65536_subsequences_in_one_scan(hip_ctx):
    """640 x 648 noise at quality 95 and 4:4:4 without restart markers: a scan of 1.0 MB, more than 125 000 lanes of 8 bytes in
    ONE segment, so 1961 groups of 64 for a grid.y of 1024: in k_jsq_round and k_jsq_write a workgroup takes a second group, whose
    first lane (like every group's) enters from the exit the previous launch left in front of it.  The stream is the project's
    encoder's (which is Pillow's, by its length and hash); the frame is ref_jpeg_np.decode of those bytes."""
    (name,) = _by_use("subsequences")
    jpg = _encode(hip_ctx, name)
    _assert_stream(name, jpg)
    scan = len(jpg) - 623 - 2
    assert scan > 8 * 65536
    want = _decoded(name, jpg)[None]
    _assert_frames(hip_ctx.decode_jpeg([jpg]), want, "host")
    _assert_frames(hip_ctx.decode_jpeg([jpg], entropy="gpu", split="subsequence"), want, "default")
    assert 1 <= hip_ctx.last_jpeg_rounds() <= 64
    _assert_frames(hip_ctx.decode_jpeg([jpg], entropy="gpu", split="subsequence", subseq_bytes=8), want, "8 bytes")
    assert 1 <= hip_ctx.last_jpeg_rounds() <= 64
    # one round launch, and the interval decoder behind it
    _assert_frames(hip_ctx.decode_jpeg([jpg], entropy="gpu", split="subsequence", max_rounds=1), want, "one round")
    # (at 8 bytes: below.)  The frame cannot tell whether the rounds did their work: lanes that k_jsq_round never ran are found stale by k_jsq_scan, and
    # k_jsq_fallback then walks the whole segment with ONE lane, slow and exact.  The device time can.  With max_rounds=1 the walk
    # is certain (a group's first lane entered from a guess); a call that has to walk takes at least as long as that one, a call
    # whose rounds converged decodes on 125 000 lanes: asked for is less than half the time (measured: 23 ms against 520 ms, and
    # 517 ms with the stride over the groups taken out of k_jsq_round).  The best of three against one: other work on the device
    # only ever adds time.
    from scannertools_amd import _native

    def timed(**kw):
        hip_ctx.timing_reset()
        _assert_frames(hip_ctx.decode_jpeg([jpg], entropy="gpu", split="subsequence", subseq_bytes=8, **kw), want, kw)
        hip_ctx.sync()
        return hip_ctx.timing_read(_native.K_JPEG)[1]

    hip_ctx.timing_enable([_native.K_JPEG])
    try:
        walk = timed(max_rounds=1)
        converged = min(timed() for _ in range(3))
    finally:
        hip_ctx.timing_enable([])
    print("by subsequence at 8 bytes: %.1f ms converged, %.1f ms with the one-lane walk" % (converged, walk))
    assert converged < walk / 2, (converged, walk)


def test_round_trip_of_workload_frames_in_a_graph(hip_ctx):
    """ImageEncoder(restart="none") -> ImageDecoder(entropy=gpu, split=subsequence) on two 1080 x 1920 frames through the
    stand-in engine: the frames ref_jpeg_np.decode gives for Pillow's streams of the two pictures (the encoder's, once they
    have Pillow's length and hash)."""
    from scannertools_amd.engine import CacheMode, Client, DeviceType, NamedStream, NamedVideoStream, PerfParams
    names = _by_use("round_trip", "none")
    assert len(names) == 2
    pics = [_picture(n) for n in names]
    want = []
    for n, p in zip(names, pics):
        jpg = _encode(hip_ctx, n, p)
        _assert_stream(n, jpg, p)
        want.append(_decoded(n, jpg))
    sc = Client()
    sc.ingest_frames("pics", np.stack(pics))
    frame = sc.io.Input([NamedVideoStream(sc, "pics")])
    img = sc.ops.ImageEncoder(frame=frame, restart="none", device=DeviceType.GPU, batch=2)
    out = NamedStream(sc, "decoded")
    sc.run(sc.io.Output(sc.ops.ImageDecoder(img=img, device=DeviceType.GPU, batch=2, args={"entropy": "gpu", "split": "subsequence"}), [out]),
           PerfParams.estimate(), cache_mode=CacheMode.Overwrite)
    rows = list(out.load())
    assert len(rows) == 2
    for n, r, w in zip(names, rows, want):
        assert r.dtype == np.uint8 and r.shape == w.shape and np.array_equal(r, w), n
