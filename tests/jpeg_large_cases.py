"""The pictures and cases of tests/golden/jpeg_large_golden.npz, shared by its generator (tests/golden/make_jpeg_large_golden.py)
and by tests/test_jpeg_large.py and tests/test_jpeg_large_gpu.py.  The pictures are not stored: picture(kind, h, w, seed, channels)
rebuilds each one, in integer arithmetic alone, and the file holds the SHA-256 of its bytes beside what Pillow made of it.

A case is one picture at one setting.  "role" says what the file holds for it: "encode" -- Pillow's stream for save(quality,
subsampling) with restart "none" (Pillow's default) or "row" (restart_marker_rows=1), which ImageEncoder must write byte for
byte; "decode" -- a stream Pillow wrote, which the ImageDecoder paths must decode to what Pillow decodes it to.  "uses" names
the tests of test_jpeg_large_gpu.py that read the case.
"""
import hashlib

import numpy as np

SAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
STORED_STREAM_LIMIT = 350 * 1000   # a longer stream is kept as its length and SHA-256


def _triangle(t, period):
    """0 .. 255 .. 0 over 2 * period steps of t, integers only."""
    t = t % (2 * period)
    return (period - np.abs(t - period)) * 255 // period


def picture(kind, h, w, seed, channels=3):
    """(h, w, channels) uint8, a function of the arguments alone.
    noise: every sample uniform in 0 .. 255.
    flat: one colour.
    smooth: per channel the mean of a triangle wave along x and one along y, periods of 90 .. 400 pixels.
    grain: smooth with -2 .. 2 of noise on it.
    qflat: every 8 x 8 block one of 16 levels (DC terms only, whatever the quality)."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, channels), dtype=np.uint8)
    if kind == "flat":
        return np.broadcast_to(rng.integers(0, 256, channels, dtype=np.uint8), (h, w, channels)).copy()
    if kind in ("smooth", "grain"):
        y, x = np.arange(h, dtype=np.int64)[:, None], np.arange(w, dtype=np.int64)[None, :]
        par = rng.integers(90, 400, (channels, 4))
        img = np.stack([(_triangle(x + par[c, 2], par[c, 0]) + _triangle(y + par[c, 3], par[c, 1])) // 2 for c in range(channels)], axis=-1)
        if kind == "grain":
            img = np.clip(img + rng.integers(-2, 3, img.shape), 0, 255)
        return img.astype(np.uint8)
    if kind == "qflat":
        lv = rng.integers(0, 16, (-(-h // 8), -(-w // 8), channels), dtype=np.uint8) * 16 + 8
        return np.repeat(np.repeat(lv, 8, axis=0), 8, axis=1)[:h, :w].copy()
    raise ValueError("no picture of kind %r" % (kind,))


def sha256(data):
    return hashlib.sha256(bytes(data)).hexdigest()


def stored(c, jpg_len):
    """Whether the file holds the case's stream itself."""
    return c["store"] and jpg_len <= STORED_STREAM_LIMIT


def case_name(c):
    name = "%s_%dx%d_%s%d_q%d" % (c["role"][:3], c["h"], c["w"], c["kind"], c["seed"], c["quality"])
    if c["channels"] == 3:
        name += "_" + c["subsampling"].replace(":", "")
    return name + {"none": "", "row": "_rstrow"}.get(c["restart"], "_rst%s" % c["restart"])


def _enc(h, w, kind, seed, quality, subsampling, uses, store=True):
    """store=False: the file holds the stream's length and SHA-256 whatever its length (the file has a cap of its own)."""
    return [dict(role="encode", h=h, w=w, channels=3, kind=kind, seed=seed, quality=quality, subsampling=subsampling, restart=r, uses=uses,
                 store=store) for r in ("none", "row")]


def _dec(h, w, kind, seed, quality, subsampling, restart, uses, channels=3):
    """restart: "none", "row" (restart_marker_rows=1) or a number of MCUs (restart_marker_blocks)."""
    return [dict(role="decode", h=h, w=w, channels=channels, kind=kind, seed=seed, quality=quality, subsampling=subsampling, restart=restart, uses=uses,
                 store=True)]


# Every shape is the smallest that crosses the threshold its comment names.
CASES = (
    # -- encoder: more MCU rows than k_jpeg_ff_count's 256 threads (258, 261), more than its first wave (130), rows of
    # 14 / 20 / 32 bits over 300 rows; the second picture of a shape is for the two-frame calls
    _enc(2064, 8, "noise", 1, 95, "4:4:4", ["tall"]) + _enc(2064, 8, "noise", 2, 95, "4:4:4", ["tall_pair"])
    + _enc(4176, 16, "noise", 3, 50, "4:2:0", ["tall"]) + _enc(4176, 16, "noise", 4, 50, "4:2:0", ["tall_pair"])
    + _enc(1040, 24, "noise", 5, 75, "4:2:2", ["tall"])
    # (at quality 100 a row ends in magnitude bits, not in an end-of-block code: seed 30 is the first from 30 up whose stream
    # without restart markers has a 0xFF byte made of two rows' bits)
    + _enc(2064, 8, "noise", 30, 100, "4:4:4", ["tall"])[:1]
    + _enc(2400, 8, "flat", 6, 95, "4:4:4", ["tall"]) + _enc(2400, 5, "flat", 7, 95, "4:2:2", ["tall"]) + _enc(4800, 3, "flat", 8, 95, "4:2:0", ["tall"])
    # -- encoder: the widest frame libjpeg writes: 384 chunks of 64 blocks per row, the longest row in bits, thousands of
    # 256-byte pack steps; 9 rows at 4:2:2 add a row of padding blocks
    + _enc(8, 65500, "noise", 9, 100, "4:4:4", ["wide"]) + _enc(16, 65500, "noise", 10, 95, "4:2:0", ["wide"])
    + _enc(9, 65500, "smooth", 11, 75, "4:2:2", ["wide"])
    # -- encoder: the workload's frame, twice for the round trip; 640 x 648 noise is the stream of more than 65 536
    # subsequences of 8 bytes
    + _enc(1080, 1920, "grain", 12, 95, "4:2:0", ["workload", "round_trip"], store=False) + _enc(1080, 1920, "grain", 13, 95, "4:2:0", ["round_trip"], store=False)
    + _enc(640, 648, "noise", 14, 95, "4:4:4", ["subsequences"])[:1]
    # -- decoder: more than 2 097 152 pixels at an odd width (k_jpeg_color<1> strides), and at a width of 4 k for the
    # frame written at an odd address
    + _dec(1449, 1451, "smooth", 20, 30, "4:2:0", "none", ["color_stride"]) + _dec(1449, 1451, "smooth", 21, 30, "4:2:2", "none", ["color_stride"])
    + _dec(1448, 1452, "smooth", 22, 30, "4:2:0", "none", ["color_stride_offset"])
    # -- decoder: 12.7 MB of coefficients per frame, two pictures, restart markers per MCU row for the device paths
    + _dec(1449, 1451, "smooth", 23, 30, "4:4:4", "row", ["byte_cut"]) + _dec(1449, 1451, "smooth", 24, 30, "4:4:4", "row", ["byte_cut"])
    # -- decoder: 66 049 restart intervals of one block; 1 089 intervals of three components
    + _dec(2056, 2056, "qflat", 25, 75, None, 1, ["many_intervals"], channels=1)
    + _dec(520, 520, "smooth", 26, 75, "4:2:0", 1, ["many_segments"])
)
CASES = tuple(CASES)


# The byte_cut call: its two streams in an order without a period, whose second sub-batch (the sixth and seventh stream) does
# not repeat the start of the first.
BYTE_CUT_ORDER = (0, 1, 1, 0, 1, 1, 0)


def pillow_settings(c):
    """The keywords of Pillow's save() for a case."""
    kw = dict(quality=c["quality"])
    if c["channels"] == 3:
        kw["subsampling"] = c["subsampling"]
    if c["restart"] == "row":
        kw["restart_marker_rows"] = 1
    elif c["restart"] != "none":
        kw["restart_marker_blocks"] = int(c["restart"])
    return kw


def enc_geometry(h, w, subsampling):
    """st_jpeg_enc_geom restated: MCU columns and rows, blocks per MCU, and the 64-block chunks k_jpeg_entropy takes a row in."""
    hs, vs = SAMPLING[subsampling]
    mcols, mrows, bpm = -(-w // (8 * hs)), -(-h // (8 * vs)), hs * vs + 2
    return dict(mcols=mcols, mrows=mrows, bpm=bpm, chunks=-(-mcols * bpm // 64))


def dec_blocks(h, w, channels, subsampling):
    """st_jpeg_blocks restated: the 8 x 8 blocks of a frame's coefficients, 128 bytes each."""
    hs, vs = SAMPLING[subsampling] if channels == 3 else (1, 1)
    mcux, mcuy = -(-w // (8 * hs)), -(-h // (8 * vs))
    return mcux * mcuy * (hs * vs + 2 if channels == 3 else 1)
