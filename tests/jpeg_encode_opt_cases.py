"""The pictures and cases of tests/golden/jpeg_encode_opt_golden.npz, shared by its generator
(tests/golden/make_jpeg_encode_opt_golden.py) and by tests/test_jpeg_encode_opt.py and tests/test_jpeg_encode_opt_gpu.py.  The
pictures are not stored: picture(kind, h, w, seed) rebuilds each one in integer arithmetic alone, and the file holds the SHA-256
of its bytes beside the stream Pillow wrote for it with optimize=True -- the stream itself up to STORED_STREAM_LIMIT bytes, its
length and SHA-256 beyond.

A case is one picture at one quality, sampling and restart mode ("row": restart_marker_rows=1; "none": Pillow's default).
"""
import hashlib

import numpy as np

SAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
RESTARTS = ("row", "none")
QUALITIES = (1, 50, 75, 95, 100)
KINDS = ("flat", "smooth", "noise", "twolevel")
STORED_STREAM_LIMIT = 2500


def picture(kind, h, w, seed):
    """(h, w, 3) uint8, a function of the arguments alone.
    flat: one colour.  gray: one gray level (chroma exactly 128: every chroma DC difference is 0).
    smooth: per channel a ramp along x plus one along y.  noise: every sample uniform in 0 .. 255.
    twolevel: each pixel one of two colours, in blotches of a few pixels."""
    rng = np.random.default_rng(seed)
    if kind == "flat":
        return np.broadcast_to(rng.integers(0, 256, 3, dtype=np.uint8), (h, w, 3)).copy()
    if kind == "gray":
        return np.full((h, w, 3), int(rng.integers(0, 256)), np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    y, x = np.arange(h, dtype=np.int64)[:, None], np.arange(w, dtype=np.int64)[None, :]
    if kind == "smooth":
        par = rng.integers(1, 6, (3, 2))
        return np.stack([((x * par[c, 0] + y * par[c, 1]) * 255 // ((w - 1) * par[c, 0] + (h - 1) * par[c, 1] + 1)) for c in range(3)],
                        axis=-1).astype(np.uint8)
    if kind == "twolevel":
        a, b = rng.integers(0, 256, (2, 3), dtype=np.uint8)
        mask = rng.integers(0, 2, (-(-h // 3), -(-w // 5)), dtype=np.uint8)
        mask = np.repeat(np.repeat(mask, 3, axis=0), 5, axis=1)[:h, :w, None]
        return np.where(mask == 1, a, b).astype(np.uint8)
    raise ValueError("no picture of kind %r" % (kind,))


def sha256(data):
    return hashlib.sha256(bytes(data)).hexdigest()


def case_name(c):
    return "%dx%d_%s%d_q%d_%s_%s" % (c["h"], c["w"], c["kind"], c["seed"], c["quality"], c["subsampling"].replace(":", ""), c["restart"])


def _case(h, w, kind, seed, quality, subsampling, restart, uses=()):
    return dict(h=h, w=w, kind=kind, seed=seed, quality=quality, subsampling=subsampling, restart=restart, uses=list(uses))


def _both(h, w, kind, seed, quality, subsampling, uses=()):
    return [_case(h, w, kind, seed, quality, subsampling, r, uses) for r in RESTARTS]


def _grid():
    """Both restart modes x the three samplings x the five qualities x the four contents: in full at 40 x 34 (h x w; edge and
    padding blocks at every sampling), and at the other sizes one quality and one content per (size, sampling) in rotation, so that
    every size meets every quality, sampling and content."""
    out, turn = [], 0
    for sub in SAMPLING:
        for q in QUALITIES:
            for ki, kind in enumerate(KINDS):
                out += _both(40, 34, kind, 10 + ki, q, sub, ["batch"] if (q, sub) == (75, "4:2:0") else ())
    for si, (h, w) in enumerate(((8, 8), (47, 33), (300, 17), (130, 100))):
        for sub in SAMPLING:
            for k in range(5):
                out += _both(h, w, KINDS[(turn + k) % 4], 20 + si, QUALITIES[(turn + 2 * k) % 5], sub)
            turn += 1
    return out


# Flat pictures 8 pixels wide at 4:4:4 have MCU rows of 6 bits after the first: the shortest rows any table allows.  Together
# these colours and heights give the streams without restart markers rows that own no byte, bytes made of three rows' bits, and
# padding bits in a byte that an earlier row than the last owns (the generator asserts it before it writes the file, and
# tests/test_jpeg_encode_opt.py finds it again); the first rows differ in length, so the 6-bit rows start at different bit phases.
SHORT_ROW_HEIGHTS = (512, 200, 72, 64, 40, 24)
SHORT_ROW_SEEDS = (0, 1, 2, 3, 4, 5)


def _special():
    out = []
    # code lengths above 16 before the limiting
    for q in (95, 100):
        out += _both(256, 256, "noise", 30, q, "4:4:4", ["long_codes"])
    for h, seed in zip(SHORT_ROW_HEIGHTS, SHORT_ROW_SEEDS):
        out += _both(h, 8, "flat", seed, 90, "4:4:4", ["short_rows"])
    out += _both(512, 8, "gray", 6, 90, "4:4:4", ["short_rows"])                    # every table but the luma DC one has ONE symbol
    out += _both(120, 16, "flat", 7, 90, "4:2:2", ["short_rows"]) + _both(240, 16, "flat", 8, 90, "4:2:0", ["short_rows"])   # rows of 8 and 12 bits
    out += _both(64, 8, "noise", 31, 90, "4:4:4", ["mixed"])                       # beside 64x8 flat in one call
    # -- the GPU tests' geometry: 258 MCU rows (the sum over the rows above takes a second turn of 256 threads), 198 blocks in a
    # row (the statistics wave takes a second, third and fourth chunk)
    out += _both(2064, 8, "flat", 9, 90, "4:4:4", ["tall"]) + _both(2064, 8, "noise", 32, 75, "4:4:4", ["tall"])
    out += _both(8, 528, "noise", 33, 75, "4:4:4", ["wide"]) + _both(8, 528, "smooth", 34, 95, "4:2:0", ["wide"])
    return out


CASES = tuple(_grid() + _special())


def pillow_settings(c):
    """The keywords of Pillow's save() for a case."""
    kw = dict(quality=c["quality"], subsampling=c["subsampling"], optimize=True)
    if c["restart"] == "row":
        kw["restart_marker_rows"] = 1
    return kw
