"""The frames the PNG encoder is tested on (tests/test_png_encode.py without a GPU, tests/test_png_encode_gpu.py on one).
CASES: name -> (frame, filter).  PICTURES: the names whose size is compared with zlib's Z_RLE; the others are adversarial."""
import numpy as np

FILTERS = ("none", "sub", "up", "average", "paeth", "adaptive")
RUN_LENGTHS = (1, 2, 3, 4, 258, 259, 260, 261, 262, 517, 518)


def gradient(h, w, c, seed=0):
    y, x = np.mgrid[0:h, 0:w]
    return ((3 * x + 2 * y)[..., None] + 40 * np.arange(c) & 255).astype(np.uint8)


def photo(h, w, c, seed=1):
    """smooth + sigma = 4 noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 128 + 90 * np.sin(x / 23.0)[..., None] * np.cos(y[..., None] / 17.0 + np.arange(c))
    return np.clip(base + rng.normal(0, 4, (h, w, c)), 0, 255).astype(np.uint8)


def noise(h, w, c, seed=2):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c)).astype(np.uint8)


def sheet(h, w, c, seed=3):
    """a picture pasted on a flat sheet, as Montage makes them"""
    out = np.zeros((h, w, c), np.uint8)
    ph, pw = h // 2, w // 2
    out[h // 4:h // 4 + ph, w // 4:w // 4 + pw] = photo(ph, pw, c, seed)
    return out


def run_lengths():
    """one row: runs of every length in RUN_LENGTHS of the value 7 between bytes that differ from it and from each other"""
    row, sep = [], 1
    for r in RUN_LENGTHS + RUN_LENGTHS[::-1]:
        row += [7] * r + [sep]
        sep = 3 - sep
    return np.array(row, np.uint8).reshape(1, -1, 1)


def fibonacci_piece():
    """one row of one piece whose symbol counts are Fibonacci numbers -- 1 for the filter-type byte 0, 1 for the end of the block,
    then 2, 3, 5 .. 10 946 for the values 1..19; 28 654 bytes, no two equal neighbours: an unlimited Huffman code would be 20
    bits deep"""
    fib = [2, 3]
    while len(fib) < 19:
        fib.append(fib[-1] + fib[-2])
    vals = np.concatenate([np.full(n, v + 1, np.uint8) for v, n in sorted(enumerate(fib), key=lambda t: -t[1])])
    out = np.zeros(len(vals), np.uint8)
    half = (len(vals) + 1) // 2
    out[0::2], out[1::2] = vals[:half], vals[half:]
    assert (out[1:] != out[:-1]).all()
    return out.reshape(1, -1, 1)


def mixed():
    """three pieces of 32 rows: noise (stored), flat (coded), noise again"""
    out = np.zeros((96, 1023, 1), np.uint8)
    out[:32] = noise(32, 1023, 1, 5)
    out[64:] = noise(32, 1023, 1, 6)
    return out


def _cases():
    c = {}
    for ch in (1, 3, 4):
        c["1x1x%d" % ch] = (np.full((1, 1, ch), 200, np.uint8), "adaptive")
    c["1x5x3"] = (photo(1, 5, 3), "adaptive")
    c["5x1x3"] = (photo(5, 1, 3), "adaptive")
    c["3x7x3"] = (photo(3, 7, 3), "adaptive")
    c["17x21x4"] = (photo(17, 21, 4), "adaptive")
    c["33x65x3"] = (photo(33, 65, 3), "adaptive")
    c["64x64x3"] = (photo(64, 64, 3), "adaptive")
    # filtered sizes 32 767, 32 768 and 32 769: one short piece, one full piece, one piece and a byte
    c["7x4680x1_32767"] = (photo(7, 4680, 1), "adaptive")
    c["128x255x1_32768"] = (photo(128, 255, 1), "adaptive")
    c["33x992x1_32769"] = (photo(33, 992, 1), "adaptive")
    c["zeros_128x1023x1"] = (np.zeros((128, 1023, 1), np.uint8), "none")   # 4 pieces, a run across every boundary
    c["zeros_40x50x3"] = (np.zeros((40, 50, 3), np.uint8), "adaptive")
    c["ones_40x50x4"] = (np.full((40, 50, 4), 255, np.uint8), "adaptive")
    c["ones_none_64x700x1"] = (np.full((64, 700, 1), 255, np.uint8), "none")
    c["runs"] = (run_lengths(), "none")
    c["noise_90x130x3"] = (noise(90, 130, 3), "none")   # every piece stored
    c["mixed"] = (mixed(), "none")
    c["fibonacci"] = (fibonacci_piece(), "none")
    for f in FILTERS:
        c["gradient_%s" % f] = (gradient(40, 61, 3), f)
        c["noise_%s" % f] = (noise(19, 23, 3, 7), f)
        c["sheet_%s" % f] = (sheet(48, 70, 3), f)
    c["photo_96x128x3"] = (photo(96, 128, 3), "adaptive")
    c["photo_gray_180x200"] = (photo(180, 200, 1), "adaptive")
    c["photo_rgba_100x90"] = (photo(100, 90, 4), "adaptive")
    c["sheet_160x200x3"] = (sheet(160, 200, 3), "adaptive")
    return c


CASES = _cases()
# The pictures whose size is compared with zlib's Z_RLE: every photo-like, gradient and sheet-like frame (noise, flat frames, the
# run and Fibonacci rows and the 1 x 1 frames are adversarial).  PICTURES have at least one piece of filtered bytes (the three
# boundary cases count: 32 767 bytes and up) and are held to a ratio.  SMALL_PICTURES are below a piece -- thumbnails -- and are
# held to a number of bytes over Z_RLE instead: a piece carries its own code tables, this format writes dynamic blocks only and
# no run symbols in the code-length sequence, so what it loses to zlib there is a fixed cost per block, not a share of the stream.
PICTURES = ("photo_96x128x3", "photo_gray_180x200", "photo_rgba_100x90", "sheet_160x200x3", "7x4680x1_32767", "128x255x1_32768",
            "33x992x1_32769")
SMALL_PICTURES = ("1x5x3", "5x1x3", "3x7x3", "17x21x4", "33x65x3", "64x64x3") + tuple("%s_%s" % (k, f) for k in ("gradient", "sheet") for f in FILTERS)
