"""Independent float64 definitions of every cv::cvtColor code ConvertColor accepts, used ONLY to cross-check the C oracle
(tests/test_color_float64.py) and the HIP ConvertColor kernels (tests/test_cvt_color_dispatch_gpu.py).

Everything here is written from the published formulas (OpenCV's "Color conversions" documentation, ITU-R BT.601, the
sRGB / D65 matrix, the FOURCC plane and byte layouts); nothing shares code or fixed-point tables with oracle/oracle.c or
the kernels.  Values are 8-bit levels, unrounded; the hexcone hues are in output units (hue range `hr`):

  luma        Y = 0.299 R + 0.587 G + 0.114 B
  YCrCb       Cr = (R - Y) 0.713 + 128, Cb = (B - Y) 0.564 + 128; inverse R = Y + 1.403 Cr', G = Y - 0.714 Cr' - 0.344 Cb',
              B = Y + 1.773 Cb' (x' = x - 128); stored Y, Cr, Cb
  YUV         U = (B - Y) 0.492 + 128, V = (R - Y) 0.877 + 128; inverse B = Y + 2.032 U', G = Y - 0.395 U' - 0.581 V',
              R = Y + 1.140 V'; stored Y, U, V
  XYZ         (X, Y, Z) = M (R, G, B) with the sRGB D65 matrix M; the inverse is numpy's inverse of M
  HSV         V = max, S = 255 (max - min) / max, H = hexcone angle x hr / 360 (hr 180, 256 for _FULL)
  HLS         L = (max + min) / 2, S = (max - min) / (max + min) below L = 1/2, (max - min) / (2 - max - min) above (on
              [0, 1]), H as HSV; the inverse codes read hue bytes modulo hr (180, 255 for _FULL): bytes past it wrap
  5x5         BGR565: b >> 3 | (g >> 2) << 5 | (r >> 3) << 11; BGR555: b >> 3 | (g >> 3) << 5 | (r >> 3) << 10 | alpha bit
              (source alpha != 0) << 15; little-endian 16-bit words; unpacking shifts the fields back up (low bits 0),
              alpha = 255 where bit 15 is set (555) or always (565); gray from a packed pixel is the luma of its fields
  4:2:0/4:2:2 NV12 = Y plane + one interleaved U V plane, NV21 the same with V U, I420 (IYUV) = Y + U plane + V plane,
              YV12 = Y + V plane + U plane, each chroma sample shared by a 2x2 block; YUY2 = Y0 U Y1 V, UYVY = U Y0 V Y1,
              YVYU = Y0 V Y1 U, one chroma pair per 2x1 block; BT.601 limited range R = 1.164 (Y - 16) + 1.596 V',
              G = 1.164 (Y - 16) - 0.813 V' - 0.391 U', B = 1.164 (Y - 16) + 2.018 U' with Y clamped below at 16

`bounds` states, per output channel, how far an 8-bit result may lie from these definitions, and why.
"""
import numpy as np

# ---- per-pixel colour formulas (float64 channel arrays in, tuple of float64 channel arrays out) --------------------


def luma(b, g, r):
    return 0.299 * r + 0.587 * g + 0.114 * b


def bgr2ycrcb(b, g, r):
    y = luma(b, g, r)
    return y, (r - y) * 0.713 + 128, (b - y) * 0.564 + 128


def ycrcb2bgr(y, cr, cb):
    cr, cb = cr - 128, cb - 128
    return y + 1.773 * cb, y - 0.714 * cr - 0.344 * cb, y + 1.403 * cr


def bgr2yuv(b, g, r):
    y = luma(b, g, r)
    return y, (b - y) * 0.492 + 128, (r - y) * 0.877 + 128


def yuv2bgr(y, u, v):
    u, v = u - 128, v - 128
    return y + 2.032 * u, y - 0.395 * u - 0.581 * v, y + 1.140 * v


SRGB_D65 = np.array([[0.412453, 0.357580, 0.180423],
                     [0.212671, 0.715160, 0.072169],
                     [0.019334, 0.119193, 0.950227]])


def rgb2xyz(r, g, b):
    return tuple(SRGB_D65[k, 0] * r + SRGB_D65[k, 1] * g + SRGB_D65[k, 2] * b for k in range(3))


def xyz2rgb(x, y, z):
    m = np.linalg.inv(SRGB_D65)
    return tuple(m[k, 0] * x + m[k, 1] * y + m[k, 2] * z for k in range(3))


def hexcone_hue(b, g, r, hr):
    """The hue angle of (b, g, r) in units of hr per turn, in [0, hr); 0 where max == min."""
    mx, mn = np.maximum(np.maximum(b, g), r), np.minimum(np.minimum(b, g), r)
    d = mx - mn
    dd = np.where(d > 0, d, 1.0)
    deg = np.where(mx == r, 60.0 * (g - b) / dd, np.where(mx == g, 120.0 + 60.0 * (b - r) / dd, 240.0 + 60.0 * (r - g) / dd))
    deg = np.where(d > 0, np.mod(deg, 360.0), 0.0)
    return deg * hr / 360.0


def bgr2hsv(b, g, r, hr):
    mx, mn = np.maximum(np.maximum(b, g), r), np.minimum(np.minimum(b, g), r)
    s = np.where(mx > 0, 255.0 * (mx - mn) / np.where(mx > 0, mx, 1.0), 0.0)
    return hexcone_hue(b, g, r, hr), s, mx


def hsv2bgr(h, s, v, hr):
    """h read modulo hr; the closed form c(n) = v - v s clip(min(k, 4 - k), 0, 1), k = (n + 6 h / hr) mod 6, n = 1, 3, 5
    for b, g, r (s on [0, 1], v in levels)."""
    h6 = np.mod(h, hr) * 6.0 / hr
    s = s / 255.0

    def c(n):
        k = np.mod(n + h6, 6.0)
        return v - v * s * np.clip(np.minimum(k, 4.0 - k), 0.0, 1.0)
    return c(1), c(3), c(5)


def bgr2hls(b, g, r, hr):
    mx, mn = np.maximum(np.maximum(b, g), r) / 255.0, np.minimum(np.minimum(b, g), r) / 255.0
    l, d = (mx + mn) / 2, mx - mn
    den = np.where(l < 0.5, mx + mn, 2.0 - mx - mn)
    s = np.where(d > 0, d / np.where(den > 0, den, 1.0), 0.0)
    return hexcone_hue(b, g, r, hr), 255.0 * l, 255.0 * s


def hls2bgr(h, l, s, hr):
    """h read modulo hr; c(n) = l - a clip(min(k - 3, 9 - k), -1, 1), a = s min(l, 1 - l), k = (n + 12 h / hr) mod 12,
    n = 0, 8, 4 for r, g, b (all on [0, 1], scaled to levels)."""
    h12 = np.mod(h, hr) * 12.0 / hr
    l, s = l / 255.0, s / 255.0
    a = s * np.minimum(l, 1.0 - l)

    def c(n):
        k = np.mod(n + h12, 12.0)
        return 255.0 * (l - a * np.clip(np.minimum(k - 3.0, 9.0 - k), -1.0, 1.0))
    return c(4), c(8), c(0)


def bt601_limited(y, u, v):
    """(b, g, r) of a limited-range BT.601 sample; Y below 16 is black."""
    yy = 1.164 * (np.maximum(y, 16.0) - 16.0)
    u, v = u - 128, v - 128
    return yy + 2.018 * u, yy - 0.813 * v - 0.391 * u, yy + 1.596 * v


# ---- 16-bit packed pixels (exact integer layouts) -------------------------------------------------------------------


def pack5x5(b, g, r, green_bits, alpha=None):
    """(lo, hi) bytes of the BGR565 (green_bits 6) / BGR555 (5) word; alpha (555 only) sets bit 15 where nonzero."""
    b, g, r = (np.asarray(x, np.int64) for x in (b, g, r))
    if green_bits == 6:
        w = (b >> 3) | ((g >> 2) << 5) | ((r >> 3) << 11)
    else:
        w = (b >> 3) | ((g >> 3) << 5) | ((r >> 3) << 10)
        if alpha is not None:
            w = w | (np.asarray(alpha) != 0).astype(np.int64) << 15
    return w & 255, w >> 8


def unpack5x5(lo, hi, green_bits):
    """(b, g, r, alpha) of a packed word."""
    w = np.asarray(lo, np.int64) | (np.asarray(hi, np.int64) << 8)
    b = (w & 31) << 3
    if green_bits == 6:
        return b, ((w >> 5) & 63) << 2, (w >> 11) << 3, np.full_like(w, 255)
    return b, ((w >> 5) & 31) << 3, ((w >> 10) & 31) << 3, np.where(w >> 15, 255, 0)


# ---- 4:2:0 / 4:2:2 source layouts -------------------------------------------------------------------------------------

# code -> (layout, output order, channels out); order 'bgr' / 'rgb' / 'gray'
YUV_SOURCES = {}
for _base, _lay in ((90, "NV12"), (92, "NV21"), (98, "YV12"), (100, "I420")):
    YUV_SOURCES[_base] = (_lay, "rgb", 3)
    YUV_SOURCES[_base + 1] = (_lay, "bgr", 3)
    YUV_SOURCES[_base + 4] = (_lay, "rgb", 4)
    YUV_SOURCES[_base + 5] = (_lay, "bgr", 4)
YUV_SOURCES[106] = ("I420", "gray", 1)          # gray from any 4:2:0 frame is its Y plane
for _base, _lay in ((107, "UYVY"), (115, "YUY2"), (117, "YVYU")):
    _rgba = _base + 4 if _lay != "UYVY" else 111
    YUV_SOURCES[_base] = (_lay, "rgb", 3)
    YUV_SOURCES[_base + 1] = (_lay, "bgr", 3)
    YUV_SOURCES[_rgba] = (_lay, "rgb", 4)
    YUV_SOURCES[_rgba + 1] = (_lay, "bgr", 4)
YUV_SOURCES[123] = ("UYVY", "gray", 1)
YUV_SOURCES[124] = ("YUY2", "gray", 1)          # = YVYU, YUYV, YUNV: the luma bytes sit where YUY2 has them

LAYOUTS_420 = ("NV12", "NV21", "YV12", "I420")
LAYOUTS_422 = ("YUY2", "UYVY", "YVYU")
# byte offsets of (Y0, U, Y1, V) inside a 4-byte 4:2:2 group
_G422 = {"YUY2": (0, 1, 2, 3), "UYVY": (1, 0, 3, 2), "YVYU": (0, 3, 2, 1)}


def yuv_layout_of(code):
    return YUV_SOURCES[code][0]


def decode_yuv(frame, layout):
    """(Y, U, V) uint8 planes at full resolution (H, W) of a 4:2:0 frame ((3H/2, W) or (3H/2, W, 1)) or a 4:2:2 frame
    ((H, W, 2)), each chroma sample replicated over the pixels that share it."""
    f = np.asarray(frame, np.uint8)
    if layout in LAYOUTS_420:
        f = f.reshape(f.shape[0], f.shape[1])
        h, w = f.shape[0] * 2 // 3, f.shape[1]
        y, c = f[:h], f[h:].reshape(-1)
        if layout in ("NV12", "NV21"):
            c = c.reshape(h // 2, w // 2, 2)
            u, v = (c[..., 0], c[..., 1]) if layout == "NV12" else (c[..., 1], c[..., 0])
        else:
            q = (h // 2) * (w // 2)
            p0, p1 = c[:q].reshape(h // 2, w // 2), c[q:].reshape(h // 2, w // 2)
            u, v = (p0, p1) if layout == "I420" else (p1, p0)
        up = lambda p: np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
        return y, up(u), up(v)
    h, w = f.shape[0], f.shape[1]
    g = f.reshape(h, w // 2, 4)
    oy0, ou, oy1, ov = _G422[layout]
    y = np.stack([g[..., oy0], g[..., oy1]], -1).reshape(h, w)
    return y, np.repeat(g[..., ou], 2, axis=1), np.repeat(g[..., ov], 2, axis=1)


def encode_yuv(y, u, v, layout):
    """The inverse of decode_yuv for planes whose chroma is constant over each block: (Y, U, V) full-resolution uint8
    planes -> the frame in `layout`."""
    h, w = y.shape
    if layout in LAYOUTS_420:
        cu, cv = u[0::2, 0::2], v[0::2, 0::2]
        if layout in ("NV12", "NV21"):
            c = np.stack([cu, cv] if layout == "NV12" else [cv, cu], -1).reshape(h // 2, w)
        else:
            c = np.concatenate([(cu if layout == "I420" else cv).reshape(-1), (cv if layout == "I420" else cu).reshape(-1)])
            c = c.reshape(h // 2, w)
        return np.concatenate([y, c], 0)[..., None].astype(np.uint8)
    g = np.empty((h, w // 2, 4), np.uint8)
    oy0, ou, oy1, ov = _G422[layout]
    g[..., oy0], g[..., oy1], g[..., ou], g[..., ov] = y[:, 0::2], y[:, 1::2], u[:, 0::2], v[:, 0::2]
    return g.reshape(h, w, 2)


def yuv_block_planes(rng, h, w, layout):
    """Random (Y, U, V) planes of an h x w frame whose chroma changes from block to block (2x2 for 4:2:0, 2x1 for 4:2:2)
    -- a wrong sample, plane or byte order moves a pixel onto a different chroma value."""
    y = rng.integers(0, 256, (h, w), dtype=np.uint8)
    by = 2 if layout in LAYOUTS_420 else 1
    cu = rng.integers(0, 256, (h // by, w // 2), dtype=np.uint8)
    cv = rng.integers(0, 256, (h // by, w // 2), dtype=np.uint8)
    up = lambda p: np.repeat(np.repeat(p, by, axis=0), 2, axis=1)
    return y, up(cu), up(cv)


def yuv_full_domain(layout, seed=0):
    """A 4096 x 4096 frame in `layout` that holds every (Y, U, V) triple exactly once: each block carries one (U, V) pair
    and 4 (4:2:0) or 2 (4:2:2) consecutive luma values; the blocks are shuffled, so neighbouring blocks (in either
    direction) hold unrelated chroma."""
    h = w = 4096
    bh = 2 if layout in LAYOUTS_420 else 1
    nb = (h // bh) * (w // 2)                                   # blocks: 2^22 (4:2:0) or 2^23 (4:2:2)
    per = nb // 65536                                           # blocks per (U, V) pair: 64 or 128
    blk = np.random.default_rng(seed).permutation(nb).astype(np.int64)
    uv, j = blk // per, blk % per
    u, v = (uv >> 8).astype(np.uint8), (uv & 255).astype(np.uint8)
    nl = 2 * bh                                                  # lumas per block
    y = np.empty((h // bh, w // 2, bh, 2), np.uint8)
    for k in range(nl):
        y[:, :, k // 2, k % 2] = ((j * nl + k) & 255).reshape(h // bh, w // 2)
    y = y.transpose(0, 2, 1, 3).reshape(h, w)
    up = lambda p: np.repeat(np.repeat(p.reshape(h // bh, w // 2), bh, axis=0), 2, axis=1)
    return encode_yuv(y, up(u), up(v), layout)


# ---- the code table ----------------------------------------------------------------------------------------------------

_HSV_FWD = {40: ("bgr", 180), 41: ("rgb", 180), 66: ("bgr", 256), 67: ("rgb", 256)}
_HSV_INV = {54: ("bgr", 180), 55: ("rgb", 180), 70: ("bgr", 255), 71: ("rgb", 255)}
_HLS_FWD = {52: ("bgr", 180), 53: ("rgb", 180), 68: ("bgr", 256), 69: ("rgb", 256)}
_HLS_INV = {60: ("bgr", 180), 61: ("rgb", 180), 72: ("bgr", 255), 73: ("rgb", 255)}
GRAY_TABLE_CODES = (6, 7, 10, 11)        # the codes whose luma uses the op's gray_bits table


def channels(code):
    """(source channels, destination channels) of a pixel code (not a 4:2:0 / 4:2:2 source)."""
    if code in (0, 2):
        return 3, 4
    if code in (1, 3):
        return 4, 3
    if code == 5:
        return 4, 4
    if code == 9:
        return 1, 4
    if code in (10, 11):
        return 4, 1
    if code in (6, 7):
        return 3, 1
    if code == 8:
        return 1, 3
    if 12 <= code <= 31:
        c = code - 12 if code < 22 else code - 22
        return [(3, 2), (3, 2), (2, 3), (2, 3), (4, 2), (4, 2), (2, 4), (2, 4), (1, 2), (2, 1)][c]
    return 3, 3


def _bgr_of(p, order):
    """(b, g, r) float64 channels of an (N, >= 3) pixel array stored in `order`."""
    p = p.astype(np.float64)
    return (p[:, 0], p[:, 1], p[:, 2]) if order == "bgr" else (p[:, 2], p[:, 1], p[:, 0])


def _out(order, b, g, r, alpha=None):
    ch = [b, g, r] if order == "bgr" else [r, g, b]
    if alpha is not None:
        ch.append(np.broadcast_to(np.asarray(alpha, np.float64), np.shape(b)))
    return np.stack([np.asarray(c, np.float64) for c in ch], 1)


def pixel_definition(code, p):
    """float64 (N, dcn) definition of `code` on the (N, scn) uint8 pixels p (any code that is not a 4:2:0 / 4:2:2
    source).  For a 4:2:0 / 4:2:2 code, p holds the decoded (Y, U, V) samples of each pixel (see decode_yuv)."""
    if code in YUV_SOURCES:
        _, order, dcn = YUV_SOURCES[code]
        y, u, v = (p[:, k].astype(np.float64) for k in range(3))
        if order == "gray":
            return y[:, None]
        b, g, r = bt601_limited(y, u, v)
        return _out(order, b, g, r, 255 if dcn == 4 else None)
    q = p.astype(np.int64)
    if code in (0, 2):                                           # BGR2BGRA, BGR2RGBA
        return _out("bgr" if code == 0 else "rgb", *_bgr_of(p, "bgr"), 255)
    if code in (1, 3):                                           # BGRA2BGR, RGBA2BGR
        return _out("bgr", *_bgr_of(p, "bgr" if code == 1 else "rgb"))
    if code == 5:                                                # BGRA2RGBA
        return _out("rgb", *_bgr_of(p, "bgr"), p[:, 3])
    if code == 4:
        return _out("rgb", *_bgr_of(p, "bgr"))
    if code in (8, 9):                                           # GRAY2BGR, GRAY2BGRA
        g = p[:, 0].astype(np.float64)
        return _out("bgr", g, g, g, 255 if code == 9 else None)
    if code in (6, 7, 10, 11):
        return luma(*_bgr_of(p, "bgr" if code in (6, 10) else "rgb"))[:, None]
    if 12 <= code <= 31:
        gb = 6 if code < 22 else 5
        c = code - 12 if code < 22 else code - 22
        if c in (0, 1, 4, 5):                                    # to packed, from BGR / RGB / BGRA / RGBA
            b, g, r = (q[:, 0], q[:, 1], q[:, 2]) if c in (0, 4) else (q[:, 2], q[:, 1], q[:, 0])
            lo, hi = pack5x5(b, g, r, gb, q[:, 3] if c in (4, 5) else None)
            return np.stack([lo, hi], 1).astype(np.float64)
        if c == 8:                                               # GRAY2BGR5x5
            lo, hi = pack5x5(q[:, 0], q[:, 0], q[:, 0], gb)
            return np.stack([lo, hi], 1).astype(np.float64)
        b, g, r, a = unpack5x5(q[:, 0], q[:, 1], gb)
        if c == 9:                                               # BGR5x52GRAY
            return luma(b.astype(np.float64), g, r)[:, None]
        return _out("bgr" if c in (2, 6) else "rgb", b, g, r, a if c in (6, 7) else None)
    if code in (32, 33):
        b, g, r = _bgr_of(p, "bgr" if code == 32 else "rgb")
        return np.stack(rgb2xyz(r, g, b), 1)
    if code in (34, 35):
        f = p.astype(np.float64)
        r, g, b = xyz2rgb(f[:, 0], f[:, 1], f[:, 2])
        return _out("bgr" if code == 34 else "rgb", b, g, r)
    if code in (36, 37):
        return np.stack(bgr2ycrcb(*_bgr_of(p, "bgr" if code == 36 else "rgb")), 1)
    if code in (82, 83):
        return np.stack(bgr2yuv(*_bgr_of(p, "bgr" if code == 82 else "rgb")), 1)
    if code in (38, 39, 84, 85):
        f = p.astype(np.float64)
        b, g, r = (ycrcb2bgr if code in (38, 39) else yuv2bgr)(f[:, 0], f[:, 1], f[:, 2])
        return _out("bgr" if code in (38, 84) else "rgb", b, g, r)
    if code in _HSV_FWD:
        order, hr = _HSV_FWD[code]
        return np.stack(bgr2hsv(*_bgr_of(p, order), hr), 1)
    if code in _HLS_FWD:
        order, hr = _HLS_FWD[code]
        return np.stack(bgr2hls(*_bgr_of(p, order), hr), 1)
    if code in _HSV_INV or code in _HLS_INV:
        order, hr = _HSV_INV[code] if code in _HSV_INV else _HLS_INV[code]
        f = p.astype(np.float64)
        if code in _HSV_INV:
            b, g, r = hsv2bgr(f[:, 0], f[:, 1], f[:, 2], hr)
        else:
            b, g, r = hls2bgr(f[:, 0], f[:, 1], f[:, 2], hr)
        return _out(order, b, g, r)
    raise KeyError(code)


ALL_CODES = sorted(set(range(0, 4)) | {4, 5, 6, 7, 8} | set(range(9, 36)) | {36, 37, 38, 39} | set(_HSV_FWD) | set(_HSV_INV)
                   | set(_HLS_FWD) | set(_HLS_INV) | {82, 83, 84, 85} | set(YUV_SOURCES))


def flow_gray(rgb):
    """st_gray_u8 / the flow path's gray: cv::cvtColor(COLOR_BGR2GRAY) applied to RGB frames, so byte 0 is weighted as
    blue -- 0.114 byte0 + 0.587 byte1 + 0.299 byte2 (the reference's quirk, kept)."""
    p = np.asarray(rgb).reshape(-1, 3).astype(np.float64)
    return luma(p[:, 0], p[:, 1], p[:, 2])


# ---- bounds --------------------------------------------------------------------------------------------------------------

# float32 arithmetic (the HSV / HLS float paths) moves a value by a few ulp of numbers below 360, and the byte / 255
# conversions' 2^-24 relative errors reach the hue through 60 / (max - min) <= 60 x 255: far below 0.01 of a level
FLOAT_SLACK = 0.01
BIAS = 0.02      # |mean signed error| of any channel that ends in one round-to-nearest (seen: <= 0.011)


def gray_bound(bits):
    """A luma table in `bits`-bit fixed point: each weight within one unit of its exact value and the three summing to
    exactly 2^bits (so gray(v, v, v) = v); the weight errors then cancel to at most one unit over 255, and the final
    rounding adds 0.5."""
    return 0.5 + 255.0 / 2 ** bits


def bounds(code, gray_bits=15):
    """[(kind, max |error|, max |mean signed error|), ...] per output channel of `code`; kind is 'v' for a plain value and
    ('hue', hr) for a hue compared on the circle of hr levels.  A bias bound of None is the HLS L tie rule below."""
    exact = ("v", 0.0, 0.0)
    if code in YUV_SOURCES:
        _, order, dcn = YUV_SOURCES[code]
        if order == "gray":
            return [exact]
        # 20-bit coefficients truncated from the decimal BT.601 values (each < 1 unit = 2^-20 below), applied to
        # |Y - 16| <= 239 and |U'|, |V'| <= 128: 0.5 + 512 x 2^-20 after the one rounding
        c = ("v", 0.5 + 512 * 2.0 ** -20, BIAS)
        return [c, c, c] + ([exact] if dcn == 4 else [])
    scn, dcn = channels(code)
    if code <= 5 or code in (8, 9) or (12 <= code <= 31 and code not in (21, 31)):
        return [exact] * dcn                                     # channel moves and bit packing: exact
    if code in GRAY_TABLE_CODES:
        return [("v", gray_bound(gray_bits), BIAS)]
    if code in (21, 31):                                         # RGB5x52Gray: the 14-bit table whatever gray_bits is
        return [("v", gray_bound(14), BIAS)]
    if code in (32, 33, 34, 35):
        # 12-bit coefficients (each within half a unit, 2^-13) over three channels of at most 255, one rounding;
        # XYZ2BGR adds the difference between OpenCV's six-decimal inverse matrix and the exact one (< 1e-6 per weight).
        # Bias: Z's three 12-bit weights all round down (0.53 units in all), about -0.53 x 127.5 / 4096 = -0.017 over
        # the cube, inside BIAS
        e = 0.5 + 3 * 255 * 2.0 ** -13 + (3 * 255 * 1e-6 if code >= 34 else 0)
        return [("v", e, BIAS)] * 3
    if code in (36, 37, 82, 83):
        # Y: the 14-bit luma table (gray_bound(14)).  The chroma is computed from the ROUNDED luma: its error reaches the
        # chroma times the gain (0.713 / 0.564, or 0.877 / 0.492), plus the gain's 14-bit quantisation (half a unit)
        # over |R - Y| <= 255, plus the final rounding
        ey = gray_bound(14)
        g1, g2 = (0.713, 0.564) if code in (36, 37) else (0.492, 0.877)
        return [("v", ey, BIAS)] + [("v", 0.5 + gg * ey + 255 * 2.0 ** -15, BIAS) for gg in (g1, g2)]
    if code in (38, 39, 84, 85):
        # Y + round(14-bit gains x chroma): one rounding, at most two gains (half a unit each) over |x - 128| <= 128
        return [("v", 0.5 + 256 * 2.0 ** -15, BIAS)] * 3
    if code in _HSV_FWD:
        hr = _HSV_FWD[code][1]
        # H: the hue division table holds round(hr 2^12 / (6 diff)) (half a unit off); the sector numerator is exact and
        # at most 5 diff, so the table costs <= 5 x 255 x 2^-13.  HSV_FULL: a hue that rounds to 256 saturates to 255
        # instead of wrapping to 0 (saturate_cast), a miss of up to one level on the circle.
        eh = 0.5 + 5 * 255 * 2.0 ** -13 if hr == 180 else 1.0
        # S: diff x round(255 2^12 / V) / 2^12: the table's half unit over diff <= 255
        return [(("hue", hr), eh, BIAS), ("v", 0.5 + 255 * 2.0 ** -13, BIAS), exact]
    if code in _HLS_FWD:
        hr = _HLS_FWD[code][1]
        # float32 throughout, one rounding per channel; HLS_FULL hue saturates at 255 like HSV_FULL.
        # L (bias None): L = (max + min) / 2 is a tie k + 1/2 whenever max + min is odd, and OpenCV computes it as
        # (max/255 + min/255) x 0.5 x 255 in float32, which lands a few ulp to either side of the tie -- not evenly (on the
        # byte cube most ties come out above), so round-half-even does not balance them and each tie may add up to
        # +-1/2: the bias bound is half the fraction of exact ties in the definition plus BIAS (Stats.check)
        eh = 0.5 + FLOAT_SLACK if hr == 180 else 1.0
        return [(("hue", hr), eh, BIAS), ("v", 0.5 + FLOAT_SLACK, None), ("v", 0.5 + FLOAT_SLACK, BIAS)]
    if code in _HSV_INV or code in _HLS_INV:
        return [("v", 0.5 + FLOAT_SLACK, BIAS)] * 3              # float32, one rounding per channel
    raise KeyError(code)


class Stats:
    """Running per-channel max |error|, sum of signed errors and counts of a uint8 result against a float64 definition
    (clipped to [0, 255]; hues compared on their circle), fed chunk by chunk."""

    def __init__(self, kinds, count_ties=None):
        self.kinds = kinds
        n = len(kinds)
        self.count_ties = count_ties or [False] * n
        self.emax, self.esum, self.n, self.where = np.zeros(n), np.zeros(n), 0, [None] * n
        self.ties = np.zeros(n)          # definition values that are exact ties k + 1/2

    def add(self, got, ref, src=None):
        got = np.asarray(got, np.float64).reshape(ref.shape)
        for k, kind in enumerate(self.kinds):
            if kind[0] == "v":
                e = got[:, k] - np.clip(ref[:, k], 0, 255)
            else:
                hr = kind[1]
                e = np.mod(got[:, k] - ref[:, k] + hr / 2.0, hr) - hr / 2.0
            i = int(np.argmax(np.abs(e)))
            if abs(e[i]) > self.emax[k]:
                self.emax[k] = abs(e[i])
                self.where[k] = (None if src is None else np.asarray(src)[i].tolist(), float(got[i, k]), float(ref[i, k]))
            self.esum[k] += e.sum()
            if self.count_ties[k]:
                r = ref[:, k]
                self.ties[k] += np.count_nonzero(np.abs(r - np.floor(r) - 0.5) < 1e-9)
        self.n += ref.shape[0]

    def merge(self, other):
        for k in range(len(self.kinds)):
            if other.emax[k] > self.emax[k]:
                self.emax[k], self.where[k] = other.emax[k], other.where[k]
        self.esum += other.esum
        self.ties += other.ties
        self.n += other.n

    def bias(self):
        return self.esum / max(self.n, 1)

    def check(self, bnds, what, bias=True):
        """Assert the bounds; `bias` False skips the mean-signed-error bounds (small inputs)."""
        b = self.bias()
        for k, (kind, emax, btol) in enumerate(bnds):
            assert self.emax[k] <= emax + 1e-9, "%s channel %d: max error %.4f > %.4f (at source %s: got %s, definition %s)" % (
                what, k, self.emax[k], emax, *(self.where[k] or (None, None, None)))
            if bias:
                tol = btol if btol is not None else 0.5 * self.ties[k] / max(self.n, 1) + BIAS
                assert abs(b[k]) <= tol, "%s channel %d: mean signed error %+.4f beyond %.4f" % (what, k, b[k], tol)


# ---- input domains --------------------------------------------------------------------------------------------------------


def pixel_domain(scn):
    """Every value a pixel of `scn` channels can take, as one frame: the 2^24 byte cube (4096 x 4096 x 3; the 4-channel
    domain adds an alpha byte from a fixed random sequence, every alpha value ~65 000 times), all 65 536 packed 16-bit
    pixels (256 x 256 x 2) or all 256 grays (16 x 16 x 1)."""
    if scn == 1:
        return np.arange(256, dtype=np.uint8).reshape(16, 16, 1)
    if scn == 2:
        return np.arange(65536, dtype="<u2").view(np.uint8).reshape(256, 256, 2)
    cube = np.arange(1 << 24, dtype="<u4").view(np.uint8).reshape(-1, 4)
    if scn == 3:
        return np.ascontiguousarray(cube[:, :3]).reshape(4096, 4096, 3)
    out = cube.copy()
    out[:, 3] = np.random.default_rng(4).integers(0, 256, 1 << 24, dtype=np.uint8)
    return out.reshape(4096, 4096, 4)


CHUNK = 1 << 19


def _pool():
    global _POOL
    if _POOL is None:
        import concurrent.futures
        import os
        _POOL = concurrent.futures.ThreadPoolExecutor(max(1, min(8, os.cpu_count() or 1)))
    return _POOL


_POOL = None


def check_pixels(code, src, got, what, gray_bits=15, bias=True):
    """Assert `bounds` for a result `got` of `code` on the pixels `src` (any shapes holding (N, scn) / (N, dcn)); chunks of
    CHUNK pixels on a few threads (numpy releases the interpreter lock).  Returns the Stats."""
    bnds = bounds(code, gray_bits)
    scn = src.shape[-1] if src.ndim > 1 else 1
    src, got = np.asarray(src).reshape(-1, scn), np.asarray(got).reshape(-1, len(bnds))
    kinds, ties = [b[0] for b in bnds], [b[2] is None for b in bnds]

    def part(i):
        st = Stats(kinds, ties)
        st.add(got[i:i + CHUNK], pixel_definition(code, src[i:i + CHUNK]), src[i:i + CHUNK])
        return st

    st = Stats(kinds, ties)
    for p in _pool().map(part, range(0, src.shape[0], CHUNK)):
        st.merge(p)
    st.check(bnds, what, bias)
    return st


def check_yuv(code, frame, got, what, bias=True):
    """check_pixels for a 4:2:0 / 4:2:2 source frame: the definition runs on its decoded (Y, U, V) samples."""
    y, u, v = decode_yuv(frame, yuv_layout_of(code))
    return check_pixels(code, np.stack([y, u, v], -1), got, what, bias=bias)
