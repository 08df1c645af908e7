"""Independent float64 definitions of the five cv::resize modes, used ONLY to cross-check the C oracle
(tests/test_resize_float64.py) and the HIP resize kernels (tests/test_resize_dispatch_gpu.py).

Each mode is written from its textbook definition as a separable pair of (dst, src) weight matrices applied in
float64; nothing here shares code or fixed-point tables with oracle/oracle.c or the kernels:

  nearest   sx = floor(dx * scale), clamped to the last column
  linear    half-pixel centres, sx = (dx + 0.5) * scale - 0.5, two taps, sample position clamped to [0, w-1]
  cubic     half-pixel centres, Keys' kernel with A = -0.75, four taps, replicate border (clamped source index)
  lanczos4  half-pixel centres, 8-tap sinc(x) sinc(x/4) window normalised to sum 1, replicate border
  area      both axes shrinking (scale >= 1): the overlap-weighted mean of the source over each destination cell;
            any axis enlarging: cv::resize's INTER_AREA enlargement rule, two taps with the weight of the
            right-hand pixel equal to its overlap with the destination cell (the box average on an enlarging axis,
            fx = (dx + 1) - (sx + 1) / scale folded to [0, 1) on a shrinking one)

scale = src / dst per axis.  As in cv::resize, an equal size is a copy and INTER_LINEAR at an exact 2 x 2
decimation is the 2 x 2 mean (= area).  Frames are (h, w) or (h, w, c) with any c; the result is float64, unrounded.
"""
import numpy as np

NEAREST, LINEAR, CUBIC, AREA, LANCZOS4 = 0, 1, 2, 3, 4


def _nearest_w(src, dst):
    s = 1.0 / (dst / src)          # cv::resize's scale: the reciprocal of dst / src, as floor() sees it
    m = np.zeros((dst, src))
    m[np.arange(dst), np.minimum(np.floor(np.arange(dst) * s).astype(int), src - 1)] = 1.0
    return m


def _linear_w(src, dst):
    s = src / dst
    m = np.zeros((dst, src))
    for d in range(dst):
        x = min(max((d + 0.5) * s - 0.5, 0.0), src - 1.0)
        i = int(np.floor(x))
        f = x - i
        m[d, i] += 1 - f
        if f > 0:
            m[d, i + 1] += f
    return m


def _cubic_kernel(t, a=-0.75):
    t = abs(t)
    if t <= 1:
        return (a + 2) * t ** 3 - (a + 3) * t ** 2 + 1
    if t < 2:
        return a * t ** 3 - 5 * a * t ** 2 + 8 * a * t - 4 * a
    return 0.0


def _lanczos_kernel(t, a=4):
    if t == 0:
        return 1.0
    if abs(t) >= a:
        return 0.0
    pt = np.pi * t
    return a * np.sin(pt) * np.sin(pt / a) / (pt * pt)


def _taps_w(src, dst, kern, lo, hi, normalise):
    """Taps floor(x)+lo .. floor(x)+hi at x = (d + 0.5) * scale - 0.5, indices clamped into the frame (replicate)."""
    s = src / dst
    m = np.zeros((dst, src))
    for d in range(dst):
        x = (d + 0.5) * s - 0.5
        i0 = int(np.floor(x))
        ks = [(i0 + k, kern(x - (i0 + k))) for k in range(lo, hi + 1)]
        tot = sum(wt for _, wt in ks) if normalise else 1.0
        for i, wt in ks:
            m[d, min(max(i, 0), src - 1)] += wt / tot
    return m


def _box_w(src, dst):
    """Overlap of destination cell d, [d*s, (d+1)*s), with source pixel i, normalised per cell."""
    s = src / dst
    m = np.zeros((dst, src))
    for d in range(dst):
        lo, hi = d * s, min((d + 1) * s, src)
        for i in range(int(np.floor(lo)), int(np.ceil(hi))):
            m[d, i] = max(0.0, min(hi, i + 1) - max(lo, i))
        m[d] /= m[d].sum()
    return m


def box_average(a, dh, dw):
    """Definition of area resampling: mean of the source (h, w, c) over each destination cell, cells of fractional
    extent weighted by their overlap (float64)."""
    return np.einsum("yi,ijc,xj->yxc", _box_w(a.shape[0], dh), np.asarray(a, np.float64), _box_w(a.shape[1], dw))


def _area_up_w(src, dst):
    """cv::resize INTER_AREA when either axis enlarges: sx = floor(d * s), the right tap's weight is
    fx = (d + 1) - (sx + 1) / s reduced to its fractional part (0 when <= 0), the tap index clamped."""
    s = src / dst
    m = np.zeros((dst, src))
    for d in range(dst):
        sx = int(np.floor(d * s))
        fx = (d + 1) - (sx + 1) / s
        fx = 0.0 if fx <= 0 else fx - np.floor(fx)
        m[d, min(sx, src - 1)] += 1 - fx
        m[d, min(sx + 1, src - 1)] += fx
    return m


def weights(mode, src, dst, other_src=None, other_dst=None):
    """(dst, src) float64 weight matrix of one axis.  other_* is the other axis (area needs both to pick its rule)."""
    if mode == NEAREST:
        return _nearest_w(src, dst)
    if mode == LINEAR:
        return _linear_w(src, dst)
    if mode == CUBIC:
        return _taps_w(src, dst, _cubic_kernel, -1, 2, False)
    if mode == LANCZOS4:
        return _taps_w(src, dst, _lanczos_kernel, -3, 4, True)
    if mode == AREA:
        if src >= dst and other_src >= other_dst:
            return _box_w(src, dst)
        return _area_up_w(src, dst)
    raise ValueError("interpolation %r" % mode)


def resize(img, width, height, mode):
    """(h, w[, c]) -> (height, width[, c]) float64, the unrounded definition of cv::resize's `mode`."""
    a = np.asarray(img, np.float64)
    two_d = a.ndim == 2
    if two_d:
        a = a[..., None]
    h, w, _ = a.shape
    if (h, w) == (height, width):
        out = a.copy()
    else:
        if mode == LINEAR and h == 2 * height and w == 2 * width:
            mode = AREA
        wy = weights(mode, h, height, w, width)
        wx = weights(mode, w, width, h, height)
        out = np.einsum("yi,ijc,xj->yxc", wy, a, wx)
    return out[..., 0] if two_d else out


def error_stats(got, ref):
    """(max |got - clip(ref)|, bias, shift_x, shift_y) of a uint8 result against the float64 definition.

    The signed error is fitted as bias + shift_x * d(ref)/dx + shift_y * d(ref)/dy (gradients in destination pixels):
    a sampling grid displaced by delta destination pixels gives shift = delta, whatever the frame's mean gradient,
    while the fixed-point rounding of cv::resize's 8-bit paths lands in `bias`.  An axis of extent 1 has no shift term
    (its entry is 0)."""
    r = np.clip(np.asarray(ref, np.float64), 0, 255)
    if r.ndim == 2:
        r = r[..., None]
    e = np.asarray(got, np.float64).reshape(r.shape) - r
    cols, names = [np.ones(e.size)], []
    for ax, name in ((1, "x"), (0, "y")):
        if r.shape[ax] > 1:
            cols.append(np.gradient(r, axis=ax).ravel())
            names.append(name)
    coef = np.linalg.lstsq(np.stack(cols, 1), e.ravel(), rcond=None)[0]
    shift = dict(zip(names, coef[1:]))
    return float(np.abs(e).max()), float(coef[0]), float(shift.get("x", 0.0)), float(shift.get("y", 0.0))


def tolerances(mode, h, w, dh, dw):
    """(max |error|, max |bias|) that an 8-bit cv::resize result may show against `resize` on a textured frame.

    Every 8-bit mode lands within 1 LSB of the definition (clipped to [0, 255]).  The bias bound is 0.05 where the
    arithmetic ends in one correct rounding; cv::resize's fixed-point paths carry a systematic offset by construction:
      INTER_LINEAR, and INTER_AREA enlarging: the vertical pass ((b0*(S0>>4))>>16) + ((b1*(S1>>4))>>16) + 2) >> 2
        truncates twice (about -1/8), and at a vertical weight of exactly 1/2 it is (S0 + S1 + 1) >> 1 (+1/4);
      the exact 2 x 2 mean (S00 + S01 + S10 + S11 + 2) >> 2 rounds halves up (+1/8);
      INTER_LANCZOS4: each 11-bit tap is rounded on its own and the eight are not renormalised, so their sum drifts from
        2048 by a few units (about -1/4 at an exact 2x reduction, where every fraction is 1/2).
    Those get 0.3.  A displaced sampling grid does not hide in the bias: error_stats' shift terms catch it."""
    if (h, w) == (dh, dw) or mode == NEAREST:
        return 0.0, 0.0
    if mode == CUBIC:
        return 1.0, 0.05
    if mode == AREA and h >= dh and w >= dw:
        return 0.51, (0.3 if (h, w) == (2 * dh, 2 * dw) else 0.05)
    if mode == LINEAR and (h, w) == (2 * dh, 2 * dw):
        return 0.51, 0.3
    return 1.0, 0.3
