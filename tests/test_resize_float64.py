"""The C oracle's cv::resize restatement (oracle.resize_u8) against the float64 definitions in tests/ref_resize_np.py,
which share no code with it: every mode, 1 to 4 channels, shrinking, enlarging, mixed per axis, 1 x N and N x 1
targets and ratios beyond 6 (where INTER_AREA leaves the vector kernels).  The tolerances pinned here are the ones
tests/test_resize_dispatch_gpu.py applies to the kernels' own output."""
import numpy as np
import pytest

import oracle
import ref_resize_np as ref
from util import smooth_texture

MODES = {"nearest": ref.NEAREST, "linear": ref.LINEAR, "cubic": ref.CUBIC, "area": ref.AREA, "lanczos4": ref.LANCZOS4}

# (h, w) -> (dh, dw)
SHAPES = [
    ((61, 83), (30, 41)),      # fractional down, both axes
    ((61, 83), (123, 167)),    # fractional up, both axes
    ((61, 83), (40, 200)),     # mixed: down in y, up in x
    ((47, 59), (94, 20)),      # mixed: up in y, down in x
    ((64, 96), (32, 48)),      # exact 2 x 2
    ((60, 90), (20, 30)),      # integer 3 x 3
    ((60, 90), (30, 18)),      # integer 5 on x, 2 on y
    ((61, 83), (1, 37)),       # 1 x N target
    ((61, 83), (29, 1)),       # N x 1 target
    ((200, 257), (29, 37)),    # ratio ~7 on both axes
    ((133, 171), (19, 17)),    # ratio 7 and ~10
    ((61, 83), (61, 83)),      # copy
]


def textured(seed, h, w, c):
    """Smooth texture (sigma 2.5 px, full 0..255 range): enough gradient everywhere for the shift terms."""
    return np.stack([smooth_texture(seed * 7 + k, h, w, 2.5) for k in range(c)], -1).astype(np.uint8)


def test_reference_weights_are_partitions_of_unity():
    for mode in MODES.values():
        for src, dst, osrc, odst in ((83, 41, 61, 30), (83, 167, 61, 123), (83, 1, 61, 29), (257, 37, 200, 29), (40, 200, 61, 83)):
            m = ref.weights(mode, src, dst, osrc, odst)
            assert m.shape == (dst, src)
            np.testing.assert_allclose(m.sum(1), 1.0, atol=1e-12)


def test_reference_matches_torch_where_conventions_coincide():
    """Away from the borders (where replicate and torch's clamp of the sample position differ) the definitions are
    torch's float bilinear / bicubic (A = -0.75, half-pixel centres), nearest and integer-cell area."""
    import torch
    import torch.nn.functional as F
    f = textured(3, 61, 83, 3).astype(np.float64)
    t = torch.from_numpy(f).permute(2, 0, 1)[None]

    def tor(mode, size, **kw):
        return F.interpolate(t, size=size, mode=mode, **kw)[0].permute(1, 2, 0).numpy()

    for dh, dw in ((30, 41), (123, 167), (40, 200)):
        np.testing.assert_allclose(ref.resize(f, dw, dh, ref.LINEAR), tor("bilinear", (dh, dw), align_corners=False), atol=1e-9)
        np.testing.assert_allclose(ref.resize(f, dw, dh, ref.CUBIC)[3:-3, 3:-3], tor("bicubic", (dh, dw), align_corners=False)[3:-3, 3:-3],
                                   atol=1e-9)
        np.testing.assert_array_equal(ref.resize(f, dw, dh, ref.NEAREST), tor("nearest", (dh, dw)))
    g = textured(4, 60, 90, 2).astype(np.float64)
    tg = torch.from_numpy(g).permute(2, 0, 1)[None]
    np.testing.assert_allclose(ref.resize(g, 30, 20, ref.AREA), F.interpolate(tg, size=(20, 30), mode="area")[0].permute(1, 2, 0).numpy(),
                               atol=1e-9)


def test_reference_lanczos4_is_a_normalised_windowed_sinc():
    """At a whole-pixel position Lanczos4 is the source pixel itself; a constant stays constant; an integer
    enlargement of a linear ramp is interpolated exactly away from the borders (the normalised window reproduces
    linear functions up to its truncation: 0.045 grey levels on a ramp of 3 per pixel)."""
    m = ref.weights(ref.LANCZOS4, 50, 25)
    assert m.shape == (25, 50)
    ramp = np.tile(np.arange(40, dtype=np.float64) * 3, (8, 1))
    up = ref.resize(ramp, 80, 8, ref.LANCZOS4)
    x = (np.arange(80) + 0.5) * 0.5 - 0.5
    np.testing.assert_allclose(up[:, 8:-8], np.tile(3 * x, (8, 1))[:, 8:-8], atol=0.05)
    const = np.full((13, 17, 2), 99.0)
    np.testing.assert_allclose(ref.resize(const, 29, 7, ref.LANCZOS4), 99.0, atol=1e-12)


def test_shift_terms_catch_a_half_pixel_shift():
    """The statistic the bias checks rely on: corner-aligned sampling (x = dx * scale, no half-pixel centres) in place of
    the definition, rounded to uint8, shows a shift of a quarter destination pixel or more at a 2x reduction, while the
    correctly centred result shows none."""
    f = textured(9, 64, 96, 3)
    good = np.rint(np.clip(ref.resize(f, 41, 30, ref.LINEAR), 0, 255))
    wy = np.zeros((30, 64)); wx = np.zeros((41, 96))
    for m, src, dst in ((wy, 64, 30), (wx, 96, 41)):
        for d in range(dst):
            x = d * src / dst
            i = int(x); fr = x - i
            m[d, i] += 1 - fr
            m[d, min(i + 1, src - 1)] += fr
    shifted = np.rint(np.clip(np.einsum("yi,ijc,xj->yxc", wy, f.astype(np.float64), wx), 0, 255))
    r = ref.resize(f, 41, 30, ref.LINEAR)
    _, _, sx, sy = ref.error_stats(good, r)
    assert abs(sx) < 0.01 and abs(sy) < 0.01
    _, _, sx, sy = ref.error_stats(shifted, r)
    assert abs(sx) > 0.2 and abs(sy) > 0.2, (sx, sy)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("cn", [1, 2, 3, 4])
def test_oracle_resize_against_float64_definition(mode, cn):
    m = MODES[mode]
    for k, ((h, w), (dh, dw)) in enumerate(SHAPES):
        f = textured(11 * k + cn, h, w, cn)
        got = oracle.resize_u8(f, dw, dh, m)
        r = ref.resize(f, dw, dh, m)
        emax, bias, sx, sy = ref.error_stats(got, r)
        tol, btol = ref.tolerances(m, h, w, dh, dw)
        what = "%s %dx%dx%d -> %dx%d" % (mode, w, h, cn, dw, dh)
        assert emax <= tol, "%s: max error %.3f > %.2f" % (what, emax, tol)
        if got.size >= 400:                      # a mean over fewer values is noise at this scale
            assert abs(bias) <= btol, "%s: bias %.3f > %.2f" % (what, bias, btol)
            assert abs(sx) <= 0.05 and abs(sy) <= 0.05, "%s: sampling grid displaced by (%.3f, %.3f) px" % (what, sx, sy)
