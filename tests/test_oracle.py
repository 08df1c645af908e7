"""CPU: the oracle against golden vectors and analytic known answers."""
import os

import numpy as np
import pytest

import oracle
from util import random_frames, smooth_texture, translated_rgb_pair

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "shot_golden.npz"))
CASES = sorted({k.rsplit("__", 1)[0] for k in GOLD.files})


# ---- A8: pinned by the reference itself (fixtures made by importing shot_detection.py) ----
@pytest.mark.parametrize("case", CASES)
def test_shot_oracle_matches_reference_golden(case):
    h = GOLD[case + "__hist"]
    assert oracle.shot_boundaries(h) == GOLD[case + "__bounds"].tolist()


# ---- A0/A1: pinned by definition -------------------------------------------------------------
@pytest.mark.parametrize("bins", [16, 256, 10])
def test_hist_oracle_matches_bincount(bins):
    f = random_frames(bins, 2, 53, 71)
    for fr in f:
        ref = np.stack([np.bincount(((fr[..., c].astype(np.int64) * bins) >> 8).ravel(), minlength=bins) for c in range(3)])
        np.testing.assert_array_equal(oracle.hist_u8c3(fr, bins), ref)


def test_hist_oracle_known_answers():
    z = np.zeros((40, 50, 3), np.uint8)
    h = oracle.hist_u8c3(z, 16)
    assert (h[:, 0] == 2000).all() and h[:, 1:].sum() == 0
    f = random_frames(1, 1, 64, 64)[0]
    h256, h16 = oracle.hist_u8c3(f, 256), oracle.hist_u8c3(f, 16)
    assert (h256.sum(axis=1) == 64 * 64).all()
    np.testing.assert_array_equal(h256.reshape(3, 16, 16).sum(axis=2), h16)   # 256 -> 16 fold


# ---- A2 -------------------------------------------------------------------------------------
def test_gray_oracle_known_answers():
    px = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0], [10, 200, 90]]], np.uint8)
    for bits, cb, cg, cr in ((15, 3735, 19235, 9798), (14, 1868, 9617, 4899)):
        assert cb + cg + cr == 1 << bits
        g = oracle.gray_u8(px, bits)[0]
        rnd = 1 << (bits - 1)
        assert g[0] == (255 * cb + rnd) >> bits == 29      # R byte gets the B weight (BGR2GRAY on RGB)
        assert g[1] == (255 * cg + rnd) >> bits
        assert g[2] == (255 * cr + rnd) >> bits
        assert g[3] == 255 and g[4] == 0
        assert g[5] == (10 * cb + 200 * cg + 90 * cr + rnd) >> bits


# ---- A3 driver geometry ------------------------------------------------------------------------
def test_level_geometry():
    assert oracle.fb_levels(1080, 1920) == 3
    assert [oracle.fb_level_geom(1080, 1920, k) for k in range(4)] == [
        (1080, 1920, 0.0, 3), (540, 960, 0.5, 3), (270, 480, 1.5, 9), (135, 240, 3.5, 19)]
    assert oracle.fb_levels(2160, 3840) == 3
    assert oracle.fb_levels(480, 640) == 3 and oracle.fb_level_geom(480, 640, 3)[:2] == (60, 80)
    assert oracle.fb_levels(48, 64) == 0          # 32-px rule crops every coarser level


def test_gaussian_kernels():
    np.testing.assert_array_equal(oracle.gaussian_kernel(3, 0.0), [0.25, 0.5, 0.25])
    for n, s in ((3, 0.5), (9, 1.5), (19, 3.5)):
        k = oracle.gaussian_kernel(n, s)
        assert abs(k.sum() - 1) < 1e-6 and np.allclose(k, k[::-1]) and k.argmax() == n // 2


def test_blur_preserves_constant_and_resize_modes():
    c = np.full((20, 30), 7.0, np.float32)
    np.testing.assert_allclose(oracle.gaussian_blur(c, 9, 1.5), 7.0, rtol=1e-6)
    a = np.arange(48, dtype=np.float32).reshape(6, 8)
    np.testing.assert_array_equal(oracle.resize_linear(a, 6, 8), a)                 # identity copy
    np.testing.assert_allclose(oracle.resize_linear(a, 3, 4), (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]) / 4)
    up = oracle.resize_linear(a, 12, 16)
    assert up.shape == (12, 16) and up[0, 0] == a[0, 0] and up[-1, -1] == a[-1, -1]


# ---- A4 -------------------------------------------------------------------------------------
def test_polyexp_recovers_quadratic_coefficients():
    h, w = 64, 80
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    a, bx, by, cxx, cyy, cxy = 3.0, 0.5, -0.25, 0.01, 0.02, -0.015
    I = a + bx * (x - 40) + by * (y - 30) + cxx * (x - 40) ** 2 + cyy * (y - 30) ** 2 + cxy * (x - 40) * (y - 30)
    R = oracle.polyexp(I.astype(np.float32))
    for yy, xx in ((30, 40), (20, 25), (45, 60)):
        exp = [by + 2 * cyy * (yy - 30) + cxy * (xx - 40), bx + 2 * cxx * (xx - 40) + cxy * (yy - 30), cyy, cxx, cxy]
        np.testing.assert_allclose(R[yy, xx], exp, atol=2e-6)


# ---- A5 quirk ---------------------------------------------------------------------------------
def test_update_matrices_last_row_col_quirk():
    f0, _ = translated_rgb_pair(9, 60, 70, 0, 0)
    R = oracle.polyexp(oracle.gray_u8(f0).astype(np.float32))
    M = oracle.update_matrices(R, R, np.zeros((60, 70, 2), np.float32))
    assert np.abs(M[:-1, :-1, 3:]).max() == 0
    assert np.abs(M[-1, :, 3:]).max() > 0 and np.abs(M[:, -1, 3:]).max() > 0


# ---- A3 end to end ----------------------------------------------------------------------------
def test_flow_oracle_recovers_translation():
    tx, ty = 3, -2
    t = smooth_texture(0, 280, 360)
    f0 = t[20:260, 20:340].astype(np.uint8)
    f1 = t[20 - ty:260 - ty, 20 - tx:340 - tx].astype(np.uint8)
    fl = oracle.farneback(f0, f1)
    inner = fl[40:-40, 40:-40]
    assert abs(np.median(inner[..., 0]) - tx) < 0.01 and abs(np.median(inner[..., 1]) - ty) < 0.01
    assert np.abs(inner - [tx, ty]).mean() < 0.01
    z = oracle.farneback(f0, f0)
    assert np.abs(z[:100, :150]).max() < 1e-3


def test_flow_oracle_direction_and_rgb_entry():
    f0, f1 = translated_rgb_pair(4, 120, 160, 2, 1)
    a = oracle.optical_flow_rgb(f0, f1)
    b = oracle.optical_flow_rgb(f1, f0)
    inner = slice(30, -30)
    assert np.median(a[inner, inner, 0]) > 1.5 and np.median(b[inner, inner, 0]) < -1.5
    np.testing.assert_array_equal(a, oracle.farneback(oracle.gray_u8(f0), oracle.gray_u8(f1)))


def test_oracle_under_address_and_ub_sanitizers():
    """The C restatement runs clean under ASan/UBSan on small and ragged shapes (1x1 ... 130x70)."""
    import subprocess
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")
    subprocess.check_call(["make", "-C", d, "asan_driver"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(d, "asan_driver")], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert out.returncode == 0, out.stderr[-2000:]
    assert "oracle sanitizer run ok" in out.stdout


# ---- flow consumers ----------------------------------------------------------------------------

def test_draw_flow_oracle_matches_reference_golden():
    """oracle.draw_flow vs outputs of the reference's vis.py (tests/golden/make_draw_flow_golden.py)."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "draw_flow_golden.npz"))
    names = sorted(k[:-4] for k in g.files if k.endswith("_out"))
    assert {"mixed", "zeros", "with_nan", "negative_max", "ragged_7x13"} <= set(names)
    for name in names:
        got = oracle.draw_flow(g[name + "_frame"], g[name + "_flow"])
        np.testing.assert_array_equal(got, g[name + "_out"], err_msg=name)


def test_flow_hist_oracle_known_answers():
    """cartToPolar/calcHist restatement: exact axis angles, cv::fastAtan2's documented 45-degree
    value, range edges."""
    fl = np.zeros((1, 8, 2), np.float32)
    fl[0, 0] = (1, 0); fl[0, 1] = (0, 1); fl[0, 2] = (-1, 0); fl[0, 3] = (0, -1)
    fl[0, 4] = (3, 4); fl[0, 5] = (1, 1); fl[0, 6] = (64, 0); fl[0, 7] = (0, 0)
    mag, deg = oracle.cart_to_polar_deg(fl)
    np.testing.assert_array_equal(mag[0], np.float32([1, 1, 1, 1, 5, np.sqrt(np.float32(2)), 64, 0]))
    np.testing.assert_array_equal(deg[0, :4], np.float32([0, 90, 180, 270]))
    assert abs(deg[0, 5] - 44.990456) < 1e-5            # cv::fastAtan2(1, 1)
    assert abs(deg[0, 4] - np.degrees(np.arctan2(4, 3))) < 0.3 and deg[0, 7] == 0
    h = oracle.flow_hist(fl)
    assert h.shape == (2, 64) and h.dtype == np.int32
    assert h[0].sum() == 7 and h[0, 1] == 5 and h[0, 5] == 1 and h[0, 0] == 1   # mag 64 dropped
    assert h[1].sum() == 8 and h[1, 0] == 3 and h[1, 16] == 1 and h[1, 32] == 1 and h[1, 48] == 1
    # histogram == bincount of floor() of the polar images
    rng = np.random.default_rng(0)
    f = (rng.standard_normal((40, 50, 2)) * 20).astype(np.float32)
    mag, deg = oracle.cart_to_polar_deg(f)
    hm = np.bincount(np.floor(mag[mag < 64].astype(np.float64)).astype(int), minlength=64)
    dd = deg.astype(np.float64) * (64 / 360.0)
    hd = np.bincount(np.floor(dd[dd < 64]).astype(int), minlength=64)
    np.testing.assert_array_equal(oracle.flow_hist(f), np.stack([hm, hd]))


def test_box_blur_oracle_matches_definition():
    """Blur op restatement vs a direct numpy evaluation of blur_kernel_cpu.cpp:62-79."""
    rng = np.random.default_rng(3)
    f = rng.integers(0, 256, (13, 17, 3), dtype=np.uint8)
    for k in (1, 2, 3, 4, 7):
        left, right = int(np.ceil(k / 2.0)) - 1, k // 2
        ref = np.zeros_like(f)
        for y in range(left, 13 - right):
            for x in range(left, 17 - right):
                win = f[y - left:y + right + 1, x - left:x + right + 1].astype(np.uint32).sum((0, 1))
                ref[y, x] = win // ((left + right + 1) ** 2)
        np.testing.assert_array_equal(oracle.box_blur(f, k), ref)


def test_resize_oracle_identities():
    """cv::resize restatement for 8-bit frames: constants are preserved by the fixed-point
    arithmetic, exact 2x decimation is the rounded 2x2 mean, nearest picks floor(x*scale), identity
    copies, target-size rules of the Resize kernel."""
    rng = np.random.default_rng(0)
    f = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)
    const = np.full((48, 64, 3), 137, np.uint8)
    for (w, h) in ((32, 24), (21, 13), (100, 77), (64, 48), (53, 30), (1, 1)):
        assert (oracle.resize_u8(const, w, h) == 137).all()
        assert oracle.resize_u8(f, w, h).shape == (h, w, 3)
    ref = ((f[0::2, 0::2].astype(int) + f[0::2, 1::2] + f[1::2, 0::2] + f[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    np.testing.assert_array_equal(oracle.resize_u8(f, 32, 24), ref)
    np.testing.assert_array_equal(oracle.resize_u8(f, 64, 48), f)
    near = oracle.resize_u8(f, 20, 10, oracle.INTER_NEAREST)
    np.testing.assert_array_equal(near, f[(np.arange(10) * 4.8).astype(int)][:, (np.arange(20) * 3.2).astype(int)])
    # a horizontal ramp stays monotone and inside the source range when up-scaled
    ramp = np.tile(np.arange(64, dtype=np.uint8)[None, :, None] * 4, (8, 1, 3))
    up = oracle.resize_u8(ramp, 256, 8)
    assert (np.diff(up[0, :, 0].astype(int)) >= 0).all() and up.min() == 0 and up.max() == 252
    assert oracle.resize_target(1920, 1080, width=426, height=240) == (426, 240)
    assert oracle.resize_target(1920, 1080, width=0, height=240, preserve_aspect=True) == (426, 240)
    assert oracle.resize_target(1920, 1080, width=426, height=0, preserve_aspect=True) == (426, 239)
    assert oracle.resize_target(320, 200, width=426, height=240, min=True) == (320, 200)
    # INTER_CUBIC / INTER_AREA: constants preserved, integer cells are the rounded float mean, the
    # 2x case equals the linear reroute, fractional cells keep the image mean
    for interp in (oracle.INTER_CUBIC, oracle.INTER_AREA):
        for (w, h) in ((32, 24), (16, 16), (21, 13), (100, 77), (90, 20), (13, 100)):
            assert (oracle.resize_u8(const, w, h, interp) == 137).all()
    f2 = rng.integers(0, 256, (48, 60, 3), dtype=np.uint8)
    blocks = f2.reshape(16, 3, 20, 3, 3).astype(np.float32).sum((1, 3)) * np.float32(1 / 9)
    np.testing.assert_array_equal(oracle.resize_u8(f2, 20, 16, oracle.INTER_AREA), np.rint(blocks).astype(np.uint8))
    np.testing.assert_array_equal(oracle.resize_u8(f2, 30, 24, oracle.INTER_AREA), oracle.resize_u8(f2, 30, 24))
    assert abs(oracle.resize_u8(f2, 21, 13, oracle.INTER_AREA).mean() - f2.mean()) < 0.3
    smooth = np.tile((np.arange(60, dtype=np.float32)[None, :, None] * 4), (48, 1, 3)).astype(np.uint8)
    cub = oracle.resize_u8(smooth, 120, 96, oracle.INTER_CUBIC).astype(int)
    lin = oracle.resize_u8(smooth, 120, 96).astype(int)
    assert np.abs(cub - lin)[:, 4:-4].max() <= 1                         # cubic reproduces a ramp
    # INTER_LANCZOS4: constants preserved, a ramp reproduced away from the edges, weights of an axis sum to 2048 +- rounding
    for (w, h) in ((32, 24), (21, 13), (100, 77), (90, 20)):
        assert (oracle.resize_u8(const, w, h, oracle.INTER_LANCZOS4) == 137).all()
    lz = oracle.resize_u8(smooth, 120, 96, oracle.INTER_LANCZOS4).astype(int)
    assert np.abs(lz - lin)[:, 8:-8].max() <= 1
    with pytest.raises(ValueError):
        oracle.resize_u8(f, 10, 10, 7)


def test_cvt_color_oracle_known_answers():
    """cv::cvtColor restatement: OpenCV's documented 8-bit values for primaries and grays, the
    HSV definition (against colorsys, within the table rounding), channel swaps."""
    import colorsys
    px = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0], [128, 128, 128],
                    [10, 200, 90], [255, 255, 0]]], np.uint8)                       # B, G, R order
    hsv = oracle.cvt_color(px, oracle.COLOR_BGR2HSV)[0]
    assert hsv[:6].tolist() == [[120, 255, 255], [60, 255, 255], [0, 255, 255], [0, 0, 255], [0, 0, 0], [0, 0, 128]]
    rng = np.random.default_rng(1)
    f = rng.integers(0, 256, (20, 30, 3), dtype=np.uint8)
    got = oracle.cvt_color(f, oracle.COLOR_BGR2HSV).reshape(-1, 3).astype(float)
    for (b, g, r), (hh, ss, vv) in zip(f.reshape(-1, 3)[:200], got[:200]):
        h, s, v = colorsys.rgb_to_hsv(r / 255., g / 255., b / 255.)
        assert vv == max(b, g, r) and abs(ss - s * 255) <= 1.01
        dh = abs(hh - h * 180)
        assert min(dh, 180 - dh) <= 1.01 or s * 255 < 8               # hue is ill-conditioned near gray
    assert oracle.cvt_color(px, oracle.COLOR_BGR2GRAY)[0, :6, 0].tolist() == [29, 150, 76, 255, 0, 128]
    assert oracle.cvt_color(px, oracle.COLOR_RGB2GRAY)[0, :6, 0].tolist() == [76, 150, 29, 255, 0, 128]
    np.testing.assert_array_equal(oracle.cvt_color(f, oracle.COLOR_BGR2RGB), f[..., ::-1])
    np.testing.assert_array_equal(oracle.cvt_color(f, oracle.COLOR_BGR2GRAY)[..., 0], oracle.gray_u8(f))
    with pytest.raises(ValueError):
        oracle.cvt_color(f, 44)   # COLOR_BGR2Lab: not restated


def test_hls_oracle_known_answers():
    """8-bit HLS: OpenCV's values for the primaries and grays (H in half degrees, L = (max + min) / 2, S = 255 for pure
    colours), the definition against colorsys within rounding, the four directions / hue ranges consistent with each
    other, and a round trip within the quantisation of the three bytes."""
    import colorsys
    px = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0], [128, 128, 128], [0, 255, 255]]], np.uint8)  # B, G, R
    hls = oracle.cvt_color(px, oracle.COLOR_BGR2HLS)[0]
    assert hls.tolist() == [[120, 128, 255], [60, 128, 255], [0, 128, 255], [0, 255, 0], [0, 0, 0], [0, 128, 0], [30, 128, 255]]
    full = oracle.cvt_color(px, oracle.COLOR_BGR2HLS_FULL)[0]
    assert full[:3].tolist() == [[171, 128, 255], [85, 128, 255], [0, 128, 255]]           # 240, 120, 0 degrees x 256 / 360
    rng = np.random.default_rng(7)
    f = rng.integers(0, 256, (20, 30, 3), dtype=np.uint8)
    got = oracle.cvt_color(f, oracle.COLOR_BGR2HLS).reshape(-1, 3).astype(float)
    for (b, g, r), (hh, ll, ss) in zip(f.reshape(-1, 3)[:300], got[:300]):
        h, l, s = colorsys.rgb_to_hls(r / 255., g / 255., b / 255.)
        assert abs(ll - l * 255) <= 0.51 and abs(ss - s * 255) <= 0.51
        dh = abs(hh - h * 180)
        assert min(dh, 180 - dh) <= 0.51 or s * 255 < 8 or max(b, g, r) - min(b, g, r) < 8
    np.testing.assert_array_equal(oracle.cvt_color(f, oracle.COLOR_RGB2HLS), oracle.cvt_color(np.ascontiguousarray(f[..., ::-1]), oracle.COLOR_BGR2HLS))
    np.testing.assert_array_equal(oracle.cvt_color(f, oracle.COLOR_HLS2RGB), oracle.cvt_color(f, oracle.COLOR_HLS2BGR)[..., ::-1])
    back = oracle.cvt_color(oracle.cvt_color(px, oracle.COLOR_BGR2HLS), oracle.COLOR_HLS2BGR)[0]
    assert np.abs(back.astype(int) - px[0].astype(int)).max() <= 1
    # hue bytes beyond the range wrap (h x 6 / 180 >= 6), s = 0 is the gray axis
    wrap = np.array([[[200, 128, 255], [20, 128, 255], [77, 90, 0]]], np.uint8)
    out = oracle.cvt_color(wrap, oracle.COLOR_HLS2BGR)[0]
    assert out[0].tolist() == out[1].tolist() and out[2].tolist() == [90, 90, 90]


def test_ycrcb_oracle_known_answers():
    """8-bit YCrCb: OpenCV's values for the primaries, the float definition within rounding, and a
    round trip within one grey level."""
    px = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0], [128, 128, 128]]], np.uint8)  # B, G, R
    y = oracle.cvt_color(px, oracle.COLOR_BGR2YCrCb)[0]
    assert y.tolist() == [[29, 107, 255], [150, 21, 43], [76, 255, 85], [255, 128, 128], [0, 128, 128], [128, 128, 128]]
    rng = np.random.default_rng(2)
    f = rng.integers(0, 256, (30, 40, 3), dtype=np.uint8)
    got = oracle.cvt_color(f, oracle.COLOR_RGB2YCrCb).astype(float)
    r, g, b = [f[..., i].astype(float) for i in range(3)]
    Y = 0.299 * r + 0.587 * g + 0.114 * b
    assert np.abs(got[..., 0] - Y).max() <= 0.51
    assert np.abs(got[..., 1] - np.clip((r - Y) * 0.713 + 128, 0, 255)).max() <= 1.01
    assert np.abs(got[..., 2] - np.clip((b - Y) * 0.564 + 128, 0, 255)).max() <= 1.01
    rt = oracle.cvt_color(oracle.cvt_color(f, oracle.COLOR_RGB2YCrCb), oracle.COLOR_YCrCb2RGB)
    interior = (got[..., 1] > 0) & (got[..., 1] < 255) & (got[..., 2] > 0) & (got[..., 2] < 255)
    assert np.abs(rt.astype(int) - f)[interior].max() <= 2


def test_hsv_inverse_and_yuv_oracle_known_answers():
    """HSV -> RGB (float path): primaries, the colorsys definition within rounding, forward/backward
    round trip within the hue quantisation; RGB2HSV is BGR2HSV on swapped bytes; the _FULL variants
    use hue ranges 256 / 255; 8-bit YUV: the float definition within rounding and a round trip."""
    import colorsys
    hsv = np.array([[[120, 255, 255], [60, 255, 255], [0, 255, 255], [0, 0, 255], [0, 0, 0], [90, 128, 200]]], np.uint8)
    bgr = oracle.cvt_color(hsv, oracle.COLOR_HSV2BGR)[0]
    assert bgr[:5].tolist() == [[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0]]
    np.testing.assert_array_equal(oracle.cvt_color(hsv, oracle.COLOR_HSV2RGB), oracle.cvt_color(hsv, oracle.COLOR_HSV2BGR)[..., ::-1])
    rng = np.random.default_rng(3)
    f = rng.integers(0, 256, (24, 32, 3), dtype=np.uint8)
    f[..., 0] %= 180
    rgb = oracle.cvt_color(f, oracle.COLOR_HSV2RGB).astype(float)
    for (h, s, v), px in zip(f.reshape(-1, 3)[:300], rgb.reshape(-1, 3)[:300]):
        ref = np.array(colorsys.hsv_to_rgb(h / 180., s / 255., v / 255.)) * 255
        assert np.abs(px - ref).max() <= 0.51, (h, s, v, px, ref)
    g = rng.integers(0, 256, (24, 32, 3), dtype=np.uint8)
    np.testing.assert_array_equal(oracle.cvt_color(g, oracle.COLOR_RGB2HSV), oracle.cvt_color(g[..., ::-1].copy(), oracle.COLOR_BGR2HSV))
    back = oracle.cvt_color(oracle.cvt_color(g, oracle.COLOR_BGR2HSV), oracle.COLOR_HSV2BGR).astype(int)
    assert np.abs(back - g).max() <= 6                      # hue is quantised to 2 degrees
    full = oracle.cvt_color(g, oracle.COLOR_BGR2HSV_FULL).astype(int)
    base = oracle.cvt_color(g, oracle.COLOR_BGR2HSV).astype(int)
    np.testing.assert_array_equal(full[..., 1:], base[..., 1:])
    dh = np.abs(full[..., 0] - base[..., 0] * 256 / 180)
    assert np.minimum(dh, 256 - dh).max() <= 1.5           # the hue circle wraps
    backf = oracle.cvt_color(oracle.cvt_color(g, oracle.COLOR_RGB2HSV_FULL), oracle.COLOR_HSV2RGB_FULL).astype(int)
    assert np.abs(backf - g).max() <= 10                   # forward range 256, backward 255 (as in cvtColor) + quantisation
    # YUV
    px = np.array([[[255, 255, 255], [0, 0, 0], [128, 128, 128]]], np.uint8)
    assert oracle.cvt_color(px, oracle.COLOR_BGR2YUV)[0].tolist() == [[255, 128, 128], [0, 128, 128], [128, 128, 128]]
    yuv = oracle.cvt_color(g, oracle.COLOR_RGB2YUV).astype(float)
    r, gg, b = [g[..., i].astype(float) for i in range(3)]
    Y = 0.299 * r + 0.587 * gg + 0.114 * b
    assert np.abs(yuv[..., 0] - Y).max() <= 0.51
    assert np.abs(yuv[..., 1] - np.clip((b - Y) * 0.492 + 128, 0, 255)).max() <= 1.01
    assert np.abs(yuv[..., 2] - np.clip((r - Y) * 0.877 + 128, 0, 255)).max() <= 1.01
    np.testing.assert_array_equal(oracle.cvt_color(g, oracle.COLOR_BGR2YUV), oracle.cvt_color(g[..., ::-1].copy(), oracle.COLOR_RGB2YUV))
    rt = oracle.cvt_color(oracle.cvt_color(g, oracle.COLOR_RGB2YUV), oracle.COLOR_YUV2RGB).astype(int)
    ok = (yuv[..., 1] > 0) & (yuv[..., 1] < 255) & (yuv[..., 2] > 0) & (yuv[..., 2] < 255)
    assert np.abs(rt - g)[ok].max() <= 3


def test_resize_oracle_against_torch_conventions():
    """Independent cross-check of the sampling conventions (not a bit pin): torch's float
    interpolate uses the same half-pixel centres (bilinear / bicubic with A = -0.75), the same
    floor(x*scale) nearest rule and the same cell averaging ('area') as the OpenCV algorithms
    restated in the oracle, so the 8-bit results must agree within the fixed-point rounding."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, (12, 16, 3)).astype(np.float32)
    img = np.clip(np.kron(base, np.ones((8, 8, 1), np.float32)) + rng.normal(0, 3, (96, 128, 3)), 0, 255).astype(np.uint8)
    t = torch.from_numpy(img).permute(2, 0, 1)[None].float()

    def tor(mode, size, **kw):
        return F.interpolate(t, size=size, mode=mode, **kw)[0].permute(1, 2, 0).numpy()

    for (dh, dw) in ((48, 64), (37, 51), (150, 170), (96, 200)):
        lin = oracle.resize_u8(img, dw, dh).astype(np.float32)
        if not (dh * 2 == 96 and dw * 2 == 128):
            assert np.abs(lin - tor("bilinear", (dh, dw), align_corners=False)).max() <= 1.0
        near = oracle.resize_u8(img, dw, dh, oracle.INTER_NEAREST)
        np.testing.assert_array_equal(near, tor("nearest", (dh, dw)).astype(np.uint8))
        cub = oracle.resize_u8(img, dw, dh, oracle.INTER_CUBIC).astype(np.float32)
        ref = np.clip(tor("bicubic", (dh, dw), align_corners=False), 0, 255)
        assert np.abs(cub - ref)[2:-2, 2:-2].max() <= 1.5            # borders: replicate vs torch's clamp of the index
    from ref_resize_np import box_average
    for (dh, dw) in ((48, 64), (32, 32), (24, 16), (37, 51), (95, 127), (13, 100 // 3)):
        area = oracle.resize_u8(img, dw, dh, oracle.INTER_AREA).astype(np.float64)
        assert np.abs(area - box_average(img, dh, dw)).max() <= 0.51
    for (dh, dw) in ((48, 64), (32, 32), (24, 16)):                   # integer cells: torch's 'area' is the same mean
        area = oracle.resize_u8(img, dw, dh, oracle.INTER_AREA).astype(np.float32)
        assert np.abs(area - tor("area", (dh, dw))).max() <= 0.51


def test_farneback_oracle_against_independent_float64_derivation():
    """The C restatement of cv::FarnebackOpticalFlow vs an independent float64 implementation of
    the published algorithm built from scipy/torch primitives (tests/ref_farneback_np.py): every
    stage and the end-to-end flow agree to float32 rounding.  Not a pin against OpenCV output, but
    it rules out indexing / border / ordering errors in the restatement."""
    import ref_farneback_np as ref
    h, w = 264, 328                                              # 3 pyramid levels + full resolution
    f0, f1 = translated_rgb_pair(21, h, w, 3, -2)
    g0, g1 = oracle.gray_u8(f0), oracle.gray_u8(f1)
    assert ref.levels_for(h, w) == oracle.fb_levels(h, w) == 3
    for k in range(4):
        a, b = oracle.fb_pyr_image(g0, k), ref.pyramid_image(g0, k)
        assert a.shape == b.shape and np.abs(a - b).max() <= 2e-4, k
    I = oracle.fb_pyr_image(g0, 1)
    R_o, R_r = oracle.polyexp(I), ref.poly_expansion(I.astype(np.float64))
    assert np.abs(R_o - R_r).max() <= 2e-4 * max(1.0, np.abs(R_r).max())
    I1 = oracle.fb_pyr_image(g1, 1)
    R1_o = oracle.polyexp(I1)
    fl = (np.random.default_rng(3).standard_normal(I.shape + (2,)) * 2).astype(np.float32)
    M_o = oracle.update_matrices(R_o, R1_o, fl)
    M_r = ref.update_matrices(R_o.astype(np.float64), R1_o.astype(np.float64), fl.astype(np.float64))
    assert np.abs(M_o - M_r).max() <= 1e-4 * max(1.0, np.abs(M_r).max())
    flow_o, _ = oracle.update_flow_blur(R_o, R1_o, M_o, 15, False)
    flow_r = ref.box_solve(M_o.astype(np.float64), 15)
    assert np.abs(flow_o - flow_r).max() <= 1e-4
    got, want = oracle.farneback(g0, g1), ref.farneback(g0, g1)
    assert np.linalg.norm(got - want) <= 2e-4 * np.linalg.norm(want)
    assert np.abs(got - want).max() <= 2e-3
    inner = got[40:-40, 40:-40]
    assert abs(np.median(inner[..., 0]) - 3) < 0.05 and abs(np.median(inner[..., 1]) + 2) < 0.05


def test_cvt_color_xyz_and_layout_family_known_answers():
    """XYZ: the float definition (sRGB primaries, D65) within the 12-bit rounding, white -> (242, 255, saturated 255),
    the inverse within rounding where nothing saturated; layout family: packing keeps the top 5 / 6 / 5 bits, the 555
    alpha bit, gray of a packed pixel with the 14-bit table, alpha added = 255."""
    rng = np.random.default_rng(3)
    f = rng.integers(0, 256, (40, 50, 3), dtype=np.uint8)
    M = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
    want = np.clip(f[..., ::-1].astype(float) @ M.T, 0, 255)          # f is BGR: reverse to R, G, B
    got = oracle.cvt_color(f, oracle.COLOR_BGR2XYZ).astype(float)
    assert np.abs(got - want).max() <= 0.6
    np.testing.assert_array_equal(oracle.cvt_color(f[..., ::-1].copy(), oracle.COLOR_RGB2XYZ), oracle.cvt_color(f, oracle.COLOR_BGR2XYZ))
    white = np.full((1, 1, 3), 255, np.uint8)
    assert oracle.cvt_color(white, oracle.COLOR_BGR2XYZ)[0, 0].tolist() == [242, 255, 255]
    dim = (f // 2 + 20).astype(np.uint8)                              # nothing saturates
    back = oracle.cvt_color(oracle.cvt_color(dim, oracle.COLOR_BGR2XYZ), oracle.COLOR_XYZ2BGR).astype(int)
    assert np.abs(back - dim).max() <= 3
    p565 = oracle.cvt_color(f, 12)
    t = p565[..., 0].astype(int) | (p565[..., 1].astype(int) << 8)
    np.testing.assert_array_equal(t, (f[..., 0] >> 3).astype(int) | ((f[..., 1] >> 2).astype(int) << 5) | ((f[..., 2] >> 3).astype(int) << 11))
    f4 = np.concatenate([f, rng.integers(0, 2, f.shape[:2] + (1,), dtype=np.uint8) * 200], axis=2)
    p555 = oracle.cvt_color(f4, 26)
    t = p555[..., 0].astype(int) | (p555[..., 1].astype(int) << 8)
    np.testing.assert_array_equal(t >> 15, (f4[..., 3] != 0).astype(int))
    np.testing.assert_array_equal(oracle.cvt_color(p555, 28)[..., 3], np.where(f4[..., 3] != 0, 255, 0))
    np.testing.assert_array_equal(oracle.cvt_color(p565, 21), oracle.cvt_color(oracle.cvt_color(p565, 14), oracle.COLOR_BGR2GRAY, gray_bits=14))
    assert oracle.cvt_color(f, 0)[..., 3].min() == 255 and np.array_equal(oracle.cvt_color(f, 2)[..., :3], f[..., ::-1])
    g = f[..., :1].copy()
    np.testing.assert_array_equal(oracle.cvt_color(g, 30), oracle.cvt_color(np.repeat(g, 3, axis=2), 22))


def test_oracle_against_opencv_golden():
    """Every tests/golden/opencv_<version>.npz present (written by tests/golden/make_opencv_golden.py on a machine with
    OpenCV) pins the oracle against REAL OpenCV output: bit-exact for the integer routines, the stated tolerances for the
    float ones.  None is committed yet -- no OpenCV in the authoring container or on the GPU pool -- so this skips, and the
    OpenCV-backed rows of DESIGN.md section 2 stay "parity unpinned" until one run elsewhere adds the file."""
    import glob
    import os
    files = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "opencv_*.npz")))
    if not files:
        pytest.skip("no tests/golden/opencv_*.npz: run tests/golden/make_opencv_golden.py where cv2 is importable")
    for path in files:
        _check_opencv_golden(path)


def _check_opencv_golden(path):
    if True:
        z = np.load(path)
        f = z["hist_in"]
        for bins in (16, 256):
            np.testing.assert_array_equal(oracle.hist_u8c3(f, bins), z["hist_%d" % bins])
        px = np.array([[[1, 2, 255]]], np.uint8)
        bits = next(b for b in (15, 14) if (oracle.cvt_color(f, oracle.COLOR_BGR2GRAY, gray_bits=b)[..., 0] == z["gray_bgr2gray"]).all())
        np.testing.assert_array_equal(oracle.cvt_color(f, oracle.COLOR_RGB2GRAY, bits)[..., 0], z["gray_rgb2gray"])
        for key in z.files:
            if key.startswith("cvt_"):
                np.testing.assert_array_equal(oracle.cvt_color(f, getattr(oracle, key[4:])), z[key], err_msg=key)
            if key.startswith("resize_") and key != "resize_in":
                size, mode = key[7:].split("_", 1)
                dw, dh = (int(v) for v in size.split("x"))
                np.testing.assert_array_equal(oracle.resize_u8(z["resize_in"], dw, dh, getattr(oracle, mode)), z[key], err_msg=key)
        omag, odeg = oracle.cart_to_polar_deg(z["polar_in"])
        assert np.abs(omag - z["polar_mag"]).max() <= 1e-5 and np.abs(odeg - z["polar_deg"]).max() <= 1e-3
        got = oracle.flow_hist(z["polar_in"])
        assert np.abs(got[0] - z["flowhist_mag"]).sum() <= 4 and np.abs(got[1] - z["flowhist_deg"]).sum() <= 4
        for key in [k[3:-5] for k in z.files if k.startswith("fb_") and k.endswith("_flow")]:
            f0, f1, ref = z["fb_%s_f0" % key], z["fb_%s_f1" % key], z["fb_%s_flow" % key]
            got = oracle.optical_flow_rgb(f0, f1, oracle.default_params(gray_bits=bits))
            rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
            assert rel <= 1e-3 and np.abs(got - ref).max() <= 1e-2, (path, key, rel, float(np.abs(got - ref).max()))
            g0 = oracle.cvt_color(f0, oracle.COLOR_BGR2GRAY, bits)[..., 0].astype(np.float32)
            assert np.abs(oracle.gaussian_blur(g0, 9, 1.5) - z["fb_%s_blur9" % key]).max() <= 1e-3


def test_opencv_golden_checker_reads_the_dump_format(tmp_path):
    """The checker above against a file in the dump script's format whose "OpenCV" arrays come from the oracle itself: proves
    that every key the dump writes is found and compared (so that the first real file cannot silently be skipped over)."""
    from util import texture_stream
    f = random_frames(0, 1, 97, 131)[0]
    out = {"cv2_version": np.array("self"), "hist_in": f}
    for bins in (16, 256):
        out["hist_%d" % bins] = oracle.hist_u8c3(f, bins)
    out["gray_bgr2gray"] = oracle.cvt_color(f, oracle.COLOR_BGR2GRAY, 15)[..., 0]
    out["gray_rgb2gray"] = oracle.cvt_color(f, oracle.COLOR_RGB2GRAY, 15)[..., 0]
    for name in ("COLOR_BGR2HSV", "COLOR_YCrCb2BGR", "COLOR_BGR2XYZ", "COLOR_HSV2BGR_FULL"):
        out["cvt_" + name] = oracle.cvt_color(f, getattr(oracle, name))
    rs = random_frames(1, 1, 97, 131)[0]
    out["resize_in"] = rs
    for mname in ("INTER_NEAREST", "INTER_LINEAR", "INTER_CUBIC", "INTER_AREA", "INTER_LANCZOS4"):
        out["resize_65x48_%s" % mname] = oracle.resize_u8(rs, 65, 48, getattr(oracle, mname))
    fl = (np.random.default_rng(2).standard_normal((60, 80, 2)) * 9).astype(np.float32)
    out["polar_in"] = fl
    out["polar_mag"], out["polar_deg"] = oracle.cart_to_polar_deg(fl)
    h = oracle.flow_hist(fl)
    out["flowhist_mag"], out["flowhist_deg"] = h[0], h[1]
    f0, f1 = translated_rgb_pair(3, 97, 131, 1, -1)
    out["fb_97x131_f0"], out["fb_97x131_f1"] = f0, f1
    out["fb_97x131_flow"] = oracle.optical_flow_rgb(f0, f1)
    out["fb_97x131_blur9"] = oracle.gaussian_blur(oracle.cvt_color(f0, oracle.COLOR_BGR2GRAY, 15)[..., 0].astype(np.float32), 9, 1.5)
    path = tmp_path / "opencv_self.npz"
    np.savez_compressed(path, **out)
    _check_opencv_golden(str(path))
    out["fb_97x131_flow"] = out["fb_97x131_flow"] + np.float32(0.05)     # and it does compare: a shifted field fails
    np.savez_compressed(path, **out)
    with pytest.raises(AssertionError):
        _check_opencv_golden(str(path))
