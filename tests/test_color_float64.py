"""The C oracle's cv::cvtColor restatement (oracle.cvt_color) against the float64 definitions in tests/ref_color_np.py,
which share no code or fixed-point tables with it: every code ConvertColor accepts, over the whole input domain of its
source (the 2^24 byte cube, the cube with alpha, all 65 536 packed pixels, all 256 grays, every (Y, U, V) triple laid out
in each 4:2:0 / 4:2:2 layout), plus random 4:2:0 / 4:2:2 frames whose chroma changes from block to block.  Two bounds per
output channel (ref_color_np.bounds, each derived there): a max |error| and a mean signed error, the second being what
catches a truncation where OpenCV rounds.  The same bounds are applied to the kernels' own output by
tests/test_cvt_color_dispatch_gpu.py."""
import functools

import numpy as np
import pytest

import oracle
import ref_color_np as ref

PIXEL_CODES = [c for c in ref.ALL_CODES if c not in ref.YUV_SOURCES]
YUV_CODES = sorted(ref.YUV_SOURCES)


@functools.lru_cache(maxsize=None)
def domain(scn):
    return ref.pixel_domain(scn)


@functools.lru_cache(maxsize=2)
def yuv_domain(layout):
    return ref.yuv_full_domain(layout)


def test_code_table_is_the_librarys():
    """The definitions cover exactly the codes the library accepts (91 codes under 139 names), with the oracle's shapes."""
    from scannertools_amd._native import COLOR_CODES
    assert len(COLOR_CODES) == 139 and set(COLOR_CODES.values()) == set(ref.ALL_CODES) and len(ref.ALL_CODES) == 91
    for code in PIXEL_CODES:
        scn, dcn = ref.channels(code)
        assert oracle.cvt_color(np.zeros((2, 4, scn), np.uint8), code).shape == (2, 4, dcn), code
    for code in YUV_CODES:
        layout, _, dcn = ref.YUV_SOURCES[code]
        src = np.zeros((6, 4, 1) if layout in ref.LAYOUTS_420 else (4, 4, 2), np.uint8)
        assert oracle.cvt_color(src, code).shape == (4, 4, dcn), code


def test_definitions_known_answers_and_inverses():
    """The definitions themselves: primaries and grays, and each inverse undoing its forward formula in float64."""
    b, g, r = np.array([255.0, 0, 0, 255, 0, 128]), np.array([0.0, 255, 0, 255, 0, 128]), np.array([0.0, 0, 255, 255, 0, 128])
    np.testing.assert_allclose(ref.luma(b, g, r), [29.07, 149.685, 76.245, 255, 0, 128])
    h, s, v = ref.bgr2hsv(b, g, r, 180)
    np.testing.assert_allclose(np.stack([h, s, v], 1), [[120, 255, 255], [60, 255, 255], [0, 255, 255], [0, 0, 255], [0, 0, 0], [0, 0, 128]])
    h, l, s2 = ref.bgr2hls(b, g, r, 180)
    np.testing.assert_allclose(np.stack([h, l, s2], 1), [[120, 127.5, 255], [60, 127.5, 255], [0, 127.5, 255], [0, 255, 0], [0, 0, 0], [0, 128, 0]])
    np.testing.assert_allclose(ref.hexcone_hue(b, g, r, 256)[:3], [170 + 2 / 3, 85 + 1 / 3, 0])
    rng = np.random.default_rng(1)
    b, g, r = (rng.uniform(0, 255, 5000) for _ in range(3))
    for hr, hri in ((180, 180), (256, 255)):
        h, s, v = ref.bgr2hsv(b, g, r, hr)
        np.testing.assert_allclose(ref.hsv2bgr(h * hri / hr, s, v, hri), (b, g, r), atol=1e-9)
        h, l, s = ref.bgr2hls(b, g, r, hr)
        np.testing.assert_allclose(ref.hls2bgr(h * hri / hr, l, s, hri), (b, g, r), atol=1e-9)
        # hue bytes past the range wrap
        np.testing.assert_allclose(ref.hsv2bgr(h + hri, s, v, hri), ref.hsv2bgr(h, s, v, hri), atol=1e-9)
    np.testing.assert_allclose(ref.ycrcb2bgr(*ref.bgr2ycrcb(b, g, r)), (b, g, r), atol=0.1)     # 3-decimal published gains
    np.testing.assert_allclose(ref.yuv2bgr(*ref.bgr2yuv(b, g, r)), (b, g, r), atol=0.1)
    np.testing.assert_allclose(ref.xyz2rgb(*ref.rgb2xyz(r, g, b)), (r, g, b), atol=1e-9)
    # BT.601 limited range: black at 16, white at 235, the 75 % bars
    np.testing.assert_allclose(np.stack(ref.bt601_limited(np.array([16.0, 235, 0]), np.full(3, 128.0), np.full(3, 128.0)), 1),
                               [[0, 0, 0], [254.916] * 3, [0, 0, 0]])
    # packing round trip keeps the top bits; 555 alpha
    q = rng.integers(0, 256, (3, 1000))
    for gb, mask_g in ((6, 0xFC), (5, 0xF8)):
        bb, gg, rr, _ = ref.unpack5x5(*ref.pack5x5(q[0], q[1], q[2], gb), gb)
        np.testing.assert_array_equal(np.stack([bb, gg, rr]), q & np.array([[0xF8], [mask_g], [0xF8]]))
    assert ref.unpack5x5(*ref.pack5x5(8, 8, 8, 5, alpha=np.array(1)), 5)[3] == 255


def test_yuv_layouts_round_trip_and_full_domain_is_complete():
    rng = np.random.default_rng(2)
    for layout in ref.LAYOUTS_420 + ref.LAYOUTS_422:
        y, u, v = ref.yuv_block_planes(rng, 38, 52, layout)
        f = ref.encode_yuv(y, u, v, layout)
        assert f.shape == ((57, 52, 1) if layout in ref.LAYOUTS_420 else (38, 52, 2))
        for a, b in zip(ref.decode_yuv(f, layout), (y, u, v)):
            np.testing.assert_array_equal(a, b)
    for layout in ("I420", "YUY2"):
        yy, uu, vv = ref.decode_yuv(yuv_domain(layout), layout)
        t = (yy.astype(np.int64) << 16) | (uu.astype(np.int64) << 8) | vv
        assert np.unique(t).size == 1 << 24


@pytest.mark.parametrize("code", PIXEL_CODES)
def test_oracle_against_definition_whole_domain(code):
    """Every pixel code over every value its source pixel can take; the codes that use the op's gray table at both widths."""
    scn, _ = ref.channels(code)
    src = domain(scn)
    for bits in ((14, 15) if code in ref.GRAY_TABLE_CODES else (15,)):
        got = oracle.cvt_color(src, code, gray_bits=bits)
        ref.check_pixels(code, src, got, "oracle code %d gray_bits %d" % (code, bits), gray_bits=bits)


@pytest.mark.parametrize("code", YUV_CODES)
def test_oracle_yuv_sources_against_definition(code):
    """Each 4:2:0 / 4:2:2 code on the frame that holds every (Y, U, V) triple of its layout, and on random frames whose
    chroma changes from block to block at heights H % 4 == 2 (an odd number of chroma rows: the planar V plane starts in
    the middle of a row pair) -- a wrong chroma sample, plane or byte order is an error of many levels here."""
    layout = ref.yuv_layout_of(code)
    f = yuv_domain(layout)
    ref.check_yuv(code, f, oracle.cvt_color(f, code), "oracle code %d (%s) whole domain" % (code, layout))
    rng = np.random.default_rng(code)
    for h, w in ((38, 52), (6, 2), (70, 98)):
        f = ref.encode_yuv(*ref.yuv_block_planes(rng, h, w, layout), layout)
        ref.check_yuv(code, f, oracle.cvt_color(f, code), "oracle code %d (%s) %dx%d" % (code, layout, w, h), bias=False)


@pytest.mark.parametrize("bits", [14, 15])
def test_flow_gray_against_definition(bits):
    """The flow path's gray (oracle.gray_u8, which st_gray_u8 must equal): OpenCV's BGR table on RGB bytes, whole cube."""
    cube = domain(3)
    got = oracle.gray_u8(cube, bits)
    st = ref.Stats([("v",)])
    for i in range(0, got.size, ref.CHUNK):
        st.add(got.reshape(-1)[i:i + ref.CHUNK], ref.flow_gray(cube.reshape(-1, 3)[i:i + ref.CHUNK])[:, None])
    st.check([("v", ref.gray_bound(bits), ref.BIAS)], "flow gray %d-bit" % bits)


def test_inputs_tell_the_layouts_apart():
    """The bounds above are tight enough to see a layout misread: a definition applied to data of a sibling layout (U / V
    swapped, Y0 / Y1 swapped, the chroma planes exchanged, chroma sited one row pair too low) misses by far more."""
    rng = np.random.default_rng(3)
    h, w = 38, 52
    for right, wrong in (("NV12", "NV21"), ("I420", "YV12"), ("YUY2", "YVYU"), ("YUY2", "UYVY"), ("UYVY", "YUY2")):
        planes = ref.yuv_block_planes(rng, h, w, right)
        f = ref.encode_yuv(*planes, right)
        good = np.stack(planes, -1).reshape(-1, 3)
        bad = np.stack(ref.decode_yuv(f, wrong), -1).reshape(-1, 3)
        code = next(c for c, v in ref.YUV_SOURCES.items() if v[0] == right and v[1] == "bgr" and v[2] == 3)
        d = ref.pixel_definition(code, bad) - ref.pixel_definition(code, good)
        assert np.abs(d).max() > 100 and np.abs(d).mean() > 10, (right, wrong, np.abs(d).max(), np.abs(d).mean())
    # 4:2:0 siting: chroma row (y + 1) / 2 instead of y / 2 for the odd luma rows
    y, u, v = ref.yuv_block_planes(rng, h, w, "NV12")
    rows = np.minimum((np.arange(h) + 1) >> 1, h // 2 - 1) * 2
    d = ref.pixel_definition(91, np.stack([y, u[rows], v[rows]], -1).reshape(-1, 3)) - ref.pixel_definition(
        91, np.stack([y, u, v], -1).reshape(-1, 3))
    assert np.abs(d).max() > 100 and np.abs(d).mean() > 5
