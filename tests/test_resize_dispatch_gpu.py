"""One case per cell of st_resize_u8_batch's launcher (csrc/st_imgproc.hip, the `if` chain after rs_plan): every
interpolation x channel count x scale band.  Each case must equal the C oracle bit for bit AND lie within
tests/ref_resize_np.py's tolerances of the float64 definition, measured on the kernel's own output -- so a kernel
and the oracle changed together around one misreading of cv::resize still fail.  Output widths are odd (53): the
last group of four columns of the vector kernels is partial."""
import numpy as np
import pytest

import oracle
import ref_resize_np as ref
from util import smooth_texture

NEAREST, LINEAR, CUBIC, AREA, LANCZOS4 = ref.NEAREST, ref.LINEAR, ref.CUBIC, ref.AREA, ref.LANCZOS4
MODE_NAMES = {NEAREST: "nearest", LINEAR: "linear", CUBIC: "cubic", AREA: "area", LANCZOS4: "lanczos4"}

# scale band -> ((h, w) source, (dh, dw) target)
BANDS = {
    "copy":         ((37, 53), (37, 53)),
    "exact2x2":     ((74, 106), (37, 53)),
    "int_x2_y3":    ((111, 106), (37, 53)),
    "int_x3_y2":    ((74, 159), (37, 53)),
    "int_x4_y3":    ((111, 212), (37, 53)),
    "int_x5_y6":    ((222, 265), (37, 53)),
    "frac_le2":     ((61, 83), (37, 53)),      # 1.65 x 1.57
    "frac_2to6":    ((150, 201), (37, 53)),    # 4.05 x 3.79
    "frac_gt6":     ((260, 375), (37, 53)),    # 7.03 x 7.08
    "enlarge_x":    ((61, 23), (37, 53)),      # y shrinks, x enlarges
    "enlarge_both": ((23, 31), (37, 53)),
}

ALL_KERNELS = {"k_resize_area2_c3_v4", "k_resize_area_c3_v4<4>", "k_resize_area_c3_v4<8>", "k_resize_area_int_c3_v4<2>",
               "k_resize_area_int_c3_v4<3>", "k_resize_area_int_c3_v4<4>", "k_resize_lanczos4_c3", "k_resize_nearest_c3_v4",
               "k_resize_cubic_c3_v4", "k_resize_linear_c3_v4<true>", "k_resize_linear_c3_v4<false>", "k_resize_u8"}


def launcher_kernel(mode, cn, h, w, dh, dw):
    """The kernel st_resize_u8_batch launches: rs_plan's mode, then the launcher's `if` chain, in their order."""
    scale_x, scale_y = 1.0 / (dw / w), 1.0 / (dh / h)
    isx, isy = int(np.rint(scale_x)), int(np.rint(scale_y))
    eps = np.finfo(np.float64).eps
    area_fast = abs(scale_x - isx) < eps and abs(scale_y - isy) < eps
    if (h, w) == (dh, dw):
        plan = "COPY"
    elif mode == NEAREST:
        plan = "NEAREST"
    elif mode == CUBIC:
        plan = "CUBIC"
    elif mode == LANCZOS4:
        plan = "LANCZOS4"
    elif mode in (LINEAR, AREA) and area_fast and isx == 2 and isy == 2:
        plan = "AREA2"
    elif mode == LINEAR:
        plan = "LINEAR"
    elif scale_x >= 1 and scale_y >= 1:
        plan = "AREA_INT" if area_fast else "AREA"
    else:
        plan = "LINEAR_AREA"
    if plan == "AREA2" and cn == 3:
        return "k_resize_area2_c3_v4"
    if plan == "AREA" and cn == 3 and scale_x <= 6:
        return "k_resize_area_c3_v4<4>" if scale_x <= 2 else "k_resize_area_c3_v4<8>"
    if plan == "AREA_INT" and cn == 3 and 2 <= isx <= 4:
        return "k_resize_area_int_c3_v4<%d>" % isx
    if plan == "LANCZOS4" and cn == 3:
        return "k_resize_lanczos4_c3"
    if plan == "NEAREST" and cn == 3:
        return "k_resize_nearest_c3_v4"
    if plan == "CUBIC" and cn == 3:
        return "k_resize_cubic_c3_v4"
    if plan == "LINEAR_AREA" and cn == 3:
        return "k_resize_linear_c3_v4<true>"
    if plan == "LINEAR" and cn == 3:
        return "k_resize_linear_c3_v4<false>"
    return "k_resize_u8"


CASES = [(MODE_NAMES[m], cn, band, launcher_kernel(m, cn, *BANDS[band][0], *BANDS[band][1]))
         for m in MODE_NAMES for cn in (1, 2, 3, 4) for band in BANDS]


def test_table_reaches_every_kernel_of_the_launcher():
    """CPU-side: the case table covers every kernel (and template instance) the launcher can pick."""
    assert {c[3] for c in CASES} == ALL_KERNELS


def frames_for(h, w, cn, seed):
    """Two distinct textured frames (smooth texture plus a little noise: gradients everywhere, no flat areas)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(2):
        t = np.stack([smooth_texture(seed * 13 + 5 * i + k, h, w, 2.0) for k in range(cn)], -1)
        out.append(np.clip(t + rng.normal(0, 2, t.shape), 0, 255).astype(np.uint8))
    return np.stack(out)


def check_against_definition(got, frame, mode, dh, dw, what):
    h, w = frame.shape[:2]
    emax, bias, sx, sy = ref.error_stats(got, ref.resize(frame, dw, dh, mode))
    tol, btol = ref.tolerances(mode, h, w, dh, dw)
    assert emax <= tol, "%s: max error %.3f > %.2f against the float64 definition" % (what, emax, tol)
    if got.size >= 400:
        assert abs(bias) <= btol, "%s: bias %.3f > %.2f" % (what, bias, btol)
        assert abs(sx) <= 0.05 and abs(sy) <= 0.05, "%s: sampling grid displaced by (%.3f, %.3f) px" % (what, sx, sy)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,cn,band,kernel", CASES, ids=["%s-c%d-%s-%s" % c for c in CASES])
def test_resize_dispatch_cell(hip_ctx, mode, cn, band, kernel):
    import torch
    m = {v: k for k, v in MODE_NAMES.items()}[mode]
    (h, w), (dh, dw) = BANDS[band]
    f = frames_for(h, w, cn, 100 * m + 10 * cn + list(BANDS).index(band))
    got = hip_ctx.resize(torch.from_numpy(f).cuda(), dw, dh, m).cpu().numpy()
    assert got.shape == (2, dh, dw, cn)
    for i in range(2):
        what = "%s (%s c%d %s) frame %d" % (kernel, mode, cn, band, i)
        np.testing.assert_array_equal(got[i], oracle.resize_u8(f[i], dw, dh, m), err_msg=what)
        check_against_definition(got[i], f[i], m, dh, dw, what)


@pytest.mark.gpu
@pytest.mark.parametrize("cn", [1, 2, 3, 4])
def test_resize_empty_tensor_batch_keeps_channels(hip_ctx, cn):
    import torch
    got = hip_ctx.resize(torch.zeros((0, 9, 11, cn), dtype=torch.uint8, device="cuda"), 5, 4)
    assert tuple(got.shape) == (0, 4, 5, cn)
