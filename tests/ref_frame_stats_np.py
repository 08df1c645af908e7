"""Float64 and exact-integer definitions of the frame statistics (BrightnessCPP / ContrastCPP / SharpnessCPP and the Python
ops Brightness / Contrast / Sharpness), written from the contract in scannertools_amd/csrc/st_framestats.hip and
independently of the product: numpy for the per-pixel definitions, Python integers and floats for the moments and the
finishing formulas."""
import math

import numpy as np

KINDS = ("BrightnessCPP", "ContrastCPP", "SharpnessCPP", "Brightness", "Contrast", "Sharpness")


def luma(frame):
    """Y of cv::cvtColor(COLOR_RGB2YUV): (R*4899 + G*9617 + B*1868 + 8192) >> 14, as int64 (h, w)."""
    f = frame.astype(np.int64)
    return (f[..., 0] * 4899 + f[..., 1] * 9617 + f[..., 2] * 1868 + 8192) >> 14


def _reflect101(i, n):
    if n == 1:
        return 0
    if i < 0:
        return -i
    if i >= n:
        return 2 * n - 2 - i
    return i


def laplacian(frame):
    """cv::Laplacian(frame, CV_64F) at ksize 1, BORDER_DEFAULT (reflect-101): int64 (h, w, 3)."""
    f = frame.astype(np.int64)
    h, w = f.shape[:2]
    ys = np.array([_reflect101(i, h) for i in range(-1, h + 1)])
    xs = np.array([_reflect101(i, w) for i in range(-1, w + 1)])
    p = f[ys][:, xs]
    return p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:] - 4 * f


def laplacian_loop(frame):
    """The same by an explicit loop over pixels (for checking `laplacian` on small frames)."""
    h, w, c = frame.shape
    out = np.zeros((h, w, c), np.int64)
    for y in range(h):
        for x in range(w):
            for ch in range(c):
                def I(yy, xx):
                    return int(frame[_reflect101(yy, h), _reflect101(xx, w), ch])
                out[y, x, ch] = I(y - 1, x) + I(y + 1, x) + I(y, x - 1) + I(y, x + 1) - 4 * I(y, x)
    return out


def moments(frame, luma_part=True, laplacian_part=True):
    """[SY, QY, S_R, S_G, S_B, Q_R, Q_G, Q_B] as Python ints (the parts not asked for are 0)."""
    m = [0] * 8
    if luma_part:
        y = luma(frame)
        m[0], m[1] = int(y.sum()), int((y * y).sum())
    if laplacian_part:
        L = laplacian(frame)
        for c in range(3):
            m[2 + c] = int(L[..., c].sum())
            m[5 + c] = int((L[..., c] * L[..., c]).sum())
    return m


def finish(m, h, w, kind):
    """The finishing formulas of the contract, in IEEE double without contraction (Python floats); np.float32 for the *CPP
    kinds, np.float64 for the others."""
    N = h * w
    SY, QY, S, Q = int(m[0]), int(m[1]), [int(v) for v in m[2:5]], [int(v) for v in m[5:8]]
    if kind in ("BrightnessCPP", "Brightness"):
        v = float(SY) * (1.0 / N) if kind == "BrightnessCPP" else float(SY) / float(N)
    elif kind in ("ContrastCPP", "Contrast"):
        v = math.sqrt(float(N * QY - SY * SY) / (float(N) * float(N)))
    elif kind == "SharpnessCPP":
        scale = 1.0 / N
        t = 0.0
        for c in range(3):
            mean = float(S[c]) * scale
            var = max(float(Q[c]) * scale - mean * mean, 0.0)
            sd = math.sqrt(var)
            t = t + sd * sd
        v = t / 3.0
    elif kind == "Sharpness":
        n3 = 3 * N
        v = float(n3 * sum(Q) - sum(S) ** 2) / (float(n3) * float(n3))
    else:
        raise ValueError(kind)
    return np.float32(v) if kind.endswith("CPP") else np.float64(v)


def stat(frame, kind):
    h, w = frame.shape[:2]
    sharp = kind.startswith("Sharpness")
    return finish(moments(frame, not sharp, sharp), h, w, kind)


def numpy_python_op(frame, kind):
    """What the reference's Python ops compute, with numpy's own reductions (old/imgproc.py:11-36)."""
    if kind == "Brightness":
        yuv = np.zeros(frame.shape, np.uint8)
        yuv[..., 0] = luma(frame)
        return np.mean(yuv, axis=(0, 1))[0]
    if kind == "Contrast":
        inten = luma(frame).astype(np.uint8).reshape(-1)
        avg = np.mean(inten)
        return np.sqrt(np.mean((inten - avg) ** 2))
    if kind == "Sharpness":
        return laplacian(frame).astype(np.float64).var()
    raise ValueError(kind)


def contrast_cpp_reference_float32(frame):
    """ContrastKernel::execute as written (old/cpp_ops/imgproc.cpp:110-123): the mean from cv::mean (double, SY * (1./N)),
    then ONE float32 running sum of ((float)Y - (float)mean)^2 in row-major order, divided by N in float, float sqrt."""
    y = luma(frame).reshape(-1)
    N = y.size
    mean = np.float32(float(int(y.sum())) * (1.0 / N))
    d = y.astype(np.float32) - mean
    run = np.cumsum(d * d, dtype=np.float32)[-1]
    return np.sqrt(np.float32(run / np.float32(N)))
