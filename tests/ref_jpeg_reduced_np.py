"""libjpeg's scaled decoding (scale 1/2, 1/4, 1/8) in numpy: the definition ImageDecoder's `scale` is held to.
It restates jdmaster's per-component choice of the inverse DCT size, jidctint's 4 x 4 and 2 x 2 reduced transforms and the 1 x 1
DC-only one, and the upsampling that is left at a reduced scale; parsing, the 8 x 8 pass, the h2v1 triangle filter and the
colour conversion are ref_jpeg_np's.  Pillow's im.draft() produces the same bytes wherever it can be asked (tests/test_jpeg_reduced.py).
CPU tests only.
"""
import numpy as np

import ref_jpeg_np as R

DENOMS = (1, 2, 4, 8)


def cdiv(a, b):
    return -(-a // b)


def scaled_size(h, w, d):
    """(oh, ow) of an (h, w) frame decoded at 1/d."""
    if d not in DENOMS:
        raise ValueError("scale denominator %r" % (d,))
    return cdiv(h, d), cdiv(w, d)


def geometry(h, w, samp, d):
    """Per component: the inverse DCT size S, the extent (dh, dw) of its reduced plane, and the upsampling factors (fv, fh) left."""
    if d not in DENOMS:
        raise ValueError("scale denominator %r" % (d,))
    m = 8 // d
    hmax, vmax = max(s[0] for s in samp), max(s[1] for s in samp)
    out = []
    for H, V in samp:
        S = m
        while S < 8 and (hmax * m) % (H * S * 2) == 0 and (vmax * m) % (V * S * 2) == 0:
            S *= 2
        out.append({"S": S, "dw": cdiv(w * H * S, hmax * 8), "dh": cdiv(h * V * S, vmax * 8),
                    "fh": hmax * m // (H * S), "fv": vmax * m // (V * S)})
    return out


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _pass4(x, n):
    """jpeg_idct_4x4's 4-point pass along the last axis (8 inputs, entry 4 unread)."""
    i0, i1, i2, i3, _, i5, i6, i7 = [x[..., k] for k in range(8)]
    t0 = i0 << 14
    t2 = 15137 * i2 - 6270 * i6
    t10, t12 = t0 + t2, t0 - t2
    a = -1730 * i7 + 11893 * i5 - 17799 * i3 + 8697 * i1
    b = -4176 * i7 - 4926 * i5 + 7373 * i3 + 20995 * i1
    return _descale(np.stack([t10 + b, t12 + a, t12 - a, t10 - b], axis=-1), n)


def _pass2(x, n):
    """jpeg_idct_2x2's 2-point pass along the last axis (entries 0, 1, 3, 5, 7 read)."""
    i0, i1, _, i3, _, i5, _, i7 = [x[..., k] for k in range(8)]
    t10 = i0 << 15
    t0 = -5906 * i7 + 6967 * i5 - 10426 * i3 + 29692 * i1
    return _descale(np.stack([t10 + t0, t10 - t0], axis=-1), n)


def idct_plane(coef, quant, S):
    """(block rows, block cols, 64) coefficients -> (S rows, S cols per block) uint8 plane."""
    if S == 8:
        return R.idct_plane(coef, quant)
    br_, bc, _ = coef.shape
    x = (coef.astype(np.int64) * quant.astype(np.int64)).reshape(br_, bc, 8, 8)
    if S == 4:
        x = _pass4(x.swapaxes(2, 3), 12).swapaxes(2, 3)   # down the columns: (4 rows, 8 cols); column 4 is never read again
        x = _pass4(x, 19)
    elif S == 2:
        x = _pass2(x.swapaxes(2, 3), 13).swapaxes(2, 3)
        x = _pass2(x, 20)
    else:
        x = _descale(x[:, :, :1, :1], 3)
    x = np.clip(x + 128, 0, 255).astype(np.uint8)
    return x.transpose(0, 2, 1, 3).reshape(br_ * S, bc * S)


def decode(data, d):
    """The frame libjpeg hands out at scale 1/d: (ceil(h/d), ceil(w/d), 3) uint8 RGB, or (.., .., 1) for one component."""
    if d == 1:
        return R.decode(data)
    return decode_parsed(R.parse(data), d)


def decode_parsed(s, d):
    """decode() for d = 2, 4 or 8 from ref_jpeg_np.parse()'s result, so that one parse serves every denominator."""
    h, w, samp = s["h"], s["w"], s["samp"]
    if len(samp) == 3 and (samp[1] != (1, 1) or samp[2] != (1, 1) or samp[0] not in ((1, 1), (2, 1), (2, 2))):
        raise ValueError("sampling")
    oh, ow = scaled_size(h, w, d)
    planes = []
    for c, g in enumerate(geometry(h, w, samp, d)):
        p = idct_plane(s["coef"][c], s["quant"][c], g["S"])[:g["dh"], :g["dw"]].astype(np.int64)
        assert g["fv"] == 1 and g["fh"] in (1, 2)
        if g["fh"] == 2:
            # libjpeg switches fancy upsampling off when min_DCT_scaled_size is 1, and never uses it on a plane <= 2 wide
            p = np.repeat(p, 2, axis=1) if (g["dw"] <= 2 or d == 8) else R._h2(p, 1, 2, 2)
        planes.append(p[:oh, :ow])
    if len(planes) == 1:
        return planes[0].astype(np.uint8)[..., None]
    y, cb, cr = planes[0], planes[1] - 128, planes[2] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)
