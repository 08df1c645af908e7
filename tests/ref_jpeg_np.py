"""Baseline JPEG in numpy: the definition the ImageDecoder op is held to, restated without any shared
code -- a bit-by-bit Huffman decoder, libjpeg's "islow" integer inverse DCT (CONST_BITS 13, PASS1_BITS 2, columns first),
"fancy" triangle upsampling (replication for planes at most 2 samples wide) and the 16-bit YCbCr -> RGB conversion.
It reads baseline streams only (SOF0, one scan, 1 or 3 components) and raises ValueError on anything else.  CPU tests only.
"""
import numpy as np


def zigzag():
    """Position k of the zigzag scan -> row-major index of the 8 x 8 block, by walking the anti-diagonals."""
    order = []
    for s in range(15):
        cells = [(i, s - i) for i in range(8) if 0 <= s - i < 8]
        order += cells if s % 2 else cells[::-1]
    return [r * 8 + c for r, c in order]


ZIGZAG = zigzag()


class _Bits:
    """MSB-first bits of an entropy-coded segment, FF00 unstuffed; stops at any other marker."""

    def __init__(self, data, pos):
        self.data, self.pos, self.acc, self.n = data, pos, 0, 0

    def bit(self):
        if self.n == 0:
            if self.pos >= len(self.data):
                raise ValueError("scan data ends early")
            b = self.data[self.pos]
            if b == 0xFF:
                nxt = self.data[self.pos + 1] if self.pos + 1 < len(self.data) else None
                while nxt == 0xFF:          # fill bytes
                    self.pos += 1
                    nxt = self.data[self.pos + 1] if self.pos + 1 < len(self.data) else None
                if nxt != 0:
                    raise ValueError("marker inside a block")
                self.pos += 2
            else:
                self.pos += 1
            self.acc, self.n = b, 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, k):
        v = 0
        for _ in range(k):
            v = (v << 1) | self.bit()
        return v

    def restart(self, index):
        self.n = 0
        while self.pos + 1 < len(self.data) and self.data[self.pos] == 0xFF and self.data[self.pos + 1] == 0xFF:
            self.pos += 1
        if self.data[self.pos:self.pos + 2] != bytes([0xFF, 0xD0 + (index & 7)]):
            raise ValueError("restart marker missing")
        self.pos += 2


def _huff_table(counts, vals):
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return table


def _symbol(br, table):
    code = 0
    for length in range(1, 17):
        code = (code << 1) | br.bit()
        if (length, code) in table:
            return table[(length, code)]
    raise ValueError("bad Huffman code")


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def parse(data):
    """Markers and entropy decoding.  Returns a dict: h, w, samp [(H, V)] per component, restart_interval, quant
    (ncomp, 64) uint16 in natural order, coef: per component an (block rows, block cols, 64) int16 array in natural order."""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise ValueError("no SOI")
    pos, quant, huff, frame, ri = 2, {}, {}, None, 0
    while True:
        if pos + 4 > len(data) or data[pos] != 0xFF:
            raise ValueError("no marker")
        while data[pos] == 0xFF:
            pos += 1
        m = data[pos]
        pos += 1
        length = int.from_bytes(data[pos:pos + 2], "big")
        seg = data[pos + 2:pos + length]
        if pos + length > len(data):
            raise ValueError("segment cut short")
        pos += length
        if m == 0xC0:
            if seg[0] != 8:
                raise ValueError("precision")
            h, w, nc = int.from_bytes(seg[1:3], "big"), int.from_bytes(seg[3:5], "big"), seg[5]
            frame = (h, w, [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(nc)])
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise ValueError("not baseline")
        elif m == 0xC4:
            i = 0
            while i < len(seg):
                counts = list(seg[i + 1:i + 17])
                n = sum(counts)
                huff[(seg[i] >> 4, seg[i] & 15)] = _huff_table(counts, seg[i + 17:i + 17 + n])
                i += 17 + n
        elif m == 0xDB:
            i = 0
            while i < len(seg):
                if seg[i] >> 4:
                    raise ValueError("16-bit quantisation table")
                q = np.zeros(64, np.uint16)
                q[ZIGZAG] = np.frombuffer(seg[i + 1:i + 65], np.uint8)
                quant[seg[i] & 15] = q
                i += 65
        elif m == 0xDD:
            ri = int.from_bytes(seg[:2], "big")
        elif m == 0xDA:
            break
    h, w, comps = frame
    nc = len(comps)
    if nc not in (1, 3) or seg[0] != nc:
        raise ValueError("components")
    sel = [(seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15) for c in range(nc)]
    samp = [(1, 1)] if nc == 1 else [(H, V) for _, H, V, _ in comps]
    hmax, vmax = max(s[0] for s in samp), max(s[1] for s in samp)
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    coef = [np.zeros((mcuy * V, mcux * H, 64), np.int16) for H, V in samp]
    br, pred, mcu = _Bits(data, pos), [0] * nc, 0
    for my in range(mcuy):
        for mx in range(mcux):
            if ri and mcu and mcu % ri == 0:
                br.restart(mcu // ri - 1)
                pred = [0] * nc
            for c, (H, V) in enumerate(samp):
                dc, ac = huff[(0, sel[c][0])], huff[(1, sel[c][1])]
                for v in range(V):
                    for hh in range(H):
                        blk = coef[c][my * V + v, mx * H + hh]
                        s = _symbol(br, dc)
                        pred[c] += _extend(br.bits(s), s)
                        blk[0] = pred[c]
                        k = 1
                        while k < 64:
                            rs = _symbol(br, ac)
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            blk[ZIGZAG[k]] = _extend(br.bits(s), s)
                            k += 1
            mcu += 1
    return {"h": h, "w": w, "samp": samp, "restart_interval": ri, "coef": coef,
            "quant": np.stack([quant[comps[c][3]] for c in range(nc)])}


def _pass(x, n):
    """One 8-point pass along the last axis of an int64 array (values stay within int32)."""
    i0, i1, i2, i3, i4, i5, i6, i7 = [x[..., k] for k in range(8)]
    z1 = (i2 + i6) * 4433
    t2, t3 = z1 - i6 * 15137, z1 + i2 * 6270
    t0, t1 = (i0 + i4) << 13, (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a, b, c, d = i7, i5, i3, i1
    z1, z2, z3, z4 = a + d, b + c, a + c, b + d
    z5 = (z3 + z4) * 9633
    a, b, c, d = a * 2446, b * 16819, c * 25172, d * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    a, b, c, d = a + z1 + z3, b + z2 + z4, c + z2 + z3, d + z1 + z4
    out = np.stack([t10 + d, t11 + c, t12 + b, t13 + a, t13 - a, t12 - b, t11 - c, t10 - d], axis=-1)
    return (out + (1 << (n - 1))) >> n


def idct_plane(coef, quant):
    """(block rows, block cols, 64) coefficients -> (8 rows, 8 cols) uint8 plane."""
    br_, bc, _ = coef.shape
    x = (coef.astype(np.int64) * quant.astype(np.int64)).reshape(br_, bc, 8, 8)
    x = _pass(x.swapaxes(2, 3), 11).swapaxes(2, 3)   # down the columns first
    x = _pass(x, 18)                                  # then along the rows
    x = np.clip(x + 128, 0, 255).astype(np.uint8)
    return x.transpose(0, 2, 1, 3).reshape(br_ * 8, bc * 8)


def _h2(p, rnd_even, rnd_odd, shift):
    """2:1 triangle filter along the last axis of an int array p (dw columns)."""
    left = np.concatenate([p[..., :1], p[..., :-1]], axis=-1)
    right = np.concatenate([p[..., 1:], p[..., -1:]], axis=-1)
    out = np.empty(p.shape[:-1] + (2 * p.shape[-1],), np.int64)
    out[..., 0::2] = (3 * p + left + rnd_even) >> shift
    out[..., 1::2] = (3 * p + right + rnd_odd) >> shift
    return out


def upsample(plane, h, w, H, V, hmax, vmax):
    """A component's block-padded plane -> (h, w) at full resolution."""
    dw, dh = -(-w * H // hmax), -(-h * V // vmax)
    p = plane[:dh, :dw].astype(np.int64)
    fh, fv = hmax // H, vmax // V
    if fh == 1 and fv == 1:
        return p[:h, :w]
    if dw <= 2:
        return np.repeat(np.repeat(p, fv, axis=0), fh, axis=1)[:h, :w]
    if fv == 1:
        return _h2(p, 1, 2, 2)[:h, :w]
    above = np.concatenate([p[:1], p[:-1]], axis=0)
    below = np.concatenate([p[1:], p[-1:]], axis=0)
    t = np.empty((2 * dh, dw), np.int64)
    t[0::2] = 3 * p + above
    t[1::2] = 3 * p + below
    return _h2(t, 8, 7, 4)[:h, :w]


def decode(data):
    """The decoded frame: (h, w, 3) uint8 RGB, or (h, w, 1) for a one-component stream."""
    s = parse(data)
    h, w, samp = s["h"], s["w"], s["samp"]
    if len(samp) == 3 and (samp[1] != (1, 1) or samp[2] != (1, 1) or samp[0] not in ((1, 1), (2, 1), (2, 2))):
        raise ValueError("sampling")
    hmax, vmax = max(x[0] for x in samp), max(x[1] for x in samp)
    planes = [upsample(idct_plane(s["coef"][c], s["quant"][c]), h, w, samp[c][0], samp[c][1], hmax, vmax) for c in range(len(samp))]
    if len(planes) == 1:
        return planes[0].astype(np.uint8)[..., None]
    y, cb, cr = planes[0], planes[1] - 128, planes[2] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def coefficients(data):
    """The layout of st_jpeg_coefficients: every component's blocks in raster order, concatenated; and the tables."""
    s = parse(data)
    return np.concatenate([c.reshape(-1) for c in s["coef"]]), s["quant"]
