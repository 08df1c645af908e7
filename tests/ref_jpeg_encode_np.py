"""libjpeg's forward path (jccolor, jcsample, jfdctint's "islow" DCT, quantisation, the dummy blocks of jccoefct) restated in
plain integer numpy, and jchuff's entropy coder in plain Python: what the ImageEncoder op must compute.  coefficients() returns
the quantised coefficients in the layout of st_jpeg_coefficients and scan() the entropy-coded bytes, so both are checked
against the streams Pillow wrote (tests/test_jpeg_encode.py) -- that guards the fixture and the restatement in DESIGN.md 4.16
at once."""
import numpy as np

I = np.int64


def rgb_to_ycc(img):
    r, g, b = (img[..., c].astype(I) for c in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _edge(a, rows, cols):
    return np.pad(a, ((0, rows - a.shape[0]), (0, cols - a.shape[1])), mode="edge")


def component(plane, hs, vs):
    """The component's samples, block-padded: the input's last column replicated before the downsampling, its last row up to
    a multiple of vs; the box filter with its alternating bias; then the downsampled last row replicated."""
    h, w = plane.shape
    cw, ch = -(-w // hs), -(-h // vs)
    nbx, nby = -(-cw // 8), -(-ch // 8)
    p = _edge(plane, ch * vs, nbx * 8 * hs)
    x = np.arange(nbx * 8, dtype=I)
    if (hs, vs) == (2, 1):
        p = (p[:, 0::2] + p[:, 1::2] + (x & 1)) >> 1
    elif (hs, vs) == (2, 2):
        p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 1 + (x & 1)) >> 2
    else:
        assert (hs, vs) == (1, 1)
    return _edge(p, nby * 8, nbx * 8)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _pass(d, first):
    """One pass of jfdctint over the last axis."""
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def blocks(comp, quant):
    """(rows / 8, cols / 8, 64) quantised coefficients, natural order, of a block-padded component."""
    bh, bw = comp.shape[0] // 8, comp.shape[1] // 8
    b = comp.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - 128          # (bh, bw, row, column)
    b = _pass(b, True)                                                   # over the rows
    b = _pass(b.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)      # over the columns
    d = quant.astype(I).reshape(8, 8) * 8
    q = (np.abs(b) + (d >> 1)) // d
    return (np.sign(b) * q).reshape(bh, bw, 64)


def coefficients(img, luma_q, chroma_q, hs, vs):
    """int16 coefficients of the (h, w, 3) picture in the layout of st_jpeg_coefficients: luma, Cb, Cr, each component's blocks
    in raster order of its MCU-padded plane.  A luma block beyond the real ones has no AC terms and the DC of the block before
    it in its MCU (jccoefct.c compress_data)."""
    h, w = img.shape[:2]
    y, cb, cr = rgb_to_ycc(img)
    mcols, mrows = -(-w // (8 * hs)), -(-h // (8 * vs))
    real = blocks(component(y, 1, 1), luma_q)
    nby, nbx = real.shape[:2]
    luma = np.zeros((mrows * vs, mcols * hs, 64), I)
    for my in range(mrows):
        for mx in range(mcols):
            prev = 0
            for k in range(hs * vs):
                by, bx = my * vs + k // hs, mx * hs + k % hs
                if by < nby and bx < nbx:
                    luma[by, bx] = real[by, bx]
                else:
                    luma[by, bx, 0] = prev
                prev = luma[by, bx, 0]
    out = [luma.reshape(-1)]
    for plane in (cb, cr):
        c = blocks(component(plane, hs, vs), chroma_q)
        assert c.shape[:2] == (mrows, mcols)
        out.append(c.reshape(-1))
    return np.concatenate(out).astype(np.int16)


ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57,
          50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def huffman_tables(header):
    """{(class, id): {symbol: (code, length)}} of the DHT segments in a stream's header (canonical codes, T.81 Annex C)."""
    tables, i = {}, 2
    while i < len(header):
        marker, length = header[i + 1], int.from_bytes(header[i + 2:i + 4], "big")
        seg = header[i + 4:i + 2 + length]
        if marker == 0xC4:
            bits, vals = seg[1:17], seg[17:]
            code, k, tab = 0, 0, {}
            for ln in range(1, 17):
                for _ in range(bits[ln - 1]):
                    tab[vals[k]] = (code, ln)
                    code, k = code + 1, k + 1
                code <<= 1
            tables[(seg[0] >> 4, seg[0] & 15)] = tab
        i += 2 + length
    return tables


class BitString:
    """Code bits appended first bit first.  The bits are kept in pieces of a few thousand and joined pairwise at the end, so that
    a row of a million bits costs no more per code than a short one (one growing integer would be shifted whole at every code)."""
    PIECE = 4096

    def __init__(self):
        self.parts, self.acc, self.n = [], 0, 0

    def put(self, code, length):
        self.acc, self.n = (self.acc << length) | code, self.n + length
        if self.n >= self.PIECE:
            self.parts.append((self.acc, self.n))
            self.acc, self.n = 0, 0

    def __len__(self):
        return self.n + sum(n for _, n in self.parts)

    def value(self):
        """(the bits as an integer, the first bit the most significant; their number)"""
        parts = self.parts + [(self.acc, self.n)]
        while len(parts) > 1:
            parts = [(parts[i][0] << parts[i + 1][1] | parts[i + 1][0], parts[i][1] + parts[i + 1][1]) if i + 1 < len(parts) else parts[i]
                     for i in range(0, len(parts), 2)]
        return parts[0]


def scan(coef, h, w, hs, vs, header):
    """The entropy-coded scan and EOI for coefficients in the layout of coefficients(): one restart interval per MCU row
    (jchuff.c encode_mcu_huff with restart_interval = MCUs per row), the tables of the header's DHT segments."""
    tabs = huffman_tables(header)
    mcols, mrows = -(-w // (8 * hs)), -(-h // (8 * vs))
    nl = mrows * vs * mcols * hs
    luma = coef[:nl * 64].reshape(mrows * vs, mcols * hs, 64).astype(int)
    chroma = [coef[(nl + c * mrows * mcols) * 64:(nl + (c + 1) * mrows * mcols) * 64].reshape(mrows, mcols, 64).astype(int) for c in range(2)]
    out = bytearray()
    for my in range(mrows):
        bits, pred = BitString(), [0, 0, 0]
        put = bits.put

        def block(b, comp):
            b = [int(v) for v in b]
            dc, ac = tabs[(0, min(comp, 1))], tabs[(1, min(comp, 1))]
            diff = b[0] - pred[comp]
            pred[comp] = b[0]
            n = abs(diff).bit_length()
            put(*dc[n])
            put((diff if diff >= 0 else diff - 1) & ((1 << n) - 1), n)
            run = 0
            for k in range(1, 64):
                v = b[ZIGZAG[k]]
                if v == 0:
                    run += 1
                    continue
                while run >= 16:
                    put(*ac[0xF0])
                    run -= 16
                n = abs(v).bit_length()
                put(*ac[run << 4 | n])
                put((v if v >= 0 else v - 1) & ((1 << n) - 1), n)
                run = 0
            if run:
                put(*ac[0])

        for mx in range(mcols):
            for k in range(hs * vs):
                block(luma[my * vs + k // hs, mx * hs + k % hs], 0)
            block(chroma[0][my, mx], 1)
            block(chroma[1][my, mx], 2)
        if len(bits) % 8:
            put((1 << (8 - len(bits) % 8)) - 1, 8 - len(bits) % 8)
        acc, nbits = bits.value()
        data = acc.to_bytes(nbits // 8, "big")
        out += data.replace(b"\xff", b"\xff\x00")
        out += bytes([0xFF, 0xD0 + my % 8]) if my < mrows - 1 else b"\xff\xd9"
    return bytes(out)
