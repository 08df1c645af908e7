"""jchuff's entropy coder for a scan WITHOUT restart markers (libjpeg's restart_interval = 0, what cv::imencode, Pillow's
save(quality=q, subsampling=s) and cjpeg write by default), in plain Python: what ImageEncoder's restart = NONE must compute.
It is tests/ref_jpeg_encode_np.scan with three changes: the DC predictors are kept across MCU rows, no MCU row is padded, and
the padding with 1-bits and the FF -> FF 00 stuffing are applied once, over the whole scan.  The coefficients and their layout
are those of ref_jpeg_encode_np.coefficients().  Checked against the streams Pillow wrote in tests/test_jpeg_encode_norst.py."""
from ref_jpeg_encode_np import ZIGZAG, BitString, coefficients, huffman_tables   # noqa: F401  (coefficients: for the callers)


def row_bits(coef, h, w, hs, vs, header):
    """Per MCU row (value, length): the row's code bits as an integer, the first bit the most significant, and their number."""
    tabs = huffman_tables(header)
    mcols, mrows = -(-w // (8 * hs)), -(-h // (8 * vs))
    nl = mrows * vs * mcols * hs
    luma = coef[:nl * 64].reshape(mrows * vs, mcols * hs, 64).astype(int)
    chroma = [coef[(nl + c * mrows * mcols) * 64:(nl + (c + 1) * mrows * mcols) * 64].reshape(mrows, mcols, 64).astype(int) for c in range(2)]
    pred = [0, 0, 0]   # only the picture's first MCU predicts from 0
    rows = []
    for my in range(mrows):
        bits = BitString()
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
        rows.append(bits.value())
    return rows


def scan_norst(coef, h, w, hs, vs, header):
    """(the entropy-coded scan and EOI, the MCU rows' bit offsets in the unstuffed scan followed by its length in bits) for
    coefficients in the layout of coefficients(): one scan, no restart interval, the tables of the header's DHT segments."""
    scan, nbits, offsets = BitString(), 0, []
    for value, length in row_bits(coef, h, w, hs, vs, header):
        offsets.append(nbits)
        scan.put(value, length)
        nbits += length
    offsets.append(nbits)
    acc, nbits = scan.value()
    if nbits % 8:
        fill = 8 - nbits % 8
        acc, nbits = (acc << fill) | ((1 << fill) - 1), nbits + fill
    return acc.to_bytes(nbits // 8, "big").replace(b"\xff", b"\xff\x00") + b"\xff\xd9", offsets


def unstuffed(jpg, header_bytes=623):
    """The scan of a stream without restart markers as it was before the stuffing (padding included)."""
    assert jpg[-2:] == b"\xff\xd9"
    return jpg[header_bytes:-2].replace(b"\xff\x00", b"\xff")
