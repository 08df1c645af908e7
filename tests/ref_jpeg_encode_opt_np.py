"""libjpeg's optimize_coding in plain Python: what ImageEncoder's optimize = 1 must compute.  Three pieces:
symbol_stats() is jchuff's htest_one_block over the coefficients of ref_jpeg_encode_np.coefficients() -- the symbols that
module's block coder emits, counted per table --, optimal_table() is jpeg_gen_optimal_table in libjpeg 6b's form (which
libjpeg-turbo keeps), and header() puts the four DHT segments built from them in the place of the Annex K ones.  The scan is
then ref_jpeg_encode_np.scan / ref_jpeg_encode_norst_np.scan_norst with that header.  Checked against the streams Pillow wrote
with optimize=True in tests/test_jpeg_encode_opt.py."""
import numpy as np

from ref_jpeg_encode_np import ZIGZAG, coefficients, huffman_tables, scan   # noqa: F401  (for the callers)
from ref_jpeg_encode_norst_np import row_bits, scan_norst, unstuffed   # noqa: F401

TABLES = ((0, 0), (1, 0), (0, 1), (1, 1))   # (class, id) in the order of the DHT segments: DC luma, AC luma, DC chroma, AC chroma
ROW, NONE = 0, 1


def symbol_stats(coef, h, w, hs, vs, restart):
    """(4, 256) int64 counts, tables in the order of TABLES.  restart ROW: the DC predictors reset at each MCU row; NONE: kept."""
    mcols, mrows = -(-w // (8 * hs)), -(-h // (8 * vs))
    nl = mrows * vs * mcols * hs
    luma = coef[:nl * 64].reshape(mrows * vs, mcols * hs, 64).astype(int)
    chroma = [coef[(nl + c * mrows * mcols) * 64:(nl + (c + 1) * mrows * mcols) * 64].reshape(mrows, mcols, 64).astype(int) for c in range(2)]
    freq = np.zeros((4, 256), np.int64)
    pred = [0, 0, 0]

    def block(b, comp):
        dc, ac = (0, 1) if comp == 0 else (2, 3)
        b = [int(v) for v in b]
        diff = b[0] - pred[comp]
        pred[comp] = b[0]
        freq[dc, abs(diff).bit_length()] += 1
        run = 0
        for k in range(1, 64):
            v = b[ZIGZAG[k]]
            if v == 0:
                run += 1
                continue
            while run >= 16:
                freq[ac, 0xF0] += 1
                run -= 16
            freq[ac, run << 4 | abs(v).bit_length()] += 1
            run = 0
        if run:
            freq[ac, 0] += 1

    for my in range(mrows):
        if restart == ROW:
            pred = [0, 0, 0]
        for mx in range(mcols):
            for k in range(hs * vs):
                block(luma[my * vs + k // hs, mx * hs + k % hs], 0)
            block(chroma[0][my, mx], 1)
            block(chroma[1][my, mx], 2)
    return freq


def code_sizes(freq):
    """The code size of each of the 257 entries (0: no code) before any limiting: the merge loop of jpeg_gen_optimal_table."""
    freq = [int(v) for v in freq] + [1]          # the reserved pseudo-symbol: no real code is all ones
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1, v = -1, None
        for i in range(257):                      # upward with <=: among equal frequencies the LARGEST index
            if freq[i] and (v is None or freq[i] <= v):
                v, c1 = freq[i], i
        c2, v = -1, None
        for i in range(257):
            if freq[i] and i != c1 and (v is None or freq[i] <= v):
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    return codesize


def optimal_table(freq):
    """(bits, vals): bits[k] codes of k + 1 bits, k < 16; vals the symbols by code length, then by value."""
    codesize = code_sizes(freq)
    assert max(codesize) <= 32, "libjpeg stops here (JERR_HUFF_CLEN_OVERFLOW)"
    bits = [0] * 33
    for s in codesize:
        if s:
            bits[s] += 1
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    vals = [s for ln in range(1, 33) for s in range(256) if codesize[s] == ln]
    return bits[1:17], vals


def dht(bits, vals, cls, ident):
    return b"\xff\xc4" + (3 + 16 + len(vals)).to_bytes(2, "big") + bytes([cls << 4 | ident]) + bytes(bits) + bytes(vals)


def header(fixed, freq):
    """`fixed` (the library's header with the Annex K tables, either restart mode) with its four DHT segments replaced by those of
    the (4, 256) counts."""
    out, i, t = bytearray(fixed[:2]), 2, 0
    while i < len(fixed):
        length = int.from_bytes(fixed[i + 2:i + 4], "big")
        if fixed[i + 1] == 0xC4:
            cls, ident = TABLES[t]
            assert fixed[i + 4] == cls << 4 | ident
            out += dht(*optimal_table(freq[t]), cls, ident)
            t += 1
        else:
            out += fixed[i:i + 2 + length]
        i += 2 + length
    assert t == 4
    return bytes(out)


def encode(coef, h, w, hs, vs, restart, fixed):
    """(the whole stream, its header's length, the counts) for coefficients in the layout of coefficients()."""
    freq = symbol_stats(coef, h, w, hs, vs, restart)
    hd = header(fixed, freq)
    body = scan(coef, h, w, hs, vs, hd) if restart == ROW else scan_norst(coef, h, w, hs, vs, hd)[0]
    return hd + body, len(hd), freq
