"""The PNG stream the ImageEncoder op writes with format = PNG, restated in numpy and plain Python.  This file
is the definition of the bytes: st_png_encode_host and the kernels are compared with it, and it is itself checked against
zlib's inflater, zlib.crc32 and zlib.adler32.  It shares no code with the library.

Stream: signature, IHDR (bit depth 8; colour type 0, 2 or 6 for 1, 3 or 4 channels; not interlaced), one IDAT per piece of
32 768 filtered bytes (the first led by the zlib header 78 01), an IDAT with the final empty stored block and the Adler-32, IEND.

Filtering: every row is its filter type and its filtered bytes.  ADAPTIVE takes, per row, the type 0..4 with the least sum of
min(b, 256 - b) over the filtered bytes, the lowest type among equals; the row above row 0 is zero.

A piece is deflated on its own.  Every maximal run of R equal bytes is one literal, (R - 1) // 258 matches (258, distance 1) and,
for the remaining r = (R - 1) % 258 bytes, one match (r, distance 1) if r >= 3, else r literals.  The piece is one dynamic block
(BFINAL = 0) followed by an empty stored block (3 zero bits, zeros to the byte boundary, 00 00 FF FF); if that is not shorter
than 5 + the piece's bytes, the piece is one stored block instead.

The choices the issue left open:
  * Code lengths: Huffman's algorithm where, of the candidates of least weight, a symbol goes before a merged node, symbols go
    in the order (count, symbol number) and merged nodes in the order they were made.  Only the NUMBER of codes per length is
    taken from the tree.  Lengths beyond the limit are folded back as libjpeg's jpeg_gen_optimal_table does: while a level i
    beyond the limit has codes, two of them leave it, one code arrives at level i - 1, and a code of the deepest level j < i - 1
    that has one moves to j + 1 together with the second.  Then the lengths are dealt out by weight: the symbols in the order
    (count, symbol number) receive the longest lengths first.  Codes are canonical (RFC 1951 3.2.2).
  * With fewer than two counted symbols the lowest-numbered uncounted ones join with weight 1, so that the code is complete.
  * The literal/length set (limit 15) counts the end-of-block symbol once.  HLIT covers the symbols up to the last used one,
    at least 257.  The distance set is the single code 0 of one bit (HDIST = 1); every match spends that bit, a zero.
  * The code-length sequence is the HLIT lengths and the distance length as they are: the symbols 16, 17 and 18 are not used.
    Its code (limit 7) is built the same way; HCLEN drops the trailing unused entries of the order 16 17 18 0 8 7 9 ..., at least 4.
"""
import heapq
import struct
import zlib

import numpy as np

PIECE = 32768
FILTERS = ("none", "sub", "up", "average", "paeth", "adaptive")
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def filter_rows(frame, filter="adaptive"):
    """(h, 1 + w * c) uint8: every row's type and filtered bytes."""
    frame = np.asarray(frame, np.uint8)
    if frame.ndim == 2:
        frame = frame[:, :, None]
    h, w, c = frame.shape
    rows = frame.reshape(h, w * c).astype(np.int64)
    out = np.zeros((h, 1 + w * c), np.uint8)
    prev = np.zeros(w * c, np.int64)
    for y in range(h):
        cur = rows[y]
        a, ul = np.zeros_like(cur), np.zeros_like(cur)
        a[c:], ul[c:] = cur[:-c], prev[:-c]
        p = a + prev - ul
        pa, pb, pc = np.abs(p - a), np.abs(p - prev), np.abs(p - ul)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, prev, ul))
        cand = [(cur - pred) & 255 for pred in (0, a, prev, (a + prev) >> 1, paeth)]
        if filter == "adaptive":
            sums = [int(np.minimum(v, 256 - v).sum()) for v in cand]
            ft = sums.index(min(sums))
        else:
            ft = FILTERS.index(filter)
        out[y, 0] = ft
        out[y, 1:] = cand[ft]
        prev = cur
    return out


def tokens(piece):
    """[(byte, 0) for a literal | (0, length) for a match at distance 1]."""
    d = np.frombuffer(bytes(piece), np.uint8)
    starts = np.flatnonzero(np.concatenate([[True], d[1:] != d[:-1]]))
    ends = np.concatenate([starts[1:], [len(d)]])
    out = []
    for s, e in zip(starts.tolist(), ends.tolist()):
        v = int(d[s])
        out.append((v, 0))
        full, r = divmod(e - s - 1, 258)
        out.extend([(0, 258)] * full)
        if r >= 3:
            out.append((0, r))
        else:
            out.extend([(v, 0)] * r)
    return out


def length_symbol(n):
    """(symbol, extra bits, their value) of a match length."""
    k = max(i for i in range(29) if LEN_BASE[i] <= n)
    return 257 + k, LEN_EXTRA[k], n - LEN_BASE[k]


def huff_lengths(counts, limit):
    counts = [int(v) for v in counts]
    weight = {i: v for i, v in enumerate(counts) if v}
    for i in range(len(counts)):
        if len(weight) >= 2:
            break
        if i not in weight:
            weight[i] = 1
    order = sorted(weight, key=lambda i: (weight[i], i))
    # heap entries (weight, 0 symbol | 1 merged, rank, node); depth through parent links
    heap = [(weight[s], 0, k, k) for k, s in enumerate(order)]
    heapq.heapify(heap)
    parent, made = {}, len(order)
    while len(heap) > 1:
        x, y = heapq.heappop(heap), heapq.heappop(heap)
        parent[x[3]] = parent[y[3]] = made
        heapq.heappush(heap, (x[0] + y[0], 1, made, made))
        made += 1
    per = [0] * (len(order) + 2)
    for k in range(len(order)):
        depth, node = 0, k
        while node in parent:
            node, depth = parent[node], depth + 1
        per[depth] += 1
    for i in range(len(per) - 1, limit, -1):
        while per[i] > 0:
            j = i - 2
            while per[j] == 0:
                j -= 1
            per[i] -= 2
            per[i - 1] += 1
            per[j + 1] += 2
            per[j] -= 1
    lengths, k = [0] * len(counts), 0
    for L in range(min(limit, len(per) - 1), 0, -1):
        for _ in range(per[L]):
            lengths[order[k]] = L
            k += 1
    return lengths


def canonical_codes(lengths):
    """The codes as they enter an LSB-first stream: bit-reversed."""
    most = max(lengths)
    per = [0] * (most + 2)
    for v in lengths:
        if v:
            per[v] += 1
    nxt, code = [0] * (most + 2), 0
    for b in range(1, most + 1):
        code = (code + per[b - 1]) << 1
        nxt[b] = code
    out = []
    for v in lengths:
        if not v:
            out.append(0)
            continue
        out.append(int(format(nxt[v], "0%db" % v)[::-1], 2))
        nxt[v] += 1
    return out


def piece_tables(piece):
    """(tokens, literal/length counts, their lengths, the code-length code's lengths, HLIT, HCLEN)."""
    toks = tokens(piece)
    counts = [0] * 286
    counts[256] = 1
    for v, n in toks:
        counts[length_symbol(n)[0] if n else v] += 1
    ll = huff_lengths(counts, 15)
    hlit = max(257, 1 + max(i for i in range(286) if ll[i]))
    seq = ll[:hlit] + [1]
    clc = [0] * 19
    for v in seq:
        clc[v] += 1
    cl = huff_lengths(clc, 7)
    hclen = max(4, 1 + max(i for i in range(19) if cl[CL_ORDER[i]]))
    return toks, counts, ll, cl, hlit, hclen


def _pack(fields):
    """fields: [(value, bits)] -> bytes, LSB first, zero bits up to the byte boundary."""
    val = np.array([f[0] for f in fields], np.int64)
    nb = np.array([f[1] for f in fields], np.int64)
    pos = np.concatenate([[0], np.cumsum(nb)])
    bits = np.zeros((int(pos[-1]) + 7) // 8 * 8, np.uint8)
    for b in range(int(nb.max()) if len(nb) else 0):
        m = nb > b
        bits[pos[:-1][m] + b] = (val[m] >> b) & 1
    return np.packbits(bits, bitorder="little").tobytes()


def deflate_piece(piece):
    piece = bytes(piece)
    toks, counts, ll, cl, hlit, hclen = piece_tables(piece)
    lc, cc = canonical_codes(ll), canonical_codes(cl)
    f = [(0, 1), (2, 2), (hlit - 257, 5), (0, 5), (hclen - 4, 4)]
    f += [(cl[CL_ORDER[i]], 3) for i in range(hclen)]
    f += [(cc[v], cl[v]) for v in ll[:hlit] + [1]]
    for v, n in toks:
        if n:
            s, eb, ev = length_symbol(n)
            f += [(lc[s], ll[s]), (ev, eb), (0, 1)]
        else:
            f.append((lc[v], ll[v]))
    f += [(lc[256], ll[256]), (0, 3)]
    coded = _pack(f) + b"\x00\x00\xff\xff"
    if len(coded) < 5 + len(piece):
        return coded
    return b"\x00" + struct.pack("<HH", len(piece), len(piece) ^ 0xFFFF) + piece


def chunk(typ, data):
    return struct.pack(">I", len(data)) + typ + data + struct.pack(">I", zlib.crc32(typ + data) & 0xFFFFFFFF)


def adler32(data):
    a, b = 1, 0
    for i in range(0, len(data), 4096):   # plain sums; the modulus is taken often enough for exact integers anyway
        for v in data[i:i + 4096]:
            a += v
            b += a
        a %= 65521
        b %= 65521
    return b << 16 | a


def encode(frame, filter="adaptive"):
    frame = np.asarray(frame, np.uint8)
    if frame.ndim == 2:
        frame = frame[:, :, None]
    h, w, c = frame.shape
    raw = filter_rows(frame, filter).tobytes()
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, {1: 0, 3: 2, 4: 6}[c], 0, 0, 0))
    for at in range(0, len(raw), PIECE):
        out += chunk(b"IDAT", (b"\x78\x01" if at == 0 else b"") + deflate_piece(raw[at:at + PIECE]))
    out += chunk(b"IDAT", b"\x01\x00\x00\xff\xff" + struct.pack(">I", adler32(raw)))
    return out + chunk(b"IEND", b"")


def chunks(stream):
    """[(type, data, stored crc)] of a PNG stream."""
    assert stream[:8] == b"\x89PNG\r\n\x1a\n"
    at, out = 8, []
    while at < len(stream):
        n, = struct.unpack(">I", stream[at:at + 4])
        out.append((stream[at + 4:at + 8], stream[at + 8:at + 8 + n], struct.unpack(">I", stream[at + 8 + n:at + 12 + n])[0]))
        at += 12 + n
    assert at == len(stream)
    return out


def unfilter(raw, h, w, c):
    """The frame of (h, 1 + w * c) filtered rows (plain Python, for the graph test's Montage check)."""
    raw = np.frombuffer(bytes(raw), np.uint8).reshape(h, 1 + w * c)
    out = np.zeros((h, w * c), np.int64)
    prev = np.zeros(w * c, np.int64)
    for y in range(h):
        ft, x = int(raw[y, 0]), raw[y, 1:].astype(np.int64)
        cur = np.zeros(w * c, np.int64)
        if ft == 0:
            cur = x
        elif ft == 2:
            cur = (x + prev) & 255
        else:
            for i in range(w * c):
                a = cur[i - c] if i >= c else 0
                b, ul = prev[i], (prev[i - c] if i >= c else 0)
                if ft == 1:
                    pred = a
                elif ft == 3:
                    pred = (a + b) >> 1
                else:
                    p = a + b - ul
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - ul)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else ul)
                cur[i] = (x[i] + pred) & 255
        out[y] = cur
        prev = cur
    return out.astype(np.uint8).reshape(h, w, c)
