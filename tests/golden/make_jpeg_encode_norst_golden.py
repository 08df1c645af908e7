"""Writes tests/golden/jpeg_encode_norst_golden.npz: pictures and the baseline JPEG streams Pillow (libjpeg-turbo) makes of them
at its defaults -- no DRI segment, no RSTn markers --, which is what the ImageEncoder op must reproduce byte for byte with
restart = NONE.  Needs Pillow; run from the repository root:

    python tests/golden/make_jpeg_encode_norst_golden.py

The keys are those of jpeg_encode_golden.npz: "img_<h>x<w>_<content>" a picture, (h, w, 3) uint8; per case "<case>__jpg"
Pillow's stream for save(quality=q, subsampling=s) and "<case>__cfg" JSON {h, w, content, quality, subsampling, img}; "cases"
lists the case names, "batch" the 33 cases of one shape; a batch case also has "<case>__dec", Pillow's decode of its stream.

What is new without markers is where the MCU rows meet: a row starts at any bit, a byte (also a 0xFF byte) can hold bits of two
rows, the DC predictors carry over, the scan is padded and stuffed once.  The shapes are the smallest at which each of these
can go wrong: the 12 shapes of make_jpeg_encode_golden.py at all three samplings, two qualities each (the transform is not
what is new); 9x200 and 8x360 (more than 64 and 128 blocks per row); 120x8 and 200x3 in one flat colour (rows of 14 / 20 / 32
bits after the first at 4:4:4 / 4:2:2 / 4:2:0: the shortest there are, two rows meeting inside most bytes, every phase of the
bit offset); 200x8 and 400x8 noise at quality 100, 4:4:4 (25 and 50 rows of three long blocks: 0xFF bytes made of two rows'
bits, a padded last byte that is 0xFF), the seeds walked from 0 upward and kept where they add such a case; 160x16 noise at
4:2:2 and 4:2:0; 33 pictures of 24x32.  COVERAGE below is asserted before the file is written, and again from the file by
tests/test_jpeg_encode_norst.py.
"""
import io
import json
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ref_jpeg_encode_norst_np as ref   # noqa: E402
from make_jpeg_encode_golden import SHAPES, SUBSAMPLINGS, content   # noqa: E402

SAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
# at least this many cases: a 0xFF byte of the unstuffed scan with bits of two MCU rows; a padded last byte that is 0xFF; a scan
# that ends byte-aligned; one that does not.  And: a case with a 14-, a 20- and a 32-bit row; an unaligned row start at every
# residue 1 .. 7 of the bit offset mod 8.
COVERAGE = dict(ff_across_rows=8, ff_last_padded=4, aligned_end=8, padded_end=8)
SEED_LIMIT = 64   # the walk over seeds is bounded
# The two qualities of a (shape, sampling) of the 12 common shapes: a high one at one sampling per shape, that sampling and the
# pair in rotation, (1, 50) at the other two.  Noise at 95 and 100 is most of the file, which may not outgrow
# jpeg_encode_golden.npz; what these shapes are here for -- edge and padding blocks whose DC differences now run on from row to
# row -- does not depend on the quality, and long codes are what the 200x8 / 400x8, 9x200 and 8x360 cases are for.
HIGH_PAIRS = [(1, 95), (50, 100)]


def encode(arr, quality, subsampling):
    buf = io.BytesIO()
    Image.fromarray(arr, "RGB").save(buf, "JPEG", quality=quality, subsampling=subsampling)
    return buf.getvalue()


def quant_tables(header):
    """The DQT segments' tables in natural order, by table id."""
    out, i = {}, 2
    while i < len(header):
        marker, length = header[i + 1], int.from_bytes(header[i + 2:i + 4], "big")
        if marker == 0xDB:
            q = np.zeros(64, np.uint16)
            q[ref.ZIGZAG] = np.frombuffer(header[i + 5:i + 69], np.uint8)
            out[header[i + 4] & 15] = q
        i += 2 + length
    return out


def properties(arr, jpg, subsampling):
    """What the coverage conditions ask of one case, from the restatement's bit offsets: {ff_across_rows, ff_last_padded,
    aligned_end, row_bits: set, residues: set}.  Asserts on the way that the restatement writes Pillow's stream."""
    hs, vs = SAMPLING[subsampling]
    h, w = arr.shape[:2]
    sos = jpg.index(b"\xff\xda")
    header = jpg[:sos + 2 + int.from_bytes(jpg[sos + 2:sos + 4], "big")]
    assert len(header) == 623 and b"\xff\xdd" not in header
    q = quant_tables(header)
    scan, offs = ref.scan_norst(ref.coefficients(arr, q[0], q[1], hs, vs), h, w, hs, vs, header)
    assert header + scan == jpg
    raw, total = ref.unstuffed(jpg), offs[-1]
    starts = offs[1:-1]   # where a row meets the one above
    across = sum(1 for o in starts if o % 8 and raw[o // 8] == 0xFF)
    return dict(ff_across_rows=across > 0, ff_last_padded=total % 8 != 0 and raw[-1] == 0xFF, aligned_end=total % 8 == 0,
                row_bits={b - a for a, b in zip(offs[:-1], offs[1:])}, residues={o % 8 for o in starts})


def coverage(props):
    """The counts and sets the conditions are stated on, over all cases."""
    props = list(props)
    return dict(ff_across_rows=sum(p["ff_across_rows"] for p in props), ff_last_padded=sum(p["ff_last_padded"] for p in props),
                aligned_end=sum(p["aligned_end"] for p in props), padded_end=sum(not p["aligned_end"] for p in props),
                row_bits=set().union(*(p["row_bits"] for p in props)), residues=set().union(*(p["residues"] for p in props)))


def check_coverage(cov):
    for key, least in COVERAGE.items():
        assert cov[key] >= least, (key, cov[key], least)
    assert {14, 20, 32} <= cov["row_bits"], sorted(cov["row_bits"])[:8]
    assert set(range(1, 8)) <= cov["residues"], cov["residues"]


def main():
    out, cases, batch, props = {}, [], [], []

    def picture(kind, h, w, seed, key=None):
        key = key or "img_%dx%d_%s" % (h, w, kind)
        if key not in out:
            out[key] = content(kind, h, w, seed)
        return key

    def add(name, key, quality, subsampling, kind):
        arr = out[key]
        jpg = encode(arr, quality, subsampling)
        out[name + "__jpg"] = np.frombuffer(jpg, np.uint8)
        out[name + "__cfg"] = np.array(json.dumps(dict(h=arr.shape[0], w=arr.shape[1], content=kind, quality=quality, subsampling=subsampling, img=key)))
        cases.append(name)
        props.append(properties(arr, jpg, subsampling))

    for si, (h, w) in enumerate(SHAPES):
        for ji, sub in enumerate(SUBSAMPLINGS):
            for q in (HIGH_PAIRS[si // 3 % 2] if ji == si % 3 else (1, 50)):
                add("%dx%d_noise_q%d_%s" % (h, w, q, sub.replace(":", "")), picture("noise", h, w, 100 + si), q, sub, "noise")
    # more than 64 / 128 blocks per row, so that the entropy kernel's wave carries bits from one pass to the next: 9x200 has 75 and
    # 78 blocks at 4:4:4 and 4:2:0 (two passes; the 52 at 4:2:2 are one), 8x360 has 135, 92 and 138 (three, two, three)
    for si, ((h, w), plan) in enumerate((((9, 200), [("4:4:4", 95, "noise"), ("4:2:0", 1, "noise"), ("4:2:0", 95, "flat")]),
                                         ((8, 360), [("4:4:4", 50, "noise"), ("4:2:2", 50, "noise"), ("4:2:0", 50, "noise")]))):
        for sub, q, kind in plan:
            add("%dx%d_%s_q%d_%s" % (h, w, kind, q, sub.replace(":", "")), picture(kind, h, w, 200 + si), q, sub, kind)
    # the shortest rows there are
    for h, w in ((120, 8), (200, 3)):
        for sub in SUBSAMPLINGS:
            add("%dx%d_flat_q95_%s" % (h, w, sub.replace(":", "")), picture("flat", h, w, 0), 95, sub, "flat")
    for sub in ("4:2:2", "4:2:0"):
        add("160x16_noise_q95_%s" % sub.replace(":", ""), picture("noise", 160, 16, 300), 95, sub, "noise")
    # 33 pictures of one shape: the batch tests and the graph round trips
    for i in range(33):
        key = picture("noise", 24, 32, 1000 + i, "img_24x32_noise%02d" % i)
        name = "24x32_batch%02d" % i
        add(name, key, 95, "4:2:0", "noise")
        out[name + "__dec"] = np.asarray(Image.open(io.BytesIO(out[name + "__jpg"].tobytes())))
        batch.append(name)
    # many rows of long codes: seeds from 0 upward, the two shapes in turn, a seed kept while it adds a case of a kind still short;
    # of 400x8, which costs the file twice as much, the first such seed only
    kept_400 = 0
    for seed in range(SEED_LIMIT):
        cov = coverage(props)
        if all(cov[k] >= COVERAGE[k] for k in ("ff_across_rows", "ff_last_padded")):
            break
        for h, w in ((200, 8), (400, 8)):
            if h == 400 and kept_400 == 1:
                continue
            arr = content("noise", h, w, seed)
            p = properties(arr, encode(arr, 100, "4:4:4"), "4:4:4")
            cov = coverage(props)
            if any(p[k] and cov[k] < COVERAGE[k] for k in ("ff_across_rows", "ff_last_padded")):
                kept_400 += h == 400
                add("%dx%d_noise%02d_q100_444" % (h, w, seed), picture("noise", h, w, seed, "img_%dx%d_noise%02d" % (h, w, seed)), 100, "4:4:4", "noise")
    cov = coverage(props)
    check_coverage(cov)
    out["cases"], out["batch"] = np.array(cases), np.array(batch)
    path = os.path.join(HERE, "jpeg_encode_norst_golden.npz")
    np.savez_compressed(path, **out)
    size, limit = os.path.getsize(path), os.path.getsize(os.path.join(HERE, "jpeg_encode_golden.npz"))
    assert size <= limit, (size, limit)
    print("%s: %d cases, %d bytes; %s" % (path, len(cases), size, {k: (sorted(v)[:6] if isinstance(v, set) else v) for k, v in cov.items()}))


if __name__ == "__main__":
    main()
