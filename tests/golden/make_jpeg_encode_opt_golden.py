"""Writes tests/golden/jpeg_encode_opt_golden.npz: what Pillow (libjpeg-turbo) writes with optimize=True for the cases of
tests/jpeg_encode_opt_cases.py, which is what the ImageEncoder op must reproduce byte for byte with optimize = 1.  Needs Pillow;
run from the repository root:

    python tests/golden/make_jpeg_encode_opt_golden.py

Keys: "cases" the case names; per case "<case>__cfg" JSON {the case's fields, img_sha: SHA-256 of the picture's bytes, jpg_len,
jpg_sha}; "<case>__jpg" the stream where it has at most STORED_STREAM_LIMIT bytes; "<case>__dec" Pillow's decode of the stream
and "<case>__plain" Pillow's stream without optimize for the cases used by "batch".  The pictures are rebuilt from their seeds (jpeg_encode_opt_cases.picture).

Every stream is first reproduced by the restatement (tests/ref_jpeg_encode_opt_np.py) from the picture, and the coverage
conditions of coverage() are asserted before the file is written; tests/test_jpeg_encode_opt.py finds them again in the file.
"""
import io
import json
import os
import sys

import numpy as np
from PIL import Image, ImageFile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ref_jpeg_encode_opt_np as ref   # noqa: E402
from jpeg_encode_opt_cases import CASES, SAMPLING, STORED_STREAM_LIMIT, case_name, picture, pillow_settings, sha256   # noqa: E402

ImageFile.MAXBLOCK = 1 << 24   # optimize=True saves of incompressible pictures need the room


def encode(arr, c):
    buf = io.BytesIO()
    Image.fromarray(arr, "RGB").save(buf, "JPEG", **pillow_settings(c))
    return buf.getvalue()


def split(jpg):
    """(header SOI .. SOS, the rest)"""
    sos = jpg.index(b"\xff\xda")
    end = sos + 2 + int.from_bytes(jpg[sos + 2:sos + 4], "big")
    return jpg[:end], jpg[end:]


def quant_tables(header):
    out, i = {}, 2
    while i < len(header):
        marker, length = header[i + 1], int.from_bytes(header[i + 2:i + 4], "big")
        if marker == 0xDB:
            q = np.zeros(64, np.uint16)
            q[ref.ZIGZAG] = np.frombuffer(header[i + 5:i + 69], np.uint8)
            out[header[i + 4] & 15] = q
        i += 2 + length
    return out


def ownership(rows):
    """Of the MCU rows (value, bits) of a scan without restart markers: (rows that own no byte, bytes holding bits of three rows
    or more, whether the padding bits lie in a byte whose first bit belongs to an earlier row than the last)."""
    starts, B = [], 0
    for _, n in rows:
        starts.append(B)
        B += n
    total = B
    owner = lambda bit: max(r for r, s in enumerate(starts) if s <= bit)   # noqa: E731
    no_byte = sum(1 for s, (_, n) in zip(starts, rows) if -(-(s + n) // 8) == -(-s // 8))
    three = sum(1 for k in range(-(-total // 8)) if owner(min(8 * k + 7, total - 1)) - owner(8 * k) >= 2)
    early_pad = total % 8 != 0 and owner(total // 8 * 8) < len(rows) - 1
    return no_byte, three, early_pad


def properties(c, arr, jpg):
    """Asserts that the restatement writes Pillow's stream; returns what the coverage conditions are stated on."""
    hs, vs = SAMPLING[c["subsampling"]]
    h, w = arr.shape[:2]
    fixed, _ = split(jpg)
    q = quant_tables(fixed)
    coef = ref.coefficients(arr, q[0], q[1], hs, vs)
    rst = ref.ROW if c["restart"] == "row" else ref.NONE
    got, hlen, freq = ref.encode(coef, h, w, hs, vs, rst, fixed)
    assert got == jpg, case_name(c)
    p = dict(longest=max(max(ref.code_sizes(f)) for f in freq), single=sum(int((f > 0).sum() == 1) for f in freq), row_bits=set(), no_byte=0,
             three=0, early_pad=False, none=rst == ref.NONE)
    if rst == ref.NONE:
        rows = ref.row_bits(coef, h, w, hs, vs, got[:hlen])
        p["row_bits"] = {n for _, n in rows}
        p["no_byte"], p["three"], p["early_pad"] = ownership(rows)
    return p


def coverage(props):
    props = list(props)
    none = [p for p in props if p["none"]]
    return dict(long_codes=sum(p["longest"] > 16 for p in props), single_symbol=sum(p["single"] for p in props),
                six_bit_streams=sum(6 in p["row_bits"] for p in none), no_byte=sum(p["no_byte"] for p in none), three=sum(p["three"] for p in none),
                early_pad=sum(p["early_pad"] for p in none), eight=sum(8 in p["row_bits"] for p in none), twelve=sum(12 in p["row_bits"] for p in none),
                longest=max(p["longest"] for p in props))


def check_coverage(cov):
    assert cov["long_codes"] >= 2 and cov["single_symbol"] >= 1 and cov["six_bit_streams"] >= 4, cov
    assert cov["no_byte"] >= 1 and cov["three"] >= 1 and cov["early_pad"] >= 1 and cov["eight"] >= 1 and cov["twelve"] >= 1, cov


def main():
    out, names, props = {}, [], []
    for c in CASES:
        name = case_name(c)
        assert name not in names, name
        arr = picture(c["kind"], c["h"], c["w"], c["seed"])
        jpg = encode(arr, c)
        props.append(properties(c, arr, jpg))
        out[name + "__cfg"] = np.array(json.dumps(dict(c, img_sha=sha256(arr.tobytes()), jpg_len=len(jpg), jpg_sha=sha256(jpg))))
        if len(jpg) <= STORED_STREAM_LIMIT:
            out[name + "__jpg"] = np.frombuffer(jpg, np.uint8)
        if "batch" in c["uses"]:
            out[name + "__dec"] = np.asarray(Image.open(io.BytesIO(jpg)))
            buf = io.BytesIO()   # and the stream without optimize, for the calls that alternate between the two settings
            Image.fromarray(arr, "RGB").save(buf, "JPEG", **dict(pillow_settings(c), optimize=False))
            out[name + "__plain"] = np.frombuffer(buf.getvalue(), np.uint8)
        names.append(name)
    cov = coverage(props)
    check_coverage(cov)
    out["cases"] = np.array(names)
    path = os.path.join(HERE, "jpeg_encode_opt_golden.npz")
    np.savez_compressed(path, **out)
    size, limit = os.path.getsize(path), os.path.getsize(os.path.join(HERE, "jpeg_encode_golden.npz"))
    assert size <= limit, (size, limit)
    print("%s: %d cases, %d bytes; %s" % (path, len(names), size, cov))


if __name__ == "__main__":
    main()
