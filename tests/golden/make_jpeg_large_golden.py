"""Writes tests/golden/jpeg_large_golden.npz: what Pillow (libjpeg-turbo) makes of pictures at the frame sizes where the JPEG
kernels' launch geometry changes -- more than 256 MCU rows, rows of 65 500 pixels, more than 2 097 152 pixels at an odd width,
more than 65 536 restart intervals, more than 1024 segments, 1080 x 1920.  Needs Pillow; run from the repository root:

    python tests/golden/make_jpeg_large_golden.py

The pictures are NOT stored: tests/jpeg_large_cases.py rebuilds each from (kind, h, w, seed), and lists the cases.  Per case:
"<case>__cfg" JSON {role, h, w, channels, kind, seed, quality, subsampling, restart, uses, store, img_sha256}; Pillow's stream as
"<case>__jpg" (uint8) where it has at most 350 000 bytes and the case asks for it ("store": the 1080 x 1920 streams do not, the
file has a cap of its own), else "<case>__jpg_sha256" and "<case>__jpg_len"; for a case of role "decode" also
"<case>__dec_sha256", the SHA-256 of the bytes of the frame Pillow decodes its stream to.  "cases" lists the names.

Every stream is checked here against the restatements the tests lean on (tests/ref_jpeg_encode_np.py,
ref_jpeg_encode_norst_np.py, ref_jpeg_np.py), and again from the file by tests/test_jpeg_large.py, which also asserts the
thresholds each case is here to cross.  The file may not outgrow 1 000 000 bytes.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_large_cases as lc   # noqa: E402
import ref_jpeg_encode_norst_np as ref_norst   # noqa: E402
import ref_jpeg_encode_np as ref_row   # noqa: E402
import ref_jpeg_np   # noqa: E402
from make_jpeg_encode_norst_golden import quant_tables   # noqa: E402
from make_jpeg_golden import decoded, encode   # noqa: E402

LIMIT = 1000 * 1000


def restated(arr, c, jpg):
    """The stream of an "encode" case by the restatement, with the header and the tables of Pillow's stream."""
    hs, vs = lc.SAMPLING[c["subsampling"]]
    sos = jpg.index(b"\xff\xda")
    header = jpg[:sos + 2 + int.from_bytes(jpg[sos + 2:sos + 4], "big")]
    q = quant_tables(header)
    coef = ref_row.coefficients(arr, q[0], q[1], hs, vs)
    if c["restart"] == "none":
        return header + ref_norst.scan_norst(coef, c["h"], c["w"], hs, vs, header)[0]
    return header + ref_row.scan(coef, c["h"], c["w"], hs, vs, header)


def main():
    out, names = {}, []
    for c in lc.CASES:
        name = lc.case_name(c)
        assert name not in names, name
        arr = lc.picture(c["kind"], c["h"], c["w"], c["seed"], c["channels"])
        jpg = encode(arr if c["channels"] == 3 else arr[..., 0], **lc.pillow_settings(c))
        if c["role"] == "encode":
            assert restated(arr, c, jpg) == jpg, name
        else:
            frame = decoded(jpg)
            assert frame.shape == arr.shape and np.array_equal(ref_jpeg_np.decode(jpg), frame), name
            out[name + "__dec_sha256"] = np.array(lc.sha256(frame.tobytes()))
        if lc.stored(c, len(jpg)):
            out[name + "__jpg"] = np.frombuffer(jpg, np.uint8)
        else:
            out[name + "__jpg_sha256"], out[name + "__jpg_len"] = np.array(lc.sha256(jpg)), np.array(len(jpg))
        out[name + "__cfg"] = np.array(json.dumps(dict(c, img_sha256=lc.sha256(arr.tobytes()))))
        names.append(name)
        print("  %-44s %8d bytes%s" % (name, len(jpg), "" if lc.stored(c, len(jpg)) else "  (hash only)"))
    out["cases"] = np.array(names)
    path = os.path.join(HERE, "jpeg_large_golden.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("%s: %d cases, %d bytes" % (path, len(names), size))
    assert size <= LIMIT, (size, LIMIT)


if __name__ == "__main__":
    main()
