"""Writes tests/golden/jpeg_restart_golden.npz: baseline JPEG streams WITH restart intervals made by Pillow (libjpeg-turbo), what
Pillow decodes them to, and corrupt variants -- what the restart-interval entropy decoder (st_jpeg_decode_batch_gpu and its CPU
twin st_jpeg_coefficients_by_interval) is held to beyond the DRI cases of jpeg_golden.npz and jpeg_encode_golden.npz.
Needs Pillow; run from the repository root:

    python tests/golden/make_jpeg_restart_golden.py

Keys: "<case>__jpg" the stream (uint8), "<case>__img" the decoded (h, w, c) uint8 frame ("<case>__same_as": the case whose
frame it shares instead), "<case>__cfg" the settings (JSON).  "cases" lists the decodable cases, "good" four streams of one
shape, "mixed" two streams of one shape with different tables, "corrupt" the corrupt variants: "<name>__jpg", "<name>__of"
(the index into "good" of the stream it was cut from) and "<name>__interval" (the interval that lost the second half of its
bytes, markers kept).  Every case is checked here against tests/ref_jpeg_np.py: it decodes the good ones to Pillow's frame
and raises on the corrupt ones.
"""
import io
import json
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ref_jpeg_np  # noqa: E402
from make_jpeg_golden import content, decoded, encode  # noqa: E402


def scan_start(jpg):
    sos = jpg.index(b"\xff\xda")
    return sos + 2 + int.from_bytes(jpg[sos + 2:sos + 4], "big")


def markers(jpg):
    """Positions of the RSTn / EOI markers of the scan (the 0xFF byte)."""
    out, p = [], scan_start(jpg)
    while p + 1 < len(jpg):
        if jpg[p] == 0xFF and jpg[p + 1] not in (0x00, 0xFF):
            out.append(p)
            if jpg[p + 1] == 0xD9:
                break
            p += 2
        else:
            p += 1
    return out


def cut_interval(jpg, k):
    """The stream without the second half of interval k's bytes; every marker stays."""
    ends = markers(jpg)
    begin = scan_start(jpg) if k == 0 else ends[k - 1] + 2
    end = ends[k]
    return jpg[:begin + (end - begin) // 2] + jpg[end:]


def main():
    out, cases = {}, []

    def add(name, jpg, cfg, same_as=None):
        out[name + "__jpg"] = np.frombuffer(jpg, np.uint8)
        img = decoded(jpg)
        assert np.array_equal(ref_jpeg_np.decode(jpg), img), name
        if same_as is None:
            out[name + "__img"] = img
        else:
            assert np.array_equal(out[same_as + "__img"], img), name
            out[name + "__same_as"] = np.array(same_as)
        out[name + "__cfg"] = np.array(json.dumps(cfg))
        cases.append(name)
        return jpg

    tall = content("noise", 16, 1048, 2001)
    kw = dict(quality=90, subsampling="4:4:4", restart_marker_blocks=1)
    many = add("16x1048_444_rst1", encode(tall, **kw), dict(kw, w=16, h=1048, content="noise"))
    assert len(markers(many)) == 262          # 261 RSTn (the counter wraps 32 times) and EOI
    kw = dict(quality=90, subsampling="4:2:0", optimize=True, restart_marker_blocks=1)
    add("16x1048_420_opt_rst1", encode(tall, **kw), dict(kw, w=16, h=1048, content="noise"))
    kw = dict(quality=70, restart_marker_blocks=2)
    gray = add("40x24_gray_rst2", encode(content("smooth", 40, 24, 2002)[..., 1], **kw), dict(kw, w=40, h=24, content="gray"))
    assert b"\xff\xdd" in gray[:scan_start(gray)]
    kw = dict(quality=60, subsampling="4:2:0", restart_marker_blocks=5)
    span = add("131x61_420_rst5", encode(content("noise", 131, 61, 2003), **kw), dict(kw, w=131, h=61, content="noise"))
    assert len(markers(span)) == 8            # 9 MCUs per row, 36 MCUs: intervals span the rows, the last one holds 1 MCU
    kw = dict(quality=80, subsampling="4:2:2", restart_marker_rows=1)
    rows = add("16x1040_422_rstrow", encode(content("smooth", 16, 1040, 2004), **kw), dict(kw, w=16, h=1040, content="smooth"))
    ends = markers(rows)
    assert len(ends) == 130
    filled = bytearray(rows)
    for k, nfill in ((77, 3), (5, 1)):        # back to front, so that the positions hold
        filled[ends[k]:ends[k]] = b"\xff" * nfill
    add("16x1040_422_rstrow_fill", bytes(filled), dict(kw, w=16, h=1040, content="smooth", fill="1 byte before marker 5, 3 before marker 77"),
        same_as="16x1040_422_rstrow")

    mixed = []
    for name, kw, seed in (("32x24_mixed_std", dict(quality=80, subsampling="4:2:0", restart_marker_rows=1), 2010),
                           ("32x24_mixed_opt", dict(quality=50, subsampling="4:2:0", restart_marker_rows=1, optimize=True), 2011)):
        add(name, encode(content("noise", 32, 24, seed), **kw), dict(kw, w=32, h=24))
        mixed.append(name)

    good, corrupt = [], []
    for i, kind in enumerate(("noise", "smooth", "smooth", "noise")):
        kw = dict(quality=95, subsampling="4:2:0", restart_marker_blocks=1)
        name = "32x24_rst1_good%d" % i
        jpg = add(name, encode(content(kind, 32, 24, 2020 + i), **kw), dict(kw, w=32, h=24, content=kind))
        good.append(name)
        if i < 2:
            for k in (0, 2):
                bad = cut_interval(jpg, k)
                assert len(markers(bad)) == len(markers(jpg)) == 4
                try:
                    ref_jpeg_np.decode(bad)
                except ValueError:
                    pass
                else:
                    raise AssertionError("ref_jpeg_np decodes " + name + " cut in interval %d" % k)
                cname = "%s_cut%d" % (name, k)
                out[cname + "__jpg"] = np.frombuffer(bad, np.uint8)
                out[cname + "__of"] = np.array(i)
                out[cname + "__interval"] = np.array(k)
                corrupt.append(cname)

    out["cases"], out["good"], out["mixed"], out["corrupt"] = np.array(cases), np.array(good), np.array(mixed), np.array(corrupt)
    path = os.path.join(HERE, "jpeg_restart_golden.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d corrupt, %d bytes" % (path, len(cases), len(corrupt), os.path.getsize(path)))
    for name in cases:
        print("  %-28s %6d bytes" % (name, out[name + "__jpg"].size))


if __name__ == "__main__":
    main()
