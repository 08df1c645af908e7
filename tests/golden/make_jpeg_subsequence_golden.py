"""Writes tests/golden/jpeg_subsequence_golden.npz: baseline JPEG streams made by Pillow (libjpeg-turbo) for the decoding by
subsequence (st_jpeg_decode_batch_gpu_split and its CPU twin st_jpeg_coefficients_by_subsequence), what Pillow decodes them to,
and corrupt variants.  Most have NO restart intervals: the whole scan is one segment, cut into fixed-size subsequences.
Needs Pillow; run from the repository root:

    python tests/golden/make_jpeg_subsequence_golden.py

Keys: "<case>__jpg" the stream (uint8), "<case>__img" the decoded (h, w, c) uint8 frame, "<case>__cfg" the settings (JSON).
"cases" lists the decodable cases; "good" four streams of one shape without DRI; "corrupt" two variants "<name>__jpg" with
"<name>__of" (the index into "good" of the stream it was cut from): every marker is there, a stretch of the scan's bytes is
not.  Every case is checked here against tests/ref_jpeg_np.py: it decodes the good ones to Pillow's frame and raises on the
corrupt ones.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ref_jpeg_np  # noqa: E402
from make_jpeg_golden import content, decoded, encode  # noqa: E402
from make_jpeg_restart_golden import markers, scan_start  # noqa: E402


def cut_scan(jpg, lo, hi):
    """The stream without the bytes from fraction lo to fraction hi of its scan; every marker stays."""
    begin, end = scan_start(jpg), markers(jpg)[-1]
    a, b = begin + int((end - begin) * lo), begin + int((end - begin) * hi)
    while jpg[a - 1] == 0xFF:       # no cut between an FF and its 00
        a += 1
    while jpg[b - 1] == 0xFF:
        b += 1
    return jpg[:a] + jpg[b:]


def main():
    out, cases = {}, []

    def add(name, jpg, cfg, dri):
        out[name + "__jpg"] = np.frombuffer(jpg, np.uint8)
        img = decoded(jpg)
        assert np.array_equal(ref_jpeg_np.decode(jpg), img), name
        assert (b"\xff\xdd\x00\x04" in jpg[:scan_start(jpg)]) == dri, name
        out[name + "__img"] = img
        out[name + "__cfg"] = np.array(json.dumps(cfg))
        cases.append(name)
        return jpg

    # noise at 4:2:0, odd width and height, no DRI: several workgroups of 64 subsequences of 128 bytes, many FF 00 pairs
    kw = dict(quality=90, subsampling="4:2:0")
    big = add("203x213_noise_420", encode(content("noise", 203, 213, 3001), **kw), dict(kw, w=203, h=213, content="noise"), False)
    assert 40000 <= len(big) <= 60000 and big.count(b"\xff\x00", scan_start(big)) > 50, (len(big), big.count(b"\xff\x00"))
    kw = dict(quality=85)
    add("61x45_gray", encode(content("smooth", 61, 45, 3002)[..., 0], **kw), dict(kw, w=61, h=45, content="gray"), False)
    kw = dict(quality=75, subsampling="4:2:0", optimize=True)
    add("97x75_420_opt", encode(content("smooth", 97, 75, 3003), **kw), dict(kw, w=97, h=75, content="smooth"), False)
    # with DRI, the intervals spanning several subsequences
    for name, sub, seed in (("264x40_422_rstrow4", "4:2:2", 3004), ("232x40_444_rstrow4", "4:4:4", 3005)):
        w, h = (int(v) for v in name.split("_")[0].split("x"))
        kw = dict(quality=80, subsampling=sub, restart_marker_rows=4)
        jpg = add(name, encode(content("smooth", w, h, seed), **kw), dict(kw, w=w, h=h, content="smooth"), True)
        ends = markers(jpg)
        assert len(ends) >= 2 and ends[0] - scan_start(jpg) > 4 * 128, (name, len(ends), ends[0] - scan_start(jpg))

    good, corrupt = [], []
    for i, kind in enumerate(("noise", "smooth", "smooth", "noise")):
        kw = dict(quality=95, subsampling="4:2:0")
        name = "32x24_good%d" % i
        jpg = add(name, encode(content(kind, 32, 24, 3020 + i), **kw), dict(kw, w=32, h=24, content=kind), False)
        good.append(name)
        if i < 2:
            bad = cut_scan(jpg, 0.25, 0.5)
            assert len(markers(bad)) == len(markers(jpg)) == 1 and len(bad) < len(jpg)
            try:
                ref_jpeg_np.decode(bad)
            except (ValueError, IndexError, KeyError):
                pass
            else:
                raise AssertionError("ref_jpeg_np decodes " + name + " with a quarter of its scan gone")
            cname = name + "_cut"
            out[cname + "__jpg"] = np.frombuffer(bad, np.uint8)
            out[cname + "__of"] = np.array(i)
            corrupt.append(cname)

    out["cases"], out["good"], out["corrupt"] = np.array(cases), np.array(good), np.array(corrupt)
    path = os.path.join(HERE, "jpeg_subsequence_golden.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 300 * 1000
    print("%s: %d cases, %d corrupt, %d bytes" % (path, len(cases), len(corrupt), os.path.getsize(path)))
    for name in cases:
        print("  %-28s %6d bytes" % (name, out[name + "__jpg"].size))


if __name__ == "__main__":
    main()
