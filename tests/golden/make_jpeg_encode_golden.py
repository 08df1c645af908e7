"""Writes tests/golden/jpeg_encode_golden.npz: pictures and the baseline JPEG streams Pillow (libjpeg-turbo) makes of them
with one restart interval per MCU row, which is what the ImageEncoder op must reproduce byte for byte.  Needs Pillow; run
from the repository root:

    python tests/golden/make_jpeg_encode_golden.py

Keys: "img_<h>x<w>_<content>" a picture, (h, w, 3) uint8; per case "<case>__jpg" Pillow's stream for
save(quality=q, subsampling=s, restart_marker_rows=1) and "<case>__cfg" JSON {h, w, content, quality, subsampling, img}
(img: the picture's key).  "cases" lists the case names, "batch" the 33 cases of one shape; a batch case also has
"<case>__dec", Pillow's decode of its own stream.

The shapes are the smallest at which each rule of the stream can go wrong: 1x1 and 8x8; 7x17 / 17x7 / 65x33 / 33x65 (edge
columns and rows, padding blocks to the right and below); 34x40 / 40x34 (rows replicated before against after the
downsampling); 24x9 / 9x24; 80x24 and 152x16 (ten intervals: RST7 wraps to RST0); 9x200 and 8x360 (more than 64 and more
than 128 blocks per interval).  Every shape is written at all three samplings.  Noise gives long codes, stuffed 0xFF bytes
and ZRL; one flat colour gives EOB only and DC difference 0; a 0 / 255 checker the extreme magnitudes (categories 11 and 10
at quality 100); a ramp short codes.
"""
import io
import json
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(1, 1), (8, 8), (7, 17), (17, 7), (65, 33), (33, 65), (34, 40), (40, 34), (24, 9), (9, 24), (80, 24), (152, 16)]   # (h, w)
ALL_QUALITIES = {(8, 8), (17, 7), (34, 40)}   # noise at every quality and all four contents; elsewhere two qualities in rotation
SUBSAMPLINGS = ["4:4:4", "4:2:2", "4:2:0"]
QUALITIES = [1, 50, 95, 100]


def content(kind, h, w, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "flat":
        return np.broadcast_to(np.array([200, 30, 90], np.uint8), (h, w, 3)).copy()
    y, x = np.mgrid[0:h, 0:w]
    if kind == "checker":
        return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
    assert kind == "ramp"
    return np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(h + w - 2, 1)], axis=-1).astype(np.uint8)


def encode(arr, quality, subsampling):
    buf = io.BytesIO()
    Image.fromarray(arr, "RGB").save(buf, "JPEG", quality=quality, subsampling=subsampling, restart_marker_rows=1)
    return buf.getvalue()


def main():
    out, cases, batch = {}, [], []

    def picture(kind, h, w, seed):
        key = "img_%dx%d_%s" % (h, w, kind)
        if key not in out:
            out[key] = content(kind, h, w, seed)
        return key

    def add(name, key, quality, subsampling, kind):
        arr = out[key]
        out[name + "__jpg"] = np.frombuffer(encode(arr, quality, subsampling), np.uint8)
        out[name + "__cfg"] = np.array(json.dumps(dict(h=arr.shape[0], w=arr.shape[1], content=kind, quality=quality, subsampling=subsampling, img=key)))
        cases.append(name)

    turn = 0
    for si, (h, w) in enumerate(SHAPES):
        for sub in SUBSAMPLINGS:
            tag = sub.replace(":", "")
            if (h, w) in ALL_QUALITIES:
                plan = [("noise", q) for q in QUALITIES] + [("flat", 95), ("checker", 100), ("checker", 1), ("ramp", 50)]
            else:
                plan = [("noise", QUALITIES[turn % 4]), ("noise", QUALITIES[(turn + 2) % 4])]
                turn += 1
            for kind, q in plan:
                add("%dx%d_%s_q%d_%s" % (h, w, kind, q, tag), picture(kind, h, w, 100 + si), q, sub, kind)
    # more than 64 blocks per interval, so that the entropy kernel carries bits from one pass of its wave to the next: 9x200 has
    # 75, 52 and 78 blocks at 4:4:4, 4:2:2 and 4:2:0 (two passes, one, two), 8x360 has 135, 92 and 138 (three, two, three)
    for si, ((h, w), plan) in enumerate((((9, 200), [("4:4:4", 95, "noise"), ("4:2:2", 100, "noise"), ("4:2:0", 1, "noise"), ("4:2:0", 95, "noise"),
                                                      ("4:2:0", 95, "flat")]),
                                         ((8, 360), [("4:4:4", 100, "noise"), ("4:2:2", 50, "noise"), ("4:2:0", 95, "noise")]))):
        for sub, q, kind in plan:
            add("%dx%d_%s_q%d_%s" % (h, w, kind, q, sub.replace(":", "")), picture(kind, h, w, 200 + si), q, sub, kind)
    # one shape, 33 different pictures: the batch tests and the graph round trip
    for i in range(33):
        key = "img_24x32_noise%02d" % i
        out[key] = content("noise", 24, 32, 1000 + i)
        name = "24x32_batch%02d" % i
        add(name, key, 95, "4:2:0", "noise")
        out[name + "__dec"] = np.asarray(Image.open(io.BytesIO(out[name + "__jpg"].tobytes())))
        batch.append(name)
    out["cases"], out["batch"] = np.array(cases), np.array(batch)
    path = os.path.join(HERE, "jpeg_encode_golden.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d bytes" % (path, len(cases), os.path.getsize(path)))


if __name__ == "__main__":
    main()
