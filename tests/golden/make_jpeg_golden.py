"""Writes tests/golden/jpeg_golden.npz: baseline JPEG streams made by Pillow (libjpeg-turbo), what Pillow decodes them to, and
streams the ImageDecoder op must refuse.  Pillow decodes with libjpeg's defaults (JDCT_ISLOW, fancy upsampling, RGB), the
same call cv::imdecode makes, so its arrays stand for the reference op's frames.  Needs Pillow; run from the repository root:

    python tests/golden/make_jpeg_golden.py

Keys: "<case>__jpg" the stream (uint8), "<case>__img" the decoded (h, w, c) uint8 frame, "<case>__cfg" the encoder settings
(JSON), and for the refused streams "<case>__jpg", "<case>__status" (the st_status) and "<case>__cause" (a word of the message).
"cases", "refused" and "batch" list the case names (the last: 33 streams of one shape for the batch tests).
"""
import io
import json
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(1, 1), (3, 3), (2, 5), (8, 8), (17, 13), (5, 40), (40, 5), (16, 16), (33, 65), (37, 53)]   # (w, h)
SETTINGS = [("q75_444", dict(quality=75, subsampling="4:4:4")),
            ("q30_422", dict(quality=30, subsampling="4:2:2")),
            ("q95_420_opt", dict(quality=95, subsampling="4:2:0", optimize=True)),
            ("q100_420_rst3", dict(quality=100, subsampling="4:2:0", restart_marker_blocks=3)),
            ("q5_420", dict(quality=5, subsampling="4:2:0")),
            ("q90_422_rstrow", dict(quality=90, subsampling="4:2:2", restart_marker_rows=1))]
ST_ERR_INVALID, ST_ERR_UNSUPPORTED = 1, 4


def content(kind, w, h, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = rng.uniform(0, 6.28, 6)
    img = np.stack([127 + 120 * np.sin(x / 3.1 + ph[0]) * np.cos(y / 4.3 + ph[1]),
                    127 + 120 * np.sin((x + y) / 5.7 + ph[2]) * np.cos(y / 2.9 + ph[3]),
                    127 + 120 * np.cos(x / 7.3 + ph[4]) * np.sin((x - y) / 3.7 + ph[5])], axis=-1)
    return np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)


def encode(arr, **kw):
    img = Image.fromarray(arr if arr.ndim == 3 else arr, "RGB" if arr.ndim == 3 else "L")
    buf = io.BytesIO()
    img.save(buf, "JPEG", **kw)
    return buf.getvalue()


def decoded(jpg):
    a = np.asarray(Image.open(io.BytesIO(jpg)))
    return np.ascontiguousarray(a if a.ndim == 3 else a[..., None])


def main():
    out, cases, refused, batch = {}, [], [], []

    def add(name, jpg, cfg):
        out[name + "__jpg"] = np.frombuffer(jpg, np.uint8)
        out[name + "__img"] = decoded(jpg)
        out[name + "__cfg"] = np.array(json.dumps(cfg))
        cases.append(name)

    seed = 0
    for w, h in SIZES:
        for kind in ("noise", "smooth"):
            for sname, kw in SETTINGS:
                seed += 1
                add("%dx%d_%s_%s" % (w, h, kind, sname), encode(content(kind, w, h, seed), **kw), dict(kw, w=w, h=h, content=kind))
        seed += 1
        add("%dx%d_gray_q60" % (w, h), encode(content("smooth", w, h, seed)[..., 1], quality=60), dict(quality=60, w=w, h=h, content="gray"))
    # COM and APP1 (EXIF with an orientation tag, which a decoder at IMREAD_UNCHANGED does not apply)
    ex = Image.Exif()
    ex[0x0112] = 6
    ex[0x010E] = "jpeg golden"
    kw = dict(quality=80, subsampling="4:2:0", comment=b"written for the ImageDecoder tests", exif=ex.tobytes())
    add("24x18_com_app1", encode(content("smooth", 24, 18, 900), **kw), dict(quality=80, subsampling="4:2:0", w=24, h=18, content="smooth", segments="COM+APP1"))
    # larger frames: several workgroups, odd block counts
    add("136x248_420", encode(content("smooth", 136, 248, 901), quality=85, subsampling="4:2:0"), dict(quality=85, subsampling="4:2:0", w=136, h=248))
    add("200x328_422", encode(content("smooth", 200, 328, 902), quality=70, subsampling="4:2:2"), dict(quality=70, subsampling="4:2:2", w=200, h=328))
    add("131x77_420_rst5", encode(content("noise", 131, 77, 903), quality=60, subsampling="4:2:0", restart_marker_blocks=5),
        dict(quality=60, subsampling="4:2:0", restart_marker_blocks=5, w=131, h=77))
    # rows that are a multiple of 16 pixels: the kernels' 16-byte path, every sampling
    for sname, kw in (("444", dict(quality=85, subsampling="4:4:4")), ("422", dict(quality=85, subsampling="4:2:2")),
                      ("420", dict(quality=85, subsampling="4:2:0", restart_marker_rows=1))):
        add("48x24_vec_" + sname, encode(content("smooth", 48, 24, 910), **kw), dict(kw, w=48, h=24))
    add("48x24_vec_gray", encode(content("smooth", 48, 24, 911)[..., 0], quality=85), dict(quality=85, w=48, h=24, content="gray"))
    # one shape, different content: the batch tests
    for i in range(33):
        name = "32x24_batch%02d" % i
        add(name, encode(content("smooth" if i % 3 else "noise", 32, 24, 1000 + i), quality=40 + i, subsampling="4:2:0"),
            dict(quality=40 + i, subsampling="4:2:0", w=32, h=24))
        batch.append(name)
    add("32x24_batch_444", encode(content("smooth", 32, 24, 1100), quality=77, subsampling="4:4:4"), dict(quality=77, subsampling="4:4:4", w=32, h=24))

    def refuse(name, jpg, status, cause):
        out[name + "__jpg"] = np.frombuffer(jpg, np.uint8)
        out[name + "__status"] = np.array(status)
        out[name + "__cause"] = np.array(cause)
        refused.append(name)

    base = encode(content("smooth", 33, 65, 950), quality=75, subsampling="4:2:0")
    sos = base.index(b"\xff\xda")
    scan = sos + 2 + int.from_bytes(base[sos + 2:sos + 4], "big")
    refuse("progressive", encode(content("smooth", 33, 65, 951), quality=75, progressive=True), ST_ERR_UNSUPPORTED, "progressive")
    buf = io.BytesIO()
    Image.fromarray(content("smooth", 16, 16, 952)).convert("CMYK").save(buf, "JPEG", quality=75)
    refuse("cmyk", buf.getvalue(), ST_ERR_UNSUPPORTED, "4 components")
    refuse("truncated_scan", base[:scan + (len(base) - scan) // 2], ST_ERR_INVALID, "scan")
    refuse("sos_cut_short", base[:sos + 7], ST_ERR_INVALID, "SOS")
    refuse("random_bytes", np.random.default_rng(953).integers(0, 256, 64, dtype=np.uint8).tobytes(), ST_ERR_INVALID, "not a JPEG")
    refuse("empty", b"", ST_ERR_INVALID, "empty")

    out["cases"], out["refused"], out["batch"] = np.array(cases), np.array(refused), np.array(batch)
    path = os.path.join(HERE, "jpeg_golden.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d refused, %d bytes" % (path, len(cases), len(refused), os.path.getsize(path)))


if __name__ == "__main__":
    main()
