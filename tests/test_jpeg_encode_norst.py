"""CPU: ImageEncoder's restart = NONE (streams without DRI and RSTn) on the host side: the restatement of libjpeg's scan
without restart intervals (tests/ref_jpeg_encode_norst_np.py) against the streams Pillow wrote at its defaults
(tests/golden/jpeg_encode_norst_golden.npz), what that fixture must contain, the 623-byte header, the refusals of a bad restart
mode at every layer, and the argument message's field 3."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import ref_jpeg_encode_norst_np as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD_PATH = os.path.join(ROOT, "tests", "golden", "jpeg_encode_norst_golden.npz")
GOLD = np.load(GOLD_PATH)
CASES = [str(c) for c in GOLD["cases"]]
BATCH = [str(c) for c in GOLD["batch"]]
SAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
ST_ERR_INVALID, ST_ERR_UNSUPPORTED = 1, 4
ROW, NONE = 0, 1


def _cfg(name):
    return json.loads(str(GOLD[name + "__cfg"]))


def _jpg(name):
    return GOLD[name + "__jpg"].tobytes()


@pytest.fixture(scope="module")
def restated():
    """Per case (header, MCU rows as (bits, length)): the library's header and the restatement's entropy coder over the
    restatement's coefficients.  Computed once, never changed."""
    from scannertools_amd.hip import jpeg_encode_header, jpeg_quant_tables
    out = {}
    for name in CASES:
        c = _cfg(name)
        hs, vs = SAMPLING[c["subsampling"]]
        header = jpeg_encode_header(c["h"], c["w"], c["quality"], c["subsampling"], restart="none")
        coef = ref.coefficients(GOLD[c["img"]], *jpeg_quant_tables(c["quality"]), hs, vs)
        out[name] = (header, coef, ref.row_bits(coef, c["h"], c["w"], hs, vs, header))
    return out


def test_restatement_equals_the_golden_streams(restated):
    """The 623-byte header from the library, the scan from scan_norst: the whole stream, byte for byte; and no stream has a DRI
    segment or a restart marker."""
    from scannertools_amd.hip import probe_jpeg
    for name in CASES:
        c, jpg = _cfg(name), _jpg(name)
        header, coef, _ = restated[name]
        hs, vs = SAMPLING[c["subsampling"]]
        scan, offs = ref.scan_norst(coef, c["h"], c["w"], hs, vs, header)
        assert len(header) == 623 and header + scan == jpg, name
        assert len(offs) == -(-c["h"] // (8 * vs)) + 1 and offs[0] == 0
        assert len(ref.unstuffed(jpg)) == -(-offs[-1] // 8), name
        info = probe_jpeg(jpg)
        assert (info["h"], info["w"], info["channels"], info["h_samp"], info["v_samp"]) == (c["h"], c["w"], 3, hs, vs)
        assert info["restart_interval"] == 0 and not re.search(rb"\xff[\xd0-\xd7]", jpg[623:]), name


def test_golden_file_holds_the_cases_the_mode_is_held_to(restated):
    """The shapes, and the coverage conditions the generator asserted when it wrote the file, found again in the file."""
    assert len(BATCH) == 33 and os.path.getsize(GOLD_PATH) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "jpeg_encode_golden.npz"))
    cfgs = [_cfg(c) for c in CASES]
    shapes = {(c["h"], c["w"]) for c in cfgs}
    common = {(1, 1), (8, 8), (7, 17), (17, 7), (65, 33), (33, 65), (34, 40), (40, 34), (24, 9), (9, 24), (80, 24), (152, 16)}
    assert common | {(9, 200), (8, 360), (120, 8), (200, 3), (200, 8), (400, 8), (160, 16), (24, 32)} == shapes
    for shape in common | {(120, 8), (200, 3)}:
        for sub in SAMPLING:
            assert len([c for c in cfgs if (c["h"], c["w"]) == shape and c["subsampling"] == sub]) >= (2 if shape in common else 1), (shape, sub)
    assert all(c["content"] == "flat" for c in cfgs if (c["h"], c["w"]) in ((120, 8), (200, 3)))
    assert all((c["quality"], c["subsampling"], c["content"]) == (100, "4:4:4", "noise") for c in cfgs if (c["h"], c["w"]) in ((200, 8), (400, 8)))
    assert {c["subsampling"] for c in cfgs if (c["h"], c["w"]) == (160, 16)} == {"4:2:2", "4:2:0"}
    assert all((c["quality"], c["subsampling"]) == (95, "4:2:0") for c in (_cfg(n) for n in BATCH))
    blocks = {-(-c["w"] // (8 * SAMPLING[c["subsampling"]][0])) * (SAMPLING[c["subsampling"]][0] * SAMPLING[c["subsampling"]][1] + 2) for c in cfgs}
    assert {75, 78, 92, 135, 138} <= blocks   # rows of more than 64 and more than 128 blocks: several passes of the entropy wave

    ff_across, ff_last, aligned, padded, row_bits, residues = 0, 0, 0, 0, set(), set()
    for name in CASES:
        rows = restated[name][2]
        offs = [sum(n for _, n in rows[:r]) for r in range(len(rows) + 1)]
        raw = ref.unstuffed(_jpg(name))
        ff_across += any(o % 8 and raw[o // 8] == 0xFF for o in offs[1:-1])   # a 0xFF byte holding bits of two MCU rows
        if offs[-1] % 8:
            padded += 1
            ff_last += raw[-1] == 0xFF
            assert _jpg(name).endswith(b"\xff\x00\xff\xd9") == (raw[-1] == 0xFF), name
        else:
            aligned += 1
        row_bits |= {n for _, n in rows}
        residues |= {o % 8 for o in offs[1:-1]}
    assert ff_across >= 8 and ff_last >= 4 and aligned >= 8 and padded >= 8, (ff_across, ff_last, aligned, padded)
    assert {14, 20, 32} <= row_bits and min(row_bits) == 14, sorted(row_bits)[:5]   # 14 bits: no row is shorter, see below
    assert set(range(1, 8)) <= residues, residues


def _owned_bytes(rows):
    """The unstuffed scan by the rule the kernels follow: row r, at bit B of the scan and L bits long, owns
    the bytes whose first bit lies in it; an owned byte is 8 bits of the row from bit 8 j + sh on (sh = -B mod 8), the last one
    completed with the leading bits of the NEXT row alone, or with 1-bits after the last row."""
    out, B = bytearray(), 0
    for r, (value, L) in enumerate(rows):
        slot = (value << (-L % 8)).to_bytes(-(-L // 8), "big")   # the row's bits, the last byte zero-filled
        tail = rows[r + 1][0] >> (rows[r + 1][1] - 8) if r + 1 < len(rows) else 0xFF
        first, sh = -(-B // 8), -B % 8
        for j in range(-(-(B + L) // 8) - first):
            v = slot[j]
            if sh:
                v = ((v << sh) | (slot[j + 1] >> (8 - sh) if j + 1 < len(slot) else 0)) & 0xFF
            end = 8 * j + sh + 8
            if end > L:
                v |= tail >> (8 - (end - L))
            out.append(v)
        B += L
    return bytes(out)


def test_ownership_rule_gives_the_golden_scans(restated):
    """One next row is enough because no row is shorter than 14 bits (three blocks at least, a DC code of 2 bits or more and
    an EOB of 2 or 4 each): the rule as the kernels apply it, in Python, against every golden scan."""
    from scannertools_amd.hip import jpeg_encode_header
    tabs = ref.huffman_tables(jpeg_encode_header(8, 8, 50, "4:4:4", restart="none"))
    shortest = {c: min(n for _, n in tabs[(0, c)].values()) + tabs[(1, c)][0][1] for c in (0, 1)}   # DC code + EOB
    assert shortest == {0: 6, 1: 4} and shortest[0] + 2 * shortest[1] == 14
    for name in CASES:
        rows = restated[name][2]
        assert all(n >= 14 for _, n in rows), name
        assert _owned_bytes(rows) == ref.unstuffed(_jpg(name)), name


def test_header_entry_point():
    from scannertools_amd import _native
    from scannertools_amd.hip import jpeg_encode_header
    L = _native.lib()
    buf, size = ctypes.create_string_buffer(1024), ctypes.c_size_t()
    seen = set()
    for name in CASES:
        c, jpg = _cfg(name), _jpg(name)
        key = (c["h"], c["w"], c["quality"], c["subsampling"])
        if key in seen:
            continue
        seen.add(key)
        hs, vs = SAMPLING[c["subsampling"]]
        assert L.st_jpeg_encode_header_rst(c["h"], c["w"], c["quality"], hs, vs, NONE, buf, 1024, ctypes.byref(size)) == 0 and size.value == 623
        none = buf.raw[:623]
        assert none == jpg[:623] and jpg[621:623] == b"\x3f\x00" and b"\xff\xdd" not in none, name
        assert none == jpeg_encode_header(c["h"], c["w"], c["quality"], c["subsampling"], restart="none")
        # ROW: the existing entry point's bytes, and NONE is those without the six bytes of the DRI segment
        assert L.st_jpeg_encode_header_rst(c["h"], c["w"], c["quality"], hs, vs, ROW, buf, 1024, ctypes.byref(size)) == 0 and size.value == 629
        row = buf.raw[:629]
        assert L.st_jpeg_encode_header(c["h"], c["w"], c["quality"], hs, vs, buf, 1024, ctypes.byref(size)) == 0 and size.value == 629
        assert row == buf.raw[:629] == jpeg_encode_header(c["h"], c["w"], c["quality"], c["subsampling"]) == jpeg_encode_header(
            c["h"], c["w"], c["quality"], c["subsampling"], restart="row")
        dri = row.index(b"\xff\xdd")
        assert row[:dri] + row[dri + 6:] == none
    assert len(seen) > 60
    # too small a buffer: the size is reported, nothing is written
    small = ctypes.create_string_buffer(b"\x55" * 622, 622)
    assert L.st_jpeg_encode_header_rst(8, 8, 50, 2, 2, NONE, small, 622, ctypes.byref(size)) == ST_ERR_INVALID and size.value == 623
    assert small.raw == b"\x55" * 622


def test_a_bad_restart_mode_is_refused_at_every_layer():
    from scannertools_amd import _native, _proto
    from scannertools_amd.hip import HipContext, jpeg_encode_header, jpeg_restart
    L = _native.lib()
    for name in ("st_jpeg_encode_header_rst", "st_jpeg_encode_batch_rst"):
        assert name in _native.SIGNATURES and hasattr(ctypes.CDLL(_native.LIB_PATH), name), name
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scannertools_hip.h")).read(), flags=re.S)
    assert re.search(r"ST_JPEG_RESTART_ROW = 0, ST_JPEG_RESTART_NONE = 1", header)
    assert re.search(r"\bst_jpeg_encode_header_rst\s*\(", header) and re.search(r"\bst_jpeg_encode_batch_rst\s*\(", header)
    buf, size = ctypes.create_string_buffer(b"\x55" * 1024, 1024), ctypes.c_size_t(7)
    for bad in (2, -1, 3, 1 << 20):
        assert L.st_jpeg_encode_header_rst(8, 8, 50, 2, 2, bad, buf, 1024, ctypes.byref(size)) == ST_ERR_INVALID
        assert buf.raw == b"\x55" * 1024 and size.value == 7
        # a null context is still refused first
        assert L.st_jpeg_encode_batch_rst(None, None, 1, 8, 8, 50, 2, 2, bad) == ST_ERR_INVALID
    assert L.st_jpeg_encode_batch_rst(None, None, 1, 8, 8, 50, 2, 2, NONE) == ST_ERR_INVALID
    # the other checks are those of the existing entry point
    assert L.st_jpeg_encode_header_rst(8, 8, 101, 2, 2, NONE, buf, 1024, ctypes.byref(size)) == ST_ERR_INVALID
    assert L.st_jpeg_encode_header_rst(8, 8, 50, 1, 2, NONE, buf, 1024, ctypes.byref(size)) == ST_ERR_UNSUPPORTED
    assert L.st_jpeg_encode_header_rst(0, 8, 50, 2, 2, NONE, buf, 1024, ctypes.byref(size)) == ST_ERR_INVALID
    assert jpeg_restart("row") == ROW and jpeg_restart("none") == NONE
    for bad in ("NONE", "mcu_row", "", None, 1, "off"):
        with pytest.raises(ValueError, match=re.escape("restart %r is not supported" % (bad,))):
            jpeg_encode_header(8, 8, 50, "4:2:0", restart=bad)
        with pytest.raises(ValueError, match=re.escape("restart %r is not supported" % (bad,))):
            HipContext.encode_jpeg(None, [], 50, "4:2:0", restart=bad)   # refused before the context is touched
    with pytest.raises(ValueError, match="restart must be one of"):
        _proto.image_encoder_args(95, "4:2:0", "rows")


def test_argument_message_field_3():
    from scannertools_amd import _proto
    # the default is not written: today's serialisations stay byte-identical
    assert _proto.image_encoder_args() == _proto.image_encoder_args(0, "", 0) == _proto.image_encoder_args(0, "", "mcu_row") == b""
    assert _proto.image_encoder_args(95, "4:2:0") == _proto.image_encoder_args(95, "4:2:0", 0) == b"\x08\x5f\x12\x054:2:0"
    assert _proto.image_encoder_args(95, "4:2:0", 1) == _proto.image_encoder_args(95, "4:2:0", "none") == b"\x08\x5f\x12\x054:2:0\x18\x01"
    assert _proto.image_encoder_args(restart="NONE") == b"\x18\x01"
    assert _proto.parse_image_encoder_args(b"\x18\x01") == {"restart": "NONE"}
    assert _proto.parse_image_encoder_args(b"\x18\x00") == {"restart": "MCU_ROW"}
    assert _proto.parse_image_encoder_args(b"\x08\x5f\x12\x054:2:0") == {"quality": 95, "subsampling": "4:2:0"}
    for q, s, r in ((1, "4:4:4", 1), (100, "", 7), (0, "4:2:2", -2)):
        want = {k: v for k, v in (("quality", q), ("subsampling", s), ("restart", {1: "NONE"}.get(r, r))) if v}
        assert _proto.parse_image_encoder_args(_proto.image_encoder_args(q, s, r)) == want
    proto = open(os.path.join(ROOT, "scannertools_amd", "scanner_kernels", "scannertools_imgproc_amd.proto")).read()
    assert re.search(r"enum Restart \{\s*MCU_ROW = 0;\s*NONE = 1;\s*\}\s*int32 quality = 1;\s*string subsampling = 2;\s*Restart restart = 3;", proto)


def _run_op(sc, mk):
    from scannertools_amd.engine import NamedStream, PerfParams
    return sc.run(sc.io.Output(mk(), [NamedStream(sc, "o")]), PerfParams.estimate())


def test_validate_refuses_a_bad_restart_without_a_gpu_context():
    from scannertools_amd import _proto
    from scannertools_amd.engine import Client, DeviceType, NamedVideoStream, _CppMultiOpNode
    sc = Client()
    sc.ingest_frames("v", np.zeros((2, 8, 8, 3), np.uint8))
    frame = sc.io.Input([NamedVideoStream(sc, "v")])
    for dev in (DeviceType.CPU, DeviceType.GPU):
        for bad in (2, 7, -1):
            with pytest.raises(RuntimeError, match=re.escape("ImageEncoder: restart %d is not supported (MCU_ROW or NONE)" % bad)):
                _run_op(sc, lambda: sc.ops.ImageEncoder(frame=frame, device=dev, restart=bad))
            with pytest.raises(RuntimeError, match=re.escape("ImageEncoder: restart %d is not supported (MCU_ROW or NONE)" % bad)):
                _run_op(sc, lambda: _CppMultiOpNode(sc, "ImageEncoder", [frame], dev, None, _proto.image_encoder_args(50, "4:4:4", bad)))
        # the other checks still come first and still name their cause
        with pytest.raises(RuntimeError, match=re.escape("quality 101 is outside 1..100")):
            _run_op(sc, lambda: sc.ops.ImageEncoder(frame=frame, device=dev, quality=101, restart="none"))
    with pytest.raises(ValueError, match="restart must be one of"):
        sc.ops.ImageEncoder(frame=frame, restart="sometimes")
    import torch
    if not torch.cuda.is_available():   # valid arguments without a GPU: a loud failure, no fallback
        for restart in ("none", "row", "mcu_row", 1):
            with pytest.raises(RuntimeError, match="st_ctx_create"):
                _run_op(sc, lambda: sc.ops.ImageEncoder(frame=frame, restart=restart))


def test_registration_is_unchanged():
    from scannertools_amd import _native, engine
    regs = [r for r in engine.registered_kernels() if r[0] == "ImageEncoder"]
    assert sorted(dev for _, dev, _, _ in regs) == [0, 1]
    assert all(kind == 1 and can_batch for _, _, kind, can_batch in regs)
    info = engine.op_info("ImageEncoder")
    assert info["input_names"] == ["frame"] and info["output_names"] == ["img"] and not info["frame_output"]
    assert info["inputs"] == 1 and info["outputs"] == 1 and info["stencil"] == [0] and not info["unbounded_state"]
    assert _native.K_COUNT == 19 and _native.lib().st_abi_version() == 1   # no new timing slot, no new ABI version


SANITIZER_MAIN = r'''
// st_jpeg_enc_host.cpp under -fsanitize=address,undefined: st_jpeg_encode_header_rst and the argument checks over the golden
// configurations, every buffer on the heap at exactly the size the call is told, so that a byte too many is caught.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "scannertools_hip.h"
#include "st_jpeg_enc_host.h"

int main(int argc, char** argv) {
  long calls = 0, configs = 0;
  for (int i = 1; i + 5 < argc; i += 6, ++configs) {
    const int h = atoi(argv[i]), w = atoi(argv[i + 1]), q = atoi(argv[i + 2]), hs = atoi(argv[i + 3]), vs = atoi(argv[i + 4]);
    std::vector<unsigned char> want(623);
    FILE* f = fopen(argv[i + 5], "rb");
    if (!f || fread(want.data(), 1, 623, f) != 623) { printf("cannot read %s\n", argv[i + 5]); return 2; }
    fclose(f);
    size_t size = 0;
    unsigned char* none = (unsigned char*)malloc(623);
    unsigned char* row = (unsigned char*)malloc(629);
    unsigned char* old = (unsigned char*)malloc(629);
    if (st_jpeg_encode_header_rst(h, w, q, hs, vs, ST_JPEG_RESTART_NONE, none, 623, &size) != ST_OK || size != 623 || memcmp(none, want.data(), 623)) {
      printf("config %ld: the header without DRI differs\n", configs); return 3;
    }
    if (st_jpeg_encode_header_rst(h, w, q, hs, vs, ST_JPEG_RESTART_ROW, row, 629, &size) != ST_OK || size != 629 ||
        st_jpeg_encode_header(h, w, q, hs, vs, old, 629, &size) != ST_OK || size != 629 || memcmp(row, old, 629)) {
      printf("config %ld: the header with DRI differs from st_jpeg_encode_header's\n", configs); return 4;
    }
    // a byte too few: refused, the size reported
    if (st_jpeg_encode_header_rst(h, w, q, hs, vs, ST_JPEG_RESTART_NONE, none, 622, &size) != ST_ERR_INVALID || size != 623) return 5;
    if (st_jpeg_encode_header_rst(h, w, q, hs, vs, ST_JPEG_RESTART_ROW, none, 623, &size) != ST_ERR_INVALID || size != 629) return 6;
    if (st_jpeg_encode_header_rst(h, w, q, hs, vs, ST_JPEG_RESTART_NONE, nullptr, 0, nullptr) != ST_ERR_INVALID) return 7;
    for (int bad : {2, -1, 3, 1 << 30, -2147483647 - 1}) {
      size = 7;
      if (st_jpeg_encode_header_rst(h, w, q, hs, vs, bad, none, 623, &size) != ST_ERR_INVALID || size != 7) return 8;
      for (size_t len : {(size_t)1, (size_t)8, (size_t)160}) {   // the message is cut to the room it is given
        char* msg = (char*)malloc(len);
        if (st_jpeg_enc_check_restart(bad, msg, len) != ST_ERR_INVALID || strlen(msg) >= len) return 9;
        free(msg);
        ++calls;
      }
      ++calls;
    }
    char msg[160];
    if (st_jpeg_enc_check_restart(ST_JPEG_RESTART_ROW, msg, sizeof msg) != ST_OK || st_jpeg_enc_check_restart(ST_JPEG_RESTART_NONE, msg, sizeof msg) != ST_OK || msg[0]) return 10;
    if (st_jpeg_encode_bound(h, w, hs, vs) < 623 + 2) return 11;
    StJpegEncGeom g;
    st_jpeg_enc_geom(h, w, hs, vs, &g);
    // a row's unstuffed bits fit its slot, and the slot is no more than half the stuffed one (+ the rounding to 16)
    const size_t bits = (size_t)g.mcols * g.bpm * kJpegEncBlockBits;
    if ((bits + 7) / 8 > st_jpeg_enc_raw_slot_bytes(g) || 2 * st_jpeg_enc_raw_slot_bytes(g) > st_jpeg_enc_slot_bytes(g) + 32) return 12;
    calls += 8;
    free(none); free(row); free(old);
  }
  if (configs < 60) { printf("only %ld configurations\n", configs); return 13; }
  printf("sanitized run ok: %ld configurations, %ld calls\n", configs, calls);
  return 0;
}
'''


def test_host_code_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program (its own main, nothing preloaded, no Python inside): st_jpeg_enc_host.cpp built with
    -fsanitize=address,undefined, st_jpeg_encode_header_rst and the argument checks run over every golden configuration."""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    (tmp_path / "main.cpp").write_text(SANITIZER_MAIN)
    exe = tmp_path / "jpeg_enc_host_asan"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "scannertools_amd", "csrc"), str(tmp_path / "main.cpp"),
           os.path.join(ROOT, "scannertools_amd", "csrc", "st_jpeg_enc_host.cpp"), "-o", str(exe)]
    # the runtimes linked into the program where their archives exist, so that nothing depends on the order of loaded libraries
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr) and "error:" not in build.stderr:
        pytest.skip("no sanitizer runtime: " + build.stderr[-300:])
    assert build.returncode == 0, build.stderr[-4000:]
    args, seen = [], set()
    for name in CASES:
        c = _cfg(name)
        key = (c["h"], c["w"], c["quality"]) + SAMPLING[c["subsampling"]]
        if key not in seen:
            seen.add(key)
            (tmp_path / (name + ".hdr")).write_bytes(_jpg(name)[:623])
            args += [str(v) for v in key] + [str(tmp_path / (name + ".hdr"))]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    p = subprocess.run([str(exe)] + args, capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0 and "sanitized run ok: %d configurations" % len(seen) in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr, p.stderr[-4000:]
    print(p.stdout.strip())
