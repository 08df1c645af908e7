"""CPU: the restart-interval entropy decoder's host side -- st_jpeg_restart_intervals (the interval scan) and
st_jpeg_coefficients_by_interval (the CPU twin of k_jpeg_entropy_dec: the same bounded core, st_jpeg_entropy.h) -- against
st_jpeg_coefficients and the numpy definition (tests/ref_jpeg_np.py) on every golden stream that has a DRI segment, the status
classes of streams it must refuse, the ImageDecoderArgs.entropy field, and the core under AddressSanitizer + UBSan in a
stand-alone program."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import ref_jpeg_np as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
GOLD = np.load(os.path.join(GOLDEN, "jpeg_golden.npz"))
ENC = np.load(os.path.join(GOLDEN, "jpeg_encode_golden.npz"))
RST = np.load(os.path.join(GOLDEN, "jpeg_restart_golden.npz"))
ST_OK, ST_ERR_INVALID, ST_ERR_UNSUPPORTED = 0, 1, 4


def _scan_start(jpg):
    sos = jpg.index(b"\xff\xda")
    return sos + 2 + int.from_bytes(jpg[sos + 2:sos + 4], "big")


def _dri(jpg):
    """The restart interval the stream's DRI segment declares before its scan; 0: none."""
    at = jpg.find(b"\xff\xdd\x00\x04", 0, _scan_start(jpg))
    return int.from_bytes(jpg[at + 4:at + 6], "big") if at >= 0 else 0


def _streams_with_dri():
    """{name: stream} of every stream of the three golden files that has restart intervals."""
    out = {}
    for tag, G, names in (("golden", GOLD, [str(c) for c in GOLD["cases"]]), ("restart", RST, [str(c) for c in RST["cases"]]),
                          ("encode", ENC, [k[:-5] for k in ENC.files if k.endswith("__jpg")])):
        for n in names:
            jpg = G[n + "__jpg"].tobytes()
            if _dri(jpg) > 0:
                out[tag + ":" + n] = jpg
    return out


DRI = _streams_with_dri()


@pytest.fixture(scope="module")
def L():
    from scannertools_amd import _native
    return _native.lib()


def _info():
    from scannertools_amd import _native
    return _native.JpegInfo()


def _intervals(L, data):
    """(status, message, (n, 2) table) of st_jpeg_restart_intervals, the table sized by the call's own count."""
    info, count = _info(), ctypes.c_size_t(0)
    st = L.st_jpeg_restart_intervals(data, len(data), None, 0, ctypes.byref(count), ctypes.byref(info))
    if st != ST_OK:
        return st, info.message.decode(), None
    table = np.zeros((count.value, 2), np.uint32)
    st = L.st_jpeg_restart_intervals(data, len(data), table.ctypes.data, count.value, ctypes.byref(count), ctypes.byref(info))
    return st, info.message.decode(), table


def _coef(fn, data):
    info = _info()
    coef = np.full(1 << 18, 12345, np.int16)
    quant = np.zeros((3, 64), np.uint16)
    st = fn(data, len(data), coef.ctypes.data, coef.size, quant.ctypes.data, ctypes.byref(info))
    return st, info.message.decode(), coef, quant, info


def test_golden_files_hold_the_restart_cases():
    kinds = {n.split(":")[0] for n in DRI}
    assert kinds == {"golden", "restart", "encode"}
    assert sum(n.startswith("golden:") for n in DRI) == 42 and sum(n.startswith("encode:") for n in DRI) == 167
    assert len(RST["cases"]) == 12 and len(RST["corrupt"]) == 4 and len(RST["good"]) == 4 and len(RST["mixed"]) == 2
    assert os.path.getsize(os.path.join(GOLDEN, "jpeg_restart_golden.npz")) < 300 * 1000
    for n in RST["cases"]:
        assert _dri(RST[str(n) + "__jpg"].tobytes()) > 0, n                       # Pillow writes DRI for the one-component case too
    assert len(RST["16x1048_444_rst1__jpg"]) > 32000                              # "a 33 KB stream"
    mixed = [RST[str(n) + "__jpg"].tobytes() for n in RST["mixed"]]
    dht = [b"".join(s[i:i + 2 + int.from_bytes(s[i + 2:i + 4], "big")] for i in range(len(s) - 1) if s[i:i + 2] == b"\xff\xc4" and i < _scan_start(s))
           for s in mixed]
    assert dht[0] != dht[1]                                                       # one shape, different tables


def test_restart_intervals_of_every_golden_stream(L):
    from scannertools_amd import hip
    for name, jpg in DRI.items():
        info = hip.probe_jpeg(jpg)
        H, V = info["h_samp"], info["v_samp"]
        mcus = -(-info["w"] // (8 * H)) * -(-info["h"] // (8 * V))
        st, msg, t = _intervals(L, jpg)
        assert st == ST_OK and msg == "", (name, st, msg)
        assert len(t) == -(-mcus // info["restart_interval"]), name
        assert np.array_equal(t, hip.jpeg_restart_intervals(jpg)), name
        assert t[0, 0] == _scan_start(jpg), name
        for k in range(len(t)):
            b, e = int(t[k, 0]), int(t[k, 1])
            assert b <= e, (name, k)
            if k:                                                                  # every begin follows the marker before it
                assert b == int(t[k - 1, 1]) + 2 and jpg[b - 2] == 0xFF and jpg[b - 1] == 0xD0 + ((k - 1) & 7), (name, k)
            assert jpg[e] == 0xFF and jpg[e + 1] not in (0x00, 0xFF), (name, k)   # every end sits on a marker
        assert jpg[int(t[-1, 1]) + 1] == 0xD9, name
    # fill bytes in front of RSTn belong to the interval they follow; the marker is found behind them
    _, _, plain = _intervals(L, RST["16x1040_422_rstrow__jpg"].tobytes())
    filled_jpg = RST["16x1040_422_rstrow_fill__jpg"].tobytes()
    _, _, filled = _intervals(L, filled_jpg)
    grow = (filled[:, 1].astype(int) - filled[:, 0]) - (plain[:, 1].astype(int) - plain[:, 0])
    assert grow[5] == 1 and grow[77] == 3 and grow.sum() == 4
    assert filled_jpg[int(filled[77, 1]) - 3:int(filled[77, 1]) + 1] == b"\xff\xff\xff\xff"


@pytest.fixture(scope="module")
def definition():
    """ref_jpeg_np.coefficients of every stream with DRI, computed once."""
    return {name: ref.coefficients(jpg) for name, jpg in DRI.items()}


def test_by_interval_equals_the_host_decoder_and_the_definition(L, definition):
    for name, jpg in DRI.items():
        st, msg, coef, quant, info = _coef(L.st_jpeg_coefficients_by_interval, jpg)
        assert st == ST_OK and msg == "", (name, st, msg)
        st2, _, coef2, quant2, _ = _coef(L.st_jpeg_coefficients, jpg)
        assert st2 == ST_OK and np.array_equal(coef, coef2) and np.array_equal(quant, quant2), name
        want, wq = definition[name]
        assert np.array_equal(coef[:want.size], want) and (coef[want.size:] == 12345).all(), name
        assert np.array_equal(quant[:len(wq)], wq), name
        assert info.restart_interval == _dri(jpg), name


def test_front_end_by_interval(L):
    from scannertools_amd import hip
    jpg = RST["131x61_420_rst5__jpg"].tobytes()
    a, qa = hip.jpeg_coefficients(jpg)
    b, qb = hip.jpeg_coefficients(jpg, by_interval=True)
    assert np.array_equal(a, b) and np.array_equal(qa, qb)
    with pytest.raises(hip.StError, match="no restart intervals"):
        hip.jpeg_coefficients(GOLD["32x24_batch00__jpg"].tobytes(), by_interval=True)
    with pytest.raises(hip.StError, match="no restart intervals"):
        hip.jpeg_restart_intervals(GOLD["32x24_batch00__jpg"].tobytes())


def _wrong_by_every_reading(L, bad, what):
    st, msg, _, _, _ = _coef(L.st_jpeg_coefficients, bad)
    assert st == ST_ERR_INVALID and msg, (what, st, msg)
    with pytest.raises((ValueError, IndexError, KeyError)):
        ref.decode(bad)


def test_status_classes(L):
    # no DRI: unsupported, by name
    without = [str(c) for c in GOLD["cases"] if _dri(GOLD[str(c) + "__jpg"].tobytes()) == 0]
    assert len(without) > 90
    for name in without:
        jpg = GOLD[name + "__jpg"].tobytes()
        st, msg, _ = _intervals(L, jpg)
        assert st == ST_ERR_UNSUPPORTED and "no restart intervals" in msg, (name, st, msg)
        st, msg, coef, _, _ = _coef(L.st_jpeg_coefficients_by_interval, jpg)
        assert st == ST_ERR_UNSUPPORTED and "no restart intervals" in msg and (coef == 12345).all(), (name, st, msg)
    # what st_jpeg_probe refuses is refused the same way
    for name in GOLD["refused"]:
        jpg = GOLD[str(name) + "__jpg"].tobytes()
        # (truncated_scan has sound markers and no DRI: it is refused for that before its scan is looked at)
        want = ST_ERR_UNSUPPORTED if str(name) == "truncated_scan" else int(GOLD[str(name) + "__status"])
        assert _intervals(L, jpg)[0] == want == _coef(L.st_jpeg_coefficients_by_interval, jpg)[0], name
    # truncations inside the scan
    for name in ("golden:33x65_noise_q90_422_rstrow", "golden:37x53_smooth_q100_420_rst3", "restart:131x61_420_rst5", "restart:40x24_gray_rst2",
                 "encode:" + [k[:-5] for k in ENC.files if k.endswith("__jpg")][-1]):
        jpg = DRI[name]
        scan = _scan_start(jpg)
        for frac in (0.0, 0.1, 0.5, 0.9):
            bad = jpg[:scan + int((len(jpg) - scan) * frac)]
            st, msg, _, _, _ = _coef(L.st_jpeg_coefficients_by_interval, bad)
            assert st == ST_ERR_INVALID and ("scan" in msg), (name, frac, st, msg)
            _wrong_by_every_reading(L, bad, (name, frac))
        st, msg, _ = _intervals(L, jpg[:scan + (len(jpg) - scan) // 2])
        assert st == ST_ERR_INVALID and "truncated or corrupt scan" in msg, (name, st, msg)
    # a wrong RSTn
    for name in ("golden:33x65_smooth_q90_422_rstrow", "restart:16x1048_444_rst1"):
        jpg = DRI[name]
        _, _, t = _intervals(L, jpg)
        for k in (0, len(t) // 2):
            e = int(t[k, 1])
            bad = jpg[:e + 1] + bytes([0xD0 + ((k + 3) & 7)]) + jpg[e + 2:]
            st, msg, _ = _intervals(L, bad)
            assert st == ST_ERR_INVALID and "no RST%d marker" % (k & 7) in msg, (name, k, st, msg)
            st, msg, _, _, _ = _coef(L.st_jpeg_coefficients_by_interval, bad)
            assert st == ST_ERR_INVALID and "no RST%d marker" % (k & 7) in msg, (name, k, st, msg)
            _wrong_by_every_reading(L, bad, (name, k))
    # the stored corrupt variants: the markers are all there, one interval's data is not
    for name in RST["corrupt"]:
        bad, k = RST[str(name) + "__jpg"].tobytes(), int(RST[str(name) + "__interval"])
        st, msg, t = _intervals(L, bad)
        assert st == ST_OK and len(t) == 4, (name, st, msg)
        st, msg, _, _, _ = _coef(L.st_jpeg_coefficients_by_interval, bad)
        assert st == ST_ERR_INVALID and "restart interval %d of 4" % k in msg, (name, st, msg)
        _wrong_by_every_reading(L, bad, name)
    # the same cut on three streams of jpeg_golden.npz
    for name in ("33x65_noise_q90_422_rstrow", "33x65_smooth_q90_422_rstrow", "37x53_noise_q100_420_rst3"):
        jpg = GOLD[name + "__jpg"].tobytes()
        _, _, t = _intervals(L, jpg)
        for k in (0, 2):
            b, e = int(t[k, 0]), int(t[k, 1])
            bad = jpg[:b + (e - b) // 2] + jpg[e:]
            st, msg, _, _, _ = _coef(L.st_jpeg_coefficients_by_interval, bad)
            assert st == ST_ERR_INVALID and "restart interval %d of" % k in msg, (name, k, st, msg)
            _wrong_by_every_reading(L, bad, (name, k))
    # arguments
    jpg = DRI["restart:40x24_gray_rst2"]
    info, count = _info(), ctypes.c_size_t(0)
    table = np.zeros((3, 2), np.uint32)
    assert L.st_jpeg_restart_intervals(jpg, len(jpg), table.ctypes.data, 3, ctypes.byref(count), ctypes.byref(info)) == ST_ERR_INVALID
    assert count.value == 8 and b"8 restart intervals" in info.message and not table.any()
    coef = np.full(64, 12345, np.int16)
    assert L.st_jpeg_coefficients_by_interval(jpg, len(jpg), coef.ctypes.data, 63, None, None) == ST_ERR_INVALID and (coef == 12345).all()


def test_image_decoder_args_entropy_field():
    from scannertools_amd import _proto
    assert _proto.image_decoder_args(None, None) == b""
    assert _proto.image_decoder_args(entropy="gpu") == b"\x10\x01" == _proto.encode([(2, "int32", 1)])     # as protoc writes it
    assert _proto.image_decoder_args(entropy="auto") == b"\x10\x02" and _proto.image_decoder_args(entropy="host") == b"\x10\x00"
    assert _proto.image_decoder_args("JPEG", "GPU") == b"\x08\x01\x10\x01"
    assert _proto.parse_image_decoder_args(b"\x08\x01") == {"image_type": "JPEG"}        # an absent field stays absent: HOST
    for mode in ("HOST", "GPU", "AUTO"):
        assert _proto.parse_image_decoder_args(_proto.image_decoder_args(entropy=mode.lower())) == {"entropy": mode}
    assert _proto.parse_image_decoder_args(_proto.image_decoder_args("JPEG", 9)) == {"image_type": "JPEG", "entropy": 9}
    with pytest.raises(ValueError, match="entropy"):
        _proto.image_decoder_args(entropy="device")
    proto = open(os.path.join(ROOT, "scannertools_amd", "scanner_kernels", "scannertools_imgproc_amd.proto")).read()
    assert "Entropy entropy = 2;" in proto and "HOST = 0;" in proto and "GPU = 1;" in proto and "AUTO = 2;" in proto
    src = open(os.path.join(ROOT, "scannertools_amd", "scanner_kernels", "image_decoder_kernel_hip.cpp")).read()
    assert "st_jpeg_decode_batch_gpu" in src and "f.number == 2" in src


def test_front_end_names_and_value_error():
    from scannertools_amd import _native, engine, hip
    for sym in ("st_jpeg_restart_intervals", "st_jpeg_coefficients_by_interval", "st_jpeg_decode_batch_gpu"):
        assert sym in _native.SIGNATURES and hasattr(_native.lib(), sym)
    assert hip.JPEG_ENTROPY_MODES == ("host", "gpu", "auto")
    for bad in ("GPU", "device", None, 1):
        with pytest.raises(ValueError, match="entropy must be one of"):
            hip.HipContext.decode_jpeg(None, [DRI["restart:40x24_gray_rst2"]], entropy=bad)       # refused before the context is touched
    with pytest.raises(ValueError, match="entropy"):
        engine._Ops.ImageDecoder(None, img=None, args={"entropy": "device"})


def test_engine_names_the_row_without_restart_intervals():
    """entropy = GPU: rows are probed on the host before a kernel instance exists, so no GPU is needed to be told which row."""
    from scannertools_amd.engine import Client, DeviceType, NamedStream, PerfParams
    good = [RST[str(n) + "__jpg"].tobytes() for n in RST["good"]]
    sc = Client()
    sc.ingest_rows("jpgs", good[:2] + [GOLD["32x24_batch00__jpg"].tobytes()] + good[2:])
    img = sc.io.Input([NamedStream(sc, "jpgs")])
    with pytest.raises(ValueError, match="row 2: no restart intervals"):
        sc.run(sc.io.Output(sc.ops.ImageDecoder(img=img, device=DeviceType.CPU, batch=8, args={"entropy": "gpu"}), [NamedStream(sc, "o")]),
               PerfParams.estimate())


SANITIZER_MAIN = r'''
// Stand-alone driver of st_jpeg_restart_intervals and st_jpeg_coefficients_by_interval under AddressSanitizer + UBSan: every
// buffer is a heap block of exactly the size the call is told, so one byte read or written past it is the sanitizer's to see.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scannertools_hip.h"
#include "st_jpeg_entropy.h"

static long calls = 0, wide_runs = 0, by_status[5] = {0, 0, 0, 0, 0};

static bool known(int st) { return st >= 0 && st <= 4; }

// The kernel's form of the core (8-byte word loads, WIDE) on the host: the entropy-coded bytes copied to a 16-byte aligned block
// padded by exactly the 16 bytes the upload promises, every interval decoded from it.  It must agree with the byte-load form.
static void wide_twin(const unsigned char* buf, size_t n, const uint32_t* table, size_t count, const int16_t* coef, size_t cap, int s2) {
  StJpegHeader* hd = new StJpegHeader;
  char msg[160];
  if (st_jpeg_parse_header(buf, n, hd, msg, sizeof msg) != ST_OK) { printf("the scan passed and the markers do not\n"); exit(3); }
  const size_t first = table[0], nbytes = table[2 * count - 1] - first, padded = (nbytes + 16 + 15) & ~(size_t)15;
  unsigned char* wide = (unsigned char*)aligned_alloc(16, padded);
  memset(wide, 0, padded);
  memcpy(wide, buf + first, nbytes);
  StJpegFrameTables* tabs = new StJpegFrameTables;
  memset(tabs, 0, sizeof *tabs);
  for (int c = 0; c < hd->ncomp; ++c) { tabs->dc[c] = hd->dc[hd->td[c]]; tabs->ac[c] = hd->ac[hd->ta[c]]; }
  const StJpegScanGeom g = st_jpeg_scan_geom(*hd);
  const StJpegZigzag zz = st_jpeg_zigzag();
  int16_t* coef2 = (int16_t*)malloc(cap * 2 ? cap * 2 : 1);
  int je = ST_JE_OK;
  for (size_t k = 0; k < count && je == ST_JE_OK; ++k)
    je = st_jpeg_decode_interval<true>(wide, (uint32_t)(table[2 * k] - first), (uint32_t)(table[2 * k + 1] - first), (long long)k * hd->restart_interval,
                                       hd->restart_interval, g, tabs, zz.nat, coef2);
  if ((je == ST_JE_OK) != (s2 == ST_OK)) { printf("word loads: status %d, byte loads: %d\n", je, s2); exit(3); }
  if (je == ST_JE_OK && memcmp(coef, coef2, cap * 2) != 0) { printf("word loads and byte loads decode different coefficients\n"); exit(3); }
  wide_runs++;
  free(coef2);
  free(wide);
  delete tabs;
  delete hd;
}

// returns the two statuses in one number; exits when a call returns no status at all
static int run(const unsigned char* data, size_t n) {
  unsigned char* buf = (unsigned char*)malloc(n ? n : 1);
  memcpy(buf, data, n);
  st_jpeg_info info;
  size_t cap = 0, count = 0;
  if (st_jpeg_probe(buf, n, &info) == ST_OK) {
    const size_t mx = ((size_t)info.w + 8 * info.h_samp - 1) / (8 * info.h_samp), my = ((size_t)info.h + 8 * info.v_samp - 1) / (8 * info.v_samp);
    cap = 64 * mx * my * (info.channels == 3 ? (size_t)info.h_samp * info.v_samp + 2 : 1);
  }
  int s1 = st_jpeg_restart_intervals(buf, n, nullptr, 0, &count, &info);
  uint32_t* table = nullptr;
  if (s1 == ST_OK) {
    table = (uint32_t*)malloc(count * 8 ? count * 8 : 1);
    s1 = st_jpeg_restart_intervals(buf, n, table, count, &count, &info);
    if (s1 == ST_OK)
      for (size_t k = 0; k < count; ++k)
        if (table[2 * k] > table[2 * k + 1] || table[2 * k + 1] > n) { printf("interval %zu outside the stream\n", k); exit(3); }
  }
  int16_t* coef = (int16_t*)malloc(cap * 2 ? cap * 2 : 1);
  unsigned short quant[192];
  const int s2 = st_jpeg_coefficients_by_interval(buf, n, coef, cap, quant, &info);
  if (s1 == ST_OK) wide_twin(buf, n, table, count, coef, cap, s2);
  free(table);
  free(coef);
  free(buf);
  if (!known(s1) || !known(s2)) { printf("a call returned %d / %d\n", s1, s2); exit(3); }
  calls += 2;
  by_status[s1]++;
  by_status[s2]++;
  return s1 * 10 + s2;
}

static std::vector<unsigned char> slurp(const char* path) {
  std::vector<unsigned char> v;
  FILE* f = fopen(path, "rb");
  if (!f) { printf("cannot read %s\n", path); exit(2); }
  unsigned char chunk[4096];
  size_t got;
  while ((got = fread(chunk, 1, sizeof chunk, f)) > 0) v.insert(v.end(), chunk, chunk + got);
  fclose(f);
  return v;
}

int main(int argc, char** argv) {
  bool fuzz = false;
  unsigned long long seed = 0x9E3779B97F4A7C15ull;
  for (int a = 1; a < argc; ++a) {
    if (!strcmp(argv[a], "--fuzz")) { fuzz = true; continue; }
    if (!strcmp(argv[a], "--whole")) { fuzz = false; continue; }
    std::vector<unsigned char> d = slurp(argv[a]);
    printf("whole %s %02d\n", argv[a], run(d.data(), d.size()));
    if (!fuzz) continue;
    for (size_t cut = 0; cut < d.size(); ++cut) run(d.data(), cut);              // every prefix
    for (int i = 0; i < 1500; ++i) {                                             // seeded single-byte corruptions
      seed = seed * 6364136223846793005ull + 1442695040888963407ull;
      const size_t pos = (size_t)((seed >> 33) % d.size());
      const unsigned char old = d[pos];
      d[pos] = (unsigned char)(seed >> 17);
      run(d.data(), d.size());
      d[pos] = old;
    }
  }
  if (wide_runs < 1000) { printf("only %ld runs of the word loads\n", wide_runs); return 3; }
  printf("sanitized run ok: %ld calls, by status %ld %ld %ld %ld %ld\n", calls, by_status[0], by_status[1], by_status[2], by_status[3], by_status[4]);
  return 0;
}
'''


def test_core_scan_and_twin_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program (its own main, nothing preloaded, no Python inside): st_jpeg_parse.cpp + st_jpeg_entropy.h built with
    -fsanitize=address,undefined, run over every prefix and 1500 seeded single-byte corruptions of three streams, and over the
    good and the corrupt streams the GPU test hands to the kernel, which runs the same core.  Wherever the scan passes, the
    kernel's form of the bit reader (aligned 8-byte words from a block padded as the upload pads it) decodes the stream too and
    must agree with the byte loads."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    (tmp_path / "main.cpp").write_text(SANITIZER_MAIN)
    exe = tmp_path / "jpeg_entropy_asan"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "scannertools_amd", "csrc"), str(tmp_path / "main.cpp"),
           os.path.join(ROOT, "scannertools_amd", "csrc", "st_jpeg_parse.cpp"), "-o", str(exe)]
    # the runtimes linked into the program where their archives exist, so that nothing depends on the order of loaded libraries
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr) and "error:" not in build.stderr:
        pytest.skip("no sanitizer runtime: " + build.stderr[-300:])
    assert build.returncode == 0, build.stderr[-4000:]
    fuzz = {"a.jpg": GOLD["17x13_noise_q100_420_rst3__jpg"], "b.jpg": RST["40x24_gray_rst2__jpg"], "c.jpg": RST["32x24_mixed_opt__jpg"]}
    whole = {str(n) + ".jpg": RST[str(n) + "__jpg"] for n in list(RST["good"]) + list(RST["corrupt"]) + list(RST["cases"])}
    for name, data in list(fuzz.items()) + list(whole.items()):
        (tmp_path / name).write_bytes(data.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0")
    p = subprocess.run([str(exe), "--fuzz"] + [str(tmp_path / n) for n in fuzz] + ["--whole"] + [str(tmp_path / n) for n in whole],
                       capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "sanitized run ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr, p.stderr[-4000:]
    lines = dict(l.split()[1:3] for l in p.stdout.splitlines() if l.startswith("whole "))
    for n in RST["cases"]:
        assert lines[str(tmp_path / (str(n) + ".jpg"))] == "00", n
    for n in RST["corrupt"]:
        assert lines[str(tmp_path / (str(n) + ".jpg"))] == "01", n     # the scan finds its markers, the decoder reports the interval
