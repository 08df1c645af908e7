"""CPU: the decoding by subsequence on the host -- st_jpeg_scan_segments and st_jpeg_coefficients_by_subsequence (the CPU twin of
the kernels of st_jpeg_subseq.hip: the same bounded core, st_jpeg_entropy.h) -- against st_jpeg_coefficients and the numpy
definition (tests/ref_jpeg_np.py) on every stream of the four golden files at several subsequence sizes, the conditions on those
inputs that make the comparison mean something, the status classes of broken streams, the ImageDecoderArgs.split field, and the
core under AddressSanitizer + UBSan in a stand-alone program."""
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
SUB = np.load(os.path.join(GOLDEN, "jpeg_subsequence_golden.npz"))
ST_OK, ST_ERR_INVALID, ST_ERR_UNSUPPORTED = 0, 1, 4
DEFAULT_S, DEFAULT_ROUNDS = 128, 64          # kStJsqDefaultSubseqBytes, kStJsqDefaultMaxRounds (st_jpeg_entropy.h)
SIZES = (8, 16, 64, 0)                       # subseq_bytes of the parity test; 0: the default


def _scan_start(jpg):
    sos = jpg.index(b"\xff\xda")
    return sos + 2 + int.from_bytes(jpg[sos + 2:sos + 4], "big")


def _dri(jpg):
    at = jpg.find(b"\xff\xdd\x00\x04", 0, _scan_start(jpg))
    return int.from_bytes(jpg[at + 4:at + 6], "big") if at >= 0 else 0


def _all_streams():
    """{name: stream} of every decodable stream of the four golden files."""
    out = {}
    for tag, G, names in (("golden", GOLD, [str(c) for c in GOLD["cases"]]), ("restart", RST, [str(c) for c in RST["cases"]]),
                          ("encode", ENC, [k[:-5] for k in ENC.files if k.endswith("__jpg")]), ("subseq", SUB, [str(c) for c in SUB["cases"]])):
        for n in names:
            out[tag + ":" + n] = G[n + "__jpg"].tobytes()
    return out


ALL = _all_streams()


@pytest.fixture(scope="module")
def L():
    from scannertools_amd import _native
    return _native.lib()


def _host(L, data):
    from scannertools_amd import _native
    info = _native.JpegInfo()
    coef = np.full(1 << 18, 12345, np.int16)
    quant = np.zeros((3, 64), np.uint16)
    st = L.st_jpeg_coefficients(data, len(data), coef.ctypes.data, coef.size, quant.ctypes.data, ctypes.byref(info))
    return st, info.message.decode(), coef, quant


def _twin(L, data, S=0, R=0):
    from scannertools_amd import _native
    info, rounds, opts = _native.JpegInfo(), ctypes.c_int(-1), _native.JpegSplitOpts(S, R)
    coef = np.full(1 << 18, 12345, np.int16)
    quant = np.zeros((3, 64), np.uint16)
    st = L.st_jpeg_coefficients_by_subsequence(data, len(data), ctypes.byref(opts), coef.ctypes.data, coef.size, quant.ctypes.data, ctypes.byref(info),
                                               ctypes.byref(rounds))
    return st, info.message.decode(), coef, quant, rounds.value


def _segments(L, data):
    from scannertools_amd import _native
    info, count = _native.JpegInfo(), ctypes.c_size_t(0)
    st = L.st_jpeg_scan_segments(data, len(data), None, 0, ctypes.byref(count), ctypes.byref(info))
    if st != ST_OK:
        return st, info.message.decode(), None
    table = np.zeros((count.value, 2), np.uint32)
    st = L.st_jpeg_scan_segments(data, len(data), table.ctypes.data, count.value, ctypes.byref(count), ctypes.byref(info))
    return st, info.message.decode(), table


def test_golden_file_holds_what_the_issue_lists():
    assert os.path.getsize(os.path.join(GOLDEN, "jpeg_subsequence_golden.npz")) < 300 * 1000
    cases = [str(c) for c in SUB["cases"]]
    assert len(cases) == 9 and len(SUB["good"]) == 4 and len(SUB["corrupt"]) == 2
    big = SUB["203x213_noise_420__jpg"].tobytes()
    assert 40000 <= len(big) <= 60000 and _dri(big) == 0 and big.count(b"\xff\x00", _scan_start(big)) > 50
    assert SUB["61x45_gray__img"].shape == (45, 61, 1) and _dri(SUB["61x45_gray__jpg"].tobytes()) == 0
    assert _dri(SUB["97x75_420_opt__jpg"].tobytes()) == 0 and _dri(SUB["264x40_422_rstrow4__jpg"].tobytes()) > 0 and _dri(SUB["232x40_444_rstrow4__jpg"].tobytes()) > 0
    assert sum(_dri(GOLD[str(c) + "__jpg"].tobytes()) == 0 for c in GOLD["cases"]) == 130
    assert sum(_dri(GOLD[str(c) + "__jpg"].tobytes()) > 0 for c in GOLD["cases"]) == 42
    for name in SUB["corrupt"]:                                                           # every marker is there, scan bytes are not
        bad, of = SUB[str(name) + "__jpg"].tobytes(), SUB[str(SUB["good"][int(SUB[str(name) + "__of"])]) + "__jpg"].tobytes()
        assert bad[:_scan_start(bad)] == of[:_scan_start(of)] and bad.endswith(b"\xff\xd9") and len(bad) < len(of) and _dri(bad) == 0


def test_segments_of_every_golden_stream(L):
    from scannertools_amd import hip
    for name, jpg in ALL.items():
        st, msg, t = _segments(L, jpg)
        assert st == ST_OK and msg == "", (name, st, msg)
        if _dri(jpg) > 0:
            assert np.array_equal(t, hip.jpeg_restart_intervals(jpg)), name              # with DRI: the interval table
        else:
            eoi = len(jpg) - 2
            assert jpg[eoi:] == b"\xff\xd9" and t.tolist() == [[_scan_start(jpg), eoi]], name   # without: the scan up to its EOI
    # what the probe refuses is refused with the probe's status and message
    from scannertools_amd import _native
    for name in GOLD["refused"]:
        if str(name) == "truncated_scan":
            continue                                                                      # sound markers: it has a segment table
        jpg = GOLD[str(name) + "__jpg"].tobytes()
        info = _native.JpegInfo()
        want = L.st_jpeg_probe(jpg, len(jpg), ctypes.byref(info))
        st, msg, _ = _segments(L, jpg)
        assert st == want == int(GOLD[str(name) + "__status"]) and msg == info.message.decode() and msg, name
    jpg = ALL["restart:40x24_gray_rst2"]
    info, count = _native.JpegInfo(), ctypes.c_size_t(0)
    table = np.zeros((3, 2), np.uint32)
    assert L.st_jpeg_scan_segments(jpg, len(jpg), table.ctypes.data, 3, ctypes.byref(count), ctypes.byref(info)) == ST_ERR_INVALID
    assert count.value == 8 and not table.any()


@pytest.fixture(scope="module")
def definition():
    """ref_jpeg_np.coefficients of every stream, computed once."""
    return {name: ref.coefficients(jpg) for name, jpg in ALL.items()}


@pytest.fixture(scope="module")
def runs(L):
    """{(name, subseq_bytes): (status, message, coefficients, tables, rounds)} of the twin at the sizes of the parity test."""
    return {(name, S): _twin(L, jpg, S) for name, jpg in ALL.items() for S in SIZES}


def test_coefficient_parity(L, definition, runs):
    assert len(ALL) == 172 + 12 + 167 + 9
    for name, jpg in ALL.items():
        st0, msg0, coef0, quant0 = _host(L, jpg)
        assert st0 == ST_OK, (name, msg0)
        want, wq = definition[name]
        assert np.array_equal(coef0[:want.size], want), name
        for S in SIZES:
            st, msg, coef, quant, rounds = runs[name, S]
            assert st == ST_OK and msg == "", (name, S, st, msg)
            assert np.array_equal(coef, coef0) and np.array_equal(quant, quant0), (name, S, int((coef != coef0).sum()))
            assert (coef[want.size:] == 12345).all() and np.array_equal(quant[:len(wq)], wq), (name, S)   # the tail is untouched
            assert 1 <= rounds <= DEFAULT_ROUNDS, (name, S, rounds)
        # max_rounds = 1: whatever has not converged after one round is decoded by the interval decoder
        for S in (8, 0):
            st, msg, coef, quant, rounds = _twin(L, jpg, S, 1)
            assert st == ST_OK and rounds == 1 and np.array_equal(coef, coef0) and np.array_equal(quant, quant0), (name, S, st, msg)


def test_the_inputs_exercise_what_the_parity_test_claims(L, runs):
    """Conditions on the inputs, not on the decoder: enough rounds, a stream that never synchronises, subsequences that start on
    both bytes of an FF 00 pair, segments shorter than a subsequence and longer than a workgroup of 64."""
    most = {S: max(runs[name, S][4] for name in ALL) for S in SIZES}
    assert most[0] >= 3 and most[8] >= 16, most
    assert runs["golden:200x328_422", 0][4] >= 3 and runs["golden:200x328_422", 8][4] >= 16
    on_00 = on_ff = never = shorter = longer = 0
    for name, jpg in ALL.items():
        _, _, t = _segments(L, jpg)
        for S in SIZES:
            s = S or DEFAULT_S
            counts = [max(1, -(-(int(e) - int(b)) // s)) for b, e in t]
            shorter += any(int(e) - int(b) < s for b, e in t)
            longer += any(c > 64 for c in counts)
            if len(t) == 1 and counts[0] > 1 and runs[name, S][4] == counts[0]:
                never += 1                                                               # as many rounds as subsequences
            for b, e in t:
                for at in range(int(b) + s, int(e), s):
                    on_00 += jpg[at - 1] == 0xFF and jpg[at] == 0x00
                    on_ff += jpg[at] == 0xFF
    assert on_00 >= 1 and on_ff >= 1 and never >= 1 and shorter >= 1 and longer >= 1, (on_00, on_ff, never, shorter, longer)


def test_front_end_by_subsequence(L):
    from scannertools_amd import hip
    jpg = ALL["golden:200x328_422"]
    a, qa = hip.jpeg_coefficients(jpg)
    b, qb, rounds = hip.jpeg_coefficients(jpg, by_subsequence=True)
    assert np.array_equal(a, b) and np.array_equal(qa, qb) and rounds >= 3
    c, qc, rounds8 = hip.jpeg_coefficients(jpg, by_subsequence=True, subseq_bytes=8)
    assert np.array_equal(a, c) and rounds8 >= 16
    assert hip.jpeg_coefficients(jpg, by_subsequence=True, max_rounds=1)[2] == 1
    for S, R in ((12, 0), (4, 0), (4104, 0), (-8, 0), (0, -1)):
        with pytest.raises(hip.StError, match="subseq_bytes"):
            hip.jpeg_coefficients(jpg, by_subsequence=True, subseq_bytes=S, max_rounds=R)
    coef = np.full(64, 12345, np.int16)
    assert L.st_jpeg_coefficients_by_subsequence(jpg, len(jpg), None, coef.ctypes.data, 63, None, None, None) == ST_ERR_INVALID and (coef == 12345).all()


def _same_class(L, bad, what, strays):
    """The twin and st_jpeg_coefficients agree on whether `bad` decodes, and on the coefficients when it does.  The one documented
    deviation is counted, not tolerated silently: bytes behind a restart interval's last block, which the
    interval decoders ignore and the host decoder takes for a missing RSTn."""
    st0, msg0, coef0, _ = _host(L, bad)
    for S in (8, 0):
        st, msg, coef, _, _ = _twin(L, bad, S)
        if st != st0 and st == ST_OK and st0 == ST_ERR_INVALID and "no RST" in msg0:
            strays.append(what)
            continue
        assert st == st0, (what, S, st, msg, st0, msg0)
        if st == ST_OK:
            assert np.array_equal(coef, coef0), (what, S)


def test_status_classes(L):
    strays = []
    rng = np.random.default_rng(20261020)
    for name in ("subseq:32x24_good0", "golden:17x13_noise_q100_420_rst3", "restart:32x24_mixed_opt"):
        jpg = ALL[name]
        assert (_dri(jpg) == 0) == name.startswith("subseq:")
        for cut in range(len(jpg)):                                                       # every prefix
            _same_class(L, jpg[:cut], (name, "prefix", cut), strays)
        for _ in range(1500):                                                             # seeded single-byte corruptions
            pos, val = int(rng.integers(0, len(jpg))), int(rng.integers(0, 256))
            _same_class(L, jpg[:pos] + bytes([val]) + jpg[pos + 1:], (name, "byte", pos, val), strays)
    assert len(strays) < 200, len(strays)                                                 # (rare: a byte changed in front of a marker)
    for name in SUB["corrupt"]:
        bad = SUB[str(name) + "__jpg"].tobytes()
        for S in (8, 16, 0):
            st, msg, _, _, _ = _twin(L, bad, S)
            assert st == ST_ERR_INVALID and msg.startswith("corrupt scan: the scan: "), (name, S, st, msg)
        assert _host(L, bad)[0] == ST_ERR_INVALID
        with pytest.raises((ValueError, IndexError, KeyError)):
            ref.decode(bad)
    for name in RST["corrupt"]:                                                           # with DRI the message names the interval
        bad, k = RST[str(name) + "__jpg"].tobytes(), int(RST[str(name) + "__interval"])
        st, msg, _, _, _ = _twin(L, bad, 8)
        assert st == ST_ERR_INVALID and "restart interval %d of 4" % k in msg, (name, st, msg)


def test_image_decoder_args_split_field():
    from scannertools_amd import _proto
    assert _proto.image_decoder_args(entropy="gpu", split="subsequence") == b"\x10\x01\x18\x01" == _proto.encode([(2, "int32", 1), (3, "int32", 1)])
    assert _proto.image_decoder_args(None, None, None) == b"" and _proto.image_decoder_args(split="interval") == b"\x18\x00"
    assert _proto.image_decoder_args("JPEG", "AUTO", "SUBSEQUENCE") == b"\x08\x01\x10\x02\x18\x01"
    assert _proto.parse_image_decoder_args(b"\x10\x01") == {"entropy": "GPU"}              # an absent field stays absent: INTERVAL
    for split in ("INTERVAL", "SUBSEQUENCE"):
        assert _proto.parse_image_decoder_args(_proto.image_decoder_args(entropy="gpu", split=split.lower())) == {"entropy": "GPU", "split": split}
    assert _proto.parse_image_decoder_args(_proto.image_decoder_args(split=7)) == {"split": 7}
    with pytest.raises(ValueError, match="split"):
        _proto.image_decoder_args(split="lane")
    proto = open(os.path.join(ROOT, "scannertools_amd", "scanner_kernels", "scannertools_imgproc_amd.proto")).read()
    assert "enum Split {" in proto and "INTERVAL = 0;" in proto and "SUBSEQUENCE = 1;" in proto and "Split split = 3;" in proto
    assert "Entropy entropy = 2;" in proto
    src = open(os.path.join(ROOT, "scannertools_amd", "scanner_kernels", "image_decoder_kernel_hip.cpp")).read()
    assert "st_jpeg_decode_batch_gpu_split" in src and "f.number == 3" in src and "invalid split" in src


def test_front_end_names_and_value_errors():
    from scannertools_amd import _native, engine, hip
    for sym in ("st_jpeg_scan_segments", "st_jpeg_coefficients_by_subsequence", "st_jpeg_decode_batch_gpu_split"):
        assert sym in _native.SIGNATURES and hasattr(_native.lib(), sym)
    assert "st_jpeg_subseq.hip" in open(os.path.join(ROOT, "scannertools_amd", "csrc", "Makefile")).read()
    assert hip.JPEG_ENTROPY_SPLITS == ("interval", "subsequence") and hip.JPEG_ENTROPY_MODES == ("host", "gpu", "auto")
    jpg = ALL["subseq:32x24_good0"]
    for bad in ("SUBSEQUENCE", "lane", None, 1):
        with pytest.raises(ValueError, match="split must be one of"):
            hip.HipContext.decode_jpeg(None, [jpg], entropy="gpu", split=bad)                 # refused before the context is touched
    with pytest.raises(ValueError, match="split='subsequence'.*entropy"):
        hip.HipContext.decode_jpeg(None, [jpg], split="subsequence")
    with pytest.raises(ValueError, match="split='subsequence'.*entropy"):
        hip.HipContext.decode_jpeg(None, [jpg], entropy="host", split="subsequence")
    with pytest.raises(ValueError, match="split"):
        engine._Ops.ImageDecoder(None, img=None, args={"entropy": "gpu", "split": "lane"})


def test_engine_asks_for_restart_intervals_only_when_split_is_interval():
    """Rows are probed on the host before a kernel instance exists.  Row 1 has no restart intervals and row 2 another shape: by
    interval the engine stops at row 1; by subsequence row 1 passes and it stops at row 2 -- no GPU is needed to see either."""
    from scannertools_amd.engine import Client, DeviceType, NamedStream, PerfParams
    rows = [RST[str(RST["good"][0]) + "__jpg"].tobytes(), ALL["subseq:32x24_good0"], ALL["subseq:61x45_gray"]]
    for args, complaint in (({"entropy": "gpu"}, "row 1: no restart intervals"), ({"entropy": "gpu", "split": "interval"}, "row 1: no restart intervals"),
                            ({"entropy": "gpu", "split": "subsequence"}, "row 2 changes shape"), ({"entropy": "auto", "split": "subsequence"}, "row 2 changes shape")):
        sc = Client()
        sc.ingest_rows("jpgs", rows)
        img = sc.io.Input([NamedStream(sc, "jpgs")])
        with pytest.raises(ValueError, match=complaint):
            sc.run(sc.io.Output(sc.ops.ImageDecoder(img=img, device=DeviceType.CPU, batch=8, args=args), [NamedStream(sc, "o")]), PerfParams.estimate())


SANITIZER_MAIN = r'''
// Stand-alone driver of st_jpeg_scan_segments and st_jpeg_coefficients_by_subsequence under AddressSanitizer + UBSan: every buffer
// is a heap block of exactly the size the call is told, so one byte read or written past it is the sanitizer's to see.  Each input
// is decoded at several subsequence sizes and with the rounds capped at one (the fallback); all must agree with one another and,
// in status class, with st_jpeg_coefficients -- except where that one takes stray bytes behind an interval for a missing RSTn.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scannertools_hip.h"
#include "st_jpeg_entropy.h"

static long calls = 0, strays = 0, wide_runs = 0, by_status[5] = {0, 0, 0, 0, 0};

// The kernels' form of the core (two aligned 8-byte words per symbol, WIDE) on the host: the entropy-coded bytes copied to a 16-byte
// aligned block padded by exactly the 16 bytes the upload promises, every segment cut into 8-byte subsequences and walked lane
// after lane from the exit of the lane before, with stores.  It must agree with the byte-load form.
static void wide_twin(const unsigned char* buf, size_t n, const int16_t* coef, size_t cap, int s2) {
  StJpegHeader* hd = new StJpegHeader;
  char msg[160];
  if (st_jpeg_parse_header(buf, n, hd, msg, sizeof msg) != ST_OK) { printf("the twin passed and the markers do not\n"); exit(3); }
  const size_t count = st_jpeg_segment_count(*hd);
  uint32_t* table = (uint32_t*)malloc(count * 8);
  if (st_jpeg_segments(buf, n, *hd, table, msg, sizeof msg) != ST_OK) { printf("the twin passed and the segments do not\n"); exit(3); }
  const size_t first = table[0], nbytes = table[2 * count - 1] - first, padded = (nbytes + 16 + 15) & ~(size_t)15;
  unsigned char* wide = (unsigned char*)aligned_alloc(16, padded);
  memset(wide, 0, padded);
  memcpy(wide, buf + first, nbytes);
  StJpegFrameTables* tabs = new StJpegFrameTables;
  memset(tabs, 0, sizeof *tabs);
  for (int c = 0; c < hd->ncomp; ++c) { tabs->dc[c] = hd->dc[hd->td[c]]; tabs->ac[c] = hd->ac[hd->ta[c]]; }
  const StJpegScanGeom g = st_jpeg_scan_geom(*hd);
  const StJpegZigzag zz = st_jpeg_zigzag();
  int16_t* coef2 = (int16_t*)calloc(cap ? cap : 1, 2);
  const long long total = (long long)hd->mcux * hd->mcuy;
  int je = ST_JE_OK;
  for (size_t k = 0; k < count && je == ST_JE_OK; ++k) {
    const uint32_t begin = (uint32_t)(table[2 * k] - first), end = (uint32_t)(table[2 * k + 1] - first), S = 8;
    const long long mcu0 = hd->restart_interval > 0 ? (long long)k * hd->restart_interval : 0;
    long long nmcu = hd->restart_interval > 0 ? hd->restart_interval : total;
    if (nmcu > total - mcu0) nmcu = total - mcu0;
    const uint32_t seg_blocks = (uint32_t)(nmcu * st_jsq_mcu_blocks(g)), nsub = st_jsq_count(end - begin, S);
    StJsqOut o;
    o.exit = st_jsq_pack(begin, 0, 0, 0);
    uint32_t before = 0, dc[3] = {0, 0, 0};
    for (uint32_t i = 0; i < nsub && je == ST_JE_OK && before < seg_blocks && o.exit != kStJsqInvalid; ++i) {
      const uint64_t sub_end = (uint64_t)begin + ((uint64_t)i + 1) * S;
      je = st_jsq_run<true, true>(wide, end, (uint32_t)(sub_end < end ? sub_end : end), i + 1 == nsub, o.exit, g, tabs, zz.nat, mcu0, seg_blocks, before, dc, coef2, &o);
      before += o.blocks;
      for (int c = 0; c < 3; ++c) dc[c] = o.dc[c];
    }
  }
  if ((je == ST_JE_OK) != (s2 == ST_OK)) { printf("word loads: status %d, byte loads: %d\n", je, s2); exit(3); }
  if (je == ST_JE_OK && memcmp(coef, coef2, cap * 2) != 0) { printf("word loads and byte loads decode different coefficients\n"); exit(3); }
  wide_runs++;
  free(coef2);
  free(wide);
  free(table);
  delete tabs;
  delete hd;
}

static int run(const unsigned char* data, size_t n) {
  unsigned char* buf = (unsigned char*)malloc(n ? n : 1);
  memcpy(buf, data, n);
  st_jpeg_info info;
  size_t cap = 0, count = 0;
  if (st_jpeg_probe(buf, n, &info) == ST_OK) {
    const size_t mx = ((size_t)info.w + 8 * info.h_samp - 1) / (8 * info.h_samp), my = ((size_t)info.h + 8 * info.v_samp - 1) / (8 * info.v_samp);
    cap = 64 * mx * my * (info.channels == 3 ? (size_t)info.h_samp * info.v_samp + 2 : 1);
  }
  int s1 = st_jpeg_scan_segments(buf, n, nullptr, 0, &count, &info);
  if (s1 == ST_OK) {
    uint32_t* table = (uint32_t*)malloc(count * 8 ? count * 8 : 1);
    s1 = st_jpeg_scan_segments(buf, n, table, count, &count, &info);
    if (s1 == ST_OK)
      for (size_t k = 0; k < count; ++k)
        if (table[2 * k] > table[2 * k + 1] || table[2 * k + 1] > n) { printf("segment %zu outside the stream\n", k); exit(3); }
    free(table);
  }
  int16_t* host = (int16_t*)malloc(cap * 2 ? cap * 2 : 1);
  int16_t* first = (int16_t*)malloc(cap * 2 ? cap * 2 : 1);
  int16_t* coef = (int16_t*)malloc(cap * 2 ? cap * 2 : 1);
  unsigned short quant[192];
  const int s0 = st_jpeg_coefficients(buf, n, host, cap, quant, &info);
  char host_msg[sizeof info.message];
  memcpy(host_msg, info.message, sizeof host_msg);
  static const st_jpeg_split_opts opts[5] = {{8, 0}, {16, 0}, {128, 0}, {0, 1}, {8, 1}};
  int s2 = -1;
  for (int v = 0; v < 5; ++v) {
    int rounds = -1;
    const int s = st_jpeg_coefficients_by_subsequence(buf, n, &opts[v], v ? coef : first, cap, quant, &info, &rounds);
    if (s < 0 || s > 4) { printf("a call returned %d\n", s); exit(3); }
    if (v == 0) s2 = s;
    if (s != s2) { printf("subseq_bytes %d / max_rounds %d: status %d, at 8 bytes %d\n", opts[v].subseq_bytes, opts[v].max_rounds, s, s2); exit(3); }
    if (s == ST_OK && v && memcmp(first, coef, cap * 2) != 0) { printf("subseq_bytes %d / max_rounds %d decodes other coefficients\n", opts[v].subseq_bytes, opts[v].max_rounds); exit(3); }
    if (s == ST_OK && (rounds < 1 || rounds > 64)) { printf("%d rounds\n", rounds); exit(3); }
    calls++;
  }
  if (s2 != s0) {
    if (s2 == ST_OK && s0 == ST_ERR_INVALID && strstr(host_msg, "no RST")) strays++;
    else { printf("by subsequence: status %d, the host decoder: %d\n", s2, s0); exit(3); }
  } else if (s2 == ST_OK && memcmp(first, host, cap * 2) != 0) { printf("by subsequence and the host decoder decode other coefficients\n"); exit(3); }
  if (s1 == ST_OK) wide_twin(buf, n, first, cap, s2);
  free(host);
  free(first);
  free(coef);
  free(buf);
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
  printf("sanitized run ok: %ld calls, %ld with stray bytes, by status %ld %ld %ld %ld %ld\n", calls, strays, by_status[0], by_status[1], by_status[2], by_status[3], by_status[4]);
  return 0;
}
'''


def test_core_and_twin_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program (its own main, nothing preloaded, no Python inside): st_jpeg_parse.cpp + st_jpeg_entropy.h built with
    -fsanitize=address,undefined, run over every prefix and 1500 seeded single-byte corruptions of three streams (one without
    restart intervals), and over the good and the corrupt streams the GPU test hands to the kernels, which run the same core."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    (tmp_path / "main.cpp").write_text(SANITIZER_MAIN)
    exe = tmp_path / "jpeg_subseq_asan"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "scannertools_amd", "csrc"), str(tmp_path / "main.cpp"),
           os.path.join(ROOT, "scannertools_amd", "csrc", "st_jpeg_parse.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr) and "error:" not in build.stderr:
        pytest.skip("no sanitizer runtime: " + build.stderr[-300:])
    assert build.returncode == 0, build.stderr[-4000:]
    fuzz = {"a.jpg": SUB["32x24_good1__jpg"], "b.jpg": RST["40x24_gray_rst2__jpg"], "c.jpg": GOLD["17x13_noise_q100_420_rst3__jpg"]}
    whole = {str(n) + ".jpg": SUB[str(n) + "__jpg"] for n in list(SUB["cases"]) + list(SUB["corrupt"])}
    whole.update({str(n) + ".jpg": RST[str(n) + "__jpg"] for n in list(RST["cases"]) + list(RST["corrupt"])})
    whole["200x328_422.jpg"] = GOLD["200x328_422__jpg"]
    for name, data in list(fuzz.items()) + list(whole.items()):
        (tmp_path / name).write_bytes(data.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0")
    p = subprocess.run([str(exe), "--fuzz"] + [str(tmp_path / n) for n in fuzz] + ["--whole"] + [str(tmp_path / n) for n in whole],
                       capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0 and "sanitized run ok" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr, p.stderr[-4000:]
    lines = dict(l.split()[1:3] for l in p.stdout.splitlines() if l.startswith("whole "))
    for n in list(SUB["cases"]) + list(RST["cases"]) + ["200x328_422"]:
        assert lines[str(tmp_path / (str(n) + ".jpg"))] == "00", n
    for n in list(SUB["corrupt"]) + list(RST["corrupt"]):
        assert lines[str(tmp_path / (str(n) + ".jpg"))] == "01", n     # the segments are found, the decoder reports the one that is short
