"""CPU: ImageEncoder's optimize = 1 (per-frame optimal Huffman tables) on the host side: the restatement of
libjpeg's optimize_coding (tests/ref_jpeg_encode_opt_np.py) against the streams Pillow wrote with optimize=True
(tests/golden/jpeg_encode_opt_golden.npz) and against live Pillow, the C core (st_jpeg_optimal_table, st_jpeg_optimal_dht) and the
host statistics (st_jpeg_symbol_stats) against the restatement, what the fixture must contain, the generalised ownership rule of
restart = NONE restated in Python, the refusals of a bad `optimize` at every layer, the argument message's field 4, and the
host-only code under the address and undefined-behaviour sanitizers as a stand-alone program."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import ref_jpeg_encode_opt_np as ref
from jpeg_encode_opt_cases import CASES, SAMPLING, STORED_STREAM_LIMIT, case_name, picture, pillow_settings, sha256

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD_PATH = os.path.join(ROOT, "tests", "golden", "jpeg_encode_opt_golden.npz")
GOLD = np.load(GOLD_PATH)
NAMES = [str(c) for c in GOLD["cases"]]
ST_ERR_INVALID, ST_ERR_UNSUPPORTED = 1, 4


def _cfg(name):
    return json.loads(str(GOLD[name + "__cfg"]))


@pytest.fixture(scope="module")
def restated():
    """Per case {cfg, img, coef, jpg, hlen, freq}: the restatement's stream over the restatement's coefficients, the quantisation
    tables and the fixed parts of the header from the library.  Computed once, never changed."""
    from scannertools_amd.hip import jpeg_encode_header, jpeg_quant_tables
    out = {}
    for c in CASES:
        name = case_name(c)
        hs, vs = SAMPLING[c["subsampling"]]
        img = picture(c["kind"], c["h"], c["w"], c["seed"])
        fixed = jpeg_encode_header(c["h"], c["w"], c["quality"], c["subsampling"], restart=c["restart"])
        coef = ref.coefficients(img, *jpeg_quant_tables(c["quality"]), hs, vs)
        jpg, hlen, freq = ref.encode(coef, c["h"], c["w"], hs, vs, ref.ROW if c["restart"] == "row" else ref.NONE, fixed)
        out[name] = dict(cfg=c, img=img, coef=coef, jpg=jpg, hlen=hlen, freq=freq)
    return out


def test_restatement_equals_the_golden_streams(restated):
    """Statistics, table and header from the restatement, the scan from the existing coders: the whole stream, byte for byte (by
    SHA-256 where the file holds no more); the DHT segments in the order DC 0, AC 0, DC 1, AC 1 after SOF0 and before DRI / SOS."""
    assert NAMES == [case_name(c) for c in CASES]
    for name in NAMES:
        cfg, r = _cfg(name), restated[name]
        assert {k: cfg[k] for k in r["cfg"]} == r["cfg"], name
        assert sha256(r["img"].tobytes()) == cfg["img_sha"], name
        assert (len(r["jpg"]), sha256(r["jpg"])) == (cfg["jpg_len"], cfg["jpg_sha"]), name
        assert (name + "__jpg" in GOLD.files) == (cfg["jpg_len"] <= STORED_STREAM_LIMIT), name
        if name + "__jpg" in GOLD.files:
            assert GOLD[name + "__jpg"].tobytes() == r["jpg"], name
        hd = r["jpg"][:r["hlen"]]
        assert r["hlen"] <= (629 if cfg["restart"] == "row" else 623), name
        assert hd[158:160] == b"\xff\xc0" and hd[-14:-12] == b"\xff\xda", name   # SOF0 ends the fixed prefix, SOS the header
        at, ids = 177, []
        for _ in range(4):
            assert hd[at:at + 2] == b"\xff\xc4", name
            ids.append(hd[at + 4])
            at += 2 + int.from_bytes(hd[at + 2:at + 4], "big")
        assert ids == [0x00, 0x10, 0x01, 0x11], name
        assert hd[at:at + 2] == (b"\xff\xdd" if cfg["restart"] == "row" else b"\xff\xda"), name


def test_restatement_equals_live_pillow(restated):
    PIL = pytest.importorskip("PIL")   # noqa: F841, N806
    import io
    from PIL import Image, ImageFile
    old, ImageFile.MAXBLOCK = ImageFile.MAXBLOCK, 1 << 24
    try:
        for c in CASES:
            buf = io.BytesIO()
            Image.fromarray(restated[case_name(c)]["img"], "RGB").save(buf, "JPEG", **pillow_settings(c))
            assert buf.getvalue() == restated[case_name(c)]["jpg"], case_name(c)
    finally:
        ImageFile.MAXBLOCK = old


def _fib(n):
    """1, 2, 3, 5, 8, ...: with the pseudo-symbol's 1 in front every merge takes in exactly the next count (1, 1, 2, ... would tie,
    and the tie rule then builds a bushier tree of half the depth)."""
    f = [1, 2]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def _synthetic():
    """name -> 256 counts.  Fibonacci-like counts give a code one bit longer per symbol: 20 of them lengths up to 20 (the limiting
    to 16 acts), 31 of them lengths up to 31, still within the 32 libjpeg accepts.  Lengths ABOVE 32 are reachable with 257
    entries -- 34 Fibonacci counts or more, 15 million symbols in all -- and libjpeg stops there; "fib40" is that histogram."""
    z = np.zeros(256, np.uint64)
    out = {}

    def put(name, pairs):
        f = z.copy()
        for s, v in pairs:
            f[s] = v
        out[name] = f

    put("one_symbol", [(0, 77)])
    put("one_symbol_last", [(255, 1)])
    put("two_symbols", [(3, 5), (200, 9)])
    put("two_equal", [(0, 4), (1, 4)])
    out["all_equal"] = np.full(256, 7, np.uint64)                       # the tie rule at every step
    out["all_ones"] = np.ones(256, np.uint64)                           # ... against the pseudo-symbol's own 1 as well
    put("dc_equal", [(s, 3) for s in range(12)])
    put("fib20", list(zip(range(20), _fib(20))))
    put("fib31_reversed", list(zip(range(200, 169, -1), _fib(31))))
    put("fib31_ac", [((i % 16) << 4 | (1 + i // 16), v) for i, v in enumerate(_fib(31))])
    put("huge", [(1, 1 << 62), (2, 1 << 61), (3, 1), (250, (1 << 62) - 5)])
    rng = np.random.default_rng(5)
    out["random_sparse"] = (rng.integers(0, 1000, 256) * (rng.integers(0, 4, 256) == 0)).astype(np.uint64)
    out["random_dense"] = rng.integers(1, 1 << 20, 256).astype(np.uint64)
    return out


def test_core_equals_the_restatement(restated):
    """st_jpeg_optimal_table against optimal_table() for the four histograms of every golden case and for the synthetic ones; the
    DHT bytes and code words of st_jpeg_optimal_dht against the restatement's segment and canonical codes."""
    from scannertools_amd.hip import jpeg_optimal_dht, jpeg_optimal_table
    hists = {(name, t): restated[name]["freq"][t] for name in NAMES for t in range(4)}
    hists.update({(name, 1): f for name, f in _synthetic().items()})
    seen = set()
    for (name, t), f in hists.items():
        key = (t, f.tobytes())
        if key in seen:
            continue
        seen.add(key)
        want_bits, want_vals = ref.optimal_table(f)
        bits, vals = jpeg_optimal_table(f)
        assert (bits.tolist(), vals.tolist()) == (want_bits, want_vals), (name, t)
        cls, ident = ref.TABLES[t]
        seg, codes = jpeg_optimal_dht(f, t)
        assert seg == ref.dht(want_bits, want_vals, cls, ident), (name, t)
        tab = ref.huffman_tables(b"\xff\xd8" + seg)[(cls, ident)]
        want_codes = np.zeros(len(codes), np.uint32)
        for s, (code, ln) in tab.items():
            if s < len(codes):
                want_codes[s] = ln << 16 | code
        assert (codes == want_codes).all(), (name, t)
        assert all(code != (1 << ln) - 1 for code, ln in tab.values()), (name, t)   # no code is all ones
    assert len(seen) > 400
    assert max(ref.code_sizes(_synthetic()["fib20"])) == 20 and max(ref.code_sizes(_synthetic()["fib31_ac"])) == 31


def test_core_where_libjpeg_stops():
    """A code of more than 32 bits before the limiting: the host entry point says so, and the table it leaves (the one the device
    encodes such a frame with) is a valid prefix code of 9- and 10-bit codes over exactly the symbols in use."""
    from scannertools_amd import _native
    f = np.zeros(256, np.uint64)
    f[:40] = _fib(40)
    assert max(ref.code_sizes(f)) > 32
    bits, vals, n = np.zeros(16, np.uint8), np.zeros(256, np.uint8), ctypes.c_int()
    assert _native.lib().st_jpeg_optimal_table(f.ctypes.data, bits.ctypes.data, vals.ctypes.data, ctypes.byref(n)) == ST_ERR_UNSUPPORTED
    assert n.value == 40 and sorted(vals[:40].tolist()) == list(range(40)) and bits.tolist() == [0] * 8 + [40] + [0] * 7
    f = np.zeros(256, np.uint64)
    f[:200] = [min(v, 1 << 55) for v in _fib(200)]
    assert _native.lib().st_jpeg_optimal_table(f.ctypes.data, bits.ctypes.data, vals.ctypes.data, ctypes.byref(n)) == ST_ERR_UNSUPPORTED
    assert n.value == 200 and bits.tolist() == [0] * 8 + [128, 72] + [0] * 6
    assert sum(int(b) * 2.0 ** -(k + 1) for k, b in enumerate(bits)) < 1
    for args in ((None, bits.ctypes.data, vals.ctypes.data, ctypes.byref(n)), (f.ctypes.data, None, vals.ctypes.data, ctypes.byref(n)),
                 (f.ctypes.data, bits.ctypes.data, None, ctypes.byref(n)), (f.ctypes.data, bits.ctypes.data, vals.ctypes.data, None)):
        assert _native.lib().st_jpeg_optimal_table(*args) == ST_ERR_INVALID


def test_host_statistics_equal_the_restatement(restated):
    """st_jpeg_symbol_stats over the restatement's coefficients, in the case's own restart mode and in the other one: the two
    modes count different DC symbols for the same picture."""
    from scannertools_amd.hip import jpeg_symbol_stats
    differ = 0
    for name in NAMES:
        r = restated[name]
        c = r["cfg"]
        got = jpeg_symbol_stats(r["coef"], c["h"], c["w"], c["subsampling"], c["restart"])
        assert got.dtype == np.uint64 and (got.astype(np.int64) == r["freq"]).all(), name
        hs, vs = SAMPLING[c["subsampling"]]
        assert int(got[0].sum()) == -(-c["h"] // (8 * vs)) * -(-c["w"] // (8 * hs)) * hs * vs, name   # one DC symbol per luma block
        if c["restart"] == "none":
            row = restated[name[:-4] + "row"]
            assert (r["freq"][[1, 3]] == row["freq"][[1, 3]]).all(), name        # the AC symbols do not depend on the mode
            differ += not (r["freq"] == row["freq"]).all()
    assert differ > 60
    from scannertools_amd import _native
    coef, out = np.zeros(3 * 64, np.int16), np.zeros(1024, np.uint64)
    L = _native.lib()
    assert L.st_jpeg_symbol_stats(coef.ctypes.data, 3 * 64, 8, 8, 1, 1, 0, out.ctypes.data) == 0
    assert out[0] == 1 and out[256] == 1 and out[512] == 2 and out[768] == 2 and out.sum() == 6
    assert L.st_jpeg_symbol_stats(coef.ctypes.data, 3 * 64 - 1, 8, 8, 1, 1, 0, out.ctypes.data) == ST_ERR_INVALID
    assert L.st_jpeg_symbol_stats(coef.ctypes.data, 3 * 64, 8, 8, 1, 1, 2, out.ctypes.data) == ST_ERR_INVALID
    assert L.st_jpeg_symbol_stats(coef.ctypes.data, 3 * 64, 8, 8, 1, 2, 0, out.ctypes.data) == ST_ERR_UNSUPPORTED
    assert L.st_jpeg_symbol_stats(None, 3 * 64, 8, 8, 1, 1, 0, out.ctypes.data) == ST_ERR_INVALID


def _rows(r):
    c = r["cfg"]
    hs, vs = SAMPLING[c["subsampling"]]
    return ref.row_bits(r["coef"], c["h"], c["w"], hs, vs, r["jpg"][:r["hlen"]])


def _owner_stats(rows):
    """(rows that own no byte, bytes holding bits of three rows or more, whether the padding bits lie in a byte whose first bit
    belongs to an earlier row than the last)"""
    starts, B = [], 0
    for _, n in rows:
        starts.append(B)
        B += n
    owner = lambda bit: max(k for k, s in enumerate(starts) if s <= bit)   # noqa: E731
    no_byte = sum(1 for s, (_, n) in zip(starts, rows) if -(-(s + n) // 8) == -(-s // 8))
    three = sum(1 for k in range(-(-B // 8)) if owner(min(8 * k + 7, B - 1)) - owner(8 * k) >= 2)
    return no_byte, three, B % 8 != 0 and owner(B // 8 * 8) < len(rows) - 1


def test_golden_file_holds_the_cases_the_switch_is_held_to(restated):
    """The grid, and the coverage conditions the generator asserted when it wrote the file, found again from the file's cases."""
    assert os.path.getsize(GOLD_PATH) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "jpeg_encode_golden.npz"))
    cfgs = [_cfg(n) for n in NAMES]
    for restart in ("row", "none"):
        for sub in SAMPLING:
            for q in (1, 50, 75, 95, 100):
                kinds = {c["kind"] for c in cfgs if (c["restart"], c["subsampling"], c["quality"]) == (restart, sub, q)}
                assert {"flat", "smooth", "noise", "twolevel"} <= kinds, (restart, sub, q)
            for shape in ((8, 8), (40, 34), (47, 33), (300, 17), (130, 100)):
                assert any((c["h"], c["w"], c["restart"], c["subsampling"]) == shape + (restart, sub) for c in cfgs), (shape, restart, sub)
    long_codes = [n for n in NAMES if max(max(ref.code_sizes(f)) for f in restated[n]["freq"]) > 16]
    assert len(long_codes) >= 2 and {(_cfg(n)["h"], _cfg(n)["w"], _cfg(n)["quality"]) for n in long_codes} >= {(256, 256, 95), (256, 256, 100)}
    assert sum(int((f > 0).sum() == 1) for n in NAMES for f in restated[n]["freq"]) >= 1            # a table with a single symbol
    gray = restated["512x8_gray6_q90_444_none"]
    assert [int((f > 0).sum()) for f in gray["freq"]] == [2, 1, 1, 1] and gray["hlen"] == 177 + 23 + 3 * 22 + 14
    six = no_byte = three = early = 0
    row_bits = set()
    for n in NAMES:
        c = _cfg(n)
        if c["restart"] != "none" or "short_rows" not in c["uses"]:
            continue
        rows = _rows(restated[n])
        lengths = {b for _, b in rows}
        row_bits |= lengths
        if (c["w"], c["subsampling"], c["kind"]) == (8, "4:4:4", "flat"):
            assert lengths - {rows[0][1]} == {6}, n
            six += 1
        a, b, e = _owner_stats(rows)
        no_byte, three, early = no_byte + a, three + b, early + e
    assert six >= 4 and no_byte >= 1 and three >= 1 and early >= 1, (six, no_byte, three, early)
    assert {6, 8, 12} <= row_bits and min(row_bits) == 6
    phases = {sum(b for _, b in _rows(restated[n])[:1]) % 8 for n in NAMES if "short_rows" in _cfg(n)["uses"] and _cfg(n)["restart"] == "none"}
    assert len(phases) >= 3, phases   # the 6-bit rows start at different bit phases


def _owned_bytes(rows):
    """The unstuffed scan by the rule the kernels follow with per-frame tables: row r, at bit B of the scan and
    L bits long, owns the bytes whose first bit lies in it -- possibly none --; an owned byte is 8 bits of the row's zero-filled
    slot from bit 8 j + sh on (sh = -B mod 8), and the LAST one is completed with the bits that follow the row in the scan: the
    leading bits of as many next rows as it takes, each read from its slot's first byte, then 1-bits after the last row."""
    slots = [(value << (-L % 8)).to_bytes(-(-L // 8), "big") for value, L in rows]
    out, B, writers = bytearray(), 0, 0
    for r, (_, L) in enumerate(rows):
        slot = slots[r]
        tail, got = 0, 0
        for rr in range(r + 1, len(rows)):
            if got >= 8:
                break
            take = min(8 - got, rows[rr][1])
            tail |= ((slots[rr][0] >> (8 - take)) << (8 - got - take)) & 0xFF
            got += take
        if got < 8:
            tail |= (1 << (8 - got)) - 1
        first, sh = -(-B // 8), -B % 8
        count = -(-(B + L) // 8) - first
        for j in range(count):
            v = slot[j]
            if sh:
                v = ((v << sh) | (slot[j + 1] >> (8 - sh) if j + 1 < len(slot) else 0)) & 0xFF
            end = 8 * j + sh + 8
            if end > L:
                assert j == count - 1
                v |= tail >> (8 - (end - L))
            out.append(v)
        writers += count
        B += L
    assert writers == -(-B // 8)   # every byte of the scan has exactly one writer
    return bytes(out)


def test_generalised_ownership_rule_gives_the_golden_scans(restated):
    """Every restart = NONE golden scan, unstuffed, from the rule as the kernels apply it; and the old rule (the next row alone)
    is wrong for the streams with 6-bit rows, which is why it had to go."""
    from test_jpeg_encode_norst import _owned_bytes as old_rule
    wrong = 0
    for n in NAMES:
        r = restated[n]
        if r["cfg"]["restart"] != "none":
            continue
        rows = _rows(r)
        raw = ref.unstuffed(r["jpg"], r["hlen"])
        assert _owned_bytes(rows) == raw, n
        if min(b for _, b in rows) < 8:
            try:
                wrong += old_rule(rows) != raw
            except (ValueError, IndexError):   # the old rule shifts by the next row's length - 8
                wrong += 1
    assert wrong >= 4


def test_bound_covers_the_golden_streams(restated):
    from scannertools_amd.hip import jpeg_encode_bound, jpeg_encode_bound_opt
    for n in NAMES:
        c = _cfg(n)
        hs, vs = SAMPLING[c["subsampling"]]
        blocks = -(-c["h"] // (8 * vs)) * -(-c["w"] // (8 * hs)) * (hs * vs + 2)
        assert jpeg_encode_bound_opt(c["h"], c["w"], c["subsampling"]) == jpeg_encode_bound(c["h"], c["w"], c["subsampling"]) + 2 * blocks
        assert c["jpg_len"] <= jpeg_encode_bound_opt(c["h"], c["w"], c["subsampling"]), n
    assert (27 + 63 * 26 + 7) // 8 == 209   # a block with any table of 16-bit codes, in bytes
    with pytest.raises(Exception):
        jpeg_encode_bound_opt(0, 8)


def test_a_bad_optimize_is_refused_at_every_layer():
    from scannertools_amd import _native, _proto
    from scannertools_amd.hip import HipContext, jpeg_optimize
    L = _native.lib()
    for name in ("st_jpeg_encode_batch_opt", "st_jpeg_optimal_table", "st_jpeg_optimal_dht", "st_jpeg_symbol_stats", "st_jpeg_encode_bound_opt",
                 "st_jpeg_encode_fetch_stats"):
        assert name in _native.SIGNATURES and hasattr(ctypes.CDLL(_native.LIB_PATH), name), name
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scannertools_hip.h")).read(), flags=re.S)
    for name in ("st_jpeg_encode_batch_opt", "st_jpeg_optimal_table", "st_jpeg_symbol_stats", "st_jpeg_encode_bound_opt"):
        assert re.search(r"\b%s\s*\(" % name, header), name
    for bad in (2, -1, 3, 1 << 20):
        assert L.st_jpeg_encode_batch_opt(None, None, 1, 8, 8, 50, 2, 2, 0, bad) == ST_ERR_INVALID   # a null context is still refused first
    assert L.st_jpeg_encode_batch_opt(None, None, 1, 8, 8, 50, 2, 2, 0, 1) == ST_ERR_INVALID
    assert jpeg_optimize(False) == 0 and jpeg_optimize(True) == 1 and jpeg_optimize(1) == 1 and jpeg_optimize(0) == 0
    for bad in (2, -1, "yes", None, 1.0, "1"):
        with pytest.raises(ValueError, match=re.escape("optimize %r is not supported" % (bad,))):
            HipContext.encode_jpeg(None, [], 50, "4:2:0", optimize=bad)   # refused before the context is touched
    for bad in ("on", None, 1.5):
        with pytest.raises(ValueError, match="optimize must be False, True or a number"):
            _proto.image_encoder_args(95, "4:2:0", 0, bad)
    buf, size = ctypes.create_string_buffer(300), ctypes.c_size_t(7)
    f = np.ones(256, np.uint64)
    for bad in (-1, 4, 1 << 20):
        assert L.st_jpeg_optimal_dht(f.ctypes.data, bad, buf, 300, ctypes.byref(size), None) == ST_ERR_INVALID and size.value == 7
    assert L.st_jpeg_optimal_dht(f.ctypes.data, 1, buf, 20, ctypes.byref(size), None) == ST_ERR_INVALID and size.value == 21 + 256


def test_argument_message_field_4():
    from scannertools_amd import _proto
    # absent when false: every serialisation the existing tests pin is unchanged
    assert _proto.image_encoder_args() == _proto.image_encoder_args(0, "", 0, False) == _proto.image_encoder_args(0, "", "mcu_row", 0) == b""
    assert _proto.image_encoder_args(95, "4:2:0") == _proto.image_encoder_args(95, "4:2:0", 0, False) == b"\x08\x5f\x12\x054:2:0"
    assert _proto.image_encoder_args(95, "4:2:0", 1) == _proto.image_encoder_args(95, "4:2:0", "none", optimize=False) == b"\x08\x5f\x12\x054:2:0\x18\x01"
    assert _proto.image_encoder_args(95, "4:2:0", 1, True) == _proto.image_encoder_args(95, "4:2:0", "none", 1) == b"\x08\x5f\x12\x054:2:0\x18\x01\x20\x01"
    assert _proto.image_encoder_args(optimize=True) == b"\x20\x01"
    assert _proto.parse_image_encoder_args(b"\x20\x01") == {"optimize": True}
    assert _proto.parse_image_encoder_args(b"\x20\x00") == {"optimize": False}
    assert _proto.parse_image_encoder_args(b"\x20\x07") == {"optimize": 7}
    assert _proto.parse_image_encoder_args(b"\x08\x5f\x12\x054:2:0\x18\x01") == {"quality": 95, "subsampling": "4:2:0", "restart": "NONE"}
    for q, s, r, o in ((1, "4:4:4", 1, True), (100, "", 0, 1), (0, "4:2:2", 1, 5), (50, "4:2:0", 0, -3)):
        want = {k: v for k, v in (("quality", q), ("subsampling", s), ("restart", {1: "NONE"}.get(r, r)), ("optimize", True if o in (1, True) else o)) if v}
        assert _proto.parse_image_encoder_args(_proto.image_encoder_args(q, s, r, o)) == want
    proto = open(os.path.join(ROOT, "scannertools_amd", "scanner_kernels", "scannertools_imgproc_amd.proto")).read()
    assert re.search(r"message ImageEncoderArgsWithRestart \{.*?Restart restart = 3;\s*bool optimize = 4;\s*\}", proto, re.S)
    assert re.search(r"message ImageEncoderArgs \{\s*int32 quality = 1;\s*string subsampling = 2;\s*\}", proto)


def _run_op(sc, mk):
    from scannertools_amd.engine import NamedStream, PerfParams
    return sc.run(sc.io.Output(mk(), [NamedStream(sc, "o")]), PerfParams.estimate())


def test_validate_refuses_a_bad_optimize_without_a_gpu_context():
    from scannertools_amd import _proto
    from scannertools_amd.engine import Client, DeviceType, NamedVideoStream, _CppMultiOpNode
    sc = Client()
    sc.ingest_frames("v", np.zeros((2, 8, 8, 3), np.uint8))
    frame = sc.io.Input([NamedVideoStream(sc, "v")])
    for dev in (DeviceType.CPU, DeviceType.GPU):
        for bad in (2, 7, -1):
            with pytest.raises(RuntimeError, match=re.escape("ImageEncoder: optimize %d is not supported (0 or 1)" % bad)):
                _run_op(sc, lambda: sc.ops.ImageEncoder(frame=frame, device=dev, optimize=bad))
            with pytest.raises(RuntimeError, match=re.escape("ImageEncoder: optimize %d is not supported (0 or 1)" % bad)):
                _run_op(sc, lambda: _CppMultiOpNode(sc, "ImageEncoder", [frame], dev, None, _proto.image_encoder_args(50, "4:4:4", 1, bad)))
        # the other checks still come first and still name their cause
        with pytest.raises(RuntimeError, match=re.escape("restart 5 is not supported (MCU_ROW or NONE)")):
            _run_op(sc, lambda: sc.ops.ImageEncoder(frame=frame, device=dev, restart=5, optimize=9))
    with pytest.raises(ValueError, match="optimize must be False, True or a number"):
        sc.ops.ImageEncoder(frame=frame, optimize="always")
    import torch
    if not torch.cuda.is_available():   # valid arguments without a GPU: a loud failure, no fallback
        for optimize in (True, 1):
            with pytest.raises(RuntimeError, match="st_ctx_create"):
                _run_op(sc, lambda: sc.ops.ImageEncoder(frame=frame, optimize=optimize))


SANITIZER_MAIN = r'''
// st_jpeg_enc_host.cpp and st_jpeg_enc_opt.h under -fsanitize=address,undefined: the table construction, the DHT bytes, the code
// words and the statistics over histograms read from a file, every buffer on the heap at exactly the size the call is told.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "scannertools_hip.h"
#include "st_jpeg_enc_host.h"
#include "st_jpeg_enc_opt.h"

int main(int argc, char** argv) {
  if (argc != 2) return 1;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  long tables = 0, refused = 0;
  for (;;) {
    uint64_t* freq = (uint64_t*)malloc(256 * sizeof(uint64_t));
    if (fread(freq, sizeof(uint64_t), 256, f) != 256) { free(freq); break; }
    uint8_t* bits = (uint8_t*)malloc(16);
    uint8_t* vals = (uint8_t*)malloc(256);
    int n = -1;
    const int st = st_jpeg_optimal_table(freq, bits, vals, &n);
    if (st != ST_OK && st != ST_ERR_UNSUPPORTED) return 3;
    refused += st == ST_ERR_UNSUPPORTED;
    int total = 0;
    double kraft = 0;
    for (int k = 0; k < 16; ++k) { total += bits[k]; kraft += bits[k] / (double)(1 << (k + 1)); }
    if (total != n || n < 0 || n > 256 || kraft >= 1.0) { printf("table %ld: %d codes for %d symbols, Kraft sum %f\n", tables, total, n, kraft); return 4; }
    for (int t = 0; t < kJpegOptTables; ++t) {
      size_t size = 0;
      if (st_jpeg_optimal_dht(freq, t, nullptr, 0, &size, nullptr) != ST_ERR_INVALID || size != (size_t)(21 + n)) return 5;
      uint8_t* seg = (uint8_t*)malloc(size);
      uint32_t* codes = (uint32_t*)malloc(sizeof(uint32_t) * st_jpeg_opt_tab_words(t));
      if (st_jpeg_optimal_dht(freq, t, seg, size, &size, codes) != ST_OK) return 6;
      if (seg[0] != 0xFF || seg[1] != 0xC4 || seg[4] != st_jpeg_opt_class_id(t) || memcmp(seg + 5, bits, 16) || memcmp(seg + 21, vals, n)) return 7;
      if (size > 1 && st_jpeg_optimal_dht(freq, t, seg, size - 1, &size, codes) != ST_ERR_INVALID) return 8;
      for (int s = 0; s < st_jpeg_opt_tab_words(t); ++s) {
        const uint32_t len = codes[s] >> 16, code = codes[s] & 0xffffu;
        if (len > 16 || (len && code == (1u << len) - 1u)) return 9;   // no code longer than 16 bits, none all ones
      }
      free(seg); free(codes);
    }
    free(freq); free(bits); free(vals);
    ++tables;
  }
  fclose(f);
  // the statistics over coefficient patterns that take every path of the block walk: runs of 16 zeros and more, a last
  // coefficient that is not zero, magnitudes at and beyond the clamps, in both restart modes and at all three samplings
  long stats = 0;
  const int shapes[4][2] = {{8, 8}, {17, 33}, {40, 34}, {9, 200}};
  for (auto& hw : shapes)
    for (int smp = 0; smp < 3; ++smp)
      for (int restart = 0; restart < 2; ++restart) {
        const int hs = smp == 0 ? 1 : 2, vs = smp == 2 ? 2 : 1;
        StJpegEncGeom g;
        st_jpeg_enc_geom(hw[0], hw[1], hs, vs, &g);
        const size_t blocks = (size_t)g.mrows * g.mcols * g.bpm;
        int16_t* coef = (int16_t*)malloc(blocks * 64 * sizeof(int16_t));
        unsigned x = 12345u + (unsigned)stats;
        for (size_t i = 0; i < blocks * 64; ++i) {
          x = x * 1664525u + 1013904223u;
          const unsigned r = x >> 16;
          coef[i] = (r % 7 == 0) ? (int16_t)((int)(r % 4095) - 2047) : (r % 97 == 1) ? (int16_t)32767 : (r % 89 == 2) ? (int16_t)-32768 : 0;
        }
        uint64_t* freq = (uint64_t*)malloc(1024 * sizeof(uint64_t));
        if (st_jpeg_symbol_stats(coef, blocks * 64, hw[0], hw[1], hs, vs, restart, freq) != ST_OK) return 10;
        uint64_t dc = 0;
        for (int s = 0; s < 256; ++s) dc += freq[s] + freq[512 + s];
        if (dc != blocks) return 11;
        for (int s = 12; s < 256; ++s) if (freq[s] || freq[512 + s]) return 12;                  // DC categories 0 .. 11 only
        for (int s = 0; s < 256; ++s) if ((s & 15) > 10 && (freq[256 + s] || freq[768 + s])) return 13;   // AC sizes 1 .. 10 only
        if (st_jpeg_symbol_stats(coef, blocks * 64 - 1, hw[0], hw[1], hs, vs, restart, freq) != ST_ERR_INVALID) return 14;
        for (int t = 0; t < 4; ++t) {
          uint8_t bits[16], vals[256];
          int n = 0;
          if (st_jpeg_optimal_table(freq + 256 * t, bits, vals, &n) != ST_OK || n > ((t & 1) ? 162 : 12)) return 15;
        }
        if (st_jpeg_encode_bound_opt(hw[0], hw[1], hs, vs) != st_jpeg_encode_bound(hw[0], hw[1], hs, vs) + 2 * (long long)blocks) return 16;
        free(coef); free(freq);
        ++stats;
      }
  for (int bad : {2, -1, 1 << 30, -2147483647 - 1})
    for (size_t len : {(size_t)1, (size_t)8, (size_t)160}) {
      char* msg = (char*)malloc(len);
      if (st_jpeg_enc_check_optimize(bad, msg, len) != ST_ERR_INVALID || strlen(msg) >= len) return 17;
      free(msg);
    }
  char msg[160];
  if (st_jpeg_enc_check_optimize(0, msg, sizeof msg) != ST_OK || st_jpeg_enc_check_optimize(1, msg, sizeof msg) != ST_OK || msg[0]) return 18;
  printf("sanitized run ok: %ld tables (%ld beyond 32 bits), %ld statistics\n", tables, refused, stats);
  return 0;
}
'''


def test_host_code_under_address_and_ub_sanitizers(tmp_path, restated):
    """A stand-alone program (its own main, nothing preloaded, no Python inside): st_jpeg_enc_host.cpp and the shared core built
    with -fsanitize=address,undefined, run over the golden histograms and the synthetic ones."""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    (tmp_path / "main.cpp").write_text(SANITIZER_MAIN)
    exe = tmp_path / "jpeg_enc_opt_asan"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "scannertools_amd", "csrc"), str(tmp_path / "main.cpp"),
           os.path.join(ROOT, "scannertools_amd", "csrc", "st_jpeg_enc_host.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr) and "error:" not in build.stderr:
        pytest.skip("no sanitizer runtime: " + build.stderr[-300:])
    assert build.returncode == 0, build.stderr[-4000:]
    hists = [restated[n]["freq"][t].astype(np.uint64) for n in NAMES for t in range(4)] + list(_synthetic().values())
    over = np.zeros(256, np.uint64)
    over[:40] = _fib(40)
    hists.append(over)
    (tmp_path / "hists.bin").write_bytes(b"".join(h.tobytes() for h in hists))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    p = subprocess.run([str(exe), str(tmp_path / "hists.bin")], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0 and "sanitized run ok: %d tables (1 beyond 32 bits), 24 statistics" % len(hists) in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr, p.stderr[-4000:]
    print(p.stdout.strip())
