"""OpticalFlow across the st_fb_params space, without a GPU.

(a) The path table with the parameters as the axis.  tests/test_flow_geometries.py restates the host predicates of
st_farneback.hip; they take the parameters as a dict here, and the predicates the parameters bring in are restated below,
each with the C function it restates: the unfused path's blur kernel and its segments (launch_blur), the expansion
instance (farneback_pass, launch_polyexp, launch_polyexp_ml), the per-level pyramid kernel, its resampling mode and its
LDS tile (pyr_plan, check_pyr_level), the table path (kTabMax) and the buffer every iteration launch reads and writes
(farneback_pass's ping-pong).  MATRIX is the (parameter set, geometry) list tests/test_flow_params_gpu.py runs, case_calls()
the calls it makes of each; test_param_matrix_reaches_every_path asserts that together they reach every entry of
REQUIRED_PARAMS, so a changed threshold makes it fail instead of silently dropping a kernel from the GPU test.

(b) The oracle against the independent float64 derivation (tests/ref_farneback_np.py) at every parameter set of the
matrix, per stage and end to end, with the bounds of test_flow_geometries.py::
test_oracle_against_float64_at_rounded_geometry -- the GPU tests compare with the oracle only, so a misreading of a
parameter shared by the oracle and the kernels would pass there.

(c) The box solve of the oracle against ref.box_solve at every window of the GPU stage test.  Measured (80 x 90, 600 x 24,
20 x 500, 540 x 960, 1080 x 1920): windows >= 9 at most 1.1e-5 px, window 7 2.5e-5, window 5 7.8e-5, window 3 3.5e-4 (a
3 x 3 window leaves the 2 x 2 solve badly conditioned on smooth stretches).  Windows >= 9 are asserted at the stage bound
1e-4; for 3, 5 and 7 the distance is printed, and the GPU test arbitrates with the float64 solve where it exceeds 1e-4.
"""
import math

import numpy as np
import pytest

import oracle
import ref_farneback_np as ref
from test_flow_geometries import (BIG, DEFAULT_WS_LIMIT, NUM_CUS, fused_path, geom, iter_plan, levels, param, pass_bytes, paths,
                                  plan_passes, poly_u8, pyr_fused_ok, single)
from util import translated_rgb_pair

K_TAB_MAX = 40                                               # kTabMax: tables of up to 40 frames / pairs ride in the launch arguments
K_MAX_TAPS = 32                                              # kMaxTaps: a level's Gaussian has at most 31 taps
PYR_OW, PYR_OH, PYR_LDS_MAX = 32, 8, 64 * 1024               # k_pyr's output tile, kPyrLdsMax
BLUR_T = 256                                                 # k_blur_update's workgroup

# ---------------------------------------------------------------- the parameter sets and the matrix of the GPU file
POLY7 = dict(poly_n=7, poly_sigma=1.5)
P_FUSED = {
    "iters1": dict(num_iters=1), "iters2": dict(num_iters=2), "iters5": dict(num_iters=5),
    "levels0": dict(num_levels=0), "levels1": dict(num_levels=1),
    "scale0.75/levels3": dict(pyr_scale=0.75, num_levels=3), "scale0.8/levels6": dict(pyr_scale=0.8, num_levels=6),
    "scale0.3/levels1": dict(pyr_scale=0.3, num_levels=1),
    "poly7": dict(POLY7), "gray14": dict(gray_bits=14),
    "poly7+scale0.6/levels3+iters2": dict(POLY7, pyr_scale=0.6, num_levels=3, num_iters=2),
}
P_UNFUSED = {
    "win3": dict(win_size=3), "win13": dict(win_size=13), "win17": dict(win_size=17), "win19": dict(win_size=19),
    "win33": dict(win_size=33), "win63": dict(win_size=63), "win9/iters2": dict(win_size=9, num_iters=2),
    "win21+poly7+scale0.7/levels5+iters4": dict(POLY7, win_size=21, pyr_scale=0.7, num_levels=5, num_iters=4),
}
P = dict(P_FUSED, **P_UNFUSED)

G1080, G480, G203 = (1080, 1920), (480, 854), (203, 317)
# every fused set at all three geometries; the unfused sets at the two smaller ones, and at 1080p (many segments, eight
# strips) the window extremes and the combined set
MATRIX = ([(n, g) for n in P_FUSED for g in (G1080, G480, G203)] +
          [(n, g) for n in P_UNFUSED for g in (G480, G203)] +
          [(n, G1080) for n in ("win3", "win63", "win21+poly7+scale0.7/levels5+iters4")])
SINGLES = [(0, 1), (16, 17), (5, 3), (7, 7)]
TAB = [(i, i + 1) for i in range(33)] + [(5, 3), (7, 7)] + [(i + 2, i) for i in range(10)]   # 45 pairs: tables in device memory
TAB_CASES = [("iters2", G203), ("win13", G203)]
SPLIT_CASES = [("scale0.75/levels3", G480), ("win17", G480)]
# pairs of the 35-pair call compared with the oracle; one at 1080p (the oracle's and, on a miss, the float64 run time)
ORACLE_PAIRS = {G1080: [16], G480: [0, 16, 32], G203: [0, 16, 32]}


def case_calls(name, g):
    """The calls the GPU file makes of one (parameter set, geometry): call name -> (pairs, workspace limit)."""
    c = {"33+2": (BIG, DEFAULT_WS_LIMIT), "8": (BIG[:8], DEFAULT_WS_LIMIT)}
    for p in SINGLES:
        c["1:%d,%d" % p] = ([p], DEFAULT_WS_LIMIT)
    if (name, g) in TAB_CASES:
        c["45"] = (TAB, DEFAULT_WS_LIMIT)
    if (name, g) in SPLIT_CASES:
        c["split"] = (BIG, split_limit(g[0], g[1], P[name]))
    return c


def split_limit(h, w, params):
    """The workspace limit of the pass-splitting calls: what a pass of 9 pairs on 10 frames needs, so that the 35 pairs
    (34 frames) go 35 -> 18 -> 9 and on in at least four passes."""
    return pass_bytes(h, w, 10, 9, params)


# ---------------------------------------------------------------- restated host predicates the parameters bring in
def blur_plan(h, w, win, num_cus=NUM_CUS):
    """launch_blur for one level of the unfused path: (kernel, rows per segment, segments).  m == 7 (a 15 x 15 window on a
    degenerate frame) takes k_blur_update_v2<7>, whole 15-row ring periods; every other radius k_blur_update with
    rows_per_segment(h, strips, 1, 2 m + 1), strips of BLUR_T - 2 m columns -- neither depends on the pair count."""
    m = win // 2
    if m == 7:
        strips = (w + 240 - 1) // 240
        segs = (num_cus * 4 + strips - 1) // strips
        rows = ((h + segs - 1) // segs + 14) // 15 * 15
        rows = max(rows, 15)
        if rows > 135 and h > 135:
            rows = 135
        return "blur_v2", rows, (h + rows - 1) // rows
    strips = (w + (BLUR_T - 2 * m) - 1) // (BLUR_T - 2 * m)
    segs = max(1, (num_cus * 8 + strips - 1) // strips)
    rows = min(h, max((h + segs - 1) // segs, 4 * (2 * m + 1)))
    return "blur_general", rows, (h + rows - 1) // rows


def polyexp_instance(h, w, npairs, params=None):
    """(poly_n, launch form): 'ml' -- all levels in one k_polyexp_ml launch (single); else k_polyexp per level, level 0
    through 'u8' (k_polyexp_u8, from the gray frames) where poly_u8 holds."""
    n = param(params, "poly_n")
    if single(h, w, npairs, params):
        return n, "ml"
    return n, "u8" if poly_u8(h, w, npairs, params) else "per_level"


def pyr_plan(h, w, k, params=None):
    """pyr_plan: the kernel that builds level k where the one-pass pyramid does not apply, and k_pyr's LDS tile.
    -> (kernel / mode, kernel size, LDS bytes): 'pyr0' (level 0 streamed), 'dec2' / 'dec4' / 'dec8' (exact decimation with
    the reference's 3 / 9 / 19 taps), else k_pyr in mode 'COPY', 'AREA2' or 'LINEAR'."""
    lh, lw, _, ks = geom(h, w, k, params)
    if (lh, lw) == (h, w) and ks == 3 and h >= 2 and w >= 8:
        return "pyr0", ks, 0
    for s, t in ((2, 3), (4, 9), (8, 19)):
        if (h, w) == (s * lh, s * lw) and ks == t:
            return "dec%d" % s, ks, 0
    mode = "COPY" if (lh, lw) == (h, w) else "AREA2" if (h, w) == (2 * lh, 2 * lw) else "LINEAR"
    sx, sy = 1.0 / (lw / w), 1.0 / (lh / h)
    r = ks // 2
    rows = math.ceil((PYR_OH - 1) * sy) + 3 + 2 * r + 1
    cols = (math.ceil((PYR_OW - 1) * sx) + 3 + 2 * r + 1 + 3) // 4 * 4
    return mode, ks, 4 * rows * 2 * PYR_OW + rows * cols


def pyr_level_ok(h, w, k, params=None):
    """check_pyr_level: at most 31 taps, and k_pyr's tile within 64 KiB of LDS."""
    _, ks, lds = pyr_plan(h, w, k, params)
    return ks <= K_MAX_TAPS - 1 and lds <= PYR_LDS_MAX


def supported(h, w, params=None):
    """check_params' pyramid test: every level of the call can be built."""
    return all(pyr_level_ok(h, w, k, params) for k in range(levels(h, w, params) + 1))


def param_paths(h, w, pairs, ws_limit=DEFAULT_WS_LIMIT, params=None):
    """paths() of test_flow_geometries.py plus the names the parameters bring in."""
    got = set(paths(h, w, pairs, ws_limit, params))
    L = levels(h, w, params)
    fused = fused_path(h, w, params)
    win, iters = param(params, "win_size"), param(params, "num_iters")
    passes = plan_passes(h, w, pairs, ws_limit, params)
    for frames, npairs in passes:
        n, form = polyexp_instance(h, w, npairs, params)
        if n == 7:
            got.add("poly7:" + form)
            if form == "u8":
                got.add("poly7:per_level")                   # levels 1.. of the same pass
        if param(params, "gray_bits") == 14 and pyr_fused_ok(h, w, params):
            got.add("gray14:fused_pyr")
        if not pyr_fused_ok(h, w, params):
            for k in range(L + 1):
                mode, ks, _ = pyr_plan(h, w, k, params)
                got.add("pyr:%s:k%d" % (mode, ks) if mode in ("COPY", "AREA2", "LINEAR") else "pyr:" + mode)
        tab_dev = len(frames) > K_TAB_MAX or npairs > K_TAB_MAX
        if fused:
            got.add("fused:iters%d" % iters)
            got.add("fused:levels%d" % L if L <= 3 else "fused:levels>3")
            if tab_dev:
                got.add("fused:tables_dev")
            for q in iter_plan(h, w, npairs, params):
                if q["src"] == "FLOW_COARSE" and abs(q["ratio"] - 2) > 0.1:
                    if q["kern"] == "tile":
                        got.add("tile:FLOW_COARSE:ratio!=2")
                    else:
                        got.add("march:FLOW_COARSE:ratio" + ("<2" if q["ratio"] < 2 else ">2"))
                if q["writes"] == "flow_ptrs" and q["src"] != "FLOW_FIELD":
                    got.add("fused:out_from_" + q["src"])    # num_iters 1: the transition launch writes the caller's frames
        else:
            if tab_dev:
                got.add("unfused:tables_dev")
            if len(passes) >= 3:
                got.add("unfused:split")
            for k in range(L + 1):
                lh, lw = geom(h, w, k, params)[:2]
                kern, rows, nseg = blur_plan(lh, lw, win)
                got.add("unfused:%s:m%d" % (kern, win // 2) if kern == "blur_general" else "unfused:" + kern)
                if nseg > 8 and npairs > 1:
                    got.add("unfused:multi_segment")
    return got


def param_matrix():
    """(parameter set, geometry, call) -> paths, for every call of tests/test_flow_params_gpu.py."""
    m = {}
    for name, (h, w) in MATRIX:
        for call, (pairs, limit) in case_calls(name, (h, w)).items():
            m[(name, h, w, call)] = param_paths(h, w, pairs, limit, P[name])
    return m


REQUIRED_PARAMS = ({"fused:iters1", "fused:iters2", "fused:iters5", "fused:levels0", "fused:levels1", "fused:levels>3",
                    "fused:out_from_FLOW_COARSE", "fused:out_from_FLOW_COARSE2", "fused:tables_dev",
                    "march:FLOW_COARSE:ratio<2", "march:FLOW_COARSE:ratio>2", "tile:FLOW_COARSE:ratio!=2",
                    "poly7:ml", "poly7:per_level", "poly7:u8",
                    "unfused:multi_segment", "unfused:tables_dev", "unfused:split",
                    "pyr:LINEAR:k3", "pyr:LINEAR:k5", "pyr:LINEAR:k7", "pyr:LINEAR:k9", "pyr:LINEAR:k13", "pyr:LINEAR:k19",
                    "gray14:fused_pyr"} |
                   {"unfused:blur_general:m%d" % m for m in (1, 6, 8, 9, 10, 16, 31)})


def test_param_matrix_reaches_every_path():
    m = param_matrix()
    missing = REQUIRED_PARAMS - set().union(*m.values())
    assert not missing, missing
    # every set the fused path accepts goes to 1080p in a call large enough to march at level 0
    for name in P_FUSED:
        assert any(p.startswith("L0:iter3") or p.startswith("L0:roles") for p in m[(name, 1080, 1920, "33+2")]), name
    # the matrix keeps to what check_params accepts, and to the path its name says
    for name, (h, w) in MATRIX:
        assert supported(h, w, P[name]), (name, h, w)
        assert fused_path(h, w, P[name]) == (name in P_FUSED), (name, h, w)


def test_param_predicates_known_cases():
    """Spot values of the restated predicates, worked by hand from the C lines."""
    # fused_path: the window alone decides at these sizes
    assert fused_path(1080, 1920) and fused_path(203, 317, dict(num_iters=5)) and not fused_path(1080, 1920, dict(win_size=13))
    # levels: 1080 * 0.8^6 = 283 >= 32; 1080 * 0.3 = 324, * 0.09 = 97; 203 * 0.3^2 = 18 < 32
    assert levels(1080, 1920, dict(pyr_scale=0.8, num_levels=6)) == 6 and levels(1080, 1920, dict(pyr_scale=0.3, num_levels=2)) == 2
    assert levels(203, 317, dict(pyr_scale=0.3, num_levels=2)) == 1 and levels(1080, 1920, dict(num_levels=0)) == 0
    # level sizes: 1080 * 0.75 = 810, * 0.5625 = 607.5 -> 608 (half to even); 1920 * 0.3 = 576
    assert [geom(1080, 1920, k, dict(pyr_scale=0.75))[:2] for k in (1, 2)] == [(810, 1440), (608, 1080)]
    assert geom(1080, 1920, 1, dict(pyr_scale=0.3))[:2] == (324, 576)
    # kernel sizes: sigma = (1 / scale - 1) / 2, size = max(3, cvRound(5 sigma) | 1): 0.3 -> 1.1667 -> 5.83 -> 6 | 1 = 7;
    # 0.09 -> 5.06 -> 25.3 -> 25; 0.6^3 -> 1.815 -> 9.07 -> 9; 0.7^5 -> 2.475 -> 12.4 -> 12 | 1 = 13
    assert geom(1080, 1920, 1, dict(pyr_scale=0.3))[3] == 7 and geom(1080, 1920, 2, dict(pyr_scale=0.3))[3] == 25
    assert geom(1080, 1920, 3, dict(pyr_scale=0.6))[3] == 9 and geom(1080, 1920, 5, dict(pyr_scale=0.7))[3] == 13
    # k_pyr's tile at 1080p, pyr_scale 0.3 level 2 (97 x 173: ratios 11.13 / 11.10, r = 12):
    # rows = ceil(7 * 11.134) + 3 + 24 + 1 = 106, cols = (ceil(31 * 11.098) + 3 + 24 + 1 + 3) / 4 * 4 = 376
    # -> 4 * 106 * 64 + 106 * 376 = 66 992 > 65 536: refused; level 1 (ratio 3.33, r = 3): 34 rows x 116 -> 12 648
    assert pyr_plan(1080, 1920, 2, dict(pyr_scale=0.3)) == ("LINEAR", 25, 66992)
    assert pyr_plan(1080, 1920, 1, dict(pyr_scale=0.3)) == ("LINEAR", 7, 4 * 34 * 64 + 34 * 116)
    assert not supported(1080, 1920, dict(pyr_scale=0.3, num_levels=2)) and supported(1080, 1920, dict(pyr_scale=0.3, num_levels=1))
    # pyr_scale 0.45 level 3 (98 x 175, ratios 11.02 / 10.97, r = 12): 106 rows x 372 -> 27 136 + 39 432 = 66 568
    assert pyr_plan(1080, 1920, 3, dict(pyr_scale=0.45))[1:] == (25, 66568)
    assert pyr_plan(1080, 1920, 5, dict(pyr_scale=0.6))[1] == 31 and not pyr_level_ok(1080, 1920, 5, dict(pyr_scale=0.6))
    assert pyr_plan(1080, 1920, 7, dict(pyr_scale=0.7))[1] == 29 and not pyr_level_ok(1080, 1920, 7, dict(pyr_scale=0.7))
    # the deepest level that can be built at 1080p, as the header lists them
    for sc, deepest in ((0.3, 1), (0.45, 2), (0.5, 3), (0.6, 4), (0.7, 6), (0.75, 8), (0.8, 10)):
        prm = dict(pyr_scale=sc, num_levels=deepest + 1)
        assert levels(1080, 1920, prm) == deepest + 1 and not supported(1080, 1920, prm), sc
        assert supported(1080, 1920, dict(pyr_scale=sc, num_levels=deepest)), sc
    # above 31 taps: 0.5^4 -> sigma 7.5 -> 37.5 -> 38 (half to even) | 1 = 39
    assert geom(2160, 4096, 4, dict(num_levels=4))[3] == 39 and not supported(2160, 4096, dict(num_levels=4))
    # the default pyramid off the one-pass geometry: dec2, then LINEAR where a side rounds (854 / 4 = 213.5 -> 214)
    assert [pyr_plan(480, 854, k)[0] for k in range(4)] == ["pyr0", "dec2", "LINEAR", "LINEAR"] and pyr_plan(480, 854, 3)[1] == 19
    # the unfused blur: radius 1 at 1080p -- 8 strips of 254, 256 segments wanted -> 5 rows, floor 4 * 3 = 12 -> 90 segments
    assert blur_plan(1080, 1920, 3) == ("blur_general", 12, 90)
    # radius 31: strips of 194 -> 10; 205 segments wanted -> 6 rows, floor 4 * 63 = 252 -> 5 segments
    assert blur_plan(1080, 1920, 63) == ("blur_general", 252, 5)
    assert blur_plan(203, 317, 63) == ("blur_general", 203, 1) and blur_plan(600, 24, 15)[0] == "blur_v2"
    # expansion instance at 1080p: up to 16 pairs one multi-level launch, above that level 0 from the gray frames
    assert polyexp_instance(1080, 1920, 8, POLY7) == (7, "ml") and polyexp_instance(1080, 1920, 35, POLY7) == (7, "u8")
    assert polyexp_instance(480, 854, 35, POLY7) == (7, "per_level") and polyexp_instance(1080, 1920, 35, dict(POLY7, pyr_scale=0.6)) == (7, "per_level")
    # the ping-pong: one iteration -- the transition launch is the last, coarse buffer 0 -> 1 -> 0 ... -> the output frames
    one = iter_plan(1080, 1920, 35, dict(num_iters=1))
    assert [(q["src"], q["reads"], q["writes"]) for q in one] == [
        ("FLOW_ZERO", None, "cflow1"), ("FLOW_COARSE2", "cflow1", "cflow0"), ("FLOW_COARSE2", "cflow0", "cflow1"),
        ("FLOW_COARSE2", "cflow1", "flow_ptrs")]
    five = [q for q in iter_plan(1080, 1920, 35, dict(num_iters=5)) if q["k"] == 0]
    assert [(q["reads"], q["writes"]) for q in five] == [("cflow1", "fbuf0"), ("fbuf0", "fbuf1"), ("fbuf1", "fbuf0"),
                                                         ("fbuf0", "fbuf1"), ("fbuf1", "flow_ptrs")]
    two = [q for q in iter_plan(1080, 1920, 35, dict(num_iters=2)) if q["k"] == 0]
    assert [(q["reads"], q["writes"]) for q in two] == [("cflow1", "fbuf0"), ("fbuf0", "flow_ptrs")]
    # ratios of the coarse source: 1080 over 810 over 608 (0.75), 1080 over 324 (0.3)
    r = [q["ratio"] for q in iter_plan(1080, 1920, 35, dict(pyr_scale=0.75)) if q["ratio"]]
    assert [round(x, 3) for x in r] == [round(608 / 456, 3), round(810 / 608, 3), round(1080 / 810, 3)]
    assert [q["src"] for q in iter_plan(1080, 1920, 35, dict(pyr_scale=0.3, num_levels=1)) if q["ratio"]] == ["FLOW_COARSE"]
    # pass_bytes counts five planes per M field on the unfused path: 2 * 3 more planes per pair
    assert pass_bytes(480, 854, 10, 9, dict(win_size=17)) - pass_bytes(480, 854, 10, 9) == 2 * 3 * 4 * 480 * 854 * 9
    # 45 pairs: tables through device memory (kTabMax = 40)
    assert "unfused:tables_dev" in param_paths(203, 317, TAB, params=P["win13"]) and len(TAB) == 45
    assert "unfused:tables_dev" not in param_paths(203, 317, BIG, params=P["win13"])


@pytest.mark.parametrize("name,g", SPLIT_CASES)
def test_split_limit_makes_three_passes(name, g):
    h, w = g
    limit = split_limit(h, w, P[name])
    passes = plan_passes(h, w, BIG, limit, P[name])
    assert len(passes) >= 3 and sum(c for _, c in passes) == len(BIG), passes
    assert len(plan_passes(h, w, BIG, params=P[name])) == 1
    assert all(pass_bytes(h, w, len(f), c, P[name]) <= limit for f, c in passes)


def test_report_param_paths():
    """The paths each (parameter set, geometry, call) takes (pytest -s shows it)."""
    for (name, h, w, call), p in param_matrix().items():
        print("%-36s %4dx%-4d %-6s %s" % (name, h, w, call, " ".join(sorted(p))))


# ---------------------------------------------------------------- the library's level geometry at every set
STAGE_SCALES = [dict(pyr_scale=s, num_levels=6) for s in (0.3, 0.45, 0.6, 0.75, 0.8)]


@pytest.mark.parametrize("h,w", [G1080, G480, G203, (264, 328), (240, 426), (61, 1027)])
def test_level_shapes_agree_at_every_set(h, w):
    """levels_for / level_shape of the float64 derivation == the oracle's fb_levels / fb_level_geom == the library's, for
    every parameter set of the matrix and of the pyramid stage test."""
    from scannertools_amd import hip
    for prm in list(P.values()) + STAGE_SCALES:
        sc, nl = param(prm, "pyr_scale"), param(prm, "num_levels")
        o, lp = oracle.default_params(**prm), hip.default_params(**prm)
        L = oracle.fb_levels(h, w, o)
        assert ref.levels_for(h, w, nl, sc) == L == hip.fb_levels(h, w, lp), prm
        for k in range(L + 1):
            want = oracle.fb_level_geom(h, w, k, o)
            assert ref.level_shape(h, w, k, sc) == want[:2], (prm, k, want)
            assert hip.fb_level_geom(h, w, k, lp) == want, (prm, k)


# ---------------------------------------------------------------- (b) oracle vs float64 at every parameter set
def _f64(g0, g1, prm):
    return ref.farneback(g0, g1, num_levels=param(prm, "num_levels"), pyr_scale=param(prm, "pyr_scale"), win=param(prm, "win_size"),
                         iters=param(prm, "num_iters"), poly_n=param(prm, "poly_n"), poly_sigma=param(prm, "poly_sigma"))


@pytest.mark.parametrize("h,w", [(203, 317), (264, 328)])
@pytest.mark.parametrize("name", list(P))
def test_oracle_against_float64_at_parameter_set(name, h, w):
    """Pyramid image of every level, the expansion, UpdateMatrices and the box solve at the set's parameters (2e-4 per
    stage, 1e-4 for the matrices and -- windows >= 9 -- the solve), then the flow end to end: relative L2 2e-4, 2e-3 px."""
    prm = P[name]
    o = oracle.default_params(**prm)
    sc, win, pn, ps = (param(prm, k) for k in ("pyr_scale", "win_size", "poly_n", "poly_sigma"))
    f0, f1 = translated_rgb_pair(21, h, w, 3, -2)
    bits = param(prm, "gray_bits")
    g0, g1 = oracle.gray_u8(f0, bits), oracle.gray_u8(f1, bits)
    L = oracle.fb_levels(h, w, o)
    assert ref.levels_for(h, w, param(prm, "num_levels"), sc) == L
    rng = np.random.default_rng(3)
    worst = {}
    for k in range(L + 1):
        I, I_r = oracle.fb_pyr_image(g0, k, o), ref.pyramid_image(g0, k, sc)
        assert I.shape == I_r.shape and np.abs(I - I_r).max() <= 2e-4, k
        R_o, R_r = oracle.polyexp(I, pn, ps), ref.poly_expansion(I.astype(np.float64), pn, ps)
        assert np.abs(R_o - R_r).max() <= 2e-4 * max(1.0, np.abs(R_r).max()), k
        R1_o = oracle.polyexp(oracle.fb_pyr_image(g1, k, o), pn, ps)
        fl = (rng.standard_normal(I.shape + (2,)) * 2).astype(np.float32)
        M_o = oracle.update_matrices(R_o, R1_o, fl)
        M_r = ref.update_matrices(R_o.astype(np.float64), R1_o.astype(np.float64), fl.astype(np.float64))
        assert np.abs(M_o - M_r).max() <= 1e-4 * max(1.0, np.abs(M_r).max()), k
        flow_o, _ = oracle.update_flow_blur(R_o, R1_o, M_o, win, False)
        d = float(np.abs(flow_o - ref.box_solve(M_o.astype(np.float64), win)).max())
        worst[k] = d
        if win >= 9:
            assert d <= 1e-4, (k, d)
    got, want = oracle.farneback(g0, g1, o), _f64(g0, g1, prm)
    rel, mx = float(np.linalg.norm(got - want) / np.linalg.norm(want)), float(np.abs(got - want).max())
    print("%s %dx%d: box solve vs float64 per level %s; flow rel L2 %.2e max-abs %.2e" % (name, h, w, {k: "%.1e" % v for k, v in worst.items()}, rel, mx))
    assert rel <= 2e-4 and mx <= 2e-3
    inner = got[40:-40, 40:-40]
    assert abs(np.median(inner[..., 0]) - 3) < 0.05 and abs(np.median(inner[..., 1]) + 2) < 0.05


# ---------------------------------------------------------------- (c) the oracle's box solve at every window
BLUR_WINDOWS = [3, 5, 7, 9, 13, 15, 17, 19, 33, 63]
BLUR_SIZES = [(80, 90), (600, 24), (20, 500), (540, 960), (1080, 1920)]
_blur_cache = {}


def blur_inputs(h, w):
    """R0, R1 (oracle expansions of a translated pair's gray frames) and M = UpdateMatrices at zero flow, (h, w, 5)."""
    if (h, w) not in _blur_cache:
        _blur_cache.clear()                                  # one size at a time (1080p: 170 MB)
        f0, f1 = translated_rgb_pair(h + 2, h, w, 2, -1)
        R0 = oracle.polyexp(oracle.gray_u8(f0).astype(np.float32))
        R1 = oracle.polyexp(oracle.gray_u8(f1).astype(np.float32))
        _blur_cache[(h, w)] = (R0, R1, oracle.update_matrices(R0, R1, np.zeros((h, w, 2), np.float32)))
    return _blur_cache[(h, w)]


@pytest.mark.parametrize("h,w", BLUR_SIZES)
def test_oracle_box_solve_against_float64(h, w):
    R0, R1, M = blur_inputs(h, w)
    for win in BLUR_WINDOWS:
        flow_o, _ = oracle.update_flow_blur(R0, R1, M, win, False)
        d = float(np.abs(flow_o - ref.box_solve(M.astype(np.float64), win)).max())
        print("box solve, oracle vs float64, %dx%d window %d: %.2e px" % (h, w, win, d))
        if win >= 9:
            assert d <= 1e-4, (win, d)


def test_oracle_window_1_is_not_a_box_filter():
    """Why win_size 1 is refused: at radius 0 the reference's running sums (restated in oracle.c) start from twice row 0 /
    column 0, so its 'box sum' at (y, x) is M[y, x] + M[y, 0] + M[0, x] + M[0, 0] -- not the 1 x 1 mean; the flow it then
    solves for is at relative L2 ~1 from the float64 derivation's."""
    h, w = 80, 90
    R0, R1, M = blur_inputs(h, w)
    flow_o, _ = oracle.update_flow_blur(R0, R1, M, 1, False)
    Md = M.astype(np.float64)
    S = Md + Md[:, :1] + Md[:1, :] + Md[:1, :1]
    g11, g12, g22, h1, h2 = [S[..., c] for c in range(5)]
    idet = 1.0 / (g11 * g22 - g12 * g12 + 1e-3)
    art = np.stack([(g11 * h2 - g12 * h1) * idet, (g22 * h1 - g12 * h2) * idet], -1)
    assert np.abs(flow_o - art).max() <= 1e-3 * max(1.0, np.abs(art).max())
    assert np.abs(flow_o - ref.box_solve(Md, 1)).max() > 0.1
