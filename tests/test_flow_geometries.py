"""Flow geometries off the 1080p / 4K landscape grid, without a GPU.

(a) The path table.  st_farneback.hip's host code picks a different launch shape for nearly every frame geometry and batch
size; the predicates it picks by are restated here (each with the C lines it restates), and every (geometry, call) case of
tests/test_geometries_gpu.py names the paths it takes.  test_path_matrix_reaches_every_path asserts that the matrix as a
whole reaches each path, so a changed threshold makes it fail instead of silently dropping a path from the GPU test.

(b) The oracle against the independent float64 derivation (tests/ref_farneback_np.py) at sizes whose pyramid levels round
(cvRound: halves to even), per stage and end to end, with the bounds of
test_oracle.py::test_farneback_oracle_against_independent_float64_derivation (264 x 328, every level exact).
ref_farneback_np gained two things for this.  level_shape(): the level size pyramid_image already computed inline, so
that the level shapes of the 4K and 1080p geometries are checked without building a float64 pyramid of them.  And the
sample positions of its bilinear resampling are now cv::resize's, rounded to float32 (_bilinear_taps): at 480 x 854 the
pyramid image of level 2 (120 x 214, ratio 3.99) differed from the oracle by 3.6e-4 with torch's exact positions, over the
2e-4 bound, and by 4.4e-5 with cv::resize's -- the difference was the position rounding that the reference itself
performs (largest where the image is steepest, growing with the column index), not an error of the oracle.
"""
import numpy as np
import pytest

import oracle
import ref_farneback_np as ref
from util import translated_rgb_pair

# geometries of tests/test_geometries_gpu.py, (rows, columns)
GEOMETRIES = [(1920, 1080), (480, 854), (720, 1280), (360, 640), (1080, 1440), (1079, 1919), (2160, 4096)]
N_FRAMES = 34
BIG = [(i, i + 1) for i in range(33)] + [(5, 3), (7, 7)]     # 33 consecutive pairs + frame-slot de-duplication
SPLIT_GEOMETRIES = [(480, 854), (1079, 1919)]

NUM_CUS = 256                                                # MI355X
DEFAULT_WS_LIMIT = 64 << 30                                  # st_context.hip: ws_limit when none is set

# csrc/st_farneback.hip constants
PE_OUT = 240                                                 # :1122 polynomial-expansion strip
B2_OUT, B2_HALO = 240, 8                                     # :1672 iteration strip, halo
F3_ANCHOR = 32                                               # :1951
FR_G = 4                                                     # :2328
FT_T = 32                                                    # :2633 tile side
K_TILE_PX = 600000                                           # :3070


def calls(h, w):
    """The calls test_geometries_gpu.py makes at (h, w): name -> pair list (all on one 34-frame tensor)."""
    c = {"33+2": BIG, "8": BIG[:8]}
    for p in ((0, 1), (16, 17), (32, 33), (5, 3), (7, 7)):
        c["1:%d,%d" % p] = [p]
    return c


# ---------------------------------------------------------------- restated host predicates
# Every predicate takes an optional `params`: a dict of st_fb_params fields that differ from st_fb_params_default()
# (tests/test_flow_params.py walks that axis); None is the reference's (3, 0.5, 15, 3, 5, 1.2), gray_bits 15.
DEFAULT_PARAMS = dict(num_levels=3, pyr_scale=0.5, win_size=15, num_iters=3, poly_n=5, poly_sigma=1.2, gray_bits=15)


def param(params, name):
    return (params or {}).get(name, DEFAULT_PARAMS[name])


def _op(params):
    return oracle.default_params(**params) if params else None


def levels(h, w, params=None):
    return oracle.fb_levels(h, w, _op(params))               # fb_levels :49


def geom(h, w, k, params=None):
    return oracle.fb_level_geom(h, w, k, _op(params))        # fb_level_geom :59 -> (lh, lw, sigma, ksize)


def pyr_fused_ok(h, w, params=None):
    """pyr_fused_ok: exactly 3 levels, sides multiples of 8, every level exactly halved, kernel sizes 3 / 3 / 9 / 19."""
    if levels(h, w, params) != 3 or h & 7 or w & 7:
        return False
    for k, ks in enumerate((3, 3, 9, 19)):
        lh, lw, _, ksize = geom(h, w, k, params)
        if lh != h >> k or lw != w >> k or ksize != ks:
            return False
    return True


def fused_path(h, w, params=None):
    """fused_path: the fused iteration kernels take the 15 x 15 window on frames whose every level is at least 2 x 2;
    every other window goes through k_update_matrices + the blur kernel with materialised M."""
    if param(params, "win_size") != 15:
        return False
    return all(min(geom(h, w, k, params)[:2]) >= 2 for k in range(levels(h, w, params) + 1))


def pyr_strip_w(w):
    """:2945-2946: the one-pass pyramid's equal strips of at most 1024 columns, rounded up to 8."""
    strips = (w + 1023) // 1024
    return strips, ((w + strips - 1) // strips + 7) // 8 * 8


def single(h, w, npairs, params=None):
    """:3279: all levels' expansions in one launch (one-pass pyramid, up to 16 pairs)."""
    return pyr_fused_ok(h, w, params) and 1 <= levels(h, w, params) <= 3 and npairs <= 16


def poly_u8(h, w, npairs, params=None):
    """:3280-3281 in the default context (ST_POLY_U8 on, role-split pyramid on, gray not folded): level 0 expanded from
    the gray frames."""
    pyr_rgb = False                                          # :3270, fold_gray is off by default
    lh, lw, sigma, ksize = geom(h, w, 0, params)
    return (pyr_fused_ok(h, w, params) and not pyr_rgb and not single(h, w, npairs, params) and ksize == 3 and sigma <= 0
            and (lh, lw) == (h, w) and w >= 8)


def aligned4(h, w, frame_ids):
    """:3264-3265 for frames of one contiguous (n, h, w, 3) uint8 tensor (base 256-byte aligned): every frame of the
    pass starts on a 4-byte boundary."""
    return all((i * 3 * h * w) % 4 == 0 for i in frame_ids)


def iter_kernel(h, w, n_pairs, coarse, num_cus=NUM_CUS):
    """launch_flow_iter :3063-3172 in the default context (lone instance): 'tile', 'roles4' / 'roles5' or 'iter3'."""
    if n_pairs * h * w <= K_TILE_PX and (h + FT_T - 1) // FT_T <= 65535:
        return "tile"
    strips = (w + B2_OUT - 1) // B2_OUT
    resident = num_cus * 2
    periods = (h + F3_ANCHOR - 1) // F3_ANCHOR
    rounds3 = wgs3 = 1
    best = 1e300
    for segs in range(1, periods + 1):
        r = (periods + segs - 1) // segs * F3_ANCHOR
        nseg = (h + r - 1) // r
        wgs = strips * n_pairs * nseg
        rounds = (wgs + resident - 1) // resident
        cost = float(rounds) * (r + 15)
        if cost < best * 0.999:
            best, rounds3, wgs3 = cost, rounds, wgs
    roles_limit = resident * 62 // 100 if coarse else resident * 95 // 100
    if rounds3 == 1 and wgs3 < roles_limit:
        best_ncw, bestr = 0, 1e300
        for ncw in (5, 4):
            outmax = 64 * ncw - 2 * B2_HALO
            rstrips = (w + outmax - 1) // outmax
            for segs in range(1, periods + 1):
                r = (periods + segs - 1) // segs * F3_ANCHOR
                nseg = (h + r - 1) // r
                wgs = rstrips * n_pairs * nseg
                rounds = (wgs + num_cus - 1) // num_cus
                cost = float(rounds) * (r + 16 + 3 * FR_G) * (1.3 if ncw == 5 else 1.0)
                if cost < bestr * 0.999:
                    bestr, best_ncw = cost, ncw
        if best_ncw:
            return "roles%d" % best_ncw
    return "iter3"


def iter_plan(h, w, npairs, params=None):
    """Every launch_flow_iter of one pass (fused path, num_iters iterations per level, coarse to fine), as
    farneback_pass's loop issues them: a dict per launch with the level `k`, the iteration `it`, the kernel `kern`, the
    source instance `src` (as chosen in launch_flow_iter; the tile kernel has one coarse instance, FLOW_COARSE), the
    buffer it reads (`reads`: None, "cflow<i>" or "fbuf<i>"), the buffer it writes (`writes`: "fbuf<i>", "cflow<i>" or
    "flow_ptrs", the caller's output frames) and, for a coarse source, the upsampling `ratio` (rows over coarse rows)."""
    L = levels(h, w, params)
    iters = param(params, "num_iters")
    out = []
    cur = 0                                                  # cflow[cur] holds the coarser level's flow
    for k in range(L, -1, -1):
        lh, lw, _, _ = geom(h, w, k, params)
        for it in range(iters):
            coarse = it == 0 and k < L
            last = it == iters - 1
            kern = iter_kernel(lh, lw, npairs, coarse)
            ratio = None
            if coarse:
                ch = geom(h, w, k + 1, params)[0]
                src = "FLOW_COARSE" if kern == "tile" or lh != 2 * ch else "FLOW_COARSE2"
                reads, ratio = "cflow%d" % cur, lh / ch
            elif it > 0:
                src, reads = "FLOW_FIELD", "fbuf%d" % ((it - 1) & 1)
            else:
                src, reads = "FLOW_ZERO", None
            writes = ("flow_ptrs" if k == 0 else "cflow%d" % (cur ^ 1)) if last else "fbuf%d" % (it & 1)
            out.append(dict(k=k, it=it, kern=kern, src=src, reads=reads, writes=writes, ratio=ratio))
        cur ^= 1
    return out


def iter_launches(h, w, npairs, params=None):
    """(level, kernel, source) of every launch of iter_plan."""
    return [(q["k"], q["kern"], q["src"]) for q in iter_plan(h, w, npairs, params)]


def align_up(v, a=256):
    return (v + a - 1) // a * a


def pass_bytes(h, w, nf, npairs, params=None):
    """pass_bytes: two flow fields per pair on the fused iteration path, two five-plane M fields on the unfused one."""
    L = levels(h, w, params)
    np0 = h * w
    npk = [geom(h, w, k, params)[0] * geom(h, w, k, params)[1] for k in range(L + 1)]
    max_coarse = max(npk[1:], default=0)
    b = align_up(np0 * nf) + align_up(4 * np0 * nf)
    if pyr_fused_ok(h, w, params):
        b += sum(align_up(4 * (np0 >> (2 * k)) * nf) for k in (1, 2, 3))
    b += sum(align_up(4 * 5 * n * nf) for n in npk)
    b += 2 * align_up(4 * (2 if fused_path(h, w, params) else 5) * np0 * npairs)
    b += 2 * align_up(4 * 2 * (max_coarse or 1) * npairs)
    b += align_up(8 * nf) + align_up(4 * 2 * npairs) + align_up(8 * npairs)
    return b + 4096


def plan_passes(h, w, pairs, ws_limit=DEFAULT_WS_LIMIT, params=None):
    """st_farneback_pairs :3413-3437: runs of pairs halved until one pass fits the limit; returns, per pass, the
    distinct frame indices it touches (in slot order) and its pair count."""
    passes, start, n = [], 0, len(pairs)
    while start < n:
        count = n - start
        while True:
            frames = []
            for a, b in pairs[start:start + count]:
                for f in (a, b):
                    if f not in frames:
                        frames.append(f)
            if pass_bytes(h, w, len(frames), count, params) <= ws_limit or count == 1:
                break
            count = (count + 1) // 2
        passes.append((frames, count))
        start += count
    return passes


def split_limit(h, w):
    """The workspace limit of the pass-splitting call: as test_flow_gpu.py's scratch-cap test, a multiple of a rough
    per-pair estimate (two expansions + flow buffers) -- 8 of them, which splits the 35 pairs into 4 passes (9, 7, 10, 9)."""
    per_pair = 4 * h * w * (5 * 2 * 1.4 + 2 * 2 + 2)
    return int(8 * per_pair)


def paths(h, w, pairs, ws_limit=DEFAULT_WS_LIMIT, params=None):
    """The set of paths one call takes (the iteration launches: on the fused path only)."""
    got = set()
    for frames, npairs in plan_passes(h, w, pairs, ws_limit, params):
        al = aligned4(h, w, frames)
        got.add("pyr_fused" if pyr_fused_ok(h, w, params) else "pyr_per_level")
        got.add("polyexp_single" if single(h, w, npairs, params) else "polyexp_per_level")
        got.add("poly_u8" if poly_u8(h, w, npairs, params) else "poly_f32")
        got.add("aligned" if al else "unaligned")
        for k, kern, src in (iter_launches(h, w, npairs, params) if fused_path(h, w, params) else []):
            if k == 0:
                got.add("L0:" + kern)
            if kern != "tile":
                got.add("march:" + src)              # k_flow_iter3 / k_flow_iter_roles instance
    return got


def path_matrix():
    """(geometry, call) -> paths, for every call of tests/test_geometries_gpu.py."""
    m = {}
    for (h, w) in GEOMETRIES:
        for name, pairs in calls(h, w).items():
            m[(h, w, name)] = paths(h, w, pairs)
        if (h, w) in SPLIT_GEOMETRIES:
            m[(h, w, "split")] = paths(h, w, BIG, split_limit(h, w))
    return m


REQUIRED = {"pyr_fused", "pyr_per_level", "polyexp_single", "polyexp_per_level", "poly_u8", "poly_f32", "aligned",
            "unaligned", "L0:tile", "L0:iter3", "march:FLOW_COARSE", "march:FLOW_COARSE2"}


def _reached(m):
    got = set().union(*m.values())
    if any(p.startswith("L0:roles") for p in got):
        got.add("L0:roles")
    return got


def test_path_matrix_reaches_every_path():
    m = path_matrix()
    missing = (REQUIRED | {"L0:roles"}) - _reached(m)
    assert not missing, missing


def test_path_table_known_cases():
    """Spot values of the restated predicates, worked by hand from the C lines."""
    assert pyr_fused_ok(1080, 1920) and pyr_fused_ok(1920, 1080) and pyr_fused_ok(360, 640)
    assert not pyr_fused_ok(480, 854) and not pyr_fused_ok(1079, 1919)
    assert not pyr_fused_ok(203, 317)                        # 2 levels
    assert pyr_strip_w(1080) == (2, 544) and pyr_strip_w(1920) == (2, 960) and pyr_strip_w(4096) == (4, 1024)
    assert 1080 % pyr_strip_w(1080)[1] != 0                  # the second strip of a portrait frame is cut short
    assert single(1920, 1080, 16) and not single(1920, 1080, 17) and not single(480, 854, 1)
    assert poly_u8(1920, 1080, 35) and not poly_u8(1920, 1080, 8) and not poly_u8(480, 854, 35)
    assert aligned4(480, 854, range(34)) and not aligned4(1079, 1919, range(34)) and aligned4(1079, 1919, [0, 4])
    assert iter_kernel(360, 640, 1, False) == "tile" and iter_kernel(1080, 1920, 35, False) == "iter3"
    assert iter_kernel(1080, 1920, 1, False).startswith("roles")
    # 1079 over 540: the generic coarse instance; 1080 over 540: the half-height one
    assert ("FLOW_COARSE" in {s for k, kern, s in iter_launches(1079, 1919, 35) if k == 0})
    assert ("FLOW_COARSE2" in {s for k, kern, s in iter_launches(1080, 1920, 35) if k == 0})


@pytest.mark.parametrize("h,w", SPLIT_GEOMETRIES)
def test_split_limit_makes_three_passes(h, w):
    passes = plan_passes(h, w, BIG, split_limit(h, w))
    assert len(passes) >= 3 and sum(c for _, c in passes) == len(BIG), passes
    assert len(plan_passes(h, w, BIG)) == 1
    # the limit still holds one pair
    assert pass_bytes(h, w, 2, 1) <= split_limit(h, w)


def test_report_paths():
    """The path each case takes (pytest -s shows it)."""
    for (h, w, name), p in path_matrix().items():
        print("%4dx%-4d %-8s %s" % (h, w, name, " ".join(sorted(p))))


# ---------------------------------------------------------------- (b) oracle vs float64 at rounded geometries
@pytest.mark.parametrize("h,w", GEOMETRIES + [(271, 433), (203, 317), (264, 328)])
def test_level_shapes_agree(h, w):
    """levels_for / level_shape of the float64 derivation == the oracle's fb_levels / fb_level_geom == the library's."""
    from scannertools_amd import hip
    L = oracle.fb_levels(h, w)
    assert ref.levels_for(h, w) == L == hip.fb_levels(h, w)
    for k in range(L + 1):
        want = oracle.fb_level_geom(h, w, k)
        assert ref.level_shape(h, w, k) == want[:2], (k, want)
        assert hip.fb_level_geom(h, w, k) == want, k


def test_rounded_level_sizes():
    """Halves round to even: 271 -> 136 -> 68 -> 34, 433 -> 216 -> 108 -> 54; 1079 -> 540 -> 270 -> 135."""
    assert [oracle.fb_level_geom(271, 433, k)[:2] for k in range(4)] == [(271, 433), (136, 216), (68, 108), (34, 54)]
    assert [oracle.fb_level_geom(1079, 1919, k)[0] for k in range(4)] == [1079, 540, 270, 135]
    assert oracle.fb_levels(203, 317) == 2


@pytest.mark.parametrize("h,w", [(271, 433), (480, 854), (203, 317)])
def test_oracle_against_float64_at_rounded_geometry(h, w):
    """As test_oracle.py's 264 x 328 check, with the same bounds, at every level of a geometry whose levels round:
    pyramid images, polynomial expansion, UpdateMatrices and the box solve; then the flow end to end."""
    f0, f1 = translated_rgb_pair(21, h, w, 3, -2)
    g0, g1 = oracle.gray_u8(f0), oracle.gray_u8(f1)
    L = oracle.fb_levels(h, w)
    assert ref.levels_for(h, w) == L
    rng = np.random.default_rng(3)
    for k in range(L + 1):
        I, I_r = oracle.fb_pyr_image(g0, k), ref.pyramid_image(g0, k)
        assert I.shape == I_r.shape and np.abs(I - I_r).max() <= 2e-4, k
        R_o, R_r = oracle.polyexp(I), ref.poly_expansion(I.astype(np.float64))
        assert np.abs(R_o - R_r).max() <= 2e-4 * max(1.0, np.abs(R_r).max()), k
        R1_o = oracle.polyexp(oracle.fb_pyr_image(g1, k))
        fl = (rng.standard_normal(I.shape + (2,)) * 2).astype(np.float32)
        M_o = oracle.update_matrices(R_o, R1_o, fl)
        M_r = ref.update_matrices(R_o.astype(np.float64), R1_o.astype(np.float64), fl.astype(np.float64))
        assert np.abs(M_o - M_r).max() <= 1e-4 * max(1.0, np.abs(M_r).max()), k
        flow_o, _ = oracle.update_flow_blur(R_o, R1_o, M_o, 15, False)
        flow_r = ref.box_solve(M_o.astype(np.float64), 15)
        assert np.abs(flow_o - flow_r).max() <= 1e-4, k
    got, want = oracle.farneback(g0, g1), ref.farneback(g0, g1)
    assert np.linalg.norm(got - want) <= 2e-4 * np.linalg.norm(want)
    assert np.abs(got - want).max() <= 2e-3
    inner = got[40:-40, 40:-40]
    assert abs(np.median(inner[..., 0]) - 3) < 0.05 and abs(np.median(inner[..., 1]) + 2) < 0.05
