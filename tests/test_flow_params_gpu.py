"""Farneback flow across the st_fb_params space: stage by stage and end to end, off the reference's parameters.

tests/test_flow_params.py names the kernels and instances every (parameter set, geometry, call) here takes and checks that
the matrix reaches each of them: the fused iteration kernels at 1, 2 and 5 iterations (the ping-pong's other parities,
the level transition that is also the last launch), the generic coarse-flow instance at upsampling ratios 1.25, 1.33,
1.67 and 3.33 on the marching, role-split and tile kernels, pyramids of one to seven levels, the 7-tap expansion in its
three launch forms, the gray table of OpenCV <= 3.4.2 in the one-pass pyramid, and the unfused path (k_update_matrices +
k_blur_update) at window radii 1 ... 31 as a whole-call path: many pairs, many segments, device tables, pass splits.

Stage level (through the st_fb_* entry points):
  - pyramid images bit-exact against the oracle at pyr_scale 0.3 ... 0.8, every level the library builds (and the first it
    does not: refused), random bytes and a smooth texture, from the 14-bit gray table too;
  - the 7-tap expansion bit-exact;
  - the box solve at windows 3 ... 63 within 1e-4 px of the oracle (windows 3, 5, 7: where the oracle itself is within
    1e-4 px of the float64 solve; elsewhere within half again of the oracle's own distance from it).
End to end, per (parameter set, geometry), on a translating texture stream:
  - batch agreement: a 35-pair call, pairs 0-7 and four single pairs in calls of their own, bit for bit -- on the unfused
    path too; a 45-pair call (tables through device memory) per path;
  - every scheduling mode of conftest.FLOW_MODES equal to the default;
  - a call split into passes by a workspace limit equal to the unsplit call, one per path;
  - pairs against the oracle: tier 1 of util.assert_flow_close (5e-3 px, relative L2 1e-4), or the kernel within half
    again of the oracle's own distance from the float64 derivation run at the same parameters; the planted translation.
Refusals: parameter sets whose pyramid cannot be built are refused before anything is launched.

Sensitivity.  Each group was run once on an MI355X against a scratch library with one planted value fault (never
committed); fault -> what failed (the tests of tests/test_flow_gpu.py that touch the same code passed with the first four):
  - from the fourth iteration on the field source reads the other ping-pong buffer -> test_against_oracle[iters5-*] (3);
  - k_pyr's 5-tap row filter takes taps[3] for its outer pair -> test_pyramid_levels_bit_exact_at_other_scales at 0.6, 0.75
    and 0.8 (9), test_pyramid_from_14_bit_gray;
  - centre tap x 1.001 in k_polyexp_u8<7> only -> test_scheduling_modes_agree, test_batch_agreement and
    test_against_oracle at [poly7-1080x1920];
  - launch_blur's segment height made to follow the pair count -> test_batch_agreement[win3-480x854], [win3-1080x1920],
    [win21+poly7+scale0.7/levels5+iters4-1080x1920];
  - q.mul left at 2 whatever pyr_scale is -> test_against_oracle at every set with pyr_scale != 0.5 (12);
  - one column too many (m + 1) in k_blur_update's horizontal sum -> test_update_flow_blur_every_window (10),
    test_against_oracle at every unfused case (19);
  - k_blur_update stores (v, u) -> test_translation at every unfused case (19);
  - centre tap x 1.001 in k_polyexp<7> -> test_polyexp_n7_bit_exact; later passes of a split call pair each frame with
    itself -> test_pass_split;
  - the parent commit's library -> test_unbuildable_pyramid_is_refused_before_any_launch (the five LDS cases: kernels had
    been launched), test_window_1_is_refused.
"""
import numpy as np
import pytest
import torch
from scipy import ndimage

import oracle
import ref_farneback_np as ref
from conftest import FLOW_MODES, make_mode_ctx
from scannertools_amd import _native
from scannertools_amd.hip import StError, default_params
from test_flow_geometries import BIG, N_FRAMES, levels, param, plan_passes
from test_flow_gpu import SIZES
from test_flow_params import (BLUR_SIZES, BLUR_WINDOWS, MATRIX, ORACLE_PAIRS, P, SINGLES, SPLIT_CASES, TAB, TAB_CASES,
                              blur_inputs, case_calls, pyr_level_ok, split_limit, supported)
from util import float64_flow, interleaved5, planar5, random_frames, smooth_texture, torch_stream, within_half_again

pytestmark = pytest.mark.gpu

STEP = 2                       # torch_stream: next(x + STEP, y - 1) = prev(x, y)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------- stage: pyramid
PYR_SCALES = [0.3, 0.45, 0.6, 0.75, 0.8]


def _pyr_sources(h, w):
    return {"bytes": np.random.default_rng(h + w).integers(0, 256, (h, w), dtype=np.uint8),
            "texture": (smooth_texture(h + w, h, w) + np.random.default_rng(1).integers(0, 8, (h, w))).clip(0, 255).astype(np.uint8)}


@pytest.mark.parametrize("h,w", [(240, 426), (203, 317), (61, 1027), (1080, 1920)])
@pytest.mark.parametrize("scale", PYR_SCALES)
def test_pyramid_levels_bit_exact_at_other_scales(hip_ctx, h, w, scale):
    """Every level of a pyramid of up to seven levels (k_pyr in its LINEAR mode at kernel sizes 3 ... 23, ratios 1.25 ...
    9.5) equals the oracle's bit for bit; the first level whose Gaussian or tile the library cannot hold is refused."""
    L = levels(h, w, dict(pyr_scale=scale, num_levels=6))
    built = 0
    for k in range(L + 1):
        prm = dict(pyr_scale=scale, num_levels=k)
        for kind, gray in _pyr_sources(h, w).items():
            if not pyr_level_ok(h, w, k, prm):
                with pytest.raises(StError) as e:
                    hip_ctx.pyr_image(cu(gray), k, default_params(**prm))
                assert e.value.status == _native.ST_ERR_UNSUPPORTED
                continue
            got = hip_ctx.pyr_image(cu(gray), k, default_params(**prm)).cpu().numpy()
            want = oracle.fb_pyr_image(gray, k, oracle.default_params(**prm))
            assert got.shape == want.shape
            np.testing.assert_array_equal(got, want, err_msg="%s level %d" % (kind, k))
            built += 1
    assert built >= 2 * min(L + 1, 2)


def test_pyramid_from_14_bit_gray(hip_ctx):
    h, w = 240, 426
    f = random_frames(14, 1, h, w)[0]
    g = hip_ctx.gray(cu(f), 14)
    g_o = oracle.gray_u8(f, 14)
    np.testing.assert_array_equal(g.cpu().numpy(), g_o)
    assert (g_o != oracle.gray_u8(f, 15)).any()
    prm = dict(pyr_scale=0.75, num_levels=4, gray_bits=14)
    for k in range(5):
        got = hip_ctx.pyr_image(g, k, default_params(**prm)).cpu().numpy()
        np.testing.assert_array_equal(got, oracle.fb_pyr_image(g_o, k, oracle.default_params(**prm)), err_msg="level %d" % k)


# ---------------------------------------------------------------- stage: 7-tap expansion
@pytest.mark.parametrize("h,w", SIZES + [(12, 300), (300, 9), (1080, 1920)])
@pytest.mark.parametrize("sigma", [1.5, 1.2])
def test_polyexp_n7_bit_exact(hip_ctx, h, w, sigma):
    I = (smooth_texture(h * w % 9973, h, w) * 1.0).astype(np.float32)
    got = hip_ctx.polyexp(cu(I), 7, sigma).cpu().numpy()
    np.testing.assert_array_equal(got, oracle.polyexp(I, 7, sigma))


# ---------------------------------------------------------------- stage: box solve
@pytest.mark.parametrize("h,w", BLUR_SIZES)
@pytest.mark.parametrize("update", [True, False])
def test_update_flow_blur_every_window(hip_ctx, h, w, update):
    """Windows >= 9: |flow - oracle| <= 1e-4 px and |M' - oracle| <= 1e-4 max|M'| (test_update_flow_blur_parity's bounds).
    Windows 3, 5, 7: the same wherever the oracle is within 1e-4 px of the float64 solve; elsewhere |flow - f64| within
    1.5 x the oracle's own distance from f64, maximised over the pixel's 3 win neighbourhood, plus 1e-4 -- every pixel.
    M' at windows 3, 5, 7 is compared with the oracle's UpdateMatrices of the KERNEL's flow (the ill-conditioned solve moves
    the oracle's own M' by more than the bound), so there it vouches for the update step alone and is only as good as the
    flow check above it."""
    R0, R1, M = blur_inputs(h, w)
    dR0, dR1, dM = cu(R0), cu(R1), cu(planar5(M))
    for win in BLUR_WINDOWS:
        ref_flow, ref_M = oracle.update_flow_blur(R0, R1, M, win, update)
        flow, Mn = hip_ctx.update_flow_blur(dR0, dR1, dM, win, update)
        flow = flow.cpu().numpy()
        d = np.abs(flow - ref_flow).max(-1)
        what = "%dx%d window %d" % (h, w, win)
        if win >= 9:
            print("box solve %s: |flow - oracle| %.2e px" % (what, d.max()))
            assert d.max() <= 1e-4, what
        else:
            f64 = ref.box_solve(M.astype(np.float64), win)
            od = np.abs(ref_flow - f64).max(-1)
            near = od <= 1e-4
            eg = np.abs(flow - f64).max(-1)
            local = ndimage.maximum_filter(od, size=3 * win, mode="nearest")
            print("box solve %s: |flow - oracle| %.2e px (%.2e where the oracle is within 1e-4 of f64: %.4f of the field), "
                  "oracle - f64 %.2e, kernel - f64 %.2e" % (what, d.max(), d[near].max() if near.any() else 0.0, near.mean(), od.max(), eg.max()))
            assert (d[near] <= 1e-4).all(), what
            assert (eg[~near] <= 1.5 * local[~near] + 1e-4).all(), what
        if update:
            Mn = interleaved5(Mn.cpu().numpy())
            if win >= 9:
                assert np.abs(Mn - ref_M).max() <= 1e-4 * np.abs(ref_M).max(), what
            else:
                # M' is a per-pixel function of the flow just solved: against UpdateMatrices of the kernel's own flow
                want = oracle.update_matrices(R0, R1, flow)
                assert np.abs(Mn - want).max() <= 1e-4 * np.abs(want).max(), what
        else:
            assert Mn is None


# ---------------------------------------------------------------- end to end: the parameter matrix
CASES = sorted(MATRIX, key=lambda c: (c[1], list(P).index(c[0])))     # geometry by geometry: one stream at a time
_stream = {}


def stream(h, w):
    """The 34-frame stream of one geometry (kept until another geometry asks)."""
    if (h, w) not in _stream:
        _stream.clear()
        torch.cuda.empty_cache()
        _stream[(h, w)] = torch_stream(N_FRAMES, h, w, h * 7 + w, step=STEP)
    return _stream[(h, w)]


@pytest.fixture(scope="module", params=CASES, ids=["%s-%dx%d" % (n, g[0], g[1]) for n, g in CASES])
def case(request, hip_ctx):
    """(name, parameter dict, h, w, frames, flows of the 35-pair call) of one (parameter set, geometry)."""
    name, (h, w) = request.param
    d = stream(h, w)
    big = hip_ctx.optical_flow(d, pairs=BIG, params=default_params(**P[name]))
    assert tuple(big.shape) == (len(BIG), h, w, 2)
    yield name, P[name], h, w, d, big
    del big
    hip_ctx.release_workspace()
    torch.cuda.empty_cache()


def test_batch_agreement(case, hip_ctx):
    name, prm, h, w, d, big = case
    lp = default_params(**prm)
    for call, (pairs, _) in case_calls(name, (h, w)).items():
        if call in ("33+2", "split"):
            continue
        got = hip_ctx.optical_flow(d, pairs=pairs, params=lp)
        if call == "45":
            # the first 35 pairs are the big call's; the other ten against a call of their own
            assert torch.equal(got[:len(BIG)], big), "%s %dx%d call 45, rows of the 35-pair call" % (name, h, w)
            assert torch.equal(got[len(BIG):], hip_ctx.optical_flow(d, pairs=TAB[len(BIG):], params=lp)), "%s %dx%d call 45, tail" % (name, h, w)
            continue
        want = big[[BIG.index(p) for p in pairs]]
        assert torch.equal(got, want), "%s %dx%d call %s" % (name, h, w, call)


def test_scheduling_modes_agree(case, mode_ctxs):
    name, prm, h, w, d, big = case
    lp = default_params(**prm)
    # the 7-tap expansion from the gray frames (k_polyexp_u8<7>) needs more than 16 pairs: polyu8 against polyf32 decides it
    sizes = (8, len(BIG)) if name == "poly7" and (h, w) == (1080, 1920) else (8,)
    for n in sizes:
        for mode in FLOW_MODES:
            got = mode_ctxs[mode].optical_flow(d, pairs=BIG[:n], params=lp)
            assert torch.equal(got, big[:n]), "%s %dx%d mode %s, %d pairs" % (name, h, w, mode, n)
            del got
    for c in mode_ctxs.values():
        c.release_workspace()


@pytest.mark.parametrize("name,g", SPLIT_CASES, ids=["%s-%dx%d" % (n, g[0], g[1]) for n, g in SPLIT_CASES])
def test_pass_split(hip_ctx, name, g):
    """One fused and one unfused set (five planes per M field in pass_bytes) in at least three passes == the unsplit call."""
    h, w = g
    prm = P[name]
    d = stream(h, w)
    big = hip_ctx.optical_flow(d, pairs=BIG, params=default_params(**prm))
    limit = split_limit(h, w, prm)
    assert len(plan_passes(h, w, BIG, limit, prm)) >= 3
    with make_mode_ctx("default", workspace_limit=limit) as small:
        got = small.optical_flow(d, pairs=BIG, params=default_params(**prm))
    assert torch.equal(got, big)
    hip_ctx.release_workspace()


def flow_close(got, want, fa, fb, prm, what):
    """Tier 1 of util.assert_flow_close, or the kernel within half again of the oracle's own distance from the float64
    derivation at the same parameters (pixel by pixel over a 3 win neighbourhood, and in L2).  -> 1 or 2."""
    d = np.abs(got - want).max(-1)
    nref = max(float(np.linalg.norm(want)), 1e-30)
    rel = float(np.linalg.norm(got - want)) / nref
    print("flow %s: |got - oracle| max %.2e px, relative L2 %.2e" % (what, d.max(), rel))
    if d.max() <= 5e-3 and np.linalg.norm(got - want) <= 1e-4 * nref + 1e-6:
        return 1
    f64 = float64_flow(fa, fb, prm)
    print("flow %s: oracle - f64 max %.2e, kernel - f64 max %.2e" % (what, np.abs(want - f64).max(), np.abs(got - f64).max()))
    assert within_half_again(got, want, f64, 3 * param(prm, "win_size")), what
    return 2


def test_against_oracle(case):
    name, prm, h, w, d, big = case
    f = d.cpu().numpy()
    o = oracle.default_params(**prm)
    for i in ORACLE_PAIRS[(h, w)]:
        a, b = BIG[i]
        flow_close(big[i].cpu().numpy(), oracle.optical_flow_rgb(f[a], f[b], o), f[a], f[b], prm, "%s %dx%d pair %d" % (name, h, w, i))


def test_translation(case):
    name, prm, h, w, d, big = case
    m = min(h, w) // 8
    for i in (0, 16, 32):
        inner = big[i, m:-m, m:-m]
        u, v = float(inner[..., 0].median()), float(inner[..., 1].median())
        assert abs(u - STEP) < 0.05 and abs(v + 1) < 0.05, (name, h, w, i, u, v)


def test_matrix_cases_cover_the_table_and_split_calls():
    assert all(c in MATRIX for c in TAB_CASES + SPLIT_CASES) and max(max(p) for p in TAB) < N_FRAMES and SINGLES[0] in BIG


# ---------------------------------------------------------------- refusals and limits
FLOW_KERNELS = (_native.K_GRAY, _native.K_PYR, _native.K_POLYEXP, _native.K_UPDATE_MATRICES, _native.K_BLUR_UPDATE)


@pytest.mark.parametrize("h,w,kw", [(1080, 1920, dict(pyr_scale=0.3, num_levels=2)), (1080, 1920, dict(pyr_scale=0.45, num_levels=3)),
                                    (1080, 1920, dict(pyr_scale=0.6, num_levels=5)), (1080, 1920, dict(pyr_scale=0.7, num_levels=7)),
                                    (1080, 1920, dict(pyr_scale=0.7, num_levels=7, win_size=9)),
                                    (512, 640, dict(num_levels=4)), (512, 640, dict(num_levels=5, win_size=21))])
def test_unbuildable_pyramid_is_refused_before_any_launch(hip_ctx, h, w, kw):
    """A parameter set one of whose levels needs more than 31 Gaussian taps (512 x 640, level 4 at pyr_scale 0.5: 39) or
    a k_pyr tile above 64 KiB of LDS: ST_ERR_UNSUPPORTED, no kernel launched, the output frames untouched, and the same
    context computes the default flow afterwards."""
    assert not supported(h, w, kw) and supported(h, w, dict(kw, num_levels=1))
    d = stream(h, w)[:3] if (h, w) == (1080, 1920) else torch_stream(3, h, w, 5, step=STEP)
    want = hip_ctx.optical_flow(d)
    with make_mode_ctx("default") as ctx:
        ctx.timing_enable(FLOW_KERNELS)
        ctx.timing_reset()
        out = torch.full((2, h, w, 2), -12345.0, dtype=torch.float32, device="cuda")
        with pytest.raises(StError) as e:
            ctx.optical_flow(d, params=default_params(**kw), out=out)
        assert e.value.status == _native.ST_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert [ctx.timing_read(k)[0] for k in FLOW_KERNELS] == [0] * len(FLOW_KERNELS)
        assert bool((out == -12345.0).all())
        ctx.timing_enable(())
        assert torch.equal(ctx.optical_flow(d), want)
    f = d[:2].cpu().numpy()
    ref_flow = oracle.optical_flow_rgb(f[0], f[1])
    got = want[0].cpu().numpy()
    assert np.abs(got - ref_flow).max() <= 5e-3 and np.linalg.norm(got - ref_flow) <= 1e-4 * np.linalg.norm(ref_flow)


def test_window_1_is_refused(hip_ctx):
    """win_size 1 / block_size 1: the reference's running sums count row 0 and column 0 twice at radius 0
    (test_flow_params.py::test_oracle_window_1_is_not_a_box_filter); the library refuses it."""
    f = torch.zeros((2, 64, 64, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(StError) as e:
        hip_ctx.optical_flow(f, params=default_params(win_size=1))
    assert e.value.status == _native.ST_ERR_UNSUPPORTED
    M = torch.zeros((5, 64, 64), dtype=torch.float32, device="cuda")
    with pytest.raises(StError) as e:
        hip_ctx.update_flow_blur(None, None, M, 1, False)
    assert e.value.status == _native.ST_ERR_UNSUPPORTED
    for bs in (0, 2, 65):
        with pytest.raises(StError):
            hip_ctx.update_flow_blur(None, None, M, bs, False)
