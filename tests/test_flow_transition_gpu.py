"""GPU parity of the level-transition flow source (FLOW_COARSE2: the flow of a pyramid level's first iteration is the
coarser level's flow up-sampled on the fly, the coarse level exactly half as tall).  k_flow_iter3 carries the
horizontally interpolated coarse rows from one batch of rows to the next; k_flow_iter_tile evaluates the generic
INTER_LINEAR expressions per pixel and k_flow_iter_roles re-reads the coarse rows of every batch.  All three must give
the same bits, and the oracle's flow within the stage tolerance.
Geometries: 1080p (not a multiple of 32 rows); strips ending just before / after a strip edge (w = 240 k +- 8, where a
lane's right coarse neighbour leaves the row); segments of 64 rows, whose vertical anchor at row 32 falls mid-segment
(1 pair of 1080 x 3832: 16 strips x 17 segments); and a 256-pair 1080p call (the benchmark's launch geometry:
whole-height segments, an anchor every 32 rows) against the tile kernel end to end.
"""
import numpy as np
import pytest
import torch

import oracle
from util import torch_stream, translated_rgb_pair

pytestmark = pytest.mark.gpu


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _transition_case(h, w, seed):
    f0, f1 = translated_rgb_pair(seed, h, w, 2, -1)
    R0 = oracle.polyexp(oracle.gray_u8(f0).astype(np.float32))
    R1 = oracle.polyexp(oracle.gray_u8(f1).astype(np.float32))
    coarse = (np.random.default_rng(seed).standard_normal((h // 2, (w + 1) // 2, 2)) * 2).astype(np.float32)
    up = oracle.resize_linear(coarse, h, w) * np.float32(2.0)
    ref = oracle.update_flow_blur(R0, R1, oracle.update_matrices(R0, R1, up), 15, False)[0]
    return R0, R1, coarse, ref


@pytest.mark.parametrize("h,w", [(1080, 1920), (1080, 3832), (200, 232), (200, 248), (136, 472), (136, 488),
                                 (270, 712), (270, 728), (96, 1912), (96, 1928), (540, 960), (270, 480)])
def test_coarse2_iteration_kernels_agree(mode_ctxs, h, w):
    assert h % 2 == 0  # the coarse level is exactly half as tall: the FLOW_COARSE2 instances
    R0, R1, coarse, ref = _transition_case(h, w, h * 7 + w)
    r0, r1, c = cu(R0), cu(R1), cu(coarse)
    outs = {}
    for mode in ("march", "tile", "roles4", "roles5"):
        outs[mode] = mode_ctxs[mode].flow_iteration(r0, r1, coarse_flow=c, pyr_scale=0.5).cpu().numpy()
        assert np.abs(outs[mode] - ref).max() <= 1e-4, (mode, np.abs(outs[mode] - ref).max())
    for mode in ("tile", "roles4", "roles5"):
        np.testing.assert_array_equal(outs["march"], outs[mode], err_msg="%dx%d %s" % (h, w, mode))


def test_coarse2_1080p_256_pairs_equal_tile(mode_ctxs):
    """The benchmark's call (256 consecutive 1080p pairs) under the default schedule against the tile kernel."""
    d = torch_stream(257, 1080, 1920, 5)
    got = mode_ctxs["default"].optical_flow(d)
    ref = mode_ctxs["tile"].optical_flow(d)
    assert got.shape == (256, 1080, 1920, 2)
    assert torch.equal(got, ref)
