"""k_flow_iter3's segment plan (launch_flow_iter), restated: segments start at multiples of 32 rows (the anchor rows of the
window sums) and the LAST one ends at the frame's last row, so they need not be equal.  For every segment count the planner
weighs the height rounded up to whole periods (the former rule) and the height rounded down, the last segment taking the
remainder; a round of resident workgroups costs its tallest segment plus the 15 rows of ring initialisation.

tests/test_flow_geometries.py's iter_kernel keeps the former rule: it still decides between the kernels (the role-split
planner reads the rounded-up plan), and describes the segment heights only of the plan this one is compared with.
"""
import pytest

F3_ANCHOR = 32
B2_OUT = 240


def old_plan(h, w, n_pairs, num_cus=256):
    """The rounded-up rule alone: (cost, rows per segment, segments)."""
    strips = (w + B2_OUT - 1) // B2_OUT
    resident = num_cus * 2
    periods = (h + F3_ANCHOR - 1) // F3_ANCHOR
    best, rows = 1e300, periods * F3_ANCHOR
    for segs in range(1, periods + 1):
        r = (periods + segs - 1) // segs * F3_ANCHOR
        nseg = (h + r - 1) // r
        rounds = (strips * n_pairs * nseg + resident - 1) // resident
        cost = float(rounds) * (r + 15)
        if cost < best * 0.999:
            best, rows = cost, r
    return best, rows, (h + rows - 1) // rows


def new_plan(h, w, n_pairs, num_cus=256):
    """launch_flow_iter's k_flow_iter3 branch: the old plan, then the rounded-down candidates."""
    strips = (w + B2_OUT - 1) // B2_OUT
    resident = num_cus * 2
    periods = (h + F3_ANCHOR - 1) // F3_ANCHOR
    best, rows, nseg = old_plan(h, w, n_pairs, num_cus)
    for segs in range(1, periods + 1):
        r = periods // segs * F3_ANCHOR
        if r < F3_ANCHOR:
            break
        last = h - (segs - 1) * r
        rounds = (strips * n_pairs * segs + resident - 1) // resident
        cost = float(rounds) * (max(r, last) + 15)
        if cost < best * 0.999:
            best, rows, nseg = cost, r, segs
    return best, rows, nseg


def segments(h, rows, nseg):
    """[y0, y1) of every workgroup row of the grid, as the kernel computes them."""
    return [(i * rows, h if i + 1 == nseg else min(h, (i + 1) * rows)) for i in range(nseg)]


@pytest.mark.parametrize("n_pairs", [1, 8, 256])
def test_segments_cover_the_frame_and_never_cost_more(n_pairs):
    for w in (240, 1920):
        for h in range(2, 2201):
            cost_old, rows_old, nseg_old = old_plan(h, w, n_pairs)
            cost, rows, nseg = new_plan(h, w, n_pairs)
            seg = segments(h, rows, nseg)
            assert all(y0 % F3_ANCHOR == 0 for y0, _ in seg), (h, seg)
            assert seg[0][0] == 0 and seg[-1][1] == h, (h, seg)
            assert all(a[1] == b[0] for a, b in zip(seg, seg[1:])), (h, seg)
            assert all(y1 > y0 for y0, y1 in seg), (h, seg)
            assert cost <= cost_old, (h, cost, cost_old)
            # the planned cost is the cost of the segments the kernel runs
            strips = (w + B2_OUT - 1) // B2_OUT
            rounds = (strips * n_pairs * nseg + 511) // 512
            assert rounds * (max(y1 - y0 for y0, y1 in seg) + 15) <= cost, (h, seg, cost)


def test_headline_levels():
    """256 pairs of 1080p: level 3 (135 x 240) becomes 64 + 71 rows instead of 96 + 39; levels 0-2 keep their one segment."""
    assert segments(135, *old_plan(135, 240, 256)[1:]) == [(0, 96), (96, 135)]
    assert segments(135, *new_plan(135, 240, 256)[1:]) == [(0, 64), (64, 135)]
    assert new_plan(135, 240, 256)[0] == 86.0 and old_plan(135, 240, 256)[0] == 111.0
    for h, w in ((1080, 1920), (540, 960), (270, 480)):
        assert new_plan(h, w, 256) == old_plan(h, w, 256) and new_plan(h, w, 256)[2] == 1
    # a few pairs of a small frame: one period per segment either way (the call sizes of tests/test_iter_segments_gpu.py)
    for n in (1, 3, 17):
        assert new_plan(135, 240, n)[1:] == old_plan(135, 240, n)[1:] == (32, 5)
        assert new_plan(200, 328, n)[1:] == old_plan(200, 328, n)[1:] == (32, 7)
