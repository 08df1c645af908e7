"""The expansion launches' segment plan (polyexp_rows in st_farneback.hip), restated.  Every segment but the last has
`rows` rows, a multiple of PE_RB = 4 and at least 12; the last takes the remainder (polyexp_body: y1 = min(h, y0 + rows)).

Step 1 is the former rule (at least num_cus * 8 workgroups where the height allows); step 2 takes the cheapest among that
cut and every finer one by the model the segment sweep supports (profiles/polyexp_segments_sweep.txt), in rows per CU:

    cost = strips * n * (h + segments * c) / num_cus + 0.85 * (rows + c)

c = 1.5 rows for the gray-source instance (k_polyexp_u8), 0 for the float-source one.  The sweep contradicts a rounds model
(ceil(workgroups / resident) rounds of rows + c), so the residency of the two instances (5 and 6 workgroups per CU) is not a
parameter of the plan and the cases run over the two instances' constants instead.

"None shorter than 12 rows" is the bound on `rows`: the ragged last segment is whatever the height leaves, as it always was
(26 rows at a few frames were and are 12 + 12 + 2), and a frame lower than 12 rows is one whole-frame segment.
"""
import pytest

PE_RB = 4
PE_OUT = 240
MIN_ROWS = 12
SEG_COST = {"u8": 1.5, "f32": 0.0}
TAIL = 0.85


def plan_cost(h, per, rows, c, num_cus=256):
    nseg = (h + rows - 1) // rows
    return float(per) * (h + nseg * c) / num_cus + TAIL * (min(rows, h) + c)


def old_rows(h, strips, n, num_cus=256):
    """The former rule: whole-height segments above num_cus * 8 workgroups, else just enough segments to reach them."""
    target, per = num_cus * 8, strips * n
    segs = max(1, (target + per - 1) // per)
    rows = (h + segs - 1) // segs
    rows = (rows + PE_RB - 1) // PE_RB * PE_RB
    return min(h, max(rows, MIN_ROWS))


def new_rows(h, strips, n, inst, num_cus=256):
    """polyexp_rows: the former plan, then every finer cut down to 12 rows; ties keep the taller segment."""
    c, per = SEG_COST[inst], strips * n
    rows = old_rows(h, strips, n, num_cus)
    best = plan_cost(h, per, rows, c, num_cus)
    for r in range((rows - 1) // PE_RB * PE_RB, MIN_ROWS - 1, -PE_RB):
        if (h + r - 1) // r > 65535:   # the segments are the grid's y dimension
            break
        cost = plan_cost(h, per, r, c, num_cus)
        if cost < best:
            best, rows = cost, r
    return rows


def segments(h, rows):
    """[y0, y1) of every workgroup row of the grid, as polyexp_body computes them."""
    return [(y0, min(h, y0 + rows)) for y0 in range(0, h, rows)]


@pytest.mark.parametrize("inst", ["u8", "f32"])
@pytest.mark.parametrize("n", [1, 2, 9, 17, 33, 257, 2049])
def test_segments_cover_the_frame_and_never_cost_more(n, inst):
    c = SEG_COST[inst]
    for strips in (1, 2, 3, 4):
        for h in range(2, 2201):
            rows_old, rows = old_rows(h, strips, n), new_rows(h, strips, n, inst)
            seg = segments(h, rows)
            assert all((y1 - y0) % PE_RB == 0 for y0, y1 in seg[:-1]), (h, seg)
            assert seg[0][0] == 0 and seg[-1][1] == h, (h, seg)
            assert all(a[1] == b[0] for a, b in zip(seg, seg[1:])), (h, seg)
            assert all(y1 > y0 for y0, y1 in seg), (h, seg)
            assert len(seg) == 1 or all(y1 - y0 >= MIN_ROWS for y0, y1 in seg[:-1]), (h, seg)
            assert rows >= MIN_ROWS or (rows == h and len(seg) == 1), (h, rows)
            # never fewer workgroups than the former rule's floor, never dearer by the model
            assert rows <= rows_old and len(seg) >= len(segments(h, rows_old)), (h, rows, rows_old)
            assert plan_cost(h, strips * n, rows, c) <= plan_cost(h, strips * n, rows_old, c), (h, rows, rows_old)


def test_headline_levels():
    """257 frames of 1080p (profiles/NOTES.md): level 0 (gray source, 8 strips) 9 segments of 120 rows instead of one of
    1080; levels 1-3 (float source) 12-row segments instead of 2, 4 and 7 segments."""
    assert old_rows(1080, 8, 257) == 1080 and new_rows(1080, 8, 257, "u8") == 120
    assert len(segments(1080, 120)) == 9
    for h, strips, nseg_old, nseg in ((540, 4, 2, 45), (270, 2, 4, 23), (135, 1, 7, 12)):
        assert len(segments(h, old_rows(h, strips, 257))) == nseg_old
        assert new_rows(h, strips, 257, "f32") == 12 and len(segments(h, 12)) == nseg
    # 33 frames of 4K (2112 workgroups of 540 rows before): level 0 in 27 segments of 80 rows
    assert old_rows(2160, 16, 33) == 540 and new_rows(2160, 16, 33, "u8") == 80


def test_small_calls_keep_their_parallelism():
    """Calls of at most 16 pairs (k_polyexp_ml, float source at every level): 12-row segments, which one or two frames
    already had; more frames had up to 68 rows."""
    for n in (2, 3, 5, 9, 17):
        for h, w in ((1080, 1920), (540, 960), (270, 480), (135, 240)):
            strips = (w + PE_OUT - 1) // PE_OUT
            assert new_rows(h, strips, n, "f32") == 12 <= old_rows(h, strips, n)
    assert old_rows(1080, 8, 2) == 12 and old_rows(1080, 8, 17) == 68


def test_a_very_tall_frame_stays_inside_the_grid():
    """One frame of 1 000 000 x 8: 12-row segments would be 83 334, more than a grid dimension holds."""
    rows = new_rows(1000000, 1, 1, "f32")
    assert rows == 16 and len(segments(1000000, rows)) == 62500 <= 65535 < len(segments(1000000, 12))
