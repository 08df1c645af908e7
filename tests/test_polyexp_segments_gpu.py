"""The expansion launches in the regime the segment planner changed: more workgroup columns (strips x frames) than
num_cus * 8, where every segment used to be the whole height.  A small frame reaches it only with many frames: 2049 frames of
72 x 250 and of 75 x 250 (two strips: 4098 columns; level 1, one strip, has 2049) in ONE optical_flow call.  The plan
(tests/test_polyexp_segments.py restates it) cuts level 0 into 12-row segments -- six at 72 rows, six and a ragged one of 3
rows at 75 -- where the former rule ran one.  A pixel's expansion does not depend on where its segment starts, so the flows must
equal, bit for bit, those of the same pairs in calls of 16 pairs, and one pair is checked against the oracle.
"""
import numpy as np
import pytest

import oracle
from test_polyexp_segments import PE_OUT, new_rows, old_rows, segments
from util import assert_flow_close, torch_stream

pytestmark = pytest.mark.gpu

N_FRAMES = 2049


@pytest.mark.parametrize("h,w,ragged", [(72, 250, False), (75, 250, True)])
def test_many_small_frames_in_one_call(hip_ctx, h, w, ragged):
    import torch
    strips = (w + PE_OUT - 1) // PE_OUT
    assert strips == 2 and strips * N_FRAMES > 256 * 8, "not the large-launch regime"
    assert old_rows(h, strips, N_FRAMES) == h, "the former rule cut this launch already"
    for inst in ("f32", "u8"):   # whichever instance the library picks for this geometry
        seg = segments(h, new_rows(h, strips, N_FRAMES, inst))
        assert len(seg) > 1, seg
        if ragged:
            assert (seg[-1][1] - seg[-1][0]) % 4 != 0 and seg[-1][1] - seg[-1][0] < seg[0][1] - seg[0][0], seg
    frames = torch_stream(N_FRAMES, h, w, seed=11 + h, step=1)
    flow = hip_ctx.optical_flow(frames)
    hip_ctx.sync()
    assert flow.shape == (N_FRAMES - 1, h, w, 2)
    for p0 in (0, (N_FRAMES - 1) // 2 - 8, N_FRAMES - 1 - 16):
        part = hip_ctx.optical_flow(frames[p0:p0 + 17])
        hip_ctx.sync()
        assert torch.equal(flow[p0:p0 + 16].view(torch.int32), part.view(torch.int32)), (
            "pairs %d..%d differ between the large call and a 16-pair call" % (p0, p0 + 15),
            int((flow[p0:p0 + 16].view(torch.int32) != part.view(torch.int32)).sum()))
    i = 1000
    a, b = frames[i].cpu().numpy(), frames[i + 1].cpu().numpy()
    assert_flow_close(flow[i].cpu().numpy(), oracle.optical_flow_rgb(a, b), a, b, "%dx%d pair %d of %d" % (h, w, i, N_FRAMES - 1))
    assert np.isfinite(flow[-1].cpu().numpy()).all()


def test_gray_source_instance_in_tall_segments(hip_ctx):
    """k_polyexp_u8 (level 0 of the default four-level pyramid, calls above 16 pairs) at segment starts other than 0 and other
    than the 12-row grid small calls use: 1100 frames of 264 x 248 are 2200 columns, one whole-height segment before and
    segments of several dozen rows now (a ragged last one); the same pairs in 32-pair calls run 12-row segments."""
    import torch
    h, w, n = 264, 248, 1100
    strips = (w + PE_OUT - 1) // PE_OUT
    assert strips * n > 256 * 8 and old_rows(h, strips, n) == h
    rows = new_rows(h, strips, n, "u8")
    assert 12 < rows < h and h % rows and new_rows(h, strips, 33, "u8") == 12, rows
    frames = torch_stream(n, h, w, seed=5, step=1)
    flow = hip_ctx.optical_flow(frames)
    hip_ctx.sync()
    for p0 in (0, 500, n - 1 - 32):
        part = hip_ctx.optical_flow(frames[p0:p0 + 33])
        hip_ctx.sync()
        assert torch.equal(flow[p0:p0 + 32].view(torch.int32), part.view(torch.int32)), (
            "pairs %d..%d differ between the large call and a 32-pair call" % (p0, p0 + 31),
            int((flow[p0:p0 + 32].view(torch.int32) != part.view(torch.int32)).sum()))
    i = 700
    a, b = frames[i].cpu().numpy(), frames[i + 1].cpu().numpy()
    assert_flow_close(flow[i].cpu().numpy(), oracle.optical_flow_rgb(a, b), a, b, "%dx%d pair %d of %d" % (h, w, i, n - 1))
