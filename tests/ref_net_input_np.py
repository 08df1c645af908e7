"""numpy restatements of the two network-input ops, written from the contracts and independent of
the HIP code: every float32 operation below is one numpy float32 operation, so each is rounded once, as in the kernels.

  facenet_*     FacenetInput: geometry, and what follows the 8-bit resize (the resize itself is oracle.resize_u8's job)
  caffe_axis    one axis of CaffeInput's box filter: begin, first member, member count per output, in float32
  caffe_input   CaffeInput in float32, operation for operation (batched: the frames' axis stays vectorised)
  caffe_input64 the float64 DEFINITION: the same windows, exact means
  caffe_bound   how far the float32 restatement may be from the definition, derived below
"""
import numpy as np

F = np.float32


# ---- FacenetInput -------------------------------------------------------------------------------
def facenet_geometry(h, w, scale):
    """(net_h, net_w): floor(float(size) * scale) in float32, rounded up to a multiple of 8."""
    out = []
    for size in (h, w):
        v = int(np.floor(F(size) * F(scale)))
        out.append(v + (8 - v % 8) % 8)
    return tuple(out)


def facenet_from_resized(resized, mean_colors):
    """(n, net_h, net_w, 3) uint8 resized frames -> (n, 3, net_w, net_h) float32: minus the mean per channel (frame order),
    every plane transposed."""
    v = resized.astype(F) - np.asarray(mean_colors, F)      # exact conversion, one float32 rounding
    return np.ascontiguousarray(v.transpose(0, 3, 2, 1))


# ---- CaffeInput ---------------------------------------------------------------------------------
def caffe_axis(n_in, n_out):
    """(begin, first, count, contiguous) per output index, int arrays of n_out entries (first = -1 and count = 0 for an empty
    window); contiguous: the members of every window are consecutive taps."""
    scale = F(n_out) / F(n_in)
    ks = F(0.5) / scale
    src = (np.arange(n_out, dtype=F) + F(0.5)) / scale
    begin = (src - ks + F(0.5)).astype(np.int32)             # truncation, as int() of a float in C
    extent = int(F(2.0) * ks + F(1.0))
    k = np.arange(extent, dtype=np.int32)
    member = np.abs(((k[None, :] + begin[:, None]).astype(F) - src[:, None]) * scale) <= F(0.5)
    count = member.sum(1).astype(np.int32)
    first = np.where(count > 0, member.argmax(1), -1).astype(np.int32)
    last = np.where(count > 0, extent - 1 - member[:, ::-1].argmax(1), -2)
    return begin, first, count, bool(np.all((count == 0) | (last - first + 1 == count)))


def _box_pass(v, axis_len_in, n_out, axis, dtype):
    """The box filter along `axis` of v (that axis has axis_len_in samples): per output the members' sum of weight * sample,
    accumulated in member order (dtype float32: weight = 1.0f / m, product and sum rounded separately; float64: the mean)."""
    begin, first, count, _ = caffe_axis(axis_len_in, n_out)
    assert (count > 0).all(), "empty window"
    v = np.moveaxis(v, axis, 0)
    out = np.empty((n_out,) + v.shape[1:], dtype)
    for x in range(n_out):
        idx = np.minimum(begin[x] + first[x] + np.arange(count[x]), axis_len_in - 1)   # edge replication
        if dtype == np.float64:
            out[x] = v[idx].astype(np.float64).sum(0) / float(count[x])
        else:
            wgt = F(1.0) / F(count[x])
            acc = np.zeros(v.shape[1:], F)
            for i in idx:
                acc = acc + wgt * v[i].astype(F)
            out[x] = acc
    return np.moveaxis(out, 0, axis)


def _caffe(frames, net_h, net_w, mean_bgr, normalize, dtype):
    frames = np.asarray(frames)
    n, h, w, _ = frames.shape
    rx = _box_pass(frames, w, net_w, 2, dtype)               # horizontal pass first: (n, h, net_w, 3)
    ry = _box_pass(rx, h, net_h, 1, dtype)                   # (n, net_h, net_w, 3)
    v = np.clip(ry, dtype(0), dtype(255))
    v = v[..., ::-1] - np.asarray(mean_bgr, F).astype(dtype)  # plane c: input channel 2 - c, minus mean_colors[c]
    if normalize:
        v = v / dtype(255.0)
    return np.ascontiguousarray(v.transpose(0, 3, 1, 2))


def caffe_input(frames, net_h, net_w, mean_bgr, normalize=False):
    """(n, h, w, 3) uint8 RGB -> (n, 3, net_h, net_w) float32, the op's arithmetic operation for operation."""
    return _caffe(frames, net_h, net_w, mean_bgr, normalize, np.float32)


def caffe_input64(frames, net_h, net_w, mean_bgr, normalize=False):
    """The definition in float64: the same windows (membership is part of the contract), exact means."""
    return _caffe(frames, net_h, net_w, mean_bgr, normalize, np.float64)


def caffe_bound(h, w, net_h, net_w, mean_bgr, normalize=False):
    """max |caffe_input - caffe_input64|, with u = 2^-24 the unit roundoff of float32 and samples of at most 255:
      horizontal  m_x members: weight fl(1 / m_x) (relative u), each product (u), a sequential sum of m_x terms (at most
                  (m_x - 1) u on the running value): the result is within (m_x + 1) u x 255 of the exact mean
      vertical    the same over m_y rows, plus the horizontal error carried through weights that sum to 1 (1 + u):
                  (m_x + m_y + 2) u x 255, with 1 % of slack for the second-order terms
      clamp       does not expand an error
      mean        one rounding of a value of at most 255 + |mean|
      normalize   the error divided by 255, and one rounding of the quotient (at most (255 + |mean|) / 255)."""
    u = 2.0 ** -24
    mx, my = int(caffe_axis(w, net_w)[2].max()), int(caffe_axis(h, net_h)[2].max())
    top = 255.0 + float(np.abs(np.asarray(mean_bgr, np.float64)).max())
    e = 1.01 * (mx + my + 2) * u * 255.0 + u * top
    if normalize:
        e = e / 255.0 + u * top / 255.0
    return e
