"""numpy restatement of the FacenetOutput contract: every operation an IEEE float32 operation
rounded on its own, exponentials through float64, the greedy suppression as written there.  Shares no code with the
library; the GPU tests compare with it bit for bit.  Also the seeded maps and templates the tests draw."""
import numpy as np

F = np.float32
VALID = [4, 5, 6, 7, 8, 9, 10, 11, 18, 19, 20, 21, 22, 23, 24]
BIG_VALID = [4, 5, 6, 7, 8, 9, 10, 11]


def geometry(h, w, scale):
    """(net_h, net_w, grid_h, grid_w): floor of the float32 product, padded to a multiple of 8, then ceil(net / 8)."""
    fw, fh = np.floor(F(w) * F(scale)), np.floor(F(h) * F(scale))
    nw, nh = int(fw), int(fh)
    nw += -nw % 8
    nh += -nh % 8
    return nh, nw, -(-nh // 8), -(-nw // 8)


def exp32(v):
    """The correctly rounded float32 of the float64 exponential."""
    with np.errstate(over="ignore", under="ignore"):
        return np.exp(np.asarray(v, F).astype(np.float64)).astype(F)


def templates(seed=0):
    """25 x 4 plausible template corners (x1, y1, x2, y2), sizes growing with the index, fractional parts included."""
    rng = np.random.default_rng(1000 + seed)
    t = np.arange(25, dtype=np.float64)
    hw, hh = 2.0 + 1.1 * t + rng.uniform(0, 1, 25), 2.5 + 1.3 * t + rng.uniform(0, 1, 25)
    return np.stack([-hw, -hh, hw, hh], axis=1).astype(F)


def make_map(seed, grid_w, grid_h, bias, sigma=0.3):
    """One detector map (125, grid_w, grid_h): confidence logits normal(bias, 1), adjustments normal(0, sigma)."""
    rng = np.random.default_rng(seed)
    m = np.empty((125, grid_w, grid_h), F)
    m[:25] = rng.normal(bias, 1.0, (25, grid_w, grid_h))
    m[25:] = rng.normal(0.0, sigma, (100, grid_w, grid_h))
    return m


def decode(map_, h, w, scale, T, threshold):
    """Survivors in candidate order: (rows float32 (m, 5), candidate indices, the scores of ALL candidates)."""
    nh, nw, gh, gw = geometry(h, w, scale)
    G = gw * gh
    map_ = np.asarray(map_, F).reshape(125, gw, gh)
    T = np.asarray(T, F).reshape(25, 4)
    valid = BIG_VALID if F(scale) > F(1.0) else VALID
    conf = np.stack([map_[t] for t in valid])                                  # (nv, gw, gh): t, xi, yi = candidate order
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        e = exp32(-conf)
        score = (1.0 / (1.0 + e.astype(np.float64))).astype(F)
        passed = ~(score.astype(np.float64) < np.float64(F(threshold)))
        xi, yi = np.meshgrid(np.arange(gw), np.arange(gh), indexing="ij")
        x = np.broadcast_to((xi * 8 - 1).astype(F), conf.shape)
        y = np.broadcast_to((yi * 8 - 1).astype(F), conf.shape)
        tw = np.stack([np.full((gw, gh), (T[t, 2] - T[t, 0]) + F(1)) for t in valid]).astype(F)
        th = np.stack([np.full((gw, gh), (T[t, 3] - T[t, 1]) + F(1)) for t in valid]).astype(F)
        adj = map_[25:].reshape(4, 25, gw, gh)
        dcx, dcy, dcw, dch = (np.stack([adj[k, t] for t in valid]) for k in range(4))
        x = x + tw * dcx
        y = y + th * dcy
        bw = tw * exp32(dcw)
        bh = th * exp32(dch)
        x = (x / F(nw)) * F(w)
        y = (y / F(nh)) * F(h)
        bw = (bw / F(nw)) * F(w)
        bh = (bh / F(nh)) * F(h)
        ok = passed & ~((bw < 0) | (bh < 0) | np.isnan(bw) | np.isnan(bh) | np.isnan(x) | np.isnan(y))
        x1, y1 = (x - bw / F(2)) / F(w), (y - bh / F(2)) / F(h)
        x2, y2 = (x + bw / F(2)) / F(w), (y + bh / F(2)) / F(h)
    for a in (x, y, bw, bh, x1, score):
        assert a.dtype == F
    rows = np.stack([x1, y1, x2, y2, score], axis=-1).reshape(-1, 5)
    idx = np.flatnonzero(ok.reshape(-1))
    assert len(rows) == len(valid) * G
    return rows[idx], idx, score.reshape(-1)


def _smin(a, b):
    return np.where(b < a, b, a)     # std::min


def _smax(a, b):
    return np.where(a < b, b, a)     # std::max


def nms(rows, overlap=0.1, offset=0.0):
    """Kept row indices, in kept order."""
    rows = np.asarray(rows, F).reshape(-1, 5)
    m = len(rows)
    if m == 0:
        return np.zeros(0, np.int64)
    x1, y1, x2, y2 = (rows[:, k] for k in range(4))
    bits = rows[:, 4].copy().view(np.uint32)
    order = np.lexsort((np.arange(m), ~bits))                                  # score bits descending, then index ascending
    o, thr, zero = F(offset), F(overlap), F(0)
    valid = np.ones(m, bool)
    kept = []
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        area = ((x2 - x1) + o) * ((y2 - y1) + o)
        for c in order:
            if not valid[c]:
                continue
            kept.append(c)
            iw = _smax(zero, (_smin(x2[c], x2) - _smax(x1[c], x1)) + o)
            ih = _smax(zero, (_smin(y2[c], y2) - _smax(y1[c], y1)) + o)
            ov = (iw * ih) / area
            assert ov.dtype == F
            valid[c] = False                                                   # visited: never looked at again
            valid &= ov < thr
    return np.asarray(kept, np.int64)


def facenet_output(map_, h, w, scale, T, threshold, overlap=0.1, offset=0.0):
    """The kept rows [x1, y1, x2, y2, score] of one frame, in kept order."""
    rows, _, _ = decode(map_, h, w, scale, T, threshold)
    return rows[nms(rows, overlap, offset)]


def threshold_margin(map_, h, w, scale, T, threshold):
    """The smallest |score - threshold| over all candidates: the tests require it to exceed 1e-6, so that no decision
    rests on a last bit of the sigmoid."""
    _, _, score = decode(map_, h, w, scale, T, threshold)
    return float(np.abs(score.astype(np.float64) - np.float64(F(threshold))).min())
