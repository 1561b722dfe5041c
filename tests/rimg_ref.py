"""numpy restatement of mh_scan_edges_from_range_image (include/molahip.h states the rule): int64 scores, float32
operations in the written order, float64 where written.  Test helper only: no product code."""
import numpy as np


def scores(R, W):
    """(scored mask, int64 score) per pixel of the uint16 image R[rows, cols] for a window of radius W."""
    R = np.asarray(R)
    assert R.dtype == np.uint16 and R.ndim == 2
    rows, cols = R.shape
    scored = np.zeros((rows, cols), bool)
    S = np.zeros((rows, cols), np.int64)
    if cols < 2 * W + 1:
        return scored, S
    r64 = R.astype(np.int64)
    cs = np.concatenate([np.zeros((rows, 1), np.int64), np.cumsum(r64, axis=1)], axis=1)
    zs = np.concatenate([np.zeros((rows, 1), np.int64), np.cumsum(R == 0, axis=1)], axis=1)
    c = np.arange(W, cols - W)
    wsum = cs[:, c + W + 1] - cs[:, c - W]
    wzero = zs[:, c + W + 1] - zs[:, c - W]
    scored[:, W:cols - W] = wzero == 0
    S[:, W:cols - W] = wsum - (2 * W + 1) * r64[:, W:cols - W]
    S[~scored] = 0
    return scored, S


def classify(R, W, score_threshold):
    """(edge mask, plane mask): edge iff float32(|S|) > float32(threshold), strictly; every other scored pixel is a plane."""
    scored, S = scores(R, W)
    edge = scored & (np.abs(S).astype(np.float32) > np.float32(score_threshold))
    return edge, scored & ~edge


def points(R, mask, fx, fy, cx, cy, range_units, range_is_depth, sensor_pose):
    """float32 xyz [k, 3] of the pixels of `mask`, in row-major pixel order, in the vehicle frame."""
    f32 = np.float32
    r, c = np.nonzero(mask)  # row-major order
    d = R[r, c].astype(f32) * f32(range_units)
    kx = (f32(cx) - c.astype(f32)) / f32(fx)
    ky = (f32(cy) - r.astype(f32)) / f32(fy)
    assert d.dtype == f32 and kx.dtype == f32 and ky.dtype == f32
    if range_is_depth:
        xs = d
    else:
        kx64, ky64 = kx.astype(np.float64), ky.astype(np.float64)
        xs = (d.astype(np.float64) / np.sqrt((1.0 + kx64 * kx64) + ky64 * ky64)).astype(f32)
    ys = xs * kx
    zs = xs * ky
    P = np.asarray(sensor_pose, np.float64).reshape(-1)[:12]
    X, Y, Z = xs.astype(np.float64), ys.astype(np.float64), zs.astype(np.float64)
    out = np.empty((len(r), 3), f32)
    for i in range(3):
        out[:, i] = (((P[4 * i] * X + P[4 * i + 1] * Y) + P[4 * i + 2] * Z) + P[4 * i + 3]).astype(f32)
    return out


def generate(R, W, score_threshold, fx, fy, cx, cy, range_units, range_is_depth, sensor_pose):
    """(edges xyz, planes xyz, edges pixel index, planes pixel index)."""
    edge, plane = classify(R, W, score_threshold)
    cols = R.shape[1]
    idx = lambda m: (np.nonzero(m)[0] * cols + np.nonzero(m)[1]).astype(np.uint32)
    cam = (fx, fy, cx, cy, range_units, range_is_depth, sensor_pose)
    return points(R, edge, *cam), points(R, plane, *cam), idx(edge), idx(plane)
