"""De-skew with a piecewise motion table, restated in numpy float64 -- no product code.

 * deskew_motion: the DEVICE rule of include/molahip_motion.h, per point;
 * GyroBufferRef / build_motion_table: the HOST rule of mola_lidar_odometry_hip/GyroDeskew.h, gyro samples to table;
 * constant_rate_table: the table a constant rate w cuts at given knots (what makes the rule equal mh_scan_deskew)."""
import numpy as np

MAX_SEGMENTS = 64
DEFAULTS = dict(enabled=False, window=[-0.06, 0.06], segments=12, max_gap=0.02, time_zero_offset=0.0, gyro_bias=[0.0, 0.0, 0.0],
                sensor_rotation=[1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], buffer_seconds=2.0)


def so3_exp(w):
    """Rodrigues for rotation vectors w [..., 3] -> [..., 3, 3]; the series below 1e-2 rad as the library's rodrigues_coeffs."""
    w = np.asarray(w, np.float64)
    th2 = (w * w).sum(-1)
    th = np.sqrt(th2)
    with np.errstate(invalid="ignore", divide="ignore"):
        small = th < 1e-2
        a_s = 1.0 - th2 / 6.0 * (1.0 - th2 / 20.0 * (1.0 - th2 / 42.0))
        b_s = 0.5 - th2 / 24.0 * (1.0 - th2 / 30.0 * (1.0 - th2 / 56.0))
        a_l = np.sin(th) / th
        b_l = 2.0 * np.sin(0.5 * th) ** 2 / th2
        a = np.where(small, a_s, a_l)
        b = np.where(small, b_s, b_l)
        x, y, z = w[..., 0], w[..., 1], w[..., 2]
        zero = np.zeros_like(x)
        W = np.stack([np.stack([zero, -z, y], -1), np.stack([z, zero, -x], -1), np.stack([-y, x, zero], -1)], -2)
        W2 = W @ W
        return np.eye(3) + a[..., None, None] * W + b[..., None, None] * W2


def segment_of(knots, t):
    """s = clamp(#{k : knot_k <= t} - 1, 0, K - 1); a NaN stamp counts no knot"""
    knots = np.asarray(knots, np.float64)
    t = np.asarray(t, np.float64)
    with np.errstate(invalid="ignore"):
        cnt = (knots[None, :] <= t[:, None]).sum(1)
    return np.clip(cnt - 1, 0, len(knots) - 1)


def deskew_motion(xyz, t32, knots, R, w, v):
    """float64 [n, 3]: R_s Exp_SO3(w_s (t - knot_s)) p + v t with t = float64(float32 stamp); NOT rounded to float"""
    p = np.asarray(xyz, np.float32).astype(np.float64).reshape(-1, 3)
    t = np.asarray(t32, np.float32).astype(np.float64)
    knots = np.asarray(knots, np.float64)
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    w = np.asarray(w, np.float64).reshape(-1, 3)
    v = np.asarray(v, np.float64).reshape(3)
    s = segment_of(knots, t)
    with np.errstate(invalid="ignore", over="ignore"):
        d = t - knots[s]
        u = np.einsum("nij,nj->ni", so3_exp(w[s] * d[:, None]), p)
        return np.einsum("nij,nj->ni", R[s], u) + v[None, :] * t[:, None], s


def constant_rate_table(knots, w):
    """(R [K, 3, 3], w [K, 3]) of a constant rate: R_s = Exp_SO3(w knot_s)"""
    knots = np.asarray(knots, np.float64)
    w = np.asarray(w, np.float64)
    return so3_exp(w[None, :] * knots[:, None]), np.repeat(w[None, :], len(knots), 0)


# ---- the host rule -------------------------------------------------------------------------------------------------------------------
class GyroBufferRef:
    """samples in strictly increasing time; one whose time does not increase (or is not finite) is dropped and counted"""

    def __init__(self, buffer_seconds=2.0):
        self.t, self.w, self.dropped, self.buffer_seconds = [], [], 0, float(buffer_seconds)

    def push(self, t, w):
        w = [float(c) for c in w]
        if not np.isfinite(t) or not np.all(np.isfinite(w)) or (self.t and not t > self.t[-1]):
            self.dropped += 1
            return False
        self.t.append(float(t))
        self.w.append(w)
        while self.t and self.t[0] < t - self.buffer_seconds:
            self.t.pop(0), self.w.pop(0)
        return True


def _mean_rate(tau, W, a, b):
    """the mean over [a, b] of the linear interpolant of (tau, W): its exact integral, piece by piece, divided by b - a"""
    def f(x, j):  # on the sample interval [tau_j, tau_j+1]
        return W[j] + (W[j + 1] - W[j]) * ((x - tau[j]) / (tau[j + 1] - tau[j]))
    j = int(np.searchsorted(tau, a, side="right")) - 1  # tau_j <= a
    j = min(max(j, 0), len(tau) - 2)
    acc = np.zeros(3)
    x0 = a
    while x0 < b:
        x1 = min(b, tau[j + 1])
        acc = acc + 0.5 * (f(x0, j) + f(x1, j)) * (x1 - x0)
        x0 = x1
        if j + 2 < len(tau):
            j += 1
        elif x0 < b:
            raise AssertionError("no coverage")
    return acc / (b - a)


def build_motion_table(buf, timestamp, opt, v):
    """None (no coverage) or dict(knots [K], R [K, 3, 3], w [K, 3], v [3])"""
    o = dict(DEFAULTS, **opt)
    lo, hi = (float(c) for c in o["window"])
    K = int(o["segments"])
    t0 = float(timestamp) + float(o["time_zero_offset"])
    tau = np.array(buf.t, np.float64) - t0
    W = np.array(buf.w, np.float64).reshape(-1, 3)
    below = np.nonzero(tau <= lo)[0]
    above = np.nonzero(tau >= hi)[0]
    if not len(below) or not len(above):
        return None
    ia, ib = int(below[-1]), int(above[0])
    if np.any(np.diff(tau[ia:ib + 1]) > float(o["max_gap"])):
        return None
    tau, W = tau[ia:ib + 1], W[ia:ib + 1]
    h = (hi - lo) / K
    knots = lo + np.arange(K) * h
    bias = np.array(o["gyro_bias"], np.float64)
    Rsv = np.array(o["sensor_rotation"], np.float64).reshape(3, 3)
    w = np.zeros((K, 3))
    for s in range(K):
        w[s] = Rsv @ (_mean_rate(tau, W, knots[s], (lo + (s + 1) * h) if s + 1 < K else hi) - bias)
    A = [np.eye(3)]
    for s in range(K - 1):
        A.append(A[-1] @ so3_exp(w[s] * h))
    s0 = int(segment_of(knots, np.array([0.0]))[0])
    Z = A[s0] @ so3_exp(w[s0] * (0.0 - knots[s0]))
    R = np.stack([Z.T @ a for a in A])
    return dict(knots=knots, R=R, w=w, v=np.array(v, np.float64).reshape(3))


# ---- the driver with the block: the CPU oracle's driver, its de-skew replaced ---------------------------------------------------------
def _oracle_base():
    from oracle import odometry_oracle as oo
    return oo.OdometryOracle


class MotionOracle(_oracle_base()):
    """OdometryOracle with the gyro_deskew: block: only _deskew_layers() is overridden.  on_gyro() feeds the buffer; a scan whose
    sweep the samples cover is de-skewed by the device rule with the host rule's table and the current vx, vy, vz (the rotations
    are cut once per scan: the twist hook changes v only), any other scan by the constant twist as before."""

    def __init__(self, *a, gyro_options=None, **kw):
        self.gyro_opt = dict(DEFAULTS, enabled=True, **(gyro_options or {}))
        self.gyro = GyroBufferRef(self.gyro_opt["buffer_seconds"])
        self._table_for = (None, None)
        super().__init__(*a, **kw)

    def on_gyro(self, t, w):
        self.gyro.push(t, w)

    def _deskew_layers(self):
        rec = self.records[-1]
        stamp = rec["timestamp"]
        if self._table_for[0] != (len(self.records), stamp):
            tab = build_motion_table(self.gyro, stamp, self.gyro_opt, np.zeros(3)) if self._t is not None else None
            self._table_for = ((len(self.records), stamp), tab)
        tab = self._table_for[1]
        rec["gyro_deskew"], rec["gyro_segments"] = tab is not None, 0 if tab is None else len(tab["knots"])
        if tab is None:
            return super()._deskew_layers()
        v = np.array([self.vars[k] for k in ("vx", "vy", "vz")])
        for name, idx in (("for_map", self.idx_map), ("for_icp", self.idx_icp)):
            out, _ = deskew_motion(self._xyz[idx], self._ta[idx], tab["knots"], tab["R"], tab["w"], v)
            setattr(self, name, np.ascontiguousarray(out.astype(np.float32)))
