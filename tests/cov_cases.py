"""Inputs, poses, scaling and the bound of the covariance checks against the closed-form Jacobian
(oracle/icp_oracle_np.py::covariance_analytic), shared by tests/test_oracle_gn.py (CPU: the C and numpy oracles, where the bound
is measured) and tests/test_gpu_solver_params.py (GPU: mh_covariance and the fused covariance, held to that bound)."""
import numpy as np

# (yaw, pitch, roll) well outside the small angles of the alignments; the last pose sits 800 m from the origin
COV_POSES = [(1.0, -2.0, 0.5, 0.4, -0.02, 0.05), (-3.0, 4.0, 1.0, 2.8, 1.2, -0.7), (500.0, -800.0, 3.0, -2.0, 0.3, 0.1)]
COV_KINDS = ("points", "planes", "both")


def cov_inputs(kind, n, spread, seed=0):
    """(pt2pt, pt2pl) of a covariance call: n pairings of each requested kind on a cloud of the given spread [m]."""
    rng = np.random.default_rng(1000 * seed + n + int(spread))
    pp = pl = None
    if kind in ("points", "both"):
        l = rng.normal(0, spread, (n, 3)).astype(np.float32)
        pp = (l, (l + rng.normal(0, 0.05, (n, 3))).astype(np.float32))
    if kind in ("planes", "both"):
        l = rng.normal(0, spread, (n, 3)).astype(np.float32)
        nrm = rng.normal(0, 1, (n, 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        pl = (l, (l + rng.normal(0, 0.2, (n, 3))).astype(np.float32), nrm.astype(np.float32))
    return pp, pl


def scaled_gap(cov, ref):
    """max |cov - ref| after scaling both by 1 / sqrt(diag(ref)): the angular block of a covariance is ~1e-2 of the
    translational one and smaller, an absolute tolerance sized by the largest entry would not see it."""
    s = 1.0 / np.sqrt(np.diag(ref))
    return float(np.abs((cov - ref) * np.outer(s, s)).max())


# The C oracle at its default steps (1e-7, 1e-7) against the closed form over the inputs of
# tests/test_oracle_gn.py::test_covariance_matches_the_closed_form, scaled: the
# largest gap measured is 6.88e-7, at the pose 800 m out (its translation column is ((y + h) - (y - h)) / 2h with
# ulp(800) / 2h = 5.7e-7 of rounding; <= 3.9e-8 at the other two poses).  The bound is ten times that: the gap is rounding
# of size eps |x| / h, and the rounding of a second finite-difference implementation (the device) is its own.
COV_FD_MEASURED = 6.88e-7
COV_FD_BOUND = 10 * COV_FD_MEASURED
