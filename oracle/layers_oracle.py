"""float64 reference of mh_icp_align_layers: one ICP alignment over several (map, scan) point-layer pairs with one Gauss-Newton
solve (the contract in include/molahip.h above mh_icp_align_layers).

TEST INFRASTRUCTURE, like the rest of oracle/.  Matching is the C oracle's matcher per pair (bit-exact with the device by the
rules of DESIGN §3.1), or any matcher with its signature (tests/test_oracle_layers.py passes icp_oracle_np's).  The solve is a
vectorised numpy restatement: each pairing contributes the rows J = [R | -R [l]x], e = R l + t - q, weighted by its pair's
weight times the robust weight; T <- T exp(-H^-1 g).  Loop control (stall test, device hook, NoPairings, MaxIterations) and the
inner-step semantics (min_delta, max_cost) are those of icp_oracle_np.gn_solve / orc_icp_align.  Covariance: the C oracle's over
the union of the final pairings.

Every decision the loop takes on a floating-point comparison is recorded with its relative margin (`margins`), and the largest
condition number of the normal equations it solved (`max_cond`): a caller that compares against the device can tell a genuine
mismatch from a decision that sits within rounding of its threshold, or from a step that rounding decides (a rank-deficient H:
one or two distinct pairings, where the device's pivoted LDL^T, like the C oracle's, solves on pivots made of rounding)."""
from __future__ import annotations

import numpy as np

from oracle import icp_oracle_np as onp
from oracle import oracle_c

TERM_NO_PAIRINGS, TERM_SOLVER_ERROR, TERM_MAX_ITERATIONS, TERM_STALLED, TERM_HOOK_REQUEST = 1, 2, 3, 4, 6


def _hat_rows(l):
    """[l]x for every row of l (n, 3) -> (n, 3, 3)."""
    z = np.zeros(len(l))
    return np.stack([np.stack([z, -l[:, 2], l[:, 1]], 1), np.stack([l[:, 2], z, -l[:, 0]], 1),
                     np.stack([-l[:, 1], l[:, 0], z], 1)], 1)


def accumulate(T, blocks, kernel, c):
    """H, g, cost of the stacked point-to-point rows of every block (local_xyz, global_xyz, weight) at pose T (3x4 or 12)."""
    T = np.asarray(T, np.float64).reshape(-1)[:12].reshape(3, 4)
    R, t = T[:, :3], T[:, 3]
    H, g, cost = np.zeros((6, 6)), np.zeros(6), 0.0
    for L, Q, wpair in blocks:
        L = np.asarray(L, np.float32).astype(np.float64).reshape(-1, 3)
        Q = np.asarray(Q, np.float32).astype(np.float64).reshape(-1, 3)
        if len(L) == 0:
            continue
        e = L @ R.T + t - Q
        e2 = np.einsum("ij,ij->i", e, e)
        w = float(wpair) * onp.robust_weight(kernel, c, e2)
        J = np.concatenate([np.broadcast_to(R, (len(L), 3, 3)), -(R @ _hat_rows(L))], 2).reshape(-1, 6)  # 3 rows per pairing
        wJ = J * np.repeat(w, 3)[:, None]
        H += wJ.T @ J
        g += wJ.T @ e.reshape(-1)
        cost += float(np.sum(w * e2))
    return H, g, cost


def gn_solve(T, blocks, inner, kernel, c, prior=None, min_delta=1e-7, max_cost=0.0):
    """Solver_GaussNewton over the blocks: up to `inner` steps, the max_cost exit before a solve, the min_delta exit after one.
    Returns (T (4x4), steps [dict(H, g, cost, delta, cond)], ok, margins)."""
    T = onp.T44(np.asarray(T, np.float64).reshape(-1)[:12])
    steps, margins = [], []
    for _ in range(inner):
        H, g, cost = accumulate(T, blocks, kernel, c)
        if prior is not None:
            Hp, gp = onp.prior_term(prior, T)
            H, g = H + Hp, g + gp
        if max_cost > 0.0:
            margins.append(("max_cost", np.sqrt(cost), max_cost))
        if np.sqrt(cost) <= max_cost:
            steps.append(dict(H=H, g=g, cost=cost, delta=np.zeros(6)))
            break
        cond = float(np.linalg.cond(H)) if np.all(np.isfinite(H)) else np.inf
        try:
            delta = -np.linalg.solve(H, g)
        except np.linalg.LinAlgError:  # exactly singular: the least-squares step (a zero pivot contributes nothing)
            delta = -np.linalg.lstsq(H, g, rcond=None)[0]
        if not np.all(np.isfinite(delta)):
            steps.append(dict(H=H, g=g, cost=cost, delta=delta, cond=cond))
            return T, steps, False, margins
        T = T @ onp.se3_exp(delta)
        steps.append(dict(H=H, g=g, cost=cost, delta=delta, cond=cond))
        dn = float(np.linalg.norm(delta))
        if min_delta > 0.0:
            margins.append(("min_delta", dn, min_delta))
        if dn < min_delta:
            break
    return T, steps, True, margins


def _sched(v, n):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float64), (max(1, n),)))


def icp_align_layers(pairs, T_guess, p: oracle_c.ICPParams, prior=None, matcher=None, n_threads=1):
    """pairs: dicts {map, local (n x 3), threshold (scalar or max_iterations values), threshold_angular_deg=0, weight=1};
    `map` is whatever `matcher(map, local, T, threshold, angular_deg)` takes (default: oracle_c.match_points on an
    oracle_c.Map).  p: oracle_c.ICPParams (threshold, threshold_angular_deg and gn.weight_pt2pt are not used: every pair carries
    its own).  Returns the keys of capi.icp_align_layers(..., want_pairs=True), plus `margins`: (name, value, threshold) of every
    stall / hook / min_delta / max_cost comparison the loop made."""
    if matcher is None:
        def matcher(m, loc, T, thr, ang):
            return oracle_c.match_points(m, loc, T, thr, ang, n_threads=n_threads)
    mi = int(p.max_iterations)
    locs = [np.asarray(e["local"], np.float32).reshape(-1, 3) for e in pairs]
    thrs = [_sched(e["threshold"], mi) for e in pairs]
    angs = [float(e.get("threshold_angular_deg", 0.0) or 0.0) for e in pairs]
    wts = [float(e.get("weight", 1.0)) for e in pairs]
    kp = _sched(p.kernel_param, mi)
    potential = int(sum(len(l) for l in locs))
    T0 = np.asarray(T_guess, np.float64).reshape(-1)[:12].copy()
    chk = np.asarray(p.hook_checkpoint if p.hook_checkpoint is not None else T0, np.float64).reshape(-1)[:12]
    chk_inv = oracle_c.pose_inverse(chk)
    empty = dict(local_idx=np.zeros(0, np.uint32), global_idx=np.zeros(0, np.uint32), global_xyz=np.zeros((0, 3), np.float32),
                 d2=np.zeros(0, np.float32))
    out = dict(T=T0.copy(), n_iterations=0, termination_reason=TERM_MAX_ITERATIONS, n_final_pairs=0, potential_pairings=potential,
               quality=0.0, pair_counts=[0] * len(pairs), pairs=[dict(empty) for _ in pairs], trace=[], cov=np.eye(6) * 1e6,
               margins=[], max_cond=0.0)
    if mi == 0:
        return out
    if potential == 0:
        out["termination_reason"] = TERM_NO_PAIRINGS
        return out
    T, Tprev = T0.copy(), T0.copy()
    term, it, last = TERM_MAX_ITERATIONS, mi, None
    margins = out["margins"]
    for k in range(mi):
        last = [matcher(pairs[i]["map"], locs[i], T, float(thrs[i][k]), angs[i]) for i in range(len(pairs))]
        n_pairs = int(sum(len(r["local_idx"]) for r in last))
        if n_pairs == 0:
            term, it = TERM_NO_PAIRINGS, k
            break
        blocks = [(locs[i][r["local_idx"]], r["global_xyz"], wts[i]) for i, r in enumerate(last)]
        T44, steps, ok, m = gn_solve(T, blocks, p.gn.max_inner_iterations, p.gn.robust_kernel, float(kp[k]), prior=prior,
                                     min_delta=p.gn.min_delta, max_cost=p.gn.max_cost)
        margins += m
        out["max_cond"] = max([out["max_cond"]] + [st_["cond"] for st_ in steps if "cond" in st_])
        if not ok:
            term, it = TERM_SOLVER_ERROR, k
            break
        T = onp.T12(T44)
        d = oracle_c.se3_log(oracle_c.pose_compose(oracle_c.pose_inverse(Tprev), T))
        dtr, drot = float(np.linalg.norm(d[:3])), float(np.linalg.norm(d[3:]))
        out["trace"].append(dict(T=T.copy(), n_pairs=n_pairs, threshold=float(thrs[0][k]), kernel_param=float(kp[k]),
                                 delta_trans=dtr, delta_rot=drot))
        if not p.disable_stall_test:
            margins += [("stall_trans", dtr, p.min_abs_step_trans), ("stall_rot", drot, p.min_abs_step_rot)]
            if dtr < p.min_abs_step_trans and drot < p.min_abs_step_rot:
                term, it = TERM_STALLED, k
                break
        if p.hook_enabled:
            S = oracle_c.pose_compose(chk_inv, T)
            ht = float(np.linalg.norm(S.reshape(3, 4)[:, 3]))
            hr = float(np.linalg.norm(oracle_c.so3_log(S)))
            margins += [("hook_trans", ht, p.hook_min_trans), ("hook_rot", hr, p.hook_min_rot)]
            if ht > p.hook_min_trans or hr > p.hook_min_rot:
                term, it = TERM_HOOK_REQUEST, k
                break
        Tprev = T.copy()
    out.update(T=T, n_iterations=it, termination_reason=term)
    if term == TERM_NO_PAIRINGS:
        return out
    n_final = int(sum(len(r["local_idx"]) for r in last))
    out["n_final_pairs"] = n_final
    out["quality"] = n_final / potential if n_final else 0.0
    out["pair_counts"] = [len(r["local_idx"]) for r in last]
    out["pairs"] = [dict(local_idx=np.asarray(r["local_idx"], np.uint32), global_idx=np.asarray(r["global_idx"], np.uint32),
                         global_xyz=np.asarray(r["global_xyz"], np.float32).reshape(-1, 3), d2=np.asarray(r["d2"], np.float32))
                    for r in last]
    if p.compute_covariance and term != TERM_SOLVER_ERROR:
        lp = np.concatenate([locs[i][r["local_idx"]] for i, r in enumerate(last)])
        gp = np.concatenate([np.asarray(r["global_xyz"], np.float32).reshape(-1, 3) for r in last])
        out["cov"] = oracle_c.covariance(T, pt2pt=(lp, gp), findif_xyz=p.cov_findif_xyz, findif_ang=p.cov_findif_ang)[0]
    return out


def nearest_decision(margins):
    """The comparison of `margins` closest to its threshold, relative: (name, |value - threshold| / threshold) or None."""
    best = None
    for name, v, thr in margins:
        if thr > 0 and np.isfinite(v):
            r = abs(v - thr) / thr
            if best is None or r < best[1]:
                best = (name, r)
    return best


def compare(r, o, pose_tol=1e-7, with_pairs=True):
    """What differs between a device result (capi.icp_align_layers(..., want_pairs=True)) and the reference's `o`: a list of
    one-line descriptions, empty when they agree.  Exact: iteration count, termination reason, every count, each iteration's
    pairing count, quality, and (with_pairs) every pair's local_idx, global_idx and d2.  Poses of the trace and the result to
    pose_tol; the covariance to the tolerance of test_gpu_parity.py::test_covariance_matches_oracle."""
    bad = []
    for k in ("n_iterations", "termination_reason", "n_final_pairs", "potential_pairings", "pair_counts", "quality"):
        if r[k] != o[k]:
            bad.append("%s %r vs %r" % (k, r[k], o[k]))
    tr, to = [t["n_pairs"] for t in r["trace"]], [t["n_pairs"] for t in o["trace"]]
    if tr != to:
        first = next((i for i, (x, y) in enumerate(zip(tr, to)) if x != y), min(len(tr), len(to)))
        bad.append("trace n_pairs differ from iteration %d (%s vs %s; lengths %d vs %d)" % (
            first, tr[first] if first < len(tr) else None, to[first] if first < len(to) else None, len(tr), len(to)))
    if with_pairs and r["pair_counts"] == o["pair_counts"]:
        for i, (x, y) in enumerate(zip(r["pairs"], o["pairs"])):
            for k in ("local_idx", "global_idx", "d2"):
                if not np.array_equal(x[k], y[k]):
                    nd = int(np.sum(x[k] != y[k]))
                    bad.append("pair %d: %d %s values differ" % (i, nd, k))
    dT = float(np.abs(np.asarray(r["T"]) - o["T"]).max())
    if not dT < pose_tol:
        bad.append("max |dT| %.3e" % dT)
    for i, (x, y) in enumerate(zip(r["trace"], o["trace"])):
        d = float(np.abs(np.asarray(x["T"]) - y["T"]).max())
        if not d < pose_tol:
            bad.append("trace pose %d: max |dT| %.3e" % (i, d))
            break
    cg, co = np.asarray(r["cov"]).reshape(6, 6), np.asarray(o["cov"]).reshape(6, 6)
    if not np.allclose(cg, co, rtol=2e-5, atol=1e-6 * np.abs(co).max()):
        bad.append("covariance: max |d| %.3e of max %.3e" % (float(np.abs(cg - co).max()), float(np.abs(co).max())))
    return bad
