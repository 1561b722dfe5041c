"""Every search route on a warm map after each kind of map update: include/molahip.h (twice) and include/molahip_live.h promise
that after mh_map_restore, mh_map_insert_frames and mh_map_erase_points / mh_map_erase_seen_through the map gives "the same
answers from every search route".  The routes are route_tables.MUTATION_ROUTES, the updates, inputs and references
tests/mutation_cases.py's; tests/test_mutation_cpu.py shows on the references alone that the partners change, that the hash table
size is kept by some kinds and changed by others, and that no (update, kind, route) is set apart.

Per route, on the handle that is updated and with scans that stay alive for the whole test:
  1. warm: the route runs twice with identical parameters, each run held to the oracle of the map BEFORE the update (the first
     run records the context's graph candidate, the second captures it; the lazy sub-voxel index is built and valid);
  2. the update -- no info() or download() between a queued update and the search behind it (a twin handle is downloaded and
     compared with the reference's dump first);
  3. one run, held to the oracle of the map AFTER the update: alignments in test_gpu_dense_cells.py's terms (iterations,
     termination, per-iteration pair counts, final pairings element by element, T within 1e-9), granular queries as
     test_gpu_parity.py compares them; capi.loop_stats() / flat_stats() show that the intended kernel ran;
  4. for the queued updates, nn_search and the alignments under MH_MATCH=q and f again from a scan of a second context of the
     same device, directly behind the update: the bits of the own-context result;
  5. the same run under MH_NO_GRAPH=1: the bits of the (replayed) one.

A one-launch loop that gives up arms a hold-off that would change the kernels later test files run: every run asserts that no
loop was abandoned."""
import contextlib
import importlib.util
import os

import numpy as np
import pytest

import dense_cases as dc
import mutation_cases as mc
import radius_ref as rr
import score_ref as sr
from mola_lidar_odometry_amd import capi
from route_tables import loop_expected

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _module(name):
    spec = importlib.util.spec_from_file_location("_" + name, os.path.join(ROOT, "tests", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# the comparison of an alignment with the oracle has ONE definition (loaded by path under a private name, as
# tests/test_gpu_solver_params.py does: nothing of it is collected here)
_dense = _module("test_gpu_dense_cells")
_assert_single_is_the_oracles, _check = _dense._assert_single_is_the_oracles, _dense._check
TIMING = ("match_kernel_ms", "total_ms", "n_match_launches", "n_host_polls", "n_enqueued_iterations")


@pytest.fixture(scope="module")
def contexts(oracle):
    """[0]: the maps' context; [1]: the second context of step 4; [2:5]: the lock-step batch's three"""
    cs = [capi.Context(0) for _ in range(5)]
    yield cs
    for c in cs:
        c.close()


class Dev:
    """A device map of a kind in the state of mutation_cases.before(kind) on one context, the scans of that context (one
    capi.Scan per host array, alive until close()), and what the updates need beside the map."""

    def __init__(self, kind, ctx, monkeypatch, with_map=True):
        self.kind, self.ctx, self.monkeypatch = kind, ctx, monkeypatch
        self._scans, self._views = {}, None
        self.m, self.occ = mc.first_device_map(kind, ctx) if with_map else (None, None)

    def scan(self, xyz):
        key = (xyz.ctypes.data, xyz.shape)
        if key not in self._scans:
            self._scans[key] = (capi.Scan(self.ctx, xyz), xyz)
        return self._scans[key][0]

    def views(self):
        if self._views is None:
            from mola_lidar_odometry_amd import capi_clean
            self._views = capi_clean.Views(self.ctx, capi_clean.clean_params(**mc.VIEW_PARAMS)).add_frames(mc.view_clouds())
        return self._views

    def reset(self):
        """the used handle back in the state of before(kind)"""
        if self.occ is not None:
            self.occ.clear()
            self.occ.insert(self.scan(mc.occ_scans(self.kind)[0]), mc.OCC_T[0])
            self.m = self.occ.search_map(mc.VS)
        else:
            mc.first_state(self.kind, self.m, self.ctx)

    def close(self):
        for s, _ in self._scans.values():
            s.close()
        for h in (self._views, self.m, self.occ):
            if h is not None:
                h.close()
        self._scans, self._views, self.m, self.occ = {}, None, None, None


@contextlib.contextmanager
def _env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        yield
    finally:
        for k in env:
            monkeypatch.delenv(k, raising=False)


# ------------------------------------------------------------------------------------------------------------ one run of a route
def _run(dev, row, sdev=None):
    """one call of the route on dev.m; the scans belong to `sdev` (a Dev of another context) or to dev"""
    sd, kind, name = sdev or dev, dev.kind, row["name"]
    s = mc.the_scan(kind)
    if row["family"] == "align":
        n = row["n"]
        return capi.icp_align(dev.m, sd.scan(s[:n]), mc.T0, mc.align_params(capi, kind, row.get("inner", 2), row.get("skip", False)),
                              prior=mc.prior(n), want_pairs=True)
    if row["family"] == "layers":
        c = mc.layer_cases(kind)[name]
        pairs, ks = dc.device_pairs(c, {"m": dev.m}, sd.scan)
        return capi.icp_align_layers(pairs, c["T0"], dc.device_params(c), prior=c["prior"], want_pairs=True, pairings_per_point=ks)
    q = sd.scan(s[:2000])
    if name == "dense":
        return capi.nn_search_dense(dev.m, q, mc.T0)
    if name == "nn":
        return capi.nn_search(dev.m, q, mc.T0, mc.NN_THR)
    if name == "nn_k3":
        return capi.nn_search_k(dev.m, q, mc.T0, mc.K3_THR, 3)
    if name in ("radius", "radius_sorted"):
        return capi.nn_search_radius(dev.m, sd.scan(s[:mc.N_RADIUS]), mc.T0, mc.RADIUS, sorted=name == "radius_sorted")
    if name == "score16":
        return capi.score_poses(dev.m, q, mc.score_poses16(), mc.SCORE_THR)
    if name == "pt2pl":
        return capi.nn_search_pt2pl(dev.m, q, mc.T0, mc.PL_THR)
    assert name == "pt2pl_knn", name
    P = mc.PLANE
    return capi.nn_search_pt2pl_knn(dev.m, q, mc.T0, 0.4, P["plane_eigen_threshold"], P["search_radius"], P["knn"], P["minimum_plane_points"])


def _run_batch(devs, kind):
    s = mc.the_scan(kind)
    return capi.icp_align_batch([d.m for d in devs], [d.scan(s[:n]) for d, n in zip(devs, mc.BATCH_SIZES)], mc.BATCH_GUESSES,
                                mc.align_params(capi, kind), priors=[mc.prior(n) for n in mc.BATCH_SIZES])


def _watched(row, kind, call):
    """the call's result, after asserting from the library's counters that the intended kernel ran"""
    l0, f0 = capi.loop_stats(), capi.flat_stats()
    r = call()
    (s1, a1), f1 = capi.loop_stats(), capi.flat_stats()
    started, flat = s1 - l0[0], tuple(x - y for x, y in zip(f1, f0))
    what = "%s: loops started %d, abandoned %d, flat launches %s" % (row["name"], started, a1 - l0[1], flat)
    assert a1 == l0[1], what                      # no loop gave up
    env = row.get("env", {})
    if row["family"] == "align":
        want = loop_expected(row["n"], env)
        if want is not None:
            assert started == (1 if want else 0), what
        if env.get("MH_MATCH") == "f":            # the plan / scan matcher, in the instantiation the switches name
            wide = 1 if env.get("MH_NO_OFF32") else 0
            assert flat[wide] > 0 and flat[1 - wide] == 0 and flat[2:] == (0, 0), what
        else:
            assert flat == (0, 0, 0, 0), what
    if row["family"] == "batch" and not env and not mc.is_ndt(kind):
        assert started == len(mc.BATCH_SIZES), what   # k_icpw_b: every job's loop
    return r


# ----------------------------------------------------------------------------------------------------------------- comparisons
def _hold(got, want, row, kind, what):
    """the device's result against the oracle's"""
    fam, name = row["family"], row["name"]
    if fam == "align":
        assert want["n_final_pairs"] > 0, what
        _assert_single_is_the_oracles(got, want, what)
        assert got["n_final_pairs_pt2pl"] == want["n_final_pairs_pt2pl"], what
        if mc.is_ndt(kind):
            assert want["n_final_pairs_pt2pl"] > 0, what
    elif fam == "layers":
        assert want["n_final_pairs"] > 0, what
        _check(got, mc.layer_cases(kind)[name], want, what)
    elif fam == "batch":
        for j, (g, o) in enumerate(zip(got, want)):
            assert (g["n_iterations"], g["termination_reason"], g["n_final_pairs"], g["n_final_pairs_pt2pl"]) == \
                (o["n_iterations"], o["termination_reason"], o["n_final_pairs"], o["n_final_pairs_pt2pl"]), (what, j)
            np.testing.assert_allclose(g["T"], o["T"], rtol=0, atol=1e-9, err_msg="%s job %d" % (what, j))
    elif name == "dense":
        found = got["global_idx"] != capi.NO_MATCH
        np.testing.assert_array_equal(np.nonzero(found)[0], want["local_idx"], err_msg=what)
        for k in ("global_idx", "d2", "global_xyz"):
            np.testing.assert_array_equal(got[k][found], want[k], err_msg="%s: %s" % (what, k))
    elif name in ("nn", "nn_k3"):
        assert len(want["local_idx"]) > 500, what
        for k in ("local_idx", "global_idx", "d2", "global_xyz"):
            np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (what, k))
        assert got["potential_pairings"] == want["potential_pairings"], what
    elif name in ("radius", "radius_sorted"):
        assert len(want.global_idx) > 100 and rr.same(got, want) is None, (what, rr.same(got, want))
    elif name == "score16":
        assert want["n_paired"].max() > 100 and sr.same(got, want) is None, (what, sr.same(got, want))
    elif name == "pt2pl":
        np.testing.assert_array_equal(got["local_idx"], want["local_idx"], err_msg=what)
        np.testing.assert_array_equal(got["centroid"], want["centroid"], err_msg=what)
        np.testing.assert_allclose(got["normal"], want["normal"], rtol=0, atol=1e-6, err_msg=what)
    else:
        assert name == "pt2pl_knn", name
        np.testing.assert_array_equal(got["local_idx"], want["local_idx"], err_msg=what)
        for k in ("centroid", "normal"):
            np.testing.assert_allclose(got[k], want[k], rtol=0, atol=1e-6, err_msg="%s: %s" % (what, k))


def _bits(x):
    """a result as something that compares equal exactly when every bit of it does (timings and launch counts left out)"""
    if isinstance(x, dict):
        return {k: _bits(v) for k, v in x.items() if k not in TIMING}
    if isinstance(x, (list, tuple)):
        return [_bits(v) for v in x]
    if isinstance(x, np.ndarray):
        return (x.dtype.str, x.shape, x.tobytes())
    if isinstance(x, float):
        return np.float64(x).tobytes()
    return x


def _same_bits(a, b, what):
    a, b = _bits(a), _bits(b)
    if a != b and isinstance(a, dict):
        assert not [k for k in a if a[k] != b.get(k)], what
    assert a == b, what


def _same_download(got, want, what):
    for k in ("xyz", "src_idx", "vox_keys", "vox_first", "vox_count"):
        assert got[k].shape == want[k].shape and got[k].tobytes() == np.ascontiguousarray(want[k], got[k].dtype).tobytes(), (what, k)


# ------------------------------------------------------------------------------------------------------------------- the test
def _second_context_row(kind, name):
    name = {"q": "ndt_q", "f": "ndt_f"}.get(name, name) if mc.is_ndt(kind) else name
    return next(r for r in mc.routes(kind) if r["name"] == name)


@pytest.mark.parametrize("mutation,kind", mc.CASES)
def test_every_route_on_a_warm_map_after(contexts, mutation, kind, monkeypatch):
    mu = mc.MUTATIONS[mutation]
    before, (after, _) = mc.before(kind), mc.after(mutation, kind)
    ctx = contexts[0]
    devs = []

    def new_dev(c=ctx, with_map=True):
        devs.append(Dev(kind, c, monkeypatch, with_map))
        return devs[-1]

    try:
        # ---- a twin handle first: the update leaves the reference's map, bit for bit, in a table of the size the rule gives
        twin = new_dev()
        _same_download(twin.m.download(), before.dump(), "before")
        assert twin.m.info().table_size == before.table
        mu.device(kind, twin)
        _same_download(twin.m.download(), after.dump(), "after")
        assert twin.m.info().table_size == after.table
        if mc.is_ndt(kind):
            g, o = twin.m.download_ndt(), after.om.dump_ndt()
            for k in ("centroid", "normal", "is_plane"):
                assert g[k].tobytes() == o[k].tobytes(), k
        twin.close()

        # ---- every route of the table but the batches: warm twice, update, search once, search without the graph
        dev, ran, own = new_dev(), [], {}
        for row in mc.routes(kind):
            if row["family"] == "batch":
                continue
            what = "%s %s %s" % (mutation, kind, row["name"])
            with _env(monkeypatch, row.get("env", {})):
                if ran:
                    dev.reset()
                for warm in (1, 2):
                    _hold(_watched(row, kind, lambda: _run(dev, row)), mc.reference(before, row), row, kind, "%s, warm run %d" % (what, warm))
                mu.device(kind, dev)
                got = _watched(row, kind, lambda: _run(dev, row))
                _hold(got, mc.reference(after, row), row, kind, what + ", after the update")
                if row["family"] != "query" and "MH_NO_GRAPH" not in row.get("env", {}):
                    with _env(monkeypatch, {"MH_NO_GRAPH": "1"}):
                        _same_bits(_run(dev, row), got, what + ", without the graph")
            own[row["name"]] = got
            ran.append(row["name"])

        # ---- the lock-step batches: three jobs on three contexts, each map updated on its own context, led by job 0
        three = [new_dev(c) for c in contexts[2:5]]
        for row in (r for r in mc.routes(kind) if r["family"] == "batch"):
            what = "%s %s %s" % (mutation, kind, row["name"])
            with _env(monkeypatch, row["env"]):
                if ran[-1] in ("icpw_b", "chain_b"):
                    for d in three:
                        d.reset()
                for warm in (1, 2):
                    _hold(_watched(row, kind, lambda: _run_batch(three, kind)), mc.reference(before, row), row, kind,
                          "%s, warm run %d" % (what, warm))
                for d in three:
                    mu.device(kind, d)
                got = _watched(row, kind, lambda: _run_batch(three, kind))
                _hold(got, mc.reference(after, row), row, kind, what + ", after the update")
                with _env(monkeypatch, {"MH_NO_GRAPH": "1"}):
                    _same_bits(_run_batch(three, kind), got, what + ", without the graph")
            ran.append(row["name"])

        # ---- a queued update, and the search of a scan of ANOTHER context directly behind it
        if mutation in mc.QUEUED:
            other = new_dev(contexts[1], with_map=False)
            for name in mc.SECOND_CONTEXT_ROUTES:
                row = _second_context_row(kind, name)
                what = "%s %s %s from a second context" % (mutation, kind, row["name"])
                d = new_dev()
                with _env(monkeypatch, row.get("env", {})):
                    for warm in (1, 2):
                        _hold(_watched(row, kind, lambda: _run(d, row, other)), mc.reference(before, row), row, kind,
                              "%s, warm run %d" % (what, warm))
                    mu.device(kind, d)
                    got = _watched(row, kind, lambda: _run(d, row, other))
                _hold(got, mc.reference(after, row), row, kind, what)
                _same_bits(got, own[row["name"]], what)
                d.close()

        # every row of the table has run for this (update, kind): none skipped or set apart
        assert [(mutation, kind, n) for n in ran] == [x for x in mc.GPU_LIST if x[:2] == (mutation, kind)]
    finally:
        for d in devs:
            d.close()
