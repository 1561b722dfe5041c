"""The route inventory of the alignment tests: which switches and layer sizes reach which kernel.  One definition, imported by
tests/test_gpu_dense_cells.py, tests/test_gpu_solver_params.py, tests/test_gpu_far_origin.py and (MUTATION_ROUTES, through
tests/mutation_cases.py) tests/test_gpu_map_mutations.py; no GPU, no inputs.

Which kernel a row runs follows from plan_alignment (csrc/mh_icp.hip) and is confirmed by the one-line mutants of DESIGN.md
section 5.  MH_MATCH=t|w|o named the tile / wave / sorted-scan matchers, which were removed: the library refuses the letters
(test_gpu_parity.py::test_retired_matcher_letters_are_refused) and no table lists them."""

# ------------------------------------------------------------------------------------------------ single pair, dense-cell maps
# test_gpu_parity.py::test_every_kernel_variant_matches_the_oracle's list, plus the
# default route's launch chain (the one-launch loops have cases of their own).  No loop starts under these switches, except under
# MH_MATCH=s alone: the row search's loop k_icp16, 2.6 ms for 2000 points and 16 iterations (profiles/dense_cells.md).
FAMILIES = [{"MH_NO_LOOP16": "1"}, {"MH_MATCH": "s"}, {"MH_MATCH": "s", "MH_NO_STEP_CHAIN": "1"},
            {"MH_MATCH": "s", "MH_NO_STEP_CHAIN": "1", "MH_NO_FUSE16": "1"}, {"MH_MATCH": "q"}, {"MH_MATCH": "p"}, {"MH_MATCH": "x"},
            {"MH_MATCH": "q", "MH_NO_GRAPH": "1"}, {"MH_MATCH": "f"}, {"MH_MATCH": "f", "MH_NO_GRAPH": "1"}]
SEARCH = [{}, {"MH_NO_PREV_BOUND": "1"}, {"MH_NO_QIDX": "1"}]

# (points, iterations) of the cases that let a loop run, sized from the loop times measured on the dense map
# (profiles/dense_cells.md) so that they stay below half the 20 ms limit: k_icp16 takes 2.6 ms for 2000 points and 16 iterations;
# k_icpw takes 1.1 ms per iteration at any of these sizes (the tower's voxel decides), 6.5 ms for six -- twelve iterations took
# 13 ms, sixteen 18 ms, so the larger budgets run on the chain alone.
LOOP16_CASES = [(129, 6), (2000, 16)]
LOOPW_CASES = [(129, 6), (2000, 6), (2561, 6)]

MULTI = ["two_pairs", "beside_capped", "k2", "k8", "k2_mixed", "k2_n1", "k2_n63", "k2_n64", "k2_n65", "k2_n129", "unique", "gated",
         "rgbd", "knn16"]


def env_id(env):
    return "-".join("%s=%s" % (k[3:], v) for k, v in env.items()) or "plain"


# ------------------------------------------------------------------------------------------------ every kernel by size
# NDT map: (points, switches, inner iterations, matched_points = skip) -> the kernel that runs the plane matcher
PLANE_MATCHER_KERNELS = [
    (1500, {}, 2, False),                              # k_icp16<true> (loop_stats: ran, not abandoned)
    (1500, {}, 1, False),
    (1500, {"MH_NO_LOOP16": "1"}, 2, False),           # k_step16<true>, streaming control
    (5000, {"MH_NO_LOOP16": "1"}, 2, False),
    (5000, {}, 2, False),                              # k_step16<true> (layers of 2561-8192 points take it by size)
    (5000, {}, 1, False),
    (5000, {"MH_NO_STEP_CHAIN": "1"}, 2, False),       # k_match16<true, false> | k_accum_both | k_solve
    (5000, {"MH_NO_FUSE16": "1"}, 2, False),           # (no effect on an NDT layer: the row kernel never fuses its first step there)
    (5000, {"MH_NO_STEP_CHAIN": "1", "MH_NO_FUSE16": "1"}, 1, False),
    (10000, {}, 2, False),                             # above the step chain by size: k_match16<true, false> | k_accum_both
    (5000, {"MH_MATCH": "p"}, 2, False),               # k_match_pl<FUSED> (its own first step) + one lane per point; k_accum_both inside
    (5000, {"MH_MATCH": "p"}, 1, False),
    (40000, {}, 2, False),                             # k_match_pl<FUSED> + plan / scan matcher, by size
    (40000, {"MH_MATCH": "p"}, 1, False),
    (5000, {"MH_MATCH": "q"}, 2, False),               # k_match_pl<FUSED> + quad matcher
    (5000, {"MH_MATCH": "f"}, 2, False),
    (5000, {}, 2, True),                               # matched_points = skip: both verdicts in the row kernel
]

# plain map: (points, switches) -> the family of the point matcher
POINT_MATCHER_KERNELS = [
    (1500, {}),                                                              # k_icp16<false>
    (1500, {"MH_NO_LOOP16": "1"}),                                           # k_step16<false>
    (3000, {"MH_LOOPW": "all"}),                                             # k_icpw
    (5000, {}),                                                              # k_step16 under streaming control
    (5000, {"MH_MATCH": "s", "MH_NO_STEP_CHAIN": "1"}),                      # k_match16<false, FUSED> | k_solve | k_accum
    (5000, {"MH_MATCH": "s", "MH_NO_STEP_CHAIN": "1", "MH_NO_FUSE16": "1"}),  # k_match16<false, false> | k_accum
    (10000, {}),                                                             # fused row kernel by size
    (20000, {}),                                                             # row kernel + k_accum by size
    (5000, {"MH_MATCH": "f"}),                                               # k_match_flat | k_accum | k_solve
    (40000, {}),                                                             # ... by size
    (5000, {"MH_MATCH": "q"}),
    (5000, {"MH_MATCH": "p"}),
    (5000, {"MH_MATCH": "x"}),
]


# ------------------------------------------------------------------------------------------------ warm maps after a map update
# tests/test_gpu_map_mutations.py runs every row on a handle that has been searched before and was then updated
# (tests/mutation_cases.py).  The sizes are the small ones at which each kernel still takes its own path (dense_cases.SIZES,
# LOOP16_CASES, LOOPW_CASES), every loop runs MUTATION_IT iterations, so the loop times of profiles/dense_cells.md still hold.
# maps: "point" (plain point maps, an occupancy map's search map among them), "ndt", "any".
MUTATION_IT = 6


def _row(family, name, maps="any", **spec):
    return dict(family=family, name=name, maps=maps, **spec)


MUTATION_ROUTES = [
    # ---- single alignments on point maps
    _row("align", "icp16_n129", "point", n=129, env={}),                                                     # k_icp16
    _row("align", "icp16_n2000", "point", n=2000, env={}),
    _row("align", "icpw_n2561", "point", n=2561, env={"MH_LOOPW": "all"}),                                   # k_icpw
    _row("align", "step16", "point", n=2000, env={"MH_NO_LOOP16": "1"}),                                     # k_step16
    _row("align", "rows_fused", "point", n=2000, env={"MH_MATCH": "s", "MH_NO_STEP_CHAIN": "1"}),            # k_match16<false, FUSED>
    _row("align", "rows", "point", n=2000, env={"MH_MATCH": "s", "MH_NO_STEP_CHAIN": "1", "MH_NO_FUSE16": "1"}),
    _row("align", "q", "point", n=2000, env={"MH_MATCH": "q"}),                                              # k_match4
    _row("align", "p", "point", n=2000, env={"MH_MATCH": "p"}),
    _row("align", "x", "point", n=2000, env={"MH_MATCH": "x"}),
    _row("align", "f", "point", n=2000, env={"MH_MATCH": "f"}),                                              # k_match_flat<true>
    _row("align", "f_off64", "point", n=2000, env={"MH_MATCH": "f", "MH_NO_OFF32": "1"}),                    # k_match_flat<false>
    _row("align", "q_nograph", "point", n=2000, env={"MH_MATCH": "q", "MH_NO_GRAPH": "1"}),
    _row("align", "f_nograph", "point", n=2000, env={"MH_MATCH": "f", "MH_NO_GRAPH": "1"}),
    # ---- the NDT kind: the rows of PLANE_MATCHER_KERNELS at 2000 points; where size alone chose the kernel there, MH_MATCH does
    _row("align", "ndt_icp16", "ndt", n=2000, env={}, inner=2),                                              # k_icp16<true>
    _row("align", "ndt_icp16_inner1", "ndt", n=2000, env={}, inner=1),
    _row("align", "ndt_step16", "ndt", n=2000, env={"MH_NO_LOOP16": "1"}, inner=2),                          # k_step16<true>
    _row("align", "ndt_step16_inner1", "ndt", n=2000, env={"MH_NO_LOOP16": "1"}, inner=1),
    _row("align", "ndt_rows", "ndt", n=2000, env={"MH_MATCH": "s", "MH_NO_STEP_CHAIN": "1"}, inner=2),       # k_match16<true, false>
    _row("align", "ndt_rows_nofuse", "ndt", n=2000, env={"MH_MATCH": "s", "MH_NO_STEP_CHAIN": "1", "MH_NO_FUSE16": "1"}, inner=1),
    _row("align", "ndt_p", "ndt", n=2000, env={"MH_MATCH": "p"}, inner=2),                                   # k_match_pl<FUSED> + a lane per point
    _row("align", "ndt_p_inner1", "ndt", n=2000, env={"MH_MATCH": "p"}, inner=1),
    _row("align", "ndt_q", "ndt", n=2000, env={"MH_MATCH": "q"}, inner=2),                                   # ... + quad matcher
    _row("align", "ndt_f", "ndt", n=2000, env={"MH_MATCH": "f"}, inner=2),                                   # ... + plan / scan matcher
    _row("align", "ndt_skip", "ndt", n=2000, env={"MH_NO_LOOP16": "1"}, inner=2, skip=True),                 # matched_points = skip
    # ---- the granular queries
    _row("query", "dense"), _row("query", "nn"), _row("query", "nn_k3"), _row("query", "radius"), _row("query", "radius_sorted"),
    _row("query", "score16"), _row("query", "pt2pl", "ndt"), _row("query", "pt2pl_knn"),
    # ---- multi-layer: two pairs that share the updated map; k-best; a plane pair; unique-global
    _row("layers", "two_pairs"), _row("layers", "k2"), _row("layers", "plane_pair"), _row("layers", "unique"),
    # ---- one lock-step batch: three jobs on three contexts, each map updated on its own context, led by job 0
    _row("batch", "icpw_b", env={}), _row("batch", "chain_b", env={"MH_LOOPW": "none"}),
]


def mutation_routes(ndt):
    """the rows that apply to a map kind"""
    return [r for r in MUTATION_ROUTES if r["maps"] in ("any", "ndt" if ndt else "point")]


def loop_expected(n, env):
    """True when a single alignment of n points under `env` runs as a one-launch loop (k_icp16 / k_icpw), False when no loop
    starts, None when the tests leave it open."""
    if (n <= 2560 and not env) or env.get("MH_LOOPW") == "all":
        return True
    if env.get("MH_NO_LOOP16") or n > 2560:
        return False
    return None
