"""The jobs of tests/test_gpu_icp_layers_batch_planes.py (mh_icp_align_layers_batch_planes), host arrays only: cases of
tests/planes_ref.py under their own names, and cases in that form built from planes_ref._pair for what they do not cover -- plane
pairs of 257 points (a plane accumulation workgroup is 256), an empty plane pair in front, a second job with a plane pair and a
pair of k = 2, jobs without any plane pair, and four plane jobs that end at four different iterations.  Everything here runs on
the CPU: tests/test_icp_layers_batch_planes_abi.py checks the spread of iteration counts on the reference alone."""
import numpy as np

import kbest_ref
import planes_ref as pr

REF_CASES = ["ref_n1", "ref_n63", "ref_n64", "ref_n65", "ref_n700", "ref_n2000", "rgbd", "gated", "dup"]  # cases of planes_ref

# the batch of test 1, in two orders: three kinds of group (plane jobs without k > 1, plane jobs with k > 1, jobs without a plane
# pair) and a job alone in its group (k > 1, no plane pair).  ORDER_A: a job of plane pairs only leads the plane group, the groups
# one after the other.  ORDER_B: the groups interleaved, the job with the empty plane pair first, a plane-less job last but one.
ORDER_A = ["ref_n2000", "ref_n1", "ref_n63", "ref_n64", "ref_n65", "n257", "ref_n700", "empty_first", "gated", "dup",
           "rgbd", "plane_k2", "plain_halves", "plain_split", "kbest_alone"]
ORDER_B = ["empty_first", "plain_split", "rgbd", "ref_n65", "kbest_alone", "dup", "ref_n1", "plane_k2", "gated", "n257", "ref_n64",
           "ref_n700", "ref_n63", "plain_halves", "ref_n2000"]
SPREAD = ["drop_at_3", "nobody_at_0", "to_the_end", "stalls"]
PLANE_LESS = ["plain_halves", "plain_split", "kbest_alone"]


def case_defs(inp):
    """name -> case (planes_ref.cases' form)."""
    s = inp.scan
    ref = pr.cases(inp)
    thr, kp, pthr = kbest_ref.schedule(40), np.full(40, 0.5), np.full(40, 0.4)
    out = {n: ref[n] for n in REF_CASES}
    out["n257"] = dict(pairs=[pr._pair("whole", s[:257], pthr, pr.RGBD), pr._pair("whole", s[1000:], thr)])
    out["empty_first"] = dict(pairs=[pr._pair("whole", np.zeros((0, 3), np.float32), pthr, pr.RGBD), pr._pair("whole", s[:700], pthr, pr.RGBD),
                                     pr._pair("whole", s[1000:], thr)])
    out["plane_k2"] = dict(pairs=[pr._pair("whole", s[:700], pthr, pr.RGBD, weight=0.5), pr._pair("whole", s[700:], thr, k=2)])
    out["plain_halves"] = dict(pairs=[pr._pair("whole", s[0::2], thr), pr._pair("whole", s[1::2], thr, weight=0.5)])
    out["plain_split"] = dict(pairs=[pr._pair("whole", s[:700], thr), pr._pair("whole", s[700:], thr)])
    out["kbest_alone"] = dict(pairs=[pr._pair("whole", s[0::2], thr, k=2), pr._pair("whole", s[1::2], thr)])
    # (test 3) four plane jobs that end at four different iterations
    drop = pthr.copy()
    drop[3:] = 1e-6
    pdrop = thr.copy()
    pdrop[3:] = 1e-6
    out["drop_at_3"] = dict(pairs=[pr._pair("whole", s[:700], drop, pr.RGBD), pr._pair("whole", s[1000:], pdrop)])
    out["nobody_at_0"] = dict(pairs=[pr._pair("whole", s[:700], pthr, pr.RGBD, gate=(2, 0)), pr._pair("whole", s[1000:], thr, gate=(1, 0))])
    out["to_the_end"] = ref["off_pose"]
    out["stalls"] = dict(pairs=[pr._pair("whole", s[1::2], pthr, pr.RGBD), pr._pair("whole", s[0::2], thr)])
    for c in out.values():
        c.setdefault("max_it", 40)
        c.setdefault("kp", kp)
        c.setdefault("inner", 2)
        c.setdefault("T0", inp.T0)
        c.setdefault("prior", None)
        c.setdefault("pkw", {})
    return out


def has_plane(c):
    return any(e["plane"] for e in c["pairs"])


def has_kbest(c):
    return any(e["k"] > 1 for e in c["pairs"])
