"""See-through voting on the device (include/molahip_clean.h) against tests/clean_ref.py, the numpy restatement of the header's
text: every word of every view, every packed vote.  Then the refusals, and the scenario of tests/clean_cases.py through
mola_hip::clean_keyframes: a street with one moving car per sweep; the cleaned set is the restatement's, the session map built
from it is one insertion of the cleaned frames and has lost the mover's trail, and the loop-closure scenario still closes.

The saturation case repeats one view 70 000 times in the neighbour list of a three-point frame: about a millisecond of device
time, so it runs at full size on the device; the restatement counts the repeated entry by its weight.

Measured on an MI355X: the street loses 9 763 of its 9 790 mover points and 361 of its 356 452 others; the cleaned session map keeps
28 of 1 234 points inside the swept volume; the 66-frame loop scenario loses 27 439 of 1 202 481 points and still accepts its four
pairs; views 1.0 ms, votes 0.4 ms, removal 0.25 ms on the street (profiles/map_cleaning.md)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import clean_cases as cc
import clean_ref as cr
import loop_cases as lc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPE = os.path.join(ROOT, "pipelines", "lidar3d-default-hip.yaml")
CLI = os.path.join(ROOT, "mola_lidar_odometry_amd", "molahip-lo-cli")
SIZES = [255, 0, 1, 256, 257, 5000, 0]   # an empty frame between two others, one at the end
SHAPES = [(1, 8), (32, 128), (5, 24), (16, 256)]
I12 = np.eye(4)[:3].reshape(12)


@pytest.fixture(scope="module")
def capi():
    from mola_lidar_odometry_amd import capi as c
    return c


@pytest.fixture(scope="module")
def cl():
    from mola_lidar_odometry_amd import capi_clean
    return capi_clean


@pytest.fixture(scope="module")
def ctx(capi):
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


def _params(A, S, **kw):
    p = dict(cr.DEFAULT, n_rings=A, n_sectors=S)
    if A == 5:  # one shape with the sensor off the vehicle's origin and a window that straddles no zero edge
        p.update(origin=(0.25, -0.5, 1.0), el_min=float(np.radians(-30.0)), el_max=float(np.radians(-1.0)))
    if A == 1:
        p.update(el_min=float(np.radians(-10.0)), el_max=float(np.radians(10.0)))
    p.update(kw)
    return p


def _frames(p, seed=0):
    return [cr.edge_cloud(n, seed + 17 * k, **p) for k, n in enumerate(SIZES)]


def _pose(rng, spread):
    yaw = rng.uniform(-np.pi, np.pi)
    c, s = np.cos(yaw), np.sin(yaw)
    t = rng.uniform(-spread, spread, 3) * [1, 1, 0.05]
    return np.array([c, -s, 0, t[0], s, c, 0, t[1], 0, 0, 1, t[2]])


# ------------------------------------------------------------------ views
@pytest.mark.parametrize("A,S", SHAPES)
def test_views_are_the_restatement_s_word_for_word(cl, ctx, A, S):
    p = _params(A, S)
    frames = _frames(p)
    ref = np.array([cr.view(f, **p) for f in frames])
    v = cl.Views(ctx, cl.clean_params(**p)).add_frames(frames)
    got = v.download()
    assert len(v) == len(frames) and got.shape == ref.shape
    assert got.tobytes() == ref.tobytes(), np.argwhere(got != ref)[:5]
    assert (got[1] == cr.EMPTY).all() and (got[6] == cr.EMPTY).all()
    if A > 1:
        assert (got[5] != cr.EMPTY).sum() > A * S // 4   # (the comparison is of filled images)
    # a shuffled copy of the same points; passes of 300 points; both appended behind what is stored
    rng = np.random.default_rng(5)
    v.add_frames([frames[5][rng.permutation(5000)]])
    v.add_frames(frames, max_points_per_pass=300)
    again = v.download()
    assert len(v) == 2 * len(frames) + 1 and again[:7].tobytes() == ref.tobytes()
    assert again[7].tobytes() == ref[5].tobytes() and again[8:].tobytes() == ref.tobytes()
    assert v.download(3, 2).tobytes() == ref[3:5].tobytes()
    v.close()


def test_a_quarter_turn_shifts_the_view_by_a_quarter_of_its_columns(cl, ctx):
    p = _params(32, 128)
    c = cr.edge_cloud(5000, 3, **p)
    got = cl.Views(ctx, cl.clean_params(**p)).add_frames([c, cr.quarter_turn(c)]).download()
    assert (np.roll(got[0], 32, axis=1) == got[1]).all()


# ------------------------------------------------------------------ votes
def _shell(p, n, r0, r1, seed):
    """a dense shell around the sensor: every bin of the elevation window holds points"""
    rng = np.random.default_rng(seed)
    e0, e1 = float(np.float32(p["el_min"])), float(np.float32(p["el_max"]))
    az, el, r = rng.uniform(-np.pi, np.pi, n), rng.uniform(e0, e1, n), rng.uniform(r0, r1, n)
    xyz = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1)
    return np.ascontiguousarray((xyz + np.asarray(p["origin"])).astype(np.float32))


def _vote_case(p, seed, n_nbr=(0, 1, 24, 3, 24, 24, 2), spread=6.0):
    """frames of SIZES points with neighbour lists of n_nbr[f] entries under random poses; the store holds the views of the same
    frames and of two dense shells (a near and a far one), so that windows without an empty bin occur"""
    rng = np.random.default_rng(seed)
    frames = _frames(p, seed)
    stored = frames + [_shell(p, 30000, 8.0, 12.0, seed + 1), _shell(p, 30000, 30.0, 40.0, seed + 2)]
    nbr_view = [rng.integers(0, len(stored), k) for k in n_nbr]
    nbr_T = [np.array([_pose(rng, spread) for _ in range(k)]).reshape(k, 12) for k in n_nbr]
    return frames, stored, nbr_view, nbr_T


def _ref_votes(p, frames, views, nbr_view, nbr_T):
    return [cr.vote(f, views, nv, nt, **p) for f, nv, nt in zip(frames, nbr_view, nbr_T)]


@pytest.mark.parametrize("A,S,wr,ws", [(32, 128, 1, 1), (32, 128, 0, 0), (32, 128, 2, 2), (32, 128, 0, 2), (1, 8, 1, 1), (5, 24, 1, 2), (16, 256, 2, 1)])
def test_votes_are_the_restatement_s_word_for_word(cl, ctx, A, S, wr, ws):
    p = _params(A, S, win_rings=wr, win_sectors=ws)
    frames, stored, nbr_view, nbr_T = _vote_case(p, 100 + A + wr)
    views = [cr.view(f, **p) for f in stored]
    ref = _ref_votes(p, frames, views, nbr_view, nbr_T)
    v = cl.Views(ctx, cl.clean_params(**p)).add_frames(stored)
    got = v.vote_frames(frames, nbr_view, nbr_T)
    for f, (g, r) in enumerate(zip(got, ref)):
        assert g.tobytes() == r.tobytes(), (f, np.argwhere(g != r)[:5], g[g != r][:5], r[g != r][:5])
    assert not got[0].any() and len(got[1]) == 0    # no neighbours: zeros
    allv = np.concatenate(ref)
    if A > 1:
        assert (allv & 0xFFFF).any() and (allv >> 16).any()   # (both kinds of evidence occur)
    # passes of 300 points: the same words
    again = v.vote_frames(frames, nbr_view, nbr_T, max_points_per_pass=300)
    assert np.concatenate(again).tobytes() == allv.tobytes()
    v.close()


def test_device_arrays_give_the_same_words(cl, ctx):
    """points and votes in device memory (read and written in place), in one pass and in passes of 300 points"""
    import torch
    p = _params(32, 128)
    frames, stored, nbr_view, nbr_T = _vote_case(p, 77)
    ref_views = np.array([cr.view(f, **p) for f in stored])
    ref = np.concatenate(_ref_votes(p, frames, list(ref_views), nbr_view, nbr_T))
    keep = [[torch.from_numpy(np.ascontiguousarray(f[:, a])).cuda() for a in range(3)] for f in stored]
    ptrs = [(x.data_ptr() if len(x) else None, y.data_ptr() if len(y) else None, z.data_ptr() if len(z) else None, len(x)) for x, y, z in keep]
    for budget in (0, 300):
        v = cl.Views(ctx, cl.clean_params(**p)).add_frames_device(ptrs, budget)
        assert v.download().tobytes() == ref_views.tobytes()
        out = torch.full((len(ref),), 0x5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()   # (the fill runs on torch's stream, the votes on the context's)
        v.vote_frames_device(ptrs[:len(frames)], nbr_view, nbr_T, out.data_ptr(), budget)
        assert out.cpu().numpy().astype(np.uint32).tobytes() == ref.tobytes()
        v.close()


def test_votes_at_the_image_s_edges_and_outside_every_range(cl, ctx):
    """points laid across sector 0 / S-1 (the window wraps), in ring 0 and ring A-1 (the window is cut), and a pose that puts
    every point outside every range"""
    p = _params(32, 128, win_rings=2, win_sectors=2)
    t = cr.tables(**p)
    rng = np.random.default_rng(9)
    n = 6000
    az = np.concatenate([rng.uniform(-0.12, 0.12, n // 2), rng.uniform(-np.pi, np.pi, n - n // 2)])      # around sector 0 / S-1
    e0, e1 = float(np.float32(p["el_min"])), float(np.float32(p["el_max"]))
    el = np.concatenate([rng.uniform(e0, e0 + 0.07, n // 3), rng.uniform(e1 - 0.07, e1, n // 3), rng.uniform(e0, e1, n - 2 * (n // 3))])
    el = el[rng.permutation(n)]

    def cloud(r):
        return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1).astype(np.float32)
    near, far = cloud(rng.uniform(5, 8, n)), cloud(rng.uniform(20, 30, n))
    frames = [near, far]
    keep, ring, sector, _ = cr.bins(near, t)
    assert {0, 1, 126, 127} <= set(sector[keep]) and {0, 31} <= set(ring[keep])
    views = [cr.view(f, **p) for f in frames]
    away = I12.copy()
    away[3] = 1000.0
    nbr_view, nbr_T = [[1, 1, 0], [0]], [np.array([I12, away, I12]), np.array([I12])]
    ref = _ref_votes(p, frames, views, nbr_view, nbr_T)
    got = cl.Views(ctx, cl.clean_params(**p)).add_frames(frames).vote_frames(frames, nbr_view, nbr_T)
    assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes()
    th = got[0] & 0xFFFF
    assert th[keep & (sector == 0)].any() and th[keep & (sector == 127)].any() and th[keep & (ring == 0)].any() and th[keep & (ring == 31)].any()
    assert th.max() == 1                                  # (the pose 1000 m away gives no evidence; nor does the own view)
    assert not (got[1] & 0xFFFF).any()                    # the far shell sees the near one in front of it: occluded


def test_a_point_exactly_on_the_margin_agrees(cl, ctx):
    """rel_margin 0.5: far2 = 2.25 exactly.  The view holds r2 = 36; q at range 4 has r2_q * far2 == 36 == r2_img: not through
    (the comparison is strict) but agreeing (closed); one ulp nearer it is through, one ulp farther it agrees."""
    p = _params(32, 128, rel_margin=0.5, win_rings=0, win_sectors=0)
    F = np.float32
    q = np.array([[np.nextafter(F(4), F(0)), 0, 0], [4, 0, 0], [np.nextafter(F(4), F(9)), 0, 0]], F)
    img = np.array([[6, 0, 0]], F)
    ref = cr.vote(q, [cr.view(img, **p)], [0], [I12], **p)
    assert list(ref) == [1, 1 << 16, 1 << 16]
    got = cl.Views(ctx, cl.clean_params(**p)).add_frames([img]).vote_frames([q], [[0]], [np.array([I12])])
    assert list(got[0]) == list(ref)


def test_the_counters_saturate_at_65535(cl, ctx):
    p = _params(32, 128, win_rings=0, win_sectors=0)
    F = np.float32
    q = np.array([[4, 0, 0], [0, 10, 0], [0, -7, 0.1]], F)          # through; agreeing; nothing there in the view
    img = np.array([[9, 0, 0], [0, 10.2, 0]], F)
    reps = 70000
    ref = cr.vote(q, [cr.view(img, **p)], [0], [I12], weights=[reps], **p)
    assert list(ref) == [65535, 65535 << 16, 0]
    got = cl.Views(ctx, cl.clean_params(**p)).add_frames([img]).vote_frames([q], [np.zeros(reps, np.uint32)], [np.tile(I12, (reps, 1))])
    assert list(got[0]) == list(ref)


def test_a_frame_never_sees_through_its_own_view(cl, ctx):
    for A, S in SHAPES:
        p = _params(A, S, win_rings=2, win_sectors=2)
        frames = [f for f in _frames(p, 40) if len(f)]
        k = len(frames)
        got = cl.Views(ctx, cl.clean_params(**p)).add_frames(frames).vote_frames(frames, [[i] for i in range(k)], [I12[None]] * k)
        allv = np.concatenate(got)
        assert not (allv & 0xFFFF).any() and (allv >> 16).any()


# ------------------------------------------------------------------ refusals
def test_refusals_come_before_any_device_work_and_leave_the_store_alone(capi, cl, ctx):
    L = cl.lib()
    p = _params(32, 128)
    frames = [cr.edge_cloud(300, 1, **p), cr.edge_cloud(200, 2, **p)]
    v = cl.Views(ctx, cl.clean_params(**p)).add_frames(frames)
    before = v.download().tobytes()
    keep, arr = cl._frames(frames)
    h = C.c_void_p()
    bad_params = [dict(n_rings=0), dict(n_rings=65), dict(n_sectors=12), dict(n_sectors=0), dict(n_sectors=264), dict(n_rings=64, n_sectors=128),
                  dict(el_min=0.5, el_max=0.2), dict(el_min=-1.6), dict(el_max=1.6), dict(min_range=0.0), dict(min_range=70.0),
                  dict(max_range=float("inf")), dict(rel_margin=0.0), dict(rel_margin=float("nan")), dict(origin=(0.0, float("nan"), 0.0)),
                  dict(win_rings=3), dict(win_sectors=3)]
    for kw in bad_params:
        assert L.mh_views_create(ctx._h, C.byref(cl.clean_params(**dict(p, **kw))), C.byref(h)) == 1, kw
        assert not h.value
    good = cl.clean_params(**p)
    assert L.mh_views_create(None, C.byref(good), C.byref(h)) == 1 and L.mh_views_create(ctx._h, None, C.byref(h)) == 1
    assert L.mh_views_create(ctx._h, C.byref(good), None) == 1
    n = C.c_uint64(0)
    assert L.mh_views_size(None, C.byref(n)) == 1 and L.mh_views_size(v._h, None) == 1
    # add_frames
    assert L.mh_views_add_frames(None, arr, 2, capi.MEM_HOST, 0) == 1
    assert L.mh_views_add_frames(v._h, None, 2, capi.MEM_HOST, 0) == 1
    assert L.mh_views_add_frames(v._h, arr, 2, 7, 0) == 1
    broken = (capi.MapFrame * 2)()
    broken[0].x, broken[0].y, broken[0].z, broken[0].n = arr[0].x, arr[0].y, arr[0].z, arr[0].n
    broken[1].x, broken[1].y, broken[1].z, broken[1].n = arr[1].x, None, arr[1].z, arr[1].n
    assert L.mh_views_add_frames(v._h, broken, 2, capi.MEM_HOST, 0) == 1
    # download
    out = np.zeros(3 * 32 * 128, np.uint32)
    assert L.mh_views_download(v._h, 1, 2, capi._vp(out)) == 1 and L.mh_views_download(v._h, 3, 0, capi._vp(out)) == 1
    assert L.mh_views_download(v._h, 0, 1, None) == 1 and L.mh_views_download(None, 0, 1, capi._vp(out)) == 1
    # vote_frames
    start = np.array([0, 1, 2], np.uint32)
    view = np.array([1, 0], np.uint32)
    T = np.tile(I12, (2, 1))
    votes = np.zeros(500, np.uint32)

    def vote(views=v._h, frames_=arr, nf=2, start_=start, view_=view, T_=T, votes_=votes, mem=capi.MEM_HOST):
        vp = lambda a: None if a is None else capi._vp(a)  # noqa: E731
        return L.mh_views_vote_frames(views, frames_, nf, vp(start_), vp(view_), vp(T_), vp(votes_), mem, 0)
    assert vote() == 0
    T_nan = T.copy()
    T_nan[1, 7] = np.nan
    T_inf = T.copy()
    T_inf[0, 0] = np.inf
    for kw in (dict(views=None), dict(frames_=None), dict(frames_=broken), dict(start_=None), dict(view_=None), dict(T_=None), dict(votes_=None),
               dict(mem=3), dict(view_=np.array([1, 2], np.uint32)), dict(T_=T_nan), dict(T_=T_inf), dict(start_=np.array([0, 2, 1], np.uint32))):
        votes[:] = 0xABCD
        assert vote(**kw) == 1, list(kw)
        assert (votes == 0xABCD).all()
    assert "mh_views_vote_frames" in L.mh_last_error_string().decode()
    # the easy cases are not refusals
    assert L.mh_views_add_frames(v._h, None, 0, capi.MEM_HOST, 0) == 0 and vote(frames_=None, nf=0, start_=None, view_=None, T_=None, votes_=None) == 0
    assert vote(start_=np.zeros(3, np.uint32), view_=None, T_=None) == 0 and not votes.any()
    assert len(v) == 2 and v.download().tobytes() == before
    v.close()


# ------------------------------------------------------------------ the scenario
@pytest.fixture(scope="module")
def street(host):
    """the 20 key-frames with their mover, cleaned by the restatement and by the device"""
    sc = cc.scenario()
    masks, votes, nb = cr.clean(sc["sweeps"], sc["poses"])
    kf = cc.keyframe_set(sc["poses"], sc["sweeps"])
    cleaned, report = host.clean_keyframes(kf, None)
    return dict(sc=sc, masks=masks, nb=nb, kf=kf, cleaned=cleaned, report=report)


def test_the_device_cleans_the_street_as_the_restatement_does(street):
    sc, kf, cleaned, report = street["sc"], street["kf"], street["cleaned"], street["report"]
    assert cleaned["maps"] == kf["maps"] and len(cleaned["frames"]) == cc.N_FRAMES
    for k, (a, b) in enumerate(zip(cleaned["frames"], kf["frames"])):
        assert a["timestamp"] == b["timestamp"] and a["pose"] == b["pose"] and a["cov"] == b["cov"] and a["twist"] == b["twist"]
        assert len(a["layers"]) == 1 and a["layers"][0][0] == 0
        want = sc["sweeps"][k][~street["masks"][k]]
        assert np.asarray(a["layers"][0][1], np.float32).tobytes() == want.tobytes(), k
        assert tuple(report["frames"][k]) == (len(sc["sweeps"][k]), int(street["masks"][k].sum()), len(street["nb"][k]))
    mv, rm = np.concatenate(sc["mover"]), np.concatenate(street["masks"])
    print("mover points", int(mv.sum()), "removed", int((mv & rm).sum()), "| other points", int((~mv).sum()), "removed", int((~mv & rm).sum()))
    print("seconds", report["seconds"], "pairs", report["pairs"])
    assert (mv & rm).sum() >= 0.90 * mv.sum()
    assert (~mv & rm).sum() <= 0.01 * (~mv).sum()
    assert report["points_in"] == len(mv) and report["points_removed"] == int(rm.sum()) and report["pairs"] == sum(len(n) for n in street["nb"])
    assert json.loads(report["json"])["points_removed"] == report["points_removed"] and set(report["seconds"]) == {"views", "votes", "removal"}


def test_the_session_map_of_the_cleaned_set_has_lost_the_mover_s_trail(host, capi, street):
    sc = street["sc"]
    built, dirty = host.build_session_maps(street["cleaned"]), host.build_session_maps(street["kf"])
    m = capi.Map(capi.Context(0), **cc.MAP_PARAMS)
    m.insert_frames([(np.asarray(f["layers"][0][1], np.float32), f["pose"]) for f in street["cleaned"]["frames"]])
    d = m.download()
    m.close()
    assert len(built) == 1 and d["xyz"].tobytes() == built[0]["xyz"].tobytes() and d["src_idx"].tobytes() == built[0]["src_idx"].tobytes()
    n_clean = int(cc.in_swept_volume(np.asarray(built[0]["xyz"], np.float64).reshape(-1, 3), sc["boxes"]).sum())
    n_dirty = int(cc.in_swept_volume(np.asarray(dirty[0]["xyz"], np.float64).reshape(-1, 3), sc["boxes"]).sum())
    print("map points inside the swept volume: uncleaned", n_dirty, "cleaned", n_clean)
    assert n_dirty > 100 and 10 * n_clean <= n_dirty


def test_file_to_file_and_the_command_line(host, street, tmp_path):
    src, out, cli_out, pipe = (str(tmp_path / n) for n in ("in.mhkf", "out.mhkf", "cli.mhkf", "pipe.yaml"))
    host.write_keyframe_file(src, street["kf"])
    host.clean_keyframes(src, None, out)
    want = str(tmp_path / "want.mhkf")
    host.write_keyframe_file(want, street["cleaned"])
    assert open(out, "rb").read() == open(want, "rb").read()
    open(pipe, "w").write("map_cleaning:\n  min_through_votes: 2\n")
    r = subprocess.run([CLI, "--clean-keyframes", src, cli_out, "-c", pipe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(cli_out, "rb").read() == open(want, "rb").read()
    summary = json.loads(r.stdout.strip().split("\n")[-1])
    assert summary["cleaning"]["points_removed"] == street["report"]["points_removed"] and summary["cleaning"]["frames"] == cc.N_FRAMES


def test_a_set_without_points_comes_back_unchanged_and_several_entries_vote_together(host, street):
    kf = street["kf"]
    empty = dict(maps=kf["maps"], frames=[dict(f, layers=None) for f in kf["frames"][:3]])
    back, report = host.clean_keyframes(empty, None)
    assert report["points_in"] == 0 and report["pairs"] == 0 and [f["pose"] for f in back["frames"]] == [f["pose"] for f in empty["frames"]]
    # every frame's sweep split into two entries: the same points go, entry by entry
    two = dict(maps=kf["maps"], frames=[dict(f, layers=[(0, f["layers"][0][1][:7000]), (0, f["layers"][0][1][7000:])]) for f in kf["frames"]])
    cleaned, report = host.clean_keyframes(two, None)
    assert report["points_removed"] == street["report"]["points_removed"]
    for k, f in enumerate(cleaned["frames"]):
        keep = ~street["masks"][k]
        assert len(f["layers"]) == 2
        assert np.asarray(f["layers"][0][1], np.float32).tobytes() == street["sc"]["sweeps"][k][:7000][keep[:7000]].tobytes()
        assert np.asarray(f["layers"][1][1], np.float32).tobytes() == street["sc"]["sweeps"][k][7000:][keep[7000:]].tobytes()


def test_the_loop_scenario_still_closes_after_cleaning(host):
    """g6's 66 frames have no movers; what cleaning takes out of them must not cost a loop"""
    import test_gpu_loop as tg
    s = lc.scenario()
    kf = lc.keyframe_set(s["est"], s["sweeps"])
    cleaned, report = host.clean_keyframes(kf, None)
    print("66-frame loop scenario: points", report["points_in"], "removed", report["points_removed"], "seconds", report["seconds"])
    with pytest.MonkeyPatch.context() as mp:
        for v in tg.ENV:
            mp.delenv(v, raising=False)
        corrected, loops = host.close_loops(cleaned, host.Config.FromYamlText(open(PIPE).read() + lc.OPTIONS))
    accepted = [(p["i"], p["j"]) for p in loops["pairs"] if p["accepted"]]
    print("accepted", accepted)
    assert accepted == [(56, 1), (59, 2), (62, 5), (65, 8)]
