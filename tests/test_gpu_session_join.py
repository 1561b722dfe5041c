"""Two sessions joined on the device (mola_hip::join_sessions) against tests/join_ref.py, the restatement on the CPU oracle, on the
scenario of tests/join_cases.py: A is 46 key-frames around three sides of a block, B 26 key-frames of another vehicle that starts
near A's end, finishes the block and drives 49 m into A's first street, recorded in a frame of its own.  The tried pairs, their
phases, the candidate counts, the kept ranks, the decisions and the iteration counts are the restatement's; every Z is its Z within
1e-6 and B's joined poses within 1e-5 (the bounds tests/test_gpu_loop.py holds the same quantities to); A's frames come back byte
for byte.  What tests/test_session_join_cpu.py holds the restatement to on this scenario is asserted of the device's result, and
the device's error against the ground truth is at most the restatement's + 1e-4 m.  Then: B recorded in another frame, a min_links
nothing reaches, the session map of the joined set, the command line.

The figures measured on an MI355X are in profiles/session_join.md."""
import json
import os
import subprocess

import numpy as np
import pytest

import join_cases as jc
import join_ref as jr
import loop_cases as lc
import test_loop_cpu as tc
import test_odometry_localize as tl
import test_session_join_cpu as tj

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPE = os.path.join(ROOT, "pipelines", "lidar3d-default-hip.yaml")
CLI = os.path.join(ROOT, "mola_lidar_odometry_amd", "molahip-lo-cli")
ENV = tl.ENV + ("MOLA_LOAD_SM", "MOLA_GENERATE_SIMPLEMAP", "MOLA_SIMPLEMAP_OUTPUT", "MOLA_MINIMUM_ICP_QUALITY")
KA, KB = jc.N_A, len(jc.B_ARCS)


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


@pytest.fixture(scope="module")
def session(host, tmp_path_factory):
    """the two sessions as key-frame sets and files, and the pipeline text with the scenario's options"""
    d = tmp_path_factory.mktemp("join")
    a, b = jc.sessions()
    text = open(PIPE).read() + jc.OPTIONS
    fa, fb, text_file = str(d / "a.mhkf"), str(d / "b.mhkf"), str(d / "pipeline.yaml")
    host.write_keyframe_file(fa, a)
    host.write_keyframe_file(fb, b)
    open(text_file, "w").write(text)
    return dict(dir=d, a=a, b=b, fa=fa, fb=fb, text=text, text_file=text_file, **jc.scenario())


def _join(host, a, b, text, out=""):
    with pytest.MonkeyPatch.context() as mp:
        for v in ENV:
            mp.delenv(v, raising=False)
        return host.join_sessions(a, b, host.Config.FromYamlText(text), out)


@pytest.fixture(scope="module")
def joined(host, session):
    """ONE run on the device, shared by the tests: (joined set, is_joined, report) and the file the same call wrote"""
    out = str(session["dir"] / "joined.mhkf")
    return _join(host, session["a"], session["b"], session["text"], out) + (out,)


def _poses_b(joined_set):
    return np.array([f["pose"] for f in joined_set["frames"][KA:]])


def _pairs(report):
    return [(p["i"], p["j"], p["phase"], p["shift"], p["dist"]) for p in report["pairs"]]


def _same_decisions(report, ref):
    assert _pairs(report) == _pairs(ref)
    worst = 0.0
    for a, b in zip(report["pairs"], ref["pairs"]):
        assert a["candidates"] == b["candidates"] and list(a["ranks"]) == b["ranks"], (a["i"], a["j"], a["ranks"], b["ranks"])
        assert a["accepted"] == b["accepted"] and a["iterations"] == b["iterations"], (a["i"], a["j"], a["quality"], b["quality"], a["iterations"], b["iterations"])
        assert abs(a["quality"] - b["quality"]) <= 1e-9
        worst = max(worst, float(np.abs(np.array(a["Z"]) - b["Z"]).max()))
    return worst


def _a_s_frames_are_untouched(joined_set, a):
    assert joined_set["maps"] == a["maps"]
    for f, g in zip(joined_set["frames"][:KA], a["frames"]):
        assert f["timestamp"] == g["timestamp"] and f["pose"] == [float(v) for v in g["pose"]] and f["cov"] == g["cov"] and f["twist"] == g["twist"]
        for (ma, xa), (mb, xb) in zip(f["layers"], g["layers"]):
            assert ma == mb and xa.tobytes() == np.asarray(xb, np.float32).tobytes()


def test_the_sessions_are_joined_as_the_restatement_joins_them(host, session, joined, oracle):
    joined_set, is_joined, report, out = joined
    ref = tj.scenario_reference()
    worst_edge = _same_decisions(report, ref)
    print("pairs", [(p["i"], p["j"], p["phase"], round(p["quality"], 4), p["iterations"], p["accepted"]) for p in report["pairs"]])
    assert is_joined and report["joined"] and ref["is_joined"] and report["links_accepted"] == len(ref["links"])
    got = _poses_b(joined_set)
    dt, dr = tc._pose_distance(got, ref["poses_b"])
    print("|Z - restatement|", worst_edge, "joined poses against the restatement: |dt|", dt, "|dr|", dr, "cost", report["cost_before"], "->",
          report["cost_after"], "iterations", report["optimizer_iterations"])
    print("seconds", report["seconds"], "counts", report["counts"])
    assert worst_edge < 1e-6
    assert dt < 1e-5 and dr < 1e-5
    # what the scenario is there for, asserted of the device's run as the CPU suite asserts it of the restatement
    links = [(p["i"], p["j"]) for p in report["pairs"] if p["accepted"]]
    assert len(links) >= ref["options"]["min_links"] and any(j >= 40 for _, j in links) and any(j <= 6 for _, j in links)
    T_anchor = next(p for p in report["pairs"] if p["accepted"])
    placed = jr.placement(np.concatenate([session["a_est"], [f["pose"] for f in session["b"]["frames"]]], 0), KA,
                          (T_anchor["j"], KA + T_anchor["i"], T_anchor["Z"]))[KA:]
    e_placed, e_joined, e_ref = (lc.position_errors(p, session["b_gt"]) for p in (placed, got, ref["poses_b"]))
    print("B against the ground truth: first frame", e_joined[0], "last frame: anchor only", e_placed[-1], "joined", e_joined[-1], "restatement", e_ref[-1],
          "maximum over B: anchor only", e_placed.max(), "joined", e_joined.max(), "restatement", e_ref.max())
    assert e_joined[-1] < e_placed[-1]
    assert np.all(e_joined <= e_ref + 1e-4)
    # A is never moved, B keeps everything but its poses; every B frame was searched once, every pair scored once
    _a_s_frames_are_untouched(joined_set, session["a"])
    assert len(joined_set["frames"]) == KA + KB
    for f, g in zip(joined_set["frames"][KA:], session["b"]["frames"]):
        assert f["timestamp"] == g["timestamp"] and f["cov"] == g["cov"] and f["twist"] == g["twist"] and f["layers"][0][1].tobytes() == g["layers"][0][1].tobytes()
    n = len(report["pairs"])
    assert report["counts"]["index"] == 1 and report["counts"]["search"] == KB and report["counts"]["score"] == n and report["counts"]["submap"] == n
    assert report["counts"]["refine"] == 4 * n and report["counts"]["optimize"] == 1
    rep = json.loads(report["json"])
    assert rep["pairs"][0]["phase"] == "anchor" and rep["joined"] is True and rep["links_accepted"] == report["links_accepted"]


def test_the_joined_file_holds_a_s_frames_byte_for_byte(host, session, joined):
    joined_set, _, _, out = joined
    again = str(session["dir"] / "joined_again.mhkf")
    host.write_keyframe_file(again, joined_set)
    J, A = open(out, "rb").read(), open(session["fa"], "rb").read()
    assert open(again, "rb").read() == J                                   # the file the call wrote is the set it returned
    empty = str(session["dir"] / "empty.mhkf")
    host.write_keyframe_file(empty, dict(maps=session["a"]["maps"], frames=[]))
    header = len(open(empty, "rb").read()) - 16                            # (a frame count and a checksum follow the header)
    assert J[:header] == A[:header] and int.from_bytes(J[header:header + 8], "little") == KA + KB
    assert J[header + 8:header + 8 + len(A) - header - 16] == A[header + 8:-8]
    # ... and the file-to-file form writes that very file
    other = str(session["dir"] / "joined_files.mhkf")
    _join(host, session["fa"], session["fb"], session["text"], other)
    assert open(other, "rb").read() == J
    assert host.read_keyframe_file(out)["frames"][KA]["pose"] == joined_set["frames"][KA]["pose"]


def test_the_join_does_not_look_at_b_s_frame(host, session, joined):
    _, b2 = jc.sessions(jc.G2)
    assert np.abs(np.array(b2["frames"][0]["pose"]) - np.array(session["b"]["frames"][0]["pose"])).max() > 100.0
    joined2, is_joined, report = _join(host, session["a"], b2, session["text"])
    assert is_joined and _pairs(report) == _pairs(joined[2])
    assert [p["accepted"] for p in report["pairs"]] == [p["accepted"] for p in joined[2]["pairs"]]
    d = float(np.abs(_poses_b(joined2) - _poses_b(joined[0])).max())
    print("B recorded in another frame: joined poses differ by", d)
    assert d < 1e-6


def test_a_min_links_nothing_reaches_leaves_a_alone(host, session, joined):
    text = session["text"].replace("session_join:\n", "session_join:\n  min_links: 9\n")
    assert "min_links: 9" in text
    out = str(session["dir"] / "never.mhkf")
    joined_set, is_joined, report = _join(host, session["a"], session["b"], text, out)
    assert is_joined is False and report["joined"] is False and 2 <= report["links_accepted"] < 9 and _pairs(report) == _pairs(joined[2])
    assert "optimize" not in report["counts"] and report["optimizer_iterations"] == 0 and not os.path.exists(out)
    alone = str(session["dir"] / "alone.mhkf")
    host.write_keyframe_file(alone, joined_set)
    assert open(alone, "rb").read() == open(session["fa"], "rb").read()


def test_the_session_map_of_the_joined_set_is_one_insertion_of_a_then_b(host, session, joined):
    from mola_lidar_odometry_amd import capi
    built, of_a = host.build_session_maps(joined[0]), host.build_session_maps(session["a"])
    assert len(built) == 1 and len(built[0]["xyz"]) > len(of_a[0]["xyz"])
    m = capi.Map(capi.Context(0), **lc.MAP_PARAMS)
    m.insert_frames([(np.asarray(f["layers"][0][1], np.float32), f["pose"]) for f in joined[0]["frames"]])
    d = m.download()
    m.close()
    print("points of the session map: A", len(of_a[0]["xyz"]), "A and B joined", len(built[0]["xyz"]))
    assert d["xyz"].tobytes() == built[0]["xyz"].tobytes() and d["src_idx"].tobytes() == built[0]["src_idx"].tobytes()


def test_the_command_line_joins_the_two_files(host, session, joined, monkeypatch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    d = session["dir"]
    out, rep, mp_file = str(d / "cli.mhkf"), str(d / "cli.json"), str(d / "cli.mhmap")
    r = subprocess.run([CLI, "--join-sessions", session["fa"], session["fb"], "--pipeline", session["text_file"], "--output-simplemap", out,
                        "--output-session-map", mp_file, "--loop-report", rep], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(out, "rb").read() == open(joined[3], "rb").read()
    report = json.load(open(rep))
    assert [(p["i"], p["j"], p["phase"], p["accepted"]) for p in report["pairs"]] == \
        [(p["i"], p["j"], ["anchor", "forward", "backward"][p["phase"]], p["accepted"]) for p in joined[2]["pairs"]]
    assert report["cost_after"] == joined[2]["cost_after"] and set(report["seconds"]) >= {"index", "search", "submap", "score", "refine", "optimize"}
    summary = json.loads(r.stdout.strip().split("\n")[-1])
    assert summary["links_accepted"] == joined[2]["links_accepted"] and summary["joined"] is True and summary["frames"] == KA + KB
    built = host.build_session_maps(joined[0])
    got = host.read_local_map_file(mp_file)
    assert len(got) == 1 and got[0]["xyz"].tobytes() == built[0]["xyz"].tobytes() and got[0]["src_idx"].tobytes() == built[0]["src_idx"].tobytes()
    # sessions that are not joined: a non-zero exit, the summary says so, nothing is written
    strict, never, never_map = str(d / "strict.yaml"), str(d / "cli_never.mhkf"), str(d / "cli_never.mhmap")
    open(strict, "w").write(session["text"].replace("session_join:\n", "session_join:\n  min_links: 9\n"))
    r = subprocess.run([CLI, "--join-sessions", session["fa"], session["fb"], "--pipeline", strict, "--output-simplemap", never, "--output-session-map", never_map],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "not joined" in r.stderr and not os.path.exists(never) and not os.path.exists(never_map)
    lines = r.stdout.strip().split("\n")
    assert json.loads(lines[-1])["joined"] is False and json.loads(lines[0])["joined"] is False   # (without --loop-report the report goes to stdout)
    # a form that is not complete is refused with the usage
    r = subprocess.run([CLI, "--join-sessions", session["fa"], session["fb"], "--pipeline", session["text_file"]], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--output-simplemap" in r.stderr
