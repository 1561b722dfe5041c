"""The occupancy grid of a recorded session, the parts that need no device: the fourth public header and its binding, the
occupancy_grid: options, the host rules (height to index, the trinary rule, the PGM / YAML pair) against tests/occgrid_ref.py
-- exactly --, the refusals, and two conditions on the cases the device is held to in tests/test_gpu_occgrid.py:

 * the clamp case tells a fold in frame order from a sum of counts: OccMapRef fed the frames in order leaves the wall cell at -33,
   fed the summed counts in one insert at -47 (counted) or 14 (once);
 * the restatement alone, on the 12 key-frames of the room: 29 505 interior cells of which 548 unknown (1.86 %: the shadow of the box,
   which no key-frame looks behind) and 0 occupied; 704 wall sites of which 10 hold no occupied cell (1.42 %); 740 outside cells of
   which 0 known."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import occgrid_cases as oc
import occgrid_ref as G
import occmap_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "molahip_occgrid.h")
CLI = os.path.join(ROOT, "mola_lidar_odometry_amd", "molahip-lo-cli")


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


@pytest.fixture(scope="module")
def og():
    from mola_lidar_odometry_amd import capi_occgrid
    return capi_occgrid


# ---- the surface -------------------------------------------------------------------------------------------------------------------
def declared():
    return sorted(set(re.findall(r"MH_API\s+[\w\s\*]+?\b(mh_\w+)\s*\(", open(HEADER).read())))


def test_the_fourth_header_is_declared_exported_and_bound(og):
    from mola_lidar_odometry_amd import capi, capi_clean, capi_live
    fns = declared()
    assert fns == sorted(og._SIGNATURES) == ["mh_occgrid_api_version", "mh_occmap_index_bounds", "mh_occmap_insert_frames", "mh_occmap_project_grid"]
    for other in (capi, capi_clean, capi_live):                      # nothing of it went into another header's table
        assert not set(fns) & set(other._SIGNATURES)
    L = og.lib()
    for fn in fns:
        assert hasattr(L, fn), fn
    assert int(L.mh_occgrid_api_version()) == og.OCCGRID_API_VERSION == 1
    assert int(L.mh_abi_version()) == 7                              # the first header's version is untouched
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(fns) <= exported and all(s.startswith("mh_") for s in exported)
    for d in re.findall(r"MH_API[^;]+;", open(HEADER).read()):       # plain C types only in the signatures
        assert not re.search(r"torch|at::|std::|Tensor|&", d), d
    first = open(os.path.join(ROOT, "include", "molahip.h")).read()
    assert "occgrid" not in first and "mh_occmap_insert_frames" not in first


def test_the_header_compiles_as_c_and_the_layout_is_the_mirror_s(og, tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "molahip_occgrid.h"
int main(void){
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(mh_occgrid_window), offsetof(mh_occgrid_window, x0), offsetof(mh_occgrid_window, y0),
    offsetof(mh_occgrid_window, nx), offsetof(mh_occgrid_window, ny), offsetof(mh_occgrid_window, z_lo), offsetof(mh_occgrid_window, z_hi));
  printf("%d %d %d %d %zu %zu %zu\n", MH_OCCGRID_API_VERSION, MH_OCCGRID_NONE, MH_ABI_VERSION, MH_MAX_INSERT_FRAMES, sizeof(mh_map_frame),
    sizeof(mh_occmap_params), sizeof(mh_occmap_info));
  return 0; }''')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    a, b = subprocess.check_output([str(exe)], text=True).strip().splitlines()
    from mola_lidar_odometry_amd import capi
    W = og.GridWindow
    assert [int(v) for v in a.split()] == [C.sizeof(W), W.x0.offset, W.y0.offset, W.nx.offset, W.ny.offset, W.z_lo.offset, W.z_hi.offset]
    assert C.sizeof(W) == 24
    assert [int(v) for v in b.split()] == [1, og.NONE, 7, og.MAX_INSERT_FRAMES, C.sizeof(capi.MapFrame), C.sizeof(capi.OccMapParams),
                                           C.sizeof(capi.OccMapInfo)]
    assert og.NONE == G.NONE == -2147483648 and C.sizeof(capi.MapFrame) == 128


def test_every_call_fails_loudly_without_a_device_and_refusals_need_none(og):
    from mola_lidar_odometry_amd import capi
    L = og.lib()
    _, arr = og.frame_table([(np.zeros((4, 3), np.float32), oc.I12)])
    n = C.c_uint64(0)
    three = (C.c_int32 * 3)()
    w = og.GridWindow(0, 0, 4, 4, 0, 0)
    out = (C.c_int32 * 16)()
    assert L.mh_occmap_insert_frames(None, arr, 1, capi.MEM_HOST, 0) == 1          # MH_ERR_INVALID_ARGUMENT, whatever the machine
    assert L.mh_occmap_index_bounds(None, three, three, C.byref(n)) == 1
    assert L.mh_occmap_project_grid(None, C.byref(w), out) == 1
    assert b"null" in L.mh_last_error_string()
    if capi.device_count() == 0:
        with pytest.raises(capi.MolahipError) as e:                                # no map without a device: nothing falls back to the host
            capi.OccMap(capi.Context(0))
        assert e.value.status == 5


def test_without_a_device_the_host_path_raises_too(host):
    from mola_lidar_odometry_amd import capi
    if capi.device_count() == 0:
        with pytest.raises(RuntimeError):
            host.build_occupancy_grid(G.room_session()[1])


# ---- options -----------------------------------------------------------------------------------------------------------------------
def _opts(host, text):
    d = dict(host.occupancy_grid_options(text))
    d.pop("z_lo"), d.pop("z_hi")
    return d


def test_the_defaults_are_lidar2d_s_and_the_restatement_s(host):
    assert _opts(host, None) == G.DEFAULTS == _opts(host, "occupancy_grid:\n") == _opts(host, host.Config.FromYamlText("other: 1\n"))
    d = host.occupancy_grid_options(None)
    assert (d["z_lo"], d["z_hi"]) == (G.z_index(-0.10, 0.05), G.z_index(1.50, 0.05)) == (-2, 30)
    assert R.five_integers(d["prob_hit"], d["prob_miss"], d["clamp_min"], d["clamp_max"], d["occupied_threshold"]) == (14, 14, -47, 47, 7)


@pytest.mark.parametrize("key,value", [("resolution", 0.1), ("prob_hit", 0.8), ("prob_miss", 0.2), ("clamp_min", 0.1), ("clamp_max", 0.9),
                                       ("occupied_threshold", 0.7), ("ray_trace_free_space", False), ("max_range", 25.0), ("decimation", 3),
                                       ("update_rule", "once"), ("target_map", "points"), ("z_min", -1.5), ("z_max", 0.25), ("margin_cells", 0)])
def test_each_key_is_read(host, key, value):
    text = "occupancy_grid:\n  %s: %s\n" % (key, str(value).lower() if isinstance(value, bool) else value)
    assert _opts(host, text) == dict(G.DEFAULTS, **{key: value})


@pytest.mark.parametrize("key,value", [("resolution", 0), ("resolution", "nan"), ("resolution", "abc"), ("prob_hit", 0), ("prob_hit", 1.0),
                                       ("prob_miss", -0.1), ("clamp_min", 1), ("clamp_max", 0.01), ("clamp_max", 1.5), ("occupied_threshold", 0),
                                       ("ray_trace_free_space", "maybe"), ("max_range", -1), ("max_range", "inf"), ("decimation", 0),
                                       ("decimation", 1.5), ("update_rule", "summed"), ("z_min", "nan"), ("z_max", -5), ("z_max", 1e9),
                                       ("margin_cells", -1), ("margin_cells", 100000), ("no_such_key", 1), ("zmin", 0)])
def test_a_bad_value_or_an_unknown_key_is_refused_by_name(host, key, value):
    with pytest.raises(RuntimeError, match=r"occupancy_grid: %s\b" % key):
        host.occupancy_grid_options("occupancy_grid:\n  %s: %s\n" % (key, value))


# the six option blocks that are read alike: (entry point, block, a number key, a count key, a boolean key)
OPTION_BLOCKS = [("occupancy_grid_options", "occupancy_grid", "resolution", "decimation", "ray_trace_free_space"),
                 ("traversability_options", "traversability", "resolution", "margin_cells", None),
                 ("costmap_options", "costmap", "cost_scaling", None, "unknown_is_obstacle"),
                 ("gyro_deskew_options", "gyro_deskew", "max_gap", None, "enabled"),
                 ("map_cleaning_options", "map_cleaning", "rel_margin", "n_rings", None),
                 ("online_map_cleaning_options", "online_map_cleaning", "rel_margin", "max_views", "enabled")]


@pytest.mark.parametrize("entry,block,key", [(e, b, k) for e, b, *keys in OPTION_BLOCKS for k in keys if k])
def test_every_block_refuses_a_list_a_map_and_text_by_name_and_takes_null_as_absent(host, entry, block, key):
    read = getattr(host, entry)
    for value in ("[1, 2]", "{a: 1}", "1x"):
        with pytest.raises(RuntimeError, match=r"%s: %s\b" % (block, key)):
            read("%s:\n  %s: %s\n" % (block, key, value))
    for null in ("~", ""):                                     # (this YAML subset's nulls)
        assert read("%s:\n  %s: %s\n" % (block, key, null)) == read()


# ---- the host rules ----------------------------------------------------------------------------------------------------------------
def test_heights_become_indices_by_the_floor_rule_on_boundaries(host):
    hand = {(0.0, 0.05): 0, (-1e-12, 0.05): -1, (0.05, 0.05): 1, (0.0499999, 0.05): 0, (-0.05, 0.05): -1, (-0.0500001, 0.05): -2,
            (1.0, 0.25): 4, (0.999999, 0.25): 3, (-0.25, 0.25): -1, (-0.250001, 0.25): -2, (3.0, 0.1): 30, (-3.0, 0.1): -30}
    for (z, res), want in hand.items():
        assert host.occupancy_grid_z_index(z, res) == G.z_index(z, res) == want, (z, res)
    rng = np.random.default_rng(2)
    for res in (0.05, 0.1, 0.2, 0.25, 0.3):
        ks = rng.integers(-400, 400, 50)
        for z in np.concatenate([ks * res, np.nextafter(ks * res, np.inf), np.nextafter(ks * res, -np.inf), rng.uniform(-20, 20, 50)]):
            assert host.occupancy_grid_z_index(float(z), res) == G.z_index(float(z), res)


def test_the_trinary_rule_on_hand_made_maxima(host):
    l_occ = 7
    mx = np.array([[G.NONE, -47, 0, 6], [7, 8, 47, G.NONE + 1], [-1, G.NONE, 2147483647, 7]], np.int32)
    want = np.array([[-1, 0, 0, 0], [100, 100, 100, 0], [0, -1, 100, 100]], np.int8)
    cells, n_occ, n_free, n_unk = host.occupancy_grid_classify(mx, l_occ)
    assert cells.dtype == np.int8 and (cells == want).all() and (n_occ, n_free, n_unk) == (5, 5, 2)
    ref = G.classify(mx, l_occ)
    assert (ref[0] == want).all() and ref[1:] == (5, 5, 2)
    cells, n_occ, n_free, n_unk = host.occupancy_grid_classify(mx, -47)          # another threshold: only NONE + 1 stays below it
    assert (n_occ, n_free, n_unk) == (9, 1, 2) and cells[1, 3] == 0


def _hand_grid():
    rng = np.random.default_rng(11)
    cells = rng.choice(np.array([G.FREE, G.OCCUPIED, G.UNKNOWN], np.int8), (5, 7))
    cells[0, 0], cells[4, 6], cells[0, 6] = G.OCCUPIED, G.FREE, G.UNKNOWN       # the corners tell a flip from a transpose
    return dict(x0=-13, y0=4, nx=7, ny=5, resolution=0.05, cells=cells)


def test_the_files_are_written_byte_for_byte_and_read_back(host, tmp_path):
    g = _hand_grid()
    prefix = str(tmp_path / "room")
    host.write_occupancy_grid(g, prefix)
    pgm = open(prefix + ".pgm", "rb").read()
    assert pgm == G.pgm_bytes(g["cells"]) and pgm.startswith(b"P5\n7 5\n255\n") and len(pgm) == 11 + 35
    assert pgm[11] == {G.OCCUPIED: 0, G.FREE: 254, G.UNKNOWN: 205}[int(g["cells"][4, 0])]   # the first byte is the top row: the largest y
    assert pgm[-7] == 0 and pgm[-1] == 205                                                  # the bottom row is row 0 of the grid
    text = open(prefix + ".yaml").read()
    assert text == G.yaml_text("room.pgm", 0.05, -13, 4)
    assert text == "image: room.pgm\nresolution: 0.05\norigin: [-0.65, 0.2, 0]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n"
    back = host.read_occupancy_grid(prefix)
    assert (back["x0"], back["y0"], back["nx"], back["ny"], back["resolution"]) == (-13, 4, 7, 5, 0.05)
    assert (back["cells"] == g["cells"]).all() and back["cells"].dtype == np.int8
    c = g["cells"]
    assert (back["cells_occupied"], back["cells_free"], back["cells_unknown"]) == (int((c == 100).sum()), int((c == 0).sum()), int((c == -1).sum()))
    # from maxima: the rule is applied on the way
    mx = np.where(c == G.UNKNOWN, G.NONE, np.where(c == G.OCCUPIED, 9, -3)).astype(np.int32)
    host.write_occupancy_grid(dict(x0=-13, y0=4, nx=7, ny=5, resolution=0.05, l_occ=7, max_logodds=mx), prefix + "2")
    assert open(prefix + "2.pgm", "rb").read() == pgm


def test_the_reader_and_the_writer_refuse_what_they_cannot_take(host, tmp_path):
    with pytest.raises(RuntimeError, match="nowhere"):
        host.read_occupancy_grid(str(tmp_path / "nowhere"))
    with pytest.raises(RuntimeError, match="cannot write"):
        host.write_occupancy_grid(_hand_grid(), str(tmp_path / "no_such_dir" / "g"))
    prefix = str(tmp_path / "g")
    host.write_occupancy_grid(_hand_grid(), prefix)
    raw = open(prefix + ".pgm", "rb").read()
    open(prefix + ".pgm", "wb").write(raw[:-1])
    with pytest.raises(RuntimeError, match="g.pgm"):
        host.read_occupancy_grid(prefix)
    open(prefix + ".pgm", "wb").write(raw[:-1] + b"\x07")
    with pytest.raises(RuntimeError, match="neither"):
        host.read_occupancy_grid(prefix)


# (this reader has no other image to hold the size against: a size is wrong when it is not the size of what follows the header)
@pytest.mark.parametrize("header", [b"P5\n7 5\n255 ", b"P5\n7 5\n255\n\n", b"P5\n7 5\n254\n", b"P5\n7 6\n255\n", b"P5\n0 5\n255\n"])
def test_an_image_whose_header_is_not_the_writer_s_is_refused(host, tmp_path, header):
    prefix = str(tmp_path / "g")
    host.write_occupancy_grid(_hand_grid(), prefix)
    raw = open(prefix + ".pgm", "rb").read()
    assert raw[:11] == b"P5\n7 5\n255\n"
    open(prefix + ".pgm", "wb").write(header + raw[11:])
    with pytest.raises(RuntimeError, match="is not a binary PGM written by write_occupancy_grid"):
        host.read_occupancy_grid(prefix)
    open(prefix + ".pgm", "wb").write(raw)
    assert (host.read_occupancy_grid(prefix)["cells"] == _hand_grid()["cells"]).all()


def test_the_cli_refuses_a_missing_file_by_name_and_an_incomplete_form(tmp_path):
    missing = str(tmp_path / "no_such_keyframes.kf")
    r = subprocess.run([CLI, "--build-occupancy-grid", missing, str(tmp_path / "out")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "no_such_keyframes.kf" in r.stderr and not os.path.exists(str(tmp_path / "out.pgm"))
    r = subprocess.run([CLI, "--build-occupancy-grid", missing], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "missing value for --build-occupancy-grid" in r.stderr
    r = subprocess.run([CLI, "--build-occupancy-grid", missing, "out", "--seq-dir", "x"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "takes no sequence" in r.stderr
    bad = tmp_path / "bad.yaml"
    bad.write_text("occupancy_grid:\n  cell_size: 0.1\n")
    r = subprocess.run([CLI, "--build-occupancy-grid", missing, "out", "-c", str(bad)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "occupancy_grid: cell_size" in r.stderr


# ---- the conditions on the GPU test's cases ----------------------------------------------------------------------------------------
def _summed_in_one_insert(frames, rule):
    """what an implementation that sums the counts of all frames and applies the rule once would leave: ONE insert of all points"""
    m = R.OccMapRef(resolution=oc.RES, update_rule=rule)
    assert all((T == oc.I12).all() for _, T in frames)
    return m.insert(np.concatenate([xyz for xyz, _ in frames]), oc.I12)


@pytest.mark.parametrize("rule,name", [(R.COUNTED, "counted"), (R.ONCE, "once")])
def test_the_clamp_case_tells_a_fold_in_frame_order_from_a_sum_of_counts(rule, name):
    frames = oc.clamp_frames()
    m = R.OccMapRef(resolution=oc.RES, update_rule=rule)
    assert (m.l_hit, m.l_miss, m.l_min, m.l_max) == (14, 14, -47, 47)
    trace = []
    for xyz, T in frames:
        m.insert(xyz, T)
        trace.append(m.cells[oc.WALL])
    assert trace == [14, 28, 42, 47, 47, 47, 33, 19, 5, -9, -23, -37, -47, -47, -33]      # l_max reached, then l_min, then a hit
    assert m.cells[oc.WALL] == oc.WALL_IN_ORDER
    summed = _summed_in_one_insert(frames, rule)
    assert summed.cells[oc.WALL] == oc.WALL_SUMMED[name] != oc.WALL_IN_ORDER
    assert set(summed.cells) == set(m.cells)                                              # the same cells, another value


def test_the_once_rule_s_own_case_is_order_sensitive_too():
    frames = oc.clamp_frames_once_own()
    m = R.OccMapRef(resolution=oc.RES, update_rule=R.ONCE)
    trace = []
    for xyz, T in frames:
        m.insert(xyz, T)
        trace.append(m.cells[oc.WALL])
    assert trace == [-14, -28, -14, 0, 14, 28, 42, 28, 14, 0, 14]                         # a frame that hits and looks through: the hit wins
    assert _summed_in_one_insert(frames, R.ONCE).cells[oc.WALL] == 14
    counted = R.OccMapRef(resolution=oc.RES, update_rule=R.COUNTED)
    for xyz, T in frames:
        counted.insert(xyz, T)
    assert counted.cells[oc.WALL] != m.cells[oc.WALL]                                     # ... and the two rules differ on it


def test_the_restatement_alone_reads_the_room():
    frames, kfset = G.room_session()
    assert len(frames) == G.ROOM_FRAMES == len(kfset["frames"]) and kfset["maps"][0]["class_name"] == "CVoxelMap"
    g = G.build(frames)
    n_in, in_unknown, in_occupied, n_sites, sites_open, n_out, out_known = G.room_shares(g)
    assert (n_in, in_unknown, in_occupied) == (29505, 548, 0)
    assert (n_sites, sites_open) == (704, 10)
    assert (n_out, out_known) == (740, 0)
    assert (g["nx"], g["ny"], g["z_lo"], g["z_hi"], g["l_occ"]) == (206, 166, -2, 30, 7)
