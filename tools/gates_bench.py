"""Gated matchers on the fused multi-layer loop against the matcher-by-matcher loop, in the stand-alone driver: molahip-lo-cli on a
pipeline with an iteration gate (the reference's pipelines/extras/lidar3d-near-far.yaml) over the synthetic city drive of
tools/multi_seq_bench.py, one sequence, MOLA_HIP_FUSE_GATES=1 against =0 in alternating runs of one build.
    python tools/gates_bench.py PIPELINE.yaml [scans=120] [out.json] [switch=MOLA_HIP_FUSE_GATES]
(switch: MOLA_HIP_FUSE_KBEST for a pipeline with pairingsPerPoint > 1, profiles/layers_kbest.md.)
Prints one line per run: steady scans/s, the profile's per-scan milliseconds and ICP counters."""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (CLI: the path of molahip-lo-cli)
from mola_lidar_odometry_amd import synth_city  # noqa: E402


def main():
    pipeline = sys.argv[1]
    n_scans = int(sys.argv[2]) if len(sys.argv) > 2 else 120
    switch = sys.argv[4] if len(sys.argv) > 4 else "MOLA_HIP_FUSE_GATES"
    tmp = tempfile.mkdtemp(prefix="molahip_gates_")
    seq, _ = synth_city.write_kitti_drive(tmp, n_scans, time_channel=True)
    print("drive written", flush=True)
    runs = {"0": [], "1": []}
    for rep in range(3):
        for mode in ("1", "0"):
            cmd = [bench.CLI, "--pipeline", pipeline, "--out", os.path.join(tmp, "t%s_%d.tum" % (mode, rep)), "--profile",
                   "--time-field", "12", "--seq-dir", seq]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=280, env=dict(os.environ, **{switch: mode}))
            if r.returncode != 0:
                print("molahip-lo-cli failed (%d): %s" % (r.returncode, r.stderr[-800:]), flush=True)
                return 3
            lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
            per = [l for l in lines if "sequence_dir" in l][0]
            prof = [l["profile_ms_per_scan"] for l in lines if "profile_ms_per_scan" in l][0]
            rec = dict(steady_scans_per_s=per["steady_scans_per_s"], scans=per["scans"], good=per["good"],
                       profile={k: v for k, v in prof.items() if k.startswith("icp.") or k.startswith("onLidar")})
            runs[mode].append(rec)
            print("%s=%s run %d: %s" % (switch, mode, rep, json.dumps(rec)), flush=True)
    if len(sys.argv) > 3:
        json.dump(runs, open(sys.argv[3], "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
