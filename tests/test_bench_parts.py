"""bench.py: a plain run measures the headline alone; --full adds every other part its --no-* options leave (no GPU)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402

ALL_PARTS = {"shared_map", "kernel_alone", "cpu_baseline", "extras", "lpt_curve"}


def parts(argv, world=1, rank=0):
    return bench.extra_parts(bench.parse_args(argv), world, rank)


def test_plain_run_measures_the_headline_alone():
    assert parts(["--gpus", "1", "--steps", "20", "--warmup", "5"]) == set()
    assert parts(["--gpus", "1", "--dump-outputs", "out"]) == set()
    assert parts(["--gpus", "2"], world=2) == parts(["--gpus", "2"], world=2, rank=1) == set()


def test_full_run_measures_every_part():
    assert parts(["--full"]) == ALL_PARTS
    # at N > 1 the CPU legs and the one-process sequence extras stay off; rank 0 alone times the kernel and runs the LPT curve
    assert parts(["--gpus", "2", "--full"], world=2) == {"shared_map", "kernel_alone", "lpt_curve"}
    assert parts(["--gpus", "2", "--full"], world=2, rank=1) == {"shared_map", "lpt_curve"}


def test_full_run_options_skip_their_parts():
    assert parts(["--full", "--no-shared-run"]) == ALL_PARTS - {"shared_map"}
    assert parts(["--full", "--no-profile"]) == ALL_PARTS - {"kernel_alone"}
    assert parts(["--full", "--no-cpu-baseline"]) == ALL_PARTS - {"cpu_baseline"}
    assert parts(["--full", "--no-lpt"]) == ALL_PARTS - {"lpt_curve"}
    assert parts(["--full", "--no-extras"]) == ALL_PARTS - {"extras", "lpt_curve"}
    assert parts(["--full", "--maps", "shared"]) == {"kernel_alone", "cpu_baseline"}
    assert parts(["--full", "--streams", "1", "--workload", "small"]) == {"kernel_alone", "cpu_baseline"}
