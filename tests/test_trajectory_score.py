"""trajectoryPositionRMSE (eqvio_amd/host/DatasetReplay.hpp), the score `eqvio_opt --batch B --groundtruth FILE` prints per slot, on the CPU through the host
program tests/host/trajectory_score.cpp: a rigid transform of the ground truth scores 0 to rounding, a constant offset d from the second frame on scores
d sqrt((F - 1) / F), rows with stamp -1 are skipped, the nearest ground-truth pose is the earlier one on a tie, and an empty input gives NaN and 0 frames."""
import __graft_entry__ as g
from test_host_units import build_and_run


def test_trajectory_position_rmse(tmp_path):
    g.build()
    out = build_and_run(tmp_path, "trajectory_score")
    print(out)
    assert out.strip().splitlines()[-1] == "ok"
