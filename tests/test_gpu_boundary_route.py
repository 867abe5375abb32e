"""EQF_OPT_QUIET_DOOR_WAIT (a doorbell wait that does not query the stream before it has lasted 2 ms) changes when the host looks at the stream and nothing
else: the same launches with the same arguments in the same order. Old route (option 0) and new route (option 1) are therefore compared BIT FOR BIT - Sigma,
the landmark planes (q0, Q) and the sensor state, the result packet (Gamma and the landmark estimates the lift wrote) and the counters of the speculation,
look-ahead and selection statistics - frame by frame on
  * bench.py's hover world at N = 50 and N = 200 (the path the headline times),
  * the wave world with the shipped EuRoC outlier thresholds (cancelled tails, removals, held landmarks),
  * one update forced to EQF_E_NOT_SPD, which must leave the state untouched on both routes.
(eqf_early_doorbell_stats is not compared: which of the two doorbells the host hears first is a race by design, and both outcomes are bit-identical.)"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from eqvio_amd.capi import OPT_QUIET_DOOR_WAIT, EqfError, PreparedFrames, VIOFilter, load_eqf_lib  # noqa: E402
from eqvio_amd.simworld import SimWorld  # noqa: E402
from test_gpu_filter_headline import counters  # noqa: E402
from test_gpu_parity import make_pair  # noqa: E402
from util import CHARTS, default_camera, synth_measurement  # noqa: E402

pytestmark = pytest.mark.gpu


def snapshot(flt):
    lib = load_eqf_lib()
    xi0, Xs, ids, q0, Q = flt.get_eqf()
    s, ids_e, p = flt.state_estimate()
    gamma = np.zeros(flt.sigma_dim() + 64)
    k = lib.eqf_last_gamma(flt.core_handle(), gamma.ctypes.data_as(C.POINTER(C.c_double)), len(gamma))
    # (k < 0: the context holds no Gamma that belongs to its present state, e.g. landmarks left behind the update; then the code itself is compared)
    return dict(xi0=xi0, Xs=Xs, ids=ids, q0=q0, Q=Q, sigma=flt.get_sigma(), est_sensor=s, est_ids=ids_e, est_p=p, gamma_len=np.array([k]), gamma=gamma[: max(k, 0)].copy()), counters(flt)


def assert_same(a, b, where):
    (sa, ka), (sb, kb) = a, b
    for name in sa:
        assert sa[name].shape == sb[name].shape and np.array_equal(sa[name], sb[name]), (where, name)
    assert ka == kb, (where, ka, kb)


def run_both(make, prepared_frames, cam, n_frames):
    """one filter per route, one after the other (a filter that has the device to itself takes the look-ahead kernel's HOME placement, as the bench line does),
    fed the same prepared frames one frame per call; returns the counters of the new route"""
    import gc

    shots = []
    for val in (0, 1):
        gc.collect()
        f = make()
        f.set_core_option(OPT_QUIET_DOOR_WAIT, val)
        prepared = PreparedFrames(cam, *bench.flatten_frames(prepared_frames))
        shots.append([])
        for k in range(n_frames):
            assert f.run_prepared(prepared, k, 1) == 1
            shots[-1].append(snapshot(f))
        f.close()
        del f
    for k in range(n_frames):
        assert_same(shots[0][k], shots[1][k], k)
    return shots[1][-1][1]


@pytest.mark.parametrize("N", [50, 200])
def test_hover_world_old_and_new_route_bit_identical(N):
    n_frames = 10
    world, frames = bench.build_workload(seed=100, n_frames=n_frames + 1, N=N)
    mk = lambda s, sensor, ids, p, t: VIOFilter(s, max_landmarks=N, sensor=sensor, ids=ids, p=p, time=t)  # noqa: E731
    k = run_both(lambda: bench.make_filter(world, bench.eurocish_settings(), N, None, frames, mk), frames[:n_frames], world.cam, n_frames)
    assert k["queued"] == n_frames and k["cancelled"] == 0 and k["la_launches"] == n_frames and k["la_fallbacks"] == 0, k


def test_wave_world_shipped_thresholds_old_and_new_route_bit_identical():
    N = 200
    s = bench.eurocish_settings()
    s.outlierThresholdAbs, s.outlierThresholdProb, s.featureRetention, s.initialPointVariance = 4.852186665580312, 0.03229809583062128, 0.18594708334486176, 129.90415638150924
    world = SimWorld(seed=321, num_points=2500, max_features=N, trajectory="wave", noise_px=0.5)
    frames = list(world.frames(9))
    sensor, ids, p = world.true_state(0.0, frames[0][2])
    p = p * (1.0 + 0.05 * np.random.default_rng(7).normal(size=(len(ids), 1)))
    k = run_both(lambda: VIOFilter(s, max_landmarks=N + 120, sensor=sensor, ids=ids, p=p, time=0.0), frames, world.cam, 8)
    assert k["cancelled"] >= 1 and k["sel_frames"] >= 3 and k["sel_discarded"] >= 3, k  # the run did meet cancelled tails and removals


def test_failed_update_leaves_the_state_untouched_on_both_routes():
    N = 60
    out = []
    for val in (0, 1):
        rng, settings, orc, core, (xi0, Xs, ids, q0, Q, S) = make_pair(CHARTS["euclid"], N, seed=5)
        core.set_option(OPT_QUIET_DOOR_WAIT, val)
        core.set_sigma(-S)  # C (-Sigma) C^T + R is indefinite
        before = core.get_state()
        cam = default_camera()
        mid, y = synth_measurement(rng, cam, ids, q0, Q, noise_px=1.0)
        with pytest.raises(EqfError) as e:
            core.vision_update(cam, mid, y, 1e-6, True, False)
            core.synchronize()
        assert e.value.code == -2  # EQF_E_NOT_SPD
        assert np.array_equal(core.get_sigma(), -S)
        for a, b in zip(core.get_state(), before):
            assert np.array_equal(a, b)
        core.set_sigma(S)  # and the context goes on: the same update on a proper Sigma
        core.vision_update(cam, mid, y, settings.measurementNoise**2, True, False)
        out.append((core.get_sigma(), core.get_state(), core.last_gamma()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][2], out[1][2])
    for a, b in zip(out[0][1], out[1][1]):
        assert np.array_equal(a, b)
