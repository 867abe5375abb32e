"""The filter batch under the Normal chart (helper module, not a test): eqf_batch_set_slot_chart, k_batch_normal / k_batch_riccati_normal / k_batch_discrete_normal
(eqvio_amd/csrc/eqf_batch.hpp). Nothing is generated here: the planted frames are those of tests/batch_scenarios.py and tests/riccati_cases.py, built by their
own generators - imported and unchanged - from settings whose coordinateChoice is Normal, so the sizes are the kernels' lane, wave and tile edges (bs.SIZES) and
the bookkeeping edges are the ones the other two charts are tested at.

 * normal(**kw) is bs.shipped_euroc with the Normal chart: what a Normal slot's ORACLE runs with, and what the generators build a scenario from.
 * batch_settings(sn) is sn with the Euclidean chart: what the batch is created with - its settings calls refuse the Normal chart, which a slot gets from
   set_slot_chart. with_chart(s, chart) is the twin of s under another chart, everything else equal.
 * make_batch(sn, slots) is a VIOFilterBatch whose every slot runs sn: created with batch_settings(sn), every (still empty) slot switched to Normal.
 * GROUPS / build_group(name): (Normal settings, scenarios), built once per process. riccati(**kw): (sn, accurate oracle settings, discrete oracle settings,
   rc.build's cases)."""
import batch_scenarios as bs
import discrete_cases as dc
import riccati_cases as rc
from eqvio_amd.capi import COORD_EUCLIDEAN, COORD_NORMAL, Settings


def with_chart(s, chart):
    o = Settings.from_buffer_copy(bytes(s))
    o.coordinateChoice = chart
    return o


def normal(**kw):
    return bs.shipped_euroc(coordinateChoice=COORD_NORMAL, **kw)


def batch_settings(sn):
    return with_chart(sn, COORD_EUCLIDEAN)


def make_batch(sn, slots, cap=64):
    from eqvio_amd.batch import VIOFilterBatch

    batch = VIOFilterBatch(batch_settings(sn), slots, cap)
    batch.set_slot_chart(None, COORD_NORMAL)
    return batch


RANK_CAP = bs.C_ABS + 1  # the one cap the ranking runs at here: every absolute outlier and the worst probabilistic one go
GROUPS = {}
for _lift in (0, 1):
    for _out in (0, 1):
        GROUPS[f"sizes_lift{_lift}_out{_out}"] = (lambda l=_lift, o=_out: normal(useDiscreteInnovationLift=l, useEquivariantOutput=o), bs.size_grid)
GROUPS["partial"] = (lambda: normal(removeLostLandmarks=0), bs.partial)
GROUPS["turnover_fixed"] = (normal, lambda s: bs.turnover(s, False))
GROUPS["turnover_median"] = (lambda: normal(useMedianDepth=1, initialSceneDepth=7.5), lambda s: bs.turnover(s, True))
GROUPS["rank"] = (lambda: normal(featureRetention=bs.retention_for(RANK_CAP), **bs.RANK_SETTINGS), bs.ranking)
GROUPS["invalid_ends"] = (normal, bs.invalid_ends)
GROUPS["failures"] = (lambda: normal(outlierThresholdAbs=1e8, outlierThresholdProb=1e8), bs.failures)
GROUPS["unequal_imu"] = (normal, bs.unequal_imu)
SIZE_GROUPS = [g for g in GROUPS if g.startswith("sizes_")]

_built = {}


def build_group(name):
    if name not in _built:
        make_settings, make_scenarios = GROUPS[name]
        s = make_settings()
        _built[name] = (s, make_scenarios(s))
    return _built[name]


def riccati(**kw):
    key = ("riccati", tuple(sorted(kw.items())))
    if key not in _built:
        sn = normal(**kw)
        _built[key] = (sn, rc.oracle_settings(sn), dc.oracle_settings(sn), rc.build(sn, "normal"))
    return _built[key]
