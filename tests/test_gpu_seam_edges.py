"""The seam edge-case table (tests/seam_edges.py) on the device: the push-relabel max-flow
(mcs_seam_flow_*, driven by seam_graphcut_device) and the sampler (mcs_seam_sample_c{1..4}_i{0,1})
at the inputs where they can go wrong -- boxes off the tile grid whose ring and overhang hold
another pair's leftovers, a sink hundreds of points away, one-row and one-column graphs, an empty
graph, a component without a terminal, coverage bit 15, 1 to 4 channels up to the largest arc,
every seam scale, mosaics that are no multiple of 2^k.  The reference is the oracle
(oracle/orc_seam.c, orc_blend.c), bit-exact; the host Dinic is the second opinion, so that a
disagreement says which of the three stands alone.  test_seam_edges_cpu.py shows that no case's
answer is trivial."""
import numpy as np
import pytest

import seam_edges as se
from oracle import oracle

pytestmark = pytest.mark.gpu


def _diff(a, b):
    return int(np.abs(a.astype(np.int16) - b.astype(np.int16)).max()) if a.size else 0


def _device_vs_references(lab, cov, smp):
    """The device's labels against the oracle's (the reference) and the host Dinic's; returns the
    labels and the driver's counters (pairs, push launches, relabel launches, global relabels,
    microseconds)."""
    from multicamera_stitching_amd import _capi
    n = smp.shape[0]
    want = oracle.seam_graphcut(lab, cov, smp)
    host = _capi.seam_graphcut_host(lab, cov, smp)
    got, st = _capi.seam_graphcut_device(lab, cov, smp, with_stats=True)
    msg = dict(device_vs_oracle=int((got != want).sum()), device_vs_host=int((got != host).sum()),
               host_vs_oracle=int((host != want).sum()), stats=st)
    if n == 2:
        # (capacity, terminal arcs cut): equal capacities and another labelling = a minimum cut
        # that is not the minimal one; a larger capacity or a cut terminal arc = no minimum cut
        msg["cut_device"] = se.cut_capacity(lab, cov, smp, got)
        msg["cut_oracle"] = se.cut_capacity(lab, cov, smp, want)
        msg["sides_device"] = se.side_counts(lab, cov, got)
        msg["sides_oracle"] = se.side_counts(lab, cov, want)
    oracle_says, host_says = np.array_equal(got, want), np.array_equal(got, host)
    assert oracle_says, msg
    assert host_says, msg
    assert st[0] == se.pairs_with_overlap(cov, n), msg
    return got, st


@pytest.mark.parametrize("name", [c["name"] for c in se.FLOW_CASES])
def test_flow_case_device_equals_oracle(name):
    case = se.FLOW_BY_NAME[name]
    lab, cov, smp = se.build_flow(name)
    got, st = _device_vs_references(lab, cov, smp)
    se.check_flow_property(case, lab, got)
    print(name, "stats", st)
    if name in ("snake", "snake_flat"):
        # the driver's own counters: the relabel fixpoint took more than one batch of
        # kRelabelBatch launches, and the flow more than one global relabel
        assert st[2] > se.RELABEL_BATCH and st[3] > 1, st


@pytest.mark.parametrize("seed", range(6))
def test_random_ragged_device_equals_oracle(seed):
    """The ragged inputs of test_seam_cpu.py (12 per seed): random owners, 1 to 4 channels,
    quantised costs, sizes 4..70."""
    from test_seam_cpu import _random_case
    rng = np.random.default_rng(seed)
    for trial in range(12):
        lab, cov, smp = _random_case(rng, trial)
        try:
            _device_vs_references(lab, cov, smp)
        except AssertionError as e:
            raise AssertionError(f"trial {trial}: {e}") from None


@pytest.mark.parametrize("name", ["snake", "quantised_ties", "sixteen_cams"])
def test_device_cut_is_deterministic(name):
    """Hong's push rule is racy by design, the cut it ends in is not: three runs in one process,
    equal labels."""
    from multicamera_stitching_amd import _capi
    lab, cov, smp = se.build_flow(name)
    runs = [_capi.seam_graphcut_device(lab, cov, smp) for _ in range(3)]
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])
    assert np.array_equal(runs[0], oracle.seam_graphcut(lab, cov, smp))


# One case per channel count in every blend mode; the others in multi-band (the plans' default).
ALL_MODES = {"chain_c3_k3", "chain_c2_k2", "chain_c1_nearest_k1", "cyl_c4_k2"}


@pytest.mark.parametrize("name", [c["name"] for c in se.PLAN_CASES])
def test_plan_seams_and_mosaic_equal_oracle(name):
    """find_seams on the noisy frames: the sampler's specialisation for the case's channels and
    interpolation at its scale, the device max-flow on what it sampled, and the stitch kernels'
    reads of the seam grid (the last grid row and column stand for a partial cell where the
    mosaic is no multiple of 2^k)."""
    case = se.PLAN_BY_NAME[name]
    pc = se.PlanCase(case)
    plan = pc.plan
    try:
        plan.set_blend(oracle.BLEND_MULTIBAND)
        plan.find_seams(pc.frames, scale_log2=case["k"])
        assert plan.seam_stats()[0] > 0, plan.seam_stats()
        labels = plan.seam_labels()
        for mode in ((2, 1, 3) if name in ALL_MODES else (2,)):
            plan.set_blend(mode)
            want, lab = pc.oracle(mode)
            off = int((labels != lab).sum())
            assert off == 0, f"mode {mode}: {off} of {lab.size} seam labels off the oracle's"
            assert np.array_equal(plan.seam_labels(), labels), mode
            assert _diff(plan.stitch_host(pc.frames).reshape(want.shape), want) == 0, mode
    finally:
        plan.close()


def test_second_find_seams_equals_a_fresh_plan():
    """find_seams again on the same plan with other frames, at another scale: the seam scratch and
    the plan's device grid are released and rebuilt, and nothing of the first call stays."""
    case = se.PLAN_BY_NAME["chain_c3_nearest_k1"]
    used, fresh = se.PlanCase(case), se.PlanCase(case, noise_seed=101)
    try:
        for pc in (used, fresh):
            pc.plan.set_blend(oracle.BLEND_MULTIBAND)
        used.plan.find_seams(used.frames, scale_log2=2)
        first = used.plan.seam_labels().copy()
        used.plan.find_seams(fresh.frames, scale_log2=case["k"])
        fresh.plan.find_seams(fresh.frames, scale_log2=case["k"])
        assert first.shape != fresh.plan.seam_labels().shape
        want, lab = fresh.oracle(oracle.BLEND_MULTIBAND)
        assert np.array_equal(used.plan.seam_labels(), fresh.plan.seam_labels())
        assert np.array_equal(used.plan.seam_labels(), lab)
        got = used.plan.stitch_host(fresh.frames)
        assert np.array_equal(got, fresh.plan.stitch_host(fresh.frames))
        assert _diff(got.reshape(want.shape), want) == 0
        # the seams depend on the capture: the first frames' seams on this grid are others
        _, lab_first = used.oracle(oracle.BLEND_MULTIBAND)
        assert not np.array_equal(lab, lab_first)
    finally:
        used.plan.close()
        fresh.plan.close()
