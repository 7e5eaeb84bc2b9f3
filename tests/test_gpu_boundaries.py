"""attpc_det_scatter at the scatter's rounding edges (tests/boundary_cases.py): mesh lines within a few ulp of a
whole-mm cell edge where the two cells are different pads, slice times on a time-bucket edge, times on the bucket
edges, positions far off the plane.  Against the reference's own transport of the same samples
(tests/golden/boundary.npz, one hop) and against the oracle, in every scatter build, the merge variant and
lone_bucket_kernel.  A kernel that contracts the mesh or slice arithmetic into FMAs fails here.  Needs a real MI355X:
``-m gpu``.

Every sample is an event of its own (its own dictionary, as in the fixture).  A test collects the samples that
differ and reports how many."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from tests import boundary_cases as bc
from tests.test_gpu_scatter_fixtures import _compare_with_dict, _configure, _plane_filling_event, device_scatter

pytestmark = pytest.mark.gpu

SEED = 0x5EED0000000A11CE  # high word set
REF_GROUPS = ("mesh", "mesh10", "mesh_lone", "lut_edge", "time", "far")
BUILDS = [(1, -1), (2, -1), (3, -1), (2, 1)]  # (scatter_variant, scatter_merge)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(golden_dir / "boundary.npz")


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _events(xyt, electrons):
    return [[(xyt[i][None], electrons[i:i + 1], bc.LABEL)] for i in range(len(xyt))]


def _differs(pts, lab, tbpad, charge, labels, event) -> str | None:
    try:
        _compare_with_dict(pts, lab, tbpad[:, 0], tbpad[:, 1], charge, labels, SEED, event)
    except AssertionError as e:
        return " ".join(str(e).split())[:160] or "differs"  # (numpy's messages start with a blank line)
    return None


def _oracle_dict(orc, raw, ev):
    keys, charge, labels = orc.transport(raw, ev)
    tbpad = np.array([orc.unpair(int(k)) for k in keys], dtype=np.int64).reshape(-1, 2)
    return tbpad, charge, labels


def _run(variant, merge, diffusion, events, **det_kw):
    """-> (clouds, stats, raw oracle descriptor) through a fresh context with the given build."""
    ctx = _abi.Context(0)
    try:
        ctx.set_option("scatter_variant", variant)
        ctx.set_option("scatter_merge", merge)
        cfg, raw, keep = _configure(ctx, diffusion, **det_kw)
        clouds, stats = device_scatter(ctx, events, seed=SEED)
    finally:
        ctx.close()
    return clouds, stats, (raw, keep)


@pytest.mark.parametrize("variant,merge", BUILDS, ids=["small", "big", "u64", "merge"])
@pytest.mark.parametrize("group", REF_GROUPS)
def test_scatter_at_decision_boundaries_vs_reference_and_oracle(fx, orc, group, variant, merge):
    """Keys, labels and the jittered time bucket exact, charges within 2, against the reference fixture (0 <= tb < 512
    mask applied to it) and against the oracle; no failed or inconsistent windows."""
    xyt, electrons = fx[f"{group}_xyt"], fx[f"{group}_electrons"]
    events = _events(xyt, electrons)
    clouds, stats, (raw, keep) = _run(variant, merge, float(fx[f"{group}_diffusion"]), events)
    assert stats["n_failed"] == 0 and stats["n_inconsistent"] == 0, stats
    o = fx[f"{group}_offsets"]
    bad_ref, bad_orc = [], []
    for e, (pts, lab) in enumerate(clouds):
        s = slice(o[e], o[e + 1])
        why = _differs(pts, lab, fx[f"{group}_tbpad"][s], fx[f"{group}_charge"][s], fx[f"{group}_labels"][s], e)
        if why:
            bad_ref.append((e, why))
        why = _differs(pts, lab, *_oracle_dict(orc, raw, events[e]), e)
        if why:
            bad_orc.append((e, why))
    print(group, variant, merge, "samples", len(events), "points", sum(len(c[0]) for c in clouds),
          "differ from reference", len(bad_ref), "from oracle", len(bad_orc))
    assert not bad_ref and not bad_orc, (f"{len(bad_ref)} of {len(events)} samples differ from the reference, "
                                         f"{len(bad_orc)} from the oracle: {(bad_ref + bad_orc)[:4]}")


@pytest.mark.parametrize("variant,merge", BUILDS, ids=["small", "big", "u64", "merge"])
def test_negative_times_give_no_points(fx, variant, merge):
    """t = -5e-324 (sigma_t^2 underflows to -0) and t = -1: dropped (deviation ii), as the
    oracle does (tests/test_boundaries_cpu.py)."""
    events = _events(fx["negtime_xyt"], fx["negtime_electrons"])
    clouds, stats, _ = _run(variant, merge, 0.277, events)
    assert stats["n_failed"] == 0 and all(len(pts) == 0 for pts, _ in clouds), [len(p) for p, _ in clouds]


@pytest.mark.parametrize("variant,merge", [(2, -1), (2, 1)], ids=["default", "merge"])
def test_slice_buckets_at_their_edges_vs_oracle(fx, orc, variant, merge):
    """Class B (longitudinal-diffusion extension, oracle only): a slice time on a bucket edge, or on t = 0."""
    events = _events(fx["slice_xyt"], fx["slice_electrons"])
    clouds, stats, (raw, keep) = _run(variant, merge, 0.277, events,
                                      longitudinal_diffusion=float(fx["slice_longitudinal_diffusion"]))
    assert stats["n_failed"] == 0 and stats["n_inconsistent"] == 0, stats
    bad = [(e, why) for e, (pts, lab) in enumerate(clouds)
           if (why := _differs(pts, lab, *_oracle_dict(orc, raw, events[e]), e))]
    print("slices", variant, merge, "samples", len(events), "differ", len(bad))
    assert not bad, f"{len(bad)} of {len(events)} samples differ from the oracle: {bad[:4]}"


@pytest.mark.parametrize("cls", ["mesh", "slice"])
def test_lone_kernel_at_decision_boundaries_vs_oracle(fx, orc, cls):
    """lone_bucket_kernel's own mesh and slice arithmetic: boundary samples inside a time bucket that overflows every
    LDS table (the plane-filling event of test_lone_time_bucket_larger_than_the_lds_table, the samples as a fifth
    track), build 1 (6144-slot table), against the oracle.  Every pad of that bucket is lit by the filler, so a moved
    pixel or slice shows as a charge (and label) difference of thousands of electrons.  Mesh: the samples of bucket
    500.  Slices: per event one class-B sample whose slice sits on the edge k - 1 | k, the filler in bucket k."""
    ctx = _abi.Context(0)
    try:
        ctx.set_option("scatter_variant", 1)
        if cls == "mesh":
            cfg, raw, keep = _configure(ctx, 0.277)
            events = [_plane_filling_event(cfg) + [(fx["mesh_lone_xyt"], fx["mesh_lone_electrons"], 3)]]
        else:
            cfg, raw, keep = _configure(ctx, 0.277, longitudinal_diffusion=float(fx["slice_longitudinal_diffusion"]))
            meta, xyt, el = fx["slice_meta"], fx["slice_xyt"], fx["slice_electrons"]
            pick = [i for i in range(len(meta)) if meta[i, 1] >= 1][::3]
            events = [_plane_filling_event(cfg, tb=float(meta[i, 1]) + 0.25) + [(xyt[i][None], el[i:i + 1], 3)]
                      for i in pick]
        clouds, stats = device_scatter(ctx, events, seed=SEED)
    finally:
        ctx.close()
    assert stats["n_failed"] == 0 and stats["n_inconsistent"] == 0, stats
    assert stats["n_lone_buckets"] >= len(events), stats
    bad = [(e, why) for e, (pts, lab) in enumerate(clouds)
           if (why := _differs(pts, lab, *_oracle_dict(orc, raw, events[e]), e))]
    print(cls, "events", len(events), "lone buckets", stats["n_lone_buckets"], "differ", len(bad))
    assert not bad, f"{len(bad)} of {len(events)} events differ from the oracle: {bad[:4]}"
