"""The rows step of the scatter kernel (rows_round / rows_round_merge + queue_put + stream_insert) through
attpc_det_scatter against the oracle, on hand-made samples aimed at what that step does per 64 mesh lines: the
mirrored pixel weights, the line number -> (entry, line) split at the edges of a wave's and a workgroup's block of
lines, and a wave that stops on a full table.  Every case runs in the three builds of the kernel and in the merge
variant.  Needs a real MI355X: ``-m gpu``.

Tolerances: keys, labels, zero-charge inserts and the jittered time bucket exact, charges
within 2 electrons (numpy's exp in the oracle's pdf against the kernel's constant weight table)."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from tests.test_gpu_scatter_fixtures import _compare_with_dict, _configure, device_scatter

pytestmark = pytest.mark.gpu

SEED = 11
LABEL = 2
# (scatter_variant, scatter_merge): two / one workgroup per CU with u32 sums, u64 sums; the merge variant of the
# two table sizes with u32 sums
BUILDS = [(1, 0), (2, 0), (3, 0), (1, 1), (2, 1)]
BUILD_IDS = ["small", "big", "u64", "small-merge", "big-merge"]
TABLE_SLOTS = {1: 6144, 2: 12288, 3: 8192}  # scatter.hip: HASH_CAP; a window aims at half of them (TARGET_KEYS)


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _run(variant, merge, diffusion, events):
    ctx = _abi.Context(0)
    try:
        ctx.set_option("scatter_variant", variant)
        ctx.set_option("scatter_merge", merge)
        cfg, raw, keep = _configure(ctx, diffusion)
        clouds, stats = device_scatter(ctx, events, seed=SEED)
    finally:
        ctx.close()
    return clouds, stats, (raw, keep)


def _oracle_dict(orc, raw, ev):
    keys, charge, labels = orc.transport(raw, ev)
    tbpad = np.array([orc.unpair(int(k)) for k in keys], dtype=np.int64).reshape(-1, 2)
    return tbpad, charge, labels


def _assert_clouds_equal_oracle(orc, raw, events, clouds):
    """-> points compared.  Collects the events that differ and reports how many."""
    bad, points = [], 0
    for e, (ev, (pts, lab)) in enumerate(zip(events, clouds)):
        tbpad, charge, labels = _oracle_dict(orc, raw, ev)
        try:
            _compare_with_dict(pts, lab, tbpad[:, 0], tbpad[:, 1], charge, labels, SEED, e)
        except AssertionError as err:
            bad.append((e, " ".join(str(err).split())[:160] or "differs"))
        points += len(pts)
    assert not bad, f"{len(bad)} of {len(events)} events differ from the oracle: {bad[:4]}"
    return points


# ---- mirror: el[9 - j] = el[j] ----
# 10x diffusion at far drift: sigma_t = 10 mm, the mesh pitch (7 mm) is wider than a pad, nearly every pixel of a line
# sits on a pad of its own -- so a pixel that took the wrong half's charge shows as a charge difference.  Off-centre
# positions (the two halves of a line see different pads), one at the plane's edge and one whose outer lines leave the
# whole-mm table (pixels fall off the plane).  Electron counts whose per-pixel truncations all differ; the last one
# puts the centre pixels of lines 4 and 5 beyond 2^28 (0.0633 x 5e9 = 3.2e8): those lines take the slow path, which
# reads the weights one by one.
MIRROR_XY = [(0.1313, -0.0877), (0.0213, 0.0117), (-0.2581, 0.0304), (0.0107, 0.2752)]
MIRROR_ELECTRONS = [3_000_001, 123_457, 5_000_000_007]


def _mirror_events():
    return [[(np.array([[x, y, 480.5 + 3.0 * k]]), np.array([n], dtype=np.int64), LABEL)]
            for x, y in MIRROR_XY for k, n in enumerate(MIRROR_ELECTRONS)]


@pytest.mark.parametrize("variant,merge", BUILDS, ids=BUILD_IDS)
def test_mirrored_pixel_charges_vs_oracle(orc, variant, merge):
    events = _mirror_events()
    clouds, stats, (raw, keep) = _run(variant, merge, 2.77, events)
    assert stats["n_failed"] == 0 and stats["n_inconsistent"] == 0, stats
    points = _assert_clouds_equal_oracle(orc, raw, events, clouds)
    per_event = [len(pts) for pts, _ in clouds]
    print("mirror", variant, merge, "points per event", per_event)
    # the premise: most pixels on a pad of their own where the whole mesh is on the plane (70 to 81 pads for 100
    # pixels), about half of the mesh off the plane at its edge
    assert max(per_event) >= 70 and min(per_event) < 50 and points == sum(per_event)


# ---- block edges: 64 lines per wave, 512 / 1 024 per workgroup and pass ----
EDGE_SAMPLES = [1, 6, 7, 51, 52, 102, 103, 205]  # x 10 lines: either side of 64, 512 and 1 024 (and of 2 x 1 024)


def _edge_events(spread_over_buckets: bool):
    events = []
    for n in EDGE_SAMPLES:
        k = np.arange(n, dtype=np.float64)
        x, y = -0.1207 + 1.1e-3 * k, 0.0411 + 0.35e-3 * k  # a straight track through small and large pads
        t = 37.25 + 2.3 * k if spread_over_buckets else np.full(n, 300.25) + 0.003 * k
        events.append([(np.column_stack([x, y, t]), (200_001 + 1_013 * np.arange(n)).astype(np.int64), LABEL)])
    return events


@pytest.mark.parametrize("variant,merge", BUILDS, ids=BUILD_IDS)
@pytest.mark.parametrize("spread_over_buckets", [False, True], ids=["one-bucket", "many-buckets"])
def test_line_blocks_at_their_edges_vs_oracle(orc, spread_over_buckets, variant, merge):
    events = _edge_events(spread_over_buckets)
    clouds, stats, (raw, keep) = _run(variant, merge, 0.277, events)
    assert stats["n_failed"] == 0 and stats["n_inconsistent"] == 0, stats
    points = _assert_clouds_equal_oracle(orc, raw, events, clouds)
    print("edges", spread_over_buckets, variant, merge, "points", points, "retried windows", stats["n_lds_overflow"])
    assert points > 1000


# ---- a wave stops on a full table ----
def _key_estimate(raw, xyt):
    """scatter.hip: key_estimate_on_track() of the samples of one track, in its float arithmetic."""
    f = np.float32
    dv = raw.length / (raw.windows_edge - raw.micromegas_edge)
    spread = f((6.0 / 4.9e-3) * (6.0 / 4.9e-3) * 2.0 * raw.diffusion * dv / raw.efield)
    est = []
    for k, (x, y, t) in enumerate(xyt):
        r = f(1.0) + np.sqrt(f(spread * f(int(min(t, 511.0)))), dtype=f)
        e = f(r * r)
        if k > 0 and int(xyt[k - 1][2]) == int(t):
            dx, dy = f(x - xyt[k - 1][0]), f(y - xyt[k - 1][1])
            e = min(e, f(r * f(np.sqrt(f(dx * dx + dy * dy), dtype=f) * f(1.0 / 4.9e-3)) + f(1.0)))
        est.append(int(min(f(e + f(0.5)), f(100.0))))
    return np.array(est)


def _overfull_event(raw, slots):
    """One track whose samples sit 24 mm apart on a grid over the small pads around the beam, about 44 per time bucket,
    in as many buckets (downwards from 500) as keep the ESTIMATED keys of the event just within 1.2 x the aimed-at
    half table: select_window() then takes the whole event as its first window (it stretches a budget by 25 % for an
    event's remainder).  On the small pads a sample lights twice the pads the estimate assumes (4.9 mm pitch), so
    that window holds more keys than the table has slots (6 723 for 6 144, 9 018 for 8 192, 13 588 for 12 288)."""
    g = np.arange(-84.0, 85.0, 24.0)
    gx, gy = np.meshgrid(g, g, indexing="ij")
    inside = gx ** 2 + gy ** 2 < 92.0 ** 2
    xy = np.column_stack([gx[inside], gy[inside]]) * 1e-3 + np.array([0.4e-3, 0.7e-3])
    per_bucket = len(xy)
    n_max = 12 * per_bucket
    k = np.arange(n_max)
    xyt = np.column_stack([xy[k % per_bucket], 500.25 - (k // per_bucket)])
    est = np.cumsum(_key_estimate(raw, xyt))
    n = int(np.searchsorted(est, 1.2 * (slots // 2), side="right"))
    assert per_bucket < n < n_max, (per_bucket, n, n_max)
    return [(xyt[:n], np.full(n, 3_000_001, dtype=np.int64), LABEL)], int(est[n - 1])


@pytest.mark.parametrize("variant,merge", BUILDS, ids=BUILD_IDS)
def test_window_that_overflows_the_table_is_retried_vs_oracle(orc, variant, merge):
    """More distinct pads in a few time buckets than the table holds, none of the buckets too large by itself: the
    waves stop on the full table, the window is done again in smaller ones, nothing goes to lone_bucket_kernel and
    nothing is lost."""
    slots = TABLE_SLOTS[variant]
    cfg, raw, keep = _configure_cpu()
    ev, estimated = _overfull_event(raw, slots)
    tbpad, charge, labels = _oracle_dict(orc, raw, ev)
    per_bucket = np.bincount(tbpad[:, 0])
    print("overfull", variant, merge, "samples", len(ev[0][0]), "estimated keys", estimated, "keys", len(tbpad),
          "slots", slots, "largest bucket", per_bucket.max())
    # the premise, from the oracle alone: the first window cannot fit, every single bucket fits easily
    assert estimated <= 1.2 * (slots // 2) and len(tbpad) > slots and per_bucket.max() < slots // 2
    other = [(np.array([[0.05, 0.04, 250.5]]), np.array([3_000_001], dtype=np.int64), LABEL)]  # an ordinary event beside it
    events = [other, ev, other]
    clouds, stats, (raw_dev, keep_dev) = _run(variant, merge, 0.277, events)
    assert stats["n_failed"] == 0 and stats["n_inconsistent"] == 0 and stats["n_lone_buckets"] == 0, stats
    assert stats["n_lds_overflow"] > 0, stats
    _assert_clouds_equal_oracle(orc, raw_dev, events, clouds)
    print("retried windows", stats["n_lds_overflow"])


def _configure_cpu():
    """The oracle's descriptor of the default detector without a device (as _configure() builds it)."""
    from attpc_engine_amd import GasTarget, nuclear_map, workloads
    from attpc_engine_amd.detector.luts import build_det_desc

    gas = GasTarget([(1, 2, 2)], 300.0, nuclear_map)
    cfg = workloads.detector_config(gas, diffusion=0.277)
    raw, keep = build_det_desc(cfg, [nuclear_map.get_data(1, 1)], fold_beam=False)
    return cfg, raw, keep
