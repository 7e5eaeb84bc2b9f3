"""The device at the layout limits of the C ABI: 8 kinematic steps (18 rows), 8 simulated nuclei per event, labels up
to 17 and 13 stopping-power tables in LDS, against the CPU oracle.  The workloads are the long decay chains of
tests/helpers.py: ``chain7`` (16 rows, the reference's default indices, a neutron at isim 2) and ``chain8`` (18 rows,
indices [17, 3, 16, 2, 9, 12, 5, 14]: non-ascending, so the last writer of a key is the nucleus with the largest
POSITION isim, not the largest row).  What they reach that no other workload does: isim 4..7 in the scatter's table
word and staging meta, the lone kernel's 8-bit nucleus masks above the low nibble, bits 3 and 4 of the records' 5-bit
label field (16 and 17 set the sign bit of the 8-byte record), the track kernel's table offset sp * ATTPC_DEDX_NODES
for sp >= 2, the kinematics rows and RNG slots of steps 3..7 and the Fano domains of rows 8..17.

Tolerances are those of test_gpu_parity.py: keys, labels, jittered time buckets exact, charges
within 2 electrons.  Needs a real MI355X: ``-m gpu``."""
import ctypes as C
import os

import numpy as np
import pytest

from attpc_engine_amd import _abi, nuclear_map
from attpc_engine_amd.detector.luts import build_det_desc, build_layout
from attpc_engine_amd.detector.simulator import simulate_batch
from tests.helpers import CHAIN8_INDICES, LONG_CHAINS, Inputs, chain7, chain8, compare_clouds, overlap_counts, sort_cloud

pytestmark = pytest.mark.gpu

CHAIN_LABELS = {"chain7": {14, 15}, "chain8": {16, 17}}
THREADS = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 8


@pytest.fixture(scope="module")
def ctx():
    return _abi.Context(0)


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


def _fresh(**options):
    ctx = _abi.Context(0)
    for key, value in options.items():
        ctx.set_option(key, value)
    return ctx


def _engine(inp, ctx, **kw):
    from attpc_engine_amd.engine import Engine
    return Engine(inp.pipeline, inp.config, inp.indices, context=ctx, **kw)


def _charged_positions(inp):
    return [isim for isim, row in enumerate(inp.indices) if inp.layout.species_of_row[row] >= 0]


# ---------------------------------------------------------------- kinematics ----------------------------------------
@pytest.mark.parametrize("name", ["chain7", "chain8"])
def test_kin_run_vs_oracle(ctx, orc, name):
    """Every row of p4 (up to 18), the vertex, status and attempts of the rejection loop over 8 steps."""
    inp = Inputs(LONG_CHAINS[name])
    inp.pipeline._ctx = ctx
    n = 3000
    vertex, p4, status, attempts = inp.pipeline.run_many(n, first_event=17, seed=11, return_status=True)
    ov, op4, ostatus, oatt = orc.kin_batch(inp.kin, 11, 17, n, threads=8)
    assert p4.shape == (n, inp.n_rows, 4)
    np.testing.assert_array_equal(status, ostatus)
    np.testing.assert_array_equal(attempts, oatt)
    np.testing.assert_allclose(vertex, ov, rtol=0, atol=1e-12)
    # 1e-9 MeV is stated for energies up to 1.5e4 MeV; here the beam row carries 2.3e4 MeV and
    # seven boosts follow one another.  A decay close to its threshold (momentum of a few MeV/c in the parent's frame,
    # the square root of a difference of squared masses of ~5e8 MeV^2) magnifies last-bit differences of device and
    # host arithmetic: at most 2e-9 MeV, on fewer than 1 component in 10^4
    diff = np.abs(p4 - op4)
    assert diff.max() <= 2e-9, diff.max()
    assert (diff > 1e-9).sum() <= p4.size // 10_000, np.argwhere(diff > 1e-9)
    assert (status == 0).all()
    if name == "chain7":
        assert (attempts > 1).sum() > 10  # events that needed a second attempt: the loop over 7 steps ran again
    over = np.argwhere(diff > 1e-9)
    print(name, "events with more than one attempt", int((attempts > 1).sum()), "max |dp4|", diff.max(),
          "components above 1e-9 MeV (event, row, component)", over.tolist())


# ---------------------------------------------------------------- tracks --------------------------------------------
def _device_tracks(ctx, det, layout, p4, vertex, seed, first):
    ctx.forget("det")  # configured through the C ABI directly: the shim's cache no longer describes the device
    ctx.check(ctx.lib.attpc_det_configure(ctx.handle, det), "det_configure")
    nt = len(p4) * layout.n_sim
    samples = np.zeros((nt, _abi.TIME_SAMPLES, 4))
    counts = np.empty(nt, dtype=np.int32)
    steps = np.empty(nt, dtype=np.int32)
    ctx.check(ctx.lib.attpc_det_tracks(ctx.handle, seed, first, len(p4), layout, _abi.dptr(np.ascontiguousarray(p4)),
                                       _abi.dptr(np.ascontiguousarray(vertex)), _abi.TIME_SAMPLES, _abi.dptr(samples),
                                       _abi.iptr(counts, _abi.C.c_int32), _abi.iptr(steps, _abi.C.c_int32)), "tracks")
    return samples, counts, steps


def _check_tracks(orc, det_raw, layout, indices, p4, vertex, seed, first, samples, counts, steps):
    """Every nucleus of every event (the neutron too: no samples) against orc.point_cloud_samples; -> samples seen
    per position isim."""
    per_isim = np.zeros(layout.n_sim, dtype=np.int64)
    for e in range(len(p4)):
        for isim, row in enumerate(indices):
            t = e * layout.n_sim + isim
            sp = layout.species_of_row[row]
            if sp < 0:
                assert counts[t] == 0 and steps[t] == 0, (e, row, counts[t], steps[t])
                continue
            ref, ref_rows = orc.point_cloud_samples(det_raw, sp, p4[e, row], vertex[e], seed, first + e, row)
            assert steps[t] == ref_rows and counts[t] == len(ref), (e, row, steps[t], ref_rows, counts[t], len(ref))
            mine = samples[t, : counts[t]]
            np.testing.assert_allclose(mine[:, :2], ref[:, :2], rtol=0, atol=1e-9)
            np.testing.assert_allclose(mine[:, 2], ref[:, 2], rtol=0, atol=1e-7)
            np.testing.assert_array_equal(mine[:, 3], ref[:, 3])  # Fano domain 1 + row, rows up to 17
            per_isim[isim] += len(ref)
    return per_isim


@pytest.mark.parametrize("species_major", [1, 0], ids=["species_major", "event_major"])
@pytest.mark.parametrize("name", ["chain7", "chain8"])
def test_tracks_vs_oracle(orc, name, species_major):
    """All 8 positions of attpc_det_tracks, with the tracks handed out nucleus by nucleus (sorted by Z, then mass) and
    event by event."""
    inp = Inputs(LONG_CHAINS[name])
    seed, first, n = 21, 1000, 6
    vertex, p4, _, _ = orc.kin_batch(inp.kin, seed, first, n, threads=8)
    ctx = _fresh(track_species_major=species_major)
    try:
        samples, counts, steps = _device_tracks(ctx, inp.det, inp.layout, p4, vertex, seed, first)
    finally:
        ctx.close()
    per_isim = _check_tracks(orc, inp.det_raw, inp.layout, inp.indices, p4, vertex, seed, first, samples, counts, steps)
    assert all(per_isim[i] > 0 for i in _charged_positions(inp)), per_isim
    print(name, "track samples per isim", per_isim.tolist())


# ---------------------------------------------------------------- clouds --------------------------------------------
# (scatter_variant, scatter_merge, compact_transfer): 0 = the context's own choice of build; 1 / 2 / 3 = the two-
# workgroup, one-workgroup and u64-sum builds; merge 1 = consecutive samples add up per pixel first; compact 2 / 1 / 0 =
# 8-byte / 16-byte transfer records / plain rows
CLOUD_SETTINGS = [(0, 0, 2), (1, 0, 2), (2, 0, 2), (3, 0, 2), (2, 1, 2), (1, 1, 2), (0, 0, 1), (0, 0, 0)]
CLOUD_IDS = [f"variant{v}_merge{m}_compact{c}" for v, m, c in CLOUD_SETTINGS]


@pytest.fixture(scope="module")
def chain_refs(orc):
    """Per chain: inputs, kinematics of 12 events and the oracle's per-event clouds (attpc_det_run's comparison) and
    its fused batch of 16 events (attpc_sim_run's)."""
    refs = {}
    for name, builder in LONG_CHAINS.items():
        inp = Inputs(builder)
        seed, first, n = 77, 5, 12  # the events of test_layout_limits_cpu.py's overlap counts
        vertex, p4, _, _ = orc.kin_batch(inp.kin, seed, first, n, threads=8)
        clouds = [orc.simulate(inp.det_raw, inp.layout, seed, first + e, p4[e], vertex[e], capacity=1 << 20)[:2]
                  for e in range(n)]
        fused = orc.sim_batch(inp.kin, inp.det_raw, inp.layout, seed=123, first=40, n=16, capacity=1 << 22,
                              threads=THREADS)
        refs[name] = (inp, seed, first, p4, vertex, clouds, fused)
    return refs


def test_long_chain_clouds_reach_the_limits(orc, chain_refs):
    """What the cloud comparisons below stand on (oracle side, the events they use): labels 14..17 occur, every charged
    position isim wins keys, and keys lit by three and more nuclei occur."""
    for name, (inp, seed, first, p4, vertex, clouds, fused) in chain_refs.items():
        wins, shared3, labels = overlap_counts(orc, inp, p4, vertex, seed, first)
        print(name, "points won per isim", wins.tolist(), "keys lit by >= 3 nuclei", shared3, "labels", sorted(labels))
        assert all(wins[i] > 0 for i in _charged_positions(inp)) and shared3 > 20
        assert CHAIN_LABELS[name] <= labels


@pytest.mark.parametrize("variant,merge,compact", CLOUD_SETTINGS, ids=CLOUD_IDS)
@pytest.mark.parametrize("name", ["chain7", "chain8"])
def test_clouds_vs_oracle(chain_refs, name, variant, merge, compact):
    """attpc_det_run (12 events) and the fused attpc_sim_run (16 events, CSR and statistics) against the oracle, for
    every scatter build, the merge variant and every transfer format."""
    inp, seed, first, p4, vertex, clouds, fused = chain_refs[name]
    ctx = _fresh(scatter_variant=variant, scatter_merge=merge, compact_transfer=compact)
    try:
        offsets, points, labels, stats = simulate_batch(p4, vertex, inp.z, inp.a, inp.config, seed, inp.indices,
                                                        first_event=first, ctx=ctx)
        res = _engine(inp, ctx).run(16, seed=123, first_event=40, fetch=True)
    finally:
        ctx.close()
    assert stats["n_failed"] == 0 and stats["n_inconsistent"] == 0
    worst = 0.0
    for e in range(len(p4)):
        a = sort_cloud(points[offsets[e]:offsets[e + 1]], labels[offsets[e]:offsets[e + 1]])
        worst = max(worst, compare_clouds(*a, *sort_cloud(*clouds[e])))
    wins = [int((labels == row).sum()) for row in inp.indices]
    assert all(wins[i] > 0 for i in _charged_positions(inp)), wins
    assert CHAIN_LABELS[name] <= set(labels.tolist())
    # fused
    np.testing.assert_allclose(res["p4"], fused["p4"], rtol=0, atol=1e-9)
    np.testing.assert_array_equal(res["offsets"], fused["offsets"])
    for e in range(16):
        lo, hi = fused["offsets"][e], fused["offsets"][e + 1]
        compare_clouds(*sort_cloud(res["points"][lo:hi], res["labels"][lo:hi]),
                       *sort_cloud(fused["points"][lo:hi], fused["labels"][lo:hi]))
    assert CHAIN_LABELS[name] <= set(res["labels"].tolist())
    st = res["stats"]
    assert st["n_points"] == fused["stats"][0] and st["n_track_samples"] == fused["stats"][1]
    assert st["key_checksum"] == fused["stats"][3]
    assert abs(int(st["charge_checksum"]) - int(fused["stats"][2])) <= 2 * max(8, st["n_points"] // 10_000)
    assert st["n_failed"] == 0 and st["n_inconsistent"] == 0
    print(name, (variant, merge, compact), "points", offsets[-1], "+", st["n_points"], "max |dq|", worst, "points won per isim",
          wins, "lone buckets", stats["n_lone_buckets"], st["n_lone_buckets"], "retried windows", stats["n_lds_overflow"],
          st["n_lds_overflow"])


@pytest.mark.parametrize("variant", [1, 3])
def test_lone_bucket_touched_by_high_positions(ctx, orc, variant):
    """A time bucket lighting more pads than the table holds goes through lone_bucket_kernel; here it is lit by all 8
    positions of chain8's layout, most of it by isim 4..7 (bits 4..7 of the lone kernel's per-pad mask), and every pad
    by several of them.  The label is that of the largest isim touching the pad: label_of[max(isim)], which is neither
    max(label) (17 and 16 sit at isim 0 and 2) nor the largest row."""
    from tests.test_gpu_scatter_fixtures import _compare_with_dict, _configure, _plane_filling_event, device_scatter
    cfg, raw, keep = _configure(ctx, 0.277)
    (grid, el, _), = _plane_filling_event(cfg, n_tracks=1)
    el = el[0]
    # (isim -> samples of the grid): isim 4..7 light one quarter of the plane each (by x), isim 5 also every 9th
    # point of the others'; the low positions are spread over the whole plane beneath them
    quarter = np.clip(((grid[:, 0] + 0.27) / 0.135).astype(int), 0, 3)
    parts = [grid[::4], grid[1::6], grid[::3], grid[2::7], grid[quarter == 0],
             np.concatenate([grid[quarter == 1], grid[quarter != 1][::9]]), grid[quarter == 2], grid[quarter == 3]]
    assert max(len(p) for p in parts) <= 10112  # MAX_BLOCKS_PER_TRACK x ARENA_BLK samples per track
    big = [(xyt, np.full(len(xyt), el, dtype=np.int64), lab) for xyt, lab in zip(parts, CHAIN8_INDICES)]
    small = [(xyt[:40] * np.array([1.0, 1.0, 0.5]), q[:40], lab) for xyt, q, lab in big]  # tb 250: an ordinary event
    ctx.set_option("scatter_variant", variant)
    try:
        clouds, stats = device_scatter(ctx, [small, big, small])
    finally:
        ctx.set_option("scatter_variant", 0)
    assert stats["n_failed"] == 0 and stats["n_inconsistent"] == 0
    assert stats["n_lone_buckets"] >= 1
    for e, (ev, (pts, lab)) in enumerate(zip([small, big, small], clouds)):
        keys, charge, labels = orc.transport(raw, ev)
        tb, pad = np.array([orc.unpair(int(k)) for k in keys], dtype=np.int64).T
        _compare_with_dict(pts, lab, tb, pad, charge, labels, 11, e)
    pts, lab = clouds[1]
    won = {int(v): int(c) for v, c in zip(*np.unique(lab, return_counts=True))}
    assert len(pts) > 8192 and all(won.get(CHAIN8_INDICES[i], 0) > 0 for i in (4, 5, 6, 7)), won
    print("variant", variant, "pads lit in the lone bucket:", len(pts), "pads won per label", won,
          "lone buckets:", stats["n_lone_buckets"])


# ---------------------------------------------------------------- Spyral rows and traces ----------------------------
@pytest.mark.parametrize("compact", [2, 0], ids=["record24", "plain"])
def test_fused_spyral_rows(orc, compact):
    """attpc_sim_run_spyral on chain8 (labels 16 and 17 through the 24-byte record's label field, or the plain rows)
    against the cloud path + convert_to_spyral + threshold + z-sort of the device's own cloud."""
    from attpc_engine_amd.detector.response import get_response
    from attpc_engine_amd.detector.writer import convert_to_spyral
    inp = Inputs(chain8)
    ctx = _fresh(compact_transfer=compact)
    try:
        eng = _engine(inp, ctx, chunk_events=5)  # several chunks
        n = 12
        fused = eng.run_spyral(n, seed=77, first_event=3)
        cloud = eng.run(n, seed=77, first_event=3, fetch=True)
        cfg = inp.config
        resp = get_response(cfg)
        thr = cfg.elec_params.adc_threshold
        for e in range(n):
            lo, hi = cloud["offsets"][e], cloud["offsets"][e + 1]
            pts, lab = np.ascontiguousarray(cloud["points"][lo:hi]), cloud["labels"][lo:hi]
            rows = convert_to_spyral(pts, 560, 10, 1.0, resp, cfg.pad_centers, cfg.pad_sizes, ctx=ctx)
            keep = rows[:, 3] > thr
            flo, fhi = fused["offsets"][e], fused["offsets"][e + 1]
            got, got_lab = fused["rows"][flo:fhi], fused["labels"][flo:fhi]
            assert len(got) == keep.sum() and fused["event_points"][e] == hi - lo
            want, want_lab = rows[keep], lab[keep]
            zorder = np.argsort(want[:, 2], kind="stable")
            assert (np.diff(got[:, 2]) >= 0).all()
            np.testing.assert_array_equal(got[:, 2], want[zorder][:, 2])
            np.testing.assert_array_equal(got[:, [5, 6]], want[zorder][:, [5, 6]])
            np.testing.assert_array_equal(got_lab, want_lab[zorder])
            o1, o2 = np.lexsort((got[:, 6], got[:, 5])), np.lexsort((want[:, 6], want[:, 5]))
            np.testing.assert_allclose(got[o1], want[o2], rtol=1e-12, atol=0)
    finally:
        ctx.close()
    assert {16, 17} <= set(fused["labels"].tolist())
    print("chain8 Spyral rows", fused["offsets"][-1], "of", cloud["offsets"][-1], "cloud points; labels",
          sorted(set(fused["labels"].tolist())))


def test_traces_vs_restatement_of_own_cloud(ctx):
    """run_traces on chain8 equals tests/trace_reference.py applied to the device's own cloud; the label of a trace
    (that of its largest-charge row) reaches 16 and 17."""
    from attpc_engine_amd.detector.response import get_response
    from tests.trace_reference import traces as reference_traces
    inp = Inputs(chain8)
    eng = _engine(inp, ctx)
    resp = get_response(inp.config)
    thr = float(inp.config.elec_params.adc_threshold)
    eng.configure_traces(inp.config, resp, thr, 0)
    n, seed, first = 8, 21, 7
    cloud = eng.run(n, seed=seed, first_event=first, fetch=True)
    res = eng.run_traces(n, seed=seed, first_event=first)
    got = (res["offsets"], res["pads"], res["samples"], res["labels"], res["trace"])
    ref = reference_traces(cloud["offsets"], cloud["points"], cloud["labels"], resp, thr, 0, first_event=first)
    for a, b, what in zip(got[:4], ref[:4], ("offsets", "pads", "samples", "labels")):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=what)
    assert got[4] == ref[4], (got[4], ref[4])
    assert {16, 17} <= set(np.asarray(res["labels"]).tolist())
    print("chain8 trace rows", got[4]["n_rows"], "labels", sorted(set(np.asarray(res["labels"]).tolist())))


# ---------------------------------------------------------------- 13 stopping-power tables -------------------------
# chain8's 7 species at table indices 6..12 behind 6 other nuclei: 13 x 1409 doubles = 146 536 bytes of dynamic LDS
OTHER_SPECIES = [(1, 3), (2, 3), (3, 6), (5, 10), (6, 12), (8, 16)]


def _det_run(ctx, det, layout, p4, vertex, seed, first):
    ctx.forget("det")
    ctx.check(ctx.lib.attpc_det_configure(ctx.handle, det), "det_configure")
    n = len(p4)
    capacity = 1 << 20
    offsets = np.zeros(n + 1, dtype=np.int64)
    points = np.empty((capacity, 3))
    labels = np.empty(capacity, dtype=np.int64)
    out = _abi.CloudOut(capacity, _abi.iptr(offsets, C.c_int64), _abi.dptr(points), _abi.iptr(labels, C.c_int64))
    stats = _abi.RunStats()
    ctx.check(ctx.lib.attpc_det_run(ctx.handle, seed, first, n, layout, _abi.dptr(np.ascontiguousarray(p4)),
                                    _abi.dptr(np.ascontiguousarray(vertex)), out, stats), "attpc_det_run")
    total = int(offsets[n])
    return offsets, points[:total], labels[:total], stats.as_dict()


def test_thirteen_stopping_power_tables(ctx, orc):
    """13 species, the most attpc_det_configure accepts (their tables fill 146.5 KB of the track kernel's dynamic
    LDS): tracks and clouds equal the oracle's on the same descriptor; 14 are refused with the LDS message, and the
    context works afterwards."""
    inp = Inputs(chain8)
    species = OTHER_SPECIES + inp.species
    assert len(species) == 13 and len(set(species)) == 13
    nuclei = [nuclear_map.get_data(z, a) for z, a in species]
    det, keep = build_det_desc(inp.config, nuclei, 1, fold_beam=True)
    det_raw, keep_raw = build_det_desc(inp.config, nuclei, 1, fold_beam=False)
    layout = build_layout(inp.z, inp.a, inp.indices, species)
    assert sorted({layout.species_of_row[row] for row in inp.indices}) == list(range(6, 13))
    seed, first, n = 31, 50, 6
    vertex, p4, _, _ = orc.kin_batch(inp.kin, seed, first, n, threads=8)
    samples, counts, steps = _device_tracks(ctx, det, layout, p4, vertex, seed, first)
    per_isim = _check_tracks(orc, det_raw, layout, inp.indices, p4, vertex, seed, first, samples, counts, steps)
    assert (per_isim > 0).all(), per_isim
    offsets, points, labels, stats = _det_run(ctx, det, layout, p4, vertex, seed, first)
    assert stats["n_failed"] == 0 and stats["n_inconsistent"] == 0
    refs = [orc.simulate(det_raw, layout, seed, first + e, p4[e], vertex[e], capacity=1 << 20)[:2] for e in range(n)]
    for e in range(n):
        compare_clouds(*sort_cloud(points[offsets[e]:offsets[e + 1]], labels[offsets[e]:offsets[e + 1]]),
                       *sort_cloud(*refs[e]))
    assert offsets[-1] > 10_000
    # 14 tables do not fit: refused, and the context keeps the 13-table configuration it had
    det14, keep14 = build_det_desc(inp.config, nuclei + [nuclear_map.get_data(7, 14)], 1, fold_beam=True)
    ctx.forget("det")
    rc = ctx.lib.attpc_det_configure(ctx.handle, det14)
    assert rc == _abi.E_INVALID and b"do not fit LDS" in ctx.lib.attpc_last_error(ctx.handle)
    again = _det_run(ctx, det, layout, p4, vertex, seed, first)
    np.testing.assert_array_equal(again[0], offsets)
    for e in range(n):
        compare_clouds(*sort_cloud(again[1][offsets[e]:offsets[e + 1]], again[2][offsets[e]:offsets[e + 1]]),
                       *sort_cloud(*refs[e]))
    print("13 species: track samples per isim", per_isim.tolist(), "cloud points", int(offsets[-1]), "(launch ran)",
          "14 species:", ctx.lib.attpc_last_error(ctx.handle).decode())


# ---------------------------------------------------------------- bulk ----------------------------------------------
def test_bulk_checksums_vs_oracle(ctx, orc):
    """chain7, 2 000 events through attpc_sim_run: point and sample counts and the key checksum equal the oracle's, the
    charge checksum within the bound of test_gpu_parity.py::test_bulk_checksums_vs_oracle."""
    inp = Inputs(chain7)
    n = 2000
    st = _engine(inp, ctx).run(n, seed=2024, first_event=100)["stats"]
    ref = orc.sim_batch(inp.kin, inp.det_raw, inp.layout, seed=2024, first=100, n=n, threads=THREADS)["stats"]
    assert st["n_points"] == ref[0] and st["n_track_samples"] == ref[1]
    assert st["key_checksum"] == ref[3] % (1 << 64)
    diff = (int(st["charge_checksum"]) - int(ref[2] % (1 << 64)) + (1 << 63)) % (1 << 64) - (1 << 63)
    gain = int(inp.config.det_params.mpgd_gain)
    flips = round(diff / gain)
    assert abs(diff - flips * gain) <= 2 * max(8, st["n_points"] // 10_000), (diff, flips)
    assert abs(flips) <= 1 + st["n_track_samples"] // 10_000_000, (diff, flips)
    assert st["n_failed"] == 0 and st["n_inconsistent"] == 0
    print("chain7 events", n, "points", st["n_points"], "charge checksum difference", diff, "lone buckets",
          st["n_lone_buckets"], "retried windows", st["n_lds_overflow"])
