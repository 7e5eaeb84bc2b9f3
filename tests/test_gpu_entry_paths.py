"""What the scatter kernel does once per entry and once per 64 mesh lines, through attpc_det_scatter against the oracle, in
the five builds of tests/test_gpu_rows_step.py:

* the nucleus of an entry, found once in the histogram pass and carried to the staging in the spare bits of the sorted
  entry list: 8 nuclei, an empty track in the middle of the layout, tracks of a single sample (no predecessor);
* the sort limit: the last sorted event (2 048 entries) and the first unsorted one (2 049);
* the look-up table offsets formed from the packed 16-bit index pairs: mesh lines on the first and the last line of the
  table and off it, in both coordinates;
* the run count of 64 mesh lines read off the queue's address chain: one block that fills the wave's queue exactly
  (256 runs) and one with a run more, which goes to the table in passes.

Needs a real MI355X: ``-m gpu``.

Tolerances (as in tests/test_gpu_rows_step.py): keys, labels, zero-charge inserts and the jittered
time bucket exact, charges within 2 electrons (numpy's exp in the oracle's pdf against the kernel's constant weight
table)."""

import numpy as np
import pytest

from attpc_engine_amd import _abi
from tests.test_gpu_rows_step import BUILD_IDS, BUILDS, _assert_clouds_equal_oracle, _configure_cpu, _oracle_dict, _run
from tests.test_gpu_scatter_fixtures import _configure

pytestmark = pytest.mark.gpu

LABELS = [2, 3, 5, 7, 8, 10, 12, 13]  # rows of the eight simulated nuclei (`indices`), in position order
WAVE_QUEUE = 256   # scatter.hip: queued runs per wave and 64 mesh lines
SORT_CAP = 2048    # scatter.hip: events with at most this many entries are sorted by time bucket
MESH = 10


@pytest.fixture(scope="module")
def orc():
    from oracle import pyoracle
    return pyoracle


@pytest.fixture(scope="module")
def cpu_det():
    cfg, raw, keep = _configure_cpu()
    return raw, keep  # (keep holds the arrays the descriptor points to)


def _track(x0, y0, t0, n, dx=0.9e-3, dy=0.4e-3, dt=0.37, electrons=200_001):
    k = np.arange(n, dtype=np.float64)
    return np.column_stack([x0 + dx * k, y0 + dy * k, t0 + dt * k]), (electrons + 1_013 * np.arange(n)).astype(np.int64)


def _event(tracks):
    """tracks: one (xyt, electrons) per position of LABELS (None: no sample)."""
    none = (np.zeros((0, 3)), np.zeros(0, dtype=np.int64))
    return [(*(t if t is not None else none), lab) for t, lab in zip(tracks, LABELS)]


# ---- the nucleus rides from the histogram pass to the staging ----
def _nucleus_events():
    """All tracks leave one vertex (their first samples share pads and time buckets: the label of such a key is the
    LAST position in LABELS that touched it), several samples per time bucket (each has a predecessor in its bucket)."""
    v = (0.0312, -0.0177, 120.3)
    fan = [(np.cos(a), np.sin(a)) for a in np.linspace(0.2, 5.9, 8)]

    def tr(k, n):
        # (a track of a single sample starts 15 mm out, on pads of its own: at the vertex a later nucleus would take its label)
        out = 15.0e-3 if n == 1 else 0.0
        return _track(v[0] + out * fan[k][0], v[1] + out * fan[k][1], v[2], n, dx=0.8e-3 * fan[k][0], dy=0.8e-3 * fan[k][1],
                      dt=0.31 + 0.02 * k)

    first = _event([tr(0, 40), tr(1, 23), tr(2, 31), None, tr(4, 17), tr(5, 1), tr(6, 29), tr(7, 35)])
    # another split of the layout: the first track empty, two empty neighbours, the last nucleus a single sample
    second = _event([None, tr(1, 50), tr(2, 1), tr(3, 9), None, None, tr(6, 64), tr(7, 1)])
    return [first, second]


@pytest.mark.parametrize("variant,merge", BUILDS, ids=BUILD_IDS)
def test_eight_nuclei_with_empty_and_single_sample_tracks_vs_oracle(orc, variant, merge):
    events = _nucleus_events()
    # the premise: position 7 present, an empty track between two others, single-sample tracks
    counts = [[len(xyt) for xyt, _, _ in ev] for ev in events]
    assert counts[0][7] > 1 and counts[0][3] == 0 and counts[0][2] > 0 and counts[0][4] > 0 and counts[0][5] == 1
    assert counts[1][0] == 0 and counts[1][7] == 1 and counts[1][2] == 1
    clouds, stats, (raw, keep) = _run(variant, merge, 0.277, events)
    assert stats["n_failed"] == 0 and stats["n_inconsistent"] == 0, stats
    points = _assert_clouds_equal_oracle(orc, raw, events, clouds)
    labels = [sorted(set(lab.tolist())) for _, lab in clouds]
    print("nuclei", variant, merge, "points", points, "labels", labels)
    # every nucleus with samples labels some point of its own, the last position among them
    assert labels == [[lab for lab, n in zip(LABELS, c) if n] for c in counts]
    assert points > 1000


# ---- the sort limit ----
def _short_tracks(per_track):
    """Eight short tracks of samples 0.25 mm apart on a 30 mm grid near the micromegas (little diffusion: a few pads per
    sample), a few samples per time bucket."""
    tracks = []
    for k, n in enumerate(per_track):
        gx, gy = (k % 3 - 1) * 30.0e-3 + 0.0213, (k // 3 - 1) * 30.0e-3 - 0.0117
        tracks.append(_track(gx, gy, 20.3 + 1.7 * k, n, dx=0.25e-3, dy=0.11e-3, dt=0.09, electrons=90_001))
    return _event(tracks)


@pytest.mark.parametrize("variant,merge", BUILDS, ids=BUILD_IDS)
def test_last_sorted_and_first_unsorted_event_vs_oracle(orc, variant, merge):
    events = [_short_tracks([SORT_CAP // 8] * 8), _short_tracks([SORT_CAP // 8 + 1] + [SORT_CAP // 8] * 7)]
    assert [sum(len(xyt) for xyt, _, _ in ev) for ev in events] == [SORT_CAP, SORT_CAP + 1]
    clouds, stats, (raw, keep) = _run(variant, merge, 0.277, events)
    assert stats["n_failed"] == 0 and stats["n_inconsistent"] == 0, stats
    points = _assert_clouds_equal_oracle(orc, raw, events, clouds)
    print("sort limit", variant, merge, "points per event", [len(p) for p, _ in clouds], "retried windows", stats["n_lds_overflow"])
    assert points > 2000 and sorted(set(clouds[0][1].tolist())) == LABELS


# ---- LUT offsets from 16-bit halves ----
def _sigma(raw, t):
    """scatter.hip stage_entry(): sigma_t = sqrt(2 D dv t / E), left to right."""
    dv = raw.length / (raw.windows_edge - raw.micromegas_edge)
    return np.sqrt(2.0 * raw.diffusion * dv * t / raw.efield)


def _line_indices(raw, c, t):
    """LUT indices of the ten mesh lines around coordinate c [m] (stage_entry(): linspace(c - 3 sigma, c + 3 sigma, 10),
    whole-mm floor, lut_n = off the table) and the lines' distance from a whole mm."""
    s = _sigma(raw, t)
    lo, hi = c + (-3.0 * s), c + 3.0 * s
    step = (hi - lo) / 9.0
    mm = np.array([lo + i * step for i in range(9)] + [hi]) * 1000.0
    idx = np.floor(mm).astype(np.int64) - raw.lut_lo
    idx[(idx < 0) | (idx >= raw.lut_n)] = raw.lut_n
    return idx, float(np.abs(mm - np.round(mm)).min())


def _edge_event(raw):
    """Samples 0.5 mm apart across the first and the last line of the look-up table, at the middle of each side and at
    the four corners."""
    first, last = raw.lut_lo * 1e-3, (raw.lut_lo + raw.lut_n) * 1e-3  # [first, last): the table
    steps = np.arange(-10.0, 10.01, 0.5) * 1e-3 + 0.13e-3
    spots = [(first, 0.0, 1, 0), (last, 0.0, 1, 0), (0.0, first, 0, 1), (0.0, last, 0, 1),
             (first, first, 1, 1), (first, last, 1, -1), (last, first, 1, -1), (last, last, 1, 1)]
    xyt = np.array([(x + sx * d, y + sy * d, 300.4) for x, y, sx, sy in spots for d in steps])
    return [(xyt, (200_001 + 1_013 * np.arange(len(xyt))).astype(np.int64), LABELS[0])]


@pytest.mark.parametrize("variant,merge", BUILDS, ids=BUILD_IDS)
def test_mesh_lines_on_the_edges_of_the_lookup_table_vs_oracle(orc, cpu_det, variant, merge):
    raw_cpu, _ = cpu_det
    ev = _edge_event(raw_cpu)
    n = raw_cpu.lut_n
    # the premise, from the descriptor alone: in both coordinates lines take index 0, index lut_n - 1 and "off the
    # table"; a line of x off the table (the largest index x byte pitch) meets a line of y on the last line and off it
    seen = {"x": set(), "y": set()}
    largest = False
    for x, y, t in ev[0][0]:
        ix, _ = _line_indices(raw_cpu, x, t)
        iy, _ = _line_indices(raw_cpu, y, t)
        seen["x"].update(ix.tolist())
        seen["y"].update(iy.tolist())
        largest = largest or (n in ix and (n - 1 in iy or n in iy))
    assert {0, n - 1, n} <= seen["x"] and {0, n - 1, n} <= seen["y"] and largest, (n, sorted(seen["x"])[:3], sorted(seen["y"])[:3])
    assert 2 * (n + 1) < 65536 and n * 2 * (n + 1) + 2 * n < 2 ** 32  # both factors 16 bit, the offset 32 bit
    clouds, stats, (raw, keep) = _run(variant, merge, 0.277, [ev])
    assert stats["n_failed"] == 0 and stats["n_inconsistent"] == 0, stats
    points = _assert_clouds_equal_oracle(orc, raw, [ev], clouds)
    print("lut edges", variant, merge, "lut_n", n, "points", points)
    assert raw.lut_n == n and raw.lut_lo == raw_cpu.lut_lo and points > 0


@pytest.mark.parametrize("lut_n", [32001, 32766, 32767])
def test_configure_refuses_a_table_whose_offsets_pass_16_bit_factors(lut_n):
    """attpc_det_configure() refuses every table of more than 32 000 lines before it reads one cell: the first size past
    the limit, the last whose byte pitch 2 (lut_n + 1) would still be a 16-bit factor, and the first whose pitch is not
    (65 536).  (The refusal is host code, but it needs a context and a context needs a device; the limit itself is
    pinned without one in tests/test_lut_limit_cpu.py.  A table of exactly 32 000 lines would take 2 GB to try.)"""
    ctx = _abi.Context(0)
    try:
        cfg, raw, keep = _configure(ctx, 0.277)
        raw.lut_n = lut_n
        ctx.forget("det")  # configured through the C ABI directly: the shim's cache no longer describes the device
        assert ctx.lib.attpc_det_configure(ctx.handle, raw) == _abi.E_INVALID
        with pytest.raises(ValueError, match="look-up table larger"):
            ctx.check(ctx.lib.attpc_det_configure(ctx.handle, raw), "attpc_det_configure")
    finally:
        ctx.close()


# ---- run totals at the queue's edge ----
def _runs_of_block(raw, lut, xyt):
    """Runs the first 64 mesh lines of an event's entries queue (rows_round(): a lane is a line of constant y and steps
    through the ten lines of x; a run is a stretch of equal pads, pad >= 0), how close a line comes to a whole mm, and the
    pads under those lines."""
    runs, margin, lines, lit = 0, 1.0, 0, set()
    for x, y, t in xyt:
        ix, mx = _line_indices(raw, x, t)
        iy, my = _line_indices(raw, y, t)
        margin = min(margin, mx, my)
        for i in range(MESH):
            if lines == 64:
                return runs, margin, lit
            pads = lut[ix, iy[i]]
            lit.update(int(p) for p in pads if p >= 0)
            ends = np.append(pads[1:] != pads[:-1], True)
            runs += int((ends & (pads >= 0)).sum())
            lines += 1
    return runs, margin, lit


def _grid_event(n, shift, tb):
    """n samples 4 mm apart beside the beam region, all in one late time bucket (one window, one staging round), every
    sample moved by `shift`."""
    k = np.arange(n, dtype=np.float64)
    x, y = 0.0213 + shift + 4.0e-3 * (k % 2), -0.0487 + 0.37 * shift + 4.0e-3 * (k // 2)
    return [(np.column_stack([x, y, tb + 1.0e-4 * k]), (200_001 + 1_013 * np.arange(n)).astype(np.int64), LABELS[0])]


@pytest.fixture(scope="module")
def queue_edge_events(cpu_det):
    """One event whose 40 mesh lines (4 samples, wave 0's only block) queue exactly WAVE_QUEUE runs and one with
    WAVE_QUEUE + 1, found by sweeping the samples' position over the pads with the look-up table on the CPU."""
    raw, _ = cpu_det
    n = raw.lut_n
    lut = np.full((n + 1, n + 1), -1, dtype=np.int64)  # [x][y], index lut_n = off the table
    lut[:n, :n] = np.ctypeslib.as_array(raw.pad_lut, shape=(n * n,)).reshape(n, n)
    found = {}
    for tb in (500.25, 470.25, 440.25, 410.25):
        for s in range(400):
            ev = _grid_event(4, 0.05e-3 * s, tb)
            runs, margin, _ = _runs_of_block(raw, lut, ev[0][0])
            if runs in (WAVE_QUEUE, WAVE_QUEUE + 1) and runs not in found and margin > 1e-6:
                found[runs] = ev
        if len(found) == 2:
            break
    assert sorted(found) == [WAVE_QUEUE, WAVE_QUEUE + 1], sorted(found)
    return [found[WAVE_QUEUE], found[WAVE_QUEUE + 1]], lut


@pytest.mark.parametrize("variant,merge", BUILDS, ids=BUILD_IDS)
def test_block_that_fills_the_queue_and_one_run_more_vs_oracle(orc, cpu_det, queue_edge_events, variant, merge):
    raw_cpu, _ = cpu_det
    events, lut = queue_edge_events
    # the premise, from the look-up table alone: 40 lines, 256 and 257 runs, one time bucket each
    assert [_runs_of_block(raw_cpu, lut, ev[0][0])[0] for ev in events] == [WAVE_QUEUE, WAVE_QUEUE + 1]
    for ev in events:
        assert len(ev[0][0]) * MESH <= 64 and len(set(np.floor(ev[0][0][:, 2]).tolist())) == 1
    clouds, stats, (raw, keep) = _run(variant, merge, 0.277, events)
    assert stats["n_failed"] == 0 and stats["n_inconsistent"] == 0 and stats["n_lds_overflow"] == 0, stats
    points = _assert_clouds_equal_oracle(orc, raw, events, clouds)
    for ev, (pts, _), want in zip(events, clouds, (WAVE_QUEUE, WAVE_QUEUE + 1)):
        tbpad, _, _ = _oracle_dict(orc, raw, ev)
        assert len(pts) == int(((tbpad[:, 0] >= 0) & (tbpad[:, 0] < 512) & (tbpad[:, 1] >= 0)).sum())
        # the run count is this file's restatement of the staging; what ties it to the kernel: the pads under the
        # restated mesh lines are exactly the pads the device lit (one time bucket: a key is a pad), and every one of them
        # ends at least one run -- so the lines and look-ups the runs were counted on are the kernel's
        runs, _, lit = _runs_of_block(raw_cpu, lut, ev[0][0])
        assert runs == want and lit == set(pts[:, 0].astype(np.int64).tolist()) and len(lit) <= runs
    print("queue edge", variant, merge, "keys per event", [len(p) for p, _ in clouds], "points", points)
