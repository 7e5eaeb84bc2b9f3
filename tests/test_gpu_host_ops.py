"""The operators on host arrays at their own chunk limits, and what they refuse (csrc/abi.hip, csrc/host_args.hpp).

Chunk seams: an operator walks its events in chunks of whole events -- 16 384 rows in ``attpc_trigger_rows``, 2^20 in
``attpc_rows_estimate`` and ``attpc_rows_thin``, 4 Mi in ``attpc_gain_rows``; 16 384 rows in ``attpc_trace_baseline`` and
``attpc_trace_pack`` -- and its result is a pure function of the event, so one call whose events straddle the limit
must equal, bit for bit, the calls on each event alone.  Event sizes L/2, L/2, 1, 0, L + 1: an exact fit, a lone row
with an empty event, one oversize event alone.

Refusals: return code and message of every entry point for offsets[0] = -1, decreasing offsets, rows without their
arrays and a sample outside 0 .. 4095, written out here; every refusal is followed by a good call on the same context.
Needs a real MI355X: ``-m gpu``."""
import ctypes as C

import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.estimate import EstimateSettings, rows_to_estimates
from attpc_engine_amd.detector.thinning import ThinSettings, rows_to_points
from attpc_engine_amd.detector.traces import (GainSettings, TriggerSettings, configure_gain, pack_traces, remove_baseline,
                                              traces_to_trigger)
from attpc_engine_amd.outputs import SummaryArrays
from tests.summary_reference import hand_made_centers

pytestmark = pytest.mark.gpu

INDICES = [2, 5, 3]
I64, I32, I16 = C.c_int64, C.c_int32, C.c_int16


@pytest.fixture(scope="module")
def ctx():
    return _abi.Context(0)


def _offsets(sizes, first=0):
    return np.concatenate([[first], first + np.cumsum(sizes)]).astype(np.int64)


def _seam_sizes(limit):
    return [limit // 2, limit // 2, 1, 0, limit + 1]


def _same_bits(a, b, what):
    """Equal bit for bit (a NaN equals itself), field by field for records."""
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if a.dtype.names:
        for name in a.dtype.names:
            _same_bits(a[name], b[name], f"{what}.{name}")
    else:
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), what


# ---------------------------------------------------------------- chunk seams ----
def test_trigger_rows_across_its_row_limit(ctx):
    rng = np.random.default_rng(101)
    offsets = _offsets(_seam_sizes(16384), first=3)  # (rows in front of the first event: the walk starts at offsets[0])
    rows = int(offsets[-1])
    pads = rng.integers(0, _abi.NUM_PADS, rows, dtype=np.int32)
    samples = rng.integers(0, 4096, (rows, _abi.NUM_TB), dtype=np.int16)
    pedestals = rng.integers(0, 4096, _abi.NUM_PADS).astype(np.int16)
    groups = rng.integers(0, 16, _abi.NUM_PADS).astype(np.uint8)
    trigger = TriggerSettings(2300, window=40, group_multiplicity=3, min_groups=9, groups=groups)
    whole = traces_to_trigger(offsets, pads, samples, trigger, pedestals, ctx)
    alone = np.concatenate([traces_to_trigger(offsets[e:e + 2], pads, samples, trigger, pedestals, ctx) for e in range(5)])
    assert whole["n_rows"].tolist() == np.diff(offsets).tolist()
    _same_bits(whole, alone, "trigger records")


@pytest.fixture(scope="module")
def spyral_rows():
    """Rows [R, 8] and labels of five events around 2^20 rows, shared by the estimate and the thinning case."""
    rng = np.random.default_rng(102)
    offsets = _offsets(_seam_sizes(1 << 20), first=2)
    n = int(offsets[-1])
    rows = np.zeros((n, 8))
    rows[:, :2] = rng.uniform(-250.0, 250.0, (n, 2))
    rows[:, 2] = rng.uniform(0.0, 1000.0, n)
    rows[:, 3] = rng.uniform(5.0, 900.0, n)
    rows[:, 4] = rng.integers(2, 4000, n) + 0.5
    labels = rng.choice(np.array(INDICES + [-1], dtype=np.int64), n)
    return offsets, rows, labels


def test_rows_estimate_across_its_row_limit(ctx, spyral_rows):
    offsets, rows, labels = spyral_rows
    settings = EstimateSettings(25.0, 30, magnetic_field=2.85)
    whole = rows_to_estimates(offsets, rows, labels, INDICES, settings, ctx)
    alone = np.concatenate([rows_to_estimates(offsets[e:e + 2], rows, labels, INDICES, settings, ctx) for e in range(5)])
    _same_bits(whole, alone, "track estimates")


def test_rows_thin_across_its_row_limit(ctx, spyral_rows):
    offsets, rows, labels = spyral_rows
    settings = ThinSettings(5.0)
    w_off, w_points, w_labels, w_info = rows_to_points(offsets, rows, labels, INDICES, settings, ctx)
    parts = [rows_to_points(offsets[e:e + 2], rows, labels, INDICES, settings, ctx) for e in range(5)]
    rebased = np.concatenate([[0], np.cumsum([p[0][1] for p in parts])])
    assert w_off.tolist() == rebased.tolist() and w_off[-1] > 0
    _same_bits(w_points, np.concatenate([p[1] for p in parts]), "thinned points")
    _same_bits(w_labels, np.concatenate([p[2] for p in parts]), "point labels")
    _same_bits(w_info, np.concatenate([p[3] for p in parts]), "thin info")


def test_gain_rows_across_its_row_limit(ctx):
    rng = np.random.default_rng(103)
    limit = 4 << 20
    offsets = _offsets([limit // 2, limit // 2, 1])
    rows = int(offsets[-1])
    cell = np.concatenate([np.arange(m) for m in np.diff(offsets)])  # distinct (pad, time bucket) cells within an event
    points = np.empty((rows, 3))
    points[:, 0], points[:, 1] = cell // _abi.NUM_TB, cell % _abi.NUM_TB
    points[:, 2] = rng.integers(0, 1 << 20, rows)
    configure_gain(ctx, GainSettings(rel_variance=0.5, pad_gain=rng.uniform(0.5, 1.5, _abi.NUM_PADS), stream=5))
    seed, first_event = 77, 1000

    def gain(off, first):
        gained = np.zeros(rows)
        ctx.check(ctx.lib.attpc_gain_rows(ctx.handle, seed, first, len(off) - 1, _abi.iptr(off, I64), _abi.dptr(points),
                                          _abi.dptr(gained)), "attpc_gain_rows")
        return gained

    whole = gain(offsets, first_event)
    alone = sum(gain(np.ascontiguousarray(offsets[e:e + 2]), first_event + e) for e in range(3))  # (disjoint rows, else 0)
    assert np.count_nonzero(whole != points[:, 2]) > rows // 2
    _same_bits(whole, alone, "gained charges")
    configure_gain(ctx, None)


def test_baseline_and_pack_across_their_row_limit(ctx):
    rng = np.random.default_rng(104)
    split = 16384
    samples = rng.integers(0, 4096, (split + 1, _abi.NUM_TB), dtype=np.int16)
    y, baseline = remove_baseline(samples, 20.0, ctx, return_baseline=True)
    for part in (slice(0, split), slice(split, None)):
        y_part, baseline_part = remove_baseline(samples[part], 20.0, ctx, return_baseline=True)
        _same_bits(y[part], y_part, "y")
        _same_bits(baseline[part], baseline_part, "baseline")
    row_start, packed = pack_traces(samples, ctx)
    start_a, packed_a = pack_traces(samples[:split], ctx)
    start_b, packed_b = pack_traces(samples[split:], ctx)
    assert row_start.tolist() == np.concatenate([start_a, start_b[1:] + start_a[-1]]).tolist()
    _same_bits(packed, np.concatenate([packed_a, packed_b]), "packed bytes")


# ---------------------------------------------------------------- refusals ----
TRIGGER_DESC = dict(threshold=100, window=64, group_multiplicity=1, min_groups=1)


class _Args:
    """Two events and three rows for every CSR entry point; ``call(name, offsets, with_rows)`` -> status."""

    def __init__(self, ctx):
        self.ctx = ctx
        centers = hand_made_centers()
        ctx.forget("summary")
        assert ctx.lib.attpc_summary_configure(ctx.handle, _abi.SummaryDesc(0, _abi.dptr(centers), len(centers), 0)) == _abi.OK
        self.layout = _abi.EventLayout()
        self.layout.n_rows, self.layout.n_sim = 6, len(INDICES)
        for s, i in enumerate(INDICES):
            self.layout.indices[s] = i
        self.points = np.array([[4.0, 4.5, 40.0], [4.0, 7.2, 60.0], [9.0, 4.5, 50.0]])
        self.labels = np.array([2, 5, 2], dtype=np.int64)
        self.rows = np.zeros((3, 8))
        self.rows[:, :5] = [[40.0, 3.0, 100.0, 50.0, 300.5], [41.0, 4.0, 105.0, 60.0, 200.5], [42.0, 5.0, 110.0, 70.0, 100.5]]
        self.pads = np.array([3, 4, 5], dtype=np.int32)
        self.samples = np.full((3, _abi.NUM_TB), 300, dtype=np.int16)
        self.trigger = TriggerSettings(**TRIGGER_DESC).desc()
        self.estimate = EstimateSettings(25.0, 30, magnetic_field=2.85).desc()
        self.thin = ThinSettings(5.0).desc()

    def call(self, name, offsets, with_rows=True):
        ctx, lib, h, lay = self.ctx, self.ctx.lib, self.ctx.handle, self.layout
        off = _abi.iptr(np.ascontiguousarray(offsets, dtype=np.int64), I64)
        points, labels = (_abi.dptr(self.points), _abi.iptr(self.labels, I64)) if with_rows else (None, None)
        rows = _abi.dptr(self.rows) if with_rows else None
        if name == "attpc_trigger_rows":
            records = np.zeros(2, dtype=_abi.TRIGGER_DTYPE)
            pads, samples = (_abi.iptr(self.pads, I32), _abi.iptr(self.samples, I16)) if with_rows else (None, None)
            return lib.attpc_trigger_rows(h, 2, off, pads, samples, None, self.trigger, _abi.iptr(records, _abi.TriggerRecord))
        if name == "attpc_rows_estimate":
            records = np.zeros((2, lay.n_sim), dtype=_abi.ESTIMATE_DTYPE)
            return lib.attpc_rows_estimate(h, 2, off, rows, labels, lay, self.estimate, _abi.iptr(records, _abi.TrackEstimate))
        if name == "attpc_rows_thin":
            point_offsets, needed = np.zeros(3, dtype=np.int64), np.zeros(1, dtype=np.int64)
            out, out_labels = np.zeros((3, 8)), np.zeros(3, dtype=np.int64)
            info = np.zeros((2, lay.n_sim), dtype=_abi.THIN_INFO_DTYPE)
            return lib.attpc_rows_thin(h, 2, off, rows, labels, lay, self.thin, 3, _abi.iptr(point_offsets, I64), _abi.dptr(out),
                                       _abi.iptr(out_labels, I64), _abi.iptr(info, _abi.ThinInfo), _abi.iptr(needed, I64))
        if name == "attpc_gain_rows":
            gained = np.zeros(3)
            return lib.attpc_gain_rows(h, 1, 0, 2, off, points, _abi.dptr(gained))
        assert name == "attpc_cloud_summary"
        return lib.attpc_cloud_summary(h, 2, off, points, labels, lay, SummaryArrays(2, n_sim=lay.n_sim).out)

    def error(self):
        return (self.ctx.lib.attpc_last_error(self.ctx.handle) or b"").decode()


@pytest.fixture(scope="module")
def args(ctx):
    return _Args(ctx)


GOOD = [0, 1, 3]
CSR_OPERATORS = ("attpc_trigger_rows", "attpc_rows_estimate", "attpc_rows_thin", "attpc_gain_rows", "attpc_cloud_summary")
# (offsets, with the row arrays) -> the message; None: E_INVALID without a message of its own
CSR_REFUSALS = {
    "first_negative": ([-1, 1, 3], True, "offsets[0] < 0"),
    "decrease": ([0, 2, 1], True, "offsets decrease at event 1"),
    "rows_without_arrays": (GOOD, False, None),
}


@pytest.mark.parametrize("condition", CSR_REFUSALS)
@pytest.mark.parametrize("name", CSR_OPERATORS)
def test_csr_operators_refuse(args, name, condition):
    offsets, with_rows, message = CSR_REFUSALS[condition]
    assert args.call(name, GOOD) == _abi.OK
    before = args.error()
    assert args.call(name, offsets, with_rows) == _abi.E_INVALID
    if message is None:
        assert args.error() == before
    else:
        assert message in args.error()
    assert args.call(name, GOOD) == _abi.OK


@pytest.mark.parametrize("name", CSR_OPERATORS)
def test_csr_operators_report_the_first_of_two_faults(args, name):
    """offsets[0] < 0 and a decrease at event 0 in one array: attpc_gain_rows looks for the decrease first, the others at
    offsets[0]; a decrease at event 0 comes before one at event 1."""
    assert args.call(name, [-1, -2, 3]) == _abi.E_INVALID
    assert ("offsets decrease at event 0" if name == "attpc_gain_rows" else "offsets[0] < 0") in args.error()
    assert args.call(name, [5, 4, 3]) == _abi.E_INVALID
    assert "offsets decrease at event 0" in args.error()
    assert args.call(name, GOOD) == _abi.OK


@pytest.mark.parametrize("value", [4096, -1])
@pytest.mark.parametrize("name", ["attpc_trace_pack", "attpc_trace_baseline", "attpc_trigger_rows"])
def test_sample_operators_refuse(ctx, args, name, value):
    samples = args.samples.copy()
    y = np.empty_like(samples)

    def call(s):
        if name == "attpc_trace_pack":
            return ctx.lib.attpc_trace_pack(ctx.handle, 3, _abi.iptr(s, I16), None, None, 0, None)
        if name == "attpc_trace_baseline":
            return ctx.lib.attpc_trace_baseline(ctx.handle, 3, _abi.iptr(s, I16), 20.0, _abi.iptr(y, I16), None)
        records = np.zeros(2, dtype=_abi.TRIGGER_DTYPE)
        return ctx.lib.attpc_trigger_rows(ctx.handle, 2, _abi.iptr(np.array(GOOD, dtype=np.int64), I64), _abi.iptr(args.pads, I32),
                                          _abi.iptr(s, I16), None, args.trigger, _abi.iptr(records, _abi.TriggerRecord))

    samples[1, 7] = value
    samples[2, 0] = value  # (the first one is reported)
    assert call(samples) == _abi.E_INVALID
    assert f"sample 7 of row 1 is {value}: 0 .. 4095" in args.error()
    assert call(args.samples) == _abi.OK
