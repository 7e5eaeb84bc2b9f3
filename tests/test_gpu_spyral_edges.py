"""The fused Spyral path (spyral_count_kernel / spyral_write_kernel, csrc/spyral.hip) against its numpy restatement
(tests/spyral_reference.py) where the kernels decide something: charges from zero to full saturation of the ADC,
thresholds at an amplitude that occurs and at the clip, kept counts either side of the wave and workgroup strides, events
the threshold empties between events it does not, responses with equal, zero and negative samples, and sort bins of
dozens of rows.  Every case takes the cloud of ``Engine.run(fetch=True)`` and the rows of ``Engine.run_spyral`` for the
same seed and ids, 3 events per chunk: offsets, event_points, labels and every column but the integral are EQUAL, the
integral is within 1e-12 of the exact sum of the 512 clipped products.  Every case first asserts, on its own cloud, that
the reference's sequential f64 sum is within 1e-13 of that exact sum -- then 1e-12 against it asks no more than DESIGN
4.4 asks against the reference's loop.  The runs are those of tests/spyral_cases.py, which tests/test_spyral_cpu.py
checks on the CPU oracle.  Not pinned: equal sort keys (two rows of one event with the same jittered time bucket cannot
be had from a run).  Needs a real MI355X: ``-m gpu``."""
import time

import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.writer import convert_to_spyral
from attpc_engine_amd.engine import Engine
from tests import spyral_cases as cases
from tests.spyral_reference import Geometry, clipped_count, convert, fused_rows, integral_sequential

pytestmark = pytest.mark.gpu

OTHER_COLUMNS = [0, 1, 2, 3, 5, 6, 7]
_T0 = time.monotonic()
_CLOUDS: dict = {}  # (run, gain) -> the cloud of Engine.run(fetch=True)
_ROWS: dict = {}    # (run, gain, response name) -> convert() of that cloud: every row, the exact integrals


@pytest.fixture(scope="module", autouse=True)
def _report_runtime():
    yield
    print(f"\ntests/test_gpu_spyral_edges.py: {time.monotonic() - _T0:.1f} s")


@pytest.fixture(scope="module")
def ctx():
    return _abi.Context(0)


def _relative(got, want):
    zero = want == 0.0
    assert (got[zero] == 0.0).all()
    return float((np.abs(got[~zero] - want[~zero]) / np.abs(want[~zero])).max(initial=0.0))


class Case:
    """One run of tests/spyral_cases.py at one gain: its engine (made anew: an Engine configures the context's detector),
    its cloud and, per response, the restatement's rows of that cloud."""

    def __init__(self, ctx, run, gain, capacity_per_event=12288):
        self.ctx, self.run, self.gain = ctx, run, gain
        self.name, self.first, self.n = run
        pipeline, self.config, indices = cases.builder(self.name, gain)()
        self.engine = Engine(pipeline, self.config, indices, context=ctx, chunk_events=3)
        self.capacity = capacity_per_event
        self.geo = Geometry.of(self.config)
        self.responses = cases.responses(self.config)
        key = (run, gain)
        if key not in _CLOUDS:
            _CLOUDS[key] = self.engine.run(self.n, seed=cases.SEED, first_event=self.first, fetch=True,
                                           capacity_per_event=capacity_per_event)
        self.cloud = _CLOUDS[key]
        self.offsets, self.points, self.labels = self.cloud["offsets"], self.cloud["points"], self.cloud["labels"]

    def converted(self, response="default"):
        key = (self.run, self.gain, response)
        if key not in _ROWS:
            rows = convert(self.points, self.responses[response], self.geo)
            # the condition of the tolerance: the reference's own loop is within 1e-13 of the exact sum on these charges
            loop = _relative(integral_sequential(self.responses[response], self.points[:, 2]), rows[:, 4])
            print(f"{self.name} gain {self.gain:g} {response}: the sequential f64 sum is within {loop:.2e} of the exact sum")
            assert loop <= 1e-13
            _ROWS[key] = rows
        return _ROWS[key]

    def amplitudes(self, event=None, response="default"):
        amp = self.converted(response)[:, 3]
        return amp if event is None else amp[self.offsets[event]:self.offsets[event + 1]]

    def want(self, threshold, response="default", event=None):
        """The restatement at ``threshold``: of the whole run, or of event ``event`` alone."""
        rows = self.converted(response)
        if event is None:
            return fused_rows(self.offsets, self.points, self.labels, self.responses[response], self.geo, threshold, converted=rows)
        lo, hi = self.offsets[event], self.offsets[event + 1]
        return fused_rows([0, hi - lo], self.points[lo:hi], self.labels[lo:hi], self.responses[response], self.geo, threshold,
                          converted=rows[lo:hi])

    def fused(self, threshold, response="default", compact=1, event=None):
        """Engine.run_spyral at ``threshold``: of the whole run, or of event ``event`` in a run of its own."""
        self.engine.configure_spyral(cases.with_settings(self.config, threshold=threshold), response=self.responses[response])
        first, n = (self.first, self.n) if event is None else (self.first + event, 1)
        self.ctx.set_option("compact_transfer", compact)
        try:
            return self.engine.run_spyral(n, seed=cases.SEED, first_event=first, capacity_per_event=self.capacity)
        finally:
            self.ctx.set_option("compact_transfer", 1)

    def check(self, threshold, response="default", compact=(1, 0), event=None, what=""):
        """The fused rows at ``threshold`` in the transfer formats ``compact`` against the restatement -> (the
        restatement's FusedRows, the worst relative error of the integral)."""
        want = self.want(threshold, response, event)
        worst = 0.0
        for c in compact:
            got = self.fused(threshold, response, c, event)
            np.testing.assert_array_equal(got["offsets"], want.offsets)
            np.testing.assert_array_equal(got["event_points"], want.event_points)
            np.testing.assert_array_equal(got["labels"], want.labels)
            np.testing.assert_array_equal(got["rows"][:, OTHER_COLUMNS], want.rows[:, OTHER_COLUMNS])
            err = _relative(got["rows"][:, 4], want.rows[:, 4])
            print(f"{what or self.name} gain {self.gain:g} {response} threshold {threshold!r} compact {c}: "
                  f"{want.offsets[-1]} of {len(self.points)} rows kept, integral within {err:.2e}")
            np.testing.assert_allclose(got["rows"][:, 4], want.rows[:, 4], rtol=1e-12, atol=0)
            for lo, hi in zip(want.offsets[:-1], want.offsets[1:]):
                assert (np.diff(got["rows"][lo:hi, 2]) >= 0).all()
            worst = max(worst, err)
        return want, worst


# ---------------------------------------------------------------- gain sweep ----
def test_gain_sweep_reaches_partial_clips_at_large_charges(ctx):
    """What the sweep is for, asserted on its own clouds: at 1e11 at least 100 kept rows with q >= 1e13 and some but not
    all samples clipped; at least 10 values of k over the sweep."""
    ks = set()
    for gain in cases.GAINS:
        case = Case(ctx, cases.SWEEP, gain)
        q, k = case.points[:, 2], clipped_count(case.responses["default"], case.points[:, 2])
        ks |= set(k.tolist())
        kept = case.amplitudes() > 40.0
        print(f"gain {gain:g}: {len(q)} rows, {int(kept.sum())} above 40, q up to {q.max():.3g}, k in {k.min()} .. {k.max()}")
        if gain == cases.GAINS[-1]:
            assert (kept & (q >= 1e13) & (k > 0) & (k < 512)).sum() >= 100
    assert len(ks) >= 10, sorted(ks)


@pytest.mark.parametrize("gain", cases.GAINS)
def test_gain_sweep(ctx, gain):
    """Default threshold of 40, both transfer formats (at 1e11 the charges do not fit the 24-byte record and the chunk
    falls back to the plain rows).  The stand-alone convert_to_spyral (the sequential kernel) is held to the same
    restatement on the partly clipped rows.  With the integral as 4095 k + q (total - prefix[k]) this test fails at 1e11
    (3634 of 22656 rows beyond 1e-12, the worst at 6.7e-11; 2.4e-14 at 1e8); with 4095 k + q tail[k] it shows 2.2e-16
    at 1e11 and 2.5e-16 at 1e8."""
    case = Case(ctx, cases.SWEEP, gain)
    case.check(40.0)
    rows = case.converted()
    k = clipped_count(case.responses["default"], case.points[:, 2])
    part = np.flatnonzero((k > 0) & (k < 512))
    if gain > cases.GAINS[0]:
        assert len(part) >= 100
    if len(part):
        alone = convert_to_spyral(np.ascontiguousarray(case.points[part]), case.geo.windows_edge, case.geo.micromegas_edge,
                                  case.geo.length, case.responses["default"], case.geo.pad_centers, case.geo.pad_sizes, ctx=ctx)
        np.testing.assert_array_equal(alone[:, OTHER_COLUMNS], rows[part][:, OTHER_COLUMNS])
        print(f"gain {gain:g}: {len(part)} partly clipped rows, sequential kernel within {_relative(alone[:, 4], rows[part, 4]):.2e}")
        np.testing.assert_allclose(alone[:, 4], rows[part, 4], rtol=1e-12, atol=0)


# ---------------------------------------------------------------- thresholds ----
def test_threshold_at_an_amplitude_that_occurs(ctx):
    """amplitude > threshold is strict: rows whose amplitude IS the threshold are dropped."""
    case = Case(ctx, cases.THRESHOLDS, cases.LOW_GAIN)
    event = int(np.argmax(np.diff(case.offsets)))
    amp = np.sort(case.amplitudes(event))
    threshold = float(amp[(3 * len(amp)) // 4])  # an amplitude of the event's own, a quarter of its rows above it
    everywhere = case.amplitudes()
    assert (everywhere == threshold).sum() >= 1 and (everywhere > threshold).sum() >= 100
    want, _ = case.check(threshold)
    assert (want.rows[:, 3] > threshold).all() and want.offsets[-1] == (everywhere > threshold).sum()
    below = float(np.nextafter(threshold, 0.0))  # one ulp lower: those rows are kept
    want_below, _ = case.check(below, compact=(1,))
    assert want_below.offsets[-1] == want.offsets[-1] + (everywhere == threshold).sum()


def test_threshold_below_and_at_zero(ctx):
    """-1.0 keeps the rows of zero charge, 0.0 drops exactly those."""
    case = Case(ctx, cases.THRESHOLDS, cases.LOW_GAIN)
    zero = case.points[:, 2] == 0.0
    assert zero.sum() >= 10 and (~zero).sum() >= 1000
    want, _ = case.check(-1.0)
    assert want.offsets[-1] == len(case.points) and (want.rows[:, 3] == 0.0).sum() == zero.sum()
    want, _ = case.check(0.0)
    assert want.offsets[-1] == (~zero).sum() and (want.rows[:, 3] > 0.0).all()


def test_threshold_at_and_just_under_the_clip(ctx):
    """Gain 1e11: nothing exceeds 4095.0; one ulp lower exactly the saturated rows survive."""
    case = Case(ctx, cases.SWEEP, cases.GAINS[-1])
    saturated = case.amplitudes() == 4095.0
    assert saturated.sum() >= 1000 and (~saturated).sum() >= 10
    want, _ = case.check(4095.0)
    assert want.offsets[-1] == 0
    np.testing.assert_array_equal(want.event_points, np.diff(case.offsets))
    want, _ = case.check(float(np.nextafter(4095.0, 0.0)))
    assert want.offsets[-1] == saturated.sum() and (want.rows[:, 3] == 4095.0).all()


def test_kept_counts_at_the_wave_and_workgroup_strides(ctx):
    """One event of at least 300 rows in runs of its own, thresholds among its own amplitudes so that 0, 1, 63, 64, 65, 255,
    256, 257 rows survive (where equal amplitudes make a count unreachable, the nearest that is)."""
    case = Case(ctx, cases.THRESHOLDS, cases.LOW_GAIN)
    event = int(np.argmax(np.diff(case.offsets)))
    amp = case.amplitudes(event)
    assert len(amp) >= 300
    values = np.unique(amp)
    reachable = np.array([(amp > v).sum() for v in values])  # rows kept with the threshold at each amplitude
    used = []
    for m in (0, 1, 63, 64, 65, 255, 256, 257):
        i = int(np.argmin(np.abs(reachable - m)))
        want, _ = case.check(float(values[i]), event=event, what=f"event {case.first + event}, {m} rows wanted")
        assert want.offsets[-1] == reachable[i]
        used.append(int(reachable[i]))
    print("kept counts used:", used)
    assert 0 in used and any(1 < c < 64 for c in used) and any(64 < c < 256 for c in used) and any(c > 256 for c in used)


def test_events_emptied_between_events_that_keep_rows(ctx):
    """The threshold at the median of the events' largest amplitudes: the kept-rows scan and the early return of the write
    kernel with empty events between filled ones; event_points stays the count before the threshold."""
    case = Case(ctx, cases.THRESHOLDS, cases.LOW_GAIN)
    top = np.array([case.amplitudes(e).max(initial=0.0) for e in range(case.n)])
    threshold = float(np.median(top))
    want, _ = case.check(threshold)
    kept = np.diff(want.offsets)
    filled = np.flatnonzero(kept > 0)
    print("rows kept per event:", kept.tolist(), "of", want.event_points.tolist())
    assert (kept == 0).sum() >= 2 and len(filled) >= 2 and (kept[filled[0]:filled[-1]] == 0).any()
    np.testing.assert_array_equal(want.event_points, np.diff(case.offsets))
    assert (want.event_points[kept == 0] > 0).any()  # emptied by the threshold, not empty from the start


# ---------------------------------------------------------------- other responses ----
@pytest.mark.parametrize("gain", [cases.GAINS[0], cases.GAINS[-1]])
@pytest.mark.parametrize("response", ["default", "bipolar", "flat", "single"])
def test_other_responses(ctx, response, gain):
    """Sorted tables with ties (flat: k is 0 or 512), zeros (default: 257 of them; single: 511) and negative lobes."""
    case = Case(ctx, cases.RESPONSES, gain)
    want, _ = case.check(40.0, response=response)
    assert want.offsets[-1] >= 1000
    k = clipped_count(case.responses[response], case.points[:, 2])
    if response == "flat":
        assert set(k.tolist()) <= {0, 512} and (gain == cases.GAINS[0] or (k == 512).any())
    if response == "single":
        np.testing.assert_array_equal(want.rows[:, 4], want.rows[:, 3])
        assert set(k.tolist()) <= {0, 1}
    if response == "bipolar":
        assert (case.responses[response] < 0.0).sum() == 226
        if gain == cases.GAINS[-1]:
            assert (want.rows[:, 4] < 0.0).any() and (want.rows[:, 4] > 0.0).any()


# ---------------------------------------------------------------- a crowded sort ----
def test_sort_bins_of_dozens_of_rows(ctx):
    """Two events of b10chain as written (a track sample every 0.1 mm, tens of thousands of rows per event), every row
    kept: (time bucket, sixteenth of the jitter) bins of 32 and more rows, ranked inside the bin on the key."""
    case = Case(ctx, cases.CROWDED, cases.GAINS[0], capacity_per_event=98304)
    fullest = [int(np.bincount(cases.sort_bins(case.points[lo:hi, 1])).max()) for lo, hi in zip(case.offsets[:-1], case.offsets[1:])]
    print("rows per event", np.diff(case.offsets).tolist(), "fullest sort bin per event", fullest)
    assert max(fullest) >= 32
    want, _ = case.check(-1.0)
    assert want.offsets[-1] == len(case.points)
