"""The multiplicity trigger of the pad traces (include/attpc_engine.h, "multiplicity trigger") restated in numpy, and a
brute-force triple loop straight from its definitions.  Integers throughout: every comparison against the device is
exact equality.  ``trigger`` is anything with the attributes of ``detector.traces.TriggerSettings`` (threshold, window,
group_multiplicity, min_groups, groups)."""
import numpy as np

from attpc_engine_amd import _abi

NUM_TB = _abi.NUM_TB
MAX_GROUPS = 16
FIELDS = ("fired", "sample", "groups", "n_rows", "n_hit_pads", "peak_group_sum", "peak_sum", "peak_sample")


class Params:
    """The trigger parameters without the package's validation (the brute force and the restatement take either)."""

    def __init__(self, threshold, window=64, group_multiplicity=1, min_groups=1, groups=None):
        self.threshold, self.window = int(threshold), int(window)
        self.group_multiplicity, self.min_groups = int(group_multiplicity), int(min_groups)
        self.groups = None if groups is None else np.asarray(groups, dtype=np.uint8)


def _pad_terms(trigger, pads, pedestals):
    pads = np.asarray(pads, dtype=np.int64)
    groups = np.zeros(len(pads), dtype=np.int64) if trigger.groups is None else np.asarray(trigger.groups)[pads].astype(np.int64)
    ped = np.zeros(len(pads), dtype=np.int64) if pedestals is None else np.broadcast_to(np.asarray(pedestals), (_abi.NUM_PADS,))[pads].astype(np.int64)
    return groups, ped


def _empty():
    return (0, -1, 0, 0, 0, 0, 0, -1)


def event_record(pads, samples, trigger, pedestals=None):
    """One event's record as a tuple in the order of FIELDS: cumulative sums over the samples give the sliding window."""
    n = len(pads)
    if n == 0:
        return _empty()
    groups, ped = _pad_terms(trigger, pads, pedestals)
    hit = (np.asarray(samples, dtype=np.int64) - ped[:, None]) > trigger.threshold  # [rows, 512]
    part = groups != 255
    m = np.zeros((MAX_GROUPS, NUM_TB), dtype=np.int64)
    np.add.at(m, groups[part], hit[part].astype(np.int64))
    P = np.concatenate([np.zeros((MAX_GROUPS, 1), dtype=np.int64), np.cumsum(m, axis=1)], axis=1)  # P[:, j + 1] = sum m[:, 0..j]
    j = np.arange(NUM_TB)
    s = P[:, j + 1] - P[:, np.maximum(j + 1 - trigger.window, 0)]
    asserts = s >= trigger.group_multiplicity
    A = asserts.sum(axis=0)
    fire = np.flatnonzero(A >= trigger.min_groups)
    total = s.sum(axis=0)
    mask = 0
    for g in np.flatnonzero(asserts.any(axis=1)):
        mask |= 1 << int(g)
    peak_sum = int(total.max())
    return (int(fire.size > 0), int(fire[0]) if fire.size else -1, mask, n, int(hit[part].any(axis=1).sum()), int(s.max()),
            peak_sum, int(np.argmax(total)) if peak_sum else -1)


def event_record_brute(pads, samples, trigger, pedestals=None):
    """The same from the definitions, loop by loop (rows x samples x window)."""
    n = len(pads)
    if n == 0:
        return _empty()
    groups, ped = _pad_terms(trigger, pads, pedestals)
    samples = np.asarray(samples)
    W, Mg = trigger.window, trigger.group_multiplicity
    hit = [[int(samples[r][j]) - int(ped[r]) > trigger.threshold for j in range(NUM_TB)] for r in range(n)]
    fired, sample, mask, peak_group, peak_sum, peak_sample = 0, -1, 0, 0, 0, -1
    for j in range(NUM_TB):
        s = [0] * MAX_GROUPS
        for i in range(max(0, j - W + 1), j + 1):
            for r in range(n):
                if groups[r] != 255 and hit[r][i]:
                    s[groups[r]] += 1
        asserting = 0
        for g in range(MAX_GROUPS):
            if s[g] >= Mg:
                asserting += 1
                mask |= 1 << g
            peak_group = max(peak_group, s[g])
        if asserting >= trigger.min_groups and not fired:
            fired, sample = 1, j
        if sum(s) > peak_sum:
            peak_sum, peak_sample = sum(s), j
    n_hit = sum(1 for r in range(n) if groups[r] != 255 and any(hit[r]))
    return (fired, sample, mask, n, n_hit, peak_group, peak_sum, peak_sample)


def records(offsets, pads, samples, trigger, pedestals=None, one=event_record):
    """The records [n] (``_abi.TRIGGER_DTYPE``) of events in CSR form."""
    offsets = np.asarray(offsets, dtype=np.int64)
    out = np.zeros(len(offsets) - 1, dtype=_abi.TRIGGER_DTYPE)
    for e in range(len(out)):
        lo, hi = offsets[e], offsets[e + 1]
        out[e] = one(pads[lo:hi], samples[lo:hi], trigger, pedestals)
    return out


def differing(got, want):
    """(event, field, got, want) of the first few fields that differ: what an assertion shows."""
    return [(int(e), f, int(got[f][e]), int(want[f][e])) for f in FIELDS for e in np.flatnonzero(got[f] != want[f])[:3]]


def pulse_rows(rng, n_rows, pedestals=None, pads=None, sigma=4.0, max_amplitude=600):
    """Integer pulses plus noise on random pads: rows [n_rows, 512] int16 in 0 .. 4095 and their pads.  0 to 2 pulses
    per row, widths 3 .. 40 samples, anywhere -- the array's ends included."""
    pads = rng.integers(0, _abi.NUM_PADS, size=n_rows) if pads is None else np.asarray(pads)
    x = np.rint(rng.normal(0.0, sigma, size=(n_rows, NUM_TB))).astype(np.int64)
    j = np.arange(NUM_TB)
    for r in range(n_rows):
        for _ in range(int(rng.integers(0, 3))):
            centre, width, amp = rng.integers(-10, NUM_TB + 10), rng.integers(3, 41), rng.integers(20, max_amplitude)
            x[r] += np.rint(amp * np.exp(-0.5 * ((j - centre) / (width / 2.355)) ** 2)).astype(np.int64)
    if pedestals is not None:
        x += np.asarray(pedestals, dtype=np.int64)[pads][:, None]
    return pads.astype(np.int32), np.clip(x, 0, 4095).astype(np.int16)
