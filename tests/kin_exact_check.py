"""The comparison of a kinematics implementation with ``tests/golden/kin_exact.npz`` (numpy only: the fixture is
all the GPU test has of ``tests/kin_exact_reference.py``).  One rule for the oracle, the device and the numpy
restatement that the mutation checks bend:

  * decided cases (every class but ``hair``): the status equals the exact one, a row is NaN exactly where the exact
    chain has none, and every row lies within K * S_row of the exact row, S_row = sum over the steps up to the row's
    own of 2^-53 E_parent(lab) max(1, E*_a / p*, E*_b / p*);
  * ``bulk`` and ``angle`` cases also within the plain 1e-9 MeV the project promised before this bound existed;
  * ``hair`` cases (excitation within 32 spacings of m1 + m2 + ex of the exact threshold): either status, but status 0
    means finite rows within K * S_row, and a forbidden case has NaN rows.

K is measured, not derived: the largest error / S_row against the exact rows, asserted at four times the measured
value."""
from __future__ import annotations

from pathlib import Path

import numpy as np

# measured largest error / S_row over the decided cases and the status-0 hair cases, and where it was seen
K_ORACLE = 1.1415  # oracle/attpc_oracle.c (gcc, -ffp-contract=off): li5_ap case 16, 1e-8 MeV above threshold, row 0
K_DEVICE = 0.9256  # kinematics.hip on an MI355X: b10_3he_chain case 44 (bulk), row 4
MARGIN = 4.0
PLAIN_MEV = 1e-9
# what a run must have compared: cases per class over the five chains and the four explicit-parent sets
EXPECTED_CASES = {"bulk": 334, "angle": 103, "energy": 50, "threshold": 188, "hair": 384}


def load(golden_dir: Path) -> dict:
    with np.load(golden_dir / "kin_exact.npz") as g:
        return {k: g[k] for k in g.files}


class Tally:
    """What the launches of one test compared: cases per class and the worst error / S_row with its case."""

    def __init__(self):
        self.cases = {}
        self.worst = (0.0, "none")
        self.worst_plain = (0.0, "none")

    def assert_complete(self):
        assert self.cases == EXPECTED_CASES, (self.cases, EXPECTED_CASES)


def compare(fx: dict, name: str, p4: np.ndarray, status: np.ndarray, k_measured: float, tally: Tally) -> None:
    """``p4`` [n, rows, 4] and ``status`` [n] of chain or decay set ``name`` against the fixture."""
    classes = [str(c) for c in fx["classes"]]
    cls = fx[f"{name}_class"]
    ref, scale, want = fx[f"{name}_p4"], fx[f"{name}_scale"], fx[f"{name}_status"]
    assert p4.shape == ref.shape and status.shape == want.shape, (name, p4.shape, ref.shape)
    hair = cls == classes.index("hair")
    decided = ~hair
    np.testing.assert_array_equal(status[decided], want[decided], err_msg=f"{name}: status of decided cases")
    np.testing.assert_array_equal(np.isnan(p4[decided]), np.isnan(ref[decided]), err_msg=f"{name}: which rows exist")
    # hair: a forbidden case has no rows, an allowed one has all of its own step's
    gave_up = hair & (status != 0)
    assert np.isnan(p4[gave_up][:, -2:]).all(), f"{name}: a forbidden hair case with rows"
    went_on = hair & (status == 0)
    assert np.isfinite(p4[went_on]).all(), \
        f"{name}: status 0 with non-finite rows at hair cases {np.flatnonzero(went_on & ~np.isfinite(p4).all(axis=(1, 2))).tolist()}"
    judged = decided | went_on
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(p4 - ref).max(axis=2)               # [n, rows]; NaN where neither has the row
        ratio = np.where(judged[:, None], err / scale, np.nan)
    assert not np.isnan(ratio[went_on]).any(), f"{name}: a hair case without exact rows"
    if np.isfinite(ratio).any():
        flat = int(np.nanargmax(ratio))
        i, r = divmod(flat, ratio.shape[1])
        if ratio[i, r] > tally.worst[0]:
            tally.worst = (float(ratio[i, r]), f"{name} case {i} ({classes[cls[i]]}) row {r}: {err[i, r]:.3e} MeV, "
                                               f"S_row {scale[i, r]:.3e}")
        assert ratio[i, r] <= MARGIN * k_measured, \
            f"{name} case {i} ({classes[cls[i]]}) row {r}: {err[i, r]:.3e} MeV = {ratio[i, r]:.3f} S_row > {MARGIN * k_measured:.3f}"
    plain = (cls == classes.index("bulk")) | (cls == classes.index("angle"))
    if np.isfinite(err[plain]).any():
        worst = float(np.nanmax(err[plain]))
        if worst > tally.worst_plain[0]:
            i = int(np.flatnonzero(plain)[np.argmax(np.where(np.isnan(err[plain]), -1.0, err[plain]).max(axis=1))])
            tally.worst_plain = (worst, f"{name} case {i}")
        assert worst <= PLAIN_MEV, f"{name}: {worst:.3e} MeV on a bulk / angle case"
    for i, c in enumerate(classes):
        tally.cases[c] = tally.cases.get(c, 0) + int((cls == i).sum())
