"""Shared builders for the tests: the same API objects -> descriptors for the oracle and
for the HIP library."""
from __future__ import annotations

import numpy as np

from attpc_engine_amd import _abi, nuclear_map, workloads
from attpc_engine_amd.detector.luts import build_det_desc, build_layout, species_for


class Inputs:
    """Descriptors of one workload.  ``det`` has the beam pads folded (product), ``det_raw``
    has the unfolded LUT (the oracle applies the beam-pad list itself)."""

    def __init__(self, name: str, ode_substeps: int = 1, **kw):
        det_overrides = {k: kw.pop(k) for k in ("path_step",) if k in kw}  # DetectorParams fields, any workload
        self.pipeline, self.config, self.indices = workloads.WORKLOADS[name](**kw)
        for key, value in det_overrides.items():
            setattr(self.config.det_params, key, value)
        self.kin, self._k1 = self.pipeline.device_desc()
        self.z = self.pipeline.get_proton_numbers()
        self.a = self.pipeline.get_mass_numbers()
        self.n_rows = len(self.z)
        if self.config is not None:
            self.species = species_for(self.z, self.a, self.indices)
            nuclei = [nuclear_map.get_data(z, a) for z, a in self.species]
            self.det, self._k2 = build_det_desc(self.config, nuclei, ode_substeps, fold_beam=True)
            self.det_raw, self._k3 = build_det_desc(self.config, nuclei, ode_substeps, fold_beam=False)
            self.layout = build_layout(self.z, self.a, self.indices, self.species)


def sort_cloud(points: np.ndarray, labels: np.ndarray):
    """Canonical order: by (pad, integer time bucket)."""
    pad = points[:, 0].astype(np.int64)
    tb = np.floor(points[:, 1]).astype(np.int64)
    order = np.lexsort((tb, pad))
    return points[order], labels[order]


def compare_clouds(pts_a, lab_a, pts_b, lab_b, charge_tol: float = 2.0):
    """Both sorted.  Keys, labels and jittered time buckets must agree exactly; charges to
    within ``charge_tol`` electrons (integer truncation of a product that differs in the
    last bits between host libm and device libm, see DESIGN.md "Tolerances")."""
    assert pts_a.shape == pts_b.shape, (pts_a.shape, pts_b.shape)
    np.testing.assert_array_equal(pts_a[:, 0], pts_b[:, 0])
    np.testing.assert_array_equal(np.floor(pts_a[:, 1]), np.floor(pts_b[:, 1]))
    np.testing.assert_array_equal(pts_a[:, 1], pts_b[:, 1])  # jitter is Philox-exact
    np.testing.assert_array_equal(lab_a, lab_b)
    diff = np.abs(pts_a[:, 2] - pts_b[:, 2])
    assert diff.max(initial=0.0) <= charge_tol, diff.max()
    return float(diff.max(initial=0.0))


# ---------------------------------------------------------------- event ids and seeds at full width ----
# Every draw of the engine is a function of (seed, global event id, ...): Philox4x32-10 with counter (event[31:0],
# event[63:32], index, domain) and key (seed[31:0], seed[63:32]), and the time-bucket jitter (Philox2x32-7, counter
# (event[31:0], event[39:32] << 24 | tb << 14 | pad), key word seed[31:0] ^ rotl(seed[63:32], 13) ^ 0x100).  The cases
# below put the ids where a narrowed id or seed would give other numbers: each range crosses (or sits past) the
# boundary named, and every seed has a high word.
U64 = 1 << 64
SEED_TYPICAL = 0xFEDCBA9876543210 & ((1 << 63) - 1)  # a 63-bit seed like simulate() draws
SEED_LO_ZERO = 0x1234567800000000                     # low word 0: a device keeping the low word runs seed 0
SEED_ALL_ONES = U64 - 1                               # every bit set; the int64 sign
SEED_MAX63 = (1 << 63) - 1                            # the largest seed simulate() / run_simulation() draw


class IdCase:
    """``n`` events from ``first_event`` at ``seed``; ``name`` says which narrowing the range is there to catch."""

    def __init__(self, name: str, first_event: int, seed: int, n: int = 24):
        assert 0 <= seed < U64 and 0 <= first_event and first_event + n <= U64
        self.name, self.first_event, self.seed, self.n = name, first_event, seed, n

    def ids(self, n: int | None = None) -> list[int]:
        return [self.first_event + e for e in range(self.n if n is None else n)]

    def __repr__(self):
        return f"IdCase({self.name}: first {self.first_event:#x}, seed {self.seed:#x}, n {self.n})"


# 24 events from 2^k - 20 cross 2^k at the 21st
ID_CASES = [
    IdCase("f32_exact", (1 << 24) - 20, SEED_TYPICAL),   # id carried as float
    IdCase("i32_sign", (1 << 31) - 20, SEED_LO_ZERO),    # id carried as int
    IdCase("u32_wrap", (1 << 32) - 20, SEED_ALL_ONES),   # event >> 32 dropped, (uint32_t) cast
    IdCase("hi_two", (1 << 33) + 17, SEED_MAX63),        # hi word used as a bool or a sign
    IdCase("jitter40", (1 << 40) - 20, SEED_TYPICAL),    # the jitter's 40-bit counter; ev << 24 overflows the checksum
    IdCase("f64_exact", (1 << 53) - 20, SEED_ALL_ONES),  # id through np.float64 / a Python float
    IdCase("top", U64 - 64, SEED_LO_ZERO),               # top of the range, int64 sign
]
ID_CASE_IDS = [c.name for c in ID_CASES]


def id_case(name: str) -> IdCase:
    return next(c for c in ID_CASES if c.name == name)


def _int32_wrap(v: int) -> int:
    return (((v & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000) % U64  # (uint64_t)(int64_t)(int32_t)v


def _through_float(v: int, dtype) -> int:
    return int(dtype(v)) % U64  # a value rounded past 2^64 wraps like the conversion on the device would


class Narrowing:
    """What a device with a narrowing bug would use instead of the correct (seed, event).  ``scope`` "all": every
    draw sees the narrowed values; "jitter": only the jitter's key word does (the Philox4x32 draws are right)."""

    def __init__(self, name: str, fn, scope: str = "all", on: str = "event"):
        self.name, self.fn, self.scope, self.on = name, fn, scope, on

    def __call__(self, seed: int, event: int) -> tuple[int, int]:
        return self.fn(seed, event)

    def __repr__(self):
        return f"Narrowing({self.name})"


NARROWINGS = [
    Narrowing("event_lo32", lambda s, e: (s, e & 0xFFFFFFFF)),
    Narrowing("event_int32", lambda s, e: (s, _int32_wrap(e))),
    Narrowing("event_float32", lambda s, e: (s, _through_float(e, np.float32))),
    Narrowing("event_float64", lambda s, e: (s, _through_float(e, np.float64))),
    Narrowing("seed_lo32", lambda s, e: (s & 0xFFFFFFFF, e), on="seed"),
    # jitter key word seed_lo ^ rotl(seed_hi, 13) ^ 0x100 with seed_hi = 0: the jitter of seed & 0xFFFFFFFF
    Narrowing("jitter_key_seed_hi_0", lambda s, e: (s & 0xFFFFFFFF, e), scope="jitter", on="seed"),
]
