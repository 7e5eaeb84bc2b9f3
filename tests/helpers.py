"""Shared builders for the tests: the same API objects -> descriptors for the oracle and
for the HIP library."""
from __future__ import annotations

import numpy as np

from attpc_engine_amd import GasTarget, _abi, nuclear_map, workloads
from attpc_engine_amd.detector.luts import build_det_desc, build_layout, species_for
from attpc_engine_amd.detector.simulator import default_indices
from attpc_engine_amd.kinematics import (
    Decay, ExcitationGaussian, KinematicsPipeline, KinematicsTargetMaterial, PolarUniform, Reaction,
)


class Inputs:
    """Descriptors of one workload: a ``workloads.WORKLOADS`` name or a builder of the same signature (such as
    ``chain7`` below).  ``det`` has the beam pads folded (product), ``det_raw`` has the unfolded LUT (the oracle
    applies the beam-pad list itself)."""

    def __init__(self, name, ode_substeps: int = 1, **kw):
        det_overrides = {k: kw.pop(k) for k in ("path_step",) if k in kw}  # DetectorParams fields, any workload
        builder = workloads.WORKLOADS[name] if isinstance(name, str) else name
        self.pipeline, self.config, self.indices = builder(**kw)
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


# ---------------------------------------------------------------- long decay chains: the layout limits ----
# ATTPC_MAX_STEPS = 8 steps (18 rows) and ATTPC_MAX_SIM = 8 simulated nuclei.  A 700 / 800 MeV 24Mg beam on the
# o16aa gas makes 26Al* by (a,d); the compound nucleus then evaporates one particle per step down to 12C (chain7) or
# 8Be (chain8).  The excitations sit above each step's separation energy, so every event is allowed; the products
# are forward-focused and start at one vertex, so 3 and more nuclei light the same (pad, time bucket) near it.
_CHAIN_DECAYS = [((13, 26), (1, 1)), ((12, 25), (0, 1)), ((12, 24), (2, 4)), ((10, 20), (1, 3)), ((9, 17), (1, 1)),
                 ((8, 16), (2, 4)), ((6, 12), (2, 4))]


def _long_chain(n_decays: int, beam_energy: float, excitations, indices, seed: int, **kw):
    nm = nuclear_map
    gas = GasTarget([(2, 4, 1)], 600.0, nm)
    steps = [Reaction(target=nm.get_data(2, 4), projectile=nm.get_data(12, 24), ejectile=nm.get_data(1, 2))]
    steps += [Decay(parent=nm.get_data(*par), residual_1=nm.get_data(*r1)) for par, r1 in _CHAIN_DECAYS[:n_decays]]
    pipeline = KinematicsPipeline(
        steps, [ExcitationGaussian(c, w) for c, w in excitations], [PolarUniform(0.0, np.pi)] * len(steps),
        beam_energy=beam_energy, target_material=KinematicsTargetMaterial(gas, (0.0, 1.0), 0.007), seed=seed, **kw)
    return pipeline, workloads.detector_config(gas), indices


def chain7(seed: int = 7, **kw):
    """7 steps, 16 rows: 4He(24Mg,d)26Al* ->p 25Mg* ->n 24Mg* ->a 20Ne* ->t 17F* ->p 16O* ->a 12C, 700 MeV beam.
    The reference's default indices [2, 4, 6, 8, 10, 12, 14, 15]: 8 nuclei (isim 0..7), species d, p, a, t, 12C;
    row 6 is the neutron (species -1, a dead track in the middle of the layout)."""
    ex = [(76.0, 1.0), (66.0, 1.0), (55.0, 1.0), (42.0, 3.0), (15.0, 1.0), (11.0, 0.5), (0.0, 0.0)]
    return _long_chain(6, 700.0, ex, default_indices(16), seed, **kw)


CHAIN8_INDICES = [17, 3, 16, 2, 9, 12, 5, 14]  # non-ascending: the last writer is the largest isim, not the largest row


def chain8(seed: int = 8, **kw):
    """8 steps, 18 rows: chain7 at 800 MeV with 12C* ->a 8Be added (rows 16, 17).  Indices ``CHAIN8_INDICES``: 8
    nuclei of 7 species (8Be, 26Al, a, d, 20Ne, p, 25Mg); labels 16 and 17 set the top bits of every label field."""
    ex = [(86.0, 1.0), (76.0, 1.0), (65.0, 1.0), (51.0, 1.0), (24.0, 1.0), (20.0, 1.0), (10.0, 0.5), (0.0, 0.0)]
    return _long_chain(7, 800.0, ex, list(CHAIN8_INDICES), seed, **kw)


LONG_CHAINS = {"chain7": chain7, "chain8": chain8}


def overlap_counts(orc, inp, p4, vertex, seed, first):
    """Oracle clouds of the events -> (points won by each position isim, keys lit by >= 3 nuclei, labels seen).  The
    nuclei touching a key come from one oracle run per nucleus alone (a nucleus' draws do not depend on the others).
    ``orc``: the oracle module (oracle/pyoracle.py)."""
    wins = np.zeros(_abi.MAX_SIM, dtype=np.int64)
    shared3, labels = 0, set()
    for e in range(len(p4)):
        pts, lab, _ = orc.simulate(inp.det_raw, inp.layout, seed, first + e, p4[e], vertex[e], capacity=1 << 20)
        labels |= set(lab.tolist())
        for isim, row in enumerate(inp.indices):
            wins[isim] += int((lab == row).sum())
        touched: dict[int, int] = {}
        for row in inp.indices:
            alone = build_layout(inp.z, inp.a, [row], inp.species)
            p1, _, _ = orc.simulate(inp.det_raw, alone, seed, first + e, p4[e], vertex[e], capacity=1 << 20)
            for k in (p1[:, 0].astype(np.int64) << 10 | np.floor(p1[:, 1]).astype(np.int64)).tolist():
                touched[k] = touched.get(k, 0) + 1
        shared3 += sum(1 for c in touched.values() if c >= 3)
    return wins, shared3, labels


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
