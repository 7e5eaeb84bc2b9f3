"""The runs of the law tests (test_laws_cpu.py on the oracle and the restatement, test_gpu_laws.py on the device): their
pipelines, sizes and seeds, fixed here before anything was run, and the few helpers both files need to turn an
engine's output into the arrays ``tests/law_analysis.py`` takes."""
from __future__ import annotations

import numpy as np

from attpc_engine_amd import GasTarget, nuclear_map, workloads
from attpc_engine_amd.detector.beam_pads import BEAM_PADS_ARRAY
from attpc_engine_amd.detector.luts import build_det_desc
from attpc_engine_amd.detector.simulator import default_indices
from attpc_engine_amd.kinematics import (
    Decay, ExcitationBreitWigner, ExcitationUniform, KinematicsPipeline, PolarArbitrary, PolarUniform, Reaction,
)
from tests import law_analysis as la
from tests.law_reference import PadPlane, fano_mu, mc_sigma

HI = 1 << 32  # a seed or an event id one high word further

# K1: o16aa as the workload defines it
K1_N, K1_SEED = 400_000, 11
K1_LAW = dict(rho_sigma=0.007, z_range=(0.0, 1.0), ex_centre=9.585, ex_sigma=0.42 / 2.355)  # reference excitation.py:80

# K2: tabulated Breit-Wigner and binned polar angle
K2_N, K2_SEED, K2_PIT_SEED = 1_000_000, 9, 0
K2_BEAM, K2_CENTROID, K2_WIDTH, K2_BINS = 24.0, 2.3, 0.8, 36
K2_BIN_WIDTH = np.pi / K2_BINS
K2_ANGLES = np.arange(K2_BINS) * K2_BIN_WIDTH
K2_PROBS = np.sin(K2_ANGLES + 0.04) ** 2
K2_PROBS = K2_PROBS / (K2_PROBS.sum() * (1.0 + 1e-12))  # PolarArbitrary refuses a sum a rounding above 1

# K3: both steps refuse, and whether step 1 passes depends on ex0
K3_N, K3_SEED = 400_000, 13
K3_BEAM, K3_RANGE0, K3_RANGE1 = 24.0, (0.0, 45.0), (0.0, 40.0)

F_EVENTS, F_SEED, F_PIT_SEED, F_CALL = 300, 21, 0, 100
J_EVENTS, J_SEED, J_MIN_PAIRS = 20, 7, 10_000
M_SEED, M_EVENT, M_CENTRE, M_SAMPLES, M_PRIMARIES = 5, 9, (0.0531, 0.0307), 40, 10_000


def k2(seed: int = K2_SEED, **kw):
    """10B(3He, a)9B, 9B a relativistic Breit-Wigner (2.3 MeV, width 0.8), sin^2 polar bins, 24 MeV, no target."""
    nm = nuclear_map
    pipeline = KinematicsPipeline(
        [Reaction(target=nm.get_data(5, 10), projectile=nm.get_data(2, 3), ejectile=nm.get_data(2, 4))],
        [ExcitationBreitWigner(nm.get_data(5, 9).mass, K2_CENTROID, K2_WIDTH)],
        [PolarArbitrary(K2_ANGLES, K2_PROBS, K2_BIN_WIDTH)], beam_energy=K2_BEAM, seed=seed, **kw)
    return pipeline, None, default_indices(4)


def k2_bw() -> tuple:
    return float(nuclear_map.get_data(5, 9).mass), K2_CENTROID, K2_WIDTH


def k3(seed: int = K3_SEED, **kw):
    """10B(3He, a)9B*, 9B* -> p + 8Be*, both excitations uniform, 24 MeV, no target."""
    nm = nuclear_map
    pipeline = KinematicsPipeline(
        [Reaction(target=nm.get_data(5, 10), projectile=nm.get_data(2, 3), ejectile=nm.get_data(2, 4)),
         Decay(parent=nm.get_data(5, 9), residual_1=nm.get_data(1, 1))],
        [ExcitationUniform(*K3_RANGE0), ExcitationUniform(*K3_RANGE1)], [PolarUniform(0.0, np.pi)] * 2,
        beam_energy=K3_BEAM, seed=seed, **kw)
    return pipeline, None, default_indices(6)


def masses_of(kin) -> np.ndarray:
    return np.array([kin.masses[i] for i in range(4 + 2 * (kin.n_steps - 1))], dtype=np.float64)


def with_field(desc, **fields):
    """A copy of a ctypes descriptor with some scalar fields changed (its pointers stay those of the original)."""
    copy = type(desc).from_buffer_copy(bytes(desc))
    for k, v in fields.items():
        setattr(copy, k, v)
    return copy


# ------------------------------------------------------------------------------------------------- Fano ----
def fano_rows(orc, inp, det, p4, vertex) -> dict:
    """{(event index, isim): (xyt [rows, 3], mu [rows])} of every track: position and time bucket of each trajectory
    row as generate_point_cloud writes them, and the mean of its Fano draw, |dKE| 1e6 / W in f64 from the oracle's
    trajectory rows (``orc.trajectory``: no draw enters them)."""
    dv = det.length / (det.windows_edge - det.micromegas_edge)
    out = {}
    for e in range(len(p4)):
        for isim, row in enumerate(inp.indices):
            sp = inp.layout.species_of_row[row]
            track = orc.trajectory(det, sp, vertex[e], p4[e, row])
            xyt = np.column_stack([track[:, 0], track[:, 1], (det.length - track[:, 2]) / dv + det.micromegas_edge])
            out[(e, isim)] = (xyt, fano_mu(track, det.species[sp].mass, det.w_value))
    return out


def fano_samples(rows: dict, inp, gain: int, kept_of, expect_trunc: bool = False) -> la.FanoSamples:
    """Kept samples of every track -> FanoSamples.  ``kept_of(e, isim)`` gives the engine's kept samples [m, 4] (x, y,
    time bucket, electrons * gain), which are aligned to the trajectory rows of ``fano_rows`` by position.
    ``expect_trunc`` (a run at Fano factor 0): assert that the kept samples are exactly the rows with trunc(mu) >= 1
    and carry exactly trunc(mu) electrons -- the alignment and mu proving themselves."""
    out = la.FanoSamples()
    for (e, isim), (xyt, mu) in rows.items():
        kept = kept_of(e, isim)
        k = la.align_kept_fast(xyt, kept[:, :3])
        n = kept[:, 3] / gain
        assert (n == np.round(n)).all() and (n >= 1).all()
        if expect_trunc:
            want = np.trunc(mu)
            np.testing.assert_array_equal(k, np.flatnonzero(want >= 1))
            np.testing.assert_array_equal(n, want[k])
        out.add(e, inp.indices[isim], k, mu[k], n)
    return out


# ------------------------------------------------------------------------------- Monte-Carlo diffusion ----
class McSetup:
    """The detector of tests/test_gpu_scatter_fixtures.py with ``mc_diffusion`` on, the hand-made samples and what
    the law expects of them."""

    def __init__(self, n_samples: int = M_SAMPLES, n_primary: int = M_PRIMARIES):
        gas = GasTarget([(1, 2, 2)], 300.0, nuclear_map)
        self.cfg = workloads.detector_config(gas, diffusion=0.277)
        self.cfg.det_params.mc_diffusion = True
        proton = [nuclear_map.get_data(1, 1)]
        self.det, self._k1 = build_det_desc(self.cfg, proton, fold_beam=True)
        self.det_raw, self._k2 = build_det_desc(self.cfg, proton, fold_beam=False)
        self.gain = int(self.det.mpgd_gain)
        self.n_primary = n_primary
        self.plane = PadPlane(self.det_raw, BEAM_PADS_ARRAY)
        tb = 100.25 + 10.0 * np.arange(n_samples)
        self.xyt = np.column_stack([np.full(n_samples, M_CENTRE[0]), np.full(n_samples, M_CENTRE[1]), tb])
        self.electrons = np.full(n_samples, n_primary * self.gain, dtype=np.int64)
        dv = self.det.length / (self.det.windows_edge - self.det.micromegas_edge)
        self.sigmas = mc_sigma(tb, self.det.diffusion, dv, self.det.efield)
        self.total = n_samples * n_primary

    def expected(self):
        return la.mc_expected(self.plane, *M_CENTRE, self.sigmas, self.n_primary)

    def observed(self, pad, charge) -> dict:
        """Cloud (pad, charge) rows of the whole event -> {pad: primaries}; every charge a multiple of the gain."""
        charge = np.asarray(charge, dtype=np.int64)
        assert (charge % self.gain == 0).all(), charge[charge % self.gain != 0][:5]
        pads, inverse = np.unique(np.asarray(pad, dtype=np.int64), return_inverse=True)
        counts = np.bincount(inverse.ravel(), weights=(charge // self.gain).astype(np.float64))
        return {int(p): int(c) for p, c in zip(pads, counts)}
