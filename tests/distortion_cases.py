"""The maps and point sets of the drift-distortion tests (tests/test_distortion_cpu.py, tests/test_gpu_distortion.py).

M, the named map: ``DistortionMap.linear_radial_field(0.05, 2.0)`` on 33 x 41 nodes, rho_max 0.292 m, length 1 m, with
the time table 4 (rho / rho_max)^2 d / length time buckets, in a drift with the edges 10 / 560.  Its largest shift is
22 mm in the plane (10 mm outward, 20 mm around, at rho_max after the full drift; 21 mm inside rho < 0.28 m) and 4 time
buckets (3.6 inside rho < 0.28 m)."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from attpc_engine_amd.detector.distortion import DistortionMap
from tests import distortion_reference as dref

N_RHO, N_D, RHO_MAX, LENGTH = 33, 41, 0.292, 1.0
MM_EDGE, WIN_EDGE = 10, 560


def drift(length: float = LENGTH, micromegas_edge: int = MM_EDGE, windows_edge: int = WIN_EDGE):
    """What a DistortionMap reads of a Config."""
    return SimpleNamespace(det_params=SimpleNamespace(length=length),
                           elec_params=SimpleNamespace(micromegas_edge=micromegas_edge, windows_edge=windows_edge))


def time_table() -> np.ndarray:
    rho = np.arange(N_RHO) * RHO_MAX / (N_RHO - 1)
    d = np.arange(N_D) * LENGTH / (N_D - 1)
    return 4.0 * (rho[:, None] / RHO_MAX) ** 2 * d[None, :] / LENGTH


def named_map() -> DistortionMap:
    field = DistortionMap.linear_radial_field(0.05, 2.0, N_RHO, N_D, RHO_MAX, LENGTH)
    return DistortionMap(field.radial, field.azimuthal, time_table(), rho_max=RHO_MAX, length=LENGTH)


def reference_map(m: DistortionMap | None = None, config=None) -> dref.Map:
    """M (or ``m``) as the restatement takes it, the three derived numbers written out here, not taken from the package."""
    m = named_map() if m is None else m
    config = drift() if config is None else config
    span = float(config.elec_params.windows_edge - config.elec_params.micromegas_edge)
    return dref.Map(m.rho_max / (m.n_rho - 1), span / (m.n_d - 1), float(config.elec_params.micromegas_edge),
                    m.radial, m.azimuthal, m.time)


def random_records(n: int = 20000, seed: int = 1, rho_limit: float = 0.28) -> np.ndarray:
    """[n, 4]: points uniform in the disc rho < rho_limit, tb uniform in 10 .. 560, electrons x gain."""
    rng = np.random.default_rng(seed)
    rho = rho_limit * np.sqrt(rng.uniform(size=n))
    phi = rng.uniform(0.0, 2.0 * np.pi, size=n)
    tb = rng.uniform(MM_EDGE, WIN_EDGE, size=n)
    q = np.floor(rng.uniform(1.0, 5000.0, size=n)) * 175000.0
    return np.ascontiguousarray(np.stack([rho * np.cos(phi), rho * np.sin(phi), tb, q], axis=1))


def edge_records() -> np.ndarray:
    """The edges of the contract: rho = 0 (and x = -0.0), rho exactly on a node, rho beyond the last node, tau < 0, tau
    beyond the last node, tau exactly on a node, a NaN and an infinite record, a q that is a NaN with a payload."""
    rho_step, tau_step = RHO_MAX / (N_RHO - 1), (WIN_EDGE - MM_EDGE) / (N_D - 1)
    rows = []
    for tb in (10.0, 123.456, 560.0):
        rows += [[0.0, 0.0, tb, 1.0], [-0.0, 0.0, tb, 2.0], [0.0, -0.0, tb, 3.0], [-0.0, -0.0, tb, 4.0]]  # rho = 0
    for i in (1, 2, 7, 16, 31, 32):  # on a node, along the axes (rho = |x| exactly) and on the last node
        rows += [[i * rho_step, 0.0, 77.7, 5.0], [0.0, -(i * rho_step), 300.25, 6.0], [-(i * rho_step), -0.0, 559.0, 7.0]]
    for j in (0, 1, 20, 39, 40):     # tau on a node
        rows += [[0.1, -0.05, MM_EDGE + j * tau_step, 8.0], [RHO_MAX, 0.0, MM_EDGE + j * tau_step, 9.0]]
    rng = np.random.default_rng(2)
    for _ in range(40):              # beyond the last radius node; before and beyond the drift
        phi = rng.uniform(0.0, 2.0 * np.pi)
        rho = rng.uniform(RHO_MAX, 0.5)
        rows.append([rho * np.cos(phi), rho * np.sin(phi), rng.uniform(MM_EDGE, WIN_EDGE), 10.0])
        rows.append([0.2 * np.cos(phi), 0.2 * np.sin(phi), rng.uniform(-50.0, MM_EDGE), 11.0])
        rows.append([0.2 * np.cos(phi), 0.2 * np.sin(phi), rng.uniform(WIN_EDGE, 700.0), 12.0])
        rows.append([rho * np.cos(phi), rho * np.sin(phi), rng.uniform(WIN_EDGE, 700.0), 13.0])
    rows += [[1.0e200, 1.0, 100.0, 14.0], [1.0e-200, 1.0e-200, 100.0, 15.0], [0.1, 0.1, 1.0e300, 16.0], [0.1, 0.1, -1.0e300, 17.0]]
    rows += [[np.nan, 0.1, 100.0, 18.0], [0.1, np.nan, 100.0, 19.0], [0.1, 0.1, np.nan, 20.0],
             [np.inf, 0.1, 100.0, 21.0], [0.1, -np.inf, 100.0, 22.0], [0.1, 0.1, np.inf, 23.0]]
    out = np.array(rows, dtype=np.float64)
    payload = np.array([0x7FF8000000ABCDEF, 0xFFF0000000000001], dtype=np.uint64).view(np.float64)  # q keeps its bits
    extra = np.array([[0.05, 0.06, 200.0, 0.0], [0.05, 0.06, 200.0, 0.0]])
    extra[:, 3] = payload
    return np.ascontiguousarray(np.concatenate([out, extra]))


def bad_descs():
    """(what, keyword changes) of every way an attpc_distort_desc can be wrong; ``tables`` entries replace one value
    of the named table."""
    nan, inf = float("nan"), float("inf")
    cases = [("rho_step", v) for v in (0.0, -1.0, nan, inf)] + [("tau_step", v) for v in (0.0, -2.0, nan, inf)]
    cases += [("tb_origin", v) for v in (nan, inf, -inf)]
    cases += [("n_rho", v) for v in (1, 0, -3, 257)] + [("n_tau", v) for v in (1, 0, -3, 257)]
    cases += [("radial", v) for v in (nan, inf, 1.0000001, -1.5)] + [("azimuthal", v) for v in (nan, -inf, -1.0000001)]
    cases += [("time", v) for v in (nan, inf, 1024.5, -1025.0)]
    return cases
