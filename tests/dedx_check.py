"""The one rule that holds a track made on the stopping-power TABLE to the smooth track of tests/golden/dedx_smooth.npz
(``get_dedx`` called in every right-hand side; tests/golden/make_dedx_smooth.py).  numpy only: tests/test_gpu_dedx_table.py
applies it to the device's kept samples, tests/test_dedx_table_cpu.py to the oracle's and to the mutants'.

A track is given as the engine delivers it: kept samples (x, y, time bucket, electrons x gain) in order, and ``n_steps``.

* alignment   kept samples carry no grid index.  Sample j takes the grid point of the smooth track nearest to it among
              those behind the index of sample j - 1 (z from the time bucket through ``length``, the drift velocity and
              ``micromegas_edge``).  A sample whose nearest grid point is not at least ten times closer than the second
              nearest is left out of the per-sample checks; at most 1 % of a track's kept samples may be.
* positions   every aligned sample within ``2 D_tab + 1e-7 m`` of the smooth track at its grid time (D_tab: the table's
              effect by two reference integrations, 1e-7 m: RK4 against the converged table solution; the factor 2
              stays below the 4 of a grid of 16 sub-bins), and within 0.5 mm (the end-to-end budget of DESIGN section 6)
* rows        ``n_steps`` within max(3, 2 %) of the smooth track's rows, and the same terminal event.  The engine does
              not deliver the event: the sample extrapolated linearly behind the last two kept ones crosses z = 1, z = 0
              or the cage -- or none of them, and then the track has handed (nearly) all its energy to the gas
* range       (tracks along +z) ``z_last - z_vertex`` equals the range by quadrature from the start energy down to the
              smooth track's energy at that sample's grid time, within ``2 D_tab + 1e-7 m``
* electrons   the running sum S_k of electrons up to grid index k obeys ``Q_k - k - q <= S_k <= Q_k + q`` with
              ``Q_k = (KE_0 - KE_smooth(t_k)) 1e6 / W`` and ``q = 2 E_tab 1e6 / W``: every sample truncates less than one
              electron, and every dropped sample held less than one
"""
from __future__ import annotations

import numpy as np

RHO_MAX = 0.292
POSITION_FLOOR = 1.0e-7    # m, RK4 on the grid against the converged solution on the same table
BUDGET = 5.0e-4            # m
LEFT_OUT_CAP = 0.01
ALIGN_RATIO = 10.0


class Fixture:
    """tests/golden/dedx_smooth.npz, case by name."""

    def __init__(self, path):
        self.g = np.load(path)
        self.names = [str(n) for n in self.g["case_names"]]

    def case(self, name: str) -> dict:
        i = self.names.index(name)
        g = self.g
        out = {"track": g[f"track_{i}"], "rows": int(g[f"rows_{i}"]), "event": str(g[f"event_{i}"]),
               "d_tab": float(g[f"d_tab_{i}"]), "e_tab": float(g[f"e_tab_{i}"]), "p4": g[f"p4_{i}"],
               "vertex": g[f"vertex_{i}"], "table_rows": int(g[f"table_rows_{i}"])}
        if f"range_{i}" in g.files:
            out["range"] = g[f"range_{i}"]
        return out


def z_of_time_bucket(tb, det):
    dv = det.length / float(det.windows_edge - det.micromegas_edge)
    return det.length - (np.asarray(tb) - float(det.micromegas_edge)) * dv


def kept_from_track(track: np.ndarray, mass: float, det) -> np.ndarray:
    """What generate_electrons and generate_point_cloud (solver.py:332-398) keep of ODE rows [n, 6] at Fano factor 0:
    (x, y, time bucket, trunc(|dKE| 1e6 / W) x gain) of the rows with at least one electron."""
    g = np.sqrt((track[:, 3:6] ** 2).sum(axis=1))
    beta = np.sqrt(g * g / (1.0 + g * g))
    ke = mass * (g / beta - 1.0)
    el = np.zeros(len(track))
    el[1:] = np.abs(np.diff(ke))
    el = (el * (1.0e6 / det.w_value)).astype(np.int64)
    keep = el >= 1
    dv = det.length / float(det.windows_edge - det.micromegas_edge)
    tb = (det.length - track[keep, 2]) / dv + float(det.micromegas_edge)
    return np.column_stack([track[keep, 0], track[keep, 1], tb, (el[keep] * int(det.mpgd_gain)).astype(np.float64)])


def align(kept_xyz: np.ndarray, grid_xyz: np.ndarray, ratio: float = ALIGN_RATIO):
    """-> (grid index [m], sure [m])."""
    index = np.empty(len(kept_xyz), dtype=np.int64)
    sure = np.zeros(len(kept_xyz), dtype=bool)
    last = 0
    for j, p in enumerate(kept_xyz):
        d = np.sqrt(((grid_xyz - p) ** 2).sum(axis=1))
        lo = min(last + 1, len(grid_xyz) - 1)
        k = lo + int(np.argmin(d[lo:]))
        others = np.delete(d, k)
        sure[j] = len(others) == 0 or ratio * d[k] <= others.min()
        index[j] = k
        last = k
    return index, sure


def ending(xyz: np.ndarray, deposited: float, ke0: float, slack: float) -> str:
    """The terminal event that the kept samples show (see the module docstring); ``deposited`` [MeV]: W x the electrons
    of the whole track, ``slack`` [MeV]: what truncation, dropped samples and the table may have kept of ``ke0``."""
    if len(xyz) >= 2:
        nxt = 2.0 * xyz[-1] - xyz[-2]
        if nxt[2] >= 1.0:
            return "z_forward"
        if nxt[2] <= 0.0:
            return "z_backward"
        if np.hypot(nxt[0], nxt[1]) >= RHO_MAX:
            return "rho"
    return "ke" if deposited >= ke0 - slack else "none"


def check_track(fx: dict, kept: np.ndarray, n_steps: int, det, along_z: bool = False, min_electrons_per_row: float = 0.0):
    """Apply the rule -> figures (dict); raises AssertionError where the track breaks it."""
    smooth, rows, d_tab, e_tab = fx["track"], fx["rows"], fx["d_tab"], fx["e_tab"]
    w = float(det.w_value)
    ke0 = float(smooth[0, 3])
    fig = {}
    xyz = np.column_stack([kept[:, 0], kept[:, 1], z_of_time_bucket(kept[:, 2], det)])
    index, sure = align(xyz, smooth[:, :3])
    fig["kept"], fig["left_out"] = len(kept), int((~sure).sum())
    assert fig["left_out"] <= LEFT_OUT_CAP * len(kept), ("left out of the alignment", fig["left_out"], len(kept))
    assert sure.any(), ("no sample aligned", len(kept))
    # positions
    bound = 2.0 * d_tab + POSITION_FLOOR
    dist = np.sqrt(((xyz - smooth[index, :3]) ** 2).sum(axis=1))[sure]
    fig["position"], fig["position_bound"] = float(dist.max(initial=0.0)), bound
    assert fig["position"] <= bound, ("position", fig["position"], bound, int(index[sure][np.argmax(dist)]))
    assert fig["position"] <= BUDGET, ("position budget", fig["position"])
    # rows and ending
    fig["rows"], fig["smooth_rows"] = int(n_steps), rows
    assert abs(int(n_steps) - rows) <= max(3, 0.02 * rows), ("rows", n_steps, rows)
    electrons = kept[:, 3] / float(det.mpgd_gain)
    running = np.cumsum(electrons)
    q = 2.0 * e_tab * 1.0e6 / w
    slack = (n_steps + q + 1.0) * w * 1.0e-6 + 2.0e-6   # truncations, the table, and the 1 eV + of the last row
    fig["event"] = ending(xyz, float(running[-1]) * w * 1.0e-6 if len(running) else 0.0, ke0, slack)
    assert fig["event"] == fx["event"], ("terminal event", fig["event"], fx["event"])
    # range identity
    if along_z:
        j = int(np.flatnonzero(sure)[-1])
        fig["range_difference"] = float(abs((xyz[j, 2] - fx["vertex"][2]) - fx["range"][index[j]]))
        assert fig["range_difference"] <= bound, ("range", fig["range_difference"], bound)
    # electrons
    k = index[sure]
    q_k = (ke0 - smooth[k, 3]) * 1.0e6 / w
    s_k = running[sure]
    fig["q_last_per_row"] = float((ke0 - smooth[-1, 3]) * 1.0e6 / w / rows)
    assert fig["q_last_per_row"] > min_electrons_per_row, ("electrons per row", fig["q_last_per_row"])
    fig["electrons_over"] = float((s_k - q_k).max(initial=-np.inf))          # must be <= q
    fig["electrons_under"] = float((q_k - k - s_k).max(initial=-np.inf))     # must be <= q
    fig["electrons_q"] = q
    assert fig["electrons_over"] <= q and fig["electrons_under"] <= q, ("electrons", fig["electrons_over"],
                                                                         fig["electrons_under"], q)
    return fig
