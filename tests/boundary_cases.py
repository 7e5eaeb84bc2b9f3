"""Deterministic samples that sit on the float -> integer decisions of the pad-plane scatter, and a host
emulation of the reference's transport that rounds either as numpy does or as a fused multiply-add would.

The scatter turns floating-point positions and times into integers in two places:

* the whole-mm LUT cell ``floor(line * 1000)`` of each of the 10 + 10 mesh lines of a sample, the lines being
  ``numpy.linspace(c - 3 sigma, c + 3 sigma, 10)`` (transporter.py:107-118, :221-227), and
* with the longitudinal-diffusion extension, the time bucket ``int(ts)`` of each slice time
  ``numpy.linspace(t - 3 sigma_l, t + 3 sigma_l, 5)[sl]`` (and its ``0 <= ts < 512`` test).

numpy rounds every product before the sum; ``a * b + c`` contracted into one FMA rounds once, and near a cell
edge the two can land in different cells.  Random inputs come within an ulp of such an edge about once in 1e14
lines, so these cases are constructed: each puts one line (or slice) a few ulp from an edge where the two
roundings disagree.  Only numpy and ``fractions`` are used (``fma`` below rounds the exact rational once).

Classes (``tests/golden/make_golden.py`` runs A, C with t >= 0 and D through the reference into
``tests/golden/boundary.npz``):

* A  mesh lines: every line index, both axes, both signs of the coordinate, sigma of t in 10..511 at the default
     diffusion and at 10x; kept only if the fused rounding changes the sample's key set.  Plus lines at the LUT's
     outer edges (floor = lo - 1, lo, hi - 1, hi).  ~2000 x gain electrons, so a moved pixel carries thousands.
* B  slice times (extension, no reference counterpart): a slice time whose bucket, or whose 0 <= ts < 512 test,
     differs between the two roundings.
* C  time edges: 0, -0, k and the double below k for k in 1, 256, 511, 512; -5e-324 and -1 (oracle only: a
     negative time is undefined behaviour in the reference).
* D  far off the plane but finite: |x| * 1000 beyond int32; must give no points.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

MESH = 10
SLICES = 5
NUM_TB = 512
LABEL = 2
GAIN = 175000
ELECTRONS = 2000 * GAIN
LONG_DIFFUSION = 0.3  # longitudinal diffusion of class B (the oracle's extension tests use the same value)


class Detector:
    """The constants the decisions depend on: the default detector (workloads.detector_config), folded LUT."""

    def __init__(self, diffusion: float = 0.277):
        from attpc_engine_amd import GasTarget, nuclear_map, workloads
        from attpc_engine_amd.detector.luts import compact_pad_lut, fold_beam_pads

        cfg = workloads.detector_config(GasTarget([(1, 2, 2)], 300.0, nuclear_map), diffusion=diffusion)
        lut, self.lut_lo = compact_pad_lut(cfg.pad_grid, cfg.pad_grid_edges)
        self.lut = fold_beam_pads(lut)
        self.lut_n = self.lut.shape[0]
        self.diffusion = float(diffusion)
        self.dv = float(cfg.drift_velocity)
        self.efield = float(cfg.det_params.efield)


# ---------------------------------------------------------------------------------------------- arithmetic ----
def fma(a: float, b: float, c: float) -> float:
    """a * b + c rounded once (what v_fma_f64 computes)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def linspace_ends(c: float, s: float, fused: bool) -> tuple[float, float]:
    """(c - 3 s, c + 3 s)."""
    if fused:
        return fma(-3.0, s, c), fma(3.0, s, c)
    return c - 3.0 * s, c + 3.0 * s


def linspace_at(lo: float, hi: float, n: int, i: int, fused: bool) -> float:
    """numpy.linspace(lo, hi, n)[i]: arange(n) * step + lo, the last element hi itself."""
    if i == n - 1:
        return hi
    step = (hi - lo) / float(n - 1)
    return fma(float(i), step, lo) if fused else float(i) * step + lo


def mesh_lines(c: float, sigma: float, fused: bool) -> list[float]:
    lo, hi = linspace_ends(c, sigma, fused)
    return [linspace_at(lo, hi, MESH, i, fused) for i in range(MESH)]


def sigma_t(det: Detector, t: float) -> float:
    """transporter.py:301, left to right; NaN for t < 0."""
    v = 2.0 * det.diffusion * det.dv * t / det.efield
    return math.sqrt(v) if v >= 0.0 or v == 0.0 else math.nan


def slice_times(det: Detector, t: float, fused: bool, dl: float = LONG_DIFFUSION) -> list[float]:
    """The 5 slice times of the longitudinal extension (oracle/attpc_oracle.c transport_track_ex)."""
    s = math.sqrt(2.0 * dl * det.dv * t / det.efield) / det.dv
    lo, hi = linspace_ends(t, s, fused)
    return [linspace_at(lo, hi, SLICES, sl, fused) for sl in range(SLICES)]


def slice_buckets(det: Detector, t: float, fused: bool) -> list[int]:
    """Time bucket of every slice, -1 where the slice is dropped (ts < 0) or masked later (ts >= 512)."""
    return [int(ts) if 0.0 <= ts < NUM_TB else -1 for ts in slice_times(det, t, fused)]


def cell(pos_m: float) -> int:
    return math.floor(pos_m * 1000.0)


def _pair(tb: int, pad: int) -> int:
    return tb * tb + tb + pad if tb >= pad else pad * pad + tb


def transport(det: Detector, x: float, y: float, t: float, electrons: int, fused: bool = False,
              label: int = LABEL) -> dict:
    """transport_track of one sample on the folded whole-mm LUT -> {key: [charge, label]} in insertion order."""
    points: dict = {}
    if not t >= 0.0:
        return points  # NaN sigma: dropped (oracle semantics; undefined in the reference)
    sigma = sigma_t(det, t)
    lo, hi = det.lut_lo, det.lut_lo + det.lut_n
    tb = int(t)

    def pad_at(cx: int, cy: int) -> int:
        if not (lo <= cx < hi and lo <= cy < hi):
            return -1
        return int(det.lut[cx - lo, cy - lo])

    def add(pad: int, q: int) -> None:
        key = _pair(tb, pad)
        points[key] = [points.get(key, [0, 0])[0] + q, label]

    if sigma == 0.0:
        pad = pad_at(cell(x), cell(y))
        if pad != -1:
            add(pad, int(electrons))
        return points
    xs, ys = mesh_lines(x, sigma, fused), mesh_lines(y, sigma, fused)
    h = 2 * 3 * sigma / (MESH - 1)
    c1 = 1 / 2 / math.pi / (sigma ** 2)
    for px in xs:
        for py in ys:
            pad = pad_at(cell(px), cell(py))
            if pad == -1:
                continue
            c2 = (-1 / 2 / sigma ** 2) * (((px - x) ** 2) + ((py - y) ** 2))
            add(pad, int(c1 * math.exp(c2) * (h * h) * electrons))
    return points


# ------------------------------------------------------------------------------------------------ class A ----
def _edge_with_pad_change(det: Detector, k0: int, other_cells: list[int], axis: int) -> int | None:
    """The whole-mm edge k nearest k0 (|k - k0| <= 3) where cells k - 1 and k lie on different pads for one of the
    other axis' lines."""
    lo, n = det.lut_lo, det.lut_n
    for dk in (0, 1, -1, 2, -2, 3, -3):
        k = k0 + dk
        if not (lo + 1 <= k < lo + n):
            continue
        for q in other_cells:
            if not (lo <= q < lo + n):
                continue
            a, b = (k - 1 - lo, q - lo), (k - lo, q - lo)
            if axis == 1:
                a, b = a[::-1], b[::-1]
            if det.lut[a] != det.lut[b]:
                return k
    return None


def mesh_cases(det: Detector, n_cases: int, seed: int, t_range=(10.0, 511.0), max_tries: int = 40000,
               scan_ulps: int = 40):
    """Class A: -> (xyt [n, 3], electrons [n], meta [n, 3] = (axis, line index, edge k))."""
    rng = np.random.default_rng(seed)
    rows, meta = [], []
    for tries in range(max_tries):
        if len(rows) >= n_cases:
            break
        line, axis, sign = tries % MESH, (tries // MESH) % 2, 1.0 if (tries // (2 * MESH)) % 2 == 0 else -1.0
        t = float(rng.uniform(*t_range))
        sigma = sigma_t(det, t)
        r, phi = 0.25 * math.sqrt(rng.uniform(0.0, 1.0)), rng.uniform(0.0, 2.0 * math.pi)
        u, v = abs(r * math.cos(phi)) * sign, r * math.sin(phi)  # u: the coordinate whose line is on the edge
        v_cells = [cell(p) for p in mesh_lines(v, sigma, False)]
        k = _edge_with_pad_change(det, cell(mesh_lines(u, sigma, False)[line]) + 1, v_cells, axis)
        if k is None:
            continue
        u += k / 1000.0 - mesh_lines(u, sigma, False)[line]  # line `line` now within an ulp or two of k mm
        cands = [u]
        up = dn = u
        for _ in range(scan_ulps):
            up, dn = math.nextafter(up, math.inf), math.nextafter(dn, -math.inf)
            cands += [up, dn]
        for c in cands:
            lo_n, hi_n = linspace_ends(c, sigma, False)
            lo_f, hi_f = linspace_ends(c, sigma, True)
            if cell(linspace_at(lo_n, hi_n, MESH, line, False)) == cell(linspace_at(lo_f, hi_f, MESH, line, True)):
                continue
            x, y = (c, v) if axis == 0 else (v, c)
            if set(transport(det, x, y, t, ELECTRONS)) != set(transport(det, x, y, t, ELECTRONS, fused=True)):
                rows.append((x, y, t))
                meta.append((axis, line, k))
                break
    xyt = np.array(rows, dtype=np.float64).reshape(-1, 3)
    return xyt, np.full(len(xyt), ELECTRONS, dtype=np.int64), np.array(meta, dtype=np.int64).reshape(-1, 3)


def lut_edge_cases(det: Detector, t: float = 200.0):
    """Class A, outer edges: line 0 or 9 on the first double whose cell is lo - 1, lo, hi - 1 or hi (both axes)."""
    sigma = sigma_t(det, t)
    lo, hi = det.lut_lo, det.lut_lo + det.lut_n
    rows, meta = [], []
    for axis in (0, 1):
        for k in (lo - 1, lo, hi - 1, hi):
            for line in (0, MESH - 1):
                u = k / 1000.0 - (mesh_lines(0.0, sigma, False)[line])
                while cell(mesh_lines(u, sigma, False)[line]) >= k:
                    u = math.nextafter(u, -math.inf)
                while cell(mesh_lines(u, sigma, False)[line]) < k:
                    u = math.nextafter(u, math.inf)
                rows.append((u, 0.0) if axis == 0 else (0.0, u))
                meta.append((axis, line, k))
    xyt = np.column_stack([np.array(rows), np.full(len(rows), t)])
    return xyt, np.full(len(xyt), ELECTRONS, dtype=np.int64), np.array(meta, dtype=np.int64)


# ------------------------------------------------------------------------------------------------ class B ----
def slice_cases(det: Detector, per_target: int = 2, scan_ulps: int = 6):
    """Class B: sample times t (positions in the pad plane's interior) where one slice's bucket, or its
    0 <= ts < 512 test, differs between numpy and fused rounding.  Targets: the slice edge at 0 and every bucket edge
    1..512, for every slice that can reach it.  A slice time lands exactly on an edge for about one t, and the two
    roundings part there with a chance of about ulp(3 sigma_l) / ulp(t): a few percent in the first buckets, under
    one percent near 512 -- so most hits are early ones."""
    targets = [(0, 0.0)] + [(sl, float(k)) for k in range(1, NUM_TB + 1) for sl in range(SLICES)]
    rows, meta = [], []
    for sl, k in targets:
        def ts_of(t):
            return slice_times(det, t, False)[sl]
        a, b = 1e-3, 600.0  # ts is increasing in t here: bisect for the t whose slice sl sits on k
        if not (ts_of(a) <= k <= ts_of(b)):
            continue
        for _ in range(200):
            m = 0.5 * (a + b)
            if m in (a, b):
                break
            a, b = (m, b) if ts_of(m) < k else (a, m)
        found, up, dn = 0, b, b
        for _ in range(scan_ulps):
            for t in (up, dn):
                if found < per_target and slice_buckets(det, t, False) != slice_buckets(det, t, True):
                    rows.append((0.05, 0.03, t))
                    meta.append((sl, int(k)))
                    found += 1
            up, dn = math.nextafter(up, math.inf), math.nextafter(dn, -math.inf)
    xyt = np.array(rows, dtype=np.float64).reshape(-1, 3)
    return xyt, np.full(len(xyt), ELECTRONS, dtype=np.int64), np.array(meta, dtype=np.int64).reshape(-1, 2)


# ------------------------------------------------------------------------------------------- classes C, D ----
def time_edge_cases(negative: bool = False):
    """Class C: times on the bucket edges (t >= 0), or the negative ones (oracle only)."""
    if negative:
        ts = [-5e-324, -1.0]
    else:
        ts = [0.0, -0.0]
        for k in (1.0, 256.0, 511.0, 512.0):
            ts += [k, math.nextafter(k, -math.inf)]
    rows = [(x, y, t) for t in ts for x, y in ((0.05, 0.03), (-0.1107, 0.0421))]
    return np.array(rows, dtype=np.float64), np.full(len(rows), ELECTRONS, dtype=np.int64)


def far_cases():
    """Class D: finite positions whose mm value is beyond int32 (sigma > 0): no points."""
    rows = []
    for far in (3.0e6, -3.0e6, 1.0e300, -1.0e300):
        rows += [(far, 0.02, 100.0), (0.02, far, 300.0), (far, far, 450.0)]
    return np.array(rows, dtype=np.float64), np.full(len(rows), ELECTRONS, dtype=np.int64)
