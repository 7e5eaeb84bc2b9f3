"""Drift distortion: the electric-field distortion map of the drift volume, applied to the track records on the device
(``attpc_det_configure_distortion``; the contract is in include/attpc_engine.h, "drift distortion",
``tests/distortion_reference.py`` restates it in numpy).  The engine's drift field is ideal; field-cage imperfections
and space charge give the real one a radial component, which pushes the drifting electrons radially and, through
E x B, azimuthally, and shifts their arrival time.  A ``DistortionMap`` holds those three shifts on a grid of (creation
radius, drift distance); with it on, every kept sample of every track is moved before anything reads it.  The stage is
opt-in (``distortion=``, ``Engine.configure_distortion``) and acts on every run function, since every one of them
integrates tracks.

Spyral corrects for this with a Garfield++ map (``garfield_file_path``, ``do_garfield_correction``).  There is no
reader for such files here: ``DistortionMap.from_function`` takes any f(rho, d), ``linear_radial_field`` is the closed
form of a field whose radial component grows linearly with the radius, and ``undistort_rows`` is the correction on
Spyral rows, so that a distorted run can be brought back on the host."""
from __future__ import annotations

import hashlib
import math

import numpy as np

from .. import _abi

MAX_NODES = 256        # per axis
MAX_SHIFT = 1.0        # m, |radial| and |azimuthal|
MAX_TIME = 1024.0      # time buckets, |time|
RHO_MAX = 0.292        # m, the radius of the pad plane


def _positive(what: str, value) -> float:
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"distortion {what} must be a number, got {value!r}")
    value = float(value)
    if not (value > 0.0 and math.isfinite(value)):
        raise ValueError(f"distortion {what} must be finite and > 0, got {value}")
    return value


def _table(what: str, values, cap: float, shape):
    """``values`` as a C-contiguous f64 table of ``shape`` (None: the table's own), or ValueError."""
    try:
        table = np.array(values, dtype=np.float64, order="C")
    except (TypeError, ValueError) as err:
        raise ValueError(f"the distortion's {what} table must be an array of numbers") from err
    if table.ndim != 2:
        raise ValueError(f"the distortion's {what} table must be [n_rho, n_d], got shape {table.shape}")
    if shape is not None and table.shape != shape:
        raise ValueError(f"the distortion's {what} table has shape {table.shape}, another has {shape}")
    if not all(2 <= n <= MAX_NODES for n in table.shape):
        raise ValueError(f"a distortion table has 2 .. {MAX_NODES} nodes per axis, got shape {table.shape}")
    if not np.all(np.abs(table) <= cap):  # (a NaN fails it)
        raise ValueError(f"the distortion's {what} values must be finite and |value| <= {cap:g}")
    return table


def _bilinear(table, i, j, fr, fs):
    """Step 3 of the contract, every operation rounded in the written order."""
    t00, t01, t10, t11 = table[i, j], table[i, j + 1], table[i + 1, j], table[i + 1, j + 1]
    lo = t00 + fs * (t01 - t00)
    hi = t10 + fs * (t11 - t10)
    return lo + fr * (hi - lo)


def _cell(a, n):
    a = np.where(a > n - 1, float(n - 1), a)
    a = np.where(a >= 0.0, a, 0.0)
    i = np.minimum(a.astype(np.int64), n - 2)
    return i, a - i


class DistortionMap:
    """The shifts of a drifting electron on a grid: ``radial`` [m, + = outward], ``azimuthal`` [m of arc, + =
    counter-clockwise] and ``time`` [time buckets, + = later], each [n_rho, n_d] (2 .. 256 nodes per axis) or None =
    zeros (at least one is given), at the creation radii rho_i = i rho_max / (n_rho - 1) and the drift distances
    d_j = j length / (n_d - 1), d = length - z; ``length`` None: the config's.  Between the nodes the map is bilinear,
    outside the grid the edge value holds.  Values are finite, at most 1 m and 1024 time buckets in size; anything else
    is ValueError."""

    slot, call = "distortion", "attpc_det_configure_distortion"

    def __init__(self, radial=None, azimuthal=None, time=None, rho_max: float = RHO_MAX, length: float | None = None):
        shape = None
        tables = []
        for what, values, cap in (("radial", radial, MAX_SHIFT), ("azimuthal", azimuthal, MAX_SHIFT), ("time", time, MAX_TIME)):
            table = None if values is None else _table(what, values, cap, shape)
            shape = shape if table is None else table.shape
            tables.append(table)
        if shape is None:
            raise ValueError("a DistortionMap needs at least one of its three tables")
        self.radial, self.azimuthal, self.time = (np.zeros(shape) if t is None else t for t in tables)
        self.n_rho, self.n_d = shape
        self.rho_max = _positive("rho_max", rho_max)
        self.length = None if length is None else _positive("length", length)

    @classmethod
    def from_function(cls, f, n_rho: int = 33, n_d: int = 41, rho_max: float = RHO_MAX, length: float = 1.0):
        """The map of ``f(rho, d) -> (dr, da, dt)`` (arrays in, arrays out) sampled on its nodes."""
        for what, n in (("n_rho", n_rho), ("n_d", n_d)):
            if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or not 2 <= int(n) <= MAX_NODES:
                raise ValueError(f"distortion {what} must be an integer in 2 .. {MAX_NODES}, got {n!r}")
        rho_max, length = _positive("rho_max", rho_max), _positive("length", length)
        rho = np.arange(int(n_rho), dtype=np.float64) * rho_max / (int(n_rho) - 1)
        d = np.arange(int(n_d), dtype=np.float64) * length / (int(n_d) - 1)
        dr, da, dt = f(rho[:, None], d[None, :])
        shape = (int(n_rho), int(n_d))
        return cls(*(np.broadcast_to(np.asarray(v, dtype=np.float64), shape) for v in (dr, da, dt)), rho_max=rho_max,
                   length=length)

    @classmethod
    def linear_radial_field(cls, epsilon_max: float, omega_tau: float, n_rho: int = 33, n_d: int = 41,
                            rho_max: float = RHO_MAX, length: float = 1.0):
        """The Langevin drift in a field whose radial component grows linearly with the radius, E_r / E_z =
        epsilon_max rho / rho_max, in B parallel to E_z with cyclotron frequency x collision time ``omega_tau``: over a
        drift distance d the electron moves dr = epsilon d / (1 + omega_tau^2) outward and da = omega_tau dr around.
        The time table is zero (first order in epsilon the arrival time does not move)."""
        eps_max, wt = float(epsilon_max), float(omega_tau)
        if not (math.isfinite(eps_max) and math.isfinite(wt)):
            raise ValueError(f"epsilon_max and omega_tau must be finite, got {epsilon_max!r}, {omega_tau!r}")
        rho_max = _positive("rho_max", rho_max)

        def field(rho, d):
            dr = (eps_max * rho / rho_max) * d / (1.0 + wt * wt)
            return dr, wt * dr, np.zeros_like(dr)

        return cls.from_function(field, n_rho, n_d, rho_max, length)

    @property
    def on(self) -> bool:
        return bool(np.any(self.radial != 0.0) or np.any(self.azimuthal != 0.0) or np.any(self.time != 0.0))

    def steps(self, config) -> tuple[float, float, float]:
        """(rho_step [m], tau_step [time buckets], tb_origin) of this map in the drift of ``config``: tb_origin is its
        micromegas_edge, and the last drift-distance node lies at windows_edge when the map's length is the config's."""
        mm, win = float(config.elec_params.micromegas_edge), float(config.elec_params.windows_edge)
        if not win > mm:
            raise ValueError("windows_edge <= micromegas_edge")
        span = win - mm
        if self.length is not None and self.length != float(config.det_params.length):
            span = span * (self.length / float(config.det_params.length))
        return self.rho_max / (self.n_rho - 1), span / (self.n_d - 1), mm

    def token(self, config):
        """None: a map that shifts nothing, the stage off."""
        if not self.on:
            return None
        h = hashlib.blake2b(digest_size=16)
        for table in (self.radial, self.azimuthal, self.time):
            h.update(table.tobytes())
        return (*self.steps(config), self.n_rho, self.n_d, h.digest())

    def desc(self, config) -> _abi.DistortDesc:
        """The ``attpc_distort_desc`` of this map in the drift of ``config`` (it refers to the map's own arrays)."""
        rho_step, tau_step, tb_origin = self.steps(config)
        return _abi.DistortDesc(rho_step, tau_step, tb_origin, self.n_rho, self.n_d, _abi.dptr(self.radial),
                                _abi.dptr(self.azimuthal), _abi.dptr(self.time))

    def shift(self, x, y, tb, config):
        """The forward map in numpy: creation points (x, y [m], ideal time bucket tb) -> the apparent (x', y', tb')."""
        rho_step, tau_step, tb_origin = self.steps(config)
        x, y, tb = (np.array(v, dtype=np.float64) for v in np.broadcast_arrays(x, y, tb))
        with np.errstate(all="ignore"):
            finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(tb)
            xs, ys, ts = (np.where(finite, v, 0.0) for v in (x, y, tb))
            rho = np.sqrt(xs * xs + ys * ys)
            i, fr = _cell(rho / rho_step, self.n_rho)
            j, fs = _cell((ts - tb_origin) / tau_step, self.n_d)
            dr, da, dt = (_bilinear(t, i, j, fr, fs) for t in (self.radial, self.azimuthal, self.time))
            safe = np.where(rho != 0.0, rho, 1.0)
            ux, uy = np.where(rho != 0.0, xs / safe, 0.0), np.where(rho != 0.0, ys / safe, 0.0)
            out = ((xs + dr * ux) - da * uy, (ys + dr * uy) + da * ux, ts + dt)
        return tuple(np.where(finite, new, old) for new, old in zip(out, (x, y, tb)))

    def undistort_rows(self, rows, config, iterations: int = 12):
        """The correction on Spyral rows [P, 8] (x mm, y mm, z mm, ...): every row's apparent point and time (z gives the
        time bucket through the writer's own relation, z = (windows_edge - tb) / (windows_edge - micromegas_edge)
        length) is taken back to where the electrons were made, by fixed-point iteration on the forward map -- one
        iteration evaluates ``shift`` at the current estimate and subtracts its discrepancy to the observed point from
        the estimate.  -> a copy of ``rows`` with new x, y, z columns, every other column untouched."""
        if isinstance(iterations, (bool, np.bool_)) or not isinstance(iterations, (int, np.integer)) or iterations < 0:
            raise ValueError(f"iterations must be an integer >= 0, got {iterations!r}")
        rows = np.array(rows, dtype=np.float64)
        if rows.ndim != 2 or rows.shape[1] < 3:
            raise ValueError(f"rows must be [P, >= 3], got shape {rows.shape}")
        mm, win = float(config.elec_params.micromegas_edge), float(config.elec_params.windows_edge)
        scale = float(config.det_params.length) * 1000.0 / (win - mm)  # mm per time bucket
        seen = (rows[:, 0] / 1000.0, rows[:, 1] / 1000.0, win - rows[:, 2] / scale)
        x, y, tb = seen
        for _ in range(int(iterations)):
            fx, fy, ft = self.shift(x, y, tb, config)
            x, y, tb = x - (fx - seen[0]), y - (fy - seen[1]), tb - (ft - seen[2])
        rows[:, 0], rows[:, 1], rows[:, 2] = x * 1000.0, y * 1000.0, (win - tb) * scale
        return rows


def _checked(distortion):
    if distortion is not None and not isinstance(distortion, DistortionMap):
        raise TypeError(f"distortion must be a DistortionMap or None, got {type(distortion).__name__}")
    return distortion


def configure_distortion(ctx: _abi.Context, distortion: DistortionMap | None, config=None) -> None:
    """``attpc_det_configure_distortion`` unless this ctx already holds the same map in the same drift (``None``, or a
    map that is zero everywhere: the stage off).  ``config``: the run's Config, whose time-bucket edges and length place
    the map's drift-distance nodes."""
    distortion = _checked(distortion)
    token = None
    if distortion is not None and distortion.on:
        if config is None:
            raise ValueError("a DistortionMap needs the run's config")
        token = distortion.token(config)
    ctx.configure(DistortionMap.slot, token, DistortionMap.call, None if token is None else distortion.desc(config))


def samples_to_distortion(samples, distortion: DistortionMap, config, ctx: _abi.Context | None = None) -> np.ndarray:
    """The stage alone, on the device (``attpc_samples_distort``): records [n, 4] (x m, y m, time bucket, electrons) ->
    the shifted records [n, 4].  It leaves the configured stage of ``ctx`` as it is."""
    if _checked(distortion) is None:
        raise TypeError("samples_to_distortion needs a DistortionMap")
    ctx = ctx or _abi.default_context()
    samples = np.ascontiguousarray(samples, dtype=np.float64)
    if samples.ndim != 2 or samples.shape[1] != 4:
        raise ValueError(f"samples must be [n, 4], got shape {samples.shape}")
    out = np.empty_like(samples)
    ctx.check(ctx.lib.attpc_samples_distort(ctx.handle, len(samples), _abi.dptr(samples), distortion.desc(config),
                                            _abi.dptr(out)), "attpc_samples_distort")
    return out
