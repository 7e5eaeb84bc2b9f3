"""Track straggling: multiple Coulomb scattering and energy-loss straggling in the track integrator, on the device
(``attpc_det_configure_straggling``; the contract is in include/attpc_engine.h, "track straggling",
``tests/straggle_reference.py`` restates it in numpy).  The integrator solves a deterministic equation of motion, so
without this stage two particles of one momentum follow one path to the last bit; with it every recorded sample of a
track gets a Gaussian kick of its direction (Rossi-Greisen, without Highland's logarithm) and a Gaussian fluctuation of
its kinetic energy (Bohr).  The stage is opt-in (``StragglingSettings``, ``straggling=``, ``Engine.configure_straggling``)
and acts on every run function, since every one of them integrates tracks.

What the model is not: it has no single-scattering tail and no Landau tail, and Bohr's variance is too large at low
velocity.  ``angular_scale`` and ``energy_scale`` exist so that a user can fit the lateral and the range straggling of
their own SRIM or LISE tables."""
from __future__ import annotations

import math

import numpy as np

from .. import _abi
from .constants import AVOGADRO
from .stage import configure_stage


def _number(what: str, value) -> float:
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"straggling {what} must be a number, got {value!r}")
    return float(value)


def _elements(target):
    """[(Z, A, stoichiometry)] and the density [g/cm^3] of a target, or ValueError."""
    compound, density = getattr(target, "compound", None), getattr(target, "density", None)
    if compound is None or density is None:
        raise ValueError("the target has no compound and density: give radiation_length and electron_density")
    density = float(density)
    if not (density > 0.0 and math.isfinite(density)):
        raise ValueError(f"the target's density must be finite and > 0, got {density}")
    elements = [(int(z), int(a), int(s)) for z, a, s in compound]
    if not elements or any(z < 1 or a < 1 or s < 1 for z, a, s in elements):
        raise ValueError(f"the target's compound must be (Z >= 1, A >= 1, stoichiometry >= 1) per element, got {compound!r}")
    return elements, density


def dahl_radiation_length(z: int, a: float) -> float:
    """Dahl's formula for the radiation length of an element in g/cm^2: 716.4 A / (Z (Z + 1) ln(287 / sqrt(Z)))."""
    return 716.4 * a / (z * (z + 1) * math.log(287.0 / math.sqrt(z)))


def radiation_length(target) -> float:
    """The radiation length X0 [m] of a gas target (``compound`` = [(Z, A, stoichiometry)], ``density`` in g/cm^3):
    Dahl's formula per element with the mass number as A, mixed by mass fraction (1 / X0 = sum w_i / X0_i) and divided
    by the density.  ValueError for a target without those attributes."""
    elements, density = _elements(target)
    total = sum(a * s for _, a, s in elements)
    inverse = sum((a * s / total) / dahl_radiation_length(z, a) for z, a, s in elements)  # cm^2 / g
    return 1.0 / inverse / density * 1.0e-2


def electron_density(target) -> float:
    """Electrons per m^3 of a gas target: density * N_A * (sum Z s) / molar mass (the target's ``molar_mass`` in g/mol
    if it has one, else the sum of its mass numbers).  ValueError for a target without compound and density."""
    elements, density = _elements(target)
    molar = float(getattr(target, "molar_mass", 0.0) or sum(a * s for _, a, s in elements))
    return density * AVOGADRO * sum(z * s for z, _, s in elements) / molar * 1.0e6


class StragglingSettings:
    """The validated settings of the track straggling (``attpc_straggle_desc``, include/attpc_engine.h):
    ``angular_scale`` and ``energy_scale`` (finite, >= 0; 0 skips that part, both 0: the stage is off),
    ``radiation_length`` [m] and ``electron_density`` [1/m^3] (finite, > 0; None: from the run's gas target,
    ``radiation_length(target)`` / ``electron_density(target)``), ``stream`` (an integer in [0, 2^16): another stream,
    other kicks)."""

    slot, call = "straggling", "attpc_det_configure_straggling"

    def __init__(self, angular_scale: float = 1.0, energy_scale: float = 1.0, radiation_length: float | None = None,
                 electron_density: float | None = None, stream: int = 0):
        self.angular_scale = _number("angular_scale", angular_scale)
        self.energy_scale = _number("energy_scale", energy_scale)
        for what in ("angular_scale", "energy_scale"):
            value = getattr(self, what)
            if not (value >= 0.0 and math.isfinite(value)):
                raise ValueError(f"straggling {what} must be finite and >= 0, got {value}")
        self.radiation_length = None if radiation_length is None else _number("radiation_length", radiation_length)
        self.electron_density = None if electron_density is None else _number("electron_density", electron_density)
        for what in ("radiation_length", "electron_density"):
            value = getattr(self, what)
            if value is not None and not (value > 0.0 and math.isfinite(value)):
                raise ValueError(f"straggling {what} must be finite and > 0, got {value}")
        if isinstance(stream, (bool, np.bool_)) or not isinstance(stream, (int, np.integer)) or not 0 <= int(stream) < 1 << 16:
            raise ValueError(f"straggling stream must be an integer in [0, 2^16), got {stream!r}")
        self.stream = int(stream)

    @property
    def on(self) -> bool:
        return self.angular_scale > 0.0 or self.energy_scale > 0.0

    def resolved(self, target=None) -> "StragglingSettings":
        """The same settings with the radiation length and the electron density filled in from ``target`` where they
        are None.  ValueError if one is missing and the target cannot give it."""
        if self.radiation_length is not None and self.electron_density is not None:
            return self
        return StragglingSettings(
            self.angular_scale, self.energy_scale,
            radiation_length(target) if self.radiation_length is None else self.radiation_length,
            electron_density(target) if self.electron_density is None else self.electron_density, self.stream)

    def token(self):
        """None: settings that change nothing (both scales 0), the stage off."""
        if not self.on:
            return None
        if self.radiation_length is None or self.electron_density is None:
            raise ValueError("unresolved StragglingSettings: call resolved(target) first")
        return (self.angular_scale, self.energy_scale, self.radiation_length, self.electron_density, self.stream)

    def desc(self) -> _abi.StraggleDesc:
        return _abi.StraggleDesc(*self.token())


def _checked(straggling):
    if straggling is not None and not isinstance(straggling, StragglingSettings):
        raise TypeError(f"straggling must be a StragglingSettings or None, got {type(straggling).__name__}")
    return straggling


def configure_straggling(ctx: _abi.Context, straggling: StragglingSettings | None, config=None) -> None:
    """``attpc_det_configure_straggling`` unless this ctx already holds the same settings (``None``, or both scales 0:
    the stage off).  ``config``: the run's Config, whose gas target gives a radiation length or an electron density the
    settings leave open."""
    straggling = _checked(straggling)
    if straggling is not None and straggling.on:
        straggling = straggling.resolved(None if config is None else config.det_params.gas_target)
    configure_stage(ctx, StragglingSettings, straggling)
