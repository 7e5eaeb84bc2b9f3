"""What every trace stage shares, and nothing of any one stage: how a settings object is applied to a context
(``configure_stage``), the type check of a stage's value (``checked``), the check of host rows in CSR form
(``host_rows``) and the event layout of a host-row operator (``layout``).  The stage modules and ``detector.traces``
import from here; this module imports none of them."""
from __future__ import annotations

import numpy as np

from .. import _abi


def configure_stage(ctx: _abi.Context, stage, settings) -> None:
    """``lib.<stage.call>`` with the descriptor of ``settings`` (an instance of the settings class ``stage``) unless the
    ctx's ``stage.slot`` already holds the same content; None, or settings that change nothing (``token()`` None): the
    stage off, a NULL descriptor, which is also what a new context holds."""
    token = None if settings is None else settings.token()
    ctx.configure(stage.slot, token, stage.call, None if token is None else settings.desc())


def checked(cls, value, name: str):
    """``value`` if it is None or a ``cls``; TypeError otherwise (``name``: the keyword it was given as)."""
    if value is not None and not isinstance(value, cls):
        article = "an" if cls.__name__[0] in "AEIOU" else "a"
        raise TypeError(f"{name} must be {article} {cls.__name__} or None, got {type(value).__name__}")
    return value


def host_rows(offsets, rows, labels, optional_labels: bool = False):
    """Host rows in CSR form as the host-row operators take them, checked: (offsets [n+1] i64, rows [R,8] f64, labels
    [R] i64 -- None stays None with ``optional_labels`` --, n events).  ValueError for offsets that are not n + 1
    non-decreasing row numbers >= 0 and for rows and labels that do not hold the rows the offsets name."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    if offsets.ndim != 1 or len(offsets) < 1 or np.any(np.diff(offsets) < 0) or offsets[0] < 0:
        raise ValueError("offsets must be n + 1 non-decreasing row numbers >= 0")
    rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 8)
    if labels is not None or not optional_labels:
        labels = np.ascontiguousarray(labels, dtype=np.int64).reshape(-1)
    given = "" if labels is None else f" {len(labels)} labels,"
    if (labels is not None and len(rows) != len(labels)) or int(offsets[-1]) > len(rows):
        raise ValueError(f"{len(rows)} rows,{given} offsets up to {int(offsets[-1])}")
    return offsets, rows, labels, len(offsets) - 1


def layout(indices, species_of_row=None) -> _abi.EventLayout:
    """The event layout of a host-row operator: an ``_abi.EventLayout`` as it is, else one of the track positions
    ``indices`` (the nucleus of every position), with ``species_of_row`` the species table of every nucleus row (-1
    beyond those given) for the operators that read it."""
    if isinstance(indices, _abi.EventLayout):
        return indices
    indices = [int(i) for i in indices]
    if len(indices) > _abi.MAX_SIM or any(not 0 <= i < _abi.MAX_ROWS for i in indices):
        raise ValueError(f"indices must be at most {_abi.MAX_SIM} rows in 0 .. {_abi.MAX_ROWS - 1}, got {indices}")
    made = _abi.EventLayout()
    made.n_rows, made.n_sim = _abi.MAX_ROWS, len(indices)
    for s, i in enumerate(indices):
        made.indices[s] = i
    if species_of_row is not None:
        species = [int(v) for v in species_of_row]
        if len(species) > _abi.MAX_ROWS:
            raise ValueError(f"species_of_row holds at most {_abi.MAX_ROWS} rows")
        for row in range(_abi.MAX_ROWS):
            made.species_of_row[row] = species[row] if row < len(species) else -1
    return made
