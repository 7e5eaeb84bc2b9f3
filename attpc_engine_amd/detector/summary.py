"""Event and track summaries of a device-resident run (EXTENSION: the reference hands out point clouds only).

What acceptance and efficiency studies ask of a million events -- how many cloud rows survive the ADC threshold, how
many pads they light, over which time buckets, how far out on the pad plane, how much charge, where the track ended --
is a small reduction over every event's cloud and track samples.  A summary run makes it on the device, behind the
scatter of every chunk and on the rows where they lie: one fixed-size record per event and one per (event, simulated
nucleus) cross the link instead of the cloud.  The contract is written out in include/attpc_engine.h;
``tests/summary_reference.py`` restates it in numpy.

``simulate_batch_summary`` is ``simulate_batch`` with the records instead of the clouds (``attpc_det_run_summary``);
``clouds_to_summary`` reduces any host cloud through the same kernel (``attpc_cloud_summary``, the cloud part only);
``Engine.run_summary`` is the fused run.  A cloud row is *kept* iff its electrons reach ``min_electrons``; the default,
``electrons_above_threshold(config)``, makes that "survives the ADC threshold as a Spyral row".
"""
from __future__ import annotations

import numpy as np

from .. import _abi
from ..outputs import SummaryArrays
from .parameters import Config

NEVER_KEPT = 1 << 62  # a min_electrons above any charge a cloud row can carry


def electrons_above_threshold(config: Config, response=None) -> int:
    """The smallest integer ``q`` with ``min(r_max * q, 4095.0) > adc_threshold`` in f64, ``r_max`` the largest sample
    of the response (default get_response(config)): the charge from which a cloud row survives the ADC threshold as a
    Spyral row (the rule of the device's Spyral write pass and writer.py:232-234).  ``NEVER_KEPT`` when no charge does
    (4095 does not exceed the threshold, or the response is all zero)."""
    from .response import get_response

    response = np.asarray(get_response(config) if response is None else response, dtype=np.float64)
    r_max = float(response.max())
    thr = float(config.elec_params.adc_threshold)

    def above(q: int) -> bool:
        return min(r_max * float(q), 4095.0) > thr

    if above(0):
        return 0
    if not (4095.0 > thr) or not (r_max > 0.0):
        return NEVER_KEPT
    q = max(int(thr / r_max), 1)
    while q > 1 and above(q - 1):
        q -= 1
    while not above(q):
        q += 1
    return q


class SummarySettings:
    """The validated settings of a summary configuration: ``min_electrons`` (an integer >= 0; None = the default of
    ``config``, ``electrons_above_threshold``) and the pad centres [n_pads, 2] of ``config`` (n_pads >= ATTPC_NUM_PADS)."""

    def __init__(self, min_electrons: int | None = 0, config: Config | None = None):
        if min_electrons is None:
            if config is None:
                raise ValueError("the default min_electrons needs a config")
            min_electrons = electrons_above_threshold(config)
        if int(min_electrons) != min_electrons or not 0 <= int(min_electrons) < 1 << 63:
            raise ValueError(f"min_electrons must be an integer in [0, 2^63), got {min_electrons}")
        self.min_electrons = int(min_electrons)
        self.centers = None
        if config is not None:
            if config.pad_centers is None:
                raise ValueError("Pad centers are not assigned: the summary needs them for rho2_max")
            self.centers = np.ascontiguousarray(config.pad_centers, dtype=np.float64)
            if self.centers.ndim != 2 or self.centers.shape[1] != 2 or len(self.centers) < _abi.NUM_PADS:
                raise ValueError(f"pad_centers must be [n_pads >= {_abi.NUM_PADS}, 2], got shape {self.centers.shape}")

    def token(self):
        return (self.min_electrons, None if self.centers is None else self.centers.tobytes())


def configure_summary(config: Config, ctx: _abi.Context, min_electrons: int | None = None) -> SummarySettings:
    """``attpc_summary_configure`` unless this ctx already holds the same settings (decided on their content):
    ``min_electrons`` (None: ``electrons_above_threshold(config)``) and the pad centres of ``config``."""
    settings = SummarySettings(min_electrons, config)
    desc = _abi.SummaryDesc(settings.min_electrons, _abi.dptr(settings.centers), len(settings.centers), 0)
    ctx.configure("summary", settings.token(), "attpc_summary_configure", desc)
    return settings


def simulate_batch_summary(momenta: np.ndarray, vertices: np.ndarray, proton_numbers, mass_numbers, config: Config,
                           seed: int, indices: list[int], first_event: int = 0, ctx: _abi.Context | None = None,
                           min_electrons: int | None = None, straggling=None, distortion=None):
    """simulate() for n events with the clouds left on the device and reduced there (``attpc_det_run_summary``) ->
    (events [n] structured, tracks [n, n_sim] structured, stats dict: the cloud's run statistics).  ``straggling`` (a
    ``detector.straggling.StragglingSettings``; None = off): the track straggling.  ``distortion`` (a
    ``detector.distortion.DistortionMap``; None = off): the drift distortion -- the tracks' end points are then the
    shifted, apparent ones."""
    from .simulator import run_batch

    SummarySettings(min_electrons, config)  # (validated before the first library call)
    arrays, stats = run_batch("attpc_det_run_summary", momenta, vertices, proton_numbers, mass_numbers, config, seed,
                              list(indices), first_event, ctx, 0,
                              configure=lambda c: configure_summary(config, c, min_electrons) and None,
                              straggling=straggling, distortion=distortion, holder=SummaryArrays, n_sim=len(indices))
    return (*arrays.result(), stats.as_dict())


def clouds_to_summary(offsets: np.ndarray, points: np.ndarray, labels: np.ndarray, indices: list[int],
                      ctx: _abi.Context, n_rows: int | None = None):
    """The cloud part of the records for any host cloud in CSR form (``attpc_cloud_summary``; ``ctx`` configured with
    ``configure_summary``): offsets [n+1], points [P,3] (pad, time bucket, electrons), labels [P]; ``indices``: the
    labels of the track records, in order (``n_rows``: nuclei per event, default max(indices) + 1) ->
    (events [n] structured, tracks [n, len(indices)] structured, their track part empty)."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    labels = np.ascontiguousarray(labels, dtype=np.int64)
    n = len(offsets) - 1
    if n < 0:
        raise ValueError("offsets needs n_events + 1 entries")
    if len(points) != len(labels) or (n and offsets[-1] > len(points)):
        raise ValueError("points / labels do not hold the rows the offsets name")
    indices = [int(i) for i in indices]
    if len(indices) > _abi.MAX_SIM:
        raise ValueError(f"at most {_abi.MAX_SIM} indices, got {len(indices)}")
    layout = _abi.EventLayout()
    layout.n_rows = int(n_rows) if n_rows is not None else max(indices, default=0) + 1
    layout.n_sim = len(indices)
    for s, row in enumerate(indices):
        layout.indices[s] = row
    arrays = SummaryArrays(n, n_sim=len(indices))
    ctx.check(ctx.lib.attpc_cloud_summary(ctx.handle, n, _abi.iptr(offsets, _abi.C.c_int64), _abi.dptr(points),
                                          _abi.iptr(labels, _abi.C.c_int64), layout, arrays.out), "attpc_cloud_summary")
    return arrays.result()
