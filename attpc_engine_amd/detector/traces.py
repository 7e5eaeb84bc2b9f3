"""Digitised GET pad traces on the device (EXTENSION: the reference stops at point clouds, its user guide's "Why Point
clouds").  The contract -- integer time bucket of every row, f64 sum of q * R in ascending t without fused multiply-add,
4095 clip of the summed signal, rint half to even, strict ADC threshold on the pad's largest sample, label of the pad's
largest charge -- is written out in include/attpc_engine.h; ``tests/trace_reference.py`` restates it in numpy.

``simulate_batch_traces`` is ``simulate_batch`` with the traces made on the device behind the scatter
(``attpc_det_run_traces``); ``clouds_to_traces`` turns any host cloud into traces (``attpc_traces``).
"""
from __future__ import annotations

import numpy as np

from .. import _abi
from .luts import build_layout, species_for
from .parameters import Config


def trace_settings(config: Config, response=None, threshold=None, offset: int = 0):
    """(response [512] f64, threshold, offset) with the defaults filled in: get_response(config) and
    ``ElectronicsParams.adc_threshold``."""
    from .response import get_response

    response = np.ascontiguousarray(get_response(config) if response is None else response, dtype=np.float64)
    if response.shape != (_abi.NUM_TB,):
        raise ValueError(f"response must have {_abi.NUM_TB} samples, got shape {response.shape}")
    threshold = float(config.elec_params.adc_threshold if threshold is None else threshold)
    return response, threshold, int(offset)


def configure_traces(config: Config, ctx: _abi.Context, response=None, threshold=None, offset: int = 0) -> None:
    """Upload the response, ADC threshold and sample offset of the traces unless this ctx already holds the same ones
    (decided on their content, as configure_spyral)."""
    response, threshold, offset = trace_settings(config, response, threshold, offset)
    token = (response.tobytes(), threshold, offset)
    if getattr(ctx, "_trace_token", None) == token:
        return
    desc = _abi.TraceDesc(_abi.dptr(response), threshold, offset, 0)
    ctx.check(ctx.lib.attpc_trace_configure(ctx.handle, desc), "attpc_trace_configure")
    ctx._trace_token = token


class TraceArrays:
    """Caller arrays of one trace call and the ``attpc_trace_out`` that points at them.  ``make``: allocator
    ``(shape, dtype) -> array`` (page-locked memory for ``Engine.run_traces(pinned=True)``)."""

    def __init__(self, n_events: int, capacity: int, make=None):
        make = make or (lambda shape, dtype: np.empty(shape, dtype=dtype))
        self.offsets = np.zeros(n_events + 1, dtype=np.int64)
        self.pads = make((capacity,), np.int32)
        self.samples = make((capacity, _abi.NUM_TB), np.int16)
        self.labels = make((capacity,), np.int64)
        self.event_points = np.zeros(n_events, dtype=np.int64)
        self.out = _abi.TraceOut(capacity, _abi.iptr(self.offsets, _abi.C.c_int64), _abi.iptr(self.pads, _abi.C.c_int32),
                                 _abi.iptr(self.samples, _abi.C.c_int16), _abi.iptr(self.labels, _abi.C.c_int64),
                                 _abi.iptr(self.event_points, _abi.C.c_int64))

    def sums(self) -> dict:
        return {"n_rows": int(self.out.n_rows), "sample_checksum": int(self.out.sample_checksum),
                "pad_checksum": int(self.out.pad_checksum)}

    def result(self):
        total = int(self.out.n_rows)
        return self.offsets, self.pads[:total], self.samples[:total], self.labels[:total]


def call_with_capacity(ctx: _abi.Context, n_events: int, capacity: int, call, what: str, make=None) -> TraceArrays:
    """Run ``call(out)`` with arrays of ``capacity`` rows; on ATTPC_E_CAPACITY once more with the exact row count."""
    while True:
        arrays = TraceArrays(n_events, max(1, int(capacity)), make)
        status = call(arrays.out)
        if status == _abi.E_CAPACITY and arrays.out.n_rows > capacity:
            capacity = int(arrays.out.n_rows)
            continue
        ctx.check(status, what)
        return arrays


def simulate_batch_traces(momenta: np.ndarray, vertices: np.ndarray, proton_numbers, mass_numbers, config: Config,
                          seed: int, indices: list[int], first_event: int = 0, ctx: _abi.Context | None = None,
                          response=None, threshold=None, offset: int = 0, capacity_per_event: int = 1024):
    """simulate() + the pad traces of every event, on the device (``attpc_det_run_traces``) ->
    (offsets [n+1], pads [R] i32, samples [R,512] i16, labels [R] i64, event_points [n] = cloud rows of every event
    before the suppression, stats dict: the cloud's run statistics plus ``n_rows`` / ``sample_checksum`` /
    ``pad_checksum`` of the traces)."""
    from .simulator import configure_detector

    ctx = ctx or _abi.default_context()
    momenta = np.ascontiguousarray(momenta, dtype=np.float64)
    vertices = np.ascontiguousarray(vertices, dtype=np.float64)
    n = momenta.shape[0]
    seed, first_event, n = _abi.check_id_range(seed, first_event, n)
    keys = species_for(proton_numbers, mass_numbers, indices)
    configure_detector(config, keys, ctx)
    configure_traces(config, ctx, response, threshold, offset)
    layout = build_layout(proton_numbers, mass_numbers, indices, keys)
    stats = _abi.RunStats()

    def call(out):
        return ctx.lib.attpc_det_run_traces(ctx.handle, int(seed), int(first_event), n, layout, _abi.dptr(momenta),
                                            _abi.dptr(vertices), out, stats)

    arrays = call_with_capacity(ctx, n, max(1024, int(capacity_per_event) * n), call, "attpc_det_run_traces")
    offsets, pads, samples, labels = arrays.result()
    return offsets, pads, samples, labels, arrays.event_points, {**stats.as_dict(), **arrays.sums()}


def clouds_to_traces(offsets: np.ndarray, points: np.ndarray, labels: np.ndarray, ctx: _abi.Context):
    """Pad traces of any host cloud in CSR form (``attpc_traces``; ``ctx`` configured with ``configure_traces``):
    offsets [n+1], points [P,3] (pad, time bucket, electrons), labels [P] ->
    (offsets [n+1], pads [R] i32, samples [R,512] i16, labels [R] i64, {n_rows, sample_checksum, pad_checksum}),
    the pad checksum taken over the events' indices 0 .. n-1."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    labels = np.ascontiguousarray(labels, dtype=np.int64)
    n = len(offsets) - 1
    if n < 0:
        raise ValueError("offsets needs n_events + 1 entries")
    if len(points) != len(labels) or (n and offsets[-1] > len(points)):
        raise ValueError("points / labels do not hold the rows the offsets name")

    def call(out):
        return ctx.lib.attpc_traces(ctx.handle, n, _abi.iptr(offsets, _abi.C.c_int64), _abi.dptr(points),
                                    _abi.iptr(labels, _abi.C.c_int64), out)

    rows = int(offsets[-1] - offsets[0]) if n else 0
    arrays = call_with_capacity(ctx, n, max(16, rows), call, "attpc_traces")
    return (*arrays.result(), arrays.sums())
