"""Caller-side output arrays of a delivered run, and the one capacity retry over them.

A run that delivers clouds, Spyral rows or pad traces writes into arrays the caller owns (``attpc_cloud_out`` /
``attpc_trace_out``, include/attpc_engine.h) and answers ATTPC_E_CAPACITY, with the rows it needs, when they are too
small.  ``RowArrays``, ``TraceArrays`` and ``PackedTraceArrays`` (the rows as packed records, ``attpc_trace_packed_out``) hold such arrays together with the struct that points at them (``SummaryArrays``: the
fixed-size records of a summary run, ``attpc_summary_out``, which have no capacity; ``SelectedArrays``: the rows of the
events that pass a selection, ``passed`` and the records of all events, ``attpc_select_out``);
``call_with_capacity`` is the only place that allocates them, calls and allocates again.
"""
from __future__ import annotations

import numpy as np

from . import _abi


def _host_empty(shape, dtype):
    return np.empty(shape, dtype=dtype)


class RowArrays:
    """Caller arrays of one cloud (``width`` 3) or Spyral row (``width`` 8) call and the ``attpc_cloud_out`` that
    points at them.  ``make`` as for TraceArrays; ``event_points=False`` hands the library NULL there."""

    def __init__(self, n_events: int, capacity: int, make=None, width: int = 3, event_points: bool = True):
        make = make or _host_empty
        self.offsets = np.zeros(n_events + 1, dtype=np.int64)
        self.rows = make((capacity, width), np.float64)
        self.labels = make((capacity,), np.int64)
        self.event_points = np.zeros(n_events, dtype=np.int64) if event_points else None
        self.out = _abi.CloudOut(capacity, _abi.iptr(self.offsets, _abi.C.c_int64), _abi.dptr(self.rows),
                                 _abi.iptr(self.labels, _abi.C.c_int64), _abi.iptr(self.event_points, _abi.C.c_int64))

    def needed(self, stats) -> int:
        """Rows the last call wanted to deliver: a cloud call reports them in its run statistics."""
        return int(stats.n_points)

    def result(self):
        total = int(self.offsets[-1])
        return self.offsets, self.rows[:total], self.labels[:total]


class TraceArrays:
    """Caller arrays of one trace call and the ``attpc_trace_out`` that points at them.  ``make``: allocator
    ``(shape, dtype) -> array`` (page-locked memory for ``Engine.run_traces(pinned=True)``)."""

    def __init__(self, n_events: int, capacity: int, make=None):
        make = make or _host_empty
        self.offsets = np.zeros(n_events + 1, dtype=np.int64)
        self.pads = make((capacity,), np.int32)
        self.samples = make((capacity, _abi.NUM_TB), np.int16)
        self.labels = make((capacity,), np.int64)
        self.event_points = np.zeros(n_events, dtype=np.int64)
        self.out = _abi.TraceOut(capacity, _abi.iptr(self.offsets, _abi.C.c_int64), _abi.iptr(self.pads, _abi.C.c_int32),
                                 _abi.iptr(self.samples, _abi.C.c_int16), _abi.iptr(self.labels, _abi.C.c_int64),
                                 _abi.iptr(self.event_points, _abi.C.c_int64))

    def needed(self, stats) -> int:
        """Rows the last call wanted to deliver: a trace call reports them in its own out struct."""
        return int(self.out.n_rows)

    def sums(self) -> dict:
        return {"n_rows": int(self.out.n_rows), "sample_checksum": int(self.out.sample_checksum),
                "pad_checksum": int(self.out.pad_checksum)}

    def result(self):
        total = int(self.out.n_rows)
        return self.offsets, self.pads[:total], self.samples[:total], self.labels[:total]


class PackedTraceArrays:
    """Caller arrays of one packed trace call (``attpc_trace_packed_out``): TraceArrays with ``row_start`` [capacity + 1]
    and ``packed`` [byte_capacity] uint8 in the place of the samples.  ``byte_capacity`` is the call's second capacity
    (``needed_shape``)."""

    def __init__(self, n_events: int, capacity: int, make=None, byte_capacity: int = 0):
        make = make or _host_empty
        byte_capacity = max(8, int(byte_capacity))
        self.offsets = np.zeros(n_events + 1, dtype=np.int64)
        self.pads = make((capacity,), np.int32)
        self.row_start = make((capacity + 1,), np.int64)
        self.packed = make((byte_capacity,), np.uint8)
        self.labels = make((capacity,), np.int64)
        self.event_points = np.zeros(n_events, dtype=np.int64)
        i64 = _abi.C.c_int64
        self.out = _abi.TracePackedOut(capacity, _abi.iptr(self.offsets, i64), _abi.iptr(self.pads, _abi.C.c_int32),
                                       _abi.iptr(self.row_start, i64), _abi.iptr(self.packed, _abi.C.c_uint8), byte_capacity,
                                       _abi.iptr(self.labels, i64), _abi.iptr(self.event_points, i64))

    def needed(self, stats) -> int:
        return int(self.out.n_rows)

    def needed_shape(self, stats) -> dict:
        """What the last call wanted of the capacities beside the rows."""
        return {"byte_capacity": int(self.out.n_bytes)}

    def sums(self) -> dict:
        return {"n_rows": int(self.out.n_rows), "n_bytes": int(self.out.n_bytes),
                "sample_checksum": int(self.out.sample_checksum), "pad_checksum": int(self.out.pad_checksum)}

    def result(self):
        total, n_bytes = int(self.out.n_rows), int(self.out.n_bytes)
        return self.offsets, self.pads[:total], self.row_start[:total + 1], self.packed[:n_bytes], self.labels[:total]


class SummaryArrays:
    """Caller arrays of one summary call -- ``events`` [n] and ``tracks`` [n, n_sim], structured
    (``_abi.EVENT_SUMMARY_DTYPE`` / ``_abi.TRACK_SUMMARY_DTYPE``) -- and the ``attpc_summary_out`` that points at them.
    The sizes are known: ``capacity`` plays no part and ATTPC_E_CAPACITY never comes."""

    def __init__(self, n_events: int, capacity: int = 0, make=None, n_sim: int = 0):
        make = make or _host_empty
        self.events = make((n_events,), _abi.EVENT_SUMMARY_DTYPE)
        self.tracks = make((n_events, n_sim), _abi.TRACK_SUMMARY_DTYPE)
        self.out = _abi.SummaryOut(self.events.ctypes.data_as(_abi.C.POINTER(_abi.EventSummary)),
                                   self.tracks.ctypes.data_as(_abi.C.POINTER(_abi.TrackSummary)))

    def needed(self, stats) -> int:
        return 0

    def result(self):
        return self.events, self.tracks


class SelectedArrays:
    """Caller arrays of one selected call -- the row arrays of its kind (``width`` 3: cloud rows, 8: Spyral rows),
    ``passed`` [n] u8 and the records of all events (``events`` [n], ``tracks`` [n, n_sim], as in SummaryArrays) -- and
    the ``attpc_select_out`` that points at them.  ``rows=False``: no row arrays (the library gets NULL there, copies
    nothing of the rows and still reports what the selection would deliver)."""

    def __init__(self, n_events: int, capacity: int, make=None, width: int = 3, n_sim: int = 0, rows: bool = True):
        make = make or _host_empty
        self.offsets = np.zeros(n_events + 1, dtype=np.int64)
        self.rows = make((capacity, width), np.float64) if rows else None
        self.labels = make((capacity,), np.int64) if rows else None
        self.event_points = np.zeros(n_events, dtype=np.int64)
        self.passed = np.zeros(n_events, dtype=np.uint8)
        self.events = np.empty((n_events,), _abi.EVENT_SUMMARY_DTYPE)
        self.tracks = np.empty((n_events, n_sim), _abi.TRACK_SUMMARY_DTYPE)
        i64 = _abi.C.c_int64
        self.out = _abi.SelectOut(_abi.SELECT_SPYRAL if width == 8 else _abi.SELECT_CLOUD, 0, capacity,
                                  _abi.iptr(self.offsets, i64), _abi.dptr(self.rows), _abi.iptr(self.labels, i64),
                                  _abi.iptr(self.event_points, i64), _abi.iptr(self.passed, _abi.C.c_uint8),
                                  self.events.ctypes.data_as(_abi.C.POINTER(_abi.EventSummary)),
                                  self.tracks.ctypes.data_as(_abi.C.POINTER(_abi.TrackSummary)), 0, 0)

    def needed(self, stats) -> int:
        """Rows the last call wanted to deliver: the selected rows, which the call reports in its own out struct
        (the run statistics keep the cloud's rows of all events)."""
        return int(self.out.n_rows)

    def result(self):
        total = int(self.offsets[-1])
        if self.rows is None:
            return self.offsets, None, None
        return self.offsets, self.rows[:total], self.labels[:total]


def call_with_capacity(ctx: _abi.Context, n_events: int, capacity: int, call, what: str, stats=None,
                       holder=TraceArrays, slack: int = 0, pinned: bool = False, cache=None, reuse: bool = False, **shape):
    """Run ``call(out)`` with ``holder(n_events, capacity, **shape)`` arrays; on ATTPC_E_CAPACITY once more with the
    rows the call reported (``holder.needed(stats)``, ``stats`` the RunStats that ``call`` fills) plus ``slack`` -- and,
    for a holder with further capacities among ``shape`` (``needed_shape(stats)``: PackedTraceArrays' byte_capacity),
    with those it reported.
    ``pinned``: the row arrays in page-locked memory (PCIe-rate copies).  ``cache``: an object whose ``_out_cache``
    attribute keeps the arrays, if ``reuse``, for its next call of the same shape -- the previous call's arrays are
    then overwritten -- and is emptied otherwise; assigning None to the attribute drops them.  Returns the holder of
    the call that went through."""
    make = ctx.pinned_empty if pinned else None
    while True:
        capacity = max(1, int(capacity))
        key = (holder, n_events, capacity, pinned, *sorted(shape.items()))
        cached = cache._out_cache if reuse else None
        if cached is not None and cached[0] == key:
            arrays = cached[1]
        else:
            arrays = holder(n_events, capacity, make, **shape)
            if cache is not None:
                cache._out_cache = (key, arrays) if reuse else None
        status = call(arrays.out)
        more = {}
        if status == _abi.E_CAPACITY and hasattr(arrays, "needed_shape"):
            more = {name: need for name, need in arrays.needed_shape(stats).items() if need > shape.get(name, 0)}
        if status == _abi.E_CAPACITY and (arrays.needed(stats) > capacity or more):
            capacity = max(capacity, arrays.needed(stats) + slack if arrays.needed(stats) > capacity else 0)
            shape.update(more)
            continue
        ctx.check(status, what)
        return arrays
