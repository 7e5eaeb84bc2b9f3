"""The records a trace or trace-row call leaves for the ``attpc_*_last`` readers (csrc/abi.hip): the nine per-event
streams -- trigger, estimates, fits, pid, reaction, cluster events and records, join events and records -- with the
reaction spectra and the cluster labels beside them.  Needs a real MI355X: run with ``-m gpu``.

Nothing here looks at what a record says (the stages' own tests do): the comparisons are of bytes, between two ways of
making or reading the same call, and of which call a reader answers for; there is no tolerance."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector.clustering import CLUSTER_DTYPE, CLUSTER_EVENT_DTYPE, ClusterSettings
from attpc_engine_amd.detector.fit import TrackFitSettings
from attpc_engine_amd.detector.joining import JOIN_DTYPE, JOIN_EVENT_DTYPE, JoinSettings
from attpc_engine_amd.detector.luts import build_layout
from attpc_engine_amd.detector.pid import Gate
from attpc_engine_amd.detector.reaction import REACTION_DTYPE
from attpc_engine_amd.detector.traces import TriggerSettings
from tests.helpers import Inputs
from tests.test_gpu_join import ESTIMATES, PARTIAL, PEAKS, THINNING
from tests.test_gpu_reaction import FIT

pytestmark = pytest.mark.gpu

C = _abi.C
SEED, FIRST = 36, (1 << 32) - 20
TRIGGER = TriggerSettings(25, window=50, group_multiplicity=60)  # (ungated)
EVERYTHING = Gate.rectangle((1e-30, 1e30), (1e-30, 1e30))
# the nine per-event streams: name -> (records per event: 1, n_sim ("sim") or ATTPC_MAX_SIM, dtype, ctypes struct) ...
STREAMS = {"trigger": (1, _abi.TRIGGER_DTYPE, _abi.TriggerRecord), "estimates": ("sim", _abi.ESTIMATE_DTYPE, _abi.TrackEstimate),
           "fits": ("sim", _abi.FIT_DTYPE, _abi.TrackFit), "pid": ("sim", _abi.PID_DTYPE, _abi.PidRecord),
           "reaction": (1, REACTION_DTYPE, _abi.ReactionRecord), "cluster_events": (1, CLUSTER_EVENT_DTYPE, _abi.ClusterEvent),
           "cluster_records": (_abi.MAX_SIM, CLUSTER_DTYPE, _abi.ClusterRecord), "join_events": (1, JOIN_EVENT_DTYPE, _abi.JoinEvent),
           "join_records": (_abi.MAX_SIM, JOIN_DTYPE, _abi.JoinRecord)}
# ... and the nine readers (attpc_<name>_last)
READERS = ("trigger", "clusters", "cluster_labels", "joins", "estimates", "fits", "pid", "reaction", "reaction_spectra")


class Setup:
    """be10dp in partial readout with noise on a context of its own, every stage behind the trace rows that leaves
    records configured by ``on()`` and removed by ``off()``."""

    def __init__(self):
        from attpc_engine_amd.detector.response import get_response
        from attpc_engine_amd.engine import Engine

        self.ctx = _abi.Context(0)
        self.inp = Inputs("be10dp")
        self.eng = Engine(self.inp.pipeline, self.inp.config, self.inp.indices, context=self.ctx)
        self.eng.configure_traces(self.inp.config, offset=int(np.argmax(get_response(self.inp.config))), **PARTIAL)
        self.eng.configure_peaks(PEAKS)
        self.n_sim = len(self.inp.indices)
        self.reaction = None

    def on(self, join=True, thinning=True, fit=True, pid=True, source="fit"):
        eng = self.eng
        eng.configure_trigger(TRIGGER)
        eng.configure_clustering(ClusterSettings(match="truth"))
        eng.configure_cluster_join(JoinSettings() if join else None)
        eng.configure_estimates(ESTIMATES)
        eng.configure_thinning(THINNING if thinning else None)
        eng.configure_track_fit(TrackFitSettings(**FIT) if fit else None)
        eng.configure_pid([EVERYTHING] * self.n_sim if pid else None)
        eng.configure_reaction(track=0, source=source, ex_range=(-4.0, 12.0), ex_bins=64, theta_bins=36)
        self.reaction = eng._reaction

    def off(self):
        eng = self.eng
        eng.configure_trigger()
        eng.configure_clustering()
        eng.configure_cluster_join()
        eng.configure_estimates()
        eng.configure_thinning()
        eng.configure_track_fit()
        eng.configure_pid()
        eng.configure_reaction()

    def chunk_events(self, n):
        self.ctx.check(self.ctx.lib.attpc_set_chunk_events(self.ctx.handle, n), "attpc_set_chunk_events")

    def read(self, first, count, n_cells=None):
        """Every reader once over events first .. first + count -> ({reader: its status}, {stream: its bytes, and
        "spectra": the cells' bytes})."""
        lib, handle = self.ctx.lib, self.ctx.handle
        per = {name: self.n_sim if how[0] == "sim" else how[0] for name, how in STREAMS.items()}
        a = {name: np.zeros((count, per[name]), dtype=how[1]) for name, how in STREAMS.items()}
        p = {name: _abi.iptr(a[name], how[2]) for name, how in STREAMS.items()}
        cells = np.zeros(self.reaction.n_cells if n_cells is None else n_cells, dtype=np.uint64)
        rc = {"trigger": lib.attpc_trigger_last(handle, first, count, p["trigger"]),
              "clusters": lib.attpc_clusters_last(handle, first, count, p["cluster_events"], p["cluster_records"]),
              "cluster_labels": lib.attpc_cluster_labels_last(handle, 0, 0, None),
              "joins": lib.attpc_joins_last(handle, first, count, p["join_events"], p["join_records"]),
              "estimates": lib.attpc_estimates_last(handle, first, count, p["estimates"]),
              "fits": lib.attpc_fits_last(handle, first, count, p["fits"]),
              "pid": lib.attpc_pid_last(handle, first, count, p["pid"]),
              "reaction": lib.attpc_reaction_last(handle, first, count, p["reaction"]),
              "reaction_spectra": lib.attpc_reaction_spectra_last(handle, cells.size, _abi.iptr(cells, C.c_uint64))}
        assert tuple(sorted(rc)) == tuple(sorted(READERS))
        return rc, {**{name: a[name].tobytes() for name in STREAMS}, "spectra": cells.tobytes()}

    def close(self):
        self.ctx.close()


def _all(status):
    return {reader: status for reader in READERS}


def _slice(whole, n_sim, first, count):
    """Events first .. first + count of the bytes of a read over a whole call."""
    out = {}
    for name, how in STREAMS.items():
        size = (n_sim if how[0] == "sim" else how[0]) * how[1].itemsize
        out[name] = whole[name][first * size:(first + count) * size]
    return out


def test_all_nine_streams_do_not_depend_on_the_chunking():
    """32 events with every stage on, as one chunk and as chunks of 5 over two track batches: the same bytes in every
    stream, read whole or in parts; a range past the call is refused."""
    n = 32
    one, many = Setup(), Setup()
    try:
        one.on()
        one.eng.run_estimates(n, seed=SEED, first_event=FIRST)
        rc, whole = one.read(0, n)
        assert rc == {**_all(_abi.OK), "cluster_labels": _abi.E_NOTCONFIGURED}, rc  # (a resident call fetches no rows)
        assert all(len(whole[name]) > 0 and whole[name] != bytes(len(whole[name])) for name in whole), [len(v) for v in whole.values()]
        # a fresh context's pilot batch is one chunk, the rest of the call another track batch: chunks of 5, 5 x 5 and 2
        many.on()
        many.chunk_events(5)
        chunked = many.eng.run_estimates(n, seed=SEED, first_event=FIRST)
        assert chunked["stats"]["launches_tracks"] >= 2, chunked["stats"]
        rc, got = many.read(0, n)
        assert rc == {**_all(_abi.OK), "cluster_labels": _abi.E_NOTCONFIGURED}, rc
        for name in whole:
            assert got[name] == whole[name], name
        for setup in (one, many):
            for first, count in ((0, 7), (7, 25), (n, 0)):
                rc, part = setup.read(first, count)
                assert rc == {**_all(_abi.OK), "cluster_labels": _abi.E_NOTCONFIGURED}, (first, count, rc)
                want = _slice(whole, setup.n_sim, first, count)
                for name in STREAMS:
                    assert part[name] == want[name], (name, first, count)
                assert part["spectra"] == whole["spectra"]
            rc, _ = setup.read(30, 3)
            for reader in ("trigger", "clusters", "joins", "estimates", "fits", "pid", "reaction"):
                assert rc[reader] == _abi.E_INVALID, (reader, rc)
    finally:
        one.close()
        many.close()


def test_which_call_a_stream_answers_for():
    """A trace call resets the trigger stream alone; a trace-row call resets every stream, whatever it makes itself; a
    spectra-only call leaves the spectra and the trigger records."""
    n = 8
    s = Setup()
    try:
        s.on()
        s.eng.run_estimates(n, seed=SEED, first_event=FIRST)
        rc, first = s.read(0, n)
        assert rc == {**_all(_abi.OK), "cluster_labels": _abi.E_NOTCONFIGURED}, rc
        # a trace call of 5 events: the trigger reader answers for it, the others for the call before
        traces = s.eng.run_traces(5, seed=SEED + 1, first_event=FIRST, fetch=False)
        rc, after = s.read(0, n)
        assert rc == {**_all(_abi.OK), "cluster_labels": _abi.E_NOTCONFIGURED, "trigger": _abi.E_INVALID}, rc
        for name in after:
            assert name == "trigger" or after[name] == first[name], name
        rc, five = s.read(0, 5)
        assert rc["trigger"] == _abi.OK and five["trigger"] == traces["trigger"].tobytes()
        # a trace-row call with every stage off
        s.off()
        s.eng.run_trace_rows(n, seed=SEED, first_event=FIRST, fetch=False)
        rc, _ = s.read(0, n)
        assert rc == _all(_abi.E_NOTCONFIGURED), rc
        # a spectra-only call
        s.on()
        spectra = s.eng.run_spectra(n, seed=SEED, first_event=FIRST)
        rc, only = s.read(0, n)
        assert rc == {**_all(_abi.E_NOTCONFIGURED), "trigger": _abi.OK, "reaction_spectra": _abi.OK}, rc
        assert only["spectra"] == first["spectra"] == spectra["spectra"].cells.tobytes() and only["trigger"] == first["trigger"]
    finally:
        s.close()


def test_a_refused_call_leaves_every_stream_off():
    """A trace-row call that is refused at its start -- here by the reaction reconstruction, whose position ``track`` is
    not ``observed_row`` in the call's layout -- leaves every stream the call would have reset turned off: the nine
    readers answer ATTPC_E_NOTCONFIGURED until the next call that succeeds.  Before the streams were one type with one
    begin, the trigger reader answered ATTPC_OK here with the records of no call, and the cluster and cluster label
    readers answered ATTPC_OK with the records of the call before."""
    n = 8
    s = Setup()
    try:
        s.on(join=False, thinning=False, fit=False, pid=False, source="estimate")  # clustering, trigger, estimates, reaction
        res = s.eng.run_trace_rows(n, seed=SEED, first_event=FIRST)
        good = {**_all(_abi.OK), "joins": _abi.E_NOTCONFIGURED, "fits": _abi.E_NOTCONFIGURED, "pid": _abi.E_NOTCONFIGURED}
        rc, first = s.read(0, n)
        assert rc == good, rc
        swapped = build_layout(s.inp.z, s.inp.a, list(s.inp.indices)[::-1], s.inp.species)
        assert swapped.indices[s.reaction.track] != s.reaction.observed_row
        stats, out = _abi.RunStats(), _abi.CloudOut()
        refused = s.ctx.lib.attpc_det_run_trace_rows(s.ctx.handle, SEED, FIRST, n, swapped, _abi.dptr(res["p4"]), _abi.dptr(res["vertex"]),
                                                     out, stats)
        assert refused == _abi.E_INVALID and b"observed_row" in s.ctx.lib.attpc_last_error(s.ctx.handle)
        rc, _ = s.read(0, n)
        assert rc == _all(_abi.E_NOTCONFIGURED), rc
        again = s.eng.run_trace_rows(n, seed=SEED, first_event=FIRST)
        rc, second = s.read(0, n)
        assert rc == good, rc
        for name in first:
            assert second[name] == first[name], name
        assert again["rows"].tobytes() == res["rows"].tobytes() and np.array_equal(again["cluster_labels"], res["cluster_labels"])
    finally:
        s.close()
