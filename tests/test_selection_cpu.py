"""Selected delivery, host side (no GPU): the header's declarations and struct layouts against their ctypes mirrors, the
exported symbols, ``Selection`` validation, ``Selection.passes`` against the independent restatement
(tests/selection_reference.py) on hand-made records with written-out answers, the Python run layer through a recording
stand-in library (calls made, configure memoised on content, the capacity retry on ``n_rows``), ``run_fused`` /
``run_simulation`` with a selection, and the generated code of the new kernels (no scratch, no fused multiply-add)."""
import ctypes as C
import math
import re
import subprocess
import sys
import tempfile
import warnings
from pathlib import Path

import numpy as np
import pytest

from attpc_engine_amd import _abi, workloads
from tests.isa_tools import device_code_objects, disassemble_objects, llvm_tool
from tests.selection_reference import hand_made_cases, passes, records, selection_of

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "attpc_engine_amd" / "_lib" / "libattpc_hip.so"
ENTRY_POINTS = ("attpc_select_configure", "attpc_sim_run_selected", "attpc_det_run_selected", "attpc_cloud_select")


# ---------------------------------------------------------------- header, layouts, symbols ----
def test_header_declares_the_entry_points_and_structs():
    header = (ROOT / "include" / "attpc_engine.h").read_text()
    for name in ENTRY_POINTS:
        assert re.search(rf"ATTPC_API int32_t {name}\(", header), name
    for name in ("attpc_select_desc", "attpc_select_out"):
        assert re.search(rf"typedef struct {name} \{{", header), name
    assert "#define ATTPC_ABI_VERSION 3" in header and _abi.ABI_VERSION == 3
    assert "#define ATTPC_SELECT_CLOUD 0" in header and "#define ATTPC_SELECT_SPYRAL 1" in header
    assert (_abi.SELECT_CLOUD, _abi.SELECT_SPYRAL) == (0, 1)
    assert _abi.SELECT_SYMBOLS == ENTRY_POINTS and "select" in _abi.CONFIGURE_SLOTS


def test_struct_layouts_match_the_header():
    structs = {"attpc_select_desc": _abi.SelectDesc, "attpc_select_out": _abi.SelectOut}
    lines = []
    for name, ctype in structs.items():
        args = ", ".join([f"sizeof({name})"] + [f"offsetof({name}, {field})" for field, _ in ctype._fields_])
        lines.append(f' printf("{" ".join(["%zu"] * (1 + len(ctype._fields_)))}\\n", {args});')
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "attpc_engine.h"\nint main(void){\n' + "\n".join(lines) +
           '\n return 0; }\n')
    with tempfile.TemporaryDirectory() as tmp:
        c = Path(tmp) / "t.c"
        c.write_text(src)
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(c), "-o", str(Path(tmp) / "t")], check=True)
        out = subprocess.run([str(Path(tmp) / "t")], capture_output=True, text=True, check=True).stdout.splitlines()
    for line, (name, ctype) in zip(out, structs.items()):
        want = [int(v) for v in line.split()]
        assert want == [C.sizeof(ctype)] + [getattr(ctype, f).offset for f, _ in ctype._fields_], name
        assert want[0] % 8 == 0, name
    assert C.sizeof(_abi.SelectDesc) == 120 and C.sizeof(_abi.SelectOut) == 88


def test_library_exports_the_entry_points():
    import __graft_entry__ as entry

    entry.build()
    lib = _abi.load_library()
    assert lib.attpc_version() == 3
    for name in ENTRY_POINTS:
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(lib, name), name
    nm = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], capture_output=True, text=True, check=True).stdout
    for name in ENTRY_POINTS:
        assert re.search(rf" T {name}$", nm, re.M), name


# ---------------------------------------------------------------- Selection: validation, descriptor, predicate ----
def test_selection_validation():
    from attpc_engine_amd.detector.selection import Selection

    for bad in (dict(n_pads=(5, 4)), dict(charge=(1, 0)), dict(tb_span=(3, 2)), dict(track_rho2_max=(1.0, 0.5)),
                dict(track_end_tb=(math.nan, 1.0)), dict(track_end_rho2=(0.0, math.nan)), dict(track_n_samples=(9, 1)),
                dict(track_mask=0b11, min_tracks=3), dict(min_tracks=1), dict(tracks=[0], min_tracks=2),
                dict(track_mask=1 << _abi.MAX_SIM), dict(tracks=[_abi.MAX_SIM]), dict(tracks=[-1]), dict(track_mask=-1),
                dict(n_kept=(-1, 5)), dict(n_kept=(0, 1 << 32)), dict(n_pads=(1.5, 3)), dict(charge=(0, 1 << 63)),
                dict(n_pads=7)):
        with pytest.raises(ValueError):
            Selection(**bad)
    with pytest.raises(TypeError):
        Selection(pads=(1, 2))
    with pytest.raises(TypeError):
        Selection(tracks=[0], track_mask=1)
    # the descriptor: open values where nothing was said, the mask from the positions, "all" by default
    d = Selection(n_pads=(3, None), charge=(None, 10), tracks=[0, 2], track_end_rho2=(None, 0.0784)).desc()
    assert (d.n_pads_lo, d.n_pads_hi) == (3, (1 << 32) - 1) and (d.n_kept_lo, d.n_kept_hi) == (0, (1 << 32) - 1)
    assert (d.charge_lo, d.charge_hi) == (-(1 << 63), 10) and (d.track_mask, d.min_tracks) == (0b101, 2)
    assert (d.track_end_rho2_lo, d.track_end_rho2_hi) == (-math.inf, 0.0784)
    assert (d.track_end_tb_lo, d.track_end_tb_hi) == (-math.inf, math.inf)
    assert Selection().desc().min_tracks == 0 and Selection(tracks=[1], min_tracks=0).desc().min_tracks == 0
    # the content token: equal settings, equal token
    assert Selection(n_pads=(3, None)).token() == Selection(n_pads=(3, (1 << 32) - 1)).token()
    assert Selection(n_pads=(3, None)).token() != Selection(n_pads=(4, None)).token()
    # positions beyond the records
    ev, tr = records([{}], [[{}]])
    with pytest.raises(ValueError):
        Selection(tracks=[1]).passes(ev, tr)


@pytest.mark.parametrize("case", hand_made_cases(), ids=lambda c: c[0])
def test_passes_on_hand_made_records(case):
    _, events, tracks, cuts, expected = case
    assert passes(events, tracks, cuts).tolist() == expected  # the restatement gives the written-out answer
    got = selection_of(cuts).passes(events, tracks)
    assert got.dtype == bool and got.tolist() == expected


def test_passes_equals_the_restatement_on_random_records():
    rng = np.random.default_rng(11)
    n, n_sim = 400, 3
    ev_list = []
    tr_list = []
    for _ in range(n):
        kept = int(rng.integers(0, 4))
        lo = int(rng.integers(0, 500))
        ev_list.append(dict(n_kept=kept, n_pads=int(rng.integers(0, 6)), tb_min=lo if kept else -1,
                            tb_max=lo + int(rng.integers(0, 6)) if kept else -1, charge=int(rng.integers(-5, 50))))
        tr_list.append([dict(n_kept=int(rng.integers(0, 4)), n_pads=int(rng.integers(0, 4)), n_samples=int(rng.integers(0, 4)),
                             rho2_max=float(rng.choice([-1.0, 0.0, 100.0, 2500.0])),
                             end_x=float(rng.choice([math.nan, 0.1, 0.3])), end_y=float(rng.choice([math.nan, 0.0, 0.4])),
                             end_tb=float(rng.choice([math.nan, 3.0, 400.0]))) for _ in range(n_sim)])
    events, tracks = records(ev_list, tr_list)
    some_passed = 0
    for trial in range(60):
        cuts = dict(track_mask=int(rng.integers(0, 8)))
        cuts["min_tracks"] = int(rng.integers(0, bin(cuts["track_mask"]).count("1") + 1))
        for name, values in (("n_kept", (0, 1, 2, 3)), ("n_pads", (0, 2, 5)), ("tb_span", (0, 1, 3, 6)), ("charge", (-5, 0, 20, 49)),
                             ("track_n_kept", (0, 1, 3)), ("track_n_pads", (0, 1, 3)), ("track_n_samples", (0, 2, 3)),
                             ("track_rho2_max", (-1.0, 0.0, 100.0, 2500.0)), ("track_end_tb", (3.0, 400.0)),
                             ("track_end_rho2", (0.0, 0.01, 0.3 * 0.3 + 0.4 * 0.4))):
            if rng.random() < 0.3:
                lo, hi = sorted(rng.choice(values, 2).tolist())
                cuts[name] = (None if rng.random() < 0.3 else lo, None if rng.random() < 0.3 else hi)
        want = passes(events, tracks, cuts)
        np.testing.assert_array_equal(selection_of(cuts).passes(events, tracks), want, err_msg=str(cuts))
        some_passed += int(0 < want.sum() < n)
    assert some_passed > 10


# ---------------------------------------------------------------- the run layer through a recording stand-in ----
ROWS = (0, 0, 1, 2)      # selected rows of event id % 4, if it passes
POINTS = (0, 5, 6, 7)    # cloud rows of event id % 4 before selection and threshold


def _passes(event_id):
    return event_id % 3 != 0


class RecordingLibrary:
    """Stands in for libattpc_hip.so (the idea of tests/test_run_layer_cpu.py).  ``calls``: (name, scalars, capacity of
    the attpc_select_out or None, names of its NULL pointers).  A selected call delivers ROWS[id % 4] rows for the ids
    with id % 3 != 0; ``refuse = rows``: the next selected call whose capacity is below ``rows`` answers
    ATTPC_E_CAPACITY with n_rows = rows (and stats.n_points = the cloud's rows, which is more)."""

    def __init__(self):
        self.calls = []
        self.refuse = 0

    def __getattr__(self, name):
        if not name.startswith("attpc_"):
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def names(self):
        return [name[len("attpc_"):] for name, *_ in self.calls]

    def of(self, name):
        return [c for c in self.calls if c[0] == "attpc_" + name]

    def _call(self, name, args):
        if name == "attpc_last_error":
            return b"recorded"
        args = args[1:]  # (the context handle)
        out = next((a for a in args if isinstance(a, _abi.SelectOut)), None)
        desc = next((a for a in args if isinstance(a, _abi.SelectDesc)), None)
        scalars = tuple(a for a in args if isinstance(a, (int, float)))
        if desc is not None:
            scalars += (int(desc.n_pads_lo), int(desc.track_mask), int(desc.min_tracks))
        nulls = ()
        if out is not None:
            nulls = tuple(f for f, ctype in out._fields_ if issubclass(ctype, C._Pointer) and not getattr(out, f))
        self.calls.append((name, scalars, None if out is None else int(out.capacity), nulls))
        if out is None:
            return _abi.OK
        _, first, n = args[:3]
        layout = next(a for a in args if isinstance(a, _abi.EventLayout))
        stats = next(a for a in args if isinstance(a, _abi.RunStats))
        width = 8 if out.kind == _abi.SELECT_SPYRAL else 3
        rows = [ROWS[(first + i) % 4] if _passes(first + i) else 0 for i in range(n)]
        stats.n_events = n
        stats.n_points = 1000 + sum(POINTS[(first + i) % 4] for i in range(n))
        out.n_passed = sum(_passes(first + i) for i in range(n))
        out.n_rows = max(self.refuse, sum(rows))
        self.refuse = 0
        row = 0
        for i in range(n):
            out.offsets[i] = row
            out.event_points[i] = POINTS[(first + i) % 4]
            out.passed[i] = int(_passes(first + i))
            out.events[i].n_points = POINTS[(first + i) % 4]
            for s in range(layout.n_sim):
                out.tracks[i * layout.n_sim + s].n_steps = 10 * i + s
            row += rows[i]
        out.offsets[n] = row
        if out.points and out.labels:
            if out.n_rows > out.capacity:
                return _abi.E_CAPACITY
            row = 0
            for i in range(n):
                for _ in range(rows[i]):
                    out.labels[row] = first + i
                    for c in range(width):
                        out.points[row * width + c] = 10.0 * (first + i) + c
                    row += 1
        return _abi.OK


class RecordingContext(_abi.Context):
    def __init__(self):
        saved, _abi._lib = _abi._lib, RecordingLibrary()
        try:
            super().__init__(0)
        finally:
            _abi._lib = saved
        self.lib.calls.clear()
        self.pinned = 0

    def pinned_empty(self, shape, dtype=np.float64):
        self.pinned += 1
        return np.empty(shape, dtype=dtype)


@pytest.fixture(scope="module")
def workload():
    return workloads.o16aa()


def test_engine_run_selected(workload):
    from attpc_engine_amd.detector.selection import Selection
    from attpc_engine_amd.engine import Engine

    pipeline, config, indices = workload
    ctx = RecordingContext()
    eng = Engine(pipeline, config, indices, context=ctx)
    lib = ctx.lib
    lib.calls.clear()
    with pytest.raises(RuntimeError):
        eng.run_selected(4)  # no selection configured
    assert lib.names() == []
    with pytest.raises(ValueError):
        eng.configure_selection(n_pads=(5, 4))  # refused before any library call
    with pytest.raises(ValueError):
        eng.configure_selection(tracks=[len(indices)])  # a position the engine does not simulate
    lib.calls.clear()
    eng._selection = None
    ctx.forget("select")
    eng.configure_selection(n_pads=(3, None), tracks=[0])
    res = eng.run_selected(8, seed=9, first_event=2)
    # summary with its defaults, then the one run call: cloud kind needs no Spyral stage
    assert lib.names() == ["select_configure", "summary_configure", "sim_run_selected"]
    assert lib.calls[0][1] == (3, 1, 1)
    name, scalars, capacity, nulls = lib.calls[2]
    assert scalars == (9, 2, 8) and capacity == 8 * 12288 and nulls == ()
    ids = np.arange(2, 10)
    assert sorted(res) == sorted(["passed", "n_passed", "n_rows", "events", "tracks", "indices", "offsets", "points", "labels",
                                  "event_points", "vertex", "p4", "status", "stats"])
    assert res["passed"].dtype == bool and res["passed"].tolist() == [_passes(i) for i in ids]
    assert res["n_passed"] == sum(_passes(i) for i in ids)
    rows = [ROWS[i % 4] if _passes(i) else 0 for i in ids]
    assert res["n_rows"] == sum(rows) and np.diff(res["offsets"]).tolist() == rows
    assert res["points"].shape == (sum(rows), 3) and res["labels"].tolist() == [i for i, r in zip(ids, rows) for _ in range(r)]
    assert res["event_points"].tolist() == [POINTS[i % 4] for i in ids]
    assert res["events"].dtype == _abi.EVENT_SUMMARY_DTYPE and res["events"]["n_points"].tolist() == [POINTS[i % 4] for i in ids]
    assert res["tracks"].shape == (8, len(indices)) and res["tracks"]["n_steps"][3].tolist() == [30 + s for s in range(len(indices))]
    assert res["indices"] == list(indices) and res["stats"]["n_events"] == 8
    assert res["p4"].shape == (8, eng.n_rows, 4) and res["vertex"].shape == (8, 3) and res["status"].shape == (8,)
    # Spyral rows: the Spyral stage with its defaults, once; the selection and the summary are on the context
    lib.calls.clear()
    res = eng.run_selected(8, seed=9, first_event=2, rows="spyral", pinned=True)
    assert lib.names() == ["spyral_configure", "sim_run_selected"] and lib.calls[1][2] == 8 * 6144
    assert res["rows"].shape == (sum(rows), 8) and "points" not in res and ctx.pinned == 2
    # memoised on content: the same cuts again make no call, other cuts one
    lib.calls.clear()
    eng.configure_selection(Selection(n_pads=(3, (1 << 32) - 1), track_mask=1, min_tracks=1))
    eng.run_selected(2)
    eng.configure_selection(n_pads=(4, None))
    eng.run_selected(2)
    assert lib.names() == ["sim_run_selected", "select_configure", "sim_run_selected"]
    # fetch=False: no row arrays go to the library, everything else comes back
    lib.calls.clear()
    res = eng.run_selected(8, seed=9, first_event=2, fetch=False)
    assert lib.calls[0][3] == ("points", "labels")
    assert res["points"] is None and res["labels"] is None and res["n_rows"] == sum(rows)
    assert res["passed"].tolist() == [_passes(i) for i in ids] and np.diff(res["offsets"]).tolist() == rows
    with pytest.raises(ValueError):
        eng.run_selected(1, rows="traces")
    with pytest.raises(ValueError):
        eng.run_selected(1, seed=-1)


def test_capacity_retry_uses_n_rows(workload):
    from attpc_engine_amd.engine import Engine

    pipeline, config, indices = workload
    ctx = RecordingContext()
    eng = Engine(pipeline, config, indices, context=ctx)
    eng.configure_selection(n_kept=(1, None))
    lib = ctx.lib
    lib.calls.clear()
    lib.refuse = 500_000  # more than the first capacity, and not what stats.n_points says
    res = eng.run_selected(8, seed=1, first_event=0, capacity_per_event=16)
    caps = [c[2] for c in lib.of("sim_run_selected")]
    assert caps == [4096, 500_000 + 4096]  # one retry, sized from n_rows plus the slack
    assert res["n_rows"] == sum(ROWS[i % 4] if _passes(i) else 0 for i in range(8))
    assert res["stats"]["n_points"] >= 1000  # (the cloud's rows: never used for the capacity)


def _kinematics(workload, n):
    pipeline, _, _ = workload
    z, a = pipeline.get_proton_numbers(), pipeline.get_mass_numbers()
    rng = np.random.default_rng(1)
    return rng.normal(size=(n, len(z), 4)), rng.normal(size=(n, 3)), z, a


def test_simulate_batch_selected_and_cloud_select(workload):
    from attpc_engine_amd.detector import Selection, clouds_to_selection, configure_selection, simulate_batch_selected

    _, config, indices = workload
    momenta, vertices, z, a = _kinematics(workload, 6)
    ctx = RecordingContext()
    lib = ctx.lib
    sel = Selection(n_pads=(2, None), tracks=[1], min_tracks=0)
    res = simulate_batch_selected(momenta, vertices, z, a, config, 7, indices, sel, first_event=11, ctx=ctx, min_electrons=250)
    assert lib.names() == ["det_configure", "summary_configure", "select_configure", "det_run_selected"]
    assert lib.calls[2][1] == (2, 2, 0) and lib.calls[3][1] == (7, 11, 6) and lib.calls[3][2] == 6 * 16384
    ids = range(11, 17)
    assert res["passed"].tolist() == [_passes(i) for i in ids] and res["points"].shape[1] == 3
    assert res["events"].shape == (6,) and res["tracks"].shape == (6, len(indices)) and res["stats"]["n_events"] == 6
    lib.calls.clear()
    res = simulate_batch_selected(momenta, vertices, z, a, config, 7, indices, sel, kind="spyral", first_event=11, ctx=ctx,
                                  min_electrons=250)
    assert lib.names() == ["spyral_configure", "det_run_selected"] and lib.calls[1][2] == 6 * 8192
    assert res["rows"].shape[1] == 8
    with pytest.raises(ValueError):
        simulate_batch_selected(momenta, vertices, z, a, config, 7, indices, sel, kind="traces", ctx=ctx)
    with pytest.raises(ValueError):
        simulate_batch_selected(momenta, vertices, z, a, config, 7, indices, Selection(tracks=[len(indices)]), ctx=ctx)
    lib.calls.clear()
    configure_selection(ctx, sel)  # the same content: skipped
    configure_selection(ctx, n_pads=(2, None), track_mask=2, min_tracks=0)
    assert lib.names() == []
    clouds_to_selection(np.array([0, 1, 2]), np.zeros((2, 3)), np.zeros(2, dtype=np.int64), [0, 2], ctx)
    assert lib.names() == ["cloud_select"] and lib.calls[0][1] == (2,)


# ---------------------------------------------------------------- run_fused / run_simulation with a selection ----
class PlainWriter:
    def __init__(self, directory):
        self.directory, self.events, self.closed = directory, [], 0

    def write(self, data, labels, config, event_number):
        self.events.append((event_number, data.shape, list(labels)))

    def get_directory_name(self):
        return self.directory

    def close(self):
        self.closed += 1


def _files(directory):
    return {p.name: dict(np.load(p)) for p in sorted(directory.glob("run_*.npz"))}


def _events(content, prefix):
    return [int(k[len(prefix):]) for k in content if k.startswith(prefix) and "@" not in k]


@pytest.fixture
def no_h5py(monkeypatch):
    monkeypatch.setitem(sys.modules, "h5py", None)
    warnings.simplefilter("ignore", RuntimeWarning)


# the events a selected run of ids 0 .. 9 hands a writer: passed (id % 3 != 0) and with a cloud (POINTS[id % 4] != 0)
WRITTEN = [i for i in range(10) if _passes(i) and POINTS[i % 4]]


def test_run_fused_with_a_selection(workload, tmp_path, no_h5py):
    from attpc_engine_amd.detector import PeakSettings, Selection, SpyralWriter, TraceWriter
    from attpc_engine_amd.engine import run_fused

    pipeline, config, indices = workload
    ctx = RecordingContext()
    lib = ctx.lib
    sel = Selection(n_pads=(3, None))
    assert WRITTEN == [1, 2, 5, 7]
    (tmp_path / "spyral").mkdir()
    run_fused(pipeline, config, SpyralWriter(tmp_path / "spyral", config, max_events_per_file=3), 10, indices, seed=8,
              batch_size=4, context=ctx, selection=sel)
    assert lib.names() == ["kin_configure", "det_configure", "select_configure", "spyral_configure", "summary_configure"] + [
        "sim_run_selected"] * 3
    assert [c[1] for c in lib.of("sim_run_selected")] == [(8, 0, 4), (8, 4, 4), (8, 8, 2)]
    files = _files(tmp_path / "spyral")
    # exactly the passed non-empty events, under their original numbers; the roll-over counts written events
    assert [_events(f, "cloud/cloud_") for f in files.values()] == [[1, 2, 5], [7]]
    assert [(int(f["cloud@min_event"]), int(f["cloud@max_event"])) for f in files.values()] == [(0, 5), (7, 7)]
    assert files["run_0000.npz"]["cloud/cloud_1"].shape == (0, 8)  # passed, a cloud, no row above the threshold
    np.testing.assert_array_equal(files["run_0001.npz"]["cloud/cloud_7"][:, 0], [70, 70])
    np.testing.assert_array_equal(files["run_0000.npz"]["cloud/labels_2"], [2])
    plain = PlainWriter(tmp_path)
    run_fused(pipeline, config, plain, 10, indices, seed=8, batch_size=4, context=ctx, selection=sel)
    assert plain.events == [(1, (0, 3), []), (2, (1, 3), [2]), (5, (0, 3), []), (7, (2, 3), [7, 7])] and plain.closed == 1
    (tmp_path / "trace").mkdir()
    lib.calls.clear()
    with pytest.raises(ValueError):
        run_fused(pipeline, config, TraceWriter(tmp_path / "trace", config), 10, indices, context=ctx, selection=sel)
    with pytest.raises(ValueError):
        run_fused(pipeline, config, SpyralWriter(tmp_path / "trace", config, peaks=PeakSettings()), 10, indices, context=ctx, selection=sel)
    assert not [n for n in lib.names() if "run" in n]


def test_run_simulation_with_a_selection(workload, tmp_path, monkeypatch, no_h5py, capsys):
    from attpc_engine_amd.detector import Selection, SpyralWriter, TraceWriter, run_simulation
    from attpc_engine_amd.io import KinematicsFileWriter

    _, config, indices = workload
    ctx = RecordingContext()
    monkeypatch.setattr(_abi, "_default_ctx", ctx)
    lib = ctx.lib
    momenta, vertices, z, a = _kinematics(workload, 10)
    writer = KinematicsFileWriter(tmp_path / "kin.npz", 10, z, a, chunk_size=4)
    writer.write_batch(0, vertices, momenta)
    writer.close()
    path = tmp_path / "kin.npz"
    run_seed = int(np.random.default_rng(5).integers(0, 1 << 63))
    sel = Selection(n_kept=(1, None))
    plain = PlainWriter(tmp_path)
    run_simulation(config, path, plain, indices, batch_size=4, seed=5, selection=sel)
    assert lib.names() == ["det_configure", "summary_configure", "select_configure"] + ["det_run_selected"] * 3
    assert [c[1] for c in lib.of("det_run_selected")] == [(run_seed, 0, 4), (run_seed, 4, 4), (run_seed, 8, 2)]
    assert [e[0] for e in plain.events] == WRITTEN and plain.events[-1] == (7, (2, 3), [7, 7]) and plain.closed == 1
    lib.calls.clear()
    (tmp_path / "spyral").mkdir()
    run_simulation(config, path, SpyralWriter(tmp_path / "spyral", config, max_events_per_file=3), indices, batch_size=4,
                   seed=5, selection=sel)
    assert lib.names() == ["spyral_configure"] + ["det_run_selected"] * 3
    files = _files(tmp_path / "spyral")
    assert [_events(f, "cloud/cloud_") for f in files.values()] == [[1, 2, 5], [7]]
    np.testing.assert_array_equal(files["run_0001.npz"]["cloud/labels_7"], [7, 7])
    lib.calls.clear()
    (tmp_path / "trace").mkdir()
    with pytest.raises(ValueError):
        run_simulation(config, path, TraceWriter(tmp_path / "trace", config), indices, seed=5, selection=sel)
    assert not [n for n in lib.names() if "run" in n]
    capsys.readouterr()


# ---------------------------------------------------------------- the generated code ----
def _kernel_notes(code_object: Path) -> dict:
    text = subprocess.run([str(llvm_tool("llvm-readelf")), "--notes", str(code_object)], capture_output=True, text=True,
                          check=True).stdout
    blocks = {}
    for block in text.split("\n  - .agpr_count:")[1:]:
        for line in block.splitlines():
            if line.strip().startswith(".name:"):
                blocks[line.split(":", 1)[1].strip()] = block
    return blocks


@pytest.mark.skipif(any(llvm_tool(t) is None for t in ("llvm-objdump", "llvm-objcopy", "llvm-readelf")),
                    reason="ROCm LLVM tools not installed")
def test_selection_kernels_use_no_scratch_and_no_fused_multiply_add():
    import __graft_entry__ as entry

    entry.build()
    with tempfile.TemporaryDirectory() as tmp:
        objects = device_code_objects(LIB, Path(tmp))
        functions = disassemble_objects(objects)
        notes = {}
        for co in objects:
            notes.update(_kernel_notes(co))
    kernels = {name: insns for name, insns in functions.items() if "select_kernel" in name or "gather_selected_kernel" in name}
    for wanted in ("select_kernel", "gather_selected_kernel"):
        assert any(wanted in n for n in kernels), sorted(functions)
    for name, insns in kernels.items():
        ops = [text.split()[0] for _, text in insns if text]
        assert not [o for o in ops if o.startswith("v_fma_f64")], name
        assert not [o for o in ops if o.startswith("scratch_")], name
        assert ".private_segment_fixed_size: 0" in notes[name], name
        if "select_kernel" in name:  # end_rho2: two rounded products and their sum
            assert ops.count("v_mul_f64") >= 2 and "v_add_f64" in ops, name
