"""Event and track summaries, host side (no GPU): the header's declarations and record layouts against their ctypes
and numpy mirrors, the exported symbols, ``electrons_above_threshold`` against its definition, the Python run layer
through a recording stand-in library, the numpy restatement of the contract on hand-made clouds with known answers,
and the generated code of the summary kernels (no scratch, no fused multiply-add)."""
import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from attpc_engine_amd import _abi, workloads
from tests.isa_tools import device_code_objects, disassemble_objects, llvm_tool
from tests.summary_reference import (assert_same_records, check_expected, csr, hand_made_centers, hand_made_events,
                                     summary)

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "attpc_engine_amd" / "_lib" / "libattpc_hip.so"
ENTRY_POINTS = ("attpc_summary_configure", "attpc_sim_run_summary", "attpc_det_run_summary", "attpc_cloud_summary")
WORKLOADS = ("o16aa", "be10dp", "b10chain")


# ---------------------------------------------------------------- header, layouts, symbols ----
def test_header_declares_the_entry_points_and_records():
    header = (ROOT / "include" / "attpc_engine.h").read_text()
    for name in ENTRY_POINTS:
        assert re.search(rf"ATTPC_API int32_t {name}\(", header), name
    for name in ("attpc_event_summary", "attpc_track_summary", "attpc_summary_desc", "attpc_summary_out"):
        assert re.search(rf"typedef struct {name} \{{", header), name
    assert "#define ATTPC_ABI_VERSION 3" in header and _abi.ABI_VERSION == 3


def test_record_layouts_match_the_header():
    structs = {"attpc_event_summary": (_abi.EventSummary, _abi.EVENT_SUMMARY_DTYPE),
               "attpc_track_summary": (_abi.TrackSummary, _abi.TRACK_SUMMARY_DTYPE),
               "attpc_summary_desc": (_abi.SummaryDesc, None), "attpc_summary_out": (_abi.SummaryOut, None)}
    lines = []
    for name, (ctype, _) in structs.items():
        args = ", ".join([f"sizeof({name})"] + [f"offsetof({name}, {field})" for field, _ in ctype._fields_])
        lines.append(f' printf("{" ".join(["%zu"] * (1 + len(ctype._fields_)))}\\n", {args});')
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "attpc_engine.h"\nint main(void){\n' + "\n".join(lines) +
           '\n printf("%d\\n", ATTPC_ABI_VERSION);\n return 0; }\n')
    with tempfile.TemporaryDirectory() as tmp:
        c = Path(tmp) / "t.c"
        c.write_text(src)
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(c), "-o", str(Path(tmp) / "t")], check=True)
        out = subprocess.run([str(Path(tmp) / "t")], capture_output=True, text=True, check=True).stdout.splitlines()
    for line, (name, (ctype, dtype)) in zip(out, structs.items()):
        want = [int(v) for v in line.split()]
        assert want == [C.sizeof(ctype)] + [getattr(ctype, f).offset for f, _ in ctype._fields_], name
        assert want[0] % 8 == 0, name
        if dtype is not None:
            assert dtype.names == tuple(f for f, _ in ctype._fields_), name
            assert want == [dtype.itemsize] + [dtype.fields[f][1] for f in dtype.names], name
    assert int(out[-1]) == 3
    assert _abi.EVENT_SUMMARY_DTYPE.itemsize == 32 and _abi.TRACK_SUMMARY_DTYPE.itemsize == 80


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


# ---------------------------------------------------------------- electrons_above_threshold ----
def _above(r_max, q, thr):
    return min(r_max * float(q), 4095.0) > thr


@pytest.mark.parametrize("name", WORKLOADS)
def test_electrons_above_threshold_on_the_workloads(name):
    from attpc_engine_amd.detector.response import get_response
    from attpc_engine_amd.detector.summary import electrons_above_threshold

    _, config, _ = getattr(workloads, name)()
    r_max = float(get_response(config).max())
    thr = float(config.elec_params.adc_threshold)
    q = electrons_above_threshold(config)
    assert q >= 1 and _above(r_max, q, thr) and not _above(r_max, q - 1, thr)
    # the rule of the Spyral rows: amplitude = min(r_max * q, 4095) must exceed the threshold
    assert abs(q - thr / r_max) <= 1.0


@pytest.mark.parametrize("thr", [0, 4094.5, 4095, 4096, -1, -0.5, 40, 1e-9])
@pytest.mark.parametrize("r_max", [3.2e-5, 1.0, 0.3, 4095.0])
def test_electrons_above_threshold_at_the_edges(thr, r_max):
    import copy

    from attpc_engine_amd.detector.summary import NEVER_KEPT, electrons_above_threshold

    _, config, _ = workloads.be10dp()
    config = copy.deepcopy(config)
    config.elec_params.adc_threshold = thr
    response = np.zeros(512)
    response[17] = r_max
    response[18] = r_max / 2
    q = electrons_above_threshold(config, response)
    if thr >= 4095:
        assert q == NEVER_KEPT and not _above(r_max, 1 << 61, thr)  # nothing survives: above any charge
    elif thr < 0:
        assert q == 0
    else:
        assert _above(r_max, q, thr) and q >= 1 and not _above(r_max, q - 1, thr), (q, thr, r_max)
    assert electrons_above_threshold(config, np.zeros(512)) == (0 if thr < 0 else NEVER_KEPT)


# ---------------------------------------------------------------- the run layer through a recording stand-in ----
class RecordingLibrary:
    """Stands in for libattpc_hip.so (the idea of tests/test_run_layer_cpu.py): every ``attpc_*`` call is recorded as
    (name, scalar arguments, positions of NULL arguments, sizes of the record arrays of its attpc_summary_out)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("attpc_"):
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def names(self):
        return [name[len("attpc_"):] for name, *_ in self.calls]

    def _call(self, name, args):
        if name == "attpc_last_error":
            return b"recorded"
        args = args[1:]  # (the context handle)
        out = next((a for a in args if isinstance(a, _abi.SummaryOut)), None)
        desc = next((a for a in args if isinstance(a, _abi.SummaryDesc)), None)
        scalars = tuple(a for a in args if isinstance(a, (int, float)))
        if desc is not None:
            scalars += (int(desc.min_electrons), int(desc.n_pads))
        nulls = tuple(i for i, a in enumerate(args) if a is None)
        self.calls.append((name, scalars, nulls, out))
        if out is not None:  # mark every record the caller must have room for
            n = args[2] if name != "attpc_cloud_summary" else args[0]
            layout = next(a for a in args if isinstance(a, _abi.EventLayout))
            for e in range(n):
                out.events[e].n_points = e + 1
                for s in range(layout.n_sim):
                    out.tracks[e * layout.n_sim + s].n_steps = 10 * e + s
            stats = next((a for a in args if isinstance(a, _abi.RunStats)), None)
            if stats is not None:
                stats.n_events = n
        return _abi.OK


class RecordingContext(_abi.Context):
    def __init__(self):
        saved, _abi._lib = _abi._lib, RecordingLibrary()
        try:
            super().__init__(0)
        finally:
            _abi._lib = saved
        self.lib.calls.clear()


def test_run_summary_makes_one_call_with_kinematics_and_sized_records():
    from attpc_engine_amd.detector.summary import electrons_above_threshold
    from attpc_engine_amd.engine import Engine

    pipeline, config, indices = workloads.o16aa()
    ctx = RecordingContext()
    eng = Engine(pipeline, config, indices, context=ctx)
    ctx.lib.calls.clear()
    res = eng.run_summary(5, seed=9, first_event=3)
    assert ctx.lib.names() == ["summary_configure", "sim_run_summary"]
    name, scalars, nulls, _ = ctx.lib.calls[0]
    assert scalars == (electrons_above_threshold(config), len(config.pad_centers)) and nulls == ()
    name, scalars, nulls, out = ctx.lib.calls[1]
    assert scalars == (9, 3, 5) and nulls == ()  # p4, vertex, status and the output struct are all there
    assert sorted(res) == ["events", "indices", "p4", "stats", "status", "tracks", "vertex"]
    assert res["events"].dtype == _abi.EVENT_SUMMARY_DTYPE and res["events"].shape == (5,)
    assert res["tracks"].dtype == _abi.TRACK_SUMMARY_DTYPE and res["tracks"].shape == (5, len(indices))
    assert res["p4"].shape == (5, eng.n_rows, 4) and res["vertex"].shape == (5, 3) and res["status"].shape == (5,)
    assert res["indices"] == list(indices) and res["stats"]["n_events"] == 5
    # the stand-in wrote through the pointers of the output struct: they are the arrays of the result
    assert res["events"]["n_points"].tolist() == [1, 2, 3, 4, 5]
    assert res["tracks"]["n_steps"].tolist() == [[10 * e + s for s in range(len(indices))] for e in range(5)]
    # configured once: the next run makes the run call alone; another min_electrons is uploaded, the same one is not
    ctx.lib.calls.clear()
    eng.run_summary(2)
    eng.configure_summary(min_electrons=0)
    eng.configure_summary(min_electrons=0)
    eng.run_summary(2)
    assert ctx.lib.names() == ["sim_run_summary", "summary_configure", "sim_run_summary"]
    assert ctx.lib.calls[1][1] == (0, len(config.pad_centers))
    with pytest.raises(ValueError):
        eng.run_summary(1, seed=-1)
    with pytest.raises(ValueError):
        eng.configure_summary(min_electrons=-1)


def test_batch_and_cloud_entry_points_through_the_stand_in():
    from attpc_engine_amd.detector import clouds_to_summary, configure_summary, simulate_batch_summary

    pipeline, config, indices = workloads.be10dp()
    z, a = pipeline.get_proton_numbers(), pipeline.get_mass_numbers()
    ctx = RecordingContext()
    rng = np.random.default_rng(1)
    events, tracks, stats = simulate_batch_summary(rng.normal(size=(4, len(z), 4)), rng.normal(size=(4, 3)), z, a, config,
                                                   7, indices, first_event=11, ctx=ctx, min_electrons=250)
    assert ctx.lib.names() == ["det_configure", "summary_configure", "det_run_summary"]
    assert ctx.lib.calls[1][1] == (250, len(config.pad_centers)) and ctx.lib.calls[2][1] == (7, 11, 4)
    assert events.shape == (4,) and tracks.shape == (4, len(indices)) and stats["n_events"] == 4
    assert events["n_points"].tolist() == [1, 2, 3, 4]
    configure_summary(config, ctx, 250)  # the same content: skipped
    assert ctx.lib.names()[3:] == []
    ev, idx, _, _ = hand_made_events()
    offsets, points, labels = csr(ev)
    events, tracks = clouds_to_summary(offsets, points, labels, idx, ctx)
    assert ctx.lib.names()[3:] == ["cloud_summary"] and ctx.lib.calls[3][1] == (len(ev),)
    assert events.shape == (len(ev),) and tracks.shape == (len(ev), len(idx))


# ---------------------------------------------------------------- the restatement on hand-made clouds ----
def test_restatement_on_hand_made_clouds():
    ev, indices, min_electrons, expected = hand_made_events()
    offsets, points, labels = csr(ev)
    events, tracks = summary(offsets, points, labels, indices, min_electrons, hand_made_centers())
    check_expected(events, tracks, expected)
    assert np.isnan(tracks["end_x"]).all() and (tracks["n_samples"] == 0).all() and (tracks["electrons"] == 0).all()
    # nothing kept above every charge, everything at 0
    none, _ = summary(offsets, points, labels, indices, 1 << 62, hand_made_centers())
    assert (none["n_kept"] == 0).all() and (none["tb_min"] == -1).all() and (none["n_points"] == events["n_points"]).all()
    every, tr = summary(offsets, points, labels, indices, 0, hand_made_centers())
    assert (every["n_kept"] == every["n_points"]).all() and (tr["n_kept"] == tr["n_points"]).all()
    # the track part from attpc_det_tracks-style arrays
    n_tracks = len(ev) * len(indices)
    samples = np.zeros((n_tracks, 4, 4))
    samples[1, :3] = [[0.1, 0.2, 30.0, 5.0], [0.2, 0.3, 31.0, 7.0], [0.3, 0.4, 32.5, 11.0]]
    counts = np.zeros(n_tracks, dtype=np.int32)
    counts[1] = 3
    steps = np.arange(n_tracks, dtype=np.int32)
    _, tr = summary(offsets, points, labels, indices, 0, hand_made_centers(), samples, counts, steps)
    assert tr[0, 1]["electrons"] == 23 and tr[0, 1]["n_samples"] == 3 and tr[0, 1]["n_steps"] == 1
    assert (tr[0, 1]["end_x"], tr[0, 1]["end_y"], tr[0, 1]["end_tb"]) == (0.3, 0.4, 32.5) and np.isnan(tr[0, 0]["end_x"])
    assert_same_records(tr, tr.copy())
    with pytest.raises(AssertionError):
        other = tr.copy()
        other[0, 1]["end_tb"] = np.nextafter(32.5, 33.0)
        assert_same_records(tr, other)


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
def test_summary_kernels_use_no_scratch_and_no_fused_multiply_add():
    import __graft_entry__ as entry

    entry.build()
    with tempfile.TemporaryDirectory() as tmp:
        objects = device_code_objects(LIB, Path(tmp))
        functions = disassemble_objects(objects)
        notes = {}
        for co in objects:
            notes.update(_kernel_notes(co))
    kernels = {name: insns for name, insns in functions.items() if "summary_" in name and "_kernel" in name}
    for wanted in ("summary_count_kernel", "summary_fill_kernel", "summary_event_kernel"):
        assert any(wanted in n for n in kernels), sorted(functions)
    for name, insns in kernels.items():
        ops = [text.split()[0] for _, text in insns if text]
        assert not [o for o in ops if o.startswith("v_fma_f64")], name
        assert not [o for o in ops if o.startswith("scratch_")], name
        assert ".private_segment_fixed_size: 0" in notes[name], name
        if "summary_event_kernel" in name:  # rho2: two rounded products and their sum
            assert ops.count("v_mul_f64") >= 2 and "v_add_f64" in ops, name
