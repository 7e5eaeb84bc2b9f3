"""Run maps, host side (no GPU): the header's declarations and struct layouts against their ctypes mirrors, the exported
symbols, ``MapsSettings`` and ``RunMaps``, the Python run layer through a recording stand-in library, the numpy
restatement of the contract on hand-made clouds with written-down answers, and the generated code of the maps kernels
(no scratch, LDS within a compute unit's)."""
import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from attpc_engine_amd import _abi, workloads
from attpc_engine_amd.detector.maps import FULL_MASK, OTHER_LABELS, MapsSettings, RunMaps
from tests import maps_reference as ref
from tests.isa_tools import device_code_objects, disassemble_objects, llvm_tool
from tests.summary_reference import csr, hand_made_events

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "attpc_engine_amd" / "_lib" / "libattpc_hip.so"
ENTRY_POINTS = ("attpc_maps_configure", "attpc_sim_run_maps", "attpc_det_run_maps", "attpc_cloud_maps")


# ---------------------------------------------------------------- header, layouts, symbols ----
def test_header_declares_the_entry_points_and_structs():
    header = (ROOT / "include" / "attpc_engine.h").read_text()
    for name in ENTRY_POINTS:
        assert re.search(rf"ATTPC_API int32_t {name}\(", header), name
    for name in ("attpc_maps_desc", "attpc_maps_out"):
        assert re.search(rf"typedef struct {name} \{{", header), name
    assert "#define ATTPC_ABI_VERSION 3" in header and _abi.ABI_VERSION == 3
    assert _abi.MAPS_SYMBOLS == ENTRY_POINTS and "maps" in _abi.CONFIGURE_SLOTS
    # the invariants the contract states
    section = header[header.index("run maps: pad and time-bucket hit maps"):]
    for phrase in ("maps(A u B) = maps(A) + maps(B)", "sum(pad_events) = sum(events[].n_pads)",
                   "sum(tb_rows) = sum(events[].n_kept)", "sum(pad_charge) = sum(tb_charge) = sum(events[].charge)"):
        assert phrase in section, phrase


def test_struct_layouts_match_the_header():
    structs = {"attpc_maps_desc": _abi.MapsDesc, "attpc_maps_out": _abi.MapsOut}
    lines = []
    for name, ctype in structs.items():
        args = ", ".join([f"sizeof({name})"] + [f"offsetof({name}, {field})" for field, _ in ctype._fields_])
        lines.append(f' printf("{" ".join(["%zu"] * (1 + len(ctype._fields_)))}\\n", {args});')
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "attpc_engine.h"\nint main(void){\n' + "\n".join(lines) +
           '\n printf("%d %d %d\\n", ATTPC_NUM_PADS, ATTPC_NUM_TB, ATTPC_MAX_SIM);\n return 0; }\n')
    with tempfile.TemporaryDirectory() as tmp:
        c = Path(tmp) / "t.c"
        c.write_text(src)
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(c), "-o", str(Path(tmp) / "t")], check=True)
        out = subprocess.run([str(Path(tmp) / "t")], capture_output=True, text=True, check=True).stdout.splitlines()
    for line, (name, ctype) in zip(out, structs.items()):
        want = [int(v) for v in line.split()]
        assert want == [C.sizeof(ctype)] + [getattr(ctype, f).offset for f, _ in ctype._fields_], name
    assert [int(v) for v in out[-1].split()] == [_abi.NUM_PADS, _abi.NUM_TB, _abi.MAX_SIM]
    assert C.sizeof(_abi.MapsDesc) == 8 and C.sizeof(_abi.MapsOut) == 56


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
    assert "maps.hip" in entry.HIP_SOURCES and '"$C/maps.hip"' in (ROOT / "tools" / "build_variant.sh").read_text()


# ---------------------------------------------------------------- MapsSettings, RunMaps ----
def test_maps_settings_validation_and_tokens():
    assert (OTHER_LABELS, FULL_MASK) == (1 << 8, 0x1ff) == (ref.OTHER, ref.FULL_MASK)
    default = MapsSettings()
    assert default.track_mask == 0xff and default.selected is False and default.token() == (0xff, False)
    assert (MapsSettings.slot, MapsSettings.call) == ("maps", "attpc_maps_configure")
    assert MapsSettings(tracks=[0, 2]).track_mask == 0b101 and MapsSettings(tracks=(1, 1)).track_mask == 0b10
    assert MapsSettings(tracks=[], other_labels=True).track_mask == 0x100
    assert MapsSettings(other_labels=True).track_mask == FULL_MASK
    d = MapsSettings(tracks=[7], other_labels=True, selected=True).desc()
    assert isinstance(d, _abi.MapsDesc) and (d.track_mask, d.selected) == (0x180, 1)
    assert MapsSettings(tracks=[1]).token() != MapsSettings(tracks=[1], selected=True).token() != MapsSettings(tracks=[2]).token()
    for bad in ({"tracks": []}, {"tracks": [8]}, {"tracks": [-1]}):
        with pytest.raises(ValueError):
            MapsSettings(**bad)
    for bad in ({"selected": 1}, {"other_labels": "yes"}):
        with pytest.raises(TypeError):
            MapsSettings(**bad)


def _random_maps(rng) -> RunMaps:
    return RunMaps(rng.integers(0, 9, _abi.NUM_PADS), rng.integers(0, 1 << 40, _abi.NUM_PADS), rng.integers(0, 9, 512),
                   rng.integers(0, 99, 512), rng.integers(0, 1 << 40, 512), n_events=int(rng.integers(5, 50)),
                   n_hit=int(rng.integers(0, 5)))


def test_run_maps_add_and_occupancy():
    rng = np.random.default_rng(3)
    a, b = _random_maps(rng), _random_maps(rng)
    c = a + b
    for name, dtype, size in (("pad_events", np.uint64, _abi.NUM_PADS), ("pad_charge", np.int64, _abi.NUM_PADS),
                              ("tb_events", np.uint64, 512), ("tb_rows", np.uint64, 512), ("tb_charge", np.int64, 512)):
        got = getattr(c, name)
        assert got.dtype == dtype and got.shape == (size,)
        assert np.array_equal(got, getattr(a, name) + getattr(b, name))
    assert (c.n_events, c.n_hit) == (a.n_events + b.n_events, a.n_hit + b.n_hit)
    assert c == b + a and c != a and sum([a, b]) == c and a + RunMaps() == a
    ref.assert_same_maps(c, b + a)
    with pytest.raises(AssertionError):
        other = b + a
        other.tb_rows[511] += 1
        ref.assert_same_maps(c, other)
    with pytest.raises(TypeError):
        a + 1
    with pytest.raises(ValueError):
        RunMaps(pad_events=np.zeros(5))
    assert np.array_equal(a.occupancy(), a.pad_events / a.n_events) and a.occupancy().dtype == np.float64
    assert not RunMaps().occupancy().any() and RunMaps().occupancy().shape == (_abi.NUM_PADS,)
    # the struct points at the object's own arrays
    out = a.out()
    out.pad_events[7], out.tb_charge[511], out.n_events, out.n_hit = 123, -5, 77, 66
    a.absorb(out)
    assert (a.pad_events[7], a.tb_charge[511], a.n_events, a.n_hit) == (123, -5, 77, 66)


# ---------------------------------------------------------------- the run layer through a recording stand-in ----
class RecordingLibrary:
    """Stands in for libattpc_hip.so (the idea of tests/test_run_layer_cpu.py): every ``attpc_*`` call is recorded as
    (name, scalar arguments and those of its descriptor, positions of NULL arguments); a maps call fills what its output
    structs point at."""

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
        scalars = tuple(a for a in args if isinstance(a, (int, float)))
        for a in args:
            if isinstance(a, _abi.MapsDesc):
                scalars += (int(a.track_mask), int(a.selected))
            if isinstance(a, _abi.SummaryDesc):
                scalars += (int(a.min_electrons),)
            if isinstance(a, _abi.SelectDesc):
                scalars += (int(a.n_pads_lo),)
        self.calls.append((name, scalars, tuple(i for i, a in enumerate(args) if a is None)))
        maps = next((a for a in args if isinstance(a, _abi.MapsOut)), None)
        if maps is not None:
            n = args[2] if name != "attpc_cloud_maps" else args[0]
            records = next(a for a in args if isinstance(a, _abi.SummaryOut))
            passed = next(a for a in args if isinstance(a, C.POINTER(C.c_uint8)))
            for e in range(n):
                records.events[e].n_points = e + 1
                passed[e] = e % 2
            maps.pad_events[10239], maps.pad_charge[0], maps.tb_events[0], maps.tb_rows[511], maps.tb_charge[5] = 1, -2, 3, 4, 5
            maps.n_events, maps.n_hit = n, n - 1
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


def _check_stand_in_maps(maps, n):
    assert isinstance(maps, RunMaps) and (maps.n_events, maps.n_hit) == (n, n - 1)
    assert (maps.pad_events[10239], maps.pad_charge[0], maps.tb_events[0], maps.tb_rows[511], maps.tb_charge[5]) == (1, -2, 3, 4, 5)


def test_run_maps_makes_one_call_and_configures_what_it_needs():
    from attpc_engine_amd.engine import Engine

    pipeline, config, indices = workloads.o16aa()
    ctx = RecordingContext()
    eng = Engine(pipeline, config, indices, context=ctx)
    ctx.lib.calls.clear()
    res = eng.run_maps(5, seed=9, first_event=3)
    assert ctx.lib.names() == ["maps_configure", "summary_configure", "sim_run_maps"]
    assert ctx.lib.calls[0][1] == (0xff, 0) and ctx.lib.calls[2][1] == (9, 3, 5) and ctx.lib.calls[2][2] == ()
    assert sorted(res) == ["events", "indices", "maps", "p4", "passed", "stats", "status", "tracks", "vertex"]
    _check_stand_in_maps(res["maps"], 5)
    assert res["events"]["n_points"].tolist() == [1, 2, 3, 4, 5] and res["tracks"].shape == (5, len(indices))
    assert res["passed"].dtype == bool and res["passed"].tolist() == [False, True, False, True, False]
    assert res["p4"].shape == (5, eng.n_rows, 4) and res["indices"] == list(indices) and res["stats"]["n_events"] == 5
    # configured once: the next run makes the run call alone; other settings are uploaded, the same ones are not
    ctx.lib.calls.clear()
    eng.run_maps(2)
    eng.configure_maps(tracks=[1], other_labels=True)
    eng.configure_maps(MapsSettings(tracks=[1], other_labels=True))
    eng.run_maps(2)
    assert ctx.lib.names() == ["sim_run_maps", "maps_configure", "sim_run_maps"] and ctx.lib.calls[1][1] == (0x102, 0)
    # maps of the selected events: not without a selection; with one, it is uploaded with the maps
    eng.configure_maps(selected=True)
    ctx.lib.calls.clear()
    with pytest.raises(RuntimeError, match="configure_selection"):
        eng.run_maps(2)
    assert ctx.lib.names() == []
    eng.configure_selection(n_pads=(20, None))
    eng.run_maps(2)
    assert ctx.lib.names() == ["select_configure", "sim_run_maps"] and ctx.lib.calls[0][1] == (20,)
    with pytest.raises(ValueError):
        eng.run_maps(1, seed=-1)
    with pytest.raises(TypeError):
        eng.configure_maps(MapsSettings(), selected=True)


def test_batch_and_cloud_entry_points_through_the_stand_in():
    from attpc_engine_amd.detector import Selection, clouds_to_maps, configure_maps, configure_summary, simulate_batch_maps

    pipeline, config, indices = workloads.be10dp()
    z, a = pipeline.get_proton_numbers(), pipeline.get_mass_numbers()
    ctx = RecordingContext()
    rng = np.random.default_rng(1)
    p4, vertex = rng.normal(size=(4, len(z), 4)), rng.normal(size=(4, 3))
    res = simulate_batch_maps(p4, vertex, z, a, config, 7, indices, first_event=11, ctx=ctx, min_electrons=250)
    assert ctx.lib.names() == ["det_configure", "summary_configure", "maps_configure", "det_run_maps"]
    assert ctx.lib.calls[1][1][-1] == 250 and ctx.lib.calls[2][1] == (0xff, 0) and ctx.lib.calls[3][1] == (7, 11, 4)
    assert sorted(res) == ["events", "maps", "passed", "stats", "tracks"] and res["stats"]["n_events"] == 4
    _check_stand_in_maps(res["maps"], 4)
    assert res["events"].shape == (4,) and res["tracks"].shape == (4, len(indices)) and res["passed"].tolist() == [0, 1, 0, 1]
    with pytest.raises(ValueError, match="Selection"):
        simulate_batch_maps(p4, vertex, z, a, config, 7, indices, maps=MapsSettings(selected=True), ctx=ctx)
    ctx.lib.calls.clear()
    simulate_batch_maps(p4, vertex, z, a, config, 7, indices, maps=MapsSettings(selected=True), ctx=ctx, min_electrons=250,
                        selection=Selection(n_pads=(3, None)))
    assert ctx.lib.names() == ["select_configure", "maps_configure", "det_run_maps"] and ctx.lib.calls[1][1] == (0xff, 1)
    # turning the mode off is a NULL descriptor; the same content again is skipped
    ctx.lib.calls.clear()
    assert configure_maps(ctx) is None and configure_maps(ctx) is None
    assert ctx.lib.names() == ["maps_configure"] and ctx.lib.calls[0][2] == (0,)
    configure_summary(config, ctx, 250)
    ev, idx, _, _ = hand_made_events()
    offsets, points, labels = csr(ev)
    ctx.lib.calls.clear()
    maps, passed, events, tracks = clouds_to_maps(offsets, points, labels, idx, ctx)
    assert ctx.lib.names() == ["cloud_maps"] and ctx.lib.calls[0][1] == (len(ev),)
    _check_stand_in_maps(maps, len(ev))
    assert passed.shape == (len(ev),) and events.shape == (len(ev),) and tracks.shape == (len(ev), len(idx))
    with pytest.raises(ValueError):
        clouds_to_maps(offsets, points[:-1], labels, idx, ctx)


# ---------------------------------------------------------------- the restatement on hand-made clouds ----
def test_restatement_on_hand_made_clouds():
    ev, indices, min_electrons, _ = hand_made_events()
    offsets, points, labels = csr(ev)
    for mask, cells in ref.hand_made_maps().items():
        want = ref.from_cells(cells)
        ref.assert_same_maps(ref.maps(offsets, points, labels, indices, min_electrons, mask), want, f"mask {mask:#x}")
        ref.assert_same_maps(ref.maps_fast(offsets, points, labels, indices, min_electrons, mask), want, f"fast, mask {mask:#x}")
    # the masks of the positions and of the other labels partition the rows: the charges and rows add up, and so do the
    # event counts here, where no event has rows of two of the masks' sets on one pad or in one bucket but event 0
    full = ref.maps(offsets, points, labels, indices, min_electrons)
    parts = [ref.maps(offsets, points, labels, indices, min_electrons, m) for m in (1, 2, 4, ref.OTHER)]
    for name in ("pad_charge", "tb_rows", "tb_charge"):
        assert np.array_equal(sum(getattr(p, name) for p in parts), getattr(full, name)), name
    assert sum(int(p.pad_events[7]) for p in parts) == 2 and full.pad_events[7] == 1  # (labels 2 and 5 of event 0)
    # only the passed events contribute, |E| counts them whether they have rows or not
    passed = np.array([True, False, False, True, True])
    some = ref.maps(offsets, points, labels, indices, min_electrons, passed=passed)
    assert (some.n_events, some.n_hit) == (3, 2) and some.pad_events[3] == 0 and some.pad_charge[7] == 600
    ref.assert_same_maps(ref.maps_fast(offsets, points, labels, indices, min_electrons, passed=passed), some)
    split = (ref.maps(offsets[:3], points, labels, indices, min_electrons)
             + ref.maps(offsets[2:], points, labels, indices, min_electrons))
    ref.assert_same_maps(split, full, "split")
    # nothing kept above every charge; at 0 the 99 electrons on pad 8 and both rows of event 1 count as well
    none = ref.maps(offsets, points, labels, indices, 1 << 62)
    assert none == RunMaps(n_events=5)
    every = ref.maps(offsets, points, labels, indices, 0)
    assert every.pad_charge[8] == 99 and every.n_hit == 4 and every.tb_rows.sum() == len(points)
    assert every.pad_charge.sum() == every.tb_charge.sum() == int(points[:, 2].astype(np.int64).sum())


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
def test_maps_kernels_use_no_scratch_and_native_atomics():
    import __graft_entry__ as entry

    entry.build()
    with tempfile.TemporaryDirectory() as tmp:
        objects = device_code_objects(LIB, Path(tmp))
        functions = disassemble_objects(objects)
        notes = {}
        for co in objects:
            notes.update(_kernel_notes(co))
    kernels = {name: insns for name, insns in functions.items() if "maps_" in name and "_kernel" in name}
    for wanted in ("maps_event_kernel", "maps_fold_kernel"):
        assert any(wanted in n for n in kernels), sorted(functions)
    for name, insns in kernels.items():
        ops = [text.split()[0] for _, text in insns if text]
        assert not [o for o in ops if o.startswith("scratch_")], name
        assert ".private_segment_fixed_size: 0" in notes[name], name
        if "maps_event_kernel" in name:
            lds = int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", notes[name]).group(1))
            assert 120 * 1024 < lds <= 160 * 1024, lds  # a whole map per workgroup, within one compute unit's LDS
            # the first-row-of-the-event test is the returned word of an LDS or; the sums are LDS and global adds, no
            # compare-and-swap loop
            assert "ds_or_rtn_b32" in ops and "ds_add_u64" in ops and "ds_add_u32" in ops, name
            assert [o for o in ops if o.startswith("global_atomic_add_x2")], name
            assert not [o for o in ops if "cmpswap" in o], name
