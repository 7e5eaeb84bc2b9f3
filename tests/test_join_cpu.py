"""The cluster joining without a GPU (include/attpc_engine.h, "cluster joining"): the contract's names everywhere; the
case set holds what it names; the restatement (tests/join_reference.py) and its mutants, each of which the exact
comparison catches; csrc/join_host.hpp, compiled alone for the host, plain and under the sanitizers (a stand-alone
program with its own main), equal to the restatement exactly; the checks of the settings."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd import detector
from attpc_engine_amd.detector import joining as jmod
from attpc_engine_amd.detector.joining import JoinSettings
from tests import cluster_reference as cref
from tests import join_cases as jc
from tests import join_reference as jref

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "attpc_engine_amd" / "csrc"
ENTRY_POINTS = ("attpc_trace_configure_cluster_join", "attpc_joins_last", "attpc_rows_cluster_join")


def _flat(text: str) -> str:
    return text.replace("\n * ", " ").replace("\n// ", " ").replace("\n", " ")


# ------------------------------------------------------------------------------------------ the contract's names ----
def test_contract_is_declared_everywhere():
    header = (ROOT / "include" / "attpc_engine.h").read_text()
    for name in ENTRY_POINTS:
        assert re.search(rf"ATTPC_API int32_t {name}\(", header) and name in _abi.EXPORTED_SYMBOLS, name
    assert _abi.JOIN_SYMBOLS == ENTRY_POINTS and "cluster_join" in _abi.CONFIGURE_SLOTS
    for struct, cls in (("attpc_join_desc", _abi.JoinDesc), ("attpc_join_event", _abi.JoinEvent), ("attpc_join_record", _abi.JoinRecord)):
        fields = re.search(rf"typedef struct {struct} \{{([^}}]*)\}} {struct};", header).group(1)
        names = [n.strip() for line in re.findall(r"^\s*(?:double|int32_t) ([\w, \[\]]+);", fields, re.M)
                 for n in re.sub(r"\[\w+\]", "", line).split(",")]
        assert names == [name for name, _ in cls._fields_], (struct, names)
    assert (C.sizeof(_abi.JoinDesc), C.sizeof(_abi.JoinEvent), C.sizeof(_abi.JoinRecord)) == (40, 32, 32)
    assert _abi.JOIN_EVENT_DTYPE == np.dtype(jref.JOIN_EVENT_DTYPE.descr, align=True) and _abi.JOIN_DTYPE.descr == jref.JOIN_DTYPE.descr
    for name, value in (("ATTPC_JOIN_CAPPED", _abi.JOIN_CAPPED), ("ATTPC_JOIN_NOT_CLUSTERED", _abi.JOIN_NOT_CLUSTERED),
                        ("ATTPC_JOIN_MAX_CLUSTERS", _abi.JOIN_MAX_CLUSTERS)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == value, name
    assert jmod.STATUS_BITS == {"CAPPED": jref.JOIN_CAPPED, "NOT_CLUSTERED": jref.JOIN_NOT_CLUSTERED}
    shared = (CSRC / "join_host.hpp").read_text()
    kernel = (CSRC / "cluster_join.hip").read_text()
    assert "asm" not in kernel and "float" not in kernel and "join_pair(" in kernel and "join_circle(" in kernel and "join_merge(" in kernel
    assert "fp contract(off)" in shared and "helix_atan2w" in shared and "estimate_kasa" in shared and "2^57" in shared
    assert "cluster_join_kernel" in (CSRC / "tracks_args.hpp").read_text()  # (the scratch dependency is written down there)
    for text in (header, shared, kernel, (ROOT / "README.md").read_text(), (ROOT / "DESIGN.md").read_text()):
        flat = _flat(text)
        assert "with every tie made definite" in flat and "Spyral iterates" in flat.replace("ITERATES", "iterates") and "compared against Spyral" in flat
    entry = (ROOT / "__graft_entry__.py").read_text()
    assert '"cluster_join.hip"' in entry and '"join_host.hpp"' in entry
    for name in ("JoinSettings", "configure_cluster_join", "joins_last", "rows_to_joined_clusters"):
        assert hasattr(detector, name) and name in detector.__all__, name
    assert "attpc_rows_cluster_join" in (ROOT / "INTEGRATION.md").read_text()


# ------------------------------------------------------------------------------------------ the cases, the restatement ----
def test_case_set_holds_what_it_names():
    jc.check_cases()


def test_restatement_on_every_case():
    """What must hold of any result, on every case and every run."""
    offsets, rows, labels, names = jc.csr()
    alone = jc.clustering_alone()
    for run, (out, events, records, jevents, jrecords) in jc.reference().items():
        s, j = jc.RUNS[run]
        a_out, a_events, a_records = alone[s.match]
        for e, name in enumerate(names):
            ev, rec, jev, jrec = events[e], records[e], jevents[e], jrecords[e]
            for field in ("n_rows", "n_range", "n_core", "n_border", "n_noise", "n_small", "status", "truth_rows"):
                assert np.array_equal(ev[field], a_events[e][field]), (run, name, field)
            used = rec["first_row"] >= 0
            assert np.array_equal(used, jrec["first_row"] >= 0) or jev["status"], (run, name)
            if jev["status"]:
                assert np.all(jrec["first_row"] == -1) and ev == a_events[e] and np.array_equal(rec, a_records[e]), (run, name)
                assert np.array_equal(out[offsets[e]:offsets[e + 1]], a_out[offsets[e]:offsets[e + 1]]), (run, name)
                continue
            assert jev["n_candidates"] == a_events[e]["n_clusters"] and ev["n_clusters"] == jev["n_candidates"] - jev["n_joined"], (run, name)
            assert jev["n_candidates"] >= jev["n_circles"] >= jev["n_taking_part"] and jev["n_joined"] <= jev["n_pairs"], (run, name)
            assert np.array_equal(rec["first_row"][used], jrec["first_row"][used]) and np.all(jrec["parts"][used] >= 1), (run, name)
            assert np.all(np.diff(rec["rows"][used]) <= 0), (run, name)
            if ev["n_clusters"] <= 8:
                assert jrec["parts"][used].sum() == jev["n_candidates"] and rec["rows"][used].sum() == ev["n_core"] + ev["n_border"], (run, name)
            assert np.all(np.isnan(jrec["radius"][used]) == np.isnan(jrec["a"][used])), (run, name)


@pytest.mark.parametrize("mutant", jref.MUTANTS)
def test_mutants_of_the_restatement_fail_the_comparison(mutant):
    offsets, rows, labels, names = jc.csr()
    caught = {}
    for run, (s, j) in jc.RUNS.items():
        wrong = jref.join(s, j, offsets, rows, labels, jc.INDICES, mutant=mutant)
        want = jc.reference()[run]
        events = [names[e] for e in range(len(names))
                  if not jref.same(tuple(w[e:e + 1] if i else w[offsets[e]:offsets[e + 1]] for i, w in enumerate(wrong)),
                                   tuple(w[e:e + 1] if i else w[offsets[e]:offsets[e + 1]] for i, w in enumerate(want)))]
        if events:
            caught[run] = events
    print(mutant, "differs on", caught)
    assert caught, mutant


def test_written_arctangent_is_that_of_the_helix_reference():
    from tests import helix_reference as href

    rng = np.random.default_rng(5)
    y, x = rng.normal(size=2000), rng.normal(size=2000)
    assert [jref.atan2w(float(a), float(b)) for a, b in zip(y, x)] == href.atan2w(y, x).tolist()
    c = np.linspace(-1.0, 1.0, 2001)
    assert np.max(np.abs(np.array([jref.acos_w(float(v)) for v in c]) - np.arccos(c))) < 1e-14


# ------------------------------------------------------------------------------------------ the host code alone ----
def _gxx():
    exe = shutil.which("g++")
    if exe is None:
        pytest.skip("g++ not available")
    return exe


def _build(exe: Path, flags: list) -> None:
    cmd = [_gxx(), "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", f"-I{CSRC}", f"-I{ROOT / 'include'}", *flags,
           "-o", str(exe), str(ROOT / "tests" / "native" / "join_check.cpp")]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]


def _settings_words(s: cref.Settings, j, indices=jc.INDICES, **changes) -> np.ndarray:
    head = [s.eps_xy, s.eps_z, s.min_samples, s.min_cluster_size, s.max_rows, {"truth": 0, "rank": 1}[s.match], 0, 0, len(indices)]
    join = {"overlap_ratio": j.overlap_ratio, "min_radius": j.min_radius, "radius_ratio": j.radius_ratio, "max_clusters": j.max_clusters,
            "reserved0": 0, "reserved1": 0, "reserved2": 0}
    join.update(changes)
    return np.array([*head, *indices, *[-1] * (8 - len(indices)), *join.values()], dtype=np.float64)


def _run(exe: Path, tmp: Path, mode: str, data: np.ndarray) -> np.ndarray:
    (tmp / "in.bin").write_bytes(np.ascontiguousarray(data, dtype=np.float64).tobytes())
    run = subprocess.run([str(exe), mode, str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True)
    assert run.returncode == 0 and "ERROR" not in run.stderr and "runtime error" not in run.stderr, (run.returncode, run.stderr[-3000:])
    return np.frombuffer((tmp / "out.bin").read_bytes(), dtype=np.float64)


def _native(exe, tmp, s, j, offsets, rows, labels, indices=jc.INDICES):
    """The stand-alone program on a CSR array -> the five results as the restatement gives them."""
    body = np.concatenate([rows, np.asarray(labels, dtype=np.float64)[:, None]], axis=1).ravel()
    words = np.concatenate([_settings_words(s, j, indices), [len(offsets) - 1], np.asarray(offsets, dtype=np.float64), body])
    out = _run(exe, tmp, "rows", words)
    n, total = len(offsets) - 1, int(offsets[-1])
    at = total
    table = out[at:at + 18 * n].reshape(n, 18).astype(np.int64)
    at += 18 * n
    events = np.zeros(n, dtype=cref.EVENT_DTYPE)
    for k, name in enumerate(cref.EVENT_DTYPE.names[:10]):
        events[name] = table[:, k]
    events["truth_rows"] = table[:, 10:]
    fields = out[at:at + 64 * n].reshape(n, 8, 8).astype(np.int64)
    at += 64 * n
    records = np.zeros((n, 8), dtype=cref.RECORD_DTYPE)
    for k, name in enumerate(cref.RECORD_DTYPE.names):
        records[name] = fields[:, :, k]
    jtable = out[at:at + 6 * n].reshape(n, 6).astype(np.int64)
    at += 6 * n
    jevents = np.zeros(n, dtype=jref.JOIN_EVENT_DTYPE)
    for k, name in enumerate(jref.JOIN_EVENT_DTYPE.names[:6]):
        jevents[name] = jtable[:, k]
    jfields = out[at:at + 40 * n].reshape(n, 8, 5)
    assert at + 40 * n == len(out)
    jrecords = np.zeros((n, 8), dtype=jref.JOIN_DTYPE)
    jrecords["parts"], jrecords["first_row"] = jfields[:, :, 0].astype(np.int64), jfields[:, :, 1].astype(np.int64)
    for k, name in enumerate(("a", "b", "radius")):
        jrecords[name] = jfields[:, :, 2 + k]
    return out[:total].astype(np.int64), events, records, jevents, jrecords


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("join")
    exe = tmp / "join_check"
    _build(exe, ["-O2"])
    return exe, tmp


def test_host_form_equals_the_restatement(native):
    exe, tmp = native
    offsets, rows, labels, _ = jc.csr()
    for run, (s, j) in jc.RUNS.items():
        assert jref.same(_native(exe, tmp, s, j, offsets, rows, labels), jc.reference()[run]), run
    for indices in ((2, 2, 0), (-1, 2, 0), (0, 1, 2, 3, 4, 5, 6, 7), ()):  # a label given twice, a negative index, eight, none
        s, j = jc.RUNS["defaults"]
        assert jref.same(_native(exe, tmp, s, j, offsets, rows, labels, indices), jref.join(s, j, offsets, rows, labels, indices)), indices


def test_sanitized_build_runs_clean(tmp_path):
    """The same program under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone executable."""
    exe = tmp_path / "join_check_san"
    _build(exe, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    offsets, rows, labels, _ = jc.csr()
    for run in ("defaults", "ratio", "two", "rank"):
        s, j = jc.RUNS[run]
        assert jref.same(_native(exe, tmp_path, s, j, offsets, rows, labels), jc.reference()[run]), run
    for field, value in BAD_SETTINGS:
        assert _run(exe, tmp_path, "desc", _settings_words(*jc.RUNS["defaults"], **{field: value})).tolist() == [1.0], (field, value)


# ------------------------------------------------------------------------------------------ the settings ----
NAN, INF = float("nan"), float("inf")
BAD_SETTINGS = [("overlap_ratio", v) for v in (0.0, -0.5, 1.0000001, NAN, INF)] + \
               [("min_radius", v) for v in (0.0, 0.0624, 5000.5, -1.0, NAN, INF)] + \
               [("radius_ratio", v) for v in (0.5, 0.999, -1.0, NAN, INF)] + \
               [("max_clusters", v) for v in (1, 0, 65, -1)] + [("reserved0", 1), ("reserved1", -1), ("reserved2", 7)]
GOOD_SETTINGS = [("overlap_ratio", 1.0), ("overlap_ratio", 1e-300), ("min_radius", 0.0625), ("min_radius", 5000.0), ("radius_ratio", 0.0),
                 ("radius_ratio", 1.0), ("radius_ratio", 1e9), ("max_clusters", 2), ("max_clusters", 64)]


def test_host_desc_checks(native):
    exe, tmp = native
    s, j = jc.RUNS["defaults"]
    assert _run(exe, tmp, "desc", _settings_words(s, j)).tolist() == [0.0]
    for field, value in GOOD_SETTINGS:
        assert _run(exe, tmp, "desc", _settings_words(s, j, **{field: value})).tolist() == [0.0], (field, value)
        assert not jref.desc_error(jref.JoinSettings(**{**vars(j), field: value})), (field, value)
    for field, value in BAD_SETTINGS:
        assert _run(exe, tmp, "desc", _settings_words(s, j, **{field: value})).tolist() == [1.0], (field, value)
        if not field.startswith("reserved"):
            assert jref.desc_error(jref.JoinSettings(**{**vars(j), field: value})), (field, value)


def test_argument_checks():
    for bad in (0.0, -0.1, 1.5, NAN, INF, "0.5", True, None):
        with pytest.raises(ValueError):
            JoinSettings(overlap_ratio=bad)
    for bad in (0.0, 0.06, 5001.0, NAN, INF, -2.0, "10", True, None):
        with pytest.raises(ValueError):
            JoinSettings(min_radius=bad)
    for bad in (0.0, 0.99, -1.0, NAN, INF, "2", True):
        with pytest.raises(ValueError):
            JoinSettings(radius_ratio=bad)
    for bad in (1, 0, 65, -3, 2.0, "3", True, None):
        with pytest.raises(ValueError):
            JoinSettings(max_clusters=bad)
    good = JoinSettings()
    assert good.token() == (0.5, 10.0, None, 32)  # the issue's starting point
    desc = good.desc()
    assert (desc.overlap_ratio, desc.min_radius, desc.radius_ratio, desc.max_clusters, list(desc.reserved)) == (0.5, 10.0, 0.0, 32, [0, 0, 0])
    desc = JoinSettings(0.25, 0.0625, 1.5, np.int64(64)).desc()
    assert (desc.overlap_ratio, desc.min_radius, desc.radius_ratio, desc.max_clusters) == (0.25, 0.0625, 1.5, 64)
    with pytest.raises(TypeError):
        jmod.configure_cluster_join(None, "defaults")
    from attpc_engine_amd.detector.traces import _checked_join

    with pytest.raises(TypeError):
        _checked_join(0.5)
    assert _checked_join(None) is None and _checked_join(good) is good
