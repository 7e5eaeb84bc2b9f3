"""The clustering without a GPU (include/attpc_engine.h, "clustering"): the contract's names everywhere; the case set
holds what it names; the restatement (tests/cluster_reference.py) on every case, its invariants, and its mutants, each of
which the exact comparison catches; scikit-learn's DBSCAN as an independent check of cores, core partition and border
rows; csrc/cluster_host.hpp, compiled alone for the host, plain and under the sanitizers, equal to the restatement
exactly; the checks of the settings; the scores; and the way ``clustering=`` reaches the library."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from attpc_engine_amd import _abi
from attpc_engine_amd.detector import clustering as kmod
from attpc_engine_amd.detector.clustering import ClusterSettings, cluster_scores, configure_clustering, rows_to_clusters
from tests import cluster_cases as cc
from tests import cluster_reference as cref

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "attpc_engine_amd" / "csrc"
ENTRY_POINTS = ("attpc_trace_configure_clustering", "attpc_clusters_last", "attpc_cluster_labels_last", "attpc_rows_cluster")


# ------------------------------------------------------------------------------------------ the contract's names ----
def test_contract_is_declared_everywhere():
    header = (ROOT / "include" / "attpc_engine.h").read_text()
    for name in ENTRY_POINTS:
        assert re.search(rf"ATTPC_API int32_t {name}\(", header) and name in _abi.EXPORTED_SYMBOLS, name
    assert _abi.CLUSTER_SYMBOLS == ENTRY_POINTS and "clustering" in _abi.CONFIGURE_SLOTS
    for struct, cls in (("attpc_cluster_desc", _abi.ClusterDesc), ("attpc_cluster_event", _abi.ClusterEvent),
                        ("attpc_cluster_record", _abi.ClusterRecord)):
        fields = re.search(rf"typedef struct {struct} \{{([^}}]*)\}} {struct};", header).group(1)
        names = re.findall(r"^\s*(?:double|int32_t|uint16_t) (\w+)(?:\[\w+\])?;", fields, re.M)
        assert names == [name for name, _ in cls._fields_], struct
    assert (C.sizeof(_abi.ClusterDesc), C.sizeof(_abi.ClusterEvent), C.sizeof(_abi.ClusterRecord)) == (40, 64, 32)
    assert _abi.ClusterEvent.truth_rows.offset == 48 and _abi.CLUSTER_EVENT_DTYPE == np.dtype(cref.EVENT_DTYPE.descr, align=True)
    assert _abi.CLUSTER_DTYPE.descr == cref.RECORD_DTYPE.descr
    for name, value in (("ATTPC_CLUSTER_MATCH_TRUTH", _abi.CLUSTER_MATCH_TRUTH), ("ATTPC_CLUSTER_MATCH_RANK", _abi.CLUSTER_MATCH_RANK),
                        ("ATTPC_CLUSTER_CAPPED", _abi.CLUSTER_CAPPED), ("ATTPC_CLUSTER_INTERNAL", _abi.CLUSTER_INTERNAL),
                        ("ATTPC_CLUSTER_DEFAULT_MAX_ROWS", _abi.CLUSTER_DEFAULT_MAX_ROWS)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == value, name
    assert kmod.STATUS_BITS == {"CAPPED": cref.CAPPED, "INTERNAL": cref.INTERNAL}
    shared = (CSRC / "cluster_host.hpp").read_text()
    assert int(re.search(r"CLUSTER_MAX_ROWS_LIMIT = (\d+);", shared).group(1)) == _abi.CLUSTER_MAX_ROWS_LIMIT
    assert "double d" not in shared and "float" not in shared  # (the metric is integer)
    kernel = (CSRC / "cluster.hip").read_text()
    assert "asm" not in kernel and "float" not in kernel and "atomicMin(parent" in kernel
    for text in (header, shared, kernel, (ROOT / "README.md").read_text(), (ROOT / "DESIGN.md").read_text()):
        assert "HDBSCAN" in text and "DBSCAN with every tie made definite" in text.replace("\n * ", " ").replace("\n// ", " ").replace("\n", " ")
    entry = (ROOT / "__graft_entry__.py").read_text()
    assert '"cluster.hip"' in entry and '"cluster_host.hpp"' in entry


# ------------------------------------------------------------------------------------------ the cases, the restatement ----
def test_case_set_holds_what_it_names():
    cc.check_cases()


def test_restatement_on_every_case():
    """What must hold of any result, on every case and every group of settings."""
    offsets, rows, labels, names = cc.csr()
    for group, (out, events, records) in cc.reference().items():
        s = cc.GROUPS[group]
        assert set(np.unique(out)) <= {-1, *cc.INDICES}, group
        for e, name in enumerate(names):
            lo, hi = offsets[e], offsets[e + 1]
            ev, rec, lab = events[e], records[e], out[lo:hi]
            assert ev["n_rows"] == hi - lo == ev["n_core"] + ev["n_border"] + ev["n_noise"], (group, name)
            used = rec["first_row"] >= 0
            assert used.sum() == min(int(ev["n_clusters"]), 8) and np.all(used[:int(used.sum())]), (group, name)
            assert np.all(np.diff(rec["rows"][used]) <= 0), (group, name)  # by rank
            assert np.all(rec["rows"][used] >= s.min_cluster_size) and np.all(rec["core_rows"][used] >= 1)
            assert np.all((rec["majority_rows"][used] > 0) == (rec["majority"][used] >= 0))
            if ev["n_clusters"] <= 8:  # every surviving cluster is recorded: the labels are theirs
                assert ev["n_core"] + ev["n_border"] == rec["rows"][used].sum(), (group, name)
                assert (lab >= 0).sum() == rec["rows"][used & (rec["label"] >= 0)].sum(), (group, name)
            given = rec["label"][used & (rec["label"] >= 0)]
            assert len(set(given)) == len(given), (group, name)  # a label goes to one cluster
            if s.match == "truth":
                assert ev["n_split"] + ev["n_fake"] + len(given) == ev["n_clusters"] or ev["n_clusters"] > 8, (group, name)
            else:
                assert ev["n_split"] == ev["n_fake"] == 0 and list(given) == list(cc.INDICES[:len(given)]), (group, name)
            assert not np.any(np.asarray(rec[~used].tolist())[:, [0, 1, 3, 4, 5, 6, 7]]) if (~used).any() else True


def test_rows_without_truth_labels_vote_for_nobody():
    offsets, rows, labels, _ = cc.csr()
    s = cc.GROUPS["rank"]
    out, events, records = cref.cluster(s, offsets, rows, None, cc.INDICES)
    want = cc.reference()["rank"]
    assert np.array_equal(out, want[0]) and not events["truth_rows"].any() and np.all(records["majority"][records["first_row"] >= 0] == -1)
    truth = cref.cluster(cc.GROUPS["base"], offsets, rows, None, cc.INDICES)
    assert np.all(truth[0] == -1) and np.array_equal(truth[1]["n_fake"], truth[1]["n_clusters"])


@pytest.mark.parametrize("mutant", cref.MUTANTS)
def test_mutants_of_the_restatement_fail_the_comparison(mutant):
    offsets, rows, labels, names = cc.csr()
    caught = {}
    for group, s in cc.GROUPS.items():
        wrong = cref.cluster(s, offsets, rows, labels, cc.INDICES, mutant=mutant)
        want = cc.reference()[group]
        events = [names[e] for e in range(len(names))
                  if not cref.same(tuple(w[e:e + 1] if i else w[offsets[e]:offsets[e + 1]] for i, w in enumerate(wrong)),
                                   tuple(w[e:e + 1] if i else w[offsets[e]:offsets[e + 1]] for i, w in enumerate(want)))]
        if events:
            caught[group] = events
    print(mutant, "differs on", caught)
    assert caught, mutant


# ------------------------------------------------------------------------------------------ scikit-learn's DBSCAN ----
SKLEARN_EVENTS = ("line of 257", "z chain of 600", "shuffled chain of 600", "chain with a gap one unit over", "blob of 300 at one z",
                  "two clusters of equal size", "ten clusters", "cluster one row under min_cluster_size", "all noise",
                  "out-of-range rows", "tracks and noise")


# (linking lengths of 33 and 17 / 47 units: on these no pair of the events below lies exactly on the ellipsoid)
SKLEARN_SETTINGS = {"33 units": cref.Settings(33 / 16, 33 / 16, 3, 5), "33 units, min_samples 4": cref.Settings(33 / 16, 33 / 16, 4, 5),
                    "17 and 47 units": cref.Settings(17 / 16, 47 / 16, 3, 5), "47 and 17 units": cref.Settings(47 / 16, 17 / 16, 5, 5)}
# (... but for at most one event per settings, which has such a pair and is left out by name; every other one is asserted)
SKLEARN_LEFT_OUT = {"33 units": "chain with a gap one unit over", "33 units, min_samples 4": "chain with a gap one unit over",
                    "17 and 47 units": "blob of 300 at one z", "47 and 17 units": None}


@pytest.mark.parametrize("which", list(SKLEARN_SETTINGS))
def test_sklearn_dbscan_agrees(which):
    """On the quantised coordinates scaled by 1/Exy, 1/Exy, 1/Ez an ellipsoid of the contract is the unit ball, so
    DBSCAN(eps=1) has the contract's neighbours wherever no pair lies on the surface (sklearn compares rounded square
    roots there), which is asserted for every event used."""
    sklearn_cluster = pytest.importorskip("sklearn.cluster", reason="scikit-learn is not installed")
    offsets, rows, labels, names = cc.csr()
    s = SKLEARN_SETTINGS[which]
    exy, ez = s.units()
    borders = 0
    for name in SKLEARN_EVENTS:
        if name == SKLEARN_LEFT_OUT[which]:  # a pair on the surface: not an event for sklearn under these settings
            continue
        e = names.index(name)
        d = {}
        cref.cluster_event(s, rows[offsets[e]:offsets[e + 1]], labels[offsets[e]:offsets[e + 1]], list(cc.INDICES), detail=d)
        assert not (d["d"] == exy * exy * ez * ez).any(), (which, name)
        row_of = d["row_of"]
        _, X, Y, Z = cref.quantise(rows[offsets[e]:offsets[e + 1]])
        scaled = np.stack([X[row_of] / exy, Y[row_of] / exy, Z[row_of] / ez], axis=1)
        # (|dZ| <= Ez is implied by d <= Exy^2 Ez^2: the unit ball lies inside the slab)
        fit = sklearn_cluster.DBSCAN(eps=1.0, min_samples=s.min_samples, algorithm="brute").fit(scaled)
        core = np.zeros(len(scaled), dtype=bool)
        core[fit.core_sample_indices_] = True
        assert np.array_equal(core, d["core"]), (which, name)
        ours, theirs = d["cluster"][core], fit.labels_[core]
        pairs = set(zip(ours.tolist(), theirs.tolist()))  # the partition of the core rows: a bijection of the ids
        assert len(pairs) == len(set(ours.tolist())) == len(set(theirs.tolist())), (which, name)
        for i in np.flatnonzero(~core & (d["cluster"] >= 0)):  # a border row lies in a cluster of one of its core neighbours
            assert d["cluster"][i] in set(d["cluster"][np.flatnonzero(d["near"][i] & core)].tolist()), (which, name, i)
            borders += 1
        assert np.array_equal(fit.labels_ < 0, d["cluster"] < 0), (which, name)  # noise, before the size cut
    print(which, "border rows checked:", borders, "left out:", SKLEARN_LEFT_OUT[which])
    assert borders > 0, which


# ------------------------------------------------------------------------------------------ the host code alone ----
def _gxx():
    exe = shutil.which("g++")
    if exe is None:
        pytest.skip("g++ not available")
    return exe


def _build(exe: Path, flags: list) -> None:
    cmd = [_gxx(), "-std=c++17", "-Wall", "-Wno-unknown-pragmas", f"-I{CSRC}", f"-I{ROOT / 'include'}", *flags,
           "-o", str(exe), str(ROOT / "tests" / "native" / "cluster_check.cpp")]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]


def _settings_words(s: cref.Settings, indices=cc.INDICES, **changes) -> np.ndarray:
    head = {"eps_xy": s.eps_xy, "eps_z": s.eps_z, "min_samples": s.min_samples, "min_cluster_size": s.min_cluster_size,
            "max_rows": s.max_rows, "match": {"truth": 0, "rank": 1}.get(s.match, s.match), "reserved0": 0, "reserved1": 0,
            "n_sim": len(indices)}
    head.update(changes)
    return np.array([*head.values(), *indices, *[-1] * (8 - len(indices))], dtype=np.float64)


def _run(exe: Path, tmp: Path, mode: str, data: np.ndarray) -> np.ndarray:
    (tmp / "in.bin").write_bytes(np.ascontiguousarray(data, dtype=np.float64).tobytes())
    run = subprocess.run([str(exe), mode, str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True)
    assert run.returncode == 0 and "ERROR" not in run.stderr and "runtime error" not in run.stderr, (run.returncode, run.stderr[-3000:])
    return np.frombuffer((tmp / "out.bin").read_bytes(), dtype=np.float64)


def _csr_words(offsets, rows, labels) -> np.ndarray:
    body = np.concatenate([rows, np.asarray(labels, dtype=np.float64)[:, None]], axis=1).ravel()
    return np.concatenate([[len(offsets) - 1], np.asarray(offsets, dtype=np.float64), body])


def _native(exe, tmp, s: cref.Settings, offsets, rows, labels, indices=cc.INDICES):
    """The stand-alone program on a CSR array -> (labels, events, records) as the restatement gives them."""
    out = _run(exe, tmp, "rows", np.concatenate([_settings_words(s, indices), _csr_words(offsets, rows, labels)]))
    n, total = len(offsets) - 1, int(offsets[-1])
    table = out[total:total + 18 * n].reshape(n, 18).astype(np.int64)
    events = np.zeros(n, dtype=cref.EVENT_DTYPE)
    for k, name in enumerate(cref.EVENT_DTYPE.names[:10]):
        events[name] = table[:, k]
    events["truth_rows"] = table[:, 10:]
    fields = out[total + 18 * n:].reshape(n, 8, 8).astype(np.int64)
    records = np.zeros((n, 8), dtype=cref.RECORD_DTYPE)
    for k, name in enumerate(cref.RECORD_DTYPE.names):
        records[name] = fields[:, :, k]
    return out[:total].astype(np.int64), events, records


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cluster")
    exe = tmp / "cluster_check"
    _build(exe, ["-O2"])
    return exe, tmp


def test_host_form_equals_the_restatement(native):
    exe, tmp = native
    offsets, rows, labels, _ = cc.csr()
    for group, s in cc.GROUPS.items():
        assert cref.same(_native(exe, tmp, s, offsets, rows, labels), cc.reference()[group]), group
    # a layout that gives a label twice, a negative index, and eight positions
    for indices in ((2, 2, 0), (-1, 2, 0), (0, 1, 2, 3, 4, 5, 6, 7), ()):
        for group in ("base", "rank"):
            s = cc.GROUPS[group]
            assert cref.same(_native(exe, tmp, s, offsets, rows, labels, indices), cref.cluster(s, offsets, rows, labels, indices)), indices


def test_sanitized_build_runs_clean(tmp_path):
    """The same program under AddressSanitizer and UndefinedBehaviorSanitizer, stand-alone."""
    exe = tmp_path / "cluster_check_san"
    _build(exe, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    offsets, rows, labels, _ = cc.csr()
    for group in ("base", "rank", "four", "capped"):
        assert cref.same(_native(exe, tmp_path, cc.GROUPS[group], offsets, rows, labels), cc.reference()[group]), group
    for field, value in BAD_SETTINGS:
        assert _run(exe, tmp_path, "desc", _settings_words(cc.GROUPS["base"], **{field: value})).tolist() == [1.0], (field, value)


def test_host_checks_the_order_of_the_rows(native):
    exe, tmp = native
    offsets, rows, labels, names = cc.csr()
    s = cc.GROUPS["base"]
    words = _run(exe, tmp, "sorted", np.concatenate([_settings_words(s), _csr_words(offsets, rows, labels)]))
    assert words.tolist() == [1.0] * len(names)  # (the out-of-range rows in the middle do not count)
    swapped = rows.copy()
    lo = offsets[names.index("line of 255")]
    swapped[[lo + 3, lo + 4]] = swapped[[lo + 4, lo + 3]]
    words = _run(exe, tmp, "sorted", np.concatenate([_settings_words(s), _csr_words(offsets, swapped, labels)]))
    assert [names[e] for e in np.flatnonzero(words == 0.0)] == ["line of 255"]


# ------------------------------------------------------------------------------------------ the settings ----
BAD_SETTINGS = [("eps_xy", v) for v in (0.0, 0.0624, 64.001, -1.0, float("nan"), float("inf"))] + \
               [("eps_z", v) for v in (0.0, 0.06, 65.0, float("nan"), -float("inf"))] + \
               [("min_samples", 0), ("min_samples", -3), ("min_cluster_size", 0), ("max_rows", 0), ("max_rows", 65536),
                ("max_rows", -1), ("match", 2), ("match", -1), ("reserved0", 1), ("reserved1", -1), ("n_sim", 9), ("n_sim", -1)]
GOOD_SETTINGS = [("eps_xy", 0.0625), ("eps_xy", 64.0), ("eps_z", 0.0625), ("eps_z", 64.0), ("min_samples", 1),
                 ("min_samples", 2**31 - 1), ("min_cluster_size", 1), ("max_rows", 1), ("max_rows", 65535), ("match", 1),
                 ("n_sim", 0), ("n_sim", 8)]


def test_host_desc_checks(native):
    exe, tmp = native
    s = cc.GROUPS["base"]
    assert _run(exe, tmp, "desc", _settings_words(s)).tolist() == [0.0]
    for field, value in GOOD_SETTINGS:
        assert _run(exe, tmp, "desc", _settings_words(s, **{field: value})).tolist() == [0.0], (field, value)
    for field, value in BAD_SETTINGS:
        assert _run(exe, tmp, "desc", _settings_words(s, **{field: value})).tolist() == [1.0], (field, value)
        if field in cref.Settings.__dataclass_fields__ and field != "match":
            assert cref.desc_error(cref.Settings(**{**vars(s), field: value})), (field, value)


def test_argument_checks():
    for field in ("eps_xy", "eps_z"):
        for bad in (0.0, 0.06, 64.5, float("nan"), float("inf"), -2.0, "2", True, None):
            with pytest.raises(ValueError):
                ClusterSettings(**{field: bad})
    for field, lo in (("min_samples", 1), ("min_cluster_size", 1), ("max_rows", 1)):
        for bad in (lo - 1, -5, 2.0, "3", True, None):
            with pytest.raises(ValueError):
                ClusterSettings(**{field: bad})
    for bad in (65536, 2**31):
        with pytest.raises(ValueError):
            ClusterSettings(max_rows=bad)
    for bad in ("Truth", 0, None, "hdbscan"):
        with pytest.raises(ValueError):
            ClusterSettings(match=bad)
    good = ClusterSettings()
    assert good.token() == (20.0, 20.0, 5, 10, 16384, "truth")  # the issue's starting point
    desc = ClusterSettings(1.5, 0.0625, 2, 3, np.int64(65535), "rank").desc()
    assert (desc.eps_xy, desc.eps_z, desc.min_samples, desc.min_cluster_size, desc.max_rows, desc.match) == (1.5, 0.0625, 2, 3, 65535, 1)
    assert list(desc.reserved) == [0, 0]
    with pytest.raises(TypeError):
        configure_clustering(None, "settings")
    with pytest.raises(TypeError):
        rows_to_clusters([0], np.zeros((0, 8)), [], cc.INDICES, "settings")
    with pytest.raises(ValueError):
        rows_to_clusters([0, 2], np.zeros((1, 8)), [0], cc.INDICES, good)
    with pytest.raises(ValueError):
        rows_to_clusters([0, 1], np.zeros((1, 8)), [0, 1], cc.INDICES, good)
    with pytest.raises(ValueError):
        rows_to_clusters([0, 1], np.zeros((1, 8)), [0], range(9), good)


# ------------------------------------------------------------------------------------------ the scores ----
def test_scores_are_those_of_the_labels():
    offsets, rows, labels, names = cc.csr()
    out, events, records = cc.reference()["base"]
    completeness, purity = cluster_scores(events, records)
    assert completeness.shape == purity.shape == (len(names), 8)
    for e, name in enumerate(names):
        lab, truth = out[offsets[e]:offsets[e + 1]], labels[offsets[e]:offsets[e + 1]]
        for s, index in enumerate(cc.INDICES):
            mine = lab == index
            if not mine.any():
                assert np.isnan(completeness[e, s]) and np.isnan(purity[e, s]), (name, s)
                continue
            matched = (mine & (truth == index)).sum()
            assert completeness[e, s] == matched / (truth == index).sum() and purity[e, s] == matched / mine.sum(), (name, s)
        assert np.isnan(completeness[e, len(cc.INDICES):]).all()
    e = names.index("tracks and noise")
    print("tracks and noise: completeness", completeness[e, :3], "purity", purity[e, :3])
    assert np.nanmin(completeness[e, :3]) < 1.0 or np.nanmin(purity[e, :3]) < 1.0  # (two tracks that touch, one that breaks)
    assert completeness[names.index("line of 255"), 0] == purity[names.index("line of 255"), 0] == 1.0


def test_scores_refuse_rank_matched_records():
    """Two clusters of one majority both labelled, or a labelled cluster without a majority, come from matching by rank
    only: the scores would sit in the wrong slots.  (Other rank-matched records cannot be told from truth-matched ones;
    the docstring calls their result undefined.)"""
    _, events, records = cc.reference()["base"]
    e = cc.csr()[3].index("two clusters with one majority")
    events, records = events[e:e + 1], records[e:e + 1].copy()
    assert records["majority"][0, 0] == records["majority"][0, 1] >= 0 and records["label"][0, 0] >= 0 > records["label"][0, 1]
    cluster_scores(events, records)
    both = records.copy()
    both["label"][0, 1] = cc.INDICES[1]  # what "rank" gives the second cluster
    with pytest.raises(ValueError, match="rank"):
        cluster_scores(events, both)
    nobody = records.copy()
    nobody["majority"][0, 0] = -1
    with pytest.raises(ValueError, match="rank"):
        cluster_scores(events, nobody)
    rank = cc.reference()["rank"]
    assert rank[2]["label"][e, 1] == cc.INDICES[1]
    with pytest.raises(ValueError, match="rank"):
        cluster_scores(rank[1], rank[2])


# ------------------------------------------------------------------------------------------ the Python layer ----
def _cluster_calls(lib):
    return [desc for name, desc in lib.configure_descs if name == "attpc_trace_configure_clustering"]


def test_clustering_reaches_the_library():
    from attpc_engine_amd import workloads
    from attpc_engine_amd.detector.estimate import EstimateSettings
    from attpc_engine_amd.detector.thinning import ThinSettings
    from attpc_engine_amd.detector.traces import TraceChain, configure_trace_rows
    from attpc_engine_amd.engine import Engine
    from tests.test_run_layer_cpu import RecordingContext

    pipeline, config, indices = workloads.o16aa()
    good = ClusterSettings(eps_xy=7.0, min_samples=4)
    with pytest.raises(TypeError):
        TraceChain(config, clustering="settings")
    with pytest.raises(TypeError):
        TraceChain(config).replace(clustering=EstimateSettings())
    chain = TraceChain(config, estimates=EstimateSettings(), thinning=ThinSettings(10.0), clustering=good)
    ctx = RecordingContext()
    chain.configure(ctx, rows=True)
    calls = _cluster_calls(ctx.lib)
    assert len(calls) == 1 and calls[0] == {"eps_xy": 7.0, "eps_z": 20.0, "min_samples": 4, "min_cluster_size": 10,
                                            "max_rows": 16384, "match": 0}
    names = ctx.lib.names()
    assert names.index("trace_configure_clustering") < names.index("trace_configure_estimates")
    chain.configure(ctx, rows=True)                           # the same settings again: the token skips the call
    chain.replace(clustering=None).configure(ctx, rows=True)  # off
    assert [c if c is None else c["min_samples"] for c in _cluster_calls(ctx.lib)] == [4, None]
    fresh = RecordingContext()
    TraceChain(config, clustering=good).configure(fresh)      # traces, not rows: the stage is not touched
    TraceChain(config).configure(fresh, rows=True)            # off on a context that never held it: no call
    assert _cluster_calls(fresh.lib) == []
    configure_trace_rows(config, fresh, clustering=good)
    configure_trace_rows(config, fresh)                       # None leaves what the ctx holds
    assert len(_cluster_calls(fresh.lib)) == 1
    engine = Engine(pipeline, config, indices, context=fresh)
    engine.configure_clustering()
    engine.configure_clustering(eps_z=3.0, match="rank")
    engine.configure_clustering(good)
    assert [c if c is None else (c["eps_z"], c["match"]) for c in _cluster_calls(fresh.lib)] == [(20.0, 0), None, (3.0, 1), (20.0, 0)]
    with pytest.raises(TypeError):
        engine.configure_clustering(good, eps_z=3.0)
