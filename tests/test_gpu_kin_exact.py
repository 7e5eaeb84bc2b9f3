"""The device's 4-vectors against exact arithmetic: ``tests/golden/kin_exact.npz`` holds the rows that
``tests/kin_exact_reference.py`` (mpmath, 60 digits, a formula of its own) gives for 1059 cases; this file needs only
the fixture and numpy.  One ``attpc_kin_calculate`` launch per chain and one ``attpc_decay_calculate`` launch per set of
explicit parents, judged by ``tests/kin_exact_check.py`` exactly as ``test_kin_exact_cpu.py`` judges the oracle.
``kin_run_kernel`` samples its own parameters, so there the invariants of its rows are checked instead.
Needs a real MI355X: run with ``-m gpu``."""
import numpy as np
import pytest

from attpc_engine_amd import _abi
from tests import kin_exact_check as chk
from tests.helpers import Inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return _abi.Context(0)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return chk.load(golden_dir)


def _device_chain(ctx, fx, name):
    """As test_gpu_parity.py::test_kin_calculate_golden configures and launches it."""
    masses = fx[f"{name}_masses"]
    desc = _abi.KinDesc()
    desc.n_steps = 1 + (len(masses) - 4) // 2
    desc.sample_limit = 1
    for i, m in enumerate(masses):
        desc.masses[i] = m
    ctx.check(ctx.lib.attpc_kin_configure(ctx.handle, desc), "configure")
    ctx._kin_owner = None
    n = len(fx[f"{name}_beam"])
    p4 = np.empty((n, len(masses), 4))
    status = np.empty(n, dtype=np.int32)
    args = [np.ascontiguousarray(fx[f"{name}_{k}"]) for k in ("beam", "ex", "th", "ph")]
    ctx.check(ctx.lib.attpc_kin_calculate(ctx.handle, n, *[_abi.dptr(a) for a in args], _abi.dptr(p4),
                                          _abi.iptr(status, _abi.C.c_int32)), "calculate")
    return p4, np.where(status == -2, 1, status)  # the fixture's convention: "not allowed" is tested first


def _device_decays(ctx, fx, name):
    m1, m2 = (float(v) for v in fx[f"{name}_m"])
    args = [np.ascontiguousarray(fx[f"{name}_{k}"]) for k in ("parent", "ex", "th", "ph")]
    n = len(args[1])
    p4 = np.empty((n, 2, 4))
    status = np.empty(n, dtype=np.int32)
    ctx.check(ctx.lib.attpc_decay_calculate(ctx.handle, n, _abi.dptr(args[0]), m1, m2, *[_abi.dptr(a) for a in args[1:]],
                                            _abi.dptr(p4), _abi.iptr(status, _abi.C.c_int32)), "decay_calculate")
    return p4, status


def test_device_against_exact(ctx, fx):
    """Decided cases: status equal, rows within 4 K_dev S_row of the exact rows, bulk and angle also within 1e-9 MeV;
    hair cases: status 0 means finite rows within the bound, a forbidden case is NaN.  No decided case is left out:
    the cases compared are counted per class."""
    sizes = [len(fx[f"{name}_class"]) for name in list(fx["chains"]) + list(fx["decay_sets"])]
    assert max(sizes) <= 600 and any(s > 256 and s % 256 for s in sizes)  # one launch past a block, with a ragged end
    tally = chk.Tally()
    results = [(str(name), _device_chain(ctx, fx, str(name))) for name in fx["chains"]]
    results += [(str(name), _device_decays(ctx, fx, str(name))) for name in fx["decay_sets"]]
    failures = []
    for name, (p4, status) in results:  # every launch is judged before the first failure is raised
        try:
            chk.compare(fx, name, p4, status, chk.K_DEVICE, tally)
        except AssertionError as err:
            failures.append(str(err))
        measured = chk.Tally()
        try:
            chk.compare(fx, name, p4, status, np.inf, measured)
        except AssertionError:
            pass
        print(f"\n{name}: largest error / S_row {measured.worst[0]:.4f} at {measured.worst[1]}; "
              f"bulk / angle {measured.worst_plain[0]:.3e} MeV at {measured.worst_plain[1]}")
    assert not failures, "\n".join(failures)
    tally.assert_complete()
    print(f"\ndevice vs exact: largest error / S_row {tally.worst[0]:.4f} at {tally.worst[1]}; "
          f"largest bulk / angle error {tally.worst_plain[0]:.3e} MeV at {tally.worst_plain[1]}")


def _no_negative_excitation(d) -> bool:
    """Can the sampler of this step return a negative excitation?  A Gaussian draw is at most 8.6 sigma from its
    centre (Box-Muller on a 53-bit uniform: sqrt(-2 ln 2^-53))."""
    if d.kind == _abi.EX_GAUSSIAN:
        return d.p0 - 9.0 * abs(d.p1) >= 0.0
    if d.kind == _abi.EX_UNIFORM:
        return min(d.p0, d.p1) >= 0.0
    return False


def _mass(rows):
    m2 = rows[..., 3] ** 2 - (rows[..., 0] ** 2 + rows[..., 1] ** 2 + rows[..., 2] ** 2)
    return np.sign(m2) * np.sqrt(np.abs(m2))


@pytest.mark.parametrize("name", ["be10dp", "b10chain"])
def test_kin_run_invariants(ctx, name):
    """Sampled events: what must hold of rows that are within tau = 1e-9 MeV of exact ones, in long double."""
    tau = np.longdouble(1e-9)
    inp = Inputs(name, context=ctx)
    _, p4, status, _ = inp.pipeline.run_many(4000, return_status=True)
    good = status == 0
    assert good.sum() >= 3900
    assert np.isfinite(p4[good]).all()                                   # status 0 never carries a NaN
    rows = p4[good].astype(np.longdouble)
    masses = np.array(list(inp.kin.masses), dtype=np.longdouble)
    assert np.abs(rows[:, 0] + rows[:, 1] - (rows[:, 2] + rows[:, 3])).max() <= 2 * tau
    n_steps = inp.kin.n_steps
    for s in range(n_steps):
        eject, resid = (2, 3) if s == 0 else (4 + 2 * (s - 1), 5 + 2 * (s - 1))
        if s > 0:  # a parent is the sum of its two products
            parent = 3 if s == 1 else 5 + 2 * (s - 2)
            assert np.abs(rows[:, parent] - (rows[:, eject] + rows[:, resid])).max() <= 2 * tau, s
        # a row within tau of exact in every component is within 4 tau E / M of its mass shell
        m_eject = _mass(rows[:, eject])
        assert (np.abs(m_eject - masses[eject]) <= 4 * tau * rows[:, eject, 3] / m_eject).all(), s
        if _no_negative_excitation(inp.kin.excitation[s]):
            m_resid = _mass(rows[:, resid])
            assert (m_resid >= masses[resid] - 4 * tau * rows[:, resid, 3] / m_resid).all(), s
