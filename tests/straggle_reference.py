"""The track straggling (include/attpc_engine.h, "track straggling") restated in numpy: the kick of one recorded sample
as a function of (g, m, Z, ds, n1, n2, n3, settings), the normals from the oracle's Philox with the kernel's Box-Muller,
and a whole track by looping ``tests.track_cases.next_sample`` (the oracle's right-hand side, RK4, the four terminal
events) with the kick behind every accepted sample.  No integrator of its own.

Every operation of ``kick`` is one IEEE double operation in the order csrc/straggle_host.hpp writes it (numpy never
fuses a multiply and an add), so the two agree bit for bit: tests/test_straggling_cpu.py proves it."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from tests import track_cases as tc

C_LIGHT = 299792458.0
HIGHLAND = 13.6                       # MeV
K_BOHR = 2.605634303273153e-29        # 4 pi (r_e m_e c^2)^2, MeV^2 m^2 (detector/constants.py STRAGGLE_K)
KE_LIMIT = 1.0e-6
DOMAIN_STRAGGLE = 0x10000000
TWO_PI = 2.0 * 3.141592653589793


@dataclass(frozen=True)
class Settings:
    angular_scale: float = 1.0
    energy_scale: float = 1.0
    radiation_length: float = 1.0     # m
    electron_density: float = 1.0     # 1 / m^3
    stream: int = 0


def step_length(gv2, h_sample):
    """ds of a sample: gv2 of the state at the previous recorded sample."""
    gv2 = np.float64(gv2)
    return C_LIGHT * np.sqrt(gv2 / (1.0 + gv2)) * h_sample


def basis(u):
    """The branch-free orthonormal basis (e1, e2) of Duff et al. for unit vectors u [..., 3]."""
    ux, uy, uz = u[..., 0], u[..., 1], u[..., 2]
    sign = np.copysign(1.0, uz)
    a = -1.0 / (sign + uz)
    b = ux * uy * a
    e1 = np.stack([1.0 + sign * ux * ux * a, sign * b, -sign * ux], axis=-1)
    e2 = np.stack([b, sign + uy * uy * a, -uy], axis=-1)
    return e1, e2


def theta0(g, mass, z, ds, settings: Settings):
    """The width of the angular kick for states g [..., 3]."""
    g = np.asarray(g, dtype=np.float64)
    g2 = (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]
    gm = np.sqrt(g2)
    beta = gm / np.sqrt(1.0 + g2)
    mom = mass * gm
    return settings.angular_scale * (HIGHLAND * abs(z) / (beta * mom)) * np.sqrt(ds / settings.radiation_length)


def omega2(g, mass, z, ds, settings: Settings):
    """Bohr's variance of the energy fluctuation for states g [..., 3], MeV^2."""
    g = np.asarray(g, dtype=np.float64)
    g2 = (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]
    gamma2 = 1.0 + g2
    beta2 = g2 / gamma2
    return ((settings.energy_scale * settings.energy_scale) * K_BOHR * (z * z) * settings.electron_density * ds * gamma2 *
            (1.0 - 0.5 * beta2))


def kick(g, mass, z, ds, n1, n2, n3, settings: Settings):
    """g' [..., 3] and clamped [...] of the kick of states g [..., 3]; every other argument a scalar or [...].  A part
    whose scale is 0 does not read its normals; with both scales 0 g comes back as it is."""
    g = np.asarray(g, dtype=np.float64)
    angular, energy = settings.angular_scale > 0.0, settings.energy_scale > 0.0
    if not angular and not energy:
        return g.copy(), np.zeros(g.shape[:-1], dtype=bool)
    with np.errstate(all="ignore"):
        g2 = (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]
        gm = np.sqrt(g2)
        gamma2 = 1.0 + g2
        gamma = np.sqrt(gamma2)
        direction = g / gm[..., None]
        if angular:
            beta = gm / gamma
            mom = mass * gm
            th = settings.angular_scale * (HIGHLAND * abs(z) / (beta * mom)) * np.sqrt(ds / settings.radiation_length)
            e1, e2 = basis(direction)
            t1, t2 = th * n1, th * n2
            d = (direction + t1[..., None] * e1) + t2[..., None] * e2
            dm = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
            direction = d / dm[..., None]
        mag = gm
        clamped = np.zeros(g.shape[:-1], dtype=bool)
        if energy:
            ke = mass * (g2 / (gamma + 1.0))
            beta2 = g2 / gamma2
            om2 = ((settings.energy_scale * settings.energy_scale) * K_BOHR * (z * z) * settings.electron_density * ds * gamma2 *
                   (1.0 - 0.5 * beta2))
            moved = ke - np.sqrt(om2) * n3
            clamped = ~(moved > KE_LIMIT)
            r = np.where(clamped, KE_LIMIT, moved) / mass
            mag = np.sqrt(r * (r + 2.0))
        return mag[..., None] * direction, clamped


# ------------------------------------------------------------------------------------------ random numbers ----
def _u53(a: int, b: int) -> float:
    return (float(a >> 5) * 67108864.0 + float(b >> 6)) / 9007199254740992.0


def uniforms(orc, seed: int, event: int, index: int, domain: int):
    """rng_pair: the two uniforms of the Philox4x32-10 block (event lo, event hi, index, domain) under the key seed."""
    r = orc.philox([event & 0xffffffff, event >> 32, index & 0xffffffff, domain], [seed & 0xffffffff, seed >> 32])
    return _u53(int(r[0]), int(r[1])), _u53(int(r[2]), int(r[3]))


def normals(orc, seed: int, event: int, k: int, row: int, stream: int):
    """(n1, n2, n3) of sample k: Box-Muller (cos, sin) of pair 2 k, cos of pair 2 k + 1, domain DOMAIN_STRAGGLE +
    stream * 32 + row."""
    domain = DOMAIN_STRAGGLE + stream * 32 + row
    ua, ub = uniforms(orc, seed, event, 2 * k, domain)
    rad = math.sqrt(-2.0 * math.log(1.0 - ua))
    n1, n2 = rad * math.cos(TWO_PI * ub), rad * math.sin(TWO_PI * ub)
    ua, ub = uniforms(orc, seed, event, 2 * k + 1, domain)
    n3 = math.sqrt(-2.0 * math.log(1.0 - ua)) * math.cos(TWO_PI * ub)
    return n1, n2, n3


# ------------------------------------------------------------------------------------------ a whole track ----
def track(orc, det, species_index: int, momentum, vertex, settings: Settings, draw, max_samples: int = tc.TIME_SAMPLES):
    """The recorded states [n, 6] (x, y, z, gamma beta) of one track with the kick behind every accepted sample, and
    what happened: ``margin``, the smallest |event function| met at any step, the firing one included (a clamped "ke",
    0 by definition, left out) -- a track whose margin is below a rounding difference may end one step apart
    elsewhere --, ``clamped``, the first sample whose energy was clamped to KE_LIMIT (None: none), and ``events``, the
    terminal events that ended the track ([]: the sample cap or the window).  ``draw(k)`` -> (n1, n2, n3) of sample k."""
    sp = det.species[species_index]
    mass, z = float(sp.mass), float(sp.Z)
    p = np.asarray(momentum, dtype=np.float64)
    state = np.array([vertex[0], vertex[1], vertex[2], p[0] / mass, p[1] / mass, p[2] / mass])
    states = [state]
    g_old = tc.event_functions(state, mass)
    margin, t_now, first_clamp, ended_by = math.inf, 0.0, None, []
    for k in range(1, max_samples):
        gv2 = (state[3] * state[3] + state[4] * state[4]) + state[5] * state[5]
        new, events, _, h_sample = tc.next_sample(orc, det, species_index, state, g_old)
        if det.path_step > 0.0:
            if t_now + h_sample > 1.0e-6 * (1.0 + 1.0e-9):
                break
            t_now += h_sample
        g_new = tc.event_functions(new, mass)
        if events or not g_new[0] == g_new[0]:
            margin = min(margin, min(abs(v) for v in g_new))
            ended_by = list(events)
            break
        ds = float(step_length(gv2, h_sample))
        g, clamped = kick(new[3:6], mass, z, ds, *draw(k), settings)
        state = np.concatenate([new[:3], g])
        g_old = tc.event_functions(state, mass)
        if bool(clamped):
            g_old = (0.0,) + tuple(g_old[1:])
            first_clamp = k if first_clamp is None else first_clamp
        margin = min(margin, min(abs(v) for v in (g_old[1:] if bool(clamped) else g_old)))
        states.append(state)
    return np.array(states), {"margin": margin, "clamped": first_clamp, "events": ended_by}


def kept_samples(orc, det, species_index: int, states: np.ndarray, seed: int, event: int, row: int):
    """The kept samples [m, 4] (x, y, time bucket, electrons * gain) of recorded states, as the oracle's
    generate_point_cloud makes them (solver.py:387-398)."""
    electrons = orc.electrons(det, species_index, states, seed, event, 1 + row)
    dv = det.length / float(det.windows_edge - det.micromegas_edge)
    keep = electrons >= 1
    out = np.empty((int(keep.sum()), 4))
    out[:, 0], out[:, 1] = states[keep, 0], states[keep, 1]
    out[:, 2] = (det.length - states[keep, 2]) / dv + float(det.micromegas_edge)
    out[:, 3] = (electrons[keep] * det.mpgd_gain).astype(np.float64)
    return out


def reference_tracks(orc, inp, p4, vertex, seed: int, first: int, settings: Settings):
    """[(kept samples [m, 4], ODE rows, info of ``track``)] of every track of a launch, in the device's order (event, simulated
    nucleus) -- what tests/test_gpu_track_paths.py's ``_oracle_tracks`` gives for the unkicked tracks."""
    out = []
    for e in range(len(p4)):
        for row in inp.indices:
            sp = inp.layout.species_of_row[row]
            event = first + e
            states, info = track(orc, inp.det_raw, sp, p4[e, row], vertex[e], settings,
                                   lambda k: normals(orc, seed, event, k, row, settings.stream))
            out.append((kept_samples(orc, inp.det_raw, sp, states, seed, event, row), len(states), info))
    return out
