"""Seeded ENERGETIC start states for the 2D solver, the cases that run from them and their float32 tolerances -- TEST
INFRASTRUCTURE shared by tests/test_flow_states_host.py, tests/test_gpu_energetic.py and oracle/make_sensitivity.py.

Why: every other comparison of an on-demand 2D kernel with the float64 oracle starts from a fluid at rest, where the convective
terms of the predictor and the velocity-dependent coefficients of the scalar transport contribute almost nothing (after 12
timesteps the largest velocity is about 0.008).  A float32 kernel that reads a wrong neighbour there stays under every float32
tolerance (DESIGN.md 21 has the measured table).  The states of this file carry velocities of 0.5 (rayleigh) and 1.0 (mixing, the speed of its lids) without any symmetry, so that
a slipped neighbour in one column or one row moves the result by 1e-4 .. 1e-2 within four timesteps.

Plain numpy, no file inputs."""
import numpy as np

NDT = 4          # timesteps of the energetic protocol
BATCH = 4        # replicas of one case, each with its own seed (state) and its own action
SEEDS = (0, 1, 2, 3)


def _smooth(rng, X, Y, L, H, n=6):
    """A sum of n long cosine waves with random amplitudes and phases, scaled to max |f| = 1: no mirror symmetry."""
    f = np.zeros_like(X)
    for _ in range(n):
        kx, ky = int(rng.integers(0, 4)), int(rng.integers(0, 4))
        f += rng.uniform(0.3, 1.0) * np.cos(kx * np.pi * X / L + rng.uniform(0, 2 * np.pi)) * np.cos(ky * np.pi * Y / H + rng.uniform(0, 2 * np.pi))
    return f / np.abs(f).max()


def energetic_state(kind, nx, ny, L, H, seed, amp=0.5, C0=1.0):
    """[4, nx+2, ny+2] float64 (u, v, p, T or C) in the reference's [i, j] layout; kind 0 = rayleigh, 1 = mixing.

    u, v: from a streamfunction at the cell corners -- twenty cosine modes with random amplitudes and phases, wavelengths down to
    a third of a unit length, times the envelope (1 - (2x/L - 1)^2m) (1 - (2y/H - 1)^2n), m = round(3 L), n = round(3 H), which
    vanishes on the walls but rises steeply from them -- differenced onto the staggered faces (the discrete divergence is zero to
    rounding) and scaled to max(|u|, |v|) = amp.  The steep envelope puts tangential velocity of the order of amp into the cells
    next to the walls; with sin(pi x / L) sin(pi y / H) the wall-adjacent columns and rows were starved (dt |conv| down to 1.5e-6
    where the interior has 1e-3), with this one every column and row keeps dt |conv| >= 1.1e-4 (tests/test_flow_states_host.py).
    The ghosts of u, v and the scalar are left to the solver's boundary stage, the first thing a timestep does.
    Scalar: rayleigh -- the conduction profile plus four long waves of amplitude <= 0.1; mixing -- a smooth field in [0.1, 0.9] C0.
    p: a smooth field of amplitude 0.05; its ghosts copy the interior neighbour (the mixing lid: 0), as in any state the
    solver itself has produced."""
    rng = np.random.default_rng([int(seed), int(kind), int(nx), int(ny)])
    dx, dy = L / nx, H / ny
    st = np.zeros((4, nx + 2, ny + 2))
    # corner (i, j), i = 1 .. nx+1, j = 1 .. ny+1, lies at ((i-1) dx, (j-1) dy); u(i, j) at ((i-1) dx, (j-1/2) dy), v(i, j) at ((i-1/2) dx, (j-1) dy)
    xc, yc = np.arange(nx + 1) * dx, np.arange(ny + 1) * dy
    X, Y = np.meshgrid(xc, yc, indexing="ij")
    psi = np.zeros_like(X)
    kxm, kym = int(np.ceil(6 * L)), int(np.ceil(6 * H))      # wavelengths down to a third of a unit length, whatever the domain
    for _ in range(20):
        kx, ky = int(rng.integers(1, kxm + 1)), int(rng.integers(1, kym + 1))
        psi += rng.uniform(0.3, 1.0) / np.sqrt(kx + ky) * np.cos(kx * np.pi * X / L + rng.uniform(0, 2 * np.pi)) * np.cos(ky * np.pi * Y / H + rng.uniform(0, 2 * np.pi))
    psi *= (1.0 - (2.0 * X / L - 1.0) ** (2 * round(3 * L))) * (1.0 - (2.0 * Y / H - 1.0) ** (2 * round(3 * H)))
    psi[0, :] = psi[-1, :] = 0.0
    psi[:, 0] = psi[:, -1] = 0.0
    u, v = st[0], st[1]
    u[1:nx + 2, 1:ny + 1] = (psi[:, 1:] - psi[:, :-1]) / dy
    v[1:nx + 1, 1:ny + 2] = -(psi[1:, :] - psi[:-1, :]) / dx
    s = amp / max(np.abs(u).max(), np.abs(v).max())
    u *= s
    v *= s
    w = u if np.abs(u).max() >= np.abs(v).max() else v        # the scaled maximum may sit one rounding off amp: state it exactly
    k = np.unravel_index(np.argmax(np.abs(w)), w.shape)
    w[k] = np.copysign(amp, w[k])
    # cell centres, ghosts included
    xm, ym = (np.arange(nx + 2) - 0.5) * dx, (np.arange(ny + 2) - 0.5) * dy
    X, Y = np.meshgrid(xm, ym, indexing="ij")
    if kind == 0:
        T = 0.5 - Y / H
        for k in range(1, 5):
            T += 0.1 * rng.uniform(-1, 1) * np.sin((1 + k % 2) * np.pi * Y / H) * np.cos(k * np.pi * X / L + rng.uniform(0, 2 * np.pi))
        st[3] = T
    else:
        st[3] = C0 * (0.5 + 0.4 * _smooth(rng, X, Y, L, H))
    st[3, 0, :] = st[3, -1, :] = 0.0
    st[3, :, 0] = st[3, :, -1] = 0.0
    p = 0.05 * _smooth(rng, X, Y, L, H)
    p[0, :], p[-1, :] = p[1, :], p[-2, :]
    p[:, 0] = p[:, 1]
    p[:, -1] = p[:, -2] if kind == 0 else 0.0
    p[0, 0] = p[0, -1] = p[-1, 0] = p[-1, -1] = 0.0
    st[2] = p
    return st


def _extent(c, n):
    """A domain length whose grid is exactly c cells of 1 / n (int(n L) == c)."""
    return c / n if int(n * (c / n)) == c else (c + 0.5) / n


def _case(kind, nx, ny, dtype, builtin=0, L=None, H=None, **kw):
    """builtin: 0, or the rows per lane of the kernel the library itself has for this grid (on-demand grids: jit.choose() says)."""
    n = 50.0 if kind == 0 else 100.0
    return dict(kind=kind, nx=nx, ny=ny, L=_extent(nx, n) if L is None else L, H=_extent(ny, n) if H is None else H, dtype=dtype,
                builtin=bool(builtin), rows=builtin or None, kw=kw, amp=0.5 if kind == 0 else 1.0)


# The cases of tests/test_gpu_energetic.py: the built-in grids of the library, then per (rows per lane, dtype, env) the smallest
# on-demand grid that __graft_entry__.build() compiles anyway (beacon_amd/jit.py: TEST_GRIDS, PRM_TEST_GRIDS, BOUNDARY_GRIDS), then
# one fuzzed grid with dx != dy (dx / dy = 0.9924) and the reference's other constructor arguments.
CASES = [
    _case(0, 50, 50, "f32", 1), _case(0, 50, 50, "f64", 1), _case(0, 128, 64, "f32", 1), _case(0, 128, 64, "f64", 1),       # ns2d_fast
    _case(1, 100, 100, "f32", 2), _case(1, 100, 100, "f64", 2),                                                               # ns2d_fast2
    _case(0, 75, 50, "f32"), _case(0, 75, 50, "f64"),               # one row per lane
    _case(0, 50, 75, "f32"), _case(0, 50, 75, "f64"),               # two rows per lane
    _case(0, 50, 150, "f32"), _case(0, 50, 150, "f64"),             # the hybrid
    _case(1, 100, 110, "f32"), _case(1, 100, 105, "f64"),           # mixing, two rows per lane
    _case(1, 100, 130, "f32"), _case(1, 105, 100, "f64"),           # mixing, the hybrid
    _case(0, 96, 65, "f32", L=1.92, H=1.31, n_sgts=3, ra=69000.0),  # dx != dy: jacobi_cell_eq is the dx == dy form
]


# The float32 one-row-per-lane strip widths that state their Jacobi cells in runs (csrc/bcn_jacobi_cells.h), one on-demand rayleigh
# grid per width: (nx, ny, strip width R, columns of the last strip RL).  R: every width in 7..26 with R - 4 <= 3 or R - 4 >= 8 (on
# eight waves nx >= 50 gives R >= 7).  RL: 3 (the four exchanged cells stay cell by cell), and 8..11 -- bodies of widths that no R
# takes the runs at, but a last strip does, because the kernel's R does.  ny = 64: no product with the activity mask of the lanes.
# beacon_amd/jit.py builds each twice (RUNS_GRIDS: with runs and cell by cell); tests/test_jacobi_runs_host.py checks the mappings,
# tests/test_gpu_jacobi_twins.py holds the two builds to each other bit for bit and both to the float64 oracle.
RUNS_TABLE = [(52, 50, 7, 3), (56, 64, 7, 7), (90, 50, 12, 6), (104, 64, 13, 13), (105, 50, 14, 7), (113, 50, 15, 8), (121, 50, 16, 9),
              (129, 64, 17, 10), (137, 50, 18, 11), (152, 50, 19, 19), (153, 50, 20, 13), (168, 50, 21, 21), (169, 50, 22, 15),
              (184, 50, 23, 23), (185, 50, 24, 17), (195, 50, 25, 20), (201, 50, 26, 19)]


def case_id(c):
    return "%s-%dx%d-%s" % (("rayleigh", "mixing")[c["kind"]], c["nx"], c["ny"], c["dtype"])


def grid_id(c):
    """Key of a case in tests/golden/energetic_sensitivity.json: the oracle is float64, so f32 and f64 cases of a grid share it."""
    return "%s-%dx%d" % (("rayleigh", "mixing")[c["kind"]], c["nx"], c["ny"])


def grids():
    """The distinct grids of CASES, in order."""
    seen, out = set(), []
    for c in CASES:
        if grid_id(c) not in seen:
            seen.add(grid_id(c))
            out.append(c)
    return out


def case_inputs(c, amp=None):
    """(states [BATCH, 4, nx+2, ny+2], actions) of a case: replica b starts from energetic_state(seed = SEEDS[b]) and takes its own
    action -- rayleigh: uniform in [-1, 1] per segment from the replica's seed; mixing: action b."""
    amp = c["amp"] if amp is None else amp
    st = np.stack([energetic_state(c["kind"], c["nx"], c["ny"], c["L"], c["H"], s, amp, **({"C0": c["kw"]["C0"]} if "C0" in c["kw"] else {}))
                   for s in SEEDS])
    if c["kind"] == 0:
        acts = np.stack([np.random.default_rng(1000 + s).uniform(-1, 1, c["kw"].get("n_sgts", 10)) for s in SEEDS])
    else:
        acts = np.arange(BATCH)
    return st, acts


def rows(c):
    """Rows per lane of the register-resident kernel of a case: 1 = ns2d_fast, 2 = ns2d_fast2, 4 = ns2d_fast4 (the hybrid)."""
    if c["rows"]:
        return c["rows"]
    from beacon_amd import jit
    return jit.choose(c["nx"], c["ny"], c["dtype"] == "f64", c["kind"])["rows"]


def family(c):
    """Tolerance family of a float32 case: (rows per lane of its register-resident kernel, env kind)."""
    return (rows(c), c["kind"])


def f32tol(u, v, p, S, obs, rwd):
    return dict(u=u, v=v, p=p, T=S, C=S, S=S, obs=obs, rwd=rwd)


# float32 tolerances of tests/test_gpu_energetic.py by (rows per lane, env): 10 x the largest distance from the float64 oracle
# MEASURED on the MI355X over the family's cases, the three runs (generic kernel, register-resident kernel plain and ticketed) and the
# four replicas; m: u v p T/C obs rwd.  tests/test_flow_states_host.py caps them from the reference alone: every catalogued one-column /
# one-row slip of tests/golden/energetic_sensitivity.json must exceed one of the u, v, T/C, obs entries tenfold.
F32_ENERGETIC = {
    # rayleigh, one row per lane: 50x50, 128x64 (the library's own kernels), 75x50
    (1, 0): f32tol(6.2e-7, 5.7e-7, 2.4e-5, 2.5e-6, 1.5e-6, 3.1e-5),     # m: 6.2e-08 5.7e-08 2.4e-06 2.5e-07 1.5e-07 3.1e-06
    # rayleigh, two rows per lane: 50x75, 96x65 (dx != dy)
    (2, 0): f32tol(9.5e-7, 8.6e-7, 7.3e-5, 2.7e-6, 1.5e-6, 3.4e-5),     # m: 9.5e-08 8.6e-08 7.3e-06 2.7e-07 1.5e-07 3.4e-06
    # rayleigh, the hybrid: 50x150
    (4, 0): f32tol(9.0e-7, 1.1e-6, 3.0e-5, 2.3e-6, 1.6e-6, 3.7e-5),     # m: 9.0e-08 1.1e-07 3.0e-06 2.3e-07 1.6e-07 3.7e-06
    # mixing, two rows per lane: 100x100 (the library's own kernel), 100x110
    (2, 1): f32tol(1.1e-6, 1.2e-6, 1.0e-5, 2.3e-6, 1.5e-6, 3.9e-7),     # m: 1.1e-07 1.2e-07 1.0e-06 2.3e-07 1.5e-07 3.9e-08
    # mixing, the hybrid: 100x130
    (4, 1): f32tol(1.1e-6, 1.1e-6, 1.1e-5, 2.3e-6, 1.4e-6, 5.9e-7),     # m: 1.1e-07 1.1e-07 1.1e-06 2.3e-07 1.4e-07 5.9e-08
}
# tests/test_gpu_jacobi_twins.py: rayleigh, one row per lane, the 17 on-demand grids of RUNS_TABLE (52x50 .. 201x50), 3 replicas, against
# the float64 oracle.  None of them exceeds the family's entry, so it stands.  Worst over the 17 grids, MEASURED on the MI355X:
#   register-resident (plain and ticketed, both plans)   m: 5.1e-08 4.2e-08 4.1e-06 2.4e-07 1.9e-07 4.8e-06
#   generic kernel, same inputs                           m: 5.1e-08 4.1e-08 4.3e-06 3.0e-07 1.5e-07 4.1e-06
# (p, T/C, obs and rwd lie above the three grids' figures beside (1, 0), within its tenfold margin.  Per grid and field the
# register-resident error is 0.08 .. 3.2 x the generic kernel's -- 153x50 p 1.7e-6 against 5.5e-7, 201x50 rwd 4.8e-6 against 1.5e-6 at
# the top, 185x50 p 3.1e-7 against 3.7e-6 at the bottom.  p follows the stop sweep, which float32 rounding moves by one in solves of
# 10^4 sweeps, in either kernel: on the 8 grids where all 12 sweep counts of the register-resident run are the oracle's its p error
# is 9.8e-8 .. 6.5e-7, on the 9 where one to six differ, 153x50 among them, 9.0e-7 .. 4.1e-6.  rwd: the register-resident kernel is
# below the generic one on 14 of the 17 grids, both between 1.3e-6 and 4.8e-6 -- taken to be the rounding of two float32 reductions
# in different orders; T, which rwd is computed from, agrees on 201x50 (2.3e-7, 2.4e-7).  The cell-by-cell twins give the same bits,
# so none of it is the runs'.)
F32_RUNS_GRIDS = F32_ENERGETIC[(1, 0)]
