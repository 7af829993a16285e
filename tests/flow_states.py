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
