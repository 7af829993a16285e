"""The energetic start states keep their promises (tests/flow_states.py), and the float32 tolerances of
tests/test_gpu_energetic.py stay under what the reference says a slipped neighbour costs (tests/golden/energetic_sensitivity.json,
written by oracle/make_sensitivity.py).  CPU only."""
import ctypes as C
import functools
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import flow_states as FS
from conftest import GOLD
from oracle import make_sensitivity as MS
from oracle import oracle as O

GRIDS = FS.grids()
GRID_IDS = [FS.grid_id(c) for c in GRIDS]
CAP_FIELDS = ("u", "v", "S", "obs")


def _sens():
    with open(os.path.join(GOLD, "energetic_sensitivity.json")) as fh:
        return json.load(fh)


def _loosest_uv():
    assert FS.F32_ENERGETIC, "flow_states.F32_ENERGETIC is empty"
    return max(max(t["u"], t["v"]) for t in FS.F32_ENERGETIC.values())


def _with_ghosts(c, st, a):
    """u, v with the ghosts the solver's boundary stage gives them (the oracle's own orc_ns2d_bc, replica's action)."""
    o = O.rayleigh(init=False, L=c["L"], H=c["H"], **c["kw"]) if c["kind"] == 0 else O.mixing(L=c["L"], H=c["H"], **c["kw"])
    o.st[:4] = st
    w = [0.0] * 4
    if c["kind"] == 0:
        av = np.array(a, dtype=np.float64)
        O.lib().orc_rayleigh_condition_action(C.byref(o.cfg), O.dp(av))
    else:
        av = np.array([float(a)])
        um = o.cfg.u_max      # mixing.py:212-234 (u_t, u_b, v_l, v_r)
        w = {0: (-um, um, 0.0, 0.0), 1: (um, -um, 0.0, 0.0), 2: (0.0, 0.0, -um, um), 3: (0.0, 0.0, um, -um)}[int(a)]
    O.lib().orc_ns2d_bc(C.byref(o.cfg), O.dp(o.u), O.dp(o.v), O.dp(o.S), O.dp(av), *[C.c_double(x) for x in w])
    return o.u.copy(), o.v.copy(), o.cfg.dx, o.cfg.dy, o.cfg.dt


def _conv(u, v, nx, ny, dx, dy):
    """The convective terms of oracle/beacon_oracle.c:87-119 in numpy: (conv of u* for i = 2..nx, j = 1..ny; of v* for i = 1..nx, j = 2..ny)."""
    i, j = np.meshgrid(np.arange(2, nx + 1), np.arange(1, ny + 1), indexing="ij")
    uE, uW = 0.5 * (u[i + 1, j] + u[i, j]), 0.5 * (u[i, j] + u[i - 1, j])
    uN, uS = 0.5 * (u[i, j + 1] + u[i, j]), 0.5 * (u[i, j] + u[i, j - 1])
    vN, vS = 0.5 * (v[i, j + 1] + v[i - 1, j + 1]), 0.5 * (v[i, j] + v[i - 1, j])
    cu = (uE * uE - uW * uW) / dx + (uN * vN - uS * vS) / dy
    i, j = np.meshgrid(np.arange(1, nx + 1), np.arange(2, ny + 1), indexing="ij")
    vE, vW = 0.5 * (v[i + 1, j] + v[i, j]), 0.5 * (v[i, j] + v[i - 1, j])
    uE, uW = 0.5 * (u[i + 1, j] + u[i + 1, j - 1]), 0.5 * (u[i, j] + u[i, j - 1])
    vN, vS = 0.5 * (v[i, j + 1] + v[i, j]), 0.5 * (v[i, j] + v[i, j - 1])
    cv = (uE * vE - uW * vW) / dx + (vN * vN - vS * vS) / dy
    return cu, cv


@pytest.mark.parametrize("c", GRIDS, ids=GRID_IDS)
def test_energetic_state_properties(c):
    """Per grid and seed of the GPU test: interior discrete divergence <= 1e-12, max(|u|, |v|) == amp exactly, u and v differ from
    their x-mirror and their y-mirror by more than 0.1 amp, the scalar of mixing stays inside [0, C0], and the same seed gives the
    same state while two seeds do not."""
    nx, ny = c["nx"], c["ny"]
    dx, dy = c["L"] / nx, c["H"] / ny
    st, _ = FS.case_inputs(c)
    AMP = c["amp"]
    assert st.shape == (FS.BATCH, 4, nx + 2, ny + 2) and st.dtype == np.float64 and np.isfinite(st).all()
    assert np.array_equal(st, FS.case_inputs(c)[0])
    for b in range(FS.BATCH):
        u, v, p, S = st[b]
        div = (u[2:nx + 2, 1:ny + 1] - u[1:nx + 1, 1:ny + 1]) / dx + (v[1:nx + 1, 2:ny + 2] - v[1:nx + 1, 1:ny + 1]) / dy
        assert np.abs(div).max() <= 1e-12, (b, np.abs(div).max())
        assert max(np.abs(u).max(), np.abs(v).max()) == AMP
        assert not u[1].any() and not u[nx + 1].any() and not v[:, 1].any() and not v[:, ny + 1].any()      # no flow through a wall
        uf, vf = u[1:nx + 2, 1:ny + 1], v[1:nx + 1, 1:ny + 2]          # the faces of u, of v: each set maps onto itself under both mirrors
        for f in (uf, vf):
            assert np.abs(f - f[::-1]).max() > 0.1 * AMP and np.abs(f - f[:, ::-1]).max() > 0.1 * AMP, b
            assert np.abs(f + f[::-1]).max() > 0.1 * AMP and np.abs(f + f[:, ::-1]).max() > 0.1 * AMP, b
        assert 0.03 <= np.abs(p).max() <= 0.05 + 1e-15 and np.abs(p - p[::-1]).max() > 0.01 and np.abs(p - p[:, ::-1]).max() > 0.01
        if c["kind"] == 1:
            assert S.min() >= 0.0 and S.max() <= c["kw"].get("C0", 1.0)
        for a in range(b):
            assert np.abs(st[a] - st[b]).max() > 0.1 * AMP


@pytest.mark.parametrize("c", GRIDS, ids=GRID_IDS)
def test_energetic_state_convective_floor(c):
    """The floor: in EVERY interior column and EVERY interior row the largest dt |convective term| of the u-equation and of the
    v-equation is at least 10 x the loosest float32 u / v tolerance of the GPU test -- no column or row where a slipped neighbour
    of a convective term would hide under the tolerance because the state starves it."""
    floor = 10.0 * _loosest_uv()
    st, acts = FS.case_inputs(c)
    for b in range(FS.BATCH):
        u, v, dx, dy, dt = _with_ghosts(c, st[b], acts[b])
        for name, cv in zip(("u", "v"), _conv(u, v, c["nx"], c["ny"], dx, dy)):
            a = dt * np.abs(cv)
            assert a.max(axis=1).min() >= floor, (b, name, "column", int(a.max(axis=1).argmin()), float(a.max(axis=1).min()), floor)
            assert a.max(axis=0).min() >= floor, (b, name, "row", int(a.max(axis=0).argmin()), float(a.max(axis=0).min()), floor)


@functools.lru_cache(maxsize=None)
def _oracle_runs(k):
    c = GRIDS[k]
    st, acts = FS.case_inputs(c)
    with ThreadPoolExecutor(max_workers=FS.BATCH) as ex:       # the ctypes calls of the oracle release the GIL
        return list(ex.map(lambda b: MS.run_replica(O.lib(), c, FS.NDT, st[b], acts[b]), range(FS.BATCH)))


@pytest.mark.parametrize("k", range(len(GRIDS)), ids=GRID_IDS)
def test_oracle_stays_energetic_for_the_protocol(k):
    """The float64 oracle takes the protocol's 4 timesteps from every state: every Jacobi solve converges below itmax, the fields
    stay finite, and the flow is still energetic at the end (interior max velocity >= 0.4 amp)."""
    c = GRIDS[k]
    nx, ny = c["nx"], c["ny"]
    for b, (st, obs, rwd, itp) in enumerate(_oracle_runs(k)):
        assert itp.min() >= 1 and itp.max() < 300000, (b, itp)
        assert np.isfinite(st).all() and np.isfinite(obs).all() and np.isfinite(rwd)
        assert max(np.abs(st[0][1:nx + 2, 1:ny + 1]).max(), np.abs(st[1][1:nx + 1, 1:ny + 2]).max()) >= 0.4 * c["amp"], b


def test_sensitivity_catalogue_covers_the_nonlinear_half():
    """The JSON holds every grid of the GPU test and every mutation of oracle/make_sensitivity.py, at least eight, each confined to
    one column or one row and matching the oracle's text exactly once."""
    data = _sens()
    assert sorted(data["effects"]) == sorted(GRID_IDS)
    assert len(MS.MUTATIONS) >= 8 and sorted(data["mutations"]) == sorted(MS.MUTATIONS)
    with open(os.path.join(os.path.dirname(GOLD), os.pardir, "oracle", "beacon_oracle.c")) as fh:
        src = fh.read()
    for name, (what, old, new) in MS.MUTATIONS.items():
        assert src.count(old) == 1, name
        assert (MS.COL in new) != (MS.ROW in new) and name.endswith("_col" if MS.COL in new else "_row"), name
        assert data["mutations"][name] == what
    for g in GRID_IDS:
        assert sorted(data["effects"][g]) == sorted(MS.MUTATIONS), g


def test_sensitivity_json_is_fresh():
    """Two mutations of one grid recomputed -- oracle source copied, mutated, built, both protocols run -- agree with the committed
    JSON within 1 %: a file that no longer describes this oracle, this generator or this catalogue is a red test."""
    c = GRIDS[GRID_IDS.index("rayleigh-50x75")]
    names = ["u_conv_diag_col", "tr_coef_south_row"]
    now = MS.sensitivity([c], names)[FS.grid_id(c)]
    was = _sens()["effects"][FS.grid_id(c)]
    for n in names:
        for p in ("energetic", "quiet"):
            for q in MS.FIELDS:
                a, b = now[n][p][q], was[n][p][q]
                assert abs(a - b) <= 0.01 * max(abs(a), abs(b)), (n, p, q, a, b)


def test_float32_tolerances_stay_under_the_cost_of_a_slip():
    """The cap, from the reference alone: for every float32 case of the GPU test and every catalogued slip, the effect the float64
    oracle measures under the energetic protocol exceeds the case's float32 tolerance at least tenfold in one of u, v, T/C, obs --
    so a kernel with that slip fails the GPU test with a margin of ten.  (The quiet protocol's column of the same file shows which
    slips the tolerances of test_jit_kernels_vs_oracle let through.)"""
    eff = _sens()["effects"]
    bad = []
    for c in FS.CASES:
        if c["dtype"] != "f32":
            continue
        t = FS.F32_ENERGETIC[FS.family(c)]
        for n, e in eff[FS.grid_id(c)].items():
            ratio = max(e["energetic"][q] / t[q] for q in CAP_FIELDS)
            if not ratio >= 10.0:
                bad.append((FS.case_id(c), n, round(ratio, 2)))
    assert not bad, bad


def test_quiet_protocol_misses_slips_the_energetic_one_sees():
    """The gap this file closes, from committed numbers: under the quiet protocol at least one catalogued slip per rayleigh grid
    stays below the float32 u tolerance of test_jit_kernels_vs_oracle (2.7e-6) in u, v, T and obs alike, while under the
    energetic protocol every slip moves one of them by more than 1e-4."""
    eff = _sens()["effects"]
    for g, muts in eff.items():
        assert all(max(e["energetic"][q] for q in CAP_FIELDS) > 1e-4 for e in muts.values()), g
        if g.startswith("rayleigh"):
            assert any(max(e["quiet"][q] for q in CAP_FIELDS) < 2.7e-6 for e in muts.values()), g
