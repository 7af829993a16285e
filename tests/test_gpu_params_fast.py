"""Per-replica physical parameters inside the register-resident 2D kernels (_VecNS2D.set_params_kernel("fast"), bcn_set_option
"params_kernel"): one handle whose replicas carry different ra / (re, pe), stepped by the table-reading instantiations of the
one-row, two-rows and hybrid kernels (csrc/ns2d_prm.h), against (1) separate uniform handles on their PLAIN register-resident
kernels, bit for bit, (2) the float64 oracle of every replica's arguments, (3) the reference's captures of mixing(re, pe); and the
dispatch, graphs and the self-check of a parameter plugin.

The bit-for-bit comparison rests on this: both variants are compiled from the same source expressions with -ffp-contract=on and
without fast-math, and the constants enter as scalars either way.

Nothing here reads the reference tree."""
import os
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLD, golden, ref_to_dev
from oracle import oracle as O

import test_gpu_params as P

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from beacon_amd import _lib
    from beacon_amd import envs as E
    from beacon_amd import vec as V

DEV = P.DEV
B = 7                             # replica b carries set b % 3
# rayleigh: 120 timesteps from the packaged state stay below 410 sweeps; mixing: 32 timesteps with random actions stay finite with
# at most 5 890 sweeps (float64 oracle).  re = 50 is unstable beyond a dozen timesteps and is not used here (only in the four
# captured timesteps of test 3, as in tests/test_gpu_params.py)
PSETS = {"rayleigh": [dict(ra=8.0e3), dict(ra=5.0e4), dict(ra=2.0e5)],
         "mixing": [dict(re=100.0, pe=1.0e4), dict(re=200.0, pe=1.0e5), dict(re=400.0, pe=2.0e3)]}


def _np(t):
    return t.detach().cpu().numpy()


def columns(name, batch=B):
    sets = PSETS[name]
    return {k: np.array([sets[b % 3][k] for b in range(batch)]) for k in sets[0]}


def _seed_state(L, H):
    """[4, nx+2, ny+2] start state of a rayleigh grid without an init file (VecRayleigh.perturbed_conduction_state)"""
    return V.VecRayleigh._derive(V.VecRayleigh.__new__(V.VecRayleigh), L, H).perturbed_conduction_state()


def make(name, dtype, grid, ndt, sched, batch=B, **kw):
    """grid: None (the reference's default: rayleigh 50x50 from the packaged state, mixing 100x100), "bench" (rayleigh 128x64 from
    tests/golden/rayleigh_128x64_init.npz) or (nx, ny) of an on-demand kernel.  set_ndt_act rebuilds the handle: the scheduling
    comes behind it."""
    if name == "rayleigh":
        if grid is None:
            env = V.VecRayleigh(batch, DEV, dtype, E.packaged_init("rayleigh"), **kw)
        elif grid == "bench":
            env = V.VecRayleigh(batch, DEV, dtype, np.load(os.path.join(GOLD, "rayleigh_128x64_init.npz"))["fields"], L=2.56, H=1.28, **kw)
        else:
            L, H = grid[0] / 50.0, grid[1] / 50.0
            env = V.VecRayleigh(batch, DEV, dtype, _seed_state(L, H), L=L, H=H, **kw)
    else:
        geo = {} if grid is None else dict(L=grid[0] / 100.0, H=grid[1] / 100.0)
        env = V.VecMixing(batch, DEV, dtype, **geo, **kw)
    if grid not in (None, "bench"):
        assert (env.nx, env.ny) == tuple(grid)
    env.set_ndt_act(ndt)
    env.set_sched(*sched)
    return env


def mixed_fast(name, dtype, grid, ndt, sched, batch=B):
    env = make(name, dtype, grid, ndt, sched, batch)
    with warnings.catch_warnings():
        warnings.simplefilter("error", V.ParamsWarning)                      # the fast path does not warn
        env.set_params_kernel("fast")
        env.set_params(**columns(name, batch))
    return env


def script(name, env, fast=False):
    """P.script -- reset, three steps across an episode end, step(None), a masked reset of replica 5, one more step -- and a MASKED
    STEP that skips replicas 1, 4, 5.  Returns the records after every call; fast: kernel_name is a register-resident kernel's
    after every step."""
    a, _ = P.inputs(name, env, 6)
    rec = []

    def after():
        rec.append(P.record(env))
        if fast and len(rec) > 1:
            assert env.kernel_name.startswith("ns2d_fast"), (len(rec), env.kernel_name)
    env.reset()
    after()
    env.set_stp(env.n_act - 2)
    for k in range(3):
        env.step(a[k])
        after()
    env.step(None)
    after()
    m = torch.zeros(env.batch, dtype=torch.uint8, device=DEV)
    m[5] = 1
    env.reset(mask=m)
    rec.append(P.record(env))
    env.step(a[4])
    after()
    m = torch.ones(env.batch, dtype=torch.uint8, device=DEV)
    m[[1, 4, 5]] = 0
    env.step(a[5], mask=m)
    after()
    torch.cuda.synchronize()
    assert int(env.status.abs().max()) == 0
    for x, y in zip(rec[-2], rec[-1]):                                        # skipped replicas keep every byte
        assert torch.equal(x[[1, 4, 5]], y[[1, 4, 5]])
    assert not torch.equal(rec[-2][4][0], rec[-1][4][0])
    return rec


# ---- 1. a mixed batch on the parameter kernels is K uniform handles on the plain kernels, bit for bit ------------------------------
S0, S2, LPT = (0,), (2, 2, 2), (1, 0, 0, 1)
CASES = [
    # rayleigh 50x50: plain launch; two persistent workgroups with chunks of two timesteps -- every workgroup carries several
    # replicas with different constants one after another, every replica changes workgroup between chunks
    ("rayleigh", "f32", None, 6, S0, "ns2d_fast_step"), ("rayleigh", "f32", None, 6, S2, "ns2d_fast_sched"),
    ("rayleigh", "f64", None, 6, S0, "ns2d_fast_step"), ("rayleigh", "f64", None, 6, S2, "ns2d_fast_sched"),
    # the two-launch LPT split: replicas reordered through A.order in the second launch
    ("rayleigh", "f32", None, 40, LPT, "ns2d_fast_step"),
    # 128x64: the bench kernel; float64 with fields in the global scratch and dead columns
    ("rayleigh", "f32", "bench", 6, S2, "ns2d_fast_sched"), ("rayleigh", "f64", "bench", 6, S2, "ns2d_fast_sched"),
    # mixing 100x100: float32 with parallel transport passes (the three sets have different rho), float64 ordered
    ("mixing", "f32", None, 4, S0, "ns2d_fast2_step"), ("mixing", "f32", None, 4, S2, "ns2d_fast2_sched"),
    ("mixing", "f64", None, 4, S0, "ns2d_fast2_step"), ("mixing", "f64", None, 4, S2, "ns2d_fast2_sched"),
    # one on-demand kernel per family (jit.PRM_TEST_GRIDS): rows 1; rows 2 float64, global scratch (the grid of the round-5 bug);
    # rows 2 mixing; rows 4
    ("rayleigh", "f32", (75, 50), 4, S2, "ns2d_fast_sched"), ("rayleigh", "f64", (50, 75), 4, S2, "ns2d_fast2_sched"),
    ("mixing", "f32", (100, 110), 4, S2, "ns2d_fast2_sched"), ("rayleigh", "f32", (50, 150), 4, S2, "ns2d_fast4_sched"),
]


@pytest.mark.parametrize("name,dtype,grid,ndt,sched,kernel", CASES,
                         ids=["%s-%s-%s-ndt%d-sched%s" % (c[0], c[1], "x".join(map(str, c[2])) if isinstance(c[2], tuple) else c[2], c[3],
                                                          "_".join(map(str, c[4]))) for c in CASES])
def test_mixed_batch_on_the_parameter_kernels_equals_uniform_handles_on_the_plain_kernels(name, dtype, grid, ndt, sched, kernel):
    """One handle of 7 replicas holding 3 parameter sets interleaved, stepped by the table-reading register-resident kernel,
    against 3 handles constructed with those values on the plain register-resident kernel under the same set_sched: obs, rwd,
    done, trunc, get_state() and the sweep counts after every call of script() are torch.equal.  No tolerance."""
    from beacon_amd import jit
    if isinstance(grid, tuple):
        assert grid + (dtype == "f64", 0 if name == "rayleigh" else 1) in jit.PRM_TEST_GRIDS
    env = mixed_fast(name, dtype, grid, ndt, sched)
    got = script(name, env, fast=True)
    assert env.kernel_name == kernel
    env.close()
    done_seen = False
    for k, kw in enumerate(PSETS[name]):
        uni = make(name, dtype, grid, ndt, sched, **kw)
        want = script(name, uni)
        assert uni.kernel_name == kernel                                      # the plain kernel of the same family, same dispatch
        uni.close()
        rows = torch.arange(k, B, 3, device=DEV)
        for call, (g, w) in enumerate(zip(got, want)):
            for what, (x, y) in enumerate(zip(g, w)):
                assert torch.equal(x[rows], y[rows]), (name, dtype, grid, "set %d" % k, "call %d" % call, "output %d" % what)
        done_seen = done_seen or bool(want[2][2].any())
    assert done_seen
    assert not torch.equal(got[-1][4][0], got[-1][4][1])                      # replicas of different sets do differ


# ---- 2. float64 against the oracle of each replica's arguments --------------------------------------------------------------------
@pytest.mark.parametrize("name,ndt", [("rayleigh", 6), ("mixing", 4)])
def test_float64_parameter_kernels_match_the_oracle_of_each_replicas_arguments(name, ndt):
    """float64, four action steps from reset through the table-reading kernels (rayleigh 50x50, mixing 100x100): fields and
    observations within 1e-9 (p 50 x, rewards 1e-8) with sweep counts EQUAL to the oracle's -- the bar of
    test_every_replica_of_a_mixed_batch_matches_the_float64_oracle_of_its_arguments.  Replicas of one parameter set receive the same
    actions, so one oracle per set serves them all."""
    n = 4
    env = mixed_fast(name, "f64", None, ndt, S0)
    a, _ = P.inputs(name, env, n, seed=17)
    a = a[:, torch.arange(B, device=DEV) % 3]
    env.reset()
    oracles = []
    for kw in PSETS[name]:
        o = O.rayleigh(init_fields=E.packaged_init("rayleigh"), **kw) if name == "rayleigh" else O.mixing(**kw)
        o.cfg.ndt_act = ndt
        o.reset()
        oracles.append(o)
    worst = {}

    def close(what, dev, ref, tol):
        d = float(np.max(np.abs(np.asarray(dev, dtype=np.float64) - np.asarray(ref, dtype=np.float64))))
        worst[what] = max(worst.get(what, 0.0), d)
        return d <= tol

    for k in range(n):
        obs, rwd, done, trunc, _ = env.step(a[k])
        torch.cuda.synchronize()
        assert int(env.status.abs().max()) == 0 and env.kernel_name.startswith("ns2d_fast")
        o_d, r_d, st, sw = _np(obs), _np(rwd), _np(env.get_state()), _np(env.sweeps)
        for s, o in enumerate(oracles):
            ob, rw, dn, tr, _ = P._oracle_step(name, o, _np(a[k, s]), None)
            for b in range(s, B, 3):
                assert bool(done[b]) == bool(dn) and bool(trunc[b]) == bool(tr)
                ref = np.swapaxes(st[b], -1, -2)
                assert close("obs", o_d[b], ob, P.F64_TOL) and close("rwd", r_d[b], rw, 1e-8), (k, b, worst)
                for i, f in enumerate("uvpS"):
                    assert close(f, ref[i], o.st[i], P.F64_TOL * (50 if f == "p" else 1)), (k, b, f, worst)
                assert np.array_equal(sw[b], o.itp), (k, b, sw[b], o.itp)
    print("MEASURED %s max |device - oracle| %s" % (name, worst))
    env.close()


# ---- 3. against the reference's captures --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [0, 1, 2])
def test_mixing_parameter_kernel_vs_the_reference_captures(geom):
    """test_mixing_batch_with_per_replica_re_pe_vs_the_reference_captures on the table-reading two-rows-per-lane kernel, at that
    test's tolerances (float64: 1e-9, p 50 x, counts within 1)."""
    g = golden("ctor_args")
    env = V.VecMixing(3, DEV, "f64", **P.MIX_GEOM[geom])
    env.set_ndt_act(4)
    with warnings.catch_warnings():
        warnings.simplefilter("error", V.ParamsWarning)
        env.set_params_kernel("fast")
        env.set_params(re=[50.0, 200.0, 400.0], pe=[1.0e3, 1.0e5, 2.0e3])
    env.reset()
    st0 = np.stack([np.stack([ref_to_dev(g["%s_%s0" % (t0, f)]) for f in "uvpC"]) for _, t0, _ in P.MIX_TAGS])
    env.set_state(st0)
    obs, rwd, _, _, _ = env.step(np.array([act for _, _, act in P.MIX_TAGS]))
    env.check_status()
    assert env.kernel_name.startswith("ns2d_fast2")
    st, sw = np.swapaxes(_np(env.get_state()), -1, -2), _np(env.sweeps)
    n = 3 * env.nx_obs_pts * env.ny_obs_pts
    for b, (tag, _, _) in enumerate(P.MIX_TAGS):
        for i, f in enumerate("uvpC"):
            d = float(np.abs(st[b][i] - g["%s_%s" % (tag, f)]).max())
            assert d <= P.F64_TOL * (50 if f == "p" else 1), (tag, f, d)
        assert float(np.abs(_np(obs)[b][-n:] - g[tag + "_obs"][-n:]).max()) <= P.F64_TOL, tag
        assert np.all(np.abs(sw[b] - g[tag + "_itp"]) <= 1), (tag, sw[b], g[tag + "_itp"])
    tag = P.MIX_TAGS[geom][0]
    assert abs(float(rwd[geom]) - float(g[tag + "_rwd"])) <= P.F64_TOL, tag
    env.close()


# ---- 4. dispatch and surface ----------------------------------------------------------------------------------------------------
def test_dispatch_follows_the_option_the_table_and_the_variant():
    name = "rayleigh"
    env = make(name, "f32", None, 6, S0)
    a, _ = P.inputs(name, env, 2)

    def stepped():
        env.reset()
        env.step(a[0])
        torch.cuda.synchronize()
        return env.kernel_name

    # off by default: a table selects the generic kernel and warns
    with pytest.warns(V.ParamsWarning):
        env.set_params(**columns(name))
    assert stepped() == "ns2d_generic_step"
    env.clear_params()
    with warnings.catch_warnings():
        warnings.simplefilter("error", V.ParamsWarning)
        assert env.set_params_kernel("fast") is env
        assert stepped() == "ns2d_fast_step"                                  # no table: no effect
        env.set_params(**columns(name))                                       # no ParamsWarning
        assert env.kernel_name == "ns2d_fast_step" and stepped() == "ns2d_fast_step"
        env.set_ndt_act(4)                                                    # a new handle: table and choice come along
        assert all(np.array_equal(env.params[k], v) for k, v in columns(name).items())
        assert stepped() == "ns2d_fast_step"
        st_fast = env.get_state().clone()
        env.clear_params()
        assert stepped() == "ns2d_fast_step"                                  # the plain kernel
        assert not torch.equal(env.get_state(), st_fast)
        env.set_params(**columns(name))
        env.set_params_kernel("generic")
        assert env.kernel_name == "ns2d_generic_step" and stepped() == "ns2d_generic_step"
        env.set_params_kernel("fast")
        assert stepped() == "ns2d_fast_step"
        assert env.set_variant(0) == 0                                        # variant 0 keeps meaning the generic kernel
        assert env.kernel_name == "ns2d_generic_step" and stepped() == "ns2d_generic_step"
    with pytest.raises(ValueError):
        env.set_params_kernel("quick")
    env.close()
    one_d = V.VecBurgers(2, DEV, "f32")
    with pytest.raises(_lib.BeaconHipError, match="unknown option 'params_kernel'"):
        one_d.set_option("params_kernel", 1)
    assert not hasattr(one_d, "set_params_kernel")
    one_d.close()


@pytest.mark.parametrize("name,dtype,ndt", [("rayleigh", "f32", 6), ("rayleigh", "f64", 6), ("mixing", "f32", 4), ("mixing", "f64", 4)])
def test_constructor_values_on_the_parameter_kernel_change_nothing(name, dtype, ndt):
    """A table equal to the constructor's values, read by the parameter kernel, against the same env without a table on the plain
    kernel (ticket scheduler): torch.equal."""
    plain = make(name, dtype, None, ndt, S2)
    want = script(name, plain)
    ctor = {k: float(v[0]) for k, v in plain.params.items()}
    plain.close()
    same = make(name, dtype, None, ndt, S2)
    same.set_params_kernel("fast").set_params(**ctor)
    got = script(name, same, fast=True)
    same.close()
    for call, (g, w) in enumerate(zip(got, want)):
        for what, (x, y) in enumerate(zip(g, w)):
            assert torch.equal(x, y), (name, dtype, call, what)


# ---- 5. graphs ------------------------------------------------------------------------------------------------------------------
def test_graph_captured_with_the_parameter_kernel_replays_a_table_rewritten_in_place():
    """rayleigh 50x50 float32, captured after set_params with the fast kernel selected: every replay reads the table in force
    then, and equals eager steps of an env with that table (the pattern of
    test_graph_captured_after_set_params_replays_a_table_rewritten_in_place)."""
    name, n, nb = "rayleigh", 3, 5
    env = make(name, "f32", None, 6, S0, nb).set_params_kernel("fast")
    tables = [columns(name, nb), {k: np.roll(v, 1) for k, v in columns(name, nb).items()}]
    a, _ = P.inputs(name, env, n, seed=23)
    env.set_params(**tables[0])
    env.reset()
    g = env.capture(a, None, n_steps=n)
    for rep, tab in enumerate(tables):
        env.set_params(**tab)                                                 # in place, before the replay
        env.reset()
        obs_seq, rwd_seq, done_seq, _ = g.replay()
        torch.cuda.synchronize()
        assert env.kernel_name == "ns2d_fast_step"
        eager = make(name, "f32", None, 6, S0, nb).set_params_kernel("fast")
        eager.set_params(**tab)
        eager.reset()
        for k in range(n):
            obs, rwd, done, _, _ = eager.step(a[k])
            assert torch.equal(obs_seq[k], obs) and torch.equal(rwd_seq[k], rwd) and torch.equal(done_seq[k], done), (rep, k)
        assert torch.equal(env.get_state(), eager.get_state())
        eager.close()
    assert not torch.equal(obs_seq[n - 1][0], obs_seq[n - 1][1])
    env.close()


# ---- 6. the self-check of a parameter plugin ------------------------------------------------------------------------------------------
def test_self_check_refuses_a_broken_parameter_plugin_and_keeps_the_generic_kernel():
    """A deliberately wrong parameter plugin (csrc/jit/ns2d_jit.hip with -DBCN_JIT_PRM=1 -DBCN_JIT_BREAK=1: 1.5 dt) next to the sound
    plain plugin of its grid: set_params_kernel("fast") compares it with the generic kernel under a per-replica table, warns, leaves
    its own `.bad` marker and does not attach it; with a table the env steps through the generic kernel, with that kernel's
    results; without one the sound plain plugin keeps running.  (The break is a flag of the parameter plugin alone,
    _plugin_prm_defs: with _plugin_defs the plain plugin would be refused first and the parameter plugin never asked for.)"""
    from beacon_amd import jit

    class Broken(V.VecRayleigh):
        _plugin_prm_defs = {"BCN_JIT_BREAK": 1}
    nx, ny, f64, kind = jit.PRM_BREAK_GRID
    defs = dict(jit.PRM_DEFS, **Broken._plugin_prm_defs)
    path = jit.build_plugin(nx, ny, f64, kind, extra_defs=defs)
    assert path is not None, "the broken parameter plugin was not built (run __graft_entry__.build())"
    key = (nx, ny, f64, kind, tuple(sorted(defs.items())))

    def clean():
        for mark in (".ok", ".bad"):
            if os.path.exists(path + mark):
                os.remove(path + mark)
        jit._LOADED.pop(key, None)
    clean()
    try:
        env = Broken(3, DEV, "f64", None, L=nx / 50.0, H=ny / 50.0)
        assert env._plugin.verified is True                                   # the plain plugin is sound
        with pytest.warns(jit.JitWarning, match="DISAGREES with the generic kernel"):
            env.set_params_kernel("fast")
        assert getattr(env, "_plugin_prm", None) is None and os.path.exists(path + ".bad")
        ref = V.VecRayleigh(3, DEV, "f64", None, L=nx / 50.0, H=ny / 50.0)
        a = np.random.default_rng(1).uniform(-1, 1, (3, 10))
        for e in (env, ref):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", V.ParamsWarning)
                e.set_ndt_act(4)                                               # (a new handle: the refused plugin stays refused)
                if e is ref:
                    assert e.set_variant(0) == 0
                e.set_params(ra=[8.0e3, 5.0e4, 2.0e5])
            e.reset()
            e.set_state(jit._seeded_rayleigh_state(e))
            e.step(a)
            e.check_status()
        assert env.kernel_name == "ns2d_generic_step"
        assert torch.equal(env.get_state(), ref.get_state()) and torch.equal(env.sweeps, ref.sweeps)
        env.clear_params()
        env.step(a)
        assert env.kernel_name.startswith("ns2d_fast")                        # the plain plugin, untouched
        env.close()
        ref.close()
    finally:
        clean()
