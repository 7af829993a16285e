"""Per-replica physical parameters on the GPU (VecEnv.set_params / bcn_set_params): one handle whose replicas carry different
constructor arguments of the reference, against (1) separate uniform handles constructed with those arguments, bit for bit,
(2) the float64 oracle / host port of every replica's arguments, at the tolerances of the existing float64 tests, (3) the
reference's own captures of mixing(re, pe) (tests/golden/ctor_args.npz); and the rest of the surface: inert when unused, graphs,
snapshots, invalid input, the 2D kernel dispatch.

Nothing here reads /root/reference."""
import warnings

import numpy as np
import pytest
import torch

from conftest import golden, ref_to_dev
from oracle import oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import beacon_amd
    from beacon_amd import _lib
    from beacon_amd import envs as E
    from beacon_amd import vec as V

DEV = "cuda:0"
F64_TOL = 1e-9                    # tests/test_gpu_parity.py: float64 2D kernels against the float64 oracle (p: 50 x)
TOL_1D = 1e-12                    # tests/test_gpu_parity.py: float64 1D kernels (burgers / sloshing goldens, shkadov_tol("f64"))
VORTEX_OBS, VORTEX_RWD = 6.9e-17, 3.4e-17     # tests/test_gpu_ode.py: TOL["vortex_f64_obs"], TOL["vortex_f64_rwd"] (absolute)
# Timesteps per action step of the 2D envs here (set_ndt_act).  mixing: ONE, so that the seven calls of script() stay within the
# horizon on which mixing(re = 50) was verified (the four timesteps of the captures in tests/golden/ctor_args.npz): at dt = 0.002 and
# dx = 0.01 the explicit momentum diffusion has 4 dt / (re dx^2) = 1.6 > 1 there, and the reference's own arithmetic -- the float64
# oracle, which the kernel still follows sweep for sweep -- leaves the stable regime after a dozen timesteps and stops converging
# after twenty (measured: 60 860 sweeps in timestep 18, ITMAX in timestep 19).  set_params checks signs, not stability, as the
# constructors do.
NDT_2D = {"rayleigh": 6, "mixing": 1}

# K = 3 parameter sets per env, inside the ranges the float64 oracle was run on (6 action steps, no blow-up, no ITMAX)
PSETS = {
    "lorenz": [dict(sigma=8.0, rho=20.0, beta=2.0), dict(sigma=10.0, rho=28.0, beta=8.0 / 3.0), dict(sigma=12.0, rho=35.0, beta=3.0)],
    "vortex": [dict(re=50.0, weight=50.0), dict(re=60.0, weight=10.0), dict(re=47.5, weight=100.0)],
    "burgers": [dict(u_target=0.3, amp=5.0), dict(u_target=0.5, amp=10.0), dict(u_target=0.7, amp=15.0)],
    "shkadov": [dict(delta=0.05), dict(delta=0.1), dict(delta=0.2)],
    "sloshing": [dict(g=5.0, alpha=5e-4, amp=5.0), dict(g=9.81, alpha=1e-3, amp=2.5), dict(g=15.0, alpha=2e-4, amp=8.0)],
    "rayleigh": [dict(ra=8.0e3), dict(ra=5.0e4), dict(ra=2.0e5)],
    "mixing": [dict(re=50.0, pe=1.0e3), dict(re=200.0, pe=1.0e5), dict(re=400.0, pe=2.0e3)],
}
NAMES = list(PSETS)
B = 7                             # replica b carries set b % 3


def _np(t):
    return t.detach().cpu().numpy()


def _init(name):
    return E.packaged_init(name) if name in ("shkadov", "sloshing", "rayleigh") else None


def make(name, dtype, batch=B, **kw):
    """an env of the existing style: every replica with the constructor arguments kw (none: the defaults)"""
    if name == "lorenz":
        return V.VecLorenz(batch, DEV, dtype, **kw)
    if name == "vortex":
        return V.VecVortex(batch, DEV, dtype, **kw)
    if name == "burgers":
        return V.VecBurgers(batch, DEV, dtype, **kw)
    if name == "shkadov":
        return V.VecShkadov(batch, DEV, dtype, _init(name), **kw)
    if name == "sloshing":
        return V.VecSloshing(batch, DEV, dtype, _init(name), **kw)
    env = V.VecRayleigh(batch, DEV, dtype, _init(name), **kw) if name == "rayleigh" else V.VecMixing(batch, DEV, dtype, **kw)
    env.set_ndt_act(NDT_2D[name])
    return env


def columns(name, batch=B):
    """{parameter: float64 [batch]} with replica b carrying PSETS[name][b % 3]"""
    sets = PSETS[name]
    return {k: np.array([sets[b % len(sets)][k] for b in range(batch)]) for k in sets[0]}


def mixed(name, dtype, batch=B):
    env = make(name, dtype, batch)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", V.ParamsWarning)
        env.set_params(**columns(name, batch))
    return env


def inputs(name, env, n, seed=5):
    """n action steps' worth of actions [n, B, ...] and explicit noise (None for envs without) for env's batch"""
    rng = np.random.default_rng(seed)
    nb = env.batch
    noise = None
    if name == "lorenz":
        a = torch.as_tensor(rng.integers(0, 3, (n, nb)), dtype=torch.int32, device=DEV)
    elif name == "mixing":
        a = torch.as_tensor(rng.integers(0, 4, (n, nb)), dtype=torch.int32, device=DEV)
    elif name == "vortex":
        a = torch.as_tensor(rng.uniform(-1, 1, (n, nb, 2)), dtype=env.tdtype, device=DEV)
    elif name == "rayleigh":
        a = torch.as_tensor(rng.uniform(-1, 1, (n, nb, env.n_sgts)), dtype=env.tdtype, device=DEV)
    elif name == "shkadov":
        a = torch.as_tensor(rng.uniform(-1, 1, (n, nb, env.n_jets)), dtype=env.tdtype, device=DEV)
        noise = torch.as_tensor(rng.uniform(-5e-4, 5e-4, (n, nb, env.ndt_act)), dtype=env.tdtype, device=DEV)
    else:
        a = torch.as_tensor(rng.uniform(-1, 1, (n, nb)), dtype=env.tdtype, device=DEV)
        if name == "burgers":
            noise = torch.as_tensor(rng.uniform(-0.1, 0.1, (n, nb)), dtype=env.tdtype, device=DEV)
    return a, noise


def record(env):
    """everything a step leaves behind, cloned: obs, rwd, done, trunc, the state and (2D) the sweep counts"""
    out = [env.obs.clone(), env.rwd.clone(), env.done.clone(), env.trunc.clone(), env.get_state().clone()]
    if hasattr(env, "sweeps"):
        out.append(env.sweeps.clone())
    return out


def script(name, env):
    """The same sequence of calls on any env: reset, three steps across the end of an episode, a step that repeats the stored
    action (step(None); the envs with inlet noise still get their explicit noise), a masked reset of replica 5 -- burgers: it
    refills that replica with its own u_target -- and one more step.  Returns the records after every call."""
    a, z = inputs(name, env, 5)
    zk = (lambda k: None) if z is None else (lambda k: z[k])
    rec = []
    env.reset()
    rec.append(record(env))
    env.set_stp(env.n_act - 2)                   # done / trunc rise at the second step
    for k in range(3):
        env.step(a[k], zk(k))
        rec.append(record(env))
    env.step(None, zk(3))
    rec.append(record(env))
    m = torch.zeros(env.batch, dtype=torch.uint8, device=DEV)
    m[5] = 1
    env.reset(mask=m)
    rec.append(record(env))
    env.step(a[4], zk(4))
    rec.append(record(env))
    torch.cuda.synchronize()
    assert int(env.status.abs().max()) == 0
    return rec


# ---- 1. a mixed batch is K separate uniform handles, bit for bit ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("name", NAMES)
def test_mixed_batch_equals_separate_uniform_handles_bit_for_bit(name, dtype):
    """One handle of 7 replicas holding 3 parameter sets interleaved against 3 handles constructed with those values (2D: the
    generic kernel, set_variant(0)), same actions and explicit noise: observations, rewards, done / trunc, get_state() and (2D)
    the sweep counts of every replica after reset, after every step, after step(None) and after a masked reset are torch.equal --
    the same kernel reads the same scalars.  No tolerance."""
    env = mixed(name, dtype)
    assert env.params.keys() == set(env.PARAMS) and all(np.array_equal(env.params[k], v) for k, v in columns(name).items())
    got = script(name, env)
    if name in ("rayleigh", "mixing"):
        assert env.kernel_name == "ns2d_generic_step"
    env.close()
    done_seen = False
    for k, kw in enumerate(PSETS[name]):
        uni = make(name, dtype, **kw)
        if name in ("rayleigh", "mixing"):
            assert uni.set_variant(0) == 0
        want = script(name, uni)
        uni.close()
        rows = torch.arange(k, B, len(PSETS[name]), device=DEV)
        for call, (g, w) in enumerate(zip(got, want)):
            for what, (x, y) in enumerate(zip(g, w)):
                assert torch.equal(x[rows], y[rows]), (name, dtype, "set %d" % k, "call %d" % call, "output %d" % what)
        done_seen = done_seen or bool(want[2][2].any())
    assert done_seen                                                    # the done / trunc comparison saw an episode end
    if name == "burgers":                                               # the masked reset refilled replica 5 with ITS u_target
        u = _np(got[5][4])[5, 0]
        assert np.all(u == np.asarray(PSETS[name][5 % 3]["u_target"], dtype=u.dtype)) and PSETS[name][5 % 3]["u_target"] != 0.5


# ---- 2. every replica against the reference's arithmetic in float64 ------------------------------------------------------------------
def _oracle(name, kw):
    if name == "lorenz":
        return O.lorenz(**kw), beacon_amd.lorenz(**kw)
    if name == "vortex":
        return beacon_amd.vortex(**kw), None
    if name == "burgers":
        return O.burgers(**kw), None
    if name == "shkadov":
        o = O.shkadov(init_fields=_init(name), **kw)
        o.rand_init = False
        return o, None
    if name == "sloshing":
        return O.sloshing(init_fields=_init(name), **kw), None
    o = O.rayleigh(init_fields=_init(name), **kw) if name == "rayleigh" else O.mixing(**kw)
    o.cfg.ndt_act = NDT_2D[name]
    return o, None


def _oracle_step(name, o, a, z):
    if name in ("lorenz", "mixing"):
        return o.step(int(a))
    if name == "vortex":
        return o.step(np.asarray(a, dtype=np.float64))
    if name == "burgers":
        return o.step([float(a)], float(z))
    if name == "shkadov":
        return o.step([float(x) for x in a], np.asarray(z, dtype=np.float64))
    if name == "sloshing":
        return o.step([float(a)])
    return o.step([float(x) for x in a])


@pytest.mark.parametrize("name", NAMES)
def test_every_replica_of_a_mixed_batch_matches_the_float64_oracle_of_its_arguments(name):
    """float64, four action steps from reset.  Each replica against oracle.<env>(its arguments) -- vortex: the host port
    beacon_amd.vortex(re, weight); lorenz: the oracle AND the host port beacon_amd.lorenz -- at the tolerance of that env's
    existing float64 test: lorenz bit for bit, vortex 6.9e-17 / 3.4e-17 (obs / rwd, absolute), the 1D envs 1e-12, the 2D envs 1e-9
    (rewards 1e-8 as in test_rayleigh_batch_vs_oracle_f64) with sweep counts EQUAL to the oracle's."""
    n = 4
    env = mixed(name, "f64")
    a, z = inputs(name, env, n, seed=17)
    env.reset()
    oracles = [_oracle(name, PSETS[name][b % 3]) for b in range(B)]
    for o, o2 in oracles:
        o.reset()
        if o2 is not None:
            o2.reset()
    worst = {}

    def close(what, dev, ref, tol):
        d = float(np.max(np.abs(np.asarray(dev, dtype=np.float64) - np.asarray(ref, dtype=np.float64))))
        worst[what] = max(worst.get(what, 0.0), d)
        return d <= tol

    for k in range(n):
        obs, rwd, done, trunc, _ = env.step(a[k], None if z is None else z[k])
        torch.cuda.synchronize()
        assert int(env.status.abs().max()) == 0
        o_d, r_d, st = _np(obs), _np(rwd), _np(env.get_state())
        sw = _np(env.sweeps) if hasattr(env, "sweeps") else None
        for b, (o, o2) in enumerate(oracles):
            ob, rw, dn, tr, _ = _oracle_step(name, o, _np(a[k, b]), None if z is None else _np(z[k, b]))
            assert bool(done[b]) == bool(dn) and bool(trunc[b]) == bool(tr)
            if name == "lorenz":
                ob2, rw2, _, _, _ = o2.step(np.int64(_np(a[k, b])))
                assert np.array_equal(o_d[b], ob) and r_d[b] == rw, (k, b)
                assert np.array_equal(o_d[b], ob2) and r_d[b] == rw2, (k, b)
                assert np.array_equal(st[b, :3], o.x)
            elif name == "vortex":
                assert close("obs", o_d[b], ob, VORTEX_OBS) and close("rwd", r_d[b], rw, VORTEX_RWD), (k, b, worst)
            elif name in ("burgers", "shkadov", "sloshing"):
                assert close("obs", o_d[b], ob, TOL_1D) and close("rwd", r_d[b], rw, TOL_1D), (k, b, worst)
                if name == "burgers":
                    assert close("u", st[b, 0], o.u, TOL_1D), (k, b, worst)
                else:
                    assert close("h", st[b, 0], o.h, TOL_1D) and close("q", st[b, 1], o.q, TOL_1D), (k, b, worst)
            else:
                ref = np.swapaxes(st[b], -1, -2)                       # [4, nx+2, ny+2], the oracle's layout
                print("MEASURED %s step %d replica %d sweeps: device %s oracle %s" % (name, k, b, sw[b].tolist(), o.itp.tolist()))
                assert close("obs", o_d[b], ob, F64_TOL) and close("rwd", r_d[b], rw, 1e-8), (k, b, worst)
                for i, f in enumerate("uvpS"):
                    assert close(f, ref[i], o.st[i], F64_TOL * (50 if f == "p" else 1)), (k, b, f, worst)
                assert np.array_equal(sw[b], o.itp), (k, b, sw[b], o.itp)
    print("MEASURED %s max |device - oracle| %s" % (name, worst))
    env.close()


# ---- 3. against the reference itself: the captures of mixing(re, pe) ----------------------------------------------------------------
MIX_TAGS = [("mix_re50_pe1e3_a0", "mix_re50_pe1e3_a0", 0), ("mix_re200_pe1e5_a1", "mix_re200_pe1e5_a1", 1),
            ("mix_re400_pe2e3_a0", "mix_re400_pe2e3_a0", 0)]
MIX_GEOM = [dict(), dict(side=0.3, C0=2.0), dict(side=0.62, C0=0.5)]   # the structural arguments of each capture (patch, reward level)


@pytest.mark.parametrize("geom", [0, 1, 2])
def test_mixing_batch_with_per_replica_re_pe_vs_the_reference_captures(geom):
    """One VecMixing float64 batch whose replicas carry (re, pe) = (50, 1e3), (200, 1e5), (400, 2e3), every replica started from
    the seeded state of ITS capture in tests/golden/ctor_args.npz and stepped with that capture's action: fields, observation
    and sweep counts (itp) of all three replicas against what the REFERENCE returned, at the tolerance of
    test_mixing_constructor_arguments_vs_reference (float64: 1e-9, p 50 x, counts within 1).  The reward measures the distance
    from a level set by side and C0, which are structural (per handle, not per replica): it is compared for the replica whose
    capture was taken with this batch's side / C0, and the three batches of this test cover every capture's reward."""
    g = golden("ctor_args")
    env = V.VecMixing(3, DEV, "f64", **MIX_GEOM[geom])
    env.set_ndt_act(4)
    with pytest.warns(V.ParamsWarning):
        env.set_params(re=[50.0, 200.0, 400.0], pe=[1.0e3, 1.0e5, 2.0e3])
    env.reset()
    st0 = np.stack([np.stack([ref_to_dev(g["%s_%s0" % (t0, f)]) for f in "uvpC"]) for _, t0, _ in MIX_TAGS])
    env.set_state(st0)
    obs, rwd, _, _, _ = env.step(np.array([act for _, _, act in MIX_TAGS]))
    env.check_status()
    assert env.kernel_name == "ns2d_generic_step"
    st, sw = np.swapaxes(_np(env.get_state()), -1, -2), _np(env.sweeps)
    n = 3 * env.nx_obs_pts * env.ny_obs_pts
    for b, (tag, _, _) in enumerate(MIX_TAGS):
        for i, f in enumerate("uvpC"):
            d = float(np.abs(st[b][i] - g["%s_%s" % (tag, f)]).max())
            assert d <= F64_TOL * (50 if f == "p" else 1), (tag, f, d)
        assert float(np.abs(_np(obs)[b][-n:] - g[tag + "_obs"][-n:]).max()) <= F64_TOL, tag
        assert np.all(np.abs(sw[b] - g[tag + "_itp"]) <= 1), (tag, sw[b], g[tag + "_itp"])
    tag = MIX_TAGS[geom][0]
    assert abs(float(rwd[geom]) - float(g[tag + "_rwd"])) <= F64_TOL, tag
    env.close()


# ---- 4. inert when unused ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("name", NAMES)
def test_constructor_values_and_cleared_tables_change_nothing(name, dtype):
    """set_params() with the constructor's own values, and clear_params() after a different table, both give what a handle that
    never called either gives, bit for bit (2D: all three on the generic kernel -- a table selects it; after clear_params() the
    kernel the env had before runs again, compared below with its own untouched twin)."""
    two_d = name in ("rayleigh", "mixing")
    plain = make(name, dtype)
    if two_d:
        plain.set_variant(0)
    want = script(name, plain)
    ctor = {k: v.copy() for k, v in plain.params.items()}
    plain.close()
    same = make(name, dtype)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", V.ParamsWarning)
        same.set_params(**{k: float(v[0]) for k, v in ctor.items()})          # scalars broadcast
    got = script(name, same)
    same.close()
    for call, (g, w) in enumerate(zip(got, want)):
        for what, (x, y) in enumerate(zip(g, w)):
            assert torch.equal(x, y), (name, dtype, "ctor values", call, what)
    cleared = make(name, dtype)
    default_kernel = cleared.kernel_name
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", V.ParamsWarning)
        cleared.set_params(**columns(name))
    cleared.reset()
    a, z = inputs(name, cleared, 1)
    cleared.step(a[0], None if z is None else z[0])                           # one step on the other table
    cleared.clear_params()
    cleared.out_buf.zero_()                                                   # (reset() writes no reward and no sweep counts:
    if two_d:                                                                 #  the untouched twin's are still 0)
        cleared.sweeps.zero_()
    assert all(np.array_equal(cleared.params[k], ctor[k]) for k in ctor)
    if two_d:
        assert cleared.kernel_name == default_kernel
        cleared.set_variant(0)
    got = script(name, cleared)
    cleared.close()
    for call, (g, w) in enumerate(zip(got, want)):
        for what, (x, y) in enumerate(zip(g, w)):
            assert torch.equal(x, y), (name, dtype, "cleared", call, what)


# ---- 5. the rest of the surface ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lorenz", "burgers", "rayleigh"])
def test_graph_captured_after_set_params_replays_a_table_rewritten_in_place(name):
    """The device table keeps its address: a graph captured after the first set_params reads, at every replay, the table in
    force then -- here rewritten between two replays -- and equals eager steps of an env with that table."""
    n, nb = 3, 5
    env = make(name, "f32", nb)
    tables = [columns(name, nb), {k: np.roll(v, 1) for k, v in columns(name, nb).items()}]
    a, z = inputs(name, env, n, seed=23)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", V.ParamsWarning)
        env.set_params(**tables[0])
        env.reset()
        g = env.capture(a, z, n_steps=n)
        for rep, tab in enumerate(tables):
            env.set_params(**tab)                                             # in place, before the replay
            env.reset()
            obs_seq, rwd_seq, done_seq, _ = g.replay()
            torch.cuda.synchronize()
            eager = make(name, "f32", nb)
            eager.set_params(**tab)
            eager.reset()
            for k in range(n):
                obs, rwd, done, _, _ = eager.step(a[k], None if z is None else z[k])
                assert torch.equal(obs_seq[k], obs) and torch.equal(rwd_seq[k], rwd) and torch.equal(done_seq[k], done), (name, rep, k)
            assert torch.equal(env.get_state(), eager.get_state())
            eager.close()
    assert not torch.equal(obs_seq[n - 1][0], obs_seq[n - 1][1])               # the replicas do differ
    env.close()


@pytest.mark.parametrize("name", ["sloshing", "lorenz"])
def test_restore_and_fork_move_state_and_leave_every_replicas_physics(name):
    env = mixed(name, "f64", 6)
    twin = make(name, "f64", 6)
    assert env.snapshot_signature() == twin.snapshot_signature()              # parameters are not in the signature
    a, z = inputs(name, env, 3, seed=3)
    env.reset()
    env.step(a[0])
    before, params = env.get_state().clone(), {k: v.copy() for k, v in env.params.items()}
    snap = env.snapshot()
    assert "params" not in snap.names() and snap.signature == twin.snapshot_signature()
    perm = np.array([3, 0, 4, 1, 5, 2])
    env.step(a[1])
    env.restore(snap, src=perm)
    assert torch.equal(env.get_state(), before[torch.as_tensor(perm, device=DEV)])
    assert all(np.array_equal(env.params[k], params[k]) for k in params)
    # replica b now continues replica perm[b]'s state under its OWN parameters: what a uniform handle of b's set does from there
    # (lorenz: get_state() is the whole state but the episode counter)
    env.step(a[2])
    if name == "lorenz":
        for k, kw in enumerate(PSETS[name]):
            uni = make(name, "f64", 6, **kw)
            uni.reset()
            uni.set_state(before[torch.as_tensor(perm, device=DEV)])
            uni.step(a[2])
            rows = torch.arange(k, 6, 3, device=DEV)
            assert torch.equal(uni.obs[rows], env.obs[rows]) and torch.equal(uni.rwd[rows], env.rwd[rows]), k
            uni.close()
    env.fork(np.array([0, 0, 0, 3, 3, 3]))
    assert all(np.array_equal(env.params[k], params[k]) for k in params)
    st = env.get_state()
    assert torch.equal(st[1], st[0]) and torch.equal(st[5], st[3])
    env.close(), twin.close()


def test_invalid_input_raises_value_error_and_launches_nothing():
    env = make("sloshing", "f32")
    env.reset()
    a, _ = inputs("sloshing", env, 1)
    env.step(a[0])
    state, params = env.get_state().clone(), env.params
    for kw in (dict(gravity=9.0), dict(g=[9.81] * (B - 1)), dict(g=np.ones((B, 2))), dict(g=float("nan")), dict(amp=[float("inf")] + [1.0] * (B - 1)),
               dict(g=0.0), dict(g=[9.81] * 3 + [-1.0] + [9.81] * (B - 4)), dict(amp=5.0, alpha=torch.full((B + 1,), 1e-3))):
        with pytest.raises(ValueError):
            env.set_params(**kw)
        assert all(np.array_equal(env.params[k], params[k]) for k in params)   # nothing changed
        assert env.kernel_name == "sloshing_step_pk_k"
    assert torch.equal(env.get_state(), state)
    env.set_params(amp=-3.0, alpha=0.0)                                        # not divisors: any finite value
    env.close()
    for name, bad in (("rayleigh", dict(ra=0.0)), ("mixing", dict(re=-1.0)), ("mixing", dict(pe=0.0)), ("shkadov", dict(delta=0.0)),
                      ("vortex", dict(re=0.0)), ("lorenz", dict(rho=float("nan")))):
        e = make(name, "f32", 2)
        with pytest.raises(ValueError) as err:
            e.set_params(**bad)
        assert list(bad)[0] in str(err.value) and "replica 0" in str(err.value)
        e.close()
    # the C ABI validates on its own, before it touches the device, and names the parameter and the replica
    e = make("shkadov", "f64", 3)
    vals = (_lib.C.c_double * 3)(0.1, 0.2, -0.5)
    assert e.lib.bcn_set_params(e.h, vals, None) == 1
    msg = e.lib.bcn_last_error().decode()
    assert "delta" in msg and "replica 2" in msg
    assert e.lib.bcn_n_params(e.h) == 1 and e.lib.bcn_param_name(e.h, 0) == b"delta" and e.lib.bcn_param_name(e.h, 1) == b""
    assert np.array_equal(e.params["delta"], np.full(3, 0.1))
    e.close()


@pytest.mark.parametrize("name", ["rayleigh", "mixing"])
def test_2d_env_with_parameters_steps_through_the_generic_kernel_and_says_so(name):
    """The first set_params on an env whose default kernel is a register-resident one warns once and names both kernels;
    kernel_name reports ns2d_generic_step while the table is set -- also on the handle set_ndt_act rebuilds -- and clear_params()
    restores the previous dispatch.  Then 256- and 1024-thread workgroups with the work arrays in LDS and in global memory: every
    launch shape of the generic kernel reads the table."""
    env = make(name, "f32", 3)
    default = env.kernel_name
    assert default != "ns2d_generic_step"
    with pytest.warns(V.ParamsWarning) as rec:
        env.set_params(**columns(name, 3))
    assert len(rec) == 1 and "ns2d_generic_step" in str(rec[0].message) and default in str(rec[0].message)
    with warnings.catch_warnings():
        warnings.simplefilter("error", V.ParamsWarning)                        # only the first call warns
        env.set_params(**columns(name, 3))
    assert env.kernel_name == "ns2d_generic_step"
    a, _ = inputs(name, env, 2)
    env.reset()
    env.step(a[0])
    env.check_status()
    assert env.kernel_name == "ns2d_generic_step"
    env.set_ndt_act(NDT_2D[name] + 1)                                                # a new handle: the table is applied again
    assert env.kernel_name == "ns2d_generic_step" and all(np.array_equal(env.params[k], v) for k, v in columns(name, 3).items())
    env.clear_params()
    assert env.kernel_name == default
    env.reset()
    env.step(a[1])
    env.check_status()
    assert env.kernel_name.startswith("ns2d_fast")
    env.close()
    # every launch shape of the generic kernel against uniform handles: 256 / 1024 threads, work arrays in LDS / in global memory
    # (100x100 float64: 3 x 102 x 102 doubles exceed the LDS budget); grids with built-in register-resident kernels only
    if name == "rayleigh":
        shapes = [("f64", 256, {}), ("f64", 1024, {}), ("f64", 256, dict(L=2.0, H=2.0)), ("f64", 0, dict(L=2.0, H=2.0))]
    else:
        shapes = [("f32", 256, {}), ("f32", 1024, {}), ("f64", 256, {}), ("f64", 1024, {})]
    nb = 3

    def run(dtype, threads, kw, params):
        e = V.VecRayleigh(nb, DEV, dtype, None, **kw) if name == "rayleigh" else V.VecMixing(nb, DEV, dtype, **kw)
        e.set_ndt_act(3)
        e.set_option("generic_threads", threads)
        if params:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", V.ParamsWarning)
                e.set_params(**params)
        else:
            assert e.set_variant(0) == 0
        acts, _ = inputs(name, e, 1, seed=9)
        e.reset()
        if name == "rayleigh":
            e.set_state(np.tile(np.ascontiguousarray(e.perturbed_conduction_state().transpose(0, 2, 1))[None], (nb, 1, 1, 1)))
        e.step(acts[0])
        e.check_status()
        assert e.kernel_name == "ns2d_generic_step"
        out = record(e)
        e.close()
        return out

    for dtype, threads, kw in shapes:
        got = run(dtype, threads, kw, columns(name, nb))
        for k in range(nb):
            want = run(dtype, threads, dict(kw, **PSETS[name][k]), None)
            for x, y in zip(got, want):
                assert torch.equal(x[k], y[k]), (name, dtype, threads, kw, k)
