"""The float32 one-row-per-lane kernels with their Jacobi cells in runs (csrc/bcn_jacobi_cells.h) held to the cell-by-cell kernels of
the same grid BIT FOR BIT, at every strip width that takes the runs, and identical replicas held to each other under load.

    a  on demand: the 17 grids of flow_states.RUNS_TABLE (every R in 7..26 that takes the runs, the last-strip bodies of width 3 and
       8..11), the default plugin against its twin built with -DBCN_JACOBI_RUNS=0 (beacon_amd/jit.py: RUNS_GRIDS, RUNS_TWIN_DEFS)
    b  built in: 128x64, 50x50, 150x50, 200x50 through csrc/ns2d_fast_runs.hip against the pinned kernels of csrc/ns2d_fast.hip (option
       "cell_runs" 1 / 0; env.cell_runs_active says which unit the dispatch takes); 100x50 (R = 10) has no runs under either setting
    c  every grid of (a) against the float64 oracle, the generic kernel beside it on the same inputs
    d  B = 4 x the device's CUs replicas, replica b a copy of replica b % 4, two env steps: every copy equals its original in every bit

a - c follow tests/test_gpu_jacobi_cells.py: 3 replicas from the energetic states of tests/flow_states.py, each with its own action,
one env step of 4 timesteps, plain launch and ticket scheduler, the default evaluation plan and conv_plan 0.  "Equal" is torch.equal on
the whole state (ghosts included), obs, rwd and the sweep counts: no tolerance, no element left out.  Every run is made once and
shared by the tests that look at it; the oracle runs once per grid.  Nothing here reads the reference tree."""
import ctypes
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import flow_states as FS
from test_gpu_parity import DEV, _oracle_replica, dev2ref, maxdiff

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from beacon_amd import jit
    from beacon_amd import vec as V

    class _Twin(V.VecRayleigh):
        """VecRayleigh on the cell-by-cell twin of its grid's on-demand kernel: attached through the normal path, first-use
        self-check included."""
        _plugin_defs = dict(jit.RUNS_TWIN_DEFS)

B = 3
LAUNCHES = [("plain", (0, 0, 0)), ("ticket", (2, 2, 2))]
PLANS = (None, 0)
TABLE = [(FS._case(0, nx, ny, "f32"), R, RL) for nx, ny, R, RL in FS.RUNS_TABLE]
BUILTIN = [FS._case(0, 128, 64, "f32", 1), FS._case(0, 50, 50, "f32", 1), FS._case(0, 150, 50, "f32", 1), FS._case(0, 200, 50, "f32", 1)]
NO_RUNS = FS._case(0, 100, 50, "f32", 1)        # R = 10: csrc/ns2d_fast_runs.hip does not have it
NAMES = list("uvpT") + ["obs", "rwd"]


def _key(c):
    return (c["nx"], c["ny"], c["builtin"])


@functools.lru_cache(maxsize=None)
def _inputs(key):
    nx, ny, builtin = key
    st0, acts = FS.case_inputs(FS._case(0, nx, ny, "f32", int(builtin)))
    dev0 = np.ascontiguousarray(np.swapaxes(st0, -1, -2))
    for a in (st0, acts, dev0):
        a.setflags(write=False)
    return st0, acts, dev0


@functools.lru_cache(maxsize=None)
def _oracle(key):
    nx, ny, builtin = key
    c = FS._case(0, nx, ny, "f32", int(builtin))
    st0, acts, _ = _inputs(key)
    with ThreadPoolExecutor(max_workers=B) as ex:       # the ctypes calls of the oracle release the GIL
        return list(ex.map(lambda b: _oracle_replica(0, c["L"], c["H"], c["kw"], FS.NDT, st0[b], acts[b]), range(B)))


@functools.lru_cache(maxsize=None)
def _run(key, which, launch, plan):
    """One env step of the protocol on `which` kernel -- "runs" / "twin" (on demand: default plugin / cell-by-cell twin; built in:
    option cell_runs 1 / 0) or "generic" -- as CPU tensors (state, obs, rwd, sweeps).  Asserts that the env ran what was asked for."""
    nx, ny, builtin = key
    c = FS._case(0, nx, ny, "f32", int(builtin))
    _, acts, dev0 = _inputs(key)
    cls = _Twin if (which == "twin" and not builtin) else V.VecRayleigh
    env = cls(B, DEV, "f32", None, L=c["L"], H=c["H"], **c["kw"])
    try:
        assert (env.nx, env.ny) == (nx, ny)
        env.set_ndt_act(FS.NDT)
        if which == "generic":
            assert env.set_variant(0) == 0
        else:
            want = 1 if which == "runs" else 0
            assert env.set_variant(1) == 1
            env.set_sched(*LAUNCHES[launch][1])
            if plan is not None:
                env.set_option("conv_plan", plan)
            if builtin:
                assert getattr(env, "_plugin", None) is None
                env.set_option("cell_runs", want)
                has_runs = key != _key(NO_RUNS)
                assert env.cell_runs_active == bool(want and has_runs), "the dispatch does not follow the option cell_runs"
            else:
                p = getattr(env, "_plugin", None)
                assert p is not None and p.verified is True, "no verified plugin for %dx%d (%s)" % (nx, ny, which)
                assert ctypes.CDLL(p.path).bcn_jit_cell_runs() == want, "the attached plugin is not the %s build" % which
                assert env.cell_runs_active is False        # a handle on a plugin never takes the library's own runs unit
        env.reset()
        env.set_state(dev0[:B].copy())
        obs, rwd, _, _, _ = env.step(acts[:B].copy())
        env.check_status()
        if which == "generic":
            assert env.kernel_name == "ns2d_generic_step"
        else:
            assert env.kernel_name == "ns2d_fast" + ("_sched" if LAUNCHES[launch][1][0] == 2 else "_step")
        return env.get_state().cpu(), obs.detach().cpu().clone(), rwd.detach().cpu().clone(), env.sweeps.cpu().clone()
    finally:
        env.close()


def _assert_equal(a, b, what):
    for name, x, y in zip(("state", "obs", "rwd", "sweeps"), a, b):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, name)
        if not torch.equal(x, y):
            ne = (x != y) | (x != x) | (y != y)
            first = torch.nonzero(ne)[0].tolist()
            raise AssertionError("%s: %s differs in %d of %d elements, first at %s: %r vs %r"
                                 % (what, name, int(ne.sum()), ne.numel(), first, x[tuple(first)].item(), y[tuple(first)].item()))


def _distinct(res):
    for a in range(B):
        for b in range(a + 1, B):
            assert not torch.equal(res[0][a], res[0][b]) and not torch.equal(res[1][a], res[1][b])


@pytest.mark.parametrize("launch", range(len(LAUNCHES)), ids=[l[0] for l in LAUNCHES])
@pytest.mark.parametrize("gi", range(len(TABLE)), ids=["%s-R%d-RL%d" % (FS.case_id(g[0]), g[1], g[2]) for g in TABLE])
def test_on_demand_runs_equal_their_cell_by_cell_twin(gi, launch):
    c, R, RL = TABLE[gi]
    m = jit.choose(c["nx"], c["ny"], False, 0)
    assert (m["rows"], m["R"], jit.geometry(1, c["nx"], c["ny"], m["R"], m["gf"], False)["rl"]) == (1, R, RL), "the mapping this case was chosen for"
    for plan in PLANS:
        runs, twin = _run(_key(c), "runs", launch, plan), _run(_key(c), "twin", launch, plan)
        assert runs[0].shape == (B, 4, c["ny"] + 2, c["nx"] + 2) and runs[3].shape == (B, FS.NDT) and int(runs[3].min()) > 0
        _assert_equal(runs, twin, "%s %s conv_plan %s, runs vs twin" % (FS.case_id(c), LAUNCHES[launch][0], plan))
        _distinct(runs)


@pytest.mark.parametrize("launch", range(len(LAUNCHES)), ids=[l[0] for l in LAUNCHES])
@pytest.mark.parametrize("gi", range(len(BUILTIN) + 1), ids=[FS.case_id(c) for c in BUILTIN + [NO_RUNS]])
def test_built_in_runs_equal_the_pinned_kernels(gi, launch):
    """Option cell_runs 1 against 0.  _run asserts what env.cell_runs_active answers: 1 and 0 -- on 100x50 0 and 0."""
    c = (BUILTIN + [NO_RUNS])[gi]
    from beacon_amd import _lib
    assert _lib.load().bcn_builtin_cell_runs(c["nx"], c["ny"]) == (0 if c is NO_RUNS else 1)
    for plan in PLANS:
        runs, pinned = _run(_key(c), "runs", launch, plan), _run(_key(c), "twin", launch, plan)
        assert runs[0].shape == (B, 4, c["ny"] + 2, c["nx"] + 2) and runs[3].shape == (B, FS.NDT) and int(runs[3].min()) > 0
        _assert_equal(runs, pinned, "%s %s conv_plan %s, cell_runs 1 vs 0" % (FS.case_id(c), LAUNCHES[launch][0], plan))
        _distinct(runs)


def test_option_cell_runs_is_refused_where_it_means_nothing():
    from beacon_amd import _lib
    env = V.VecRayleigh(2, DEV, "f64", None)
    try:
        env.set_option("cell_runs", 0)
        assert env.cell_runs_active is False
        env.set_option("cell_runs", 1)
        assert env.cell_runs_active is False                # float64: the runs are float32 kernels
        with pytest.raises(_lib.BeaconHipError):
            env.set_option("cell_runs", 2)
    finally:
        env.close()
    env = V.VecRayleigh(2, DEV, "f32", None)
    try:
        assert env.cell_runs_active is True                 # the default
        assert env.set_variant(0) == 0 and env.cell_runs_active is False
        assert env.set_variant(1) == 1 and env.cell_runs_active is True
    finally:
        env.close()
    one_d = V.VecBurgers(2, DEV, "f32")
    try:
        with pytest.raises(_lib.BeaconHipError, match="unknown option 'cell_runs'"):
            one_d.set_option("cell_runs", 0)
    finally:
        one_d.close()


def _errors(res, ref):
    st, obs, rwd = dev2ref(res[0]), res[1].double().numpy(), res[2].double().numpy()
    err = dict.fromkeys(NAMES, 0.0)
    for b in range(B):
        rst, rob, rrw, _ = ref[b]
        n = min(obs.shape[1], rob.shape[0])
        for i, F in enumerate("uvpT"):
            err[F] = max(err[F], maxdiff(st[b][i], rst[i], tag=F))
        err["obs"] = max(err["obs"], maxdiff(obs[b][-n:], rob[-n:], tag="obs"))
        err["rwd"] = max(err["rwd"], maxdiff(rwd[b], rrw, tag="rwd"))
    return err


@pytest.mark.parametrize("launch", range(len(LAUNCHES)), ids=[l[0] for l in LAUNCHES])
@pytest.mark.parametrize("gi", range(len(TABLE)), ids=["%s-R%d-RL%d" % (FS.case_id(g[0]), g[1], g[2]) for g in TABLE])
def test_on_demand_runs_vs_oracle_beside_the_generic_kernel(gi, launch):
    """Fields (ghosts included), obs and rwd of the kernels with runs and of the generic kernel within flow_states.F32_RUNS_GRIDS of the
    float64 oracle; the sweep count of every timestep equal under both plans.  The MEASURED lines carry both kernels' errors per field
    and their ratio (more than 3 x the generic kernel's on a field is a finding, not a number to tolerate)."""
    c, R, RL = TABLE[gi]
    ref = _oracle(_key(c))
    t = FS.F32_RUNS_GRIDS
    gen = _errors(_run(_key(c), "generic", None, None), ref)
    fails = ["generic %s: %.3e > %.1e" % (F, gen[F], t[F]) for F in NAMES if not gen[F] <= t[F]]
    sweeps = {}
    for plan in PLANS:
        res = _run(_key(c), "runs", launch, plan)
        err = _errors(res, ref)
        sweeps[plan] = res[3].numpy().astype(np.int64)
        print("MEASURED %s R %d RL %d %s conv_plan %s: runs %s | generic %s | ratio %s | sweeps %s, oracle %s"
              % (FS.case_id(c), R, RL, LAUNCHES[launch][0], "default" if plan is None else plan,
                 " ".join("%s %.1e" % (F, err[F]) for F in NAMES), " ".join("%s %.1e" % (F, gen[F]) for F in NAMES),
                 " ".join("%s %.2f" % (F, err[F] / gen[F] if gen[F] > 0 else float("inf")) for F in NAMES),
                 sweeps[plan].tolist(), [ref[b][3].tolist() for b in range(B)]))
        fails += ["conv_plan %s %s: %.3e > %.1e" % (plan, F, err[F], t[F]) for F in NAMES if not err[F] <= t[F]]
    assert not fails, fails
    # the default plan skips evaluations, never sweeps: it stops where the plan that evaluates every sweep stops
    assert sweeps[None].shape == (B, FS.NDT) and np.array_equal(sweeps[None], sweeps[0]), (sweeps[None].tolist(), sweeps[0].tolist())


# d. identical replicas under load: (case, on demand?) -- built in: the moved barrier at R = 16, 15, 25; on demand: the smallest width with
# the barrier between two runs (90x50, R = 12), a last body of width 9 (121x50) and the widest strips (201x50, R = 26)
LOAD = [FS._case(0, 128, 64, "f32", 1), FS._case(0, 150, 50, "f32", 1), FS._case(0, 200, 50, "f32", 1),
        FS._case(0, 90, 50, "f32"), FS._case(0, 121, 50, "f32"), FS._case(0, 201, 50, "f32")]
# (mode 2 with grid 0: one persistent workgroup per CU drawing tickets of 2 timesteps -- the scheduler as a trainer runs it; the plain
# launch: one workgroup per replica, four waiting per CU)
LOAD_LAUNCHES = [("ticket", (2, 0, 2), "ns2d_fast_sched"), ("plain", (0, 0, 0), "ns2d_fast_step")]
LOAD_STEPS = 2


def _load_run(c, batch, sched, name):
    """LOAD_STEPS env steps of `batch` replicas, replica b from energetic state b % 4 with action b % 4: per step (state, obs, rwd,
    sweeps), on the device."""
    _, acts, dev0 = _inputs(_key(c))
    assert dev0.shape[0] == 4 and batch % 4 == 0
    env = V.VecRayleigh(batch, DEV, "f32", None, L=c["L"], H=c["H"], **c["kw"])
    try:
        env.set_ndt_act(FS.NDT)
        assert env.set_variant(1) == 1
        if c["builtin"]:
            assert env.cell_runs_active is True
        else:
            p = getattr(env, "_plugin", None)
            assert p is not None and p.verified is True and ctypes.CDLL(p.path).bcn_jit_cell_runs() == 1
        env.set_sched(*sched)
        env.reset()
        env.set_state(torch.tensor(dev0).to(device=DEV, dtype=torch.float32).repeat(batch // 4, 1, 1, 1))
        a = torch.tensor(acts).to(device=DEV, dtype=torch.float32).repeat(batch // 4, 1)
        out = []
        for k in range(LOAD_STEPS):
            obs, rwd, _, _, _ = env.step(a if k == 0 else -a)
            env.check_status()
            assert env.kernel_name == name
            out.append((env.get_state(), obs.detach().clone(), rwd.detach().clone(), env.sweeps.clone()))
        return out
    finally:
        env.close()


@pytest.mark.parametrize("launch", range(len(LOAD_LAUNCHES)), ids=[l[0] for l in LOAD_LAUNCHES])
@pytest.mark.parametrize("gi", range(len(LOAD)), ids=[FS.case_id(c) for c in LOAD])
def test_identical_replicas_stay_bit_identical_under_load(gi, launch):
    """Race / hazard detector of the barrier inside the second sweep's inner cells (csrc/ns2d_fast_impl.h: BCN_TAIL2): 4 workgroups'
    worth of replicas per CU, every one a copy of one of four.  After each of two env steps every copy equals its original in state,
    obs, rwd and sweep counts, the first four equal a run of those four alone, and the four differ from each other."""
    c = LOAD[gi]
    tag, sched, name = LOAD_LAUNCHES[launch]
    ncu = torch.cuda.get_device_properties(DEV).multi_processor_count
    big = -(-4 * ncu // 4) * 4
    assert big > ncu
    four = _load_run(c, 4, (2, 2, 2) if sched[0] == 2 else sched, name)
    many = _load_run(c, big, sched, name)
    for k in range(LOAD_STEPS):
        for what, x, y in zip(("state", "obs", "rwd", "sweeps"), many[k], four[k]):
            assert x.shape[0] == big and y.shape[0] == 4
            ne = (x.reshape(big // 4, 4, -1) != x[:4].reshape(1, 4, -1)).any(-1)
            bad = torch.nonzero(ne)
            assert bad.numel() == 0, ("%s %s step %d: %s of %d copies differ from their original, first (group, original) %s"
                                      % (FS.case_id(c), tag, k, what, int(ne.sum()), bad[0].tolist()))
            assert torch.isfinite(x.float()).all()
            assert torch.equal(x[:4], y), "%s %s step %d: %s of the first four differ from the run of four replicas" % (FS.case_id(c), tag, k, what)
        st, obs = many[k][0], many[k][1]
        assert int(many[k][3].min()) > 0
        for a in range(4):
            for b in range(a + 1, 4):
                assert not torch.equal(st[a], st[b]) and not torch.equal(obs[a], obs[b])
    assert not torch.equal(many[0][0][:4], many[1][0][:4])      # the second step moved the state
