"""The device's inlet-noise stream -- what step(a) without a noise tensor and every random-start reset draw inside the kernels
(bcn_set_noise, bcn_shkadov_reset_random; csrc/env1d.h: bcn_philox4x32, bcn_device_noise) -- held to its host restatement
(tests/noise_ref.py, pinned on its own by tests/test_noise_host.py) and, through it, to the float64 oracle.

Two kinds of comparison, no tolerance of this file's own:
  bit for bit   the inlet value burgers keeps in its state against u_target + device_noise(...) formed on the host; an env under
                device noise against its twin that is handed the host's values for the same counters as an explicit noise tensor
                (one kernel, two sources of the same numbers: no rounding differs, in float32 either); drawn counts; counters.
  the project's against the oracle fed the host's noise: float64 at the levels of tests/test_gpu_shapes1d.py (fields and
                observations bit-identical, rewards within F64_RWD), float32 at BURGERS_F32 / shkadov_tol; the float32 fused reset
                against the step kernel's loop within SHK_PK_VS_SCALAR, as tests/test_gpu_randinit.py does.
Every comparison prints its maximum difference before it asserts.  The draw counter is read from env.snapshot().view("nctr").

Not reached: the `it >= 128` branch of csrc/shkadov_action.inc (timesteps beyond the 128 staged in LDS draw in place).  VecShkadov
fixes ndt_act = 50, so no constructor gets there, and none is contorted to."""
import numpy as np
import pytest
import torch

import noise_ref as NR
from beacon_amd import envs as E
from beacon_amd import vec as V
from oracle import oracle as O
from test_gpu_parity import shkadov_tol
from test_gpu_randinit import assert_same, make as make_shkadov, record as record_shkadov
from test_gpu_shapes1d import BURGERS_F32, F64_RWD, SHK_PK_VS_SCALAR, expected_shape

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NP = {"f64": np.float64, "f32": np.float32}
SEED_HI = (7 << 32) | 5                                       # a seed whose high word matters
SEGS = ("a_last", "a_prev", "stp")

# burgers: (dtype, one_wave) -> at 130 / 256 / 500 / 512 cells the one-wave kernel with masks, the one without (FIT), the packed
# float32 kernels with and without masks (one_wave = 1), the scalar one-wave kernels in their place (one_wave = 2), and the
# general LDS-halo kernel (one_wave = 0)
BURGERS_MODES = [("f64", 1), ("f64", 0), ("f32", 0), ("f32", 1), ("f32", 2)]
BURGERS_GRIDS = (130, 256, 500, 512)
# shkadov: (K, NT, n) of tests/test_gpu_randinit.py -- ragged grids, the full packed grid (4, 64, 256), the single-buffer (4, 1024)
SHK_SHAPES = [(1, 128, 125), (2, 128, 255), (4, 64, 253), (8, 64, 505), (4, 64, 256), (4, 1024, 4096)]
SHK_MODES = [("f64", 0), ("f32", 1), ("f32", 2)]


# ---- helpers ---------------------------------------------------------------------------------------------------------------------
def make_burgers(n, dtype, B, one_wave=1, seed=5, offset=0):
    env = V.VecBurgers(B, DEV, dtype, nx=n)
    env.set_option("one_wave", one_wave)
    env.set_noise_seed(seed, offset)
    env.reset()
    return env


def counters(env):
    torch.cuda.synchronize()
    return env.snapshot().view("nctr").cpu().numpy().astype(np.int64)


def host_noise(env, ctr):
    """The host's values for this env's replicas at draw counters ctr [B], in the env's precision: [B] (burgers, one per action
    step) or [B, ndt_act] (shkadov, one per timestep)."""
    b, ctr = np.arange(env.batch), np.asarray(ctr, dtype=np.int64)
    dt = NP[V.dtype_name(env.tdtype)]
    if isinstance(env, V.VecBurgers):
        return NR.device_noise(env.seed, env.replica_offset, b, ctr, 0, env.sigma, dt)
    return NR.device_noise(env.seed, env.replica_offset, b[:, None], ctr[:, None], np.arange(env.ndt_act)[None, :], env.sigma, dt)


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV)


def actions(env, rng):
    return dev(rng.uniform(-1, 1, (env.batch, env.n_jets) if isinstance(env, V.VecShkadov) else (env.batch,)).astype(
        NP[V.dtype_name(env.tdtype)]))


def record(env):
    """everything a step writes but the draw counter"""
    snap = env.snapshot()
    torch.cuda.synchronize()
    return dict(state=env.get_state().clone(), obs=env.obs.clone(), rwd=env.rwd.clone(), done=env.done.clone(),
                trunc=env.trunc.clone(), **{s: snap.view(s).clone() for s in SEGS})


def assert_twins(A, Bv, what):
    ra, rb = record(A), record(Bv)
    worst = {k: float((ra[k].double() - rb[k].double()).abs().max()) for k in ra}
    print("MEASURED %s: max |device noise - the same values passed| %s" % (what, {k: "%.2e" % v for k, v in worst.items()}))
    for k in ra:
        assert torch.equal(ra[k], rb[k]), (what, k, worst[k])


class Twins(object):
    """Env A steps under device noise; env B, built by the same call, is handed the host's values at A's counters -- which are
    kept HERE, on the host, by the documented rule (one tick per replica per step under device noise) and compared with A's
    after every step.  B's own counters never move."""

    def __init__(self, mk):
        self.A, self.B = mk(), mk()
        self.ctr = np.zeros(self.A.batch, dtype=np.int64)

    def step(self, acts, what, mask=None):
        nz = dev(host_noise(self.A, self.ctr))
        m = None if mask is None else dev(np.asarray(mask, dtype=np.uint8))
        self.A.step(acts, None, mask=m)
        self.B.step(acts, nz, mask=m)
        self.ctr += 1 if mask is None else (np.asarray(mask) != 0)
        self.check(what)

    def check(self, what):
        assert_twins(self.A, self.B, what)
        got = counters(self.A)
        print("MEASURED %s: draw counters %s, by the rule %s" % (what, got[:8].tolist(), self.ctr[:8].tolist()))
        assert np.array_equal(got, self.ctr), (what, got, self.ctr)
        assert not counters(self.B).any()

    def close(self):
        self.A.close(), self.B.close()


def moved(env, before):
    """the comparison is not one of two untouched states"""
    return not torch.equal(env.get_state(), before)


# ---- a. the burgers inlet, bit for bit ---------------------------------------------------------------------------------------------
def burgers_inlet(env):
    torch.cuda.synchronize()
    return env.get_state()[:, 0, 0].cpu().numpy()


def want_inlet(env, ctr):
    dt = NP[V.dtype_name(env.tdtype)]
    want = dt(env.u_target) + host_noise(env, ctr)
    assert want.dtype == dt
    return want


@pytest.mark.parametrize("offset", [0, 37])
@pytest.mark.parametrize("seed", [5, SEED_HI], ids=["seed5", "seed_hi"])
@pytest.mark.parametrize("dtype,one_wave", BURGERS_MODES, ids=["%s-ow%d" % m for m in BURGERS_MODES])
def test_burgers_inlet_is_the_host_value(dtype, one_wave, seed, offset):
    """After step(0) the state holds u[0] = u_target + noise (burgers.py:137): three consecutive steps, 67 replicas (more than one
    wave of blocks, an odd count), each the host's u_target + device_noise(seed, offset, b, step, 0) formed in the env's precision."""
    B = 67
    for n in (130, 512):
        env = make_burgers(n, dtype, B, one_wave, seed, offset)
        zero = torch.zeros(B, dtype=env.tdtype, device=DEV)
        seen = []
        for i in range(3):
            env.step(zero)
            got, want = burgers_inlet(env), want_inlet(env, np.full(B, i))
            print("MEASURED burgers %s n=%d one_wave=%d seed=%#x offset=%d step %d (%s): max |inlet - host| %.2e"
                  % (dtype, n, one_wave, seed, offset, i, env.kernel_name, np.abs(got.astype(np.float64) - want).max()))
            assert np.array_equal(got, want), (n, i)
            assert np.array_equal(counters(env), np.full(B, i + 1))              # the number of device-noise steps taken
            seen.append(got)
        assert len(np.unique(np.stack(seen))) > 0.99 * 3 * B                     # 201 draws, not one repeated
        if one_wave == 1 and dtype == "f32":
            assert env.kernel_name == "burgers_step_pk_k"
        if one_wave == 0:
            assert env.kernel_shape[1] > 64                                      # the LDS-halo kernel: more than one wave
        env.close()


# ---- b. device noise = the same values passed explicitly, every shape -------------------------------------------------------------
@pytest.mark.parametrize("dtype,one_wave", BURGERS_MODES, ids=["%s-ow%d" % m for m in BURGERS_MODES])
def test_burgers_device_noise_equals_the_host_values_passed_explicitly(dtype, one_wave):
    names = set()
    for n in BURGERS_GRIDS:
        t = Twins(lambda: make_burgers(n, dtype, 5, one_wave, SEED_HI, 3))
        rng = np.random.default_rng([1, n])
        before = t.A.get_state().clone()
        for i in range(3):
            t.step(actions(t.A, rng), "burgers %s n=%d one_wave=%d step %d" % (dtype, n, one_wave, i))
        assert moved(t.A, before) and t.A.kernel_name == t.B.kernel_name and t.A.kernel_shape == t.B.kernel_shape
        names.add((t.A.kernel_name, t.A.kernel_shape))
        t.close()
    print("MEASURED burgers %s one_wave=%d kernels: %s" % (dtype, one_wave, sorted(names)))
    assert len(names) >= 2                                                       # the grids do select different instantiations


SHK_CASES = [(dt, K, NT, n, ow) for (dt, ow) in SHK_MODES for (K, NT, n) in SHK_SHAPES]


@pytest.mark.parametrize("dtype,K,NT,n,one_wave", SHK_CASES, ids=["%s-K%d-NT%d-n%d-ow%d" % c for c in SHK_CASES])
def test_shkadov_device_noise_equals_the_host_values_passed_explicitly(dtype, K, NT, n, one_wave):
    """[B, ndt_act] values, one per timestep: a timestep index that is off by one or constant within the action step, or a row of
    s_nz staged wrongly in this instantiation, changes the film against the twin's."""
    assert expected_shape(n, K) == (K, NT), "the grid does not select this shape: a mistake in the test"
    t = Twins(lambda: make_shkadov(n, dtype, 3, K, one_wave, seed=SEED_HI, offset=2))
    for env in (t.A, t.B):
        env.reset()
    rng = np.random.default_rng([2, n])
    before = t.A.get_state().clone()
    for i in range(3):
        t.step(actions(t.A, rng), "shkadov %s (%d,%d) n=%d one_wave=%d step %d" % (dtype, K, NT, n, one_wave, i))
        assert t.A.kernel_shape == (K, NT) and t.B.kernel_shape == (K, NT) and t.A.kernel_name == "shkadov_step_k"
    assert moved(t.A, before)
    # the inlet cell keeps 1 + the LAST timestep's value
    h0 = t.A.get_state()[:, 0, 0].cpu().numpy()
    want = NP[dtype](1) + host_noise(t.A, t.ctr - 1)[:, -1]
    print("MEASURED shkadov %s n=%d: max |h[0] - (1 + host value of the last timestep)| %.2e" % (dtype, n, np.abs(h0.astype(np.float64) - want).max()))
    assert np.array_equal(h0, want)
    t.close()


# ---- c. masked steps and resets --------------------------------------------------------------------------------------------------
def twins_for(name, dtype):
    if name == "burgers":
        return Twins(lambda: make_burgers(130, dtype, 4, 1, 5, 0))
    t = Twins(lambda: make_shkadov(255, dtype, 4, 2, 0 if dtype == "f64" else 1, seed=5))
    t.A.reset(), t.B.reset()
    return t


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ["burgers", "shkadov"])
def test_masked_replica_keeps_its_counter_and_resets_leave_it_alone(name, dtype):
    """A replica that a mask leaves out of a step keeps its draw counter, and its next draw is the host's value at the unticked
    counter; reset() and reset(mask) leave every counter where it is (include/beacon_hip.h: bcn_set_noise), so the episode after
    a reset goes on in the stream; set_noise_seed sets them back to 0."""
    t = twins_for(name, dtype)
    rng = np.random.default_rng(3)
    tag = "%s %s" % (name, dtype)
    t.step(actions(t.A, rng), tag + " all")
    t.step(actions(t.A, rng), tag + " masked [1,0,1,1]", mask=[1, 0, 1, 1])
    assert t.ctr.tolist() == [2, 1, 2, 2]
    t.step(actions(t.A, rng), tag + " all, replica 1 one draw behind")
    assert t.ctr.tolist() == [3, 2, 3, 3]
    for env in (t.A, t.B):
        env.reset()
    t.check(tag + " reset()")
    assert counters(t.A).tolist() == [3, 2, 3, 3]
    t.step(actions(t.A, rng), tag + " first step of the next episode")
    m = dev(np.array([0, 1, 1, 0], dtype=np.uint8))
    for env in (t.A, t.B):
        env.reset(mask=m)
    t.check(tag + " reset(mask)")
    assert counters(t.A).tolist() == [4, 3, 4, 4]
    t.step(actions(t.A, rng), tag + " after reset(mask)")
    assert counters(t.A).tolist() == [5, 4, 5, 5]
    if name == "burgers":
        assert np.array_equal(burgers_inlet(t.A), want_inlet(t.A, [4, 3, 4, 4]))
    t.A.set_noise_seed(t.A.seed, t.A.replica_offset)
    assert counters(t.A).tolist() == [0, 0, 0, 0]
    t.close()


# ---- d. end to end against the oracle --------------------------------------------------------------------------------------------
def dist(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def check_vs_oracle(name, dtype, k, st, obs, rwd, o, res, worst, fails, where):
    """One replica after its k-th action step against the oracle object `o` and its step result `res`, at the levels of
    tests/test_gpu_shapes1d.py: compare()."""
    def check(what, d, tol):
        worst[what] = max(worst.get(what, 0.0), d)
        if not d <= tol:
            fails.append((what, d, tol) + where)

    nf = 3 if name == "burgers" else 2
    want_obs, want_rwd = np.asarray(res[0], np.float64), float(res[1])
    if dtype == "f64":
        check("fields_differ", float(not np.array_equal(st[:nf], o.w[:nf])), 0.0)
        check("obs_differ", float(not np.array_equal(obs, want_obs)), 0.0)
        check("rwd", dist(rwd, want_rwd), F64_RWD)
    elif name == "burgers":
        check("fields", dist(st[:nf], o.w[:nf]), BURGERS_F32["fields"])
        check("obs", dist(obs, want_obs), BURGERS_F32["obs"])
        check("rwd", dist(rwd, want_rwd), BURGERS_F32["rwd"])
    else:
        check("h", dist(st[0], o.w[0]), shkadov_tol("f32", k))
        check("q", dist(st[1], o.w[1]), 5 * shkadov_tol("f32", k))
        check("obs", dist(obs, want_obs), shkadov_tol("f32", k))
        check("rwd", dist(rwd, want_rwd), shkadov_tol("f32", k, reward=True))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name,n", [("burgers", 130), ("burgers", 512), ("shkadov", None)], ids=["burgers130", "burgers512", "shkadov_film"])
def test_three_steps_under_device_noise_against_the_oracle(name, n, dtype):
    """The path a training loop runs, against the oracle stepped with the host's noise (float32: the float32 values, cast to
    double): burgers at N = 130 and 512, shkadov on the packaged film with 5 jets."""
    B = 4
    if name == "burgers":
        env = make_burgers(n, dtype, B, 1, SEED_HI, 1)
        ors = [O.burgers(nx=n) for _ in range(B)]
    else:
        init = E.packaged_init("shkadov")
        env = make_shkadov(None, dtype, B, seed=SEED_HI, offset=1)
        env.reset()
        ors = [O.shkadov(init_fields=init) for _ in range(B)]
        for o in ors:
            o.rand_init = False
    for o in ors:
        o.reset()
    rng = np.random.default_rng([4, n or 0])
    worst, fails = {}, []
    for i in range(3):
        acts = rng.uniform(-1, 1, (B, env.n_jets) if name == "shkadov" else (B,))
        nz = host_noise(env, np.full(B, i)).astype(np.float64)
        env.step(acts)
        torch.cuda.synchronize()
        st, obs, rwd = (x.double().cpu().numpy() for x in (env.get_state(), env.obs, env.rwd))
        for b, o in enumerate(ors):
            res = o.step([acts[b]], nz[b]) if name == "burgers" else o.step(acts[b].tolist(), nz[b])
            check_vs_oracle(name, dtype, i + 1, st[b], obs[b], rwd[b], o, res, worst, fails, (i, b))
            assert bool(env.done[b]) == res[2] and bool(env.trunc[b]) == res[3] and int(env.status[b]) == 0
    print("MEASURED %s %s n=%s, three steps under device noise: max |device - oracle| %s"
          % (name, dtype, n, {k: "%.2e" % v for k, v in worst.items()}))
    assert not fails, fails[:6]
    assert counters(env).tolist() == [3] * B
    env.close()


# ---- e. the random-start reset with sigma > 0 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [3, 400])
def test_drawn_counts_are_the_host_counts(R):
    """B = 64, a seed with a high word, replica offset 1: n_rand is drawn_count() at the counter the reset found, and the counter
    moves by the count's tick plus one per warm-up step, a second reset drawing at the counter the first one left."""
    B = 64
    env = make_shkadov(255, "f64", B, 2, 0, seed=SEED_HI, offset=1)
    env.set_random_init(R)
    ctr = np.zeros(B, dtype=np.int64)
    for r in range(2):
        env.reset()
        torch.cuda.synchronize()
        got, want = env.n_rand.cpu().numpy().astype(np.int64), NR.drawn_count(SEED_HI, 1, np.arange(B), ctr, R)
        print("MEASURED R=%d reset %d: counts differ at %d of %d replicas; device min %d max %d"
              % (R, r, int((got != want).sum()), B, got.min(), got.max()))
        assert np.array_equal(got, want)
        ctr = ctr + 1 + want
        assert np.array_equal(counters(env), ctr)
    assert env.sigma > 0
    env.close()


def test_fused_reset_against_the_oracle_with_the_hosts_noise_f64():
    """float64, counts [0, 2, 5] on the packaged film, from a counter that is not 0: warm-up step i of replica b draws at counter
    ctr0 + 1 + i.  Fields and observations bit for bit, the level test_against_the_oracle_without_noise_f64 asserts."""
    init = E.packaged_init("shkadov")
    counts = [0, 2, 5]
    env = make_shkadov(None, "f64", 3, seed=SEED_HI)
    env.set_random_init(5)
    env.reset_random_device([0, 0, 0])
    env.step(None, None, mask=dev(np.array([1, 0, 1], dtype=np.uint8)))
    ctr0 = counters(env)
    assert ctr0.tolist() == [2, 1, 2]
    env.reset_random_device(counts)
    torch.cuda.synchronize()
    st, obs = env.get_state().cpu().numpy(), env.obs.cpu().numpy()
    worst = 0.0
    for b, n in enumerate(counts):
        o = O.shkadov(init_fields=init)
        nz = NR.device_noise(SEED_HI, 0, b, ctr0[b] + 1 + np.arange(n)[:, None], np.arange(o.cfg.ndt_act)[None, :], env.sigma, np.float64)
        ob, _ = o.reset(n_rand=n, noise=nz)
        worst = max(worst, dist(st[b, :2], o.w[:2]), dist(obs[b], ob))
        print("MEASURED fused reset f64 replica %d, %d warm-up steps: max |device - oracle| h,q %.2e obs %.2e"
              % (b, n, dist(st[b, :2], o.w[:2]), dist(obs[b], ob)))
        assert np.array_equal(st[b, :2], o.w[:2]), (b, n)
        assert np.array_equal(obs[b], ob), (b, n)
        assert o.stp == 0
        if n > 0:
            assert not np.array_equal(o.w[0], init[0][:o.nx])
    assert np.array_equal(counters(env), ctr0 + 1 + np.array(counts)) and env.get_stp().tolist() == [0, 0, 0]
    assert env.n_rand.tolist() == counts
    env.close()


def yardstick_explicit(env, n, ctr0):
    """The yardstick of tests/test_gpu_randinit.py with step(None, host_noise, mask) in place of step(None, None, mask): reset,
    masked steps fed the host's values at counters ctr0 + 1 + i, then stp = 0 and the counters the fused reset must leave
    (explicit noise moves none) through a Snapshot."""
    assert env.rand_steps is None
    n = np.asarray(n)
    env.reset()
    for i in range(int(n.max())):
        env.step(None, dev(host_noise(env, ctr0 + 1 + i)), mask=dev((n > i).astype(np.uint8)))
    snap = env.snapshot()
    snap.view("stp")[:] = 0
    snap.view("nctr")[:] = dev((ctr0 + 1 + n).astype(np.int32))
    env.restore(snap)
    return env


FUSED_CASES = [(dt, K, NT, n, ow) for (dt, ow) in SHK_MODES for (K, NT, n) in [(2, 128, 255), (4, 64, 256)]]


@pytest.mark.parametrize("dtype,K,NT,n,one_wave", FUSED_CASES, ids=["%s-K%d-NT%d-n%d-ow%d" % c for c in FUSED_CASES])
def test_fused_reset_equals_masked_steps_fed_the_hosts_noise(dtype, K, NT, n, one_wave):
    """float64 bit for bit; float32 within SHK_PK_VS_SCALAR (the looped kernel's contractions: tests/test_gpu_randinit.py) with
    counters and stored actions bit for bit."""
    counts = [0, 1, 3, 2]
    F, Y = make_shkadov(n, dtype, 4, K, one_wave, seed=SEED_HI, offset=1), make_shkadov(n, dtype, 4, K, one_wave, seed=SEED_HI, offset=1)
    F.set_random_init(3)
    F.reset_random_device(counts)
    torch.cuda.synchronize()
    assert F.kernel_shape == (K, NT) and F.kernel_name == "shkadov_warm_k"
    yardstick_explicit(Y, counts, np.zeros(4, dtype=np.int64))
    assert Y.kernel_shape == (K, NT) and Y.kernel_name == "shkadov_step_k"
    got, want = record_shkadov(F), record_shkadov(Y)
    assert max(counts) <= 3                                                      # the float32 bounds hold for up to three action steps
    assert_same(got, want, "explicit-noise yardstick %s (%d,%d) n=%d one_wave=%d" % (dtype, K, NT, n, one_wave), f32_vs_step=dtype == "f32")
    assert got["nctr"].tolist() == [1 + c for c in counts] and got["stp"].tolist() == [0] * 4
    F.close(), Y.close()


@pytest.mark.parametrize("dtype,K,NT,n,one_wave", FUSED_CASES, ids=["%s-K%d-NT%d-n%d-ow%d" % c for c in FUSED_CASES])
def test_first_step_after_the_fused_reset_draws_at_one_plus_n(dtype, K, NT, n, one_wave):
    def mk():
        env = make_shkadov(n, dtype, 4, K, one_wave, seed=SEED_HI)
        env.set_random_init(3)
        env.reset_random_device([0, 1, 3, 2])
        return env
    t = Twins(mk)
    t.ctr = np.array([1, 2, 4, 3], dtype=np.int64)                               # 1 + n[b]
    # B took the same fused reset, so its counters stand where A's do; from here on they stay
    assert np.array_equal(counters(t.A), t.ctr) and np.array_equal(counters(t.B), t.ctr)
    nz = dev(host_noise(t.A, t.ctr))
    a = actions(t.A, np.random.default_rng(6))
    t.A.step(a)
    t.B.step(a, nz)
    assert_twins(t.A, t.B, "first step after the fused reset %s (%d,%d) n=%d one_wave=%d" % (dtype, K, NT, n, one_wave))
    assert np.array_equal(counters(t.A), t.ctr + 1) and np.array_equal(counters(t.B), t.ctr)
    assert t.A.kernel_shape == (K, NT) and t.A.kernel_name == "shkadov_step_k"
    t.close()


# ---- f. graph replay -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_graph_replay_draws_the_hosts_values_burgers(dtype):
    """Two captured steps, replayed twice: the inlet after the replays is the host's value at counters 1 and 3."""
    B = 6
    env = make_burgers(130, dtype, B, 1, SEED_HI, 2)
    g = env.capture(torch.zeros((2, B), dtype=env.tdtype, device=DEV), None, n_steps=2)
    assert not counters(env).any()                                               # a capture runs nothing
    for r in range(2):
        g.replay()
        got, want = burgers_inlet(env), want_inlet(env, np.full(B, 2 * r + 1))
        print("MEASURED burgers %s replay %d: max |inlet - host at counter %d| %.2e"
              % (dtype, r, 2 * r + 1, np.abs(got.astype(np.float64) - want).max()))
        assert np.array_equal(got, want)
        assert counters(env).tolist() == [2 * r + 2] * B
    env.close()


@pytest.mark.parametrize("dtype,one_wave", SHK_MODES, ids=["%s-ow%d" % m for m in SHK_MODES])
def test_graph_replay_draws_the_hosts_values_shkadov(dtype, one_wave):
    """(4, 64, 256): the inlet cell, and the whole film against the twin stepped eagerly with the host's values at counters 0 .. 3."""
    B = 3
    G, Y = make_shkadov(256, dtype, B, 4, one_wave, seed=SEED_HI), make_shkadov(256, dtype, B, 4, one_wave, seed=SEED_HI)
    G.reset(), Y.reset()
    acts = dev(np.random.default_rng(7).uniform(-1, 1, (4, B, G.n_jets)).astype(NP[dtype]))
    a_in = acts[:2].clone()
    g = G.capture(a_in, None, n_steps=2)
    for r in range(2):
        a_in.copy_(acts[2 * r:2 * r + 2])
        g.replay()
        for i in (2 * r, 2 * r + 1):
            Y.step(acts[i], dev(host_noise(Y, np.full(B, i))))
        assert_twins(G, Y, "shkadov %s one_wave=%d replay %d" % (dtype, one_wave, r))
        h0 = G.get_state()[:, 0, 0].cpu().numpy()
        assert np.array_equal(h0, NP[dtype](1) + host_noise(G, np.full(B, 2 * r + 1))[:, -1])
        assert counters(G).tolist() == [2 * r + 2] * B
    assert G.kernel_shape == (4, 64)
    G.close(), Y.close()


# ---- g. fork and restore ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ["burgers", "shkadov"])
def test_fork_copies_the_counter_and_restore_repeats_the_draws(name, dtype):
    """fork(src = [0, 0, 0, 0]): every replica takes replica 0's state and draw counter but draws under its OWN index; restore(snap)
    takes the counters back, so the same step draws the same values again."""
    t = twins_for(name, dtype)
    rng = np.random.default_rng(8)
    tag = "%s %s" % (name, dtype)
    t.step(actions(t.A, rng), tag + " all")
    t.step(actions(t.A, rng), tag + " replica 0 alone", mask=[1, 0, 0, 0])
    assert t.ctr.tolist() == [2, 1, 1, 1]
    for env in (t.A, t.B):
        env.fork([0, 0, 0, 0])
    t.ctr[:] = t.ctr[0]                                                          # the counter of source 0 ...
    t.check(tag + " fork")
    snaps = [env.snapshot() for env in (t.A, t.B)]
    a = actions(t.A, rng)
    t.step(a, tag + " first step of the copies")                                 # ... under indices 0 .. 3: host_noise(b, 2)
    first = record(t.A)
    assert not torch.equal(first["state"][0], first["state"][1])                 # the copies part
    if name == "burgers":
        assert np.array_equal(burgers_inlet(t.A), want_inlet(t.A, [2, 2, 2, 2]))
    for env, s in zip((t.A, t.B), snaps):
        env.restore(s)
    t.ctr[:] = 2
    t.check(tag + " restore")
    t.step(a, tag + " the same step again")
    again = record(t.A)
    for k in first:
        assert torch.equal(first[k], again[k]), k
    t.close()


# ---- h. the training path --------------------------------------------------------------------------------------------------------
def test_training_path_against_the_oracle_f64():
    """VecShkadov on the packaged film with set_random_init(3), stp set two steps from the end, three step_autoreset() calls: an
    episode ends and restarts inside the run.  The oracle loop takes the host's counts and the host's noise; fields and
    observations bit for bit, rewards within F64_RWD, n_rand and the draw counters exactly."""
    B, R = 3, 3
    init = E.packaged_init("shkadov")
    env = make_shkadov(None, "f64", B, seed=SEED_HI, offset=4)
    env.set_random_init(R)
    ors = [O.shkadov(init_fields=init) for _ in range(B)]
    ctr = np.zeros(B, dtype=np.int64)
    ndt = ors[0].cfg.ndt_act

    def oracle_reset(b):
        n = int(NR.drawn_count(SEED_HI, 4, b, ctr[b], R))
        nz = NR.device_noise(SEED_HI, 4, b, ctr[b] + 1 + np.arange(n)[:, None], np.arange(ndt)[None, :], env.sigma, np.float64)
        ctr[b] += 1 + n
        return n, ors[b].reset(n_rand=n, noise=nz)[0]

    env.reset()
    n_want = [oracle_reset(b)[0] for b in range(B)]
    assert env.n_rand.tolist() == n_want and np.array_equal(counters(env), ctr)
    env.set_stp(env.n_act - 2)
    for o in ors:
        o.stp = o.n_act - 2
    rng = np.random.default_rng(9)
    worst, fails, ended = {}, [], 0
    for i in range(3):
        acts = rng.uniform(-1, 1, (B, env.n_jets))
        obs, rwd, done, trunc, info = env.step_autoreset(acts)
        torch.cuda.synchronize()
        obs, rwd, fin = obs.cpu().numpy(), rwd.cpu().numpy(), info.final_obs.cpu().numpy()
        for b, o in enumerate(ors):
            nz = NR.device_noise(SEED_HI, 4, b, ctr[b], np.arange(ndt), env.sigma, np.float64)
            ctr[b] += 1
            res = o.step(acts[b].tolist(), nz)
            assert bool(done[b]) == res[2] and bool(trunc[b]) == res[3], (i, b)
            want_obs = res[0]
            if res[2] or res[3]:
                ended += 1
                assert np.array_equal(fin[b], res[0]), (i, b)                    # the terminal observation
                n_want[b], want_obs = oracle_reset(b)                            # ... and the first of the next episode
            check_vs_oracle("shkadov", "f64", i + 1, env.get_state()[b].cpu().numpy(), obs[b], rwd[b], o, (want_obs, res[1]), worst, fails, (i, b))
        assert env.n_rand.tolist() == n_want and np.array_equal(counters(env), ctr), (i, env.n_rand.tolist(), n_want, counters(env), ctr)
        assert env.get_stp().tolist() == [o.stp for o in ors]
    print("MEASURED training path f64: %d episodes ended; counts %s, counters %s; max |device - oracle| %s"
          % (ended, n_want, ctr.tolist(), {k: "%.2e" % v for k, v in worst.items()}))
    assert ended == B and not fails, fails[:6]
    env.close()
