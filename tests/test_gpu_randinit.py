"""shkadov's device-side random-start reset on the GPU (VecShkadov.set_random_init / reset_random_device, bcn_shkadov_reset_random,
kernel shkadov_warm_k): one launch that resets a replica and lets it take its own n[b] uncontrolled action steps under device
noise with the fields in registers.

The yardstick is the path that existed before, built from existing primitives (yardstick() below): reset(mask); the count's tick
of the draw counter, by editing a Snapshot's nctr view and restoring it; masked step(None, None, mask = n > i) for i < max(n);
stp back to 0 through a Snapshot.  Compared: get_state(), obs and the snapshot segments a_last, a_prev, stp, nctr.
float64: bit for bit.  float32: the same body text with the same flags, but hipcc contracts a few multiply-adds of the looped kernel
differently from the step kernel's (measured on an MI355X at (4, 256), n = 1021, one_wave = 1: 7.7e-9 on the state after three action
steps, observations equal; DESIGN.md, "Random-start reset on the device"), so float32 fused-against-yardstick comparisons use the
project's variant-against-variant bounds for up to three action steps (tests/test_gpu_shapes1d.py: SHK_PK_VS_SCALAR, 5e-6 on h, q
and observations, 5e-4 on the rhs arrays) -- no new number -- with the stored actions and counters still bit for bit, and n[b] = 0
still bit for bit.  Comparisons of the fused kernel with itself (restore, shards, set_params, the training loop) stay bit for bit
in both precisions.  Every comparison prints its maxima before it asserts."""
import numpy as np
import pytest
import torch

from beacon_amd import envs as E
from beacon_amd import vec as V
from oracle import oracle as O
from test_gpu_shapes1d import SHK_PK_VS_SCALAR, ctor_kwargs, expected_shape

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 11
COUNTS = [0, 1, 3, 2]
SEGS = ("a_last", "a_prev", "stp", "nctr")


def make(n, dtype, B, K=0, one_wave=1, seed=SEED, offset=0, **over):
    """n: a grid length for the constructors of tests/test_gpu_shapes1d.py (flat film), or None: the packaged film, nx = 1100"""
    if n is None:
        env = V.VecShkadov(B, DEV, dtype, E.packaged_init("shkadov"), n_jets=5, **over)
    else:
        kw = dict(ctor_kwargs("shkadov", n))
        kw.update(over)
        env = V.VecShkadov(B, DEV, dtype, None, **kw)
        assert env.nx == n
    env.set_option("one_wave", one_wave)
    env.set_option("cells_per_thread", K)
    env.set_noise_seed(seed, offset)
    return env


def yardstick(env, n, mask=None):
    """What the fused reset must compute, from reset / snapshot / restore / masked step alone (the env's switch is off)."""
    assert env.rand_steps is None
    m = torch.ones(env.batch, dtype=torch.bool, device=DEV) if mask is None else torch.as_tensor(mask, device=DEV).bool()
    n = torch.as_tensor(n, device=DEV)
    env.reset(mask=m)
    snap = env.snapshot()
    snap.view("nctr")[m] += 1                                # the count's tick
    env.restore(snap)
    for i in range(int(n[m].max()) if bool(m.any()) else 0):
        env.step(None, None, mask=m & (n > i))
    snap = env.snapshot()
    snap.view("stp")[m] = 0
    env.restore(snap)
    return env


def record(env):
    snap = env.snapshot()
    assert "obs_hist" not in snap.names()                    # shkadov keeps no observation history: nothing more to compare
    torch.cuda.synchronize()
    return dict(state=env.get_state().clone(), obs=env.obs.clone(), **{s: snap.view(s).clone() for s in SEGS})


def assert_same(got, want, what, rows=None, f32_vs_step=False):
    """bit for bit; f32_vs_step: the float32 fused kernel against the step kernel's loop, at most three action steps -- h, q,
    observations and the rhs arrays within SHK_PK_VS_SCALAR, everything else bit for bit"""
    worst = {}
    for k in want:
        a, b = (got[k], want[k]) if rows is None else (got[k][rows], want[k][rows])
        worst[k] = float((a.double() - b.double()).abs().max()) if a.numel() else 0.0
    if f32_vs_step:
        st = (got["state"].double() - want["state"].double()).abs()
        worst["hq"], worst["rhs"] = float(st[:, :2].max()), float(st[:, 2:].max())
    print("MEASURED %s: max |fused - yardstick| %s" % (what, {k: "%.2e" % v for k, v in worst.items()}))
    for k in want:
        a, b = (got[k], want[k]) if rows is None else (got[k][rows], want[k][rows])
        if f32_vs_step and k in ("state", "obs"):
            continue
        assert torch.equal(a, b), (what, k, worst[k])
    if f32_vs_step:
        assert rows is None
        assert worst["hq"] <= SHK_PK_VS_SCALAR["hq"] and worst["rhs"] <= SHK_PK_VS_SCALAR["rhs"] and worst["obs"] <= SHK_PK_VS_SCALAR["obs"], (what, worst)


# ---- 1. explicit counts, every kind of kernel shape ------------------------------------------------------------------------------
# (K, NT, n): the ragged grids n = K NT - K + 1 (the last live thread holds one cell), the single-buffer float64 shape (4, 1024)
# at n = 4096 (two barriers per timestep; float32: the packed timestep), and one grid that fills (4, 64), where float32 runs packed
SHAPES = [(1, 128, 125), (2, 128, 255), (4, 64, 253), (4, 256, 1021), (8, 64, 505), (4, 1024, 4096), (4, 64, 256)]
assert all(n == K * NT - K + 1 or n == K * NT for K, NT, n in SHAPES if K > 1)
CASES1 = [(dt, K, NT, n, ow) for dt in ("f64", "f32") for (K, NT, n) in SHAPES for ow in ((0,) if dt == "f64" else (1, 2))]


@pytest.mark.parametrize("dtype,K,NT,n,one_wave", CASES1, ids=["%s-K%d-NT%d-n%d-ow%d" % c for c in CASES1])
def test_explicit_counts_equal_reset_and_masked_steps(dtype, K, NT, n, one_wave):
    assert expected_shape(n, K) == (K, NT), "the grid does not select this shape: a mistake in the test"
    B = 3 if n >= 4096 else 4
    counts = COUNTS[:B] if B == 4 else [0, 1, 3]
    F, Y = make(n, dtype, B, K, one_wave), make(n, dtype, B, K, one_wave)
    F.set_random_init(3)
    F.reset_random_device(counts)
    torch.cuda.synchronize()
    assert F.kernel_shape == (K, NT) and F.kernel_name == "shkadov_warm_k", (F.kernel_shape, F.kernel_name)
    yardstick(Y, counts)
    assert Y.kernel_shape == (K, NT) and Y.kernel_name == "shkadov_step_k"
    got, want = record(F), record(Y)
    assert max(counts) <= 3                                  # the float32 bounds hold for up to three action steps
    assert_same(got, want, "%s (%d,%d) n=%d one_wave=%d" % (dtype, K, NT, n, one_wave), f32_vs_step=dtype == "f32")
    assert F.n_rand.tolist() == counts
    assert got["nctr"].tolist() == [1 + c for c in counts] and got["stp"].tolist() == [0] * B     # the tick, one per noisy step
    # n[b] = 0: a plain reset plus the tick
    P = make(n, dtype, B, K, one_wave)
    P.reset()
    assert torch.equal(got["state"][0], P.get_state()[0]) and torch.equal(got["obs"][0], P.obs[0])
    # every replica with n > 0 moved away from the reset film (the comparison above is not one of two untouched films)
    assert all(not torch.equal(got["state"][b], P.get_state()[b]) for b in range(B) if counts[b] > 0)
    for env in (F, Y, P):
        env.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_default_dispatch_on_the_packaged_film(dtype):
    """nx = 1100, the shape the launcher picks by itself; counts beyond rand_steps and below 0 are clamped."""
    B = 4
    F, Y = make(None, dtype, B), make(None, dtype, B)
    F.set_random_init(3)
    F.reset_random_device([0, 1, 7, -2])
    yardstick(Y, COUNTS[:2] + [3, 0])
    torch.cuda.synchronize()
    assert F.kernel_shape == Y.kernel_shape and Y.kernel_shape != (0, 0)
    assert F.n_rand.tolist() == [0, 1, 3, 0]
    assert_same(record(F), record(Y), "%s packaged film, default shape %s" % (dtype, F.kernel_shape), f32_vs_step=dtype == "f32")
    F.close(), Y.close()


# ---- 2. against the oracle -------------------------------------------------------------------------------------------------------
def test_against_the_oracle_without_noise_f64():
    """sigma = 0: the reference's reset with rand_init, n uncontrolled steps of zero noise -- fields and observations bit for bit
    (the level DESIGN.md §14 records for float64); the draw counter takes the tick and nothing else."""
    init = E.packaged_init("shkadov")
    counts = [0, 2, 5]
    env = make(None, "f64", 3)
    env.sigma = 0.0
    env.set_noise_seed(SEED)
    env.set_random_init(5)
    env.reset_random_device(counts)
    torch.cuda.synchronize()
    st, obs = env.get_state().cpu().numpy(), env.obs.cpu().numpy()
    for b, n in enumerate(counts):
        o = O.shkadov(init_fields=init)
        ob, _ = o.reset(n_rand=n, noise=np.zeros((n, o.cfg.ndt_act)))
        assert np.array_equal(st[b, :2], o.w[:2]), (b, n)
        assert np.array_equal(obs[b], ob), (b, n)
        assert o.stp == 0
    assert env.snapshot().view("nctr").tolist() == [1, 1, 1] and env.get_stp().tolist() == [0, 0, 0]
    env.close()


# ---- 3. what it must not touch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_leaves_rwd_done_trunc_status_and_masked_replicas_alone(dtype):
    B = 4
    env = make(255, dtype, B, 2, 0)
    env.set_random_init(3)
    env.reset()
    acts = torch.as_tensor(np.random.default_rng(2).uniform(-1, 1, (B, env.n_jets)), device=DEV, dtype=env.tdtype)
    env.step(acts)
    env.step(acts)
    env.rwd.fill_(-7.5), env.done.fill_(3), env.trunc.fill_(5), env.status.fill_(-9)
    env.obs[1] = -777.25
    env._n_rand.fill_(-5)
    before = record(env)
    outs = [x.clone() for x in (env.rwd, env.done, env.trunc, env.status)]
    mask = torch.as_tensor([1, 0, 1, 1], dtype=torch.uint8, device=DEV)
    env.reset(mask=mask)
    after = record(env)
    for x, y in zip(outs, (env.rwd, env.done, env.trunc, env.status)):
        assert torch.equal(x, y)                                               # every row, reset or not
    for k in before:
        assert torch.equal(before[k][1], after[k][1]), k                       # the masked replica: state, obs, counters
    assert int(env.n_rand[1]) == -5 and all(0 <= int(env.n_rand[b]) <= 3 for b in (0, 2, 3))
    assert after["stp"].tolist() == [0, 2, 0, 0]
    assert all(not torch.equal(before["state"][b], after["state"][b]) for b in (0, 2, 3))
    env.close()


# ---- 4. drawn counts -------------------------------------------------------------------------------------------------------------
def test_drawn_counts():
    B, R = 64, 3
    env = make(255, "f64", B, 2, 0)
    env.set_random_init(R)
    snap = env.snapshot()
    env.reset()
    n1, r1 = env.n_rand.clone(), record(env)
    assert int(n1.min()) >= 0 and int(n1.max()) <= R
    assert sorted(set(n1.tolist())) == [0, 1, 2, 3]                            # a miss: 4 (3/4)^64 = 4e-8
    assert r1["nctr"].tolist() == (1 + n1).tolist()
    # the drawn counts do what explicit counts do
    Y = yardstick(make(255, "f64", B, 2, 0), n1)
    assert_same(r1, record(Y), "drawn counts against the yardstick with the same counts")
    Y.close()
    # a second reset draws again; a restored run redraws the same
    env.reset()
    n2 = env.n_rand.clone()
    assert not torch.equal(n1, n2) and int(n2.min()) >= 0 and int(n2.max()) <= R
    env.restore(snap)
    env.reset()
    assert torch.equal(env.n_rand, n1)
    assert_same(record(env), r1, "restore(snap) and the same reset")
    # shard invariance: replica b of an env at replica_offset 1 is replica b + 1 of the env at offset 0
    S = make(255, "f64", B, 2, 0, offset=1)
    S.set_random_init(R)
    S.reset()
    rs = record(S)
    assert torch.equal(S.n_rand[:B - 1], n1[1:])
    for k in r1:
        assert torch.equal(rs[k][:B - 1], r1[k][1:]), k
    S.close(), env.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_per_replica_delta_equals_an_env_constructed_with_it(dtype):
    deltas = [0.1, 0.08, 0.15]
    P = make(255, dtype, 3, 2, 0)
    P.set_params(delta=deltas)
    P.set_random_init(3)
    P.reset_random_device([2, 3, 1])
    rp = record(P)
    for b, d in enumerate(deltas):
        Cb = make(255, dtype, 3, 2, 0, delta=d)
        Cb.set_random_init(3)
        Cb.reset_random_device([2, 3, 1])
        rc = record(Cb)
        for k in rp:
            assert torch.equal(rp[k][b], rc[k][b]), (b, k)
        Cb.close()
    assert not torch.equal(rp["state"][0], rp["state"][1])
    P.close()


# ---- 5. in the training loop -----------------------------------------------------------------------------------------------------
def loop_env(ops=True):
    env = make(255, "f32", 6, 2, 0)
    env.use_torch_ops(ops)
    env.set_random_init(2)
    env.reset()
    env.set_stp(env.n_act - 1 - (np.arange(6) % 4))                            # episodes end at steps 0 .. 3
    return env


def loop_actions(env, n):
    return torch.as_tensor(np.random.default_rng(5).uniform(-1, 1, (n, env.batch, env.n_jets)), device=DEV, dtype=env.tdtype)


def test_step_autoreset_equals_step_track_and_masked_reset():
    A, M, Cc = loop_env(), loop_env(), loop_env(ops=False)                     # fused, by hand, fused through ctypes
    acts = loop_actions(A, 5)
    resets = 0
    for i in range(5):
        oa, ra, da, ta, _ = A.step_autoreset(acts[i])
        oc, rc, dc, tc, _ = Cc.step_autoreset(acts[i])
        M.step(acts[i])
        ep = M.track_episodes()
        M.reset(mask=ep.finished.clone())
        resets += int(ep.finished.sum())
        for got in ((oa, ra, da, ta), (oc, rc, dc, tc)):
            for x, y in zip(got, (M.obs, M.rwd, M.done, M.trunc)):
                assert torch.equal(x, y), i
    assert resets >= 6
    assert_same(record(A), record(M), "step_autoreset against step + track + reset(mask)")
    assert_same(record(Cc), record(M), "the ctypes binding")
    assert torch.equal(A.n_rand, M.n_rand) and torch.equal(Cc.n_rand, M.n_rand)
    assert int(A.n_rand.min()) >= 0 and int(A.n_rand.max()) <= 2
    for env in (A, M, Cc):
        env.close()


def test_captured_autoreset_rollout_restarts_from_random_phases():
    n = 4
    G, Eg = loop_env(), loop_env()
    acts = loop_actions(G, 2 * n)
    a_in = acts[:n].clone()
    g = G.capture(a_in, None, n_steps=n, autoreset=True)
    seqs = []
    for r in range(2):
        a_in.copy_(acts[r * n:(r + 1) * n])
        seqs.append([x.clone() for x in g.replay()])
    torch.cuda.synchronize()
    assert int(seqs[0][2].sum()) > 0                                           # episodes ended inside the graph
    k = 0
    for r in range(2):
        for i in range(n):
            outs = Eg.step_autoreset(acts[k])[:4]
            for got, want in zip(seqs[r], outs):
                assert torch.equal(got[i], want), (r, i)
            k += 1
    assert_same(record(G), record(Eg), "captured against eager step_autoreset")
    assert torch.equal(G.n_rand, Eg.n_rand)
    G.close(), Eg.close()
