"""The off-policy learner on the device (beacon_amd.TD3, beacon_amd.Replay, libbeacon_td3.so) against tests/td3_ref.py -- torch autograd
in float64 on the CPU, the ring, the sampling and the three random streams in NumPy -- on the MI355X.

How errors are measured (as in tests/test_gpu_learner.py): err(q) = max |device - reference| / max(1, max |reference|) for a quantity
q -- a gradient segment, a statistic, a parameter segment.  The reference gets the device's inputs (weights and rows as the device
holds them, cast to float64) and the host restatement's indices and draws, so the error is the kernels' arithmetic alone.

A condition on the inputs: min(Q'_1, Q'_2), the two clamps and relu are not smooth, and the device must take the reference's branch
on every live row.  check_margins asserts on the REFERENCE alone that |Q'_1 - Q'_2|, the distance of mu' + h eps from each bound, of
sigma z from +-c_noise and of every relu pre-activation from 0 exceed 100 x the case's tolerance.  The clamp case lies BEYOND the
clamps in some rows (asserted too), never near them.  The seeds below were found on the CPU with td3_ref for which that holds.

float64: f64_tol(m, chain) = (m + max(640, chain)) x 2^-53 x 500, the summation-order bound of tests/test_gpu_learner.py: a gradient
entry is the W-weighted mean of m per-row terms, each behind a chain of dot products of `chain` terms, so another order of the same
sums moves it by at most (m + chain) u max |term|, and the terms stay below 500 (asserted on the reference: row_term_max).  For the
critic the chain is D + sum(hidden), D = obs_dim + act_dim.  The policy gradient runs through TWO networks -- down Q_1 to the action
columns, then down mu -- so its chain is (D + sum(hidden)) + (obs_dim + sum(hidden)).
float32: the project's rule -- every tolerance in F32_TOL is at most 10 x the worst error measured on the MI355X over the cases, and
at most 10 x what td3_ref in float32 on the CPU (another summation order) shows against float64 on the same case; the three numbers
stand next to each other there."""
import types

import numpy as np
import pytest
import torch

import td3_ref as R
from beacon_amd import td3 as _td3  # noqa: F401  (the module under test: importing it touches neither a compiler nor the GPU)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U64 = 2.0 ** -53
SEED = 0x1234567887654321
GAMMA = 0.9
DTYPES = [torch.float32, torch.float64]


def f64_tol(m, chain=640):
    return (m + max(640, chain)) * U64 * 500.0


# float32: quantity -> case / shape / preset -> (tolerance, the error measured on the MI355X, the error of td3_ref in float32 on the CPU
# on the same case).  Every tolerance is at most 10 x either number.
F32_TOL = {
    "act": {"a1": (8.5e-7, 8.755e-8, 8.563e-8), "a16": (1.5e-6, 1.604e-7, 1.526e-7), "a3": (2.0e-6, 2.464e-7, 2.099e-7)},
    "critic_grad": {"one": (9.6e-7, 2.145e-7, 9.668e-8), "straddle": (1.6e-6, 2.081e-7, 1.638e-7), "wide": (1.2e-6, 1.463e-7, 1.234e-7),
                    "tiles": (2.4e-7, 2.487e-8, 1.167e-6), "clamps": (1.6e-6, 1.748e-7, 1.613e-7)},
    "critic_stats": {"one": (9.4e-7, 1.528e-7, 9.469e-8), "straddle": (2.3e-7, 2.343e-8, 9.102e-8), "wide": (1.3e-7, 1.383e-8, 1.079e-7),
                     "tiles": (5.1e-8, 5.135e-9, 2.420e-7), "clamps": (5.7e-7, 6.741e-8, 5.703e-8)},
    "policy_grad": {"one": (3.4e-7, 3.485e-8, 3.485e-8), "straddle": (9.1e-8, 1.182e-8, 9.148e-9), "wide": (2.7e-7, 4.000e-8, 2.763e-8),
                    "tiles": (6.3e-8, 6.328e-9, 5.151e-8), "clamps": (2.1e-7, 3.825e-8, 2.135e-8)},
    "policy_stats": {"one": (6.5e-7, 6.860e-8, 6.579e-8), "straddle": (1.5e-7, 1.511e-8, 4.750e-8), "wide": (2.4e-7, 2.424e-8, 2.744e-8),
                     "tiles": (2.0e-8, 2.008e-9, 2.932e-9), "clamps": (2.5e-7, 3.080e-8, 2.581e-8)},
    "adam_params": {"clamps": (6.4e-7, 6.541e-8, 6.417e-8)}, "polyak": {"clamps": (9.4e-7, 9.482e-8, 9.482e-8)},
    "e2e_params": {"td3": (9.7e-7, 9.781e-8, 9.781e-8), "ddpg": (1.2e-4, 1.232e-5, 5.677e-5)}}

# (name, m float32 / float64, obs_dim float32 / float64, act_dim, hidden, activation, n_critics, options, data seed)
#   one       a single row
#   straddle  a partial second tile (65 / 33 rows); the action columns straddle a K-slab (62 + 3 / 30 + 3); relu; dead rows of NaN
#   wide      the two-pass register tile at every layer, 16 actions, one critic, rows with boot = 0
#   tiles     more tiles than the backward launches' grid (129 > 128: a workgroup walks a second tile), dead rows; one critic and no
#             smoothing: no 8 193 draws keep |Q'_1 - Q'_2| and sigma z away from their kinks
#   clamps    both clamps of the smoothing noise and both bounds of a' are hit; widths that are no multiple of 4
CASES = [("one", (1, 1), (3, 3), 1, (7,), "tanh", 2, {}, 1),
         ("straddle", (65, 33), (62, 30), 3, (7,), "relu", 2, {"dead": True}, 24),
         ("wide", (65, 33), (6, 6), 16, (128, 128, 128), "tanh", 1, {"boot0": True}, 10),
         ("tiles", (8193, 4097), (3, 3), 2, (7,), "tanh", 1, {"dead": True, "target_noise": 0.0}, 4),
         ("clamps", (65, 33), (5, 5), 2, (33, 5), "tanh", 2, {"clamp": True, "dead": True}, 5)]
IDS = [c[0] for c in CASES]
# what (grid, tiles) must satisfy for the case to be in the regime it is named for
REGIME = {"tiles": lambda grid, tiles: grid == 128 and tiles == 129}


def tag(dtype):
    return "f64" if dtype == torch.float64 else "f32"


def npdt(dtype):
    return np.float64 if dtype == torch.float64 else np.float32


def tile_rows(dtype):
    return 32 if dtype == torch.float64 else 64


def err(dev, ref):
    ref = torch.as_tensor(np.asarray(ref)).double().reshape(-1)
    if ref.numel() == 0:
        return 0.0
    return float((torch.as_tensor(dev).double().cpu().reshape(-1) - ref).abs().max() / max(1.0, float(ref.abs().max())))


def tol_of(dtype, key, sub, m, chain):
    return f64_tol(m, chain) if dtype == torch.float64 else F32_TOL[key][sub][0]


class _Env(object):
    """what TD3 reads of an env: most tests need no solver behind the observation rows"""
    _norm_on = False
    action_is_int = False

    def __init__(self, batch, obs_dim, act_dim, dtype, low=-1.0, high=1.0):
        self.batch, self.obs_dim, self.tdtype, self.device = batch, obs_dim, dtype, torch.device(DEV)
        self.action_space = types.SimpleNamespace(low=np.full(act_dim, low), high=np.full(act_dim, high))
        self.obs = None


def unpack(case, dtype):
    name, ms, ods, ad, hidden, activation, nc, opt, seed = case
    k = 1 if dtype == torch.float64 else 0
    return name, ms[k], ods[k], ad, hidden, activation, nc, opt, seed


def make_data(case, dtype):
    """the case's weights, targets, ring, minibatch and hyperparameters on the CPU, in the values the device will hold"""
    name, m, od, ad, hidden, activation, nc, opt, seed = unpack(case, dtype)
    rng = np.random.default_rng(seed)
    nd = npdt(dtype)
    rnd = lambda d: {k: v.astype(nd).astype(np.float64) for k, v in d.items()}
    clamp = bool(opt.get("clamp"))
    low, high = (-0.5, 1.5) if clamp else (-1.0, 1.0)
    W = rnd(R.random_weights(od, ad, hidden, nc, seed))
    Wt = rnd(R.random_weights(od, ad, hidden, nc, seed + 100, scale=3.0 if clamp else 1.0))
    Cn = m + 7
    ring = R.Ring(Cn, od, ad, nd)
    ring.obs[:], ring.next_obs[:] = rng.standard_normal((Cn, od)), rng.standard_normal((Cn, od))
    ring.act[:], ring.rwd[:] = rng.uniform(low, high, (Cn, ad)), rng.standard_normal(Cn)
    ring.boot[:] = (rng.uniform(size=Cn) > 0.3) if opt.get("boot0") else 1
    ring.live[:] = (rng.uniform(size=Cn) > 0.25) if opt.get("dead") else 1
    dead = ring.live == 0
    for a in (ring.obs, ring.next_obs, ring.act, ring.rwd):
        a[dead] = np.nan                                # a dead row may hold anything
    ring.head[:] = (0, Cn, Cn, 5)
    hyper = dict(gamma=GAMMA, target_noise=opt.get("target_noise", 0.8 if clamp else 0.2), noise_clip=0.5)
    ctr = 3                                              # the smoothing stream's counter
    idx = R.sample_idx(m, SEED, Cn, 5)
    z = R.smooth_normals(SEED, m, ctr, ad, nd)
    return dict(W=W, Wt=Wt, ring=ring, idx=idx, z=z, ctr=ctr, hyper=hyper, low=low, high=high, batch=ring.gather(idx))


def make_ref(case, dtype, d, rdtype=torch.float64):
    name, m, od, ad, hidden, activation, nc, opt, seed = unpack(case, dtype)
    return R.Ref(od, ad, hidden, activation, d["low"], d["high"], nc, d["W"], d["Wt"], dtype=rdtype)


def make_agent(case, dtype, d, batch=4, **kw):
    from beacon_amd import TD3
    name, m, od, ad, hidden, activation, nc, opt, seed = unpack(case, dtype)
    env = _Env(batch, od, ad, dtype, d["low"], d["high"])
    agent = TD3(env, hidden=hidden, activation=activation, twin=nc == 2, seed=SEED, **dict(d["hyper"], **kw))
    nets = [[(d["W"]["%s_w%d" % (n, l)], d["W"]["%s_b%d" % (n, l)]) for l in range(len(hidden) + 1)] for n in ("mu", "q1", "q2")[:1 + nc]]
    agent.load(*nets)
    for k, v in d["Wt"].items():
        agent.target_weights[k].copy_(torch.as_tensor(v).to(dtype).view(agent.target_weights[k].shape))
    ring = d["ring"]
    mem = agent.replay(ring.C)
    for k in ("obs", "next_obs", "act", "rwd", "boot", "live", "head"):
        getattr(mem, k).copy_(torch.as_tensor(getattr(ring, k)).view(getattr(mem, k).shape))
    return agent, mem


def check_margins(case, dtype, ref, c, tol):
    """the module docstring's condition, on the reference's numbers"""
    name, m, od, ad, hidden, activation, nc, opt, seed = unpack(case, dtype)
    mg = dict(c["margins"], relu=ref.min_pre)
    print("td3 margins %s %s: %s (100 tol = %.3e)" % (name, tag(dtype), {k: "%.3e" % v for k, v in mg.items()}, 100 * tol))
    assert all(v > 100 * tol for v in mg.values()), (mg, tol)
    assert c["row_term_max"] <= 500.0
    if opt.get("clamp"):
        lv = c["live"]
        assert (c["noise_raw"][lv] > 0.5).any() and (c["noise_raw"][lv] < -0.5).any()
        assert (c["a_raw"][lv] > 1.5).any() and (c["a_raw"][lv] < -0.5).any()


@pytest.fixture(scope="module")
def refs():
    """(case name, dtype tag) -> the data and the float64 / float32 references' critic and policy results: computed once, read-only"""
    cache = {}

    def get(case, dtype):
        key = (case[0], tag(dtype))
        if key not in cache:
            d = make_data(case, dtype)
            ref = make_ref(case, dtype, d)
            c = ref.critic(d["batch"], d["z"], **d["hyper"])
            c["live"] = d["batch"]["w"] > 0
            p = ref.policy(d["batch"])
            out = dict(d=d, ref=ref, c=c, p=p, c32=None, p32=None)
            if dtype == torch.float32:
                r32 = make_ref(case, dtype, d, torch.float32)
                out["c32"], out["p32"] = r32.critic(d["batch"], d["z"], **d["hyper"]), r32.policy(d["batch"])
            cache[key] = out
        return cache[key]
    return get


def chains(case, dtype):
    name, m, od, ad, hidden, activation, nc, opt, seed = unpack(case, dtype)
    c = od + ad + sum(hidden)
    return c, c + od + sum(hidden)


def stat_err(dev, want, keys):
    return max(abs(dev[k] - want[k]) / max(1.0, abs(want[k])) for k in keys)


# ---- act ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("shape", [(1, (7,), "tanh"), (16, (33, 5), "relu"), (3, (128, 128, 128), "tanh")], ids=lambda s: "a%d-%s" % (s[0], "_".join(map(str, s[1]))))
def test_act(shape, dtype):
    from beacon_amd import TD3
    ad, hidden, activation = shape
    od, B, off = 11, tile_rows(dtype) + 1, 2 ** 32 - 3
    nd = npdt(dtype)
    rng = np.random.default_rng(ad)
    W = {k: v.astype(nd).astype(np.float64) for k, v in R.random_weights(od, ad, hidden, 1, 17).items()}
    env = _Env(B, od, ad, dtype, -0.5, 1.5)
    agent = TD3(env, hidden=hidden, activation=activation, twin=False, seed=SEED, replica_offset=off, explore_noise=0.7)
    agent.load(*[[(W["%s_w%d" % (n, l)], W["%s_b%d" % (n, l)]) for l in range(len(hidden) + 1)] for n in ("mu", "q1")])
    ref = R.Ref(od, ad, hidden, activation, -0.5, 1.5, 1, W)
    obs_np = rng.standard_normal((B, od)).astype(nd)
    obs = torch.as_tensor(obs_np).to(DEV)
    tol = tol_of(dtype, "act", "a%d" % ad, 1, od + sum(hidden))
    # deterministic: mu, no tick
    a = agent.act(obs, mode="deterministic")
    assert a is agent.actions and tuple(a.shape) == (B, ad)
    mu, _ = ref.act(obs_np.astype(np.float64), np.zeros((B, ad)), 0.7)
    e_det = err(a, mu)
    assert not bool(agent.counters.any())
    # noisy: the host's draws; counters tick; actions pushed past a bound equal it exactly
    agent.counters.copy_(torch.arange(B, dtype=torch.int32) * 3)
    ctr = np.arange(B) * 3
    z = R.explore_normals(SEED, off, ctr, ad, nd)
    _, want = ref.act(obs_np.astype(np.float64), z, 0.7)
    raw = mu + 1.0 * 0.7 * z
    a = agent.act(obs, mode="noisy").clone()
    e_noisy = err(a, want)
    assert agent.counters.cpu().tolist() == (ctr + 1).tolist()
    hi, lo = raw > 1.5 + 1e-3, raw < -0.5 - 1e-3
    assert hi.any() and lo.any() if ad > 1 else (hi.any() or lo.any())
    an = a.cpu().numpy()
    assert (an[hi] == nd(1.5)).all() and (an[lo] == nd(-0.5)).all() and an.min() >= -0.5 and an.max() <= 1.5
    # uniform: low + (high - low) u on the same stream, at the ticked counters
    u = R.explore_uniforms(SEED, off, ctr + 1, ad, nd)
    a = agent.act(obs, mode="uniform").clone()
    e_uni = err(a, -0.5 + 2.0 * u)
    assert float(a.min()) >= -0.5 and float(a.max()) <= 1.5 and agent.counters.cpu().tolist() == (ctr + 2).tolist()
    # masked rows and their counters are untouched, bit for bit
    mask = torch.as_tensor(np.arange(B) % 3 != 0)
    before, cb = agent.actions.clone(), agent.counters.clone()
    agent.act(obs, mask=mask, mode="noisy")
    skipped = ~mask.to(DEV)
    assert torch.equal(agent.actions[skipped], before[skipped]) and torch.equal(agent.counters[skipped], cb[skipped])
    assert torch.equal(agent.counters[~skipped], cb[~skipped] + 1) and not torch.equal(agent.actions[~skipped], before[~skipped])
    mu32 = R.Ref(od, ad, hidden, activation, -0.5, 1.5, 1, W, dtype=torch.float32).act(obs_np.astype(np.float64), z, 0.7)
    print("td3 act errors a%d %s %s: det %.3e noisy %.3e uniform %.3e (cpu32 det %.3e noisy %.3e)"
          % (ad, hidden, tag(dtype), e_det, e_noisy, e_uni, err(mu32[0], mu), err(mu32[1], want)))
    assert max(e_det, e_noisy, e_uni) <= tol, (e_det, e_noisy, e_uni, tol)


# ---- the replay memory -------------------------------------------------------------------------
def _mem_equals(mem, ring):
    for k in ("head", "obs", "act", "rwd", "next_obs", "boot", "live"):
        got, want = getattr(mem, k).cpu().numpy(), getattr(ring, k)
        assert got.dtype == want.dtype and got.tobytes() == want.reshape(got.shape).tobytes(), k


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_append_fabricated_rollouts(dtype):
    from beacon_amd import TD3, _lib as main
    T, B, od, ad, Cn = 4, 3, 5, 2, 17
    nd = npdt(dtype)
    agent = TD3(_Env(B, od, ad, dtype), hidden=(7,), seed=SEED)
    mem, ring = agent.replay(Cn), R.Ring(Cn, od, ad, nd)
    rng = np.random.default_rng(0)

    def rollout(cursor):
        obs, act, rwd = rng.standard_normal((T + 1, B, od)).astype(nd), rng.standard_normal((T, B, ad)).astype(nd), rng.standard_normal((T, B)).astype(nd)
        fo = (rng.standard_normal((T, B, od)) + 100.0).astype(nd)
        done, trunc, valid = np.zeros((T, B), np.uint8), np.zeros((T, B), np.uint8), np.ones((T, B), np.uint8)
        done[0, 1], trunc[1, 2] = 1, 1
        done[1, 0] = trunc[1, 0] = 1
        valid[1, 1] = 0
        obs[1, 1] = np.nan
        host = (obs, act, rwd, done, trunc, valid, fo)
        dev = [torch.as_tensor(x).to(DEV) for x in host]
        ro = types.SimpleNamespace(T=T, batch=B, flags=main.RO_FINAL_OBS, obs=dev[0], act=dev[1], rwd=dev[2], done=dev[3], trunc=dev[4], valid=dev[5],
                                   final_obs=dev[6], cursor=torch.tensor([cursor, 0, 0, 0], dtype=torch.int32, device=DEV))
        return ro, host
    for cursor, head in ((T, [12, 12, 12, 0]), (T, [7, 17, 24, 0]), (2, [13, 17, 30, 0]), (0, [13, 17, 30, 0]), (T + 3, [8, 17, 42, 0])):
        ro, host = rollout(cursor)
        assert mem.append(ro) is mem
        ring.append(*host, cursor=cursor)
        assert ring.head.tolist() == head
        _mem_equals(mem, ring)
    # all four (done, trunc) combinations and a valid = 0 row went in
    assert set(zip(*(x.reshape(-1).tolist() for x in host[3:5]))) == {(0, 0), (1, 0), (0, 1), (1, 1)} and not host[5].all()
    assert 0 < int(mem.boot.sum()) < Cn and 0 < int(mem.live.sum()) < Cn


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_append_from_an_env(dtype):
    from beacon_amd import TD3, vec as V
    B, T = 4, 3
    env = V.VecBurgers(B, DEV, dtype)
    agent = TD3(env, hidden=(7,), seed=3)
    w = R.random_weights(agent.obs_dim, agent.act_dim, (7,), 2, 1)
    agent.load(*[[(w["%s_w%d" % (n, l)], w["%s_b%d" % (n, l)]) for l in range(2)] for n in ("mu", "q1", "q2")])
    mem, ro = agent.replay(2 * T * B + 1), env.rollout(T)
    ring = R.Ring(mem.capacity, agent.obs_dim, agent.act_dim, npdt(env.tdtype))
    env.reset()
    env.set_stp(env.n_act - 1 - np.arange(B) % 3)               # episodes end at steps 0, 1, 2 of what follows
    ended = 0
    for it in range(3):
        ro.begin()
        for _ in range(T):
            env.step_autoreset(agent.act(mode="uniform" if it == 0 else "noisy"))
        mem.append(ro)
        n, _ = ro.check()
        assert n == T
        ended += int(ro.done.sum())
        host = [getattr(ro, k).cpu().numpy() for k in ("obs", "act", "rwd", "done", "trunc", "valid", "final_obs")]
        ring.append(host[0], host[1].reshape(T, B, agent.act_dim), *host[2:], cursor=n)
        _mem_equals(mem, ring)
    assert ring.head.tolist() == [(3 * T * B) % mem.capacity, mem.capacity, 3 * T * B, 0] and ended > 0
    env.close()


def test_sample_matches_the_restatement_and_a_captured_sample_follows_the_memory():
    from beacon_amd import TD3
    B, od, ad, Cn, m = 3, 5, 2, 4000, 1000
    agent = TD3(_Env(B, od, ad, torch.float32), hidden=(7,), seed=SEED)
    mem = agent.replay(Cn)
    idx = torch.full((m,), -1, dtype=torch.int32, device=DEV)
    mem.sample(idx)                                           # an empty memory: stored = max(0, 1)
    assert not bool(idx.any()) and mem.head.cpu().tolist() == [0, 0, 0, 1]
    mem.head.copy_(torch.tensor([5, 777, 777, 1], dtype=torch.int32))
    for k in range(3):
        mem.sample(idx)
        assert np.array_equal(idx.cpu().numpy(), R.sample_idx(m, SEED, 777, 1 + k)) and int(mem.head[3]) == 2 + k
    # captured: a replay reads stored and the counter from the device at that time
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        mem.sample(idx)
    g.replay()
    assert np.array_equal(idx.cpu().numpy(), R.sample_idx(m, SEED, 777, 4)) and int(mem.head[3]) == 5
    mem.head[1:2].fill_(3999)                                 # what a further append does to the rows stored
    g.replay()
    got = idx.cpu().numpy()
    assert np.array_equal(got, R.sample_idx(m, SEED, 3999, 5)) and got.max() >= 777 and int(mem.head[3]) == 6
    agent.set_seed(SEED + 1)
    assert int(mem.head[3]) == 0 and mem.head.cpu().tolist()[:3] == [5, 3999, 777]


# ---- the gradients -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gradients_and_stats_match_reference(case, dtype, refs):
    name, m, od, ad, hidden, activation, nc, opt, seed = unpack(case, dtype)
    r = refs(case, dtype)
    d, ref, c, p = r["d"], r["ref"], r["c"], r["p"]
    cchain, pchain = chains(case, dtype)
    tols = {k: tol_of(dtype, k, name, m, pchain if k.startswith("policy") else cchain) for k in ("critic_grad", "critic_stats", "policy_grad", "policy_stats")}
    check_margins(case, dtype, ref, c, max(tols.values()))
    if opt.get("dead"):
        assert 0 < d["batch"]["w"].sum() < m and np.isnan(d["batch"]["s"]).any()
    if opt.get("boot0"):
        assert 0 < d["batch"]["boot"].sum() < m
    agent, mem = make_agent(case, dtype, d)
    plan = agent.plan(mem, 1, m)
    tiles = -(-m // tile_rows(dtype))
    if name in REGIME:
        assert REGIME[name](agent.grid, tiles), (agent.grid, tiles)
    plan.idx.copy_(torch.as_tensor(d["idx"]).to(torch.int32))
    agent.step_count[2:3].fill_(d["ctr"])
    params0, target0 = agent.params.clone(), agent.target.clone()
    plan.critic_grad()
    cnames, pnames = ref.names_of(0), ref.names_of(1)
    ge = {k: err(plan.grads[k], c["grads"][k]) for k in cnames}
    st = agent.stats_dict()
    ckeys = ("critic_loss", "q1_mean", "q2_mean", "target_mean", "W", "critic_grad_norm")
    se = stat_err(st, c["stats"], ckeys)
    assert not any(bool(plan.grads[k].any()) for k in pnames)             # the critic step leaves mu's gradient alone
    qgrad = {k: plan.grads[k].clone() for k in cnames}
    plan.actor_grad()
    pe = {k: err(plan.grads[k], p["grads"][k]) for k in pnames}
    st = agent.stats_dict()
    pse = stat_err(st, p["stats"], ("policy_loss", "W", "policy_grad_norm"))
    assert all(torch.equal(plan.grads[k], qgrad[k]) for k in cnames)      # and the policy step the critics'
    assert stat_err(st, c["stats"], ckeys) == se
    assert torch.equal(agent.params, params0) and torch.equal(agent.target, target0)
    assert int(agent.step_count[2]) == d["ctr"] and mem.head.cpu().tolist() == d["ring"].head.tolist()
    line = "td3 errors %s %s: critic grad %.3e (%s) stats %.3e | policy grad %.3e (%s) stats %.3e" % (
        name, tag(dtype), max(ge.values()), max(ge, key=ge.get), se, max(pe.values()), max(pe, key=pe.get), pse)
    if r["c32"] is not None:
        c32, p32 = r["c32"], r["p32"]
        line += " | cpu32: critic grad %.3e stats %.3e policy grad %.3e stats %.3e" % (
            max(err(c32["grads"][k], c["grads"][k]) for k in cnames), stat_err(c32["stats"], c["stats"], ckeys),
            max(err(p32["grads"][k], p["grads"][k]) for k in pnames), stat_err(p32["stats"], p["stats"], ("policy_loss", "W", "policy_grad_norm")))
    print(line)
    assert max(ge.values()) <= tols["critic_grad"], (ge, tols)
    assert se <= tols["critic_stats"], (se, tols)
    assert max(pe.values()) <= tols["policy_grad"], (pe, tols)
    assert pse <= tols["policy_stats"], (pse, tols)


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_gradients_are_bit_reproducible(dtype, refs):
    case = CASES[4]
    d = refs(case, dtype)["d"]
    m = unpack(case, dtype)[1]
    outs = []
    for _ in range(2):
        agent, mem = make_agent(case, dtype, d)
        plan = agent.plan(mem, 2, m)
        plan.run()
        outs.append([x.clone() for x in (plan.grad, agent.stats, agent.params, agent.target, agent.state, mem.buf, plan.idx)])
    assert all(a.view(torch.uint8).equal(b.view(torch.uint8)) for a, b in zip(*outs))


# ---- Adam and Polyak ---------------------------------------------------------------------------
def _adam_reference(case, dtype, d, rdtype):
    """the three steps of test_adam_and_polyak with td3_ref's own Adam, in `rdtype`: the float32 yardstick"""
    ref = make_ref(case, dtype, d, rdtype)
    for _ in range(3):
        ref.adam(0, ref.critic(d["batch"], d["z"], **d["hyper"])["grads"], 1e-2)
        ref.adam(1, ref.policy(d["batch"])["grads"], 1e-2)
        ref.polyak(0.25)
    return ref


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_adam_and_polyak(dtype, refs):
    case = CASES[4]
    name, m, od, ad, hidden, activation, nc, opt, seed = unpack(case, dtype)
    d = refs(case, dtype)["d"]
    agent, mem = make_agent(case, dtype, d, lr=1e-2, tau=0.25)
    ref = make_ref(case, dtype, d)
    plan = agent.plan(mem, 1, m)
    plan.idx.copy_(torch.as_tensor(d["idx"]).to(torch.int32))
    cn, pn = ref.names_of(0), ref.names_of(1)
    # torch.optim.Adam on the reference's parameters with the reference's gradients
    tp = {k: v.clone().requires_grad_(True) for k, v in ref.W.items()}
    opts = [torch.optim.Adam([tp[k] for k in cn], lr=1e-2, betas=(0.9, 0.999), eps=1e-8), torch.optim.Adam([tp[k] for k in pn], lr=1e-2, betas=(0.9, 0.999), eps=1e-8)]
    worst = {"adam_params": 0.0, "polyak": 0.0}
    for step in range(3):
        agent.step_count[2:3].fill_(d["ctr"])
        z = d["z"]
        ref.W = {k: v.detach().clone() for k, v in tp.items()}
        c = ref.critic(d["batch"], z, **d["hyper"])
        before = {k: agent.weights[k].clone() for k in ref.names}
        tbefore = agent.target.clone()
        plan.critic_step()
        for k in cn:
            tp[k].grad = c["grads"][k].clone()
        opts[0].step()
        assert all(torch.equal(agent.weights[k], before[k]) for k in pn) and torch.equal(agent.target, tbefore)      # mu and the targets stay
        assert not any(torch.equal(agent.weights[k], before[k]) for k in cn)
        ref.W = {k: v.detach().clone() for k, v in tp.items()}
        p = ref.policy(d["batch"])
        before = {k: agent.weights[k].clone() for k in ref.names}
        plan.actor_grad().adam(1)
        for k in pn:
            tp[k].grad = p["grads"][k].clone()
        opts[1].step()
        assert all(torch.equal(agent.weights[k], before[k]) for k in cn) and torch.equal(agent.target, tbefore)      # q1, q2 and the targets stay
        worst["adam_params"] = max([worst["adam_params"]] + [err(agent.weights[k], tp[k].detach()) for k in ref.names])
        plan.polyak()                                                                                             # the targets move here alone
        ref.W = {k: v.detach().clone() for k, v in tp.items()}
        ref.polyak(0.25)
        assert not torch.equal(agent.target, tbefore)
        worst["polyak"] = max([worst["polyak"]] + [err(agent.target_weights[k], ref.Wt[k]) for k in ref.names])
        assert agent.step_count.cpu().tolist() == [step + 1, step + 1, d["ctr"] + 1, 0]
    print("td3 adam errors %s: params %.3e targets %.3e" % (tag(dtype), worst["adam_params"], worst["polyak"]))
    cchain, pchain = chains(case, dtype)
    if dtype == torch.float32:
        r64, r32 = (_adam_reference(case, dtype, d, t) for t in (torch.float64, torch.float32))
        print("td3 adam errors cpu32: params %.3e targets %.3e" % (max(err(r32.W[k], r64.W[k]) for k in ref.names), max(err(r32.Wt[k], r64.Wt[k]) for k in ref.names)))
    for k, v in worst.items():
        assert v <= tol_of(dtype, k, name, m, pchain), (k, v)


# ---- end to end ----------------------------------------------------------------------------------
def _run_reference(case, dtype, d, n_updates, delay, lr, tau, rdtype=torch.float64):
    name, m, od, ad, hidden, activation, nc, opt, seed = unpack(case, dtype)
    ref = make_ref(case, dtype, d, rdtype)
    ring = d["ring"]
    head3, ctr = int(ring.head[3]), d["ctr"]
    for k in range(n_updates):
        idx = R.sample_idx(m, SEED, int(ring.head[1]), head3 + k)
        batch = ring.gather(idx)
        c = ref.critic(batch, R.smooth_normals(SEED, m, ctr + k, ad, npdt(dtype)), **d["hyper"])
        ref.adam(0, c["grads"], lr)
        if (k + 1) % delay == 0:
            ref.adam(1, ref.policy(batch)["grads"], lr)
            ref.polyak(tau)
    return ref


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("preset", ["td3", "ddpg"])
def test_end_to_end_update(preset, dtype, refs):
    from beacon_amd import TD3
    case = CASES[4] if preset == "td3" else CASES[2]
    name, m, od, ad, hidden, activation, nc, opt, seed = unpack(case, dtype)
    d = refs(case, dtype)["d"]
    lr, tau = 1e-3, 0.05
    if preset == "ddpg":
        d = dict(d, hyper=dict(d["hyper"], target_noise=0.0))
        agent, mem = make_agent(case, dtype, d, lr=lr, tau=tau, policy_delay=1)
        assert (agent.twin, agent.policy_delay, agent.target_noise) == (False, 1, 0.0)
        preset_agent = TD3.ddpg(agent.env, hidden=hidden)
        assert (preset_agent.twin, preset_agent.policy_delay, preset_agent.target_noise, preset_agent.n_critics) == (False, 1, 0.0, 1)
        delay = 1
    else:
        agent, mem = make_agent(case, dtype, d, lr=lr, tau=tau, policy_delay=2)
        delay = 2
    agent.step_count[2:3].fill_(d["ctr"])
    assert agent.update(mem, n_updates=6, batch_size=m) is agent
    ref = _run_reference(case, dtype, d, 6, delay, lr, tau)
    assert agent.step_count.cpu().tolist() == [6, 6 // delay, d["ctr"] + 6, 0] and int(mem.head[3]) == int(d["ring"].head[3]) + 6
    ep = max(err(agent.weights[k], ref.W[k]) for k in ref.names)
    et = max(err(agent.target_weights[k], ref.Wt[k]) for k in ref.names)
    line = "td3 e2e errors %s %s: params %.3e targets %.3e" % (preset, tag(dtype), ep, et)
    if dtype == torch.float32:
        r32 = _run_reference(case, dtype, d, 6, delay, lr, tau, torch.float32)
        line += " (cpu32 params %.3e)" % max(err(r32.W[k], ref.W[k]) for k in ref.names)
    print(line)
    # six steps of Adam: a parameter moves by at most lr per step whatever the gradient, and by lr x (relative gradient error) from
    # an error in it; under err()'s floor of 1 the float64 bound is the gradient's own
    tol = tol_of(dtype, "e2e_params", preset, m, chains(case, dtype)[1])
    assert ep <= tol and et <= tol, (ep, et, tol)
    assert set(agent.stats_dict()) == set(R.STATS)


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_captured_plan_equals_eager(dtype, refs):
    case = CASES[4]
    d = refs(case, dtype)["d"]
    m = unpack(case, dtype)[1]
    outs = []
    for captured in (False, True):
        agent, mem = make_agent(case, dtype, d, policy_delay=2)
        plan = agent.plan(mem, 2, m)
        if captured:
            g = plan.capture()
            assert int(mem.head[3]) == int(d["ring"].head[3]) and agent.step_count.cpu().tolist() == [0, 0, 0, 0]      # nothing ran
            g.replay()
            g.replay()
        else:
            plan.run().run()
        torch.cuda.synchronize()
        outs.append([x.clone() for x in (agent.params, agent.target, agent.state, mem.buf, plan.idx, plan.grad)])
    assert all(a.view(torch.uint8).equal(b.view(torch.uint8)) for a, b in zip(*outs))
    assert outs[0][2].view(torch.uint8).any() and int(mem.head[3]) == int(d["ring"].head[3]) + 4
