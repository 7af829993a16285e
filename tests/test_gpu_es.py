"""The evolution-strategies learner on the device (beacon_amd.ES, libbeacon_es.so) against tests/es_ref.py -- NumPy float64 on the CPU, the
stream through tests/noise_ref.py -- on the MI355X.

The data seeds of the act cases (CASES, the `seed` column) were found on the CPU with es_ref: for them every top-two gap of the
float64 reference's head exceeds 100 tolerances on every row, so the device must take the reference's first maximum.

How errors are measured (as in tests/test_gpu_dqn.py): err(q) = max |device - reference| / max(1, max |reference|) for a quantity q.
The reference gets the device's inputs (theta or pop and the rows as the device holds them, cast to float64), so the error is the
kernels' arithmetic alone.

float64: f64_tol(m, chain) = (m + max(640, chain)) x 2^-53 x 500 of tests/test_gpu_learner.py with the chain obs_dim + sum(hidden); for
the gradient the pair count is added to the chain.
float32: the project's rule -- every tolerance in F32_TOL is at most 10 x the error measured on the MI355X for that case, and at most
10 x what es_ref with float32 arithmetic on the CPU (another summation order) shows against float64 on the same case; the three
numbers stand next to each other there.  Every comparison prints its two errors before it asserts ("ES_ERR key case device cpu")."""
import types

import numpy as np
import pytest
import torch

import es_ref as R
from beacon_amd import ES  # noqa: F401  (the class under test: importing it touches neither a compiler nor the GPU)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U64 = 2.0 ** -53
SEED = 0x1234567887654321
DTYPES = [torch.float32, torch.float64]


def f64_tol(m, chain=640):
    return (m + max(640, chain)) * U64 * 500.0


# float32: quantity -> case -> (tolerance, the error measured on the MI355X, the error of es_ref in float32 arithmetic on the CPU on the
# same case).  Every tolerance is at most 10 x either number (rounded down to two digits).
F32_TOL = {
    "pop": {
        "gen0": (8.8e-08, 9.684e-09, 8.811e-09),
        "gen1": (8.4e-08, 8.407e-09, 9.456e-09),
    },
    "act": {
        "m2r1": (6.5e-07, 6.588e-08, 1.124e-07),
        "m6r3": (1.2e-06, 3.930e-07, 1.294e-07),
        "m130r1": (1.6e-06, 1.827e-07, 1.679e-07),
        "m2r70": (2.0e-06, 2.059e-07, 2.443e-07),
        "walk": (1.5e-06, 1.504e-07, 2.204e-07),
        "k130": (6.4e-06, 7.433e-07, 6.475e-07),
        "wide": (4.5e-05, 8.715e-06, 4.503e-06),
    },
    # test_update: the worst of its three generations
    "grad": {
        "ties": (6.6e-07, 8.407e-08, 6.613e-08),
        "chunks": (2.2e-07, 5.136e-08, 2.239e-08),
    },
    "stats": {
        "ties": (3.9e-08, 3.411e-08, 3.954e-09),
        "chunks": (7.8e-09, 1.006e-09, 7.888e-10),
    },
    "theta": {
        "ties": (4.0e-07, 4.061e-08, 4.061e-08),
        "chunks": (5.7e-07, 5.731e-08, 5.731e-08),
    },
}

# (name, M, R, obs_dim, hidden, n_out, activation, group, data seed)
#   m2r1     the smallest population
#   m6r3     a member boundary inside a tile; two members per workgroup, so the second workgroup's group is the last, whole one
#   m130r1   more members than a tile has rows; eight per workgroup, the last group partial (130 = 16 x 8 + 2); act_dim 1
#   m2r70    a member across three tiles, each tile on a workgroup of its own; the last tile partial (70 = 32 + 32 + 6)
#   walk     a member across 513 tiles on 512 workgroups: workgroup 0 walks a second tile; n = 2
#   k130     obs_dim 130: three (float32) / five (float64) K-slabs, the last of two columns, and no multiple of 4 (the scalar staging);
#            odd widths; 16 outputs
#   wide     3 x 128 at obs_dim 512: the 16-byte staging over eight / sixteen slabs, hidden slabs read from the activations; 16 outputs
CASES = [("m2r1", 2, 1, 6, (8,), 2, "tanh", 0, 1),
         ("m6r3", 6, 3, 7, (9, 6), 3, "relu", 2, 1),
         ("m130r1", 130, 1, 5, (16,), 1, "tanh", 8, 1),
         ("m2r70", 2, 70, 12, (20, 12), 3, "tanh", 0, 1),
         ("walk", 2, 513 * 32, 3, (4,), 2, "relu", 0, 1),
         ("k130", 4, 2, 130, (5, 7), 16, "relu", 0, 2),
         ("wide", 2, 3, 512, (128, 128, 128), 16, "tanh", 0, 3)]
IDS = [c[0] for c in CASES]


def tag(dtype):
    return "f64" if dtype == torch.float64 else "f32"


def npdt(dtype):
    return np.float64 if dtype == torch.float64 else np.float32


def err(dev, ref):
    ref = torch.as_tensor(np.asarray(ref)).double().reshape(-1)
    if ref.numel() == 0:
        return 0.0
    return float((torch.as_tensor(np.asarray(dev) if not torch.is_tensor(dev) else dev).double().cpu().reshape(-1) - ref).abs().max() / max(1.0, float(ref.abs().max())))


def check(key, sub, dtype, dev, ref64, ref32, m, chain):
    """the device's error against the float64 reference, printed next to the float32 reference's, then the assertion"""
    e = err(dev, ref64)
    c = err(ref32, ref64) if ref32 is not None else 0.0
    tol = f64_tol(m, chain) if dtype == torch.float64 else F32_TOL[key][sub][0]
    print("ES_ERR %s %s %s device %.3e cpu_f32 %.3e tol %.3e" % (key, sub, tag(dtype), e, c, tol))
    assert e <= tol, (key, sub, tag(dtype), e, tol)
    return tol


class _Env(object):
    """what ES reads of an env: most tests need no solver behind the observation rows"""
    _norm_on = False

    def __init__(self, batch, obs_dim, dtype, kind, n_out, low=-1.0, high=1.0):
        self.batch, self.obs_dim, self.tdtype, self.device = batch, obs_dim, dtype, torch.device(DEV)
        self.action_is_int = kind == 1
        self.action_space = types.SimpleNamespace(n=n_out) if kind == 1 else types.SimpleNamespace(low=np.full(n_out, low), high=np.full(n_out, high))
        self.obs = None


def pairs_of(w, n_layers):
    return [(w["pi_w%d" % l], w["pi_b%d" % l]) for l in range(n_layers)]


def layouts(agent):
    """(the float64 reference's layout, the float32-arithmetic one or None) for the agent's dtype"""
    nd = npdt(agent.tdtype)
    lay = R.Layout(agent.obs_dim, agent.hidden, agent.n_out, nd)
    return lay, (R.Layout(agent.obs_dim, agent.hidden, agent.n_out, nd, np.float32) if nd == np.float32 else None)


def host(t):
    return t.detach().cpu().numpy()


def case_data(case, dtype):
    """the weights of theta, the observation rows (as the device holds them, in float64) of a case"""
    name, M, Rr, od, hidden, n_out, activation, group, seed = case
    w = R.random_weights(od, hidden, n_out, 100 + seed, scale=1.5)
    rng = np.random.default_rng(200 + seed)
    if name == "walk":      # 37 distinct rows, a period coprime to the tile: every row's place is checked, and 2 x 37 margins hold, not 32 832
        obs = rng.standard_normal((37, od))[np.arange(M * Rr) % 37].astype(npdt(dtype))
    else:
        obs = rng.standard_normal((M * Rr, od)).astype(npdt(dtype))
    return w, obs


def case_agent(case, dtype, kind, sigma=0.3):
    name, M, Rr, od, hidden, n_out, activation, group, seed = case
    w, obs = case_data(case, dtype)
    agent = ES(_Env(M * Rr, od, dtype, kind, n_out, -0.5, 1.5), members=M, hidden=hidden, activation=activation, sigma=sigma, seed=SEED, group=group)
    agent.load(pairs_of(w, len(hidden) + 1))
    return agent, torch.as_tensor(obs, device=DEV)


# ---- begin -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_begin(dtype):
    M, Rr, od, hidden, n_out = 6, 2, 5, (5, 7), 3
    nd = npdt(dtype)
    agent = ES(_Env(M * Rr, od, dtype, 0, n_out), members=M, hidden=hidden, sigma=0.1, seed=SEED)
    agent.load(pairs_of(R.random_weights(od, hidden, n_out, 3), 3))
    lay, lay32 = layouts(agent)
    assert lay.E == agent.n_elems and lay.used.sum() < lay.E
    flat = agent.theta.view(dtype)
    flat[torch.as_tensor(~lay.used, device=DEV)] = 7.0                  # the gaps of theta: written as theta's
    flat[lay.offsets["pi_b0"]] = -0.0
    theta = host(flat).astype(np.float64)
    eps = float(np.finfo(nd).eps)
    for gen in (0, 1):
        agent.gen[0] = gen
        agent.fit.fill_(3.0), agent.len.fill_(9), agent.alive.fill_(0)
        agent.begin()
        torch.cuda.synchronize()
        pop = host(agent.pop).astype(np.float64)
        ref32 = R.perturb(theta, 0.1, SEED, gen, M, lay32) if lay32 else None
        check("pop", "gen%d" % gen, dtype, pop, R.perturb(theta, 0.1, SEED, gen, M, lay), ref32, 1, od + sum(hidden))
        # antithetic within one rounding of each member and one of the sum; the gaps are theta's
        bound = 2.0 * eps * np.maximum(np.maximum(np.abs(pop[0::2]), np.abs(pop[1::2])), np.abs(theta))
        assert (np.abs(pop[0::2] + pop[1::2] - 2.0 * theta) <= bound).all()
        assert np.array_equal(pop[:, ~lay.used], np.full((M, int((~lay.used).sum())), 7.0)) and (pop[0, lay.used] != theta[lay.used]).mean() > 0.9
        assert not bool(agent.fit.any()) and not bool(agent.len.any()) and bool((agent.alive == 1).all())
        if gen == 0:
            first = pop
    assert (first[:, lay.used] != pop[:, lay.used]).mean() > 0.99            # a second generation differs from the first
    assert (first[0, lay.used] != first[2, lay.used]).mean() > 0.99          # and a pair from its neighbour
    # sigma = 0: every member IS theta, bit for bit (the -0.0 too)
    agent.set_hyper(sigma=0.0)
    agent.begin()
    torch.cuda.synchronize()
    assert all(torch.equal(agent.pop[p].view(torch.uint8), agent.theta) for p in range(M))
    assert int(agent.gen[0]) == 1                                           # begin does not tick


# ---- act, bit for bit against existing code ------------------------------------------------------------------------------------
SHAPES = [("small", 70, 1, 11, (24, 17), 3, "tanh"), ("wide", 2, 35, 496, (128, 128, 128), 16, "relu")]


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_act_equals_td3_and_dqn_bit_for_bit(shape, dtype):
    from beacon_amd import DQN, TD3
    name, M, Rr, od, hidden, n, activation = shape
    B, nl = M * Rr, len(hidden) + 1
    w = R.random_weights(od, hidden, n, 7, scale=1.5)
    obs = torch.as_tensor(np.random.default_rng(8).standard_normal((B, od)).astype(npdt(dtype)), device=DEV)
    # Box
    td3 = TD3(_Env(B, od, dtype, 0, n, -0.5, 1.5), hidden=hidden, activation=activation, seed=1)
    dq = [od + n] + list(hidden) + [1]
    zq = [(np.zeros((dq[l + 1], dq[l])), np.zeros(dq[l + 1])) for l in range(nl)]
    td3.load(pairs_of(w, nl), zq, zq)
    want = td3.act(obs, mode="deterministic").clone()
    agent = ES(_Env(B, od, dtype, 0, n, -0.5, 1.5), members=M, hidden=hidden, activation=activation, sigma=0.0)
    agent.load(pairs_of(w, nl)).begin()
    assert torch.equal(agent.act(obs), want) and bool(want.abs().sum() > 0)
    agent.actions.zero_()
    agent.pop.fill_(float("nan"))                                          # the shared form reads theta alone
    assert torch.equal(agent.act(obs, shared=True), want)
    # Discrete
    dqn = DQN(_Env(B, od, dtype, 1, n), hidden=hidden, activation=activation, dueling=False, seed=1)
    dqn.load(pairs_of(w, nl))
    want = dqn.act(obs, mode="greedy").clone()
    agent = ES(_Env(B, od, dtype, 1, n), members=M, hidden=hidden, activation=activation, sigma=0.0)
    agent.load(pairs_of(w, nl)).begin()
    assert torch.equal(agent.act(obs), want) and len(torch.unique(want)) > 1 and want.dtype == torch.int32
    agent.actions.fill_(-1)
    agent.pop.fill_(float("nan"))
    assert torch.equal(agent.act(obs, shared=True), want)


# ---- act, per member -----------------------------------------------------------------------------------------------------------
def case_reference(case, dtype, pop, obs):
    """the float64 reference's heads and Box actions for a case's population, and the float32-arithmetic Box actions (or None)"""
    name, M, Rr, od, hidden, n_out, activation, group, seed = case
    nd = npdt(dtype)
    lay = R.Layout(od, hidden, n_out, nd)
    rows = R.member_rows(pop, Rr)
    h, _ = R.heads(rows, obs, lay, activation)
    a = R.act(rows, obs, lay, activation, 0, -0.5, 1.5)
    a32 = R.act(rows, obs, R.Layout(od, hidden, n_out, nd, np.float32), activation, 0, -0.5, 1.5) if nd == np.float32 else None
    return h, a, a32


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_act_per_member(case, dtype):
    name, M, Rr, od, hidden, n_out, activation, group, seed = case
    agent, obs = case_agent(case, dtype, 0)
    agent.begin()
    assert agent.group == (group or 1)
    torch.cuda.synchronize()
    pop = host(agent.pop).astype(np.float64)
    assert (pop[0] != pop[1]).any()
    h, a, a32 = case_reference(case, dtype, pop, host(obs).astype(np.float64))
    act = agent.act(obs)
    torch.cuda.synchronize()
    tol = check("act", name, dtype, act, a, a32, 1, od + sum(hidden))
    assert a.min() >= -0.5 and a.max() <= 1.5 and a.std() > 0.05
    # the members differ: under theta itself the actions are others
    assert err(agent.act(obs, shared=True), a) > 1e-3
    if n_out < 2:
        return
    # Discrete with the same network: the reference's first maximum, whose margin the data seed guarantees
    assert (R.top_two_gap(h) > 100 * tol * max(1.0, float(np.abs(h).max()))).all(), float(R.top_two_gap(h).min())
    disc, _ = case_agent(case, dtype, 1)
    disc.pop.copy_(agent.pop)
    got = disc.act(obs)
    torch.cuda.synchronize()
    want = R.first_argmax(h)
    assert np.array_equal(host(got), want) and got.dtype == torch.int32 and (len(np.unique(want)) > 1 or M * Rr < 4)


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_act_mask_keeps_skipped_rows(dtype):
    case = CASES[1]
    M, Rr = case[1], case[2]
    for kind, sentinel in ((0, 77.0), (1, -5)):
        agent, obs = case_agent(case, dtype, kind)
        agent.begin()
        full = agent.act(obs).clone()
        mask = torch.as_tensor(np.random.default_rng(4).uniform(size=M * Rr) < 0.5, device=DEV)
        assert 0 < int(mask.sum()) < M * Rr
        agent.actions.fill_(sentinel)
        got = agent.act(obs, mask=mask)
        torch.cuda.synchronize()
        assert torch.equal(got[mask], full[mask]) and bool((got[~mask] == sentinel).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_grouping_does_not_matter(dtype):
    """the same population rows with R = 1 and with R = 3 on repeated observations, one and several members per workgroup, and a
    member across tiles: equal actions bit for bit"""
    M, od, hidden, n_out = 6, 7, (9, 6), 3
    w = R.random_weights(od, hidden, n_out, 5, scale=1.5)
    obs1 = torch.as_tensor(np.random.default_rng(9).standard_normal((M, od)).astype(npdt(dtype)), device=DEV)
    outs = []
    for Rr, group in ((1, 0), (1, 4), (3, 0), (3, 2), (40, 0)):
        agent = ES(_Env(M * Rr, od, dtype, 0, n_out), members=M, hidden=hidden, activation="relu", sigma=0.3, seed=SEED, group=group)
        agent.load(pairs_of(w, 3)).begin()
        assert agent.group == (group or 1)
        a = agent.act(obs1.repeat_interleave(Rr, dim=0).contiguous())
        torch.cuda.synchronize()
        a = a.view(M, Rr, n_out)
        assert all(torch.equal(a[:, r], a[:, 0]) for r in range(Rr))
        outs.append((a[:, 0].clone(), agent.pop.clone()))
    assert all(torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]) for o in outs[1:])
    assert len(torch.unique(outs[0][0])) > M


# ---- observe -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_observe_fabricated(dtype):
    B, M, T = 6, 2, 4
    nd = npdt(dtype)
    rng = np.random.default_rng(11)
    rwd = rng.standard_normal((T, B)).astype(nd) * 3.0
    rwd[1, 2], rwd[2, 4] = np.nan, np.nan                                   # replica 2 is alive at step 1, replica 4 is done by step 2
    done, trunc = np.zeros((T, B), np.uint8), np.zeros((T, B), np.uint8)
    done[0, 0] = 1                                                         # finishes at step 1: one reward
    trunc[1, 4] = 1
    done[2, 3], trunc[2, 3] = 1, 1
    done[3, 0] = 1                                                         # a later episode's end: nothing
    agent = ES(_Env(B, 3, dtype, 0, 2), members=M, hidden=(4,))
    agent.begin()
    fit, ln, alive = np.zeros(B), np.zeros(B, np.int32), np.ones(B, np.uint8)
    for t in range(T):
        args = [torch.as_tensor(x[t], device=DEV) for x in (rwd, done, trunc)]
        if t % 2:
            args[1], args[2] = args[1].bool(), args[2].bool()
        agent.observe(*args)
        R.observe(fit, ln, alive, rwd[t], done[t], trunc[t])
    torch.cuda.synchronize()
    assert np.array_equal(host(agent.fit), fit, equal_nan=True) and np.isnan(fit[2]) and not np.isnan(fit[4])
    assert host(agent.len).tolist() == ln.tolist() == [1, 4, 4, 3, 2, 4] and host(agent.alive).tolist() == alive.tolist() == [0, 1, 1, 0, 0, 1]
    assert fit[0] == float(rwd[0, 0]) and fit[4] == float(rwd[0, 4]) + float(rwd[1, 4])


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("cls", ["VecLorenz", "VecBurgers"])
def test_observe_from_an_env(cls, dtype):
    from beacon_amd import vec as V
    B, M, T = 8, 4, 4
    env = getattr(V, cls)(B, DEV, dtype)
    agent = ES(env, members=M, hidden=(7,), sigma=0.2, seed=3)
    agent.load(pairs_of(R.random_weights(agent.obs_dim, (7,), agent.n_out, 2), 2))
    env.reset()
    agent.begin()
    steps = []
    for _ in range(T):
        env.step_autoreset(agent.act())
        agent.observe()
        steps.append([x.clone() for x in (env.rwd, env.done, env.trunc)])
    torch.cuda.synchronize()
    env.check_status()
    fit, ln, alive = np.zeros(B), np.zeros(B, np.int32), np.ones(B, np.uint8)
    for rwd, done, trunc in steps:
        R.observe(fit, ln, alive, host(rwd), host(done), host(trunc))
    print("ES_FIT %s %s" % (cls, fit.tolist()))
    assert np.isfinite(fit).all()
    assert np.array_equal(host(agent.fit), fit)
    assert host(agent.len).tolist() == ln.tolist() and host(agent.alive).tolist() == alive.tolist() and ln.max() == T
    env.close()


# ---- update --------------------------------------------------------------------------------------------------------------------
# (name, M, R, the fitness of three generations as a function of the rng)
def _fit_ties(rng, M, Rr):
    f = rng.permutation(M * Rr).astype(np.float64).reshape(M, Rr) * 0.5 - 1.0          # well separated
    f[3] = f[1]                                                            # a tie across members
    f[4, 1] = np.nan                                                       # one NaN member
    return f.reshape(-1)


def _fit_chunks(rng, M, Rr):
    return rng.permutation(M * Rr).astype(np.float64) * 0.25 - 3.0


UPDATES = [("ties", 6, 2, _fit_ties, dict(weight_decay=0.01, max_grad_norm=0.5)),
           ("chunks", 2 * (R.PAIR_CHUNK + 1), 1, _fit_chunks, dict(weight_decay=0.0, max_grad_norm=None))]


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("case", UPDATES, ids=[u[0] for u in UPDATES])
def test_update(case, dtype):
    name, M, Rr, make_fit, hyper = case
    od, hidden, n_out, sigma, lr = 5, (5, 3), 2, 0.1, 0.05
    nd = npdt(dtype)
    agent = ES(_Env(M * Rr, od, dtype, 0, n_out), members=M, hidden=hidden, sigma=sigma, lr=lr, seed=SEED, **hyper)
    agent.load(pairs_of(R.random_weights(od, hidden, n_out, 3), 3))
    lay, lay32 = layouts(agent)
    assert lay.used.sum() < lay.E
    theta0 = host(agent.theta.view(dtype)).astype(np.float64)
    mk = lambda l: R.Ref(l, "tanh", 0, M, theta0, SEED, sigma, lr, weight_decay=hyper["weight_decay"], max_grad_norm=hyper["max_grad_norm"] or 0.0)
    ref, ref32 = mk(lay), (mk(lay32) if lay32 else None)
    rng = np.random.default_rng(21)
    chain, pairs = od + sum(hidden), M // 2
    worst = {"grad": (0, None, None), "stats": (0, None, None)}
    for gen in range(3):
        fit = make_fit(rng, M, Rr)
        agent.begin()
        agent.fit.copy_(torch.as_tensor(fit))
        agent.update()
        torch.cuda.synchronize()
        F, util, grad, st = ref.update(fit)
        r32 = ref32.update(fit) if ref32 else None
        assert np.array_equal(host(agent.member_fit), F) and np.array_equal(host(agent.util), util) and abs(util.sum()) < 1e-12
        if name == "ties":
            assert F[4] == -np.inf and util[3] > util[1] and util[3] - util[1] == pytest.approx(1.0 / (M - 1)) and st["nan_members"] == 1
            assert st["grad_norm"] > hyper["max_grad_norm"]                # the clip acts
        g = host(agent.grad)
        assert not g[~lay.used].any() and np.abs(g[lay.used]).min() > 0
        check("grad", name, dtype, g, grad, r32[2] if r32 else None, 1, chain + pairs)
        dev_stats = host(agent.stats)
        want = np.array([st[k] for k in R.STATS])
        assert dev_stats[4] == want[4] and dev_stats[5] == want[5] and dev_stats[7] == 0.0
        check("stats", name, dtype, dev_stats, want, np.array([r32[3][k] for k in R.STATS]) if r32 else None, M, chain + pairs)
        assert host(agent.gen).tolist() == [gen + 1, gen + 1, 0, 0]
        assert agent.stats_dict()["generation"] == gen + 1 and agent.stats_dict()["fit_max"] == dev_stats[3]
    check("theta", name, dtype, host(agent.theta.view(dtype)), ref.theta, ref32.theta if ref32 else None, 3, chain + pairs)
    assert np.abs(ref.theta - theta0)[lay.used].min() > 0 and np.array_equal(host(agent.theta.view(dtype))[~lay.used], theta0[~lay.used])
    best = agent.best()
    assert torch.equal(best["pi_w0"], agent.member(int(dev_stats[4]))["pi_w0"]) and best["pi_w0"].data_ptr() != agent.member(int(dev_stats[4]))["pi_w0"].data_ptr()


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def learning_agent(dtype):
    L = R.LEARN
    lay, theta0, obs, target = R.learning_setup(npdt(dtype))
    agent = ES(_Env(L["members"], L["obs_dim"], dtype, 0, L["act_dim"], L["low"], L["high"]), hidden=L["hidden"], sigma=L["sigma"], lr=L["lr"], seed=L["seed"])
    w = lay.unpack(theta0)
    agent.load(pairs_of(w, 2))
    return agent, torch.as_tensor(obs.astype(npdt(dtype)), device=DEV), torch.as_tensor(target, device=DEV)


def device_generation(agent, obs, target, rwd, ones, zeros):
    """one generation with the fitness -|a - a*|^2 computed by torch ops from agent.actions and fed through observe"""
    agent.begin()
    a = agent.act(obs)
    rwd.copy_(-((a.double() - target) ** 2).sum(dim=1))
    agent.observe(rwd, ones, zeros)
    agent.update()


def flags(B):
    return torch.ones(B, dtype=torch.uint8, device=DEV), torch.zeros(B, dtype=torch.uint8, device=DEV)


def test_end_to_end_float64():
    dtype = torch.float64
    agent, obs, target = learning_agent(dtype)
    ref, obs_h, target_h = R.learning_ref()
    M = ref.M
    tol = f64_tol(M, ref.lay.obs_dim + sum(ref.lay.hidden) + M // 2)
    rwd = torch.zeros(M, dtype=dtype, device=DEV)
    ones, zeros = flags(M)
    for gen in range(3):
        ref.begin()
        fit = R.learning_fitness(ref.act(obs_h), target_h)
        s = np.sort(fit)
        # a condition on the reference: neighbouring member fitnesses further apart than 100 tolerances, so the device ranks as it does
        assert (np.diff(s) > 100 * tol * max(1.0, float(np.abs(s).max()))).all(), float(np.diff(s).min())
        ref.update(fit)
        device_generation(agent, obs, target, rwd, ones, zeros)
        torch.cuda.synchronize()
        e = err(agent.theta.view(dtype), ref.theta)
        print("ES_ERR e2e gen%d f64 device %.3e tol %.3e" % (gen, e, tol))
        assert e <= tol and np.array_equal(np.argsort(host(agent.member_fit)), np.argsort(fit))
    assert host(agent.gen).tolist() == [3, 3, 0, 0]


def test_end_to_end_float32_learns():
    """Ranks may flip among near-ties in float32, so nothing is compared element-wise: after 20 generations the fitness of theta has
    improved by at least half of what the float64 reference improves (the half: the margin for rank flips, which ES tolerates)"""
    dtype = torch.float32
    ref, obs_h, target_h = R.learning_ref()
    of_ref = lambda: float(R.learning_fitness(ref.act(obs_h, shared=True), target_h).mean())
    r0 = of_ref()
    for _ in range(20):
        ref.begin()
        ref.update(R.learning_fitness(ref.act(obs_h), target_h))
    r1 = of_ref()
    agent, obs, target = learning_agent(dtype)
    M = ref.M
    rwd = torch.zeros(M, dtype=dtype, device=DEV)
    ones, zeros = flags(M)
    of_dev = lambda: float(-((agent.act(obs, shared=True).double() - target) ** 2).sum(dim=1).mean())
    d0 = of_dev()
    for _ in range(20):
        device_generation(agent, obs, target, rwd, ones, zeros)
    d1 = of_dev()
    print("ES_LEARN reference %.4f -> %.4f, device f32 %.4f -> %.4f" % (r0, r1, d0, d1))
    assert r1 - r0 > 0.3 and abs(d0 - r0) < 1e-5
    assert d1 - d0 >= 0.5 * (r1 - r0)


# ---- graph ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_captured_generation_equals_eager(dtype):
    outs = []
    for captured in (False, True):
        agent, obs, target = learning_agent(dtype)
        M = agent.members
        rwd = torch.zeros(M, dtype=dtype, device=DEV)
        ones, zeros = flags(M)
        if captured:
            agent._stream()
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(g):
                device_generation(agent, obs, target, rwd, ones, zeros)
            assert host(agent.gen).tolist() == [0, 0, 0, 0] and not bool(agent.pop.any())           # nothing ran
            g.replay()
            g.replay()
        else:
            device_generation(agent, obs, target, rwd, ones, zeros)
            device_generation(agent, obs, target, rwd, ones, zeros)
        torch.cuda.synchronize()
        outs.append([x.clone() for x in (agent.theta, agent.pop, agent.state, agent.grad, agent.actions, rwd)])
    assert all(a.view(torch.uint8).equal(b.view(torch.uint8)) for a, b in zip(*outs))
    assert host(agent.gen).tolist() == [2, 2, 0, 0] and bool(outs[0][1].any())
