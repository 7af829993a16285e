"""The DQN learner on the device (beacon_amd.DQN, libbeacon_dqn.so, over beacon_amd.Replay) against tests/dqn_ref.py -- torch autograd in
float64 on the CPU, the first-maximum rule, stream 10 and the append of int32 actions in NumPy -- on the MI355X.

How errors are measured (as in tests/test_gpu_td3.py): err(q) = max |device - reference| / max(1, max |reference|) for a quantity q -- a
gradient segment, a statistic, a parameter segment.  The reference gets the device's inputs (weights and rows as the device holds
them, cast to float64) and the host restatement's indices, so the error is the kernels' arithmetic alone.

A condition on the inputs: every max taken (the online argmax of double Q-learning, the target's max, max_j Q_j(s) of the q_max_mean
statistic), the Huber kink at |delta| = kappa and relu are not smooth, and the device must take the reference's branch on every live
row.  check_margins asserts on the float64 REFERENCE alone that the top-two gap of every max taken, ||delta| - kappa| and every relu
pre-activation exceed 100 x the case's tolerance, over every live row: no case skips rows.  The `kinks` case has two bit-identical
head rows (1 and 2) in both networks, so that its maxima tie EXACTLY on the rows where those win and the first-maximum rule decides
y; its gaps are taken with the duplicate removed, and that the tie decides on live rows is asserted too.  The data seeds in the case
table were found on the CPU with dqn_ref for which that holds.

float64: f64_tol(m, chain) = (m + max(640, chain)) x 2^-53 x 500, the summation-order bound of tests/test_gpu_learner.py, with the chain
of the one network, obs_dim + sum(hidden).
float32: the project's rule -- every tolerance in F32_TOL is at most 10 x the error measured on the MI355X for that case, and at most
10 x what dqn_ref in float32 on the CPU (another summation order) shows against float64 on the same case; the three numbers stand
next to each other there."""
import types

import numpy as np
import pytest
import torch

import dqn_ref as R
from beacon_amd import DQN  # noqa: F401  (the class under test: importing it touches neither a compiler nor the GPU)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U64 = 2.0 ** -53
SEED = 0x1234567887654321
GAMMA = 0.9
DTYPES = [torch.float32, torch.float64]


def f64_tol(m, chain=640):
    return (m + max(640, chain)) * U64 * 500.0


# float32: quantity -> "case flags" -> (tolerance, the error measured on the MI355X, the error of dqn_ref in float32 on the CPU on the same
# case).  Every tolerance is at most 10 x either number (rounded down to two digits).
F32_TOL = {
    "q_values": {
        "act-plain": (1.1e-06, 1.111e-07, 1.580e-07),
        "act-dueling": (1.8e-06, 1.868e-07, 2.612e-07),
    },
    "grad": {
        "one double-huber": (2.8e-07, 2.823e-08, 3.551e-08),
        "one plain-mse": (1.0e-06, 1.043e-07, 1.043e-07),
        "one double-dueling-mse": (6.7e-07, 9.857e-08, 6.761e-08),
        "one plain-dueling-huber": (5.0e-07, 5.040e-08, 5.040e-08),
        "straddle double-huber": (7.1e-07, 7.122e-08, 8.926e-08),
        "straddle plain-mse": (2.7e-06, 2.794e-07, 2.885e-07),
        "straddle double-dueling-mse": (2.5e-06, 2.612e-07, 2.560e-07),
        "straddle plain-dueling-huber": (2.3e-06, 2.354e-07, 2.984e-07),
        "wide16 double-huber": (5.3e-07, 7.418e-08, 5.354e-08),
        "wide16 plain-mse": (9.9e-07, 1.668e-07, 9.953e-08),
        "wide15d double-dueling-huber": (1.3e-06, 2.199e-07, 1.340e-07),
        "wide15d plain-dueling-mse": (3.0e-06, 3.282e-07, 3.073e-07),
        "tiles double-huber": (4.6e-08, 4.677e-09, 2.778e-07),
        "tiles plain-dueling-mse": (3.3e-07, 3.316e-08, 1.154e-06),
        "kinks double-huber": (2.9e-07, 4.312e-08, 2.967e-08),
        "kinks plain-huber": (2.5e-07, 3.465e-08, 2.524e-08),
        "kinks double-dueling-huber": (3.5e-07, 3.521e-08, 5.952e-08),
        "kinks plain-dueling-huber": (3.4e-07, 3.451e-08, 5.835e-08),
    },
    "stats": {
        "one double-huber": (6.9e-07, 6.956e-08, 1.061e-07),
        "one plain-mse": (4.6e-07, 4.681e-08, 4.681e-08),
        "one double-dueling-mse": (6.8e-07, 8.199e-08, 6.827e-08),
        "one plain-dueling-huber": (6.2e-07, 6.226e-08, 7.946e-08),
        "straddle double-huber": (1.1e-06, 1.190e-07, 1.774e-07),
        "straddle plain-mse": (1.1e-06, 1.190e-07, 1.774e-07),
        "straddle double-dueling-mse": (1.5e-06, 2.028e-07, 1.523e-07),
        "straddle plain-dueling-huber": (1.5e-06, 2.028e-07, 1.523e-07),
        "wide16 double-huber": (6.5e-07, 9.156e-08, 6.578e-08),
        "wide16 plain-mse": (1.3e-06, 1.655e-07, 1.305e-07),
        "wide15d double-dueling-huber": (6.7e-07, 1.422e-07, 6.754e-08),
        "wide15d plain-dueling-mse": (4.7e-07, 8.931e-08, 4.767e-08),
        "tiles double-huber": (2.8e-07, 2.826e-08, 5.184e-08),
        "tiles plain-dueling-mse": (2.9e-07, 2.936e-08, 5.267e-08),
        "kinks double-huber": (2.9e-07, 2.996e-08, 4.369e-08),
        "kinks plain-huber": (1.8e-07, 4.168e-08, 1.834e-08),
        "kinks double-dueling-huber": (3.9e-07, 3.956e-08, 2.074e-07),
        "kinks plain-dueling-huber": (6.6e-07, 6.638e-08, 1.947e-07),
    },
    "adam_params": {
        "kinks": (6.4e-07, 6.402e-08, 6.402e-08),
    },
    "e2e_params": {
        "double": (7.6e-07, 1.052e-07, 7.684e-08),
        "plain": (1.3e-06, 1.315e-07, 1.315e-07),
        "double-dueling": (1.3e-06, 1.336e-07, 1.336e-07),
        "plain-dueling": (6.8e-07, 6.825e-08, 6.825e-08),
    },
}

# (name, m float32 / float64, obs_dim float32 / float64, n, hidden, activation, options, data seed, flag combinations (double, dueling, huber))
#   one       a single row
#   straddle  two tiles, the second with one row (65 / 33 rows); the first layer crosses a K-slab (obs_dim 70 / 40); relu; dead rows whose
#             fields are NaN, one of them dead by its stored action; one idx entry of -1
#   wide16    3 x 128 under obs_dim 512 with 16 plain head rows: the LDS limit, the two-pass register tile at every layer; m = TB; rows with
#             boot = 0
#   wide15d   the same with n = 15 and the dueling head's value row as the 16th
#   tiles     more tiles than the backward launch's grid (129 > 128: a workgroup walks a second tile) with lorenz's sizes
#   kinks     Huber rows on both sides of kappa; rows 1 and 2 of the head bit-identical in both networks: exact ties in the online argmax
#             (double) and in the target's max, decided by the first-maximum rule; widths that are no multiple of 4
ALL4 = ((True, False, 1.0), (False, False, None), (True, True, None), (False, True, 1.0))
CASES = [("one", (1, 1), (3, 3), 2, (4,), "tanh", {}, 1, ALL4),
         ("straddle", (65, 33), (70, 40), 4, (24, 17), "relu", {"dead": True, "neg_idx": True}, 1, ALL4),
         ("wide16", (64, 32), (512, 512), 16, (128, 128, 128), "tanh", {"boot0": True}, 1, ((True, False, 1.0), (False, False, None))),
         ("wide15d", (64, 32), (512, 512), 15, (128, 128, 128), "tanh", {"boot0": True}, 1, ((True, True, 1.0), (False, True, None))),
         ("tiles", (129 * 64, 129 * 32), (6, 6), 3, (8,), "tanh", {"dead": True}, 1, ((True, False, 1.0), (False, True, None))),
         ("kinks", (65, 33), (5, 5), 4, (33, 5), "tanh", {"tie": True, "dead": True, "boot0": True},  1,
          ((True, False, 0.5), (False, False, 0.5), (True, True, 0.5), (False, True, 0.5)))]
IDS = [c[0] for c in CASES]
KINKS = CASES[5]
REGIME = {"tiles": lambda grid, tiles: grid == 128 and tiles == 129}
KEYS = ("loss", "q_mean", "target_mean", "td_abs_mean", "W", "grad_norm", "q_max_mean", "spare")


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


def flags_id(flags):
    double, dueling, huber = flags
    return "%s%s-%s" % ("double" if double else "plain", "-dueling" if dueling else "", "mse" if huber is None else "huber")


class _Env(object):
    """what DQN reads of an env: most tests need no solver behind the observation rows"""
    _norm_on = False
    action_is_int = True

    def __init__(self, batch, obs_dim, n, dtype):
        self.batch, self.obs_dim, self.tdtype, self.device = batch, obs_dim, dtype, torch.device(DEV)
        self.action_space = types.SimpleNamespace(n=n)
        self.obs = None


def unpack(case, dtype):
    name, ms, ods, n, hidden, activation, opt, seed, combos = case
    k = 1 if dtype == torch.float64 else 0
    return name, ms[k], ods[k], n, hidden, activation, opt, seed


def make_data(case, dtype, dueling):
    """the case's weights, targets, ring and minibatch on the CPU, in the values the device will hold"""
    name, m, od, n, hidden, activation, opt, seed = unpack(case, dtype)
    rng = np.random.default_rng(seed)
    nd = npdt(dtype)
    W = R.random_weights(od, n, hidden, dueling, seed, scale=1.5)
    Wt = R.random_weights(od, n, hidden, dueling, seed + 100, scale=1.5)
    L = len(hidden)
    if opt.get("tie"):                                       # rows 1 and 2 of the head: the same weights and bias, in both networks
        for w in (W, Wt):
            w["q_w%d" % L][2], w["q_b%d" % L][2] = w["q_w%d" % L][1], w["q_b%d" % L][1]
    rnd = lambda d: {k: v.astype(nd).astype(np.float64) for k, v in d.items()}
    W, Wt = rnd(W), rnd(Wt)
    Cn = min(m, 200) + 7
    ring = R.Ring(Cn, od, 1, nd)
    ring.obs[:], ring.next_obs[:] = rng.standard_normal((Cn, od)), rng.standard_normal((Cn, od))
    ring.act[:, 0], ring.rwd[:] = rng.integers(0, n, Cn), rng.standard_normal(Cn)
    ring.boot[:] = (rng.uniform(size=Cn) > 0.3) if opt.get("boot0") else 1
    ring.live[:] = (rng.uniform(size=Cn) > 0.25) if opt.get("dead") else 1
    dead = ring.live == 0
    for a in (ring.obs, ring.next_obs, ring.act, ring.rwd):
        a[dead] = np.nan                                # a dead row may hold anything
    ring.head[:] = (0, Cn, Cn, 5)
    idx = R.sample_idx(m, SEED, Cn, 5)
    if opt.get("dead"):                                 # one sampled live row dead by its stored action alone
        victim = int(idx[np.flatnonzero(ring.live[idx] != 0)[1]])
        ring.act[victim, 0] = n
    if opt.get("neg_idx"):
        idx[3] = -1
    safe = np.clip(idx, 0, Cn - 1)
    batch = ring.gather(safe)
    batch["w"] = batch["w"] * (idx >= 0)
    return dict(W=W, Wt=Wt, ring=ring, idx=idx, batch=batch)


def make_ref(case, dtype, d, dueling, rdtype=torch.float64):
    name, m, od, n, hidden, activation, opt, seed = unpack(case, dtype)
    return R.Ref(od, n, hidden, activation, dueling, d["W"], d["Wt"], dtype=rdtype)


def make_agent(case, dtype, d, flags, batch=4, **kw):
    from beacon_amd import DQN
    name, m, od, n, hidden, activation, opt, seed = unpack(case, dtype)
    double, dueling, huber = flags
    env = _Env(batch, od, n, dtype)
    agent = DQN(env, hidden=hidden, activation=activation, double=double, dueling=dueling, huber=huber, seed=SEED, **dict(dict(gamma=GAMMA), **kw))
    for k in agent.weights:
        agent.weights[k].copy_(torch.as_tensor(d["W"][k]).to(dtype).view(agent.weights[k].shape))
        agent.target_weights[k].copy_(torch.as_tensor(d["Wt"][k]).to(dtype).view(agent.target_weights[k].shape))
    ring = d["ring"]
    mem = agent.replay(ring.C)
    for k in ("obs", "next_obs", "act", "rwd", "boot", "live", "head"):
        getattr(mem, k).copy_(torch.as_tensor(getattr(ring, k)).view(getattr(mem, k).shape))
    return agent, mem


def case_margins(case, dtype, d, ref, out, flags):
    """the module docstring's condition, on the float64 reference's numbers: {name: margin}"""
    name, m, od, n, hidden, activation, opt, seed = unpack(case, dtype)
    double, dueling, huber = flags
    lv = out["live"]
    mg = dict(out["margins"], relu=ref.min_pre)
    if opt.get("tie"):
        # the deliberate exact ties excepted: the gaps with the duplicate of row 1 removed
        z = lambda x: np.where(lv[:, None], np.nan_to_num(x), 0.0)
        for key, rows, target in (("gap_online", d["batch"]["s2"], False), ("gap_target", d["batch"]["s2"], True), ("gap_qmax", d["batch"]["s"], False)):
            if key in mg:
                q = ref.q_values(z(rows), target=target)
                assert np.array_equal(q[:, 1], q[:, 2])
                mg[key] = float(R.top_two_gap(np.delete(q, 2, axis=1))[lv].min())
                if key != "gap_qmax":                        # the tie decides y on live rows: the maximum is the duplicated value
                    assert (out["gaps"][key][lv] == 0.0).any() and (R.first_argmax(q)[lv] == 1).any() and not (R.first_argmax(q) == 2).any()
    return mg


def check_margins(case, dtype, d, ref, out, flags, tol):
    mg = case_margins(case, dtype, d, ref, out, flags)
    print("dqn margins %s %s %s: %s (100 tol = %.3e)" % (case[0], flags_id(flags), tag(dtype), {k: "%.3e" % v for k, v in mg.items()}, 100 * tol))
    assert all(v > 100 * tol for v in mg.values()), (mg, tol)
    assert out["row_term_max"] <= 500.0
    huber, lv = flags[2], out["live"]
    if case[0] == "kinks":
        assert (np.abs(out["delta"][lv]) > huber).any() and (np.abs(out["delta"][lv]) < huber).any()


@pytest.fixture(scope="module")
def refs():
    """(case name, dtype tag, flags) -> the data and the float64 / float32 references' results: computed once, read-only"""
    cache = {}

    def get(case, dtype, flags):
        key = (case[0], tag(dtype), flags)
        if key not in cache:
            double, dueling, huber = flags
            d = make_data(case, dtype, dueling)
            ref = make_ref(case, dtype, d, dueling)
            out = ref.loss(d["batch"], GAMMA, double, huber)
            o32 = make_ref(case, dtype, d, dueling, torch.float32).loss(d["batch"], GAMMA, double, huber) if dtype == torch.float32 else None
            cache[key] = dict(d=d, ref=ref, out=out, o32=o32)
        return cache[key]
    return get


def chain_of(case, dtype):
    name, m, od, n, hidden, activation, opt, seed = unpack(case, dtype)
    return od + sum(hidden)


def stat_err(dev, want, keys=KEYS):
    return max(abs(dev[k] - want[k]) / max(1.0, abs(want[k])) for k in keys)


def report(key, sub, dtype, gpu, cpu32=None):
    """one line per measured error: what F32_TOL's second and third columns are copied from"""
    print("dqn err %s | %s | %s gpu=%.3e cpu32=%s" % (key, sub, tag(dtype), gpu, "-" if cpu32 is None else "%.3e" % cpu32))


# ---- act ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("dueling", [False, True], ids=["plain", "dueling"])
def test_act(dueling, dtype):
    from beacon_amd import DQN
    od, n, hidden, B, off = 11, 4, (33, 5), 130, 2 ** 32 - 3
    nd = npdt(dtype)
    rng = np.random.default_rng(3)
    W = {k: v.astype(nd).astype(np.float64) for k, v in R.random_weights(od, n, hidden, dueling, 17).items()}
    env = _Env(B, od, n, dtype)
    agent = DQN(env, hidden=hidden, activation="relu", dueling=dueling, eps=0.3, seed=SEED, replica_offset=off)
    agent.load([(W["q_w%d" % l], W["q_b%d" % l]) for l in range(len(hidden) + 1)])
    ref = R.Ref(od, n, hidden, "relu", dueling, W)
    obs_np = rng.standard_normal((B, od)).astype(nd)
    obs = torch.as_tensor(obs_np).to(DEV)
    sub = "act-dueling" if dueling else "act-plain"
    # q_values: against the reference, and bit for bit what act() takes its argmax of
    q = agent.q_values(obs)
    assert tuple(q.shape) == (B, n) and q.dtype == dtype
    q_np = q.cpu().numpy().astype(np.float64)
    q_ref = ref.q_values(obs_np.astype(np.float64))
    e_q = err(q, q_ref)
    c32 = err(R.Ref(od, n, hidden, "relu", dueling, W, dtype=torch.float32).q_values(obs_np.astype(np.float64)), q_ref) if dtype == torch.float32 else None
    report("q_values", sub, dtype, e_q, c32)
    assert e_q <= tol_of(dtype, "q_values", sub, 1, od + sum(hidden)), e_q
    out = torch.empty_like(q)
    assert agent.q_values(obs, out=out) is out and torch.equal(out, q)
    # greedy: the first maximum of those values; no tick
    a = agent.act(obs, mode="greedy")
    assert a is agent.actions and a.dtype == torch.int32 and tuple(a.shape) == (B,)
    greedy = R.first_argmax(q_np)
    assert np.array_equal(a.cpu().numpy(), greedy) and not bool(agent.counters.any())
    clear = R.top_two_gap(q_ref) > 100 * tol_of(dtype, "q_values", sub, 1, od + sum(hidden))
    assert clear.sum() > B // 2 and np.array_equal(greedy[clear], R.first_argmax(q_ref)[clear])      # and the reference's where its gap is clear
    # epsilon: the host's draws; counters tick; a float eps and a device tensor are the same launch
    ctr0 = np.arange(B) * 3
    for eps, mode in ((0.3, "epsilon"), (0.0, "epsilon"), (1.0, "epsilon"), (torch.full((1,), 0.3, dtype=dtype, device=DEV), "epsilon"), (0.3, "uniform")):
        agent.set_hyper(eps=eps)
        agent.counters.copy_(torch.as_tensor(ctr0, dtype=torch.int32))
        agent.actions.fill_(-1)
        got = agent.act(obs, mode=mode).cpu().numpy()
        u, rnd = R.act_draws(SEED, off, ctr0, n, nd)
        e = float(np.asarray(0.3 if torch.is_tensor(eps) else eps, dtype=nd))          # eps is rounded once to the env dtype
        want = R.act(q_np, u, rnd, mode, e)
        assert np.array_equal(got, want), (eps, mode)
        assert np.array_equal(agent.counters.cpu().numpy(), ctr0 + 1)
        if mode == "epsilon" and e == 0.0:
            assert np.array_equal(got, greedy)
        if (mode == "epsilon" and e == 1.0) or mode == "uniform":
            assert np.array_equal(got, rnd) and set(got.tolist()) == set(range(n))
        if mode == "epsilon" and 0.0 < e < 1.0:
            assert (got != greedy).any() and (u >= e).any() and (u < e).any()
    # the schedule a caller writes with a tensor op: the launch reads the value of the time it runs
    sched = torch.zeros(1, dtype=dtype, device=DEV)
    agent.set_hyper(eps=sched)
    agent.counters.copy_(torch.as_tensor(ctr0, dtype=torch.int32))
    assert np.array_equal(agent.act(obs, mode="epsilon").cpu().numpy(), greedy)
    sched.fill_(1.0)
    agent.counters.copy_(torch.as_tensor(ctr0, dtype=torch.int32))
    assert np.array_equal(agent.act(obs, mode="epsilon").cpu().numpy(), R.act_draws(SEED, off, ctr0, n, nd)[1])
    # a mask: replicas with 0 keep their action and their counter
    agent.set_hyper(eps=0.3)
    mask = (np.arange(B) % 3 != 0)
    agent.counters.copy_(torch.as_tensor(ctr0, dtype=torch.int32))
    agent.actions.fill_(-7)
    got = agent.act(obs, mask=mask, mode="epsilon").cpu().numpy()
    u, rnd = R.act_draws(SEED, off, ctr0, n, nd)
    assert np.array_equal(got, np.where(mask, R.act(q_np, u, rnd, "epsilon", float(np.asarray(0.3, dtype=nd))), -7))
    assert np.array_equal(agent.counters.cpu().numpy(), ctr0 + mask)


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("dueling", [False, True], ids=["plain", "dueling"])
def test_act_returns_the_lower_index_of_identical_head_rows(dueling, dtype):
    from beacon_amd import DQN
    od, n, hidden, B = 6, 4, (8,), 130
    nd = npdt(dtype)
    W = {k: v.astype(nd).astype(np.float64) for k, v in R.random_weights(od, n, hidden, dueling, 5).items()}
    W["q_w1"][2], W["q_b1"][2] = W["q_w1"][1], W["q_b1"][1]
    W["q_b1"][1:3] += 1.0                                     # and the pair wins often
    agent = DQN(_Env(B, od, n, dtype), hidden=hidden, dueling=dueling, seed=SEED)
    agent.load([(W["q_w%d" % l], W["q_b%d" % l]) for l in range(2)])
    obs = torch.as_tensor(np.random.default_rng(0).standard_normal((B, od)).astype(nd)).to(DEV)
    q = agent.q_values(obs).cpu().numpy()
    assert np.array_equal(q[:, 1], q[:, 2])                   # bit-identical rows give bit-identical values
    a = agent.act(obs, mode="greedy").cpu().numpy()
    assert (a == 1).sum() > B // 4 and not (a == 2).any() and np.array_equal(a, R.first_argmax(q))


# ---- append --------------------------------------------------------------------------------------
def _fake_rollout(rng, T, B, od, nd, n, cursor, bad=()):
    from beacon_amd import _lib as main
    obs, fin = rng.standard_normal((T + 1, B, od)).astype(nd), rng.standard_normal((T, B, od)).astype(nd)
    act = rng.integers(0, n, (T, B)).astype(np.int32)
    for (t, b, v) in bad:
        act[t, b] = v
    rwd = rng.standard_normal((T, B)).astype(nd)
    done, trunc = (rng.uniform(size=(T, B)) < 0.3).astype(np.uint8), (rng.uniform(size=(T, B)) < 0.3).astype(np.uint8)
    valid = (rng.uniform(size=(T, B)) < 0.8).astype(np.uint8)
    host = dict(obs=obs, act=act, rwd=rwd, done=done, trunc=trunc, valid=valid, final_obs=fin, cursor=np.array([cursor, 0, 0, 0], dtype=np.int32))
    ro = types.SimpleNamespace(T=T, batch=B, flags=main.RO_FINAL_OBS, **{k: torch.as_tensor(v).to(DEV) for k, v in host.items()})
    return host, ro


def _ring_equals(mem, ring):
    for k in ("head", "obs", "act", "rwd", "next_obs", "boot", "live"):
        got, want = getattr(mem, k).cpu().numpy(), getattr(ring, k)
        assert got.tobytes() == want.reshape(got.shape).astype(got.dtype).tobytes(), k


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("shape", [(3, 4, 7, (3, 2)), (12, 1, 0, (12, 5))], ids=["T3B4", "T12B1"])
def test_append_wraps_the_ring_byte_for_byte(shape, dtype):
    """C = 12: T B of 12 and then a partial cursor (5 of 12 with B = 1; 2 of 3 steps with B = 4, from a write position of 7)"""
    from beacon_amd import DQN
    T, B, h0, cursors = shape
    od, n, Cn = 3, 3, 12
    nd = npdt(dtype)
    rng = np.random.default_rng(4)
    agent = DQN(_Env(B, od, n, dtype), hidden=(4,), seed=SEED)
    mem = agent.replay(Cn)
    ring = R.Ring(Cn, od, 1, nd)
    ring.head[0] = h0
    mem.head.copy_(torch.as_tensor(ring.head))
    for cursor in cursors:
        host, ro = _fake_rollout(rng, T, B, od, nd, n, cursor, bad=((0, 0, n), (1, 0, -1)))
        assert mem.append(ro) is mem
        R.append_int(ring, host["obs"], host["act"], host["rwd"], host["done"], host["trunc"], host["valid"], host["final_obs"], cursor)
        _ring_equals(mem, ring)
    assert ring.head.tolist() == [(h0 + sum(cursors) * B) % Cn, Cn, sum(cursors) * B, 0]
    assert (ring.act == n).any()
    # an out-of-range stored action is kept as it is and yields a dead row: W counts the others
    mem.live.fill_(1)
    ring.live[:] = 1
    plan = agent.plan(mem, 1, Cn)
    plan.idx.copy_(torch.arange(Cn, dtype=torch.int32))
    plan.grad_step()
    okay = (ring.act[:, 0] >= 0) & (ring.act[:, 0] < n)
    st = agent.stats_dict()
    assert 0 < okay.sum() < Cn and st["W"] == okay.sum() and all(np.isfinite(v) for v in st.values())


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_append_from_lorenz(dtype):
    from beacon_amd import DQN, vec as V
    B, T = 8, 3
    env = V.VecLorenz(B, DEV, dtype)
    agent = DQN(env, hidden=(8,), seed=3)
    nd = np.float64 if dtype == "f64" else np.float32
    mem, ro = agent.replay(2 * T * B + 5), env.rollout(T)
    ring = R.Ring(mem.capacity, agent.obs_dim, 1, nd)
    env.reset()
    env.set_stp(env.n_act - 1 - np.arange(B) % 3)               # episodes end at steps 0, 1, 2 of what follows
    ended = 0
    for it in range(3):
        ro.begin()
        for _ in range(T):
            env.step_autoreset(agent.act(mode="uniform"))
        assert ro.act.dtype == torch.int32 and tuple(ro.act.shape) == (T, B)
        mem.append(ro)
        ended += int((ro.done | ro.trunc).sum())
        h = {k: getattr(ro, k).cpu().numpy() for k in ("obs", "act", "rwd", "done", "trunc", "valid", "final_obs")}
        R.append_int(ring, h["obs"], h["act"], h["rwd"], h["done"], h["trunc"], h["valid"], h["final_obs"], T)
        _ring_equals(mem, ring)
    assert ring.head.tolist()[:3] == [(3 * T * B) % mem.capacity, mem.capacity, 3 * T * B] and set(np.unique(ring.act)) <= {0.0, 1.0, 2.0}
    assert ended >= B                                           # episodes ended inside the rollouts: final_obs rows were taken
    env.close()


# ---- the gradient --------------------------------------------------------------------------------
GRAD_PARAMS = [(c, f) for c in CASES for f in c[8]]


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("case,flags", GRAD_PARAMS, ids=["%s-%s" % (c[0], flags_id(f)) for c, f in GRAD_PARAMS])
def test_gradient_and_stats_match_reference(case, flags, dtype, refs):
    name, m, od, n, hidden, activation, opt, seed = unpack(case, dtype)
    double, dueling, huber = flags
    r = refs(case, dtype, flags)
    d, ref, out = r["d"], r["ref"], r["out"]
    chain = chain_of(case, dtype)
    sub = "%s %s" % (name, flags_id(flags))
    tols = {k: tol_of(dtype, k, sub, m, chain) for k in ("grad", "stats")}
    check_margins(case, dtype, d, ref, out, flags, max(tols.values()))
    lv = out["live"]
    if opt.get("dead"):
        assert 0 < lv.sum() < m and np.isnan(d["ring"].obs).any()
    if opt.get("boot0"):
        assert (d["batch"]["boot"][lv] == 0).any() and (d["batch"]["boot"][lv] == 1).any()
    if opt.get("neg_idx"):
        assert d["idx"][3] == -1 and not lv[3]
    agent, mem = make_agent(case, dtype, d, flags)
    if name.startswith("wide"):
        assert agent.lds_bytes == (158336 if dtype == torch.float64 else 160256) and agent.n_head == 16      # the LDS limit
    plan = agent.plan(mem, 1, m)
    tiles = -(-m // tile_rows(dtype))
    if name in REGIME:
        assert REGIME[name](agent.grid, tiles), (agent.grid, tiles)
    plan.idx.copy_(torch.as_tensor(d["idx"]).to(torch.int32))
    params0, target0 = agent.params.clone(), agent.target.clone()
    plan.grad_step()
    ge = {k: err(plan.grads[k], out["grads"][k]) for k in ref.names}
    st = agent.stats_dict()
    se = stat_err(st, out["stats"])
    assert all(np.isfinite(v) for v in st.values()) and set(st) == set(R.STATS) and st["W"] == out["stats"]["W"] and st["spare"] == 0.0
    assert torch.equal(agent.params, params0) and torch.equal(agent.target, target0)
    assert agent.step_count.cpu().tolist() == [0, 0, 0, 0] and mem.head.cpu().tolist() == d["ring"].head.tolist()
    o32 = r["o32"]
    f32 = o32 is not None
    report("grad", sub, dtype, max(ge.values()), max(err(o32["grads"][k], out["grads"][k]) for k in ref.names) if f32 else None)
    report("stats", sub, dtype, se, stat_err(o32["stats"], out["stats"]) if f32 else None)
    assert max(ge.values()) <= tols["grad"], (ge, tols)
    assert se <= tols["stats"], (se, tols)


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_gradients_are_bit_reproducible(dtype, refs):
    flags = KINKS[8][2]
    d = refs(KINKS, dtype, flags)["d"]
    m = unpack(KINKS, dtype)[1]
    outs = []
    for _ in range(2):
        agent, mem = make_agent(KINKS, dtype, d, flags)
        plan = agent.plan(mem, 2, m)
        plan.run()
        outs.append([x.clone() for x in (plan.grad, agent.stats, agent.params, agent.target, agent.state, mem.buf, plan.idx)])
    assert all(a.view(torch.uint8).equal(b.view(torch.uint8)) for a, b in zip(*outs))


# ---- Adam and Polyak ---------------------------------------------------------------------------
def _adam_reference(dtype, d, flags, rdtype):
    """the three steps of test_adam_and_polyak with dqn_ref's own Adam, in `rdtype`: the float32 yardstick"""
    ref = make_ref(KINKS, dtype, d, flags[1], rdtype)
    for _ in range(3):
        ref.adam(ref.loss(d["batch"], GAMMA, flags[0], flags[2])["grads"], 1e-2)
    return ref


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_adam_and_polyak(dtype, refs):
    flags = KINKS[8][2]
    double, dueling, huber = flags
    name, m, od, n, hidden, activation, opt, seed = unpack(KINKS, dtype)
    d = refs(KINKS, dtype, flags)["d"]
    agent, mem = make_agent(KINKS, dtype, d, flags, lr=1e-2, tau=1.0)
    ref = make_ref(KINKS, dtype, d, dueling)
    plan = agent.plan(mem, 1, m)
    plan.idx.copy_(torch.as_tensor(d["idx"]).to(torch.int32))
    # torch.optim.Adam on the reference's parameters with the reference's gradients
    tp = {k: v.clone().requires_grad_(True) for k, v in ref.W.items()}
    opt_ = torch.optim.Adam([tp[k] for k in ref.names], lr=1e-2, betas=(0.9, 0.999), eps=1e-8)
    worst = 0.0
    target0 = agent.target.clone()
    for step in range(3):
        ref.W = {k: v.detach().clone() for k, v in tp.items()}
        g = ref.loss(d["batch"], GAMMA, double, huber)["grads"]
        before = {k: agent.weights[k].clone() for k in ref.names}
        plan.grad_step().adam()
        for k in ref.names:
            tp[k].grad = g[k].clone()
        opt_.step()
        assert not any(torch.equal(agent.weights[k], before[k]) for k in ref.names)
        assert torch.equal(agent.target, target0)                        # the target is bit-identical until Polyak
        worst = max([worst] + [err(agent.weights[k], tp[k].detach()) for k in ref.names])
        assert agent.step_count.cpu().tolist() == [step + 1, 0, 0, 0]
    c32 = None
    if dtype == torch.float32:
        r64, r32 = (_adam_reference(dtype, d, flags, t) for t in (torch.float64, torch.float32))
        c32 = max(err(r32.W[k], r64.W[k]) for k in ref.names)
    report("adam_params", name, dtype, worst, c32)
    assert worst <= tol_of(dtype, "adam_params", name, m, chain_of(KINKS, dtype)), worst
    # Polyak at tau = 1: the hard copy, bit for bit
    assert not torch.equal(agent.target, agent.params)
    plan.polyak()
    assert torch.equal(agent.target, agent.params)
    # and at tau = 0.25 the formula, from a target that differs
    agent.target.copy_(target0)
    agent.set_hyper(tau=0.25)
    plan.polyak()
    for k in ref.names:
        t0 = torch.as_tensor(d["Wt"][k]).to(dtype).view(agent.shapes[k])
        p = agent.weights[k].cpu()
        assert torch.equal(agent.target_weights[k].cpu(), t0 + torch.tensor(0.25, dtype=dtype) * (p - t0)), k


# ---- end to end ----------------------------------------------------------------------------------
def _run_reference(dtype, d, flags, n_updates, lr, tau, target_every, rdtype=torch.float64):
    name, m, od, n, hidden, activation, opt, seed = unpack(KINKS, dtype)
    ref = make_ref(KINKS, dtype, d, flags[1], rdtype)
    ring = d["ring"]
    head3 = int(ring.head[3])
    for k in range(n_updates):
        idx = R.sample_idx(m, SEED, int(ring.head[1]), head3 + k)
        ref.adam(ref.loss(ring.gather(idx), GAMMA, flags[0], flags[2])["grads"], lr)
        if (k + 1) % target_every == 0:
            ref.polyak(tau)
    return ref


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("flags", KINKS[8], ids=[flags_id(f).rsplit("-", 1)[0] for f in KINKS[8]])
def test_end_to_end_update(flags, dtype, refs):
    name, m, od, n, hidden, activation, opt, seed = unpack(KINKS, dtype)
    preset = flags_id(flags).rsplit("-", 1)[0]
    d = refs(KINKS, dtype, flags)["d"]
    lr, tau = 1e-3, 0.05
    agent, mem = make_agent(KINKS, dtype, d, flags, lr=lr, tau=tau)
    target0 = agent.target.clone()
    assert agent.update(mem, n_updates=1, batch_size=m, target_every=2) is agent and torch.equal(agent.target, target0)      # no target step yet
    agent, mem = make_agent(KINKS, dtype, d, flags, lr=lr, tau=tau)
    assert agent.update(mem, n_updates=6, batch_size=m, target_every=2) is agent
    ref = _run_reference(dtype, d, flags, 6, lr, tau, 2)
    assert agent.step_count.cpu().tolist() == [6, 0, 0, 0] and int(mem.head[3]) == int(d["ring"].head[3]) + 6
    ep = max(err(agent.weights[k], ref.W[k]) for k in ref.names)
    et = max(err(agent.target_weights[k], ref.Wt[k]) for k in ref.names)
    c32 = None
    if dtype == torch.float32:
        r32 = _run_reference(dtype, d, flags, 6, lr, tau, 2, torch.float32)
        c32 = max(err(r32.W[k], ref.W[k]) for k in ref.names)
    report("e2e_params", preset, dtype, max(ep, et), c32)
    # six steps of Adam: a parameter moves by at most lr per step whatever the gradient, and by lr x (relative gradient error) from an
    # error in it; under err()'s floor of 1 the float64 bound is the gradient's own
    tol = tol_of(dtype, "e2e_params", preset, m, chain_of(KINKS, dtype))
    assert ep <= tol and et <= tol, (ep, et, tol)
    st = agent.stats_dict()
    assert set(st) == set(R.STATS) and all(np.isfinite(v) for v in st.values())


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_captured_plan_equals_eager(dtype, refs):
    flags = KINKS[8][2]
    d = refs(KINKS, dtype, flags)["d"]
    m = unpack(KINKS, dtype)[1]
    outs = []
    for captured in (False, True):
        agent, mem = make_agent(KINKS, dtype, d, flags)
        plan = agent.plan(mem, 3, m, target_every=2)
        if captured:
            g = plan.capture()
            assert int(mem.head[3]) == int(d["ring"].head[3]) and agent.step_count.cpu().tolist() == [0, 0, 0, 0]      # nothing ran
            g.replay()
            torch.cuda.synchronize()
            first = plan.idx.clone()
            g.replay()
            torch.cuda.synchronize()
            assert not torch.equal(plan.idx, first)                      # a replay draws new samples
        else:
            plan.run().run()
        torch.cuda.synchronize()
        outs.append([x.clone() for x in (agent.params, agent.target, agent.state, mem.buf, plan.idx, plan.grad)])
    assert all(a.view(torch.uint8).equal(b.view(torch.uint8)) for a, b in zip(*outs))
    assert outs[0][2].view(torch.uint8).any() and int(mem.head[3]) == int(d["ring"].head[3]) + 6


# ---- real envs -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("dueling", [False, True], ids=["plain", "dueling"])
def test_loop_on_lorenz(dueling, dtype):
    from beacon_amd import DQN, vec as V
    B, T = 64, 8
    env = V.VecLorenz(B, DEV, dtype)
    agent = DQN(env, hidden=(8,), dueling=dueling, seed=3)
    w = R.random_weights(agent.obs_dim, agent.n_actions, (8,), dueling, 1)
    agent.load([(w["q_w%d" % l], w["q_b%d" % l]) for l in range(2)])
    mem, ro = agent.replay(2 * T * B + 1), env.rollout(T)
    env.reset()
    before = {k: v.clone() for k, v in agent.weights.items()}
    for it in range(3):
        ro.begin()
        for _ in range(T):
            env.step_autoreset(agent.act(mode="uniform" if it == 0 else "epsilon"))
        mem.append(ro)
        assert ro.check()[0] == T
        agent.update(mem, n_updates=2, batch_size=96, target_every=2)
    st = agent.stats_dict()
    assert all(np.isfinite(v) for v in st.values()) and st["W"] >= 1.0
    assert mem.head.cpu().tolist() == [(3 * T * B) % mem.capacity, mem.capacity, 3 * T * B, 6]
    assert agent.step_count.cpu().tolist() == [6, 0, 0, 0] and agent.counters.cpu().tolist() == [3 * T] * B
    assert all(bool(torch.isfinite(v).all()) and not torch.equal(v, before[k]) for k, v in agent.weights.items())
    assert not torch.equal(agent.target, agent.params) and set(mem.act.unique().cpu().tolist()) <= {0.0, 1.0, 2.0}
    env.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_one_iteration_on_mixing(dtype):
    from beacon_amd import DQN, vec as V
    B, T = 2, 2
    env = V.VecMixing(B, DEV, dtype)
    agent = DQN(env, hidden=(16,), seed=3)
    assert (agent.obs_dim, agent.n_actions) == (192, 4)
    w = R.random_weights(192, 4, (16,), False, 1)
    agent.load([(w["q_w%d" % l], w["q_b%d" % l]) for l in range(2)])
    mem, ro = agent.replay(16), env.rollout(T)
    env.reset()
    ro.begin()
    for _ in range(T):
        env.step_autoreset(agent.act(mode="epsilon"))
    mem.append(ro)
    assert ro.check()[0] == T and torch.equal(mem.act[:T * B, 0].cpu(), ro.act.reshape(-1).cpu().to(mem.act.dtype))
    agent.update(mem, n_updates=1, batch_size=8)
    st = agent.stats_dict()
    assert all(np.isfinite(v) for v in st.values()) and st["W"] == 8.0
    assert mem.head.cpu().tolist() == [T * B, T * B, T * B, 1] and agent.step_count.cpu().tolist() == [1, 0, 0, 0]
    env.close()
