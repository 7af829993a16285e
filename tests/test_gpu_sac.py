"""Soft actor-critic on the device (beacon_amd.SAC, libbeacon_sac.so, over beacon_amd.Replay) against tests/sac_ref.py -- torch autograd
in float64 on the CPU, the three random streams in NumPy -- on the MI355X.

How errors are measured (as in tests/test_gpu_td3.py): err(q) = max |device - reference| / max(1, max |reference|) for a quantity q -- a
gradient segment, a statistic, a parameter segment.  The reference gets the device's inputs (weights and rows as the device holds
them, cast to float64) and the host restatement's indices and draws, so the error is the kernels' arithmetic alone.

A condition on the inputs: min(Q_1, Q_2) in the target and in the policy step, the log-std clamp at -20 and 2 and relu are not smooth,
and the device must take the reference's branch on every live row.  check_margins asserts on the float64 REFERENCE alone that |Q'_1 -
Q'_2| at (s', a'), |Q_1 - Q_2| at (s, a~), the distance of every raw log-std (of both draws) from each clamp bound and of every relu
pre-activation from 0 exceed 100 x the case's tolerance, over every live row: no case skips rows.  The `clamps` case lies BEYOND both
clamp bounds in some live rows and has |u| > 15 in some (asserted too), never near a bound.  Per-row terms stay below 500.  The data
seeds in the case table were found on the CPU with sac_ref for which that holds.

float64: f64_tol(m, chain) = (m + max(640, chain)) x 2^-53 x 500, the summation-order bound of tests/test_gpu_td3.py.  For the critic
the chain is D + sum(hidden), D = obs_dim + act_dim.  The policy gradient runs through TWO networks -- down a critic to the action
columns, then down pi -- so its chain is (D + sum(hidden)) + (obs_dim + sum(hidden)); the two critics run one after the other, not
chained.
float32: the project's rule -- every tolerance in F32_TOL is at most 10 x the error measured on the MI355X for that case, and at most
10 x what sac_ref in float32 on the CPU (another summation order) shows against float64 on the same case; the three numbers stand
next to each other there."""
import types

import numpy as np
import pytest
import torch

import sac_ref as R
import td3_ref as R3
from beacon_amd import sac as _sac  # noqa: F401  (the module under test: importing it touches neither a compiler nor the GPU)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U64 = 2.0 ** -53
SEED = 0x1234567887654321
GAMMA = 0.9
CTR_NEXT, CTR_PI = 3, 4                        # the counters of streams 8 and 9 the cases start from
DTYPES = [torch.float32, torch.float64]


def f64_tol(m, chain=640):
    return (m + max(640, chain)) * U64 * 500.0


# float32: quantity -> case / shape / preset -> (tolerance, the error measured on the MI355X, the error of sac_ref in float32 on the CPU
# on the same case).  Every tolerance is at most 10 x either number.
F32_TOL = {
    "act": {"a1": (7.4e-07, 7.493e-08, 1.165e-07), "a16": (1.2e-06, 1.216e-07, 1.320e-07), "a3": (2.3e-06, 2.824e-07, 2.374e-07),
            "a16w": (3.5e-06, 3.591e-07, 3.928e-07)},
    "critic_grad": {"one": (1.1e-06, 1.134e-07, 1.244e-07), "straddle": (1.6e-06, 2.033e-07, 1.698e-07), "wide": (2.6e-06, 3.342e-07, 2.623e-07),
                    "tiles": (1.0e-06, 1.019e-07, 3.218e-07), "clamps": (2.7e-06, 3.490e-07, 2.707e-07)},
    "critic_stats": {"one": (1.6e-06, 1.669e-07, 1.669e-07), "straddle": (1.4e-06, 1.423e-07, 2.369e-07), "wide": (9.4e-07, 1.413e-07, 9.440e-08),
                     "tiles": (7.5e-07, 9.204e-08, 7.585e-08), "clamps": (4.3e-07, 1.647e-07, 4.327e-08)},
    "policy_grad": {"one": (2.3e-06, 2.389e-07, 2.349e-07), "straddle": (1.2e-06, 1.294e-07, 1.549e-07), "wide": (1.1e-06, 2.542e-07, 1.158e-07),
                    "tiles": (2.1e-07, 2.129e-08, 9.574e-07), "clamps": (8.1e-07, 8.167e-08, 1.720e-07)},
    "policy_stats": {"one": (3.5e-06, 3.607e-07, 3.545e-07), "straddle": (7.7e-07, 7.792e-08, 1.549e-07), "wide": (6.5e-07, 6.555e-08, 1.045e-07),
                     "tiles": (2.7e-07, 2.771e-08, 4.678e-07), "clamps": (1.8e-07, 1.886e-08, 1.465e-07)},
    "adam_params": {"clamps": (1.0e-06, 1.019e-07, 1.019e-07)},
    "polyak": {"clamps": (9.3e-07, 9.338e-08, 9.338e-08)},
    "e2e_params": {"auto-twin": (2.3e-06, 2.356e-07, 2.356e-07), "auto-single": (1.4e-06, 1.464e-07, 1.464e-07), "fixed-twin": (9.9e-07, 1.013e-07, 9.924e-08),
                   "fixed-single": (1.1e-06, 1.275e-07, 1.143e-07)}}

# (name, m float32 / float64, obs_dim float32 / float64, act_dim, hidden, activation, n_critics, options, data seed)
#   one       a single row
#   straddle  a partial second tile (65 / 33 rows); the action columns straddle a K-slab (62 + 3 / 30 + 3); relu; dead rows of NaN
#   wide      16 actions under 3 x 128: the 32-row head at the LDS limit, the two-pass register tile at every layer; one critic; rows
#             with boot = 0
#   tiles     more tiles than the backward launches' grid (129 > 128: a workgroup walks a second tile), dead rows; one critic: no 8 193
#             rows keep |Q_1 - Q_2| away from 0 twice
#   clamps    a scaled head: raw log-std above 2 and below -20 and |u| > 15 among the live rows; widths that are no multiple of 4;
#             bounds (-0.5, 1.5); a small temperature keeps alpha log pi', and with it (Q - y)^2, below 500
CASES = [("one", (1, 1), (3, 3), 1, (7,), "tanh", 2, {}, 1),
         ("straddle", (65, 33), (62, 30), 3, (7,), "relu", 2, {"dead": True}, 1),
         ("wide", (65, 33), (6, 6), 16, (128, 128, 128), "tanh", 1, {"boot0": True}, 1),
         ("tiles", (8193, 4097), (3, 3), 2, (7,), "tanh", 1, {"dead": True}, 1),
         ("clamps", (65, 33), (5, 5), 2, (33, 5), "tanh", 2, {"clamp": True, "dead": True, "alpha": 0.05}, 6)]
IDS = [c[0] for c in CASES]
# what (grid, tiles) must satisfy for the case to be in the regime it is named for
REGIME = {"tiles": lambda grid, tiles: grid == 128 and tiles == 129}
CKEYS = ("critic_loss", "q1_mean", "q2_mean", "target_mean", "W", "critic_grad_norm", "next_logp_mean", "alpha")
PKEYS = ("policy_loss", "W", "policy_grad_norm", "logp_mean", "alpha", "alpha_grad")


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
    """what SAC reads of an env: most tests need no solver behind the observation rows"""
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
    """the case's weights, targets, ring, minibatch and draws on the CPU, in the values the device will hold"""
    name, m, od, ad, hidden, activation, nc, opt, seed = unpack(case, dtype)
    rng = np.random.default_rng(seed)
    nd = npdt(dtype)
    clamp = bool(opt.get("clamp"))
    low, high = (-0.5, 1.5) if clamp else (-1.0, 1.0)
    W = R.random_weights(od, ad, hidden, nc, seed, alpha=opt.get("alpha", 0.7))
    Wt = R.random_weights(od, ad, hidden, nc, seed + 100, alpha=opt.get("alpha", 0.7))
    if clamp:                                                # the head scaled: means of +-20 or so, raw log-stds of +-40 or so
        L = len(hidden)
        W["pi_w%d" % L][:ad] *= 12.0
        W["pi_w%d" % L][ad:] *= 30.0
        W["pi_b%d" % L][ad:] -= 6.0
    rnd = lambda d: {k: v.astype(nd).astype(np.float64) for k, v in d.items()}
    W, Wt = rnd(W), rnd(Wt)
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
    idx = R.sample_idx(m, SEED, Cn, 5)
    return dict(W=W, Wt=Wt, ring=ring, idx=idx, z8=R.next_normals(SEED, m, CTR_NEXT, ad, nd), z9=R.pi_normals(SEED, m, CTR_PI, ad, nd),
                low=low, high=high, batch=ring.gather(idx), te=-float(ad), alpha=opt.get("alpha", 0.7))


def make_ref(case, dtype, d, rdtype=torch.float64):
    name, m, od, ad, hidden, activation, nc, opt, seed = unpack(case, dtype)
    return R.Ref(od, ad, hidden, activation, d["low"], d["high"], nc, d["W"], d["Wt"], dtype=rdtype)


def make_agent(case, dtype, d, batch=4, **kw):
    from beacon_amd import SAC
    name, m, od, ad, hidden, activation, nc, opt, seed = unpack(case, dtype)
    env = _Env(batch, od, ad, dtype, d["low"], d["high"])
    agent = SAC(env, hidden=hidden, activation=activation, twin=nc == 2, seed=SEED, **dict(dict(gamma=GAMMA, alpha=d["alpha"]), **kw))
    nets = [[(d["W"]["%s_w%d" % (n, l)], d["W"]["%s_b%d" % (n, l)]) for l in range(len(hidden) + 1)] for n in ("pi", "q1", "q2")[:1 + nc]]
    agent.load(*nets)
    for k in agent.weights:
        agent.weights[k].copy_(torch.as_tensor(d["W"][k]).to(dtype).view(agent.weights[k].shape))
        agent.target_weights[k].copy_(torch.as_tensor(d["Wt"][k]).to(dtype).view(agent.target_weights[k].shape))
    ring = d["ring"]
    mem = agent.replay(ring.C)
    for k in ("obs", "next_obs", "act", "rwd", "boot", "live", "head"):
        getattr(mem, k).copy_(torch.as_tensor(getattr(ring, k)).view(getattr(mem, k).shape))
    agent.step_count[3:4].fill_(CTR_NEXT)
    agent.step_count[4:5].fill_(CTR_PI)
    return agent, mem


def check_margins(case, dtype, ref, c, p, tol):
    """the module docstring's condition, on the float64 reference's numbers"""
    name, m, od, ad, hidden, activation, nc, opt, seed = unpack(case, dtype)
    mg = {"twin_target": c["margins"]["twin"], "twin_policy": p["margins"]["twin"], "clamp_next": c["margins"]["clamp"],
          "clamp_policy": p["margins"]["clamp"], "relu": ref.min_pre}
    print("sac margins %s %s: %s (100 tol = %.3e)" % (name, tag(dtype), {k: "%.3e" % v for k, v in mg.items()}, 100 * tol))
    assert all(v > 100 * tol for v in mg.values()), (mg, tol)
    assert c["row_term_max"] <= 500.0 and p["row_term_max"] <= 500.0, (c["row_term_max"], p["row_term_max"])
    if opt.get("clamp"):
        lv = c["live"]
        for r in (c, p):
            assert (r["raw"][lv] > 2.0).any() and (r["raw"][lv] < -20.0).any() and (np.abs(r["u"][lv]) > 15.0).any()
            assert ((r["raw"][lv] > -20.0) & (r["raw"][lv] < 2.0)).any()             # and some rows pass gradient


@pytest.fixture(scope="module")
def refs():
    """(case name, dtype tag) -> the data and the float64 / float32 references' critic and policy results: computed once, read-only"""
    cache = {}

    def get(case, dtype):
        key = (case[0], tag(dtype))
        if key not in cache:
            d = make_data(case, dtype)
            ref = make_ref(case, dtype, d)
            c = ref.critic(d["batch"], d["z8"], GAMMA)
            c["live"] = d["batch"]["w"] > 0
            p = ref.policy(d["batch"], d["z9"], d["te"])
            out = dict(d=d, ref=ref, c=c, p=p, c32=None, p32=None)
            if dtype == torch.float32:
                r32 = make_ref(case, dtype, d, torch.float32)
                out["c32"], out["p32"] = r32.critic(d["batch"], d["z8"], GAMMA), r32.policy(d["batch"], d["z9"], d["te"])
            cache[key] = out
        return cache[key]
    return get


def chains(case, dtype):
    name, m, od, ad, hidden, activation, nc, opt, seed = unpack(case, dtype)
    c = od + ad + sum(hidden)
    return c, c + od + sum(hidden)


def stat_err(dev, want, keys):
    return max(abs(dev[k] - want[k]) / max(1.0, abs(want[k])) for k in keys)


def report(key, sub, dtype, gpu, cpu32=None):
    """one line per measured error: what F32_TOL's second and third columns are copied from"""
    print("sac err %s %s %s gpu=%.3e cpu32=%s" % (key, sub, tag(dtype), gpu, "-" if cpu32 is None else "%.3e" % cpu32))


# ---- act ---------------------------------------------------------------------------------------
ACT_SHAPES = [("a1", 1, (7,), "tanh"), ("a16", 16, (33, 5), "relu"), ("a3", 3, (128, 128, 128), "tanh"), ("a16w", 16, (128, 128, 128), "tanh")]


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("shape", ACT_SHAPES, ids=lambda s: s[0])
def test_act(shape, dtype):
    from beacon_amd import SAC
    sub, ad, hidden, activation = shape
    od, B, off = 11, tile_rows(dtype) + 1, 2 ** 32 - 3
    nd = npdt(dtype)
    rng = np.random.default_rng(ad)
    W = {k: v.astype(nd).astype(np.float64) for k, v in R.random_weights(od, ad, hidden, 1, 17).items()}
    env = _Env(B, od, ad, dtype, -0.5, 1.5)
    agent = SAC(env, hidden=hidden, activation=activation, twin=False, seed=SEED, replica_offset=off)
    agent.load(*[[(W["%s_w%d" % (n, l)], W["%s_b%d" % (n, l)]) for l in range(len(hidden) + 1)] for n in ("pi", "q1")])
    ref = R.Ref(od, ad, hidden, activation, -0.5, 1.5, 1, W)
    r32 = R.Ref(od, ad, hidden, activation, -0.5, 1.5, 1, W, dtype=torch.float32)
    obs_np = rng.standard_normal((B, od)).astype(nd)
    obs = torch.as_tensor(obs_np).to(DEV)
    tol = tol_of(dtype, "act", sub, 1, od + sum(hidden))
    # deterministic: c + h tanh(mean), no tick
    a = agent.act(obs, mode="deterministic")
    assert a is agent.actions and tuple(a.shape) == (B, ad)
    det, _ = ref.act(obs_np.astype(np.float64), np.zeros((B, ad)))
    e_det = err(a, det)
    assert not bool(agent.counters.any())
    # sample: the host's draws; counters tick; actions stay inside the Box
    agent.counters.copy_(torch.arange(B, dtype=torch.int32) * 3)
    ctr = np.arange(B) * 3
    z = R.act_normals(SEED, off, ctr, ad, nd)
    _, want = ref.act(obs_np.astype(np.float64), z)
    a = agent.act(obs, mode="sample").clone()
    e_smp = err(a, want)
    assert agent.counters.cpu().tolist() == (ctr + 1).tolist()
    assert float(a.min()) >= -0.5 and float(a.max()) <= 1.5 and np.abs(want - det).max() > 0.1
    # uniform: low + (high - low) u on the same stream, at the ticked counters
    u = R.act_uniforms(SEED, off, ctr + 1, ad, nd)
    a = agent.act(obs, mode="uniform").clone()
    e_uni = err(a, -0.5 + 2.0 * u)
    assert float(a.min()) >= -0.5 and float(a.max()) <= 1.5 and agent.counters.cpu().tolist() == (ctr + 2).tolist()
    # masked rows and their counters are untouched, bit for bit
    mask = torch.as_tensor(np.arange(B) % 3 != 0)
    before, cb = agent.actions.clone(), agent.counters.clone()
    agent.act(obs, mask=mask, mode="sample")
    skipped = ~mask.to(DEV)
    assert torch.equal(agent.actions[skipped], before[skipped]) and torch.equal(agent.counters[skipped], cb[skipped])
    assert torch.equal(agent.counters[~skipped], cb[~skipped] + 1) and not torch.equal(agent.actions[~skipped], before[~skipped])
    a32 = r32.act(obs_np.astype(np.float64), z)
    report("act", sub, dtype, max(e_det, e_smp, e_uni), max(err(a32[0], det), err(a32[1], want)))
    assert max(e_det, e_smp, e_uni) <= tol, (e_det, e_smp, e_uni, tol)


# ---- the gradients -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gradients_and_stats_match_reference(case, dtype, refs):
    name, m, od, ad, hidden, activation, nc, opt, seed = unpack(case, dtype)
    r = refs(case, dtype)
    d, ref, c, p = r["d"], r["ref"], r["c"], r["p"]
    cchain, pchain = chains(case, dtype)
    tols = {k: tol_of(dtype, k, name, m, pchain if k.startswith("policy") else cchain) for k in ("critic_grad", "critic_stats", "policy_grad", "policy_stats")}
    check_margins(case, dtype, ref, c, p, max(tols.values()))
    if opt.get("dead"):
        assert 0 < d["batch"]["w"].sum() < m and np.isnan(d["batch"]["s"]).any()
    if opt.get("boot0"):
        assert 0 < d["batch"]["boot"].sum() < m
    agent, mem = make_agent(case, dtype, d)
    if name == "wide":
        assert agent.lds_bytes == (158336 if dtype == torch.float64 else 160256)          # the 32-row head at the limit
    plan = agent.plan(mem, 1, m)
    tiles = -(-m // tile_rows(dtype))
    if name in REGIME:
        assert REGIME[name](agent.grid, tiles), (agent.grid, tiles)
    plan.idx.copy_(torch.as_tensor(d["idx"]).to(torch.int32))
    params0, target0 = agent.params.clone(), agent.target.clone()
    plan.critic_grad()
    cnames, pnames = ref.names_of(0), ref.names_of(1) + ["log_alpha"]
    ge = {k: err(plan.grads[k], c["grads"][k]) for k in cnames}
    st = agent.stats_dict()
    se = stat_err(st, c["stats"], CKEYS)
    assert not any(bool(plan.grads[k].any()) for k in pnames)             # the critic step leaves pi's and alpha's gradient alone
    qgrad = {k: plan.grads[k].clone() for k in cnames}
    plan.actor_grad()
    pe = {k: err(plan.grads[k], p["grads"][k]) for k in pnames}
    st = agent.stats_dict()
    pse = stat_err(st, p["stats"], PKEYS)
    assert all(torch.equal(plan.grads[k], qgrad[k]) for k in cnames)      # and the policy step the critics'
    assert stat_err(st, c["stats"], CKEYS) == se
    assert all(np.isfinite(v) for v in st.values()) and set(st) == set(R.STATS)
    assert torch.equal(agent.params, params0) and torch.equal(agent.target, target0)
    assert agent.step_count.cpu().tolist()[:5] == [0, 0, 0, CTR_NEXT, CTR_PI] and mem.head.cpu().tolist() == d["ring"].head.tolist()
    c32, p32 = r["c32"], r["p32"]
    f32 = c32 is not None
    report("critic_grad", name, dtype, max(ge.values()), max(err(c32["grads"][k], c["grads"][k]) for k in cnames) if f32 else None)
    report("critic_stats", name, dtype, se, stat_err(c32["stats"], c["stats"], CKEYS) if f32 else None)
    report("policy_grad", name, dtype, max(pe.values()), max(err(p32["grads"][k], p["grads"][k]) for k in pnames) if f32 else None)
    report("policy_stats", name, dtype, pse, stat_err(p32["stats"], p["stats"], PKEYS) if f32 else None)
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
    """the three steps of test_adam_and_polyak with sac_ref's own Adam, in `rdtype`: the float32 yardstick"""
    ref = make_ref(case, dtype, d, rdtype)
    for _ in range(3):
        ref.adam(0, ref.critic(d["batch"], d["z8"], GAMMA)["grads"], 1e-2)
        g = ref.policy(d["batch"], d["z9"], d["te"])["grads"]
        ref.adam(1, g, 1e-2)
        ref.adam(2, g, 3e-2)
        ref.polyak(0.25)
    return ref


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_adam_and_polyak(dtype, refs):
    case = CASES[4]
    name, m, od, ad, hidden, activation, nc, opt, seed = unpack(case, dtype)
    d = refs(case, dtype)["d"]
    agent, mem = make_agent(case, dtype, d, lr=1e-2, lr_alpha=3e-2, tau=0.25)
    ref = make_ref(case, dtype, d)
    plan = agent.plan(mem, 1, m)
    plan.idx.copy_(torch.as_tensor(d["idx"]).to(torch.int32))
    cn, pn, an = ref.names_of(0), ref.names_of(1), ref.names_of(2)
    # torch.optim.Adam on the reference's parameters with the reference's gradients
    tp = {k: v.clone().requires_grad_(True) for k, v in ref.W.items()}
    opts = [torch.optim.Adam([tp[k] for k in names], lr=lr, betas=(0.9, 0.999), eps=1e-8) for names, lr in ((cn, 1e-2), (pn, 1e-2), (an, 3e-2))]
    worst = {"adam_params": 0.0, "polyak": 0.0}
    for step in range(3):
        agent.step_count[3:4].fill_(CTR_NEXT)
        agent.step_count[4:5].fill_(CTR_PI)
        ref.W = {k: v.detach().clone() for k, v in tp.items()}
        c = ref.critic(d["batch"], d["z8"], GAMMA)
        before = {k: agent.weights[k].clone() for k in ref.names}
        tbefore = agent.target.clone()
        plan.critic_step()
        for k in cn:
            tp[k].grad = c["grads"][k].clone()
        opts[0].step()
        assert all(torch.equal(agent.weights[k], before[k]) for k in pn + an) and torch.equal(agent.target, tbefore)      # pi, alpha, targets stay
        assert not any(torch.equal(agent.weights[k], before[k]) for k in cn)
        ref.W = {k: v.detach().clone() for k, v in tp.items()}
        p = ref.policy(d["batch"], d["z9"], d["te"])
        before = {k: agent.weights[k].clone() for k in ref.names}
        plan.actor_grad().adam(1)
        assert all(torch.equal(agent.weights[k], before[k]) for k in cn + an) and torch.equal(agent.target, tbefore)      # q, alpha, targets stay
        before = {k: agent.weights[k].clone() for k in ref.names}
        plan.adam(2)
        assert all(torch.equal(agent.weights[k], before[k]) for k in cn + pn) and not torch.equal(agent.weights["log_alpha"], before["log_alpha"])
        for k in pn + an:
            tp[k].grad = p["grads"][k].clone()
        opts[1].step()
        opts[2].step()
        worst["adam_params"] = max([worst["adam_params"]] + [err(agent.weights[k], tp[k].detach()) for k in ref.names])
        plan.polyak()                                                                                             # the targets move here alone
        ref.W = {k: v.detach().clone() for k, v in tp.items()}
        ref.polyak(0.25)
        assert not torch.equal(agent.target, tbefore)
        worst["polyak"] = max([worst["polyak"]] + [err(agent.target_weights[k], ref.Wt[k]) for k in ref.names])
        assert agent.step_count.cpu().tolist()[:5] == [step + 1, step + 1, step + 1, CTR_NEXT + 1, CTR_PI + 1]
    cchain, pchain = chains(case, dtype)
    c32 = (None, None)
    if dtype == torch.float32:
        r64, r32 = (_adam_reference(case, dtype, d, t) for t in (torch.float64, torch.float32))
        c32 = (max(err(r32.W[k], r64.W[k]) for k in ref.names), max(err(r32.Wt[k], r64.Wt[k]) for k in ref.names))
    report("adam_params", name, dtype, worst["adam_params"], c32[0])
    report("polyak", name, dtype, worst["polyak"], c32[1])
    for k, v in worst.items():
        assert v <= tol_of(dtype, k, name, m, pchain), (k, v)


# ---- end to end ----------------------------------------------------------------------------------
def _run_reference(case, dtype, d, n_updates, auto, lr, lr_alpha, tau, rdtype=torch.float64):
    name, m, od, ad, hidden, activation, nc, opt, seed = unpack(case, dtype)
    ref = make_ref(case, dtype, d, rdtype)
    ring = d["ring"]
    head3 = int(ring.head[3])
    for k in range(n_updates):
        idx = R.sample_idx(m, SEED, int(ring.head[1]), head3 + k)
        batch = ring.gather(idx)
        ref.adam(0, ref.critic(batch, R.next_normals(SEED, m, CTR_NEXT + k, ad, npdt(dtype)), GAMMA)["grads"], lr)
        g = ref.policy(batch, R.pi_normals(SEED, m, CTR_PI + k, ad, npdt(dtype)), d["te"])["grads"]
        ref.adam(1, g, lr)
        if auto:
            ref.adam(2, g, lr_alpha)
        ref.polyak(tau)
    return ref


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("twin", [True, False], ids=["twin", "single"])
@pytest.mark.parametrize("auto", [True, False], ids=["auto", "fixed"])
def test_end_to_end_update(auto, twin, dtype, refs):
    case = CASES[4] if twin else CASES[2]
    name, m, od, ad, hidden, activation, nc, opt, seed = unpack(case, dtype)
    preset = "%s-%s" % ("auto" if auto else "fixed", "twin" if twin else "single")
    d = refs(case, dtype)["d"]
    lr, lr_alpha, tau = 1e-3, 3e-3, 0.05
    agent, mem = make_agent(case, dtype, d, lr=lr, lr_alpha=lr_alpha, tau=tau, auto_alpha=auto)
    assert (agent.twin, agent.n_critics, agent.auto_alpha) == (twin, nc, auto) and agent.entropy_target() == -float(ad)
    la0 = agent.log_alpha.clone()
    assert agent.update(mem, n_updates=6, batch_size=m) is agent
    ref = _run_reference(case, dtype, d, 6, auto, lr, lr_alpha, tau)
    assert agent.step_count.cpu().tolist()[:5] == [6, 6, 6 if auto else 0, CTR_NEXT + 6, CTR_PI + 6]
    assert int(mem.head[3]) == int(d["ring"].head[3]) + 6 and torch.equal(agent.log_alpha, la0) != auto
    ep = max(err(agent.weights[k], ref.W[k]) for k in ref.names)
    et = max(err(agent.target_weights[k], ref.Wt[k]) for k in ref.names)
    c32 = None
    if dtype == torch.float32:
        r32 = _run_reference(case, dtype, d, 6, auto, lr, lr_alpha, tau, torch.float32)
        c32 = max(err(r32.W[k], ref.W[k]) for k in ref.names)
    report("e2e_params", preset, dtype, max(ep, et), c32)
    # six steps of Adam: a parameter moves by at most lr per step whatever the gradient, and by lr x (relative gradient error) from
    # an error in it; under err()'s floor of 1 the float64 bound is the gradient's own
    tol = tol_of(dtype, "e2e_params", preset, m, chains(case, dtype)[1])
    assert ep <= tol and et <= tol, (ep, et, tol)
    st = agent.stats_dict()
    assert set(st) == set(R.STATS) and all(np.isfinite(v) for v in st.values())


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_captured_plan_equals_eager(dtype, refs):
    case = CASES[4]
    d = refs(case, dtype)["d"]
    m = unpack(case, dtype)[1]
    outs = []
    for captured in (False, True):
        agent, mem = make_agent(case, dtype, d)
        plan = agent.plan(mem, 2, m)
        if captured:
            g = plan.capture()
            assert int(mem.head[3]) == int(d["ring"].head[3]) and agent.step_count.cpu().tolist()[:5] == [0, 0, 0, CTR_NEXT, CTR_PI]      # nothing ran
            g.replay()
            torch.cuda.synchronize()
            first = (plan.idx.clone(), plan.xb.clone())
            g.replay()
            torch.cuda.synchronize()
            assert not torch.equal(plan.idx, first[0]) and not torch.equal(plan.xb, first[1])        # a replay draws new samples and noise
        else:
            plan.run().run()
        torch.cuda.synchronize()
        outs.append([x.clone() for x in (agent.params, agent.target, agent.state, mem.buf, plan.idx, plan.grad)])
    assert all(a.view(torch.uint8).equal(b.view(torch.uint8)) for a, b in zip(*outs))
    assert outs[0][2].view(torch.uint8).any() and int(mem.head[3]) == int(d["ring"].head[3]) + 4


# ---- a real env, and the memory shared with TD3 ---------------------------------------------------
def _nets(w, names, n_layers):
    return [[(w["%s_w%d" % (n, l)], w["%s_b%d" % (n, l)]) for l in range(n_layers)] for n in names]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_loop_on_a_real_env(dtype):
    from beacon_amd import SAC, vec as V
    B, T = 4, 3
    env = V.VecBurgers(B, DEV, dtype)
    agent = SAC(env, hidden=(7,), seed=3)
    agent.load(*_nets(R.random_weights(agent.obs_dim, agent.act_dim, (7,), 2, 1), ("pi", "q1", "q2"), 2))
    mem, ro = agent.replay(2 * T * B + 1), env.rollout(T)
    env.reset()
    env.set_stp(env.n_act - 1 - np.arange(B) % 3)               # episodes end at steps 0, 1, 2 of what follows
    before = agent.params.clone()
    for it in range(3):
        ro.begin()
        for _ in range(T):
            env.step_autoreset(agent.act(mode="uniform" if it == 0 else "sample"))
        mem.append(ro)
        assert ro.check()[0] == T
        agent.update(mem, n_updates=2, batch_size=8)
    st = agent.stats_dict()
    assert all(np.isfinite(v) for v in st.values()) and st["W"] >= 1.0 and st["alpha"] > 0.0
    assert mem.head.cpu().tolist() == [(3 * T * B) % mem.capacity, mem.capacity, 3 * T * B, 6]
    assert agent.step_count.cpu().tolist()[:5] == [6, 6, 6, 6, 6]
    for k in agent.weights:
        assert bool(torch.isfinite(agent.weights[k]).all()), k
    changed = {k for k in agent.weights if not torch.equal(agent.weights[k], _sac._views(before, agent.params_layout, agent.tdtype)[k].view(agent.shapes[k]))}
    assert changed == set(agent.weights)
    env.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_replay_is_shared_with_td3(dtype):
    from beacon_amd import SAC, TD3, vec as V
    B, T = 4, 3
    env = V.VecBurgers(B, DEV, dtype)
    sac, td3 = SAC(env, hidden=(7,), seed=3), TD3(env, hidden=(7,), seed=3)
    mems = [a.replay(2 * T * B + 1) for a in (sac, td3)]
    assert mems[0].lib is mems[1].lib is td3.lib and mems[0].layout == mems[1].layout
    ro = env.rollout(T)
    env.reset()
    env.set_stp(env.n_act - 1 - np.arange(B) % 3)
    for it in range(3):
        ro.begin()
        for _ in range(T):
            env.step_autoreset(sac.act(mode="uniform"))
        for mem in mems:
            mem.append(ro)
    assert mems[0].buf.cpu().numpy().tobytes() == mems[1].buf.cpu().numpy().tobytes() and bool(mems[0].live.any())
    idx = [torch.zeros(32, dtype=torch.int32, device=DEV) for _ in mems]
    for mem, i in zip(mems, idx):
        mem.sample(i)
    assert torch.equal(idx[0], idx[1]) and np.array_equal(idx[0].cpu().numpy(), R3.sample_idx(32, 3, mems[0].capacity, 0))
    sac.set_seed(4)
    assert int(mems[0].head[3]) == 0 and int(mems[1].head[3]) == 1
    env.close()
