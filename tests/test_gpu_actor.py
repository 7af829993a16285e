"""The on-device actor (beacon_amd.Actor, libbeacon_actor.so) against tests/actor_ref.py, the float64 NumPy restatement of
include/beacon_actor.h, on the MI355X.

How errors are measured: for a quantity q (dist, value, raw, logp, z), err(q) = max |device - reference| / max(1, max |reference|)
over the case -- relative to the quantity's scale, with a floor of 1 so that an entry that cancels to nearly zero is held to the
absolute bound.  The reference gets the device's inputs (the float32 weights and observations cast to float64), so the error is the
kernel's arithmetic alone.

float64: 1e-12, the bound of summation-order differences at these widths (K <= 384 terms of size <= 10: 384 x 10 x 2^-53 = 4e-13).
float32: every tolerance below is at most 10 x the worst error measured over CASES on the MI355X -- the project's rule; both
numbers stand next to each tolerance."""
import numpy as np
import pytest
import torch

import actor_ref as R
import rollout_ref

pytestmark = pytest.mark.gpu

F64_TOL = 1e-12
# float32 tolerance per quantity: (tolerance, worst measured error over CASES x 2 calls)
F32_TOL = {"dist": (3.2e-6, 3.230e-7), "value": (3.9e-6, 3.912e-7), "raw": (3.1e-6, 3.166e-7), "logp": (1.4e-6, 1.718e-7), "z": (1.5e-6, 1.520e-7)}
DELTA, CAP = 1e-5, 0.005          # categorical: a draw within DELTA of a cumulative boundary may fall either way; at most CAP of all draws may

# (B, obs_dim, hidden, activation, kind, act_dim / classes, weight scale): every B, obs_dim, hidden spec, activation and act_dim of
# the issue at least once; B = 65 / 257 are partial tiles behind one / several full ones, obs_dim = 384 takes six K-slabs (float64: twelve),
# hidden 128 takes the two-pass register tile, 17 and 5 and 3 are partial output groups, odd act_dim leaves half a pair unused; scale 8
# saturates tanh and spreads the logits.
CASES = [(1, 1, (5,), "tanh", "gaussian", 1, 1.0),
         (3, 6, (64, 64), "tanh", "categorical", 3, 1.0),
         (65, 33, (17, 128, 3), "relu", "gaussian", 5, 1.0),
         (257, 384, (64, 64), "tanh", "gaussian", 10, 1.0),
         (65, 6, (64, 64), "relu", "categorical", 4, 1.0),
         (257, 33, (5,), "tanh", "gaussian", 2, 1.0),
         (65, 384, (17, 128, 3), "tanh", "categorical", 3, 1.0),
         (257, 6, (64, 64), "tanh", "gaussian", 2, 8.0),
         (65, 6, (64, 64), "tanh", "categorical", 4, 8.0),
         # the limits of the ABI: obs_dim 512 (eight K-slabs; float64: sixteen), three layers of 128, 16 actions / classes, and widths
         # above 64 that are no multiple of 4.  F64_TOL's derivation at K = 512: 512 x 10 x 2^-53 = 5.7e-13
         (65, 512, (128, 128, 128), "tanh", "gaussian", 16, 1.0),
         (65, 512, (100, 65), "relu", "categorical", 16, 1.0),
         # a first layer whose K ends in a partial SECOND slab in float32 too (65 = 64 + 1, 100 = 64 + 36; 33 does so in float64 only)
         (65, 65, (64, 64), "tanh", "gaussian", 3, 1.0),
         (65, 100, (64, 64), "relu", "categorical", 5, 1.0),
         # one hidden unit (one output group, three of its four columns padding) and 127 (the two-pass tile, one column short) behind 4
         (65, 6, (1,), "tanh", "gaussian", 2, 1.0),
         (65, 33, (4, 127), "tanh", "categorical", 3, 1.0),
         # full tiles only: no zero-staged row anywhere (64 = one float32 tile, two float64 tiles; 128 = two / four)
         (64, 6, (64, 64), "tanh", "gaussian", 4, 1.0),
         (128, 33, (5,), "relu", "categorical", 2, 1.0)]


class _Env(object):
    """what Actor reads of an env: most tests need no solver behind the observation rows"""
    _norm_on = False

    def __init__(self, batch, obs_dim, kind, n, dtype):
        from beacon_amd import spaces
        self.batch, self.obs_dim, self.tdtype, self.device = batch, obs_dim, dtype, torch.device("cuda", torch.cuda.current_device())
        self.action_is_int = kind == "categorical"
        self.action_space = spaces.discrete(n) if self.action_is_int else spaces.box(-1.0, 1.0, (n,))
        self.obs = None


def _weights(obs_dim, hidden, n, scale, seed):
    """[(W, b)] of both networks and log_std: entries of size 1 / sqrt(in) (x scale), float64"""
    rng = np.random.default_rng(seed)
    nets = []
    for head in (n, 1):
        dims, layers = [obs_dim] + list(hidden) + [head], []
        for i, o in zip(dims[:-1], dims[1:]):
            layers.append((rng.uniform(-1.0, 1.0, (o, i)) * scale / np.sqrt(i), rng.uniform(-0.1, 0.1, o)))
        nets.append(layers)
    return nets[0], nets[1], rng.uniform(-1.0, 0.5, n)


def _actor(B, obs_dim, hidden, activation, kind, n, scale, dtype, seed=7, wseed=1, replica_offset=0):
    """(actor, reference weights as the device holds them, in float64)"""
    from beacon_amd import Actor
    env = _Env(B, obs_dim, kind, n, dtype)
    a = Actor(env, hidden=hidden, activation=activation, seed=seed, replica_offset=replica_offset)
    pi, vf, ls = _weights(obs_dim, hidden, n, scale, wseed)
    a.load(pi, vf, ls if kind == "gaussian" else None)
    back = lambda net: [(a.weights["%s_w%d" % (net, l)].double().cpu().numpy(), a.weights["%s_b%d" % (net, l)].double().cpu().numpy())
                        for l in range(len(hidden) + 1)]
    return a, (back("pi"), back("vf"), a.weights["log_std"].double().cpu().numpy())


def _obs(B, obs_dim, dtype, seed=3):
    return torch.as_tensor(np.random.default_rng(seed).uniform(-1.0, 1.0, (B, obs_dim)), dtype=dtype).cuda()


def _ref(a, w, obs, counters, deterministic=False):
    return R.act(obs.double().cpu().numpy(), w[0], w[1], w[2], a.activation, "gaussian" if a.kind == 0 else "categorical",
                 np.float64 if a.tdtype == torch.float64 else np.float32, a.seed, a.replica_offset, counters, a.low, a.high, deterministic)


def _err(dev, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(dev.double().cpu().numpy().reshape(ref.shape) - ref).max() / max(1.0, np.abs(ref).max()))


def _near(ref):
    """which draws lie within DELTA of one of the reference's cumulative boundaries"""
    return (np.abs(ref["u"][:, None] - ref["cum"]) <= DELTA).any(axis=1)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", CASES, ids=["%dx%d-%s-%s-%s%d-x%g" % (c[0], c[1], "_".join(map(str, c[2])), c[3], c[4][:3], c[5], c[6]) for c in CASES])
def test_outputs_match_reference(case, dtype):
    B, obs_dim, hidden, activation, kind, n, scale = case
    a, w = _actor(B, obs_dim, hidden, activation, kind, n, scale, dtype)
    obs = _obs(B, obs_dim, dtype)
    tol = (lambda q: F64_TOL) if dtype == torch.float64 else (lambda q: F32_TOL[q][0])
    worst = {}
    for call in range(2):                                       # the second call draws with counter 1
        acts = a.act(obs)
        ref = _ref(a, w, obs, np.full(B, call))
        assert acts is a.actions
        assert a.counters.cpu().tolist() == [call + 1] * B      # the exact integers
        errs = {q: _err(getattr(a, q), ref[q]) for q in ("dist", "value")}
        if kind == "gaussian":
            errs.update({q: _err(getattr(a, q), ref[q]) for q in ("raw", "logp")})
            z = (a.raw - a.dist) / torch.exp(a.weights["log_std"])
            errs["z"] = _err(z, ref["z"])
            assert torch.equal(a.actions, a.raw.clamp(a.low, a.high))                      # actions == clip(raw) exactly
        else:
            errs["raw"] = _err(a.raw, ref["raw"])
            near = _near(ref)
            # the reference alone, first: the exemption is rare enough to rely on (expected share 2 DELTA (n - 1): 3e-4 at 16 classes)
            assert near.mean() <= CAP, near.mean()
            dev = a.actions.cpu().numpy()
            assert np.array_equal(dev[~near], ref["actions"][~near])
            assert torch.equal(a.logp, a.dist.gather(1, a.actions.long()[:, None])[:, 0])    # logp == dist[action] exactly
        print("actor errors %s %s call %d: %s" % (case, "f64" if dtype == torch.float64 else "f32", call,
                                                  " ".join("%s=%.3e" % kv for kv in sorted(errs.items()))))
        worst = {q: max(e, worst.get(q, 0.0)) for q, e in errs.items()}
    for q, e in worst.items():
        assert e <= tol(q), (q, e, tol(q))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_gaussian_stream(dtype):
    """set_seed restarts the stream; replica_offset = k on a batch equals rows k .. of a larger batch, bit for bit."""
    case = (65, 6, (64, 64), "tanh", "gaussian", 5, 1.0)
    a, w = _actor(*case, dtype)
    obs = _obs(65, 6, dtype)
    first = [(a.act(obs).clone(), a.raw.clone(), a.logp.clone()) for _ in range(2)]
    assert not torch.equal(first[0][1], first[1][1])
    a.set_seed(7)
    assert a.counters.cpu().tolist() == [0] * 65
    for k in range(2):
        a.act(obs)
        assert torch.equal(a.raw, first[k][1]) and torch.equal(a.logp, first[k][2]) and torch.equal(a.actions, first[k][0])
    a.set_seed(8)
    a.act(obs)
    assert not torch.equal(a.raw, first[0][1])
    b, _ = _actor(60, 6, (64, 64), "tanh", "gaussian", 5, 1.0, dtype, replica_offset=5)
    tail = obs[5:].contiguous()
    for k in range(2):
        b.act(tail)
        assert torch.equal(b.raw, first[k][1][5:]) and torch.equal(b.logp, first[k][2][5:])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_categorical_stream(dtype):
    """The device's class equals the float64 reference's for every draw that is not within DELTA = 1e-5 of one of the reference's
    cumulative boundaries, and such draws are at most 0.5 % of all draws of this test.  The cap is a condition, checked first on the
    CPU with actor_ref alone over this test's own seeds (expected share 2 DELTA (n - 1) <= 6e-5): only then is the exemption relied on."""
    draws = near_all = 0
    for n, seed in ((3, 11), (4, 12)):
        a, w = _actor(4096, 6, (64, 64), "tanh", "categorical", n, 2.0, dtype, seed=seed)
        obs = _obs(4096, 6, dtype)
        refs = [_ref(a, w, obs, np.full(4096, call)) for call in range(3)]
        share = float(np.mean([_near(r).mean() for r in refs]))
        assert share <= CAP, share                               # the reference alone: the exemption is rare enough to rely on
        for call, ref in enumerate(refs):
            a.act(obs)
            near = _near(ref)
            dev = a.actions.cpu().numpy()
            assert np.array_equal(dev[~near], ref["actions"][~near])
            assert ((dev >= 0) & (dev < n)).all() and len(set(dev.tolist())) == n       # every class is drawn
            assert torch.equal(a.logp, a.dist.gather(1, a.actions.long()[:, None])[:, 0])
            draws, near_all = draws + near.size, near_all + int(near.sum())
    assert near_all <= CAP * draws, (near_all, draws)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_deterministic_mode(dtype):
    a, w = _actor(65, 6, (64, 64), "tanh", "gaussian", 5, 1.0, dtype)
    obs = _obs(65, 6, dtype)
    a.act(obs, deterministic=True)
    assert a.counters.cpu().tolist() == [0] * 65                 # no draw, no tick
    assert torch.equal(a.raw, a.dist) and torch.equal(a.actions, a.dist.clamp(-1.0, 1.0))
    ref = _ref(a, w, obs, np.zeros(65), deterministic=True)
    tol = F64_TOL if dtype == torch.float64 else F32_TOL["logp"][0]
    assert _err(a.logp, ref["logp"]) <= tol
    assert torch.equal(a.logp, a.logp[:1].expand(65))            # the density at the mean does not depend on the state
    c, w = _actor(65, 6, (64, 64), "tanh", "categorical", 4, 1.0, dtype)
    c.act(obs, deterministic=True)
    assert c.counters.cpu().tolist() == [0] * 65
    assert torch.equal(c.actions.long(), c.dist.argmax(dim=1)) and torch.equal(c.logp, c.dist.max(dim=1).values)
    # a constructed tie: a zero head with the bias (0, 1, 1, 0.5) makes classes 1 and 2 equal for every row -> the first of them
    head = len(c.hidden)
    c.weights["pi_w%d" % head].zero_()
    c.weights["pi_b%d" % head].copy_(torch.tensor([0.0, 1.0, 1.0, 0.5], dtype=dtype))
    c.act(obs, deterministic=True)
    assert c.actions.cpu().tolist() == [1] * 65 and torch.equal(c.dist[:, 1], c.dist[:, 2]) and torch.equal(c.logp, c.dist[:, 1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind,n", [("gaussian", 5), ("categorical", 3)])
def test_mask(kind, n, dtype):
    a, _ = _actor(65, 6, (64, 64), "tanh", kind, n, 1.0, dtype)
    b, _ = _actor(65, 6, (64, 64), "tanh", kind, n, 1.0, dtype)
    obs = _obs(65, 6, dtype)
    mask = torch.as_tensor(np.random.default_rng(5).integers(0, 2, 65), dtype=torch.uint8).cuda()
    mask[64] = 0
    mask[0] = 1
    names = ("actions", "raw", "logp", "value", "dist", "counters")
    for t in (a, b):
        t.act(obs)                                               # call 0: everything written
    before = {q: getattr(a, q).clone() for q in names}
    a.act(obs, mask=mask)
    b.act(obs)
    m = mask.bool()
    for q in names:
        va, vb = getattr(a, q), getattr(b, q)
        assert torch.equal(va[~m], before[q][~m]), q             # masked rows of every output and their counters: untouched
        assert torch.equal(va[m], vb[m]), q                      # the others: what an unmasked call writes
    assert a.counters[m].cpu().tolist() == [2] * int(m.sum()) and a.counters[~m].cpu().tolist() == [1] * int((~m).sum())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_values_equal_act_bit_for_bit(dtype):
    for B in (65, 512):                                          # 512 = T B of the rollout test below
        a, _ = _actor(B, 33, (17, 128, 3), "tanh", "gaussian", 2, 1.0, dtype)
        obs = _obs(B, 33, dtype)
        a.act(obs)
        assert torch.equal(a.values(obs), a.value)
        if B == 65:
            assert torch.equal(a.values(obs[:1].contiguous()), a.value[:1])
            out = torch.zeros(65, dtype=dtype, device="cuda")
            assert a.values(obs, out=out) is out and torch.equal(out, a.value)
            assert torch.equal(a.values(obs[3:40].contiguous()), a.value[3:40])          # another tile position, the same bits


def _env_case(name):
    import beacon_amd
    return beacon_amd.VecBurgers(64, dtype="f32", seed=5) if name == "burgers" else beacon_amd.VecLorenz(65, dtype="f32")


@pytest.mark.parametrize("name", ["burgers", "lorenz"])
def test_rollout_eager_equals_graph(name):
    from beacon_amd import Actor
    T = 8
    env = _env_case(name)
    actor = Actor(env, hidden=(64, 64), seed=21)
    pi, vf, ls = _weights(env.obs_dim, (64, 64), actor.act_dim, 2.0, 9)
    actor.load(pi, vf, ls if actor.kind == 0 else None)
    ro = env.rollout(T)
    actor.attach(ro)
    assert tuple(actor.logp_seq.shape) == (T, env.batch) and tuple(actor.raw_seq.shape) == (T, env.batch, actor.act_dim)

    def start():
        if name == "burgers":
            env.set_noise_seed(5)                                # the inlet noise's counters back to 0
        actor.set_seed(21)
        env.episodes.clear()
        env.reset()
        actor.seq.zero_()
        ro.clear()
        ro.begin()

    start()
    per_step = []
    for t in range(T):
        a = actor.act()
        per_step.append([x.clone() for x in (a, actor.logp, actor.value, actor.raw)])
        env.step_autoreset(a)
    assert ro.check() == (T, False)
    for t, (a, logp, value, raw) in enumerate(per_step):         # row t is what step t's act produced; the env was handed the same
        assert torch.equal(actor.logp_seq[t], logp) and torch.equal(actor.value_seq[t], value) and torch.equal(actor.raw_seq[t], raw)
        assert torch.equal(ro.act[t].reshape(a.shape), a)
    eager = (actor.seq.clone(), ro.buf.clone(), actor.state.clone())
    last = actor.seq.clone()
    actor.act()                                                  # a ninth act: the rollout is full, no slot is written
    assert torch.equal(actor.seq, last) and ro.check() == (T, False)

    # GAE from the actor's numbers, against the NumPy restatement fed with the same
    last_value = actor.values(env.obs)
    final_values = actor.values(ro.final_obs.reshape(T * env.batch, env.obs_dim)).view(T, env.batch)
    adv, ret = ro.compute_gae(actor.value_seq, last_value, final_values, gamma=0.99, lam=0.95)
    np64 = lambda x: x.double().cpu().numpy()
    rwd, val = np64(ro.rwd), np64(actor.value_seq)
    radv, rret = rollout_ref.gae_ref(rwd, val, np64(last_value), ro.done.cpu().numpy(), ro.trunc.cpu().numpy(), ro.valid.cpu().numpy(),
                                     np64(final_values), 0.99, 0.95)
    # the tolerance of tests/test_gpu_rollout.py: the recurrence's float64 bound plus the one float32 rounding on store
    bound, u = rollout_ref.gae_bound(T, radv, val, rwd)[None, :], 2.0 ** -24
    assert (np.abs(np64(adv) - radv) <= bound + u * (np.abs(radv) + bound)).all()
    assert (np.abs(np64(ret) - rret) <= bound + 2.0 ** -53 * (np.abs(radv) + np.abs(val)) + u * (np.abs(rret) + bound)).all()

    # the same loop, one step captured in the caller's graph and replayed T times
    start()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        env.step_autoreset(actor.act())
    # (the capture launched nothing)
    for _ in range(T):
        g.replay()
    torch.cuda.synchronize()
    assert ro.check() == (T, False)
    assert torch.equal(actor.seq, eager[0]) and torch.equal(ro.buf, eager[1]) and torch.equal(actor.state, eager[2])
    env.close()


def test_default_obs_is_norm_obs_while_normalising():
    import beacon_amd
    from beacon_amd import Actor
    env = beacon_amd.VecLorenz(65, dtype="f32")
    actor = Actor(env, hidden=(8,), seed=1)
    pi, vf, _ = _weights(6, (8,), 3, 1.0, 2)
    actor.load(pi, vf)
    env.set_normalize()
    env.reset()
    env.step(torch.ones(65, dtype=torch.int32, device="cuda"))
    assert not torch.equal(env._norm.norm_obs, env.obs)
    actor.act(deterministic=True)
    default = actor.dist.clone()
    actor.act(obs=env._norm.norm_obs, deterministic=True)
    assert torch.equal(actor.dist, default)
    actor.act(obs=env.obs, deterministic=True)
    assert not torch.equal(actor.dist, default)
    env.close()
