"""The per-jet mode of the actor and the learner (Actor(env, per_jet=True); Learner.grad(rows_per_weight=...)) on the MI355X.

The oracle is the mode's defining property: a per-jet actor over B replicas of A jets computes, bit for bit, what the plain actor
computes for a batch of B A rows [B A, n_obs] with act_dim 1, the same seed and replica_offset A in place of replica_offset; the
mask of act() and the weights of the learner stay per replica and are indexed on the device by row / A.  So every comparison here is
exact equality against the plain path on a flat twin (a stand-in env of B A replicas), with the per-replica arrays expanded by
repeat_interleave for the twin only.  The plain path itself is held to NumPy / autograd by tests/test_gpu_actor*.py and
tests/test_gpu_learner.py; no tolerance appears in this file.

Tiles are 64 rows (float32) and 32 rows (float64): (13, 5) puts replica 12 across the float32 tile edge (rows 60 .. 64), (7, 20)
spans tiles in both dtypes with A above the 16 action components of a plain actor, (65, 3) is three and a bit float32 tiles."""
import types

import numpy as np
import pytest
import torch

from test_gpu_actor import _weights

pytestmark = pytest.mark.gpu

NAMES = ("actions", "raw", "dist", "logp", "value", "counters")
DTYPES = pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
HIDDEN, N_OBS = (16, 16), 3


class _JetEnv(object):
    """what Actor(per_jet=True) reads of a VecShkadov: most tests need no film behind the observation rows"""
    _norm_on = False
    action_is_int = False

    def __init__(self, batch, n_jets, n_obs, dtype):
        from beacon_amd import spaces
        self.batch, self.n_jets, self.n_obs, self.obs_dim = batch, n_jets, n_obs, n_jets * n_obs
        self.tdtype, self.device = dtype, torch.device("cuda", torch.cuda.current_device())
        self.action_space = spaces.box(-1.0, 1.0, (n_jets,))
        self.obs = None


def _flat(rows, n_obs, dtype):
    """the twin's env: every (replica, jet) a replica of its own with one action component"""
    return _JetEnv(rows, 1, n_obs, dtype)


def _pair(B, A, off, dtype, n_obs=N_OBS, hidden=HIDDEN, seed=7):
    """(the per-jet actor, its flat twin): the same weights, the same seed, replica_offset against replica_offset A"""
    from beacon_amd import Actor
    a = Actor(_JetEnv(B, A, n_obs, dtype), hidden=hidden, seed=seed, replica_offset=off, per_jet=True)
    t = Actor(_flat(B * A, n_obs, dtype), hidden=hidden, seed=seed, replica_offset=off * A)
    pi, vf, ls = _weights(n_obs, hidden, 1, 2.0, 1)
    a.load(pi, vf, ls)
    t.load(pi, vf, ls)
    assert torch.equal(a.params, t.params) and (a.agents, a.rows, t.agents, t.rows) == (A, B * A, 1, B * A)
    return a, t


def _obs(B, A, n_obs, dtype, seed=3):
    return torch.as_tensor(np.random.default_rng(seed).uniform(-1.0, 1.0, (B, A * n_obs)), dtype=dtype).cuda()


def _same(a, t, what=""):
    for q in NAMES:
        va, vt = getattr(a, q), getattr(t, q)
        assert tuple(va.shape) == (a.batch, a.agents), (q, va.shape)
        assert torch.equal(va.reshape(-1), vt.reshape(-1)), (what, q)


# ---- 1. per-jet equals the flat twin ---------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("B,A,off", [(1, 1, 0), (13, 5, 0), (13, 5, 3), (7, 20, 0), (65, 3, 2)])
def test_per_jet_equals_the_flat_twin(B, A, off, dtype):
    a, t = _pair(B, A, off, dtype)
    obs = _obs(B, A, N_OBS, dtype)
    rows = obs.view(B * A, N_OBS)
    for call in range(2):
        acts = a.act(obs if call == 0 else rows)               # both shapes of an explicit obs are the same bytes
        t.act(rows)
        assert acts is a.actions and tuple(acts.shape) == (B, A)
        _same(a, t, "call %d" % call)
        assert a.counters.cpu().reshape(-1).tolist() == [call + 1] * (B * A)
        assert torch.equal(a.actions, a.raw.clamp(a.low, a.high))
    first = a.raw.clone()
    if B * A > 1:
        assert len(set(a.raw.reshape(-1).cpu().tolist())) == B * A                     # every row has a draw of its own
    a.act(obs, deterministic=True)
    t.act(rows, deterministic=True)
    _same(a, t, "deterministic")
    assert torch.equal(a.raw, a.dist) and not torch.equal(a.raw, first)
    assert a.counters.cpu().reshape(-1).tolist() == [2] * (B * A)                      # no draw, no tick
    assert torch.equal(a.values(rows), a.value.reshape(-1))


def test_a_plain_actor_still_refuses_twenty_jets():
    from beacon_amd import Actor
    with pytest.raises(ValueError, match="20 components"):
        Actor(_JetEnv(7, 20, N_OBS, torch.float32), hidden=HIDDEN)


# ---- 2. the mask is per replica ----------------------------------------------------------------------------------------------------
@DTYPES
def test_mask_is_per_replica(dtype):
    B, A = 13, 5
    a, t = _pair(B, A, 0, dtype)
    obs = _obs(B, A, N_OBS, dtype)
    rows = obs.view(B * A, N_OBS)
    a.act(obs)
    t.act(rows)
    before = {q: getattr(a, q).clone() for q in NAMES}
    mask = torch.ones(B, dtype=torch.uint8, device="cuda")
    mask[[2, 7, 12]] = 0                                        # replica 12: rows 60 .. 64, across the float32 tile edge
    a.act(obs, mask=mask)
    t.act(rows, mask=mask.repeat_interleave(A))
    _same(a, t, "masked")
    m = mask.bool()
    for q in NAMES:
        assert torch.equal(getattr(a, q)[~m], before[q][~m]), q                        # all five rows of a masked replica, bit for bit
    assert not torch.equal(a.raw[m], before["raw"][m])
    assert a.counters[m].cpu().reshape(-1).tolist() == [2] * (10 * A) and a.counters[~m].cpu().reshape(-1).tolist() == [1] * (3 * A)
    a.act(obs, mask=mask.bool())                                # a bool mask, and a host list, are the same per-replica bytes
    t.act(rows, mask=mask.repeat_interleave(A))
    _same(a, t, "bool mask")
    a.act(obs, mask=mask.cpu().tolist())
    t.act(rows, mask=mask.repeat_interleave(A))
    _same(a, t, "list mask")


# ---- 3. the default observations while the env normalises ---------------------------------------------------------------------------
@DTYPES
def test_default_obs_is_norm_obs_while_normalising(dtype):
    B, A = 13, 5
    a, t = _pair(B, A, 0, dtype)
    env = a.env
    env.obs = _obs(B, A, N_OBS, dtype, seed=4)
    env._norm = types.SimpleNamespace(norm_obs=_obs(B, A, N_OBS, dtype, seed=5))
    env._norm_on = True
    a.act()
    t.act(env._norm.norm_obs.view(B * A, N_OBS))
    _same(a, t, "norm_obs")
    normed = a.dist.clone()
    env._norm_on = False
    a.act()
    t.act(env.obs.view(B * A, N_OBS))
    _same(a, t, "obs")
    assert not torch.equal(a.dist, normed)


# ---- 4. the real env: rollout, eager against graph -------------------------------------------------------------------------------------
T_RO, B_RO, A_RO = 4, 13, 5
_RO = {}


def _rollout(dtype):
    """VecShkadov(13, n_jets=5) with per-jet rewards, a per-jet actor attached to its rollout, T = 4 steps run eagerly and then
    again from a one-step graph replayed four times.  Built once per dtype: {env, actor, ro, eager, graph, full}."""
    if dtype in _RO:
        return _RO[dtype]
    import beacon_amd
    from beacon_amd import Actor
    from beacon_amd.envs import packaged_init
    T = T_RO
    env = beacon_amd.VecShkadov(B_RO, "cuda:0", "f64" if dtype == torch.float64 else "f32", init_fields=packaged_init("shkadov"), n_jets=A_RO,
                                t_act=0.15, seed=5)              # episodes of two steps: the rollout crosses an auto-reset
    env.set_jet_rewards()
    actor = Actor(env, hidden=HIDDEN, seed=21, per_jet=True)
    pi, vf, ls = _weights(env.n_obs, HIDDEN, 1, 2.0, 9)
    actor.load(pi, vf, ls)
    ro = env.rollout(T)
    actor.attach(ro)

    def start():
        env.set_noise_seed(5)                                    # the inlet noise's counters back to 0
        actor.set_seed(21)
        env.episodes.clear()
        env.reset()
        actor.seq.zero_()
        ro.clear()
        ro.begin()

    def snap():
        return {"act": ro.act.clone(), "logp_seq": actor.logp_seq.clone(), "value_seq": actor.value_seq.clone(), "raw_seq": actor.raw_seq.clone(),
                "rwd_jets": ro.rwd_jets.clone(), "counters": actor.counters.clone(), "valid": ro.valid.clone(), "obs": ro.obs.clone()}

    start()
    per_step = []
    for _ in range(T):
        acts = actor.act()
        per_step.append((acts.clone(), actor.logp.clone(), actor.value.clone(), actor.raw.clone()))
        env.step_autoreset(acts)
    assert ro.check() == (T, False)
    eager = snap()
    seq = actor.seq.clone()
    actor.act()                                                  # the rollout is full: a further act writes no slot
    full = torch.equal(actor.seq, seq) and ro.check() == (T, False)
    start()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        env.step_autoreset(actor.act())
    for _ in range(T):
        g.replay()
    torch.cuda.synchronize()
    assert ro.check() == (T, False)
    _RO[dtype] = dict(env=env, actor=actor, ro=ro, eager=eager, graph=snap(), full=full, per_step=per_step)
    return _RO[dtype]


@DTYPES
def test_real_env_rollout_eager_equals_graph(dtype):
    r = _rollout(dtype)
    env, actor, ro, T, B, A = r["env"], r["actor"], r["ro"], T_RO, B_RO, A_RO
    assert (env.n_jets, actor.agents, actor.obs_dim, actor.rows) == (A, A, env.n_obs, B * A)
    assert tuple(actor.logp_seq.shape) == tuple(actor.value_seq.shape) == (T, B * A) and tuple(actor.raw_seq.shape) == (T, B * A, 1)
    assert tuple(ro.act.shape) == (T, B, A) and tuple(ro.rwd_jets.shape) == (T, B, A)
    for k, v in r["eager"].items():
        assert torch.equal(v, r["graph"][k]), k
    e = r["eager"]
    assert e["counters"].cpu().reshape(-1).tolist() == [T] * (B * A)
    assert torch.equal(e["act"].reshape(T, B * A), e["raw_seq"].reshape(T, B * A).clamp(actor.low, actor.high))     # the Box clip of every jet
    for t, (acts, logp, value, raw) in enumerate(r["per_step"]):                   # row t is what step t's act produced
        assert torch.equal(e["act"][t], acts) and torch.equal(e["logp_seq"][t], logp.reshape(-1))
        assert torch.equal(e["value_seq"][t], value.reshape(-1)) and torch.equal(e["raw_seq"][t].reshape(-1), raw.reshape(-1))
    assert float(e["rwd_jets"].abs().min()) > 0.0 and int(ro.done.sum()) >= B      # rewards were recorded, episodes ended
    assert r["full"]
    # the per-jet rows are what the flat twin computes from the recorded observations of step 0
    from beacon_amd import Actor
    twin = Actor(_flat(B * A, env.n_obs, dtype), hidden=HIDDEN, seed=21)
    twin.params.copy_(actor.params)
    twin.act(e["obs"][0].reshape(B * A, env.n_obs))
    assert torch.equal(twin.raw.reshape(-1), e["raw_seq"][0].reshape(-1)) and torch.equal(twin.logp, e["logp_seq"][0])
    # GAE takes the actor's shapes as they are
    last_value = actor.values(env.obs.view(-1, env.n_obs))
    final_values = actor.values(ro.final_obs.view(-1, env.n_obs))
    adv, ret = ro.compute_gae(actor.value_seq, last_value, final_values, per_jet=True)
    assert tuple(adv.shape) == tuple(ret.shape) == (T, B * A) == (4, 65)
    assert bool(torch.isfinite(adv).all()) and float(adv.abs().max()) > 0.0


# ---- 5. Learner.grad with one weight per replica ------------------------------------------------------------------------------------------
@DTYPES
def test_grad_with_rows_per_weight_equals_expanded_weights(dtype):
    from beacon_amd import Learner
    B, A, T = 13, 5, 4
    N, R = T * B * A, B * A
    a, t = _pair(B, A, 0, dtype)
    hp = dict(clip_range=0.2, vf_coef=0.5, ent_coef=0.01)
    la, lt = Learner(a, **hp), Learner(t, **hp)
    rng = np.random.default_rng(11)
    dev = lambda x, dt=dtype: torch.as_tensor(x, dtype=dt).cuda()
    obs, act = dev(rng.uniform(-1.0, 1.0, (N, N_OBS))), dev(rng.uniform(-1.5, 1.5, (N, 1)))
    logp_old, adv, ret = dev(rng.uniform(-2.0, -0.5, N)), dev(rng.normal(size=N)), dev(rng.normal(size=N))
    w8 = dev(rng.integers(0, 2, T * B), torch.uint8)
    w8[12] = 0                                                   # step 0's replica 12: the rows 60 .. 64 across the float32 tile edge
    wr = dev(rng.uniform(0.25, 2.0, T * B)) * w8.to(dtype)
    idx = dev(np.random.default_rng(12).permutation(N)[:150], torch.int32)
    cursor = dev([2, 0, 0, 0], torch.int32)                      # two of the four steps are recorded
    seen = []
    for weight, kw in ((w8, {}), (wr, {}), (w8, dict(idx=idx)), (wr, dict(idx=idx, _cursor=cursor, _rows_per_step=R)),
                       (w8.bool(), dict(_cursor=cursor, _rows_per_step=R)), (None, dict(idx=idx))):
        la.grad(obs, act, logp_old, adv, ret, weight=weight, rows_per_weight=A, **kw)
        lt.grad(obs, act, logp_old, adv, ret, weight=None if weight is None else weight.repeat_interleave(A), **kw)
        assert torch.equal(la.grad_buf, lt.grad_buf), kw                   # every gradient segment
        assert torch.equal(la.stats, lt.stats), kw                         # all eight statistics
        for name in la.grads:
            assert torch.equal(la.grads[name], lt.grads[name]), name
        st = la.stats_dict()
        assert st["grad_norm"] > 0.0 and st["weight"] > 0.0
        seen.append(st["weight"])
    assert seen[0] == float(w8.sum()) * A                        # every replica's byte counted once per jet
    assert seen[4] == float(w8[:2 * B].sum()) * A                # ... and only for the recorded steps under the cursor
    assert seen[5] == float((idx < N).sum())                     # no weight array: every selected row counts 1


# ---- 6. Learner.update -------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_update_equals_the_flat_twin_driven_by_hand(dtype):
    from beacon_amd import Actor, Learner
    r = _rollout(dtype)
    env, actor, ro, T, B, A = r["env"], r["actor"], r["ro"], T_RO, B_RO, A_RO
    R, N, epochs, nmb, seed = B * A, T * B * A, 2, 3, 1234
    hp = dict(lr=3e-4, clip_range=0.2, vf_coef=0.5, ent_coef=0.01, max_grad_norm=0.5, betas=(0.9, 0.999), eps=1e-5)
    ln = Learner(actor, **hp)
    # advantages of the whole-replica GAE are T B elements: not what a per-jet actor is updated with
    zeros = torch.zeros(T, B, dtype=dtype, device="cuda")
    adv1, ret1 = ro.compute_gae(zeros, zeros[0], zeros, per_jet=False)
    with pytest.raises(ValueError, match=r"compute_gae\(\.\.\., per_jet=True\)"):
        ln.update(ro, adv1, ret1)
    adv, ret = ro.compute_gae(actor.value_seq, actor.values(env.obs.view(-1, env.n_obs)), actor.values(ro.final_obs.view(-1, env.n_obs)), per_jet=True)
    twin = Actor(_flat(R, env.n_obs, dtype), hidden=HIDDEN, seed=21)
    twin.params.copy_(actor.params)
    lt = Learner(twin, **hp)
    before = actor.params.clone()
    gen = torch.Generator(device="cuda").manual_seed(seed)
    assert ln.update(ro, adv, ret, epochs=epochs, minibatches=nmb, generator=gen) is ln
    assert ro.check() == (T, False) and int(ln.step_count[0]) == epochs * nmb

    # the twin, by hand: the plain path's rows, the valid bytes expanded to one per row, the same permutations
    obs, raw, logp_old = ro.obs[:-1].reshape(N, env.n_obs), actor.raw_seq.reshape(N, 1), actor.logp_seq.reshape(N)
    valid = ro.valid.view(T, B).repeat_interleave(A, dim=1).contiguous().reshape(N)
    assert int(ro.valid.sum()) == T * B
    a1, r1 = adv.reshape(N), ret.reshape(N)
    steps = torch.arange(T, device="cuda", dtype=torch.int32).view(T, 1)
    w = (valid.view(T, R) * (steps < ro.cursor[0])).reshape(N).to(dtype)                # Learner.update's standardisation, on N rows
    cnt = w.sum().clamp_(min=1.0)
    mean = (torch.where(w > 0, a1, torch.zeros_like(a1))).sum() / cnt
    var = (torch.where(w > 0, a1 - mean, torch.zeros_like(a1)) ** 2).sum() / (cnt - 1.0).clamp_(min=1.0)
    a1 = (a1 - mean) / (var.sqrt() + 1e-8)
    assert float(cnt) == N                                       # the pool: every valid step counts once per jet
    gen2 = torch.Generator(device="cuda").manual_seed(seed)
    for _ in range(epochs):
        perm = torch.randperm(N, device="cuda", generator=gen2).to(torch.int32)
        for k in range(nmb):
            lt.grad(obs, raw, logp_old, a1, r1, weight=valid, idx=perm[k * N // nmb:(k + 1) * N // nmb], _cursor=ro.cursor, _rows_per_step=R)
            lt.step()
    assert torch.equal(actor.params, twin.params) and torch.equal(ln.opt, lt.opt)
    assert torch.equal(ln.stats, lt.stats)
    assert not torch.equal(actor.params, before)                 # the comparison is of an update that happened
