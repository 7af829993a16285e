"""The on-device actor's sampler where tests/test_gpu_actor.py does not take it, on the MI355X: both tails of Box-Muller on draws
built on purpose (tests/actor_draws.py), a key with a non-zero high word, a global replica index and a draw counter that wrap at
2^32, per-row counters, categorical classes rarer than that module's exemption, mask and deterministic mode under an attached
rollout, other Box bounds, and non-finite observation rows next to healthy ones.  tests/test_actor_draws_host.py checks on the CPU
that the constructed draws are what these tests take them for.

The references, the weights and the case-wide error metric err(q) = max |device - reference| / max(1, max |reference|) with F32_TOL /
F64_TOL are those of tests/test_gpu_actor.py.  The tail test has a metric of its own, per element and relative to the radius."""
import numpy as np
import pytest
import torch

import actor_draws as D
import actor_ref as R
import test_gpu_actor as T

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
NAMES = ("actions", "raw", "logp", "value", "dist", "counters")

# test_gaussian_tails_exact_z.  float64: both sides take the log of the same double u1; a handful of 2^-53 roundings remain (the log,
# the square root, the angle 2 pi u2 <= 2 pi formed on the reference's side, sine / cosine, the product): about 10 x headroom.
TAIL_F64_TOL = 1e-13
# float32, against the float64 reference: (tolerance, worst measured on the MI355X over the 128 rows x 2 components); at most 10 x.
# z: |raw - z_ref| / radius_ref per element; logp: |logp - logp_ref| / max(1, |logp_ref|) per row.  The CPU emulation of the header's
# formula with correctly rounded functions gives 1.0e-7 for z (tests/test_actor_draws_host.py).  A library built for the experiment
# with logf(u1) in the branch k >= 2^23 measured z = 0.150 here -- and passed every case of tests/test_gpu_actor.py.
TAIL_F32_TOL = {"z": (1.0e-6, 1.079e-7), "logp": (2.3e-6, 2.376e-7)}


def _np(dtype):
    return np.float64 if dtype == torch.float64 else np.float32


def _tol(dtype):
    return (lambda q: T.F64_TOL) if dtype == torch.float64 else (lambda q: T.F32_TOL[q][0])


class _BoxEnv(T._Env):
    """a Gaussian env with bounds of its own"""

    def __init__(self, batch, obs_dim, n, dtype, low, high):
        from beacon_amd import spaces
        super().__init__(batch, obs_dim, "gaussian", n, dtype)
        self.action_space = spaces.box(low, high, (n,))


def _build(env, hidden=(5,), activation="tanh", scale=1.0, wseed=1, seed=D.SEED, replica_offset=D.OFFSET):
    """an actor on `env` with the weights of test_gpu_actor._weights, keyed and offset as the constructed draws are"""
    from beacon_amd import Actor
    a = Actor(env, hidden=hidden, activation=activation, seed=seed, replica_offset=replica_offset)
    pi, vf, ls = T._weights(env.obs_dim, hidden, a.act_dim, scale, wseed)
    a.load(pi, vf, ls if a.kind == 0 else None)
    return a


def _stored(a):
    """the weights as the device holds them now, in float64: what the reference is fed"""
    back = lambda net: [(a.weights["%s_w%d" % (net, l)].double().cpu().numpy(), a.weights["%s_b%d" % (net, l)].double().cpu().numpy())
                        for l in range(len(a.hidden) + 1)]
    return back("pi"), back("vf"), a.weights["log_std"].double().cpu().numpy()


def _zero_policy(a):
    for name, t in a.weights.items():
        if name.startswith("pi_") or name == "log_std":
            t.zero_()


def _set_counters(a, ctr):
    """per-row counters through the int32 view (2^32 - 1 is written as -1)"""
    a.counters.copy_(torch.tensor(np.asarray(ctr, dtype=np.int64).astype(np.uint32).view(np.int32).copy()))


def _counters(a):
    return a.counters.cpu().numpy().view(np.uint32).astype(np.int64)


def _errs(a, ref, names):
    errs = {q: T._err(getattr(a, q), ref[q]) for q in names if q != "z"}
    if "z" in names:
        errs["z"] = T._err((a.raw - a.dist) / torch.exp(a.weights["log_std"]), ref["z"])
    return errs


def _check(errs, dtype, what):
    print("actor edges %s %s: %s" % (what, "f64" if dtype == torch.float64 else "f32", " ".join("%s=%.3e" % kv for kv in sorted(errs.items()))))
    for q, e in errs.items():
        tol = _tol(dtype)("raw" if q == "actions" else q)                    # a Gaussian action is raw or a bound
        assert e <= tol, (what, q, e, tol)


@DTYPES
def test_gaussian_tails_exact_z(dtype):
    """Radii of 4.5 .. 5.9 on the even rows and 4e-4 .. 9e-3 on the odd rows, with a zero policy network and log_std = 0: the mean is
    exactly 0 and raw IS z, so no cancellation and no larger entry of the case hides an error of the radius.  Then a second call on
    ordinary draws at every row's own counter + 1."""
    ctr = D.extreme_counters()
    rows = np.arange(D.B)
    a = _build(T._Env(D.B, 3, "gaussian", 2, dtype))
    _zero_policy(a)
    obs = T._obs(D.B, 3, dtype)
    _set_counters(a, ctr)
    z_ref = R.normals(D.SEED, D.OFFSET, rows, ctr, 2, _np(dtype))
    radius = D.pair0(ctr, _np(dtype))[2]
    logp_ref = (-0.5 * z_ref * z_ref - R.HALF_LN_2PI).sum(axis=1)
    assert radius[0::2].min() >= 4.0 and radius[1::2].max() <= 1e-2           # the draws are what they were built to be
    acts = a.act(obs)
    assert torch.equal(a.dist, torch.zeros_like(a.dist))
    raw, logp = a.raw.double().cpu().numpy(), a.logp.double().cpu().numpy()
    ez = np.abs(raw - z_ref) / radius[:, None]
    el = np.abs(logp - logp_ref) / np.maximum(1.0, np.abs(logp_ref))
    print("actor tails %s: z even rows %.3e, odd rows %.3e; logp even rows %.3e, odd rows %.3e"
          % ("f64" if dtype == torch.float64 else "f32", ez[0::2].max(), ez[1::2].max(), el[0::2].max(), el[1::2].max()))
    tz, tl = (TAIL_F64_TOL, TAIL_F64_TOL) if dtype == torch.float64 else (TAIL_F32_TOL["z"][0], TAIL_F32_TOL["logp"][0])
    assert ez.max() <= tz, (ez.max(), tz)                                    # the worst element / the worst row: each one is held
    assert el.max() <= tl, (el.max(), tl)
    assert acts is a.actions and torch.equal(acts, a.raw.clamp(-1.0, 1.0))
    assert (acts != a.raw).any(dim=1)[0::2].all()                            # a radius >= 4 leaves the Box in at least one component
    assert torch.equal(acts[1::2], a.raw[1::2])                              # a radius <= 1e-2 never does
    assert np.array_equal(_counters(a), ctr + 1)
    # ordinary draws, every row at another counter: a launch that read one counter for all rows, or a row's neighbour's, fails here
    assert len(set(ctr.tolist())) > D.B // 2
    a.act(obs)
    ref = T._ref(a, _stored(a), obs, ctr + 1)
    assert np.array_equal(_counters(a), ctr + 2)
    _check(_errs(a, ref, ("raw", "logp", "z")), dtype, "tails, second call")


@DTYPES
def test_key_words_index_wrap_and_counter_wrap(dtype):
    """The setup of the tail test with trained-size weights and five components (an unused half pair): seed_hi != 0, the global index
    wraps at row 3, and row 7 draws at counter 2^32 - 1 and then at 0."""
    ctr = np.array(D.extreme_counters())
    ctr[7] = 0xFFFFFFFF
    a = _build(T._Env(D.B, 6, "gaussian", 5, dtype))
    w = _stored(a)
    obs = T._obs(D.B, 6, dtype)
    _set_counters(a, ctr)
    assert int(a.counters[7]) == -1
    a.act(obs)
    first = a.raw.clone()
    _check(_errs(a, T._ref(a, w, obs, ctr), ("dist", "value", "raw", "logp", "z")), dtype, "keys and wraps")
    assert torch.equal(a.actions, a.raw.clamp(a.low, a.high))
    after = (ctr + 1) & 0xFFFFFFFF
    assert after[7] == 0 and np.array_equal(_counters(a), after)
    a.act(obs)
    ref = T._ref(a, w, obs, after)
    _check(_errs(a, ref, ("raw", "logp", "z")), dtype, "keys and wraps, second call")
    tol = _tol(dtype)("raw")
    assert T._err(a.raw[7:8], ref["raw"][7:8]) <= tol                        # row 7 by itself, at counter 0
    assert np.array_equal(_counters(a), after + 1)
    # the high key word reaches the generator: the same low word under seed_hi = 0 is another stream (and matches its own reference)
    lo = _build(T._Env(D.B, 6, "gaussian", 5, dtype), seed=D.SEED & 0xFFFFFFFF)
    assert lo.seed >> 32 == 0 and lo.seed & 0xFFFFFFFF == a.seed & 0xFFFFFFFF and torch.equal(lo.params, a.params)
    _set_counters(lo, ctr)
    lo.act(obs)
    assert not torch.equal(lo.raw, first)
    assert T._err(lo.raw, first.double().cpu().numpy()) > 1e-3
    _check(_errs(lo, T._ref(lo, w, obs, ctr), ("raw", "logp", "z")), dtype, "seed_hi = 0")
    # ... and so does the offset: without it, rows 3 .. draw what rows 0 .. of an unsharded batch draw, not what they drew above
    un = _build(T._Env(D.B, 6, "gaussian", 5, dtype), replica_offset=0)
    _set_counters(un, ctr)
    un.act(obs)
    assert T._err(un.raw, first.double().cpu().numpy()) > 1e-3
    _check(_errs(un, T._ref(un, w, obs, ctr), ("raw", "logp", "z")), dtype, "replica_offset = 0")


@DTYPES
def test_categorical_tails(dtype):
    """Four classes of probability (2^-17, 1/2, 1/2 - 2^-16, 2^-17) from the head's bias alone, on the counters whose uniform is
    smallest (even rows) or largest (odd rows): the first class is drawn although it is rarer than test_gpu_actor.DELTA is wide, and
    the last class takes the remainder."""
    ctr = D.extreme_counters()
    a = _build(T._Env(D.B, 3, "categorical", 4, dtype))
    _zero_policy(a)
    a.weights["pi_b%d" % len(a.hidden)].copy_(torch.tensor(np.log(np.array(D.TAIL_P)), dtype=dtype))
    obs = T._obs(D.B, 3, dtype)
    _set_counters(a, ctr)
    ref = T._ref(a, _stored(a), obs, ctr)                                    # fed the device's stored bias
    near = (np.abs(ref["u"][:, None] - ref["cum"]) <= D.DELTA_TAIL).any(axis=1)
    counts = np.bincount(ref["actions"][~near], minlength=4)
    # the reference alone, before the device is read: the exemption is rare enough to rely on, and every class is still checked
    assert near.mean() <= D.CAP_TAIL, near.mean()
    assert counts.min() >= 17, counts
    a.act(obs)
    dev = a.actions.cpu().numpy()
    assert ((dev >= 0) & (dev < 4)).all()
    assert np.array_equal(dev[~near], ref["actions"][~near])
    assert torch.equal(a.logp, a.dist.gather(1, a.actions.long()[:, None])[:, 0])     # logp == dist[action] exactly
    assert {0, 3} <= set(dev.tolist())
    assert np.array_equal(_counters(a), ctr + 1)
    _check(_errs(a, ref, ("dist", "raw", "value")), dtype, "categorical tails")


@DTYPES
def test_mask_and_deterministic_under_attached_rollout(dtype):
    import beacon_amd
    from beacon_amd import Actor
    B, Tn, SENT = 65, 3, -777.0
    env = beacon_amd.VecLorenz(B, dtype="f64" if dtype == torch.float64 else "f32")
    actor = Actor(env, hidden=(5,), seed=D.SEED, replica_offset=D.OFFSET)
    pi, vf, _ = T._weights(env.obs_dim, (5,), actor.act_dim, 2.0, 9)
    actor.load(pi, vf)
    ro = env.rollout(Tn)
    actor.attach(ro)
    env.reset()
    ro.clear()
    ro.begin()
    seqs = (("logp_seq", "logp"), ("value_seq", "value"), ("raw_seq", "raw"))
    for s, _ in seqs:
        getattr(actor, s).fill_(SENT)
    mask = torch.as_tensor(np.random.default_rng(5).integers(0, 2, B), dtype=torch.uint8).cuda()
    mask[0], mask[1], mask[63], mask[64] = 1, 0, 1, 0
    m = mask.bool()
    acts = actor.act(mask=mask)                                              # t = 0
    for s, q in seqs:
        seq, out = getattr(actor, s), getattr(actor, q)
        assert torch.equal(seq[0][m], out[m]) and not (seq[0][m] == SENT).any(), s
        assert (seq[0][~m] == SENT).all(), s                                 # a masked replica writes no slot either
        assert (seq[1:] == SENT).all(), s
    for q in NAMES:
        assert not getattr(actor, q)[~m].any(), q                            # ... and no state row: still the zeros of a new actor
    assert actor.counters[m].cpu().tolist() == [1] * int(m.sum())
    env.step_autoreset(acts)
    assert ro.check() == (1, False)
    row0 = [getattr(actor, s)[0].clone() for s, _ in seqs]
    before = actor.counters.clone()
    actor.act(deterministic=True)                                            # t = 1: every row, no draw
    assert torch.equal(actor.counters, before)
    assert torch.equal(actor.actions.long(), actor.dist.argmax(dim=1)) and torch.equal(actor.logp, actor.dist.max(dim=1).values)
    for (s, q), old in zip(seqs, row0):
        seq = getattr(actor, s)
        assert torch.equal(seq[1], getattr(actor, q)) and not (seq[1] == SENT).any(), s
        assert torch.equal(seq[0], old) and (seq[2] == SENT).all(), s
    env.close()


@DTYPES
@pytest.mark.parametrize("low,high", [(-0.25, 0.75), (0.5, 0.5)], ids=["asym", "degenerate"])
def test_box_bounds(low, high, dtype):
    """actions == clamp(raw, low, high) exactly for a Box that is not +-1 and for low == high; raw and logp match the reference, which
    gets the same bounds: logp is the density of the UNCLIPPED sample."""
    B, n = 65, 3
    a = _build(_BoxEnv(B, 4, n, dtype, low, high))
    assert (a.low, a.high) == (low, high)
    w = _stored(a)
    obs = T._obs(B, 4, dtype)
    a.act(obs)
    ref = T._ref(a, w, obs, np.zeros(B))
    assert torch.equal(a.actions, a.raw.clamp(low, high))
    assert (a.actions == low).any() and (a.actions == high).any() and (a.raw < low).any() and (a.raw > high).any()
    if low < high:
        assert ((a.actions > low) & (a.actions < high)).any()
    else:
        assert (a.actions == low).all()
    _check(_errs(a, ref, ("dist", "raw", "logp", "z", "actions")), dtype, "box [%g, %g]" % (low, high))
    # the density of the clipped action would be told apart: on the rows that were clipped it is another number altogether
    acts, raw, logp = (getattr(a, q).double().cpu().numpy() for q in ("actions", "raw", "logp"))
    clipped = (acts != raw).any(axis=1)
    z_clip = (acts - ref["dist"]) / np.exp(w[2])
    lp_clip = (-0.5 * z_clip * z_clip - w[2] - R.HALF_LN_2PI).sum(axis=1)
    assert clipped.sum() >= B // 2 and np.median(np.abs(lp_clip - logp)[clipped]) > 0.1


@DTYPES
@pytest.mark.parametrize("kind,n", [("gaussian", 3), ("categorical", 4)])
def test_non_finite_rows_stay_in_their_rows(kind, n, dtype):
    """Rows 1 and 64 NaN, row 2 +-inf: rows 0 and 3 share a lane's four-replica register chunk with them, row 64 is the one valid
    row of the last tile.  Every other row of every output is bit for bit what the clean run writes."""
    B = 65
    clean, bad = (_build(T._Env(B, 6, kind, n, dtype)) for _ in range(2))
    obs = T._obs(B, 6, dtype)
    pobs = obs.clone()
    pobs[1], pobs[64] = float("nan"), float("nan")
    pobs[2, 0::2], pobs[2, 1::2] = float("inf"), float("-inf")
    keep = torch.ones(B, dtype=torch.bool, device="cuda")
    keep[[1, 2, 64]] = False
    for deterministic in (False, True):
        clean.act(obs, deterministic=deterministic)
        bad.act(pobs, deterministic=deterministic)
        for q in NAMES:
            vc, vb = getattr(clean, q), getattr(bad, q)
            assert torch.isfinite(vc.double()).all(), q
            assert torch.equal(vb[keep], vc[keep]), (q, deterministic)
        if kind == "categorical":
            assert ((bad.actions >= 0) & (bad.actions < n)).all(), deterministic
        assert bad.counters.cpu().tolist() == [1] * B                         # the poisoned rows tick too; deterministic mode ticks none
    assert not torch.isfinite(bad.value[[1, 2, 64]]).all()                    # the poison did reach the networks
