"""Running normalisation of observations and rewards on the GPU: VecEnv.set_normalize / normalize_outputs / normalizer
(csrc/normalize.hip, include/beacon_hip.h: bcn_normalize).  The yardstick is `Ref` below, a float64 NumPy restatement of the
formulas of the header, fed the values the kernel reads, upcast exactly from the env's dtype.  The kernel is compared with itself
only where the claim is determinism.

Tolerances (derived, not measured; tests/test_normalize_host.py checks `Ref` against numpy.longdouble on the hardest column):
  counts     exact
  means      1e-12 of the column's largest |x|: a float64 sum of n terms errs by about log2(n) 2^-53 relative to that
  variances  rtol 1e-7: a deviation-based float64 reduction over <= 4096 samples errs by at most about n 2^-53 |mean| / std =
             4.5e-8 on the cancellation column (|mean| / std = 1e5), the sum-of-squares form by at least 2^-53 (mean / std)^2 = 1e-6
  outputs    absolute 2e-6 (float32: two ulps at the clip bound 10, for one rounding of a float64 result) and 1e-6 (float64: the
             variance tolerance carried to |y| <= 10).  An element whose reference lies that close to a clip bound may land on
             either side of it and still passes; none is left out."""
import numpy as np
import pytest
import torch

from beacon_amd import vec as V
from beacon_amd import _lib
from beacon_amd.envs import packaged_init

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NP = {"f32": np.float32, "f64": np.float64}
OUT_TOL = {"f32": 2e-6, "f64": 1e-6}
STATS = ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count")
PUBLIC = STATS + ("ret", "norm_obs", "norm_rwd", "norm_final_obs")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")


def make(case, B, dtype):
    if case == "rayleigh":
        return V.VecRayleigh(B, DEV, dtype, init_fields=packaged_init("rayleigh"))          # the built-in 50x50 grid: rows of 192 reals
    return {"burgers": V.VecBurgers, "lorenz": V.VecLorenz, "shkadov": V.VecShkadov}[case](B, DEV, dtype)


class Ref(object):
    """bcn_normalize in NumPy float64 (include/beacon_hip.h)."""

    def __init__(self, B, n, gamma=0.99, eps=1e-8, clip_obs=10.0, clip_rwd=10.0):
        self.gamma, self.eps, self.clip_obs, self.clip_rwd = gamma, eps, clip_obs, clip_rwd
        self.obs_mean, self.obs_var, self.obs_count = np.zeros(n), np.ones(n), np.zeros(1)
        self.ret_mean, self.ret_var, self.ret_count = np.zeros(1), np.ones(1), np.zeros(1)
        self.ret = np.zeros(B)
        self.norm_obs, self.norm_rwd, self.norm_final_obs = np.zeros((B, n)), np.zeros(B), np.zeros((B, n))
        self.obs_max, self.ret_max = np.zeros(n), 0.0          # the largest |x| that was counted, for the tolerance of the means

    @staticmethod
    def _merge(mean, var, count, x):
        n = x.shape[0]
        if n == 0:
            return mean, var, count
        mb = x.mean(axis=0)
        m2 = ((x - mb) ** 2).sum(axis=0)                       # from deviations
        d, tot = mb - mean, count + n
        return mean + d * n / tot, (var * count + m2 + d * d * count * n / tot) / tot, tot

    def __call__(self, obs, rwd, status, done, trunc, mask=None, kind="step", training=True, finished=None, final_obs=None):
        obs, rwd = np.asarray(obs).astype(np.float64), np.asarray(rwd).astype(np.float64)          # exact upcasts
        B = obs.shape[0]
        on = np.ones(B, dtype=bool) if mask is None else np.asarray(mask) != 0
        S = on & ((np.asarray(status) & (_lib.ST_ITMAX | _lib.ST_BLOWUP)) == 0) if kind == "step" else on
        with np.errstate(invalid="ignore"):
            if training:
                self.obs_mean, self.obs_var, self.obs_count = self._merge(self.obs_mean, self.obs_var, self.obs_count, obs[S])
                if S.any():
                    self.obs_max = np.maximum(self.obs_max, np.abs(obs[S]).max(axis=0))
                if kind == "step":
                    self.ret[on] = self.gamma * self.ret[on] + rwd[on]
                    self.ret_mean, self.ret_var, self.ret_count = self._merge(self.ret_mean, self.ret_var, self.ret_count, self.ret[S][:, None])
                    if S.any():
                        self.ret_max = max(self.ret_max, float(np.abs(self.ret[S]).max()))
            apply = lambda x: np.clip((x - self.obs_mean) / np.sqrt(self.obs_var + self.eps), -self.clip_obs, self.clip_obs)
            self.norm_obs[on] = apply(obs[on])
            if kind == "step":
                self.norm_rwd[on] = np.clip(rwd[on] / np.sqrt(self.ret_var[0] + self.eps), -self.clip_rwd, self.clip_rwd)
                if training:
                    self.ret[on & ((np.asarray(done) | np.asarray(trunc)) != 0)] = 0.0
                if finished is not None:
                    f = on & (np.asarray(finished) != 0)
                    self.norm_final_obs[f] = apply(np.asarray(final_obs).astype(np.float64)[f])     # never counted
            elif training:
                self.ret[on] = 0.0
        return self


def host(t):
    return t.detach().cpu().numpy()


def assert_follows(nz, ref, dtype, where=""):
    """every public segment of the Normalizer against the reference, within the tolerances of the module docstring"""
    assert float(nz.obs_count[0]) == ref.obs_count[0] and float(nz.ret_count[0]) == ref.ret_count[0], (where, "counts")
    err = np.abs(host(nz.obs_mean) - ref.obs_mean)
    assert (err <= 1e-12 * np.maximum(ref.obs_max, 1e-300)).all(), (where, "obs_mean", err.max())
    err = abs(float(nz.ret_mean[0]) - ref.ret_mean[0])
    assert err <= 1e-12 * max(ref.ret_max, 1e-300), (where, "ret_mean", err)
    for name in ("obs_var", "ret_var"):
        got, want = host(getattr(nz, name)), getattr(ref, name)
        assert np.isfinite(got).all() and np.allclose(got, want, rtol=1e-7, atol=0.0), (where, name, np.abs(got / want - 1).max())
    got = host(nz.ret)
    assert np.allclose(got, ref.ret, rtol=1e-14, atol=1e-14 * max(ref.ret_max, 1e-300), equal_nan=True), (where, "ret")
    for name in ("norm_obs", "norm_rwd", "norm_final_obs"):
        got, want = host(getattr(nz, name)).astype(np.float64), getattr(ref, name)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (where, name, "NaN pattern")
        err = np.nan_to_num(np.abs(got - want), nan=0.0)
        assert (err <= OUT_TOL[dtype]).all(), (where, name, err.max())


def public(nz):
    return {name: getattr(nz, name).clone() for name in PUBLIC}


def synth(rng, B, n, dtype, factor):
    """one call's inputs in the env dtype: column 0 the cancellation case 1e3 + 1e-2 N(0, 1), column 1 constant, the others
    N(0, 1) times scales from 1e-3 to 1e3 (times `factor`)"""
    x = rng.standard_normal((B, n)) * np.logspace(-3, 3, n) * factor
    x[:, 0] = 1e3 + 1e-2 * rng.standard_normal(B)
    x[:, 1] = 0.5
    rwd = rng.standard_normal(B) * 1e-2 * factor
    done = (rng.random(B) < 0.2).astype(np.uint8)
    trunc = (rng.random(B) < 0.1).astype(np.uint8)
    return x.astype(NP[dtype]), rwd.astype(NP[dtype]), np.zeros(B, dtype=np.int32), done, trunc


def feed(env, x, rwd, status, done, trunc):
    for view, a in ((env.obs, x), (env.rwd, rwd), (env.status, status), (env.done, done), (env.trunc, trunc)):
        view.copy_(torch.from_numpy(a).to(DEV).view_as(view))


# ---- 1. synthetic inputs: every shape, both dtypes ------------------------------------------------------------------------------
# lorenz: 42 replicas of 6 reals per trip, slabs of at least 168 replicas: 505 = 3 * 168 + 1 is the first batch with three slabs,
# uneven ones (169, 169, 167); 4096 has 24.  burgers (5 reals, 51 replicas per trip): a single replica, either side of a wavefront, four slabs.  shkadov: rows of
# 50 reals, 5 replicas per trip.  rayleigh: rows of 192 reals as three chunks of 64 columns.
SHAPES = [("burgers", 1), ("burgers", 63), ("burgers", 65), ("burgers", 1000), ("lorenz", 4096), ("lorenz", 505), ("shkadov", 130),
          ("rayleigh", 3)]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("case,B", SHAPES)
def test_five_calls_on_synthetic_inputs_follow_the_reference(case, B, dtype):
    _need_gpu()
    env = make(case, B, dtype).set_normalize()
    nz, n = env.normalizer, env.obs_dim
    ref = Ref(B, n)
    rng = np.random.default_rng(1000 + B)
    for k in range(5):
        x, rwd, status, done, trunc = synth(rng, B, n, dtype, (1.0, 1.0, 1.0, 1.0, 0.02)[k])
        mask = None
        if k == 1:
            mask = np.zeros(B, dtype=np.uint8)                               # nobody: nothing may change
        elif k == 2:
            mask = np.zeros(B, dtype=np.uint8)
            mask[B // 2] = 1                                                 # a single replica
        elif k == 3:
            mask = (rng.random(B) < 0.6).astype(np.uint8)
            bad = np.nonzero(mask)[0][:2] if B > 2 else np.zeros(0, dtype=np.int64)
            status[bad] = _lib.ST_BLOWUP                                     # two blown-up replicas with NaN rows: stepped, never counted
            x[bad], rwd[bad], done[bad] = np.nan, np.nan, 1
            hot = np.nonzero(mask)[0][2:3]                                   # one counted replica a million times off: with N samples
            x[hot, 2:] *= NP[dtype](1e6)                                     # counted so far its outputs are near sqrt(N), past the clip
        elif k == 4 and B > 1:
            status[B - 1] = _lib.ST_ITMAX
            x[B - 1, 2:] = 1e30                                              # finite, and never counted either
        feed(env, x, rwd, status, done, trunc)
        before = public(nz)
        assert env.normalize_outputs(mask) is nz
        ref(x, rwd, status, done, trunc, mask)
        if k == 1:
            for name in PUBLIC:
                assert torch.equal(getattr(nz, name), before[name]), (name, "changed under an all-zero mask")
        assert_follows(nz, ref, dtype, "call %d" % k)
        for name in STATS:
            assert bool(torch.isfinite(getattr(nz, name)).all()), (k, name)
    hit = np.abs(ref.norm_obs) == 10.0
    if B >= 130:
        assert hit.any() and not hit.all()                                   # some outputs sit on the clip (the ITMAX row; call 3: `hot`)
    assert np.abs(ref.norm_obs[:, 1]).max() <= OUT_TOL[dtype]                # the constant column: variance 0, output 0, no NaN
    assert float(nz.obs_var[1]) == 0.0
    env.close()


# ---- 2. modes -------------------------------------------------------------------------------------------------------------------
def _two_calls(env, ref, rng, dtype):
    for k in range(2):
        inp = synth(rng, env.batch, env.obs_dim, dtype, 1.0)
        feed(env, *inp)
        env.normalize_outputs()
        ref(*inp)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_reset_kind_touches_observation_statistics_only(dtype):
    _need_gpu()
    B = 300
    env = make("lorenz", B, dtype).set_normalize(gamma=0.9)
    nz, ref, rng = env.normalizer, Ref(B, env.obs_dim, gamma=0.9), np.random.default_rng(3)
    _two_calls(env, ref, rng, dtype)
    x, rwd, status, done, trunc = synth(rng, B, env.obs_dim, dtype, 2.0)
    mask = (rng.random(B) < 0.3).astype(np.uint8)
    status[np.nonzero(mask)[0][:3]] = _lib.ST_BLOWUP                         # the status row is stale in a reset: ignored
    feed(env, x, rwd, status, done, trunc)
    before = public(nz)
    env.normalize_outputs(mask, kind="reset")
    ref(x, rwd, status, done, trunc, mask, kind="reset")
    for name in ("ret_mean", "ret_var", "ret_count", "norm_rwd", "norm_final_obs"):
        assert torch.equal(getattr(nz, name), before[name]), name
    m = torch.from_numpy(mask).to(DEV) != 0
    assert bool((nz.ret[m] == 0).all()) and torch.equal(nz.ret[~m], before["ret"][~m])
    assert torch.equal(nz.norm_obs[~m], before["norm_obs"][~m])
    assert float(nz.obs_count[0]) == float(before["obs_count"][0]) + int(mask.sum())
    assert_follows(nz, ref, dtype, "reset")
    with pytest.raises(ValueError, match="kind"):
        env.normalize_outputs(kind="rest")
    env.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kind", ["step", "reset"])
def test_evaluation_mode_changes_no_statistics(kind, dtype):
    _need_gpu()
    B = 65
    env = make("burgers", B, dtype).set_normalize()
    nz, ref, rng = env.normalizer, Ref(B, env.obs_dim), np.random.default_rng(4)
    _two_calls(env, ref, rng, dtype)
    nz.training = False
    inp = synth(rng, B, env.obs_dim, dtype, 3.0)
    mask = (rng.random(B) < 0.7).astype(np.uint8)
    feed(env, *inp)
    before = public(nz)
    env.normalize_outputs(mask, kind=kind)
    ref(*inp, mask=mask, kind=kind, training=False)
    for name in STATS + ("ret",):
        assert torch.equal(getattr(nz, name), before[name]), name
    assert not torch.equal(nz.norm_obs, before["norm_obs"])
    assert_follows(nz, ref, dtype, "evaluation")
    env.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_state_dict_round_trip_continues_bit_for_bit(dtype):
    _need_gpu()
    B = 65
    A, C = make("burgers", B, dtype).set_normalize(gamma=0.95, clip_obs=5.0), make("burgers", B, dtype).set_normalize()
    rng = np.random.default_rng(5)
    _two_calls(A, Ref(B, A.obs_dim), rng, dtype)
    C.normalizer.load_state_dict(A.normalizer.state_dict())
    assert (C.normalizer.gamma, C.normalizer.clip_obs) == (0.95, 5.0)
    inp = synth(rng, B, A.obs_dim, dtype, 1.0)
    for env in (A, C):
        feed(env, *inp)
        env.normalize_outputs()
    assert torch.equal(A.normalizer.buf, C.normalizer.buf)
    assert float(C.normalizer.obs_count[0]) == 3 * B
    with pytest.raises(ValueError, match="Normalizer.load_state_dict"):
        make("burgers", B + 1, dtype).set_normalize().normalizer.load_state_dict(A.normalizer.state_dict())
    A.close(), C.close()


# ---- 3. integration -------------------------------------------------------------------------------------------------------------
def actions(env, n, seed):
    g = torch.Generator().manual_seed(seed)
    if env.action_is_int:
        return torch.randint(0, 3, (n, env.batch), generator=g, dtype=torch.int32).to(DEV)
    shape = (n, env.batch) if env.n_actions == 1 else (n, env.batch, env.n_actions)
    return (2.0 * torch.rand(shape, generator=g, dtype=torch.float64) - 1.0).to(device=DEV, dtype=env.tdtype)


def raw(env):
    return host(env.obs), host(env.rwd), host(env.status), host(env.done), host(env.trunc)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("case,B", [("burgers", 64), ("lorenz", 257)])
def test_step_with_the_feature_on_leaves_the_env_as_it_was(case, B, dtype):
    """three step()s beside a twin without the feature: the raw outputs and the state are equal bit for bit, what reset() and
    step() return are the normaliser's tensors, and those follow the reference fed the raw outputs"""
    _need_gpu()
    env, twin = make(case, B, dtype).set_normalize(), make(case, B, dtype)
    nz, ref = env.normalizer, Ref(B, env.obs_dim)
    assert not twin._norm_on and twin._norm is None
    acts = actions(env, 3, 8)
    obs, _ = env.reset()
    twin.reset()
    assert obs is nz.norm_obs and torch.equal(env.obs, twin.obs)
    ref(*raw(env), kind="reset")
    assert_follows(nz, ref, dtype, "reset")
    for k in range(3):
        obs, rwd, done, trunc, _ = env.step(acts[k])
        twin.step(acts[k])
        assert obs is nz.norm_obs and rwd is nz.norm_rwd and done is env.done and trunc is env.trunc
        for name in ("obs", "rwd", "done", "trunc", "status"):
            assert torch.equal(getattr(env, name), getattr(twin, name)), (k, name)
        assert torch.equal(env.get_state(), twin.get_state()), k
        ref(*raw(env))
        assert_follows(nz, ref, dtype, "step %d" % k)
    assert float(nz.obs_count[0]) == 4 * B
    env.set_normalize(False)
    assert env.step(acts[0])[0] is env.obs                                   # off again: the raw tensors
    with pytest.raises(AttributeError, match="set_normalize"):
        env.normalizer
    env.close(), twin.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("case,B", [("burgers", 64), ("lorenz", 257)])
def test_step_autoreset_counts_reset_rows_and_normalises_terminal_rows(case, B, dtype):
    _need_gpu()
    env = make(case, B, dtype).set_normalize()
    nz, ref = env.normalizer, Ref(B, env.obs_dim)
    acts = actions(env, 2, 9)
    env.reset()
    ref(*raw(env), kind="reset")
    env.set_stp(env.n_act - 2)                                               # every episode ends at the second step
    counted = B
    for k in range(2):
        obs, rwd, done, trunc, ep = env.step_autoreset(acts[k])
        assert obs is nz.norm_obs and rwd is nz.norm_rwd and ep is env.episodes
        o, r, st, d, t = raw(env)                                            # obs: behind the masked reset
        ref(o, r, st, d, t, finished=host(ep.finished), final_obs=host(ep.final_obs))
        counted += int(((st & 3) == 0).sum())
        assert_follows(nz, ref, dtype, "step %d" % k)
        assert float(nz.obs_count[0]) == counted
        assert int(ep.finished.sum()) == (B if k == 1 else 0)
    assert bool((nz.ret == 0).all())                                         # zero after the end
    fin = host(env.episodes.final_obs).astype(np.float64)
    want = np.clip((fin - ref.obs_mean) / np.sqrt(ref.obs_var + 1e-8), -10.0, 10.0)
    assert np.abs(host(nz.norm_final_obs) - want).max() <= OUT_TOL[dtype]    # the terminal rows, with the statistics that never saw them
    env.close()


def _five_steps(env, acts):
    env.reset()
    env.set_stp(env.n_act - 3)
    for k in range(5):
        env.step_autoreset(acts[k])
    return env.normalizer.buf.clone()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_the_same_sequence_gives_the_same_bits_in_both_bindings(dtype):
    _need_gpu()
    env = make("lorenz", 257, dtype).set_normalize()
    acts = actions(env, 5, 10)
    first = _five_steps(env, acts)
    env.episodes.clear()
    env.normalizer.clear()
    assert torch.equal(_five_steps(env, acts), first)
    other = make("lorenz", 257, dtype).set_normalize()
    assert other.use_torch_ops(False) is False                               # ctypes
    assert torch.equal(_five_steps(other, acts), first)
    env.close(), other.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_a_replayed_autoreset_graph_gives_what_the_eager_calls_give(dtype):
    _need_gpu()
    A, G = make("lorenz", 257, dtype).set_normalize(), make("lorenz", 257, dtype).set_normalize()
    acts = actions(A, 4, 12)
    for env in (A, G):
        env.reset()
        env.set_stp(env.n_act - 2)
    eager_obs, eager_rwd = [], []
    for k in range(4):
        obs, rwd = A.step_autoreset(acts[k])[:2]
        eager_obs.append(obs.clone()), eager_rwd.append(rwd.clone())
    graph = G.capture(acts, None, n_steps=4, autoreset=True)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(G.normalizer.buf, A.normalizer.buf)
    assert torch.equal(graph.norm_obs_seq, torch.stack(eager_obs)) and torch.equal(graph.norm_rwd_seq, torch.stack(eager_rwd))
    assert torch.equal(G.obs, A.obs) and torch.equal(G.rwd, A.rwd)
    assert float(G.normalizer.obs_count[0]) == 5 * 257
    A.close(), G.close()
