"""Fused auto-reset and on-device episode statistics on the GPU: VecEnv.step_autoreset / track_episodes / capture(autoreset=True)
(csrc/episode.hip, include/beacon_hip.h: bcn_episode_*).  The yardstick is the path that existed before: step(); final =
obs.clone(); reset_done(), with the statistics kept by plain torch code in this file.  Every comparison is bitwise (torch.equal):
the bookkeeping is one add per step in the env's dtype and copies, so there is no tolerance to state."""
import numpy as np
import pytest
import torch

from beacon_amd import vec as V
from beacon_amd.envs import packaged_init

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _short(n):
    return lambda e: e.set_ndt_act(n)


# name -> (class, constructor kwargs, batch, what to do after construction).  2D: the smallest built-in grids, the action step
# shortened; ODE: more than one bookkeeping workgroup (256 replicas each)
CASES = {
    "rayleigh": (V.VecRayleigh, lambda: dict(init_fields=packaged_init("rayleigh")), 8, _short(5)),      # 50x50, obs rows of 192 reals
    "mixing": (V.VecMixing, dict, 8, _short(5)),                                                         # 100x100
    "burgers": (V.VecBurgers, dict, 37, None),                                                           # obs rows of 5 reals: 4-byte units (f32)
    "shkadov": (V.VecShkadov, dict, 37, None),
    "sloshing": (V.VecSloshing, dict, 37, None),
    "lorenz": (V.VecLorenz, dict, 300, None),                                                            # obs rows of 6 reals: 8-byte units (f32)
    "vortex": (V.VecVortex, dict, 300, None),
}
STATS = ("finished", "ret", "len", "last_ret", "last_len", "count", "sum_ret", "sum_len")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")


def make(case, dtype):
    cls, kw, B, post = CASES[case]
    env = cls(B, DEV, dtype, **kw())
    if post is not None:
        post(env)
    return env


def actions(env, n, seed):
    """n steps of seeded random actions [n, B, ...] on the device, in the env's action type"""
    g = torch.Generator().manual_seed(seed)
    if env.action_is_int:
        hi = 4 if isinstance(env, V.VecMixing) else 3
        return torch.randint(0, hi, (n, env.batch), generator=g, dtype=torch.int32).to(DEV)
    shape = (n, env.batch) if env.n_actions == 1 and not isinstance(env, V.VecRayleigh) else (n, env.batch, env.n_actions)
    return (2.0 * torch.rand(shape, generator=g, dtype=torch.float64) - 1.0).to(device=DEV, dtype=env.tdtype)


def stagger(env, period, shift=0):
    """episode counters so that replica b ends its episode at step 1 + (b + shift) % period from now"""
    env.set_stp(env.n_act - 1 - (np.arange(env.batch) + shift) % period)


class RefStats(object):
    """the statistics of EpisodeStats kept the way a trainer would: small torch ops, one update per step"""

    def __init__(self, env):
        B, dev = env.batch, env.device
        self.ret = torch.zeros(B, dtype=env.tdtype, device=dev)
        self.len = torch.zeros(B, dtype=torch.int32, device=dev)
        self.last_ret, self.last_len = self.ret.clone(), self.len.clone()
        self.count = torch.zeros(B, dtype=torch.int32, device=dev)
        self.sum_ret = torch.zeros(B, dtype=torch.float64, device=dev)
        self.sum_len = torch.zeros(B, dtype=torch.int64, device=dev)
        self.finished = torch.zeros(B, dtype=torch.uint8, device=dev)
        self.final_obs = torch.zeros((B, env.obs_dim), dtype=env.tdtype, device=dev)

    def update(self, obs, rwd, done, trunc, mask=None):
        sel = torch.ones_like(done, dtype=torch.bool) if mask is None else mask.to(DEV).bool()
        fin = ((done | trunc) != 0) & sel
        self.ret = torch.where(sel, self.ret + rwd, self.ret)
        self.len = torch.where(sel, self.len + 1, self.len)
        self.last_ret = torch.where(fin, self.ret, self.last_ret)
        self.last_len = torch.where(fin, self.len, self.last_len)
        self.count = self.count + fin.to(torch.int32)
        self.sum_ret = torch.where(fin, self.sum_ret + self.ret.double(), self.sum_ret)
        self.sum_len = self.sum_len + torch.where(fin, self.len.long(), torch.zeros_like(self.sum_len))
        self.ret = torch.where(fin, torch.zeros_like(self.ret), self.ret)
        self.len = torch.where(fin, torch.zeros_like(self.len), self.len)
        self.final_obs = torch.where(fin[:, None], obs, self.final_obs)
        self.finished = fin.to(torch.uint8)
        return fin


def assert_same_stats(ep, ref, where=""):
    for name in STATS:
        assert torch.equal(getattr(ep, name), getattr(ref, name)), (where, name)
    assert torch.equal(ep.final_obs, ref.final_obs), (where, "final_obs")


def assert_same_env(a, b, where=""):
    for name in ("obs", "rwd", "done", "trunc", "status"):
        assert torch.equal(getattr(a, name), getattr(b, name)), (where, name)
    assert torch.equal(a.get_state(), b.get_state()), (where, "state")
    assert np.array_equal(a.get_stp(), b.get_stp()), (where, "stp")


def eager_reference_step(env, ref, a, z=None, mask=None):
    """what step_autoreset replaces: step, rescue the terminal rows, bookkeeping in torch, reset the replicas that finished"""
    obs, rwd, done, trunc, _ = env.step(a, z, mask=mask)
    final = obs.clone()
    fin = ref.update(final, rwd, done, trunc, mask)
    if mask is None:
        env.reset_done()
    else:
        env.reset(mask=fin)           # reset_done() would also reset a skipped replica whose stale done byte is 1
    return fin


# ---- 1. equivalence with the eager path: every env, both dtypes ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("case", list(CASES))
def test_step_autoreset_equals_step_clone_reset_done(case, dtype):
    """Two envs from the same constructor arguments, seeds and actions, episode counters staggered (twice) so that every replica
    ends two episodes, at different steps: A runs step_autoreset, B runs step(); obs.clone(); reset_done() with RefStats.  After
    every step the outputs, state, episode counters and every statistic are equal bit for bit."""
    _need_gpu()
    A, B = make(case, dtype), make(case, dtype)
    ref = RefStats(B)
    n1, n2 = 5, 4
    acts = actions(A, n1 + n2, 5)
    A.reset()
    B.reset()
    reset_obs = B.obs.clone()
    ends = torch.zeros(A.batch, dtype=torch.int64, device=DEV)
    for k in range(n1 + n2):
        if k == 0:
            stagger(A, 4), stagger(B, 4)                  # ends at steps 1..4 of 5
        if k == n1:
            stagger(A, 3, 1), stagger(B, 3, 1)            # ends at steps 1..3 of 4
        obs, rwd, done, trunc, info = A.step_autoreset(acts[k])
        assert obs is A.obs and rwd is A.rwd and done is A.done and trunc is A.trunc and info is A.episodes
        fin = eager_reference_step(B, ref, acts[k])
        assert_same_env(A, B, (case, dtype, k))
        assert_same_stats(info, ref, (case, dtype, k))
        assert torch.equal(info.finished.bool(), (done | trunc) != 0)
        assert torch.equal(obs[fin], reset_obs[fin])                    # same-step autoreset: fresh rows
        ends += fin
    assert int(ends.min()) >= 2                                          # at least two episode ends per replica
    assert int(info.count.min()) >= 2 and torch.equal(info.count.long(), ends)
    tot = info.totals()
    assert tot["episodes"] == int(ends.sum()) and tot["length_sum"] == int(ref.sum_len.sum())
    assert tot["length_mean"] == tot["length_sum"] / tot["episodes"]
    assert tot["return_mean"] == tot["return_sum"] / tot["episodes"]
    if case == "lorenz":
        # rewards are 0 or 1: every sum is an integer and exact in any order
        rsum = tot["return_sum"]
        assert rsum == int(rsum) and 0 <= rsum <= tot["length_sum"]
        assert rsum == int(info.sum_ret.cpu().numpy().astype(np.int64).sum())
        assert torch.equal(info.last_ret, info.last_ret.round()) and torch.equal(info.sum_ret, info.sum_ret.round())
        assert tot["return_mean"] == rsum / tot["episodes"]
    A.close(), B.close()


# ---- 2. masks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,dtype", [("burgers", "f32"), ("lorenz", "f64"), ("rayleigh", "f32")])
def test_masked_step_autoreset_leaves_skipped_replicas_alone(case, dtype):
    """step_autoreset(mask=m): replicas with m == 0 keep state, counters, output rows and every statistic; one of them carries a
    stale done byte (it finished in an unmasked plain step() and was not reset) and is neither reset nor counted."""
    _need_gpu()
    A, B = make(case, dtype), make(case, dtype)
    ref = RefStats(B)
    acts = actions(A, 6, 9)
    nB = A.batch
    m = torch.as_tensor((np.arange(nB) % 3 != 0).astype(np.uint8))          # replicas 0, 3, 6, .. are skipped
    skipped = (m == 0).to(DEV)
    for env in (A, B):
        env.reset()
        stp = env.n_act - 2 - (np.arange(nB) % 3)           # replicas 0, 3, .. end at the plain step below; the others 1, 2 steps later
        stp[0::3] = env.n_act - 1
        env.set_stp(stp)
        env.step(acts[0])                                    # plain step: done rises for the replicas that will be skipped
    assert bool(A.done[skipped].all()) and not bool(A.done[~skipped].any())
    for k in range(1, 6):
        before = [A.obs.clone(), A.rwd.clone(), A.done.clone(), A.trunc.clone(), A.status.clone(), A.get_state(), A.get_stp()]
        stats0 = {n: getattr(A.episodes, n).clone() for n in STATS + ("final_obs",)}
        obs, rwd, done, trunc, info = A.step_autoreset(acts[k], mask=m)
        eager_reference_step(B, ref, acts[k], mask=m)
        assert_same_env(A, B, (case, k))
        assert_same_stats(info, ref, (case, k))
        after = [A.obs, A.rwd, A.done, A.trunc, A.status, A.get_state()]
        for x, y in zip(before, after):
            assert torch.equal(x[skipped], y[skipped])
        assert np.array_equal(before[6][skipped.cpu().numpy()], A.get_stp()[skipped.cpu().numpy()])   # not reset: stp stays n_act
        for n in STATS + ("final_obs",):
            assert torch.equal(stats0[n][skipped], getattr(info, n)[skipped]), n
        assert int(info.finished[skipped].max()) == 0 and int(info.count[skipped].max()) == 0
        assert bool(A.done[skipped].all())                                    # the stale byte is still there
    assert int(info.count[~skipped].min()) >= 1
    A.close(), B.close()


# ---- 3. graphs --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,dtype", [("burgers", "f32"), ("lorenz", "f32"), ("vortex", "f64"), ("rayleigh", "f32")])
def test_captured_autoreset_rollout_crosses_episode_ends(case, dtype):
    """capture(n_steps=n, autoreset=True) replayed twice == 2n eager step_autoreset calls: per-step sequences, final state,
    statistics.  Episodes end inside both replays."""
    _need_gpu()
    n = 4
    G, E = make(case, dtype), make(case, dtype)
    acts = actions(G, 2 * n, 21)
    for env in (G, E):
        env.reset()
        stagger(env, 7)                                      # ends at steps 1..7 of 8
    a_in = acts[:n].clone()
    g = G.capture(a_in, None, n_steps=n, autoreset=True)
    seqs = []
    for r in range(2):
        a_in.copy_(acts[r * n:(r + 1) * n])
        seqs.append([x.clone() for x in g.replay()])
    torch.cuda.synchronize()
    k = 0
    for r in range(2):
        assert int(seqs[r][2].sum()) > 0                                      # an episode ended inside this replay
        for i in range(n):
            obs, rwd, done, trunc, info = E.step_autoreset(acts[k])
            for got, want in zip(seqs[r], (obs, rwd, done, trunc)):
                assert torch.equal(got[i], want), (case, r, i)
            k += 1
    assert_same_env(G, E, case)
    assert_same_stats(G.episodes, E.episodes, case)
    assert int(G.episodes.count.sum()) == G.batch
    G.close(), E.close()


@pytest.mark.parametrize("case", ["burgers", "lorenz"])
def test_capture_without_autoreset_still_records_plain_steps(case):
    _need_gpu()
    n = 3
    G, E = make(case, "f32"), make(case, "f32")
    acts = actions(G, n, 4)
    for env in (G, E):
        env.reset()
        stagger(env, 2)
    g = G.capture(acts, None, n_steps=n)
    assert g.autoreset is False
    obs_seq, rwd_seq, done_seq, trunc_seq = g.replay()
    for i in range(n):
        obs, rwd, done, trunc, _ = E.step(acts[i])
        assert torch.equal(obs_seq[i], obs) and torch.equal(rwd_seq[i], rwd)
        assert torch.equal(done_seq[i], done) and torch.equal(trunc_seq[i], trunc)
    assert_same_env(G, E, case)
    assert getattr(G, "_episodes", None) is None                               # nothing was tracked, nothing allocated
    assert np.array_equal(G.get_stp(), E.get_stp()) and int(G.get_stp().max()) > G.n_act - 1    # and nothing was reset
    G.close(), E.close()


# ---- 4. double-buffered outputs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["burgers", "vortex"])
def test_step_autoreset_with_double_buffer(case):
    """with double_buffer() the bookkeeping and the reset act on the buffer the step just wrote: the results returned per step
    equal those of a single-buffer run, with and without a mask."""
    _need_gpu()
    D, S = make(case, "f32").double_buffer(), make(case, "f32")
    acts = actions(D, 8, 13)
    m = torch.as_tensor((np.arange(D.batch) % 4 != 1).astype(np.uint8))
    for env in (D, S):
        env.reset()
        stagger(env, 5)
    bufs = set()
    for k in range(8):
        mask = m if k in (2, 5) else None
        d = D.step_autoreset(acts[k], mask=mask)
        s = S.step_autoreset(acts[k], mask=mask)
        bufs.add(d[0].data_ptr())
        for x, y in zip(d[:4], s[:4]):
            assert torch.equal(x, y), (case, k)
        assert torch.equal(D.status, S.status)
        assert_same_stats(d[4], s[4], (case, k))
    assert len(bufs) == 2 and int(D.episodes.count.min()) >= 1
    assert_same_env(D, S, case)
    D.close(), S.close()


# ---- 5. bookkeeping alone, clear, checkpoints, the two bindings -----------------------------------------------------------------
@pytest.mark.parametrize("case,dtype", [("sloshing", "f32"), ("lorenz", "f64")])
def test_track_episodes_with_manual_resets(case, dtype):
    _need_gpu()
    A, M = make(case, dtype), make(case, dtype)
    acts = actions(A, 6, 3)
    for env in (A, M):
        env.reset()
        stagger(env, 5)
    for k in range(6):
        A.step_autoreset(acts[k])
        M.step(acts[k])
        ep = M.track_episodes()
        assert ep is M.episodes
        assert torch.equal(ep.final_obs[ep.finished.bool()], M.obs[ep.finished.bool()])
        M.reset_done()
        assert_same_env(A, M, (case, k))
        assert_same_stats(A.episodes, ep, (case, k))
    A.close(), M.close()


def test_clear_state_dict_and_totals():
    _need_gpu()
    env = make("lorenz", "f32")
    env.reset()
    stagger(env, 3)
    acts = actions(env, 4, 8)
    tot0 = env.episodes.totals()
    assert tot0["episodes"] == 0 and tot0["length_sum"] == 0 and np.isnan(tot0["return_mean"])
    for k in range(4):
        env.step_autoreset(acts[k])
    ep = env.episodes
    assert ep.buf.dtype == torch.uint8 and ep.ret.data_ptr() == ep.buf.data_ptr()                  # views, no copies
    assert all(seg["offset"] % 16 == 0 for seg in ep.layout)
    assert ep.final_obs.shape == (env.batch, env.obs_dim) and ep.sum_ret.dtype == torch.float64 and ep.sum_len.dtype == torch.int64
    tot = ep.totals()
    assert tot["episodes"] == int(ep.count.sum()) > 0 and tot["length_sum"] == int(ep.sum_len.sum())
    sd = ep.state_dict()
    assert sd["buf"].device.type == "cpu"
    keep = {n: getattr(ep, n).clone() for n in ep.NAMES}
    m = torch.as_tensor((np.arange(env.batch) % 2).astype(np.uint8))
    sel = m.bool().to(DEV)
    assert ep.clear(m) is ep
    for n in ep.NAMES:
        v = getattr(ep, n)
        assert int((v[sel] != 0).sum()) == 0 and torch.equal(v[~sel], keep[n][~sel]), n
    ep.load_state_dict(sd)
    for n in ep.NAMES:
        assert torch.equal(getattr(ep, n), keep[n]), n
    ep.clear()
    assert int(ep.buf.max()) == 0
    other = make("vortex", "f32")
    with pytest.raises(ValueError):
        other.episodes.load_state_dict(sd)
    env.close(), other.close()


@pytest.mark.parametrize("case", ["shkadov", "lorenz"])
def test_ctypes_and_torch_op_bindings_agree(case):
    _need_gpu()
    T, C = make(case, "f32"), make(case, "f32")
    assert T.use_torch_ops(True) and not C.use_torch_ops(False)
    acts = actions(T, 6, 17)
    m = torch.as_tensor((np.arange(T.batch) % 5 != 0).astype(np.uint8))
    for env in (T, C):
        env.reset()
        stagger(env, 4)
    for k in range(6):
        mask = m if k == 3 else None
        T.step_autoreset(acts[k], mask=mask)
        C.step_autoreset(acts[k], mask=mask)
        assert_same_env(T, C, (case, k))
        assert_same_stats(T.episodes, C.episodes, (case, k))
    assert int(T.episodes.count.min()) >= 1
    T.close(), C.close()
