"""GPU tests of the on-device rollout storage and GAE (VecEnv.rollout, Rollout; csrc/rollout.hip): what the recording launch stores
against per-step clones of what the step returned, bit for bit -- plain, under masks, with the normaliser and the per-jet rewards in
play, eager and replayed from graphs, in both bindings -- the overflow rule, "off means off", and compute_gae against the float64
NumPy restatement of the recurrence (tests/rollout_ref.py, itself checked on the CPU by tests/test_rollout_host.py)."""
import functools

import numpy as np
import pytest
import torch

from beacon_amd import vec as V
from beacon_amd.envs import packaged_init
from rollout_ref import gae_bound, gae_inputs, gae_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NP = {"f32": np.float32, "f64": np.float64}
U_OUT = {"f32": 2.0 ** -24, "f64": 0.0}          # the one rounding of a float32 store


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")


def make(case, B, dtype):
    if case == "rayleigh":
        return V.VecRayleigh(B, DEV, dtype, init_fields=packaged_init("rayleigh"))          # the built-in 50x50 grid: rows of 192 reals
    return {"burgers": V.VecBurgers, "lorenz": V.VecLorenz, "shkadov": V.VecShkadov}[case](B, DEV, dtype)


def actions(env, n, seed):
    """[n, B, ...] in the shape and element type the env's step takes"""
    g = torch.Generator().manual_seed(seed)
    if env.action_is_int:
        return torch.randint(0, 3, (n, env.batch), generator=g, dtype=torch.int32).to(DEV)
    flat = env.n_actions == 1 and not isinstance(env, V.VecRayleigh)
    shape = (n, env.batch) if flat else (n, env.batch, env.n_actions)
    return (2.0 * torch.rand(shape, generator=g, dtype=torch.float64) - 1.0).to(device=DEV, dtype=env.tdtype)


def stagger(env):
    """episodes end at steps 0, 1, 2 of what follows"""
    env.set_stp(env.n_act - 1 - np.arange(env.batch) % 3)


def run(env, acts, mask=None):
    """step_autoreset per row of acts; per step, clones of everything the rollout is to hold"""
    seen = []
    for a in acts:
        obs, rwd, done, trunc, ep = env.step_autoreset(a, mask=mask)
        seen.append(dict(obs=obs.clone(), rwd=rwd.clone(), done=done.clone(), trunc=trunc.clone(), status=env.status.clone(),
                         finished=ep.finished.clone(), final_obs=ep.final_obs.clone()))
    return seen


def assert_holds(ro, seen, acts, first_obs):
    T, B = len(seen), ro.batch
    assert torch.equal(ro.obs[0], first_obs)
    for t, s in enumerate(seen):
        assert torch.equal(ro.obs[t + 1], s["obs"]), t
        assert torch.equal(ro.rwd[t], s["rwd"]) and torch.equal(ro.status[t], s["status"]), t
        assert torch.equal(ro.done[t], s["done"]) and torch.equal(ro.trunc[t], s["trunc"]), t
        assert torch.equal(ro.act[t].reshape(B, -1), acts[t].reshape(B, -1)) and ro.act.dtype == acts.dtype, t
        fin = s["finished"].bool()
        assert torch.equal(ro.final_obs[t][fin], s["final_obs"][fin]), t
        assert not ro.final_obs[t][~fin].any(), t                            # rows of unfinished replicas: still the zeros of a fresh buffer
    assert bool((ro.valid[:T] == 1).all())


# ---- 1. recording is bit-exact ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,B,dtype", [("burgers", 65, "f32"), ("burgers", 1, "f32"), ("lorenz", 505, "f32"), ("lorenz", 505, "f64"),
                                          ("shkadov", 130, "f32"), ("rayleigh", 3, "f32")])
def test_recording_is_bit_exact(case, B, dtype):
    _need_gpu()
    env = make(case, B, dtype)
    ro = env.rollout(5)
    assert env._rollout is ro and ro.T == 5 and not ro.buf.any()
    first = env.reset()[0].clone()
    stagger(env)
    assert ro.begin() is ro
    acts = actions(env, 5, 3)
    seen = run(env, acts)
    ends = torch.stack([s["finished"] for s in seen]).sum(1).cpu().tolist()
    assert ends[:3] == [len(range(k, B, 3)) for k in range(3)] and (B < 2 or sum(1 for e in ends if e) >= 2)
    assert_holds(ro, seen, acts, first)
    assert ro.check() == (5, False)
    assert tuple(ro.rwd_jets.shape) == (5, B, 0)
    env.close()


# ---- 2. two ends of one replica in one window -----------------------------------------------------------------------------------
def test_two_episode_ends_of_one_replica_are_both_kept():
    _need_gpu()
    env = make("lorenz", 8, "f32")
    ro = env.rollout(6)
    env.reset()
    stp = np.zeros(8, dtype=np.int32)
    stp[0] = env.n_act - 1
    env.set_stp(stp)
    ro.begin()
    acts = actions(env, 6, 4)
    for t in range(6):
        if t == 3:                                                           # replica 0 again, three steps into its second episode
            stp = env.get_stp()
            stp[0] = env.n_act - 1
            env.set_stp(stp)
        env.step_autoreset(acts[t])
    ends = torch.nonzero(ro.trunc[:, 0]).flatten().cpu().tolist()
    assert ends == [0, 3] and ro.check() == (6, False)
    a, b = ro.final_obs[0, 0], ro.final_obs[3, 0]
    assert a.any() and b.any() and not torch.equal(a, b)
    assert torch.equal(env.episodes.final_obs[0], b)                        # what EpisodeStats keeps: the last one only
    assert not ro.final_obs[:, 1:].any() and not ro.trunc[:, 1:].any()
    env.close()


# ---- 3. overflow ----------------------------------------------------------------------------------------------------------------
def test_a_record_into_a_full_rollout_writes_nothing_but_the_flag():
    _need_gpu()
    env = make("lorenz", 505, "f32")
    ro = env.rollout(5)
    env.reset()
    stagger(env)
    ro.begin()
    acts = actions(env, 6, 5)
    run(env, acts[:5])
    assert ro.check() == (5, False)
    before = ro.buf.clone()
    env.step_autoreset(acts[5])
    assert ro.cursor[:2].cpu().tolist() == [5, 1]
    assert torch.equal(ro.buf[:4], before[:4]) and torch.equal(ro.buf[8:], before[8:])      # no byte but cursor[1]
    with pytest.raises(V.RolloutOverflow):
        ro.check()
    env.step_autoreset(acts[5])                                               # sticky, and still nothing written
    assert torch.equal(ro.buf[8:], before[8:]) and ro.cursor[:2].cpu().tolist() == [5, 1]
    ro.begin()
    assert ro.check() == (0, False) and torch.equal(ro.obs[0], env.obs)
    env.close()


# ---- 4. masks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,B", [("burgers", 65), ("lorenz", 505)])
def test_masked_steps(case, B):
    _need_gpu()
    env, twin = make(case, B, "f32"), make(case, B, "f32")
    ro = env.rollout(4)
    for e in (env, twin):
        e.reset()
        stagger(e)
    ro.begin()
    acts = actions(env, 4, 6)
    if env.action_is_int:
        acts.clamp_(min=1)                                                   # no zero action: a row that was not written shows
    g = torch.Generator().manual_seed(7)
    masks = [(torch.rand(B, generator=g) < 0.5).to(DEV) for _ in range(4)]
    masks[1] = None
    for t in range(4):
        fn, tfn = (env.step, twin.step) if t == 2 else (env.step_autoreset, twin.step_autoreset)
        out, tout = fn(acts[t], mask=masks[t]), tfn(acts[t], mask=masks[t])
        for x, y in zip(out[:4], tout[:4]):
            assert torch.equal(x, y), t                                      # the env's own outputs: those of an env without a rollout
        assert torch.equal(env.status, twin.status), t
        m = torch.ones(B, dtype=torch.bool, device=DEV) if masks[t] is None else masks[t]
        assert torch.equal(ro.valid[t], m.to(torch.uint8)), t
        off = ~m
        assert not ro.rwd[t][off].any() and not ro.done[t][off].any() and not ro.trunc[t][off].any(), t
        assert torch.equal(ro.obs[t + 1][off], ro.obs[t][off]), t           # a skipped replica keeps its row
        assert torch.equal(ro.obs[t + 1], out[0]) and torch.equal(ro.rwd[t][m], out[1][m]), t
        assert torch.equal(ro.done[t][m], out[2][m]) and torch.equal(ro.trunc[t][m], out[3][m]), t
        assert torch.equal(ro.act[t].reshape(B, -1)[m], acts[t].reshape(B, -1)[m]) and not ro.act[t].reshape(B, -1)[off].any(), t
        assert not ro.final_obs[t][off].any(), t
        if t != 2:
            fin = env.episodes.finished.bool()
            assert not (fin & off).any() and torch.equal(ro.final_obs[t][fin], env.episodes.final_obs[fin]), t
    assert torch.equal(env.snapshot().buf, twin.snapshot().buf)
    assert ro.check() == (4, False)
    env.close(), twin.close()


# ---- 5. with the normaliser, with the per-jet rewards ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_with_normalisation_the_slots_hold_the_normalised_outputs(dtype):
    _need_gpu()
    env = make("lorenz", 257, dtype).set_normalize()
    nz, ro = env.normalizer, env.rollout(5)
    first = env.reset()[0]
    assert first is nz.norm_obs
    first = first.clone()
    stagger(env)
    ro.begin()
    acts = actions(env, 5, 8)
    seen = []
    for t in range(5):
        obs, rwd, done, trunc, ep = env.step_autoreset(acts[t])
        assert obs is nz.norm_obs and rwd is nz.norm_rwd
        seen.append(dict(obs=obs.clone(), rwd=rwd.clone(), done=done.clone(), trunc=trunc.clone(), status=env.status.clone(),
                         finished=ep.finished.clone(), final_obs=nz.norm_final_obs.clone()))
    assert_holds(ro, seen, acts, first)
    assert not torch.equal(ro.obs[5], env.obs) and ro.check() == (5, False)  # (the raw observations are something else)
    env.close()


def test_with_jet_rewards_the_slots_hold_the_per_jet_rewards():
    _need_gpu()
    env = make("shkadov", 130, "f32").set_jet_rewards()
    ro = env.rollout(5, final_obs=False)
    assert tuple(ro.rwd_jets.shape) == (5, 130, env.n_jets) and tuple(ro.final_obs.shape) == (5, 130, 0)
    first = env.reset()[0].clone()
    stagger(env)
    ro.begin()
    acts = actions(env, 5, 9)
    jets = []
    for t in range(5):
        obs, rwd = env.step_autoreset(acts[t])[:2]
        jets.append(env.rwd_jets.clone())
        assert torch.equal(ro.obs[t + 1], obs) and torch.equal(ro.rwd[t], rwd)
    assert torch.equal(ro.rwd_jets, torch.stack(jets)) and torch.equal(ro.obs[0], first)
    assert torch.equal(ro.act, acts) and ro.check() == (5, False)
    env.close()


# ---- 6. graphs, 7. off means off, and the two bindings ----------------------------------------------------------------------------
@pytest.mark.parametrize("case,B", [("burgers", 65), ("lorenz", 505)])
def test_replayed_graphs_fill_the_bytes_the_eager_steps_fill(case, B):
    _need_gpu()
    env = make(case, B, "f32")
    ro = env.rollout(5)
    env.reset()
    stagger(env)
    snap = env.snapshot()
    a = actions(env, 1, 10)[0].contiguous()
    ro.begin()
    for _ in range(5):
        env.step_autoreset(a)
    eager = ro.buf.clone()
    assert ro.check() == (5, False) and ro.trunc.any()

    env.restore(snap)
    ro.clear().begin()
    one = env.capture(a, None, keep_steps=False, autoreset=True)            # one step; the slot comes from the device cursor
    for _ in range(5):
        one.replay()
    torch.cuda.synchronize()
    assert torch.equal(ro.buf, eager)

    env.restore(snap)
    ro.clear().begin()
    five = env.capture(a.unsqueeze(0).expand(5, *a.shape).contiguous(), None, n_steps=5, autoreset=True, keep_steps=False)
    five.replay()
    torch.cuda.synchronize()
    assert torch.equal(ro.buf, eager)
    env.restore(snap)
    ro.begin()                                                                # a second begin() + replay reproduces them
    five.replay()
    torch.cuda.synchronize()
    assert torch.equal(ro.buf, eager) and ro.check() == (5, False)
    env.close()


@pytest.mark.parametrize("case,B", [("burgers", 65), ("lorenz", 505)])
def test_off_means_off(case, B):
    _need_gpu()
    env, twin = make(case, B, "f32"), make(case, B, "f32")
    env.rollout(5)
    assert twin._rollout is None and "rollout_record" not in (twin._ops or twin._cfn)
    acts = actions(env, 6, 11)
    for e in (env, twin):
        e.reset()
        stagger(e)
    assert env.snapshot_signature() == twin.snapshot_signature()
    env._rollout.begin()
    for t in range(6):                                                        # (the sixth overflows: that changes nothing either)
        out, tout = env.step_autoreset(acts[t]), twin.step_autoreset(acts[t])
        for x, y in zip(out[:4], tout[:4]):
            assert torch.equal(x, y), t
    assert torch.equal(env.snapshot().buf, twin.snapshot().buf) and torch.equal(env.out_buf, twin.out_buf)
    assert torch.equal(env.episodes.buf, twin.episodes.buf)
    kept = env._rollout
    assert env.rollout(None) is kept and env._rollout is None and env.rollout(5) is kept      # detach keeps the buffer
    env.close(), twin.close()


def test_both_bindings_record_and_estimate_the_same_bits():
    _need_gpu()
    bufs = []
    for torch_ops in (True, False):
        env = make("lorenz", 257, "f32")
        if env.use_torch_ops(torch_ops) != torch_ops:
            pytest.skip("the torch extension is not built")
        ro = env.rollout(4)
        env.reset()
        stagger(env)
        ro.begin()
        for a in actions(env, 4, 12):
            env.step_autoreset(a)
        g = torch.Generator().manual_seed(13)
        v, lv, fv = (torch.randn(s, generator=g).to(DEV) for s in ((4, 257), (257,), (4, 257)))
        ro.compute_gae(v, lv, fv)
        assert ro.check() == (4, False)
        bufs.append(ro.buf.clone())
        env.close()
    assert torch.equal(bufs[0], bufs[1])


# ---- 8. GAE against the float64 yardstick ----------------------------------------------------------------------------------------
SENTINEL = 777.0


@functools.lru_cache(maxsize=None)
def _gae_case(T, B, cols, dtype, with_final, n):
    """inputs and reference of one case, computed once"""
    rng = np.random.default_rng(1000 * T + B + cols)
    x = gae_inputs(rng, T, B * cols, cols, dtype=NP[dtype])
    if T >= 7:
        x["rwd"][T // 2, (B * cols) // 3] = np.nan                          # a NaN travels back to the start of its episode, no further
    fv = x["final_values"].copy()
    fv[np.repeat(x["trunc"], cols, axis=1) == 0] = np.nan                   # rows without trunc are never used
    x["final_values_fed"] = fv
    adv, ret = gae_ref(x["rwd"], x["values"], x["last_value"], x["done"], x["trunc"], x["valid"], fv if with_final else None, 0.99, 0.95,
                       cols, n)
    return x, adv, ret


def assert_gae(ro, x, adv_ref, ret_ref, dtype, T, cols, n):
    adv, ret = (v.double().cpu().numpy() for v in ro.gae_views(cols))
    assert adv.shape == adv_ref.shape == ret.shape
    assert (adv[n:] == SENTINEL).all() and (ret[n:] == SENTINEL).all()      # rows behind the cursor keep the sentinel
    adv, ret, adv_ref, ret_ref, val = adv[:n], ret[:n], adv_ref[:n], ret_ref[:n], x["values"][:n]
    assert np.array_equal(np.isnan(adv), np.isnan(adv_ref)) and np.array_equal(np.isnan(ret), np.isnan(ret_ref))
    bound = gae_bound(T, adv_ref, val, x["rwd"][:n])[None, :]
    u = U_OUT[dtype]
    with np.errstate(invalid="ignore"):
        tol_adv = bound + u * (np.abs(adv_ref) + bound)
        tol_ret = bound + 2.0 ** -53 * (np.abs(adv_ref) + np.abs(val)) + u * (np.abs(ret_ref) + bound)      # one more rounding
        ok = ~np.isnan(adv_ref)
        err_adv, err_ret = np.abs(adv - adv_ref), np.abs(ret - ret_ref)
        print("gae T=%d cols=%d %s: worst adv %.3g, ret %.3g of the tolerance" % (T, cols, dtype, (err_adv[ok] / tol_adv[ok]).max(initial=0.0),
                                                                                 (err_ret[ok] / tol_ret[ok]).max(initial=0.0)))
        assert (err_adv[ok] <= tol_adv[ok]).all() and (err_ret[ok] <= tol_ret[ok]).all()      # no element left out
    skipped = np.repeat(x["valid"][:n], cols, axis=1) == 0
    assert (adv[skipped] == 0).all() and np.array_equal(ret[skipped], val[skipped].astype(NP[dtype]).astype(np.float64))


@pytest.mark.parametrize("with_final", [True, False])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("T,B,cols,n", [(1, 1, 1, None), (7, 65, 1, None), (64, 1000, 1, None), (16, 130, 5, None), (7, 65, 1, 3)])
def test_gae_follows_the_float64_restatement(T, B, cols, n, dtype, with_final):
    _need_gpu()
    x, adv_ref, ret_ref = _gae_case(T, B, cols, dtype, with_final, n)
    if cols > 1:
        env = V.VecShkadov(B, DEV, dtype, n_jets=cols).set_jet_rewards()
    else:
        env = make("lorenz", B, dtype)
    ro = env.rollout(T)
    dev = lambda a, dt=env.tdtype: torch.as_tensor(a).to(device=DEV, dtype=dt)
    # synthetic inputs, written through the views
    if cols > 1:
        ro.rwd_jets.copy_(dev(x["rwd"]).view(T, B, cols))
        ro.rwd.fill_(float("nan"))                                           # per_jet: the rewards come from rwd_jets alone
    else:
        ro.rwd.copy_(dev(x["rwd"]))
    for name in ("done", "trunc", "valid"):
        getattr(ro, name).copy_(dev(x[name], torch.uint8))
    ro.cursor[0] = T if n is None else n
    for v in ro.gae_views(cols):
        v.fill_(SENTINEL)
    values, last, final = dev(x["values"]), dev(x["last_value"]), dev(x["final_values_fed"]) if with_final else None
    out = ro.compute_gae(values, last, final, gamma=0.99, lam=0.95, per_jet=cols > 1)
    assert out[0] is ro.adv and out[1] is ro.ret and tuple(ro.adv.shape) == (T, B * cols)
    assert_gae(ro, x, adv_ref, ret_ref, dtype, T, cols, T if n is None else n)
    once = ro.buf.clone()
    ro.compute_gae(values, last, final, gamma=0.99, lam=0.95, per_jet=cols > 1)
    assert torch.equal(ro.buf, once)                                         # two runs: the same bytes
    for bad in ((values[:, :-1].contiguous(), last, final), (values.double() if dtype == "f32" else values.float(), last, final),
                (values.cpu(), last, final), (values, last[:-1].contiguous() if B * cols > 1 else last.cpu(), final)):
        with pytest.raises(ValueError):
            ro.compute_gae(*bad)
    env.close()


# ---- 9. end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_recorded_rollout_to_advantages(dtype):
    _need_gpu()
    B, T = 505, 32
    env = make("lorenz", B, dtype)
    ro = env.rollout(T)
    env.reset()
    env.set_stp(env.n_act - 1 - np.arange(B) % 40)                           # ends spread over the window, some replicas none
    ro.begin()
    acts = actions(env, T, 14)
    g = torch.Generator().manual_seed(15)
    masks = [None if t % 5 else (torch.rand(B, generator=g) < 0.8).to(DEV) for t in range(T)]
    for t in range(T):
        env.step_autoreset(acts[t], mask=masks[t])
    assert ro.check() == (T, False) and ro.trunc.any() and not ro.valid.all()
    values, final = (torch.randn((T, B), generator=g, dtype=torch.float64).to(device=DEV, dtype=env.tdtype) for _ in range(2))
    last = torch.randn((B,), generator=g, dtype=torch.float64).to(device=DEV, dtype=env.tdtype)
    for v in ro.gae_views(1):
        v.fill_(SENTINEL)
    ro.compute_gae(values, last, final)
    h = lambda t: t.double().cpu().numpy() if t.is_floating_point() else t.cpu().numpy()
    x = dict(rwd=h(ro.rwd), values=h(values), valid=h(ro.valid))
    adv_ref, ret_ref = gae_ref(x["rwd"], x["values"], h(last), h(ro.done), h(ro.trunc), x["valid"], h(final), 0.99, 0.95)
    assert_gae(ro, x, adv_ref, ret_ref, dtype, T, 1, T)
    env.close()
