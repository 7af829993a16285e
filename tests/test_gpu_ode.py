"""The batched ODE envs on the GPU (VecLorenz, VecVortex: csrc/ode_env.h) against the reference's captured episodes
(tests/golden/lorenz.npz, vortex.npz) and the host ports beacon_amd.lorenz / beacon_amd.vortex, which are bit-exact against them
(tests/test_host.py).  Every tolerance is <= 10 x the error measured on an MI355X, written next to it."""
import math

import numpy as np
import pytest
import torch

import beacon_amd
from beacon_amd import vec as V
from conftest import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LZ_TAGS = ("a0", "a1", "a2", "rnd")

# measured on an MI355X (max over the test's replicas and steps; "rel": divided by the largest |value| of the same column)
TOL = {
    # float64 vortex: the device's cos / sin differ from glibc's in the last bit on some arguments; absolute errors on values of
    # order 1e-3 (obs) / 1e-5 (rwd), max over the golden episodes, 64 replicas x 40 steps and 2 000 replicas x 10 steps
    "vortex_f64_obs": 6.9e-17,    # measured 6.9e-18
    "vortex_f64_rwd": 3.4e-17,    # measured 3.5e-18
    "lorenz_f32_obs": 3.3e-6,     # rel, one step from each golden state, measured 3.4e-7
    "vortex_f32_obs": 9.8e-6,     # rel, measured 9.8e-7
    "vortex_f32_rwd": 4e-4,       # rel, measured 4.0e-5
    "vortex_f32_episode_obs": 2.1e-4,  # rel, a whole 800-step episode (257 replicas, random actions) against float64, measured 2.1e-5
    "lorenz_f32_10steps": 6.2e-6,  # rel, 10 action steps from reset with random actions (2 000 of 2^20 replicas), measured 6.3e-7
    "vortex_f32_10steps": 1.8e-5,  # rel, measured 1.9e-6
}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")


def _np(t):
    return t.detach().cpu().numpy()


def _rel(a, r):
    """max over columns of max |a - r| / max |r| (of that column)"""
    a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
    if r.ndim == 1:
        a, r = a[:, None], r[:, None]
    a, r = a.reshape(-1, r.shape[-1]), r.reshape(-1, r.shape[-1])
    scale = np.maximum(np.abs(r).max(axis=0), 1e-300)
    return float((np.abs(a - r).max(axis=0) / scale).max())


def _report(name, err):
    print("MEASURED %s %.3e (tolerance %.1e)" % (name, err, TOL[name]))
    assert err <= TOL[name], (name, err)


def _host_t(k, dt):
    """the host port's time after k timesteps: t += dt accumulated"""
    t = 0.0
    for _ in range(k):
        t += dt
    return t


# ---- 1. lorenz float64: the four golden episodes bit for bit ---------------------------------------------------------------------
def test_lorenz_f64_golden_episodes_bit_exact():
    _need_gpu()
    g = golden("lorenz")
    B = 3108                                       # 12 full workgroups and a partial one
    env = V.VecLorenz(B, DEV, "f64")
    tag = [LZ_TAGS[b % 4] for b in range(B)]
    acts = torch.as_tensor(np.stack([g[t + "_actions"] for t in tag], axis=1), dtype=torch.int32, device=DEV)   # [500, B]
    obs0, _ = env.reset()
    assert torch.equal(obs0, torch.as_tensor(np.stack([g[t + "_reset_obs"] for t in tag]), device=DEV))
    gobs = torch.as_tensor(np.stack([g[t + "_obs"] for t in tag], axis=1), device=DEV)          # [500, B, 6]
    grwd = torch.as_tensor(np.stack([g[t + "_rwd"] for t in tag], axis=1), device=DEV)
    gdone = torch.as_tensor(np.stack([g[t + "_done"] for t in tag], axis=1), device=DEV)         # [500, B, 2]
    for k in range(acts.shape[0]):
        obs, rwd, done, trunc, _ = env.step(acts[k])
        assert torch.equal(obs, gobs[k]), k
        assert torch.equal(rwd, grwd[k]), k
        assert torch.equal(done.bool(), gdone[k, :, 0]) and torch.equal(trunc.bool(), gdone[k, :, 1]), k
    assert int(env.status.abs().max()) == 0
    st = _np(env.get_state())
    assert np.array_equal(st[:, :3], np.stack([g[t + "_hx"][-1] for t in tag]))
    assert np.array_equal(st[:, 7], np.array([g[t + "_actions"][-1] for t in tag], np.float64))
    assert np.array_equal(env.get_stp(), np.full(B, 500))
    env.close()


# ---- 2. vortex float64: the "zero" (800 steps) and "rnd" (120 steps) episodes, interleaved ------------------------------------
def test_vortex_f64_golden_episodes():
    _need_gpu()
    g = golden("vortex")
    B = 2 * 300 + 1
    env = V.VecVortex(B, DEV, "f64")
    is_rnd = np.arange(B) % 2 == 1
    n = g["zero_actions"].shape[0]
    nr = g["rnd_actions"].shape[0]
    A = np.zeros((n, B, 2))
    A[:, ~is_rnd] = g["zero_actions"][:, None]
    A[:nr, is_rnd] = g["rnd_actions"][:, None]
    acts = torch.as_tensor(A, device=DEV)
    obs0, _ = env.reset()
    assert torch.equal(obs0[0], torch.as_tensor(g["zero_reset_obs"], device=DEV))
    eo = er = 0.0
    for k in range(n):
        obs, rwd, done, trunc, _ = env.step(acts[k])
        o, r = _np(obs), _np(rwd)
        eo = max(eo, float(np.abs(o[~is_rnd] - g["zero_obs"][k]).max()))
        er = max(er, float(np.abs(r[~is_rnd] - g["zero_rwd"][k]).max()))
        assert np.array_equal(_np(done)[~is_rnd].astype(bool), np.full((~is_rnd).sum(), g["zero_done"][k, 0]))
        if k < nr:
            eo = max(eo, float(np.abs(o[is_rnd] - g["rnd_obs"][k]).max()))
            er = max(er, float(np.abs(r[is_rnd] - g["rnd_rwd"][k]).max()))
            assert np.array_equal(_np(trunc)[is_rnd].astype(bool), np.full(is_rnd.sum(), g["rnd_done"][k, 1]))
    _report("vortex_f64_obs", eo)
    _report("vortex_f64_rwd", er)
    st = _np(env.get_state())
    assert np.abs(st[~is_rnd, :4] - g["zero_hx"][-1]).max() <= max(TOL["vortex_f64_obs"], 0.0)
    assert np.array_equal(st[:, 8], np.full(B, _host_t(5 * n, 0.1)))       # t accumulated as the reference does
    env.close()


# ---- 3. float32: one action step from every golden state ---------------------------------------------------------------------
def test_lorenz_f32_one_step_from_every_golden_state():
    _need_gpu()
    g = golden("lorenz")
    rows, acts, gobs, grwd = [], [], [], []
    for tag in LZ_TAGS:
        hx, a = g[tag + "_hx"], g[tag + "_actions"]
        for k in range(a.shape[0]):
            u_prev = 1 if k == 0 else a[k - 1]
            rows.append(list(hx[k]) + [0.0, 0.0, 0.0, _host_t(k, 0.05), float(u_prev)])
            acts.append(a[k])
            gobs.append(g[tag + "_obs"][k])
            grwd.append(g[tag + "_rwd"][k])
    B = len(rows)                                  # 2 000
    env = V.VecLorenz(B, DEV, "f32")
    env.reset()
    env.set_state(np.array(rows))
    obs, rwd, _, _, _ = env.step(torch.as_tensor(np.array(acts), dtype=torch.int32, device=DEV))
    gobs, grwd = np.array(gobs), np.array(grwd)
    _report("lorenz_f32_obs", _rel(_np(obs), gobs))
    # the reward's sign: replicas whose x0 lies in the rounding zone (the observation tolerance) are left out
    x0 = gobs[:, 0]
    keep = np.abs(x0) > TOL["lorenz_f32_obs"] * np.abs(x0).max()
    assert keep.sum() > 0.99 * B
    assert np.array_equal(_np(rwd)[keep], grwd[keep])
    env.close()


def _vortex_golden_states(g):
    """(state rows, actions, golden obs, golden rwd) of every step of both episodes: the state before step k from hx[5k], t and y
    rebuilt the way the host port accumulates them"""
    wf = 0.74
    rows, acts, gobs, grwd = [], [], [], []
    for tag in ("zero", "rnd"):
        hx, a = g[tag + "_hx"], g[tag + "_actions"]
        for k in range(a.shape[0]):
            x = hx[5 * k]
            t = _host_t(5 * k, 0.1)
            y = 2.0 * (x[2] * math.cos(wf * t) - x[3] * math.sin(wf * t))
            u_prev = np.zeros(2) if k == 0 else a[k - 1]
            rows.append(list(x) + [0.0] * 4 + [t, y, 0.0, 0.0] + list(u_prev))
            acts.append(a[k])
            gobs.append(g[tag + "_obs"][k])
            grwd.append(g[tag + "_rwd"][k])
    return np.array(rows), np.array(acts), np.array(gobs), np.array(grwd)


def test_vortex_f32_one_step_from_every_golden_state():
    _need_gpu()
    rows, acts, gobs, grwd = _vortex_golden_states(golden("vortex"))
    B = rows.shape[0]                              # 920
    env = V.VecVortex(B, DEV, "f32")
    env.reset()
    env.set_state(rows)
    obs, rwd, _, _, _ = env.step(acts)
    _report("vortex_f32_obs", _rel(_np(obs), gobs))
    _report("vortex_f32_rwd", _rel(_np(rwd), grwd))
    env.close()


def test_vortex_f32_episode_against_f64():
    _need_gpu()
    B = 257
    rng = np.random.default_rng(11)
    A = rng.uniform(-1, 1, (800, B, 2))
    e32, e64 = V.VecVortex(B, DEV, "f32"), V.VecVortex(B, DEV, "f64")
    e32.reset(), e64.reset()
    a32, a64 = torch.as_tensor(A, dtype=torch.float32, device=DEV), torch.as_tensor(A, device=DEV)
    o32, o64 = [], []
    for k in range(800):
        o32.append(e32.step(a32[k])[0].double().clone())
        o64.append(e64.step(a64[k])[0].clone())
    _report("vortex_f32_episode_obs", _rel(_np(torch.stack(o32)), _np(torch.stack(o64))))
    e32.close(), e64.close()


# ---- 4. masks, auto-reset and repeated actions against one host object per replica ---------------------------------------------
def _state_rows_equal(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("name", ["lorenz", "vortex"])
def test_masks_auto_reset_and_repeated_actions_match_host_objects(name):
    _need_gpu()
    B, n = 64, 40
    rng = np.random.default_rng(5)
    env = (V.VecLorenz if name == "lorenz" else V.VecVortex)(B, DEV, "f64")
    hosts = [(beacon_amd.lorenz if name == "lorenz" else beacon_amd.vortex)() for _ in range(B)]
    tol_o, tol_r = (0.0, 0.0) if name == "lorenz" else (TOL["vortex_f64_obs"], TOL["vortex_f64_rwd"])

    def close(dev, ref, tol=tol_o):
        return np.abs(np.asarray(dev, np.float64) - np.asarray(ref, np.float64)).max() <= tol

    env.reset()
    for h in hosts:
        h.reset()
    # episodes end within the window: start the counters near n_act (the host objects get the same counters)
    stp0 = np.array([env.n_act - 5 - (b % 23) for b in range(B)], np.int32)
    env.set_stp(stp0)
    for b, h in enumerate(hosts):
        h.stp = int(stp0[b])
    none_steps = {3, 11, 12, 30}
    for k in range(n):
        if k in (10, 26):                          # a masked reset; the step right after it repeats the stored action
            m = rng.random(B) < 0.4
            before = _np(env.get_state()).copy()
            obs_before = _np(env.obs).copy()
            env.reset(mask=torch.as_tensor(m, device=DEV))
            for b in np.nonzero(m)[0]:
                hosts[b].reset()
            after = _np(env.get_state())
            assert _state_rows_equal(after[~m], before[~m]) and np.array_equal(_np(env.obs)[~m], obs_before[~m])
            for b in np.nonzero(m)[0]:
                assert close(_np(env.obs)[b], hosts[b].get_obs())
        if name == "lorenz":
            a = None if k in none_steps else rng.integers(0, 3, B)
        else:
            a = None if k in none_steps else rng.uniform(-1, 1, (B, 2))
        step_mask = (rng.random(B) < 0.7) if k == 17 else None
        before = _np(env.get_state()).copy()
        prev = [_np(x).copy() for x in (env.obs, env.rwd, env.done, env.trunc)]
        obs, rwd, done, trunc, _ = env.step(None if a is None else (torch.as_tensor(a, device=DEV)), mask=(
            None if step_mask is None else torch.as_tensor(step_mask, device=DEV)))
        o, r, d, t = _np(obs), _np(rwd), _np(done), _np(trunc)
        for b in range(B):
            if step_mask is not None and not step_mask[b]:
                continue
            ho, hr, hd, ht, _ = hosts[b].step(None if a is None else (np.int64(a[b]) if name == "lorenz" else a[b]))
            assert close(o[b], ho) and close(r[b], hr, tol_r), (k, b)
            assert bool(d[b]) == hd and bool(t[b]) == ht, (k, b)
        if step_mask is not None:
            skip = ~step_mask
            assert _state_rows_equal(_np(env.get_state())[skip], before[skip])
            for cur, old in zip((o, r, d, t), prev):
                assert np.array_equal(cur[skip], old[skip])
        # auto-reset of the replicas whose episode just ended
        ended = d.astype(bool)
        env.reset_done()
        for b in np.nonzero(ended)[0]:
            hosts[b].reset()
            assert close(_np(env.obs)[b], hosts[b].get_obs())
    assert np.array_equal(env.get_stp(), np.array([h.stp for h in hosts]))
    env.close()


# ---- 5. graph capture ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("name", ["lorenz", "vortex"])
def test_captured_graph_equals_eager_steps(name, dtype):
    _need_gpu()
    B, n = 1000, 16
    rng = np.random.default_rng(3)
    cls = V.VecLorenz if name == "lorenz" else V.VecVortex
    eager, graphed = cls(B, DEV, dtype), cls(B, DEV, dtype)
    if name == "lorenz":
        acts = torch.as_tensor(rng.integers(0, 3, (n, B)), dtype=torch.int32, device=DEV)
    else:
        acts = torch.as_tensor(rng.uniform(-1, 1, (n, B, 2)), dtype=eager.tdtype, device=DEV)
    eager.reset()
    seq = []
    for k in range(n):
        seq.append([x.clone() for x in eager.step(acts[k])[:4]])
    graphed.reset()
    g = graphed.capture(acts, n_steps=n)
    obs_seq, rwd_seq, done_seq, trunc_seq = g.replay()
    torch.cuda.synchronize()
    for k in range(n):
        assert torch.equal(obs_seq[k], seq[k][0]) and torch.equal(rwd_seq[k], seq[k][1]), k
        assert torch.equal(done_seq[k], seq[k][2]) and torch.equal(trunc_seq[k], seq[k][3]), k
    assert torch.equal(graphed.get_state(), eager.get_state())
    eager.close(), graphed.close()


# ---- 6. the two bindings --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lorenz", "vortex"])
def test_torch_ops_and_ctypes_agree_and_bad_actions_raise(name):
    _need_gpu()
    B, n = 300, 12
    rng = np.random.default_rng(9)
    cls = V.VecLorenz if name == "lorenz" else V.VecVortex
    for dtype in ("f32", "f64"):
        ops, ct = cls(B, DEV, dtype), cls(B, DEV, dtype)
        assert ops.use_torch_ops(True) and not ct.use_torch_ops(False)
        ops.reset(), ct.reset()
        assert torch.equal(ops.obs, ct.obs)
        for k in range(n):
            if name == "lorenz":
                a = None if k == 4 else torch.as_tensor(rng.integers(0, 3, B), dtype=torch.int32, device=DEV)
            else:
                a = None if k == 4 else torch.as_tensor(rng.uniform(-1, 1, (B, 2)), dtype=ops.tdtype, device=DEV)
            r1 = [x.clone() for x in ops.step(a)[:4]]
            r2 = [x.clone() for x in ct.step(a)[:4]]
            for x, y in zip(r1, r2):
                assert torch.equal(x, y), k
        assert torch.equal(ops.get_state(), ct.get_state())
        op = ops._ops[name + "_step"]
        outs = (ops.obs, ops.rwd, ops.done, ops.trunc, ops.status)
        if name == "lorenz":
            bad = [torch.zeros(B + 1, dtype=torch.int32, device=DEV), torch.zeros(B, dtype=torch.int64, device=DEV),
                   torch.zeros(B, dtype=torch.int32)]
        else:
            other = torch.float64 if dtype == "f32" else torch.float32
            bad = [torch.zeros((B, 3), dtype=ops.tdtype, device=DEV), torch.zeros((B, 2), dtype=other, device=DEV),
                   torch.zeros((B, 2), dtype=ops.tdtype)]
        for x in bad:
            with pytest.raises(RuntimeError):
                op(ops.h.value, x, *outs)
        with pytest.raises(RuntimeError):          # the wrong size through the env itself
            ops.step(torch.zeros(B + 1, dtype=torch.int32, device=DEV) if name == "lorenz"
                     else torch.zeros((B, 3), dtype=ops.tdtype, device=DEV))
        # calls that make no sense for these envs are errors, not crashes
        from beacon_amd import _lib
        assert ops.lib.bcn_set_variant(ops.h, 1) == 1                       # BCN_ERR_ARG
        for call in (lambda: ops.set_sched(0), lambda: ops.set_option("conv_plan", 0), lambda: ops.set_slow_mode_bound([]),
                     lambda: _lib.check(ops.lib.bcn_set_noise(ops.h, 0.1, 1, 0)),
                     lambda: _lib.check(ops.lib.bcn_set_fast_plugin(ops.h, None, 0))):
            with pytest.raises(_lib.BeaconHipError):
                call()
        ops.close(), ct.close()


# ---- 7. a large batch against the host port -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("name", ["lorenz", "vortex"])
def test_large_batch_matches_host_port(name, dtype):
    _need_gpu()
    B, n, nchk = 1 << 20, 10, 2000
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1234)
    cls = V.VecLorenz if name == "lorenz" else V.VecVortex
    env = cls(B, DEV, dtype)
    env.reset()
    if name == "lorenz":
        acts = torch.randint(0, 3, (n, B), generator=gen, device=DEV, dtype=torch.int32)
    else:
        acts = (2.0 * torch.rand((n, B, 2), generator=gen, device=DEV, dtype=torch.float64) - 1.0).to(env.tdtype)
    obs = []
    for k in range(n):
        obs.append(env.step(acts[k])[0].clone())
    rwd = _np(env.rwd)
    idx = np.sort(np.random.default_rng(8).choice(B, nchk, replace=False))
    idx[-1] = B - 1                                  # the last replica of the last workgroup
    A = _np(acts)[:, idx].astype(np.float64)
    dev_obs = np.stack([_np(o)[idx] for o in obs]).astype(np.float64)
    ref_obs = np.zeros_like(dev_obs)
    ref_rwd = np.zeros(nchk)
    for j in range(nchk):
        h = beacon_amd.lorenz() if name == "lorenz" else beacon_amd.vortex()
        h.reset()
        for k in range(n):
            o, r, _, _, _ = h.step(np.int64(A[k, j]) if name == "lorenz" else A[k, j])
            ref_obs[k, j] = o
        ref_rwd[j] = r
    if dtype == "f64" and name == "lorenz":
        assert np.array_equal(dev_obs, ref_obs) and np.array_equal(rwd[idx], ref_rwd)
    elif dtype == "f64":
        _report("vortex_f64_obs", float(np.abs(dev_obs - ref_obs).max()))
        _report("vortex_f64_rwd", float(np.abs(rwd[idx] - ref_rwd).max()))
    else:
        _report(name + "_f32_10steps", _rel(dev_obs, ref_obs))
    env.close()


# ---- 8. the two observation stores (option obs_stage) at workgroup boundaries -------------------------------------------------------
# float32 defaults to obs_stage 0 (one row per lane), float64 to 1 (rows staged through LDS): without the option <float, true> and
# <double, false> of both step kernels never run.  B = 257 leaves ONE live lane in the second workgroup, 300 leaves 44.
def _ode_make(name, dtype, B, stage):
    env = (V.VecLorenz if name == "lorenz" else V.VecVortex)(B, DEV, dtype)
    env.set_option("obs_stage", stage)
    return env


def _ode_actions(name, rng, n, B):
    return rng.integers(0, 3, (n, B)) if name == "lorenz" else rng.uniform(-1, 1, (n, B, 2))


def _ode_step(name, env, a):
    return env.step(torch.as_tensor(a, dtype=torch.int32, device=DEV) if name == "lorenz" else torch.as_tensor(a, device=DEV))


def _ode_check_rows(name, dtype, dev_obs, dev_rwd, ref_obs, ref_rwd, what):
    """device rows against the host port's, with the bounds of this file: float64 lorenz bit for bit, float64 vortex the measured
    cos / sin difference, float32 the bounds of the 10-step comparison from reset (observations, relative per column) and of the
    one-step comparisons (vortex reward, relative; lorenz reward: the sign, outside the rounding zone of x0)"""
    dev_obs, ref_obs = np.asarray(dev_obs, np.float64), np.asarray(ref_obs, np.float64)
    dev_rwd, ref_rwd = np.asarray(dev_rwd, np.float64), np.asarray(ref_rwd, np.float64)
    if dtype == "f64" and name == "lorenz":
        assert np.array_equal(dev_obs, ref_obs) and np.array_equal(dev_rwd, ref_rwd), what
    elif dtype == "f64":
        eo, er = float(np.abs(dev_obs - ref_obs).max()), float(np.abs(dev_rwd - ref_rwd).max())
        print("MEASURED %s vortex f64 obs %.3e rwd %.3e" % (what, eo, er))
        assert eo <= TOL["vortex_f64_obs"] and er <= TOL["vortex_f64_rwd"], (what, eo, er)
    else:
        eo = _rel(dev_obs, ref_obs)
        print("MEASURED %s %s f32 obs rel %.3e" % (what, name, eo))
        assert eo <= TOL[name + "_f32_10steps"], (what, eo)
        if name == "vortex":
            er = _rel(dev_rwd.reshape(-1), ref_rwd.reshape(-1))
            print("MEASURED %s vortex f32 rwd rel %.3e" % (what, er))
            assert er <= TOL["vortex_f32_rwd"], (what, er)
        else:
            x0 = ref_obs[..., 0]
            keep = np.abs(x0) > TOL["lorenz_f32_10steps"] * np.abs(x0).max()
            assert np.array_equal(dev_rwd[keep], ref_rwd[keep]), what


@pytest.mark.parametrize("B", [1, 257, 300])
@pytest.mark.parametrize("stage", [0, 1])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("name", ["lorenz", "vortex"])
def test_obs_store_variants_match_the_host_port(name, dtype, stage, B):
    """Five action steps from reset with random actions, every replica against the host port; float64: state, observations, reward,
    done and status of the two stores are bitwise equal (the arithmetic is the same code, built without contraction)."""
    _need_gpu()
    n = 5
    acts = _ode_actions(name, np.random.default_rng(B), n, B)
    env = _ode_make(name, dtype, B, stage)
    other = _ode_make(name, dtype, B, 1 - stage) if dtype == "f64" else None
    hosts = [(beacon_amd.lorenz if name == "lorenz" else beacon_amd.vortex)() for _ in range(B)]
    obs0, _ = env.reset()
    for b, h in enumerate(hosts):
        h.reset()
    _ode_check_rows(name, dtype, _np(obs0), np.zeros(B), np.stack([h.get_obs() for h in hosts]), np.zeros(B), "reset B=%d" % B)
    if other is not None:
        assert torch.equal(other.reset()[0], obs0)
    ref_obs, ref_rwd, dev_obs, dev_rwd = np.zeros((n, B, env.n_obs)), np.zeros((n, B)), [], []
    for k in range(n):
        obs, rwd, done, trunc, _ = _ode_step(name, env, acts[k])
        dev_obs.append(_np(obs).copy()), dev_rwd.append(_np(rwd).copy())
        for b, h in enumerate(hosts):
            o, r, d, t, _ = h.step(np.int64(acts[k, b]) if name == "lorenz" else acts[k, b])
            ref_obs[k, b], ref_rwd[k, b] = o, r
            assert bool(done[b]) == d and bool(trunc[b]) == t
        assert int(env.status.abs().max()) == 0
        if other is not None:
            o2 = _ode_step(name, other, acts[k])
            for x, y in zip((obs, rwd, done, trunc, env.status, env.get_state()), o2[:4] + (other.status, other.get_state())):
                assert torch.equal(x, y), (k, "the two stores differ")
    _ode_check_rows(name, dtype, np.stack(dev_obs), np.stack(dev_rwd), ref_obs, ref_rwd, "%d steps B=%d stage=%d" % (n, B, stage))
    assert np.array_equal(env.get_stp(), np.full(B, n))
    env.close()
    if other is not None:
        other.close()


@pytest.mark.parametrize("stage", [0, 1])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("name", ["lorenz", "vortex"])
def test_obs_store_variants_leave_masked_rows_untouched(name, dtype, stage):
    """B = 300 with rows switched off on both sides of the workgroup boundary and at the end of the partial workgroup (b = 255,
    256, 299): the staged store's guard is `e < n && act[e / NOBS]`, element by element.  The masked rows of an obs_out filled
    with a sentinel stay bitwise untouched, as do their state, reward, done and status; the live rows are right.  The same for a
    masked reset, which always stores through LDS."""
    _need_gpu()
    B, SENT = 300, -777.25
    acts = _ode_actions(name, np.random.default_rng(7), 3, B)
    env = _ode_make(name, dtype, B, stage)
    hosts = [(beacon_amd.lorenz if name == "lorenz" else beacon_amd.vortex)() for _ in range(B)]
    env.reset()
    for h in hosts:
        h.reset()
    _ode_step(name, env, acts[0])
    for b, h in enumerate(hosts):
        h.step(np.int64(acts[0, b]) if name == "lorenz" else acts[0, b])
    live = np.ones(B, bool)
    live[[255, 256, 299]] = False
    off = torch.as_tensor(~live, device=DEV)
    # a masked step
    env.obs.fill_(SENT)
    before = [x.clone() for x in (env.get_state(), env.rwd, env.done, env.trunc, env.status)]
    a = acts[1]
    obs, rwd, done, trunc, _ = env.step(torch.as_tensor(a, dtype=torch.int32 if name == "lorenz" else env.tdtype, device=DEV),
                                        mask=torch.as_tensor(live, device=DEV))
    assert torch.equal(obs[off], torch.full_like(obs[off], SENT)), "a masked observation row was written"
    for x, y in zip(before, (env.get_state(), rwd, done, trunc, env.status)):
        assert torch.equal(x[off], y[off])
    ref = [hosts[b].step(np.int64(a[b]) if name == "lorenz" else a[b]) for b in np.nonzero(live)[0]]
    _ode_check_rows(name, dtype, _np(obs)[live], _np(rwd)[live], np.stack([r[0] for r in ref]), np.array([r[1] for r in ref]),
                    "masked step stage=%d" % stage)
    # a masked reset: the rows on both sides of the boundary are reset, their neighbours are not
    sel = np.zeros(B, bool)
    sel[[0, 254, 257, 298]] = True
    env.obs.fill_(SENT)
    st_before = env.get_state().clone()
    obs, _ = env.reset(mask=torch.as_tensor(sel, device=DEV))
    keep = torch.as_tensor(~sel, device=DEV)
    assert torch.equal(obs[keep], torch.full_like(obs[keep], SENT)), "a masked observation row was written by reset"
    assert _state_rows_equal(_np(env.get_state())[~sel], _np(st_before)[~sel])
    for b in np.nonzero(sel)[0]:
        hosts[b].reset()
    _ode_check_rows(name, dtype, _np(obs)[sel], np.zeros(sel.sum()), np.stack([hosts[b].get_obs() for b in np.nonzero(sel)[0]]),
                    np.zeros(sel.sum()), "masked reset stage=%d" % stage)
    # ... and everybody steps on from there
    obs, rwd, _, _, _ = _ode_step(name, env, acts[2])
    ref = [h.step(np.int64(acts[2, b]) if name == "lorenz" else acts[2, b]) for b, h in enumerate(hosts)]
    # (b = 255, 256, 299 missed one step: their hosts did too)
    _ode_check_rows(name, dtype, _np(obs), _np(rwd), np.stack([r[0] for r in ref]), np.array([r[1] for r in ref]),
                    "step after the masked reset stage=%d" % stage)
    env.close()
