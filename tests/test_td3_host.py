"""CPU-side checks of the off-policy learner (no GPU): the header, the binding and the library of libbeacon_td3.so agree and the unit is
one of the build machinery's; the layouts; every cfg and argument error is refused without a device; tests/td3_ref.py's gradients
against central finite differences of both losses (the policy's runs through Q_1 into mu); the sampling and the append
restatements."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from conftest import ROOT

import td3_ref as R
from beacon_amd import td3 as _td3  # noqa: F401  (the module under test: importing it touches neither a compiler nor the GPU)
from test_actor_host import _bare

NAMES = {"bcn_td3_params_layout", "bcn_td3_params_bytes", "bcn_td3_state_layout", "bcn_td3_state_bytes", "bcn_td3_work_layout",
         "bcn_td3_work_bytes", "bcn_replay_layout", "bcn_replay_bytes", "bcn_td3_grid", "bcn_td3_act", "bcn_replay_append", "bcn_replay_sample",
         "bcn_td3_critic_grad", "bcn_td3_actor_grad", "bcn_td3_adam", "bcn_td3_polyak", "bcn_td3_last_error"}


def _lib():
    from beacon_amd import build, td3
    if build.hipcc() is None and not os.path.exists(td3.LIB):
        pytest.skip("no hipcc and no prebuilt library")
    return td3.load()


def _cfg(**kw):
    from beacon_amd import td3
    d = dict(batch=4, obs_dim=6, act_dim=2, dtype=0, hidden=(64, 64), activation="tanh", low=-1.0, high=1.0, n_critics=2)
    d.update(kw)
    return td3.make_cfg(**d)


def test_header_binding_and_library_agree():
    import beacon_amd
    from beacon_amd import learner, td3
    hdr = open(os.path.join(ROOT, "include", "beacon_td3.h")).read()
    declared = set(re.findall(r"BCN_TD3_API\s+[\w\s\*]+?\b(bcn_\w+)\s*\(", hdr))
    assert declared == NAMES == set(td3.SIGNATURES)
    assert int(re.search(r"#define BCN_TD3_API_VERSION (\d+)", hdr).group(1)) == td3.API_VERSION == 1
    for macro, value in (("MAX_IN", td3.MAX_IN), ("MAX_GRID", td3.MAX_GRID), ("MAX_SEGS", td3.MAX_SEGS)):
        assert int(re.search(r"#define BCN_TD3_%s (\d+)" % macro, hdr).group(1)) == value, macro
    L = _lib()
    for name in NAMES:
        assert hasattr(L, name)
    nm = subprocess.run(["nm", "-D", "--defined-only", td3.LIB], capture_output=True, text=True, check=True).stdout
    assert {l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("bcn_")} == NAMES
    # the structs the binding passes are the header's, field for field, and as large as the compiler makes them
    sizes = {"bcn_td3_cfg": 64, "bcn_td3_seg": 40, "bcn_td3_batch": 96, "bcn_td3_adam_hyper": 40}
    for struct, cls in (("bcn_td3_cfg", td3.Td3Cfg), ("bcn_td3_seg", td3.Td3Seg), ("bcn_td3_batch", td3.Td3Batch), ("bcn_td3_adam_hyper", td3.Td3Adam)):
        body = re.search(r"typedef struct \{([^{}]*)\} %s;" % struct, hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for d in body.split(";"):
            if d.strip():
                parts = [p.strip() for p in d.split(",")]
                fields += [parts[0].split()[-1]] + parts[1:]
        fields = [re.sub(r"\[\d+\]$", "", f.lstrip("*")) for f in fields]
        assert [f[:-4] if f.endswith("_dev") else f for f in fields] == [f[0] for f in cls._fields_], struct
        assert C.sizeof(cls) == sizes[struct], (struct, C.sizeof(cls))
    # the other headers know nothing of it
    for other in ("beacon_hip.h", "beacon_actor.h", "beacon_learner.h", "beacon_epochs.h"):
        assert "TD3" not in open(os.path.join(ROOT, "include", other)).read().upper().replace("BEACON_TD3_H", "")
    # a unit of its own, on the one build machinery; the network it shares is among what its .sig hashes
    assert td3._UNIT.__class__ is learner._UNIT.__class__
    assert [os.path.basename(s) for s in td3.sources()] == sorted(td3.FILE_FLAGS) == ["td3.hip", "td3_f64.hip"]
    assert td3.FILE_FLAGS["td3_f64.hip"] == ["-ffp-contract=off"]
    deps = {os.path.basename(f) for f in td3._UNIT.deps()}
    assert {"td3.hip", "td3_f64.hip", "td3_impl.h", "policy_net.h", "beacon_td3.h"} <= deps
    assert beacon_amd.TD3 is td3.TD3 and beacon_amd.Replay is td3.Replay and "TD3" in beacon_amd.__doc__
    assert "Not covered" in td3.TD3.__doc__ and "NORMALISED" in td3.Replay.__doc__
    assert td3.STATS == R.STATS


def test_struct_sizes_match_a_compiled_header(tmp_path):
    """sizeof of every struct as a C compiler lays the header out"""
    import shutil
    from beacon_amd import td3
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "beacon_td3.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(bcn_td3_cfg), '
                   'sizeof(bcn_td3_seg), sizeof(bcn_td3_batch), sizeof(bcn_td3_adam_hyper)); return 0; }\n')
    exe = tmp_path / "s"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(c) for c in (td3.Td3Cfg, td3.Td3Seg, td3.Td3Batch, td3.Td3Adam)]


@pytest.mark.parametrize("dtype,esz", [(0, 4), (1, 8)])
@pytest.mark.parametrize("hidden", [(7,), (33, 5), (17, 128, 3)])
@pytest.mark.parametrize("n_critics", [1, 2])
def test_layouts(dtype, esz, hidden, n_critics):
    from beacon_amd import td3
    _lib()
    od, ad, B = 33, 5, 9
    cfg = _cfg(batch=B, obs_dim=od, act_dim=ad, dtype=dtype, hidden=hidden, n_critics=n_critics)
    segs, nbytes = td3.layout("params", cfg)
    want = []
    for net, first, head in (("mu", od, ad), ("q1", od + ad, 1), ("q2", od + ad, 1))[:1 + n_critics]:
        dims = [first] + list(hidden) + [head]
        for l in range(len(hidden) + 1):
            want += [("%s_w%d" % (net, l), dims[l + 1] * dims[l]), ("%s_b%d" % (net, l), dims[l + 1])]
    assert [(s["name"], s["row_elems"]) for s in segs] == want == [(n, s["row_elems"]) for n, s in zip(R.segment_names(len(hidden), n_critics), segs)]

    def in_order(segs, nbytes, size_of):
        end = 0
        for s in segs:
            assert s["offset"] % 16 == 0 and end <= s["offset"] < end + 16 and s["planes"] == 0, s
            end = s["offset"] + s["row_elems"] * size_of[s["elem"]]
        assert end <= nbytes < end + 16 and nbytes % 16 == 0
    size_of = {td3.REAL: esz, td3.I32: 4, td3.U32: 4, td3.F64: 8, td3.U8: 1}
    in_order(segs, nbytes, size_of)
    assert all(s["elem"] == td3.REAL for s in segs)
    n = nbytes // esz
    st, sb = td3.layout("state", cfg)
    assert [(s["name"], s["elem"], s["row_elems"]) for s in st] == [("counters", td3.U32, B), ("step", td3.I32, 4), ("stats", td3.F64, 8),
                                                                    ("adam_m", td3.REAL, n), ("adam_v", td3.REAL, n)]
    in_order(st, sb, size_of)
    grid = int(td3.load().bcn_td3_grid(C.byref(cfg)))
    assert grid == min(td3.MAX_GRID, max(8, (64 << 20) // nbytes))
    for m in (1, 65):
        wk, wb = td3.layout("work", cfg, m)
        assert [(s["name"], s["elem"], s["row_elems"]) for s in wk] == [
            ("grad", td3.REAL, n), ("wg_stats", td3.F64, td3.MAX_GRID * 8), ("norm2", td3.F64, (n + 255) // 256), ("slabs", td3.REAL, grid * n),
            ("rw", td3.REAL, 3 * m), ("xa", td3.REAL, m * (od + ad)), ("xb", td3.REAL, m * (od + ad))]
        in_order(wk, wb, size_of)
        assert wk[0]["offset"] == 0
    for cap in (1, 17):
        rp, rb = td3.layout("replay", cfg, cap)
        assert [(s["name"], s["elem"], s["row_elems"]) for s in rp] == [
            ("head", td3.I32, 4), ("obs", td3.REAL, cap * od), ("act", td3.REAL, cap * ad), ("rwd", td3.REAL, cap), ("next_obs", td3.REAL, cap * od),
            ("boot", td3.U8, cap), ("live", td3.U8, cap)]
        in_order(rp, rb, size_of)


def test_cfg_errors_are_refused_by_the_library():
    from beacon_amd import td3
    L = _lib()
    for kw, word in ((dict(obs_dim=500, act_dim=13), "obs_dim"), (dict(act_dim=0), "act_dim"), (dict(act_dim=17), "act_dim"), (dict(n_critics=3), "n_critics"),
                     (dict(n_critics=0), "n_critics"), (dict(hidden=(129,)), "hidden"), (dict(hidden=()), "n_hidden"), (dict(activation=2), "activation"),
                     (dict(dtype=2), "dtype"), (dict(low=1.0, high=-1.0), "low"), (dict(obs_dim=0), "obs_dim")):
        cfg = _cfg(**kw)
        assert L.bcn_td3_params_bytes(C.byref(cfg)) == 0 and word in L.bcn_td3_last_error().decode(), kw
        with pytest.raises(td3.BeaconTd3Error, match=word):
            td3.layout("params", cfg)
        # the launches refuse it before they touch a device: the pointers are never read
        one = C.c_void_p(16)
        assert L.bcn_td3_act(C.byref(cfg), one, one, None, one, one, 0, 0.1, 0, 0, None) == 1 and word in L.bcn_td3_last_error().decode()
        assert L.bcn_td3_polyak(C.byref(cfg), one, one, 0.005, None) == 1
    assert td3.layout("params", _cfg(obs_dim=499, act_dim=13))[1] > 0              # 512 is allowed
    cfg = _cfg(batch=3)
    one = C.c_void_p(16)
    # T B > C
    assert L.bcn_replay_append(C.byref(cfg), 11, one, 4, one, one, one, one, one, one, one, one, None) == 1
    assert "capacity" in L.bcn_td3_last_error().decode()
    # no final_obs
    assert L.bcn_replay_append(C.byref(cfg), 12, one, 4, one, one, one, one, one, one, None, one, None) == 1
    assert "final_obs" in L.bcn_td3_last_error().decode()
    assert L.bcn_replay_sample(0, 0, one, one, None) == 1 and L.bcn_replay_sample(4, 0, None, one, None) == 1
    b = td3.Td3Batch(params=16, target=16, mem=16, idx=16, work=16, state=16, m=0, capacity=8, gamma=0.99, target_noise=0.2, noise_clip=0.5, seed=0)
    assert L.bcn_td3_critic_grad(C.byref(cfg), C.byref(b), None) == 1 and "m = 0" in L.bcn_td3_last_error().decode()
    b.m, b.gamma = 4, 1.5
    assert L.bcn_td3_critic_grad(C.byref(cfg), C.byref(b), None) == 1 and "gamma" in L.bcn_td3_last_error().decode()
    b.gamma, b.idx = 0.99, None
    assert L.bcn_td3_actor_grad(C.byref(cfg), C.byref(b), None) == 1 and "idx_dev" in L.bcn_td3_last_error().decode()
    h = td3.Td3Adam(lr=1e-3, beta1=1.0, beta2=0.999, eps=1e-8, max_grad_norm=0.0)
    assert L.bcn_td3_adam(C.byref(cfg), one, one, one, 0, C.byref(h), None) == 1 and "beta1" in L.bcn_td3_last_error().decode()
    h.beta1 = 0.9
    assert L.bcn_td3_adam(C.byref(cfg), one, one, one, 2, C.byref(h), None) == 1 and "which" in L.bcn_td3_last_error().decode()
    assert L.bcn_td3_polyak(C.byref(cfg), one, one, 1.5, None) == 1 and "tau" in L.bcn_td3_last_error().decode()


def test_argument_errors_need_no_gpu():
    from beacon_amd import TD3, Replay, _lib as main
    _lib()
    env = _bare("VecBurgers")
    for bad in ((), (64, 64, 64, 64), (0,), (129,), (64.5,), "wide", None):
        with pytest.raises(ValueError, match="hidden"):
            TD3(env, hidden=bad)
    with pytest.raises(ValueError, match="activation"):
        TD3(env, activation="gelu")
    for kw, word in ((dict(lr=-1.0), "lr"), (dict(gamma=1.5), "gamma"), (dict(tau=-0.1), "tau"), (dict(policy_delay=0), "policy_delay"),
                     (dict(policy_delay=2.0), "policy_delay"), (dict(explore_noise=float("nan")), "explore_noise"), (dict(target_noise=-1), "target_noise"),
                     (dict(noise_clip="x"), "noise_clip"), (dict(betas=(0.9,)), "betas"), (dict(betas=(0.9, 1.0)), "betas"), (dict(seed=-1), "seed"),
                     (dict(twin=1), "twin"), (dict(max_grad_norm="big"), "max_grad_norm")):
        with pytest.raises(ValueError, match=word):
            TD3(env, **kw)
    with pytest.raises(ValueError, match="per_jet"):
        TD3(_bare("VecShkadov"), per_jet=True)
    for cls in ("VecMixing", "VecLorenz"):
        with pytest.raises(ValueError, match="discrete"):
            TD3(_bare(cls))
    wide = types.SimpleNamespace(action_space=env.action_space, batch=4, tdtype=torch.float32, device="cpu",
                                 obs_dim=513 - int(np.asarray(env.action_space.low).size))
    with pytest.raises(ValueError, match="at most 512"):
        TD3(wide)
    agent = TD3(env, hidden=(7,))
    assert agent.max_grad_norm == 0.0 and agent.n_critics == 2 and not any(bool(v.any()) for v in agent.weights.values())
    with pytest.raises(ValueError, match="unknown"):
        agent.set_hyper(clip_range=0.2)
    with pytest.raises(ValueError, match="mode"):
        agent.act(mode="greedy")
    with pytest.raises(ValueError, match="obs must be"):
        agent.act(obs=torch.zeros(3, agent.obs_dim))
    with pytest.raises(RuntimeError, match="ROCm device"):
        agent.act(obs=torch.zeros(agent.batch, agent.obs_dim))
    d = TD3.ddpg(env, hidden=(7,))
    assert (d.twin, d.policy_delay, d.target_noise, d.n_critics) == (False, 1, 0.0, 1) and "q2_w0" not in d.weights
    with pytest.raises(ValueError, match="capacity"):
        agent.replay(0)
    with pytest.raises(ValueError, match="agent must be"):
        Replay(env, 8)
    mem = agent.replay(11)
    od, ad, B = agent.obs_dim, agent.act_dim, agent.batch

    def fake_ro(T, flags=main.RO_FINAL_OBS, batch=B, dtype=torch.float32):
        return types.SimpleNamespace(T=T, flags=flags, batch=batch, obs=torch.zeros(T + 1, batch, od, dtype=dtype), act=torch.zeros(T, batch, ad, dtype=dtype),
                                     rwd=torch.zeros(T, batch, dtype=dtype), final_obs=torch.zeros(T, batch, od if flags else 0, dtype=dtype),
                                     done=torch.zeros(T, batch, dtype=torch.uint8), trunc=torch.zeros(T, batch, dtype=torch.uint8),
                                     valid=torch.zeros(T, batch, dtype=torch.uint8), cursor=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="final_obs"):
        mem.append(fake_ro(2, flags=0))
    with pytest.raises(ValueError, match="T B <= 11"):
        mem.append(fake_ro(3))                       # T B = 12 > C = 11
    with pytest.raises(ValueError, match="replicas"):
        mem.append(fake_ro(2, batch=B + 1))
    with pytest.raises(ValueError, match="ro.obs must be float32"):
        mem.append(fake_ro(2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="ROCm device"):
        mem.append(fake_ro(2))
    with pytest.raises(ValueError, match="n_updates"):
        agent.plan(mem, 0, 4)
    with pytest.raises(ValueError, match="batch_size"):
        agent.plan(mem, 1, 0)
    with pytest.raises(ValueError, match="Replay of this agent"):
        agent.plan(d.replay(4), 1, 4)
    with pytest.raises(ValueError, match="q2"):
        d.load([(np.zeros((7, od)), np.zeros(7)), (np.zeros((ad, 7)), np.zeros(ad))], [(np.zeros((7, od + ad)), np.zeros(7)), (np.zeros((1, 7)), np.zeros(1))],
               [(np.zeros((7, od + ad)), np.zeros(7)), (np.zeros((1, 7)), np.zeros(1))])
    with pytest.raises(ValueError, match=r"q1\[0\] must be W \[7, %d\]" % (od + ad)):
        agent.load([(np.zeros((7, od)), np.zeros(7)), (np.zeros((ad, 7)), np.zeros(ad))], [(np.zeros((7, od)), np.zeros(7)), (np.zeros((1, 7)), np.zeros(1))],
                   [(np.zeros((7, od + ad)), np.zeros(7)), (np.zeros((1, 7)), np.zeros(1))])
    # checkpoints: a round trip, and a foreign state refused
    w = R.random_weights(od, ad, (7,), 2, 3)
    agent.load(*[[(w["%s_w%d" % (n, l)], w["%s_b%d" % (n, l)]) for l in range(2)] for n in ("mu", "q1", "q2")])
    assert torch.equal(agent.params, agent.target) and bool(agent.params.any())
    other = TD3(env, hidden=(7,))
    other.load_state_dict(agent.state_dict())
    assert torch.equal(other.params, agent.params) and torch.equal(other.target, agent.target) and other.seed == agent.seed
    with pytest.raises(ValueError, match="another agent"):
        TD3(env, hidden=(8,)).load_state_dict(agent.state_dict())
    with pytest.raises(ValueError, match="another agent"):
        d.load_state_dict(agent.state_dict())
    mem2 = agent.replay(11).load_state_dict(mem.state_dict())
    assert torch.equal(mem2.buf, mem.buf)
    with pytest.raises(ValueError, match="another memory"):
        agent.replay(12).load_state_dict(mem.state_dict())


# ---- td3_ref against finite differences ----------------------------------------------------------
def _fd_case(activation, n_critics, seed):
    od, ad, hidden, m = 5, 3, (6, 4), 40
    rng = np.random.default_rng(seed)
    W, Wt = R.random_weights(od, ad, hidden, n_critics, seed), R.random_weights(od, ad, hidden, n_critics, seed + 100, scale=3.0)      # (a saturated mu': a' reaches both bounds)
    batch = {"s": rng.standard_normal((m, od)), "a": rng.uniform(-1, 1, (m, ad)), "r": rng.standard_normal(m), "s2": rng.standard_normal((m, od)),
             "boot": (rng.uniform(size=m) > 0.3).astype(np.float64), "w": (rng.uniform(size=m) > 0.25).astype(np.float64)}
    for k in ("s", "a", "r", "s2"):
        batch[k][batch["w"] == 0] = np.nan               # a dead row may hold anything
    z = rng.standard_normal((m, ad))
    mk = lambda w, dtype=torch.float64: R.Ref(od, ad, hidden, activation, -0.5, 1.5, n_critics, w, Wt, dtype=dtype)
    return W, batch, z, mk


@pytest.mark.parametrize("activation", ["tanh", "relu"])
@pytest.mark.parametrize("n_critics", [1, 2])
def test_reference_gradients_match_finite_differences(activation, n_critics):
    W, batch, z, mk = _fd_case(activation, n_critics, 11)
    hyper = dict(gamma=0.9, target_noise=0.8, noise_clip=0.5)
    ref = mk(W)
    c, p = ref.critic(batch, z, **hyper), ref.policy(batch)
    assert np.isfinite(c["loss"]) and np.isfinite(p["loss"]) and batch["w"].sum() < len(batch["w"])
    # the case sits on both clamps of the noise and both bounds of a' in some live row: y there is a constant, as everywhere
    live = batch["w"] > 0
    assert (c["noise_raw"][live] > 0.5).any() and (c["noise_raw"][live] < -0.5).any()
    assert (c["a_raw"][live] > 1.5).any() and (c["a_raw"][live] < -0.5).any()
    assert set(c["grads"]) == set(ref.names_of(0)) and set(p["grads"]) == set(ref.names_of(1))
    assert not any(k.startswith("mu") for k in c["grads"]) and all(k.startswith("mu") for k in p["grads"])
    rng = np.random.default_rng(5)
    h = 1e-6
    for which, out, f in ((0, c, lambda r: r.critic(batch, z, **hyper)["loss"]), (1, p, lambda r: r.policy(batch)["loss"])):
        scale = max(float(g.abs().max()) for g in out["grads"].values())
        for name in ref.names_of(which):
            g = out["grads"][name].numpy()
            for _ in range(3):
                at = tuple(int(rng.integers(n)) for n in g.shape)
                Wp, Wm = {k: np.array(v) for k, v in W.items()}, {k: np.array(v) for k, v in W.items()}
                Wp[name][at] += h
                Wm[name][at] -= h
                fd = (f(mk(Wp)) - f(mk(Wm))) / (2 * h)
                # central difference: O(h^2 f''') truncation and eps |f| / h rounding, both below 1e-8 of the gradient's scale here
                assert abs(fd - g[at]) <= 1e-7 * max(1.0, scale), (name, at, fd, g[at])


def test_reference_policy_gradient_leaves_the_critic_alone_and_y_carries_no_gradient():
    W, batch, z, mk = _fd_case("tanh", 2, 3)
    ref = mk(W)
    # moving the TARGET parameters moves y and the loss, moving mu's parameters does not move the critic loss at all
    base = ref.critic(batch, z, 0.9, 0.2, 0.5)["loss"]
    W2 = {k: (v + 0.1 if k.startswith("mu") else v) for k, v in W.items()}
    assert mk(W2).critic(batch, z, 0.9, 0.2, 0.5)["loss"] == base
    # float32 runs the same arithmetic
    r32 = mk(W, torch.float32)
    assert abs(r32.critic(batch, z, 0.9, 0.2, 0.5)["loss"] - base) < 1e-5 * max(1.0, abs(base))
    # Adam's first step moves every element by lr (sign of the gradient), Polyak is the explicit formula
    g = ref.critic(batch, z, 0.9, 0.2, 0.5)["grads"]
    before = {k: v.clone() for k, v in ref.W.items()}
    ref.adam(0, g, lr=1e-3)
    for k in ref.names_of(0):
        moved = (ref.W[k] - before[k]).numpy()
        assert np.allclose(moved[g[k].numpy() != 0], -1e-3 * np.sign(g[k].numpy()[g[k].numpy() != 0]), rtol=1e-4)
    assert all(torch.equal(ref.W[k], before[k]) for k in ref.names_of(1)) and ref.steps == [1, 0]
    t0 = {k: v.clone() for k, v in ref.Wt.items()}
    ref.polyak(0.25)
    assert all(torch.allclose(ref.Wt[k], 0.75 * t0[k] + 0.25 * ref.W[k], rtol=0, atol=1e-15) for k in ref.names)


# ---- the sampling restatement --------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 7, 0xDEADBEEFCAFEF00D])
def test_sampling_restatement(seed):
    for stored in (1, 2, 17, 64 * 37):
        idx = R.sample_idx(5000, seed, stored, 3)
        assert idx.min() >= 0 and idx.max() < stored
        if stored == 1:
            assert not idx.any()
    assert not R.sample_idx(100, seed, 0, 0).any()                 # an empty memory: stored = max(head[1], 1)
    # chi-square over 64 bins at stored = 64 k: 63 degrees of freedom, the 99.99 % quantile is 117.4
    for k in (1, 37):
        n = 64 * 200
        idx = R.sample_idx(n, seed, 64 * k, 9)
        cnt = np.bincount(idx // k, minlength=64)
        chi2 = float(((cnt - n / 64) ** 2 / (n / 64)).sum())
        assert chi2 < 117.4, (seed, k, chi2)
    # another head[3] is another draw, another seed too; the same is the same
    a, b = R.sample_idx(256, seed, 1000, 0), R.sample_idx(256, seed, 1000, 1)
    assert (a != b).mean() > 0.9 and (a != R.sample_idx(256, seed + 1, 1000, 0)).mean() > 0.9
    assert np.array_equal(a, R.sample_idx(256, seed, 1000, 0))
    assert np.array_equal(R.sample_idx(300, seed, 1000, 0)[:256], a)          # a pure function of (i, seed, stored, drawn)
    # word 0 spelled out for one element
    from noise_ref import philox4x32_10
    w0 = int(philox4x32_10(5, 2, 0, 5, seed & 0xFFFFFFFF, seed >> 32)[0])
    assert int(R.sample_idx(6, seed, 1000, 2)[5]) == (w0 * 1000) >> 32


# ---- the append restatement ----------------------------------------------------------------------
def test_append_restatement():
    T, B, od, ad, Cn = 4, 3, 5, 2, 17
    rng = np.random.default_rng(0)

    def rollout(k):
        obs, act, rwd = rng.standard_normal((T + 1, B, od)), rng.standard_normal((T, B, ad)), rng.standard_normal((T, B))
        fo = rng.standard_normal((T, B, od)) + 100.0
        done, trunc, valid = np.zeros((T, B), np.uint8), np.zeros((T, B), np.uint8), np.ones((T, B), np.uint8)
        done[0, 1], trunc[1, 2] = 1, 1                       # terminated; (trunc alone: a flag pair the envs do not emit, boot = 1)
        done[2, 0] = trunc[2, 0] = 1                         # the time limit
        valid[3, 1] = 0
        return obs, act, rwd, done, trunc, valid, fo
    ring = R.Ring(Cn, od, ad)
    r1 = rollout(0)
    ring.append(*r1, cursor=T)
    assert ring.head.tolist() == [12, 12, 12, 0]
    obs, act, rwd, done, trunc, valid, fo = r1
    assert np.array_equal(ring.obs[:12], obs[:T].reshape(12, od)) and np.array_equal(ring.act[:12], act.reshape(12, ad))
    # the boot table over the four (done, trunc) combinations
    assert [int(ring.boot[t * B + b]) for t, b in ((0, 0), (0, 1), (1, 2), (2, 0))] == [1, 0, 1, 1]
    for t, b in ((0, 1), (1, 2), (2, 0)):
        assert np.array_equal(ring.next_obs[t * B + b], fo[t, b])
    assert np.array_equal(ring.next_obs[0], obs[1, 0]) and ring.live[:12].tolist() == [1] * 10 + [0, 1]
    # the second append wraps: slots 12 .. 16, then 0 .. 6
    r2 = rollout(1)
    ring.append(*r2, cursor=9)                               # a cursor beyond T counts T steps
    assert ring.head.tolist() == [7, 17, 24, 0]
    assert np.array_equal(ring.obs[12:], r2[0][:T].reshape(12, od)[:5]) and np.array_equal(ring.obs[:7], r2[0][:T].reshape(12, od)[5:])
    assert np.array_equal(ring.obs[7:12], obs[:T].reshape(12, od)[7:12])          # the rest keeps the first rollout's rows
    # a partial rollout appends its recorded steps only
    before = ring.obs.copy()
    ring.append(*rollout(2), cursor=2)
    assert ring.head.tolist() == [13, 17, 30, 0] and np.array_equal(ring.obs[13:], before[13:]) and not np.array_equal(ring.obs[7:13], before[7:13])
    ring.append(*rollout(3), cursor=-1)
    assert ring.head.tolist() == [13, 17, 30, 0]
    b = ring.gather([0, 13])
    assert set(b) == {"s", "a", "r", "s2", "boot", "w"} and b["s"].shape == (2, od)
