"""CPU-side checks of the DQN learner (no GPU): the header, the binding and the library of libbeacon_dqn.so agree and the unit is one of
the build machinery's; the layouts; every cfg and argument error is refused without a device, the LDS sum at the limits is TD3's; a
Replay for a DQN agent; tests/dqn_ref.py's gradients against central finite differences for all (double, dueling) combinations and
both losses; the first-maximum rule; stream 10; the restatement of the append of int32 actions."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from conftest import ROOT

import dqn_ref as R
from beacon_amd import DQN  # noqa: F401  (importing it touches neither a compiler nor the GPU)
from beacon_amd import dqn as _dqn  # noqa: F401
from noise_ref import philox4x32_10
from test_actor_host import _bare

NAMES = {"bcn_dqn_params_layout", "bcn_dqn_params_bytes", "bcn_dqn_state_layout", "bcn_dqn_state_bytes", "bcn_dqn_work_layout",
         "bcn_dqn_work_bytes", "bcn_dqn_grid", "bcn_dqn_lds_bytes", "bcn_dqn_act", "bcn_dqn_q", "bcn_dqn_append", "bcn_dqn_grad", "bcn_dqn_adam",
         "bcn_dqn_polyak", "bcn_dqn_last_error"}
STRUCTS = (("bcn_dqn_cfg", "DqnCfg", 40), ("bcn_dqn_seg", "DqnSeg", 40), ("bcn_dqn_batch", "DqnBatch", 128), ("bcn_dqn_adam_hyper", "DqnAdam", 40))


def _lib():
    from beacon_amd import build, dqn
    if build.hipcc() is None and not os.path.exists(dqn.LIB):
        pytest.skip("no hipcc and no prebuilt library")
    return dqn.load()


def _cfg(**kw):
    from beacon_amd import dqn
    d = dict(batch=4, obs_dim=6, n_actions=3, dtype=0, hidden=(64, 64), activation="tanh", dueling=False)
    d.update(kw)
    return dqn.make_cfg(**d)


def test_header_binding_and_library_agree():
    import beacon_amd
    from beacon_amd import dqn, learner, sac, td3
    hdr = open(os.path.join(ROOT, "include", "beacon_dqn.h")).read()
    declared = set(re.findall(r"BCN_DQN_API\s+[\w\s\*]+?\b(bcn_\w+)\s*\(", hdr))
    assert declared == NAMES == set(dqn.SIGNATURES)
    assert int(re.search(r"#define BCN_DQN_API_VERSION (\d+)", hdr).group(1)) == dqn.API_VERSION == 1
    for macro, value in (("MAX_OBS", dqn.MAX_OBS), ("MAX_ACTIONS", dqn.MAX_ACTIONS), ("MAX_GRID", dqn.MAX_GRID), ("MAX_SEGS", dqn.MAX_SEGS),
                         ("LDS_LIMIT", dqn.LDS_LIMIT)):
        assert int(re.search(r"#define BCN_DQN_%s (\d+)" % macro, hdr).group(1)) == value, macro
    stat_enum = re.search(r"enum \{ (BCN_DQN_STAT_LOSS[^}]*)\}", hdr).group(1)
    stat_names = [n.strip().split(" = ")[0][len("BCN_DQN_STAT_"):].lower() for n in stat_enum.split(",")][:-1]
    assert tuple(stat_names) == tuple(s.lower() for s in dqn.STATS) and dqn.STATS == R.STATS and len(stat_names) == 8
    assert [m for m, _ in sorted(dqn.MODES.items(), key=lambda kv: kv[1])] == ["greedy", "epsilon", "uniform"]
    assert re.search(r"enum \{ BCN_DQN_GREEDY = 0, BCN_DQN_EPSILON = 1, BCN_DQN_UNIFORM = 2 \}", hdr)
    L = _lib()
    for name in NAMES:
        assert hasattr(L, name)
    nm = subprocess.run(["nm", "-D", "--defined-only", dqn.LIB], capture_output=True, text=True, check=True).stdout
    assert {l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("bcn_")} == NAMES
    # the structs the binding passes are the header's, field for field, and as large as the compiler makes them
    for struct, cls, size in STRUCTS:
        cls = getattr(dqn, cls)
        body = re.search(r"typedef struct \{([^{}]*)\} %s;" % struct, hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for d in body.split(";"):
            if d.strip():
                parts = [p.strip() for p in d.split(",")]
                fields += [parts[0].split()[-1]] + parts[1:]
        fields = [re.sub(r"\[\d+\]$", "", f.lstrip("*")) for f in fields]
        assert [f[:-4] if f.endswith("_dev") else f for f in fields] == [f[0] for f in cls._fields_], struct
        assert C.sizeof(cls) == size, (struct, C.sizeof(cls))
    # the header states its formulas: both head forms, the first maximum, both targets, both losses, stream 10
    for word in ("Q_j = (V + A_j) - (sum_k A_k) / n", "FIRST maximum", "A NaN\n *                  never wins", "double_q:", "kappa (|delta| - kappa / 2)",
                 "counter (replica_offset + b, counters[b], 0, 10)", "mulhi32(w[3], n)"):
        assert word in hdr, word
    # a unit of its own, on the one build machinery; what it shares is among what its .sig hashes
    assert dqn._UNIT.__class__ is learner._UNIT.__class__ is td3._UNIT.__class__ is sac._UNIT.__class__
    assert [os.path.basename(s) for s in dqn.sources()] == sorted(dqn.FILE_FLAGS) == ["dqn.hip", "dqn_f64.hip"]
    assert dqn.FILE_FLAGS["dqn_f64.hip"] == ["-ffp-contract=off"]
    deps = {os.path.basename(f) for f in dqn._UNIT.deps()}
    assert {"dqn.hip", "dqn_f64.hip", "dqn_impl.h", "td3_impl.h", "policy_net.h", "beacon_dqn.h"} <= deps and "sac_impl.h" not in deps
    assert beacon_amd.DQN is dqn.DQN and "DQN" in beacon_amd.__doc__ and dqn.Replay is td3.Replay
    assert "Not covered" in dqn.DQN.__doc__ and all(w in dqn.DQN.__doc__ for w in ("per_jet", "prioritised", "n-step", "ShardedVecEnv", "noisy", "n > 16"))
    # the kernels are plain HIP C++: no inline assembly and no atomics in the unit's own sources
    for f in ("dqn.hip", "dqn_f64.hip", "dqn_impl.h"):
        text = open(os.path.join(ROOT, "beacon_amd", "csrc", "dqn", f)).read()
        assert "asm" not in re.sub(r"//.*", "", text) and "atomicAdd" not in text, f


def test_struct_sizes_match_a_compiled_header(tmp_path):
    """sizeof of every struct as a C compiler lays the header out"""
    import shutil
    from beacon_amd import dqn
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "beacon_dqn.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(bcn_dqn_cfg), '
                   'sizeof(bcn_dqn_seg), sizeof(bcn_dqn_batch), sizeof(bcn_dqn_adam_hyper)); return 0; }\n')
    exe = tmp_path / "s"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(getattr(dqn, c)) for _, c, _ in STRUCTS] == [s for _, _, s in STRUCTS]


@pytest.mark.parametrize("dtype,esz", [(0, 4), (1, 8)])
@pytest.mark.parametrize("hidden", [(7,), (33, 5), (17, 128, 3)])
@pytest.mark.parametrize("dueling", [False, True])
def test_layouts(dtype, esz, hidden, dueling):
    from beacon_amd import dqn
    _lib()
    od, n, B = 33, 5, 9
    cfg = _cfg(batch=B, obs_dim=od, n_actions=n, dtype=dtype, hidden=hidden, dueling=dueling)
    segs, nbytes = dqn.layout("params", cfg)
    dims = [od] + list(hidden) + [n + int(dueling)]
    want = []
    for l in range(len(hidden) + 1):
        want += [("q_w%d" % l, dims[l + 1] * dims[l]), ("q_b%d" % l, dims[l + 1])]
    assert [(s["name"], s["row_elems"]) for s in segs] == want == [(k, s["row_elems"]) for k, s in zip(R.segment_names(len(hidden)), segs)]

    def in_order(segs, nbytes, size_of):
        end = 0
        for s in segs:
            assert s["offset"] % 16 == 0 and end <= s["offset"] < end + 16 and s["planes"] == 0, s
            end = s["offset"] + s["row_elems"] * size_of[s["elem"]]
        assert end <= nbytes < end + 16 and nbytes % 16 == 0
    size_of = {dqn.REAL: esz, dqn.I32: 4, dqn.U32: 4, dqn.F64: 8, dqn.U8: 1}
    in_order(segs, nbytes, size_of)
    assert all(s["elem"] == dqn.REAL for s in segs)
    nel = nbytes // esz
    st, sb = dqn.layout("state", cfg)
    assert [(s["name"], s["elem"], s["row_elems"]) for s in st] == [("counters", dqn.U32, B), ("step", dqn.I32, 4), ("stats", dqn.F64, 8),
                                                                    ("adam_m", dqn.REAL, nel), ("adam_v", dqn.REAL, nel)]
    in_order(st, sb, size_of)
    grid = int(dqn.load().bcn_dqn_grid(C.byref(cfg)))
    assert grid == min(dqn.MAX_GRID, max(8, (64 << 20) // nbytes))
    wk, wb = dqn.layout("work", cfg)
    assert [(s["name"], s["elem"], s["row_elems"]) for s in wk] == [
        ("grad", dqn.REAL, nel), ("wg_stats", dqn.F64, dqn.MAX_GRID * 8), ("norm2", dqn.F64, (nel + 255) // 256), ("slabs", dqn.REAL, grid * nel)]
    in_order(wk, wb, size_of)
    assert wk[0]["offset"] == 0


def test_lds_sum_at_the_limits_is_td3s():
    """csrc/dqn/dqn_impl.h states the sum per dtype; the library computes it on the host and refuses what exceeds the limit before a
    launch.  The largest sum -- 16 head rows (n = 16 plain, n = 15 dueling) under 3 x 128 at obs_dim 512 -- is TD3's and SAC's, no larger."""
    from beacon_amd import dqn, sac, td3
    L = _lib()
    impl = open(os.path.join(ROOT, "beacon_amd", "csrc", "dqn", "dqn_impl.h")).read()
    worst = {}
    for dtype, (TB, KS) in ((0, (64, 64)), (1, (32, 32))):
        esz, TBP = (8 if dtype else 4), TB + 4
        for n, dueling, hidden in ((16, False, (128, 128, 128)), (15, True, (128, 128, 128)), (2, False, (7,)), (15, True, (3, 5)), (3, False, (128,)), (16, False, (1,))):
            cfg = _cfg(obs_dim=512, n_actions=n, dueling=dueling, hidden=hidden, dtype=dtype)
            hmax = max(hidden)
            wcols = ((max(hmax, n + int(dueling)) + 3) & ~3) + 4
            want = esz * (len(hidden) * hmax * TBP + KS * TBP + KS * wcols + 16 * TBP) + 4 * TB
            got = int(L.bcn_dqn_lds_bytes(C.byref(cfg)))
            assert got == want <= dqn.LDS_LIMIT, (dtype, n, dueling, hidden, got, want)
            worst[dtype] = max(worst.get(dtype, 0), got)
        assert dqn.layout("params", _cfg(obs_dim=512, n_actions=16, hidden=(128, 128, 128), dtype=dtype))[1] > 0
        # SAC's sum at its limits, computed by libbeacon_sac.so (TD3's by construction: tests/test_sac_host.py)
        assert worst[dtype] == int(sac.load().bcn_sac_lds_bytes(C.byref(sac.make_cfg(4, 6, 16, dtype, (128, 128, 128), "tanh"))))
    assert worst == {0: 160256, 1: 158336}
    assert "160 256" in impl and "158 336" in impl and "163 840" in impl and "DQN_LDS_LIMIT (160 * 1024)" in impl
    for hmax in (1, 64, 127, 128):
        for n, dueling in ((2, False), (8, True), (16, False), (15, True)):
            for nl in (1, 2, 3):
                for dtype in (0, 1):
                    assert 0 < int(L.bcn_dqn_lds_bytes(C.byref(_cfg(n_actions=n, dueling=dueling, hidden=(hmax,) * nl, dtype=dtype)))) <= worst[dtype]
    assert td3.MAX_IN == dqn.MAX_OBS == 512


def test_cfg_errors_are_refused_by_the_library():
    from beacon_amd import dqn
    L = _lib()
    one = C.c_void_p(16)
    for kw, word in ((dict(obs_dim=513), "obs_dim"), (dict(obs_dim=0), "obs_dim"), (dict(n_actions=1), "n_actions"), (dict(n_actions=17), "n_actions"),
                     (dict(n_actions=16, dueling=True), "n_actions + dueling"), (dict(dueling=2), "dueling"), (dict(hidden=(129,)), "hidden"),
                     (dict(hidden=()), "n_hidden"), (dict(activation=2), "activation"), (dict(dtype=2), "dtype")):
        cfg = _cfg(**kw)
        assert L.bcn_dqn_params_bytes(C.byref(cfg)) == 0 and word in L.bcn_dqn_last_error().decode(), kw
        assert L.bcn_dqn_lds_bytes(C.byref(cfg)) == 0 and L.bcn_dqn_grid(C.byref(cfg)) == 0 and L.bcn_dqn_work_bytes(C.byref(cfg)) == 0
        with pytest.raises(dqn.BeaconDqnError, match=re.escape(word)):
            dqn.layout("params", cfg)
        # the launches refuse it before they touch a device: the pointers are never read
        assert L.bcn_dqn_act(C.byref(cfg), one, one, None, one, one, 0, 0.0, None, 0, 0, None) == 1 and word in L.bcn_dqn_last_error().decode()
        assert L.bcn_dqn_q(C.byref(cfg), one, one, 4, one, None) == 1
        assert L.bcn_dqn_polyak(C.byref(cfg), one, one, 0.005, None) == 1
    assert dqn.layout("params", _cfg(obs_dim=512, n_actions=16))[1] > 0 and dqn.layout("params", _cfg(n_actions=15, dueling=True))[1] > 0
    assert L.bcn_dqn_state_bytes(C.byref(_cfg(batch=0))) == 0 and "batch" in L.bcn_dqn_last_error().decode()
    cfg = _cfg(batch=3)
    # bcn_dqn_act, bcn_dqn_q
    for args, word in (((None, one, None, one, one, 0, 0.0, None, 0, 0), "params_dev"), ((one, None, None, one, one, 0, 0.0, None, 0, 0), "obs_dev"),
                       ((one, one, None, None, one, 0, 0.0, None, 0, 0), "state_dev"), ((one, one, None, one, None, 0, 0.0, None, 0, 0), "actions_dev"),
                       ((one, one, None, one, one, 3, 0.0, None, 0, 0), "mode"), ((one, one, None, one, one, -1, 0.0, None, 0, 0), "mode"),
                       ((one, one, None, one, one, 1, 1.5, None, 0, 0), "eps"), ((one, one, None, one, one, 1, float("nan"), None, 0, 0), "eps"),
                       ((one, one, None, one, one, 1, 0.1, None, 0, -1), "replica_offset")):
        assert L.bcn_dqn_act(C.byref(cfg), *(args + (None,))) == 1 and word in L.bcn_dqn_last_error().decode(), word
    for args, word in (((None, one, 4, one), "params_dev"), ((one, None, 4, one), "rows_dev"), ((one, one, 4, None), "q_dev"), ((one, one, 0, one), "n_rows")):
        assert L.bcn_dqn_q(C.byref(cfg), *(args + (None,))) == 1 and word in L.bcn_dqn_last_error().decode(), word
    # bcn_dqn_append
    ok = [12, one, one, one, one, one, one, one, 4, one, one, one, one, one, one, one, one]
    for at, val, word in ((0, 0, "capacity"), (0, 11, "T B <= capacity"), (8, 0, "T >= 1"), (1, None, "head_dev"), (3, None, "act_dev"), (10, None, "ro_act_dev"),
                          (15, None, "ro_final_obs_dev"), (16, None, "ro_cursor_dev")):
        args = list(ok)
        args[at] = val
        assert L.bcn_dqn_append(C.byref(cfg), *(args + [None])) == 1 and word in L.bcn_dqn_last_error().decode(), (word, L.bcn_dqn_last_error().decode())
    # the gradient
    good = dict(params=16, target=16, obs=16, act=16, rwd=16, next_obs=16, boot=16, live=16, idx=16, work=16, state=16, m=4, capacity=8, gamma=0.99,
                huber=1.0, double_q=1, reserved=0)
    for kw, word in [(dict(m=0), "m = 0"), (dict(m=1 << 31), "m = "), (dict(gamma=1.5), "gamma"), (dict(gamma=float("nan")), "gamma"),
                     (dict(target=None), "target_dev"), (dict(capacity=0), "capacity"), (dict(huber=float("inf")), "huber"), (dict(double_q=2), "double_q"),
                     (dict(idx=None), "idx_dev"), (dict(work=None), "work_dev"), (dict(state=None), "state_dev"), (dict(params=None), "params_dev")] + \
                    [({seg: None}, seg + "_dev") for seg in ("obs", "act", "rwd", "next_obs", "boot", "live")]:
        b = dqn.DqnBatch(**dict(good, **kw))
        assert L.bcn_dqn_grad(C.byref(cfg), C.byref(b), None) == 1 and word in L.bcn_dqn_last_error().decode(), (kw, L.bcn_dqn_last_error().decode())
    assert L.bcn_dqn_grad(C.byref(cfg), None, None) == 1 and "batch is NULL" in L.bcn_dqn_last_error().decode()
    assert L.bcn_dqn_grad(None, C.byref(dqn.DqnBatch(**good)), None) == 1 and "cfg is NULL" in L.bcn_dqn_last_error().decode()
    # Adam and Polyak
    h = dqn.DqnAdam(lr=1e-3, beta1=1.0, beta2=0.999, eps=1e-8, max_grad_norm=0.0)
    assert L.bcn_dqn_adam(C.byref(cfg), one, one, one, C.byref(h), None) == 1 and "beta1" in L.bcn_dqn_last_error().decode()
    h.beta1 = 0.9
    assert L.bcn_dqn_adam(C.byref(cfg), one, None, one, C.byref(h), None) == 1 and "NULL" in L.bcn_dqn_last_error().decode()
    h.lr = -1.0
    assert L.bcn_dqn_adam(C.byref(cfg), one, one, one, C.byref(h), None) == 1 and "lr" in L.bcn_dqn_last_error().decode()
    h.lr, h.eps = 1e-3, -1.0
    assert L.bcn_dqn_adam(C.byref(cfg), one, one, one, C.byref(h), None) == 1 and "eps" in L.bcn_dqn_last_error().decode()
    assert L.bcn_dqn_polyak(C.byref(cfg), one, one, 1.5, None) == 1 and "tau" in L.bcn_dqn_last_error().decode()
    assert L.bcn_dqn_polyak(C.byref(cfg), None, one, 0.5, None) == 1 and "NULL" in L.bcn_dqn_last_error().decode()


def test_argument_errors_need_no_gpu():
    from beacon_amd import DQN, SAC, TD3, Replay, _lib as main
    _lib()
    env = _bare("VecLorenz")
    assert env.action_is_int and int(env.action_space.n) == 3
    for bad in ((), (64, 64, 64, 64), (0,), (129,), (64.5,), "wide", None):
        with pytest.raises(ValueError, match="hidden"):
            DQN(env, hidden=bad)
    with pytest.raises(ValueError, match="activation"):
        DQN(env, activation="gelu")
    for kw, word in ((dict(lr=-1.0), "lr"), (dict(gamma=1.5), "gamma"), (dict(tau=-0.1), "tau"), (dict(huber=0.0), "huber"), (dict(huber=-1.0), "huber"),
                     (dict(huber=float("nan")), "huber"), (dict(eps=1.5), "eps"), (dict(eps=-0.1), "eps"), (dict(eps=torch.zeros(2)), "eps"),
                     (dict(eps=torch.zeros(1, dtype=torch.float64)), "eps"), (dict(double=1), "double"), (dict(dueling=1), "dueling"),
                     (dict(betas=(0.9,)), "betas"), (dict(betas=(0.9, 1.0)), "betas"), (dict(seed=-1), "seed"), (dict(max_grad_norm="big"), "max_grad_norm"),
                     (dict(eps_adam=-1.0), "eps_adam"), (dict(replica_offset=-1), "replica_offset")):
        with pytest.raises(ValueError, match=word):
            DQN(env, **kw)
    with pytest.raises(ValueError, match="per_jet"):
        DQN(env, per_jet=True)
    # Box envs: refused, and the message names the agents that take them; TD3 and SAC keep refusing the discrete envs
    for cls in ("VecBurgers", "VecShkadov"):
        with pytest.raises(ValueError, match="Box.*TD3 / SAC"):
            DQN(_bare(cls))
    for cls in ("VecMixing", "VecLorenz"):
        for other in (TD3, SAC):
            with pytest.raises(ValueError, match="discrete"):
                other(_bare(cls))
    mk = lambda n, od=5: types.SimpleNamespace(action_space=types.SimpleNamespace(n=n), action_is_int=True, batch=4, tdtype=torch.float32, device="cpu", obs_dim=od)
    for n, kw in ((1, {}), (17, {}), (16, dict(dueling=True)), (0, {})):
        with pytest.raises(ValueError, match="2 .. 16"):
            DQN(mk(n), **kw)
    with pytest.raises(ValueError, match="at most 512"):
        DQN(mk(4, od=513))
    with pytest.raises(ValueError, match="ShardedVecEnv"):
        DQN(types.SimpleNamespace(action_space=types.SimpleNamespace(n=3), action_is_int=True, batch=4, tdtype=torch.float32, device="cpu", obs_dim=5, global_batch=8))
    assert DQN(mk(16), hidden=(7,)).n_head == 16 and DQN(mk(15), hidden=(7,), dueling=True).n_head == 16 and DQN(mk(4, od=512), hidden=(7,)).obs_dim == 512
    mix = DQN(_bare("VecMixing"))
    assert (mix.n_actions, mix.obs_dim) == (4, 192) and mix.weights["q_w2"].shape == (4, 64)
    agent = DQN(env, hidden=(7,), dueling=True)
    assert agent.max_grad_norm == 0.0 and agent.double and agent.dueling and agent.huber == 1.0 and agent.eps == 0.1 and agent.lr == 1e-3
    assert agent.lds_bytes > 0 and agent.actions.dtype == torch.int32 and tuple(agent.actions.shape) == (agent.batch,)
    assert not any(bool(v.any()) for v in agent.weights.values())
    assert agent.weights["q_w1"].shape == (4, 7) and agent.step_count.numel() == 4 and agent.stats.numel() == 8
    agent.set_hyper(huber=None, eps=torch.full((1,), 0.25))
    assert agent.huber is None and float(agent.eps[0]) == 0.25 and agent.state_dict()["hyper"]["eps"] == 0.25
    with pytest.raises(ValueError, match="unknown"):
        agent.set_hyper(policy_delay=2)
    with pytest.raises(ValueError, match="mode"):
        agent.act(mode="noisy")
    with pytest.raises(ValueError, match="obs must be"):
        agent.act(obs=torch.zeros(3, agent.obs_dim))
    with pytest.raises(ValueError, match="mask must hold"):
        agent.act(obs=torch.zeros(agent.batch, agent.obs_dim), mask=[1, 0])
    with pytest.raises(RuntimeError, match="ROCm device"):
        agent.act(obs=torch.zeros(agent.batch, agent.obs_dim))
    with pytest.raises(ValueError, match="obs must be"):
        agent.q_values(torch.zeros(3, agent.obs_dim + 1))
    with pytest.raises(RuntimeError, match="ROCm device"):
        agent.q_values(torch.zeros(3, agent.obs_dim))
    # a Replay for a DQN agent: the TD3 library's memory with act_dim = 1, constructed and refused without a GPU
    with pytest.raises(ValueError, match="capacity"):
        agent.replay(0)
    with pytest.raises(ValueError, match=r"Replay: agent must be a beacon_amd\.TD3, got 'VecLorenz'"):
        Replay(env, 8)
    mem = agent.replay(11)
    assert isinstance(mem, Replay) and mem in agent._mems and [s["name"] for s in mem.layout] == ["head", "obs", "act", "rwd", "next_obs", "boot", "live"]
    assert mem.obs.shape == (11, agent.obs_dim) and mem.act.shape == (11, 1) and mem.act.dtype == torch.float32
    # obs_dim = 512: bcn_replay_layout takes obs_dim + act_dim <= 512, so the ring is kept as a tensor per segment, with the same surface
    wide = DQN(mk(4, od=512), hidden=(7,))
    wmem = wide.replay(9)
    assert type(wmem) is _dqn.SplitReplay and isinstance(wmem, Replay) and wmem.obs.shape == (9, 512) and wmem.act.shape == (9, 1) and wmem in wide._mems
    assert wmem.head.dtype == torch.int32 and wmem.head.numel() == 4 and wmem.boot.dtype == wmem.live.dtype == torch.uint8 and wmem.lib is mem.lib
    assert type(DQN(mk(4, od=511), hidden=(7,)).replay(9)) is Replay
    wmem.rwd.fill_(2.0)
    other_w = wide.replay(9).load_state_dict(wmem.state_dict())
    assert torch.equal(other_w.rwd, wmem.rwd)
    with pytest.raises(ValueError, match="another memory"):
        wide.replay(8).load_state_dict(wmem.state_dict())
    with pytest.raises(ValueError, match=r"ro.act must be int32"):
        wmem.append(types.SimpleNamespace(T=2, flags=main.RO_FINAL_OBS, batch=4, act=torch.zeros(2, 4)))
    mem.head[3:4].fill_(5)
    agent.counters.fill_(3)
    agent.set_seed(9)
    assert int(mem.head[3]) == 0 and not bool(agent.counters.any()) and agent.seed == 9
    od, B = agent.obs_dim, agent.batch

    def fake_ro(T, flags=main.RO_FINAL_OBS, batch=B, dtype=torch.float32, act=None):
        return types.SimpleNamespace(T=T, flags=flags, batch=batch, obs=torch.zeros(T + 1, batch, od, dtype=dtype),
                                     act=torch.zeros(T, batch, dtype=torch.int32) if act is None else act,
                                     rwd=torch.zeros(T, batch, dtype=dtype), final_obs=torch.zeros(T, batch, od if flags else 0, dtype=dtype),
                                     done=torch.zeros(T, batch, dtype=torch.uint8), trunc=torch.zeros(T, batch, dtype=torch.uint8),
                                     valid=torch.zeros(T, batch, dtype=torch.uint8), cursor=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="final_obs"):
        mem.append(fake_ro(2, flags=0))
    with pytest.raises(ValueError, match="T B <= 11"):
        mem.append(fake_ro(3))                       # T B = 12 > C = 11
    with pytest.raises(ValueError, match="replicas"):
        mem.append(fake_ro(2, batch=B + 1))
    # a rollout whose actions are no int32 [T, B]: a Box env's, or another shape
    for act in (torch.zeros(2, B, 1), torch.zeros(2, B), torch.zeros(2, B, dtype=torch.int64), torch.zeros(2, B, 1, dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"ro.act must be int32 \[2, %d\]" % B):
            mem.append(fake_ro(2, act=act))
    with pytest.raises(ValueError, match="ro.obs must be float32"):
        mem.append(fake_ro(2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="ROCm device"):
        mem.append(fake_ro(2))
    # and TD3's memory keeps refusing integer actions
    with pytest.raises(ValueError, match="ro.act must be float32"):
        TD3(_bare("VecBurgers"), hidden=(7,)).replay(64).append(types.SimpleNamespace(**dict(vars(fake_ro(2, batch=4)), obs=torch.zeros(3, 4, _bare("VecBurgers").obs_dim),
                                                                                                 final_obs=torch.zeros(2, 4, _bare("VecBurgers").obs_dim))))
    with pytest.raises(ValueError, match="n_updates"):
        agent.plan(mem, 0, 4)
    with pytest.raises(ValueError, match="batch_size"):
        agent.plan(mem, 1, 0)
    with pytest.raises(ValueError, match="target_every"):
        agent.plan(mem, 1, 4, target_every=0)
    other = DQN(env, hidden=(7,), dueling=True)
    with pytest.raises(ValueError, match="Replay of this agent"):
        agent.plan(other.replay(4), 1, 4)
    plan = agent.plan(mem, 2, 4, target_every=2)
    assert set(plan.grads) == set(agent.weights) and plan.idx.numel() == 4 and plan.target_every == 2
    q = [(np.zeros((7, od)), np.zeros(7)), (np.zeros((4, 7)), np.zeros(4))]
    with pytest.raises(ValueError, match=r"q\[1\] must be W \[4, 7\]"):
        agent.load([q[0], (np.zeros((3, 7)), np.zeros(3))])              # a plain head: the value row is missing
    with pytest.raises(ValueError, match="2 .W, b. pairs"):
        agent.load(q[:1])
    import torch.nn as nn
    with pytest.raises(ValueError, match="expected Linear and Tanh"):
        agent.load_modules(nn.Sequential(nn.Linear(od, 7), nn.ReLU(), nn.Linear(7, 4)))
    torch.manual_seed(0)
    net = nn.Sequential(nn.Linear(od, 7), nn.Tanh(), nn.Linear(7, 4))
    agent.load_modules(net)
    assert torch.equal(agent.weights["q_w1"], net[2].weight.detach()) and torch.equal(agent.params, agent.target) and bool(agent.params.any())
    # checkpoints: a round trip, and a foreign state refused
    other.load_state_dict(agent.state_dict())
    assert torch.equal(other.params, agent.params) and torch.equal(other.target, agent.target) and other.seed == agent.seed
    assert other.huber is None and other.eps == 0.25
    with pytest.raises(ValueError, match="another agent"):
        DQN(env, hidden=(8,), dueling=True).load_state_dict(agent.state_dict())
    with pytest.raises(ValueError, match="another agent"):
        DQN(env, hidden=(7,)).load_state_dict(agent.state_dict())


# ---- dqn_ref against finite differences --------------------------------------------------------------
def _fd_case(activation, dueling, seed):
    od, n, hidden, m = 5, 4, (6, 4), 40
    rng = np.random.default_rng(seed)
    W, Wt = R.random_weights(od, n, hidden, dueling, seed, scale=2.0), R.random_weights(od, n, hidden, dueling, seed + 100, scale=2.0)
    batch = {"s": rng.standard_normal((m, od)), "a": rng.integers(0, n, (m, 1)).astype(np.float64), "r": 2.0 * rng.standard_normal(m),
             "s2": rng.standard_normal((m, od)), "boot": (rng.uniform(size=m) > 0.3).astype(np.float64), "w": (rng.uniform(size=m) > 0.25).astype(np.float64)}
    batch["a"][3], batch["a"][4], batch["a"][5] = n, -1.0, 1.5          # three dead rows by their action
    for k in ("s", "r", "s2"):
        batch[k][batch["w"] == 0] = np.nan               # a dead row may hold anything
    mk = lambda w: R.Ref(od, n, hidden, activation, dueling, w, Wt)
    return W, batch, mk


@pytest.mark.parametrize("activation", ["tanh", "relu"])
@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("dueling", [False, True])
@pytest.mark.parametrize("huber", [None, 0.7])
def test_reference_gradients_match_finite_differences(activation, double, dueling, huber):
    W, batch, mk = _fd_case(activation, dueling, 11)
    ref = mk(W)
    out = ref.loss(batch, 0.9, double, huber)
    lv = out["live"]
    assert np.isfinite(out["loss"]) and set(out["grads"]) == set(ref.names) and 0 < lv.sum() < len(lv) and not lv[3:6].any()
    assert (batch["boot"][lv] == 0).any() and (batch["boot"][lv] == 1).any()
    if huber is not None:                                # rows on both sides of the kink
        assert (np.abs(out["delta"][lv]) > huber).any() and (np.abs(out["delta"][lv]) < huber).any()
    # y carries no gradient: with boot = 0 everywhere and r = Q_a(s) the loss and its gradient vanish
    rng = np.random.default_rng(5)
    h = 1e-6
    f = lambda r: r.loss(batch, 0.9, double, huber)["loss"]
    scale = max(float(g.abs().max()) for g in out["grads"].values())
    L = len(ref.hidden)
    for name in ref.names:
        g = out["grads"][name].numpy()
        ats = [tuple(int(rng.integers(k)) for k in g.shape) for _ in range(3)]
        if dueling and name in ("q_w%d" % L, "q_b%d" % L):              # the value row and an advantage row
            ats = [(ref.n,) + a[1:] for a in ats[:2]] + [(1,) + a[1:] for a in ats[:2]]
        for at in ats:
            Wp, Wm = {k: np.array(v) for k, v in W.items()}, {k: np.array(v) for k, v in W.items()}
            Wp[name][at] += h
            Wm[name][at] -= h
            fd = (f(mk(Wp)) - f(mk(Wm))) / (2 * h)
            # central difference: O(h^2 f''') truncation and eps |f| / h rounding, both below 1e-8 of the gradient's scale here; j* and y
            # move with the parameters only through a kink, which the margins below keep 1e-3 away
            assert abs(fd - g[at]) <= 1e-7 * max(1.0, scale), (name, at, fd, g[at])
    assert all(v > 1e-3 for v in out["margins"].values()), out["margins"]
    if dueling:                                          # the advantage rows' bias gradients cancel: sum_j (1[j = a] - 1 / n) = 0
        assert abs(float(out["grads"]["q_b%d" % L][:ref.n].sum())) < 1e-12
    # the online network on s' decides j* only with double; the target's values are y's in both
    W2 = {k: v.numpy() + 0.05 * np.random.default_rng(1).standard_normal(v.shape) for k, v in ref.Wt.items()}
    assert R.Ref(5, 4, (6, 4), activation, dueling, W, W2).loss(batch, 0.9, double, huber)["loss"] != out["loss"]
    # the header's gradient at the head, from delta: g = w delta or w clamp(delta)
    g_want = out["delta"] * lv if huber is None else np.clip(out["delta"], -huber, huber) * lv
    W_sum = max(lv.sum(), 1)
    bias = out["grads"]["q_b%d" % L].numpy()
    a = np.where(lv, np.nan_to_num(batch["a"].reshape(-1)), 0).astype(int)
    want = np.zeros(ref.n + int(dueling))
    for i in np.flatnonzero(lv):
        if dueling:
            want[:ref.n] += g_want[i] * ((np.arange(ref.n) == a[i]) - 1.0 / ref.n)
            want[ref.n] += g_want[i]
        else:
            want[a[i]] += g_want[i]
    assert np.allclose(bias, want / W_sum, rtol=0, atol=1e-12)


def test_reference_statistics_adam_and_polyak():
    W, batch, mk = _fd_case("tanh", True, 3)
    ref = mk(W)
    out = ref.loss(batch, 0.9, True, 0.7)
    lv, st = out["live"], out["stats"]
    t, w, live = ref._batch(batch)
    q = ref.q_values(np.where(lv[:, None], np.nan_to_num(batch["s"]), 0.0))
    a = t["a"].numpy()
    assert st["W"] == lv.sum() and abs(st["q_mean"] - q[np.arange(len(lv)), a][lv].mean()) < 1e-12
    assert abs(st["q_max_mean"] - q.max(axis=1)[lv].mean()) < 1e-12 and abs(st["td_abs_mean"] - np.abs(out["delta"][lv]).mean()) < 1e-12
    assert abs(st["target_mean"] - out["y"][lv].mean()) < 1e-12 and st["spare"] == 0.0 and st["q_max_mean"] >= st["q_mean"]
    # the dueling combination: Q - V - A is the same shift for every action, and mean_j Q_j = V
    h = ref.head(ref.W, torch.as_tensor(np.where(lv[:, None], np.nan_to_num(batch["s"]), 0.0))).numpy()
    assert np.allclose(q.mean(axis=1), h[:, ref.n], atol=1e-12) and np.allclose(q - h[:, :ref.n], (q - h[:, :ref.n])[:, :1], atol=1e-12)
    # float32 runs the same arithmetic
    r32 = R.Ref(5, 4, (6, 4), "tanh", True, W, ref.Wt, dtype=torch.float32)
    assert abs(r32.loss(batch, 0.9, True, 0.7)["loss"] - out["loss"]) < 1e-5 * max(1.0, abs(out["loss"]))
    # Adam's first step moves every element by lr (sign of the gradient); Polyak is the explicit formula; tau = 1 the copy
    before = {k: v.clone() for k, v in ref.W.items()}
    ref.adam(out["grads"], lr=1e-3)
    for k in ref.names:
        moved, gk = (ref.W[k] - before[k]).numpy(), out["grads"][k].numpy()
        assert np.allclose(moved[gk != 0], -1e-3 * np.sign(gk[gk != 0]), rtol=1e-4)
    assert ref.steps == 1
    t0 = {k: v.clone() for k, v in ref.Wt.items()}
    ref.polyak(0.25)
    assert all(torch.allclose(ref.Wt[k], 0.75 * t0[k] + 0.25 * ref.W[k], rtol=0, atol=1e-15) for k in ref.names)
    ref.polyak(1.0)
    assert all(torch.equal(ref.Wt[k], ref.W[k]) for k in ref.names)


# ---- the first maximum ---------------------------------------------------------------------------------
def test_first_maximum_rule():
    nan, inf = np.nan, np.inf
    q = np.array([[1.0, 3.0, 3.0, 2.0],          # an exact tie: the lower index
                  [5.0, 5.0, 5.0, 5.0],
                  [nan, 1.0, 2.0, 2.0],          # a NaN never wins, wherever it stands
                  [1.0, nan, 0.5, 1.0],
                  [0.0, 1.0, nan, 1.0],
                  [nan, nan, nan, nan],          # nothing wins: 0
                  [-inf, -inf, -inf, -inf],
                  [nan, -inf, -1.0, nan],
                  [-0.0, 0.0, -1.0, 0.0],        # -0 == +0: no strict >
                  [1.0, inf, inf, nan]])
    assert R.first_argmax(q).tolist() == [1, 0, 2, 0, 1, 0, 0, 2, 0, 1]
    rng = np.random.default_rng(0)
    r = rng.standard_normal((500, 7))
    assert np.array_equal(R.first_argmax(r), r.argmax(axis=1))                    # without ties and NaN: numpy's
    r[:, 5] = r[:, 2]
    assert np.array_equal(R.first_argmax(r), r.argmax(axis=1)) and (R.first_argmax(r) != 5).all()
    assert np.allclose(R.top_two_gap(np.array([[1.0, 3.0, 3.0], [0.0, -1.0, 4.0]])), [0.0, 4.0])
    # acting: greedy takes it; epsilon takes the random action exactly where u < eps
    u, rnd = np.array([0.0, 0.5, 0.999]), np.array([3, 3, 3])
    q3 = q[:3]
    assert R.act(q3, u, rnd, R.GREEDY).tolist() == [1, 0, 2] and R.act(q3, u, rnd, R.UNIFORM).tolist() == [3, 3, 3]
    assert R.act(q3, u, rnd, R.EPSILON, 0.0).tolist() == [1, 0, 2] and R.act(q3, u, rnd, R.EPSILON, 1.0).tolist() == [3, 3, 3]
    assert R.act(q3, u, rnd, R.EPSILON, 0.5).tolist() == [3, 0, 2]


# ---- stream 10 -----------------------------------------------------------------------------------------
# pinned: (u of replica 0 at counter 11 in the float64 and the float32 form, rnd of replicas 0 .. 3 at counter 11 for n = 4)
PINNED = {
    0: (0.04929978729721951, 0.049299776554107666, [2, 2, 1, 3]),
    7: (0.5349322679511651, 0.5349322557449341, [3, 0, 1, 3]),
    0xDEADBEEFCAFEF00D: (0.05678832697412839, 0.05678832530975342, [1, 3, 1, 3]),
}


@pytest.mark.parametrize("seed", [0, 7, 0xDEADBEEFCAFEF00D])
def test_stream_10(seed):
    import td3_ref as R3
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    B, n, off = 4096, 4, 2 ** 32 - 3
    ctr = np.arange(B) * 3 + 1
    for dtype in (np.float32, np.float64):
        u, rnd = R.act_draws(seed, off, ctr, n, dtype)
        assert u.shape == rnd.shape == (B,) and u.min() >= 0.0 and u.max() < 1.0 and rnd.min() == 0 and rnd.max() == n - 1
        # one element spelled out from the words; the global index wraps at 2^32 inside the batch
        w = philox4x32_10(np.array([(off + 5) & 0xFFFFFFFF]), np.array([int(ctr[5])]), 0, 10, k0, k1)
        assert u[5] == float(R3.single_uniform(w, dtype)[0]) and rnd[5] == (int(w[3][0]) * n) >> 32
        # the u < eps decision at its ends: never at 0, always at 1
        q = np.tile(np.array([0.0, 1.0, 0.5, 0.25]), (B, 1))
        assert (R.act(q, u, rnd, R.EPSILON, 0.0) == 1).all() and np.array_equal(R.act(q, u, rnd, R.EPSILON, 1.0), rnd)
        mid = R.act(q, u, rnd, R.EPSILON, 0.3)
        assert np.array_equal(mid, np.where(u < 0.3, rnd, 1)) and abs((u < 0.3).mean() - 0.3) < 5 * np.sqrt(0.21 / B)
        # uniform over n = 4 bins: chi-square with 3 degrees of freedom, 16.27 is its 0.999 quantile
        counts = np.bincount(rnd, minlength=n)
        assert ((counts - B / n) ** 2 / (B / n)).sum() < 16.27, counts
        # the range of mulhi32 for every n of the agent
        for nn in (2, 3, 15, 16):
            r2 = R.act_draws(seed, off, ctr, nn, dtype)[1]
            assert r2.min() == 0 and r2.max() == nn - 1
        # another stream than TD3's exploration (4) and SAC's acting (7) at the same counters; a pure function of (replica, counter, seed)
        assert (u != R3.explore_uniforms(seed, off, ctr, 1, dtype)[:, 0]).mean() > 0.99
        assert np.array_equal(R.act_draws(seed, off, ctr[:100], n, dtype)[0], u[:100]) and (R.act_draws(seed + 1, off, ctr, n, dtype)[0] != u).mean() > 0.99
    u64, rnd = R.act_draws(seed, 0, np.full(4, 11), 4, np.float64)
    u32, _ = R.act_draws(seed, 0, np.full(4, 11), 4, np.float32)
    got = (float(u64[0]), float(u32[0]), rnd.tolist())
    assert got == PINNED[seed], (seed, got)


# ---- the append of int32 actions -----------------------------------------------------------------------
def test_append_restatement():
    """wrap, final_obs where the step ended an episode, the boot table, partial cursors, the int -> real conversion, an out-of-range
    action (stored as it is: the gradient launch makes the row dead)"""
    od, B, T, Cn = 3, 4, 3, 12
    rng = np.random.default_rng(2)
    for dtype in (np.float32, np.float64):
        ring = R.Ring(Cn, od, 1, dtype)
        runs = []
        for k, cursor in enumerate((3, 2, 0, 7, -1)):
            obs, fin = rng.standard_normal((T + 1, B, od)).astype(dtype), rng.standard_normal((T, B, od)).astype(dtype)
            act = rng.integers(0, 3, (T, B)).astype(np.int32)
            act[0, 1], act[1, 2] = 7, -2                                         # out of range: stored as 7.0 and -2.0
            rwd = rng.standard_normal((T, B)).astype(dtype)
            done, trunc = (rng.uniform(size=(T, B)) < 0.3).astype(np.uint8), (rng.uniform(size=(T, B)) < 0.3).astype(np.uint8)
            valid = (rng.uniform(size=(T, B)) < 0.8).astype(np.uint8)
            h0 = int(ring.head[0])
            R.append_int(ring, obs, act, rwd, done, trunc, valid, fin, cursor)
            nrec = min(max(cursor, 0), T)
            runs.append(nrec)
            assert int(ring.head[0]) == (h0 + nrec * B) % Cn and int(ring.head[1]) == min(sum(runs) * B, Cn) and int(ring.head[2]) == sum(runs) * B
            for t in range(nrec):
                for b in range(B):
                    s = (h0 + t * B + b) % Cn
                    f = bool(done[t, b] or trunc[t, b])
                    assert ring.act[s, 0] == float(act[t, b]) and ring.act.dtype == dtype and ring.rwd[s] == rwd[t, b]
                    assert np.array_equal(ring.next_obs[s], fin[t, b] if f else obs[t + 1, b]) and np.array_equal(ring.obs[s], obs[t, b])
                    assert ring.boot[s] == (0 if (done[t, b] and not trunc[t, b]) else 1) and ring.live[s] == valid[t, b]
        assert runs == [3, 2, 0, 3, 0] and int(ring.head[0]) == (8 * B) % Cn and int(ring.head[1]) == Cn      # the ring wrapped
        # every int32 below 2^24 is exact in float32; the reference refuses what is no int32 [T, B]
        assert np.float32(np.int32(2 ** 24 - 1)) == 2 ** 24 - 1
        with pytest.raises(AssertionError):
            R.append_int(ring, obs, act.astype(np.int64), rwd, done, trunc, valid, fin, 1)
    # the dead row: the reference's loss gives an out-of-range stored action weight 0
    ref = R.Ref(od, 3, (4,), "tanh", False, R.random_weights(od, 3, (4,), False, 0))
    ring.live[:] = 1
    out = ref.loss(ring.gather(np.arange(Cn)), 0.9)
    bad = (ring.act[:, 0] < 0) | (ring.act[:, 0] >= 3)
    assert bad.any() and not out["live"][bad].any() and out["live"][~bad].all() and out["stats"]["W"] == (~bad).sum()
