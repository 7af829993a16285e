"""CPU-side checks of soft actor-critic (no GPU): the header, the binding and the library of libbeacon_sac.so agree and the unit is one
of the build machinery's; the layouts; every cfg and argument error is refused without a device, the LDS sum at the limits is
accepted; a Replay for a SAC agent; tests/sac_ref.py's gradients against central finite differences of all three losses; log pi
against torch.distributions and, where tanh saturates, against the closed form; the three stream restatements."""
import ctypes as C
import math
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from conftest import ROOT

import sac_ref as R
import td3_ref as R3
from beacon_amd import SAC  # noqa: F401  (importing it touches neither a compiler nor the GPU)
from beacon_amd import sac as _sac  # noqa: F401
from noise_ref import philox4x32_10
from test_actor_host import _bare

NAMES = {"bcn_sac_params_layout", "bcn_sac_params_bytes", "bcn_sac_state_layout", "bcn_sac_state_bytes", "bcn_sac_work_layout",
         "bcn_sac_work_bytes", "bcn_sac_grid", "bcn_sac_lds_bytes", "bcn_sac_act", "bcn_sac_critic_grad", "bcn_sac_actor_grad", "bcn_sac_adam",
         "bcn_sac_polyak", "bcn_sac_last_error"}
STRUCTS = (("bcn_sac_cfg", "SacCfg", 64), ("bcn_sac_seg", "SacSeg", 40), ("bcn_sac_batch", "SacBatch", 128), ("bcn_sac_adam_hyper", "SacAdam", 40))


def _lib():
    from beacon_amd import build, sac
    if build.hipcc() is None and not os.path.exists(sac.LIB):
        pytest.skip("no hipcc and no prebuilt library")
    return sac.load()


def _cfg(**kw):
    from beacon_amd import sac
    d = dict(batch=4, obs_dim=6, act_dim=2, dtype=0, hidden=(64, 64), activation="tanh", low=-1.0, high=1.0, n_critics=2)
    d.update(kw)
    return sac.make_cfg(**d)


def test_header_binding_and_library_agree():
    import beacon_amd
    from beacon_amd import learner, sac, td3
    hdr = open(os.path.join(ROOT, "include", "beacon_sac.h")).read()
    declared = set(re.findall(r"BCN_SAC_API\s+[\w\s\*]+?\b(bcn_\w+)\s*\(", hdr))
    assert declared == NAMES == set(sac.SIGNATURES)
    assert int(re.search(r"#define BCN_SAC_API_VERSION (\d+)", hdr).group(1)) == sac.API_VERSION == 1
    for macro, value in (("MAX_IN", sac.MAX_IN), ("MAX_GRID", sac.MAX_GRID), ("MAX_SEGS", sac.MAX_SEGS), ("LDS_LIMIT", sac.LDS_LIMIT)):
        assert int(re.search(r"#define BCN_SAC_%s (\d+)" % macro, hdr).group(1)) == value, macro
    stat_enum = re.search(r"enum \{ (BCN_SAC_STAT_CRITIC_LOSS[^}]*)\}", hdr).group(1)
    stat_names = [n.strip().split(" = ")[0][len("BCN_SAC_STAT_"):].lower() for n in stat_enum.split(",")][:-1]
    assert len(stat_names) == len(sac.STATS) == 12 and sac.STATS == R.STATS
    L = _lib()
    for name in NAMES:
        assert hasattr(L, name)
    nm = subprocess.run(["nm", "-D", "--defined-only", sac.LIB], capture_output=True, text=True, check=True).stdout
    assert {l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("bcn_")} == NAMES
    # the structs the binding passes are the header's, field for field, and as large as the compiler makes them
    for struct, cls, size in STRUCTS:
        cls = getattr(sac, cls)
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
    # the cfg is bcn_td3_cfg's, field for field: the memory is laid out through libbeacon_td3.so with the same values
    assert [(n, t) for n, t in sac.SacCfg._fields_] == [(n, t) for n, t in td3.Td3Cfg._fields_]
    # the other five headers know nothing of it
    for other in ("beacon_hip.h", "beacon_actor.h", "beacon_learner.h", "beacon_epochs.h", "beacon_td3.h"):
        assert "SAC" not in open(os.path.join(ROOT, "include", other)).read().upper(), other
    # a unit of its own, on the one build machinery; what it shares is among what its .sig hashes
    assert sac._UNIT.__class__ is learner._UNIT.__class__ is td3._UNIT.__class__
    assert [os.path.basename(s) for s in sac.sources()] == sorted(sac.FILE_FLAGS) == ["sac.hip", "sac_f64.hip"]
    assert sac.FILE_FLAGS["sac_f64.hip"] == ["-ffp-contract=off"]
    deps = {os.path.basename(f) for f in sac._UNIT.deps()}
    assert {"sac.hip", "sac_f64.hip", "sac_impl.h", "td3_impl.h", "policy_net.h", "beacon_sac.h"} <= deps
    assert beacon_amd.SAC is sac.SAC and "SAC" in beacon_amd.__doc__ and sac.Replay is td3.Replay
    assert "Not covered" in sac.SAC.__doc__ and all(w in sac.SAC.__doc__ for w in ("per_jet", "prioritised", "n-step", "ShardedVecEnv"))


def test_struct_sizes_match_a_compiled_header(tmp_path):
    """sizeof of every struct as a C compiler lays the header out"""
    import shutil
    from beacon_amd import sac
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "beacon_sac.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(bcn_sac_cfg), '
                   'sizeof(bcn_sac_seg), sizeof(bcn_sac_batch), sizeof(bcn_sac_adam_hyper)); return 0; }\n')
    exe = tmp_path / "s"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(getattr(sac, c)) for _, c, _ in STRUCTS] == [s for _, _, s in STRUCTS]


@pytest.mark.parametrize("dtype,esz", [(0, 4), (1, 8)])
@pytest.mark.parametrize("hidden", [(7,), (33, 5), (17, 128, 3)])
@pytest.mark.parametrize("n_critics", [1, 2])
def test_layouts(dtype, esz, hidden, n_critics):
    from beacon_amd import sac
    _lib()
    od, ad, B = 33, 5, 9
    cfg = _cfg(batch=B, obs_dim=od, act_dim=ad, dtype=dtype, hidden=hidden, n_critics=n_critics)
    segs, nbytes = sac.layout("params", cfg)
    want = []
    for net, first, head in (("pi", od, 2 * ad), ("q1", od + ad, 1), ("q2", od + ad, 1))[:1 + n_critics]:
        dims = [first] + list(hidden) + [head]
        for l in range(len(hidden) + 1):
            want += [("%s_w%d" % (net, l), dims[l + 1] * dims[l]), ("%s_b%d" % (net, l), dims[l + 1])]
    want += [("log_alpha", 1)]
    assert [(s["name"], s["row_elems"]) for s in segs] == want == [(n, s["row_elems"]) for n, s in zip(R.segment_names(len(hidden), n_critics), segs)]

    def in_order(segs, nbytes, size_of):
        end = 0
        for s in segs:
            assert s["offset"] % 16 == 0 and end <= s["offset"] < end + 16 and s["planes"] == 0, s
            end = s["offset"] + s["row_elems"] * size_of[s["elem"]]
        assert end <= nbytes < end + 16 and nbytes % 16 == 0
    size_of = {sac.REAL: esz, sac.I32: 4, sac.U32: 4, sac.F64: 8, sac.U8: 1}
    in_order(segs, nbytes, size_of)
    assert all(s["elem"] == sac.REAL for s in segs)
    assert segs[-1]["name"] == "log_alpha" and segs[-1]["offset"] % 16 == 0 and segs[-1]["offset"] + 16 == nbytes      # the last segment, alone in its 16 bytes
    n = nbytes // esz
    st, sb = sac.layout("state", cfg)
    assert [(s["name"], s["elem"], s["row_elems"]) for s in st] == [("counters", sac.U32, B), ("step", sac.I32, 8), ("stats", sac.F64, 12),
                                                                    ("adam_m", sac.REAL, n), ("adam_v", sac.REAL, n)]
    in_order(st, sb, size_of)
    grid = int(sac.load().bcn_sac_grid(C.byref(cfg)))
    assert grid == min(sac.MAX_GRID, max(8, (64 << 20) // nbytes))
    for m in (1, 65):
        wk, wb = sac.layout("work", cfg, m)
        assert [(s["name"], s["elem"], s["row_elems"]) for s in wk] == [
            ("grad", sac.REAL, n), ("wg_stats", sac.F64, sac.MAX_GRID * 12), ("norm2", sac.F64, (n + 255) // 256), ("slabs", sac.REAL, grid * n),
            ("rw", sac.REAL, 4 * m), ("xa", sac.REAL, m * (od + ad)), ("xb", sac.REAL, m * (od + ad))]
        in_order(wk, wb, size_of)
        assert wk[0]["offset"] == 0


def test_lds_sum_is_stated_checked_and_accepted_at_the_limits():
    """csrc/sac/sac_impl.h states the sum per dtype; the library computes it on the host and refuses what exceeds the limit before a
    launch.  Within the cfg ranges the largest sum is act_dim 16 under 3 x 128, and it must be accepted in both dtypes."""
    from beacon_amd import sac
    L = _lib()
    impl = open(os.path.join(ROOT, "beacon_amd", "csrc", "sac", "sac_impl.h")).read()
    worst = {}
    for dtype, (TB, KS) in ((0, (64, 64)), (1, (32, 32))):
        esz, TBP = (8 if dtype else 4), TB + 4
        for ad, hidden in ((16, (128, 128, 128)), (1, (7,)), (16, (33, 5)), (3, (128,)), (16, (1,))):
            cfg = _cfg(act_dim=ad, hidden=hidden, dtype=dtype)
            hmax = max(hidden)
            wcols = ((max(hmax, 2 * ad) + 3) & ~3) + 4
            want = esz * (len(hidden) * hmax * TBP + KS * TBP + KS * wcols + 16 * TBP) + 4 * TB
            got = int(L.bcn_sac_lds_bytes(C.byref(cfg)))
            assert got == want <= sac.LDS_LIMIT, (dtype, ad, hidden, got, want)
            worst[dtype] = max(worst.get(dtype, 0), got)
        assert 2 * 16 <= KS                                   # the head's 32 rows fit the staging buffer they are held in
        assert sac.layout("params", _cfg(act_dim=16, hidden=(128, 128, 128), dtype=dtype))[1] > 0
    assert worst == {0: 160256, 1: 158336}
    assert "160 256" in impl and "158 336" in impl and "163 840" in impl and "SAC_LDS_LIMIT (160 * 1024)" in impl
    # no cfg inside the ranges exceeds the limit (the sum grows with every width and with act_dim, and the largest is accepted), so
    # the library's refusal of a larger sum cannot be provoked through the ABI: what is checked here is that the sum it tests is
    # the stated one, for every width up to the limits
    for hmax in (1, 64, 127, 128):
        for ad in (1, 8, 16):
            for L in (1, 2, 3):
                for dtype in (0, 1):
                    assert 0 < int(_lib().bcn_sac_lds_bytes(C.byref(_cfg(act_dim=ad, hidden=(hmax,) * L, dtype=dtype)))) <= worst[dtype]


def test_cfg_errors_are_refused_by_the_library():
    from beacon_amd import sac
    L = _lib()
    one = C.c_void_p(16)
    for kw, word in ((dict(obs_dim=500, act_dim=13), "obs_dim"), (dict(act_dim=0), "act_dim"), (dict(act_dim=17), "act_dim"), (dict(n_critics=3), "n_critics"),
                     (dict(n_critics=0), "n_critics"), (dict(hidden=(129,)), "hidden"), (dict(hidden=()), "n_hidden"), (dict(activation=2), "activation"),
                     (dict(dtype=2), "dtype"), (dict(low=1.0, high=-1.0), "low"), (dict(low=0.5, high=0.5), "low < high"),
                     (dict(low=float("-inf"), high=1.0), "finite"), (dict(obs_dim=0), "obs_dim")):
        cfg = _cfg(**kw)
        assert L.bcn_sac_params_bytes(C.byref(cfg)) == 0 and word in L.bcn_sac_last_error().decode(), kw
        assert L.bcn_sac_lds_bytes(C.byref(cfg)) == 0 and L.bcn_sac_grid(C.byref(cfg)) == 0
        with pytest.raises(sac.BeaconSacError, match=word):
            sac.layout("params", cfg)
        # the launches refuse it before they touch a device: the pointers are never read
        assert L.bcn_sac_act(C.byref(cfg), one, one, None, one, one, 0, 0, 0, None) == 1 and word in L.bcn_sac_last_error().decode()
        assert L.bcn_sac_polyak(C.byref(cfg), one, one, 0.005, None) == 1
    assert sac.layout("params", _cfg(obs_dim=499, act_dim=13))[1] > 0              # 512 is allowed
    assert L.bcn_sac_state_bytes(C.byref(_cfg(batch=0))) == 0 and "batch" in L.bcn_sac_last_error().decode()
    assert L.bcn_sac_work_bytes(C.byref(_cfg()), 0) == 0 and "m = 0" in L.bcn_sac_last_error().decode()
    cfg = _cfg(batch=3)
    # bcn_sac_act
    for args, word in (((None, one, None, one, one, 0, 0, 0), "params_dev"), ((one, None, None, one, one, 0, 0, 0), "obs_dev"),
                       ((one, one, None, None, one, 0, 0, 0), "state_dev"), ((one, one, None, one, None, 0, 0, 0), "actions_dev"),
                       ((one, one, None, one, one, 3, 0, 0), "mode"), ((one, one, None, one, one, -1, 0, 0), "mode"),
                       ((one, one, None, one, one, 1, 0, -1), "replica_offset")):
        assert L.bcn_sac_act(C.byref(cfg), *(args + (None,))) == 1 and word in L.bcn_sac_last_error().decode(), word
    # the gradients
    good = dict(params=16, target=16, obs=16, act=16, rwd=16, next_obs=16, boot=16, live=16, idx=16, work=16, state=16, m=4, capacity=8, gamma=0.99,
                target_entropy=-2.0, seed=0)
    for fn, kw, word in [(L.bcn_sac_critic_grad, dict(m=0), "m = 0"), (L.bcn_sac_critic_grad, dict(m=1 << 31), "m = "), (L.bcn_sac_critic_grad, dict(gamma=1.5), "gamma"),
                         (L.bcn_sac_critic_grad, dict(gamma=float("nan")), "gamma"), (L.bcn_sac_critic_grad, dict(target=None), "target_dev"),
                         (L.bcn_sac_critic_grad, dict(capacity=0), "capacity"), (L.bcn_sac_actor_grad, dict(target_entropy=float("inf")), "target_entropy"),
                         (L.bcn_sac_actor_grad, dict(idx=None), "idx_dev"), (L.bcn_sac_actor_grad, dict(work=None), "work_dev"),
                         (L.bcn_sac_actor_grad, dict(state=None), "state_dev"), (L.bcn_sac_actor_grad, dict(params=None), "params_dev")] + \
                        [(f, {seg: None}, seg + "_dev") for f in (L.bcn_sac_critic_grad, L.bcn_sac_actor_grad) for seg in ("obs", "act", "rwd", "next_obs", "boot", "live")]:
        b = sac.SacBatch(**dict(good, **kw))
        assert fn(C.byref(cfg), C.byref(b), None) == 1 and word in L.bcn_sac_last_error().decode(), (kw, L.bcn_sac_last_error().decode())
    assert L.bcn_sac_critic_grad(C.byref(cfg), None, None) == 1 and "batch is NULL" in L.bcn_sac_last_error().decode()
    assert L.bcn_sac_critic_grad(None, C.byref(sac.SacBatch(**good)), None) == 1 and "cfg is NULL" in L.bcn_sac_last_error().decode()
    # Adam and Polyak
    h = sac.SacAdam(lr=1e-3, beta1=1.0, beta2=0.999, eps=1e-8, max_grad_norm=0.0)
    assert L.bcn_sac_adam(C.byref(cfg), one, one, one, 0, C.byref(h), None) == 1 and "beta1" in L.bcn_sac_last_error().decode()
    h.beta1 = 0.9
    for which in (3, -1):
        assert L.bcn_sac_adam(C.byref(cfg), one, one, one, which, C.byref(h), None) == 1 and "which" in L.bcn_sac_last_error().decode()
    assert L.bcn_sac_adam(C.byref(cfg), one, None, one, 2, C.byref(h), None) == 1 and "NULL" in L.bcn_sac_last_error().decode()
    h.lr = -1.0
    assert L.bcn_sac_adam(C.byref(cfg), one, one, one, 2, C.byref(h), None) == 1 and "lr" in L.bcn_sac_last_error().decode()
    h.lr, h.eps = 1e-3, -1.0
    assert L.bcn_sac_adam(C.byref(cfg), one, one, one, 2, C.byref(h), None) == 1 and "eps" in L.bcn_sac_last_error().decode()
    assert L.bcn_sac_polyak(C.byref(cfg), one, one, 1.5, None) == 1 and "tau" in L.bcn_sac_last_error().decode()
    assert L.bcn_sac_polyak(C.byref(cfg), None, one, 0.5, None) == 1 and "NULL" in L.bcn_sac_last_error().decode()


def test_argument_errors_need_no_gpu():
    from beacon_amd import SAC, TD3, Replay, _lib as main
    _lib()
    env = _bare("VecBurgers")
    for bad in ((), (64, 64, 64, 64), (0,), (129,), (64.5,), "wide", None):
        with pytest.raises(ValueError, match="hidden"):
            SAC(env, hidden=bad)
    with pytest.raises(ValueError, match="activation"):
        SAC(env, activation="gelu")
    for kw, word in ((dict(lr=-1.0), "lr"), (dict(gamma=1.5), "gamma"), (dict(tau=-0.1), "tau"), (dict(alpha=0.0), "alpha"), (dict(alpha=-1.0), "alpha"),
                     (dict(alpha=float("nan")), "alpha"), (dict(auto_alpha=1), "auto_alpha"), (dict(target_entropy="low"), "target_entropy"),
                     (dict(target_entropy=float("inf")), "target_entropy"), (dict(lr_alpha=-1e-3), "lr_alpha"), (dict(betas=(0.9,)), "betas"),
                     (dict(betas=(0.9, 1.0)), "betas"), (dict(seed=-1), "seed"), (dict(twin=1), "twin"), (dict(max_grad_norm="big"), "max_grad_norm"),
                     (dict(eps=-1.0), "eps"), (dict(replica_offset=-1), "replica_offset")):
        with pytest.raises(ValueError, match=word):
            SAC(env, **kw)
    with pytest.raises(ValueError, match="per_jet"):
        SAC(_bare("VecShkadov"), per_jet=True)
    for cls in ("VecMixing", "VecLorenz"):
        with pytest.raises(ValueError, match="discrete"):
            SAC(_bare(cls))
    n_act = int(np.asarray(env.action_space.low).size)
    mk = lambda lo, hi, od=5: types.SimpleNamespace(action_space=types.SimpleNamespace(low=np.asarray(lo, dtype=np.float64), high=np.asarray(hi, dtype=np.float64)),
                                                    batch=4, tdtype=torch.float32, device="cpu", obs_dim=od)
    with pytest.raises(ValueError, match="at most 512"):
        SAC(mk([-1.0] * n_act, [1.0] * n_act, od=513 - n_act))
    with pytest.raises(ValueError, match="one finite scalar bound pair"):
        SAC(mk([-1.0, -2.0], [1.0, 1.0]))
    with pytest.raises(ValueError, match="one finite scalar bound pair"):
        SAC(mk([-1.0, -1.0], [1.0, np.inf]))
    with pytest.raises(ValueError, match="low < high"):
        SAC(mk([0.5, 0.5], [0.5, 0.5]))                          # low == high: TD3 takes it, ln h does not
    assert TD3(mk([0.5, 0.5], [0.5, 0.5]), hidden=(7,)).low == 0.5
    with pytest.raises(ValueError, match="1 .. 16"):
        SAC(mk([-1.0] * 17, [1.0] * 17))
    agent = SAC(env, hidden=(7,), alpha=0.5)
    assert agent.max_grad_norm == 0.0 and agent.n_critics == 2 and agent.auto_alpha and agent.entropy_target() == -float(agent.act_dim)
    assert agent.alpha_lr() == agent.lr == 3e-4 and agent.lds_bytes > 0
    assert abs(float(agent.log_alpha[0]) - math.log(0.5)) < 1e-6
    assert not any(bool(v.any()) for k, v in agent.weights.items() if k != "log_alpha")
    assert agent.weights["pi_w1"].shape == (2 * agent.act_dim, 7) and agent.step_count.numel() == 8 and agent.stats.numel() == 12
    agent.set_hyper(target_entropy=-0.5, lr_alpha=1e-2)
    assert agent.entropy_target() == -0.5 and agent.alpha_lr() == 1e-2
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
    single = SAC(env, hidden=(7,), twin=False, auto_alpha=False)
    assert (single.twin, single.n_critics, single.auto_alpha) == (False, 1, False) and "q2_w0" not in single.weights
    # a Replay for a SAC agent: the TD3 library's memory, constructed and refused without a GPU
    with pytest.raises(ValueError, match="capacity"):
        agent.replay(0)
    with pytest.raises(ValueError, match=r"Replay: agent must be a beacon_amd\.TD3, got 'VecBurgers'"):
        Replay(env, 8)
    mem = agent.replay(11)
    tmem = TD3(env, hidden=(7,)).replay(11)
    assert isinstance(mem, Replay) and mem.layout == tmem.layout and mem.buf.numel() == tmem.buf.numel() and mem in agent._mems
    assert mem.obs.shape == (11, agent.obs_dim) and mem.act.shape == (11, agent.act_dim) and mem.lib is tmem.lib
    mem.head[3:4].fill_(5)
    agent.step_count[3:5].fill_(7)
    agent.set_seed(9)
    assert int(mem.head[3]) == 0 and agent.step_count.tolist() == [0] * 8 and agent.seed == 9
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
    with pytest.raises(ValueError, match="idx must be"):
        mem.sample(torch.zeros(4))
    with pytest.raises(ValueError, match="n_updates"):
        agent.plan(mem, 0, 4)
    with pytest.raises(ValueError, match="batch_size"):
        agent.plan(mem, 1, 0)
    with pytest.raises(ValueError, match="Replay of this agent"):
        agent.plan(single.replay(4), 1, 4)
    with pytest.raises(ValueError, match="Replay of this agent"):
        agent.plan(tmem, 1, 4)
    plan = agent.plan(mem, 2, 4)
    assert set(plan.grads) == set(agent.weights) and plan.rw.numel() == 4 * 4
    pi = [(np.zeros((7, od)), np.zeros(7)), (np.zeros((2 * ad, 7)), np.zeros(2 * ad))]
    q = [(np.zeros((7, od + ad)), np.zeros(7)), (np.zeros((1, 7)), np.zeros(1))]
    with pytest.raises(ValueError, match="q2"):
        single.load(pi, q, q)
    with pytest.raises(ValueError, match=r"pi\[1\] must be W \[%d, 7\]" % (2 * ad)):
        agent.load([pi[0], (np.zeros((ad, 7)), np.zeros(ad))], q, q)              # a TD3 head: half the rows
    import torch.nn as nn
    with pytest.raises(ValueError, match="expected Linear and Tanh"):
        agent.load_modules(nn.Sequential(nn.Linear(od, 7), nn.ReLU(), nn.Linear(7, 2 * ad)), None, None)
    # checkpoints: a round trip, and a foreign state refused
    w = R.random_weights(od, ad, (7,), 2, 3)
    agent.load(*[[(w["%s_w%d" % (n, l)], w["%s_b%d" % (n, l)]) for l in range(2)] for n in ("pi", "q1", "q2")])
    assert torch.equal(agent.params, agent.target) and bool(agent.params.any()) and abs(float(agent.log_alpha[0]) - math.log(0.5)) < 1e-6
    other = SAC(env, hidden=(7,))
    other.load_state_dict(agent.state_dict())
    assert torch.equal(other.params, agent.params) and torch.equal(other.target, agent.target) and other.seed == agent.seed
    assert other.entropy_target() == -0.5 and other.alpha_lr() == 1e-2
    with pytest.raises(ValueError, match="another agent"):
        SAC(env, hidden=(8,)).load_state_dict(agent.state_dict())
    with pytest.raises(ValueError, match="another agent"):
        single.load_state_dict(agent.state_dict())


# ---- sac_ref against finite differences ------------------------------------------------------------
def _fd_case(activation, n_critics, seed):
    od, ad, hidden, m = 5, 3, (6, 4), 40
    rng = np.random.default_rng(seed)
    W, Wt = R.random_weights(od, ad, hidden, n_critics, seed, alpha=0.3), R.random_weights(od, ad, hidden, n_critics, seed + 100)
    batch = {"s": rng.standard_normal((m, od)), "a": rng.uniform(-0.5, 1.5, (m, ad)), "r": rng.standard_normal(m), "s2": rng.standard_normal((m, od)),
             "boot": (rng.uniform(size=m) > 0.3).astype(np.float64), "w": (rng.uniform(size=m) > 0.25).astype(np.float64)}
    for k in ("s", "a", "r", "s2"):
        batch[k][batch["w"] == 0] = np.nan               # a dead row may hold anything
    z8, z9 = rng.standard_normal((m, ad)), rng.standard_normal((m, ad))
    mk = lambda w, dtype=torch.float64: R.Ref(od, ad, hidden, activation, -0.5, 1.5, n_critics, w, Wt, dtype=dtype)
    return W, batch, z8, z9, mk


@pytest.mark.parametrize("activation", ["tanh", "relu"])
@pytest.mark.parametrize("n_critics", [1, 2])
def test_reference_gradients_match_finite_differences(activation, n_critics):
    W, batch, z8, z9, mk = _fd_case(activation, n_critics, 11)
    te = -3.0
    ref = mk(W)
    c, p = ref.critic(batch, z8, 0.9), ref.policy(batch, z9, te)
    assert np.isfinite(c["loss"]) and np.isfinite(p["loss"]) and np.isfinite(p["alpha_loss"]) and batch["w"].sum() < len(batch["w"])
    assert set(c["grads"]) == set(ref.names_of(0)) and set(p["grads"]) == set(ref.names_of(1)) | {"log_alpha"}
    assert not any(k.startswith("pi") for k in c["grads"]) and not any(k.startswith("q") for k in p["grads"])
    if n_critics == 2:                                   # the per-row min takes each critic somewhere
        t, w, live = ref._batch(batch)
        with torch.no_grad():
            a = ref.pi(ref.W, t["s"], torch.as_tensor(z9))[0]
            q1, q2 = ref.q(ref.W, 0, t["s"], a), ref.q(ref.W, 1, t["s"], a)
        assert bool((q2 < q1)[live].any()) and bool((q1 < q2)[live].any())
    rng = np.random.default_rng(5)
    h = 1e-6
    L = len(ref.hidden)
    # the alpha loss as a function of log_alpha with log pi a constant: -log_alpha sum w (log pi + te) / W, linear in log_alpha
    lp_const = p["stats"]["logp_mean"]
    for which, out, f in ((0, c, lambda r: r.critic(batch, z8, 0.9)["loss"]), (1, p, lambda r: r.policy(batch, z9, te)["loss"]),
                          (2, p, lambda r: r.policy(batch, z9, te)["alpha_loss"])):
        names = ref.names_of(which)
        scale = max(float(out["grads"][k].abs().max()) for k in names)
        for name in names:
            g = out["grads"][name].numpy()
            # both halves of the head: a mean row and a log-std row of pi's last matrix and bias
            ats = [tuple(int(rng.integers(n)) for n in g.shape) for _ in range(3)]
            if name in ("pi_w%d" % L, "pi_b%d" % L):
                ats = [(1,) + a[1:] for a in ats[:2]] + [(ref.ad + 1,) + a[1:] for a in ats[:2]]
            for at in ats:
                Wp, Wm = {k: np.array(v) for k, v in W.items()}, {k: np.array(v) for k, v in W.items()}
                Wp[name][at] += h
                Wm[name][at] -= h
                fd = (f(mk(Wp)) - f(mk(Wm))) / (2 * h)
                # central difference: O(h^2 f''') truncation and eps |f| / h rounding, both below 1e-8 of the gradient's scale here
                assert abs(fd - g[at]) <= 1e-7 * max(1.0, scale), (name, at, fd, g[at])
    assert abs(float(p["grads"]["log_alpha"][0]) + (lp_const + te)) < 1e-12           # W = sum w >= 1 here: -(mean log pi + target_entropy)
    # alpha reaches the critic loss through y only, as a constant of it, and the policy loss as a constant: no gradient to log_alpha
    # from either (names_of), yet both move with it
    W2 = dict(W, log_alpha=W["log_alpha"] + 0.5)
    assert mk(W2).critic(batch, z8, 0.9)["loss"] != c["loss"] and mk(W2).policy(batch, z9, te)["loss"] != p["loss"]


def test_reference_losses_leave_the_other_networks_alone():
    W, batch, z8, z9, mk = _fd_case("tanh", 2, 3)
    ref = mk(W)
    base_c, base_p = ref.critic(batch, z8, 0.9), ref.policy(batch, z9, -3.0)
    # y carries no gradient, but it is the CURRENT policy's: moving pi moves y and the critic loss; moving the TARGET critics too
    W2 = {k: (v + 0.1 if k.startswith("pi") else v) for k, v in W.items()}
    assert mk(W2).critic(batch, z8, 0.9)["loss"] != base_c["loss"]
    r2 = R.Ref(5, 3, (6, 4), "tanh", -0.5, 1.5, 2, W, {k: v + (0.1 if k.startswith("q") else 0.0) for k, v in ref.Wt.items()})
    assert r2.critic(batch, z8, 0.9)["loss"] != base_c["loss"] and r2.policy(batch, z9, -3.0)["loss"] == base_p["loss"]
    # the target's pi segments are never read
    r3 = R.Ref(5, 3, (6, 4), "tanh", -0.5, 1.5, 2, W, {k: v + (0.1 if k.startswith("pi") else 0.0) for k, v in ref.Wt.items()})
    assert r3.critic(batch, z8, 0.9)["loss"] == base_c["loss"]
    # float32 runs the same arithmetic
    r32 = mk(W, torch.float32)
    assert abs(r32.critic(batch, z8, 0.9)["loss"] - base_c["loss"]) < 1e-5 * max(1.0, abs(base_c["loss"]))
    assert abs(r32.policy(batch, z9, -3.0)["loss"] - base_p["loss"]) < 1e-5 * max(1.0, abs(base_p["loss"]))
    # Adam's first step moves every element by lr (sign of the gradient), per optimiser; Polyak is the explicit formula
    g = dict(base_c["grads"], **base_p["grads"])
    before = {k: v.clone() for k, v in ref.W.items()}
    ref.adam(0, g, lr=1e-3)
    for k in ref.names_of(0):
        moved, gk = (ref.W[k] - before[k]).numpy(), g[k].numpy()
        assert np.allclose(moved[gk != 0], -1e-3 * np.sign(gk[gk != 0]), rtol=1e-4)
    assert all(torch.equal(ref.W[k], before[k]) for k in ref.names_of(1) + ref.names_of(2)) and ref.steps == [1, 0, 0]
    ref.adam(2, g, lr=1e-2)
    assert abs(float(ref.W["log_alpha"][0] - before["log_alpha"][0]) + 1e-2 * np.sign(float(g["log_alpha"][0]))) < 1e-6 and ref.steps == [1, 0, 1]
    assert all(torch.equal(ref.W[k], before[k]) for k in ref.names_of(1))
    t0 = {k: v.clone() for k, v in ref.Wt.items()}
    ref.polyak(0.25)
    assert all(torch.allclose(ref.Wt[k], 0.75 * t0[k] + 0.25 * ref.W[k], rtol=0, atol=1e-15) for k in ref.names)


# ---- log pi ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounds", [(-1.0, 1.0), (-0.5, 1.5), (0.0, 7.0)])
def test_log_pi_matches_torch_distributions(bounds):
    import torch.distributions as D
    low, high = bounds
    c, h = (high + low) / 2.0, (high - low) / 2.0
    rng = np.random.default_rng(0)
    m, n = 200, 3
    mean, raw = torch.as_tensor(rng.uniform(-1.5, 1.5, (m, n))), torch.as_tensor(rng.uniform(-3.0, 0.0, (m, n)))
    z = torch.as_tensor(rng.uniform(-1.5, 1.5, (m, n)))
    a, lp, u, _ = R.squash(torch.cat([mean, raw], dim=1), z, c, h)
    assert float(u.abs().max()) <= 3.0
    dist = D.TransformedDistribution(D.Normal(mean, torch.exp(raw)), [D.transforms.TanhTransform(cache_size=1), D.transforms.AffineTransform(c, h)])
    want = dist.log_prob(a).sum(dim=1)
    assert float((lp - want).abs().max()) < 1e-10 * max(1.0, float(want.abs().max())), float((lp - want).abs().max())
    assert float((a - (c + h * torch.tanh(mean + torch.exp(raw) * z))).abs().max()) == 0.0
    # the clamp: raw beyond the bounds is the bound
    far = torch.tensor([[0.3, 5.0], [0.3, -30.0]], dtype=torch.float64)
    zz = torch.tensor([[0.5], [0.5]], dtype=torch.float64)
    assert float(R.squash(far, zz, c, h)[2][0, 0]) == 0.3 + float(torch.exp(torch.tensor(2.0, dtype=torch.float64))) * 0.5 and float(R.squash(far, zz, c, h)[2][1, 0]) == 0.3 + float(torch.exp(torch.tensor(-20.0, dtype=torch.float64))) * 0.5


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_log_pi_is_finite_and_correct_where_tanh_saturates(dtype):
    """at |u| = 30 (and beyond) log(1 - tanh(u)^2) evaluated directly is -inf, so the naive log pi is +inf; the header's form is the
    closed form log(1 - t^2) = -2 |u| + 2 ln 2 - 2 log1p(exp(-2 |u|)) evaluated in float64"""
    h, c = 1.0, 0.5
    for umag in (30.0, 45.0, 300.0):
        mean = torch.tensor([[umag], [-umag], [umag - 0.25], [-umag + 0.25]], dtype=dtype)
        raw = torch.full((4, 1), -1.0, dtype=dtype)
        z = torch.tensor([[0.0], [0.0], [0.5], [-0.5]], dtype=dtype)
        a, lp, u, _ = R.squash(torch.cat([mean, raw], dim=1), z, c, h)
        assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(a).all())
        naive = (-0.5 * z * z - raw - 0.5 * math.log(2 * math.pi) - math.log(h) - torch.log(1 - torch.tanh(u) ** 2))[:, 0]
        assert bool(torch.isinf(naive).all())
        u64, z64 = u.double()[:, 0], z.double()[:, 0]
        log1mt2 = -2.0 * u64.abs() + 2.0 * math.log(2.0) - 2.0 * torch.log1p(torch.exp(-2.0 * u64.abs()))
        want = -0.5 * z64 * z64 + 1.0 - 0.5 * math.log(2 * math.pi) - math.log(h) - log1mt2
        rel = 1e-13 if dtype == torch.float64 else 4 * 2.0 ** -24               # a handful of roundings of numbers of magnitude |u|
        assert float((lp.double() - want).abs().max()) <= rel * float(want.abs().max()), (umag, lp, want)
        assert abs(float(want[0]) - (2.0 * umag + 1.0 - 0.5 * math.log(2 * math.pi) - 2.0 * math.log(2.0))) < 1e-9 * umag
    # the gradient there is the header's: d log pi / du = 2 t, finite
    mean = torch.tensor([[30.0], [-30.0]], dtype=torch.float64, requires_grad=True)
    lp = R.squash(torch.cat([mean, torch.zeros(2, 1, dtype=torch.float64)], dim=1), torch.zeros(2, 1, dtype=torch.float64), c, h)[1]
    g = torch.autograd.grad(lp.sum(), mean)[0]
    assert torch.allclose(g[:, 0], torch.tensor([2.0, -2.0], dtype=torch.float64), atol=1e-12)


def test_log_pi_derivatives_are_the_headers():
    """d log pi / du_j = 2 t_j; d / d ls_j = -1 + sd_j z_j 2 t_j; the clamp passes gradient on [-20, 2], both ends included"""
    rng = np.random.default_rng(1)
    mean = torch.as_tensor(rng.standard_normal((6, 2))).requires_grad_(True)
    raw = torch.tensor([[-20.0, 2.0], [-20.5, 2.5], [0.3, -1.0], [-25.0, 1.9], [1.0, -19.0], [3.0, -21.0]], dtype=torch.float64, requires_grad=True)
    z = torch.as_tensor(rng.standard_normal((6, 2)))
    a, lp, u, _ = R.squash(torch.cat([mean, raw], dim=1), z, 0.5, 1.0)
    gm, gr = torch.autograd.grad(lp.sum(), [mean, raw])
    t = torch.tanh(u.detach())
    passes = ((raw.detach() >= -20.0) & (raw.detach() <= 2.0)).double()
    sd = torch.exp(raw.detach().clamp(-20.0, 2.0))
    assert torch.allclose(gm, 2.0 * t, atol=1e-12)
    assert torch.allclose(gr, passes * (-1.0 + sd * z * 2.0 * t), atol=1e-10)
    assert passes.tolist() == [[1, 1], [0, 0], [1, 1], [0, 1], [1, 1], [0, 0]]


# ---- the streams -------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 7, 0xDEADBEEFCAFEF00D])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_stream_restatements(seed, dtype):
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    n, m, off = 5, 64, 2 ** 32 - 3
    ctr = np.arange(m) * 3 + 1
    got = {7: R.act_normals(seed, off, ctr, n, dtype), 8: R.next_normals(seed, m, 11, n, dtype), 9: R.pi_normals(seed, m, 11, n, dtype)}
    assert all(v.shape == (m, n) and np.isfinite(v).all() for v in got.values())
    # one element of each stream spelled out from the words: row 5, components 2 and 3 are pair index 1
    for stream, (c0, c1) in ((7, ((off + 5) & 0xFFFFFFFF, int(ctr[5]))), (8, (5, 11)), (9, (5, 11))):
        w = philox4x32_10(np.array([c0]), np.array([c1]), 1, stream, k0, k1)
        u1, u2 = R3.pair_uniforms(w, dtype)
        radius = math.sqrt(-2.0 * math.log(float(u1[0])))
        assert abs(got[stream][5, 2] - radius * math.cos(2.0 * math.pi * float(u2[0]))) < 1e-12
        assert abs(got[stream][5, 3] - radius * math.sin(2.0 * math.pi * float(u2[0]))) < 1e-12
    # the streams differ from each other and from TD3's (4 exploration, 6 smoothing) at the same counters
    assert np.abs(got[8] - got[9]).min() > 0 and np.abs(got[8] - R3.smooth_normals(seed, m, 11, n, dtype)).min() > 0
    assert np.abs(got[7] - R3.explore_normals(seed, off, ctr, n, dtype)).min() > 0
    # pure functions of (row, counter, seed); an odd n stops at the first half of the last pair
    assert np.array_equal(R.next_normals(seed, m + 9, 11, n, dtype)[:m], got[8]) and np.array_equal(R.pi_normals(seed, m, 11, n - 1, dtype), got[9][:, :n - 1])
    assert (R.next_normals(seed, m, 12, n, dtype) != got[8]).all() and (R.next_normals(seed + 1, m, 11, n, dtype) != got[8]).all()
    # standard normal to what 320 draws show: mean within 5 sigma / sqrt(N), variance within 30 %
    for v in got.values():
        assert abs(v.mean()) < 5.0 / math.sqrt(v.size) and 0.7 < v.var() < 1.3
    # the uniform mode: the single uniform of stream 7 at index j = the action component
    u = R.act_uniforms(seed, off, ctr, n, dtype)
    w = philox4x32_10(np.array([(off + 5) & 0xFFFFFFFF]), np.array([int(ctr[5])]), 2, 7, k0, k1)
    assert u.shape == (m, n) and u.min() >= 0.0 and u.max() < 1.0 and u[5, 2] == float(R3.single_uniform(w, dtype)[0])


# pinned values: the first row of each stream at counter 11 (acting: replica_offset 0, counters 11), float64 forms
PINNED = {
    0: [-0.20262957304286136, -0.35785752410435506, -0.7618490118677683, 0.9370896220207214],
    7: [-0.6969563555009323, 1.8303452803086826, -0.16165315147491469, 0.7842346429824829],
    0xDEADBEEFCAFEF00D: [-0.16893714255862355, 2.2110185289780397, -0.20088816823258715, 0.8730040788650513],
}


@pytest.mark.parametrize("seed", [0, 7, 0xDEADBEEFCAFEF00D])
def test_streams_are_pinned(seed):
    got = [float(R.act_normals(seed, 0, np.array([11]), 2, np.float64)[0, 0]), float(R.next_normals(seed, 1, 11, 2, np.float64)[0, 1]),
           float(R.pi_normals(seed, 1, 11, 2, np.float32)[0, 0]), float(R.act_uniforms(seed, 0, np.array([11]), 1, np.float32)[0, 0])]
    assert np.allclose(got, PINNED[seed], rtol=0, atol=1e-15), (seed, got)
