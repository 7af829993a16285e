"""CPU-side checks of the evolution-strategies learner (no GPU): the header, the binding and the library of libbeacon_es.so agree and the
unit is one of the build machinery's; the layouts; every cfg and argument error is refused without a device, the LDS sum and the
group rule; tests/es_ref.py's rank rule on ties, NaN and all-equal fitness, its gradient against the closed form for M = 2, its
bookkeeping; and the learning condition of the issue on the CPU."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from conftest import ROOT

import es_ref as R
from beacon_amd import ES  # noqa: F401  (importing it touches neither a compiler nor the GPU)
from test_actor_host import _bare

NAMES = {"bcn_es_params_layout", "bcn_es_params_bytes", "bcn_es_state_layout", "bcn_es_state_bytes", "bcn_es_work_layout", "bcn_es_work_bytes",
         "bcn_es_group", "bcn_es_lds_bytes", "bcn_es_begin", "bcn_es_act", "bcn_es_observe", "bcn_es_update", "bcn_es_last_error"}
STRUCTS = (("bcn_es_cfg", "EsCfg", 72), ("bcn_es_seg", "EsSeg", 40), ("bcn_es_hyper", "EsHyper", 56))


def _lib():
    from beacon_amd import build, es
    if build.hipcc() is None and not os.path.exists(es.LIB):
        pytest.skip("no hipcc and no prebuilt library")
    return es.load()


def _cfg(**kw):
    from beacon_amd import es
    d = dict(batch=8, members=4, obs_dim=6, kind=0, n_out=3, dtype=0, hidden=(64, 64), activation="tanh", low=-1.0, high=1.0, group=0)
    d.update(kw)
    return es.make_cfg(**d)


def test_header_binding_and_library_agree():
    import beacon_amd
    from beacon_amd import dqn, es, td3
    hdr = open(os.path.join(ROOT, "include", "beacon_es.h")).read()
    declared = set(re.findall(r"BCN_ES_API\s+[\w\s\*]+?\b(bcn_\w+)\s*\(", hdr))
    assert declared == NAMES == set(es.SIGNATURES)
    assert int(re.search(r"#define BCN_ES_API_VERSION (\d+)", hdr).group(1)) == es.API_VERSION == 1
    for macro, value in (("MAX_MEMBERS", es.MAX_MEMBERS), ("MAX_OBS", es.MAX_OBS), ("MAX_ACT", es.MAX_ACT), ("PAIR_CHUNK", es.PAIR_CHUNK),
                         ("TILE_ROWS", es.TILE_ROWS), ("MAX_GROUP", es.MAX_GROUP), ("WANT_GRID", es.WANT_GRID), ("MAX_SEGS", es.MAX_SEGS),
                         ("LDS_LIMIT", es.LDS_LIMIT)):
        assert int(re.search(r"#define BCN_ES_%s (\d+)" % macro, hdr).group(1)) == value, macro
    assert es.MAX_MEMBERS == 16384 and es.LDS_LIMIT == 163840 and es.PAIR_CHUNK == R.PAIR_CHUNK
    stat_enum = re.search(r"enum \{ (BCN_ES_STAT_FIT_MEAN[^}]*)\}", hdr).group(1)
    stat_names = [n.strip().split(" = ")[0][len("BCN_ES_STAT_"):].lower() for n in stat_enum.split(",")][:-1]
    assert tuple(stat_names) == es.STATS == R.STATS and len(stat_names) == 8
    L = _lib()
    for name in NAMES:
        assert hasattr(L, name)
    nm = subprocess.run(["nm", "-D", "--defined-only", es.LIB], capture_output=True, text=True, check=True).stdout
    assert {l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("bcn_")} == NAMES
    # the structs the binding passes are the header's, field for field
    for struct, cls, size in STRUCTS:
        cls = getattr(es, cls)
        body = re.search(r"typedef struct \{([^{}]*)\} %s;" % struct, hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for d in body.split(";"):
            if d.strip():
                parts = [p.strip() for p in d.split(",")]
                fields += [parts[0].split()[-1]] + parts[1:]
        fields = [re.sub(r"\[\d+\]$", "", f.lstrip("*")) for f in fields]
        assert fields == [f[0] for f in cls._fields_], struct
        assert C.sizeof(cls) == size, (struct, C.sizeof(cls))
    # the header states its formulas, orders and launch counts
    for word in ("fma(s sigma, eps_j[e], theta[e])", "(j, gen[0], e >> 1, 11)", "FIRST maximum", "bcn_es_begin, ONE launch", "bcn_es_act, ONE launch",
                 "bcn_es_observe, ONE launch", "bcn_es_update, SEVEN launches", "rank_p / (M - 1) - 0.5", "F_q == F_p and q < p", "a NaN F_p counts as -inf",
                 "-(g[e]) + weight_decay theta[e]", "j ascending", "c ascending", "t = gen[1] + 1", "sigma <= 0 is an argument error"):
        assert word in hdr, word
    # a unit of its own, on the one build machinery; what it shares is among what its .sig hashes
    assert es._UNIT.__class__ is dqn._UNIT.__class__ is td3._UNIT.__class__
    assert [os.path.basename(s) for s in es.sources()] == sorted(es.FILE_FLAGS) == ["es.hip", "es_f64.hip"]
    assert es.FILE_FLAGS["es_f64.hip"] == ["-ffp-contract=off"] and es.FILE_FLAGS["es.hip"] == []
    deps = {os.path.basename(f) for f in es._UNIT.deps()}
    assert {"es.hip", "es_f64.hip", "es_impl.h", "td3_impl.h", "policy_net.h", "beacon_es.h"} <= deps and "dqn_impl.h" not in deps and "sac_impl.h" not in deps
    assert beacon_amd.ES is es.ES and "ES(env" in beacon_amd.__doc__ and "libbeacon_es.so" in beacon_amd.__doc__
    assert "Not covered" in es.ES.__doc__ and all(w in es.ES.__doc__ for w in ("per_jet", "ShardedVecEnv", "CMA-ES", "RAW rewards", "norm_obs"))
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "es._UNIT" in entry and "es.load()" in entry
    # the kernels are plain HIP C++: no inline assembly and no atomics in the unit's own sources
    for f in ("es.hip", "es_f64.hip", "es_impl.h"):
        text = open(os.path.join(ROOT, "beacon_amd", "csrc", "es", f)).read()
        assert "asm" not in re.sub(r"//.*", "", text) and "atomicAdd" not in text and "atomic" not in re.sub(r"//.*", "", text), f


def test_struct_sizes_match_a_compiled_header(tmp_path):
    """sizeof of every struct as a C compiler lays the header out"""
    import shutil
    from beacon_amd import es
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "beacon_es.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(bcn_es_cfg), '
                   'sizeof(bcn_es_seg), sizeof(bcn_es_hyper)); return 0; }\n')
    exe = tmp_path / "s"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(getattr(es, c)) for _, c, _ in STRUCTS] == [s for _, _, s in STRUCTS]


@pytest.mark.parametrize("dtype,esz", [(0, 4), (1, 8)])
@pytest.mark.parametrize("hidden", [(7,), (33, 5), (17, 128, 3)])
@pytest.mark.parametrize("kind,n_out", [(0, 5), (1, 3)])
def test_layouts(dtype, esz, hidden, kind, n_out):
    from beacon_amd import es
    _lib()
    od, M, B = 33, 6, 18
    cfg = _cfg(batch=B, members=M, obs_dim=od, kind=kind, n_out=n_out, dtype=dtype, hidden=hidden)
    segs, nbytes = es.layout("params", cfg)
    lay = R.Layout(od, hidden, n_out, np.float64 if dtype else np.float32)
    assert [(s["name"], s["row_elems"], s["offset"]) for s in segs] == [(k, int(np.prod(lay.shapes[k])), lay.offsets[k] * esz) for k in lay.names]
    assert nbytes == lay.E * esz and int(lay.used.sum()) == sum(s["row_elems"] for s in segs)
    if hidden == (33, 5):
        assert lay.used.sum() < lay.E                        # odd widths leave gaps: they must be handled

    def in_order(segs, nbytes, size_of):
        end = 0
        for s in segs:
            assert s["offset"] % 16 == 0 and end <= s["offset"] < end + 16 and s["planes"] == 0, s
            end = s["offset"] + s["row_elems"] * size_of[s["elem"]]
        assert end <= nbytes < end + 16 and nbytes % 16 == 0
    size_of = {es.REAL: esz, es.I32: 4, es.U32: 4, es.F64: 8, es.U8: 1}
    in_order(segs, nbytes, size_of)
    assert all(s["elem"] == es.REAL for s in segs)
    nel = nbytes // esz
    st, sb = es.layout("state", cfg)
    assert [(s["name"], s["elem"], s["row_elems"]) for s in st] == [
        ("gen", es.I32, 4), ("fit", es.F64, B), ("len", es.I32, B), ("alive", es.U8, B), ("member_fit", es.F64, M), ("util", es.F64, M),
        ("stats", es.F64, 8), ("adam_m", es.REAL, nel), ("adam_v", es.REAL, nel)]
    in_order(st, sb, size_of)
    wk, wb = es.layout("work", cfg)
    assert [(s["name"], s["elem"], s["row_elems"]) for s in wk] == [("grad", es.REAL, nel), ("norm2", es.F64, (nel + 255) // 256), ("partial", es.F64, nel)]
    in_order(wk, wb, size_of)
    assert wk[0]["offset"] == 0
    # the partial sums: one row per chunk of PAIR_CHUNK pairs
    big = _cfg(batch=2 * (es.PAIR_CHUNK + 1), members=2 * (es.PAIR_CHUNK + 1), obs_dim=od, kind=kind, n_out=n_out, dtype=dtype, hidden=hidden)
    assert es.layout("work", big)[0][2]["row_elems"] == 2 * nel


def test_lds_sum_and_group_rule():
    from beacon_amd import es
    L = _lib()
    impl = open(os.path.join(ROOT, "beacon_amd", "csrc", "es", "es_impl.h")).read()
    TR = es.TILE_ROWS
    for dtype, KS in ((0, 64), (1, 32)):
        esz = 8 if dtype else 4
        for M, Rr, hidden, n_out, group in ((4, 1, (64, 64), 10, 0), (4096, 1, (64, 64), 10, 0), (1024, 2, (8,), 2, 0), (16384, 1, (128, 128, 128), 16, 0),
                                            (2, 70, (128, 128, 128), 16, 0), (6, 3, (5, 7), 3, 2), (8, 4, (16,), 4, 8), (1024, 8, (8,), 2, 0)):
            cfg = _cfg(batch=M * Rr, members=M, obs_dim=512, n_out=n_out, hidden=hidden, dtype=dtype, group=group)
            nmax = max(max(hidden), n_out)
            hp = (nmax + 3) & ~3
            lds = lambda G: esz * (2 * TR * hp + TR * (KS + 4) + G * nmax * (KS + 4))
            if group:
                want = group
            else:
                want = max(1, min(es.MAX_GROUP, TR // Rr, M // 512))
                while want > 1 and lds(want) > es.LDS_LIMIT:
                    want -= 1
            G = int(L.bcn_es_group(C.byref(cfg)))
            assert G == want and int(L.bcn_es_lds_bytes(C.byref(cfg))) == lds(G) <= es.LDS_LIMIT, (dtype, M, Rr, hidden, G, want)
    assert int(L.bcn_es_lds_bytes(C.byref(_cfg(obs_dim=512, n_out=16, hidden=(128, 128, 128), dtype=0)))) == 76288
    assert int(L.bcn_es_lds_bytes(C.byref(_cfg(obs_dim=512, n_out=16, hidden=(128, 128, 128), dtype=1)))) == 111616
    assert "76 288" in impl and "111 616" in impl and "163 840" in impl
    # 16384 members of 3 x 128: the rule would take 8 members per workgroup, the LDS sum takes it down
    assert int(L.bcn_es_group(C.byref(_cfg(batch=16384, members=16384, hidden=(128, 128, 128), dtype=0)))) == 3
    assert int(L.bcn_es_group(C.byref(_cfg(batch=16384, members=16384, hidden=(64, 64), dtype=0)))) == 7
    # a forced group whose sum exceeds the limit is refused, by every function that sizes or launches
    one = C.c_void_p(16)
    for dtype in (0, 1):
        cfg = _cfg(batch=8, members=8, hidden=(128,), dtype=dtype, group=8)
        assert L.bcn_es_lds_bytes(C.byref(cfg)) == 0 and "LDS" in L.bcn_es_last_error().decode() and "163840" in L.bcn_es_last_error().decode()
        assert L.bcn_es_state_bytes(C.byref(cfg)) == 0 and L.bcn_es_group(C.byref(cfg)) == 0
        assert L.bcn_es_act(C.byref(cfg), one, 0, one, None, one, None) == 1 and "LDS" in L.bcn_es_last_error().decode()
        assert L.bcn_es_begin(C.byref(cfg), one, one, one, 0.1, 0, None) == 1 and "LDS" in L.bcn_es_last_error().decode()
        with pytest.raises(es.BeaconEsError, match="LDS"):
            es.layout("state", cfg)


def test_cfg_and_argument_errors_are_refused_by_the_library():
    from beacon_amd import es
    L = _lib()
    one = C.c_void_p(16)
    hyper = lambda **kw: es.EsHyper(**dict(dict(sigma=0.1, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=0.0, weight_decay=0.0), **kw))
    for kw, word in ((dict(obs_dim=513), "obs_dim"), (dict(obs_dim=0), "obs_dim"), (dict(n_out=17), "act_dim"), (dict(n_out=0), "act_dim"),
                     (dict(kind=1, n_out=17), "n_actions"), (dict(kind=1, n_out=1), "n_actions"), (dict(kind=2), "kind"), (dict(hidden=(129,)), "hidden"),
                     (dict(hidden=()), "n_hidden"), (dict(activation=2), "activation"), (dict(dtype=2), "dtype"), (dict(low=1.0, high=-1.0), "low"),
                     (dict(low=float("nan")), "low"), (dict(group=9), "group"), (dict(group=-1), "group")):
        cfg = _cfg(**kw)
        assert L.bcn_es_params_bytes(C.byref(cfg)) == 0 and word in L.bcn_es_last_error().decode(), kw
        assert L.bcn_es_lds_bytes(C.byref(cfg)) == 0 and L.bcn_es_group(C.byref(cfg)) == 0 and L.bcn_es_work_bytes(C.byref(cfg)) == 0
        with pytest.raises(es.BeaconEsError, match=re.escape(word)):
            es.layout("params", cfg)
        # the launches refuse it before they touch a device: the pointers are never read
        assert L.bcn_es_act(C.byref(cfg), one, 0, one, None, one, None) == 1 and word in L.bcn_es_last_error().decode()
        assert L.bcn_es_begin(C.byref(cfg), one, one, one, 0.1, 0, None) == 1
        assert L.bcn_es_observe(C.byref(cfg), one, one, one, one, None) == 1
        assert L.bcn_es_update(C.byref(cfg), one, one, one, C.byref(hyper()), 0, None) == 1
    # the population: odd M, M not dividing B, M > 16384, M < 2; a group whose rows exceed a tile
    for kw, word in ((dict(batch=9, members=3), "members"), (dict(batch=10, members=4), "no multiple"), (dict(batch=16386, members=16386), "members"),
                     (dict(batch=4, members=0), "members"), (dict(batch=2, members=4), "no multiple"), (dict(batch=0, members=2), "no multiple"),
                     (dict(batch=40, members=4, group=4), "fit a tile")):
        cfg = _cfg(**kw)
        assert L.bcn_es_state_bytes(C.byref(cfg)) == 0 and word in L.bcn_es_last_error().decode(), (kw, L.bcn_es_last_error().decode())
        assert L.bcn_es_params_bytes(C.byref(cfg)) > 0                 # one row's layout does not depend on the population
        assert L.bcn_es_act(C.byref(cfg), one, 0, one, None, one, None) == 1 and L.bcn_es_begin(C.byref(cfg), one, one, one, 0.1, 0, None) == 1
        assert L.bcn_es_observe(C.byref(cfg), one, one, one, one, None) == 1 and L.bcn_es_update(C.byref(cfg), one, one, one, C.byref(hyper()), 0, None) == 1
    assert L.bcn_es_state_bytes(C.byref(_cfg(batch=16384, members=16384, obs_dim=512, n_out=16))) > 0
    assert L.bcn_es_state_bytes(C.byref(_cfg(kind=1, n_out=16))) > 0 and L.bcn_es_state_bytes(C.byref(_cfg(kind=1, n_out=2, low=1.0, high=-1.0))) > 0
    assert L.bcn_es_params_bytes(None) == 0 and "cfg is NULL" in L.bcn_es_last_error().decode()
    cfg = _cfg()
    odd = C.c_void_p(20)
    # begin
    for args, word in (((None, one, one, 0.1, 0), "theta_dev"), ((one, None, one, 0.1, 0), "pop_dev"), ((one, one, None, 0.1, 0), "state_dev"),
                       ((one, one, one, -0.1, 0), "sigma"), ((one, one, one, float("nan"), 0), "sigma"), ((one, one, one, float("inf"), 0), "sigma"),
                       ((odd, one, one, 0.1, 0), "16-byte")):
        assert L.bcn_es_begin(C.byref(cfg), *(args + (None,))) == 1 and word in L.bcn_es_last_error().decode(), word
    # act
    for args, word in (((None, 0, one, None, one), "weights_dev"), ((one, 2, one, None, one), "shared"), ((one, 0, None, None, one), "obs_dev"),
                       ((one, 0, one, None, None), "actions_dev"), ((odd, 1, one, None, one), "16-byte")):
        assert L.bcn_es_act(C.byref(cfg), *(args + (None,))) == 1 and word in L.bcn_es_last_error().decode(), word
    # observe
    for args, word in (((None, one, one, one), "state_dev"), ((one, None, one, one), "rwd_dev"), ((one, one, None, one), "done_dev"), ((one, one, one, None), "trunc_dev")):
        assert L.bcn_es_observe(C.byref(cfg), *(args + (None,))) == 1 and word in L.bcn_es_last_error().decode(), word
    # update: sigma <= 0 is an error here (begin takes 0)
    for kw, word in ((dict(sigma=0.0), "sigma"), (dict(sigma=-1.0), "sigma"), (dict(sigma=float("nan")), "sigma"), (dict(sigma=1e-60), "sigma"),
                     (dict(lr=-1.0), "lr"), (dict(beta1=1.0), "beta1"), (dict(beta2=-0.1), "beta2"), (dict(eps=-1.0), "eps"), (dict(eps=0.0), "eps"), (dict(eps=1e-60), "eps"),
                     (dict(max_grad_norm=float("inf")), "max_grad_norm"), (dict(weight_decay=-1.0), "weight_decay")):
        assert L.bcn_es_update(C.byref(cfg), one, one, one, C.byref(hyper(**kw)), 0, None) == 1 and word in L.bcn_es_last_error().decode(), kw
    for args, word in (((None, one, one), "theta_dev"), ((one, None, one), "state_dev"), ((one, one, None), "work_dev")):
        assert L.bcn_es_update(C.byref(cfg), *(args + (C.byref(hyper()), 0, None))) == 1 and word in L.bcn_es_last_error().decode(), word
    assert L.bcn_es_update(C.byref(cfg), one, one, one, None, 0, None) == 1 and "hyper is NULL" in L.bcn_es_last_error().decode()


def test_argument_errors_need_no_gpu():
    from beacon_amd import ES, es
    _lib()
    env = _bare("VecLorenz")
    assert env.action_is_int and int(env.action_space.n) == 3
    for bad in ((), (64, 64, 64, 64), (0,), (129,), (64.5,), "wide", None):
        with pytest.raises(ValueError, match="hidden"):
            ES(env, hidden=bad)
    with pytest.raises(ValueError, match="activation"):
        ES(env, activation="gelu")
    for kw, word in ((dict(lr=-1.0), "lr"), (dict(sigma=-0.1), "sigma"), (dict(sigma=float("nan")), "sigma"), (dict(weight_decay=-1.0), "weight_decay"),
                     (dict(betas=(0.9,)), "betas"), (dict(betas=(0.9, 1.0)), "betas"), (dict(seed=-1), "seed"), (dict(max_grad_norm="big"), "max_grad_norm"),
                     (dict(eps_adam=-1.0), "eps_adam"), (dict(eps_adam=0.0), "eps_adam"), (dict(group=9), "group"), (dict(group=1.5), "group")):
        with pytest.raises(ValueError, match=word):
            ES(env, **kw)
    with pytest.raises(ValueError, match="per_jet"):
        ES(env, per_jet=True)
    # members: even, dividing the batch, at most 16384
    for members in (3, 1, 0, 6, 2.0, True):
        with pytest.raises(ValueError, match="members"):
            ES(env, members=members)
    with pytest.raises(ValueError, match="members"):
        ES(_bare("VecLorenz", batch=5))                                 # the default, env.batch, is odd
    mk = lambda batch=4, od=5, **space: types.SimpleNamespace(action_space=types.SimpleNamespace(**space), action_is_int="n" in space, batch=batch,
                                                              tdtype=torch.float32, device="cpu", obs_dim=od)
    with pytest.raises(ValueError, match="16384"):
        ES(mk(batch=16386, n=3))
    for n in (1, 17, 0):
        with pytest.raises(ValueError, match="2 .. 16"):
            ES(mk(n=n))
    with pytest.raises(ValueError, match="1 .. 16"):
        ES(mk(low=-np.ones(17), high=np.ones(17)))
    with pytest.raises(ValueError, match="one finite scalar bound pair"):
        ES(mk(low=np.array([-1.0, -2.0]), high=np.ones(2)))             # more than one bound pair
    with pytest.raises(ValueError, match="one finite scalar bound pair"):
        ES(mk(low=-np.ones(2), high=np.array([1.0, np.inf])))
    with pytest.raises(ValueError, match="at most 512"):
        ES(mk(od=513, n=4))
    with pytest.raises(ValueError, match="neither a Box nor a Discrete"):
        ES(mk())
    with pytest.raises(ValueError, match="ShardedVecEnv"):
        ES(types.SimpleNamespace(action_space=types.SimpleNamespace(n=3), action_is_int=True, batch=4, tdtype=torch.float32, device="cpu", obs_dim=5, global_batch=8))
    with pytest.raises(es.BeaconEsError, match="fit a tile"):
        ES(mk(batch=64, n=3), members=2, group=2)
    # Box and Discrete envs alike
    box = ES(_bare("VecBurgers"), hidden=(7,))
    assert box.kind == es.BOX and box.actions.dtype == torch.float32 and tuple(box.actions.shape) == (4, box.n_out) and box.members == 4 and box.replicas == 1
    agent = ES(env, members=2, hidden=(7,), sigma=0.1)
    assert agent.kind == es.DISCRETE and agent.actions.dtype == torch.int32 and tuple(agent.actions.shape) == (4,) and agent.replicas == 2
    assert agent.max_grad_norm == 0.0 and agent.sigma == 0.1 and agent.lr == 0.01 and agent.weight_decay == 0.0 and agent.group == 1 and agent.lds_bytes > 0
    assert not any(bool(v.any()) for v in agent.weights.values()) and tuple(agent.pop.shape) == (2, agent.n_elems)
    assert agent.weights["pi_w1"].shape == (3, 7) and agent.gen.numel() == 4 and agent.stats.numel() == 8 and agent.fit.dtype == torch.float64
    assert agent.fit.numel() == agent.len.numel() == agent.alive.numel() == 4 and agent.member_fit.numel() == agent.util.numel() == 2
    assert set(agent.grads) == set(agent.weights) and set(agent.member(1)) == set(agent.weights) and agent.member(1)["pi_w0"].shape == (7, agent.obs_dim)
    agent.member(1)["pi_b0"].fill_(2.0)
    lay = R.Layout(agent.obs_dim, (7,), 3, np.float32, np.float32)
    assert agent.n_elems == lay.E and float(agent.pop[1, lay.offsets["pi_b0"]]) == 2.0 and float(agent.pop[0].abs().sum()) == 0.0
    assert float(agent.pop[1].sum()) == 14.0                              # the view is exactly the segment
    with pytest.raises(ValueError, match="member"):
        agent.member(2)
    with pytest.raises(ValueError, match="unknown"):
        agent.set_hyper(gamma=0.9)
    with pytest.raises(ValueError, match="obs must be"):
        agent.act(obs=torch.zeros(3, agent.obs_dim))
    with pytest.raises(ValueError, match="mask must hold"):
        agent.act(obs=torch.zeros(agent.batch, agent.obs_dim), mask=[1, 0])
    with pytest.raises(RuntimeError, match="ROCm device"):
        agent.act(obs=torch.zeros(agent.batch, agent.obs_dim))
    with pytest.raises(RuntimeError, match="ROCm device"):
        agent.begin()
    z8 = torch.zeros(4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="rwd must be"):
        agent.observe(torch.zeros(4, dtype=torch.float64), z8, z8)
    with pytest.raises(ValueError, match="trunc must be"):
        agent.observe(torch.zeros(4), z8, torch.zeros(4))
    with pytest.raises(RuntimeError, match="ROCm device"):
        agent.observe(torch.zeros(4), z8, torch.zeros(4, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="ROCm device"):
        agent.update()
    agent.set_hyper(sigma=0.0)
    with pytest.raises(ValueError, match="sigma"):
        agent.update()
    agent.set_hyper(sigma=0.1)
    od = agent.obs_dim
    pi = [(np.zeros((7, od)), np.zeros(7)), (np.zeros((3, 7)), np.zeros(3))]
    with pytest.raises(ValueError, match=r"pi\[1\] must be W \[3, 7\]"):
        agent.load([pi[0], (np.zeros((4, 7)), np.zeros(4))])
    with pytest.raises(ValueError, match="2 .W, b. pairs"):
        agent.load(pi[:1])
    import torch.nn as nn
    with pytest.raises(ValueError, match="expected Linear and Tanh"):
        agent.load_modules(nn.Sequential(nn.Linear(od, 7), nn.ReLU(), nn.Linear(7, 3)))
    torch.manual_seed(0)
    net = nn.Sequential(nn.Linear(od, 7), nn.Tanh(), nn.Linear(7, 3))
    agent.load_modules(net)
    assert torch.equal(agent.weights["pi_w1"], net[2].weight.detach()) and bool(agent.theta.any())
    # theta is the reference's packing of the same weights
    packed = lay.pack({"pi_w0": net[0].weight.detach().numpy(), "pi_b0": net[0].bias.detach().numpy(), "pi_w1": net[2].weight.detach().numpy(),
                       "pi_b1": net[2].bias.detach().numpy()})
    assert np.array_equal(agent.theta.view(torch.float32).numpy(), packed)
    # checkpoints: a round trip, and a foreign state refused
    other = ES(env, members=2, hidden=(7,))
    agent.gen[0] = 5
    other.load_state_dict(agent.state_dict())
    assert torch.equal(other.theta, agent.theta) and torch.equal(other.pop, agent.pop) and int(other.gen[0]) == 5 and other.sigma == 0.1 and other.seed == agent.seed
    with pytest.raises(ValueError, match="another agent"):
        ES(env, members=2, hidden=(8,)).load_state_dict(agent.state_dict())
    with pytest.raises(ValueError, match="another agent"):
        ES(env, members=4, hidden=(7,)).load_state_dict(agent.state_dict())


# ---- the rank rule -----------------------------------------------------------------------------------------------------
def test_rank_rule_on_ties_nan_and_equal_fitness():
    nan, inf = np.nan, np.inf
    F, u, st = R.ranks(np.array([3.0, 1.0, 3.0, nan, -2.0, 1.0]), 6)
    # ascending: nan (-inf) 0, -2 -> 1, the two 1s -> 2, 3 by index, the two 3s -> 4, 5 by index
    assert (u * 5 + 2.5).tolist() == [4, 2, 5, 0, 1, 3] and F[3] == -inf and abs(u.sum()) < 1e-15
    assert st["nan_members"] == 1 and st["fit_max"] == 3.0 and st["best_member"] == 0 and st["fit_min"] == -2.0 and abs(st["fit_mean"] - 6.0 / 5) < 1e-15
    # all equal: the ranks are the indices, the utilities still sum to 0
    F, u, st = R.ranks(np.full(8, 0.25), 8)
    assert np.array_equal(u, np.arange(8) / 7 - 0.5) and abs(u.sum()) < 1e-15 and st["fit_std"] == 0.0 and st["best_member"] == 0
    # all NaN: every member counts as -inf, ranks by index, statistics 0
    F, u, st = R.ranks(np.full(4, nan), 4)
    assert np.array_equal(u, np.arange(4) / 3 - 0.5) and st["nan_members"] == 4 and st["fit_mean"] == 0.0 and st["fit_max"] == 0.0
    # replicas: the member's mean for r ascending; one NaN replica makes the member NaN
    F, u, st = R.ranks(np.array([1.0, 2.0, 4.0, nan, -1.0, -1.0, 0.5, 0.25]), 4)
    assert F.tolist() == [1.5, -inf, -1.0, 0.375] and (u * 3 + 1.5).tolist() == [3, 0, 1, 2]
    rng = np.random.default_rng(0)
    for M in (2, 10, 130):
        f = rng.standard_normal(M)
        f[rng.integers(M)] = f[0]                                          # maybe a tie
        F, u, st = R.ranks(f, M)
        assert sorted((u + 0.5) * (M - 1)) == pytest.approx(list(range(M)), abs=1e-9) and abs(u.sum()) < 1e-12
        assert np.array_equal(np.argsort(np.argsort(f, kind="stable"), kind="stable"), np.rint((u + 0.5) * (M - 1)).astype(int))


def test_gradient_closed_form_for_two_members():
    """M = 2: u = (+-0.5), so g = (u_0 - u_1) eps_0 / (2 sigma) = +-eps_0 / (2 sigma), towards the better member"""
    for dtype in (np.float64, np.float32):
        lay = R.Layout(5, (3, 2), 2, dtype, dtype)
        assert lay.used.sum() < lay.E
        theta = lay.pack(R.random_weights(5, (3, 2), 2, 1))
        z = R.eps(9, 4, 2, lay.E, dtype)
        assert z.shape == (1, lay.E) and abs(z.mean()) < 0.5 and 0.5 < z.std() < 1.5
        for fit, sign in (([1.0, 0.0], 1.0), ([0.0, 1.0], -1.0), ([0.0, 0.0], -1.0), ([np.nan, -5.0], -1.0)):
            _, u, _ = R.ranks(np.array(fit), 2)
            assert u.tolist() == [0.5 * sign, -0.5 * sign]
            g = R.gradient(u, theta, 0.1, 0.0, 9, 4, lay)
            want = np.where(lay.used, -(sign * z[0].astype(dtype).astype(np.float64) / (2 * float(dtype(0.1)))), 0.0)
            assert np.allclose(g, want, rtol=1e-6 if dtype == np.float32 else 1e-14, atol=0) and not g[~lay.used].any()
        # weight decay adds wd theta; the noise of another generation or seed is another gradient
        gw = R.gradient(u, theta, 0.1, 0.5, 9, 4, lay)
        assert np.allclose(gw - g, 0.5 * theta, atol=1e-6 if dtype == np.float32 else 1e-14)
        assert not np.allclose(R.gradient(u, theta, 0.1, 0.0, 9, 5, lay), g) and not np.allclose(R.gradient(u, theta, 0.1, 0.0, 10, 4, lay), g)
        # the perturbation: antithetic around theta, theta on the gaps, theta itself at sigma = 0
        pop = R.perturb(theta, 0.1, 9, 4, 2, lay)
        assert np.allclose(pop[0] + pop[1], 2 * theta, atol=1e-6 if dtype == np.float32 else 1e-15) and np.array_equal(pop[:, ~lay.used], np.tile(theta[~lay.used], (2, 1)))
        assert np.allclose((pop[0] - theta)[lay.used], 0.1 * z[0][lay.used], atol=1e-6 if dtype == np.float32 else 1e-15)
        assert np.array_equal(R.perturb(theta, 0.0, 9, 4, 2, lay), np.tile(theta, (2, 1)))


def test_observe_restatement():
    fit, ln, alive = np.zeros(4), np.zeros(4, np.int32), np.ones(4, np.uint8)
    R.observe(fit, ln, alive, [1.0, 2.0, np.nan, 4.0], [0, 1, 0, 0], [0, 0, 0, 1])
    assert fit[[0, 1, 3]].tolist() == [1.0, 2.0, 4.0] and np.isnan(fit[2]) and ln.tolist() == [1, 1, 1, 1] and alive.tolist() == [1, 0, 1, 0]
    R.observe(fit, ln, alive, [10.0, 20.0, 30.0, 40.0], [1, 1, 1, 1], [0, 0, 0, 0])
    assert fit[[0, 1, 3]].tolist() == [11.0, 2.0, 4.0] and np.isnan(fit[2]) and ln.tolist() == [2, 1, 2, 1] and not alive.any()
    R.observe(fit, ln, alive, [1.0] * 4, [0] * 4, [0] * 4)
    assert fit[0] == 11.0 and ln.tolist() == [2, 1, 2, 1]


def test_reference_acts_per_member():
    """replica b runs row b // R; the shared form is every row under theta; the first maximum decides a discrete action"""
    lay = R.Layout(4, (5,), 3)
    rng = np.random.default_rng(3)
    pop = np.stack([lay.pack(R.random_weights(4, (5,), 3, s)) for s in range(4)])
    obs = rng.standard_normal((8, 4))
    a = R.act(R.member_rows(pop, 2), obs, lay, "tanh", 0, -0.5, 1.5)
    for b in range(8):
        W = lay.unpack(pop[b // 2])
        h = np.tanh(W["pi_w0"] @ obs[b] + W["pi_b0"])
        assert np.allclose(a[b], 0.5 + 1.0 * np.tanh(W["pi_w1"] @ h + W["pi_b1"]), atol=1e-15)
    assert a.min() >= -0.5 and a.max() <= 1.5
    d = R.act(R.member_rows(pop, 2), obs, lay, "relu", 1)
    h, min_pre = R.heads(R.member_rows(pop, 2), obs, lay, "relu")
    assert np.array_equal(d, h.argmax(axis=1)) and 0 < min_pre < np.inf
    assert R.first_argmax(np.array([[1.0, 2.0, 2.0], [np.nan, np.nan, np.nan]])).tolist() == [1, 0]


# ---- the learning condition -------------------------------------------------------------------------------------------------
def test_reference_learns_on_the_cpu():
    """obs_dim 6, hidden (8,), act_dim 2, bounds (-0.5, 1.5), sigma 0.1, lr 0.05, M = 64, R = 1, 20 generations on fixed uniform observation
    rows with the fitness -|a - a*|^2: the mean fitness of theta rises from -0.70 to -0.063"""
    ref, obs, target = R.learning_ref()
    L = R.LEARN
    assert (ref.lay.obs_dim, ref.lay.hidden, ref.lay.n_out, ref.low, ref.high, ref.sigma, ref.lr, ref.M, len(obs)) == (6, (8,), 2, -0.5, 1.5, 0.1, 0.05, 64, 64)
    assert obs.min() >= -1.0 and obs.max() <= 1.0 and L["members"] == 64
    of_theta = lambda: float(R.learning_fitness(ref.act(obs, shared=True), target).mean())
    first = of_theta()
    for _ in range(20):
        ref.begin()
        ref.update(R.learning_fitness(ref.act(obs), target))
    last = of_theta()
    print("fitness of theta: %.4f -> %.4f" % (first, last))
    assert ref.gen == ref.steps == 20 and first < -0.3
    assert last > -0.1
