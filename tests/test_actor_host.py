"""CPU-side checks of the on-device actor (no GPU): the header, the binding and the library agree on the entry points, the main
library's C ABI is untouched, the layout functions, the argument errors of Actor, tests/actor_ref.py against itself, and the DPP
wait-state scan of libbeacon_actor.so."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import actor_ref as R
import isa_hazards as H
import noise_ref as N

NAMES = {"bcn_actor_params_layout", "bcn_actor_params_bytes", "bcn_actor_state_layout", "bcn_actor_state_bytes", "bcn_actor_seq_layout",
         "bcn_actor_seq_bytes", "bcn_actor_act", "bcn_actor_values", "bcn_actor_last_error"}


def _lib():
    from beacon_amd import actor, build
    if build.hipcc() is None and not os.path.exists(actor.LIB):
        pytest.skip("no hipcc and no prebuilt library")
    return actor.load()


def test_header_binding_and_library_agree():
    from beacon_amd import actor
    hdr = open(os.path.join(ROOT, "include", "beacon_actor.h")).read()
    declared = set(re.findall(r"BCN_ACTOR_API\s+[\w\s\*]+?\b(bcn_actor_\w+)\s*\(", hdr))
    assert declared == NAMES == set(actor.SIGNATURES)
    assert int(re.search(r"#define BCN_ACTOR_API_VERSION (\d+)", hdr).group(1)) == actor.API_VERSION == 1
    L = _lib()
    for name in NAMES:
        assert hasattr(L, name)
    nm = subprocess.run(["nm", "-D", "--defined-only", actor.LIB], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if " T " in l}
    assert {e for e in exported if e.startswith("bcn_")} == NAMES, exported ^ NAMES
    # the limits the Python layer checks first are the header's
    for macro, val in (("MAX_OBS", actor.MAX_OBS), ("MAX_HIDDEN", actor.MAX_HIDDEN), ("MAX_LAYERS", actor.MAX_LAYERS), ("MAX_ACT", actor.MAX_ACT),
                       ("MAX_SEGS", actor.MAX_SEGS)):
        assert int(re.search(r"#define BCN_ACTOR_%s (\d+)" % macro, hdr).group(1)) == val


def test_main_library_abi_is_untouched():
    from beacon_amd import _lib, build, vec
    hdr = open(os.path.join(ROOT, "include", "beacon_hip.h")).read()
    assert len(re.findall(r"BCN_API\s+[\w\s\*]+?\b(bcn_\w+)\s*\(", hdr)) == 78
    ops = vec._ALL_OPS + vec._NORM_OPS + vec._ROLLOUT_OPS + vec._RENDER_OPS
    for name in NAMES:
        assert name not in _lib.SIGNATURES and name[4:] not in ops
    assert not any("actor" in n for n in _lib.SIGNATURES) and not any("actor" in n for n in ops)
    # the new units live in a directory of their own: the main library's source list does not see them
    assert not any("actor" in os.path.basename(s) for s in build.sources())
    import beacon_amd
    assert beacon_amd.Actor is __import__("beacon_amd.actor", fromlist=["Actor"]).Actor


def _cfg(**kw):
    from beacon_amd import actor
    d = dict(batch=65, obs_dim=6, dtype=0, hidden=(64, 64), activation="tanh", kind=0, act_dim=2, low=-1.0, high=1.0)
    d.update(kw)
    return actor.make_cfg(**d)


def test_layouts():
    from beacon_amd import actor
    _lib()
    for dtype, esz in ((0, 4), (1, 8)):
        cfg = _cfg(dtype=dtype, hidden=(17, 128, 3), act_dim=5, obs_dim=33)
        segs, nbytes = actor.layout("params", cfg)
        dims = [33, 17, 128, 3]
        want = []
        for net, head in (("pi", 5), ("vf", 1)):
            for l in range(4):
                out = dims[l + 1] if l < 3 else head
                want += [("%s_w%d" % (net, l), out * dims[l]), ("%s_b%d" % (net, l), out)]
        want.append(("log_std", 5))
        assert [(s["name"], s["row_elems"]) for s in segs] == want
        assert all(s["planes"] == 0 and s["elem"] == 0 and s["offset"] % 16 == 0 for s in segs)
        end = 0
        for s in segs:                                # in order, no overlap
            assert s["offset"] >= end
            end = s["offset"] + s["row_elems"] * esz
        assert nbytes >= end and nbytes % 16 == 0
        segs, nbytes = actor.layout("state", cfg)
        assert [(s["name"], s["elem"], s["row_elems"]) for s in segs] == [("counters", 2, 1), ("actions", 0, 5), ("raw", 0, 5), ("logp", 0, 1),
                                                                         ("value", 0, 1), ("dist", 0, 5)]
        end = 0
        for s in segs:
            assert s["offset"] % 16 == 0 and s["offset"] >= end and s["planes"] == 1
            end = s["offset"] + 65 * s["row_elems"] * (4 if s["elem"] else esz)
        assert nbytes >= end
        segs, nbytes = actor.layout("seq", cfg, T=8)
        assert [(s["name"], s["planes"], s["row_elems"]) for s in segs] == [("logp_seq", 8, 1), ("value_seq", 8, 1), ("raw_seq", 8, 5)]
        assert all(s["offset"] % 16 == 0 for s in segs) and nbytes >= segs[2]["offset"] + 8 * 65 * 5 * esz
    cat = actor.layout("state", _cfg(kind=1, act_dim=3))[0]
    assert (cat[1]["name"], cat[1]["elem"], cat[1]["row_elems"]) == ("actions", 1, 1)
    assert actor.layout("params", _cfg(kind=1, act_dim=3))[0][-1]["row_elems"] == 0       # no log_std, the name stays


def test_layout_bytes_are_monotone_in_every_field():
    from beacon_amd import actor
    _lib()
    base = dict(batch=65, obs_dim=6, dtype=0, hidden=(64, 64), act_dim=2)
    b = lambda which, **kw: actor.layout(which, _cfg(**dict(base, **kw)), *((8,) if which == "seq" else ()))[1]
    for which, bigger in (("params", [dict(obs_dim=7), dict(dtype=1), dict(hidden=(64, 64, 64)), dict(hidden=(65, 64)), dict(hidden=(64, 65)), dict(act_dim=3)]),
                          ("state", [dict(batch=69), dict(dtype=1), dict(act_dim=3)]),       # (segments round up to 16 bytes: four more rows always show)
                          ("seq", [dict(batch=69), dict(dtype=1), dict(act_dim=3)])):
        for kw in bigger:
            assert b(which, **kw) > b(which), (which, kw)
    assert actor.layout("seq", _cfg(), 9)[1] > actor.layout("seq", _cfg(), 8)[1]
    assert b("state", batch=66) >= b("state") and b("seq", batch=66) >= b("seq")
    assert b("params", batch=1000) == b("params")       # the parameters do not scale with the batch


def test_layout_refuses_bad_cfg_with_code_and_message():
    from beacon_amd import actor
    L = _lib()
    segs = (actor.ActorSeg * actor.MAX_SEGS)()
    assert L.bcn_actor_params_layout(None, segs, actor.MAX_SEGS) == 0 and b"NULL" in L.bcn_actor_last_error()
    assert L.bcn_actor_params_bytes(None) == 0
    for kw, word in ((dict(obs_dim=0), "obs_dim"), (dict(obs_dim=513), "obs_dim"), (dict(dtype=2), "dtype"), (dict(hidden=()), "n_hidden"),
                     (dict(hidden=(64, 129)), "hidden[1]"), (dict(hidden=(0,)), "hidden[0]"), (dict(activation=2), "activation"), (dict(kind=2), "kind"),
                     (dict(act_dim=17), "act_dim"), (dict(act_dim=0), "act_dim"), (dict(kind=1, act_dim=1), "act_dim"), (dict(low=1.0, high=-1.0), "low")):
        cfg = _cfg(**kw)
        assert L.bcn_actor_params_layout(C.byref(cfg), segs, actor.MAX_SEGS) == 0, kw
        assert word.encode() in L.bcn_actor_last_error(), (kw, L.bcn_actor_last_error())
        assert L.bcn_actor_params_bytes(C.byref(cfg)) == 0 and L.bcn_actor_state_bytes(C.byref(cfg)) == 0
        with pytest.raises(actor.BeaconActorError, match=re.escape(word)):
            actor.layout("params", cfg)
    cfg = _cfg(batch=0)
    assert L.bcn_actor_state_layout(C.byref(cfg), segs, actor.MAX_SEGS) == 0 and b"batch" in L.bcn_actor_last_error()
    cfg = _cfg()
    assert L.bcn_actor_seq_layout(C.byref(cfg), 0, segs, actor.MAX_SEGS) == 0 and b"T = 0" in L.bcn_actor_last_error()
    # the launches check before they touch a device: error codes, not crashes
    assert L.bcn_actor_act(C.byref(cfg), None, None, None, None, 0, 0, 0, None, 0, None, None) == 1 and b"NULL" in L.bcn_actor_last_error()
    assert L.bcn_actor_values(C.byref(_cfg(dtype=3)), None, None, 1, None, None) == 1 and b"dtype" in L.bcn_actor_last_error()
    assert L.bcn_actor_params_layout(C.byref(cfg), None, 0) == 13         # the count without an array


def _bare(cls, batch=4, dtype="f32"):
    """an env of class `cls` without a handle and without a device (the trick of test_render_host.py) plus what Actor reads of it"""
    import torch
    from beacon_amd import vec
    c = getattr(vec, cls)
    env = c._derive(c.__new__(c))._make_spaces()
    env.batch, env.tdtype, env.device = batch, vec._DT[dtype][0], torch.device("cpu")
    env.obs_dim = int(env.observation_space.shape[0])
    return env


def test_actor_argument_errors_need_no_gpu():
    import torch
    from beacon_amd import Actor
    _lib()
    env = _bare("VecBurgers")
    for bad in ((), (64, 64, 64, 64), (0,), (129,), (64.5,), "wide", None):
        with pytest.raises(ValueError, match="hidden"):
            Actor(env, hidden=bad)
    with pytest.raises(ValueError, match="activation"):
        Actor(env, activation="gelu")
    with pytest.raises(ValueError, match="seed"):
        Actor(env, seed=-1)
    with pytest.raises(ValueError, match="replica_offset"):
        Actor(env, replica_offset=-1)
    a = Actor(env, hidden=(5, 7), seed=3)
    assert (a.kind, a.act_dim, a.low, a.high, a.obs_dim, a.seed) == (0, 1, -1.0, 1.0, 5, 3)
    assert tuple(a.actions.shape) == (4, 1) and tuple(a.weights["pi_w1"].shape) == (7, 5) and tuple(a.weights["vf_w2"].shape) == (1, 7)
    lay = lambda dims: [(torch.zeros(o, i), torch.zeros(o)) for i, o in zip(dims[:-1], dims[1:])]
    a.load(lay([5, 5, 7, 1]), lay([5, 5, 7, 1]), log_std=[0.5])
    assert float(a.weights["log_std"][0]) == 0.5
    with pytest.raises(ValueError, match=r"pi\[1\]"):
        a.load(lay([5, 5, 8, 1]), lay([5, 5, 7, 1]))
    with pytest.raises(ValueError, match="vf must be 3"):
        a.load(lay([5, 5, 7, 1]), lay([5, 5, 1]))
    with pytest.raises(ValueError, match="log_std"):
        a.load(lay([5, 5, 7, 1]), lay([5, 5, 7, 1]), log_std=[0.0, 0.0])
    nn = torch.nn
    a.load_modules(nn.Sequential(nn.Linear(5, 5), nn.Tanh(), nn.Linear(5, 7), nn.Tanh(), nn.Linear(7, 1)),
                   nn.Sequential(nn.Linear(5, 5), nn.Tanh(), nn.Linear(5, 7), nn.Tanh(), nn.Linear(7, 1)))
    with pytest.raises(ValueError, match="ReLU"):
        a.load_modules(nn.Sequential(nn.Linear(5, 5), nn.ReLU(), nn.Linear(5, 7), nn.Tanh(), nn.Linear(7, 1)), nn.Sequential())
    with pytest.raises(ValueError, match="obs"):
        a.act(obs=torch.zeros(4, 6))
    with pytest.raises(ValueError, match="obs"):
        a.act(obs=torch.zeros(4, 5, dtype=torch.float64))
    with pytest.raises(ValueError, match="mask"):
        a.act(obs=torch.zeros(4, 5), mask=[1, 0])
    with pytest.raises(ValueError, match="obs_rows"):
        a.values(torch.zeros(3, 4))
    with pytest.raises(ValueError, match="out"):
        a.values(torch.zeros(3, 5), out=torch.zeros(2))
    with pytest.raises(ValueError, match="rollout"):
        a.attach(object())
    with pytest.raises(RuntimeError, match="no CPU fallback"):     # a missing device is an error, never a host evaluation
        a.act(obs=torch.zeros(4, 5))
    d = a.state_dict()
    b = Actor(env, hidden=(5, 7)).load_state_dict(d)
    assert torch.equal(b.params, a.params) and b.seed == 3
    with pytest.raises(ValueError, match="another actor"):
        Actor(env, hidden=(5, 8)).load_state_dict(d)
    lor = Actor(_bare("VecLorenz", 3, "f64"), hidden=(8,), activation="relu")
    assert (lor.kind, lor.act_dim, lor.obs_dim) == (1, 3, 6) and lor.actions.dtype == torch.int32 and tuple(lor.actions.shape) == (3,)
    assert lor.dist.dtype == torch.float64 and tuple(lor.dist.shape) == (3, 3) and lor.weights["log_std"].numel() == 0


def test_reference_stream_is_its_own():
    seed, off = 0x1234567887654321, 5
    b, ctr = np.meshgrid(np.arange(64), np.arange(8), indexing="ij")
    for j in range(3):
        mine = np.stack(R.words(seed, off, b.ravel(), ctr.ravel(), j))
        k0, k1 = N._key(seed)
        for last in (0, 1):                               # the inlet noise's and the warm-up count's counters for the same seed
            other = np.stack(N.philox4x32_10(b.ravel() + off, ctr.ravel(), j, last, k0, k1))
            assert not np.any(np.all(mine == other, axis=0))
    # the counters themselves are distinct tuples: (b, c, j, 2) over the test's range gives as many distinct outputs
    w = np.stack([np.stack(R.words(seed, off, b.ravel(), ctr.ravel(), j)) for j in range(3)], axis=-1).reshape(4, -1)
    assert len({tuple(c) for c in w.T}) == w.shape[1]


def test_reference_uniforms_and_categorical_rule():
    zero = tuple(np.zeros(1, dtype=np.uint64) for _ in range(4))
    ones = tuple(np.full(1, 0xFFFFFFFF, dtype=np.uint64) for _ in range(4))
    for dt in (np.float32, np.float64):
        u1, u2 = R.pair_uniforms(zero, dt)
        assert u1[0] > 0.0 and u2[0] == 0.0 and np.isfinite(np.sqrt(-2.0 * np.log(u1[0])))
        u1, u2 = R.pair_uniforms(ones, dt)
        assert 0.0 < u1[0] <= 1.0 and u2[0] < 1.0
        assert R.single_uniform(zero, dt)[0] == 0.0 and R.single_uniform(ones, dt)[0] < 1.0
    assert R.pair_uniforms(zero, np.float32)[0][0] == 2.0 ** -25 and R.pair_uniforms(ones, np.float32)[0][0] == 1.0 - 2.0 ** -25
    w = R.words(7, 0, np.arange(4096), 0, 0)
    assert R.pair_uniforms(w, np.float32)[0].min() > 0.0 and R.pair_uniforms(w, np.float64)[0].min() > 0.0
    # the last class takes the remainder: u -> 1 and rounding in the cumulative sum never fall off the end
    dist = R.log_softmax(np.array([[0.3, -1.0, 2.0, 0.1], [1.0, 0.0, -1.0, 0.0]]))
    for u in (1.0 - 2.0 ** -53, 1.0):
        a, _ = R.categorical(dist, np.full(2, u))
        assert a.tolist() == [3, 3]
    a, _ = R.categorical(dist, np.zeros(2))
    assert a.tolist() == [0, 0]
    assert R.first_argmax(np.log(np.array([[0.2, 0.4, 0.4]]))).tolist() == [1]
    # the normals are standard: mean 0, variance 1 over 2 x 8192 draws (4 sigma of the estimators)
    z = R.normals(11, 0, np.arange(8192), np.zeros(8192, dtype=np.int64), 2, np.float32)
    assert abs(z.mean()) < 4.0 / np.sqrt(z.size) and abs(z.var() - 1.0) < 4.0 * np.sqrt(2.0 / z.size)
    g = R.gaussian(np.zeros((1, 2)), [0.0, np.log(2.0)], np.array([[1.0, -3.0]]), -1.0, 1.0)
    assert g[1].tolist() == [[1.0, -6.0]] and g[0].tolist() == [[1.0, -1.0]]
    assert abs(g[2][0] - (-0.5 - 4.5 - np.log(2.0) - np.log(2.0 * np.pi))) < 1e-15


def test_actor_units_compile_for_gfx950_without_dpp_hazards():
    from beacon_amd import actor, build
    tool = H.objdump()
    if tool is None or (build.hipcc() is None and not os.path.exists(actor.LIB)):
        pytest.skip("no llvm-objdump / no hipcc and no prebuilt library")
    assert sorted(os.path.basename(s) for s in actor.sources()) == sorted(actor.FILE_FLAGS) == ["actor.hip", "actor_f64.hip"]
    assert "-ffp-contract=off" in actor.FILE_FLAGS["actor_f64.hip"]
    lib = actor.build_actor()
    assert not actor.stale()
    rep = H.scan_file(lib, tool)
    H.summarise(rep)
    assert rep["code_objects"] >= 1 and not rep["findings"], rep["findings"]
    # no inline assembly in the new units (the allow-list test walks them too)
    for f in os.listdir(actor.SRC_DIR):
        assert "asm" not in re.sub(r"//.*", "", open(os.path.join(actor.SRC_DIR, f)).read()), f
