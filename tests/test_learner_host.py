"""CPU-side checks of the on-device learner (no GPU): the header, the binding and the library agree on the entry points, the main
and the actor ABI are untouched, the gradient layout is the actor's parameter layout, the optimiser and work layouts, every refusal
with its code and a message naming the field, Learner's argument errors on a bare env, tests/learner_ref.py against a central finite
difference, and the DPP wait-state scan of libbeacon_learner.so."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import isa_hazards as H
import learner_ref as R
from test_actor_host import NAMES as ACTOR_NAMES, _bare, _cfg

NAMES = {"bcn_learner_grad_layout", "bcn_learner_grad_bytes", "bcn_learner_opt_layout", "bcn_learner_opt_bytes", "bcn_learner_work_layout",
         "bcn_learner_work_bytes", "bcn_learner_grid", "bcn_learner_grad", "bcn_learner_step", "bcn_learner_last_error"}


def _lib():
    from beacon_amd import build, learner
    if build.hipcc() is None and not os.path.exists(learner.LIB):
        pytest.skip("no hipcc and no prebuilt library")
    return learner.load()


def test_header_binding_and_library_agree():
    from beacon_amd import learner
    hdr = open(os.path.join(ROOT, "include", "beacon_learner.h")).read()
    declared = set(re.findall(r"BCN_LEARNER_API\s+[\w\s\*]+?\b(bcn_learner_\w+)\s*\(", hdr))
    assert declared == NAMES == set(learner.SIGNATURES)
    assert int(re.search(r"#define BCN_LEARNER_API_VERSION (\d+)", hdr).group(1)) == learner.API_VERSION == 1
    assert int(re.search(r"#define BCN_LEARNER_MAX_GRID (\d+)", hdr).group(1)) == learner.MAX_GRID
    assert len(learner.STATS) == 8
    L = _lib()
    for name in NAMES:
        assert hasattr(L, name)
    nm = subprocess.run(["nm", "-D", "--defined-only", learner.LIB], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if " T " in l}
    assert {e for e in exported if e.startswith("bcn_")} == NAMES, exported ^ NAMES
    # the structs the binding passes are the header's, field for field
    for struct, cls in (("bcn_learner_batch", learner.LearnerBatch), ("bcn_learner_loss", learner.LearnerLoss), ("bcn_learner_adam", learner.LearnerAdam)):
        body = re.search(r"typedef struct \{([^{}]*)\} %s;" % struct, hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [n.strip().lstrip("*") for decl in body.split(";") if decl.strip() for n in decl.split(",")]
        fields = [f.split()[-1].lstrip("*") for f in fields]
        assert [f[:-4] if f.endswith("_dev") else f for f in fields] == [f[0] for f in cls._fields_], struct


def test_main_and_actor_abi_are_untouched():
    from beacon_amd import _lib, actor, build, learner, vec
    hdr = open(os.path.join(ROOT, "include", "beacon_hip.h")).read()
    assert len(re.findall(r"BCN_API\s+[\w\s\*]+?\b(bcn_\w+)\s*\(", hdr)) == 78
    ops = vec._ALL_OPS + vec._NORM_OPS + vec._ROLLOUT_OPS + vec._RENDER_OPS
    for name in NAMES:
        assert name not in _lib.SIGNATURES and name not in actor.SIGNATURES and name[4:] not in ops
    assert not any("learner" in n for n in _lib.SIGNATURES) and not any("learner" in n for n in ops)
    assert set(actor.SIGNATURES) == ACTOR_NAMES and actor.API_VERSION == 1
    assert not any("learner" in os.path.basename(s) for s in build.sources() + actor.sources())
    # neither header is a dependency of the main library: its signature does not move with them
    deps = {os.path.basename(f) for f in build._deps()}
    assert "beacon_learner.h" not in deps and "beacon_actor.h" not in deps and "beacon_hip.h" in deps
    assert not any("learner" in d for d in deps)
    # the learner's units include the actor's kernel header and the network's (policy_net.h): both are among what the .sig hashes
    ldeps = {os.path.basename(f) for f in learner._UNIT.deps()}
    assert {"learner.hip", "learner_f64.hip", "learner_impl.h", "actor_impl.h", "policy_net.h", "beacon_actor.h", "beacon_learner.h", "env1d.h"} <= ldeps
    assert actor._UNIT.__class__ is learner._UNIT.__class__                       # one build machinery
    import beacon_amd
    assert beacon_amd.Learner is learner.Learner and "Learner" in beacon_amd.__doc__


def test_the_shared_network_header_moves_both_signatures(monkeypatch):
    """csrc/actor/policy_net.h is compiled into both libraries: a change of its content makes both stale.  Nothing on disk is touched:
    the bytes the signature reads for that one file are changed."""
    import builtins
    import io
    from beacon_amd import actor, learner
    hdr = os.path.join(actor.SRC_DIR, "policy_net.h")
    assert hdr in actor._UNIT.deps() and hdr in learner._UNIT.deps()
    before = actor.signature(), learner.signature()
    real_open = builtins.open

    def edited(f, mode="r", *a, **kw):
        if mode == "rb" and os.path.abspath(f) == hdr:
            with real_open(f, "rb") as fh:
                return io.BytesIO(fh.read() + b"\n// edited\n")
        return real_open(f, mode, *a, **kw)
    monkeypatch.setattr(builtins, "open", edited)
    after = actor.signature(), learner.signature()
    assert after[0] != before[0] and after[1] != before[1]
    assert actor._UNIT.stale() and learner._UNIT.stale()          # whatever .sig is on disk holds another hash, or there is none
    monkeypatch.undo()
    assert (actor.signature(), learner.signature()) == before


CFGS = [dict(), dict(dtype=1), dict(dtype=0, hidden=(17, 128, 3), act_dim=5, obs_dim=33), dict(dtype=1, hidden=(17, 128, 3), act_dim=5, obs_dim=33),
        dict(kind=1, act_dim=3), dict(hidden=(1,), obs_dim=1, act_dim=1), dict(dtype=1, hidden=(128, 128, 128), obs_dim=512, act_dim=16)]


def test_gradient_layout_is_the_parameter_layout():
    from beacon_amd import actor, learner
    _lib()
    for kw in CFGS:
        cfg = _cfg(**kw)
        assert learner.layout("grad", cfg) == actor.layout("params", cfg), kw


def test_optimiser_and_work_layouts():
    from beacon_amd import actor, learner
    L = _lib()
    for kw in CFGS:
        cfg = _cfg(**kw)
        esz = 8 if kw.get("dtype") else 4
        pbytes = actor.layout("params", cfg)[1]
        ne = pbytes // esz
        segs, nbytes = learner.layout("opt", cfg)
        assert [(s["name"], s["elem"], s["planes"], s["row_elems"]) for s in segs] == [("m", 0, 0, ne), ("v", 0, 0, ne), ("step", 1, 0, 4)]
        assert segs[0]["offset"] == 0 and segs[1]["offset"] >= pbytes and segs[2]["offset"] >= segs[1]["offset"] + pbytes
        assert all(s["offset"] % 16 == 0 for s in segs) and nbytes >= segs[2]["offset"] + 16
        grid = L.bcn_learner_grid(C.byref(cfg))
        assert grid == min(learner.MAX_GRID, max(8, (64 << 20) // pbytes))
        segs, nbytes = learner.layout("work", cfg)
        assert [(s["name"], s["elem"]) for s in segs] == [("stats", learner.F64), ("wg_stats", learner.F64), ("norm2", learner.F64), ("slabs", 0)]
        assert segs[0]["row_elems"] == 8 and segs[1]["row_elems"] == 8 * grid and segs[2]["row_elems"] == -(-ne // 64) and segs[3]["row_elems"] == grid * ne
        end = 0
        for s in segs:
            assert s["offset"] % 16 == 0 and s["offset"] >= end
            end = s["offset"] + s["row_elems"] * (esz if s["elem"] == 0 else 8)
        assert nbytes >= end
    assert L.bcn_learner_grid(C.byref(_cfg())) == 256                                        # a policy-sized network takes the whole grid
    assert L.bcn_learner_grid(C.byref(_cfg(dtype=1, hidden=(128, 128, 128), obs_dim=512, act_dim=16))) < 256      # the widest does not


def _args(learner, **kw):
    """a complete, valid argument set of bcn_learner_grad with non-NULL dummy pointers (never dereferenced: the checks come first)"""
    p = C.c_void_p(64)
    b = dict(obs=p, act=p, logp_old=p, adv=p, ret=p, weight=None, idx=None, cursor=None, n_rows=8, m=8, weight_kind=0, rows_per_step=0)
    b.update(kw)
    return learner.LearnerBatch(**b)


def test_every_refusal_has_its_code_and_names_the_field():
    from beacon_amd import actor, learner
    L = _lib()
    A = actor.load()
    err = lambda: L.bcn_learner_last_error().decode()
    segs = (actor.ActorSeg * actor.MAX_SEGS)()
    p = C.c_void_p(64)
    loss = learner.LearnerLoss(clip=0.2, vf_coef=0.5, ent_coef=0.0)
    adam = learner.LearnerAdam(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=0.5)
    good = _cfg()
    # a cfg the actor refuses, the learner refuses, with the same text
    assert L.bcn_learner_grad_layout(None, segs, actor.MAX_SEGS) == 0 and "NULL" in err()
    for kw, word in ((dict(obs_dim=0), "obs_dim"), (dict(obs_dim=513), "obs_dim"), (dict(dtype=2), "dtype"), (dict(hidden=()), "n_hidden"),
                     (dict(hidden=(64, 129)), "hidden[1]"), (dict(hidden=(0,)), "hidden[0]"), (dict(activation=2), "activation"), (dict(kind=2), "kind"),
                     (dict(act_dim=17), "act_dim"), (dict(act_dim=0), "act_dim"), (dict(kind=1, act_dim=1), "act_dim"), (dict(low=1.0, high=-1.0), "low")):
        cfg = _cfg(**kw)
        assert A.bcn_actor_params_layout(C.byref(cfg), segs, actor.MAX_SEGS) == 0
        for fn in ("grad", "opt", "work"):
            assert getattr(L, "bcn_learner_%s_layout" % fn)(C.byref(cfg), segs, actor.MAX_SEGS) == 0, (fn, kw)
            assert getattr(L, "bcn_learner_%s_bytes" % fn)(C.byref(cfg)) == 0, (fn, kw)
        assert L.bcn_learner_grid(C.byref(cfg)) == 0
        assert word in err() and err() == A.bcn_actor_last_error().decode(), (kw, err())
        assert L.bcn_learner_grad(C.byref(cfg), p, C.byref(_args(learner)), C.byref(loss), p, p, None) == 1 and word in err()
        assert L.bcn_learner_step(C.byref(cfg), p, p, p, p, C.byref(adam), None) == 1 and word in err()
        with pytest.raises(learner.BeaconLearnerError, match=re.escape(word)):
            learner.layout("grad", cfg)
    # NULL pointers
    g = lambda cfg=good, params=p, batch=None, lo=loss, grad=p, work=p: L.bcn_learner_grad(
        C.byref(cfg), params, None if batch is False else C.byref(batch or _args(learner)), None if lo is None else C.byref(lo), grad, work, None)
    assert L.bcn_learner_grad(None, p, C.byref(_args(learner)), C.byref(loss), p, p, None) == 1 and "cfg is NULL" in err()
    for kw, word in ((dict(params=None), "params_dev"), (dict(batch=False), "batch"), (dict(lo=None), "loss"), (dict(grad=None), "grad_dev"),
                     (dict(work=None), "work_dev")):
        assert g(**kw) == 1 and "NULL" in err() and word in err(), (kw, err())
    for field in ("obs", "act", "logp_old", "adv", "ret"):
        assert g(batch=_args(learner, **{field: None})) == 1 and "NULL" in err() and field + "_dev" in err()
    assert g(batch=_args(learner, weight_kind=1)) == 1 and "weight_dev" in err()
    assert g(batch=_args(learner, weight_kind=3)) == 1 and "weight_kind" in err()
    # m, n_rows, the cursor's stride, clip
    for kw, word in ((dict(m=0), "batch.m"), (dict(m=-3), "batch.m"), (dict(m=1 << 31), "batch.m"), (dict(n_rows=0), "batch.n_rows"),
                     (dict(m=9), "batch.m"), (dict(cursor=p, rows_per_step=0), "rows_per_step")):
        assert g(batch=_args(learner, **kw)) == 1 and word in err(), (kw, err())
    for clip in (-0.1, float("nan")):
        assert g(lo=learner.LearnerLoss(clip=clip, vf_coef=0.5, ent_coef=0.0)) == 1 and "loss.clip" in err()
    # Adam
    s = lambda params=p, grad=p, opt=p, work=p, ad=adam: L.bcn_learner_step(C.byref(good), params, grad, opt, work, None if ad is None else C.byref(ad), None)
    for kw, word in ((dict(params=None), "params_dev"), (dict(grad=None), "grad_dev"), (dict(opt=None), "opt_dev"), (dict(work=None), "work_dev"),
                     (dict(ad=None), "adam")):
        assert s(**kw) == 1 and "NULL" in err() and word in err(), (kw, err())
    for b1, b2, word in ((1.0, 0.999, "beta1"), (-0.1, 0.999, "beta1"), (0.9, 1.0, "beta2"), (0.9, -1e-3, "beta2"), (float("nan"), 0.5, "beta1")):
        assert s(ad=learner.LearnerAdam(lr=1e-3, beta1=b1, beta2=b2, eps=1e-8, max_grad_norm=0.0)) == 1 and "adam." + word in err()
    assert L.bcn_learner_grad_layout(C.byref(good), None, 0) == 13                         # the count without an array


def test_learner_argument_errors_need_no_gpu():
    from beacon_amd import Actor, Learner
    _lib()
    env = _bare("VecBurgers")
    a = Actor(env, hidden=(5, 7), seed=3)
    with pytest.raises(ValueError, match="actor"):
        Learner(env)
    for kw, word in ((dict(lr=-1.0), "lr"), (dict(lr="fast"), "lr"), (dict(clip_range=-0.2), "clip_range"), (dict(vf_coef=float("nan")), "vf_coef"),
                     (dict(ent_coef=None), "ent_coef"), (dict(eps=-1e-8), "eps"), (dict(betas=(0.9, 1.0)), r"betas\[1\]"),
                     (dict(betas=(-0.1, 0.9)), r"betas\[0\]"), (dict(betas=0.9), "betas"), (dict(max_grad_norm="big"), "max_grad_norm")):
        with pytest.raises(ValueError, match=word):
            Learner(a, **kw)
    ln = Learner(a, lr=1e-3, max_grad_norm=None)
    assert ln.max_grad_norm == 0.0 and ln.betas == (0.9, 0.999) and ln.grid == 256
    assert set(ln.grads) == set(a.weights) and all(ln.grads[k].shape == a.weights[k].shape and ln.grads[k].dtype == a.tdtype for k in a.weights)
    assert ln.m.numel() == ln.v.numel() == a.params.numel() // 4 and ln.step_count.dtype == torch.int32 and ln.stats.dtype == torch.float64
    assert ln.stats.numel() == 8
    with pytest.raises(ValueError, match="unknown"):
        ln.set_hyper(momentum=0.9)
    z = lambda *shape: torch.zeros(*shape)
    ok = dict(obs_rows=z(6, 5), actions=z(6, 1), logp_old=z(6), adv=z(6), ret=z(6))
    for kw, word in ((dict(obs_rows=z(6, 4)), "obs_rows"), (dict(obs_rows=z(0, 5)), "obs_rows"), (dict(obs_rows=z(6, 5).double()), "obs_rows"),
                     (dict(actions=z(6, 2)), "actions"), (dict(actions=z(6, 1).int()), "actions"), (dict(logp_old=z(5)), "logp_old"),
                     (dict(adv=z(7)), "adv"), (dict(ret=z(6).double()), "ret"), (dict(ret=[0.0] * 6), "ret"), (dict(weight=z(5)), "weight"),
                     (dict(weight=z(6).int()), "weight"), (dict(idx=z(3).long()), "idx"), (dict(idx=z(2, 2).int()), "idx"), (dict(idx=z(0).int()), "idx")):
        with pytest.raises(ValueError, match=word):
            ln.grad(**dict(ok, **kw))
    with pytest.raises(RuntimeError, match="no CPU fallback"):     # a missing device is an error, never a host evaluation
        ln.grad(**ok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ln.grad(**dict(ok, weight=z(6).bool(), idx=z(3).int()))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ln.step()
    with pytest.raises(ValueError, match="attached"):
        ln.update(object(), z(6), z(6))
    d = ln.state_dict()
    other = Learner(a).load_state_dict(d)
    assert other.lr == 1e-3 and other.max_grad_norm == 0.0 and torch.equal(other.opt, ln.opt)
    with pytest.raises(ValueError, match="another learner"):
        Learner(Actor(env, hidden=(5, 8))).load_state_dict(d)
    cat = Learner(Actor(_bare("VecLorenz", 3, "f64"), hidden=(8,), activation="relu"))
    assert cat.grads["log_std"].numel() == 0 and cat.m.dtype == torch.float64
    with pytest.raises(ValueError, match="actions"):
        cat.grad(torch.zeros(4, 6, dtype=torch.float64), torch.zeros(4, dtype=torch.float64), *(torch.zeros(4, dtype=torch.float64),) * 3)


def test_reference_gradient_equals_a_central_finite_difference():
    """tests/learner_ref.py on a 1-5-1 network: backward() against (L(theta + h) - L(theta - h)) / 2 h for every parameter, with both clip
    branches, weights and an entropy term in play; and the formulas of include/beacon_learner.h for logp and the entropy directly."""
    rng = np.random.default_rng(4)
    for kind, act_dim, activation in ((0, 1, "tanh"), (1, 3, "tanh")):
        w = {}
        for net, head in (("pi", act_dim), ("vf", 1)):
            for l, (i, o) in enumerate(((1, 5), (5, head))):
                w["%s_w%d" % (net, l)] = rng.uniform(-1, 1, (o, i))
                w["%s_b%d" % (net, l)] = rng.uniform(-0.5, 0.5, o)
        w["log_std"] = rng.uniform(-0.5, 0.5, act_dim)
        ref = R.Ref(w, (5,), activation, kind)
        m = 12
        obs = rng.uniform(-1, 1, (m, 1))
        act = rng.uniform(-1, 1, (m, 1)) if kind == 0 else rng.integers(0, act_dim, m)
        adv, ret, wt = rng.normal(size=m), rng.normal(size=m), rng.integers(0, 3, m).astype(np.float64)
        with torch.no_grad():
            logp = ref.terms(obs, act, np.zeros(m), adv, ret, None, 0.2, 0.5, 0.01)["logp"].numpy()
        logp_old = logp + rng.choice([-1.0, 1.0], m) * rng.uniform(0.02, 0.5, m)
        hyper = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01)
        grads, stats, t = ref.grad(obs, act, logp_old, adv, ret, wt, **hyper)
        assert 0.0 < stats["clip_frac"] < 1.0 and (np.abs(np.abs(t["ratio"].numpy() - 1.0) - 0.2) > 1e-3).all()
        assert stats["weight"] == wt.sum() and abs(stats["loss"] - (stats["pg_loss"] + 0.5 * stats["vf_loss"] - 0.01 * stats["entropy"])) < 1e-14
        if kind == 0:                                         # the header's closed forms
            mean = ref.pi(torch.as_tensor(obs)).detach().numpy()
            z = (act - mean) * np.exp(-w["log_std"])
            assert np.abs(t["logp"].numpy() - (-0.5 * z * z - w["log_std"] - 0.5 * np.log(2 * np.pi)).sum(1)).max() < 1e-14
            assert abs(stats["entropy"] - (w["log_std"] + 0.5 * np.log(2 * np.pi * np.e)).sum() * 1.0) < 1e-13
        h = 1e-6
        for name, p in ref.named:
            flat = p.data.view(-1)
            for i in range(flat.numel()):
                keep = float(flat[i])
                vals = []
                for sgn in (1.0, -1.0):
                    flat[i] = keep + sgn * h
                    with torch.no_grad():
                        vals.append(float(ref.terms(obs, act, logp_old, adv, ret, wt, **hyper)["loss"]))
                flat[i] = keep
                fd = (vals[0] - vals[1]) / (2 * h)
                # the central difference's own error: h^2 |L'''| / 6 + rounding 2^-53 |L| / h, both far below 1e-7 here
                assert abs(fd - float(grads[name].view(-1)[i])) < 1e-7, (kind, name, i, fd, float(grads[name].view(-1)[i]))
    # Adam + clip_grad_norm_ is torch's: one step from zero moments moves every parameter by lr against the gradient's sign
    before = [p.detach().clone() for p in ref.parameters()]
    opt = ref.adam(1e-3, (0.9, 0.999), 1e-12)
    norm = ref.clip_and_step(opt, 0.5 * stats["grad_norm"])
    assert abs(norm - stats["grad_norm"]) < 1e-12
    for b, p in zip(before, ref.parameters()):
        nz = p.grad != 0
        assert torch.allclose((b - p.detach())[nz], 1e-3 * torch.sign(p.grad[nz]), rtol=1e-6, atol=0)
    assert ref.moments(opt)[2] == 1


def test_float32_reference_agrees_with_the_float64_one():
    """Ref(dtype=torch.float32) on two cases of tests/test_gpu_learner.py, on the float32 data of the case: per segment, its error
    against the float64 reference is below 1e-5 of the segment's max |ref| (measured: at most 1.4e-6) -- and it is not the float64
    answer under another name, which would leave it without the float32 roundoff that the GPU test measures the device against."""
    import test_gpu_learner as G
    for i in (1, 8):                                  # 65 x 33 (17, 128, 3) relu Gaussian; 2305 x 6 (64, 64) tanh, categorical 16
        case, cid = G.CASES[i], G.IDS[i]
        d = G.case_data(case, torch.float32, G.SEEDS[cid])
        assert set(d["grads32"]) == set(d["grads"])
        rels = {}
        for k, g in d["grads"].items():
            assert d["grads32"][k].dtype == torch.float32 and g.dtype == torch.float64 and float(g.abs().max()) > 0.0, k
            rels[k] = G.rel(d["grads32"][k], g)
        print("float32 reference %s: rel %.3e .. %.3e" % (cid, min(rels.values()), max(rels.values())))
        assert max(rels.values()) < 1e-5, rels
        assert min(rels.values()) > 2.0 ** -30, rels  # float32 roundoff is there in every segment
    # the same loss in the same precision: the statistics agree to float32 roundoff too
    r32 = R.Ref(d["w"], case[2], case[3], 1, dtype=torch.float32)
    _, s32, t32 = r32.grad(d["obs"], d["act"], d["logp_old"], d["adv"], d["ret"], None, G.CLIP, G.VF_COEF, G.ENT_COEF)
    assert t32["loss"].dtype == torch.float32 and all(p.dtype == torch.float32 for p in r32.parameters())
    for k, v in d["stats"].items():
        assert abs(s32[k] - v) <= 1e-5 * max(1.0, abs(v)), (k, s32[k], v)


def test_every_gpu_case_has_data_that_exercises_it():
    """check_reference of tests/test_gpu_learner.py on every case, in both dtypes: a seed that leaves a ratio on a clip boundary, a relu
    pre-activation at 0, clip_frac outside [0.2, 0.8] or a row term outside f64_tol's bound is found here, without a GPU; and the
    late-Adam test's three reference steps keep their margins."""
    import test_gpu_learner as G
    assert len(G.CASES) == len(G.IDS) == len(set(G.IDS)) == len(G.SEEDS) == 11
    for case, cid in zip(G.CASES, G.IDS):
        for dtype in (torch.float64, torch.float32):
            d = G.case_data(case, dtype, G.SEEDS[cid])
            G.check_reference(case, d)
            assert (d["grads32"] is None) == (dtype == torch.float64)
    # the selections: the first idx case is 130 rows of 257, the second names every row and 100 of them twice
    d = G.case_data(G.CASES[4], torch.float32, G.SEEDS[G.IDS[4]])
    assert d["m"] == 130 and len(set(d["idx"].tolist())) == 130
    d = G.case_data(G.CASES[7], torch.float32, G.SEEDS[G.IDS[7]])
    assert d["m"] == 16485 > d["obs"].shape[0] and set(d["idx"].tolist()) == set(range(16385))
    assert 0.25 < float((d["weight"] == 0).double().mean()) < 0.42
    # the regimes the cases are named for, from the library's own grid
    from beacon_amd import actor, learner
    L = _lib()
    for i, cid in enumerate(G.IDS):
        if cid not in G.REGIME:
            continue
        m, obs_dim, hidden, activation, kind, n, _ = G.CASES[i]
        rows = G.case_data(G.CASES[i], torch.float32, G.SEEDS[cid])["m"]
        for f64 in (False, True):
            cfg = _cfg(dtype=int(f64), hidden=hidden, obs_dim=obs_dim, act_dim=n, kind=int(kind == "categorical"))
            grid = L.bcn_learner_grid(C.byref(cfg))
            assert G.REGIME[cid](grid, G.n_tiles(rows, torch.float64 if f64 else torch.float32), f64), (cid, f64, grid)
    for dtype in (torch.float64, torch.float32):
        _, _, _, norms, margins = G.late_reference(dtype, 0.0)
        assert min(r for r, _ in margins) > 1e-4 and min(p for _, p in margins) > 1e-5 and min(norms) > 1.2 * 0.5, (margins, norms)


def test_learner_units_compile_for_gfx950_without_dpp_hazards():
    from beacon_amd import build, learner
    tool = H.objdump()
    if tool is None or (build.hipcc() is None and not os.path.exists(learner.LIB)):
        pytest.skip("no llvm-objdump / no hipcc and no prebuilt library")
    assert sorted(os.path.basename(s) for s in learner.sources()) == sorted(learner.FILE_FLAGS) == ["learner.hip", "learner_f64.hip"]
    assert "-ffp-contract=off" in learner.FILE_FLAGS["learner_f64.hip"]
    lib = learner.build_learner()
    assert not learner.stale()
    rep = H.scan_file(lib, tool)
    H.summarise(rep)
    assert rep["code_objects"] >= 1 and not rep["findings"], rep["findings"]
    # no inline assembly in the new units (the allow-list test walks them too)
    for f in os.listdir(learner.SRC_DIR):
        assert "asm" not in re.sub(r"//.*", "", open(os.path.join(learner.SRC_DIR, f)).read()), f
