"""CPU-side checks of the per-jet mode of the actor and the learner (no GPU): the appended cfg field in the header and the binding,
the layouts of a cfg with agents, the library's refusals with a code and a message naming the field, the argument errors of
Actor(per_jet=True) and Learner.grad(rows_per_weight=...) on bare envs, and the per-row Philox keys of tests/actor_ref.py when it is
called the way the per-jet rows are keyed: B n_jets rows with replica_offset n_jets."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import actor_ref as R
from test_actor_host import _bare, _cfg


def _libs():
    from beacon_amd import actor, build, learner
    if build.hipcc() is None and not (os.path.exists(actor.LIB) and os.path.exists(learner.LIB)):
        pytest.skip("no hipcc and no prebuilt libraries")
    return actor.load(), learner.load()


def test_cfg_fields_are_the_headers():
    from beacon_amd import actor
    hdr = open(os.path.join(ROOT, "include", "beacon_actor.h")).read()
    body = re.search(r"typedef struct \{([^{}]*)\} bcn_actor_cfg;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        if not decl.strip():
            continue
        ctype, names = decl.strip().split(None, 1)
        for n in names.split(","):
            m = re.match(r"(\w+)(?:\[(\d+)\])?$", n.strip())
            base = {"int32_t": C.c_int32, "double": C.c_double}[ctype]
            fields.append((m.group(1), base * int(m.group(2)) if m.group(2) else base))
    got = actor.ActorCfg._fields_
    assert [n for n, _ in fields] == [n for n, _ in got]
    assert all(C.sizeof(a) == C.sizeof(b) and (a is b or hasattr(b, "_length_")) for (_, a), (_, b) in zip(fields, got))
    assert fields[-1][0] == "agents" and fields[-2][0] == "high"          # appended: every older field keeps its offset
    assert actor.ActorCfg.agents.offset == actor.ActorCfg.high.offset + 8
    assert actor.make_cfg(4, 5, 0, (8,), "tanh", 0, 1).agents == 1 and _cfg(agents=5).agents == 5
    assert actor.ActorCfg().agents == 0                                    # a zero-filled tail: the old behaviour
    # the learner's batch: the new field is the last one too (tests/test_learner_host.py compares every name with the header)
    from beacon_amd import learner
    assert learner.LearnerBatch._fields_[-1][0] == "rows_per_weight" and learner.LearnerBatch._fields_[-2][0] == "rows_per_step"
    assert learner.LearnerBatch().rows_per_weight == 0


def test_layouts_with_agents_are_those_of_the_rows():
    from beacon_amd import actor
    _libs()
    for dtype in (0, 1):
        for B, A in ((13, 5), (7, 20), (65, 3)):
            with_a, flat, zero = (_cfg(batch=B * A, obs_dim=6, act_dim=1, dtype=dtype, agents=a) for a in (A, 1, 0))
            for which, extra in (("params", ()), ("state", ()), ("seq", (4,))):
                assert actor.layout(which, with_a, *extra) == actor.layout(which, flat, *extra) == actor.layout(which, zero, *extra)


def test_library_refuses_bad_agents_with_code_and_message():
    from beacon_amd import actor, learner
    L, LL = _libs()
    segs = (actor.ActorSeg * actor.MAX_SEGS)()
    p = C.c_void_p(64)
    neg = _cfg(agents=-1)
    for fn in ("params", "state"):
        assert getattr(L, "bcn_actor_%s_layout" % fn)(C.byref(neg), segs, actor.MAX_SEGS) == 0 and b"cfg.agents" in L.bcn_actor_last_error()
        assert getattr(L, "bcn_actor_%s_bytes" % fn)(C.byref(neg)) == 0
    assert L.bcn_actor_seq_bytes(C.byref(neg), 4) == 0 and b"cfg.agents" in L.bcn_actor_last_error()
    assert L.bcn_actor_act(C.byref(neg), p, p, p, None, 0, 0, 0, None, 0, None, None) == 1 and b"cfg.agents" in L.bcn_actor_last_error()
    assert L.bcn_actor_values(C.byref(neg), p, p, 1, p, None) == 1 and b"cfg.agents" in L.bcn_actor_last_error()
    with pytest.raises(actor.BeaconActorError, match="agents"):
        actor.layout("params", neg)
    assert LL.bcn_learner_grad_bytes(C.byref(neg)) == 0 and b"cfg.agents" in LL.bcn_learner_last_error()
    odd = _cfg(batch=66, agents=5)
    assert L.bcn_actor_state_layout(C.byref(odd), segs, actor.MAX_SEGS) == 0
    assert b"cfg.agents" in L.bcn_actor_last_error() and b"cfg.batch" in L.bcn_actor_last_error()
    assert L.bcn_actor_state_bytes(C.byref(odd)) == 0 and L.bcn_actor_seq_bytes(C.byref(odd), 4) == 0
    assert L.bcn_actor_act(C.byref(odd), p, p, p, None, 0, 0, 0, None, 0, None, None) == 1 and b"cfg.agents" in L.bcn_actor_last_error()
    with pytest.raises(actor.BeaconActorError, match="agents"):
        actor.layout("state", odd)
    # where the batch is not needed it is not looked at: the parameters, the value launch's cfg check and the learner
    assert actor.layout("params", odd) == actor.layout("params", _cfg(batch=66))
    assert LL.bcn_learner_grad_bytes(C.byref(odd)) == L.bcn_actor_params_bytes(C.byref(odd)) > 0
    assert L.bcn_actor_state_layout(C.byref(_cfg(batch=65, agents=5)), segs, actor.MAX_SEGS) == 6
    # the learner's new batch field
    loss = learner.LearnerLoss(clip=0.2, vf_coef=0.5, ent_coef=0.0)
    good = _cfg()

    def grad(**kw):
        b = dict(obs=p, act=p, logp_old=p, adv=p, ret=p, weight=None, idx=None, cursor=None, n_rows=10, m=10, weight_kind=0, rows_per_step=0)
        b.update(kw)
        return LL.bcn_learner_grad(C.byref(good), p, C.byref(learner.LearnerBatch(**b)), C.byref(loss), p, p, None)
    for rpw in (-1, 3, 4, 20):
        assert grad(rows_per_weight=rpw) == 1 and "batch.rows_per_weight" in LL.bcn_learner_last_error().decode(), rpw
    assert "batch.n_rows" in LL.bcn_learner_last_error().decode()


class _Jets(object):
    """what Actor(per_jet=True) reads of a VecShkadov, on the CPU"""
    _norm_on = False
    action_is_int = False

    def __init__(self, batch, n_jets, n_obs, dtype=torch.float32):
        from beacon_amd import spaces
        self.batch, self.n_jets, self.n_obs, self.obs_dim = batch, n_jets, n_obs, n_jets * n_obs
        self.tdtype, self.device = dtype, torch.device("cpu")
        self.action_space = spaces.box(-1.0, 1.0, (n_jets,))
        self.obs = None


def test_per_jet_argument_errors_need_no_gpu():
    from beacon_amd import Actor, Learner
    _libs()
    for env in (_bare("VecBurgers"), _bare("VecLorenz", 3, "f64")):                  # a Box without jets, a Discrete
        with pytest.raises(ValueError, match="per_jet=True needs"):
            Actor(env, hidden=(5,), per_jet=True)
    env = _Jets(4, 20, 3)
    with pytest.raises(ValueError, match="20 components"):                           # as one agent the film is too wide, as today
        Actor(env, hidden=(5,))
    bad = _Jets(4, 20, 3)
    bad.obs_dim = 61
    with pytest.raises(ValueError, match="per_jet=True needs"):
        Actor(bad, hidden=(5,), per_jet=True)
    a = Actor(env, hidden=(5, 7), seed=3, replica_offset=2, per_jet=True)
    assert (a.kind, a.act_dim, a.obs_dim, a.agents, a.batch, a.rows, a.cfg.batch, a.cfg.agents) == (0, 1, 3, 20, 4, 80, 80, 20)
    for name in ("actions", "raw", "dist", "logp", "value", "counters"):
        assert tuple(getattr(a, name).shape) == (4, 20), name
    assert a.counters.dtype == torch.int32 and tuple(a.weights["pi_w0"].shape) == (5, 3) and tuple(a.weights["pi_w2"].shape) == (1, 7)
    for obs in (torch.zeros(4, 61), torch.zeros(80, 4), torch.zeros(4, 20, 3), torch.zeros(4, 60, dtype=torch.float64), torch.zeros(80, 60)[:, :3]):
        with pytest.raises(ValueError, match="obs"):
            a.act(obs=obs)
    with pytest.raises(ValueError, match="mask must hold 4"):
        a.act(obs=torch.zeros(4, 60), mask=torch.ones(80, dtype=torch.uint8))
    for obs in (torch.zeros(4, 60), torch.zeros(80, 3)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):                   # both shapes pass the checks
            a.act(obs=obs, mask=[1, 0, 1, 1])
    with pytest.raises(ValueError, match="obs_rows"):
        a.values(torch.zeros(4, 60))
    d = a.state_dict()
    assert d["agents"] == 20 and d["batch"] == 4
    assert Actor(env, hidden=(5, 7), per_jet=True).load_state_dict(d).replica_offset == 2
    flat = _Jets(80, 1, 3)
    with pytest.raises(ValueError, match="another actor"):
        Actor(flat, hidden=(5, 7)).load_state_dict(d)
    plain = Actor(flat, hidden=(5, 7))
    old = plain.state_dict()
    assert old.pop("agents") == 1
    plain.load_state_dict(old)                                                       # a state from before the field: a plain actor's
    with pytest.raises(ValueError, match="another actor"):
        Actor(_Jets(80, 1, 3), hidden=(5, 7), per_jet=True).load_state_dict(dict(old, agents=2))

    # Learner.grad: rows_per_weight is checked before any launch
    ln = Learner(Actor(_Jets(2, 5, 3), hidden=(5,), per_jet=True))
    z = lambda *shape, **kw: torch.zeros(*shape, **kw)
    ok = dict(obs_rows=z(10, 3), actions=z(10, 1), logp_old=z(10), adv=z(10), ret=z(10))
    for kw in (dict(rows_per_weight=0), dict(rows_per_weight=3), dict(rows_per_weight=-5), dict(rows_per_weight=2.0), dict(rows_per_weight=True),
               dict(rows_per_weight=None), dict(rows_per_weight=3, weight=z(3))):
        with pytest.raises(ValueError, match="rows_per_weight"):
            ln.grad(**dict(ok, **kw))
    for kw in (dict(rows_per_weight=5, weight=z(10)), dict(rows_per_weight=5, weight=z(3)), dict(rows_per_weight=2, weight=z(2, dtype=torch.uint8)),
               dict(rows_per_weight=1, weight=z(2))):
        with pytest.raises(ValueError, match="weight"):
            ln.grad(**dict(ok, **kw))
    for kw in (dict(rows_per_weight=5, weight=z(2)), dict(rows_per_weight=5, weight=z(2, dtype=torch.uint8)), dict(rows_per_weight=10, weight=z(1).bool()),
               dict(rows_per_weight=2), dict(weight=z(10))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ln.grad(**dict(ok, **kw))


def test_reference_keys_of_the_per_jet_rows_are_distinct():
    """Row b A + j of a per-jet actor is keyed as row b A + j of a flat batch with replica_offset A: word 0 is
    (replica_offset A + b A + j) mod 2^32.  For (B, A) = (13, 5) no two rows share a draw, over shards and draw counters."""
    B, A, seed = 13, 5, 0x1234567887654321
    rows = np.arange(B * A)
    seen = {}
    for off in (0, 3):
        for ctr in (0, 1):
            w = np.stack(R.words(seed, off * A, rows, ctr, 0))
            assert len({tuple(c) for c in w.T}) == B * A
            seen[off, ctr] = w
    # replica_offset stays the index of the shard's first REPLICA: shard 3's rows are the unsharded batch's rows 15 ..
    whole = np.stack(R.words(seed, 0, np.arange((B + 3) * A), 0, 0))
    assert np.array_equal(seen[3, 0], whole[:, 3 * A:])
    assert not np.array_equal(seen[0, 0], seen[0, 1])
    # and the index wraps as the plain actor's does
    hi = np.stack(R.words(seed, ((1 << 32) // A + 1) * A, rows[:4], 0, 0))
    assert np.array_equal(hi, np.stack(R.words(seed, ((1 << 32) // A + 1) * A - (1 << 32), rows[:4], 0, 0)))
