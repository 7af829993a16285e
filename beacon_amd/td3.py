"""Off-policy learning on the device: libbeacon_td3.so (include/beacon_td3.h; csrc/td3/) and the classes Replay and TD3 over it.

A Replay is a ring of transitions on the device that Rollouts are appended to and minibatches are sampled from with the project's
one Philox definition; a TD3 is a deterministic policy mu(s) with one or two critics Q(s, a), their targets and two Adam
optimisers.  Acting is ONE launch; an update of one minibatch -- sample, critic gradient, Adam, and on every policy_delay-th
minibatch policy gradient through Q_1, Adam, Polyak -- is 8 or 15 launches of the library's own: no host read, no allocation, no
atomics, every sum in a fixed order, bit-reproducible, and capturable as ONE graph whose replays draw new samples and new noise
(the counters live on the device).  tests/td3_ref.py restates it on the host.

The library is a unit of its own, built and bound like the actor's, the learner's and the epochs' (build.py: one Unit each); its
table is SIGNATURES below.  Importing this module touches neither a compiler nor the GPU."""
import ctypes as C
import os
import weakref

import numpy as np
import torch

from . import _lib
from . import actor as _actor
from . import build as _build

API_VERSION = 1                           # include/beacon_td3.h: BCN_TD3_API_VERSION
# the float64 unit: one rounding per written operation, as actor_f64.hip and learner_f64.hip
FILE_FLAGS = {"td3.hip": [],
              "td3_f64.hip": ["-ffp-contract=off"]}
REAL, I32, U32, F64, U8 = 0, 1, 2, 3, 4   # BCN_TD3_REAL ...
DETERMINISTIC, NOISY, UNIFORM = 0, 1, 2
MODES = {"deterministic": DETERMINISTIC, "noisy": NOISY, "uniform": UNIFORM}
OPT_CRITIC, OPT_POLICY = 0, 1
MAX_IN, MAX_GRID, MAX_SEGS = 512, 128, 32
STATS = ("critic_loss", "q1_mean", "q2_mean", "target_mean", "policy_loss", "W", "critic_grad_norm", "policy_grad_norm")
_vp = C.c_void_p


class Td3Cfg(C.Structure):
    """bcn_td3_cfg"""
    _fields_ = [("batch", C.c_int32), ("obs_dim", C.c_int32), ("act_dim", C.c_int32), ("dtype", C.c_int32), ("n_hidden", C.c_int32),
                ("hidden", C.c_int32 * 3), ("activation", C.c_int32), ("low", C.c_double), ("high", C.c_double), ("n_critics", C.c_int32)]


class Td3Seg(C.Structure):
    """bcn_td3_seg"""
    _fields_ = [("name", C.c_char * 16), ("offset", C.c_uint64), ("elem", C.c_int32), ("planes", C.c_int32), ("row_elems", C.c_int64)]


class Td3Batch(C.Structure):
    """bcn_td3_batch"""
    _fields_ = [("params", _vp), ("target", _vp), ("mem", _vp), ("idx", _vp), ("work", _vp), ("state", _vp), ("m", C.c_int64),
                ("capacity", C.c_int64), ("gamma", C.c_double), ("target_noise", C.c_double), ("noise_clip", C.c_double), ("seed", C.c_uint64)]


class Td3Adam(C.Structure):
    """bcn_td3_adam_hyper"""
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("max_grad_norm", C.c_double)]


_cfgp, _segp, _batchp = C.POINTER(Td3Cfg), C.POINTER(Td3Seg), C.POINTER(Td3Batch)
# every symbol include/beacon_td3.h declares: (restype, argtypes)
SIGNATURES = {
    "bcn_td3_params_layout": (C.c_int, [_cfgp, _segp, C.c_int]),
    "bcn_td3_params_bytes": (C.c_size_t, [_cfgp]),
    "bcn_td3_state_layout": (C.c_int, [_cfgp, _segp, C.c_int]),
    "bcn_td3_state_bytes": (C.c_size_t, [_cfgp]),
    "bcn_td3_work_layout": (C.c_int, [_cfgp, C.c_int64, _segp, C.c_int]),
    "bcn_td3_work_bytes": (C.c_size_t, [_cfgp, C.c_int64]),
    "bcn_replay_layout": (C.c_int, [_cfgp, C.c_int64, _segp, C.c_int]),
    "bcn_replay_bytes": (C.c_size_t, [_cfgp, C.c_int64]),
    "bcn_td3_grid": (C.c_int, [_cfgp]),
    "bcn_td3_act": (C.c_int, [_cfgp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_double, C.c_uint64, C.c_int64, _vp]),
    "bcn_replay_append": (C.c_int, [_cfgp, C.c_int64, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "bcn_replay_sample": (C.c_int, [C.c_int64, C.c_uint64, _vp, _vp, _vp]),
    "bcn_td3_critic_grad": (C.c_int, [_cfgp, _batchp, _vp]),
    "bcn_td3_actor_grad": (C.c_int, [_cfgp, _batchp, _vp]),
    "bcn_td3_adam": (C.c_int, [_cfgp, _vp, _vp, _vp, C.c_int, C.POINTER(Td3Adam), _vp]),
    "bcn_td3_polyak": (C.c_int, [_cfgp, _vp, _vp, C.c_double, _vp]),
    "bcn_td3_last_error": (C.c_char_p, []),
}


class BeaconTd3Error(RuntimeError):
    pass


# ---- the library -------------------------------------------------------------------------
# (the units include the network the actor and the learner run, csrc/actor/policy_net.h, through the actor's kernel header: the
# dependency rule of build.py follows the #include lines there)
SRC_DIR, HEADER = os.path.join(_build.CSRC, "td3"), os.path.join(_build.INC, "beacon_td3.h")
LIB, OBJ = os.path.join(_build.PKG, "libbeacon_td3.so"), os.path.join(_build.OBJ, "td3")
_UNIT = _build.hip_library(LIB, SRC_DIR, FILE_FLAGS, OBJ, SIGNATURES)
sources, signature, stale, load = _UNIT.sources, _UNIT.signature, _UNIT.stale, _UNIT.load


def build_td3(force=False, verbose=False):
    """Compile csrc/td3/*.hip for gfx950 and link libbeacon_td3.so.  Returns its path."""
    return _UNIT.build(force=force, verbose=verbose)


def _check(rc):
    if rc != 0:
        raise BeaconTd3Error("libbeacon_td3: error %d: %s" % (rc, load().bcn_td3_last_error().decode()))


def make_cfg(batch, obs_dim, act_dim, dtype, hidden, activation, low=-1.0, high=1.0, n_critics=2):
    """bcn_td3_cfg from plain values (dtype: 0 / 1; activation: "tanh" / "relu" or 0 / 1).  No range check: the library's."""
    hid = [int(h) for h in hidden]
    return Td3Cfg(batch=int(batch), obs_dim=int(obs_dim), act_dim=int(act_dim), dtype=int(dtype), n_hidden=len(hid),
                  hidden=(C.c_int32 * 3)(*(hid + [0] * 3)[:3]), activation=_actor._ACTIVATIONS.get(activation, activation),
                  low=float(low), high=float(high), n_critics=int(n_critics))


def layout(which, cfg, arg=None):
    """([segment dicts], bytes) of the "params", "state", "work" (arg: the minibatch rows m) or "replay" (arg: the capacity)
    buffer of `cfg`; BeaconTd3Error with the library's text for what it refuses.  No device needed."""
    L = load()
    segs = (Td3Seg * MAX_SEGS)()
    extra = () if which in ("params", "state") else (int(arg),)
    prefix = "bcn_replay" if which == "replay" else "bcn_td3_" + which
    k = getattr(L, prefix + "_layout")(C.byref(cfg), *(extra + (segs, MAX_SEGS)))
    nbytes = getattr(L, prefix + "_bytes")(C.byref(cfg), *extra)
    if k == 0 or nbytes == 0:
        raise BeaconTd3Error("libbeacon_td3: %s" % L.bcn_td3_last_error().decode())
    return ([dict(name=g.name.decode(), offset=int(g.offset), elem=int(g.elem), planes=int(g.planes), row_elems=int(g.row_elems))
             for g in segs[:k]], int(nbytes))


def _views(buf, segs, real):
    out = {}
    for s in segs:
        dt = {REAL: real, I32: torch.int32, U32: torch.int32, F64: torch.float64, U8: torch.uint8}[s["elem"]]
        out[s["name"]] = buf[s["offset"]:s["offset"] + s["row_elems"] * torch.empty((), dtype=dt).element_size()].view(dt)
    return out


def _number(who, name, x, lo=None, lo_open=False, hi=None, hi_closed=False):
    if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not np.isfinite(x):
        raise ValueError("%s: %s must be a finite number, got %r" % (who, name, x))
    x = float(x)
    if lo is not None and (x <= lo if lo_open else x < lo):
        raise ValueError("%s: %s must be %s %g, got %r" % (who, name, ">" if lo_open else ">=", lo, x))
    if hi is not None and (x > hi if hi_closed else x >= hi):
        raise ValueError("%s: %s must be %s %g, got %r" % (who, name, "<=" if hi_closed else "<", hi, x))
    return x


def _count(who, name, x):
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < 1:
        raise ValueError("%s: %s must be an integer >= 1, got %r" % (who, name, x))
    return int(x)


_p = _actor._ptr


# ---- the replay memory -------------------------------------------------------------------
class Replay(object):
    """A ring of `capacity` transitions on the device (agent.replay(capacity) makes one; include/beacon_td3.h states the layout):
    `buf`, one uint8 tensor, and typed no-copy views of its segments --
      head int32 [4]: [0] the write position, [1] the rows stored (<= capacity), [2] the rows ever appended (it wraps), [3] the
      samples drawn; obs [C, obs_dim], act [C, act_dim], rwd [C], next_obs [C, obs_dim]; boot, live uint8 [C].
    append(ro) moves the recorded steps of a Rollout into the ring (TWO launches, the rollout's cursor read on the device):
    next_obs is the rollout's final_obs row where the step ended an episode, else obs[t + 1]; boot = 1 unless the episode TERMINATED
    (done without trunc: the bootstrap rule of Rollout.compute_gae); live = valid.  The memory copies what the rollout holds: under
    env.set_normalize those are the NORMALISED observations and rewards, as of the statistics at the time of each step.
    sample(idx) draws idx.numel() row numbers with replacement (TWO launches; a pure function of (m, seed, head[1], head[3])).
    Not covered: compaction (a row with live = 0 occupies a slot and weighs nothing), prioritised sampling, n-step returns."""

    def __init__(self, agent, capacity):
        from . import dqn as _dqn, sac as _sac            # (here, not at the top: both import this module)
        if not isinstance(agent, (TD3, _sac.SAC, _dqn.DQN)):
            raise ValueError("Replay: agent must be a beacon_amd.TD3, got %r" % (type(agent).__name__,))
        if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or not 1 <= int(capacity) < 1 << 31:
            raise ValueError("Replay: capacity must be an integer in 1 .. 2^31 - 1, got %r" % (capacity,))
        self.agent, self.capacity = agent, int(capacity)
        # a SAC agent's memory is this library's too: its replay_cfg is a bcn_td3_cfg of the same batch, dims, dtype and widths; a DQN
        # agent's likewise, with act_dim = 1 (the action index), and its append is libbeacon_dqn.so's: ro.act is int32 [T, B] there
        self._int_act = isinstance(agent, _dqn.DQN)
        self.cfg, self.lib = (agent.cfg, agent.lib) if isinstance(agent, TD3) else (agent.replay_cfg, load())
        self.tdtype, self.device = agent.tdtype, agent.device
        self.layout, nbytes = layout("replay", self.cfg, self.capacity)
        self.buf = torch.zeros((nbytes,), dtype=torch.uint8, device=self.device)
        v = _views(self.buf, self.layout, self.tdtype)
        Cn = self.capacity
        self.head, self.rwd, self.boot, self.live = v["head"], v["rwd"], v["boot"], v["live"]
        self.obs, self.next_obs = v["obs"].view(Cn, agent.obs_dim), v["next_obs"].view(Cn, agent.obs_dim)
        self.act = v["act"].view(Cn, agent.act_dim)
        self._keep = None

    def append(self, ro):
        """The steps `ro` has recorded since its begin(), into the ring.  ValueError -- before any launch -- for a rollout without
        final_obs, of another batch, observation width, dtype or device, with integer actions, or with T B > capacity."""
        a = self.agent
        if not (int(getattr(ro, "flags", 0)) & _lib.RO_FINAL_OBS):
            raise ValueError("Replay.append: the rollout has no final_obs segment: make it with env.rollout(T, final_obs=True) -- "
                             "next_obs of a step that ends an episode is the terminal observation")
        T = int(ro.T)
        if int(ro.batch) != a.batch or T * a.batch > self.capacity:
            raise ValueError("Replay.append: a rollout of T = %d steps of %d replicas; this memory takes T B <= %d of %d replicas"
                             % (T, int(ro.batch), self.capacity, a.batch))
        if self._int_act and (ro.act.dtype != torch.int32 or ro.act.device != self.device or tuple(ro.act.shape) != (T, a.batch)):
            raise ValueError("Replay.append: ro.act must be int32 [%d, %d] on %s for a DQN agent (the rollout of a discrete env), got %s %s"
                             % (T, a.batch, self.device, str(ro.act.dtype).replace("torch.", ""), tuple(ro.act.shape)))
        for name, cols in (("obs", a.obs_dim), ("final_obs", a.obs_dim), ("act", a.act_dim), ("rwd", None)):
            if self._int_act and name == "act":
                continue
            t = getattr(ro, name)
            if t.dtype != self.tdtype or t.device != self.device or (cols is not None and t.shape[-1] != cols):
                raise ValueError("Replay.append: ro.%s must be %s on %s%s" % (name, str(self.tdtype).replace("torch.", ""), self.device,
                                                                            "" if cols is None else " with rows of %d" % cols))
        stream = a._stream()
        self._keep = ro
        if self._int_act:
            a._append(self, ro, T)
            return self
        _check(self.lib.bcn_replay_append(C.byref(self.cfg), self.capacity, _p(self.buf), T, _p(ro.obs), _p(ro.act), _p(ro.rwd), _p(ro.done),
                                          _p(ro.trunc), _p(ro.valid), _p(ro.final_obs), _p(ro.cursor), stream))
        return self

    def sample(self, idx, seed=None):
        """idx (int32 [m] on the device) = m row numbers below max(head[1], 1); then head[3] += 1.  Returns idx."""
        if not torch.is_tensor(idx) or idx.dtype != torch.int32 or idx.device != self.device or not idx.is_contiguous() or idx.numel() < 1:
            raise ValueError("Replay.sample: idx must be a contiguous int32 tensor of at least one element on %s" % self.device)
        _check(self.lib.bcn_replay_sample(idx.numel(), self.agent.seed if seed is None else int(seed), _p(self.head), _p(idx), self.agent._stream()))
        return idx

    def state_dict(self):
        """For checkpoints: the buffer on the CPU and what it was laid out for."""
        a = self.agent
        return {"buf": self.buf.cpu(), "capacity": self.capacity, "obs_dim": a.obs_dim, "act_dim": a.act_dim,
                "dtype": "f64" if self.tdtype == torch.float64 else "f32"}

    def load_state_dict(self, d):
        a = self.agent
        cur = {"capacity": self.capacity, "obs_dim": a.obs_dim, "act_dim": a.act_dim, "dtype": "f64" if self.tdtype == torch.float64 else "f32"}
        if any(d.get(k) != v for k, v in cur.items()) or d["buf"].numel() != self.buf.numel():
            raise ValueError("Replay.load_state_dict: the state is of another memory (%s); this one is %s" % ({k: d.get(k) for k in cur}, cur))
        self.buf.copy_(d["buf"])
        return self


# ---- the agent ---------------------------------------------------------------------------
class TD3(object):
    """TD3 (Fujimoto, van Hoof, Meger 2018) / DDPG on the device for one VecEnv with a Box action space (include/beacon_td3.h states
    every formula, order and stream; csrc/td3/td3_impl.h is the kernels).

        agent = TD3(env, hidden=(64, 64), lr=1e-3, gamma=0.99, tau=0.005, policy_delay=2,
                    explore_noise=0.1, target_noise=0.2, noise_clip=0.5, twin=True, seed=None)
        agent.load_modules(mu, q1, q2)        # nn.Sequential of Linear + Tanh/ReLU; also sets the targets
        mem = agent.replay(capacity); ro = env.rollout(T)
        env.reset()
        for it in range(n_iter):
            ro.begin()
            for _ in range(T):
                env.step_autoreset(agent.act(mode="uniform" if it < warm else "noisy"))
            mem.append(ro)
            agent.update(mem, n_updates=T, batch_size=256)

    mu maps obs_dim -> act_dim, a = c + h tanh(head) with c, h the centre and half width of the Box; the critics map [obs | a] -> 1.
    Owns `params` and `target` (one uint8 buffer each in the layout of bcn_td3_params_layout; `weights` / `target_weights` map the
    segment names -- mu_w0, mu_b0, ... q1_w0, ... q2_w0 ... -- to typed views, matrices [out, in]), `state` (counters int32 [B]: the
    exploration stream's uint32 draw counters' bits; step_count int32 [4]: [0] the critic's Adam steps, [1] the policy's, [2] the
    smoothing draws; stats float64 [8]; adam_m, adam_v) and `actions` [B, act_dim].  Fresh parameters are zero.
    act(): ONE launch.  update(mem, n_updates, batch_size): per minibatch sample (2 launches) + critic gradient (4) + Adam (2), and
    on every policy_delay-th minibatch ((k + 1) % policy_delay == 0, plain control flow) policy gradient through Q_1 (4) + Adam (2) +
    Polyak (1).  plan(mem, n_updates, batch_size) is the same chain allocated once, with run() and capture().
    The hyperparameters are plain attributes and ARGUMENTS of the launches: a captured graph keeps what it was recorded with.
    max_grad_norm (None or <= 0: off, the default) clips each optimiser's gradient by its own global norm.
    stats_dict() is the only host read.
    Not covered: discrete action spaces (mixing, lorenz) and per_jet policies -- ValueError; Boxes with different bounds per
    component; SAC; prioritised replay; n-step returns; ShardedVecEnv."""

    def __init__(self, env, hidden=(64, 64), activation="tanh", lr=1e-3, gamma=0.99, tau=0.005, policy_delay=2, explore_noise=0.1,
                 target_noise=0.2, noise_clip=0.5, twin=True, seed=None, replica_offset=0, betas=(0.9, 0.999), eps=1e-8,
                 max_grad_norm=None, per_jet=False):
        if per_jet:
            raise ValueError("TD3: per_jet policies are not covered: the deterministic policy and its critics serve the whole action row")
        try:
            hid = [int(h) for h in hidden]
            ok = all(int(h) == h and not isinstance(h, bool) for h in hidden)
        except (TypeError, ValueError):
            hid, ok = [], False
        if not ok or not 1 <= len(hid) <= _actor.MAX_LAYERS or any(not 1 <= h <= _actor.MAX_HIDDEN for h in hid):
            raise ValueError("TD3: hidden must be 1 .. %d integer widths of 1 .. %d, got %r" % (_actor.MAX_LAYERS, _actor.MAX_HIDDEN, hidden))
        if activation not in _actor._ACTIVATIONS:
            raise ValueError("TD3: activation must be 'tanh' or 'relu', got %r" % (activation,))
        space = getattr(env, "action_space", None)
        if space is None:
            raise ValueError("TD3: env has no action_space")
        if getattr(env, "action_is_int", False) or not (hasattr(space, "low") and hasattr(space, "high")):
            raise ValueError("TD3: env.action_space is discrete; a deterministic policy needs a Box (the discrete envs, mixing and lorenz, "
                             "are not covered)")
        lo, hi = np.asarray(space.low, dtype=np.float64).reshape(-1), np.asarray(space.high, dtype=np.float64).reshape(-1)
        act_dim, obs_dim = int(lo.size), int(env.obs_dim)
        if not 1 <= act_dim <= _actor.MAX_ACT:
            raise ValueError("TD3: env.action_space has %d components; the policy takes 1 .. %d" % (act_dim, _actor.MAX_ACT))
        if np.any(lo != lo[0]) or np.any(hi != hi[0]) or not np.isfinite(lo[0]) or not np.isfinite(hi[0]) or not lo[0] <= hi[0]:
            raise ValueError("TD3: env.action_space must be one finite scalar bound pair for all components")
        if obs_dim < 1 or obs_dim + act_dim > MAX_IN:
            raise ValueError("TD3: env.obs_dim + act_dim = %d + %d; a critic reads rows of at most %d" % (obs_dim, act_dim, MAX_IN))
        if not isinstance(twin, (bool, np.bool_)):
            raise ValueError("TD3: twin must be True or False, got %r" % (twin,))
        self.env = env
        self.batch, self.obs_dim, self.act_dim, self.tdtype, self.device = int(env.batch), obs_dim, act_dim, env.tdtype, torch.device(env.device)
        self.hidden, self.activation, self.low, self.high, self.twin = tuple(hid), activation, float(lo[0]), float(hi[0]), bool(twin)
        self.n_critics = 2 if twin else 1
        self.set_hyper(lr=lr, gamma=gamma, tau=tau, policy_delay=policy_delay, explore_noise=explore_noise, target_noise=target_noise,
                       noise_clip=noise_clip, betas=betas, eps=eps, max_grad_norm=max_grad_norm)
        self.cfg = make_cfg(self.batch, obs_dim, act_dim, 1 if self.tdtype == torch.float64 else 0, hid, activation, self.low, self.high, self.n_critics)
        self.lib = load()
        self.params_layout, nbytes = layout("params", self.cfg)
        self.params = torch.zeros((nbytes,), dtype=torch.uint8, device=self.device)
        self.target = torch.zeros((nbytes,), dtype=torch.uint8, device=self.device)
        self.shapes = {}
        for net, first, head in (("mu", obs_dim, act_dim), ("q1", obs_dim + act_dim, 1), ("q2", obs_dim + act_dim, 1))[:1 + self.n_critics]:
            dims = [first] + hid + [head]
            for l in range(len(hid) + 1):
                self.shapes["%s_w%d" % (net, l)] = (dims[l + 1], dims[l])
                self.shapes["%s_b%d" % (net, l)] = (dims[l + 1],)
        self.weights = {k: v.view(self.shapes[k]) for k, v in _views(self.params, self.params_layout, self.tdtype).items()}
        self.target_weights = {k: v.view(self.shapes[k]) for k, v in _views(self.target, self.params_layout, self.tdtype).items()}
        self.state_layout, nbytes = layout("state", self.cfg)
        self.state = torch.zeros((nbytes,), dtype=torch.uint8, device=self.device)
        v = _views(self.state, self.state_layout, self.tdtype)
        self.counters, self.step_count, self.stats, self.adam_m, self.adam_v = v["counters"], v["step"], v["stats"], v["adam_m"], v["adam_v"]
        self.actions = torch.zeros((self.batch, act_dim), dtype=self.tdtype, device=self.device)
        self.grid = int(self.lib.bcn_td3_grid(C.byref(self.cfg)))
        self._mems, self._plan, self._keep = weakref.WeakSet(), None, None
        if seed is None:
            seed = getattr(env, "seed", None) if isinstance(getattr(env, "seed", None), (int, np.integer)) else 0
        self.set_seed(seed, replica_offset)

    @classmethod
    def ddpg(cls, env, **kw):
        """DDPG (Lillicrap et al. 2016) as a preset: one critic, a policy step behind every critic step, no target smoothing."""
        return cls(env, **dict(kw, twin=False, policy_delay=1, target_noise=0.0))

    def set_hyper(self, **kw):
        """Check and set hyperparameters by name (those of the constructor).  ValueError names the field; nothing is set then."""
        new = {}
        for k, x in kw.items():
            if k in ("lr", "eps", "explore_noise", "target_noise", "noise_clip"):
                new[k] = _number("TD3", k, x, lo=0.0)
            elif k in ("gamma", "tau"):
                new[k] = _number("TD3", k, x, lo=0.0, hi=1.0, hi_closed=True)
            elif k == "policy_delay":
                new[k] = _count("TD3", k, x)
            elif k == "max_grad_norm":
                new[k] = 0.0 if x is None else _number("TD3", k, x)
            elif k == "betas":
                try:
                    b1, b2 = x
                except (TypeError, ValueError):
                    raise ValueError("TD3: betas must be a pair of numbers in [0, 1), got %r" % (x,))
                new[k] = (_number("TD3", "betas[0]", b1, lo=0.0, hi=1.0), _number("TD3", "betas[1]", b2, lo=0.0, hi=1.0))
            else:
                raise ValueError("TD3: unknown hyperparameter %r" % (k,))
        for k, x in new.items():
            setattr(self, k, x)
        return self

    def set_seed(self, seed, replica_offset=0):
        """Key all three streams (exploration, replay sampling, target smoothing) by `seed` with replica 0 at the global index
        `replica_offset`, and zero their counters: `counters`, step_count[2] and head[3] of every memory of this agent."""
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
            raise ValueError("TD3.set_seed: seed must be an integer in [0, 2^64), got %r" % (seed,))
        if isinstance(replica_offset, bool) or not isinstance(replica_offset, (int, np.integer)) or not 0 <= int(replica_offset) < 1 << 62:
            raise ValueError("TD3.set_seed: replica_offset must be a non-negative integer, got %r" % (replica_offset,))
        self.seed, self.replica_offset = int(seed), int(replica_offset)
        self.counters.zero_()
        self.step_count[2:3].zero_()
        for mem in self._mems:
            mem.head[3:4].zero_()
        return self

    # -- parameters -------------------------------------------------------------------------
    def load(self, mu, q1, q2=None):
        """Copy the networks into the parameter buffer AND the target buffer: mu, q1, q2 = [(W, b), ...] for the hidden layers and
        the head, W [out, in] (q*'s first matrix [hidden[0], obs_dim + act_dim], observation columns first).  q2 belongs to a twin
        agent.  ValueError for a wrong count or shape; nothing is written then."""
        nets = [("mu", mu), ("q1", q1)] + ([("q2", q2)] if self.twin else [])
        if not self.twin and q2 is not None:
            raise ValueError("TD3.load: q2 given, but this agent has one critic (twin=False)")
        todo = []
        for net, layers in nets:
            if layers is None or len(layers) != len(self.hidden) + 1:
                raise ValueError("TD3.load: %s must be %d (W, b) pairs" % (net, len(self.hidden) + 1))
            for l, (W, b) in enumerate(layers):
                W, b = torch.as_tensor(W), torch.as_tensor(b)
                want = self.shapes["%s_w%d" % (net, l)]
                if tuple(W.shape) != want or b.numel() != want[0]:
                    raise ValueError("TD3.load: %s[%d] must be W [%d, %d] and b [%d], got %s and %s"
                                     % (net, l, want[0], want[1], want[0], tuple(W.shape), tuple(b.shape)))
                todo += [("%s_w%d" % (net, l), W), ("%s_b%d" % (net, l), b.reshape(-1))]
        with torch.no_grad():
            for name, t in todo:
                self.weights[name].copy_(t.detach().to(device=self.device, dtype=self.tdtype))
        return self.sync_targets()

    def load_modules(self, mu, q1, q2=None):
        """load() from torch.nn.Sequential modules of Linear layers with this agent's activation between them (Tanh / ReLU); the
        squashing of mu's head is the library's and no part of the module."""
        import torch.nn as nn
        want = nn.Tanh if self.activation == "tanh" else nn.ReLU

        def pairs(what, m):
            if m is None:
                return None
            out = []
            for sub in m:
                if isinstance(sub, nn.Linear):
                    if sub.bias is None:
                        raise ValueError("TD3.load_modules: %s has a Linear without bias" % what)
                    out.append((sub.weight, sub.bias))
                elif not isinstance(sub, want):
                    raise ValueError("TD3.load_modules: %s holds a %s; expected Linear and %s only" % (what, type(sub).__name__, want.__name__))
            return out
        return self.load(pairs("mu", mu), pairs("q1", q1), pairs("q2", q2))

    def sync_targets(self):
        """target = params (one copy on the device)."""
        self.target.copy_(self.params)
        return self

    def state_dict(self):
        """For checkpoints: the three buffers on the CPU, what they were laid out for, seed, offset and hyperparameters."""
        return {"params": self.params.cpu(), "target": self.target.cpu(), "state": self.state.cpu(), "batch": self.batch, "obs_dim": self.obs_dim,
                "act_dim": self.act_dim, "dtype": "f64" if self.tdtype == torch.float64 else "f32", "hidden": self.hidden,
                "activation": self.activation, "n_critics": self.n_critics, "seed": self.seed, "replica_offset": self.replica_offset,
                "hyper": {k: getattr(self, k) for k in ("lr", "gamma", "tau", "policy_delay", "explore_noise", "target_noise", "noise_clip",
                                                        "betas", "eps", "max_grad_norm")}}

    def load_state_dict(self, d):
        keys = ("batch", "obs_dim", "act_dim", "dtype", "activation", "n_critics")
        cur = {"batch": self.batch, "obs_dim": self.obs_dim, "act_dim": self.act_dim, "dtype": "f64" if self.tdtype == torch.float64 else "f32",
               "activation": self.activation, "n_critics": self.n_critics}
        if (any(d.get(k) != cur[k] for k in keys) or tuple(d.get("hidden", ())) != self.hidden or d["params"].numel() != self.params.numel()
                or d["state"].numel() != self.state.numel()):
            raise ValueError("TD3.load_state_dict: the state is of another agent (%s, hidden %s); this one is %s, hidden %s"
                             % ({k: d.get(k) for k in keys}, tuple(d.get("hidden", ())), cur, self.hidden))
        self.set_hyper(**d["hyper"])
        self.params.copy_(d["params"])
        self.target.copy_(d["target"])
        self.state.copy_(d["state"])
        self.seed, self.replica_offset = int(d["seed"]), int(d["replica_offset"])
        return self

    # -- launches ---------------------------------------------------------------------------
    def _stream(self):
        if self.device.type != "cuda":
            raise RuntimeError("TD3: the launches need a ROCm device (no CPU fallback); this agent's env is on %s" % self.device)
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def act(self, obs=None, mask=None, mode="noisy"):
        """ONE launch on the current stream, no host synchronisation, nothing allocated: mu on `obs` ([B, obs_dim]; default: what the
        env's last reset() / step() returned -- env._norm.norm_obs while it normalises, else env.obs) into `actions`, which it
        returns.  mode: "deterministic" a = mu(s); "noisy" a = clamp(mu(s) + h explore_noise z, low, high); "uniform" a = low +
        (high - low) u, for warm-up steps (mu is not evaluated).  The stochastic modes tick the replicas' draw counters.  `mask`
        ([B] bool / uint8): replicas with 0 keep their action row and their counter."""
        if mode not in MODES:
            raise ValueError("TD3.act: mode must be 'deterministic', 'noisy' or 'uniform', got %r" % (mode,))
        env = self.env
        if obs is None:
            obs = env._norm.norm_obs if getattr(env, "_norm_on", False) else env.obs
        if (not torch.is_tensor(obs) or obs.dtype != self.tdtype or obs.device != self.device or not obs.is_contiguous() or obs.dim() != 2
                or tuple(obs.shape) != (self.batch, self.obs_dim)):
            raise ValueError("TD3.act: obs must be a contiguous %s tensor [%d, %d] on %s"
                             % ("f64" if self.tdtype == torch.float64 else "f32", self.batch, self.obs_dim, self.device))
        m = None
        if mask is not None:
            if not torch.is_tensor(mask):
                mask = torch.as_tensor(np.asarray(mask))
            if mask.numel() != self.batch:
                raise ValueError("TD3.act: mask must hold %d values" % self.batch)
            m = mask.to(device=self.device, dtype=torch.uint8).reshape(self.batch).contiguous()
        stream = self._stream()
        self._keep = (obs, m)                # alive behind the asynchronous launch
        _check(self.lib.bcn_td3_act(C.byref(self.cfg), _p(self.params), _p(obs), _p(m), _p(self.state), _p(self.actions), MODES[mode],
                                    self.explore_noise, self.seed, self.replica_offset, stream))
        return self.actions

    def replay(self, capacity):
        """A Replay of `capacity` transitions of this agent's env."""
        mem = Replay(self, capacity)
        self._mems.add(mem)
        return mem

    def plan(self, mem, n_updates, batch_size):
        """The update as a chain of the library's own launches, allocated once: a Plan (plan.run(), plan.capture())."""
        return Plan(self, mem, n_updates, batch_size)

    def update(self, mem, n_updates, batch_size):
        """n_updates minibatches of batch_size sampled rows of `mem` (the class docstring).  The plan -- idx and the work buffer --
        is allocated by the first call and reused while (mem, n_updates, batch_size) stay the same.  Returns self."""
        p = self._plan
        if p is None or p.mem is not mem or (p.n_updates, p.batch_size) != (n_updates, batch_size):
            p = self._plan = Plan(self, mem, n_updates, batch_size)
        p.run()
        return self

    def stats_dict(self):
        """The statistics of the last critic and policy steps as a dict of floats: the one host read."""
        return dict(zip(STATS, self.stats.cpu().tolist()))


class Plan(object):
    """n_updates TD3 minibatches over a Replay as a chain of launches (agent.plan(mem, n_updates, batch_size) makes one).  Owns `idx`
    int32 [batch_size] and `work` (bcn_td3_work_layout; `grads` maps the segment names to views of its gradient segment).
    run(): per minibatch k  sample -> critic_step(); and where (k + 1) % policy_delay == 0  policy_step().  The pieces are public:
    sample(), critic_grad(), adam(which), actor_grad(), polyak().  capture(): run() recorded as ONE graph; a replay draws new samples
    and new smoothing noise (their counters live on the device) with the hyperparameters of the time of the capture."""

    def __init__(self, agent, mem, n_updates, batch_size):
        if not isinstance(agent, TD3):
            raise ValueError("TD3.plan: agent must be a beacon_amd.TD3, got %r" % (type(agent).__name__,))
        if not isinstance(mem, Replay) or mem.agent is not agent:
            raise ValueError("TD3.plan: mem must be a Replay of this agent (agent.replay(capacity))")
        self.agent, self.mem = agent, mem
        self.n_updates, self.batch_size = _count("TD3.plan", "n_updates", n_updates), _count("TD3.plan", "batch_size", batch_size)
        if self.batch_size >= 1 << 31:
            raise ValueError("TD3.plan: batch_size = %d; a minibatch covers 2^31 - 1 rows" % self.batch_size)
        self.lib, self.device = agent.lib, agent.device
        self.idx = torch.zeros((self.batch_size,), dtype=torch.int32, device=self.device)
        self.work_layout, nbytes = layout("work", agent.cfg, self.batch_size)
        self.work = torch.zeros((nbytes,), dtype=torch.uint8, device=self.device)      # zeros: the slabs' gaps are read (header)
        v = _views(self.work, self.work_layout, agent.tdtype)
        self.grad = v["grad"]
        self.grads = {k: g.view(agent.shapes[k]) for k, g in _views(self.grad.view(torch.uint8), agent.params_layout, agent.tdtype).items()}
        self.xa, self.xb, self.rw = v["xa"], v["xb"], v["rw"]

    def _batch(self):
        a = self.agent
        return Td3Batch(params=_p(a.params), target=_p(a.target), mem=_p(self.mem.buf), idx=_p(self.idx), work=_p(self.work), state=_p(a.state),
                        m=self.batch_size, capacity=self.mem.capacity, gamma=a.gamma, target_noise=a.target_noise, noise_clip=a.noise_clip,
                        seed=a.seed)

    def sample(self):
        self.mem.sample(self.idx)
        return self

    def critic_grad(self):
        """Loss, statistics and gradient of the critics for the rows of `idx`: FOUR launches."""
        b = self._batch()
        _check(self.lib.bcn_td3_critic_grad(C.byref(self.agent.cfg), C.byref(b), self.agent._stream()))
        return self

    def actor_grad(self):
        """Loss and gradient of the policy through Q_1 for the rows of `idx` (behind critic_grad() of the same rows): FOUR launches."""
        b = self._batch()
        _check(self.lib.bcn_td3_actor_grad(C.byref(self.agent.cfg), C.byref(b), self.agent._stream()))
        return self

    def adam(self, which):
        """One Adam step of the critic (OPT_CRITIC) or the policy (OPT_POLICY) segments from the gradient buffer: TWO launches."""
        a = self.agent
        h = Td3Adam(lr=a.lr, beta1=a.betas[0], beta2=a.betas[1], eps=a.eps, max_grad_norm=a.max_grad_norm)
        _check(self.lib.bcn_td3_adam(C.byref(a.cfg), _p(a.params), _p(self.work), _p(a.state), int(which), C.byref(h), a._stream()))
        return self

    def polyak(self):
        """target += tau (params - target) over the whole buffer: ONE launch."""
        a = self.agent
        _check(self.lib.bcn_td3_polyak(C.byref(a.cfg), _p(a.params), _p(a.target), a.tau, a._stream()))
        return self

    def critic_step(self):
        return self.critic_grad().adam(OPT_CRITIC)

    def policy_step(self):
        return self.actor_grad().adam(OPT_POLICY).polyak()

    def run(self):
        """The update.  No host synchronisation, nothing allocated.  Returns self."""
        self.agent._stream()
        delay = self.agent.policy_delay
        for k in range(self.n_updates):
            self.sample().critic_step()
            if (k + 1) % delay == 0:
                self.policy_step()
        return self

    def capture(self):
        """run() recorded as ONE graph; nothing is launched.  Returns the torch.cuda.CUDAGraph."""
        self.agent._stream()
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize(self.device)
        with torch.cuda.graph(g):
            self.run()
        return g
