"""The on-device actor of a rollout: libbeacon_actor.so (include/beacon_actor.h; csrc/actor/) and the class Actor over it.

ONE launch reads the observation rows the last reset() / step() left, evaluates a policy MLP and a value MLP, draws the action
from the project's Philox stream and writes action, log-probability and value -- under a rollout also into the slot the
rollout's device cursor names -- so that `act -> step_autoreset -> (normalise) -> record` is a chain of the library's own
launches that a caller captures in one graph, and Rollout.compute_gae gets its values without a framework forward pass.

The library is a unit of its own, like the torch extension: its entry points take no env handle, only device pointers and
sizes; they are bound here through ctypes in a table of their own (SIGNATURES below -- not _lib.SIGNATURES).  Built in-tree
with the flags of the main library (build.FLAGS) on first use; the sidecar .sig holds a hash of its sources, the headers they
include and the flags (build.py: the machinery, shared with every library of the package).  Importing this module touches neither a compiler nor the GPU."""
import ctypes as C
import os

import numpy as np
import torch

from . import build as _build

API_VERSION = 1                           # include/beacon_actor.h: BCN_ACTOR_API_VERSION
# per-file flags, as build.FILE_FLAGS.  The float64 unit: one rounding per written operation, for the same reason as rollout.hip
# (its NumPy restatement is the same sequence); the float32 unit may contract (its sums are explicit fma chains either way).
FILE_FLAGS = {"actor.hip": [],
              "actor_f64.hip": ["-ffp-contract=off"]}

TANH, RELU = 0, 1
GAUSSIAN, CATEGORICAL = 0, 1
MAX_OBS, MAX_HIDDEN, MAX_LAYERS, MAX_ACT, MAX_SEGS = 512, 128, 3, 16, 20
_ACTIVATIONS = {"tanh": TANH, "relu": RELU}
_vp = C.c_void_p


class ActorCfg(C.Structure):
    """bcn_actor_cfg"""
    _fields_ = [("batch", C.c_int32), ("obs_dim", C.c_int32), ("dtype", C.c_int32), ("n_hidden", C.c_int32), ("hidden", C.c_int32 * 3),
                ("activation", C.c_int32), ("kind", C.c_int32), ("act_dim", C.c_int32), ("low", C.c_double), ("high", C.c_double),
                ("agents", C.c_int32)]          # appended: rows per replica, 0 means 1


class ActorSeg(C.Structure):
    """bcn_actor_seg: one named segment, [planes][rows][row_elems] elements at `offset` bytes (planes = 0: row_elems elements)."""
    _fields_ = [("name", C.c_char * 16), ("offset", C.c_uint64), ("elem", C.c_int32), ("planes", C.c_int32), ("row_elems", C.c_int64)]


_cfgp, _segp = C.POINTER(ActorCfg), C.POINTER(ActorSeg)
# every symbol include/beacon_actor.h declares: (restype, argtypes)
SIGNATURES = {
    "bcn_actor_params_layout": (C.c_int, [_cfgp, _segp, C.c_int]),
    "bcn_actor_params_bytes": (C.c_size_t, [_cfgp]),
    "bcn_actor_state_layout": (C.c_int, [_cfgp, _segp, C.c_int]),
    "bcn_actor_state_bytes": (C.c_size_t, [_cfgp]),
    "bcn_actor_seq_layout": (C.c_int, [_cfgp, C.c_int, _segp, C.c_int]),
    "bcn_actor_seq_bytes": (C.c_size_t, [_cfgp, C.c_int]),
    "bcn_actor_act": (C.c_int, [_cfgp, _vp, _vp, _vp, _vp, C.c_uint64, C.c_int64, C.c_int, _vp, C.c_int, _vp, _vp]),
    "bcn_actor_values": (C.c_int, [_cfgp, _vp, _vp, C.c_int64, _vp, _vp]),
    "bcn_actor_last_error": (C.c_char_p, []),
}


class BeaconActorError(RuntimeError):
    pass


# ---- the library -------------------------------------------------------------------------
SRC_DIR, HEADER = os.path.join(_build.CSRC, "actor"), os.path.join(_build.INC, "beacon_actor.h")
LIB, OBJ = os.path.join(_build.PKG, "libbeacon_actor.so"), os.path.join(_build.OBJ, "actor")
_UNIT = _build.hip_library(LIB, SRC_DIR, FILE_FLAGS, OBJ, SIGNATURES)
sources, signature, stale, load = _UNIT.sources, _UNIT.signature, _UNIT.stale, _UNIT.load


def build_actor(force=False, verbose=False):
    """Compile csrc/actor/*.hip for gfx950 and link libbeacon_actor.so.  Returns its path."""
    return _UNIT.build(force=force, verbose=verbose)


def _check(rc):
    if rc != 0:
        raise BeaconActorError("libbeacon_actor: error %d: %s" % (rc, load().bcn_actor_last_error().decode()))


def make_cfg(batch, obs_dim, dtype, hidden, activation, kind, act_dim, low=-1.0, high=1.0, agents=1):
    """bcn_actor_cfg from plain values (dtype: 0 / 1; activation: "tanh" / "relu" or 0 / 1; agents: rows per replica, with
    `batch` the number of rows).  No range check: the library's."""
    hid = [int(h) for h in hidden]
    return ActorCfg(batch=int(batch), obs_dim=int(obs_dim), dtype=int(dtype), n_hidden=len(hid), hidden=(C.c_int32 * 3)(*(hid + [0] * 3)[:3]),
                    activation=_ACTIVATIONS.get(activation, activation), kind=int(kind), act_dim=int(act_dim), low=float(low), high=float(high),
                    agents=int(agents))


def layout(which, cfg, T=None):
    """([segment dicts], bytes) of the "params", "state" or "seq" (with T) buffer of `cfg`; BeaconActorError with the library's text
    for a cfg it refuses.  No device needed."""
    L = load()
    segs = (ActorSeg * MAX_SEGS)()
    extra = () if which != "seq" else (int(T),)
    k = getattr(L, "bcn_actor_%s_layout" % which)(C.byref(cfg), *(extra + (segs, MAX_SEGS)))
    nbytes = getattr(L, "bcn_actor_%s_bytes" % which)(C.byref(cfg), *extra)
    if k == 0 or nbytes == 0:
        raise BeaconActorError("libbeacon_actor: %s" % L.bcn_actor_last_error().decode())
    return ([dict(name=g.name.decode(), offset=int(g.offset), elem=int(g.elem), planes=int(g.planes), row_elems=int(g.row_elems))
             for g in segs[:k]], int(nbytes))


_ELEM = {1: torch.int32, 2: torch.int32}     # BCN_ACTOR_I32, BCN_ACTOR_U32 (the counters' bits as int32); 0: the env dtype


def _views(buf, segs, rows, real, shapes):
    """{name: typed no-copy view} of every segment; `shapes`: name -> the view's shape (default: flat)."""
    out = {}
    for s in segs:
        dt = _ELEM.get(s["elem"], real)
        n = (s["planes"] * rows if s["planes"] else 1) * s["row_elems"]
        v = buf[s["offset"]:s["offset"] + n * torch.empty((), dtype=dt).element_size()].view(dt)
        out[s["name"]] = v.view(shapes[s["name"]]) if s["name"] in shapes else v
    return out


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ---- the class ---------------------------------------------------------------------------
class Actor(object):
    """A policy MLP and a value MLP of one VecEnv, evaluated and sampled on the device in ONE launch (include/beacon_actor.h states
    the arithmetic and the random stream; csrc/actor/actor_impl.h is the kernel).

        actor = Actor(env, hidden=(64, 64)); actor.load_modules(pi, vf); ro = env.rollout(T); actor.attach(ro); ro.begin()
        for _ in range(T):
            env.step_autoreset(actor.act())
        adv, ret = ro.compute_gae(actor.value_seq, actor.values(env.obs), actor.values(ro.final_obs.view(-1, env.obs_dim)))

    Kind, act_dim and bounds come from env.action_space / env.action_is_int (a Box gives a diagonal Gaussian with a
    state-independent log_std, clipped to the Box; a Discrete(n) gives a categorical policy); obs_dim, batch, dtype and device come
    from the env.  `hidden`: 1 .. 3 widths of 1 .. 128, the same for both networks; `activation`: "tanh" or "relu".  `seed`
    defaults to the env's noise seed where it has one (the actor's Philox counters differ from the noise's in their last word, so
    the seed may be shared), else 0; `replica_offset`: the global index of replica 0 (sharded batches).
    Owns `params` (one uint8 buffer in the layout of bcn_actor_params_layout; `weights` maps the segment names -- pi_w0, pi_b0, ...
    vf_w0, ... log_std -- to typed views, matrices [out, in]) and `state` (bcn_actor_state_layout) with the views
      counters int32 [B] (the uint32 draw counters' bits), actions [B, act_dim] (or int32 [B]), raw [B, act_dim], logp [B],
      value [B], dist [B, act_dim]
    and, once attach()ed to a Rollout of T steps, `seq` with logp_seq [T, B], value_seq [T, B], raw_seq [T, B, act_dim].
    Fresh parameters are zero (log_std too): load() / load_modules() / load_state_dict() fill them.

    per_jet=True (a VecShkadov: n_jets, n_obs, a Box of n_jets components): every jet is an agent of the ONE policy, the mode of the
    reference's shkadov_separable.  A = n_jets, obs_dim = n_obs, act_dim = 1, a row per (replica, jet): row b A + j is jet j of
    replica b, with its own draw, log-probability, value and counter -- bit for bit what a plain actor computes for a batch of
    B A rows [B A, n_obs] with replica_offset A in place of replica_offset.  A is not limited by the 16 action components.

        env = VecShkadov(B, n_jets=5); env.set_jet_rewards()
        actor = Actor(env, hidden=(64, 64), per_jet=True); ro = env.rollout(T); actor.attach(ro); env.reset(); ro.begin()
        for _ in range(T):
            env.step_autoreset(actor.act())
        adv, ret = ro.compute_gae(actor.value_seq, actor.values(env.obs.view(-1, env.n_obs)),
                                  actor.values(ro.final_obs.view(-1, env.n_obs)), per_jet=True)

    Then counters, actions, raw, logp, value and dist are all [B, A], logp_seq and value_seq [T, B A] (what compute_gae(per_jet=True)
    takes), raw_seq [T, B A, 1]; the mask of act() and the rollout's `valid` stay per replica, and the kernels index them by
    row / A.  Observation normalisation keeps its per-column statistics; rwd_jets stays raw."""

    def __init__(self, env, hidden=(64, 64), activation="tanh", seed=None, replica_offset=0, per_jet=False):
        try:
            hid = [int(h) for h in hidden]
            ok = all(int(h) == h and not isinstance(h, bool) for h in hidden)
        except (TypeError, ValueError):
            hid, ok = [], False
        if not ok or not 1 <= len(hid) <= MAX_LAYERS or any(not 1 <= h <= MAX_HIDDEN for h in hid):
            raise ValueError("Actor: hidden must be 1 .. %d integer widths of 1 .. %d, got %r" % (MAX_LAYERS, MAX_HIDDEN, hidden))
        if activation not in _ACTIVATIONS:
            raise ValueError("Actor: activation must be 'tanh' or 'relu', got %r" % (activation,))
        space = getattr(env, "action_space", None)
        if space is None:
            raise ValueError("Actor: env has no action_space")
        agents, obs_dim = 1, int(env.obs_dim)
        if per_jet:
            # every jet is an agent of the one policy: a row per (replica, jet), n_obs observations in, one action component out
            lo = hi = None
            if not getattr(env, "action_is_int", False) and hasattr(space, "low") and hasattr(space, "high"):
                lo, hi = np.asarray(space.low, dtype=np.float64).reshape(-1), np.asarray(space.high, dtype=np.float64).reshape(-1)
            nj, no = getattr(env, "n_jets", None), getattr(env, "n_obs", None)
            if (lo is None or not all(isinstance(x, (int, np.integer)) and not isinstance(x, bool) and x >= 1 for x in (nj, no))
                    or lo.size != nj or hi.size != nj or np.any(lo != lo[0]) or np.any(hi != hi[0]) or int(env.obs_dim) != nj * no):
                raise ValueError("Actor: per_jet=True needs an env with n_jets, n_obs (obs_dim = n_jets n_obs) and a Box action space of "
                                 "n_jets components with one bound pair -- a VecShkadov")
            kind, act_dim, low, high, agents, obs_dim = GAUSSIAN, 1, float(lo[0]), float(hi[0]), int(nj), int(no)
        elif getattr(env, "action_is_int", False):
            kind, act_dim, low, high = CATEGORICAL, int(space.n), 0.0, 0.0
            if not 2 <= act_dim <= MAX_ACT:
                raise ValueError("Actor: env.action_space has %d classes; a categorical actor takes 2 .. %d" % (act_dim, MAX_ACT))
        else:
            lo, hi = np.asarray(space.low, dtype=np.float64).reshape(-1), np.asarray(space.high, dtype=np.float64).reshape(-1)
            kind, act_dim = GAUSSIAN, int(lo.size)
            if not 1 <= act_dim <= MAX_ACT:
                raise ValueError("Actor: env.action_space has %d components; a Gaussian actor takes 1 .. %d" % (act_dim, MAX_ACT))
            if np.any(lo != lo[0]) or np.any(hi != hi[0]):
                raise ValueError("Actor: env.action_space must be one scalar bound pair for all components")
            low, high = float(lo[0]), float(hi[0])
        if not 1 <= obs_dim <= MAX_OBS:
            raise ValueError("Actor: %s = %d; an actor reads 1 .. %d observations per %s"
                             % ("env.n_obs" if per_jet else "env.obs_dim", obs_dim, MAX_OBS, "jet" if per_jet else "replica"))
        self.env = env
        self.batch, self.obs_dim, self.tdtype, self.device = int(env.batch), obs_dim, env.tdtype, torch.device(env.device)
        self.per_jet, self.agents, self.rows = bool(per_jet), agents, int(env.batch) * agents      # rows: what the library calls batch
        if per_jet and self.rows >= 1 << 31:
            raise ValueError("Actor: %d replicas of %d jets are %d rows; one launch covers 2^31 - 1" % (self.batch, agents, self.rows))
        self.hidden, self.activation, self.kind, self.act_dim, self.low, self.high = tuple(hid), activation, kind, act_dim, low, high
        self.cfg = make_cfg(self.rows, self.obs_dim, 1 if self.tdtype == torch.float64 else 0, hid, activation, kind, act_dim, low, high, agents)
        self.lib = load()
        self.params_layout, nbytes = layout("params", self.cfg)
        self.params = torch.zeros((nbytes,), dtype=torch.uint8, device=self.device)
        dims = [self.obs_dim] + hid
        shapes = {}
        for net, head in (("pi", act_dim), ("vf", 1)):
            for l in range(len(hid) + 1):
                shapes["%s_w%d" % (net, l)] = (dims[l + 1] if l < len(hid) else head, dims[l])
        self.weights = _views(self.params, self.params_layout, 1, self.tdtype, shapes)
        self.state_layout, nbytes = layout("state", self.cfg)
        self.state = torch.zeros((nbytes,), dtype=torch.uint8, device=self.device)
        B, n = self.batch, act_dim
        if per_jet:                                  # a row per (replica, jet), one element each: every view is [B, n_jets]
            shapes = {k: (B, agents) for k in ("counters", "actions", "raw", "logp", "value", "dist")}
        else:
            shapes = {"raw": (B, n), "dist": (B, n), **({} if kind == CATEGORICAL else {"actions": (B, n)})}
        v = _views(self.state, self.state_layout, self.rows, self.tdtype, shapes)
        self.counters, self.actions, self.raw, self.logp, self.value, self.dist = (v[k] for k in ("counters", "actions", "raw", "logp", "value", "dist"))
        self.rollout, self.seq, self.T = None, None, 0
        self.logp_seq = self.value_seq = self.raw_seq = None
        if seed is None:
            seed = getattr(env, "seed", None) if isinstance(getattr(env, "seed", None), (int, np.integer)) else 0
        self.set_seed(seed, replica_offset)

    # -- parameters -------------------------------------------------------------------------
    def _layers(self, what, layers, net, head):
        dims = [self.obs_dim] + list(self.hidden) + [head]
        if layers is None or len(layers) != len(dims) - 1:
            raise ValueError("Actor.load: %s must be %d (W, b) pairs" % (what, len(dims) - 1))
        out = []
        for l, (W, b) in enumerate(layers):
            W, b = torch.as_tensor(W), torch.as_tensor(b)
            if tuple(W.shape) != (dims[l + 1], dims[l]) or b.numel() != dims[l + 1]:
                raise ValueError("Actor.load: %s[%d] must be W [%d, %d] and b [%d], got %s and %s"
                                 % (what, l, dims[l + 1], dims[l], dims[l + 1], tuple(W.shape), tuple(b.shape)))
            out += [("%s_w%d" % (net, l), W), ("%s_b%d" % (net, l), b.reshape(-1))]
        return out

    def load(self, pi, vf, log_std=None):
        """Copy both networks into the parameter buffer: pi, vf = [(W, b), ...] for the hidden layers and the head, W [out, in] as
        the framework's Linear.weight (tensors or arrays on any device, any float dtype); log_std [act_dim] (Gaussian kind; None
        keeps what is there).  ValueError for a wrong count or shape; nothing is written then."""
        todo = self._layers("pi", pi, "pi", self.act_dim) + self._layers("vf", vf, "vf", 1)
        if log_std is not None:
            ls = torch.as_tensor(log_std)
            if self.kind != GAUSSIAN or ls.numel() != self.act_dim:
                raise ValueError("Actor.load: log_std must hold %d values and belongs to a Gaussian actor" % self.act_dim)
            todo.append(("log_std", ls.reshape(-1)))
        with torch.no_grad():
            for name, t in todo:
                self.weights[name].copy_(t.detach().to(device=self.device, dtype=self.tdtype))
        return self

    def load_modules(self, pi_module, vf_module, log_std=None):
        """load() from two torch.nn.Sequential of Linear layers with this actor's activation between them (Tanh / ReLU)."""
        import torch.nn as nn
        want = nn.Tanh if self.activation == "tanh" else nn.ReLU

        def pairs(what, m):
            out = []
            for sub in m:
                if isinstance(sub, nn.Linear):
                    if sub.bias is None:
                        raise ValueError("Actor.load_modules: %s has a Linear without bias" % what)
                    out.append((sub.weight, sub.bias))
                elif not isinstance(sub, want):
                    raise ValueError("Actor.load_modules: %s holds a %s; expected Linear and %s only" % (what, type(sub).__name__, want.__name__))
            return out
        return self.load(pairs("pi_module", pi_module), pairs("vf_module", vf_module), log_std)

    def state_dict(self):
        """For checkpoints: both buffers on the CPU, what they were laid out for (`agents`: the rows per replica, 1 for a plain
        actor), seed and replica offset."""
        return {"params": self.params.cpu(), "state": self.state.cpu(), "batch": self.batch, "obs_dim": self.obs_dim,
                "dtype": "f64" if self.tdtype == torch.float64 else "f32", "hidden": self.hidden, "activation": self.activation,
                "kind": self.kind, "act_dim": self.act_dim, "seed": self.seed, "replica_offset": self.replica_offset, "agents": self.agents}

    def load_state_dict(self, d):
        keys = ("batch", "obs_dim", "dtype", "activation", "kind", "act_dim", "agents")
        cur = {"batch": self.batch, "obs_dim": self.obs_dim, "dtype": "f64" if self.tdtype == torch.float64 else "f32",
               "activation": self.activation, "kind": self.kind, "act_dim": self.act_dim, "agents": self.agents}
        d = dict(d, agents=d.get("agents", 1))       # a state written before there were agents is of a plain actor
        if (any(d[k] != cur[k] for k in keys) or tuple(d["hidden"]) != self.hidden or d["params"].numel() != self.params.numel()
                or d["state"].numel() != self.state.numel()):
            raise ValueError("Actor.load_state_dict: the state is of another actor (%s, hidden %s); this one is %s, hidden %s"
                             % ({k: d[k] for k in keys}, tuple(d["hidden"]), cur, self.hidden))
        self.params.copy_(d["params"])
        self.state.copy_(d["state"])
        self.seed, self.replica_offset = int(d["seed"]), int(d["replica_offset"])
        return self

    def set_seed(self, seed, replica_offset=0):
        """Key the sampling stream by `seed` (0 <= seed < 2^64) with replica 0 at the global index `replica_offset`, and zero the draw
        counters.  Both are ARGUMENTS of the launch: a captured graph keeps the values it was recorded with."""
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
            raise ValueError("Actor.set_seed: seed must be an integer in [0, 2^64), got %r" % (seed,))
        if isinstance(replica_offset, bool) or not isinstance(replica_offset, (int, np.integer)) or not 0 <= int(replica_offset) < 1 << 62:
            raise ValueError("Actor.set_seed: replica_offset must be a non-negative integer, got %r" % (replica_offset,))
        self.seed, self.replica_offset = int(seed), int(replica_offset)
        self.counters.zero_()
        return self

    # -- launches ---------------------------------------------------------------------------
    def _stream(self):
        if self.device.type != "cuda":
            raise RuntimeError("Actor: the launches need a ROCm device (no CPU fallback); this actor's env is on %s" % self.device)
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _rows(self, name, t, rows):
        if (not torch.is_tensor(t) or t.dtype != self.tdtype or t.device != self.device or not t.is_contiguous() or t.dim() != 2
                or t.shape[1] != self.obs_dim or t.shape[0] != (rows if rows is not None else max(int(t.shape[0]), 1))):
            raise ValueError("Actor: %s must be a contiguous %s tensor [%s, %d] on %s"
                             % (name, "f64" if self.tdtype == torch.float64 else "f32", rows if rows is not None else "n", self.obs_dim, self.device))
        return t

    def act(self, obs=None, mask=None, deterministic=False):
        """ONE launch on the current stream, no host synchronisation, nothing allocated: both networks on `obs` ([B, obs_dim];
        default: what the env's last reset() / step() returned -- env._norm.norm_obs while it normalises, else env.obs), the draw
        (deterministic=True: the mean / the first most probable class, no draw, no counter tick), the outputs into `state` and,
        with a rollout attached, into the slot its device cursor names.  `mask` ([B] bool / uint8): replicas with 0 keep their
        output rows and counters.  Returns `actions`: what env.step() / step_autoreset() take.
        per_jet: `obs` is [B, n_jets n_obs] or [B n_jets, n_obs] (the same bytes); `mask` stays [B], and a replica with 0 keeps
        all of its jets' rows and counters; `actions` is [B, n_jets]."""
        env = self.env
        if obs is None:
            obs = env._norm.norm_obs if getattr(env, "_norm_on", False) else env.obs
        if self.per_jet:
            # the row is jet-major: [B, n_jets n_obs] IS [B n_jets, n_obs], the same bytes
            if (not torch.is_tensor(obs) or obs.dtype != self.tdtype or obs.device != self.device or not obs.is_contiguous() or obs.dim() != 2
                    or tuple(obs.shape) not in ((self.batch, self.agents * self.obs_dim), (self.rows, self.obs_dim))):
                raise ValueError("Actor: obs must be a contiguous %s tensor [%d, %d] or [%d, %d] on %s"
                                 % ("f64" if self.tdtype == torch.float64 else "f32", self.batch, self.agents * self.obs_dim, self.rows,
                                    self.obs_dim, self.device))
        else:
            self._rows("obs", obs, self.batch)
        m = None
        if mask is not None:
            if not torch.is_tensor(mask):
                mask = torch.as_tensor(np.asarray(mask))
            if mask.numel() != self.batch:
                raise ValueError("Actor.act: mask must hold %d values" % self.batch)
            m = mask.to(device=self.device, dtype=torch.uint8).reshape(self.batch).contiguous()
        self._keep = (obs, m)                # alive behind the asynchronous launch
        ro = self.rollout
        _check(self.lib.bcn_actor_act(C.byref(self.cfg), _ptr(self.params), _ptr(obs), _ptr(self.state), _ptr(m), self.seed, self.replica_offset,
                                      1 if deterministic else 0, None if ro is None else _ptr(ro.cursor), self.T, _ptr(self.seq), self._stream()))
        return self.actions

    def values(self, obs_rows, out=None):
        """The value network alone on any number of rows, ONE launch: obs_rows [n, obs_dim] -> [n] (`out`, or a new tensor).  The
        same arithmetic as in act(): bit for bit the `value` it writes for the same row.  For the last_value and final_values of
        Rollout.compute_gae."""
        self._rows("obs_rows", obs_rows, None)
        n = int(obs_rows.shape[0])
        if out is None:
            out = torch.empty((n,), dtype=self.tdtype, device=self.device)
        elif (not torch.is_tensor(out) or out.dtype != self.tdtype or out.device != self.device or out.numel() != n or not out.is_contiguous()):
            raise ValueError("Actor.values: out must be a contiguous tensor of %d elements of the env dtype on %s" % (n, self.device))
        _check(self.lib.bcn_actor_values(C.byref(self.cfg), _ptr(self.params), _ptr(obs_rows), n, _ptr(out), self._stream()))
        return out

    def attach(self, rollout):
        """Allocate logp_seq / value_seq [T, B] and raw_seq [T, B, act_dim] for `rollout` (a Rollout of this actor's env; None:
        detach) and make every later act() pass its device cursor: the act of step t -- launched BEFORE the step, whose record
        advances the cursor -- writes row t; with the rollout full it writes no slot.  Returns self."""
        if rollout is None:
            self.rollout, self.T = None, 0
            return self
        if (not hasattr(rollout, "cursor") or int(getattr(rollout, "batch", -1)) != self.batch or rollout.buf.device != self.device):
            raise ValueError("Actor.attach: rollout must be a Rollout of %d replicas on %s" % (self.batch, self.device))
        T = int(rollout.T)
        cfg_layout, nbytes = layout("seq", self.cfg, T)
        if self.seq is None or self.seq.numel() != nbytes:
            self.seq = torch.zeros((nbytes,), dtype=torch.uint8, device=self.device)
        B, n = self.rows, self.act_dim               # per_jet: B n_jets columns, the shape Rollout.compute_gae(per_jet=True) takes
        v = _views(self.seq, cfg_layout, B, self.tdtype, {"logp_seq": (T, B), "value_seq": (T, B), "raw_seq": (T, B, n)})
        self.seq_layout, self.logp_seq, self.value_seq, self.raw_seq = cfg_layout, v["logp_seq"], v["value_seq"], v["raw_seq"]
        self.rollout, self.T = rollout, T
        return self
