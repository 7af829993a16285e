"""Value-based learning for the discrete envs on the device: libbeacon_dqn.so (include/beacon_dqn.h; csrc/dqn/) and the class DQN over it.

A DQN is ONE Q network with one output per action (optionally a dueling head: n advantage rows and a value row in one matrix), its
target, and one Adam optimiser.  It trains over the same Replay as TD3 and SAC (beacon_amd.td3.Replay, laid out and sampled through
libbeacon_td3.so with act_dim = 1: the ring's act segment holds the action index; this library receives the memory's segments as plain
device pointers, and brings the append that reads int32 rollout actions).  Acting is ONE launch that writes the int32 [B] actions the
discrete envs take; one minibatch -- sample (2 launches), gradient (3: the two target passes, the online pass, loss, backward pass
in one kernel; reduce; finish), Adam (2), Polyak (1) -- is 8 launches, 7 without the target step: no host read, no allocation, no
atomics, every sum in a fixed order, bit-reproducible, and capturable as ONE graph whose replays draw new samples (the counters live
on the device).  tests/dqn_ref.py restates it on the host.

The library is a unit of its own, built and bound like the other six (build.py: one Unit each); its table is SIGNATURES below.
Importing this module touches neither a compiler nor the GPU."""
import ctypes as C
import os
import weakref

import numpy as np
import torch

from . import actor as _actor
from . import build as _build
from . import td3 as _td3
from .td3 import Replay, _count, _number, _p, _views

API_VERSION = 1                           # include/beacon_dqn.h: BCN_DQN_API_VERSION
# the float64 unit: one rounding per written operation, as td3_f64.hip
FILE_FLAGS = {"dqn.hip": [],
              "dqn_f64.hip": ["-ffp-contract=off"]}
REAL, I32, U32, F64, U8 = 0, 1, 2, 3, 4   # BCN_DQN_REAL ...
GREEDY, EPSILON, UNIFORM = 0, 1, 2
MODES = {"greedy": GREEDY, "epsilon": EPSILON, "uniform": UNIFORM}
MAX_OBS, MAX_ACTIONS, MAX_GRID, MAX_SEGS, LDS_LIMIT = 512, 16, 128, 16, 163840
STATS = ("loss", "q_mean", "target_mean", "td_abs_mean", "W", "grad_norm", "q_max_mean", "spare")
_vp = C.c_void_p


class DqnCfg(C.Structure):
    """bcn_dqn_cfg"""
    _fields_ = [("batch", C.c_int32), ("obs_dim", C.c_int32), ("n_actions", C.c_int32), ("dtype", C.c_int32), ("n_hidden", C.c_int32),
                ("hidden", C.c_int32 * 3), ("activation", C.c_int32), ("dueling", C.c_int32)]


class DqnSeg(C.Structure):
    """bcn_dqn_seg"""
    _fields_ = [("name", C.c_char * 16), ("offset", C.c_uint64), ("elem", C.c_int32), ("planes", C.c_int32), ("row_elems", C.c_int64)]


class DqnBatch(C.Structure):
    """bcn_dqn_batch"""
    _fields_ = [("params", _vp), ("target", _vp), ("obs", _vp), ("act", _vp), ("rwd", _vp), ("next_obs", _vp), ("boot", _vp), ("live", _vp),
                ("idx", _vp), ("work", _vp), ("state", _vp), ("m", C.c_int64), ("capacity", C.c_int64), ("gamma", C.c_double),
                ("huber", C.c_double), ("double_q", C.c_int32), ("reserved", C.c_int32)]


class DqnAdam(C.Structure):
    """bcn_dqn_adam_hyper"""
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("max_grad_norm", C.c_double)]


_cfgp, _segp, _batchp = C.POINTER(DqnCfg), C.POINTER(DqnSeg), C.POINTER(DqnBatch)
# every symbol include/beacon_dqn.h declares: (restype, argtypes)
SIGNATURES = {
    "bcn_dqn_params_layout": (C.c_int, [_cfgp, _segp, C.c_int]),
    "bcn_dqn_params_bytes": (C.c_size_t, [_cfgp]),
    "bcn_dqn_state_layout": (C.c_int, [_cfgp, _segp, C.c_int]),
    "bcn_dqn_state_bytes": (C.c_size_t, [_cfgp]),
    "bcn_dqn_work_layout": (C.c_int, [_cfgp, _segp, C.c_int]),
    "bcn_dqn_work_bytes": (C.c_size_t, [_cfgp]),
    "bcn_dqn_grid": (C.c_int, [_cfgp]),
    "bcn_dqn_lds_bytes": (C.c_size_t, [_cfgp]),
    "bcn_dqn_act": (C.c_int, [_cfgp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_double, _vp, C.c_uint64, C.c_int64, _vp]),
    "bcn_dqn_q": (C.c_int, [_cfgp, _vp, _vp, C.c_int64, _vp, _vp]),
    "bcn_dqn_append": (C.c_int, [_cfgp, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "bcn_dqn_grad": (C.c_int, [_cfgp, _batchp, _vp]),
    "bcn_dqn_adam": (C.c_int, [_cfgp, _vp, _vp, _vp, C.POINTER(DqnAdam), _vp]),
    "bcn_dqn_polyak": (C.c_int, [_cfgp, _vp, _vp, C.c_double, _vp]),
    "bcn_dqn_last_error": (C.c_char_p, []),
}


class BeaconDqnError(RuntimeError):
    pass


# ---- the library -------------------------------------------------------------------------
# (the units include csrc/td3/td3_impl.h and, through it, the network of csrc/actor/policy_net.h: the dependency rule of build.py
# follows the #include lines there)
SRC_DIR, HEADER = os.path.join(_build.CSRC, "dqn"), os.path.join(_build.INC, "beacon_dqn.h")
LIB, OBJ = os.path.join(_build.PKG, "libbeacon_dqn.so"), os.path.join(_build.OBJ, "dqn")
_UNIT = _build.hip_library(LIB, SRC_DIR, FILE_FLAGS, OBJ, SIGNATURES)
sources, signature, stale, load = _UNIT.sources, _UNIT.signature, _UNIT.stale, _UNIT.load


def build_dqn(force=False, verbose=False):
    """Compile csrc/dqn/*.hip for gfx950 and link libbeacon_dqn.so.  Returns its path."""
    return _UNIT.build(force=force, verbose=verbose)


def _check(rc):
    if rc != 0:
        raise BeaconDqnError("libbeacon_dqn: error %d: %s" % (rc, load().bcn_dqn_last_error().decode()))


def make_cfg(batch, obs_dim, n_actions, dtype, hidden, activation, dueling=False):
    """bcn_dqn_cfg from plain values (dtype: 0 / 1; activation: "tanh" / "relu" or 0 / 1).  No range check: the library's."""
    hid = [int(h) for h in hidden]
    return DqnCfg(batch=int(batch), obs_dim=int(obs_dim), n_actions=int(n_actions), dtype=int(dtype), n_hidden=len(hid),
                  hidden=(C.c_int32 * 3)(*(hid + [0] * 3)[:3]), activation=_actor._ACTIVATIONS.get(activation, activation),
                  dueling=int(dueling))


def layout(which, cfg):
    """([segment dicts], bytes) of the "params", "state" or "work" buffer of `cfg`; BeaconDqnError with the library's text for what
    it refuses.  No device needed.  (The replay memory's layout is beacon_amd.td3.layout("replay", ...).)"""
    L = load()
    segs = (DqnSeg * MAX_SEGS)()
    k = getattr(L, "bcn_dqn_%s_layout" % which)(C.byref(cfg), segs, MAX_SEGS)
    nbytes = getattr(L, "bcn_dqn_%s_bytes" % which)(C.byref(cfg))
    if k == 0 or nbytes == 0:
        raise BeaconDqnError("libbeacon_dqn: %s" % L.bcn_dqn_last_error().decode())
    return ([dict(name=g.name.decode(), offset=int(g.offset), elem=int(g.elem), planes=int(g.planes), row_elems=int(g.row_elems))
             for g in segs[:k]], int(nbytes))


# ---- the agent ---------------------------------------------------------------------------
class DQN(object):
    """DQN (Mnih et al. 2015) on the device for one VecEnv with a Discrete action space -- VecMixing, VecLorenz -- with the three
    standard switches: double Q-learning (van Hasselt et al. 2016), dueling heads (Wang et al. 2016) and the Huber loss
    (include/beacon_dqn.h states every formula, order and stream; csrc/dqn/dqn_impl.h is the kernels).

        agent = DQN(env, hidden=(64, 64), activation="tanh", lr=1e-3, gamma=0.99, tau=0.005,
                    double=True, dueling=False, huber=1.0, eps=0.1, seed=None)
        agent.load_modules(q)            # nn.Sequential: obs_dim -> ... -> n (dueling: n + 1 head rows, V last); also sets the target
        mem = agent.replay(capacity); ro = env.rollout(T)
        env.reset()
        for it in range(n_iter):
            ro.begin()
            for _ in range(T):
                env.step_autoreset(agent.act(mode="uniform" if it < warm else "epsilon"))
            mem.append(ro)
            agent.update(mem, n_updates=T, batch_size=256)

    q maps obs_dim -> n = action_space.n outputs, Q_j = head_j; with dueling=True the head has n + 1 rows, A_j = head_j, V = head_n
    and Q_j = (V + A_j) - mean_k A_k.  The greedy action is the FIRST maximum.  y = r + gamma boot Q_target(s', j*) with j* the
    online network's argmax (double=True) or the target's own (double=False); the loss is the mean over live rows of delta^2 / 2
    (huber=None) or of the Huber function with kappa = huber.
    Owns `params` and `target` (one uint8 buffer each in the layout of bcn_dqn_params_layout; `weights` / `target_weights` map the
    segment names -- q_w0, q_b0, ... -- to typed views, matrices [out, in]), `state` (counters int32 [B]: the acting stream's uint32
    draw counters' bits; step_count int32 [4]: [0] the Adam steps; stats float64 [8]; adam_m, adam_v) and `actions` int32 [B].
    Fresh parameters are zero.
    act(): ONE launch; mode "greedy", "epsilon" (the random action where u < eps) or "uniform" (warm-up; Q is not evaluated).
    `eps` is a float or a one-element device tensor of the env dtype that the kernel reads: a captured act() follows a schedule
    the caller writes with a tensor op.  q_values(rows) -> [rows, n]: ONE launch, for diagnostics.
    update(mem, n_updates, batch_size, target_every=1): per minibatch k sample (2 launches) + gradient (3) + Adam (2), and where
    (k + 1) % target_every == 0 -- plain control flow -- Polyak (1; tau = 1 is the hard copy).  plan(mem, n_updates, batch_size,
    target_every) is the same chain allocated once, with run() and capture().
    The hyperparameters are plain attributes and ARGUMENTS of the launches: a captured graph keeps what it was recorded with.
    max_grad_norm (None or <= 0: off, the default) clips the gradient by its global norm.  stats_dict() is the only host read.
    Not covered: Box action spaces (TD3 / SAC take those) -- ValueError; prioritised replay; n-step returns; distributional /
    noisy heads; per_jet policies and ShardedVecEnv -- ValueError; n > 16 actions (15 with dueling)."""

    def __init__(self, env, hidden=(64, 64), activation="tanh", lr=1e-3, gamma=0.99, tau=0.005, double=True, dueling=False, huber=1.0,
                 eps=0.1, seed=None, replica_offset=0, betas=(0.9, 0.999), eps_adam=1e-8, max_grad_norm=None, per_jet=False):
        if per_jet:
            raise ValueError("DQN: per_jet policies are not covered: the Q network serves the whole replica")
        if type(env).__name__ == "ShardedVecEnv" or hasattr(env, "global_batch"):
            raise ValueError("DQN: ShardedVecEnv is not covered: the agent's buffers live on one device")
        try:
            hid = [int(h) for h in hidden]
            ok = all(int(h) == h and not isinstance(h, bool) for h in hidden)
        except (TypeError, ValueError):
            hid, ok = [], False
        if not ok or not 1 <= len(hid) <= _actor.MAX_LAYERS or any(not 1 <= h <= _actor.MAX_HIDDEN for h in hid):
            raise ValueError("DQN: hidden must be 1 .. %d integer widths of 1 .. %d, got %r" % (_actor.MAX_LAYERS, _actor.MAX_HIDDEN, hidden))
        if activation not in _actor._ACTIVATIONS:
            raise ValueError("DQN: activation must be 'tanh' or 'relu', got %r" % (activation,))
        space = getattr(env, "action_space", None)
        if space is None:
            raise ValueError("DQN: env has no action_space")
        if not getattr(env, "action_is_int", False) or not hasattr(space, "n"):
            raise ValueError("DQN: env.action_space is a Box; a Q network with one output per action needs a Discrete space (TD3 / SAC "
                             "take the Box envs)")
        for name, flag in (("double", double), ("dueling", dueling)):
            if not isinstance(flag, (bool, np.bool_)):
                raise ValueError("DQN: %s must be True or False, got %r" % (name, flag))
        n, obs_dim = int(space.n), int(env.obs_dim)
        if not 2 <= n or n + int(dueling) > MAX_ACTIONS:
            raise ValueError("DQN: env.action_space has %d actions; the head takes 2 .. %d (%d with dueling: the value row is the head's last)"
                             % (n, MAX_ACTIONS, MAX_ACTIONS - 1))
        if not 1 <= obs_dim <= MAX_OBS:
            raise ValueError("DQN: env.obs_dim = %d; the network reads rows of at most %d" % (obs_dim, MAX_OBS))
        self.env = env
        self.batch, self.obs_dim, self.n_actions, self.tdtype, self.device = int(env.batch), obs_dim, n, env.tdtype, torch.device(env.device)
        self.act_dim = 1                                  # the ring's act segment: [C, 1], the action index
        self.hidden, self.activation, self.double, self.dueling = tuple(hid), activation, bool(double), bool(dueling)
        self.n_head = n + int(self.dueling)
        self.set_hyper(lr=lr, gamma=gamma, tau=tau, huber=huber, eps=eps, betas=betas, eps_adam=eps_adam, max_grad_norm=max_grad_norm)
        dt = 1 if self.tdtype == torch.float64 else 0
        self.cfg = make_cfg(self.batch, obs_dim, n, dt, hid, activation, self.dueling)
        # the memory is libbeacon_td3.so's: the same batch, obs_dim, dtype and widths as a bcn_td3_cfg, and act_dim = 1
        self.replay_cfg = _td3.make_cfg(self.batch, obs_dim, 1, dt, hid, activation, -1.0, 1.0, 1)
        self.lib = load()
        self.params_layout, nbytes = layout("params", self.cfg)
        self.params = torch.zeros((nbytes,), dtype=torch.uint8, device=self.device)
        self.target = torch.zeros((nbytes,), dtype=torch.uint8, device=self.device)
        self.shapes = {}
        dims = [obs_dim] + hid + [self.n_head]
        for l in range(len(hid) + 1):
            self.shapes["q_w%d" % l] = (dims[l + 1], dims[l])
            self.shapes["q_b%d" % l] = (dims[l + 1],)
        self.weights = {k: v.view(self.shapes[k]) for k, v in _views(self.params, self.params_layout, self.tdtype).items()}
        self.target_weights = {k: v.view(self.shapes[k]) for k, v in _views(self.target, self.params_layout, self.tdtype).items()}
        self.state_layout, nbytes = layout("state", self.cfg)
        self.state = torch.zeros((nbytes,), dtype=torch.uint8, device=self.device)
        v = _views(self.state, self.state_layout, self.tdtype)
        self.counters, self.step_count, self.stats, self.adam_m, self.adam_v = v["counters"], v["step"], v["stats"], v["adam_m"], v["adam_v"]
        self.actions = torch.zeros((self.batch,), dtype=torch.int32, device=self.device)
        self.grid = int(self.lib.bcn_dqn_grid(C.byref(self.cfg)))
        self.lds_bytes = int(self.lib.bcn_dqn_lds_bytes(C.byref(self.cfg)))
        self._mems, self._plan, self._keep = weakref.WeakSet(), None, None
        if seed is None:
            seed = getattr(env, "seed", None) if isinstance(getattr(env, "seed", None), (int, np.integer)) else 0
        self.set_seed(seed, replica_offset)

    _HYPER = ("lr", "gamma", "tau", "huber", "eps", "betas", "eps_adam", "max_grad_norm")

    def set_hyper(self, **kw):
        """Check and set hyperparameters by name (lr, gamma, tau, huber, eps, betas, eps_adam, max_grad_norm).  ValueError names the
        field; nothing is set then.  eps: a number in [0, 1], or a one-element tensor of the env dtype on the env's device."""
        new = {}
        for k, x in kw.items():
            if k in ("lr", "eps_adam"):
                new[k] = _number("DQN", k, x, lo=0.0)
            elif k in ("gamma", "tau"):
                new[k] = _number("DQN", k, x, lo=0.0, hi=1.0, hi_closed=True)
            elif k == "huber":
                new[k] = None if x is None else _number("DQN", k, x, lo=0.0, lo_open=True)
            elif k == "eps":
                if torch.is_tensor(x):
                    if x.numel() != 1 or x.dtype != self.tdtype or x.device != self.device or not x.is_contiguous():
                        raise ValueError("DQN: eps as a tensor must hold one %s element on %s" % (str(self.tdtype).replace("torch.", ""), self.device))
                    new[k] = x
                else:
                    new[k] = _number("DQN", k, x, lo=0.0, hi=1.0, hi_closed=True)
            elif k == "max_grad_norm":
                new[k] = 0.0 if x is None else _number("DQN", k, x)
            elif k == "betas":
                try:
                    b1, b2 = x
                except (TypeError, ValueError):
                    raise ValueError("DQN: betas must be a pair of numbers in [0, 1), got %r" % (x,))
                new[k] = (_number("DQN", "betas[0]", b1, lo=0.0, hi=1.0), _number("DQN", "betas[1]", b2, lo=0.0, hi=1.0))
            else:
                raise ValueError("DQN: unknown hyperparameter %r" % (k,))
        for k, x in new.items():
            setattr(self, k, x)
        return self

    def set_seed(self, seed, replica_offset=0):
        """Key both streams (acting, replay sampling) by `seed` with replica 0 at the global index `replica_offset`, and zero their
        counters: `counters` and head[3] of every memory of this agent."""
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
            raise ValueError("DQN.set_seed: seed must be an integer in [0, 2^64), got %r" % (seed,))
        if isinstance(replica_offset, bool) or not isinstance(replica_offset, (int, np.integer)) or not 0 <= int(replica_offset) < 1 << 62:
            raise ValueError("DQN.set_seed: replica_offset must be a non-negative integer, got %r" % (replica_offset,))
        self.seed, self.replica_offset = int(seed), int(replica_offset)
        self.counters.zero_()
        for mem in self._mems:
            mem.head[3:4].zero_()
        return self

    # -- parameters -------------------------------------------------------------------------
    def load(self, q):
        """Copy the network into the parameter buffer AND the target buffer: q = [(W, b), ...] for the hidden layers and the head, W
        [out, in] (the head [n, h_last], or [n + 1, h_last] with dueling: the advantage rows, then the value row).  ValueError for
        a wrong count or shape; nothing is written then."""
        if q is None or len(q) != len(self.hidden) + 1:
            raise ValueError("DQN.load: q must be %d (W, b) pairs" % (len(self.hidden) + 1))
        todo = []
        for l, (W, b) in enumerate(q):
            W, b = torch.as_tensor(W), torch.as_tensor(b)
            want = self.shapes["q_w%d" % l]
            if tuple(W.shape) != want or b.numel() != want[0]:
                raise ValueError("DQN.load: q[%d] must be W [%d, %d] and b [%d], got %s and %s"
                                 % (l, want[0], want[1], want[0], tuple(W.shape), tuple(b.shape)))
            todo += [("q_w%d" % l, W), ("q_b%d" % l, b.reshape(-1))]
        with torch.no_grad():
            for name, t in todo:
                self.weights[name].copy_(t.detach().to(device=self.device, dtype=self.tdtype))
        return self.sync_targets()

    def load_modules(self, q):
        """load() from a torch.nn.Sequential of Linear layers with this agent's activation between them (Tanh / ReLU); the dueling
        combination is the library's and no part of the module."""
        import torch.nn as nn
        want = nn.Tanh if self.activation == "tanh" else nn.ReLU
        out = []
        for sub in q:
            if isinstance(sub, nn.Linear):
                if sub.bias is None:
                    raise ValueError("DQN.load_modules: q has a Linear without bias")
                out.append((sub.weight, sub.bias))
            elif not isinstance(sub, want):
                raise ValueError("DQN.load_modules: q holds a %s; expected Linear and %s only" % (type(sub).__name__, want.__name__))
        return self.load(out)

    def sync_targets(self):
        """target = params (one copy on the device)."""
        self.target.copy_(self.params)
        return self

    def state_dict(self):
        """For checkpoints: the three buffers on the CPU, what they were laid out for, seed, offset and hyperparameters (eps as a
        float: a tensor's current value)."""
        hyper = {k: getattr(self, k) for k in self._HYPER}
        if torch.is_tensor(hyper["eps"]):
            hyper["eps"] = float(hyper["eps"].reshape(-1)[0])
        return {"params": self.params.cpu(), "target": self.target.cpu(), "state": self.state.cpu(), "batch": self.batch, "obs_dim": self.obs_dim,
                "n_actions": self.n_actions, "dtype": "f64" if self.tdtype == torch.float64 else "f32", "hidden": self.hidden,
                "activation": self.activation, "double": self.double, "dueling": self.dueling, "seed": self.seed,
                "replica_offset": self.replica_offset, "hyper": hyper}

    def load_state_dict(self, d):
        keys = ("batch", "obs_dim", "n_actions", "dtype", "activation", "dueling")
        cur = {"batch": self.batch, "obs_dim": self.obs_dim, "n_actions": self.n_actions, "dtype": "f64" if self.tdtype == torch.float64 else "f32",
               "activation": self.activation, "dueling": self.dueling}
        if (any(d.get(k) != cur[k] for k in keys) or tuple(d.get("hidden", ())) != self.hidden or d["params"].numel() != self.params.numel()
                or d["state"].numel() != self.state.numel()):
            raise ValueError("DQN.load_state_dict: the state is of another agent (%s, hidden %s); this one is %s, hidden %s"
                             % ({k: d.get(k) for k in keys}, tuple(d.get("hidden", ())), cur, self.hidden))
        self.set_hyper(**d["hyper"])
        self.double = bool(d.get("double", self.double))
        self.params.copy_(d["params"])
        self.target.copy_(d["target"])
        self.state.copy_(d["state"])
        self.seed, self.replica_offset = int(d["seed"]), int(d["replica_offset"])
        return self

    # -- launches ---------------------------------------------------------------------------
    def _stream(self):
        if self.device.type != "cuda":
            raise RuntimeError("DQN: the launches need a ROCm device (no CPU fallback); this agent's env is on %s" % self.device)
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _rows(self, who, obs, rows):
        if (not torch.is_tensor(obs) or obs.dtype != self.tdtype or obs.device != self.device or not obs.is_contiguous() or obs.dim() != 2
                or obs.shape[1] != self.obs_dim or (rows is not None and obs.shape[0] != rows) or obs.shape[0] < 1):
            raise ValueError("DQN.%s: obs must be a contiguous %s tensor [%s, %d] on %s"
                             % (who, "f64" if self.tdtype == torch.float64 else "f32", "rows" if rows is None else rows, self.obs_dim, self.device))
        return obs

    def act(self, obs=None, mask=None, mode="epsilon"):
        """ONE launch on the current stream, no host synchronisation, nothing allocated: Q on `obs` ([B, obs_dim]; default: what the
        env's last reset() / step() returned -- env._norm.norm_obs while it normalises, else env.obs) into `actions` int32 [B],
        which it returns.  mode: "greedy" the first maximum of Q; "epsilon" the random action where u < eps, else greedy; "uniform"
        the random action, for warm-up steps (Q is not evaluated).  The stochastic modes tick the replicas' draw counters.  `mask`
        ([B] bool / uint8): replicas with 0 keep their action and their counter."""
        if mode not in MODES:
            raise ValueError("DQN.act: mode must be 'greedy', 'epsilon' or 'uniform', got %r" % (mode,))
        env = self.env
        if obs is None:
            obs = env._norm.norm_obs if getattr(env, "_norm_on", False) else env.obs
        self._rows("act", obs, self.batch)
        m = None
        if mask is not None:
            if not torch.is_tensor(mask):
                mask = torch.as_tensor(np.asarray(mask))
            if mask.numel() != self.batch:
                raise ValueError("DQN.act: mask must hold %d values" % self.batch)
            m = mask.to(device=self.device, dtype=torch.uint8).reshape(self.batch).contiguous()
        stream = self._stream()
        eps_t = self.eps if torch.is_tensor(self.eps) else None
        self._keep = (obs, m, eps_t)         # alive behind the asynchronous launch
        _check(self.lib.bcn_dqn_act(C.byref(self.cfg), _p(self.params), _p(obs), _p(m), _p(self.state), _p(self.actions), MODES[mode],
                                    0.0 if eps_t is not None else self.eps, _p(eps_t), self.seed, self.replica_offset, stream))
        return self.actions

    def q_values(self, rows, out=None, target=False):
        """Q of `rows` ([rows, obs_dim]) -> [rows, n]: ONE launch, the values act() takes its argmax of (target=True: of the target
        network).  `out`: a tensor to write into (else one is allocated)."""
        self._rows("q_values", rows, None)
        if out is None:
            out = torch.empty((rows.shape[0], self.n_actions), dtype=self.tdtype, device=self.device)
        elif (not torch.is_tensor(out) or out.dtype != self.tdtype or out.device != self.device or not out.is_contiguous()
              or tuple(out.shape) != (rows.shape[0], self.n_actions)):
            raise ValueError("DQN.q_values: out must be a contiguous tensor [%d, %d] of the env dtype on %s" % (rows.shape[0], self.n_actions, self.device))
        stream = self._stream()
        self._keep = (rows, out)
        _check(self.lib.bcn_dqn_q(C.byref(self.cfg), _p(self.target if target else self.params), _p(rows), rows.shape[0], _p(out), stream))
        return out

    def replay(self, capacity):
        """A Replay of `capacity` transitions of this agent's env: the memory TD3 uses, through libbeacon_td3.so, with the action
        index in its [C, 1] act segment.  (obs_dim = 512: a SplitReplay, the same ring with a tensor per segment.)"""
        mem = (SplitReplay if self.obs_dim + 1 > _td3.MAX_IN else Replay)(self, capacity)
        self._mems.add(mem)
        return mem

    def _append(self, mem, ro, T):
        """Replay.append for this agent: the int32 [T, B] actions of `ro` into the ring (TWO launches)."""
        stream = self._stream()
        _check(self.lib.bcn_dqn_append(C.byref(self.cfg), mem.capacity, _p(mem.head), _p(mem.obs), _p(mem.act), _p(mem.rwd), _p(mem.next_obs),
                                       _p(mem.boot), _p(mem.live), T, _p(ro.obs), _p(ro.act), _p(ro.rwd), _p(ro.done), _p(ro.trunc),
                                       _p(ro.valid), _p(ro.final_obs), _p(ro.cursor), stream))

    def plan(self, mem, n_updates, batch_size, target_every=1):
        """The update as a chain of the libraries' own launches, allocated once: a Plan (plan.run(), plan.capture())."""
        return Plan(self, mem, n_updates, batch_size, target_every)

    def update(self, mem, n_updates, batch_size, target_every=1):
        """n_updates minibatches of batch_size sampled rows of `mem` (the class docstring).  The plan -- idx and the work buffer --
        is allocated by the first call and reused while (mem, n_updates, batch_size, target_every) stay the same.  Returns self."""
        p = self._plan
        if p is None or p.mem is not mem or (p.n_updates, p.batch_size, p.target_every) != (n_updates, batch_size, target_every):
            p = self._plan = Plan(self, mem, n_updates, batch_size, target_every)
        p.run()
        return self

    def stats_dict(self):
        """The statistics of the last gradient as a dict of floats: the one host read."""
        return dict(zip(STATS, self.stats.cpu().tolist()))


class SplitReplay(Replay):
    """The Replay of a DQN agent whose obs_dim is 512.  bcn_replay_layout lays a ring out for a bcn_td3_cfg, whose rows [obs | a] end at
    512 columns: 512 observation columns plus the action index are one more than it accepts.  The ring itself needs no packed layout
    -- bcn_dqn_append and bcn_dqn_grad take its segments as separate pointers and bcn_replay_sample reads `head` alone -- so this
    memory keeps every segment in a tensor of its own: the same views (head, obs, act, rwd, next_obs, boot, live), the same append()
    and sample(), no `buf` and no `layout`."""

    SEGMENTS = ("head", "obs", "act", "rwd", "next_obs", "boot", "live")

    def __init__(self, agent, capacity):
        if not isinstance(agent, DQN):
            raise ValueError("SplitReplay: agent must be a beacon_amd.DQN, got %r" % (type(agent).__name__,))
        if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or not 1 <= int(capacity) < 1 << 31:
            raise ValueError("Replay: capacity must be an integer in 1 .. 2^31 - 1, got %r" % (capacity,))
        self.agent, self.capacity, self._int_act = agent, int(capacity), True
        self.cfg, self.lib = None, _td3.load()
        self.tdtype, self.device = agent.tdtype, agent.device
        Cn, z = self.capacity, lambda shape, dt: torch.zeros(shape, dtype=dt, device=agent.device)
        self.head = z((4,), torch.int32)
        self.obs, self.next_obs = z((Cn, agent.obs_dim), self.tdtype), z((Cn, agent.obs_dim), self.tdtype)
        self.act, self.rwd = z((Cn, 1), self.tdtype), z((Cn,), self.tdtype)
        self.boot, self.live = z((Cn,), torch.uint8), z((Cn,), torch.uint8)
        self.layout = self.buf = self._keep = None

    def state_dict(self):
        a = self.agent
        return dict({k: getattr(self, k).cpu() for k in self.SEGMENTS}, capacity=self.capacity, obs_dim=a.obs_dim, act_dim=1,
                    dtype="f64" if self.tdtype == torch.float64 else "f32")

    def load_state_dict(self, d):
        a = self.agent
        cur = {"capacity": self.capacity, "obs_dim": a.obs_dim, "act_dim": 1, "dtype": "f64" if self.tdtype == torch.float64 else "f32"}
        if any(d.get(k) != v for k, v in cur.items()) or any(k not in d for k in self.SEGMENTS):
            raise ValueError("Replay.load_state_dict: the state is of another memory (%s); this one is %s" % ({k: d.get(k) for k in cur}, cur))
        for k in self.SEGMENTS:
            getattr(self, k).copy_(d[k])
        return self


class Plan(object):
    """n_updates DQN minibatches over a Replay as a chain of launches (agent.plan(mem, n_updates, batch_size, target_every) makes
    one).  Owns `idx` int32 [batch_size] and `work` (bcn_dqn_work_layout; `grads` maps the segment names to views of its gradient
    segment).  run(): per minibatch k  sample -> grad -> adam; and where (k + 1) % target_every == 0  polyak.  The pieces are public:
    sample(), grad_step(), adam(), polyak().  capture(): run() recorded as ONE graph; a replay draws new samples (the counter lives
    on the device) with the hyperparameters of the time of the capture."""

    def __init__(self, agent, mem, n_updates, batch_size, target_every=1):
        if not isinstance(agent, DQN):
            raise ValueError("DQN.plan: agent must be a beacon_amd.DQN, got %r" % (type(agent).__name__,))
        if not isinstance(mem, Replay) or mem.agent is not agent:
            raise ValueError("DQN.plan: mem must be a Replay of this agent (agent.replay(capacity))")
        self.agent, self.mem = agent, mem
        self.n_updates, self.batch_size = _count("DQN.plan", "n_updates", n_updates), _count("DQN.plan", "batch_size", batch_size)
        self.target_every = _count("DQN.plan", "target_every", target_every)
        if self.batch_size >= 1 << 31:
            raise ValueError("DQN.plan: batch_size = %d; a minibatch covers 2^31 - 1 rows" % self.batch_size)
        self.lib, self.device = agent.lib, agent.device
        self.idx = torch.zeros((self.batch_size,), dtype=torch.int32, device=self.device)
        self.work_layout, nbytes = layout("work", agent.cfg)
        self.work = torch.zeros((nbytes,), dtype=torch.uint8, device=self.device)      # zeros: the slabs' gaps are read (header)
        v = _views(self.work, self.work_layout, agent.tdtype)
        self.grad = v["grad"]
        self.grads = {k: g.view(agent.shapes[k]) for k, g in _views(self.grad.view(torch.uint8), agent.params_layout, agent.tdtype).items()}

    def _batch(self):
        a, m = self.agent, self.mem
        return DqnBatch(params=_p(a.params), target=_p(a.target), obs=_p(m.obs), act=_p(m.act), rwd=_p(m.rwd), next_obs=_p(m.next_obs),
                        boot=_p(m.boot), live=_p(m.live), idx=_p(self.idx), work=_p(self.work), state=_p(a.state), m=self.batch_size,
                        capacity=m.capacity, gamma=a.gamma, huber=0.0 if a.huber is None else a.huber, double_q=int(a.double), reserved=0)

    def sample(self):
        self.mem.sample(self.idx)
        return self

    def grad_step(self):
        """Loss, statistics and gradient for the rows of `idx`: THREE launches."""
        b = self._batch()
        _check(self.lib.bcn_dqn_grad(C.byref(self.agent.cfg), C.byref(b), self.agent._stream()))
        return self

    def adam(self):
        """One Adam step from the gradient buffer: TWO launches."""
        a = self.agent
        h = DqnAdam(lr=a.lr, beta1=a.betas[0], beta2=a.betas[1], eps=a.eps_adam, max_grad_norm=a.max_grad_norm)
        _check(self.lib.bcn_dqn_adam(C.byref(a.cfg), _p(a.params), _p(self.work), _p(a.state), C.byref(h), a._stream()))
        return self

    def polyak(self):
        """target += tau (params - target) over the whole buffer (tau = 1: the hard copy): ONE launch."""
        a = self.agent
        _check(self.lib.bcn_dqn_polyak(C.byref(a.cfg), _p(a.params), _p(a.target), a.tau, a._stream()))
        return self

    def run(self):
        """The update.  No host synchronisation, nothing allocated.  Returns self."""
        self.agent._stream()
        for k in range(self.n_updates):
            self.sample().grad_step().adam()
            if (k + 1) % self.target_every == 0:
                self.polyak()
        return self

    def capture(self):
        """run() recorded as ONE graph; nothing is launched.  Returns the torch.cuda.CUDAGraph."""
        self.agent._stream()
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize(self.device)
        with torch.cuda.graph(g):
            self.run()
        return g
