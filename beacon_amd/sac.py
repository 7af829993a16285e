"""Soft actor-critic on the device: libbeacon_sac.so (include/beacon_sac.h; csrc/sac/) and the class SAC over it.

A SAC is a tanh-squashed Gaussian policy pi(a | s) with a state-dependent log-std (ONE head matrix of 2 act_dim rows), one or two
critics Q(s, a) with their targets, a learned temperature alpha = exp(log_alpha) and three Adam optimisers.  It trains over the same
Replay as TD3 (beacon_amd.td3.Replay, laid out, appended and sampled through libbeacon_td3.so; this library receives the memory's six
row segments as plain device pointers).  Acting is ONE launch; one minibatch -- sample (2 launches), critic gradient (4), Adam (2),
policy gradient through the smaller of the critics into both halves of the head (4), Adam (2), with a learned temperature its Adam
step (2), Polyak (1) -- is 17 launches, 15 with a fixed temperature: no host read, no allocation, no atomics, every sum in a fixed
order, bit-reproducible, and capturable as ONE graph whose replays draw new samples and new noise (the counters live on the
device).  tests/sac_ref.py restates it on the host.

The library is a unit of its own, built and bound like the other five (build.py: one Unit each); its table is SIGNATURES below.
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

API_VERSION = 1                           # include/beacon_sac.h: BCN_SAC_API_VERSION
# the float64 unit: one rounding per written operation, as td3_f64.hip
FILE_FLAGS = {"sac.hip": [],
              "sac_f64.hip": ["-ffp-contract=off"]}
REAL, I32, U32, F64, U8 = 0, 1, 2, 3, 4   # BCN_SAC_REAL ...
DETERMINISTIC, SAMPLE, UNIFORM = 0, 1, 2
MODES = {"deterministic": DETERMINISTIC, "sample": SAMPLE, "uniform": UNIFORM}
OPT_CRITIC, OPT_POLICY, OPT_ALPHA = 0, 1, 2
MAX_IN, MAX_GRID, MAX_SEGS, LDS_LIMIT = 512, 128, 32, 163840
STATS = ("critic_loss", "q1_mean", "q2_mean", "target_mean", "policy_loss", "W", "critic_grad_norm", "policy_grad_norm", "logp_mean",
         "next_logp_mean", "alpha", "alpha_grad")
_vp = C.c_void_p


class SacCfg(C.Structure):
    """bcn_sac_cfg"""
    _fields_ = [("batch", C.c_int32), ("obs_dim", C.c_int32), ("act_dim", C.c_int32), ("dtype", C.c_int32), ("n_hidden", C.c_int32),
                ("hidden", C.c_int32 * 3), ("activation", C.c_int32), ("low", C.c_double), ("high", C.c_double), ("n_critics", C.c_int32)]


class SacSeg(C.Structure):
    """bcn_sac_seg"""
    _fields_ = [("name", C.c_char * 16), ("offset", C.c_uint64), ("elem", C.c_int32), ("planes", C.c_int32), ("row_elems", C.c_int64)]


class SacBatch(C.Structure):
    """bcn_sac_batch"""
    _fields_ = [("params", _vp), ("target", _vp), ("obs", _vp), ("act", _vp), ("rwd", _vp), ("next_obs", _vp), ("boot", _vp), ("live", _vp),
                ("idx", _vp), ("work", _vp), ("state", _vp), ("m", C.c_int64), ("capacity", C.c_int64), ("gamma", C.c_double),
                ("target_entropy", C.c_double), ("seed", C.c_uint64)]


class SacAdam(C.Structure):
    """bcn_sac_adam_hyper"""
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("max_grad_norm", C.c_double)]


_cfgp, _segp, _batchp = C.POINTER(SacCfg), C.POINTER(SacSeg), C.POINTER(SacBatch)
# every symbol include/beacon_sac.h declares: (restype, argtypes)
SIGNATURES = {
    "bcn_sac_params_layout": (C.c_int, [_cfgp, _segp, C.c_int]),
    "bcn_sac_params_bytes": (C.c_size_t, [_cfgp]),
    "bcn_sac_state_layout": (C.c_int, [_cfgp, _segp, C.c_int]),
    "bcn_sac_state_bytes": (C.c_size_t, [_cfgp]),
    "bcn_sac_work_layout": (C.c_int, [_cfgp, C.c_int64, _segp, C.c_int]),
    "bcn_sac_work_bytes": (C.c_size_t, [_cfgp, C.c_int64]),
    "bcn_sac_grid": (C.c_int, [_cfgp]),
    "bcn_sac_lds_bytes": (C.c_size_t, [_cfgp]),
    "bcn_sac_act": (C.c_int, [_cfgp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_uint64, C.c_int64, _vp]),
    "bcn_sac_critic_grad": (C.c_int, [_cfgp, _batchp, _vp]),
    "bcn_sac_actor_grad": (C.c_int, [_cfgp, _batchp, _vp]),
    "bcn_sac_adam": (C.c_int, [_cfgp, _vp, _vp, _vp, C.c_int, C.POINTER(SacAdam), _vp]),
    "bcn_sac_polyak": (C.c_int, [_cfgp, _vp, _vp, C.c_double, _vp]),
    "bcn_sac_last_error": (C.c_char_p, []),
}


class BeaconSacError(RuntimeError):
    pass


# ---- the library -------------------------------------------------------------------------
# (the units include csrc/td3/td3_impl.h and, through it, the network of csrc/actor/policy_net.h: the dependency rule of build.py
# follows the #include lines there)
SRC_DIR, HEADER = os.path.join(_build.CSRC, "sac"), os.path.join(_build.INC, "beacon_sac.h")
LIB, OBJ = os.path.join(_build.PKG, "libbeacon_sac.so"), os.path.join(_build.OBJ, "sac")
_UNIT = _build.hip_library(LIB, SRC_DIR, FILE_FLAGS, OBJ, SIGNATURES)
sources, signature, stale, load = _UNIT.sources, _UNIT.signature, _UNIT.stale, _UNIT.load


def build_sac(force=False, verbose=False):
    """Compile csrc/sac/*.hip for gfx950 and link libbeacon_sac.so.  Returns its path."""
    return _UNIT.build(force=force, verbose=verbose)


def _check(rc):
    if rc != 0:
        raise BeaconSacError("libbeacon_sac: error %d: %s" % (rc, load().bcn_sac_last_error().decode()))


def make_cfg(batch, obs_dim, act_dim, dtype, hidden, activation, low=-1.0, high=1.0, n_critics=2):
    """bcn_sac_cfg from plain values (dtype: 0 / 1; activation: "tanh" / "relu" or 0 / 1).  No range check: the library's."""
    hid = [int(h) for h in hidden]
    return SacCfg(batch=int(batch), obs_dim=int(obs_dim), act_dim=int(act_dim), dtype=int(dtype), n_hidden=len(hid),
                  hidden=(C.c_int32 * 3)(*(hid + [0] * 3)[:3]), activation=_actor._ACTIVATIONS.get(activation, activation),
                  low=float(low), high=float(high), n_critics=int(n_critics))


def layout(which, cfg, arg=None):
    """([segment dicts], bytes) of the "params", "state" or "work" (arg: the minibatch rows m) buffer of `cfg`; BeaconSacError with
    the library's text for what it refuses.  No device needed.  (The replay memory's layout is beacon_amd.td3.layout("replay", ...).)"""
    L = load()
    segs = (SacSeg * MAX_SEGS)()
    extra = () if which in ("params", "state") else (int(arg),)
    k = getattr(L, "bcn_sac_%s_layout" % which)(C.byref(cfg), *(extra + (segs, MAX_SEGS)))
    nbytes = getattr(L, "bcn_sac_%s_bytes" % which)(C.byref(cfg), *extra)
    if k == 0 or nbytes == 0:
        raise BeaconSacError("libbeacon_sac: %s" % L.bcn_sac_last_error().decode())
    return ([dict(name=g.name.decode(), offset=int(g.offset), elem=int(g.elem), planes=int(g.planes), row_elems=int(g.row_elems))
             for g in segs[:k]], int(nbytes))


# ---- the agent ---------------------------------------------------------------------------
class SAC(object):
    """Soft actor-critic (Haarnoja et al. 2018, the version with a learned temperature) on the device for one VecEnv with a Box action
    space (include/beacon_sac.h states every formula, order and stream; csrc/sac/sac_impl.h is the kernels).

        agent = SAC(env, hidden=(64, 64), lr=3e-4, gamma=0.99, tau=0.005, alpha=1.0, auto_alpha=True, twin=True, seed=None)
        agent.load_modules(pi, q1, q2)        # nn.Sequential of Linear + Tanh/ReLU; pi's last Linear has 2 act_dim outputs
        mem = agent.replay(capacity); ro = env.rollout(T)
        env.reset()
        for it in range(n_iter):
            ro.begin()
            for _ in range(T):
                env.step_autoreset(agent.act(mode="uniform" if it < warm else "sample"))
            mem.append(ro)
            agent.update(mem, n_updates=T, batch_size=256)

    pi maps obs_dim -> 2 act_dim: rows 0 .. n - 1 of the head are the mean m, rows n .. 2n - 1 the raw log-std; ls = clamp(raw, -20,
    2), u = m + exp(ls) z, a = c + h tanh(u) with c, h the centre and half width of the Box; log pi is the squashed Gaussian's density
    in the form that stays finite where tanh saturates.  The critics map [obs | a] -> 1.
    Owns `params` and `target` (one uint8 buffer each in the layout of bcn_sac_params_layout; `weights` / `target_weights` map the
    segment names -- pi_w0, pi_b0, ... q1_w0, ... q2_w0 ..., log_alpha -- to typed views, matrices [out, in]), `state` (counters int32
    [B]: the acting stream's uint32 draw counters' bits; step_count int32 [8]: [0] the critic's Adam steps, [1] the policy's, [2] the
    temperature's, [3] and [4] the counters of the critic step's and the policy step's draws; stats float64 [12]; adam_m, adam_v)
    and `actions` [B, act_dim].  Fresh network parameters are zero; log_alpha starts at ln(alpha).
    act(): ONE launch.  update(mem, n_updates, batch_size): per minibatch sample (2 launches) + critic gradient (4) + Adam (2) + policy
    gradient (4) + Adam (2) + -- with auto_alpha, plain control flow -- the temperature's Adam (2) + Polyak (1): 17 launches, 15 with
    auto_alpha=False.  plan(mem, n_updates, batch_size) is the same chain allocated once, with run() and capture().
    target_entropy=None means -act_dim; lr_alpha=None means lr.  The hyperparameters are plain attributes and ARGUMENTS of the
    launches: a captured graph keeps what it was recorded with.  max_grad_norm (None or <= 0: off, the default) clips the critic's
    and the policy's gradient, each by its own global norm.  stats_dict() is the only host read.
    Not covered: discrete action spaces (mixing, lorenz) and per_jet policies -- ValueError; Boxes with different bounds per
    component; prioritised replay; n-step returns; ShardedVecEnv."""

    def __init__(self, env, hidden=(64, 64), activation="tanh", lr=3e-4, gamma=0.99, tau=0.005, alpha=1.0, auto_alpha=True,
                 target_entropy=None, lr_alpha=None, twin=True, seed=None, replica_offset=0, betas=(0.9, 0.999), eps=1e-8,
                 max_grad_norm=None, per_jet=False):
        if per_jet:
            raise ValueError("SAC: per_jet policies are not covered: the policy and its critics serve the whole action row")
        try:
            hid = [int(h) for h in hidden]
            ok = all(int(h) == h and not isinstance(h, bool) for h in hidden)
        except (TypeError, ValueError):
            hid, ok = [], False
        if not ok or not 1 <= len(hid) <= _actor.MAX_LAYERS or any(not 1 <= h <= _actor.MAX_HIDDEN for h in hid):
            raise ValueError("SAC: hidden must be 1 .. %d integer widths of 1 .. %d, got %r" % (_actor.MAX_LAYERS, _actor.MAX_HIDDEN, hidden))
        if activation not in _actor._ACTIVATIONS:
            raise ValueError("SAC: activation must be 'tanh' or 'relu', got %r" % (activation,))
        space = getattr(env, "action_space", None)
        if space is None:
            raise ValueError("SAC: env has no action_space")
        if getattr(env, "action_is_int", False) or not (hasattr(space, "low") and hasattr(space, "high")):
            raise ValueError("SAC: env.action_space is discrete; a squashed Gaussian needs a Box (the discrete envs, mixing and lorenz, "
                             "are not covered)")
        lo, hi = np.asarray(space.low, dtype=np.float64).reshape(-1), np.asarray(space.high, dtype=np.float64).reshape(-1)
        act_dim, obs_dim = int(lo.size), int(env.obs_dim)
        if not 1 <= act_dim <= _actor.MAX_ACT:
            raise ValueError("SAC: env.action_space has %d components; the policy takes 1 .. %d" % (act_dim, _actor.MAX_ACT))
        if np.any(lo != lo[0]) or np.any(hi != hi[0]) or not np.isfinite(lo[0]) or not np.isfinite(hi[0]):
            raise ValueError("SAC: env.action_space must be one finite scalar bound pair for all components")
        if not lo[0] < hi[0]:
            raise ValueError("SAC: env.action_space needs low < high, got low = %g, high = %g: the log-density holds ln((high - low) / 2)"
                             % (lo[0], hi[0]))
        if obs_dim < 1 or obs_dim + act_dim > MAX_IN:
            raise ValueError("SAC: env.obs_dim + act_dim = %d + %d; a critic reads rows of at most %d" % (obs_dim, act_dim, MAX_IN))
        if not isinstance(twin, (bool, np.bool_)):
            raise ValueError("SAC: twin must be True or False, got %r" % (twin,))
        if not isinstance(auto_alpha, (bool, np.bool_)):
            raise ValueError("SAC: auto_alpha must be True or False, got %r" % (auto_alpha,))
        alpha = _number("SAC", "alpha", alpha, lo=0.0, lo_open=True)
        self.env = env
        self.batch, self.obs_dim, self.act_dim, self.tdtype, self.device = int(env.batch), obs_dim, act_dim, env.tdtype, torch.device(env.device)
        self.hidden, self.activation, self.low, self.high, self.twin = tuple(hid), activation, float(lo[0]), float(hi[0]), bool(twin)
        self.n_critics, self.auto_alpha, self.alpha0 = 2 if twin else 1, bool(auto_alpha), alpha
        self.set_hyper(lr=lr, gamma=gamma, tau=tau, target_entropy=target_entropy, lr_alpha=lr_alpha, betas=betas, eps=eps,
                       max_grad_norm=max_grad_norm)
        dt = 1 if self.tdtype == torch.float64 else 0
        self.cfg = make_cfg(self.batch, obs_dim, act_dim, dt, hid, activation, self.low, self.high, self.n_critics)
        # the memory is libbeacon_td3.so's: the same batch, dims, dtype and widths as a bcn_td3_cfg
        self.replay_cfg = _td3.make_cfg(self.batch, obs_dim, act_dim, dt, hid, activation, self.low, self.high, self.n_critics)
        self.lib = load()
        self.params_layout, nbytes = layout("params", self.cfg)
        self.params = torch.zeros((nbytes,), dtype=torch.uint8, device=self.device)
        self.target = torch.zeros((nbytes,), dtype=torch.uint8, device=self.device)
        self.shapes = {"log_alpha": (1,)}
        for net, first, head in (("pi", obs_dim, 2 * act_dim), ("q1", obs_dim + act_dim, 1), ("q2", obs_dim + act_dim, 1))[:1 + self.n_critics]:
            dims = [first] + hid + [head]
            for l in range(len(hid) + 1):
                self.shapes["%s_w%d" % (net, l)] = (dims[l + 1], dims[l])
                self.shapes["%s_b%d" % (net, l)] = (dims[l + 1],)
        self.weights = {k: v.view(self.shapes[k]) for k, v in _views(self.params, self.params_layout, self.tdtype).items()}
        self.target_weights = {k: v.view(self.shapes[k]) for k, v in _views(self.target, self.params_layout, self.tdtype).items()}
        self.log_alpha = self.weights["log_alpha"]
        self.log_alpha.fill_(float(np.log(alpha)))
        self.target_weights["log_alpha"].fill_(float(np.log(alpha)))
        self.state_layout, nbytes = layout("state", self.cfg)
        self.state = torch.zeros((nbytes,), dtype=torch.uint8, device=self.device)
        v = _views(self.state, self.state_layout, self.tdtype)
        self.counters, self.step_count, self.stats, self.adam_m, self.adam_v = v["counters"], v["step"], v["stats"], v["adam_m"], v["adam_v"]
        self.actions = torch.zeros((self.batch, act_dim), dtype=self.tdtype, device=self.device)
        self.grid = int(self.lib.bcn_sac_grid(C.byref(self.cfg)))
        self.lds_bytes = int(self.lib.bcn_sac_lds_bytes(C.byref(self.cfg)))
        self._mems, self._plan, self._keep = weakref.WeakSet(), None, None
        if seed is None:
            seed = getattr(env, "seed", None) if isinstance(getattr(env, "seed", None), (int, np.integer)) else 0
        self.set_seed(seed, replica_offset)

    def set_hyper(self, **kw):
        """Check and set hyperparameters by name (lr, gamma, tau, target_entropy, lr_alpha, betas, eps, max_grad_norm).  ValueError
        names the field; nothing is set then."""
        new = {}
        for k, x in kw.items():
            if k in ("lr", "eps"):
                new[k] = _number("SAC", k, x, lo=0.0)
            elif k == "lr_alpha":
                new[k] = None if x is None else _number("SAC", k, x, lo=0.0)
            elif k == "target_entropy":
                new[k] = None if x is None else _number("SAC", k, x)
            elif k in ("gamma", "tau"):
                new[k] = _number("SAC", k, x, lo=0.0, hi=1.0, hi_closed=True)
            elif k == "max_grad_norm":
                new[k] = 0.0 if x is None else _number("SAC", k, x)
            elif k == "betas":
                try:
                    b1, b2 = x
                except (TypeError, ValueError):
                    raise ValueError("SAC: betas must be a pair of numbers in [0, 1), got %r" % (x,))
                new[k] = (_number("SAC", "betas[0]", b1, lo=0.0, hi=1.0), _number("SAC", "betas[1]", b2, lo=0.0, hi=1.0))
            else:
                raise ValueError("SAC: unknown hyperparameter %r" % (k,))
        for k, x in new.items():
            setattr(self, k, x)
        return self

    def entropy_target(self):
        """target_entropy, None meaning -act_dim"""
        return float(-self.act_dim) if self.target_entropy is None else self.target_entropy

    def alpha_lr(self):
        """lr_alpha, None meaning lr"""
        return self.lr if self.lr_alpha is None else self.lr_alpha

    def set_seed(self, seed, replica_offset=0):
        """Key all four streams (acting, replay sampling, the critic step's and the policy step's draws) by `seed` with replica 0 at the
        global index `replica_offset`, and zero their counters: `counters`, step_count[3], step_count[4] and head[3] of every memory
        of this agent."""
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
            raise ValueError("SAC.set_seed: seed must be an integer in [0, 2^64), got %r" % (seed,))
        if isinstance(replica_offset, bool) or not isinstance(replica_offset, (int, np.integer)) or not 0 <= int(replica_offset) < 1 << 62:
            raise ValueError("SAC.set_seed: replica_offset must be a non-negative integer, got %r" % (replica_offset,))
        self.seed, self.replica_offset = int(seed), int(replica_offset)
        self.counters.zero_()
        self.step_count[3:5].zero_()
        for mem in self._mems:
            mem.head[3:4].zero_()
        return self

    # -- parameters -------------------------------------------------------------------------
    def load(self, pi, q1, q2=None):
        """Copy the networks into the parameter buffer AND the target buffer: pi, q1, q2 = [(W, b), ...] for the hidden layers and
        the head, W [out, in] (pi's head [2 act_dim, h_last]: mean rows, then raw log-std rows; q*'s first matrix [hidden[0], obs_dim
        + act_dim], observation columns first).  q2 belongs to a twin agent.  log_alpha is left as it is.  ValueError for a wrong
        count or shape; nothing is written then."""
        nets = [("pi", pi), ("q1", q1)] + ([("q2", q2)] if self.twin else [])
        if not self.twin and q2 is not None:
            raise ValueError("SAC.load: q2 given, but this agent has one critic (twin=False)")
        todo = []
        for net, layers in nets:
            if layers is None or len(layers) != len(self.hidden) + 1:
                raise ValueError("SAC.load: %s must be %d (W, b) pairs" % (net, len(self.hidden) + 1))
            for l, (W, b) in enumerate(layers):
                W, b = torch.as_tensor(W), torch.as_tensor(b)
                want = self.shapes["%s_w%d" % (net, l)]
                if tuple(W.shape) != want or b.numel() != want[0]:
                    raise ValueError("SAC.load: %s[%d] must be W [%d, %d] and b [%d], got %s and %s"
                                     % (net, l, want[0], want[1], want[0], tuple(W.shape), tuple(b.shape)))
                todo += [("%s_w%d" % (net, l), W), ("%s_b%d" % (net, l), b.reshape(-1))]
        with torch.no_grad():
            for name, t in todo:
                self.weights[name].copy_(t.detach().to(device=self.device, dtype=self.tdtype))
        return self.sync_targets()

    def load_modules(self, pi, q1, q2=None):
        """load() from torch.nn.Sequential modules of Linear layers with this agent's activation between them (Tanh / ReLU); the
        clamp, the squashing and the split of pi's last Linear into mean and log-std are the library's and no part of the module."""
        import torch.nn as nn
        want = nn.Tanh if self.activation == "tanh" else nn.ReLU

        def pairs(what, m):
            if m is None:
                return None
            out = []
            for sub in m:
                if isinstance(sub, nn.Linear):
                    if sub.bias is None:
                        raise ValueError("SAC.load_modules: %s has a Linear without bias" % what)
                    out.append((sub.weight, sub.bias))
                elif not isinstance(sub, want):
                    raise ValueError("SAC.load_modules: %s holds a %s; expected Linear and %s only" % (what, type(sub).__name__, want.__name__))
            return out
        return self.load(pairs("pi", pi), pairs("q1", q1), pairs("q2", q2))

    def sync_targets(self):
        """target = params (one copy on the device)."""
        self.target.copy_(self.params)
        return self

    _HYPER = ("lr", "gamma", "tau", "target_entropy", "lr_alpha", "betas", "eps", "max_grad_norm")

    def state_dict(self):
        """For checkpoints: the three buffers on the CPU, what they were laid out for, seed, offset and hyperparameters."""
        return {"params": self.params.cpu(), "target": self.target.cpu(), "state": self.state.cpu(), "batch": self.batch, "obs_dim": self.obs_dim,
                "act_dim": self.act_dim, "dtype": "f64" if self.tdtype == torch.float64 else "f32", "hidden": self.hidden,
                "activation": self.activation, "n_critics": self.n_critics, "auto_alpha": self.auto_alpha, "seed": self.seed,
                "replica_offset": self.replica_offset, "hyper": {k: getattr(self, k) for k in self._HYPER}}

    def load_state_dict(self, d):
        keys = ("batch", "obs_dim", "act_dim", "dtype", "activation", "n_critics")
        cur = {"batch": self.batch, "obs_dim": self.obs_dim, "act_dim": self.act_dim, "dtype": "f64" if self.tdtype == torch.float64 else "f32",
               "activation": self.activation, "n_critics": self.n_critics}
        if (any(d.get(k) != cur[k] for k in keys) or tuple(d.get("hidden", ())) != self.hidden or d["params"].numel() != self.params.numel()
                or d["state"].numel() != self.state.numel()):
            raise ValueError("SAC.load_state_dict: the state is of another agent (%s, hidden %s); this one is %s, hidden %s"
                             % ({k: d.get(k) for k in keys}, tuple(d.get("hidden", ())), cur, self.hidden))
        self.set_hyper(**d["hyper"])
        self.auto_alpha = bool(d.get("auto_alpha", self.auto_alpha))
        self.params.copy_(d["params"])
        self.target.copy_(d["target"])
        self.state.copy_(d["state"])
        self.seed, self.replica_offset = int(d["seed"]), int(d["replica_offset"])
        return self

    # -- launches ---------------------------------------------------------------------------
    def _stream(self):
        if self.device.type != "cuda":
            raise RuntimeError("SAC: the launches need a ROCm device (no CPU fallback); this agent's env is on %s" % self.device)
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def act(self, obs=None, mask=None, mode="sample"):
        """ONE launch on the current stream, no host synchronisation, nothing allocated: pi on `obs` ([B, obs_dim]; default: what the
        env's last reset() / step() returned -- env._norm.norm_obs while it normalises, else env.obs) into `actions`, which it
        returns.  mode: "sample" a ~ pi(. | s); "deterministic" a = c + h tanh(mean); "uniform" a = low + (high - low) u, for warm-up
        steps (pi is not evaluated).  The stochastic modes tick the replicas' draw counters.  `mask` ([B] bool / uint8): replicas
        with 0 keep their action row and their counter."""
        if mode not in MODES:
            raise ValueError("SAC.act: mode must be 'sample', 'deterministic' or 'uniform', got %r" % (mode,))
        env = self.env
        if obs is None:
            obs = env._norm.norm_obs if getattr(env, "_norm_on", False) else env.obs
        if (not torch.is_tensor(obs) or obs.dtype != self.tdtype or obs.device != self.device or not obs.is_contiguous() or obs.dim() != 2
                or tuple(obs.shape) != (self.batch, self.obs_dim)):
            raise ValueError("SAC.act: obs must be a contiguous %s tensor [%d, %d] on %s"
                             % ("f64" if self.tdtype == torch.float64 else "f32", self.batch, self.obs_dim, self.device))
        m = None
        if mask is not None:
            if not torch.is_tensor(mask):
                mask = torch.as_tensor(np.asarray(mask))
            if mask.numel() != self.batch:
                raise ValueError("SAC.act: mask must hold %d values" % self.batch)
            m = mask.to(device=self.device, dtype=torch.uint8).reshape(self.batch).contiguous()
        stream = self._stream()
        self._keep = (obs, m)                # alive behind the asynchronous launch
        _check(self.lib.bcn_sac_act(C.byref(self.cfg), _p(self.params), _p(obs), _p(m), _p(self.state), _p(self.actions), MODES[mode],
                                    self.seed, self.replica_offset, stream))
        return self.actions

    def replay(self, capacity):
        """A Replay of `capacity` transitions of this agent's env: the memory TD3 uses, through libbeacon_td3.so."""
        mem = Replay(self, capacity)
        self._mems.add(mem)
        return mem

    def plan(self, mem, n_updates, batch_size):
        """The update as a chain of the libraries' own launches, allocated once: a Plan (plan.run(), plan.capture())."""
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
    """n_updates SAC minibatches over a Replay as a chain of launches (agent.plan(mem, n_updates, batch_size) makes one).  Owns `idx`
    int32 [batch_size] and `work` (bcn_sac_work_layout; `grads` maps the segment names to views of its gradient segment).
    run(): per minibatch  sample -> critic_step() -> policy_step() (with agent.auto_alpha its alpha step inside) .  The pieces are
    public: sample(), critic_grad(), adam(which), actor_grad(), polyak().  capture(): run() recorded as ONE graph; a replay draws new
    samples and new noise (their counters live on the device) with the hyperparameters of the time of the capture."""

    def __init__(self, agent, mem, n_updates, batch_size):
        if not isinstance(agent, SAC):
            raise ValueError("SAC.plan: agent must be a beacon_amd.SAC, got %r" % (type(agent).__name__,))
        if not isinstance(mem, Replay) or mem.agent is not agent:
            raise ValueError("SAC.plan: mem must be a Replay of this agent (agent.replay(capacity))")
        self.agent, self.mem = agent, mem
        self.n_updates, self.batch_size = _count("SAC.plan", "n_updates", n_updates), _count("SAC.plan", "batch_size", batch_size)
        if self.batch_size >= 1 << 31:
            raise ValueError("SAC.plan: batch_size = %d; a minibatch covers 2^31 - 1 rows" % self.batch_size)
        self.lib, self.device = agent.lib, agent.device
        self.idx = torch.zeros((self.batch_size,), dtype=torch.int32, device=self.device)
        self.work_layout, nbytes = layout("work", agent.cfg, self.batch_size)
        self.work = torch.zeros((nbytes,), dtype=torch.uint8, device=self.device)      # zeros: the slabs' gaps are read (header)
        v = _views(self.work, self.work_layout, agent.tdtype)
        self.grad = v["grad"]
        self.grads = {k: g.view(agent.shapes[k]) for k, g in _views(self.grad.view(torch.uint8), agent.params_layout, agent.tdtype).items()}
        self.xa, self.xb, self.rw = v["xa"], v["xb"], v["rw"]

    def _batch(self):
        a, m = self.agent, self.mem
        return SacBatch(params=_p(a.params), target=_p(a.target), obs=_p(m.obs), act=_p(m.act), rwd=_p(m.rwd), next_obs=_p(m.next_obs),
                        boot=_p(m.boot), live=_p(m.live), idx=_p(self.idx), work=_p(self.work), state=_p(a.state), m=self.batch_size,
                        capacity=m.capacity, gamma=a.gamma, target_entropy=a.entropy_target(), seed=a.seed)

    def sample(self):
        self.mem.sample(self.idx)
        return self

    def critic_grad(self):
        """Loss, statistics and gradient of the critics for the rows of `idx`: FOUR launches."""
        b = self._batch()
        _check(self.lib.bcn_sac_critic_grad(C.byref(self.agent.cfg), C.byref(b), self.agent._stream()))
        return self

    def actor_grad(self):
        """Loss and gradient of the policy through the smaller critic, and the temperature's gradient, for the rows of `idx` (behind
        critic_grad() of the same rows): FOUR launches."""
        b = self._batch()
        _check(self.lib.bcn_sac_actor_grad(C.byref(self.agent.cfg), C.byref(b), self.agent._stream()))
        return self

    def adam(self, which):
        """One Adam step of the critic (OPT_CRITIC), the policy (OPT_POLICY) or the temperature (OPT_ALPHA, at lr_alpha) from the
        gradient buffer: TWO launches."""
        a = self.agent
        h = SacAdam(lr=a.alpha_lr() if int(which) == OPT_ALPHA else a.lr, beta1=a.betas[0], beta2=a.betas[1], eps=a.eps, max_grad_norm=a.max_grad_norm)
        _check(self.lib.bcn_sac_adam(C.byref(a.cfg), _p(a.params), _p(self.work), _p(a.state), int(which), C.byref(h), a._stream()))
        return self

    def polyak(self):
        """target += tau (params - target) over the whole buffer: ONE launch."""
        a = self.agent
        _check(self.lib.bcn_sac_polyak(C.byref(a.cfg), _p(a.params), _p(a.target), a.tau, a._stream()))
        return self

    def critic_step(self):
        return self.critic_grad().adam(OPT_CRITIC)

    def policy_step(self):
        self.actor_grad().adam(OPT_POLICY)
        if self.agent.auto_alpha:
            self.adam(OPT_ALPHA)
        return self.polyak()

    def run(self):
        """The update.  No host synchronisation, nothing allocated.  Returns self."""
        self.agent._stream()
        for _ in range(self.n_updates):
            self.sample().critic_step().policy_step()
        return self

    def capture(self):
        """run() recorded as ONE graph; nothing is launched.  Returns the torch.cuda.CUDAGraph."""
        self.agent._stream()
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize(self.device)
        with torch.cuda.graph(g):
            self.run()
        return g
