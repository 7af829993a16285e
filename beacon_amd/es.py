"""Evolution strategies on the device: libbeacon_es.so (include/beacon_es.h; csrc/es/) and the class ES over it.

An ES agent (Salimans et al. 2017) holds ONE parameter vector theta and, per generation, a population of M perturbed copies of it in
antithetic pairs, pop[2j] = theta + sigma eps_j and pop[2j + 1] = theta - sigma eps_j.  The batch of the env is the population: with
R = batch / M replicas per member, replica b runs the policy of member b / R -- an MLP whose weights differ per row group, which is
the one kernel the other libraries do not have.  The fitness of a member is the mean return of its replicas' first episodes; the
update ranks the members, forms the centred-rank gradient estimate from regenerated noise and takes an Adam step on theta.  No
backward pass, no replay memory, no value network: begin (1 launch), act (1) and observe (1) per step, update (7), no host read, no
allocation, no atomics, every sum in a fixed order, bit-reproducible, and capturable as ONE graph whose replays draw new
perturbations (the generation counter lives on the device).  tests/es_ref.py restates it on the host.

The library is a unit of its own, built and bound like the other seven (build.py: one Unit each); its table is SIGNATURES below.
Importing this module touches neither a compiler nor the GPU."""
import ctypes as C
import os

import numpy as np
import torch

from . import actor as _actor
from . import build as _build
from .td3 import _number, _p, _views

API_VERSION = 1                           # include/beacon_es.h: BCN_ES_API_VERSION
# the float64 unit: one rounding per written operation, as td3_f64.hip
FILE_FLAGS = {"es.hip": [],
              "es_f64.hip": ["-ffp-contract=off"]}
REAL, I32, U32, F64, U8 = 0, 1, 2, 3, 4   # BCN_ES_REAL ...
BOX, DISCRETE = 0, 1
MAX_MEMBERS, MAX_OBS, MAX_ACT, PAIR_CHUNK, TILE_ROWS, MAX_GROUP, WANT_GRID, MAX_SEGS, LDS_LIMIT = 16384, 512, 16, 64, 32, 8, 1024, 16, 163840
STATS = ("fit_mean", "fit_std", "fit_min", "fit_max", "best_member", "nan_members", "grad_norm", "spare")
_vp = C.c_void_p


class EsCfg(C.Structure):
    """bcn_es_cfg"""
    _fields_ = [("batch", C.c_int32), ("members", C.c_int32), ("obs_dim", C.c_int32), ("kind", C.c_int32), ("act_dim", C.c_int32),
                ("n_actions", C.c_int32), ("dtype", C.c_int32), ("n_hidden", C.c_int32), ("hidden", C.c_int32 * 3), ("activation", C.c_int32),
                ("group", C.c_int32), ("reserved", C.c_int32), ("low", C.c_double), ("high", C.c_double)]


class EsSeg(C.Structure):
    """bcn_es_seg"""
    _fields_ = [("name", C.c_char * 16), ("offset", C.c_uint64), ("elem", C.c_int32), ("planes", C.c_int32), ("row_elems", C.c_int64)]


class EsHyper(C.Structure):
    """bcn_es_hyper"""
    _fields_ = [("sigma", C.c_double), ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("max_grad_norm", C.c_double), ("weight_decay", C.c_double)]


_cfgp, _segp = C.POINTER(EsCfg), C.POINTER(EsSeg)
# every symbol include/beacon_es.h declares: (restype, argtypes)
SIGNATURES = {
    "bcn_es_params_layout": (C.c_int, [_cfgp, _segp, C.c_int]),
    "bcn_es_params_bytes": (C.c_size_t, [_cfgp]),
    "bcn_es_state_layout": (C.c_int, [_cfgp, _segp, C.c_int]),
    "bcn_es_state_bytes": (C.c_size_t, [_cfgp]),
    "bcn_es_work_layout": (C.c_int, [_cfgp, _segp, C.c_int]),
    "bcn_es_work_bytes": (C.c_size_t, [_cfgp]),
    "bcn_es_group": (C.c_int, [_cfgp]),
    "bcn_es_lds_bytes": (C.c_size_t, [_cfgp]),
    "bcn_es_begin": (C.c_int, [_cfgp, _vp, _vp, _vp, C.c_double, C.c_uint64, _vp]),
    "bcn_es_act": (C.c_int, [_cfgp, _vp, C.c_int, _vp, _vp, _vp, _vp]),
    "bcn_es_observe": (C.c_int, [_cfgp, _vp, _vp, _vp, _vp, _vp]),
    "bcn_es_update": (C.c_int, [_cfgp, _vp, _vp, _vp, C.POINTER(EsHyper), C.c_uint64, _vp]),
    "bcn_es_last_error": (C.c_char_p, []),
}


class BeaconEsError(RuntimeError):
    pass


# ---- the library -------------------------------------------------------------------------
# (the units include csrc/td3/td3_impl.h and, through it, csrc/actor/policy_net.h: the dependency rule of build.py follows the
# #include lines there)
SRC_DIR, HEADER = os.path.join(_build.CSRC, "es"), os.path.join(_build.INC, "beacon_es.h")
LIB, OBJ = os.path.join(_build.PKG, "libbeacon_es.so"), os.path.join(_build.OBJ, "es")
_UNIT = _build.hip_library(LIB, SRC_DIR, FILE_FLAGS, OBJ, SIGNATURES)
sources, signature, stale, load = _UNIT.sources, _UNIT.signature, _UNIT.stale, _UNIT.load


def build_es(force=False, verbose=False):
    """Compile csrc/es/*.hip for gfx950 and link libbeacon_es.so.  Returns its path."""
    return _UNIT.build(force=force, verbose=verbose)


def _check(rc):
    if rc != 0:
        raise BeaconEsError("libbeacon_es: error %d: %s" % (rc, load().bcn_es_last_error().decode()))


def make_cfg(batch, members, obs_dim, kind, n_out, dtype, hidden, activation, low=-1.0, high=1.0, group=0):
    """bcn_es_cfg from plain values (kind: 0 Box / 1 Discrete; n_out: act_dim or n_actions; dtype: 0 / 1; activation: "tanh" / "relu" or
    0 / 1).  No range check: the library's."""
    hid = [int(h) for h in hidden]
    return EsCfg(batch=int(batch), members=int(members), obs_dim=int(obs_dim), kind=int(kind), act_dim=int(n_out) if kind == BOX else 0,
                 n_actions=int(n_out) if kind != BOX else 0, dtype=int(dtype), n_hidden=len(hid), hidden=(C.c_int32 * 3)(*(hid + [0] * 3)[:3]),
                 activation=_actor._ACTIVATIONS.get(activation, activation), group=int(group), reserved=0, low=float(low), high=float(high))


def layout(which, cfg):
    """([segment dicts], bytes) of the "params" (theta, and one row of pop), "state" or "work" buffer of `cfg`; BeaconEsError with the
    library's text for what it refuses.  No device needed."""
    L = load()
    segs = (EsSeg * MAX_SEGS)()
    k = getattr(L, "bcn_es_%s_layout" % which)(C.byref(cfg), segs, MAX_SEGS)
    nbytes = getattr(L, "bcn_es_%s_bytes" % which)(C.byref(cfg))
    if k == 0 or nbytes == 0:
        raise BeaconEsError("libbeacon_es: %s" % L.bcn_es_last_error().decode())
    return ([dict(name=g.name.decode(), offset=int(g.offset), elem=int(g.elem), planes=int(g.planes), row_elems=int(g.row_elems))
             for g in segs[:k]], int(nbytes))


# ---- the agent ---------------------------------------------------------------------------
class ES(object):
    """Evolution strategies (Salimans et al. 2017: antithetic Gaussian perturbations, centred ranks, Adam) on the device for one VecEnv
    with a Box or a Discrete action space (include/beacon_es.h states every formula, order and stream; csrc/es/es_impl.h is the
    kernels).

        agent = ES(env, members=None, hidden=(64, 64), activation="tanh", sigma=0.05, lr=0.01, weight_decay=0.0, seed=None)
        agent.load_modules(pi)                      # nn.Sequential: obs_dim -> ... -> act_dim (or n actions) -> theta
        for generation in range(n):
            env.reset(); agent.begin()
            for _ in range(T):
                env.step_autoreset(agent.act()); agent.observe()
            agent.update()                          # the next begin() draws generation gen + 1
        agent.act(shared=True)                      # theta itself on every replica, for evaluation

    `members` M defaults to env.batch (one replica per member); otherwise it is even and divides the batch, and replica b runs member
    b // R, R = batch / M.  pi maps obs_dim -> act_dim with a = c + h tanh(head) (Box: c, h the centre and half width, TD3's
    deterministic action) or -> n with the FIRST maximum as the action (Discrete: DQN's greedy action, int32).
    Owns `theta` (one uint8 buffer in the layout of bcn_es_params_layout; `weights` maps the segment names -- pi_w0, pi_b0, ... -- to
    typed views, matrices [out, in]), `pop` ([M, E] of the env dtype, E the elements of theta with the gaps between segments;
    member(p) is the dict of views of row p), `state` (gen int32 [4]: [0] the generation, [1] the Adam steps; fit float64 [B]; len int32
    [B]; alive uint8 [B]; member_fit, util float64 [M]; stats float64 [8]; adam_m, adam_v), `work` (`grad`, `grads` the views of its
    segments) and `actions` ([B, act_dim] of the env dtype, or int32 [B]).  Fresh parameters are zero.
    begin(): ONE launch -- the perturbation of generation gen[0] and fit = 0, len = 0, alive = 1.  act(): ONE launch.  observe(): ONE
    launch -- where a replica is alive its reward is added to its fitness, and done | trunc ends it: the fitness is the return of the
    replica's FIRST episode of the generation.  observe() reads env.rwd, env.done and env.trunc: the RAW rewards, also under
    env.set_normalize (a rank is invariant under the normaliser's scale, and its running statistics would make the fitness of a
    generation depend on the ones before); act() reads env._norm.norm_obs while the env normalises, as the other agents do.
    update(): SEVEN launches -- member fitness, ranks and statistics, the gradient's partial sums, their reduction, its norm, Adam,
    the tick of gen[0] and gen[1].  The hyperparameters are plain attributes and ARGUMENTS of the launches: a captured graph keeps
    what it was recorded with.  max_grad_norm (None or <= 0: off, the default) clips the gradient by its global norm.
    The host reads: stats_dict() (the statistics and the generation counter, two small copies) and best() (stats[best_member]).
    Not covered: per_jet policies and ShardedVecEnv -- ValueError; Boxes with different bounds per component -- ValueError; fitness
    shaping other than centred ranks; CMA-ES and natural ES (a full covariance); novelty search; observation statistics shared
    across members (virtual batch normalisation); mirrored sampling across generations; more than 16384 members."""

    def __init__(self, env, members=None, hidden=(64, 64), activation="tanh", sigma=0.05, lr=0.01, weight_decay=0.0, seed=None,
                 betas=(0.9, 0.999), eps_adam=1e-8, max_grad_norm=None, group=0, per_jet=False):
        if per_jet:
            raise ValueError("ES: per_jet policies are not covered: a member's policy serves the whole replica")
        if type(env).__name__ == "ShardedVecEnv" or hasattr(env, "global_batch"):
            raise ValueError("ES: ShardedVecEnv is not covered: the agent's buffers live on one device")
        try:
            hid = [int(h) for h in hidden]
            ok = all(int(h) == h and not isinstance(h, bool) for h in hidden)
        except (TypeError, ValueError):
            hid, ok = [], False
        if not ok or not 1 <= len(hid) <= _actor.MAX_LAYERS or any(not 1 <= h <= _actor.MAX_HIDDEN for h in hid):
            raise ValueError("ES: hidden must be 1 .. %d integer widths of 1 .. %d, got %r" % (_actor.MAX_LAYERS, _actor.MAX_HIDDEN, hidden))
        if activation not in _actor._ACTIVATIONS:
            raise ValueError("ES: activation must be 'tanh' or 'relu', got %r" % (activation,))
        space = getattr(env, "action_space", None)
        if space is None:
            raise ValueError("ES: env has no action_space")
        obs_dim, batch = int(env.obs_dim), int(env.batch)
        low, high = -1.0, 1.0
        if getattr(env, "action_is_int", False) and hasattr(space, "n"):
            kind, n_out = DISCRETE, int(space.n)
            if not 2 <= n_out <= MAX_ACT:
                raise ValueError("ES: env.action_space has %d actions; the head takes 2 .. %d" % (n_out, MAX_ACT))
        elif hasattr(space, "low") and hasattr(space, "high"):
            lo, hi = np.asarray(space.low, dtype=np.float64).reshape(-1), np.asarray(space.high, dtype=np.float64).reshape(-1)
            kind, n_out = BOX, int(lo.size)
            if not 1 <= n_out <= MAX_ACT:
                raise ValueError("ES: env.action_space has %d components; the policy takes 1 .. %d" % (n_out, MAX_ACT))
            if np.any(lo != lo[0]) or np.any(hi != hi[0]) or not np.isfinite(lo[0]) or not np.isfinite(hi[0]) or not lo[0] <= hi[0]:
                raise ValueError("ES: env.action_space must be one finite scalar bound pair for all components")
            low, high = float(lo[0]), float(hi[0])
        else:
            raise ValueError("ES: env.action_space is neither a Box nor a Discrete space")
        if not 1 <= obs_dim <= MAX_OBS:
            raise ValueError("ES: env.obs_dim = %d; the network reads rows of at most %d" % (obs_dim, MAX_OBS))
        if members is None:
            members = batch
        if isinstance(members, bool) or not isinstance(members, (int, np.integer)):
            raise ValueError("ES: members must be an integer, got %r" % (members,))
        members = int(members)
        if members < 2 or members % 2 or members > MAX_MEMBERS:
            raise ValueError("ES: members = %d; the population is antithetic pairs: an even number in 2 .. %d" % (members, MAX_MEMBERS))
        if batch % members:
            raise ValueError("ES: members = %d does not divide env.batch = %d: every member runs the same number of replicas" % (members, batch))
        if isinstance(group, bool) or not isinstance(group, (int, np.integer)) or not 0 <= int(group) <= MAX_GROUP:
            raise ValueError("ES: group must be an integer in 0 .. %d (0: the library chooses), got %r" % (MAX_GROUP, group))
        self.env = env
        self.batch, self.members, self.replicas, self.obs_dim, self.tdtype, self.device = batch, members, batch // members, obs_dim, env.tdtype, torch.device(env.device)
        self.kind, self.n_out, self.low, self.high = kind, n_out, low, high
        self.act_dim = n_out if kind == BOX else 1
        self.hidden, self.activation = tuple(hid), activation
        self.set_hyper(sigma=sigma, lr=lr, weight_decay=weight_decay, betas=betas, eps_adam=eps_adam, max_grad_norm=max_grad_norm)
        dt = 1 if self.tdtype == torch.float64 else 0
        self.cfg = make_cfg(batch, members, obs_dim, kind, n_out, dt, hid, activation, low, high, int(group))
        self.lib = load()
        self.params_layout, nbytes = layout("params", self.cfg)
        self.state_layout, sbytes = layout("state", self.cfg)          # (the first call that checks batch, members and the LDS sum)
        self.theta = torch.zeros((nbytes,), dtype=torch.uint8, device=self.device)
        self.n_elems = nbytes // (8 if dt else 4)
        self.pop = torch.zeros((members, self.n_elems), dtype=self.tdtype, device=self.device)
        self.shapes = {}
        dims = [obs_dim] + hid + [n_out]
        for l in range(len(hid) + 1):
            self.shapes["pi_w%d" % l] = (dims[l + 1], dims[l])
            self.shapes["pi_b%d" % l] = (dims[l + 1],)
        self.weights = {k: v.view(self.shapes[k]) for k, v in _views(self.theta, self.params_layout, self.tdtype).items()}
        self.state = torch.zeros((sbytes,), dtype=torch.uint8, device=self.device)
        v = _views(self.state, self.state_layout, self.tdtype)
        self.gen, self.fit, self.len, self.alive = v["gen"], v["fit"], v["len"], v["alive"]
        self.member_fit, self.util, self.stats, self.adam_m, self.adam_v = v["member_fit"], v["util"], v["stats"], v["adam_m"], v["adam_v"]
        self.work_layout, wbytes = layout("work", self.cfg)
        self.work = torch.zeros((wbytes,), dtype=torch.uint8, device=self.device)
        self.grad = _views(self.work, self.work_layout, self.tdtype)["grad"]
        self.grads = {k: g.view(self.shapes[k]) for k, g in _views(self.grad.view(torch.uint8), self.params_layout, self.tdtype).items()}
        if kind == BOX:
            self.actions = torch.zeros((batch, n_out), dtype=self.tdtype, device=self.device)
        else:
            self.actions = torch.zeros((batch,), dtype=torch.int32, device=self.device)
        self.group = int(self.lib.bcn_es_group(C.byref(self.cfg)))
        self.lds_bytes = int(self.lib.bcn_es_lds_bytes(C.byref(self.cfg)))
        self._keep = None
        if seed is None:
            seed = getattr(env, "seed", None) if isinstance(getattr(env, "seed", None), (int, np.integer)) else 0
        self.set_seed(seed)

    _HYPER = ("sigma", "lr", "weight_decay", "betas", "eps_adam", "max_grad_norm")

    def set_hyper(self, **kw):
        """Check and set hyperparameters by name (sigma, lr, weight_decay, betas, eps_adam, max_grad_norm).  ValueError names the
        field; nothing is set then.  sigma = 0 is legal for begin() (pop == theta) and refused by update()."""
        new = {}
        for k, x in kw.items():
            if k in ("sigma", "lr", "weight_decay"):
                new[k] = _number("ES", k, x, lo=0.0)
            elif k == "eps_adam":            # > 0: Adam runs over the gaps of theta too, where the step is 0 / (0 + eps)
                new[k] = _number("ES", k, x, lo=0.0, lo_open=True)
            elif k == "max_grad_norm":
                new[k] = 0.0 if x is None else _number("ES", k, x)
            elif k == "betas":
                try:
                    b1, b2 = x
                except (TypeError, ValueError):
                    raise ValueError("ES: betas must be a pair of numbers in [0, 1), got %r" % (x,))
                new[k] = (_number("ES", "betas[0]", b1, lo=0.0, hi=1.0), _number("ES", "betas[1]", b2, lo=0.0, hi=1.0))
            else:
                raise ValueError("ES: unknown hyperparameter %r" % (k,))
        for k, x in new.items():
            setattr(self, k, x)
        return self

    def set_seed(self, seed):
        """Key the perturbation stream by `seed`.  The generation counter gen[0] stays: (seed, generation) names a population."""
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
            raise ValueError("ES.set_seed: seed must be an integer in [0, 2^64), got %r" % (seed,))
        self.seed = int(seed)
        return self

    # -- parameters -------------------------------------------------------------------------
    def load(self, pi):
        """Copy the network into theta: pi = [(W, b), ...] for the hidden layers and the head, W [out, in].  ValueError for a wrong
        count or shape; nothing is written then.  pop keeps what it holds until the next begin()."""
        if pi is None or len(pi) != len(self.hidden) + 1:
            raise ValueError("ES.load: pi must be %d (W, b) pairs" % (len(self.hidden) + 1))
        todo = []
        for l, (W, b) in enumerate(pi):
            W, b = torch.as_tensor(W), torch.as_tensor(b)
            want = self.shapes["pi_w%d" % l]
            if tuple(W.shape) != want or b.numel() != want[0]:
                raise ValueError("ES.load: pi[%d] must be W [%d, %d] and b [%d], got %s and %s"
                                 % (l, want[0], want[1], want[0], tuple(W.shape), tuple(b.shape)))
            todo += [("pi_w%d" % l, W), ("pi_b%d" % l, b.reshape(-1))]
        with torch.no_grad():
            for name, t in todo:
                self.weights[name].copy_(t.detach().to(device=self.device, dtype=self.tdtype))
        return self

    def load_modules(self, pi):
        """load() from a torch.nn.Sequential of Linear layers with this agent's activation between them (Tanh / ReLU); the squashing
        of a Box action and the argmax of a Discrete one are the library's and no part of the module."""
        import torch.nn as nn
        want = nn.Tanh if self.activation == "tanh" else nn.ReLU
        out = []
        for sub in pi:
            if isinstance(sub, nn.Linear):
                if sub.bias is None:
                    raise ValueError("ES.load_modules: pi has a Linear without bias")
                out.append((sub.weight, sub.bias))
            elif not isinstance(sub, want):
                raise ValueError("ES.load_modules: pi holds a %s; expected Linear and %s only" % (type(sub).__name__, want.__name__))
        return self.load(out)

    def member(self, p):
        """{segment name: view} of row p of `pop`, matrices [out, in]."""
        if isinstance(p, bool) or not isinstance(p, (int, np.integer)) or not 0 <= int(p) < self.members:
            raise ValueError("ES.member: p must be an integer in 0 .. %d, got %r" % (self.members - 1, p))
        row = self.pop[int(p)].view(torch.uint8)
        return {k: v.view(self.shapes[k]) for k, v in _views(row, self.params_layout, self.tdtype).items()}

    def best(self):
        """{segment name: tensor}: a copy of the member that stats[best_member] of the last update() names (a host read)."""
        return {k: v.clone() for k, v in self.member(int(self.stats[4].item())).items()}

    def state_dict(self):
        """For checkpoints: the three buffers on the CPU, what they were laid out for, the seed and the hyperparameters."""
        return {"theta": self.theta.cpu(), "pop": self.pop.cpu(), "state": self.state.cpu(), "batch": self.batch, "members": self.members,
                "obs_dim": self.obs_dim, "kind": self.kind, "n_out": self.n_out, "dtype": "f64" if self.tdtype == torch.float64 else "f32",
                "hidden": self.hidden, "activation": self.activation, "seed": self.seed, "hyper": {k: getattr(self, k) for k in self._HYPER}}

    def load_state_dict(self, d):
        keys = ("batch", "members", "obs_dim", "kind", "n_out", "dtype", "activation")
        cur = {"batch": self.batch, "members": self.members, "obs_dim": self.obs_dim, "kind": self.kind, "n_out": self.n_out,
               "dtype": "f64" if self.tdtype == torch.float64 else "f32", "activation": self.activation}
        if (any(d.get(k) != cur[k] for k in keys) or tuple(d.get("hidden", ())) != self.hidden or d["theta"].numel() != self.theta.numel()
                or d["state"].numel() != self.state.numel()):
            raise ValueError("ES.load_state_dict: the state is of another agent (%s, hidden %s); this one is %s, hidden %s"
                             % ({k: d.get(k) for k in keys}, tuple(d.get("hidden", ())), cur, self.hidden))
        self.set_hyper(**d["hyper"])
        self.theta.copy_(d["theta"])
        self.pop.copy_(d["pop"])
        self.state.copy_(d["state"])
        self.seed = int(d["seed"])
        return self

    # -- launches ---------------------------------------------------------------------------
    def _stream(self):
        if self.device.type != "cuda":
            raise RuntimeError("ES: the launches need a ROCm device (no CPU fallback); this agent's env is on %s" % self.device)
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def begin(self):
        """ONE launch: pop = theta +- sigma eps of generation gen[0], and fit = 0, len = 0, alive = 1.  Returns self."""
        _check(self.lib.bcn_es_begin(C.byref(self.cfg), _p(self.theta), _p(self.pop), _p(self.state), self.sigma, self.seed, self._stream()))
        return self

    def act(self, obs=None, mask=None, shared=False):
        """ONE launch on the current stream, no host synchronisation, nothing allocated: replica b's action from `obs` ([B, obs_dim];
        default: what the env's last reset() / step() returned -- env._norm.norm_obs while it normalises, else env.obs) under member
        b // R of `pop`, or under theta itself with shared=True, into `actions`, which it returns.  `mask` ([B] bool / uint8):
        replicas with 0 keep their action."""
        env = self.env
        if obs is None:
            obs = env._norm.norm_obs if getattr(env, "_norm_on", False) else env.obs
        if (not torch.is_tensor(obs) or obs.dtype != self.tdtype or obs.device != self.device or not obs.is_contiguous()
                or tuple(obs.shape) != (self.batch, self.obs_dim)):
            raise ValueError("ES.act: obs must be a contiguous %s tensor [%d, %d] on %s"
                             % ("f64" if self.tdtype == torch.float64 else "f32", self.batch, self.obs_dim, self.device))
        m = None
        if mask is not None:
            if not torch.is_tensor(mask):
                mask = torch.as_tensor(np.asarray(mask))
            if mask.numel() != self.batch:
                raise ValueError("ES.act: mask must hold %d values" % self.batch)
            m = mask.to(device=self.device, dtype=torch.uint8).reshape(self.batch).contiguous()
        stream = self._stream()
        self._keep = (obs, m)                # alive behind the asynchronous launch
        _check(self.lib.bcn_es_act(C.byref(self.cfg), _p(self.theta if shared else self.pop), 1 if shared else 0, _p(obs), _p(m),
                                   _p(self.actions), stream))
        return self.actions

    def observe(self, rwd=None, done=None, trunc=None):
        """ONE launch: where alive, fit += rwd, len += 1, and done | trunc ends the replica's generation.  Defaults: env.rwd, env.done,
        env.trunc -- the RAW rewards of the last step, also while the env normalises.  Returns self."""
        env = self.env
        rwd = env.rwd if rwd is None else rwd
        done = env.done if done is None else done
        trunc = env.trunc if trunc is None else trunc
        if (not torch.is_tensor(rwd) or rwd.dtype != self.tdtype or rwd.device != self.device or not rwd.is_contiguous() or rwd.numel() != self.batch):
            raise ValueError("ES.observe: rwd must be a contiguous %s tensor [%d] on %s"
                             % ("f64" if self.tdtype == torch.float64 else "f32", self.batch, self.device))
        flags = []
        for name, t in (("done", done), ("trunc", trunc)):
            if not torch.is_tensor(t) or t.device != self.device or t.numel() != self.batch or t.dtype not in (torch.uint8, torch.bool) or not t.is_contiguous():
                raise ValueError("ES.observe: %s must be a contiguous bool / uint8 tensor [%d] on %s" % (name, self.batch, self.device))
            flags.append(t.view(torch.uint8) if t.dtype == torch.bool else t)
        stream = self._stream()
        self._keep = (rwd, flags[0], flags[1])
        _check(self.lib.bcn_es_observe(C.byref(self.cfg), _p(self.state), _p(rwd), _p(flags[0]), _p(flags[1]), stream))
        return self

    def hyper(self):
        return EsHyper(sigma=self.sigma, lr=self.lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps_adam,
                       max_grad_norm=self.max_grad_norm, weight_decay=self.weight_decay)

    def update(self):
        """SEVEN launches: ranks and statistics of the generation's fitness, the gradient estimate from regenerated noise, Adam on
        theta, and the tick of the generation counter.  No host synchronisation, nothing allocated.  Returns self."""
        if not self.sigma > 0.0:
            raise ValueError("ES.update: sigma = %r; the gradient estimate divides by it" % (self.sigma,))
        h = self.hyper()
        _check(self.lib.bcn_es_update(C.byref(self.cfg), _p(self.theta), _p(self.state), _p(self.work), C.byref(h), self.seed, self._stream()))
        return self

    def stats_dict(self):
        """The statistics of the last update() as a dict of floats, and `generation` (gen[0]): two small device-to-host copies."""
        d = dict(zip(STATS, self.stats.cpu().tolist()))
        d["generation"] = int(self.gen[0].item())
        return d
