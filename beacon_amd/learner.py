"""The PPO update of an on-device actor: libbeacon_learner.so (include/beacon_learner.h; csrc/learner/) and the class Learner over it.

Learner.grad computes the clipped-surrogate loss of a minibatch and its gradient with respect to every parameter of an Actor
(three launches: backward into per-workgroup slabs, the reduction in a fixed order, the norm); Learner.step applies Adam to
actor.params in place (two launches: the update and the tick of the device-side step counter).  No host synchronisation, no
allocation, no atomics: every buffer is bit-reproducible, and both calls can be captured in a graph.  Learner.update is the
convenience over a Rollout the actor is attached to.

The library is a unit of its own, built and bound like the actor's (build.py: one Unit each); its table is SIGNATURES below.  Importing this
module touches neither a compiler nor the GPU."""
import ctypes as C
import os

import numpy as np
import torch

from . import actor as _actor
from . import build as _build

API_VERSION = 1                           # include/beacon_learner.h: BCN_LEARNER_API_VERSION
# the float64 unit: one rounding per written operation, as actor_f64.hip
FILE_FLAGS = {"learner.hip": [],
              "learner_f64.hip": ["-ffp-contract=off"]}
W_NONE, W_U8, W_REAL = 0, 1, 2
F64 = 3                                   # BCN_LEARNER_F64, the element type of the statistics
MAX_GRID = 256
STATS = ("loss", "pg_loss", "vf_loss", "entropy", "approx_kl", "clip_frac", "weight", "grad_norm")
_vp = C.c_void_p


class LearnerBatch(C.Structure):
    """bcn_learner_batch"""
    _fields_ = [("obs", _vp), ("act", _vp), ("logp_old", _vp), ("adv", _vp), ("ret", _vp), ("weight", _vp), ("idx", _vp), ("cursor", _vp),
                ("n_rows", C.c_int64), ("m", C.c_int64), ("weight_kind", C.c_int32), ("rows_per_step", C.c_int32),
                ("rows_per_weight", C.c_int32)]     # appended: consecutive rows that share one weight, 0 means 1


class LearnerLoss(C.Structure):
    """bcn_learner_loss"""
    _fields_ = [("clip", C.c_double), ("vf_coef", C.c_double), ("ent_coef", C.c_double)]


class LearnerAdam(C.Structure):
    """bcn_learner_adam"""
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("max_grad_norm", C.c_double),
                ("target_kl", C.c_double), ("lr_end", C.c_double), ("lr_steps", C.c_double)]     # appended: the KL stop rule and the lr schedule, 0 means none


_cfgp, _segp = C.POINTER(_actor.ActorCfg), C.POINTER(_actor.ActorSeg)
# every symbol include/beacon_learner.h declares: (restype, argtypes)
SIGNATURES = {
    "bcn_learner_grad_layout": (C.c_int, [_cfgp, _segp, C.c_int]),
    "bcn_learner_grad_bytes": (C.c_size_t, [_cfgp]),
    "bcn_learner_opt_layout": (C.c_int, [_cfgp, _segp, C.c_int]),
    "bcn_learner_opt_bytes": (C.c_size_t, [_cfgp]),
    "bcn_learner_work_layout": (C.c_int, [_cfgp, _segp, C.c_int]),
    "bcn_learner_work_bytes": (C.c_size_t, [_cfgp]),
    "bcn_learner_grid": (C.c_int, [_cfgp]),
    "bcn_learner_grad": (C.c_int, [_cfgp, _vp, C.POINTER(LearnerBatch), C.POINTER(LearnerLoss), _vp, _vp, _vp]),
    "bcn_learner_step": (C.c_int, [_cfgp, _vp, _vp, _vp, _vp, C.POINTER(LearnerAdam), _vp]),
    "bcn_learner_last_error": (C.c_char_p, []),
}


class BeaconLearnerError(RuntimeError):
    pass


# ---- the library -------------------------------------------------------------------------
# (the units include the network both libraries run, csrc/actor/policy_net.h, and the actor's kernel header that brings it: the
# dependency rule of build.py follows the #include lines there)
SRC_DIR, HEADER = os.path.join(_build.CSRC, "learner"), os.path.join(_build.INC, "beacon_learner.h")
LIB, OBJ = os.path.join(_build.PKG, "libbeacon_learner.so"), os.path.join(_build.OBJ, "learner")
_UNIT = _build.hip_library(LIB, SRC_DIR, FILE_FLAGS, OBJ, SIGNATURES)
sources, signature, stale, load = _UNIT.sources, _UNIT.signature, _UNIT.stale, _UNIT.load


def build_learner(force=False, verbose=False):
    """Compile csrc/learner/*.hip for gfx950 and link libbeacon_learner.so.  Returns its path."""
    return _UNIT.build(force=force, verbose=verbose)


def _check(rc):
    if rc != 0:
        raise BeaconLearnerError("libbeacon_learner: error %d: %s" % (rc, load().bcn_learner_last_error().decode()))


def layout(which, cfg):
    """([segment dicts], bytes) of the "grad", "opt" or "work" buffer of `cfg` (an actor.make_cfg); BeaconLearnerError with the
    library's text for a cfg it refuses.  No device needed."""
    L = load()
    segs = (_actor.ActorSeg * _actor.MAX_SEGS)()
    k = getattr(L, "bcn_learner_%s_layout" % which)(C.byref(cfg), segs, _actor.MAX_SEGS)
    nbytes = getattr(L, "bcn_learner_%s_bytes" % which)(C.byref(cfg))
    if k == 0 or nbytes == 0:
        raise BeaconLearnerError("libbeacon_learner: %s" % L.bcn_learner_last_error().decode())
    return ([dict(name=g.name.decode(), offset=int(g.offset), elem=int(g.elem), planes=int(g.planes), row_elems=int(g.row_elems))
             for g in segs[:k]], int(nbytes))


def _seg_view(buf, seg, real):
    dt = {0: real, 1: torch.int32, 2: torch.int32, F64: torch.float64}[seg["elem"]]
    n = seg["row_elems"] * torch.empty((), dtype=dt).element_size()
    return buf[seg["offset"]:seg["offset"] + n].view(dt)


def _number(name, x, lo=None, lo_open=False, hi=None):
    if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not np.isfinite(x):
        raise ValueError("Learner: %s must be a finite number, got %r" % (name, x))
    x = float(x)
    if lo is not None and (x <= lo if lo_open else x < lo):
        raise ValueError("Learner: %s must be %s %g, got %r" % (name, ">" if lo_open else ">=", lo, x))
    if hi is not None and x >= hi:
        raise ValueError("Learner: %s must be < %g, got %r" % (name, hi, x))
    return x


# ---- the class ---------------------------------------------------------------------------
class Learner(object):
    """PPO on the device for one Actor (include/beacon_learner.h states the loss, the gradient and Adam; csrc/learner/learner_impl.h
    is the kernels).

        learner = Learner(actor, lr=3e-4)
        ... the rollout of Actor's docstring ...
        adv, ret = ro.compute_gae(actor.value_seq, actor.values(env.obs), ...)
        learner.update(ro, adv, ret, epochs=10, minibatches=4)         # actor.params are the new policy; the next act() uses them

    Owns `grad` (one uint8 buffer in the layout of the actor's parameters; `grads` maps the segment names to typed views shaped as
    actor.weights), `opt` (the Adam moments `m`, `v` as flat views over the whole parameter buffer and `step_count`, int32 [4]:
    [0] the steps taken, advanced on the device, [1] the permutations a plan has drawn, [2] the KL stop flag, [3] the steps it
    skipped) and `work` (the slabs; `stats`: float64 [8] on the device -- loss, pg loss, value loss, entropy, approx_kl, clip_frac,
    W, the gradient norm before clipping -- read by stats_dict(), the only host read).
    The hyperparameters are plain attributes (lr, clip_range, vf_coef, ent_coef, max_grad_norm, betas, eps, target_kl, lr_end,
    lr_steps): they are ARGUMENTS of the launches, so a captured graph keeps what it was recorded with.  max_grad_norm <= 0 or
    None: no clipping.
    A per-jet actor (Actor(env, per_jet=True)) is updated the same way: update() then takes adv / ret of
    ro.compute_gae(..., per_jet=True), every (step, replica, jet) is a row and the rollout's per-replica `valid` bytes weigh all
    jets of their replica (grad's rows_per_weight).
    Two hyperparameters are decided ON THE DEVICE and so keep working when a captured update is replayed (include/beacon_learner.h):
    target_kl (None or 0: off) -- step() applies no minibatch whose approx_kl exceeds 1.5 target_kl and none behind it until the
    next plan.run() clears the flag (step_count[2]; `skipped` reads step_count[3], the steps not taken); lr_steps > 0 -- the rate
    goes linearly from lr to lr_end over lr_steps steps taken, read from step_count[0].
    learner.plan(ro, epochs, minibatches) is the update as a chain of the library's own launches (beacon_amd/epochs.py).
    Not covered: ShardedVecEnv (no gradient all-reduce), value clipping."""

    def __init__(self, actor, lr=3e-4, clip_range=0.2, vf_coef=0.5, ent_coef=0.0, max_grad_norm=0.5, betas=(0.9, 0.999), eps=1e-8,
                 target_kl=None, lr_end=0.0, lr_steps=0):
        if not isinstance(actor, _actor.Actor):
            raise ValueError("Learner: actor must be a beacon_amd.Actor, got %r" % (type(actor).__name__,))
        self.actor = actor
        self.set_hyper(lr=lr, clip_range=clip_range, vf_coef=vf_coef, ent_coef=ent_coef, max_grad_norm=max_grad_norm, betas=betas, eps=eps,
                       target_kl=target_kl, lr_end=lr_end, lr_steps=lr_steps)
        self.cfg, self.tdtype, self.device = actor.cfg, actor.tdtype, actor.device
        self.lib = load()
        self.grad_layout, nbytes = layout("grad", self.cfg)
        if [(s["name"], s["offset"], s["row_elems"]) for s in self.grad_layout] != [(s["name"], s["offset"], s["row_elems"]) for s in actor.params_layout] \
                or nbytes != actor.params.numel():
            raise BeaconLearnerError("libbeacon_learner and libbeacon_actor disagree on the parameter layout")
        self.grad_buf = torch.zeros((nbytes,), dtype=torch.uint8, device=self.device)
        self.grads = {s["name"]: _seg_view(self.grad_buf, s, self.tdtype).view(actor.weights[s["name"]].shape) for s in self.grad_layout}
        self.opt_layout, nbytes = layout("opt", self.cfg)
        self.opt = torch.zeros((nbytes,), dtype=torch.uint8, device=self.device)
        self.m, self.v, self.step_count = (_seg_view(self.opt, s, self.tdtype) for s in self.opt_layout)
        self.work_layout, nbytes = layout("work", self.cfg)
        self.work = torch.zeros((nbytes,), dtype=torch.uint8, device=self.device)
        self.stats = _seg_view(self.work, self.work_layout[0], self.tdtype)
        self.grid = int(self.lib.bcn_learner_grid(C.byref(self.cfg)))
        self._keep = None

    def set_hyper(self, **kw):
        """Check and set hyperparameters by name (those of the constructor).  ValueError names the field; nothing is set then."""
        new = {}
        for k, x in kw.items():
            if k == "lr":
                new[k] = _number("lr", x, lo=0.0)
            elif k == "clip_range":
                new[k] = _number("clip_range", x, lo=0.0)
            elif k in ("vf_coef", "ent_coef"):
                new[k] = _number(k, x)
            elif k == "eps":
                new[k] = _number("eps", x, lo=0.0)
            elif k == "max_grad_norm":
                new[k] = 0.0 if x is None else _number("max_grad_norm", x)
            elif k == "target_kl":
                new[k] = 0.0 if x is None else _number("target_kl", x, lo=0.0)
            elif k in ("lr_end", "lr_steps"):
                new[k] = _number(k, x, lo=0.0)
            elif k == "betas":
                try:
                    b1, b2 = x
                except (TypeError, ValueError):
                    raise ValueError("Learner: betas must be a pair of numbers in [0, 1), got %r" % (x,))
                new[k] = (_number("betas[0]", b1, lo=0.0, hi=1.0), _number("betas[1]", b2, lo=0.0, hi=1.0))
            else:
                raise ValueError("Learner: unknown hyperparameter %r" % (k,))
        for k, x in new.items():
            setattr(self, k, x)
        return self

    # -- launches ---------------------------------------------------------------------------
    def _stream(self):
        if self.device.type != "cuda":
            raise RuntimeError("Learner: the launches need a ROCm device (no CPU fallback); this learner's actor is on %s" % self.device)
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _vec(self, name, t, n, dtype=None, cols=None):
        dtype = dtype or self.tdtype
        if (not torch.is_tensor(t) or t.dtype != dtype or t.device != self.device or not t.is_contiguous()
                or t.numel() != n * (cols or 1)):
            raise ValueError("Learner.grad: %s must be a contiguous %s tensor of %d%s elements on %s"
                             % (name, str(dtype).replace("torch.", ""), n, " x %d" % cols if cols else "", self.device))
        return t

    def grad(self, obs_rows, actions, logp_old, adv, ret, weight=None, idx=None, _cursor=None, _rows_per_step=0, rows_per_weight=1):
        """Loss, statistics and gradient of one minibatch: THREE launches on the current stream, no host synchronisation, nothing
        allocated.  obs_rows [N, obs_dim]; actions [N, act_dim] (Gaussian: the unclipped samples, actor.raw_seq) or int32 [N]
        (categorical); logp_old, adv, ret [N] (any shape with N elements); weight: None (all 1), or uint8 / bool / the env dtype
        [N / rows_per_weight], >= 0 (ro.valid is the intended one; rows_per_weight: an integer >= 1 that divides N -- row s takes
        weight[s // rows_per_weight], so the n_jets rows of a replica share its one `valid` byte); idx: None -- the minibatch is all N rows -- or an int32 tensor of row numbers:
        the minibatch is those rows, gathered on the device while staging.  Rows of weight 0 may hold anything, NaN included.
        Contiguous device tensors of the env dtype.  Returns (grads, stats): {segment name: view of the gradient buffer} and the
        float64 [8] statistics ON THE DEVICE (stats_dict() reads them).  ValueError for a wrong shape, dtype or device, before any
        launch."""
        a = self.actor
        if not torch.is_tensor(obs_rows) or obs_rows.dim() != 2 or obs_rows.shape[1] != a.obs_dim or obs_rows.shape[0] < 1:
            raise ValueError("Learner.grad: obs_rows must be a contiguous tensor [N >= 1, %d] of the env dtype on %s" % (a.obs_dim, self.device))
        N = int(obs_rows.shape[0])
        self._vec("obs_rows", obs_rows, N, cols=a.obs_dim)
        if a.kind == _actor.CATEGORICAL:
            self._vec("actions", actions, N, dtype=torch.int32)
        else:
            self._vec("actions", actions, N, cols=a.act_dim)
        self._vec("logp_old", logp_old, N)
        self._vec("adv", adv, N)
        self._vec("ret", ret, N)
        if isinstance(rows_per_weight, bool) or not isinstance(rows_per_weight, (int, np.integer)) or rows_per_weight < 1 \
                or N % int(rows_per_weight):
            raise ValueError("Learner.grad: rows_per_weight must be an integer >= 1 that divides the %d rows, got %r" % (N, rows_per_weight))
        rpw = int(rows_per_weight)
        wk = W_NONE
        if weight is not None:
            if torch.is_tensor(weight) and weight.dtype == torch.bool:
                weight = weight.view(torch.uint8)
            wk = W_U8 if torch.is_tensor(weight) and weight.dtype == torch.uint8 else W_REAL
            self._vec("weight", weight, N // rpw, dtype=torch.uint8 if wk == W_U8 else self.tdtype)
        m = N
        if idx is not None:
            if not torch.is_tensor(idx) or idx.dtype != torch.int32 or idx.device != self.device or not idx.is_contiguous() or idx.dim() != 1 \
                    or idx.numel() < 1:
                raise ValueError("Learner.grad: idx must be a contiguous 1-D int32 tensor of at least one row number on %s" % self.device)
            m = int(idx.numel())
        stream = self._stream()
        self._keep = (obs_rows, actions, logp_old, adv, ret, weight, idx, _cursor)      # alive behind the asynchronous launches
        p = _actor._ptr
        b = LearnerBatch(obs=p(obs_rows), act=p(actions), logp_old=p(logp_old), adv=p(adv), ret=p(ret), weight=p(weight), idx=p(idx),
                         cursor=p(_cursor), n_rows=N, m=m, weight_kind=wk, rows_per_step=int(_rows_per_step), rows_per_weight=rpw)
        loss = LearnerLoss(clip=self.clip_range, vf_coef=self.vf_coef, ent_coef=self.ent_coef)
        _check(self.lib.bcn_learner_grad(C.byref(self.cfg), p(a.params), C.byref(b), C.byref(loss), p(self.grad_buf), p(self.work), stream))
        return self.grads, self.stats

    def step(self):
        """One Adam step on actor.params IN PLACE from the gradient of the last grad(), clipped to max_grad_norm: TWO launches on the
        current stream, no host synchronisation.  The step counter advances on the device.  Under target_kl the step may be
        skipped there, and with lr_steps its rate comes from the counter (the class docstring)."""
        stream = self._stream()
        p = _actor._ptr
        h = LearnerAdam(lr=self.lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, max_grad_norm=self.max_grad_norm,
                        target_kl=self.target_kl, lr_end=self.lr_end, lr_steps=self.lr_steps)
        _check(self.lib.bcn_learner_step(C.byref(self.cfg), p(self.actor.params), p(self.grad_buf), p(self.opt), p(self.work), C.byref(h), stream))
        return self

    def stats_dict(self):
        """The statistics of the last grad() as a dict of floats: the one host read."""
        return dict(zip(STATS, self.stats.cpu().tolist()))

    def update(self, ro, adv, ret, epochs=10, minibatches=4, normalize_adv=True, generator=None):
        """PPO epochs over the Rollout `ro` this learner's actor is attached to: obs = ro.obs[:-1], the actions actor.raw_seq
        (Gaussian) or ro.act (categorical), logp_old = actor.logp_seq, the weights ro.valid; adv, ret [T, B] from
        ro.compute_gae.  With normalize_adv the advantages are standardised once over the valid entries of the recorded steps
        (torch ops on the device; mean and the unbiased standard deviation + 1e-8).  Per epoch one torch.randperm of the T B rows
        on the device (`generator`: a torch.Generator of that device, for reproducible minibatches) is cut into `minibatches`
        index ranges, and each gets grad() + step().  Rows of steps the rollout has not recorded get weight 0 ON THE DEVICE, from
        its cursor: the host never reads it.  No host synchronisation.  Returns self.
        With a per-jet actor (A = n_jets) the rows are the T B A (step, replica, jet) triples: obs = ro.obs[:-1] read as
        [T B A, n_obs], the actions actor.raw_seq, adv and ret [T, B A] from ro.compute_gae(..., per_jet=True); ro.valid is passed as
        it is, T B bytes, each weighing the A rows of its replica on the device.  The standardisation pools all jets: a valid step
        counts A times."""
        a = self.actor
        if a.rollout is not ro or ro is None:
            raise ValueError("Learner.update: ro must be the Rollout this learner's actor is attached to")
        for name, x in (("epochs", epochs), ("minibatches", minibatches)):
            if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < 1:
                raise ValueError("Learner.update: %s must be an integer >= 1, got %r" % (name, x))
        T, B, A = int(ro.T), a.batch, a.agents
        N = T * B * A
        if minibatches > N:
            raise ValueError("Learner.update: %d minibatches of %d rows" % (minibatches, N))
        if A > 1:
            for name, x in (("adv", adv), ("ret", ret)):
                if not torch.is_tensor(x) or x.numel() != N:
                    raise ValueError("Learner.update: with a per-jet actor %s must hold %d x %d x %d elements: pass what "
                                     "ro.compute_gae(..., per_jet=True) returns" % (name, T, B, A))
        self._vec("adv", adv, N)
        self._vec("ret", ret, N)
        self._stream()
        obs = ro.obs[:-1].reshape(N, a.obs_dim)
        actions = ro.act.reshape(N) if a.kind == _actor.CATEGORICAL else a.raw_seq.reshape(N, a.act_dim)
        logp_old = a.logp_seq.reshape(N)
        valid = ro.valid.reshape(T * B)              # per replica: grad's rows_per_weight = A spreads a byte over its A rows
        adv, ret = adv.reshape(N), ret.reshape(N)
        if normalize_adv:
            t = torch.arange(T, device=self.device, dtype=torch.int32).view(T, 1)
            w = valid.view(T, B) * (t < ro.cursor[0])
            if A > 1:
                w = w.view(T, B, 1).expand(T, B, A)
            w = w.reshape(N).to(self.tdtype)
            cnt = w.sum().clamp_(min=1.0)
            mean = (torch.where(w > 0, adv, torch.zeros_like(adv))).sum() / cnt
            var = (torch.where(w > 0, adv - mean, torch.zeros_like(adv)) ** 2).sum() / (cnt - 1.0).clamp_(min=1.0)
            adv = (adv - mean) / (var.sqrt() + 1e-8)
        for _ in range(int(epochs)):
            perm = torch.randperm(N, device=self.device, generator=generator).to(torch.int32)
            for k in range(int(minibatches)):
                idx = perm[k * N // minibatches:(k + 1) * N // minibatches]
                self.grad(obs, actions, logp_old, adv, ret, weight=valid, idx=idx, _cursor=ro.cursor, _rows_per_step=B * A, rows_per_weight=A)
                self.step()
        return self

    def plan(self, ro, epochs=10, minibatches=4, seed=None, normalize_adv=True):
        """The update over `ro` as a chain of the library's own launches, allocated once: an epochs.Plan (plan.run(adv, ret),
        plan.capture(adv, ret)).  update() stays what it is."""
        from . import epochs as _epochs
        return _epochs.Plan(self, ro, epochs=epochs, minibatches=minibatches, seed=seed, normalize_adv=normalize_adv)

    @property
    def skipped(self):
        """The steps the KL stop rule has skipped so far (step_count[3]): a host read."""
        return int(self.step_count[3])

    # -- checkpoints ------------------------------------------------------------------------
    def state_dict(self):
        """For checkpoints: the optimiser buffer on the CPU, what it was laid out for, and the hyperparameters."""
        return {"opt": self.opt.cpu(), "params_bytes": int(self.actor.params.numel()), "dtype": "f64" if self.tdtype == torch.float64 else "f32",
                "lr": self.lr, "clip_range": self.clip_range, "vf_coef": self.vf_coef, "ent_coef": self.ent_coef,
                "max_grad_norm": self.max_grad_norm, "betas": tuple(self.betas), "eps": self.eps,
                "target_kl": self.target_kl, "lr_end": self.lr_end, "lr_steps": self.lr_steps}

    def load_state_dict(self, d):
        dt = "f64" if self.tdtype == torch.float64 else "f32"
        if d["params_bytes"] != self.actor.params.numel() or d["dtype"] != dt or d["opt"].numel() != self.opt.numel():
            raise ValueError("Learner.load_state_dict: the state is of another learner (%d parameter bytes, %s); this one has %d, %s"
                             % (d["params_bytes"], d["dtype"], self.actor.params.numel(), dt))
        # (a state written before there were a stop rule and a schedule has neither)
        self.set_hyper(**{k: d[k] for k in ("lr", "clip_range", "vf_coef", "ent_coef", "max_grad_norm", "betas", "eps")},
                       **{k: d.get(k, 0.0) for k in ("target_kl", "lr_end", "lr_steps")})
        self.opt.copy_(d["opt"])
        return self
