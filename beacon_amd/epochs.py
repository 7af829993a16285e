"""A whole PPO update without the host: libbeacon_epochs.so (include/beacon_epochs.h; csrc/epochs/) and the class Plan over it.

What Learner.update() takes from the framework -- torch.randperm for the minibatches, about ten torch launches for the advantage
standardisation -- is here the library's own: bcn_epochs_permute draws an epoch's shuffle from the project's one Philox definition,
keyed by a seed and counted by a device word, and bcn_epochs_begin standardises the advantages with float64 sums in a fixed order
and clears the learner's KL stop flag.  A Plan strings them together with Learner.grad() and Learner.step(): seeded, restated on the
host (tests/epochs_ref.py), bit-reproducible, and capturable as ONE graph whose replays draw new permutations.

The library is a unit of its own, built and bound like the actor's and the learner's (build.py: one Unit each); its table is
SIGNATURES below.  Importing this module touches neither a compiler nor the GPU."""
import ctypes as C
import os

import numpy as np
import torch

from . import actor as _actor
from . import build as _build
from . import learner as _learner

API_VERSION = 1                           # include/beacon_epochs.h: BCN_EPOCHS_API_VERSION
# one rounding per written operation: the float64 sums are the sequence the header states
FILE_FLAGS = {"epochs.hip": ["-ffp-contract=off"]}
W_NONE, W_U8, W_REAL = 0, 1, 2
F64 = 3                                   # BCN_EPOCHS_F64
GRID, CHUNK, ROUNDS, MAX_SEGS = 64, 1024, 6, 4
MOMENTS = ("mean", "var", "count", "denom")
_vp = C.c_void_p


class EpochsSeg(C.Structure):
    """bcn_epochs_seg"""
    _fields_ = [("name", C.c_char * 16), ("offset", C.c_uint64), ("elem", C.c_int32), ("planes", C.c_int32), ("row_elems", C.c_int64)]


class EpochsBatch(C.Structure):
    """bcn_epochs_batch"""
    _fields_ = [("adv", _vp), ("adv_out", _vp), ("weight", _vp), ("cursor", _vp), ("step", _vp), ("work", _vp),
                ("n_rows", C.c_int64), ("dtype", C.c_int32), ("normalize", C.c_int32), ("weight_kind", C.c_int32),
                ("rows_per_step", C.c_int32), ("rows_per_weight", C.c_int32)]


# every symbol include/beacon_epochs.h declares: (restype, argtypes)
SIGNATURES = {
    "bcn_epochs_work_layout": (C.c_int, [C.POINTER(EpochsSeg), C.c_int]),
    "bcn_epochs_work_bytes": (C.c_size_t, []),
    "bcn_epochs_permute": (C.c_int, [C.c_int64, C.c_uint64, _vp, _vp, _vp]),
    "bcn_epochs_begin": (C.c_int, [C.POINTER(EpochsBatch), _vp]),
    "bcn_epochs_last_error": (C.c_char_p, []),
}


class BeaconEpochsError(RuntimeError):
    pass


# ---- the library -------------------------------------------------------------------------
SRC_DIR, HEADER = os.path.join(_build.CSRC, "epochs"), os.path.join(_build.INC, "beacon_epochs.h")
LIB, OBJ = os.path.join(_build.PKG, "libbeacon_epochs.so"), os.path.join(_build.OBJ, "epochs")
_UNIT = _build.hip_library(LIB, SRC_DIR, FILE_FLAGS, OBJ, SIGNATURES)
sources, signature, stale, load = _UNIT.sources, _UNIT.signature, _UNIT.stale, _UNIT.load


def build_epochs(force=False, verbose=False):
    """Compile csrc/epochs/epochs.hip for gfx950 and link libbeacon_epochs.so.  Returns its path."""
    return _UNIT.build(force=force, verbose=verbose)


def _check(rc):
    if rc != 0:
        raise BeaconEpochsError("libbeacon_epochs: error %d: %s" % (rc, load().bcn_epochs_last_error().decode()))


def work_layout():
    """([segment dicts], bytes) of the work buffer of bcn_epochs_begin.  No device needed."""
    L = load()
    segs = (EpochsSeg * MAX_SEGS)()
    k = L.bcn_epochs_work_layout(segs, MAX_SEGS)
    return ([dict(name=g.name.decode(), offset=int(g.offset), elem=int(g.elem), planes=int(g.planes), row_elems=int(g.row_elems))
             for g in segs[:k]], int(L.bcn_epochs_work_bytes()))


def _count(name, x):
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < 1:
        raise ValueError("Learner.plan: %s must be an integer >= 1, got %r" % (name, x))
    return int(x)


# ---- the class ---------------------------------------------------------------------------
class Plan(object):
    """PPO epochs over a Rollout as a chain of the library's own launches (learner.plan(ro, ...) makes one):

        plan = learner.plan(ro, epochs=10, minibatches=4, seed=7, normalize_adv=True)     # allocates, once
        plan.run(adv, ret)            # what learner.update(ro, adv, ret, ...) does, without torch.randperm and torch arithmetic
        g = plan.capture(adv, ret)    # the same launches in ONE graph; g.replay()

    run(): bcn_epochs_begin (the KL stop flag cleared; with normalize_adv the advantages standardised over the active rows into
    `adv_norm`: three launches, else one); per epoch bcn_epochs_permute into `idx` (the permutation and the tick of its counter,
    learner.step_count[1]) and per minibatch k learner.grad(idx = idx[k N // nmb : (k + 1) N // nmb]) + learner.step().  No host
    synchronisation, nothing allocated; it reads what update() reads of the rollout and the actor -- obs = ro.obs[:-1], the actions
    actor.raw_seq or ro.act, logp_old = actor.logp_seq, the weights ro.valid, the rollout's cursor -- and with a per-jet actor the
    rows are the T B A (step, replica, jet) triples under rows_per_weight = A.
    The permutation of an epoch is a pure function of (N, seed, learner.step_count[1]): tests/epochs_ref.py restates it.  `seed`
    defaults to the actor's (the stream's Philox counters differ from the actor's in their last word).
    Owns `idx` int32 [N], `adv_norm` [N] (with normalize_adv), `work` (bcn_epochs_work_layout; `moments`: float64 [4] on the
    device -- mean, var, the count of active rows, sqrt(var) + 1e-8 of the last standardisation).
    target_kl and the learning-rate schedule are the LEARNER's hyperparameters (Learner.set_hyper), not the plan's: under target_kl
    the steps behind the stopping minibatch of an update are skipped on the device -- their grad() launches still run and move
    nothing -- and the next run() clears the flag."""

    def __init__(self, learner, ro, epochs=10, minibatches=4, seed=None, normalize_adv=True):
        if not isinstance(learner, _learner.Learner):
            raise ValueError("Learner.plan: learner must be a beacon_amd.Learner, got %r" % (type(learner).__name__,))
        self.learner, a = learner, learner.actor
        self.epochs, self.minibatches = _count("epochs", epochs), _count("minibatches", minibatches)
        if seed is None:
            seed = a.seed
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
            raise ValueError("Learner.plan: seed must be an integer in [0, 2^64), got %r" % (seed,))
        if not isinstance(normalize_adv, (bool, np.bool_)):
            raise ValueError("Learner.plan: normalize_adv must be True or False, got %r" % (normalize_adv,))
        if ro is None or a.rollout is not ro:
            raise ValueError("Learner.plan: ro must be the Rollout this learner's actor is attached to")
        self.seed, self.normalize_adv, self.ro = int(seed), bool(normalize_adv), ro
        self.T, self.B, self.A = int(ro.T), a.batch, a.agents
        N = self.N = self.T * self.B * self.A
        if N >= 1 << 31:
            raise ValueError("Learner.plan: %d rows; one permutation covers 2^31 - 1" % N)
        if self.minibatches > N:
            raise ValueError("Learner.plan: %d minibatches of %d rows" % (self.minibatches, N))
        self.lib = load()
        self.tdtype, self.device = learner.tdtype, learner.device
        self.idx = torch.zeros((N,), dtype=torch.int32, device=self.device)
        nmb = self.minibatches
        self._slices = [self.idx[k * N // nmb:(k + 1) * N // nmb] for k in range(nmb)]       # views: made once
        self.adv_norm = torch.zeros((N,), dtype=self.tdtype, device=self.device) if self.normalize_adv else None
        self.work_layout, nbytes = work_layout()
        self.work = torch.zeros((nbytes,), dtype=torch.uint8, device=self.device)
        s = self.work_layout[0]
        self.moments = self.work[s["offset"]:s["offset"] + 8 * s["row_elems"]].view(torch.float64)
        self._keep = None

    def moments_dict(self):
        """The moments of the last standardisation as a dict of floats: a host read."""
        return dict(zip(MOMENTS, self.moments.cpu().tolist()))

    def run(self, adv, ret):
        """The update (the class docstring).  adv, ret: what ro.compute_gae returned, T B (A) elements of the env dtype on the
        device.  ValueError for a wrong shape, dtype or device before any launch.  Returns self."""
        ln, a, ro = self.learner, self.learner.actor, self.ro
        if a.rollout is not ro:
            raise ValueError("Learner.plan: the actor is no longer attached to this plan's Rollout")
        N, A = self.N, self.A
        if A > 1:
            for name, x in (("adv", adv), ("ret", ret)):
                if not torch.is_tensor(x) or x.numel() != N:
                    raise ValueError("Learner.plan: with a per-jet actor %s must hold %d x %d x %d elements: pass what "
                                     "ro.compute_gae(..., per_jet=True) returns" % (name, self.T, self.B, A))
        ln._vec("adv", adv, N)
        ln._vec("ret", ret, N)
        stream = ln._stream()
        obs = ro.obs[:-1].reshape(N, a.obs_dim)
        actions = ro.act.reshape(N) if a.kind == _actor.CATEGORICAL else a.raw_seq.reshape(N, a.act_dim)
        logp_old = a.logp_seq.reshape(N)
        valid = ro.valid.reshape(self.T * self.B)        # per replica: rows_per_weight = A spreads a byte over its A rows
        adv, ret = adv.reshape(N), ret.reshape(N)
        if valid.dtype == torch.bool:
            valid = valid.view(torch.uint8)
        p = _actor._ptr
        self._keep = (adv, ret, valid, ro.cursor)        # alive behind the asynchronous launches
        b = EpochsBatch(adv=p(adv), adv_out=p(self.adv_norm), weight=p(valid), cursor=p(ro.cursor), step=p(ln.step_count), work=p(self.work),
                        n_rows=N, dtype=1 if self.tdtype == torch.float64 else 0, normalize=int(self.normalize_adv),
                        weight_kind=W_U8 if valid.dtype == torch.uint8 else W_REAL, rows_per_step=self.B * A, rows_per_weight=A)
        _check(self.lib.bcn_epochs_begin(C.byref(b), stream))
        used = self.adv_norm if self.normalize_adv else adv
        epoch_word = C.c_void_p(ln.step_count.data_ptr() + 4)                 # step_count[1]
        for _ in range(self.epochs):
            _check(self.lib.bcn_epochs_permute(N, self.seed, epoch_word, p(self.idx), stream))
            for idx in self._slices:
                ln.grad(obs, actions, logp_old, used, ret, weight=valid, idx=idx, _cursor=ro.cursor, _rows_per_step=self.B * A, rows_per_weight=A)
                ln.step()
        return self

    def capture(self, adv, ret):
        """run(adv, ret) recorded as ONE graph; nothing is launched.  Returns the torch.cuda.CUDAGraph: every replay() is an update
        from the buffers' contents at that time, with new permutations (their counter lives on the device), the stop rule and the
        schedule at work.  The learner's hyperparameters are those at the time of the capture."""
        self.learner._stream()
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize(self.device)
        with torch.cuda.graph(g):
            self.run(adv, ret)
        self._graph_keep = (adv, ret)
        return g
