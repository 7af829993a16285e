"""Batched (vectorised) envs: B independent replicas of one beacon env advanced by one HIP
launch per step().  Same reset()/step() surface as the reference's Gym classes, with a
leading batch dimension; tensors stay on the GPU (torch is only the allocator / stream
provider -- all arithmetic happens in libbeacon_hip.so).

Derived parameters are computed exactly as the reference constructors do (citations are
file:line into /root/reference/beacon/)."""
import ctypes as C
import os
import math

import numpy as np
import torch

from . import _lib
from . import spaces
from .spaces import Box, Discrete   # noqa: F401  (stand-in classes, kept importable from here)

_DT = {"f32": (torch.float32, _lib.F32), "f64": (torch.float64, _lib.F64),
       "float32": (torch.float32, _lib.F32), "float64": (torch.float64, _lib.F64),
       torch.float32: (torch.float32, _lib.F32), torch.float64: (torch.float64, _lib.F64)}


def out_layout(batch, obs_dim, esz):
    """Byte offsets of the packed per-step outputs of `batch` replicas."""
    def up(x):
        return (x + 15) // 16 * 16
    o_obs = 0
    o_rwd = up(o_obs + batch * obs_dim * esz)
    o_status = up(o_rwd + batch * esz)
    o_done = up(o_status + batch * 4)
    o_trunc = up(o_done + batch)
    return {"obs": o_obs, "rwd": o_rwd, "status": o_status, "done": o_done, "trunc": o_trunc,
            "bytes": up(o_trunc + batch)}


def unpack_outputs(buf, batch, obs_dim, tdtype):
    """Typed views (obs[B, n], rwd[B], status[B] int32, done[B] u8, trunc[B] u8) of one packed byte buffer."""
    esz = torch.empty((), dtype=tdtype).element_size()
    lay = out_layout(batch, obs_dim, esz)
    obs = buf[lay["obs"]:lay["obs"] + batch * obs_dim * esz].view(tdtype).view(batch, obs_dim)
    rwd = buf[lay["rwd"]:lay["rwd"] + batch * esz].view(tdtype)
    status = buf[lay["status"]:lay["status"] + batch * 4].view(torch.int32)
    done = buf[lay["done"]:lay["done"] + batch]
    trunc = buf[lay["trunc"]:lay["trunc"] + batch]
    return obs, rwd, status, done, trunc


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def dtype_name(tdtype):
    return "f64" if tdtype == torch.float64 else "f32"


def _mask_u8(mask, batch, device, what=None):
    """A replica mask ([B] bool / uint8 tensor or array) as a contiguous uint8 [B] tensor on `device` (the same memory when it is
    one already).  `what`: raise ValueError under that name for a mask of another length."""
    if not torch.is_tensor(mask):
        mask = torch.as_tensor(np.asarray(mask))
    if what is not None and mask.numel() != batch:
        raise ValueError("%s: mask must hold %d values" % (what, batch))
    return mask.to(device=device, dtype=torch.uint8).reshape(batch).contiguous()


# element types of a segment other than the env's own (BCN_SNAP_REAL)
_SEG_ELEM = {_lib.SNAP_I32: torch.int32, _lib.SNAP_U32: torch.int32, _lib.SNAP_U8: torch.uint8, _lib.SNAP_F64: torch.float64,
             _lib.SNAP_I64: torch.int64}


def _segments(segs, k):
    """The first k bcn_snapshot_seg structs (bcn_snapshot_layout, bcn_episode_layout) as plain dicts."""
    return [dict(name=g.name.decode(), offset=int(g.offset), elem=int(g.elem), planes=int(g.planes), row_elems=int(g.row_elems))
            for g in segs[:k]]


def _seg_view(buf, layout, name, n, real, rows_2d=()):
    """(segment dict, typed no-copy view) of the segment `name` of `buf`, laid out for n replicas of an env computing in `real`;
    KeyError for an unknown name.  A segment with planes = 0 does not scale with the replicas: row_elems is its length and the view
    is flat.  The others hold planes x n rows: [planes * n, row_elems] when row_elems > 1 or the name is in `rows_2d`, else flat."""
    for seg in layout:
        if seg["name"] == name:
            break
    else:
        raise KeyError(name)
    dt = _SEG_ELEM.get(seg["elem"], real)
    rows, row = int(seg["planes"]) * n, int(seg["row_elems"])
    v = buf[seg["offset"]:seg["offset"] + max(rows, 1) * row * torch.empty((), dtype=dt).element_size()].view(dt)
    return seg, (v.view(rows, row) if rows and (row > 1 or name in rows_2d) else v)


_POSITIVE_PARAMS = ("ra", "re", "pe", "delta", "g")       # divisors / arguments of roots (include/beacon_hip.h: bcn_set_params)

_OPS = ("rayleigh_reset", "rayleigh_step", "mixing_reset", "mixing_step", "burgers_reset", "burgers_step", "shkadov_reset",
        "shkadov_step", "sloshing_reset", "sloshing_step")
_ODE_OPS = ("lorenz_reset", "lorenz_step", "vortex_reset", "vortex_step")     # the ODE envs (csrc/ode_env.h)
_STATE_OPS = ("snapshot_save", "snapshot_load")                               # every env (csrc/snapshot.hip)
_EPISODE_OPS = ("episode_track",)                                             # every env (csrc/episode.hip)
_WARM_OPS = ("shkadov_reset_random",)                                         # shkadov (csrc/shkadov_warm_f32.hip, _f64.hip)
_JET_OPS = ("shkadov_jet_rewards",)                                           # shkadov (csrc/shkadov_jets.hip)
_ALL_OPS = _OPS + _ODE_OPS + _STATE_OPS + _EPISODE_OPS + _WARM_OPS + _JET_OPS
_NORM_OPS = ("normalize",)                                                    # every env (csrc/normalize.hip)
_ROLLOUT_OPS = ("rollout_begin", "rollout_record", "rollout_gae")             # every env (csrc/rollout.hip); resolved at the first attach
_RENDER_OPS = ("render",)                                                     # the grid envs (csrc/render.hip); resolved by the first renderer()


def _op_table():
    """{name: torch.ops.beacon.<name>.default} of the torch extension (beacon_amd/torch_ext.py), or None without it."""
    from . import torch_ext
    ops = torch_ext.load()
    return None if ops is None else {n: getattr(ops, n).default for n in _ALL_OPS + _NORM_OPS}


def _c_table(lib):
    """{name: bcn_<name> of libbeacon_hip.so}: the same entry points through ctypes, resolved once per env."""
    return {n: getattr(lib, "bcn_" + n) for n in _ALL_OPS + _NORM_OPS}


def _rollout_tables(lib, with_ops):
    """({name: torch op} or None, {name: bcn_<name>}) of _ROLLOUT_OPS: kept out of _op_table / _c_table, merged into an env's tables
    when a rollout is first attached (VecEnv.rollout)."""
    ops = None
    if with_ops:
        from . import torch_ext
        ext = torch_ext.load()
        ops = None if ext is None else {n: getattr(ext, n).default for n in _ROLLOUT_OPS}
    return ops, {n: getattr(lib, "bcn_" + n) for n in _ROLLOUT_OPS}


def _render_tables(lib, with_ops):
    """({name: torch op} or None, {name: bcn_<name>}) of _RENDER_OPS, as _rollout_tables: merged into an env's tables by its first
    renderer()."""
    ops = None
    if with_ops:
        from . import torch_ext
        ext = torch_ext.load()
        ops = None if ext is None or not hasattr(ext, "render") else {n: getattr(ext, n).default for n in _RENDER_OPS}
    return ops, {n: getattr(lib, "bcn_" + n) for n in _RENDER_OPS}


class Renderer(object):
    """RGB frames of `n` replicas of one VecEnv, drawn on the device (VecEnv.renderer; csrc/render.hip; the pixel rules:
    include/beacon_hip.h, bcn_render).  Owns `replicas` (int32 [n] on the device, or None: every replica in order), `lut` (uint8
    [256, 3], the field panel's colour table) and `frames`, uint8 [n, H_px, W_px, 3]; `shape` is (H_px, W_px).  Bookkeeping, like a
    Rollout: in no Snapshot; it reads the env's handle at every draw(), so it survives set_ndt_act."""

    def __init__(self, env, cfg, replicas, lut):
        self.env, self.cfg = env, cfg
        H, W = C.c_int(0), C.c_int(0)
        _lib.check(env.lib.bcn_render_shape(env.h, C.byref(cfg), C.byref(H), C.byref(W)))
        self.shape = (int(H.value), int(W.value))
        self.replicas = None
        if replicas is not None:
            if torch.is_tensor(replicas) and replicas.device.type == "cuda":      # not read on the host: the kernel skips bad indices
                idx = replicas
            else:
                host = np.asarray(replicas.cpu() if torch.is_tensor(replicas) else replicas, dtype=np.int64).reshape(-1)
                if host.size and (host.min() < 0 or host.max() >= env.batch):
                    raise ValueError("renderer: replica indices must lie in [0, %d)" % env.batch)
                idx = torch.as_tensor(host)
            self.replicas = idx.to(device=env.device, dtype=torch.int32).reshape(-1).contiguous()
        self.n = env.batch if self.replicas is None else int(self.replicas.numel())
        self.lut = None
        if env._panel == "field":
            if lut is None:
                from .render import colormap_lut
                lut = colormap_lut()
            t = torch.as_tensor(np.asarray(lut.cpu() if torch.is_tensor(lut) else lut))
            if t.dtype != torch.uint8 or tuple(t.shape) != (256, 3):
                raise ValueError("renderer: lut must be a uint8 [256, 3] table")
            self.lut = t.to(env.device).contiguous()
        self.frames = torch.empty((self.n,) + self.shape + (3,), dtype=torch.uint8, device=env.device)
        c = cfg
        self._scalars = (int(c.plane), int(c.scale), int(c.width), int(c.height), int(c.strip), int(c.has_range), float(c.lo), float(c.hi),
                         float(c.ref))

    def draw(self, out=None):
        """Enqueue ONE launch on the current stream that paints the replicas' present state and return the frames: the renderer's own
        `frames` (nothing is allocated: fit for torch.cuda.graph and for a loop next to step()), or `out`, a contiguous uint8
        [n, H_px, W_px, 3] device tensor of the caller.  No host synchronisation."""
        env = self.env
        if not getattr(env, "h", None) or not env.h.value:
            raise RuntimeError("Renderer.draw: the env it was made for is closed")
        buf = self.frames
        if out is not None:
            if (not torch.is_tensor(out) or out.dtype != torch.uint8 or out.device != env.device or tuple(out.shape) != tuple(buf.shape)
                    or not out.is_contiguous()):
                raise ValueError("Renderer.draw: out must be a contiguous uint8 %s tensor on %s" % (tuple(buf.shape), env.device))
            buf = out
        if env._ops is not None:
            env._ops["render"](env.h.value, buf, self.lut, self.replicas, *self._scalars)
        else:
            _lib.check(env._cfn["render"](env.h, C.byref(self.cfg), _ptr(self.lut), _ptr(self.replicas), self.n, _ptr(buf), env._stream()))
        return buf


class Snapshot(object):
    """Everything one VecEnv needs to continue its episodes bit for bit (VecEnv.snapshot / restore / fork), for `batch` replicas:
    `buf`, one uint8 tensor in the layout of include/beacon_hip.h (bcn_snapshot_*), and `meta`, a dict of plain values:
    env (class name), kind, dtype ("f32" / "f64"), batch, signature (bcn_snapshot_signature: env kind, dtype, constructor
    values, segment shapes), layout (the segments: name, offset, elem, planes, row_elems), field_shape, ctor (the env's
    constructor kwargs), version (of the library that wrote it), noise (sigma, seed, replica_offset: kernel arguments, recorded
    only) and gen_state (the env's torch generator, or None)."""

    ROWS_2D = ("obs", "obs_hist", "a_last", "a_prev")    # [batch, row_elems] also where a row is one element long

    def __init__(self, buf, meta):
        if not torch.is_tensor(buf) or buf.dtype != torch.uint8 or buf.dim() != 1:
            raise ValueError("Snapshot: buf must be a 1-D uint8 tensor")
        self.buf, self.meta = buf, dict(meta)

    batch = property(lambda self: int(self.meta["batch"]))
    signature = property(lambda self: int(self.meta["signature"]))
    device = property(lambda self: self.buf.device)

    def names(self):
        return [seg["name"] for seg in self.meta["layout"]]

    def view(self, name):
        """Typed view (no copy) of one segment: "fields" [planes, batch, ...] (the planes of get_state() in front of the batch
        axis), "obs_hist", "a_last" / "ia_last" / "iu", "a_prev", "stp", "nctr" (the uint32 counters as int32 bits), "obs", "rwd",
        "status", "done", "trunc" -- whichever the env has (names()).  KeyError for any other name."""
        seg, v = _seg_view(self.buf, self.meta["layout"], name, self.batch, _DT[self.meta["dtype"]][0], self.ROWS_2D)
        if name == "fields":
            return v.view((int(seg["planes"]), self.batch) + tuple(self.meta.get("field_shape") or ()))
        return v

    def to(self, device):
        """The same snapshot with `buf` on `device` (self when it is there already)."""
        buf = self.buf.to(device)
        return self if buf is self.buf else Snapshot(buf, self.meta)

    def save(self, path):
        """torch.save of `buf` (moved to the CPU) and `meta`."""
        torch.save({"buf": self.buf.cpu(), "meta": self.meta}, path)

    @staticmethod
    def load(path, device=None):
        d = torch.load(path, map_location="cpu", weights_only=True)
        snap = Snapshot(d["buf"], d["meta"])
        return snap if device is None else snap.to(device)


class _SegBuffer(object):
    """One uint8 device buffer `buf` that a bcn_*_layout / bcn_*_bytes pair of the library lays out for an env (the segments:
    include/beacon_hip.h), with a typed no-copy view of every segment as an attribute of its name.  A subclass states NAMES (the
    segments, in buffer order), C_FUNCS (the pair), ROWS_2D (the segments viewed [B, row_elems] even where a row is one element
    long; the others are 2-D only when row_elems > 1, and a segment with planes = 0 is flat [row_elems]), and SHAPE_KEY / NOUN: the
    env attribute its rows are as long as, recorded by state_dict(), and what load_state_dict() calls it.
    Bookkeeping, like `sweeps`: not part of a Snapshot or of snapshot_signature(); restore() / fork() move env state and leave
    these buffers where they are -- clear(mask) is the tool after a fork."""

    NAMES, C_FUNCS, ROWS_2D = (), (), ()
    SHAPE_KEY, NOUN = "obs_dim", "observations"

    def __init__(self, env, layout_args=()):
        """layout_args: what the pair takes between the handle and the segment array besides (Rollout: T, flags)."""
        segs = (_lib.SnapshotSeg * 16)()
        k = getattr(env.lib, self.C_FUNCS[0])(env.h, *(tuple(layout_args) + (segs, 16)))
        nbytes = getattr(env.lib, self.C_FUNCS[1])(env.h, *layout_args)
        if k != len(self.NAMES) or nbytes == 0:
            raise _lib.BeaconHipError("libbeacon_hip: %s" % env.lib.bcn_last_error().decode())
        self.batch, self.tdtype = env.batch, env.tdtype
        setattr(self, self.SHAPE_KEY, getattr(env, self.SHAPE_KEY))
        self.buf = torch.zeros((nbytes,), dtype=torch.uint8, device=env.device)
        self._bind(_segments(segs, k))

    def _bind(self, layout):
        self.layout = layout
        assert tuple(seg["name"] for seg in layout) == self.NAMES
        for name in self.NAMES:
            setattr(self, name, self.view(name))

    def view(self, name):
        """Typed view (no copy) of one segment; KeyError for an unknown name."""
        return _seg_view(self.buf, self.layout, name, self.batch, self.tdtype, self.ROWS_2D)[1]

    def clear(self, mask=None):
        """Zero every segment of the replicas selected by `mask` ([B] bool / uint8 tensor or array; None: all).  No host
        synchronisation."""
        if mask is None:
            self.buf.zero_()
            return self
        m = _mask_u8(mask, self.batch, self.buf.device) != 0
        for name in self.NAMES:
            v = getattr(self, name)
            v.masked_fill_(m[:, None] if v.dim() == 2 else m, 0)
        return self

    def state_dict(self):
        """For checkpoints: the buffer on the CPU and what it was laid out for."""
        return {"buf": self.buf.cpu(), "batch": self.batch, self.SHAPE_KEY: getattr(self, self.SHAPE_KEY), "dtype": dtype_name(self.tdtype)}

    def load_state_dict(self, d):
        key, mine = self.SHAPE_KEY, getattr(self, self.SHAPE_KEY)
        if (int(d["batch"]), int(d[key]), _DT[d["dtype"]][0]) != (self.batch, mine, self.tdtype) or d["buf"].numel() != self.buf.numel():
            raise ValueError("%s.load_state_dict: statistics of %s replicas x %s %s (%s), this env has %d x %d"
                             % (type(self).__name__, d["batch"], d[key], self.NOUN, d["dtype"], self.batch, mine))
        self.buf.copy_(d["buf"])
        return self


class EpisodeStats(_SegBuffer):
    """Episode statistics of one VecEnv, kept on the device by VecEnv.step_autoreset / track_episodes (csrc/episode.hip): `buf`,
    one uint8 tensor in the layout of bcn_episode_layout (include/beacon_hip.h), and typed no-copy views of its segments, all [B]
    but the last:
      ret, len            return (env dtype) and length (int32) of the episode in progress
      last_ret, last_len  those of the replica's last finished episode
      count               finished episodes (int32)
      sum_ret, sum_len    sums of the returns (float64) and lengths (int64) of the finished episodes
      finished            uint8, 1 where the last tracked step ended an episode (done | trunc): which rows of `obs` are fresh
      final_obs           [B, obs_dim], the terminal observation; a row is written when its replica finishes and kept until it finishes again
    Batch totals are not kept: totals() sums the columns.  Bookkeeping (_SegBuffer)."""

    NAMES = ("ret", "len", "last_ret", "last_len", "count", "sum_ret", "sum_len", "finished", "final_obs")
    C_FUNCS = ("bcn_episode_layout", "bcn_episode_bytes")
    ROWS_2D = ("final_obs",)

    def totals(self):
        """The one host read: {"episodes", "return_sum", "length_sum", "return_mean", "length_mean"} over the batch, from
        count.sum(), sum_ret.sum() and sum_len.sum() (the means are nan before the first episode ends)."""
        t = torch.stack([self.count.sum().double(), self.sum_ret.sum(), self.sum_len.sum().double()]).cpu().tolist()
        n, ls = int(round(t[0])), int(round(t[2]))
        return {"episodes": n, "return_sum": t[1], "length_sum": ls,
                "return_mean": t[1] / n if n else float("nan"), "length_mean": ls / n if n else float("nan")}


class JetStats(_SegBuffer):
    """Per-jet rewards and episode returns of one VecShkadov, kept on the device by the launch that follows every step while
    VecShkadov.set_jet_rewards is on (csrc/shkadov_jets.hip): `buf`, one uint8 tensor in the layout of bcn_shkadov_jets_layout
    (include/beacon_hip.h), and typed no-copy views of its segments, all [B, n_jets]:
      rwd_jets   the reward of every jet after the last step (shkadov_separable.get_rwd, shkadov.py:469-481)
      ret        the return (env dtype) of every jet in the episode in progress
      last_ret   that of the replica's last finished episode
      sum_ret    the sum (float64) of the finished returns
    Episode lengths and counts are those of EpisodeStats: all jets of a replica share one episode clock.  Bookkeeping
    (_SegBuffer)."""

    NAMES = ("rwd_jets", "ret", "last_ret", "sum_ret")
    C_FUNCS = ("bcn_shkadov_jets_layout", "bcn_shkadov_jets_bytes")
    ROWS_2D = NAMES
    SHAPE_KEY, NOUN = "n_jets", "jets"


class Normalizer(_SegBuffer):
    """Running normalisation of the observations and rewards of one VecEnv, kept on the device by the launches that follow every
    reset and step while VecEnv.set_normalize is on (csrc/normalize.hip; what the VecNormalize wrapper of the RL libraries
    computes): `buf`, one uint8 tensor in the layout of bcn_normalize_layout (include/beacon_hip.h), and typed no-copy views of
    its segments:
      obs_mean, obs_var [obs_dim], obs_count [1]   float64: running mean, population variance and sample count of every column
      ret_mean, ret_var, ret_count [1]             float64: those of the discounted return
      ret [B]                                      float64: the discounted return of every replica
      norm_obs [B, obs_dim], norm_rwd [B]          env dtype: what reset() / step() return while the feature is on
      norm_final_obs [B, obs_dim]                  env dtype: the normalised terminal observations of step_autoreset()
    (`scratch` is private to the kernels.)  `training` (bool): False freezes the statistics -- evaluation -- and only the three
    outputs are written.  gamma, eps, clip_obs, clip_rwd: the arguments of the launch, set by VecEnv.set_normalize.
    Bookkeeping (_SegBuffer): restore() / fork() leave the normaliser where it is.  state_dict() / load_state_dict() are for
    checkpoints and for evaluation with the statistics of a training run."""

    NAMES = ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count", "ret", "norm_obs", "norm_rwd", "norm_final_obs",
             "scratch")
    C_FUNCS = ("bcn_normalize_layout", "bcn_normalize_bytes")
    KINDS = {"step": 0, "reset": 1}              # include/beacon_hip.h: BCN_NORM_STEP, BCN_NORM_RESET
    ARGS = ("gamma", "eps", "clip_obs", "clip_rwd")     # of the launch, in its order

    def __init__(self, env, gamma=0.99, eps=1e-8, clip_obs=10.0, clip_rwd=10.0, training=True):
        self.gamma, self.eps, self.clip_obs, self.clip_rwd = float(gamma), float(eps), float(clip_obs), float(clip_rwd)
        self.training = bool(training)
        super().__init__(env)
        self.clear()

    def clear(self):
        """Back to the initial state: counts 0, means 0, variances 1, returns 0 (and the outputs zeroed).  No host
        synchronisation."""
        self.buf.zero_()
        self.obs_var.fill_(1.0)
        self.ret_var.fill_(1.0)
        return self

    def state_dict(self):
        """For checkpoints: the buffer on the CPU, what it was laid out for and the arguments of the launch."""
        return dict(super().state_dict(), **{name: getattr(self, name) for name in self.ARGS})

    def load_state_dict(self, d):
        super().load_state_dict(d)
        for name in self.ARGS:
            if name in d:
                setattr(self, name, float(d[name]))
        return self


class RolloutOverflow(RuntimeError):
    """A step was recorded into a Rollout that already held its T steps (Rollout.check)."""


class Rollout(_SegBuffer):
    """The transitions of up to T steps of one VecEnv, kept on the device by the launch that follows every step while the rollout
    is attached (VecEnv.rollout; csrc/rollout.hip), and the advantages and returns computed from them (compute_gae): `buf`, one
    uint8 tensor in the layout of bcn_rollout_layout (include/beacon_hip.h), and typed no-copy views of its segments:
      cursor     int32 [4]: [0] steps recorded so far, [1] sticky overflow flag
      obs        [T + 1, B, obs_dim]: obs[0] from begin(); step t writes obs[t + 1] = what the step returned (post-reset rows under
                 step_autoreset; norm_obs while normalising)
      act        [T, B, act_dim] in the env dtype, or int32 [T, B] for the discrete envs: the actions handed to the step (a step
                 called with actions=None records zeros)
      rwd        [T, B] (norm_rwd while normalising); status int32 [T, B]; done, trunc uint8 [T, B]: the terminal step's
      valid      uint8 [T, B]: 1 where the replica was stepped (no mask, or mask byte != 0)
      final_obs  [T, B, obs_dim] (final_obs=True; else [T, B, 0]): under step_autoreset, rows where episodes.finished hold the
                 terminal observation (norm_final_obs while normalising); the other rows are left as they are
      rwd_jets   [T, B, n_jets] for a VecShkadov with set_jet_rewards() on at attach time (else [T, B, 0])
      adv, ret   [T, B cols], written by compute_gae
    The slot a step writes comes from `cursor` on the device, never from the host: an eager loop, a one-step graph replayed T
    times and a T-step graph are the same launches and fill slots 0 .. T - 1.  A record into a full rollout writes no slot and
    raises the overflow flag, which check() reports.  A replica a mask skips gets valid = 0, rwd = 0, done = trunc = 0; its
    obs[t + 1] row is its unchanged current row; its act and final_obs rows are not written.
    Bookkeeping (_SegBuffer): in no Snapshot, snapshot_signature() unchanged, restore() / fork() leave it alone.  Not covered:
    ShardedVecEnv and the single-env mirrors (beacon_amd/envs.py), as for the other bookkeeping buffers."""

    NAMES = ("cursor", "obs", "act", "rwd", "status", "done", "trunc", "valid", "final_obs", "rwd_jets", "adv", "ret")
    C_FUNCS = ("bcn_rollout_layout", "bcn_rollout_bytes")
    ROWS_2D = ("obs", "act", "final_obs", "rwd_jets")        # [planes, B, row_elems] also where a row is one element long

    def __init__(self, env, T, final_obs=True):
        import weakref
        if isinstance(T, bool) or not isinstance(T, (int, np.integer)) or int(T) < 1:
            raise ValueError("Rollout: T must be an integer >= 1, got %r" % (T,))
        self.T = int(T)
        jets = bool(getattr(env, "_jets_on", False))
        self.flags = (_lib.RO_FINAL_OBS if final_obs else 0) | (_lib.RO_JETS if jets else 0)
        self.n_jets = int(env.n_actions) if jets else 0
        self._env = weakref.ref(env)
        super().__init__(env, (self.T, self.flags))

    def view(self, name):
        """Typed view (no copy) of one segment, the step axis in front; KeyError for an unknown name.  "adv" / "ret": as the last
        compute_gae laid them out ([T, B] before the first)."""
        if name in ("adv", "ret"):
            return self.gae_views(getattr(self, "cols", 1))[name == "ret"]
        seg, v = _seg_view(self.buf, self.layout, name, self.batch, self.tdtype, self.ROWS_2D)
        if not seg["planes"]:
            return v
        if name in self.ROWS_2D and seg["elem"] == _lib.SNAP_REAL:
            return v.view(int(seg["planes"]), self.batch, int(seg["row_elems"]))
        return v.view(int(seg["planes"]), self.batch)

    def gae_views(self, cols=1):
        """(adv, ret) as [T, B cols] views: where compute_gae with that many columns per replica writes them (cols: 1, or n_jets
        for per_jet=True)."""
        out = []
        for name in ("adv", "ret"):
            v = _seg_view(self.buf, self.layout, name, self.batch, self.tdtype)[1].reshape(-1)
            out.append(v[:self.T * self.batch * cols].view(self.T, self.batch * cols))
        return tuple(out)

    def clear(self):
        """Zero every segment, the cursor included.  No host synchronisation."""
        self.buf.zero_()
        return self

    def begin(self):
        """Start a rollout: cursor = 0, overflow = 0, obs[0] = what the env's reset() / step() currently return (norm_obs while
        normalising).  ONE launch, no host synchronisation; it can be captured.  The other segments keep their contents and are
        overwritten slot by slot.  Returns self."""
        env = self._env()
        if env is None:
            raise RuntimeError("Rollout.begin: the env of this rollout is gone")
        env._call("rollout_begin", self.buf, env.out_buf, env._norm.buf if env._norm_on else None)
        return self

    def check(self):
        """The one host read: (steps recorded, False); raises RolloutOverflow when a step was recorded into the full rollout
        (that step wrote nothing; begin() clears the flag)."""
        n, over = self.cursor[:2].cpu().tolist()
        if over:
            raise RolloutOverflow("Rollout.check: a step was recorded behind the last of %d slots (it wrote nothing); begin() starts over" % self.T)
        return int(n), False

    def compute_gae(self, values, last_value, final_values=None, gamma=0.99, lam=0.95, per_jet=False):
        """Generalised advantage estimation over the recorded steps, ONE launch with a lane per column (csrc/rollout.hip), no host
        synchronisation.  values [T, B cols], last_value [B cols], final_values [T, B cols] or None: contiguous device tensors of
        the env dtype (any shape with those element counts); cols = 1, or n_jets with per_jet=True (which needs the rwd_jets
        segment and takes the rewards from it).  The number of recorded steps n is read from the cursor on the device; rows
        t >= n of adv / ret are not written.  Per column, t = n - 1 .. 0, nv = last_value, gae = 0:
          valid = 0:  adv = 0, ret = values[t]; nv and gae pass through (a skipped step is transparent)
          else        fin = done | trunc; boot = final_values[t] if final_values is given and trunc is set, else 0 (the time limit
                      sets done = trunc = 1 and bootstraps; shkadov's blow-up sets done alone and is terminal);
                      delta = rwd[t] + gamma (boot if fin else nv) - values[t]; gae = delta + (0 if fin else gamma lam gae);
                      adv[t] = gae, ret[t] = gae + values[t], nv = values[t]
        in float64 whatever the env dtype, rounded once on store.  Only rows of final_values where trunc is set are used: the others may hold anything.
        ValueError for a wrong shape, dtype or device.  Returns (adv, ret), [T, B cols] views that `adv` / `ret` name from then on."""
        env = self._env()
        if env is None:
            raise RuntimeError("Rollout.compute_gae: the env of this rollout is gone")
        if per_jet and not self.flags & _lib.RO_JETS:
            raise ValueError("Rollout.compute_gae: per_jet=True needs the rwd_jets segment (set_jet_rewards() on when the rollout is attached)")
        cols = self.n_jets if per_jet else 1
        n = self.batch * cols
        for name, t, numel in (("values", values, self.T * n), ("last_value", last_value, n), ("final_values", final_values, self.T * n)):
            if t is None and name == "final_values":
                continue
            if (not torch.is_tensor(t) or t.dtype != self.tdtype or t.device != self.buf.device or t.numel() != numel
                    or not t.is_contiguous()):
                raise ValueError("Rollout.compute_gae: %s must be a contiguous %s tensor of %d elements on %s"
                                 % (name, dtype_name(self.tdtype), numel, self.buf.device))
        if not (0.0 <= float(gamma) <= 1.0 and 0.0 <= float(lam) <= 1.0):
            raise ValueError("Rollout.compute_gae: gamma and lam must lie in [0, 1]")
        env._call("rollout_gae", self.buf, values, last_value, final_values, self.T, self.flags, cols, float(gamma), float(lam))
        self.cols = cols
        self.adv, self.ret = self.gae_views(cols)
        return self.adv, self.ret


class ParamsWarning(UserWarning):
    """A 2D env whose default kernel is a register-resident one received per-replica parameters: it steps through the generic
    kernel until clear_params() (VecEnv.set_params).  set_params_kernel("fast") on the env selects the register-resident kernels
    that read the table instead, and with them in force set_params does not warn."""


class VecEnv(object):
    """Common machinery.  Subclasses set self.cfg and implement _create/_reset/_step."""

    action_is_int = False
    PARAMS = ()              # names of the per-replica physical parameters (set_params), in the order of the C ABI's value rows
    needs_noise = False
    _plugin_defs = None      # extra -D flags of this class's on-demand kernels (tests: the deliberately broken plugin)
    _plugin_prm_defs = None  # ... of their table-reading twins alone (set_params_kernel), on top of _plugin_defs
    _norm = None             # set_normalize: the Normalizer, allocated by the first call and kept
    _norm_on = False         # ... whether the normalising launches follow every reset and step
    _mask = None             # the replica mask in force in the library (_apply_mask, _masked); None: none
    _rollout = None          # rollout: the Rollout attached (a recording launch follows every step); None: none, nothing extra runs
    _rollout_kept = None     # ... the last one allocated, kept across rollout(None)
    _panel = None            # renderer: "field" (rayleigh, mixing), "line" (burgers, shkadov, sloshing), None: nothing to draw
    _render_merged = False   # ... whether _RENDER_OPS are in this env's tables

    def __init__(self, batch, device="cuda:0", dtype="f32"):
        if not torch.cuda.is_available():
            raise RuntimeError("beacon_amd needs a ROCm GPU: the solver path is HIP-only (no CPU fallback)")
        self.lib = _lib.load()
        # the torch.library ops over the same C ABI (beacon_amd/torch_ext.py): one dispatcher call per reset() / step();
        # None (no compiler and no prebuilt extension, or BEACON_TORCH_EXT=0): the ctypes binding below
        self._ops = _op_table()
        self._cfn = _c_table(self.lib)
        self.batch = int(batch)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("device must be a cuda (ROCm) device")
        self.dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", self.dev_index)
        self.tdtype, self.cdtype = _DT[dtype]
        self.h = C.c_void_p()
        self._mask = None
        self._create()
        self.obs_dim = self.lib.bcn_n_obs(self.h)       # observation length per replica
        self.n_actions = self.lib.bcn_n_act(self.h)
        self._alloc_outputs()

    def _alloc_outputs(self):
        """Per-step outputs live in ONE byte buffer [obs | rwd | status | done | trunc] (segments 16-byte
        aligned), so the trainer-facing gather of a sharded batch is a single collective on `out_buf`
        (beacon_amd/dist.py); obs / rwd / ... are typed views of it.  There may be two such buffers
        (double_buffer): `out_buf`, `obs`, `rwd`, `status`, `done`, `trunc` always name the one the last
        reset() / step() wrote."""
        B, esz = self.batch, torch.empty((), dtype=self.tdtype).element_size()
        self.out_layout = out_layout(B, self.obs_dim, esz)
        self.out_bufs, self._views, self._rotate = [], [], 0
        self._add_out_buf()
        self._bind_outputs(0)

    def _add_out_buf(self):
        buf = torch.zeros((self.out_layout["bytes"],), dtype=torch.uint8, device=self.device)
        self.out_bufs.append(buf)
        self._views.append(unpack_outputs(buf, self.batch, self.obs_dim, self.tdtype))

    def _bind_outputs(self, k):
        self._cur = k
        self.out_buf = self.out_bufs[k]
        self.obs, self.rwd, self.status, self.done, self.trunc = self._views[k]

    def double_buffer(self, on=True, nbuf=2):
        """Rotate through `nbuf` packed output buffers: step k writes buffer k % nbuf, so that a consumer of step k's
        outputs on another stream -- the sharded batch's gather to rank 0 (beacon_amd/dist.py), a device-to-host copy --
        may still be reading them while the next nbuf - 1 steps run.  After every step() the attributes obs / rwd / done /
        trunc / status / out_buf are re-bound to the buffer that step wrote (so hold on to the tensors a step RETURNS, not
        to the attributes, and expect them to be overwritten nbuf steps later).  reset() writes the current buffer.
        A step with a replica mask first copies the previous buffer (the rows of skipped replicas keep their values).
        Not for captured graphs (StepGraph records fixed addresses)."""
        while on and len(self.out_bufs) < int(nbuf):
            self._add_out_buf()
        self._rotate = int(nbuf) if on else 0
        if not on:
            self._bind_outputs(self._cur)
        return self

    def _next_outputs(self, carry):
        """Called by step() before the launch: with rotating outputs, switch to the next buffer."""
        if not self._rotate:
            return
        prev = self.out_buf
        self._bind_outputs((self._cur + 1) % self._rotate)
        if carry:
            self.out_buf.copy_(prev)

    # -- plumbing ---------------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _call(self, name, *args):
        """The entry point `name` (one of _OPS, _ODE_OPS, _STATE_OPS, _EPISODE_OPS, _WARM_OPS, _JET_OPS, _NORM_OPS, _ROLLOUT_OPS) through the binding in force: the torch op, or
        bcn_<name> through ctypes.  `args`: what both take between the handle and the stream, in their common order -- tensors
        (None: a null pointer), ints and floats; the op reads torch's current stream itself, ctypes gets it appended."""
        if self._ops is not None:
            return self._ops[name](self.h.value, *args)
        _lib.check(self._cfn[name](self.h, *[a if a is None or isinstance(a, (int, float)) else C.c_void_p(a.data_ptr()) for a in args],
                                   self._stream()))

    def _int_actions(self, actions):
        """Discrete actions -> contiguous int32 [B] device tensor; None (the kernel repeats the stored action) stays None."""
        if actions is None:
            return None
        if not torch.is_tensor(actions):
            actions = torch.as_tensor(np.asarray(actions, dtype=np.int64))
        return actions.to(device=self.device, dtype=torch.int32).reshape(self.batch).contiguous()

    def _noise_setup(self, seed):
        """The envs with inlet noise (burgers, shkadov), once their handle exists: the kernel's own draws (set_noise_seed) and the
        torch generator `gen` of draw_noise() / reset_random() both start from the constructor's seed."""
        self.set_noise_seed(seed, 0)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(self.seed)

    def _real(self, x, shape):
        """actions / noise / init fields -> contiguous device tensor of the env dtype."""
        if x is None:
            return None
        if (torch.is_tensor(x) and x.dtype == self.tdtype and x.device == self.device and tuple(x.shape) == tuple(shape)
                and x.is_contiguous()):
            return x                      # what a trainer passes every step: nothing to convert
        if not torch.is_tensor(x):
            x = torch.as_tensor(np.asarray(x, dtype=np.float64))
        x = x.to(device=self.device, dtype=self.tdtype).reshape(shape).contiguous()
        return x

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.lib.bcn_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- state ------------------------------------------------------------------------------
    def state_shape(self):
        raise NotImplementedError

    def get_state(self):
        """Solver fields of every replica as one device tensor (layout: include/beacon_hip.h)."""
        out = torch.empty((self.batch,) + self.state_shape(), dtype=self.tdtype, device=self.device)
        _lib.check(self.lib.bcn_get_state(self.h, _ptr(out), 1, self._stream()))
        return out

    def set_state(self, state):
        st = self._real(state, (self.batch,) + self.state_shape())
        _lib.check(self.lib.bcn_set_state(self.h, _ptr(st), 1, self._stream()))
        torch.cuda.current_stream(self.device).synchronize()  # `st` may be a temporary

    # -- snapshots --------------------------------------------------------------------------
    def snapshot_signature(self):
        """bcn_snapshot_signature of this env: equal for two envs exactly when they can exchange snapshots.  It covers env kind,
        dtype, the constructor's values (set_ndt_act builds a new handle, so its ndt_act counts) and the segment shapes; options,
        variant and noise settings made on the handle afterwards are not in it (they do not change what the bytes mean)."""
        return int(self.lib.bcn_snapshot_signature(self.h))

    def _snap_meta(self):
        segs = (_lib.SnapshotSeg * 16)()
        k = self.lib.bcn_snapshot_layout(self.h, self.batch, segs, 16)
        if k <= 0:
            raise _lib.BeaconHipError("libbeacon_hip: %s" % self.lib.bcn_last_error().decode())
        shape = self.state_shape()
        return dict(env=type(self).__name__, kind=int(self.lib.bcn_env_kind(self.h)), dtype=dtype_name(self.tdtype),
                    batch=self.batch, signature=self.snapshot_signature(), layout=_segments(segs, k),
                    field_shape=list(shape[1:]) if len(shape) > 1 else [], ctor=dict(getattr(self, "_ctor", {})),
                    version=self.lib.bcn_version().decode(), noise=None, gen_state=None)

    def _snap_volatile(self, meta):
        gen = getattr(self, "gen", None)
        # (inside a graph capture the generator is left alone: its state is host-side and not part of what the graph replays)
        meta["gen_state"] = None if gen is None or torch.cuda.is_current_stream_capturing() else gen.get_state()
        meta["noise"] = (dict(sigma=float(self.sigma), seed=int(self.seed), replica_offset=int(self.replica_offset))
                         if self.needs_noise else None)

    def _check_snap(self, snap, what):
        if not isinstance(snap, Snapshot):
            raise ValueError("%s: a Snapshot expected, got %s" % (what, type(snap).__name__))
        if snap.signature != self.snapshot_signature():
            raise ValueError("%s: the snapshot was taken from another configuration (%s %s, signature %#x; this env: %s, %#x)"
                             % (what, snap.meta.get("env"), snap.meta.get("dtype"), snap.signature, type(self).__name__,
                                self.snapshot_signature()))
        if snap.buf.device != self.device:
            raise ValueError("%s: the snapshot lives on %s, this env on %s (Snapshot.to moves it)" % (what, snap.buf.device, self.device))
        if snap.buf.numel() != self.lib.bcn_snapshot_bytes_n(self.h, snap.batch) or not snap.buf.is_contiguous():
            raise ValueError("%s: %d bytes do not hold %d replicas of this env" % (what, snap.buf.numel(), snap.batch))

    def snapshot(self, out=None):
        """Save every replica -- solver fields, observation history, stored actions, episode and noise-draw counters, and the
        outputs (obs, rwd, status, done, trunc) of the last reset() / step() -- into a Snapshot: ONE kernel launch on the current
        stream, no host synchronisation, so it can be captured into a graph.  `out`: a Snapshot of this env's signature and batch to
        overwrite (nothing is allocated; `out` itself is returned).  Not saved, because they are outputs only or kernel arguments:
        `sweeps`, `actions_norm`, counters, options, the noise sigma / seed / replica_offset (recorded in meta["noise"])."""
        if out is None:
            nbytes = self.lib.bcn_snapshot_bytes(self.h)
            out = Snapshot(torch.zeros((nbytes,), dtype=torch.uint8, device=self.device), self._snap_meta())
        else:
            self._check_snap(out, "snapshot(out=)")
            if out.batch != self.batch:
                raise ValueError("snapshot(out=): out holds %d replicas, this env %d" % (out.batch, self.batch))
        self._snap_volatile(out.meta)
        self._call("snapshot_save", out.buf, self.out_buf)
        return out

    def restore(self, snap, src=None, mask=None):
        """Load replicas from a Snapshot of the same signature: replica b takes replica src[b] of `snap` (src None: b, which needs
        snap.batch == batch) where mask[b] is nonzero (None: everywhere); the others keep state, counters and output rows.  ONE
        launch on the current stream.  Returns (obs, rwd, done, trunc) as they were when the snapshot was taken (gathered); the
        env's obs / rwd / done / trunc / status hold them (with double_buffer(): the current buffer).
        Raises ValueError on the host, before any launch, when the signatures differ, the snapshot lives on another device,
        src is None and the batches differ, or a `src` given as a list / array / CPU tensor holds an index outside [0, snap.batch).
        A `src` that is a device tensor is not read on the host; the kernel leaves replicas with an index out of range untouched.
        The noise sigma, seed and replica_offset are kernel arguments: restore does not change them (meta["noise"] records those
        of the source).  The env's torch generator `gen` is set back on an identity restore (src and mask None) only."""
        self._check_snap(snap, "restore")
        if src is None:
            if snap.batch != self.batch:
                raise ValueError("restore: the snapshot holds %d replicas, this env %d: pass src" % (snap.batch, self.batch))
        else:
            if not torch.is_tensor(src) or src.device.type != "cuda":
                host = np.asarray(src.numpy() if torch.is_tensor(src) else src)
                if host.shape != (self.batch,) or not np.issubdtype(host.dtype, np.integer):
                    raise ValueError("restore: src must hold %d integers" % self.batch)
                if host.size and (host.min() < 0 or host.max() >= snap.batch):
                    raise ValueError("restore: src holds an index outside [0, %d)" % snap.batch)
                src = torch.as_tensor(host.astype(np.int32))
            if src.numel() != self.batch:
                raise ValueError("restore: src must hold %d integers" % self.batch)
            if src.device != self.device or src.dtype != torch.int32 or not src.is_contiguous():
                src = src.to(device=self.device, dtype=torch.int32).reshape(self.batch).contiguous()
        if mask is not None:
            mask = _mask_u8(mask, self.batch, self.device, "restore")
        self._keep_restore = (src, mask)
        self._call("snapshot_load", snap.buf, snap.batch, src, mask, self.out_buf)
        gen = getattr(self, "gen", None)
        if (gen is not None and src is None and mask is None and snap.meta.get("gen_state") is not None
                and not torch.cuda.is_current_stream_capturing()):
            gen.set_state(snap.meta["gen_state"])
        return self.obs, self.rwd, self.done, self.trunc

    def fork(self, src, mask=None):
        """replica b <- replica src[b] of THIS env (where mask[b] is nonzero): a snapshot() into a scratch Snapshot the env keeps
        and reuses, then a restore() from it -- two launches, nothing allocated after the first call; any src (permutations,
        duplicates) is safe because source and destination are different buffers.  What planning by shooting (copy the current
        state into B candidates), population-based training (overwrite the worst with the best) and resets from a developed
        replica need.  Device noise (burgers, shkadov; step() without `noise`): the draw counter is copied from the source but the
        Philox counter is keyed by the replica's OWN global index, so copies of one source draw different noise from then on --
        what exploration wants; identical continuations need an explicit `noise` tensor."""
        scratch = getattr(self, "_fork_snap", None)
        if scratch is not None and scratch.signature != self.snapshot_signature():
            scratch = None
        self._fork_snap = self.snapshot(out=scratch)
        return self.restore(self._fork_snap, src, mask)

    def get_stp(self):
        buf = (C.c_int32 * self.batch)()
        _lib.check(self.lib.bcn_get_stp(self.h, buf, self._stream()))
        return np.frombuffer(buf, dtype=np.int32).copy()

    def set_stp(self, stp):
        arr = np.ascontiguousarray(np.broadcast_to(np.asarray(stp, dtype=np.int32), (self.batch,)))
        _lib.check(self.lib.bcn_set_stp(self.h, arr.ctypes.data_as(_lib.c_i32p), self._stream()))

    def set_variant(self, v):
        return self.lib.bcn_set_variant(self.h, int(v))

    def set_sched(self, mode=-1, grid=0, q=0, lpt_min_batch=0):
        """Scheduling of the register-resident 2D kernels (include/beacon_hip.h: bcn_set_sched);
        results do not depend on it."""
        _lib.check(self.lib.bcn_set_sched(self.h, int(mode), int(grid), int(q), int(lpt_min_batch)))

    def _attach_plugin(self, kind):
        """2D envs: a grid without a built-in register-resident kernel gets one compiled for it (beacon_amd/jit.py);
        when that is not possible the generic kernel stays selected."""
        if self.lib.bcn_set_variant(self.h, 1) == 1 and os.environ.get("BEACON_JIT_FORCE") != "1":
            return
        from . import jit
        f64 = self.tdtype == torch.float64
        p = jit.plugin_for(self.nx, self.ny, f64, kind, getattr(self, "_plugin_defs", None))
        if p is None:
            return
        if p.verified is None and not jit.CHECKING:
            # first use of this shared object: compared with the generic kernel before any env runs on it (jit.verify)
            ctor, cls, dev, dt = dict(self._ctor), type(self), self.device, dtype_name(self.tdtype)
            jit.verify(p, lambda batch: cls(batch, dev, dt, **ctor), kind, f64)
        if p.verified or jit.CHECKING:
            _lib.check(self.lib.bcn_set_fast_plugin(self.h, p.fn, p.scratch))
            self._plugin = p

    def _slow_mode_bound(self, kind):
        """The per-grid constants of conv_plan 3's slow-mode landing guard (beacon_amd/stoprule.py), for grids the library has
        not built in.  The one-row and two-rows-per-lane kernels (ny <= 128) use them; the hybrid and the generic kernel do not."""
        if self.ny > 128 or min(self.nx, self.ny) < 48 or os.environ.get("BEACON_STOPRULE") == "0":
            return
        two = C.c_double * 2
        if self.lib.bcn_get_slow_mode_bound(self.h, two(), two()) > 0:
            return
        from . import stoprule
        cx = self.dy * self.dy / (2.0 * (self.dx * self.dx + self.dy * self.dy))
        b = stoprule.bounds(self.nx, self.ny, kind, cx)
        if b:
            _lib.check(self.lib.bcn_set_slow_mode_bound(self.h, len(b), two(*[c for c, _ in b]), two(*[v for _, v in b])))

    def set_slow_mode_bound(self, pairs):
        """pairs: up to two (cutoff, bound) of this grid (beacon_amd/stoprule.py: bounds); [] clears them.  The library trusts the
        caller: constants below the grid's true ones void the proof of conv_plan 3's landings (tests/test_gpu_parity.py shows it)."""
        two = C.c_double * 2
        _lib.check(self.lib.bcn_set_slow_mode_bound(self.h, len(pairs), two(*[c for c, _ in pairs]), two(*[b for _, b in pairs])))

    def slow_mode_bound(self):
        """[(cutoff, bound)] in force (include/beacon_hip.h: bcn_get_slow_mode_bound); empty: the guard is BCN_CONV_GUARD alone."""
        two = C.c_double * 2
        c, b = two(), two()
        n = self.lib.bcn_get_slow_mode_bound(self.h, c, b)
        return [(c[k], b[k]) for k in range(max(n, 0))]

    def use_torch_ops(self, on=True):
        """Switch this env between the two bindings of the C ABI: the torch.library ops (default when the extension is built)
        and ctypes.  Returns whether the ops are in use.  Results do not depend on it (tests/test_gpu_parity.py)."""
        self._ops = _op_table() if on else None
        if self._rollout_kept is not None:
            self._merge_rollout_ops()
        if self._render_merged:
            self._merge_render_ops()
        return self._ops is not None

    def set_option(self, name, value):
        """Solver options by name (include/beacon_hip.h: bcn_set_option), e.g. ("conv_plan", 0)."""
        _lib.check(self.lib.bcn_set_option(self.h, name.encode(), int(value)))

    def set_noise_seed(self, seed, replica_offset=0):
        """Envs with inlet noise (burgers, shkadov): step() without an explicit `noise` tensor lets the step kernel draw
        uniform(-sigma, sigma) itself (include/beacon_hip.h: bcn_set_noise) -- keyed by `seed`, the global replica index
        `replica_offset + b`, the replica's count of such steps and the timestep.
        Two things to know: (1) `env.gen` (a torch generator) only feeds draw_noise() and reset_random(); seeding IT does not
        change the noise of step(a) without a `noise` tensor -- this method does.  (2) sigma, seed and offset are kernel
        ARGUMENTS: a graph recorded by capture() keeps the values it was recorded with (only the per-replica draw counters
        live on the device and advance at replay), so re-capture after changing the seed."""
        self.seed, self.replica_offset = int(seed), int(replica_offset)
        _lib.check(self.lib.bcn_set_noise(self.h, float(self.sigma), self.seed, self.replica_offset))

    def get_counters(self):
        """uint64 [B, 4] of the last step, per replica: shader cycles inside the Jacobi loop / in the whole replica, late
        stops of the extrapolating residual plan, repeated timesteps (include/beacon_hip.h: bcn_get_counters)."""
        n = _lib.COUNTER_WORDS
        buf = (C.c_uint64 * (n * self.batch))()
        _lib.check(self.lib.bcn_get_counters_n(self.h, buf, n, self._stream()))     # the sized form: the buffer cannot be overrun
        return np.frombuffer(buf, dtype=np.uint64).reshape(self.batch, n).copy()

    @property
    def kernel_name(self):
        return self.lib.bcn_kernel_name(self.h).decode()

    @property
    def kernel_shape(self):
        """(cells per thread, threads per replica) of the 1D step kernel the last step() launched -- the launcher overrides
        the options cells_per_thread / one_wave where they do not fit the grid (include/beacon_hip.h: bcn_kernel_shape);
        (0, 0) before the first step and for the envs without the notion."""
        k, nt = C.c_int(0), C.c_int(0)
        _lib.check(self.lib.bcn_kernel_shape(self.h, C.byref(k), C.byref(nt)))
        return (k.value, nt.value)

    def check_status(self):
        """Synchronise and raise if any replica reported a solver failure (the reference
        prints and exit(1)s on Poisson non-convergence: rayleigh.py:221-224)."""
        st = self.status.cpu().numpy()
        if (st & _lib.ST_ITMAX).any():
            bad = np.nonzero(st & _lib.ST_ITMAX)[0]
            raise RuntimeError("Exceeded max number of iterations in solver (replicas %s)" % bad[:8].tolist())
        return st

    # -- per-replica physical parameters ----------------------------------------------------
    @property
    def params(self):
        """{name: float64 [B] ndarray} of the physical parameters in force, one value per replica (PARAMS of the class; the
        constructor's values broadcast when set_params was never called or clear_params() undid it)."""
        n, B = len(self.PARAMS), self.batch
        buf = np.empty((n, B), dtype=np.float64)
        _lib.check(self.lib.bcn_get_params(self.h, buf.ctypes.data_as(C.POINTER(C.c_double))))
        return {name: buf[k].copy() for k, name in enumerate(self.PARAMS)}

    def set_params(self, **cols):
        """Give every replica its own physics: each keyword is one of PARAMS (the reference's constructor arguments: lorenz sigma,
        rho, beta; vortex re, weight; burgers u_target, amp; shkadov delta; sloshing amp, alpha, g; rayleigh ra; mixing re, pe) and
        takes a scalar or a length-B sequence / ndarray / tensor; names not given keep their current per-replica values.
        ValueError -- before anything is launched or changed -- for an unknown name, a wrong length, a non-finite value or a value
        <= 0 where the solver divides by it (ra, re, pe, delta, g).
        Parameters are configuration, like the noise sigma / seed: they take effect at the next reset() / step() and alter no
        state; they are not part of a Snapshot or of snapshot_signature(), and restore() / fork() move state between replicas
        while every replica keeps its physics; masks work as before.  A replica whose parameters equal the constructor arguments
        of another env computes what that env computes, bit for bit (the same kernel reads the same constants).
        Graphs: the device table keeps its address from the first call on and later calls rewrite it in place, so a graph
        captured after a set_params replays whatever table is in force at replay time; one captured before the first call keeps
        the constructor's values.
        2D envs: by default only the generic kernel reads the table.  While parameters are set the env steps through
        ns2d_generic_step (kernel_name says so; the first call warns once with ParamsWarning when that is not the default kernel),
        and clear_params() restores the previous dispatch.  The fast path: set_params_kernel("fast") -- before or after this call --
        selects the register-resident kernels that read the table (kernel_name then starts with ns2d_fast, and nothing warns)."""
        unknown = [k for k in cols if k not in self.PARAMS]
        if unknown:
            raise ValueError("%s.set_params: unknown parameter %s (this env has %s)" % (type(self).__name__, ", ".join(map(repr, unknown)),
                                                                                     ", ".join(self.PARAMS)))
        cur, B = self.params, self.batch
        vals = np.empty((len(self.PARAMS), B), dtype=np.float64)
        for k, name in enumerate(self.PARAMS):
            if name not in cols:
                vals[k] = cur[name]
                continue
            v = cols[name]
            v = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
            v = v.astype(np.float64)
            if v.ndim > 1 or (v.ndim == 1 and v.shape[0] != B):
                raise ValueError("%s.set_params: %s has shape %s; a scalar or %d values (one per replica)" % (type(self).__name__, name,
                                                                                                           tuple(v.shape), B))
            vals[k] = v
        for k, name in enumerate(self.PARAMS):
            bad = ~np.isfinite(vals[k])
            if name in _POSITIVE_PARAMS:
                bad |= ~(vals[k] > 0.0)
            if bad.any():
                b = int(np.nonzero(bad)[0][0])
                raise ValueError("%s.set_params: %s of replica %d is %r; it must be finite%s" % (
                    type(self).__name__, name, b, float(vals[k, b]), " and > 0" if name in _POSITIVE_PARAMS else ""))
        before = self.kernel_name
        _lib.check(self.lib.bcn_set_params(self.h, vals.ctypes.data_as(C.POINTER(C.c_double)), self._stream()))
        self._params = vals                       # re-applied when the handle is rebuilt (set_ndt_act)
        if before != "ns2d_generic_step" and self.kernel_name == "ns2d_generic_step" and not getattr(self, "_params_warned", False):
            import warnings
            self._params_warned = True
            warnings.warn("%s: per-replica parameters are read by the generic kernel only: this env now steps through %s instead of "
                          "%s, until clear_params()" % (type(self).__name__, self.kernel_name, before), ParamsWarning, stacklevel=2)
        return self

    def clear_params(self):
        """Back to the constructor's parameters for every replica (and, 2D envs, to the kernel that ran before set_params)."""
        _lib.check(self.lib.bcn_set_params(self.h, None, self._stream()))
        self._params = None
        return self

    def _reapply_params(self):
        """After the handle was rebuilt: the new one takes the table the old one had."""
        vals = getattr(self, "_params", None)
        if vals is not None:
            _lib.check(self.lib.bcn_set_params(self.h, vals.ctypes.data_as(C.POINTER(C.c_double)), self._stream()))

    # -- replica masks ----------------------------------------------------------------------
    def _apply_mask(self, mask):
        """mask: None (all replicas) or a [B] bool/uint8 tensor/array; replicas with 0 are skipped
        by the next reset/step launch (their state and output rows stay as they are)."""
        if mask is None:
            self._mask = None
            _lib.check(self.lib.bcn_set_mask(self.h, None))
            return
        self._mask = _mask_u8(mask, self.batch, self.device)
        _lib.check(self.lib.bcn_set_mask(self.h, _ptr(self._mask)))

    def _masked(self, mask, fn):
        """THE mask frame of reset() / step() / step_autoreset() / capture(): fn(m) with `mask` in force in the library, m being
        its uint8 form (None: all replicas); whatever mask is in force afterwards -- the caller's, or ep.finished, which
        _reset_finished leaves there -- is cleared, also when fn raises.  No mask now and none set: nothing to tell the library."""
        if mask is not None or self._mask is not None:
            self._apply_mask(mask)
        try:
            return fn(self._mask)
        finally:
            if self._mask is not None:
                self._apply_mask(None)

    # -- Gym surface ------------------------------------------------------------------------
    def reset(self, mask=None):
        """Reset every replica, or only those selected by `mask` (what a trainer does when it calls
        reset() on the one env whose episode ended)."""
        return self._masked(mask, self._enqueue_reset)

    def _enqueue_reset(self, m):
        self._reset()
        if self._norm_on:
            self._normalize("reset", m)
            return self._norm.norm_obs, None
        return self.obs, None

    def _after_step(self):
        """What an env launches directly behind its step kernel in step() / step_autoreset() / capture(), under the same replica
        mask (VecShkadov.set_jet_rewards).  Nothing by default."""

    def _enqueue_step(self, actions, noise, stepped, ep):
        """THE launches of one step, in the one order that is right, and what the step returns.  `stepped`: the mask in force
        (_masked), `ep`: the EpisodeStats of a step with auto-reset, else None.
          1. the step kernel;
          2. _after_step: the per-jet rewards read the film, so they come in front of the masked reset, which overwrites it;
          3. with `ep`: the bookkeeping launch and the env's own reset under ep.finished (the caller's _masked clears that mask);
          4. the normalisation LAST: it counts the reset rows of obs, and normalises ep.final_obs without counting it;
          5. with a rollout attached (rollout), the recording launch behind all of them: it stores what the step returns."""
        self._step(actions, noise)
        self._after_step()
        if ep is not None:
            self._track(ep, stepped)
            self._reset_finished(ep)
        if self._norm_on:
            self._normalize("step", stepped, ep)
        if self._rollout is not None:
            self._record(self._rollout, stepped, ep)
        if self._norm_on:
            return self._norm.norm_obs, self._norm.norm_rwd, self.done, self.trunc, ep
        return self.obs, self.rwd, self.done, self.trunc, ep

    def step(self, actions=None, noise=None, mask=None):
        if self._rotate:
            self._next_outputs(carry=mask is not None)
        if mask is None and self._mask is None:       # the common case: one frame, no closure
            return self._enqueue_step(actions, noise, None, None)
        return self._masked(mask, lambda m: self._enqueue_step(actions, noise, m, None))

    # -- episodes ---------------------------------------------------------------------------
    @property
    def episodes(self):
        """The EpisodeStats of this env, created (zeroed) on first use."""
        ep = getattr(self, "_episodes", None)
        if ep is None:
            ep = self._episodes = EpisodeStats(self)
        return ep

    def _track(self, ep, mask):
        self._call("episode_track", self.out_buf, ep.buf, mask)

    def _reset_finished(self, ep):
        """the env's own masked reset with ep.finished as the device mask (what reset_done() launches with done.clone()); the
        caller clears the mask"""
        self._mask = ep.finished
        _lib.check(self.lib.bcn_set_mask(self.h, _ptr(ep.finished)))
        self._reset()

    def track_episodes(self, mask=None):
        """The bookkeeping launch alone, for callers who keep resetting by hand: updates `episodes` from the outputs of the last
        step() (call it once per step, before reset_done(), which overwrites the terminal rows of `obs`).  `mask`: the mask that
        step was given.  Returns the EpisodeStats."""
        if mask is not None:
            mask = _mask_u8(mask, self.batch, self.device)
        ep = self.episodes
        self._keep_track = mask           # keeps the converted mask alive behind the asynchronous launch (as _keep, _done_mask do)
        self._track(ep, mask)
        return ep

    def step_autoreset(self, actions=None, noise=None, mask=None):
        """step() with same-step auto-reset and on-device episode statistics: the step kernel, ONE bookkeeping launch
        (csrc/episode.hip) and the env's own masked reset of the replicas that finished (done | trunc) -- three launches, no host
        synchronisation, nothing allocated after the first call.  Returns (obs, rwd, done, trunc, info):
          rwd, done, trunc  the terminal step's;
          obs               rows of finished replicas hold the RESET observation (the first of the next episode);
          info              `episodes` (EpisodeStats): info.final_obs rows hold the terminal observation -- what bootstrapping on
                            truncation needs -- info.finished says which rows are fresh, and ret / len / last_ret / last_len /
                            count / sum_ret / sum_len are the running statistics.
        Bit for bit what step(...); final = obs.clone(); reset_done() computes.  `mask`: as in step(); a skipped replica keeps
        state, output rows and statistics, and is not reset even when its stale done byte is 1.  With double_buffer() it acts
        on the buffer the step just wrote.
        Not covered: restore() / fork() do not move episode statistics (EpisodeStats.clear(mask) after a fork); ShardedVecEnv has
        no step_autoreset; the single-env mirrors (beacon_amd/envs.py) neither; next-step autoreset mode is not offered."""
        ep = self.episodes
        if self._rotate:
            self._next_outputs(carry=mask is not None)
        return self._masked(mask, lambda m: self._enqueue_step(actions, noise, m, ep))

    # -- rollout storage --------------------------------------------------------------------
    def rollout(self, T, final_obs=True):
        """Attach on-device rollout storage for T steps and return it (Rollout; csrc/rollout.hip).  While attached, step(),
        step_autoreset() and every step a capture() records enqueue ONE recording launch (and the one lane that advances the
        cursor) LAST -- behind the masked reset and the normalisation -- which stores the step's observations, actions, reward,
        status, flags, validity and, under step_autoreset() with final_obs=True, the terminal observations of the replicas that
        finished, into the slot the device cursor names; reset() records nothing.  No host synchronisation, nothing allocated
        after the attach.  The loop:
            ro = env.rollout(T); ro.begin()
            for t in range(T): env.step_autoreset(policy(ro.obs[t]))
            ro.compute_gae(critic(ro.obs)[:-1], critic(ro.obs)[-1], final_values=critic(ro.final_obs))
        Unlike episodes.final_obs, which keeps the LAST terminal observation of a replica, ro.final_obs keeps the one of every
        step, so a rollout that crosses two episode ends of one replica can bootstrap both.
        The buffer is allocated by the first call and reused by later calls with the same T, final_obs and jet setting (a
        VecShkadov with set_jet_rewards() on gets the rwd_jets segment; the setting is read at attach time).  rollout(None)
        detaches -- the default, in which every call launches exactly what it always did -- keeps the buffer and returns it.
        With StepGraph, keep_steps=False plus a rollout is the lean form: the per-step copies of keep_steps store a subset of
        what the rollout holds.  A graph records whether a rollout was attached at capture().
        The rollout is bookkeeping, like `episodes`: it is in no Snapshot, snapshot_signature() does not change, restore() /
        fork() leave it where it is.  ShardedVecEnv does not offer this, the single-env mirrors neither."""
        if T is None:
            self._rollout = None
            return self._rollout_kept
        jets = bool(getattr(self, "_jets_on", False))
        ro = self._rollout_kept
        want = (_lib.RO_FINAL_OBS if final_obs else 0) | (_lib.RO_JETS if jets else 0)
        if ro is None or (ro.T, ro.flags) != (int(T), want):
            ro = Rollout(self, T, final_obs)
        if self._rollout_kept is None:
            self._rollout_kept = ro
            self._merge_rollout_ops()
        self._rollout_kept = self._rollout = ro
        return ro

    def _merge_rollout_ops(self):
        """_ROLLOUT_OPS into this env's tables of both bindings (they are in neither _op_table() nor _c_table())."""
        ops, cfn = _rollout_tables(self.lib, self._ops is not None)
        if self._ops is not None:
            if ops is None:
                raise RuntimeError("the torch extension in use lacks the rollout ops: rebuild it (beacon_amd/torch_ext.py)")
            self._ops = dict(self._ops, **ops)
        self._cfn = dict(self._cfn, **cfn)

    def _record(self, ro, stepped, ep):
        """the recording launch of one step: the sources are the normaliser's, the episode buffer's and the per-jet buffer's exactly
        when those are in play"""
        k = self._keep                    # what _step handed the kernel: the converted actions (with the noise, for the envs that take it)
        jets = getattr(self, "_jets", None) if (ro.flags & _lib.RO_JETS and getattr(self, "_jets_on", False)) else None
        self._call("rollout_record", self.out_buf, ro.buf, k[0] if isinstance(k, tuple) else k, None if ep is None else ep.buf,
                   self._norm.buf if self._norm_on else None, None if jets is None else jets.buf, stepped, ro.T, ro.flags)

    # -- running normalisation --------------------------------------------------------------
    def set_normalize(self, on=True, gamma=0.99, eps=1e-8, clip_obs=10.0, clip_rwd=10.0, training=True):
        """Running normalisation of observations and rewards on the device (the VecNormalize wrapper of the RL libraries; Normalizer,
        csrc/normalize.hip).  While on, reset(), reset_done(), step(), step_autoreset() and every step a capture() records
        (autoreset=True included) enqueue bcn_normalize LAST -- in step_autoreset() behind the masked reset -- and return
        `normalizer.norm_obs` and `normalizer.norm_rwd` in place of obs and rwd: two small launches, one with training=False; no
        host synchronisation, nothing allocated after the first call.  Per call, over the replicas S that were stepped (or reset)
        and whose status holds neither BCN_ST_ITMAX nor BCN_ST_BLOWUP (a reset ignores the status):
          observations  the batch mean and the sum of squared deviations of every column over S are merged into obs_mean / obs_var /
                        obs_count; norm_obs = clip((obs - obs_mean) / sqrt(obs_var + eps), +-clip_obs) with the merged statistics
          rewards       ret = gamma ret + rwd; ret_mean / ret_var / ret_count merged from ret over S; norm_rwd = clip(rwd /
                        sqrt(ret_var + eps), +-clip_rwd); ret = 0 where done | trunc.  A reset zeroes ret of the replicas it touches
          step_autoreset  the reset rows of obs are what is counted; the terminal rows, info.final_obs, are normalised into
                        normalizer.norm_final_obs (where info.finished) with the same statistics and not counted
        all in float64, rounded once to the env dtype.  training=False (evaluation) applies the statistics and changes none;
        `normalizer.training` can be flipped at any time.  A replica a mask skips keeps its rows and its ret.  A StepGraph
        captured while on also has norm_obs_seq / norm_rwd_seq (keep_steps); the settings are recorded at capture().
        obs, rwd, done, trunc, status and the env's state are untouched: they are bit for bit those of an env without the
        feature.  set_normalize(False) -- the default, in which every call launches exactly what it always did -- keeps the
        Normalizer and its statistics.
        The normaliser is bookkeeping, like `episodes`: it is in no Snapshot, snapshot_signature() does not change, restore() /
        fork() leave it where it is; Normalizer.state_dict() / load_state_dict() carry it to a checkpoint or an evaluation env.
        ShardedVecEnv does not offer this (each rank would hold its own statistics), the single-env mirrors neither."""
        if on:
            if not (0.0 <= float(gamma) <= 1.0) or not float(eps) > 0.0 or not float(clip_obs) > 0.0 or not float(clip_rwd) > 0.0:
                raise ValueError("%s.set_normalize: gamma must lie in [0, 1], eps, clip_obs and clip_rwd must be > 0"
                                 % type(self).__name__)
            if self._norm is None:
                self._norm = Normalizer(self)
            nz = self._norm
            nz.gamma, nz.eps, nz.clip_obs, nz.clip_rwd, nz.training = float(gamma), float(eps), float(clip_obs), float(clip_rwd), bool(training)
        self._norm_on = bool(on)
        return self

    @property
    def normalizer(self):
        """The Normalizer of this env (set_normalize)."""
        if not self._norm_on or self._norm is None:
            raise AttributeError("%s.normalizer: normalisation is off -- call set_normalize() first" % type(self).__name__)
        return self._norm

    def _normalize(self, kind, mask, ep=None):
        nz = self._norm
        self._call("normalize", self.out_buf, nz.buf, None if ep is None else ep.buf, mask, Normalizer.KINDS[kind], int(nz.training),
                   nz.gamma, nz.eps, nz.clip_obs, nz.clip_rwd)

    def normalize_outputs(self, mask=None, kind="step", episodes=None):
        """The normalising launch alone, the counterpart of track_episodes(): for callers who sequence things by hand.  Updates
        `normalizer` from the current outputs (obs, rwd, status, done, trunc).  `mask`: the mask the step or reset was given;
        kind: "step" or "reset"; episodes: an EpisodeStats whose final_obs rows are normalised where `finished` (what
        step_autoreset() passes).  Needs set_normalize().  Returns the Normalizer."""
        nz = self.normalizer
        if kind not in Normalizer.KINDS:
            raise ValueError("%s.normalize_outputs: kind %r; \"step\" or \"reset\"" % (type(self).__name__, kind))
        if mask is not None:
            mask = _mask_u8(mask, self.batch, self.device)
        self._keep_norm = mask            # alive behind the asynchronous launch
        self._normalize(kind, mask, episodes)
        return nz

    def capture(self, actions, noise=None, n_steps=None, keep_steps=True, autoreset=False):
        """Record step() calls into ONE HIP graph (torch.cuda.CUDAGraph) and return it as a StepGraph: replay()
        relaunches them with a single host call.  step() only enqueues work on the current stream (no host
        synchronisation, no host read), so it can be captured -- on its own, as here, or inside a caller's graph next to
        the policy network.  For the 1D envs at the reference batch sizes the kernel of one step (38 us, burgers B=1024)
        is shorter than the host work of launching it through Python; a graph of n steps runs at the kernel rate.
        `actions` (and `noise`): STATIC device tensors the graph reads at every replay -- [B, ...] for one step, or
        [n_steps, B, ...] for n_steps steps (step k uses actions[k]); overwrite them in place between replays.
        keep_steps=False leaves out the per-step copies of obs / rwd / done / trunc (only the last step's stay, in the
        env's own tensors): every extra graph node costs a few microseconds between two kernels.
        The recorded kernels keep the noise seed / sigma they were captured with (set_noise_seed): change the seed, then
        capture again.
        autoreset=True records step_autoreset() instead: per step the step kernel, the bookkeeping launch and the masked reset, so
        a replayed rollout crosses episode ends.  obs_seq[k] then holds the post-reset observations, done_seq / trunc_seq the
        terminal flags, and `episodes` accumulates across replays (its final_obs holds the LAST terminal observation of each
        replica).  The default records exactly the step() calls.
        With a rollout attached (rollout) every recorded step is followed by the recording launch, and keep_steps keeps its
        default: keep_steps=False plus a rollout is the lean form, begin() between replays starts the next rollout."""
        return StepGraph(self, actions, noise, n_steps, keep_steps, autoreset)

    # -- frames -----------------------------------------------------------------------------
    def _render_range(self):
        """(lo, hi, ref) of the reference's render(): the colour range of the field panel / the axes of the line panel."""
        raise NotImplementedError

    def _render_cfg(self, scale, width, height, strip, field, vmin, vmax, ref):
        """The bcn_render_cfg of a renderer() call, checked on the host before the library or the device is touched."""
        who = type(self).__name__ + ".renderer"
        if self._panel is None:
            raise ValueError("%s: this env keeps no trajectory on the device: there is nothing to draw" % who)
        if field not in _lib.PLANES:
            raise ValueError("%s: field %r; one of %s" % (who, field, ", ".join(sorted(_lib.PLANES))))
        if (vmin is None) != (vmax is None):
            raise ValueError("%s: vmin and vmax go together" % who)
        if self._panel == "field":
            if int(scale) < 1:
                raise ValueError("%s: scale = %r; an integer >= 1" % (who, scale))
            if vmin is None and field != "scalar":
                raise ValueError("%s: field %r has no default range: pass vmin and vmax" % (who, field))
        else:
            if field != "scalar":
                raise ValueError("%s: field %r belongs to the 2D envs" % (who, field))
            if int(width) < 1 or int(height) < 1:
                raise ValueError("%s: width and height must be >= 1" % who)
        lo, hi, r = self._render_range()
        if vmin is not None:
            lo, hi = float(vmin), float(vmax)
        if ref is not None:
            r = float(ref)
        if not (math.isfinite(lo) and math.isfinite(hi) and math.isfinite(r) and hi > lo):
            raise ValueError("%s: range (%r, %r), ref %r: finite values with vmax > vmin" % (who, lo, hi, r))
        if strip is not None and int(strip) < 0:
            raise ValueError("%s: strip = %r rows; >= 0, or None for an eighth of the panel" % (who, strip))
        return _lib.RenderCfg(plane=_lib.PLANES[field], scale=int(scale), width=int(width), height=int(height),
                              strip=-1 if strip is None else int(strip), has_range=1, lo=lo, hi=hi, ref=r)

    def renderer(self, replicas=None, scale=1, width=512, height=128, strip=None, field="scalar", vmin=None, vmax=None, lut=None,
                 ref=None):
        """A Renderer: uint8 RGB frames [n, H_px, W_px, 3] of the replicas `replicas` (a list / array / tensor of indices, in that
        order; None: all), painted on the device from the state the step kernels leave -- ONE launch per draw(), no download
        (csrc/render.hip; the pixel rules: include/beacon_hip.h, bcn_render).
          rayleigh, mixing     the field panel: `field` ("scalar": T / C, or "u", "v", "p") with every cell `scale` x `scale` pixels, top
                               row = top of the domain, coloured through `lut` (uint8 [256, 3]; None: render.colormap_lut(), RdBu_r)
                               over (vmin, vmax) -- default (Tc, Th) / (0, C0) as in the reference; u, v, p need a range
          burgers u, shkadov h, sloshing h   the line panel, `width` x `height` pixels over (vmin, vmax) with the level `ref` in grey --
                               default the reference's axes: u_target -+ 2 sigma and u_target; (0, 2) and 1; (0.25, 1.75) and 1; a
                               replica with a non-finite sample shows red columns
          under it             `strip` rows of control bars (None: an eighth of the panel; 0: none): the stored action, red up for
                               positive and blue down for negative; shkadov's jets take equal cells, not their place along the film
        draw() enqueues the launch and returns the renderer's own buffer, so it allocates nothing and can be recorded inside
        torch.cuda.graph or called in a loop next to step().  ValueError, before anything touches the device, for scale < 1, an
        unknown field, u / v / p without a range, vmax <= vmin, and for the ODE envs (lorenz, vortex)."""
        cfg = self._render_cfg(scale, width, height, strip, field, vmin, vmax, ref)
        if not self._render_merged:
            self._merge_render_ops()
        return Renderer(self, cfg, replicas, lut)

    def _merge_render_ops(self):
        """_RENDER_OPS into this env's tables of both bindings, as _merge_rollout_ops."""
        ops, cfn = _render_tables(self.lib, self._ops is not None)
        if self._ops is not None:
            if ops is None:
                raise RuntimeError("the torch extension in use lacks the render op: rebuild it (beacon_amd/torch_ext.py)")
            self._ops = dict(self._ops, **ops)
        self._cfn = dict(self._cfn, **cfn)
        self._render_merged = True

    def render_rgb(self, **kw):
        """One-shot convenience: renderer(**kw).draw() -- a fresh buffer per call; keep a Renderer for a loop."""
        return self.renderer(**kw).draw()

    def reset_done(self):
        """Auto-reset: re-initialise the replicas whose last step() returned done (their rows of
        `obs` become the reset observation).  Entirely on the device, no host synchronisation."""
        self._done_mask = self.done.clone()
        return self.reset(mask=self._done_mask)

    def warmup(self, n_steps, actions=None):
        """Equivalent of the reference's init.py generators (rayleigh/init.py:13-28): n uncontrolled action steps
        (zero / repeated action), e.g. to develop the flow on a grid that ships no init_field.dat.  The per-step
        rewards are kept in `self.warmup_rwd` [n_steps, B] (rayleigh: minus the Nusselt history the reference's
        generator plots); episode counters are reset afterwards."""
        rw = []
        for _ in range(int(n_steps)):
            self._step(actions, None)
            rw.append(self.rwd.clone())
        self.warmup_rwd = torch.stack(rw) if rw else torch.empty((0, self.batch), dtype=self.tdtype, device=self.device)
        self.check_status()
        self.set_stp(0)
        return self.get_state()


class StepGraph(object):
    """n step() calls (autoreset: step_autoreset() calls) of one VecEnv on static inputs, as a HIP graph (VecEnv.capture).  After replay() the env's own
    obs / rwd / done / trunc hold the last step's results; `obs_seq`, `rwd_seq`, `done_seq`, `trunc_seq` ([n, B, ...])
    hold every step's -- and `rwd_jets_seq` ([n, B, n_jets]) for a VecShkadov captured with set_jet_rewards() on, `norm_obs_seq` /
    `norm_rwd_seq` (the shapes of obs_seq / rwd_seq) for an env captured with set_normalize() on."""

    def __init__(self, env, actions, noise=None, n_steps=None, keep_steps=True, autoreset=False):
        self.env, self.actions, self.noise, self.autoreset = env, actions, noise, bool(autoreset)
        ep = env.episodes if autoreset else None          # allocated before the capture
        self.n = 1 if n_steps is None else int(n_steps)
        seq = n_steps is not None
        n = self.n if keep_steps else 0
        self.obs_seq = torch.empty((n,) + tuple(env.obs.shape), dtype=env.obs.dtype, device=env.device)
        self.rwd_seq = torch.empty((n,) + tuple(env.rwd.shape), dtype=env.rwd.dtype, device=env.device)
        self.done_seq = torch.empty((n,) + tuple(env.done.shape), dtype=env.done.dtype, device=env.device)
        self.trunc_seq = torch.empty((n,) + tuple(env.trunc.shape), dtype=env.trunc.dtype, device=env.device)
        jets = getattr(env, "_jets", None) if getattr(env, "_jets_on", False) else None      # VecShkadov.set_jet_rewards
        if jets is not None:
            self.rwd_jets_seq = torch.empty((n,) + tuple(jets.rwd_jets.shape), dtype=jets.rwd_jets.dtype, device=env.device)
        norm = env._norm if env._norm_on else None                                            # VecEnv.set_normalize
        if norm is not None:
            self.norm_obs_seq = torch.empty_like(self.obs_seq)
            self.norm_rwd_seq = torch.empty_like(self.rwd_seq)
        self.graph = torch.cuda.CUDAGraph()
        gen = getattr(env, "gen", None)
        if gen is not None and noise is None:
            self.graph.register_generator_state(gen)      # the env draws its own noise: a graph-safe generator
        torch.cuda.synchronize(env.device)
        with torch.cuda.graph(self.graph):
            for k in range(self.n):
                a = actions[k] if seq else actions
                z = None if noise is None else (noise[k] if seq else noise)
                env._masked(None, lambda m: env._enqueue_step(a, z, m, ep))
                if not keep_steps:
                    continue
                self.obs_seq[k].copy_(env.obs)
                self.rwd_seq[k].copy_(env.rwd)
                self.done_seq[k].copy_(env.done)
                self.trunc_seq[k].copy_(env.trunc)
                if jets is not None:
                    self.rwd_jets_seq[k].copy_(jets.rwd_jets)
                if norm is not None:
                    self.norm_obs_seq[k].copy_(norm.norm_obs)
                    self.norm_rwd_seq[k].copy_(norm.norm_rwd)

    def replay(self):
        self.graph.replay()
        return self.obs_seq, self.rwd_seq, self.done_seq, self.trunc_seq


# ---------------------------------------------------------------------------------------------
class _VecNS2D(VecEnv):
    """What the two 2D envs (rayleigh, mixing) share on the host."""

    _kind = 0                # BCN_RAYLEIGH / BCN_MIXING
    _params_kernel = "generic"
    _panel = "field"

    def set_ndt_act(self, n):
        """Test hook: shorten the action step (the goldens for big grids use ndt_act=5).  The handle is built anew."""
        self.close()
        self.ndt_act = int(n)
        self.h = C.c_void_p()
        self._create()
        self._apply_params_kernel()
        self._reapply_params()
        self.sweeps = torch.zeros((self.batch, self.ndt_act), dtype=torch.int32, device=self.device)

    def state_shape(self):
        return (4, self.ny + 2, self.nx + 2)

    def set_params_kernel(self, which):
        """Which kernel steps this env while per-replica parameters are set (set_params): "generic" (the default) -- the generic
        kernel -- or "fast" -- the env's register-resident kernel in its table-reading form (include/beacon_hip.h: option
        "params_kernel"; built into the library for the built-in grids).  On a grid with an on-demand kernel, "fast" builds that
        kernel's table-reading twin (beacon_amd/jit.py: PRM_DEFS, a shared object of its own), compares it with the generic kernel
        under a per-replica table before its first use, and attaches it; a twin that cannot be built or fails the comparison
        warns with JitWarning and leaves the generic kernel in charge of steps with a table.  The choice survives set_ndt_act.
        With "fast" a replica computes, bit for bit, what an env constructed with its parameters computes.  Returns self."""
        if which not in ("fast", "generic"):
            raise ValueError("%s.set_params_kernel: %r; \"fast\" or \"generic\"" % (type(self).__name__, which))
        self._params_kernel = which
        self._apply_params_kernel()
        return self

    @property
    def cell_runs_active(self):
        """Whether the next step under variant 1 goes through the library's float32 kernels with the Jacobi cells in runs
        (csrc/ns2d_fast_runs.hip): False for float64, for an env on a kernel plugin (the plugin says it of itself:
        bcn_jit_cell_runs), for a grid that unit does not have, and after set_option("cell_runs", 0), which sends the env to the
        cell-by-cell kernels of the same grid (include/beacon_hip.h: option "cell_runs").  The library answers from the predicate
        its dispatch uses.  Like every option, "cell_runs" is lost when set_ndt_act builds the handle anew."""
        fn = self.lib.bcn_cell_runs_active          # an internal query of the library, like bcn_jit_builtin: not in _lib.SIGNATURES
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p]
        return bool(fn(self.h))

    def _apply_params_kernel(self):
        fast = self._params_kernel == "fast"
        _lib.check(self.lib.bcn_set_option(self.h, b"params_kernel", 1 if fast else 0))
        if fast and getattr(self, "_plugin", None) is not None:
            self._attach_plugin_params()

    def _attach_plugin_params(self):
        """The table-reading twin of this env's on-demand kernel: built, verified at its first use (jit.verify with a per-replica
        table) and handed to the library (bcn_set_fast_plugin_params)."""
        from . import jit
        f64 = self.tdtype == torch.float64
        defs = dict(self._plugin_defs or {})
        defs.update(self._plugin_prm_defs or {})
        defs.update(jit.PRM_DEFS)
        p = jit.plugin_for(self.nx, self.ny, f64, self._kind, defs)
        if p is None or p.fn_prm is None:
            return
        if p.verified is None and not jit.CHECKING:
            ctor, cls, dev, dt = dict(self._ctor), type(self), self.device, dtype_name(self.tdtype)
            jit.verify(p, lambda batch: cls(batch, dev, dt, **ctor), self._kind, f64, params=True)
        if p.verified or jit.CHECKING:
            _lib.check(self.lib.bcn_set_fast_plugin_params(self.h, p.fn_prm))
            self._plugin_prm = p


class VecRayleigh(_VecNS2D):
    """rayleigh/rayleigh.py:16-366.  `init_fields`: [4, nx+2, ny+2] in the reference's [i, j]
    layout (u, v, p, T) -- what load() parses from init_field.dat (:356-362) -- or None
    (init=False: all-zero fields)."""

    PARAMS = ("ra",)

    def _render_range(self):
        return float(self.Tc), float(self.Th), 0.0               # rayleigh.py:306-308

    def __init__(self, batch, device="cuda:0", dtype="f32", init_fields=None,
                 L=1.0, H=1.0, n_sgts=10, ra=1.0e4):
        self._derive(L, H, n_sgts, ra)
        self._ctor = dict(L=L, H=H, n_sgts=n_sgts, ra=ra)     # a twin of this env (the JIT self-check builds some)
        self._init_np = None if init_fields is None else np.asarray(init_fields, dtype=np.float64)
        super().__init__(batch, device, dtype)
        self._post_init()

    def _derive(self, L=1.0, H=1.0, n_sgts=10, ra=1.0e4):
        self.L, self.H, self.ra, self.n_sgts = L, H, ra, n_sgts
        self.nx, self.ny = int(50 * L), int(50 * H)                       # :26-27
        self.pr, self.Tc, self.Th, self.C = 0.71, -0.5, 0.5, 0.75         # :29-32
        self.dt, self.dt_act, self.t_warmup, self.t_act = 0.01, 2.0, 200.0, 200.0
        self.nx_obs_pts, self.ny_obs_pts, self.n_obs_steps = 4 * int(L), 4 * int(H), 4
        self.dx, self.dy = float(L / self.nx), float(H / self.ny)         # :45-46
        self.ndt_act = int(self.dt_act / self.dt)                         # :48
        self.n_act = int(self.t_act / self.dt_act)                        # :50
        self.n_warmup = int(self.t_warmup / self.dt_act)
        self.nx_sgts = self.nx // n_sgts                                  # :52
        self.n_obs_tot = 3 * self.n_obs_steps * self.nx_obs_pts * self.ny_obs_pts
        self.nx_obs, self.ny_obs = self.nx // self.nx_obs_pts, self.ny // self.ny_obs_pts
        self.tol, self.itmax = 1.0e-8, 300000                             # :414-417
        return self

    def _make_spaces(self):
        self.action_space = spaces.box(-self.C, self.C, (self.n_sgts,))         # rayleigh.py:75-78
        self.observation_space = spaces.sym_box(1.0, self.n_obs_tot)            # :81-86
        return self

    def _post_init(self):
        n_sgts = self.n_sgts
        self._make_spaces()
        self.actions_norm = torch.zeros((self.batch, n_sgts), dtype=self.tdtype, device=self.device)
        self.sweeps = torch.zeros((self.batch, self.ndt_act), dtype=torch.int32, device=self.device)
        self._init_dev = None
        if self._init_np is not None:
            assert self._init_np.shape == (4, self.nx + 2, self.ny + 2)
            # reference arrays are [i, j]; the device layout is [j, i] (x fastest)
            self._init_dev = self._real(np.ascontiguousarray(self._init_np.transpose(0, 2, 1)),
                                        (4, self.ny + 2, self.nx + 2))

    def _create(self):
        c = _lib.RayleighCfg(nx=self.nx, ny=self.ny, ndt_act=self.ndt_act, n_act=self.n_act,
                             n_sgts=self.n_sgts, nx_sgts=self.nx_sgts, nx_obs_pts=self.nx_obs_pts,
                             ny_obs_pts=self.ny_obs_pts, nx_obs=self.nx_obs, ny_obs=self.ny_obs,
                             n_obs_steps=self.n_obs_steps, itmax=self.itmax, dx=self.dx, dy=self.dy,
                             dt=self.dt, pr=self.pr, ra=self.ra, Tc=self.Tc, Th=self.Th, C=self.C,
                             tol=self.tol)
        self.cfg = c
        _lib.check(self.lib.bcn_rayleigh_create(C.byref(c), self.batch, self.cdtype, self.dev_index,
                                                C.byref(self.h)))
        self._attach_plugin(0)
        self._slow_mode_bound(0)

    def perturbed_conduction_state(self, seed=2024):
        """Start state of a warm-up on a grid without an init file, [4, nx+2, ny+2] in the reference's [i, j] layout:
        u = v = p = 0, T = the conduction profile plus five seeded long-wave perturbations of amplitude <= 0.02 (from
        the reference's all-zero start, rayleigh/init.py:13, an exactly x-uniform state never leaves pure conduction)."""
        rng = np.random.default_rng(seed)
        xm = (np.arange(self.nx + 2) - 0.5) * self.dx
        ym = (np.arange(self.ny + 2) - 0.5) * self.dy
        X, Y = np.meshgrid(xm, ym, indexing="ij")
        T = self.Th + (self.Tc - self.Th) * Y / self.H
        for k in range(1, 6):
            T += 0.02 * rng.uniform(-1, 1) * np.sin(np.pi * Y / self.H) * np.cos(k * np.pi * X / self.L + rng.uniform(0, 6.28))
        T[:, 0] = 0.0
        T[:, -1] = 0.0
        st = np.zeros((4, self.nx + 2, self.ny + 2))
        st[3] = T
        return st

    def develop(self, n_steps=None, seed=2024):
        """The reference's init.py on the device (rayleigh/init.py:13-28: n_warmup uncontrolled action steps, then
        dump): every replica starts from perturbed_conduction_state(seed) and takes n_steps (default n_warmup = 100)
        zero-action steps.  Returns the developed fields of replica 0 as [4, nx+2, ny+2] float64 in the reference's
        layout -- what VecRayleigh(init_fields=...) takes -- and keeps minus the Nusselt history in `warmup_rwd`."""
        st0 = self.perturbed_conduction_state(seed)
        self.reset()
        self.set_state(np.tile(np.ascontiguousarray(st0.transpose(0, 2, 1))[None], (self.batch, 1, 1, 1)))
        zero = torch.zeros((self.batch, self.n_sgts), dtype=self.tdtype, device=self.device)
        st = self.warmup(self.n_warmup if n_steps is None else n_steps, zero)
        return np.ascontiguousarray(st[0].double().cpu().numpy().transpose(0, 2, 1))

    def _reset(self):
        self._call("rayleigh_reset", self._init_dev, self.obs)

    def _step(self, actions, noise=None):
        a = self._real(actions, (self.batch, self.n_sgts))
        self._keep = a
        self._call("rayleigh_step", a, self.actions_norm, self.obs, self.rwd, self.done, self.trunc, self.status, self.sweeps)


class VecMixing(_VecNS2D):
    """mixing/mixing.py:16-378"""

    PARAMS = ("re", "pe")
    _kind = 1

    action_is_int = True

    def _render_range(self):
        return 0.0, float(self.C0), 0.0                          # mixing.py:296-298

    def __init__(self, batch, device="cuda:0", dtype="f32", L=1.0, H=1.0, re=100.0, pe=10000.0,
                 side=0.5, C0=1.0):
        self._derive(L, H, re, pe, side, C0)
        self._ctor = dict(L=L, H=H, re=re, pe=pe, side=side, C0=C0)
        super().__init__(batch, device, dtype)
        self._make_spaces()
        self.sweeps = torch.zeros((self.batch, self.ndt_act), dtype=torch.int32, device=self.device)

    def _make_spaces(self):
        self.action_space = spaces.discrete(4)                                  # mixing.py:61
        self.observation_space = spaces.sym_box(1.0, self.n_obs_tot)            # :65-70
        return self

    def _derive(self, L=1.0, H=1.0, re=100.0, pe=10000.0, side=0.5, C0=1.0):
        self.L, self.H, self.re, self.pe, self.side, self.C0 = L, H, re, pe, side, C0
        self.nx, self.ny = int(100 * L), int(100 * H)                    # :27-28
        self.nu = 0.01
        self.u_max = re * self.nu / L                                    # :34
        self.dt, self.dt_act, self.t_act = 0.002, 0.5, 50.0
        self.nx_obs_pts, self.ny_obs_pts, self.n_obs_steps = 4 * int(L), 4 * int(H), 4
        self.dx, self.dy = float(L / self.nx), float(H / self.ny)
        self.ndt_act = int(self.dt_act / self.dt)
        self.n_act = int(self.t_act / self.dt_act)
        self.n_obs_tot = 3 * self.n_obs_steps * self.nx_obs_pts * self.ny_obs_pts
        self.nx_obs, self.ny_obs = self.nx // self.nx_obs_pts, self.ny // self.ny_obs_pts
        self.tol, self.itmax = 1.0e-4, 300000                            # :423-426
        self.i_min = math.floor(0.5 * (L - side) / self.dx)              # :90-93
        self.i_max = self.i_min + math.floor(side / self.dx)
        self.j_min = math.floor(0.5 * (H - side) / self.dy)
        self.j_max = self.j_min + math.floor(side / self.dy)
        return self

    def _create(self):
        c = _lib.MixingCfg(nx=self.nx, ny=self.ny, ndt_act=self.ndt_act, n_act=self.n_act,
                           nx_obs_pts=self.nx_obs_pts, ny_obs_pts=self.ny_obs_pts, nx_obs=self.nx_obs,
                           ny_obs=self.ny_obs, n_obs_steps=self.n_obs_steps, itmax=self.itmax,
                           i_min=self.i_min, i_max=self.i_max, j_min=self.j_min, j_max=self.j_max,
                           dx=self.dx, dy=self.dy, dt=self.dt, re=self.re, pe=self.pe, u_max=self.u_max,
                           C0=self.C0, ref_c=(self.side * self.side) / (self.L * self.H) * self.C0,
                           tol=self.tol)
        self.cfg = c
        _lib.check(self.lib.bcn_mixing_create(C.byref(c), self.batch, self.cdtype, self.dev_index,
                                              C.byref(self.h)))
        self._attach_plugin(1)
        self._slow_mode_bound(1)

    def _reset(self):
        self._call("mixing_reset", self.obs)

    def _step(self, actions, noise=None):
        a = self._int_actions(actions)
        self._keep = a
        self._call("mixing_step", a, self.obs, self.rwd, self.done, self.trunc, self.status, self.sweeps)


class VecBurgers(VecEnv):
    """burgers/burgers.py:17-227.  `nx` is a kwarg here (a literal 500 in the reference, :26)."""

    PARAMS = ("u_target", "amp")

    needs_noise = True
    _panel = "line"

    def _render_range(self):
        return self.u_target - 2 * self.sigma, self.u_target + 2 * self.sigma, float(self.u_target)   # burgers.py:184-189

    def __init__(self, batch, device="cuda:0", dtype="f32", u_target=0.5, amp=10.0, sigma=0.1,
                 ctrl_pos=1.0, L=2.0, nx=500, seed=0):
        self._derive(u_target, amp, sigma, ctrl_pos, L, nx)
        self._ctor = dict(u_target=u_target, amp=amp, sigma=sigma, ctrl_pos=ctrl_pos, L=L, nx=nx, seed=seed)
        super().__init__(batch, device, dtype)
        self._make_spaces()
        self._noise_setup(seed)

    def _make_spaces(self):
        self.action_space = spaces.box(-1.0, 1.0, (1,))                         # burgers.py:54-57
        self.observation_space = spaces.box(np.zeros(self.n_obs_pts), np.ones(self.n_obs_pts), (self.n_obs_pts,))  # :60-65
        return self

    def _derive(self, u_target=0.5, amp=10.0, sigma=0.1, ctrl_pos=1.0, L=2.0, nx=500):
        self.L, self.nx, self.amp, self.sigma, self.u_target = L, nx, amp, sigma, u_target
        self.t_max, self.dt_act, self.n_obs_pts = 10.0, 0.05, 5
        self.dx = float(L / nx)                                          # :36
        self.ctrl_pos = int(ctrl_pos / self.dx)                          # :37
        self.dt = 0.2 * self.dx                                          # :38
        self.ndt_act = int(self.dt_act / self.dt)                        # :40
        self.n_act = int(self.t_max / self.dt_act)                       # :42
        return self

    def _create(self):
        c = _lib.BurgersCfg(nx=self.nx, ndt_act=self.ndt_act, n_act=self.n_act, ctrl_pos=self.ctrl_pos,
                            n_obs_pts=self.n_obs_pts, dx=self.dx, dt=self.dt, amp=self.amp,
                            u_target=self.u_target)
        self.cfg = c
        _lib.check(self.lib.bcn_burgers_create(C.byref(c), self.batch, self.cdtype, self.dev_index,
                                               C.byref(self.h)))

    def state_shape(self):
        return (3, self.nx)

    def draw_noise(self):
        """An explicit noise tensor of the reference's law, np.random.uniform(-sigma, sigma, 1) (burgers.py:127), from the
        env's torch generator -- for callers that want to see or reuse the draws.  step(a) without `noise` needs none:
        the kernel draws its own (set_noise_seed)."""
        r = torch.rand((self.batch,), generator=self.gen, device=self.device, dtype=self.tdtype)
        return (2.0 * r - 1.0) * self.sigma

    def _reset(self):
        self._call("burgers_reset", self.obs)

    def _step(self, actions, noise=None):
        a = self._real(actions, (self.batch,))
        nz = None if noise is None else self._real(noise, (self.batch,))     # None: drawn inside the kernel
        self._keep = (a, nz)
        self._call("burgers_step", a, nz, self.obs, self.rwd, self.done, self.trunc, self.status)


class VecShkadov(VecEnv):
    """shkadov/shkadov.py:16-372.  `init_fields`: [2, >=nx] (h_init, q_init) as load() parses
    them (:364-368), or None for the flat film h=q=1."""

    PARAMS = ("delta",)

    needs_noise = True
    _panel = "line"
    rand_steps = None        # set_random_init: None = every reset restarts from the film itself
    _jets = None             # set_jet_rewards: the JetStats, allocated by the first call and kept
    _jets_on = False         # ... whether the per-jet launch follows every step
    _jets_stats = 0          # ... and whether it keeps the per-jet returns (the kernel's with_stats)

    def _render_range(self):
        return 0.0, 2.0, 1.0                                     # shkadov.py:287-291

    def __init__(self, batch, device="cuda:0", dtype="f32", init_fields=None, L0=150.0, n_jets=5,
                 jet_pos=150.0, jet_space=10.0, delta=0.1, t_act=20.0, seed=0):
        self._derive(L0, n_jets, jet_pos, jet_space, delta, t_act)
        self._ctor = dict(L0=L0, n_jets=n_jets, jet_pos=jet_pos, jet_space=jet_space, delta=delta, t_act=t_act, seed=seed)
        self._init_np = None if init_fields is None else np.asarray(init_fields, dtype=np.float64)
        super().__init__(batch, device, dtype)
        self._make_spaces()
        self._noise_setup(seed)
        self._init_dev = None
        if self._init_np is not None:
            self._init_dev = self._real(np.ascontiguousarray(self._init_np[:, :self.nx]), (2, self.nx))
        self.rand_steps = None                     # set_random_init: None = reset() restarts from the packaged film itself
        self._n_rand = torch.zeros((self.batch,), dtype=torch.int32, device=self.device)   # written by the fused reset
        self.n_rand = self._n_rand

    def _make_spaces(self):
        self.action_space = spaces.box(-1.0, 1.0, (self.n_jets,))               # shkadov.py:96-99
        self.observation_space = spaces.sym_box(1.0, self.n_obs * self.n_jets)  # :105-110
        return self

    def _derive(self, L0=150.0, n_jets=5, jet_pos=150.0, jet_space=10.0, delta=0.1, t_act=20.0):
        self.L = L0 + jet_space * (n_jets + 2)                           # :32
        self.nx = int(5 * self.L)                                        # :33
        self.dt, self.dt_act, self.t_act = 0.001, 0.05, t_act
        self.n_warmup_ref = int(200.0 / self.dt_act)                     # :36,62 t_warmup = 200 -> 4000 action steps (init.py)
        self.sigma, self.delta, self.n_jets, self.jet_amp = 5.0e-4, delta, n_jets, 5.0
        self.eps, self.blowup_rwd, self.h_max = 1.0e-8, -1.0, 5.0
        self.dx = float(self.L / self.nx)                                # :56
        self.ndt_act = int(self.dt_act / self.dt)
        self.n_act = int(t_act / self.dt_act)
        self.n_interp = int(0.02 / self.dt)                              # :63
        self.jet_pos = int(jet_pos / self.dx)                            # :64
        self.jet_hw = int(2.0 / self.dx)                                 # :65
        self.jet_space = int(jet_space / self.dx)                        # :67
        self.l_rwd = int(10.0 / self.dx)                                 # :70
        self.n_obs = int(10.0)                                           # :71
        self.l_obs = int(10.0 / self.dx)                                 # :72
        self.obs_stride = int(1.0 / self.dx)                             # :245
        return self

    def _create(self):
        c = _lib.ShkadovCfg(nx=self.nx, ndt_act=self.ndt_act, n_act=self.n_act, n_jets=self.n_jets,
                            jet_pos=self.jet_pos, jet_hw=self.jet_hw, jet_space=self.jet_space,
                            l_obs=self.l_obs, l_rwd=self.l_rwd, n_obs=self.n_obs,
                            obs_stride=self.obs_stride, n_interp=self.n_interp, dx=self.dx, dt=self.dt,
                            delta=self.delta, jet_amp=self.jet_amp, eps=self.eps,
                            h_blow=5.0 * self.h_max, blowup_rwd=self.blowup_rwd)
        self.cfg = c
        _lib.check(self.lib.bcn_shkadov_create(C.byref(c), self.batch, self.cdtype, self.dev_index,
                                               C.byref(self.h)))

    def state_shape(self):
        return (4, self.nx)

    def draw_noise(self):
        r = torch.rand((self.batch, self.ndt_act), generator=self.gen, device=self.device, dtype=self.tdtype)
        return (2.0 * r - 1.0) * self.sigma

    def reset_random(self, rand_steps=400, n_steps=None):
        """reset() followed by a per-replica random number of uncontrolled steps, the batched form
        of shkadov.reset with rand_init (shkadov.py:119-123: n = random.randint(0, rand_steps)).
        n_steps: optional explicit int tensor [B]; drawn on the device otherwise.
        This is the whole-batch HOST loop (one host synchronisation, up to rand_steps masked step() launches, counts from the
        torch generator `gen`); it cannot be captured and cannot restart only the replicas that finished.  set_random_init()
        makes every reset -- reset(mask), reset_done(), step_autoreset(), capture(..., autoreset=True) -- do the same thing in
        one kernel launch on the device."""
        jets_on, self._jets_on = self._jets_on, False          # a reset produces no rewards (set_jet_rewards)
        norm_on, self._norm_on = self._norm_on, False          # ... and is normalised once, at its end (set_normalize)
        try:
            self.reset()
            if n_steps is None:
                n_steps = torch.randint(0, rand_steps + 1, (self.batch,), generator=self.gen, device=self.device)
            n_steps = torch.as_tensor(n_steps).to(self.device)
            self.n_rand = n_steps
            for i in range(int(n_steps.max().item())):
                self.step(None, None, mask=(n_steps > i))
        finally:
            self._jets_on, self._norm_on = jets_on, norm_on
        self.set_stp(0)
        if norm_on:
            self._normalize("reset", None)
            return self._norm.norm_obs, None
        return self.obs, None

    def set_random_init(self, rand_steps=400):
        """The reference's default reset, rand_init = True (shkadov.py:51-52, 119-123), on the device: while this is on, every
        reset of this env -- reset(), reset(mask), reset_done(), step_autoreset(), capture(..., autoreset=True) -- reloads the film
        and then lets each replica it touches take its OWN n[b] uncontrolled action steps under the device's inlet noise, n[b]
        uniform on {0 .. rand_steps}, in ONE kernel launch (bcn_shkadov_reset_random: no host synchronisation, the fields stay
        in registers between the steps), after which stp is 0 again.  `n_rand` (int32 [B]) holds the counts of the last such
        reset for the replicas it touched.  set_random_init(None) turns it off (the default): reset() restarts from the film itself.
        The counts come from the env's Philox stream (set_noise_seed: seed, replica_offset, the per-replica draw counter that a
        Snapshot carries), one tick per reset: consecutive resets differ, a restored run repeats, shards agree with the single
        batch.  rand_steps is configuration like sigma and the seed -- a kernel argument, recorded in no Snapshot; a captured
        graph keeps the value it was recorded with.  With sigma = 0 the warm-up runs without noise."""
        if rand_steps is not None:
            if isinstance(rand_steps, bool) or not isinstance(rand_steps, (int, np.integer)) or not 0 <= int(rand_steps) <= 65535:
                raise ValueError("VecShkadov.set_random_init: rand_steps must be an integer in [0, 65535] or None, got %r" % (rand_steps,))
            rand_steps = int(rand_steps)
        self.rand_steps = rand_steps
        return self

    def reset_random_device(self, n_steps=None, mask=None):
        """The reset that set_random_init() switches on, called directly: reset(mask) with EXPLICIT counts n_steps (int [B]; each
        clamped to [0, rand_steps] by the kernel), or with drawn ones (None) -- one launch either way, and the draw counter ticks
        either way.  For tests, measurements and callers who want the reference's numbers of steps.  Needs set_random_init()."""
        if self.rand_steps is None:
            raise ValueError("VecShkadov.reset_random_device: set_random_init(rand_steps) first")
        if n_steps is not None:
            n_steps = torch.as_tensor(n_steps)
            if n_steps.numel() != self.batch or n_steps.is_floating_point():
                raise ValueError("VecShkadov.reset_random_device: n_steps must hold %d integers" % self.batch)
            n_steps = n_steps.to(device=self.device, dtype=torch.int32).reshape(self.batch).contiguous()
        self._masked(mask, lambda m: self._reset_random(n_steps))
        return self.obs, None

    def _reset_random(self, n_steps=None):
        self._keep_n = n_steps                     # alive behind the asynchronous launch
        self.n_rand = self._n_rand
        self._call("shkadov_reset_random", self._init_dev, n_steps, self.rand_steps, self._n_rand, self.obs)

    def _reset(self):
        if self.rand_steps is not None:
            self._reset_random(None)
        else:
            self._call("shkadov_reset", self._init_dev, self.obs)

    def _step(self, actions, noise=None):
        a = self._real(actions, (self.batch, self.n_jets))
        nz = None if noise is None else self._real(noise, (self.batch, self.ndt_act))   # None: drawn inside the kernel
        self._keep = (a, nz)
        self._call("shkadov_step", a, nz, self.obs, self.rwd, self.done, self.trunc, self.status)

    # -- the multi-agent form: every jet an agent (shkadov_separable, shkadov.py:376-481) ------------
    def set_jet_rewards(self, on=True, stats=True):
        """Per-jet rewards on the device, for trainers of the reference's multi-agent shkadov (shkadov_separable: every jet an
        agent with its own 10 observations and its own reward, shkadov.py:469-481).  While on, ONE extra launch
        (bcn_shkadov_jet_rewards, csrc/shkadov_jets.hip) directly follows the step kernel in step(), in step_autoreset() -- in
        front of the bookkeeping launch and the masked reset, which overwrites the film -- and in every step a capture()
        records; it writes
          rwd_jets [B, n_jets]   -(sum of (h - 1)^2 dx over the l_rwd cells downstream of the jet) / (n_jets l_rwd), or blowup_rwd
                                 in every jet of a replica whose step reported a blow-up (:441-445); the rows sum to `rwd` up to
                                 rounding
        and, with stats=True, keeps `jet_episodes` (JetStats: ret, last_ret, sum_ret, all [B, n_jets]) with the semantics of
        EpisodeStats, per jet.  A StepGraph captured while on also has rwd_jets_seq [n, B, n_jets] (keep_steps).  No host
        synchronisation, nothing allocated after the first call; a replica a mask skips keeps its rows; with double_buffer() the
        launch reads the outputs the step just wrote.  warmup(), reset() and the random-start resets produce no rewards and
        launch nothing extra.  `obs_jets` is the matching per-jet view of the observations.
        set_jet_rewards(False) turns it off -- the default, in which step() launches exactly what it always did -- and keeps the
        buffer.  The setting is recorded into a graph at capture(): re-capture after changing it.
        rwd_jets and jet_episodes are bookkeeping, like `episodes`: they are in no Snapshot, snapshot_signature() does not
        change, and restore() / fork() leave them where they are (JetStats.clear(mask) after a fork).  `rwd`, `done` and `trunc`
        are untouched: all jets of a replica share one episode clock.  ShardedVecEnv does not offer this."""
        if on and self._jets is None:
            self._jets = JetStats(self)
        self._jets_on, self._jets_stats = bool(on), int(bool(stats))
        return self

    def _jets_or_raise(self, what):
        if not self._jets_on or self._jets is None:
            raise AttributeError("%s.%s: per-jet rewards are off -- call set_jet_rewards() first" % (type(self).__name__, what))
        return self._jets

    @property
    def rwd_jets(self):
        """[B, n_jets] rewards of every jet after the last step() (a no-copy view; set_jet_rewards)."""
        return self._jets_or_raise("rwd_jets").rwd_jets

    @property
    def jet_episodes(self):
        """The JetStats of this env (set_jet_rewards(stats=True))."""
        jets = self._jets_or_raise("jet_episodes")
        if not self._jets_stats:
            raise ValueError("%s.jet_episodes: per-jet returns are not kept -- set_jet_rewards(True, stats=True)" % type(self).__name__)
        return jets

    @property
    def obs_jets(self):
        """`obs` regrouped per jet, [B, n_jets, n_obs], without a copy: the row is jet-major (shkadov.py:243-248), so obs_jets[b, j]
        is what shkadov_separable.get_obs(j) returns (:455-466)."""
        return self.obs.view(self.batch, self.n_jets, self.n_obs)

    def _after_step(self):
        if self._jets_on:
            self._call("shkadov_jet_rewards", self.out_buf, self._jets.buf, self._jets_stats)


class VecSloshing(VecEnv):
    """sloshing/sloshing.py:16-320.  `init_fields`: [2, nx+2] (h_init, q_init incl. ghosts)."""

    PARAMS = ("amp", "alpha", "g")
    _panel = "line"

    def _render_range(self):
        return 0.25, 1.75, 1.0                                   # sloshing.py:266-270

    def __init__(self, batch, device="cuda:0", dtype="f32", init_fields=None, L=2.5, amp=5.0,
                 alpha=0.0005, g=9.81):
        self._derive(L, amp, alpha, g)
        self._ctor = dict(L=L, amp=amp, alpha=alpha, g=g)
        self._init_np = None if init_fields is None else np.asarray(init_fields, dtype=np.float64)
        super().__init__(batch, device, dtype)
        self._make_spaces()
        self._init_dev = None
        if self._init_np is not None:
            self._init_dev = self._real(self._init_np, (2, self.nx + 2))

    def _make_spaces(self):
        self.action_space = spaces.box(-1.0, 1.0, (1,))                         # sloshing.py:73-76
        self.observation_space = spaces.sym_box(1.0, self.n_obs)                # :81-86
        return self

    def _derive(self, L=2.5, amp=5.0, alpha=0.0005, g=9.81):
        self.L, self.amp, self.alpha, self.g = L, amp, alpha, g
        self.nx = int(80 * L)                                            # :24
        self.dt, self.dt_act, self.t_warmup, self.t_act = 0.001, 0.05, 2.0, 10.0
        self.dx = float(L / self.nx)
        self.ndt_act = int(self.dt_act / self.dt)
        self.n_act = int(self.t_act / self.dt_act)
        self.n_warmup = int(self.t_warmup / self.dt_act)
        self.n_interp = int(0.01 / self.dt)                              # :48
        self.n_obs = self.nx // 2 + (1 if self.nx % 2 else 0)            # :39
        return self

    def _create(self):
        c = _lib.SloshingCfg(nx=self.nx, ndt_act=self.ndt_act, n_act=self.n_act, n_interp=self.n_interp,
                             dx=self.dx, dt=self.dt, g=self.g, amp=self.amp, alpha=self.alpha)
        self.cfg = c
        _lib.check(self.lib.bcn_sloshing_create(C.byref(c), self.batch, self.cdtype, self.dev_index,
                                                C.byref(self.h)))

    def state_shape(self):
        return (4, self.nx + 2)

    @staticmethod
    def signal(t, dt):
        """Excitation used by the reference's warm-up generator (sloshing.py:134-138)."""
        return 0.5 * (np.cos(np.pi * t) + 3.0 * np.cos(4.0 * np.pi * t))

    def _reset(self):
        self._call("sloshing_reset", self._init_dev, self.obs)

    def _step(self, actions, noise=None):
        a = self._real(actions, (self.batch,))
        self._keep = a
        self._call("sloshing_step", a, self.obs, self.rwd, self.done, self.trunc, self.status)


class VecLorenz(VecEnv):
    """lorenz/lorenz.py:18-264 (the host port: beacon_amd/lorenz.py).  One lane per replica (csrc/ode_env.h); Discrete(3)
    actions as int32 [B] (force -1, 0, 1), obs = (x, f(x) of the last RK stage), reward 1 while x0 < 0.
    State rows (get_state / set_state): [B, 8] = x0, x1, x2, fx0, fx1, fx2, t, u."""

    PARAMS = ("sigma", "rho", "beta")

    action_is_int = True

    def __init__(self, batch, device="cuda:0", dtype="f32", sigma=10.0, rho=28.0, beta=8.0 / 3.0):
        self._derive(sigma, rho, beta)
        self._ctor = dict(sigma=sigma, rho=rho, beta=beta)
        super().__init__(batch, device, dtype)
        self._make_spaces()

    def _derive(self, sigma=10.0, rho=28.0, beta=8.0 / 3.0):
        self.sigma, self.rho, self.beta = sigma, rho, beta
        self.dt, self.dt_act, self.t_max = 0.05, 0.05, 25.0               # lorenz.py:26-36
        self.n_obs = 6
        self.ndt_act = int(self.dt_act / self.dt)
        self.n_act = int(self.t_max / self.dt_act)
        return self

    def _make_spaces(self):
        self.action_space = spaces.discrete(3)                                  # lorenz.py:49
        self.observation_space = spaces.sym_box(1.0, self.n_obs)               # :51-55
        return self

    def _create(self):
        c = _lib.LorenzCfg(ndt_act=self.ndt_act, n_act=self.n_act, dt=self.dt, sigma=self.sigma, rho=self.rho, beta=self.beta)
        self.cfg = c
        _lib.check(self.lib.bcn_lorenz_create(C.byref(c), self.batch, self.cdtype, self.dev_index, C.byref(self.h)))

    def state_shape(self):
        return (8,)

    def _reset(self):
        self._call("lorenz_reset", self.obs)

    def _step(self, actions, noise=None):
        a = self._int_actions(actions)
        self._keep = a
        self._call("lorenz_step", a, self.obs, self.rwd, self.done, self.trunc, self.status)


class VecVortex(VecEnv):
    """vortex/vortex.py:17-283 (the host port: beacon_amd/vortex.py).  One lane per replica (csrc/ode_env.h); Box(-1, 1, (2,))
    actions [B, 2] = (modulus, phase) of the feedback.  State rows (get_state / set_state): [B, 14] = ar, ai, yr, yi,
    fx0..fx3, t, y, kmod, kphase, u0, u1."""

    PARAMS = ("re", "weight")

    def __init__(self, batch, device="cuda:0", dtype="f32", re=50.0, weight=50.0):
        self._derive(re, weight)
        self._ctor = dict(re=re, weight=weight)
        super().__init__(batch, device, dtype)
        self._make_spaces()

    def _derive(self, re=50.0, weight=50.0):
        self.lmbda_re, self.lmbda_cx = 9.153, 3.239                       # vortex.py:26-48
        self.mu_re, self.mu_cx = 308.9, -1025.0
        self.alpha_re, self.alpha_cx = 0.03492, 0.01472
        self.beta, self.re, self.re_crit = 1.0, re, 46.6
        self.omega_s, self.omega_f = 1.1, 0.74
        self.gamma, self.mass, self.weight = 0.023, 10.0, weight
        self.dt, self.dt_act, self.t_max = 0.1, 0.5, 400.0
        self.n_obs = 8
        self.ndt_act = int(self.dt_act / self.dt)
        self.n_act = int(self.t_max / self.dt_act)
        self.mod_min, self.mod_max = 0.0, 0.3
        self.phase_min, self.phase_max = -math.pi, math.pi
        return self

    def _make_spaces(self):
        self.action_space = spaces.box(-1.0, 1.0, (2,))                         # vortex.py:69-72
        self.observation_space = spaces.sym_box(1.0e-4, self.n_obs)             # :74-79
        return self

    def _create(self):
        c = _lib.VortexCfg(ndt_act=self.ndt_act, n_act=self.n_act, dt=self.dt, lmbda_re=self.lmbda_re, lmbda_cx=self.lmbda_cx,
                           mu_re=self.mu_re, mu_cx=self.mu_cx, alpha_re=self.alpha_re, alpha_cx=self.alpha_cx, beta=self.beta,
                           re=self.re, re_crit=self.re_crit, omega_s=self.omega_s, omega_f=self.omega_f, gamma=self.gamma,
                           mass=self.mass, weight=self.weight, mod_min=self.mod_min, mod_max=self.mod_max,
                           phase_min=self.phase_min, phase_max=self.phase_max)
        self.cfg = c
        _lib.check(self.lib.bcn_vortex_create(C.byref(c), self.batch, self.cdtype, self.dev_index, C.byref(self.h)))

    def state_shape(self):
        return (14,)

    def _reset(self):
        self._call("vortex_reset", self.obs)

    def _step(self, actions, noise=None):
        a = self._real(actions, (self.batch, 2))
        self._keep = a
        self._call("vortex_step", a, self.obs, self.rwd, self.done, self.trunc, self.status)
