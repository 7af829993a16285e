"""CPU-side checks of the on-device rollout storage and GAE (VecEnv.rollout, Rollout, bcn_rollout_*): the five C entry points in
the header, the binding and the built library, the op tables, the torch ops' schemas, the Python surface, the launch sequence of a
step with a rollout attached, the kernels' build for gfx950, and -- because the GPU tests lean on it -- the float64 NumPy
restatement of the GAE recurrence against an independent extended-precision formulation."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from rollout_ref import gae_bound, gae_explicit, gae_inputs, gae_ref

NEW = ("bcn_rollout_bytes", "bcn_rollout_layout", "bcn_rollout_begin", "bcn_rollout_record", "bcn_rollout_gae")


def test_entry_points_are_declared_bound_and_exported_and_refuse_null_handles():
    import ctypes as C
    from beacon_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "beacon_hip.h")).read()
    assert re.search(r"BCN_API size_t bcn_rollout_bytes\(bcn_env_t h, int T, int flags\);", hdr)
    assert re.search(r"BCN_API int bcn_rollout_layout\(bcn_env_t h, int T, int flags, bcn_snapshot_seg\* segs, int max_segs\);", hdr)
    assert re.search(r"BCN_API int bcn_rollout_begin\(bcn_env_t h, void\* ro_buf_dev, const void\* out_buf_dev, const void\* norm_buf_dev, "
                     r"void\* stream\);", hdr)
    assert re.search(r"BCN_API int bcn_rollout_record\(bcn_env_t h, const void\* out_buf_dev, void\* ro_buf_dev, const void\* act_dev, "
                     r"const void\* ep_buf_dev,\s+const void\* norm_buf_dev, const void\* jets_buf_dev, const uint8_t\* mask_dev, int T, "
                     r"int flags, void\* stream\);", hdr)
    assert re.search(r"BCN_API int bcn_rollout_gae\(bcn_env_t h, void\* ro_buf_dev, const void\* values_dev, const void\* last_value_dev, "
                     r"const void\* final_values_dev,\s+int T, int flags, int cols, double gamma, double lam, void\* stream\);", hdr)
    assert re.search(r"enum \{ BCN_RO_FINAL_OBS = 1, BCN_RO_JETS = 2 \};", hdr) and (_lib.RO_FINAL_OBS, _lib.RO_JETS) == (1, 2)
    assert int(re.search(r"#define BCN_API_VERSION (\d+)", hdr).group(1)) == 4 and _lib.API_VERSION == 4     # no buffer changed size
    vp, ci, dbl = C.c_void_p, C.c_int, C.c_double
    assert _lib.SIGNATURES["bcn_rollout_bytes"] == (C.c_size_t, [vp, ci, ci])
    assert _lib.SIGNATURES["bcn_rollout_layout"] == (ci, [vp, ci, ci, C.POINTER(_lib.SnapshotSeg), ci])
    assert _lib.SIGNATURES["bcn_rollout_begin"] == (ci, [vp, vp, vp, vp, vp])
    assert _lib.SIGNATURES["bcn_rollout_record"] == (ci, [vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp])
    assert _lib.SIGNATURES["bcn_rollout_gae"] == (ci, [vp, vp, vp, vp, vp, ci, ci, ci, dbl, dbl, vp])
    if build.hipcc() is None and not os.path.exists(build.LIB):
        pytest.skip("no hipcc and no prebuilt library")
    L = _lib.load()
    for name in NEW:
        assert hasattr(L, name)
    assert L.bcn_api_version() == 4
    segs = (_lib.SnapshotSeg * 16)()
    assert L.bcn_rollout_bytes(None, 5, 0) == 0 and b"bcn_rollout_bytes: null handle" in L.bcn_last_error()
    assert L.bcn_rollout_layout(None, 5, 0, segs, 16) == 0 and b"bcn_rollout_layout: null handle" in L.bcn_last_error()
    assert L.bcn_rollout_begin(None, None, None, None, None) == 1 and b"bcn_rollout_begin: null handle" in L.bcn_last_error()
    assert L.bcn_rollout_record(None, None, None, None, None, None, None, None, 5, 0, None) == 1
    assert b"bcn_rollout_record: null handle" in L.bcn_last_error()
    assert L.bcn_rollout_gae(None, None, None, None, None, 5, 0, 1, 0.99, 0.95, None) == 1
    assert b"bcn_rollout_gae: null handle" in L.bcn_last_error()


def test_op_tables():
    from beacon_amd import vec
    assert vec._ROLLOUT_OPS == ("rollout_begin", "rollout_record", "rollout_gae")
    # what tests/test_normalize_host.py pins: the new names are in none of these
    assert vec._NORM_OPS == ("normalize",)
    assert vec._ALL_OPS == vec._OPS + vec._ODE_OPS + vec._STATE_OPS + vec._EPISODE_OPS + vec._WARM_OPS + vec._JET_OPS
    assert not set(vec._ROLLOUT_OPS) & (set(vec._ALL_OPS) | set(vec._NORM_OPS))

    class FakeLib(object):
        def __getattr__(self, name):
            return name
    assert set(vec._c_table(FakeLib())) == set(vec._ALL_OPS) | set(vec._NORM_OPS)
    ops, cfn = vec._rollout_tables(FakeLib(), False)                          # resolved separately, merged at the first attach
    assert ops is None and cfn == {n: "bcn_" + n for n in vec._ROLLOUT_OPS}


def test_torch_extension_defines_and_registers_the_rollout_ops():
    from beacon_amd import build, torch_ext, vec
    src = open(os.path.join(ROOT, "beacon_amd", "csrc", "torch", "beacon_torch.cpp")).read()
    for name in vec._ROLLOUT_OPS:
        assert src.count('m.def("%s(' % name) == 1 and src.count('m.impl("%s"' % name) == 2, name          # CUDA and Meta
    if (shutil.which("g++") is None and torch_ext.stale()) or (build.hipcc() is None and not os.path.exists(build.LIB)):
        pytest.skip("no compiler and no prebuilt extension")
    path = torch_ext.build_ext()
    assert path and os.path.exists(path) and not torch_ext.stale()
    ops = torch_ext.load()
    table, _ = vec._rollout_tables(FakeLibrary(), True)
    assert ops is not None and set(table) == set(vec._ROLLOUT_OPS)
    assert str(ops.rollout_begin.default._schema) == "beacon::rollout_begin(int handle, Tensor(a!) ro_buf, Tensor out_buf, Tensor? norm_buf) -> ()"
    assert str(ops.rollout_record.default._schema) == (
        "beacon::rollout_record(int handle, Tensor out_buf, Tensor(a!) ro_buf, Tensor? act, Tensor? ep_buf, Tensor? norm_buf, "
        "Tensor? jets_buf, Tensor? mask, int T, int flags) -> ()")
    assert str(ops.rollout_gae.default._schema) == (
        "beacon::rollout_gae(int handle, Tensor(a!) ro_buf, Tensor values, Tensor last_value, Tensor? final_values, int T, int flags, "
        "int cols, float gamma, float lam) -> ()")
    meta = lambda dt=torch.uint8: torch.zeros(16, dtype=dt, device="meta")
    ops.rollout_begin(0, meta(), meta(), None)
    ops.rollout_begin(0, meta(), meta(), meta())
    ops.rollout_record(0, meta(), meta(), None, None, None, None, None, 5, 0)
    ops.rollout_record(0, meta(), meta(), meta(torch.float32), meta(), meta(), meta(), meta(), 5, 3)
    ops.rollout_gae(0, meta(), meta(torch.float32), meta(torch.float32), None, 5, 0, 1, 0.99, 0.95)
    ops.rollout_gae(0, meta(), meta(torch.float32), meta(torch.float32), meta(torch.float32), 5, 2, 5, 0.99, 0.95)
    cpu = lambda dt=torch.uint8: torch.zeros(16, dtype=dt)
    with pytest.raises((NotImplementedError, RuntimeError)):                # CUDA key only: CPU tensors find no kernel
        ops.rollout_begin(0, cpu(), cpu(), None)
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.rollout_record(0, cpu(), cpu(), None, None, None, None, None, 5, 0)
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.rollout_gae(0, cpu(), cpu(torch.float32), cpu(torch.float32), None, 5, 0, 1, 0.99, 0.95)


class FakeLibrary(object):
    def __getattr__(self, name):
        return name


def test_python_surface_exists_and_is_off_by_default():
    import inspect
    import beacon_amd
    from beacon_amd import vec
    assert beacon_amd.Rollout is vec.Rollout and issubclass(vec.Rollout, vec._SegBuffer)
    assert issubclass(beacon_amd.RolloutOverflow, RuntimeError)
    sig = inspect.signature(vec.VecEnv.rollout).parameters
    assert list(sig) == ["self", "T", "final_obs"] and sig["final_obs"].default is True
    sig = inspect.signature(vec.Rollout.compute_gae).parameters
    assert list(sig) == ["self", "values", "last_value", "final_values", "gamma", "lam", "per_jet"]
    assert [sig[k].default for k in list(sig)[3:]] == [None, 0.99, 0.95, False]
    for m in ("begin", "check", "compute_gae", "clear", "state_dict", "load_state_dict", "view"):
        assert callable(getattr(vec.Rollout, m))
    assert vec.Rollout.NAMES == ("cursor", "obs", "act", "rwd", "status", "done", "trunc", "valid", "final_obs", "rwd_jets", "adv", "ret")
    assert vec.Rollout.state_dict is vec._SegBuffer.state_dict and vec.Rollout.load_state_dict is vec._SegBuffer.load_state_dict
    assert vec.VecEnv.__dict__["_rollout"] is None                           # a class-level default: envs built with __new__ have it
    for cls in (vec.VecEnv, vec.VecRayleigh, vec.VecMixing, vec.VecBurgers, vec.VecShkadov, vec.VecSloshing, vec.VecLorenz, vec.VecVortex):
        env = cls.__new__(cls)
        assert env._rollout is None and env.rollout(None) is None
    doc = vec.VecEnv.rollout.__doc__ + vec.Rollout.__doc__
    assert "Snapshot" in doc and "snapshot_signature" in doc and "restore()" in doc and "ShardedVecEnv" in doc and "mirrors" in doc
    # the base class takes the extra layout arguments of the pair, and the three older subclasses call it as before
    sig = inspect.signature(vec._SegBuffer.__init__).parameters
    assert list(sig) == ["self", "env", "layout_args"] and sig["layout_args"].default == ()


# ---- the launch sequence of a step with a rollout attached (the technique of tests/test_pipeline_host.py) --------------------
S, J, T, R, N, REC = "shkadov_step", "shkadov_jet_rewards", "episode_track", "shkadov_reset", "normalize", "rollout_record"


class _Lib(object):
    @staticmethod
    def bcn_set_mask(h, ptr):
        return 0


def _env(jets, norm, attach=True, ro_jets=None):
    """A VecShkadov without a handle and without a device whose _call records (entry point, mask) -- and, for rollout_record, its
    pointer arguments spelled by the buffer they belong to."""
    from beacon_amd import _lib, vec
    env = vec.VecShkadov.__new__(vec.VecShkadov)
    env.h, env.lib, env._mask, env._rotate = None, _Lib(), None, 0
    env.batch, env.n_jets, env.ndt_act, env._init_dev = 4, 2, 5, None
    env._n_rand = env.n_rand = torch.zeros(4, dtype=torch.int32)
    env.out_buf = torch.zeros(16, dtype=torch.uint8)
    env.obs, env.rwd, env.done, env.trunc, env.status = (torch.zeros(4) for _ in range(5))
    ep = vec.EpisodeStats.__new__(vec.EpisodeStats)
    ep.buf, ep.finished = torch.zeros(16, dtype=torch.uint8), torch.zeros(4, dtype=torch.uint8)
    env._episodes = ep
    env._jets = vec.JetStats.__new__(vec.JetStats)
    env._jets.buf = torch.zeros(16, dtype=torch.uint8)
    env._jets_on, env._jets_stats = jets, 1
    nz = env._norm = vec.Normalizer.__new__(vec.Normalizer)
    nz.buf, nz.norm_obs, nz.norm_rwd = torch.zeros(16, dtype=torch.uint8), torch.zeros(4), torch.zeros(4)
    nz.training, nz.gamma, nz.eps, nz.clip_obs, nz.clip_rwd = True, 0.99, 1e-8, 10.0, 10.0
    env._norm_on = norm
    ro = vec.Rollout.__new__(vec.Rollout)
    ro.buf, ro.T = torch.zeros(16, dtype=torch.uint8), 7
    ro.flags = _lib.RO_FINAL_OBS | (_lib.RO_JETS if (jets if ro_jets is None else ro_jets) else 0)
    if attach:
        env._rollout = ro
    env.ro = ro
    env.user_mask = torch.ones(4, dtype=torch.uint8)
    env.actions = torch.zeros(4, 2)
    env._real = lambda x, shape: x                                       # no device here: the action tensor goes through as it is
    env.log = []

    def label(m):
        return None if m is None else "mask" if m is env.user_mask else "finished" if m is ep.finished else "unknown"

    def call(name, *args):
        if name == T:
            env.log.append((name, label(args[2])))
        elif name == N:
            env.log.append((name, label(args[3]), args[4], args[2] is not None))
        elif name == REC:
            out_buf, ro_buf, act, ep_buf, norm_buf, jets_buf, mask, steps, flags = args
            assert out_buf is env.out_buf and ro_buf is ro.buf and (steps, flags) == (ro.T, ro.flags)
            assert act is None or act is env.actions
            assert ep_buf is None or ep_buf is ep.buf
            assert norm_buf is None or norm_buf is nz.buf
            assert jets_buf is None or jets_buf is env._jets.buf
            env.log.append((name, label(mask), act is not None, ep_buf is not None, norm_buf is not None, jets_buf is not None))
        else:
            env.log.append((name, label(env._mask)))

    def apply_mask(mask):
        env._mask = mask

    env._call, env._apply_mask = call, apply_mask
    return env


# today's sequences (tests/test_pipeline_host.py: STEP, STEP_AUTORESET); "M": the mask the call was given
STEP = {
    (False, False): [(S, "M")],
    (True, False): [(S, "M"), (J, "M")],
    (False, True): [(S, "M"), (N, "M", 0, False)],
    (True, True): [(S, "M"), (J, "M"), (N, "M", 0, False)],
}
STEP_AUTORESET = {
    (False, False): [(S, "M"), (T, "M"), (R, "finished")],
    (True, False): [(S, "M"), (J, "M"), (T, "M"), (R, "finished")],
    (False, True): [(S, "M"), (T, "M"), (R, "finished"), (N, "M", 0, True)],
    (True, True): [(S, "M"), (J, "M"), (T, "M"), (R, "finished"), (N, "M", 0, True)],
}


def _given(seq, m):
    return [tuple(m if x == "M" else x for x in rec) for rec in seq]


@pytest.mark.parametrize("autoreset", [False, True])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("with_actions", [False, True])
@pytest.mark.parametrize("jets,norm", sorted(STEP))
def test_a_step_with_a_rollout_enqueues_todays_sequence_and_one_record_last(jets, norm, with_actions, masked, autoreset):
    env = _env(jets, norm)
    fn = env.step_autoreset if autoreset else env.step
    out = fn(env.actions if with_actions else None, None, env.user_mask if masked else None)
    m = "mask" if masked else None
    today = _given((STEP_AUTORESET if autoreset else STEP)[jets, norm], m)
    # the pointer arguments are the normaliser's, the episode buffer's and the per-jet buffer's exactly when those are in play
    assert env.log == today + [(REC, m, with_actions, autoreset, norm, jets)]
    assert env._mask is None
    assert out[0] is (env._norm.norm_obs if norm else env.obs) and out[1] is (env._norm.norm_rwd if norm else env.rwd)
    assert out[2] is env.done and out[3] is env.trunc and out[4] is (env.episodes if autoreset else None)


@pytest.mark.parametrize("autoreset", [False, True])
@pytest.mark.parametrize("jets,norm", sorted(STEP))
def test_without_a_rollout_and_after_detaching_nothing_extra_is_enqueued(jets, norm, autoreset):
    env = _env(jets, norm, attach=False)
    fn = env.step_autoreset if autoreset else env.step
    fn(None, None, None)
    assert env.log == _given((STEP_AUTORESET if autoreset else STEP)[jets, norm], None)
    env.log, env._rollout = [], env.ro
    env._rollout_kept = env.ro
    assert env.rollout(None) is env.ro and env._rollout is None            # detaches, keeps the buffer
    fn(None, None, None)
    assert env.log == _given((STEP_AUTORESET if autoreset else STEP)[jets, norm], None)


def test_reset_records_nothing_and_a_rollout_without_the_jets_segment_gets_no_jets_pointer():
    env = _env(True, True)
    env.reset()
    assert env.log == [(R, None), (N, None, 1, False)]
    env = _env(True, False, ro_jets=False)                                 # jet rewards switched on after the attach
    env.step(None, None, None)
    assert env.log[-1] == (REC, None, False, False, False, False)
    env = _env(False, False, ro_jets=True)                                 # ... and switched off after it
    env.step(None, None, None)
    assert env.log[-1] == (REC, None, False, False, False, False)


def test_views_put_the_step_axis_in_front():
    from beacon_amd import _lib, vec
    RL, I32, U8 = _lib.SNAP_REAL, _lib.SNAP_I32, _lib.SNAP_U8
    steps, B, n, nj = 3, 5, 6, 2

    def build(act, final, jets, tdtype):
        rows = [("cursor", I32, 0, 4), ("obs", RL, steps + 1, n), act, ("rwd", RL, steps, 1), ("status", I32, steps, 1),
                ("done", U8, steps, 1), ("trunc", U8, steps, 1), ("valid", U8, steps, 1), ("final_obs", RL, steps, n if final else 0),
                ("rwd_jets", RL, steps, nj if jets else 0), ("adv", RL, steps, nj if jets else 1), ("ret", RL, steps, nj if jets else 1)]
        el = {RL: torch.empty((), dtype=tdtype).element_size(), U8: 1, I32: 4}
        off, lay = 0, []
        for name, elem, planes, row in rows:
            lay.append(dict(name=name, offset=off, elem=elem, planes=planes, row_elems=row))
            off = (off + (planes * B if planes else 1) * row * el[elem] + 15) // 16 * 16
        ro = vec.Rollout.__new__(vec.Rollout)
        ro.batch, ro.tdtype, ro.T, ro.n_jets, ro.buf = B, tdtype, steps, nj if jets else 0, torch.zeros(off, dtype=torch.uint8)
        ro._bind(lay)
        return ro

    for tdtype in (torch.float32, torch.float64):
        ro = build(("act", RL, steps, 1), True, False, tdtype)
        assert tuple(ro.cursor.shape) == (4,) and ro.cursor.dtype == torch.int32
        assert tuple(ro.obs.shape) == (steps + 1, B, n) and tuple(ro.final_obs.shape) == (steps, B, n) and ro.obs.dtype == tdtype
        assert tuple(ro.act.shape) == (steps, B, 1) and ro.act.dtype == tdtype                    # real actions: [T, B, act_dim]
        for name in ("rwd", "status", "done", "trunc", "valid", "adv", "ret"):
            assert tuple(getattr(ro, name).shape) == (steps, B), name
        assert tuple(ro.rwd_jets.shape) == (steps, B, 0)
        assert (ro.status.dtype, ro.done.dtype, ro.valid.dtype) == (torch.int32, torch.uint8, torch.uint8)
        ro = build(("act", I32, steps, 1), False, True, tdtype)
        assert tuple(ro.act.shape) == (steps, B) and ro.act.dtype == torch.int32                  # discrete actions: int32 [T, B]
        assert tuple(ro.final_obs.shape) == (steps, B, 0) and tuple(ro.rwd_jets.shape) == (steps, B, nj)
        assert tuple(ro.adv.shape) == (steps, B)                                                  # [T, B] before the first compute_gae
        adv, ret = ro.gae_views(nj)
        assert tuple(adv.shape) == tuple(ret.shape) == (steps, B * nj)
        assert adv.data_ptr() == ro.adv.data_ptr() and ret.data_ptr() == ro.ret.data_ptr()
        for k, name in enumerate(ro.NAMES):                                                       # no copies, no overlap
            ro.view(name).fill_(k + 1) if name not in ("adv", "ret") else ro.gae_views(nj)[name == "ret"].fill_(k + 1)
        for k, name in enumerate(ro.NAMES):
            v = ro.view(name) if name not in ("adv", "ret") else ro.gae_views(nj)[name == "ret"]
            assert bool((v == k + 1).all()), name
        with pytest.raises(KeyError):
            ro.view("nope")
        assert ro.clear() is ro and not ro.buf.any()


def test_compute_gae_refuses_wrong_inputs_before_any_launch():
    from beacon_amd import vec
    ro = vec.Rollout.__new__(vec.Rollout)
    ro.batch, ro.tdtype, ro.T, ro.n_jets, ro.flags, ro.buf = 4, torch.float32, 3, 0, 1, torch.zeros(16, dtype=torch.uint8)

    class Env(object):
        def _call(self, *a):
            raise AssertionError("launched")
    env = Env()
    ro._env = lambda: env
    v, lv = torch.zeros(3, 4), torch.zeros(4)
    for bad in ((torch.zeros(3, 5), lv, None), (v, torch.zeros(5), None), (v, lv, torch.zeros(2, 4)), (v.double(), lv, None),
                (v, lv.double(), None), (v.numpy(), lv, None), (torch.zeros(4, 3).t(), lv, None)):
        with pytest.raises(ValueError, match="Rollout.compute_gae"):
            ro.compute_gae(*bad)
    with pytest.raises(ValueError, match="per_jet"):
        ro.compute_gae(v, lv, per_jet=True)
    with pytest.raises(ValueError, match="gamma"):
        ro.compute_gae(v, lv, gamma=1.5)
    with pytest.raises(ValueError, match="T must be"):
        vec.Rollout(None, 0)


def test_rollout_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """csrc/rollout.hip with the library's own flags: the record, the cursor's own launch, the begin and the GAE kernel (two dtypes,
    with and without final values), each without a private segment."""
    from beacon_amd import build
    cc = build.hipcc()
    if cc is None:
        pytest.skip("no hipcc")
    src = os.path.join(build.CSRC, "rollout.hip")
    assert src in build.sources()
    asm = str(tmp_path / "rollout.s")
    subprocess.check_call(build.compile_cmd(src, asm, mode=("--cuda-device-only", "-S")))
    text = open(asm).read()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    names = sorted(re.search(r"rollout_(\w+?)_k", k).group(1) for k in kernels)
    assert names == ["advance", "begin", "gae", "gae", "gae", "gae", "record"], kernels
    assert re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text) == ["0"] * 7
    assert "ds_" not in re.sub(r";.*", "", text) and "atomic" not in text                        # no LDS, no atomics


# ---- the yardstick itself ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_final", [True, False])
def test_the_float64_restatement_agrees_with_the_explicit_discounted_sums(with_final):
    """The GPU tests compare the kernel with gae_ref.  Here gae_ref itself is held against an independent formulation -- every
    column cut into episodes at done | trunc, skipped steps dropped, every advantage the explicit discounted sum of the deltas of
    the rest of its episode, in numpy.longdouble -- to 8 T 2^-53 A per column (rollout_ref.gae_bound)."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("numpy.longdouble is no wider than float64 here")
    T, ncols = 64, 50
    rng = np.random.default_rng(5)
    x = gae_inputs(rng, T, ncols)
    fin = (x["done"] | x["trunc"]) != 0
    assert 0.1 < fin.mean() < 0.3 and 0.03 < 1.0 - x["valid"].mean() < 0.2
    assert (x["trunc"] != 0).any() and ((x["done"] != 0) & (x["trunc"] == 0)).any()          # both flag combinations
    fv = x["final_values"] if with_final else None
    args = (x["rwd"], x["values"], x["last_value"], x["done"], x["trunc"], x["valid"], fv)
    adv, ret = gae_ref(*args)
    ladv, lret = gae_explicit(*args)
    bound = gae_bound(T, adv, x["values"], x["rwd"])
    err_adv = np.abs((adv.astype(np.longdouble) - ladv).astype(np.float64)).max(axis=0)
    err_ret = np.abs((ret.astype(np.longdouble) - lret).astype(np.float64)).max(axis=0)
    print("restatement against explicit sums: adv %.3g, ret %.3g of the bound" % ((err_adv / bound).max(), (err_ret / bound).max()))
    assert (err_adv <= bound).all() and (err_ret <= bound).all()
    skipped = x["valid"] == 0
    assert (adv[skipped] == 0).all() and (ret[skipped] == x["values"][skipped]).all()
    if with_final:                                                           # the bootstrap matters: without it the answer differs
        assert np.abs(adv - gae_ref(*args[:-1])[0]).max() > 0.1
    # n < T: the rows behind the cursor are left alone, the others are those of a rollout of n steps
    a3, r3 = gae_ref(*args, n=3)
    s3 = tuple(v[:3] if v is not None and v.ndim == 2 else v for v in args)
    assert np.isnan(a3[3:]).all() and np.isnan(r3[3:]).all() and np.array_equal(a3[:3], gae_ref(*s3)[0])
