"""ctypes binding of libbeacon_hip.so (include/beacon_hip.h).

The product path has NO CPU fallback: if the HIP library cannot be built/loaded, or no
GPU is visible, every env constructor raises."""
import ctypes as C

from . import build as _build

c_i32p = C.POINTER(C.c_int32)
c_u8p = C.POINTER(C.c_uint8)
vp = C.c_void_p

F32, F64 = 0, 1
ST_OK, ST_ITMAX, ST_BLOWUP, ST_PLAN = 0, 1, 2, 4
API_VERSION, COUNTER_WORDS = 4, 4          # include/beacon_hip.h: BCN_API_VERSION, BCN_COUNTER_WORDS


class RayleighCfg(C.Structure):
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("ndt_act", C.c_int32), ("n_act", C.c_int32),
                ("n_sgts", C.c_int32), ("nx_sgts", C.c_int32), ("nx_obs_pts", C.c_int32),
                ("ny_obs_pts", C.c_int32), ("nx_obs", C.c_int32), ("ny_obs", C.c_int32),
                ("n_obs_steps", C.c_int32), ("itmax", C.c_int32),
                ("dx", C.c_double), ("dy", C.c_double), ("dt", C.c_double),
                ("pr", C.c_double), ("ra", C.c_double), ("Tc", C.c_double), ("Th", C.c_double),
                ("C", C.c_double), ("tol", C.c_double)]


class MixingCfg(C.Structure):
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("ndt_act", C.c_int32), ("n_act", C.c_int32),
                ("nx_obs_pts", C.c_int32), ("ny_obs_pts", C.c_int32), ("nx_obs", C.c_int32),
                ("ny_obs", C.c_int32), ("n_obs_steps", C.c_int32), ("itmax", C.c_int32),
                ("i_min", C.c_int32), ("i_max", C.c_int32), ("j_min", C.c_int32), ("j_max", C.c_int32),
                ("dx", C.c_double), ("dy", C.c_double), ("dt", C.c_double),
                ("re", C.c_double), ("pe", C.c_double), ("u_max", C.c_double), ("C0", C.c_double),
                ("ref_c", C.c_double), ("tol", C.c_double)]


class BurgersCfg(C.Structure):
    _fields_ = [("nx", C.c_int32), ("ndt_act", C.c_int32), ("n_act", C.c_int32), ("ctrl_pos", C.c_int32),
                ("n_obs_pts", C.c_int32),
                ("dx", C.c_double), ("dt", C.c_double), ("amp", C.c_double), ("u_target", C.c_double)]


class ShkadovCfg(C.Structure):
    _fields_ = [("nx", C.c_int32), ("ndt_act", C.c_int32), ("n_act", C.c_int32), ("n_jets", C.c_int32),
                ("jet_pos", C.c_int32), ("jet_hw", C.c_int32), ("jet_space", C.c_int32),
                ("l_obs", C.c_int32), ("l_rwd", C.c_int32), ("n_obs", C.c_int32), ("obs_stride", C.c_int32),
                ("n_interp", C.c_int32),
                ("dx", C.c_double), ("dt", C.c_double), ("delta", C.c_double), ("jet_amp", C.c_double),
                ("eps", C.c_double), ("h_blow", C.c_double), ("blowup_rwd", C.c_double)]


class SloshingCfg(C.Structure):
    _fields_ = [("nx", C.c_int32), ("ndt_act", C.c_int32), ("n_act", C.c_int32), ("n_interp", C.c_int32),
                ("dx", C.c_double), ("dt", C.c_double), ("g", C.c_double), ("amp", C.c_double),
                ("alpha", C.c_double)]


class LorenzCfg(C.Structure):
    _fields_ = [("ndt_act", C.c_int32), ("n_act", C.c_int32),
                ("dt", C.c_double), ("sigma", C.c_double), ("rho", C.c_double), ("beta", C.c_double)]


class VortexCfg(C.Structure):
    _fields_ = [("ndt_act", C.c_int32), ("n_act", C.c_int32), ("dt", C.c_double),
                ("lmbda_re", C.c_double), ("lmbda_cx", C.c_double), ("mu_re", C.c_double), ("mu_cx", C.c_double),
                ("alpha_re", C.c_double), ("alpha_cx", C.c_double), ("beta", C.c_double), ("re", C.c_double),
                ("re_crit", C.c_double), ("omega_s", C.c_double), ("omega_f", C.c_double), ("gamma", C.c_double),
                ("mass", C.c_double), ("weight", C.c_double), ("mod_min", C.c_double), ("mod_max", C.c_double),
                ("phase_min", C.c_double), ("phase_max", C.c_double)]


class SnapshotSeg(C.Structure):
    """bcn_snapshot_seg: one named segment of a snapshot, [planes][n][row_elems] elements at `offset` bytes."""
    _fields_ = [("name", C.c_char * 16), ("offset", C.c_uint64), ("elem", C.c_int32), ("planes", C.c_int32),
                ("row_elems", C.c_int64)]


class RenderCfg(C.Structure):
    """bcn_render_cfg: what a frame shows (plane, scale or width / height, strip, ranges)."""
    _fields_ = [("plane", C.c_int32), ("scale", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("strip", C.c_int32),
                ("has_range", C.c_int32), ("lo", C.c_double), ("hi", C.c_double), ("ref", C.c_double)]


PLANES = {"scalar": 0, "u": 1, "v": 2, "p": 3}           # include/beacon_hip.h: BCN_PLANE_*
SNAP_REAL, SNAP_I32, SNAP_U32, SNAP_U8 = 0, 1, 2, 3      # include/beacon_hip.h: BCN_SNAP_*
SNAP_F64, SNAP_I64 = 4, 5                                # (bcn_episode_layout only)
RO_FINAL_OBS, RO_JETS = 1, 2                             # include/beacon_hip.h: BCN_RO_*

# every symbol include/beacon_hip.h declares: (restype, argtypes)
SIGNATURES = {
    "bcn_rayleigh_create": (C.c_int, [C.POINTER(RayleighCfg), C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
    "bcn_rayleigh_reset": (C.c_int, [vp, vp, vp, vp]),
    "bcn_rayleigh_step": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "bcn_mixing_create": (C.c_int, [C.POINTER(MixingCfg), C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
    "bcn_mixing_reset": (C.c_int, [vp, vp, vp]),
    "bcn_mixing_step": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "bcn_burgers_create": (C.c_int, [C.POINTER(BurgersCfg), C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
    "bcn_burgers_reset": (C.c_int, [vp, vp, vp]),
    "bcn_burgers_step": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "bcn_shkadov_create": (C.c_int, [C.POINTER(ShkadovCfg), C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
    "bcn_shkadov_reset": (C.c_int, [vp, vp, vp, vp]),
    "bcn_shkadov_reset_random": (C.c_int, [vp, vp, vp, C.c_int, vp, vp, vp]),
    "bcn_shkadov_step": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "bcn_sloshing_create": (C.c_int, [C.POINTER(SloshingCfg), C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
    "bcn_sloshing_reset": (C.c_int, [vp, vp, vp, vp]),
    "bcn_sloshing_step": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp]),
    "bcn_lorenz_create": (C.c_int, [C.POINTER(LorenzCfg), C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
    "bcn_lorenz_reset": (C.c_int, [vp, vp, vp]),
    "bcn_lorenz_step": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp]),
    "bcn_vortex_create": (C.c_int, [C.POINTER(VortexCfg), C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
    "bcn_vortex_reset": (C.c_int, [vp, vp, vp]),
    "bcn_vortex_step": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp]),
    "bcn_env_kind": (C.c_int, [vp]),
    "bcn_batch": (C.c_int, [vp]),
    "bcn_dtype": (C.c_int, [vp]),
    "bcn_n_obs": (C.c_int, [vp]),
    "bcn_n_act": (C.c_int, [vp]),
    "bcn_ndt_act": (C.c_int, [vp]),
    "bcn_device": (C.c_int, [vp]),
    "bcn_state_elems": (C.c_size_t, [vp]),
    "bcn_get_state": (C.c_int, [vp, vp, C.c_int, vp]),
    "bcn_set_state": (C.c_int, [vp, vp, C.c_int, vp]),
    "bcn_set_mask": (C.c_int, [vp, vp]),
    "bcn_get_stp": (C.c_int, [vp, c_i32p, vp]),
    "bcn_set_stp": (C.c_int, [vp, c_i32p, vp]),
    "bcn_set_variant": (C.c_int, [vp, C.c_int]),
    "bcn_get_counters": (C.c_int, [vp, C.POINTER(C.c_uint64), vp]),
    "bcn_get_counters_n": (C.c_int, [vp, C.POINTER(C.c_uint64), C.c_int, vp]),
    "bcn_api_version": (C.c_int, []),
    "bcn_set_fast_plugin": (C.c_int, [vp, vp, C.c_size_t]),
    "bcn_set_fast_plugin_params": (C.c_int, [vp, vp]),
    "bcn_set_option": (C.c_int, [vp, C.c_char_p, C.c_int]),
    "bcn_set_noise": (C.c_int, [vp, C.c_double, C.c_uint64, C.c_int64]),
    "bcn_set_sched": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    "bcn_set_slow_mode_bound": (C.c_int, [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "bcn_get_slow_mode_bound": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "bcn_snapshot_bytes": (C.c_size_t, [vp]),
    "bcn_snapshot_bytes_n": (C.c_size_t, [vp, C.c_int]),
    "bcn_snapshot_layout": (C.c_int, [vp, C.c_int, C.POINTER(SnapshotSeg), C.c_int]),
    "bcn_snapshot_signature": (C.c_uint64, [vp]),
    "bcn_snapshot_save": (C.c_int, [vp, vp, vp, vp]),
    "bcn_snapshot_load": (C.c_int, [vp, vp, C.c_int, vp, vp, vp, vp]),
    "bcn_episode_bytes": (C.c_size_t, [vp]),
    "bcn_episode_layout": (C.c_int, [vp, C.POINTER(SnapshotSeg), C.c_int]),
    "bcn_episode_track": (C.c_int, [vp, vp, vp, vp, vp]),
    "bcn_shkadov_jets_bytes": (C.c_size_t, [vp]),
    "bcn_shkadov_jets_layout": (C.c_int, [vp, C.POINTER(SnapshotSeg), C.c_int]),
    "bcn_shkadov_jet_rewards": (C.c_int, [vp, vp, vp, C.c_int, vp]),
    "bcn_normalize_bytes": (C.c_size_t, [vp]),
    "bcn_normalize_layout": (C.c_int, [vp, C.POINTER(SnapshotSeg), C.c_int]),
    "bcn_normalize": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, vp]),
    "bcn_rollout_bytes": (C.c_size_t, [vp, C.c_int, C.c_int]),
    "bcn_rollout_layout": (C.c_int, [vp, C.c_int, C.c_int, C.POINTER(SnapshotSeg), C.c_int]),
    "bcn_rollout_begin": (C.c_int, [vp, vp, vp, vp, vp]),
    "bcn_rollout_record": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp]),
    "bcn_rollout_gae": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, vp]),
    "bcn_render_shape": (C.c_int, [vp, C.POINTER(RenderCfg), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bcn_render": (C.c_int, [vp, C.POINTER(RenderCfg), vp, vp, C.c_int, vp, vp]),
    "bcn_n_params": (C.c_int, [vp]),
    "bcn_param_name": (C.c_char_p, [vp, C.c_int]),
    "bcn_set_params": (C.c_int, [vp, C.POINTER(C.c_double), vp]),
    "bcn_get_params": (C.c_int, [vp, C.POINTER(C.c_double)]),
    "bcn_derive_params_host": (C.c_int, [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "bcn_kernel_name": (C.c_char_p, [vp]),
    "bcn_kernel_shape": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bcn_destroy": (C.c_int, [vp]),
    "bcn_last_error": (C.c_char_p, []),
    "bcn_version": (C.c_char_p, []),
}

_LIB = None


def lib_path():
    return _build.LIB


def load():
    """dlopen the in-tree library (building it first when stale and hipcc is present)."""
    global _LIB
    if _LIB is None:
        # RTLD_GLOBAL: the on-demand kernel plugins resolve bcn_set_error against it
        L = _build.MAIN.load(SIGNATURES, mode=C.RTLD_GLOBAL,
                             no_compiler="libbeacon_hip.so is missing or older than its sources and hipcc is not "
                                         "available to build it; beacon_amd has no CPU fallback")
        if L.bcn_api_version() != API_VERSION:
            raise RuntimeError("libbeacon_hip.so has API version %d, this binding expects %d" % (L.bcn_api_version(), API_VERSION))
        _LIB = L
    return _LIB


class BeaconHipError(RuntimeError):
    pass


def check(rc):
    if rc != 0:
        raise BeaconHipError("libbeacon_hip: error %d: %s" % (rc, load().bcn_last_error().decode()))
