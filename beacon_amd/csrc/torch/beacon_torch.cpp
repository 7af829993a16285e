// beacon_torch.cpp -- the thin PyTorch-ROCm extension over the C ABI (include/beacon_hip.h): torch.library ops
//   beacon::{rayleigh,mixing,burgers,shkadov,sloshing,lorenz,vortex}_{step,reset}(int handle, Tensor ...) -> ()
//   beacon::shkadov_reset_random(int handle, Tensor? init_fields, Tensor? n_steps, int rand_steps, Tensor? n_out, Tensor obs) -> ()
//   beacon::snapshot_{save,load}(int handle, Tensor ...) -> ()
//   beacon::episode_track(int handle, Tensor out_buf, Tensor ep_buf, Tensor? mask) -> ()
//   beacon::shkadov_jet_rewards(int handle, Tensor out_buf, Tensor jets_buf, int with_stats) -> ()
//   beacon::normalize(int handle, Tensor out_buf, Tensor norm_buf, Tensor? ep_buf, Tensor? mask, int kind, int training, float gamma, float eps,
//                     float clip_obs, float clip_rwd) -> ()
//   beacon::rollout_begin(int handle, Tensor ro_buf, Tensor out_buf, Tensor? norm_buf) -> ()
//   beacon::rollout_record(int handle, Tensor out_buf, Tensor ro_buf, Tensor? act, Tensor? ep_buf, Tensor? norm_buf, Tensor? jets_buf, Tensor? mask,
//                          int T, int flags) -> ()
//   beacon::rollout_gae(int handle, Tensor ro_buf, Tensor values, Tensor last_value, Tensor? final_values, int T, int flags, int cols, float gamma,
//                       float lam) -> ()
//   beacon::render(int handle, Tensor rgb, Tensor? lut, Tensor? replicas, int plane, int scale, int width, int height, int strip, int has_range,
//                  float lo, float hi, float ref) -> ()
// Each op is ONE dispatcher call that takes device tensors, reads torch's current HIP stream in C++ and forwards to the
// bcn_* entry point of libbeacon_hip.so -- no ctypes marshalling, no Python-side stream query (what the per-call host cost of
// the ctypes binding was made of: scripts/host_cost.py), and an op CUDA-graph capture and fake-tensor tracing can see (Meta kernels below).  The ops
// mutate their output tensors in place and return nothing; the size, dtype and device of EVERY tensor are checked here (a short buffer is an error, not an out-of-bounds write), the values by the library.
// Host code only: compiled with g++ against the torch headers (beacon_amd/torch_ext.py), linked to libbeacon_hip.so.
//
// The boundary each op stands in for is the reference's env method (rayleigh.py:89-157, mixing.py:73-135, burgers.py:68-117,
// shkadov.py:113-185, sloshing.py:92-166): reset() -> obs, step(a) -> (obs, rwd, done, trunc).
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include "../../../include/beacon_hip.h"

namespace {

using at::Tensor;
using OptT = const std::optional<Tensor>&;

inline bcn_env_t H(int64_t h) { return reinterpret_cast<bcn_env_t>(static_cast<intptr_t>(h)); }

inline void* stream_of(const Tensor& t) {
  return static_cast<void*>(c10::hip::getCurrentHIPStream(t.device().index()).stream());
}

inline void check(int rc, const char* what) {
  TORCH_CHECK(rc == BCN_OK, "libbeacon_hip: ", what, " failed with error ", rc, ": ", bcn_last_error());
}

// device pointer of a contiguous tensor on the handle's device, of the handle's dtype where `real`
inline void on_device(const Tensor& t, bcn_env_t h, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous(), name, ": contiguous device tensor expected");
  TORCH_CHECK(t.device().index() == bcn_device(h), name, ": lives on device ", (int)t.device().index(), " but the handle was created on device ",
              bcn_device(h));
}
inline void* dp(const Tensor& t, bcn_env_t h, bool real, const char* name) {
  on_device(t, h, name);
  if (real) {
    const auto want = bcn_dtype(h) == BCN_F64 ? at::kDouble : at::kFloat;
    TORCH_CHECK(t.scalar_type() == want, name, ": dtype ", t.scalar_type(), " but the handle computes in ", want);
  }
  return t.data_ptr();
}
inline void* dpo(OptT t, bcn_env_t h, bool real, const char* name) { return t.has_value() ? dp(*t, h, real, name) : nullptr; }
inline void rows(const Tensor& t, bcn_env_t h, int64_t per, const char* name) {
  TORCH_CHECK(t.numel() == (int64_t)bcn_batch(h) * per, name, ": ", t.numel(), " elements, expected batch ", bcn_batch(h), " x ", per);
}
// per-replica output words: `per` elements per replica, on the handle's device
inline uint8_t* u8(const Tensor& t, bcn_env_t h, int64_t per, const char* name) {
  on_device(t, h, name);
  TORCH_CHECK(t.scalar_type() == at::kByte, name, ": uint8 tensor expected");
  rows(t, h, per, name);
  return t.data_ptr<uint8_t>();
}
inline int32_t* i32(const Tensor& t, bcn_env_t h, int64_t per, const char* name) {
  on_device(t, h, name);
  TORCH_CHECK(t.scalar_type() == at::kInt, name, ": int32 tensor expected");
  rows(t, h, per, name);
  return t.data_ptr<int32_t>();
}
// optional real input of `per` elements per replica (actions, noise)
inline void* dpr(OptT t, bcn_env_t h, int64_t per, const char* name) {
  if (!t.has_value()) return nullptr;
  rows(*t, h, per, name);
  return dp(*t, h, true, name);
}

// The outputs of an env op, checked -- size, dtype, device and contiguity of each -- with what every op needs next to them: the
// handle and torch's current stream on the outputs' device.  reset ops have obs alone, step ops all five.
struct Outs {
  bcn_env_t h;
  void *obs, *rwd = nullptr, *stream;
  uint8_t *done = nullptr, *trunc = nullptr;
  int32_t* status = nullptr;
  Outs(int64_t h_, const Tensor& obs_) : h(H(h_)) {
    rows(obs_, h, bcn_n_obs(h), "obs");
    obs = dp(obs_, h, true, "obs");
    stream = stream_of(obs_);
  }
  Outs(int64_t h_, const Tensor& obs_, const Tensor& rwd_, const Tensor& done_, const Tensor& trunc_, const Tensor& status_) : Outs(h_, obs_) {
    rows(rwd_, h, 1, "rwd");
    rwd = dp(rwd_, h, true, "rwd");
    done = u8(done_, h, 1, "done");
    trunc = u8(trunc_, h, 1, "trunc");
    status = i32(status_, h, 1, "status");
  }
};
inline const int32_t* int_actions(OptT actions, bcn_env_t h) { return actions.has_value() ? i32(*actions, h, 1, "actions") : nullptr; }

// ---- rayleigh (rayleigh.py:89-157) -------------------------------------------------------------------------------------
void rayleigh_reset(int64_t h_, OptT init_fields, const Tensor& obs) {
  const Outs o(h_, obs);
  check(bcn_rayleigh_reset(o.h, dpo(init_fields, o.h, true, "init_fields"), o.obs, o.stream), "bcn_rayleigh_reset");
}
void rayleigh_step(int64_t h_, OptT actions, const Tensor& actions_norm, const Tensor& obs, const Tensor& rwd, const Tensor& done,
                   const Tensor& trunc, const Tensor& status, const Tensor& sweeps) {
  const Outs o(h_, obs, rwd, done, trunc, status);
  rows(actions_norm, o.h, bcn_n_act(o.h), "actions_norm");
  check(bcn_rayleigh_step(o.h, dpr(actions, o.h, bcn_n_act(o.h), "actions"), dp(actions_norm, o.h, true, "actions_norm"), o.obs, o.rwd, o.done,
                          o.trunc, o.status, i32(sweeps, o.h, bcn_ndt_act(o.h), "sweeps"), o.stream),
        "bcn_rayleigh_step");
}

// ---- mixing (mixing.py:73-135) -----------------------------------------------------------------------------------------
void mixing_reset(int64_t h_, const Tensor& obs) {
  const Outs o(h_, obs);
  check(bcn_mixing_reset(o.h, o.obs, o.stream), "bcn_mixing_reset");
}
void mixing_step(int64_t h_, OptT actions, const Tensor& obs, const Tensor& rwd, const Tensor& done, const Tensor& trunc,
                 const Tensor& status, const Tensor& sweeps) {
  const Outs o(h_, obs, rwd, done, trunc, status);
  check(bcn_mixing_step(o.h, int_actions(actions, o.h), o.obs, o.rwd, o.done, o.trunc, o.status, i32(sweeps, o.h, bcn_ndt_act(o.h), "sweeps"),
                        o.stream),
        "bcn_mixing_step");
}

// ---- burgers (burgers.py:68-117) ---------------------------------------------------------------------------------------
void burgers_reset(int64_t h_, const Tensor& obs) {
  const Outs o(h_, obs);
  check(bcn_burgers_reset(o.h, o.obs, o.stream), "bcn_burgers_reset");
}
void burgers_step(int64_t h_, OptT actions, OptT noise, const Tensor& obs, const Tensor& rwd, const Tensor& done, const Tensor& trunc,
                  const Tensor& status) {
  const Outs o(h_, obs, rwd, done, trunc, status);
  check(bcn_burgers_step(o.h, dpr(actions, o.h, 1, "actions"), dpr(noise, o.h, 1, "noise"), o.obs, o.rwd, o.done, o.trunc, o.status, o.stream),
        "bcn_burgers_step");
}

// ---- shkadov (shkadov.py:113-185) --------------------------------------------------------------------------------------
void shkadov_reset(int64_t h_, OptT init_fields, const Tensor& obs) {
  const Outs o(h_, obs);
  check(bcn_shkadov_reset(o.h, dpo(init_fields, o.h, true, "init_fields"), o.obs, o.stream), "bcn_shkadov_reset");
}
// shkadov.reset with rand_init (shkadov.py:119-123) in one launch: n_steps (the counts; None: drawn on the device) and n_out (the
// counts taken) are int32 [B]
void shkadov_reset_random(int64_t h_, OptT init_fields, OptT n_steps, int64_t rand_steps, OptT n_out, const Tensor& obs) {
  const Outs o(h_, obs);
  TORCH_CHECK(rand_steps >= 0 && rand_steps <= 65535, "rand_steps: ", rand_steps, " outside [0, 65535]");
  const int32_t* n = n_steps.has_value() ? i32(*n_steps, o.h, 1, "n_steps") : nullptr;
  int32_t* taken = n_out.has_value() ? i32(*n_out, o.h, 1, "n_out") : nullptr;
  check(bcn_shkadov_reset_random(o.h, dpo(init_fields, o.h, true, "init_fields"), n, (int)rand_steps, taken, o.obs, o.stream),
        "bcn_shkadov_reset_random");
}
void shkadov_step(int64_t h_, OptT actions, OptT noise, const Tensor& obs, const Tensor& rwd, const Tensor& done, const Tensor& trunc,
                  const Tensor& status) {
  const Outs o(h_, obs, rwd, done, trunc, status);
  check(bcn_shkadov_step(o.h, dpr(actions, o.h, bcn_n_act(o.h), "actions"), dpr(noise, o.h, bcn_ndt_act(o.h), "noise"), o.obs, o.rwd, o.done,
                         o.trunc, o.status, o.stream),
        "bcn_shkadov_step");
}

// ---- sloshing (sloshing.py:92-166) -------------------------------------------------------------------------------------
void sloshing_reset(int64_t h_, OptT init_fields, const Tensor& obs) {
  const Outs o(h_, obs);
  check(bcn_sloshing_reset(o.h, dpo(init_fields, o.h, true, "init_fields"), o.obs, o.stream), "bcn_sloshing_reset");
}
void sloshing_step(int64_t h_, OptT actions, const Tensor& obs, const Tensor& rwd, const Tensor& done, const Tensor& trunc,
                   const Tensor& status) {
  const Outs o(h_, obs, rwd, done, trunc, status);
  check(bcn_sloshing_step(o.h, dpr(actions, o.h, 1, "actions"), o.obs, o.rwd, o.done, o.trunc, o.status, o.stream), "bcn_sloshing_step");
}

// ---- lorenz (lorenz.py:60-117), vortex (vortex.py:82-146) --------------------------------------------------------------
void lorenz_reset(int64_t h_, const Tensor& obs) {
  const Outs o(h_, obs);
  check(bcn_lorenz_reset(o.h, o.obs, o.stream), "bcn_lorenz_reset");
}
void lorenz_step(int64_t h_, OptT actions, const Tensor& obs, const Tensor& rwd, const Tensor& done, const Tensor& trunc,
                 const Tensor& status) {
  const Outs o(h_, obs, rwd, done, trunc, status);
  check(bcn_lorenz_step(o.h, int_actions(actions, o.h), o.obs, o.rwd, o.done, o.trunc, o.status, o.stream), "bcn_lorenz_step");
}
void vortex_reset(int64_t h_, const Tensor& obs) {
  const Outs o(h_, obs);
  check(bcn_vortex_reset(o.h, o.obs, o.stream), "bcn_vortex_reset");
}
void vortex_step(int64_t h_, OptT actions, const Tensor& obs, const Tensor& rwd, const Tensor& done, const Tensor& trunc,
                 const Tensor& status) {
  const Outs o(h_, obs, rwd, done, trunc, status);
  check(bcn_vortex_step(o.h, dpr(actions, o.h, bcn_n_act(o.h), "actions"), o.obs, o.rwd, o.done, o.trunc, o.status, o.stream), "bcn_vortex_step");
}

// ---- snapshots (include/beacon_hip.h: bcn_snapshot_save / bcn_snapshot_load) --------------------------------------------
// bytes of the packed output buffer of the handle's batch (include/beacon_hip.h: bcn_out_layout)
inline int64_t out_buf_bytes(bcn_env_t h) {
  return (int64_t)bcn_out_layout((size_t)bcn_batch(h), (size_t)bcn_n_obs(h), bcn_dtype(h) == BCN_F64 ? 8 : 4).bytes;
}
inline uint8_t* bytes_of(const Tensor& t, bcn_env_t h, int64_t n, const char* name) {
  on_device(t, h, name);
  TORCH_CHECK(t.scalar_type() == at::kByte, name, ": uint8 tensor expected");
  TORCH_CHECK(t.numel() == n, name, ": ", t.numel(), " bytes, expected ", n);
  TORCH_CHECK((reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0, name, ": must be 16-byte aligned");
  return t.data_ptr<uint8_t>();
}
void snapshot_save(int64_t h_, const Tensor& snap, const Tensor& out_buf) {
  bcn_env_t h = H(h_);
  uint8_t* s = bytes_of(snap, h, (int64_t)bcn_snapshot_bytes(h), "snap");
  check(bcn_snapshot_save(h, s, bytes_of(out_buf, h, out_buf_bytes(h), "out_buf"), stream_of(snap)), "bcn_snapshot_save");
}
void snapshot_load(int64_t h_, const Tensor& snap, int64_t n_src, OptT src, OptT mask, const Tensor& out_buf) {
  bcn_env_t h = H(h_);
  TORCH_CHECK(n_src >= 1 && n_src <= INT32_MAX, "n_src: ", n_src, " replicas");
  TORCH_CHECK(src.has_value() || n_src == bcn_batch(h), "snapshot of ", n_src, " replicas into a batch of ", bcn_batch(h), " needs src");
  const uint8_t* s = bytes_of(snap, h, (int64_t)bcn_snapshot_bytes_n(h, (int)n_src), "snap");
  const int32_t* idx = src.has_value() ? i32(*src, h, 1, "src") : nullptr;
  const uint8_t* m = mask.has_value() ? u8(*mask, h, 1, "mask") : nullptr;
  check(bcn_snapshot_load(h, s, (int)n_src, idx, m, bytes_of(out_buf, h, out_buf_bytes(h), "out_buf"), stream_of(out_buf)), "bcn_snapshot_load");
}

// ---- episode statistics (include/beacon_hip.h: bcn_episode_track) -------------------------------------------------------
void episode_track(int64_t h_, const Tensor& out_buf, const Tensor& ep_buf, OptT mask) {
  bcn_env_t h = H(h_);
  const uint8_t* o = bytes_of(out_buf, h, out_buf_bytes(h), "out_buf");
  uint8_t* e = bytes_of(ep_buf, h, (int64_t)bcn_episode_bytes(h), "ep_buf");
  const uint8_t* m = mask.has_value() ? u8(*mask, h, 1, "mask") : nullptr;
  check(bcn_episode_track(h, o, e, m, stream_of(ep_buf)), "bcn_episode_track");
}

// ---- per-jet rewards of shkadov (include/beacon_hip.h: bcn_shkadov_jet_rewards; shkadov.py:469-481) ----------------------
void shkadov_jet_rewards(int64_t h_, const Tensor& out_buf, const Tensor& jets_buf, int64_t with_stats) {
  bcn_env_t h = H(h_);
  TORCH_CHECK(h && bcn_env_kind(h) == BCN_SHKADOV, "shkadov_jet_rewards: the handle is not a shkadov env");
  const uint8_t* o = bytes_of(out_buf, h, out_buf_bytes(h), "out_buf");
  uint8_t* j = bytes_of(jets_buf, h, (int64_t)bcn_shkadov_jets_bytes(h), "jets_buf");
  check(bcn_shkadov_jet_rewards(h, o, j, with_stats != 0, stream_of(jets_buf)), "bcn_shkadov_jet_rewards");
}

// ---- running normalisation of observations and rewards (include/beacon_hip.h: bcn_normalize) ----------------------------
void normalize(int64_t h_, const Tensor& out_buf, const Tensor& norm_buf, OptT ep_buf, OptT mask, int64_t kind, int64_t training, double gamma,
               double eps, double clip_obs, double clip_rwd) {
  bcn_env_t h = H(h_);
  const uint8_t* o = bytes_of(out_buf, h, out_buf_bytes(h), "out_buf");
  uint8_t* n = bytes_of(norm_buf, h, (int64_t)bcn_normalize_bytes(h), "norm_buf");
  const uint8_t* e = ep_buf.has_value() ? bytes_of(*ep_buf, h, (int64_t)bcn_episode_bytes(h), "ep_buf") : nullptr;
  const uint8_t* m = mask.has_value() ? u8(*mask, h, 1, "mask") : nullptr;
  TORCH_CHECK(kind == BCN_NORM_STEP || kind == BCN_NORM_RESET, "kind: ", kind, " is neither BCN_NORM_STEP nor BCN_NORM_RESET");
  check(bcn_normalize(h, o, n, e, m, (int)kind, training != 0, gamma, eps, clip_obs, clip_rwd, stream_of(norm_buf)), "bcn_normalize");
}

// ---- rollout storage and GAE (include/beacon_hip.h: bcn_rollout_begin / bcn_rollout_record / bcn_rollout_gae) --------------
// the rollout buffer of T steps under `flags`: its exact size, with the message of the library for a T or flags it refuses
inline uint8_t* rollout_buf(const Tensor& t, bcn_env_t h, int64_t T, int64_t flags) {
  TORCH_CHECK(h, "rollout: null handle");
  TORCH_CHECK(T >= 1 && T <= INT32_MAX && flags >= 0 && flags <= INT32_MAX, "rollout: T = ", T, ", flags = ", flags);
  const size_t n = bcn_rollout_bytes(h, (int)T, (int)flags);
  TORCH_CHECK(n > 0, "libbeacon_hip: ", bcn_last_error());
  return bytes_of(t, h, (int64_t)n, "ro_buf");
}
void rollout_begin(int64_t h_, const Tensor& ro_buf, const Tensor& out_buf, OptT norm_buf) {
  bcn_env_t h = H(h_);
  TORCH_CHECK(h, "rollout_begin: null handle");
  on_device(ro_buf, h, "ro_buf");                // T is not known here: at least the cursor and obs[0], obs[1] (T = 1, no flags)
  TORCH_CHECK(ro_buf.scalar_type() == at::kByte && ro_buf.numel() >= (int64_t)bcn_rollout_bytes(h, 1, 0), "ro_buf: uint8 tensor of at least ",
              bcn_rollout_bytes(h, 1, 0), " bytes expected");
  const uint8_t* o = bytes_of(out_buf, h, out_buf_bytes(h), "out_buf");
  const uint8_t* n = norm_buf.has_value() ? bytes_of(*norm_buf, h, (int64_t)bcn_normalize_bytes(h), "norm_buf") : nullptr;
  check(bcn_rollout_begin(h, ro_buf.data_ptr(), o, n, stream_of(ro_buf)), "bcn_rollout_begin");
}
void rollout_record(int64_t h_, const Tensor& out_buf, const Tensor& ro_buf, OptT act, OptT ep_buf, OptT norm_buf, OptT jets_buf, OptT mask,
                    int64_t T, int64_t flags) {
  bcn_env_t h = H(h_);
  uint8_t* r = rollout_buf(ro_buf, h, T, flags);
  const uint8_t* o = bytes_of(out_buf, h, out_buf_bytes(h), "out_buf");
  const void* a = nullptr;
  if (act.has_value()) {                         // element type and row length: those of the act segment
    bcn_snapshot_seg lay[3];
    TORCH_CHECK(bcn_rollout_layout(h, (int)T, (int)flags, lay, 3) > 0, "libbeacon_hip: ", bcn_last_error());
    a = lay[2].elem == BCN_SNAP_I32 ? static_cast<const void*>(i32(*act, h, lay[2].row_elems, "act")) : dpr(act, h, lay[2].row_elems, "act");
  }
  const uint8_t* e = ep_buf.has_value() ? bytes_of(*ep_buf, h, (int64_t)bcn_episode_bytes(h), "ep_buf") : nullptr;
  const uint8_t* n = norm_buf.has_value() ? bytes_of(*norm_buf, h, (int64_t)bcn_normalize_bytes(h), "norm_buf") : nullptr;
  const uint8_t* j = nullptr;
  if (jets_buf.has_value()) {
    TORCH_CHECK(bcn_env_kind(h) == BCN_SHKADOV, "jets_buf: the handle is not a shkadov env");
    j = bytes_of(*jets_buf, h, (int64_t)bcn_shkadov_jets_bytes(h), "jets_buf");
  }
  const uint8_t* m = mask.has_value() ? u8(*mask, h, 1, "mask") : nullptr;
  check(bcn_rollout_record(h, o, r, a, e, n, j, m, (int)T, (int)flags, stream_of(ro_buf)), "bcn_rollout_record");
}
void rollout_gae(int64_t h_, const Tensor& ro_buf, const Tensor& values, const Tensor& last_value, OptT final_values, int64_t T, int64_t flags,
                 int64_t cols, double gamma, double lam) {
  bcn_env_t h = H(h_);
  uint8_t* r = rollout_buf(ro_buf, h, T, flags);
  TORCH_CHECK(cols == 1 || ((flags & BCN_RO_JETS) && cols == bcn_n_act(h)), "cols: ", cols, "; 1, or the jet count with BCN_RO_JETS");
  rows(values, h, T * cols, "values");
  rows(last_value, h, cols, "last_value");
  if (final_values.has_value()) rows(*final_values, h, T * cols, "final_values");
  check(bcn_rollout_gae(h, r, dp(values, h, true, "values"), dp(last_value, h, true, "last_value"), dpo(final_values, h, true, "final_values"),
                        (int)T, (int)flags, (int)cols, gamma, lam, stream_of(ro_buf)),
        "bcn_rollout_gae");
}

// ---- frames (include/beacon_hip.h: bcn_render) ---------------------------------------------------------------------------
// rgb: uint8 [n, H_px, W_px, 3] for the shape bcn_render_shape gives; lut: uint8 [256, 3]; replicas: int32 [n] (None: n is the batch)
void render(int64_t h_, const Tensor& rgb, OptT lut, OptT replicas, int64_t plane, int64_t scale, int64_t width, int64_t height, int64_t strip,
            int64_t has_range, double lo, double hi, double ref) {
  bcn_env_t h = H(h_);
  TORCH_CHECK(h, "render: null handle");
  for (int64_t v : {plane, scale, width, height, strip}) TORCH_CHECK(v >= INT32_MIN && v <= INT32_MAX, "render: argument ", v, " out of range");
  bcn_render_cfg cfg;
  cfg.plane = (int32_t)plane; cfg.scale = (int32_t)scale; cfg.width = (int32_t)width; cfg.height = (int32_t)height; cfg.strip = (int32_t)strip;
  cfg.has_range = has_range != 0; cfg.lo = lo; cfg.hi = hi; cfg.ref = ref;
  int H_px = 0, W_px = 0;
  check(bcn_render_shape(h, &cfg, &H_px, &W_px), "bcn_render_shape");
  on_device(rgb, h, "rgb");
  TORCH_CHECK(rgb.scalar_type() == at::kByte, "rgb: uint8 tensor expected");
  TORCH_CHECK(rgb.dim() == 4 && rgb.size(1) == H_px && rgb.size(2) == W_px && rgb.size(3) == 3, "rgb: [n, ", H_px, ", ", W_px, ", 3] expected, got ",
              rgb.sizes());
  const int64_t n = rgb.size(0);
  TORCH_CHECK(n <= INT32_MAX, "rgb: ", n, " frames");
  const int32_t* idx = nullptr;
  if (replicas.has_value()) {
    on_device(*replicas, h, "replicas");
    TORCH_CHECK(replicas->scalar_type() == at::kInt && replicas->numel() == n, "replicas: int32 tensor of ", n, " indices expected");
    idx = replicas->data_ptr<int32_t>();
  } else {
    TORCH_CHECK(n == bcn_batch(h), "rgb: ", n, " frames for a batch of ", bcn_batch(h), " need replicas");
  }
  const uint8_t* table = nullptr;
  if (lut.has_value()) {
    on_device(*lut, h, "lut");
    TORCH_CHECK(lut->scalar_type() == at::kByte && lut->numel() == 768, "lut: uint8 [256, 3] expected");
    table = lut->data_ptr<uint8_t>();
  }
  check(bcn_render(h, &cfg, table, idx, (int)n, rgb.data_ptr<uint8_t>(), stream_of(rgb)), "bcn_render");
}

// Meta (fake-tensor) kernels: the ops return nothing and their outputs keep their shapes, so tracing needs no more than this.
void reset2_meta(int64_t, const Tensor&) {}
void reset3_meta(int64_t, OptT, const Tensor&) {}
void reset_random_meta(int64_t, OptT, OptT, int64_t, OptT, const Tensor&) {}
void rayleigh_step_meta(int64_t, OptT, const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&) {}
void mixing_step_meta(int64_t, OptT, const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&) {}
void noisy_step_meta(int64_t, OptT, OptT, const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&) {}
void sloshing_step_meta(int64_t, OptT, const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor&) {}   // also lorenz, vortex
void snapshot_save_meta(int64_t, const Tensor&, const Tensor&) {}
void snapshot_load_meta(int64_t, const Tensor&, int64_t, OptT, OptT, const Tensor&) {}
void episode_track_meta(int64_t, const Tensor&, const Tensor&, OptT) {}
void shkadov_jet_rewards_meta(int64_t, const Tensor&, const Tensor&, int64_t) {}
void normalize_meta(int64_t, const Tensor&, const Tensor&, OptT, OptT, int64_t, int64_t, double, double, double, double) {}
void rollout_begin_meta(int64_t, const Tensor&, const Tensor&, OptT) {}
void rollout_record_meta(int64_t, const Tensor&, const Tensor&, OptT, OptT, OptT, OptT, OptT, int64_t, int64_t) {}
void rollout_gae_meta(int64_t, const Tensor&, const Tensor&, const Tensor&, OptT, int64_t, int64_t, int64_t, double, double) {}
void render_meta(int64_t, const Tensor&, OptT, OptT, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, double, double, double) {}

}  // namespace

// Outputs are written in place (annotated (x!)); the ops return nothing.  `handle` is the bcn_env_t of bcn_*_create as an
// integer.  Registered for the CUDA dispatch key, which is what ROCm tensors carry.
TORCH_LIBRARY(beacon, m) {
  m.def("rayleigh_reset(int handle, Tensor? init_fields, Tensor(a!) obs) -> ()");
  m.def("rayleigh_step(int handle, Tensor? actions, Tensor(a!) actions_norm, Tensor(b!) obs, Tensor(c!) rwd, Tensor(d!) done, "
        "Tensor(e!) trunc, Tensor(f!) status, Tensor(g!) sweeps) -> ()");
  m.def("mixing_reset(int handle, Tensor(a!) obs) -> ()");
  m.def("mixing_step(int handle, Tensor? actions, Tensor(a!) obs, Tensor(b!) rwd, Tensor(c!) done, Tensor(d!) trunc, "
        "Tensor(e!) status, Tensor(f!) sweeps) -> ()");
  m.def("burgers_reset(int handle, Tensor(a!) obs) -> ()");
  m.def("burgers_step(int handle, Tensor? actions, Tensor? noise, Tensor(a!) obs, Tensor(b!) rwd, Tensor(c!) done, Tensor(d!) trunc, "
        "Tensor(e!) status) -> ()");
  m.def("shkadov_reset(int handle, Tensor? init_fields, Tensor(a!) obs) -> ()");
  m.def("shkadov_reset_random(int handle, Tensor? init_fields, Tensor? n_steps, int rand_steps, Tensor(a!)? n_out, Tensor(b!) obs) -> ()");
  m.def("shkadov_step(int handle, Tensor? actions, Tensor? noise, Tensor(a!) obs, Tensor(b!) rwd, Tensor(c!) done, Tensor(d!) trunc, "
        "Tensor(e!) status) -> ()");
  m.def("sloshing_reset(int handle, Tensor? init_fields, Tensor(a!) obs) -> ()");
  m.def("sloshing_step(int handle, Tensor? actions, Tensor(a!) obs, Tensor(b!) rwd, Tensor(c!) done, Tensor(d!) trunc, "
        "Tensor(e!) status) -> ()");
  m.def("lorenz_reset(int handle, Tensor(a!) obs) -> ()");
  m.def("lorenz_step(int handle, Tensor? actions, Tensor(a!) obs, Tensor(b!) rwd, Tensor(c!) done, Tensor(d!) trunc, "
        "Tensor(e!) status) -> ()");
  m.def("vortex_reset(int handle, Tensor(a!) obs) -> ()");
  m.def("vortex_step(int handle, Tensor? actions, Tensor(a!) obs, Tensor(b!) rwd, Tensor(c!) done, Tensor(d!) trunc, "
        "Tensor(e!) status) -> ()");
  m.def("snapshot_save(int handle, Tensor(a!) snap, Tensor out_buf) -> ()");
  m.def("snapshot_load(int handle, Tensor snap, int n_src, Tensor? src, Tensor? mask, Tensor(a!) out_buf) -> ()");
  m.def("episode_track(int handle, Tensor out_buf, Tensor(a!) ep_buf, Tensor? mask) -> ()");
  m.def("shkadov_jet_rewards(int handle, Tensor out_buf, Tensor(a!) jets_buf, int with_stats) -> ()");
  m.def("normalize(int handle, Tensor out_buf, Tensor(a!) norm_buf, Tensor? ep_buf, Tensor? mask, int kind, int training, float gamma, "
        "float eps, float clip_obs, float clip_rwd) -> ()");
  m.def("rollout_begin(int handle, Tensor(a!) ro_buf, Tensor out_buf, Tensor? norm_buf) -> ()");
  m.def("rollout_record(int handle, Tensor out_buf, Tensor(a!) ro_buf, Tensor? act, Tensor? ep_buf, Tensor? norm_buf, Tensor? jets_buf, "
        "Tensor? mask, int T, int flags) -> ()");
  m.def("rollout_gae(int handle, Tensor(a!) ro_buf, Tensor values, Tensor last_value, Tensor? final_values, int T, int flags, int cols, "
        "float gamma, float lam) -> ()");
  m.def("render(int handle, Tensor(a!) rgb, Tensor? lut, Tensor? replicas, int plane, int scale, int width, int height, int strip, "
        "int has_range, float lo, float hi, float ref) -> ()");
}

TORCH_LIBRARY_IMPL(beacon, CUDA, m) {
  m.impl("rayleigh_reset", &rayleigh_reset);
  m.impl("rayleigh_step", &rayleigh_step);
  m.impl("mixing_reset", &mixing_reset);
  m.impl("mixing_step", &mixing_step);
  m.impl("burgers_reset", &burgers_reset);
  m.impl("burgers_step", &burgers_step);
  m.impl("shkadov_reset", &shkadov_reset);
  m.impl("shkadov_reset_random", &shkadov_reset_random);
  m.impl("shkadov_step", &shkadov_step);
  m.impl("sloshing_reset", &sloshing_reset);
  m.impl("sloshing_step", &sloshing_step);
  m.impl("lorenz_reset", &lorenz_reset);
  m.impl("lorenz_step", &lorenz_step);
  m.impl("vortex_reset", &vortex_reset);
  m.impl("vortex_step", &vortex_step);
  m.impl("snapshot_save", &snapshot_save);
  m.impl("snapshot_load", &snapshot_load);
  m.impl("episode_track", &episode_track);
  m.impl("shkadov_jet_rewards", &shkadov_jet_rewards);
  m.impl("normalize", &normalize);
  m.impl("rollout_begin", &rollout_begin);
  m.impl("rollout_record", &rollout_record);
  m.impl("rollout_gae", &rollout_gae);
  m.impl("render", &render);
}

TORCH_LIBRARY_IMPL(beacon, Meta, m) {
  m.impl("rayleigh_reset", &reset3_meta);
  m.impl("rayleigh_step", &rayleigh_step_meta);
  m.impl("mixing_reset", &reset2_meta);
  m.impl("mixing_step", &mixing_step_meta);
  m.impl("burgers_reset", &reset2_meta);
  m.impl("burgers_step", &noisy_step_meta);
  m.impl("shkadov_reset", &reset3_meta);
  m.impl("shkadov_reset_random", &reset_random_meta);
  m.impl("shkadov_step", &noisy_step_meta);
  m.impl("sloshing_reset", &reset3_meta);
  m.impl("sloshing_step", &sloshing_step_meta);
  m.impl("lorenz_reset", &reset2_meta);
  m.impl("lorenz_step", &sloshing_step_meta);
  m.impl("vortex_reset", &reset2_meta);
  m.impl("vortex_step", &sloshing_step_meta);
  m.impl("snapshot_save", &snapshot_save_meta);
  m.impl("snapshot_load", &snapshot_load_meta);
  m.impl("episode_track", &episode_track_meta);
  m.impl("shkadov_jet_rewards", &shkadov_jet_rewards_meta);
  m.impl("normalize", &normalize_meta);
  m.impl("rollout_begin", &rollout_begin_meta);
  m.impl("rollout_record", &rollout_record_meta);
  m.impl("rollout_gae", &rollout_gae_meta);
  m.impl("render", &render_meta);
}
