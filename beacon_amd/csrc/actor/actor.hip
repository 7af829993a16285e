// actor.hip -- the C ABI of libbeacon_actor.so (include/beacon_actor.h): the three layouts, the two launches, and the float32
// instantiation of the kernel (actor_impl.h).  The float64 instantiation is actor_f64.hip, built without FMA contraction.  The cfg
// rules, the parameter layout and the network's part of the argument block are policy_net.h, shared with the learner's library.
#include "actor_impl.h"

static thread_local PolicyErr g_actor_err;

extern "C" BCN_ACTOR_API const char* bcn_actor_last_error(void) { return g_actor_err.text; }

ACTOR_DEFINE_LAUNCH(float)

// ---- cfg and layouts ---------------------------------------------------------------------
static bool actor_cfg_ok(const bcn_actor_cfg* c, bool need_batch) { return policy_cfg_ok(c, need_batch, &g_actor_err); }

static int actor_state_desc(const bcn_actor_cfg* c, PolicySegDesc* d) {
  const size_t n = (size_t)c->act_dim;
  const bool cat = c->kind == BCN_ACTOR_CATEGORICAL;
  const PolicySegDesc s[6] = {{"counters", BCN_ACTOR_U32, 1, 1}, {"actions", cat ? BCN_ACTOR_I32 : BCN_ACTOR_REAL, 1, cat ? 1 : n},
                             {"raw", BCN_ACTOR_REAL, 1, n}, {"logp", BCN_ACTOR_REAL, 1, 1}, {"value", BCN_ACTOR_REAL, 1, 1},
                             {"dist", BCN_ACTOR_REAL, 1, n}};
  memcpy(d, s, sizeof(s));
  return 6;
}

static int actor_seq_desc(const bcn_actor_cfg* c, int T, PolicySegDesc* d) {
  const PolicySegDesc s[3] = {{"logp_seq", BCN_ACTOR_REAL, T, 1}, {"value_seq", BCN_ACTOR_REAL, T, 1}, {"raw_seq", BCN_ACTOR_REAL, T, (size_t)c->act_dim}};
  memcpy(d, s, sizeof(s));
  return 3;
}

extern "C" {

BCN_ACTOR_API int bcn_actor_params_layout(const bcn_actor_cfg* cfg, bcn_actor_seg* segs, int max_segs) {
  if (!actor_cfg_ok(cfg, false)) return 0;
  size_t bytes;
  return policy_params_lay(cfg, segs, max_segs, &bytes);
}

BCN_ACTOR_API size_t bcn_actor_params_bytes(const bcn_actor_cfg* cfg) {
  if (!actor_cfg_ok(cfg, false)) return 0;
  size_t bytes;
  policy_params_lay(cfg, nullptr, 0, &bytes);
  return bytes;
}

BCN_ACTOR_API int bcn_actor_state_layout(const bcn_actor_cfg* cfg, bcn_actor_seg* segs, int max_segs) {
  if (!actor_cfg_ok(cfg, true)) return 0;
  PolicySegDesc d[BCN_ACTOR_MAX_SEGS];
  const int nd = actor_state_desc(cfg, d);
  policy_lay(d, nd, (size_t)cfg->batch, policy_esz(cfg), segs, max_segs);
  return nd;
}

BCN_ACTOR_API size_t bcn_actor_state_bytes(const bcn_actor_cfg* cfg) {
  if (!actor_cfg_ok(cfg, true)) return 0;
  PolicySegDesc d[BCN_ACTOR_MAX_SEGS];
  return policy_lay(d, actor_state_desc(cfg, d), (size_t)cfg->batch, policy_esz(cfg), nullptr, 0);
}

BCN_ACTOR_API int bcn_actor_seq_layout(const bcn_actor_cfg* cfg, int T, bcn_actor_seg* segs, int max_segs) {
  if (!actor_cfg_ok(cfg, true)) return 0;
  if (T < 1) { g_actor_err.set("T = %d: must be >= 1", T); return 0; }
  PolicySegDesc d[BCN_ACTOR_MAX_SEGS];
  const int nd = actor_seq_desc(cfg, T, d);
  policy_lay(d, nd, (size_t)cfg->batch, policy_esz(cfg), segs, max_segs);
  return nd;
}

BCN_ACTOR_API size_t bcn_actor_seq_bytes(const bcn_actor_cfg* cfg, int T) {
  if (!actor_cfg_ok(cfg, true)) return 0;
  if (T < 1) { g_actor_err.set("T = %d: must be >= 1", T); return 0; }
  PolicySegDesc d[BCN_ACTOR_MAX_SEGS];
  return policy_lay(d, actor_seq_desc(cfg, T, d), (size_t)cfg->batch, policy_esz(cfg), nullptr, 0);
}

}  // extern "C"

// ---- launches ----------------------------------------------------------------------------
// the part of the argument block that the cfg and the parameter layout decide
template <typename real>
static void actor_fill(const bcn_actor_cfg* c, const void* params, const void* obs, long long n_rows, ActorArgs<real>* a) {
  memset(a, 0, sizeof(*a));
  policy_fill_net<real>(c, params, a);
  a->obs = static_cast<const real*>(obs);
  a->n_rows = n_rows;
  a->low = (real)c->low; a->high = (real)c->high;
}

template <typename real>
static int actor_act_t(const bcn_actor_cfg* c, const void* params, const void* obs, void* state, const uint8_t* mask, uint64_t seed,
                       int64_t replica_offset, int deterministic, const int32_t* cursor, int T, void* seq, void* stream) {
  ActorArgs<real> a;
  actor_fill<real>(c, params, obs, (long long)c->batch, &a);
  bcn_actor_seg s[BCN_ACTOR_MAX_SEGS];
  bcn_actor_state_layout(c, s, BCN_ACTOR_MAX_SEGS);
  char* st = static_cast<char*>(state);
  a.counters = reinterpret_cast<uint32_t*>(st + s[0].offset);
  a.actions = st + s[1].offset;
  a.raw = reinterpret_cast<real*>(st + s[2].offset);
  a.logp = reinterpret_cast<real*>(st + s[3].offset);
  a.value = reinterpret_cast<real*>(st + s[4].offset);
  a.dist = reinterpret_cast<real*>(st + s[5].offset);
  a.mask = mask;
  a.agents = policy_agents(c);
  a.seed_lo = (uint32_t)(seed & 0xffffffffull); a.seed_hi = (uint32_t)(seed >> 32);
  // row 0's global index: the first replica's times the rows per replica, in 64 bits (the kernel adds b and keeps the low word)
  a.replica_offset = (long long)((unsigned long long)replica_offset * (unsigned long long)a.agents);
  a.deterministic = deterministic != 0;
  if (cursor) {
    bcn_actor_seq_layout(c, T, s, BCN_ACTOR_MAX_SEGS);
    char* sq = static_cast<char*>(seq);
    a.cursor = cursor; a.T = T;
    a.logp_seq = reinterpret_cast<real*>(sq + s[0].offset);
    a.value_seq = reinterpret_cast<real*>(sq + s[1].offset);
    a.raw_seq = reinterpret_cast<real*>(sq + s[2].offset);
  }
  const int e = actor_launch<real>(a, stream);
  if (e) { g_actor_err.set("bcn_actor_act: launch -> %s", hipGetErrorString((hipError_t)e)); return BCN_ACTOR_ERR_HIP; }
  return BCN_ACTOR_OK;
}

template <typename real>
static int actor_values_t(const bcn_actor_cfg* c, const void* params, const void* obs, int64_t n_rows, void* out, void* stream) {
  ActorArgs<real> a;
  actor_fill<real>(c, params, obs, (long long)n_rows, &a);
  a.values_only = 1;
  a.value = static_cast<real*>(out);
  const int e = actor_launch<real>(a, stream);
  if (e) { g_actor_err.set("bcn_actor_values: launch -> %s", hipGetErrorString((hipError_t)e)); return BCN_ACTOR_ERR_HIP; }
  return BCN_ACTOR_OK;
}

extern "C" {

BCN_ACTOR_API int bcn_actor_act(const bcn_actor_cfg* cfg, const void* params_dev, const void* obs_dev, void* state_dev, const uint8_t* mask_dev,
                                uint64_t seed, int64_t replica_offset, int deterministic, const int32_t* cursor_dev, int T, void* seq_dev,
                                void* stream) {
  if (!actor_cfg_ok(cfg, true)) return BCN_ACTOR_ERR_ARG;
  if (!params_dev || !obs_dev || !state_dev) { g_actor_err.set("bcn_actor_act: params_dev, obs_dev and state_dev must not be NULL"); return BCN_ACTOR_ERR_ARG; }
  if (cursor_dev && (T < 1 || !seq_dev)) { g_actor_err.set("bcn_actor_act: a cursor needs T >= 1 and seq_dev"); return BCN_ACTOR_ERR_ARG; }
  return cfg->dtype ? actor_act_t<double>(cfg, params_dev, obs_dev, state_dev, mask_dev, seed, replica_offset, deterministic, cursor_dev, T, seq_dev, stream)
                    : actor_act_t<float>(cfg, params_dev, obs_dev, state_dev, mask_dev, seed, replica_offset, deterministic, cursor_dev, T, seq_dev, stream);
}

BCN_ACTOR_API int bcn_actor_values(const bcn_actor_cfg* cfg, const void* params_dev, const void* obs_dev, int64_t n_rows, void* out_dev,
                                   void* stream) {
  if (!actor_cfg_ok(cfg, false)) return BCN_ACTOR_ERR_ARG;
  if (!params_dev || !obs_dev || !out_dev) { g_actor_err.set("bcn_actor_values: params_dev, obs_dev and out_dev must not be NULL"); return BCN_ACTOR_ERR_ARG; }
  if (n_rows < 1 || n_rows > 0x7fffffffll * 32) { g_actor_err.set("bcn_actor_values: n_rows = %lld is outside what one launch covers", (long long)n_rows); return BCN_ACTOR_ERR_ARG; }
  return cfg->dtype ? actor_values_t<double>(cfg, params_dev, obs_dev, n_rows, out_dev, stream)
                    : actor_values_t<float>(cfg, params_dev, obs_dev, n_rows, out_dev, stream);
}

}  // extern "C"
