// actor.hip -- the C ABI of libbeacon_actor.so (include/beacon_actor.h): cfg checks, the three layouts, the two launches, and the
// float32 instantiation of the kernel (actor_impl.h).  The float64 instantiation is actor_f64.hip, built without FMA contraction.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "actor_impl.h"

static thread_local char g_actor_err[512] = "";

static void actor_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_actor_err, sizeof(g_actor_err), fmt, ap);
  va_end(ap);
}

extern "C" BCN_ACTOR_API const char* bcn_actor_last_error(void) { return g_actor_err; }

ACTOR_DEFINE_LAUNCH(float)

// ---- cfg and layouts ---------------------------------------------------------------------
static bool actor_cfg_ok(const bcn_actor_cfg* c, bool need_batch) {
  if (!c) { actor_set_error("cfg is NULL"); return false; }
  if (need_batch && c->batch < 1) { actor_set_error("cfg.batch = %d: must be >= 1", c->batch); return false; }
  if (c->obs_dim < 1 || c->obs_dim > BCN_ACTOR_MAX_OBS) { actor_set_error("cfg.obs_dim = %d: must lie in 1 .. %d", c->obs_dim, BCN_ACTOR_MAX_OBS); return false; }
  if (c->dtype != 0 && c->dtype != 1) { actor_set_error("cfg.dtype = %d: must be 0 (float32) or 1 (float64)", c->dtype); return false; }
  if (c->n_hidden < 1 || c->n_hidden > BCN_ACTOR_MAX_LAYERS) { actor_set_error("cfg.n_hidden = %d: must lie in 1 .. %d", c->n_hidden, BCN_ACTOR_MAX_LAYERS); return false; }
  for (int l = 0; l < c->n_hidden; l++)
    if (c->hidden[l] < 1 || c->hidden[l] > BCN_ACTOR_MAX_HIDDEN) {
      actor_set_error("cfg.hidden[%d] = %d: must lie in 1 .. %d", l, c->hidden[l], BCN_ACTOR_MAX_HIDDEN);
      return false;
    }
  if (c->activation != BCN_ACTOR_TANH && c->activation != BCN_ACTOR_RELU) { actor_set_error("cfg.activation = %d: must be 0 (tanh) or 1 (relu)", c->activation); return false; }
  if (c->kind != BCN_ACTOR_GAUSSIAN && c->kind != BCN_ACTOR_CATEGORICAL) { actor_set_error("cfg.kind = %d: must be 0 (Gaussian) or 1 (categorical)", c->kind); return false; }
  const int lo = c->kind == BCN_ACTOR_GAUSSIAN ? 1 : 2;
  if (c->act_dim < lo || c->act_dim > BCN_ACTOR_MAX_ACT) { actor_set_error("cfg.act_dim = %d: must lie in %d .. %d for this kind", c->act_dim, lo, BCN_ACTOR_MAX_ACT); return false; }
  if (c->kind == BCN_ACTOR_GAUSSIAN && !(c->low <= c->high)) { actor_set_error("cfg.low = %g, cfg.high = %g: need low <= high", c->low, c->high); return false; }
  return true;
}

struct ActorSegDesc { char name[16]; int elem; int planes; size_t row_elems; };

static size_t actor_up16(size_t x) { return (x + 15) & ~(size_t)15; }

// lays nd segments out for `rows` rows per plane; returns the bytes
static size_t actor_lay(const ActorSegDesc* d, int nd, size_t rows, size_t esz, bcn_actor_seg* segs, int max_segs) {
  size_t off = 0;
  for (int k = 0; k < nd; k++) {
    off = actor_up16(off);
    if (segs && k < max_segs) {
      memset(&segs[k], 0, sizeof(segs[k]));
      strncpy(segs[k].name, d[k].name, sizeof(segs[k].name) - 1);
      segs[k].offset = off; segs[k].elem = d[k].elem; segs[k].planes = d[k].planes; segs[k].row_elems = (int64_t)d[k].row_elems;
    }
    off += (d[k].planes == 0 ? 1 : (size_t)d[k].planes * rows) * d[k].row_elems * (d[k].elem == BCN_ACTOR_REAL ? esz : 4);
  }
  return actor_up16(off);
}

static int actor_params_desc(const bcn_actor_cfg* c, ActorSegDesc* d) {
  int nd = 0;
  for (int net = 0; net < 2; net++) {
    size_t in = (size_t)c->obs_dim;
    for (int l = 0; l <= c->n_hidden; l++) {
      const size_t out = l < c->n_hidden ? (size_t)c->hidden[l] : (net == 0 ? (size_t)c->act_dim : 1);
      snprintf(d[nd].name, sizeof(d[nd].name), "%s_w%d", net ? "vf" : "pi", l);
      d[nd].elem = BCN_ACTOR_REAL; d[nd].planes = 0; d[nd].row_elems = out * in; nd++;
      snprintf(d[nd].name, sizeof(d[nd].name), "%s_b%d", net ? "vf" : "pi", l);
      d[nd].elem = BCN_ACTOR_REAL; d[nd].planes = 0; d[nd].row_elems = out; nd++;
      in = out;
    }
  }
  snprintf(d[nd].name, sizeof(d[nd].name), "log_std");
  d[nd].elem = BCN_ACTOR_REAL; d[nd].planes = 0; d[nd].row_elems = c->kind == BCN_ACTOR_GAUSSIAN ? (size_t)c->act_dim : 0; nd++;
  return nd;
}

static int actor_state_desc(const bcn_actor_cfg* c, ActorSegDesc* d) {
  const size_t n = (size_t)c->act_dim;
  const bool cat = c->kind == BCN_ACTOR_CATEGORICAL;
  const ActorSegDesc s[6] = {{"counters", BCN_ACTOR_U32, 1, 1}, {"actions", cat ? BCN_ACTOR_I32 : BCN_ACTOR_REAL, 1, cat ? 1 : n},
                             {"raw", BCN_ACTOR_REAL, 1, n}, {"logp", BCN_ACTOR_REAL, 1, 1}, {"value", BCN_ACTOR_REAL, 1, 1},
                             {"dist", BCN_ACTOR_REAL, 1, n}};
  memcpy(d, s, sizeof(s));
  return 6;
}

static int actor_seq_desc(const bcn_actor_cfg* c, int T, ActorSegDesc* d) {
  const ActorSegDesc s[3] = {{"logp_seq", BCN_ACTOR_REAL, T, 1}, {"value_seq", BCN_ACTOR_REAL, T, 1}, {"raw_seq", BCN_ACTOR_REAL, T, (size_t)c->act_dim}};
  memcpy(d, s, sizeof(s));
  return 3;
}

static size_t actor_esz(const bcn_actor_cfg* c) { return c->dtype ? 8 : 4; }

extern "C" {

BCN_ACTOR_API int bcn_actor_params_layout(const bcn_actor_cfg* cfg, bcn_actor_seg* segs, int max_segs) {
  if (!actor_cfg_ok(cfg, false)) return 0;
  ActorSegDesc d[BCN_ACTOR_MAX_SEGS];
  const int nd = actor_params_desc(cfg, d);
  actor_lay(d, nd, 1, actor_esz(cfg), segs, max_segs);
  return nd;
}

BCN_ACTOR_API size_t bcn_actor_params_bytes(const bcn_actor_cfg* cfg) {
  if (!actor_cfg_ok(cfg, false)) return 0;
  ActorSegDesc d[BCN_ACTOR_MAX_SEGS];
  return actor_lay(d, actor_params_desc(cfg, d), 1, actor_esz(cfg), nullptr, 0);
}

BCN_ACTOR_API int bcn_actor_state_layout(const bcn_actor_cfg* cfg, bcn_actor_seg* segs, int max_segs) {
  if (!actor_cfg_ok(cfg, true)) return 0;
  ActorSegDesc d[BCN_ACTOR_MAX_SEGS];
  const int nd = actor_state_desc(cfg, d);
  actor_lay(d, nd, (size_t)cfg->batch, actor_esz(cfg), segs, max_segs);
  return nd;
}

BCN_ACTOR_API size_t bcn_actor_state_bytes(const bcn_actor_cfg* cfg) {
  if (!actor_cfg_ok(cfg, true)) return 0;
  ActorSegDesc d[BCN_ACTOR_MAX_SEGS];
  return actor_lay(d, actor_state_desc(cfg, d), (size_t)cfg->batch, actor_esz(cfg), nullptr, 0);
}

BCN_ACTOR_API int bcn_actor_seq_layout(const bcn_actor_cfg* cfg, int T, bcn_actor_seg* segs, int max_segs) {
  if (!actor_cfg_ok(cfg, true)) return 0;
  if (T < 1) { actor_set_error("T = %d: must be >= 1", T); return 0; }
  ActorSegDesc d[BCN_ACTOR_MAX_SEGS];
  const int nd = actor_seq_desc(cfg, T, d);
  actor_lay(d, nd, (size_t)cfg->batch, actor_esz(cfg), segs, max_segs);
  return nd;
}

BCN_ACTOR_API size_t bcn_actor_seq_bytes(const bcn_actor_cfg* cfg, int T) {
  if (!actor_cfg_ok(cfg, true)) return 0;
  if (T < 1) { actor_set_error("T = %d: must be >= 1", T); return 0; }
  ActorSegDesc d[BCN_ACTOR_MAX_SEGS];
  return actor_lay(d, actor_seq_desc(cfg, T, d), (size_t)cfg->batch, actor_esz(cfg), nullptr, 0);
}

}  // extern "C"

// ---- launches ----------------------------------------------------------------------------
// the part of the argument block that the cfg and the parameter layout decide
template <typename real>
static void actor_fill(const bcn_actor_cfg* c, const void* params, const void* obs, long long n_rows, ActorArgs<real>* a) {
  memset(a, 0, sizeof(*a));
  a->params = static_cast<const real*>(params);
  a->obs = static_cast<const real*>(obs);
  a->n_rows = n_rows;
  a->obs_dim = c->obs_dim; a->n_hidden = c->n_hidden; a->activation = c->activation; a->kind = c->kind; a->act_dim = c->act_dim;
  int hmax = 0;
  for (int l = 0; l < c->n_hidden; l++) { a->hidden[l] = c->hidden[l]; hmax = c->hidden[l] > hmax ? c->hidden[l] : hmax; }
  a->hmax_pad = hmax;
  const int omax = hmax > c->act_dim ? hmax : c->act_dim;
  a->wcols = ((omax + 3) & ~3) + 4;
  a->low = (real)c->low; a->high = (real)c->high;
  bcn_actor_seg s[BCN_ACTOR_MAX_SEGS];
  const int ns = bcn_actor_params_layout(c, s, BCN_ACTOR_MAX_SEGS);
  const int per = 2 * (c->n_hidden + 1);
  for (int l = 0; l <= c->n_hidden; l++) {
    a->pi.w[l] = (unsigned)(s[2 * l].offset / sizeof(real));       a->pi.b[l] = (unsigned)(s[2 * l + 1].offset / sizeof(real));
    a->vf.w[l] = (unsigned)(s[per + 2 * l].offset / sizeof(real)); a->vf.b[l] = (unsigned)(s[per + 2 * l + 1].offset / sizeof(real));
  }
  a->log_std = (unsigned)(s[ns - 1].offset / sizeof(real));
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
  a.seed_lo = (uint32_t)(seed & 0xffffffffull); a.seed_hi = (uint32_t)(seed >> 32);
  a.replica_offset = (long long)replica_offset;
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
  if (e) { actor_set_error("bcn_actor_act: launch -> %s", hipGetErrorString((hipError_t)e)); return BCN_ACTOR_ERR_HIP; }
  return BCN_ACTOR_OK;
}

template <typename real>
static int actor_values_t(const bcn_actor_cfg* c, const void* params, const void* obs, int64_t n_rows, void* out, void* stream) {
  ActorArgs<real> a;
  actor_fill<real>(c, params, obs, (long long)n_rows, &a);
  a.values_only = 1;
  a.value = static_cast<real*>(out);
  const int e = actor_launch<real>(a, stream);
  if (e) { actor_set_error("bcn_actor_values: launch -> %s", hipGetErrorString((hipError_t)e)); return BCN_ACTOR_ERR_HIP; }
  return BCN_ACTOR_OK;
}

extern "C" {

BCN_ACTOR_API int bcn_actor_act(const bcn_actor_cfg* cfg, const void* params_dev, const void* obs_dev, void* state_dev, const uint8_t* mask_dev,
                                uint64_t seed, int64_t replica_offset, int deterministic, const int32_t* cursor_dev, int T, void* seq_dev,
                                void* stream) {
  if (!actor_cfg_ok(cfg, true)) return BCN_ACTOR_ERR_ARG;
  if (!params_dev || !obs_dev || !state_dev) { actor_set_error("bcn_actor_act: params_dev, obs_dev and state_dev must not be NULL"); return BCN_ACTOR_ERR_ARG; }
  if (cursor_dev && (T < 1 || !seq_dev)) { actor_set_error("bcn_actor_act: a cursor needs T >= 1 and seq_dev"); return BCN_ACTOR_ERR_ARG; }
  return cfg->dtype ? actor_act_t<double>(cfg, params_dev, obs_dev, state_dev, mask_dev, seed, replica_offset, deterministic, cursor_dev, T, seq_dev, stream)
                    : actor_act_t<float>(cfg, params_dev, obs_dev, state_dev, mask_dev, seed, replica_offset, deterministic, cursor_dev, T, seq_dev, stream);
}

BCN_ACTOR_API int bcn_actor_values(const bcn_actor_cfg* cfg, const void* params_dev, const void* obs_dev, int64_t n_rows, void* out_dev,
                                   void* stream) {
  if (!actor_cfg_ok(cfg, false)) return BCN_ACTOR_ERR_ARG;
  if (!params_dev || !obs_dev || !out_dev) { actor_set_error("bcn_actor_values: params_dev, obs_dev and out_dev must not be NULL"); return BCN_ACTOR_ERR_ARG; }
  if (n_rows < 1 || n_rows > 0x7fffffffll * 32) { actor_set_error("bcn_actor_values: n_rows = %lld is outside what one launch covers", (long long)n_rows); return BCN_ACTOR_ERR_ARG; }
  return cfg->dtype ? actor_values_t<double>(cfg, params_dev, obs_dev, n_rows, out_dev, stream)
                    : actor_values_t<float>(cfg, params_dev, obs_dev, n_rows, out_dev, stream);
}

}  // extern "C"
