// dqn.hip -- libbeacon_dqn.so (include/beacon_dqn.h): the C ABI, the layouts, the argument checks, and the float32 instantiation of
// the kernels of dqn_impl.h.  The float64 instantiation is dqn_f64.hip (built without FMA contraction).
#include <math.h>

#include "dqn_impl.h"

DQN_DEFINE_LAUNCH(float)

static thread_local PolicyErr g_dqn_err;

// ---- cfg, layouts ------------------------------------------------------------------------------------------------------------
static int dqn_hmax(const bcn_dqn_cfg* c) {
  int hmax = 0;
  for (int l = 0; l < c->n_hidden; l++) hmax = c->hidden[l] > hmax ? c->hidden[l] : hmax;
  return hmax;
}

static int dqn_rows(const bcn_dqn_cfg* c) { return c->n_actions + (c->dueling ? 1 : 0); }

static int dqn_wcols(const bcn_dqn_cfg* c) {
  const int hmax = dqn_hmax(c);
  const int omax = hmax > dqn_rows(c) ? hmax : dqn_rows(c);
  return ((omax + 3) & ~3) + 4;
}

static size_t dqn_lds_of(const bcn_dqn_cfg* c) {
  return c->dtype ? td3_lds_bytes<double>(c->n_hidden, dqn_hmax(c), dqn_wcols(c)) : td3_lds_bytes<float>(c->n_hidden, dqn_hmax(c), dqn_wcols(c));
}

static bool dqn_cfg_ok(const bcn_dqn_cfg* c, bool need_batch) {
  PolicyErr* err = &g_dqn_err;
  if (!c) { err->set("cfg is NULL"); return false; }
  if (need_batch && c->batch < 1) { err->set("cfg.batch = %d: must be >= 1", c->batch); return false; }
  if (c->dueling != 0 && c->dueling != 1) { err->set("cfg.dueling = %d: must be 0 or 1", c->dueling); return false; }
  if (c->n_actions < 2 || c->n_actions + c->dueling > BCN_DQN_MAX_ACTIONS) {
    err->set("cfg.n_actions = %d, cfg.dueling = %d: need n_actions >= 2 and n_actions + dueling <= %d (the head's rows)", c->n_actions, c->dueling,
             BCN_DQN_MAX_ACTIONS);
    return false;
  }
  if (c->obs_dim < 1 || c->obs_dim > BCN_DQN_MAX_OBS) { err->set("cfg.obs_dim = %d: must lie in 1 .. %d", c->obs_dim, BCN_DQN_MAX_OBS); return false; }
  if (c->dtype != 0 && c->dtype != 1) { err->set("cfg.dtype = %d: must be 0 (float32) or 1 (float64)", c->dtype); return false; }
  if (c->n_hidden < 1 || c->n_hidden > BCN_ACTOR_MAX_LAYERS) { err->set("cfg.n_hidden = %d: must lie in 1 .. %d", c->n_hidden, BCN_ACTOR_MAX_LAYERS); return false; }
  for (int l = 0; l < c->n_hidden; l++)
    if (c->hidden[l] < 1 || c->hidden[l] > BCN_ACTOR_MAX_HIDDEN) {
      err->set("cfg.hidden[%d] = %d: must lie in 1 .. %d", l, c->hidden[l], BCN_ACTOR_MAX_HIDDEN);
      return false;
    }
  if (c->activation != BCN_ACTOR_TANH && c->activation != BCN_ACTOR_RELU) { err->set("cfg.activation = %d: must be 0 (tanh) or 1 (relu)", c->activation); return false; }
  const size_t lds = dqn_lds_of(c);
  if (lds > (size_t)DQN_LDS_LIMIT) {
    err->set("cfg: the tile kernels need %zu bytes of LDS for these widths, the device has %d", lds, DQN_LDS_LIMIT);
    return false;
  }
  return true;
}

static size_t dqn_esz(const bcn_dqn_cfg* c) { return c->dtype ? 8 : 4; }

struct DqnSegDesc { char name[16]; int elem; size_t n; };

static size_t dqn_lay(const DqnSegDesc* d, int nd, size_t esz, bcn_dqn_seg* segs, int max_segs) {
  size_t off = 0;
  for (int k = 0; k < nd; k++) {
    off = (off + 15) & ~(size_t)15;
    if (segs && k < max_segs) {
      memset(&segs[k], 0, sizeof(segs[k]));
      strncpy(segs[k].name, d[k].name, sizeof(segs[k].name) - 1);
      segs[k].offset = off; segs[k].elem = d[k].elem; segs[k].planes = 0; segs[k].row_elems = (int64_t)d[k].n;
    }
    off += d[k].n * (d[k].elem == BCN_DQN_REAL ? esz : d[k].elem == BCN_DQN_F64 ? 8 : d[k].elem == BCN_DQN_U8 ? 1 : 4);
  }
  return (off + 15) & ~(size_t)15;
}

static void dqn_desc(DqnSegDesc* d, const char* name, int elem, size_t n) {
  memset(d, 0, sizeof(*d));
  strncpy(d->name, name, sizeof(d->name) - 1);
  d->elem = elem; d->n = n;
}

static int dqn_params_lay(const bcn_dqn_cfg* c, bcn_dqn_seg* segs, int max_segs, size_t* bytes) {
  DqnSegDesc d[BCN_DQN_MAX_SEGS];
  int nd = 0;
  size_t in = (size_t)c->obs_dim;
  for (int l = 0; l <= c->n_hidden; l++) {
    const size_t out = l < c->n_hidden ? (size_t)c->hidden[l] : (size_t)dqn_rows(c);
    char name[16];
    snprintf(name, sizeof(name), "q_w%d", l);
    dqn_desc(&d[nd++], name, BCN_DQN_REAL, out * in);
    snprintf(name, sizeof(name), "q_b%d", l);
    dqn_desc(&d[nd++], name, BCN_DQN_REAL, out);
    in = out;
  }
  *bytes = dqn_lay(d, nd, dqn_esz(c), segs, max_segs);
  return nd;
}

static size_t dqn_n_elems(const bcn_dqn_cfg* c) {
  size_t bytes;
  dqn_params_lay(c, nullptr, 0, &bytes);
  return bytes / dqn_esz(c);
}

static int dqn_grid_of(const bcn_dqn_cfg* c) {
  const size_t slab = dqn_n_elems(c) * dqn_esz(c);
  size_t g = ((size_t)64 << 20) / slab;
  g = g < 8 ? 8 : g;
  return (int)(g > BCN_DQN_MAX_GRID ? BCN_DQN_MAX_GRID : g);
}

static int dqn_state_lay(const bcn_dqn_cfg* c, bcn_dqn_seg* segs, int max_segs, size_t* bytes) {
  DqnSegDesc d[5];
  const size_t n = dqn_n_elems(c);
  dqn_desc(&d[0], "counters", BCN_DQN_U32, (size_t)c->batch);
  dqn_desc(&d[1], "step", BCN_DQN_I32, 4);
  dqn_desc(&d[2], "stats", BCN_DQN_F64, BCN_DQN_N_STATS);
  dqn_desc(&d[3], "adam_m", BCN_DQN_REAL, n);
  dqn_desc(&d[4], "adam_v", BCN_DQN_REAL, n);
  *bytes = dqn_lay(d, 5, dqn_esz(c), segs, max_segs);
  return 5;
}

static int dqn_work_lay(const bcn_dqn_cfg* c, bcn_dqn_seg* segs, int max_segs, size_t* bytes) {
  DqnSegDesc d[4];
  const size_t n = dqn_n_elems(c);
  dqn_desc(&d[0], "grad", BCN_DQN_REAL, n);
  dqn_desc(&d[1], "wg_stats", BCN_DQN_F64, (size_t)BCN_DQN_MAX_GRID * BCN_DQN_N_STATS);
  dqn_desc(&d[2], "norm2", BCN_DQN_F64, (n + TD3_NT - 1) / TD3_NT);
  dqn_desc(&d[3], "slabs", BCN_DQN_REAL, (size_t)dqn_grid_of(c) * n);
  *bytes = dqn_lay(d, 4, dqn_esz(c), segs, max_segs);
  return 4;
}

// ---- the argument block --------------------------------------------------------------------------------------------------------
template <typename real>
static void dqn_fill_cfg(const bcn_dqn_cfg* c, DqnArgs<real>* S) {
  memset(S, 0, sizeof(*S));
  Td3Args<real>* a = &S->t;
  a->obs_dim = c->obs_dim; a->act_dim = c->n_actions; a->D = c->obs_dim; a->n_hidden = c->n_hidden;
  a->activation = c->activation; a->n_critics = 1;
  for (int l = 0; l < c->n_hidden; l++) a->hidden[l] = c->hidden[l];
  a->hmax_pad = dqn_hmax(c);
  a->wcols = dqn_wcols(c);
  S->n_head = dqn_rows(c); S->dueling = c->dueling ? 1 : 0;
  S->inv_n = real(1) / real(c->n_actions);
  bcn_dqn_seg s[BCN_DQN_MAX_SEGS];
  size_t bytes;
  dqn_params_lay(c, s, BCN_DQN_MAX_SEGS, &bytes);
  for (int l = 0; l <= c->n_hidden; l++) {
    a->mu.w[l] = (unsigned)(s[2 * l].offset / sizeof(real));
    a->mu.b[l] = (unsigned)(s[2 * l + 1].offset / sizeof(real));
  }
}

struct DqnWork { char *grad, *wg_stats, *norm2, *slabs; };
static DqnWork dqn_work_of(const bcn_dqn_cfg* c, void* work) {
  bcn_dqn_seg s[4];
  size_t bytes;
  dqn_work_lay(c, s, 4, &bytes);
  char* p = static_cast<char*>(work);
  return DqnWork{p + s[0].offset, p + s[1].offset, p + s[2].offset, p + s[3].offset};
}

struct DqnState { char *counters, *step, *stats, *m, *v; };
static DqnState dqn_state_of(const bcn_dqn_cfg* c, void* state) {
  bcn_dqn_seg s[5];
  size_t bytes;
  dqn_state_lay(c, s, 5, &bytes);
  char* p = static_cast<char*>(state);
  return DqnState{p + s[0].offset, p + s[1].offset, p + s[2].offset, p + s[3].offset, p + s[4].offset};
}

template <typename real>
static int dqn_act_t(const bcn_dqn_cfg* c, const void* params, const void* obs, long long n_rows, const uint8_t* mask, void* state, int32_t* actions,
                     void* q_out, int mode, double eps, const void* eps_dev, uint64_t seed, int64_t replica_offset, void* stream) {
  constexpr int TB = ActorGeom<real>::TB;
  DqnArgs<real> S;
  dqn_fill_cfg<real>(c, &S);
  Td3Args<real>& a = S.t;
  a.params = static_cast<const real*>(params);
  a.obs = static_cast<const real*>(obs); a.n_rows = n_rows; a.mask = mask;
  a.counters = state ? reinterpret_cast<uint32_t*>(dqn_state_of(c, state).counters) : nullptr;
  a.mode = mode;
  S.actions_i = actions; S.q_out = static_cast<real*>(q_out);
  S.eps = (real)eps; S.eps_dev = static_cast<const real*>(eps_dev);
  a.seed_lo = (uint32_t)(seed & 0xffffffffull); a.seed_hi = (uint32_t)(seed >> 32); a.replica_offset = replica_offset;
  return dqn_launch_tile<real>(DQN_K_ACT, S, (int)((n_rows + TB - 1) / TB), stream);
}

template <typename real>
static int dqn_grad_t(const bcn_dqn_cfg* c, const bcn_dqn_batch* b, void* stream) {
  constexpr int TB = ActorGeom<real>::TB;
  DqnArgs<real> S;
  dqn_fill_cfg<real>(c, &S);
  Td3Args<real>& a = S.t;
  a.m_obs = static_cast<const real*>(b->obs_dev); a.m_act = static_cast<const real*>(b->act_dev);
  a.m_rwd = static_cast<const real*>(b->rwd_dev); a.m_next = static_cast<const real*>(b->next_obs_dev);
  a.m_boot = b->boot_dev; a.m_live = b->live_dev; a.capacity = b->capacity;
  const DqnWork w = dqn_work_of(c, b->work_dev);
  const DqnState s = dqn_state_of(c, b->state_dev);
  a.params = static_cast<const real*>(b->params_dev); a.target = static_cast<const real*>(b->target_dev);
  a.idx = b->idx_dev; a.m = b->m; a.tiles = (b->m + TB - 1) / TB;
  a.gamma = (real)b->gamma;
  S.huber = b->huber > 0.0 ? (real)b->huber : real(0);
  S.double_q = b->double_q ? 1 : 0;
  a.slabs = reinterpret_cast<real*>(w.slabs); a.slab_elems = dqn_n_elems(c); a.wg_stats = reinterpret_cast<double*>(w.wg_stats);
  const int gmax = dqn_grid_of(c);
  const int grid = a.tiles < gmax ? (int)a.tiles : gmax;
  const int e = dqn_launch_tile<real>(DQN_K_Q, S, grid, stream);
  if (e) return e;
  Td3ReduceArgs<real> r;
  memset(&r, 0, sizeof(r));
  r.slabs = a.slabs; r.slab_elems = a.slab_elems; r.used = grid; r.wg_stats = a.wg_stats; r.grad = reinterpret_cast<real*>(w.grad);
  r.e0 = 0; r.e1 = (int)a.slab_elems;
  r.norm2 = reinterpret_cast<double*>(w.norm2); r.stats = reinterpret_cast<double*>(s.stats); r.which = 0;
  return dqn_launch_reduce<real>(r, (r.e1 - r.e0 + TD3_NT - 1) / TD3_NT, r.stats + BCN_DQN_STAT_GRAD_NORM, stream);
}

// the double launches live in dqn_f64.hip
template <> int dqn_launch_tile<double>(int kernel, const DqnArgs<double>& a, int grid, void* stream);
template <> int dqn_launch_reduce<double>(const Td3ReduceArgs<double>& r, int blocks, double* norm_out, void* stream);
template <> int dqn_launch_adam<double>(const Td3AdamArgs<double>& a, void* stream);
template <> int dqn_launch_polyak<double>(const double* params, double* target, int n, double tau, void* stream);
template <> int dqn_launch_append<double>(const DqnReplayArgs<double>& a, void* stream);

template <typename real>
static int dqn_adam_t(const bcn_dqn_cfg* c, void* params, void* work, void* state, const bcn_dqn_adam_hyper* h, void* stream) {
  const DqnWork w = dqn_work_of(c, work);
  const DqnState s = dqn_state_of(c, state);
  Td3AdamArgs<real> a;
  memset(&a, 0, sizeof(a));
  a.params = static_cast<real*>(params); a.grad = reinterpret_cast<const real*>(w.grad);
  a.m = reinterpret_cast<real*>(s.m); a.v = reinterpret_cast<real*>(s.v); a.step = reinterpret_cast<int32_t*>(s.step);
  a.norm = reinterpret_cast<const double*>(s.stats) + BCN_DQN_STAT_GRAD_NORM;
  a.e0 = 0; a.e1 = (int)dqn_n_elems(c); a.which = 0;
  a.lr = h->lr; a.beta1 = h->beta1; a.beta2 = h->beta2; a.eps = h->eps; a.max_grad_norm = h->max_grad_norm;
  return dqn_launch_adam<real>(a, stream);
}

template <typename real>
static int dqn_append_t(const bcn_dqn_cfg* c, int64_t capacity, int32_t* head, void* obs, void* act, void* rwd, void* next, uint8_t* boot, uint8_t* live,
                        int T, const void* r_obs, const int32_t* r_act, const void* r_rwd, const uint8_t* r_done, const uint8_t* r_trunc,
                        const uint8_t* r_valid, const void* r_final, const int32_t* r_cursor, void* stream) {
  DqnReplayArgs<real> S;
  memset(&S, 0, sizeof(S));
  ReplayArgs<real>& a = S.r;
  a.head = head; a.obs = static_cast<real*>(obs); a.act = static_cast<real*>(act); a.rwd = static_cast<real*>(rwd); a.next = static_cast<real*>(next);
  a.boot = boot; a.live = live; a.C = capacity; a.T = T; a.B = c->batch; a.od = c->obs_dim; a.ad = 1;
  a.r_obs = static_cast<const real*>(r_obs); a.r_act = nullptr; a.r_rwd = static_cast<const real*>(r_rwd); a.r_final = static_cast<const real*>(r_final);
  a.r_done = r_done; a.r_trunc = r_trunc; a.r_valid = r_valid; a.cursor = r_cursor;
  S.r_act_i = r_act;
  return dqn_launch_append<real>(S, stream);
}

static int dqn_hip(const char* fn, int e) {
  if (e) { g_dqn_err.set("%s: launch -> %s", fn, hipGetErrorString((hipError_t)e)); return BCN_DQN_ERR_HIP; }
  return BCN_DQN_OK;
}

extern "C" {

BCN_DQN_API const char* bcn_dqn_last_error(void) { return g_dqn_err.text; }

BCN_DQN_API int bcn_dqn_params_layout(const bcn_dqn_cfg* cfg, bcn_dqn_seg* segs, int max_segs) {
  size_t bytes;
  return dqn_cfg_ok(cfg, false) ? dqn_params_lay(cfg, segs, max_segs, &bytes) : 0;
}
BCN_DQN_API size_t bcn_dqn_params_bytes(const bcn_dqn_cfg* cfg) {
  size_t bytes = 0;
  if (dqn_cfg_ok(cfg, false)) dqn_params_lay(cfg, nullptr, 0, &bytes);
  return bytes;
}
BCN_DQN_API int bcn_dqn_state_layout(const bcn_dqn_cfg* cfg, bcn_dqn_seg* segs, int max_segs) {
  size_t bytes;
  return dqn_cfg_ok(cfg, true) ? dqn_state_lay(cfg, segs, max_segs, &bytes) : 0;
}
BCN_DQN_API size_t bcn_dqn_state_bytes(const bcn_dqn_cfg* cfg) {
  size_t bytes = 0;
  if (dqn_cfg_ok(cfg, true)) dqn_state_lay(cfg, nullptr, 0, &bytes);
  return bytes;
}
BCN_DQN_API int bcn_dqn_work_layout(const bcn_dqn_cfg* cfg, bcn_dqn_seg* segs, int max_segs) {
  size_t bytes;
  return dqn_cfg_ok(cfg, false) ? dqn_work_lay(cfg, segs, max_segs, &bytes) : 0;
}
BCN_DQN_API size_t bcn_dqn_work_bytes(const bcn_dqn_cfg* cfg) {
  size_t bytes = 0;
  if (dqn_cfg_ok(cfg, false)) dqn_work_lay(cfg, nullptr, 0, &bytes);
  return bytes;
}
BCN_DQN_API int bcn_dqn_grid(const bcn_dqn_cfg* cfg) { return dqn_cfg_ok(cfg, false) ? dqn_grid_of(cfg) : 0; }
BCN_DQN_API size_t bcn_dqn_lds_bytes(const bcn_dqn_cfg* cfg) { return dqn_cfg_ok(cfg, false) ? dqn_lds_of(cfg) : 0; }

BCN_DQN_API int bcn_dqn_act(const bcn_dqn_cfg* cfg, const void* params_dev, const void* obs_dev, const uint8_t* mask_dev, void* state_dev,
                            int32_t* actions_dev, int mode, double eps, const void* eps_dev, uint64_t seed, int64_t replica_offset,
                            void* stream) {
  if (!dqn_cfg_ok(cfg, true)) return BCN_DQN_ERR_ARG;
  if (!params_dev) { g_dqn_err.set("bcn_dqn_act: params_dev is NULL"); return BCN_DQN_ERR_ARG; }
  if (!obs_dev) { g_dqn_err.set("bcn_dqn_act: obs_dev is NULL"); return BCN_DQN_ERR_ARG; }
  if (!state_dev) { g_dqn_err.set("bcn_dqn_act: state_dev is NULL"); return BCN_DQN_ERR_ARG; }
  if (!actions_dev) { g_dqn_err.set("bcn_dqn_act: actions_dev is NULL"); return BCN_DQN_ERR_ARG; }
  if (mode < BCN_DQN_GREEDY || mode > BCN_DQN_UNIFORM) { g_dqn_err.set("bcn_dqn_act: mode = %d: must be 0 (greedy), 1 (epsilon) or 2 (uniform)", mode); return BCN_DQN_ERR_ARG; }
  if (!eps_dev && !(eps >= 0.0 && eps <= 1.0)) { g_dqn_err.set("bcn_dqn_act: eps = %g: must lie in [0, 1]", eps); return BCN_DQN_ERR_ARG; }
  if (replica_offset < 0) { g_dqn_err.set("bcn_dqn_act: replica_offset = %lld: must be >= 0", (long long)replica_offset); return BCN_DQN_ERR_ARG; }
  return dqn_hip("bcn_dqn_act", cfg->dtype ? dqn_act_t<double>(cfg, params_dev, obs_dev, cfg->batch, mask_dev, state_dev, actions_dev, nullptr, mode, eps, eps_dev, seed, replica_offset, stream)
                                           : dqn_act_t<float>(cfg, params_dev, obs_dev, cfg->batch, mask_dev, state_dev, actions_dev, nullptr, mode, eps, eps_dev, seed, replica_offset, stream));
}

BCN_DQN_API int bcn_dqn_q(const bcn_dqn_cfg* cfg, const void* params_dev, const void* rows_dev, int64_t n_rows, void* q_dev, void* stream) {
  if (!dqn_cfg_ok(cfg, false)) return BCN_DQN_ERR_ARG;
  if (!params_dev) { g_dqn_err.set("bcn_dqn_q: params_dev is NULL"); return BCN_DQN_ERR_ARG; }
  if (!rows_dev) { g_dqn_err.set("bcn_dqn_q: rows_dev is NULL"); return BCN_DQN_ERR_ARG; }
  if (!q_dev) { g_dqn_err.set("bcn_dqn_q: q_dev is NULL"); return BCN_DQN_ERR_ARG; }
  if (n_rows < 1 || n_rows > 0x7fffffffll) { g_dqn_err.set("bcn_dqn_q: n_rows = %lld: must lie in 1 .. 2^31 - 1", (long long)n_rows); return BCN_DQN_ERR_ARG; }
  return dqn_hip("bcn_dqn_q", cfg->dtype ? dqn_act_t<double>(cfg, params_dev, rows_dev, n_rows, nullptr, nullptr, nullptr, q_dev, BCN_DQN_GREEDY, 0.0, nullptr, 0, 0, stream)
                                         : dqn_act_t<float>(cfg, params_dev, rows_dev, n_rows, nullptr, nullptr, nullptr, q_dev, BCN_DQN_GREEDY, 0.0, nullptr, 0, 0, stream));
}

BCN_DQN_API int bcn_dqn_append(const bcn_dqn_cfg* cfg, int64_t capacity, int32_t* head_dev, void* obs_dev, void* act_dev, void* rwd_dev,
                               void* next_obs_dev, uint8_t* boot_dev, uint8_t* live_dev, int T, const void* ro_obs_dev,
                               const int32_t* ro_act_dev, const void* ro_rwd_dev, const uint8_t* ro_done_dev, const uint8_t* ro_trunc_dev,
                               const uint8_t* ro_valid_dev, const void* ro_final_obs_dev, const int32_t* ro_cursor_dev, void* stream) {
  if (!dqn_cfg_ok(cfg, true)) return BCN_DQN_ERR_ARG;
  if (capacity < 1 || capacity > 0x7fffffffll) { g_dqn_err.set("bcn_dqn_append: capacity = %lld: must lie in 1 .. 2^31 - 1", (long long)capacity); return BCN_DQN_ERR_ARG; }
  if (T < 1 || (long long)T * cfg->batch > capacity) {
    g_dqn_err.set("bcn_dqn_append: T = %d steps of %d replicas: need T >= 1 and T B <= capacity = %lld", T, cfg->batch, (long long)capacity);
    return BCN_DQN_ERR_ARG;
  }
  const void* ptrs[15] = {head_dev, obs_dev, act_dev, rwd_dev, next_obs_dev, boot_dev, live_dev, ro_obs_dev, ro_act_dev, ro_rwd_dev, ro_done_dev,
                          ro_trunc_dev, ro_valid_dev, ro_final_obs_dev, ro_cursor_dev};
  const char* names[15] = {"head_dev", "obs_dev", "act_dev", "rwd_dev", "next_obs_dev", "boot_dev", "live_dev", "ro_obs_dev", "ro_act_dev", "ro_rwd_dev",
                           "ro_done_dev", "ro_trunc_dev", "ro_valid_dev", "ro_final_obs_dev", "ro_cursor_dev"};
  for (int k = 0; k < 15; k++)
    if (!ptrs[k]) { g_dqn_err.set("bcn_dqn_append: %s is NULL", names[k]); return BCN_DQN_ERR_ARG; }
  return dqn_hip("bcn_dqn_append",
                 cfg->dtype ? dqn_append_t<double>(cfg, capacity, head_dev, obs_dev, act_dev, rwd_dev, next_obs_dev, boot_dev, live_dev, T, ro_obs_dev, ro_act_dev,
                                                   ro_rwd_dev, ro_done_dev, ro_trunc_dev, ro_valid_dev, ro_final_obs_dev, ro_cursor_dev, stream)
                            : dqn_append_t<float>(cfg, capacity, head_dev, obs_dev, act_dev, rwd_dev, next_obs_dev, boot_dev, live_dev, T, ro_obs_dev, ro_act_dev,
                                                  ro_rwd_dev, ro_done_dev, ro_trunc_dev, ro_valid_dev, ro_final_obs_dev, ro_cursor_dev, stream));
}

BCN_DQN_API int bcn_dqn_grad(const bcn_dqn_cfg* cfg, const bcn_dqn_batch* b, void* stream) {
  const char* fn = "bcn_dqn_grad";
  if (!dqn_cfg_ok(cfg, true)) return BCN_DQN_ERR_ARG;
  if (!b) { g_dqn_err.set("%s: batch is NULL", fn); return BCN_DQN_ERR_ARG; }
  if (!b->params_dev) { g_dqn_err.set("%s: batch.params_dev is NULL", fn); return BCN_DQN_ERR_ARG; }
  if (!b->target_dev) { g_dqn_err.set("%s: batch.target_dev is NULL", fn); return BCN_DQN_ERR_ARG; }
  const void* mem[6] = {b->obs_dev, b->act_dev, b->rwd_dev, b->next_obs_dev, b->boot_dev, b->live_dev};
  const char* names[6] = {"obs_dev", "act_dev", "rwd_dev", "next_obs_dev", "boot_dev", "live_dev"};
  for (int k = 0; k < 6; k++)
    if (!mem[k]) { g_dqn_err.set("%s: batch.%s is NULL (a segment of the replay memory)", fn, names[k]); return BCN_DQN_ERR_ARG; }
  if (!b->idx_dev) { g_dqn_err.set("%s: batch.idx_dev is NULL", fn); return BCN_DQN_ERR_ARG; }
  if (!b->work_dev) { g_dqn_err.set("%s: batch.work_dev is NULL", fn); return BCN_DQN_ERR_ARG; }
  if (!b->state_dev) { g_dqn_err.set("%s: batch.state_dev is NULL", fn); return BCN_DQN_ERR_ARG; }
  if (b->m < 1 || b->m > 0x7fffffffll) { g_dqn_err.set("%s: m = %lld: must lie in 1 .. 2^31 - 1", fn, (long long)b->m); return BCN_DQN_ERR_ARG; }
  if (b->capacity < 1 || b->capacity > 0x7fffffffll) { g_dqn_err.set("%s: batch.capacity = %lld: must lie in 1 .. 2^31 - 1", fn, (long long)b->capacity); return BCN_DQN_ERR_ARG; }
  if (!(b->gamma >= 0.0 && b->gamma <= 1.0)) { g_dqn_err.set("%s: batch.gamma = %g: must lie in [0, 1]", fn, b->gamma); return BCN_DQN_ERR_ARG; }
  if (!isfinite(b->huber)) { g_dqn_err.set("%s: batch.huber = %g: must be finite (<= 0: the squared loss)", fn, b->huber); return BCN_DQN_ERR_ARG; }
  if (b->double_q != 0 && b->double_q != 1) { g_dqn_err.set("%s: batch.double_q = %d: must be 0 or 1", fn, b->double_q); return BCN_DQN_ERR_ARG; }
  return dqn_hip(fn, cfg->dtype ? dqn_grad_t<double>(cfg, b, stream) : dqn_grad_t<float>(cfg, b, stream));
}

BCN_DQN_API int bcn_dqn_adam(const bcn_dqn_cfg* cfg, void* params_dev, void* work_dev, void* state_dev, const bcn_dqn_adam_hyper* h, void* stream) {
  if (!dqn_cfg_ok(cfg, true)) return BCN_DQN_ERR_ARG;
  if (!params_dev || !work_dev || !state_dev || !h) { g_dqn_err.set("bcn_dqn_adam: params_dev, work_dev, state_dev or hyper is NULL"); return BCN_DQN_ERR_ARG; }
  if (!(h->lr >= 0.0)) { g_dqn_err.set("bcn_dqn_adam: hyper.lr = %g: must be >= 0", h->lr); return BCN_DQN_ERR_ARG; }
  if (!(h->beta1 >= 0.0 && h->beta1 < 1.0) || !(h->beta2 >= 0.0 && h->beta2 < 1.0)) {
    g_dqn_err.set("bcn_dqn_adam: hyper.beta1 = %g, hyper.beta2 = %g: must lie in [0, 1)", h->beta1, h->beta2);
    return BCN_DQN_ERR_ARG;
  }
  if (!(h->eps >= 0.0)) { g_dqn_err.set("bcn_dqn_adam: hyper.eps = %g: must be >= 0", h->eps); return BCN_DQN_ERR_ARG; }
  return dqn_hip("bcn_dqn_adam", cfg->dtype ? dqn_adam_t<double>(cfg, params_dev, work_dev, state_dev, h, stream)
                                            : dqn_adam_t<float>(cfg, params_dev, work_dev, state_dev, h, stream));
}

BCN_DQN_API int bcn_dqn_polyak(const bcn_dqn_cfg* cfg, const void* params_dev, void* target_dev, double tau, void* stream) {
  if (!dqn_cfg_ok(cfg, false)) return BCN_DQN_ERR_ARG;
  if (!params_dev || !target_dev) { g_dqn_err.set("bcn_dqn_polyak: params_dev or target_dev is NULL"); return BCN_DQN_ERR_ARG; }
  if (!(tau >= 0.0 && tau <= 1.0)) { g_dqn_err.set("bcn_dqn_polyak: tau = %g: must lie in [0, 1]", tau); return BCN_DQN_ERR_ARG; }
  const int n = (int)dqn_n_elems(cfg);
  return dqn_hip("bcn_dqn_polyak", cfg->dtype ? dqn_launch_polyak<double>(static_cast<const double*>(params_dev), static_cast<double*>(target_dev), n, tau, stream)
                                              : dqn_launch_polyak<float>(static_cast<const float*>(params_dev), static_cast<float*>(target_dev), n, (float)tau, stream));
}

}  // extern "C"
