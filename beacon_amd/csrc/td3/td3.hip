// td3.hip -- libbeacon_td3.so (include/beacon_td3.h): the C ABI, the layouts, the argument checks, and the float32 instantiation of
// the kernels of td3_impl.h.  The float64 instantiation is td3_f64.hip (built without FMA contraction).
#include "td3_impl.h"

TD3_DEFINE_LAUNCH(float)

static thread_local PolicyErr g_td3_err;

// ---- cfg, layouts ------------------------------------------------------------------------------------------------------------
static bool td3_cfg_ok(const bcn_td3_cfg* c, bool need_batch) {
  PolicyErr* err = &g_td3_err;
  if (!c) { err->set("cfg is NULL"); return false; }
  if (need_batch && c->batch < 1) { err->set("cfg.batch = %d: must be >= 1", c->batch); return false; }
  if (c->act_dim < 1 || c->act_dim > BCN_ACTOR_MAX_ACT) { err->set("cfg.act_dim = %d: must lie in 1 .. %d", c->act_dim, BCN_ACTOR_MAX_ACT); return false; }
  if (c->obs_dim < 1 || (long long)c->obs_dim + c->act_dim > BCN_TD3_MAX_IN) {
    err->set("cfg.obs_dim = %d, cfg.act_dim = %d: need obs_dim >= 1 and obs_dim + act_dim <= %d (a critic's input row)", c->obs_dim, c->act_dim, BCN_TD3_MAX_IN);
    return false;
  }
  if (c->dtype != 0 && c->dtype != 1) { err->set("cfg.dtype = %d: must be 0 (float32) or 1 (float64)", c->dtype); return false; }
  if (c->n_hidden < 1 || c->n_hidden > BCN_ACTOR_MAX_LAYERS) { err->set("cfg.n_hidden = %d: must lie in 1 .. %d", c->n_hidden, BCN_ACTOR_MAX_LAYERS); return false; }
  for (int l = 0; l < c->n_hidden; l++)
    if (c->hidden[l] < 1 || c->hidden[l] > BCN_ACTOR_MAX_HIDDEN) {
      err->set("cfg.hidden[%d] = %d: must lie in 1 .. %d", l, c->hidden[l], BCN_ACTOR_MAX_HIDDEN);
      return false;
    }
  if (c->activation != BCN_ACTOR_TANH && c->activation != BCN_ACTOR_RELU) { err->set("cfg.activation = %d: must be 0 (tanh) or 1 (relu)", c->activation); return false; }
  if (!(c->low <= c->high)) { err->set("cfg.low = %g, cfg.high = %g: need low <= high", c->low, c->high); return false; }
  if (c->n_critics != 1 && c->n_critics != 2) { err->set("cfg.n_critics = %d: must be 1 or 2", c->n_critics); return false; }
  return true;
}

static size_t td3_esz(const bcn_td3_cfg* c) { return c->dtype ? 8 : 4; }

struct Td3SegDesc { char name[16]; int elem; size_t n; };

static size_t td3_lay(const Td3SegDesc* d, int nd, size_t esz, bcn_td3_seg* segs, int max_segs) {
  size_t off = 0;
  for (int k = 0; k < nd; k++) {
    off = (off + 15) & ~(size_t)15;
    if (segs && k < max_segs) {
      memset(&segs[k], 0, sizeof(segs[k]));
      strncpy(segs[k].name, d[k].name, sizeof(segs[k].name) - 1);
      segs[k].offset = off; segs[k].elem = d[k].elem; segs[k].planes = 0; segs[k].row_elems = (int64_t)d[k].n;
    }
    off += d[k].n * (d[k].elem == BCN_TD3_REAL ? esz : d[k].elem == BCN_TD3_F64 ? 8 : d[k].elem == BCN_TD3_U8 ? 1 : 4);
  }
  return (off + 15) & ~(size_t)15;
}

static void td3_desc(Td3SegDesc* d, const char* name, int elem, size_t n) {
  memset(d, 0, sizeof(*d));
  strncpy(d->name, name, sizeof(d->name) - 1);
  d->elem = elem; d->n = n;
}

static int td3_params_lay(const bcn_td3_cfg* c, bcn_td3_seg* segs, int max_segs, size_t* bytes) {
  Td3SegDesc d[BCN_TD3_MAX_SEGS];
  int nd = 0;
  for (int net = 0; net <= c->n_critics; net++) {
    size_t in = net == 0 ? (size_t)c->obs_dim : (size_t)c->obs_dim + c->act_dim;
    for (int l = 0; l <= c->n_hidden; l++) {
      const size_t out = l < c->n_hidden ? (size_t)c->hidden[l] : (net == 0 ? (size_t)c->act_dim : 1);
      char name[16];
      snprintf(name, sizeof(name), "%s_w%d", net == 0 ? "mu" : (net == 1 ? "q1" : "q2"), l);
      td3_desc(&d[nd++], name, BCN_TD3_REAL, out * in);
      snprintf(name, sizeof(name), "%s_b%d", net == 0 ? "mu" : (net == 1 ? "q1" : "q2"), l);
      td3_desc(&d[nd++], name, BCN_TD3_REAL, out);
      in = out;
    }
  }
  *bytes = td3_lay(d, nd, td3_esz(c), segs, max_segs);
  return nd;
}

static size_t td3_n_elems(const bcn_td3_cfg* c) {
  size_t bytes;
  td3_params_lay(c, nullptr, 0, &bytes);
  return bytes / td3_esz(c);
}

static int td3_grid_of(const bcn_td3_cfg* c) {
  const size_t slab = td3_n_elems(c) * td3_esz(c);
  size_t g = ((size_t)64 << 20) / slab;
  g = g < 8 ? 8 : g;
  return (int)(g > BCN_TD3_MAX_GRID ? BCN_TD3_MAX_GRID : g);
}

static int td3_state_lay(const bcn_td3_cfg* c, bcn_td3_seg* segs, int max_segs, size_t* bytes) {
  Td3SegDesc d[5];
  const size_t n = td3_n_elems(c);
  td3_desc(&d[0], "counters", BCN_TD3_U32, (size_t)c->batch);
  td3_desc(&d[1], "step", BCN_TD3_I32, 4);
  td3_desc(&d[2], "stats", BCN_TD3_F64, BCN_TD3_N_STATS);
  td3_desc(&d[3], "adam_m", BCN_TD3_REAL, n);
  td3_desc(&d[4], "adam_v", BCN_TD3_REAL, n);
  *bytes = td3_lay(d, 5, td3_esz(c), segs, max_segs);
  return 5;
}

static int td3_work_lay(const bcn_td3_cfg* c, int64_t m, bcn_td3_seg* segs, int max_segs, size_t* bytes) {
  Td3SegDesc d[7];
  const size_t n = td3_n_elems(c), D = (size_t)c->obs_dim + c->act_dim;
  td3_desc(&d[0], "grad", BCN_TD3_REAL, n);
  td3_desc(&d[1], "wg_stats", BCN_TD3_F64, (size_t)BCN_TD3_MAX_GRID * BCN_TD3_N_STATS);
  td3_desc(&d[2], "norm2", BCN_TD3_F64, (n + TD3_NT - 1) / TD3_NT);
  td3_desc(&d[3], "slabs", BCN_TD3_REAL, (size_t)td3_grid_of(c) * n);
  td3_desc(&d[4], "rw", BCN_TD3_REAL, 3 * (size_t)m);
  td3_desc(&d[5], "xa", BCN_TD3_REAL, (size_t)m * D);
  td3_desc(&d[6], "xb", BCN_TD3_REAL, (size_t)m * D);
  *bytes = td3_lay(d, 7, td3_esz(c), segs, max_segs);
  return 7;
}

static int td3_replay_lay(const bcn_td3_cfg* c, int64_t C, bcn_td3_seg* segs, int max_segs, size_t* bytes) {
  Td3SegDesc d[7];
  td3_desc(&d[0], "head", BCN_TD3_I32, 4);
  td3_desc(&d[1], "obs", BCN_TD3_REAL, (size_t)C * c->obs_dim);
  td3_desc(&d[2], "act", BCN_TD3_REAL, (size_t)C * c->act_dim);
  td3_desc(&d[3], "rwd", BCN_TD3_REAL, (size_t)C);
  td3_desc(&d[4], "next_obs", BCN_TD3_REAL, (size_t)C * c->obs_dim);
  td3_desc(&d[5], "boot", BCN_TD3_U8, (size_t)C);
  td3_desc(&d[6], "live", BCN_TD3_U8, (size_t)C);
  *bytes = td3_lay(d, 7, td3_esz(c), segs, max_segs);
  return 7;
}

static bool td3_m_ok(const char* fn, int64_t m) {
  if (m < 1 || m > 0x7fffffffll) { g_td3_err.set("%s: m = %lld: must lie in 1 .. 2^31 - 1", fn, (long long)m); return false; }
  return true;
}

static bool td3_capacity_ok(const char* fn, int64_t C) {
  if (C < 1 || C > 0x7fffffffll) { g_td3_err.set("%s: capacity = %lld: must lie in 1 .. 2^31 - 1", fn, (long long)C); return false; }
  return true;
}

// ---- the argument block --------------------------------------------------------------------------------------------------------
template <typename real>
static void td3_fill_cfg(const bcn_td3_cfg* c, Td3Args<real>* a) {
  memset(a, 0, sizeof(*a));
  a->obs_dim = c->obs_dim; a->act_dim = c->act_dim; a->D = c->obs_dim + c->act_dim; a->n_hidden = c->n_hidden;
  a->activation = c->activation; a->n_critics = c->n_critics;
  int hmax = 0;
  for (int l = 0; l < c->n_hidden; l++) { a->hidden[l] = c->hidden[l]; hmax = c->hidden[l] > hmax ? c->hidden[l] : hmax; }
  a->hmax_pad = hmax;
  const int omax = hmax > c->act_dim ? hmax : c->act_dim;
  a->wcols = ((omax + 3) & ~3) + 4;
  a->low = (real)c->low; a->high = (real)c->high;
  a->center = (real)((c->high + c->low) / 2.0); a->half = (real)((c->high - c->low) / 2.0);
  bcn_td3_seg s[BCN_TD3_MAX_SEGS];
  size_t bytes;
  td3_params_lay(c, s, BCN_TD3_MAX_SEGS, &bytes);
  const int per = 2 * (c->n_hidden + 1);
  for (int net = 0; net <= c->n_critics; net++) {
    ActorNet& n = net == 0 ? a->mu : a->q[net - 1];
    for (int l = 0; l <= c->n_hidden; l++) {
      n.w[l] = (unsigned)(s[net * per + 2 * l].offset / sizeof(real));
      n.b[l] = (unsigned)(s[net * per + 2 * l + 1].offset / sizeof(real));
    }
  }
}

template <typename real>
static void td3_fill_mem(const bcn_td3_cfg* c, const void* mem, int64_t C, Td3Args<real>* a) {
  bcn_td3_seg s[7];
  size_t bytes;
  td3_replay_lay(c, C, s, 7, &bytes);
  const char* p = static_cast<const char*>(mem);
  a->m_obs = reinterpret_cast<const real*>(p + s[1].offset); a->m_act = reinterpret_cast<const real*>(p + s[2].offset);
  a->m_rwd = reinterpret_cast<const real*>(p + s[3].offset); a->m_next = reinterpret_cast<const real*>(p + s[4].offset);
  a->m_boot = reinterpret_cast<const uint8_t*>(p + s[5].offset); a->m_live = reinterpret_cast<const uint8_t*>(p + s[6].offset);
  a->capacity = C;
}

struct Td3Work { char *grad, *wg_stats, *norm2, *slabs, *rw, *xa, *xb; };
static Td3Work td3_work_of(const bcn_td3_cfg* c, int64_t m, void* work) {
  bcn_td3_seg s[7];
  size_t bytes;
  td3_work_lay(c, m, s, 7, &bytes);
  char* p = static_cast<char*>(work);
  return Td3Work{p + s[0].offset, p + s[1].offset, p + s[2].offset, p + s[3].offset, p + s[4].offset, p + s[5].offset, p + s[6].offset};
}

struct Td3State { char *counters, *step, *stats, *m, *v; };
static Td3State td3_state_of(const bcn_td3_cfg* c, void* state) {
  bcn_td3_seg s[5];
  size_t bytes;
  td3_state_lay(c, s, 5, &bytes);
  char* p = static_cast<char*>(state);
  return Td3State{p + s[0].offset, p + s[1].offset, p + s[2].offset, p + s[3].offset, p + s[4].offset};
}

// the element range of an optimiser's segments: the mu segments in front, the q segments behind them
static void td3_range(const bcn_td3_cfg* c, int which, int* e0, int* e1) {
  bcn_td3_seg s[BCN_TD3_MAX_SEGS];
  size_t bytes;
  td3_params_lay(c, s, BCN_TD3_MAX_SEGS, &bytes);
  const int split = (int)(s[2 * (c->n_hidden + 1)].offset / td3_esz(c));
  if (which == BCN_TD3_OPT_POLICY) { *e0 = 0; *e1 = split; }
  else { *e0 = split; *e1 = (int)(bytes / td3_esz(c)); }
}

template <typename real>
static int td3_act_t(const bcn_td3_cfg* c, const void* params, const void* obs, const uint8_t* mask, void* state, void* actions, int mode,
                     double sigma, uint64_t seed, int64_t replica_offset, void* stream) {
  constexpr int TB = ActorGeom<real>::TB;
  Td3Args<real> a;
  td3_fill_cfg<real>(c, &a);
  a.params = static_cast<const real*>(params);
  a.obs = static_cast<const real*>(obs); a.n_rows = c->batch; a.mask = mask;
  a.counters = reinterpret_cast<uint32_t*>(td3_state_of(c, state).counters);
  a.actions = static_cast<real*>(actions); a.mode = mode; a.sigma = (real)sigma;
  a.seed_lo = (uint32_t)(seed & 0xffffffffull); a.seed_hi = (uint32_t)(seed >> 32); a.replica_offset = replica_offset;
  return td3_launch_tile<real>(TD3_K_ACT, a, (c->batch + TB - 1) / TB, stream);
}

template <typename real>
static int td3_grad_t(const bcn_td3_cfg* c, const bcn_td3_batch* b, int which, void* stream) {
  constexpr int TB = ActorGeom<real>::TB;
  Td3Args<real> a;
  td3_fill_cfg<real>(c, &a);
  td3_fill_mem<real>(c, b->mem_dev, b->capacity, &a);
  const Td3Work w = td3_work_of(c, b->m, b->work_dev);
  const Td3State s = td3_state_of(c, b->state_dev);
  a.params = static_cast<const real*>(b->params_dev); a.target = static_cast<const real*>(b->target_dev);
  a.idx = b->idx_dev; a.m = b->m; a.tiles = (b->m + TB - 1) / TB;
  a.gamma = (real)b->gamma; a.sigma_t = (real)b->target_noise; a.c_noise = (real)b->noise_clip;
  a.seed_lo = (uint32_t)(b->seed & 0xffffffffull); a.seed_hi = (uint32_t)(b->seed >> 32);
  a.step = reinterpret_cast<const int32_t*>(s.step);
  a.rw = reinterpret_cast<real*>(w.rw); a.xa = reinterpret_cast<real*>(w.xa); a.xb = reinterpret_cast<real*>(w.xb);
  a.slabs = reinterpret_cast<real*>(w.slabs); a.slab_elems = td3_n_elems(c); a.wg_stats = reinterpret_cast<double*>(w.wg_stats);
  const int gmax = td3_grid_of(c);
  const int grid = a.tiles < gmax ? (int)a.tiles : gmax;
  int e = td3_launch_tile<real>(which == BCN_TD3_OPT_CRITIC ? TD3_K_NEXT : TD3_K_MU, a, (int)a.tiles, stream);
  if (e) return e;
  e = td3_launch_tile<real>(which == BCN_TD3_OPT_CRITIC ? TD3_K_CRITIC : TD3_K_ACTOR, a, grid, stream);
  if (e) return e;
  Td3ReduceArgs<real> r;
  memset(&r, 0, sizeof(r));
  r.slabs = a.slabs; r.slab_elems = a.slab_elems; r.used = grid; r.wg_stats = a.wg_stats; r.grad = reinterpret_cast<real*>(w.grad);
  td3_range(c, which, &r.e0, &r.e1);
  r.norm2 = reinterpret_cast<double*>(w.norm2); r.stats = reinterpret_cast<double*>(s.stats); r.which = which;
  return td3_launch_reduce<real>(r, (r.e1 - r.e0 + TD3_NT - 1) / TD3_NT,
                                 r.stats + (which == BCN_TD3_OPT_CRITIC ? BCN_TD3_STAT_CRITIC_NORM : BCN_TD3_STAT_POLICY_NORM), stream);
}

static bool td3_batch_ok(const char* fn, const bcn_td3_cfg* c, const bcn_td3_batch* b, bool critic) {
  if (!td3_cfg_ok(c, true)) return false;
  if (!b) { g_td3_err.set("%s: batch is NULL", fn); return false; }
  if (!b->params_dev) { g_td3_err.set("%s: batch.params_dev is NULL", fn); return false; }
  if (critic && !b->target_dev) { g_td3_err.set("%s: batch.target_dev is NULL", fn); return false; }
  if (!b->mem_dev) { g_td3_err.set("%s: batch.mem_dev is NULL", fn); return false; }
  if (!b->idx_dev) { g_td3_err.set("%s: batch.idx_dev is NULL", fn); return false; }
  if (!b->work_dev) { g_td3_err.set("%s: batch.work_dev is NULL", fn); return false; }
  if (!b->state_dev) { g_td3_err.set("%s: batch.state_dev is NULL", fn); return false; }
  if (!td3_m_ok(fn, b->m) || !td3_capacity_ok(fn, b->capacity)) return false;
  if (critic) {
    if (!(b->gamma >= 0.0 && b->gamma <= 1.0)) { g_td3_err.set("%s: batch.gamma = %g: must lie in [0, 1]", fn, b->gamma); return false; }
    if (!(b->target_noise >= 0.0)) { g_td3_err.set("%s: batch.target_noise = %g: must be >= 0", fn, b->target_noise); return false; }
    if (!(b->noise_clip >= 0.0)) { g_td3_err.set("%s: batch.noise_clip = %g: must be >= 0", fn, b->noise_clip); return false; }
  }
  return true;
}

// the double launches live in td3_f64.hip
template <> int td3_launch_tile<double>(int kernel, const Td3Args<double>& a, int grid, void* stream);
template <> int td3_launch_reduce<double>(const Td3ReduceArgs<double>& r, int blocks, double* norm_out, void* stream);
template <> int td3_launch_adam<double>(const Td3AdamArgs<double>& a, void* stream);
template <> int td3_launch_polyak<double>(const double* params, double* target, int n, double tau, void* stream);
template <> int td3_launch_append<double>(const ReplayArgs<double>& a, void* stream);

template <typename real>
static int td3_adam_t(const bcn_td3_cfg* c, void* params, void* work, void* state, int which, const bcn_td3_adam_hyper* h, void* stream) {
  const Td3Work w = td3_work_of(c, 1, work);
  const Td3State s = td3_state_of(c, state);
  Td3AdamArgs<real> a;
  memset(&a, 0, sizeof(a));
  a.params = static_cast<real*>(params); a.grad = reinterpret_cast<const real*>(w.grad);
  a.m = reinterpret_cast<real*>(s.m); a.v = reinterpret_cast<real*>(s.v); a.step = reinterpret_cast<int32_t*>(s.step);
  a.norm = reinterpret_cast<const double*>(s.stats) + (which == BCN_TD3_OPT_CRITIC ? BCN_TD3_STAT_CRITIC_NORM : BCN_TD3_STAT_POLICY_NORM);
  td3_range(c, which, &a.e0, &a.e1);
  a.which = which;
  a.lr = h->lr; a.beta1 = h->beta1; a.beta2 = h->beta2; a.eps = h->eps; a.max_grad_norm = h->max_grad_norm;
  return td3_launch_adam<real>(a, stream);
}

template <typename real>
static int td3_append_t(const bcn_td3_cfg* c, int64_t C, void* mem, int T, const void* obs, const void* act, const void* rwd, const uint8_t* done,
                        const uint8_t* trunc, const uint8_t* valid, const void* final_obs, const int32_t* cursor, void* stream) {
  bcn_td3_seg s[7];
  size_t bytes;
  td3_replay_lay(c, C, s, 7, &bytes);
  char* p = static_cast<char*>(mem);
  ReplayArgs<real> a;
  memset(&a, 0, sizeof(a));
  a.head = reinterpret_cast<int32_t*>(p + s[0].offset);
  a.obs = reinterpret_cast<real*>(p + s[1].offset); a.act = reinterpret_cast<real*>(p + s[2].offset);
  a.rwd = reinterpret_cast<real*>(p + s[3].offset); a.next = reinterpret_cast<real*>(p + s[4].offset);
  a.boot = reinterpret_cast<uint8_t*>(p + s[5].offset); a.live = reinterpret_cast<uint8_t*>(p + s[6].offset);
  a.C = C; a.T = T; a.B = c->batch; a.od = c->obs_dim; a.ad = c->act_dim;
  a.r_obs = static_cast<const real*>(obs); a.r_act = static_cast<const real*>(act); a.r_rwd = static_cast<const real*>(rwd);
  a.r_final = static_cast<const real*>(final_obs); a.r_done = done; a.r_trunc = trunc; a.r_valid = valid; a.cursor = cursor;
  return td3_launch_append<real>(a, stream);
}

static int td3_hip(const char* fn, int e) {
  if (e) { g_td3_err.set("%s: launch -> %s", fn, hipGetErrorString((hipError_t)e)); return BCN_TD3_ERR_HIP; }
  return BCN_TD3_OK;
}

extern "C" {

BCN_TD3_API const char* bcn_td3_last_error(void) { return g_td3_err.text; }

BCN_TD3_API int bcn_td3_params_layout(const bcn_td3_cfg* cfg, bcn_td3_seg* segs, int max_segs) {
  size_t bytes;
  return td3_cfg_ok(cfg, false) ? td3_params_lay(cfg, segs, max_segs, &bytes) : 0;
}
BCN_TD3_API size_t bcn_td3_params_bytes(const bcn_td3_cfg* cfg) {
  size_t bytes = 0;
  if (td3_cfg_ok(cfg, false)) td3_params_lay(cfg, nullptr, 0, &bytes);
  return bytes;
}
BCN_TD3_API int bcn_td3_state_layout(const bcn_td3_cfg* cfg, bcn_td3_seg* segs, int max_segs) {
  size_t bytes;
  return td3_cfg_ok(cfg, true) ? td3_state_lay(cfg, segs, max_segs, &bytes) : 0;
}
BCN_TD3_API size_t bcn_td3_state_bytes(const bcn_td3_cfg* cfg) {
  size_t bytes = 0;
  if (td3_cfg_ok(cfg, true)) td3_state_lay(cfg, nullptr, 0, &bytes);
  return bytes;
}
BCN_TD3_API int bcn_td3_work_layout(const bcn_td3_cfg* cfg, int64_t m, bcn_td3_seg* segs, int max_segs) {
  size_t bytes;
  return td3_cfg_ok(cfg, false) && td3_m_ok("bcn_td3_work_layout", m) ? td3_work_lay(cfg, m, segs, max_segs, &bytes) : 0;
}
BCN_TD3_API size_t bcn_td3_work_bytes(const bcn_td3_cfg* cfg, int64_t m) {
  size_t bytes = 0;
  if (td3_cfg_ok(cfg, false) && td3_m_ok("bcn_td3_work_bytes", m)) td3_work_lay(cfg, m, nullptr, 0, &bytes);
  return bytes;
}
BCN_TD3_API int bcn_replay_layout(const bcn_td3_cfg* cfg, int64_t capacity, bcn_td3_seg* segs, int max_segs) {
  size_t bytes;
  return td3_cfg_ok(cfg, false) && td3_capacity_ok("bcn_replay_layout", capacity) ? td3_replay_lay(cfg, capacity, segs, max_segs, &bytes) : 0;
}
BCN_TD3_API size_t bcn_replay_bytes(const bcn_td3_cfg* cfg, int64_t capacity) {
  size_t bytes = 0;
  if (td3_cfg_ok(cfg, false) && td3_capacity_ok("bcn_replay_bytes", capacity)) td3_replay_lay(cfg, capacity, nullptr, 0, &bytes);
  return bytes;
}
BCN_TD3_API int bcn_td3_grid(const bcn_td3_cfg* cfg) { return td3_cfg_ok(cfg, false) ? td3_grid_of(cfg) : 0; }

BCN_TD3_API int bcn_td3_act(const bcn_td3_cfg* cfg, const void* params_dev, const void* obs_dev, const uint8_t* mask_dev, void* state_dev,
                            void* actions_dev, int mode, double sigma, uint64_t seed, int64_t replica_offset, void* stream) {
  if (!td3_cfg_ok(cfg, true)) return BCN_TD3_ERR_ARG;
  if (!params_dev) { g_td3_err.set("bcn_td3_act: params_dev is NULL"); return BCN_TD3_ERR_ARG; }
  if (!obs_dev) { g_td3_err.set("bcn_td3_act: obs_dev is NULL"); return BCN_TD3_ERR_ARG; }
  if (!state_dev) { g_td3_err.set("bcn_td3_act: state_dev is NULL"); return BCN_TD3_ERR_ARG; }
  if (!actions_dev) { g_td3_err.set("bcn_td3_act: actions_dev is NULL"); return BCN_TD3_ERR_ARG; }
  if (mode < BCN_TD3_DETERMINISTIC || mode > BCN_TD3_UNIFORM) { g_td3_err.set("bcn_td3_act: mode = %d: must be 0 (deterministic), 1 (noisy) or 2 (uniform)", mode); return BCN_TD3_ERR_ARG; }
  if (!(sigma >= 0.0)) { g_td3_err.set("bcn_td3_act: sigma = %g: must be >= 0", sigma); return BCN_TD3_ERR_ARG; }
  if (replica_offset < 0) { g_td3_err.set("bcn_td3_act: replica_offset = %lld: must be >= 0", (long long)replica_offset); return BCN_TD3_ERR_ARG; }
  return td3_hip("bcn_td3_act", cfg->dtype ? td3_act_t<double>(cfg, params_dev, obs_dev, mask_dev, state_dev, actions_dev, mode, sigma, seed, replica_offset, stream)
                                           : td3_act_t<float>(cfg, params_dev, obs_dev, mask_dev, state_dev, actions_dev, mode, sigma, seed, replica_offset, stream));
}

BCN_TD3_API int bcn_replay_append(const bcn_td3_cfg* cfg, int64_t capacity, void* mem_dev, int T, const void* obs_dev, const void* act_dev,
                                  const void* rwd_dev, const uint8_t* done_dev, const uint8_t* trunc_dev, const uint8_t* valid_dev,
                                  const void* final_obs_dev, const int32_t* cursor_dev, void* stream) {
  if (!td3_cfg_ok(cfg, true) || !td3_capacity_ok("bcn_replay_append", capacity)) return BCN_TD3_ERR_ARG;
  if (T < 1) { g_td3_err.set("bcn_replay_append: T = %d: must be >= 1", T); return BCN_TD3_ERR_ARG; }
  if ((long long)T * cfg->batch > capacity) {
    g_td3_err.set("bcn_replay_append: T batch = %d x %d = %lld transitions exceed the capacity %lld: one append may not lap the ring", T, cfg->batch,
                  (long long)T * cfg->batch, (long long)capacity);
    return BCN_TD3_ERR_ARG;
  }
  const void* ptrs[9] = {mem_dev, obs_dev, act_dev, rwd_dev, done_dev, trunc_dev, valid_dev, final_obs_dev, cursor_dev};
  const char* names[9] = {"mem_dev", "obs_dev", "act_dev", "rwd_dev", "done_dev", "trunc_dev", "valid_dev", "final_obs_dev", "cursor_dev"};
  for (int k = 0; k < 9; k++)
    if (!ptrs[k]) { g_td3_err.set("bcn_replay_append: %s is NULL%s", names[k], k == 7 ? " (the rollout needs its final_obs segment)" : ""); return BCN_TD3_ERR_ARG; }
  return td3_hip("bcn_replay_append", cfg->dtype ? td3_append_t<double>(cfg, capacity, mem_dev, T, obs_dev, act_dev, rwd_dev, done_dev, trunc_dev, valid_dev, final_obs_dev, cursor_dev, stream)
                                                 : td3_append_t<float>(cfg, capacity, mem_dev, T, obs_dev, act_dev, rwd_dev, done_dev, trunc_dev, valid_dev, final_obs_dev, cursor_dev, stream));
}

BCN_TD3_API int bcn_replay_sample(int64_t m, uint64_t seed, int32_t* head_dev, int32_t* idx_dev, void* stream) {
  if (!td3_m_ok("bcn_replay_sample", m)) return BCN_TD3_ERR_ARG;
  if (!head_dev) { g_td3_err.set("bcn_replay_sample: head_dev is NULL"); return BCN_TD3_ERR_ARG; }
  if (!idx_dev) { g_td3_err.set("bcn_replay_sample: idx_dev is NULL"); return BCN_TD3_ERR_ARG; }
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(replay_sample_kernel<float>, dim3((unsigned)((m + TD3_NT - 1) / TD3_NT)), dim3(TD3_NT), 0, st, (long long)m,
                     (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), (const int32_t*)head_dev, idx_dev);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) {
    hipLaunchKernelGGL(replay_sample_tick_kernel<float>, dim3(1), dim3(64), 0, st, head_dev);
    e = hipGetLastError();
  }
  return td3_hip("bcn_replay_sample", (int)e);
}

BCN_TD3_API int bcn_td3_critic_grad(const bcn_td3_cfg* cfg, const bcn_td3_batch* batch, void* stream) {
  if (!td3_batch_ok("bcn_td3_critic_grad", cfg, batch, true)) return BCN_TD3_ERR_ARG;
  return td3_hip("bcn_td3_critic_grad", cfg->dtype ? td3_grad_t<double>(cfg, batch, BCN_TD3_OPT_CRITIC, stream) : td3_grad_t<float>(cfg, batch, BCN_TD3_OPT_CRITIC, stream));
}

BCN_TD3_API int bcn_td3_actor_grad(const bcn_td3_cfg* cfg, const bcn_td3_batch* batch, void* stream) {
  if (!td3_batch_ok("bcn_td3_actor_grad", cfg, batch, false)) return BCN_TD3_ERR_ARG;
  return td3_hip("bcn_td3_actor_grad", cfg->dtype ? td3_grad_t<double>(cfg, batch, BCN_TD3_OPT_POLICY, stream) : td3_grad_t<float>(cfg, batch, BCN_TD3_OPT_POLICY, stream));
}

BCN_TD3_API int bcn_td3_adam(const bcn_td3_cfg* cfg, void* params_dev, void* work_dev, void* state_dev, int which,
                             const bcn_td3_adam_hyper* h, void* stream) {
  if (!td3_cfg_ok(cfg, true)) return BCN_TD3_ERR_ARG;
  if (!params_dev || !work_dev || !state_dev || !h) { g_td3_err.set("bcn_td3_adam: params_dev, work_dev, state_dev or hyper is NULL"); return BCN_TD3_ERR_ARG; }
  if (which != BCN_TD3_OPT_CRITIC && which != BCN_TD3_OPT_POLICY) { g_td3_err.set("bcn_td3_adam: which = %d: must be 0 (critic) or 1 (policy)", which); return BCN_TD3_ERR_ARG; }
  if (!(h->lr >= 0.0)) { g_td3_err.set("bcn_td3_adam: hyper.lr = %g: must be >= 0", h->lr); return BCN_TD3_ERR_ARG; }
  if (!(h->beta1 >= 0.0 && h->beta1 < 1.0) || !(h->beta2 >= 0.0 && h->beta2 < 1.0)) {
    g_td3_err.set("bcn_td3_adam: hyper.beta1 = %g, hyper.beta2 = %g: must lie in [0, 1)", h->beta1, h->beta2);
    return BCN_TD3_ERR_ARG;
  }
  if (!(h->eps >= 0.0)) { g_td3_err.set("bcn_td3_adam: hyper.eps = %g: must be >= 0", h->eps); return BCN_TD3_ERR_ARG; }
  return td3_hip("bcn_td3_adam", cfg->dtype ? td3_adam_t<double>(cfg, params_dev, work_dev, state_dev, which, h, stream)
                                            : td3_adam_t<float>(cfg, params_dev, work_dev, state_dev, which, h, stream));
}

BCN_TD3_API int bcn_td3_polyak(const bcn_td3_cfg* cfg, const void* params_dev, void* target_dev, double tau, void* stream) {
  if (!td3_cfg_ok(cfg, false)) return BCN_TD3_ERR_ARG;
  if (!params_dev || !target_dev) { g_td3_err.set("bcn_td3_polyak: params_dev or target_dev is NULL"); return BCN_TD3_ERR_ARG; }
  if (!(tau >= 0.0 && tau <= 1.0)) { g_td3_err.set("bcn_td3_polyak: tau = %g: must lie in [0, 1]", tau); return BCN_TD3_ERR_ARG; }
  const int n = (int)td3_n_elems(cfg);
  return td3_hip("bcn_td3_polyak", cfg->dtype ? td3_launch_polyak<double>(static_cast<const double*>(params_dev), static_cast<double*>(target_dev), n, tau, stream)
                                              : td3_launch_polyak<float>(static_cast<const float*>(params_dev), static_cast<float*>(target_dev), n, (float)tau, stream));
}

}  // extern "C"
