// sac.hip -- libbeacon_sac.so (include/beacon_sac.h): the C ABI, the layouts, the argument checks, and the float32 instantiation of
// the kernels of sac_impl.h.  The float64 instantiation is sac_f64.hip (built without FMA contraction).
#include <math.h>

#include "sac_impl.h"

SAC_DEFINE_LAUNCH(float)

static thread_local PolicyErr g_sac_err;

// ---- cfg, layouts ------------------------------------------------------------------------------------------------------------
static int sac_wcols(const bcn_sac_cfg* c) {
  int hmax = 0;
  for (int l = 0; l < c->n_hidden; l++) hmax = c->hidden[l] > hmax ? c->hidden[l] : hmax;
  const int omax = hmax > 2 * c->act_dim ? hmax : 2 * c->act_dim;
  return ((omax + 3) & ~3) + 4;
}

static int sac_hmax(const bcn_sac_cfg* c) {
  int hmax = 0;
  for (int l = 0; l < c->n_hidden; l++) hmax = c->hidden[l] > hmax ? c->hidden[l] : hmax;
  return hmax;
}

static size_t sac_lds_of(const bcn_sac_cfg* c) {
  return c->dtype ? td3_lds_bytes<double>(c->n_hidden, sac_hmax(c), sac_wcols(c)) : td3_lds_bytes<float>(c->n_hidden, sac_hmax(c), sac_wcols(c));
}

static bool sac_cfg_ok(const bcn_sac_cfg* c, bool need_batch) {
  PolicyErr* err = &g_sac_err;
  if (!c) { err->set("cfg is NULL"); return false; }
  if (need_batch && c->batch < 1) { err->set("cfg.batch = %d: must be >= 1", c->batch); return false; }
  if (c->act_dim < 1 || c->act_dim > BCN_ACTOR_MAX_ACT) { err->set("cfg.act_dim = %d: must lie in 1 .. %d", c->act_dim, BCN_ACTOR_MAX_ACT); return false; }
  if (c->obs_dim < 1 || (long long)c->obs_dim + c->act_dim > BCN_SAC_MAX_IN) {
    err->set("cfg.obs_dim = %d, cfg.act_dim = %d: need obs_dim >= 1 and obs_dim + act_dim <= %d (a critic's input row)", c->obs_dim, c->act_dim, BCN_SAC_MAX_IN);
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
  if (!(c->low < c->high) || !isfinite(c->low) || !isfinite(c->high)) {
    err->set("cfg.low = %g, cfg.high = %g: need finite low < high (the log-density holds ln((high - low) / 2))", c->low, c->high);
    return false;
  }
  if (c->n_critics != 1 && c->n_critics != 2) { err->set("cfg.n_critics = %d: must be 1 or 2", c->n_critics); return false; }
  const size_t lds = sac_lds_of(c);
  if (lds > (size_t)SAC_LDS_LIMIT) {
    err->set("cfg: the tile kernels need %zu bytes of LDS for these widths, the device has %d", lds, SAC_LDS_LIMIT);
    return false;
  }
  return true;
}

static size_t sac_esz(const bcn_sac_cfg* c) { return c->dtype ? 8 : 4; }

struct SacSegDesc { char name[16]; int elem; size_t n; };

static size_t sac_lay(const SacSegDesc* d, int nd, size_t esz, bcn_sac_seg* segs, int max_segs) {
  size_t off = 0;
  for (int k = 0; k < nd; k++) {
    off = (off + 15) & ~(size_t)15;
    if (segs && k < max_segs) {
      memset(&segs[k], 0, sizeof(segs[k]));
      strncpy(segs[k].name, d[k].name, sizeof(segs[k].name) - 1);
      segs[k].offset = off; segs[k].elem = d[k].elem; segs[k].planes = 0; segs[k].row_elems = (int64_t)d[k].n;
    }
    off += d[k].n * (d[k].elem == BCN_SAC_REAL ? esz : d[k].elem == BCN_SAC_F64 ? 8 : d[k].elem == BCN_SAC_U8 ? 1 : 4);
  }
  return (off + 15) & ~(size_t)15;
}

static void sac_desc(SacSegDesc* d, const char* name, int elem, size_t n) {
  memset(d, 0, sizeof(*d));
  strncpy(d->name, name, sizeof(d->name) - 1);
  d->elem = elem; d->n = n;
}

static int sac_params_lay(const bcn_sac_cfg* c, bcn_sac_seg* segs, int max_segs, size_t* bytes) {
  SacSegDesc d[BCN_SAC_MAX_SEGS];
  int nd = 0;
  for (int net = 0; net <= c->n_critics; net++) {
    size_t in = net == 0 ? (size_t)c->obs_dim : (size_t)c->obs_dim + c->act_dim;
    for (int l = 0; l <= c->n_hidden; l++) {
      const size_t out = l < c->n_hidden ? (size_t)c->hidden[l] : (net == 0 ? 2 * (size_t)c->act_dim : 1);
      char name[16];
      snprintf(name, sizeof(name), "%s_w%d", net == 0 ? "pi" : (net == 1 ? "q1" : "q2"), l);
      sac_desc(&d[nd++], name, BCN_SAC_REAL, out * in);
      snprintf(name, sizeof(name), "%s_b%d", net == 0 ? "pi" : (net == 1 ? "q1" : "q2"), l);
      sac_desc(&d[nd++], name, BCN_SAC_REAL, out);
      in = out;
    }
  }
  sac_desc(&d[nd++], "log_alpha", BCN_SAC_REAL, 1);
  *bytes = sac_lay(d, nd, sac_esz(c), segs, max_segs);
  return nd;
}

static size_t sac_n_elems(const bcn_sac_cfg* c) {
  size_t bytes;
  sac_params_lay(c, nullptr, 0, &bytes);
  return bytes / sac_esz(c);
}

static int sac_grid_of(const bcn_sac_cfg* c) {
  const size_t slab = sac_n_elems(c) * sac_esz(c);
  size_t g = ((size_t)64 << 20) / slab;
  g = g < 8 ? 8 : g;
  return (int)(g > BCN_SAC_MAX_GRID ? BCN_SAC_MAX_GRID : g);
}

static int sac_state_lay(const bcn_sac_cfg* c, bcn_sac_seg* segs, int max_segs, size_t* bytes) {
  SacSegDesc d[5];
  const size_t n = sac_n_elems(c);
  sac_desc(&d[0], "counters", BCN_SAC_U32, (size_t)c->batch);
  sac_desc(&d[1], "step", BCN_SAC_I32, 8);
  sac_desc(&d[2], "stats", BCN_SAC_F64, BCN_SAC_N_STATS);
  sac_desc(&d[3], "adam_m", BCN_SAC_REAL, n);
  sac_desc(&d[4], "adam_v", BCN_SAC_REAL, n);
  *bytes = sac_lay(d, 5, sac_esz(c), segs, max_segs);
  return 5;
}

static int sac_work_lay(const bcn_sac_cfg* c, int64_t m, bcn_sac_seg* segs, int max_segs, size_t* bytes) {
  SacSegDesc d[7];
  const size_t n = sac_n_elems(c), D = (size_t)c->obs_dim + c->act_dim;
  sac_desc(&d[0], "grad", BCN_SAC_REAL, n);
  sac_desc(&d[1], "wg_stats", BCN_SAC_F64, (size_t)BCN_SAC_MAX_GRID * BCN_SAC_N_STATS);
  sac_desc(&d[2], "norm2", BCN_SAC_F64, (n + TD3_NT - 1) / TD3_NT);
  sac_desc(&d[3], "slabs", BCN_SAC_REAL, (size_t)sac_grid_of(c) * n);
  sac_desc(&d[4], "rw", BCN_SAC_REAL, 4 * (size_t)m);
  sac_desc(&d[5], "xa", BCN_SAC_REAL, (size_t)m * D);
  sac_desc(&d[6], "xb", BCN_SAC_REAL, (size_t)m * D);
  *bytes = sac_lay(d, 7, sac_esz(c), segs, max_segs);
  return 7;
}

static bool sac_m_ok(const char* fn, int64_t m) {
  if (m < 1 || m > 0x7fffffffll) { g_sac_err.set("%s: m = %lld: must lie in 1 .. 2^31 - 1", fn, (long long)m); return false; }
  return true;
}

// ---- the argument block --------------------------------------------------------------------------------------------------------
struct SacRanges { int split, la, end; };      // elements: pi in [0, split), q in [split, la), log_alpha at la
static SacRanges sac_ranges(const bcn_sac_cfg* c) {
  bcn_sac_seg s[BCN_SAC_MAX_SEGS];
  size_t bytes;
  const int ns = sac_params_lay(c, s, BCN_SAC_MAX_SEGS, &bytes);
  SacRanges r;
  r.split = (int)(s[2 * (c->n_hidden + 1)].offset / sac_esz(c));
  r.la = (int)(s[ns - 1].offset / sac_esz(c));
  r.end = (int)(bytes / sac_esz(c));
  return r;
}

template <typename real>
static void sac_fill_cfg(const bcn_sac_cfg* c, SacArgs<real>* S) {
  memset(S, 0, sizeof(*S));
  Td3Args<real>* a = &S->t;
  a->obs_dim = c->obs_dim; a->act_dim = c->act_dim; a->D = c->obs_dim + c->act_dim; a->n_hidden = c->n_hidden;
  a->activation = c->activation; a->n_critics = c->n_critics;
  for (int l = 0; l < c->n_hidden; l++) a->hidden[l] = c->hidden[l];
  a->hmax_pad = sac_hmax(c);
  a->wcols = sac_wcols(c);
  a->low = (real)c->low; a->high = (real)c->high;
  a->center = (real)((c->high + c->low) / 2.0); a->half = (real)((c->high - c->low) / 2.0);
  S->ln_half = (real)log((c->high - c->low) / 2.0);
  bcn_sac_seg s[BCN_SAC_MAX_SEGS];
  size_t bytes;
  const int ns = sac_params_lay(c, s, BCN_SAC_MAX_SEGS, &bytes);
  const int per = 2 * (c->n_hidden + 1);
  for (int net = 0; net <= c->n_critics; net++) {
    ActorNet& n = net == 0 ? a->mu : a->q[net - 1];
    for (int l = 0; l <= c->n_hidden; l++) {
      n.w[l] = (unsigned)(s[net * per + 2 * l].offset / sizeof(real));
      n.b[l] = (unsigned)(s[net * per + 2 * l + 1].offset / sizeof(real));
    }
  }
  S->la = (unsigned)(s[ns - 1].offset / sizeof(real));
}

struct SacWork { char *grad, *wg_stats, *norm2, *slabs, *rw, *xa, *xb; };
static SacWork sac_work_of(const bcn_sac_cfg* c, int64_t m, void* work) {
  bcn_sac_seg s[7];
  size_t bytes;
  sac_work_lay(c, m, s, 7, &bytes);
  char* p = static_cast<char*>(work);
  return SacWork{p + s[0].offset, p + s[1].offset, p + s[2].offset, p + s[3].offset, p + s[4].offset, p + s[5].offset, p + s[6].offset};
}

struct SacState { char *counters, *step, *stats, *m, *v; };
static SacState sac_state_of(const bcn_sac_cfg* c, void* state) {
  bcn_sac_seg s[5];
  size_t bytes;
  sac_state_lay(c, s, 5, &bytes);
  char* p = static_cast<char*>(state);
  return SacState{p + s[0].offset, p + s[1].offset, p + s[2].offset, p + s[3].offset, p + s[4].offset};
}

template <typename real>
static int sac_act_t(const bcn_sac_cfg* c, const void* params, const void* obs, const uint8_t* mask, void* state, void* actions, int mode,
                     uint64_t seed, int64_t replica_offset, void* stream) {
  constexpr int TB = ActorGeom<real>::TB;
  SacArgs<real> S;
  sac_fill_cfg<real>(c, &S);
  Td3Args<real>& a = S.t;
  a.params = static_cast<const real*>(params);
  a.obs = static_cast<const real*>(obs); a.n_rows = c->batch; a.mask = mask;
  a.counters = reinterpret_cast<uint32_t*>(sac_state_of(c, state).counters);
  a.actions = static_cast<real*>(actions); a.mode = mode;
  a.seed_lo = (uint32_t)(seed & 0xffffffffull); a.seed_hi = (uint32_t)(seed >> 32); a.replica_offset = replica_offset;
  return sac_launch_tile<real>(SAC_K_ACT, S, (c->batch + TB - 1) / TB, stream);
}

template <typename real>
static int sac_grad_t(const bcn_sac_cfg* c, const bcn_sac_batch* b, int which, void* stream) {
  constexpr int TB = ActorGeom<real>::TB;
  SacArgs<real> S;
  sac_fill_cfg<real>(c, &S);
  Td3Args<real>& a = S.t;
  a.m_obs = static_cast<const real*>(b->obs_dev); a.m_act = static_cast<const real*>(b->act_dev);
  a.m_rwd = static_cast<const real*>(b->rwd_dev); a.m_next = static_cast<const real*>(b->next_obs_dev);
  a.m_boot = b->boot_dev; a.m_live = b->live_dev; a.capacity = b->capacity;
  const SacWork w = sac_work_of(c, b->m, b->work_dev);
  const SacState s = sac_state_of(c, b->state_dev);
  a.params = static_cast<const real*>(b->params_dev); a.target = static_cast<const real*>(b->target_dev);
  a.idx = b->idx_dev; a.m = b->m; a.tiles = (b->m + TB - 1) / TB;
  a.gamma = (real)b->gamma;
  a.seed_lo = (uint32_t)(b->seed & 0xffffffffull); a.seed_hi = (uint32_t)(b->seed >> 32);
  a.step = reinterpret_cast<const int32_t*>(s.step);
  a.rw = reinterpret_cast<real*>(w.rw); a.xa = reinterpret_cast<real*>(w.xa); a.xb = reinterpret_cast<real*>(w.xb);
  a.slabs = reinterpret_cast<real*>(w.slabs); a.slab_elems = sac_n_elems(c); a.wg_stats = reinterpret_cast<double*>(w.wg_stats);
  const int gmax = sac_grid_of(c);
  const int grid = a.tiles < gmax ? (int)a.tiles : gmax;
  const bool critic = which == BCN_SAC_OPT_CRITIC;
  int e = sac_launch_tile<real>(critic ? SAC_K_NEXT : SAC_K_PI, S, (int)a.tiles, stream);
  if (e) return e;
  e = sac_launch_tile<real>(critic ? SAC_K_CRITIC : SAC_K_ACTOR, S, grid, stream);
  if (e) return e;
  SacReduceArgs<real> R;
  memset(&R, 0, sizeof(R));
  Td3ReduceArgs<real>& r = R.r;
  r.slabs = a.slabs; r.slab_elems = a.slab_elems; r.used = grid; r.wg_stats = a.wg_stats; r.grad = reinterpret_cast<real*>(w.grad);
  const SacRanges rg = sac_ranges(c);
  r.e0 = critic ? rg.split : 0; r.e1 = critic ? rg.la : rg.split;
  r.norm2 = reinterpret_cast<double*>(w.norm2); r.stats = reinterpret_cast<double*>(s.stats); r.which = which;
  R.params = a.params; R.la = rg.la; R.target_entropy = b->target_entropy;
  return sac_launch_reduce<real>(R, (r.e1 - r.e0 + TD3_NT - 1) / TD3_NT, r.stats + (critic ? BCN_SAC_STAT_CRITIC_NORM : BCN_SAC_STAT_POLICY_NORM), stream);
}

static bool sac_batch_ok(const char* fn, const bcn_sac_cfg* c, const bcn_sac_batch* b, bool critic) {
  if (!sac_cfg_ok(c, true)) return false;
  if (!b) { g_sac_err.set("%s: batch is NULL", fn); return false; }
  if (!b->params_dev) { g_sac_err.set("%s: batch.params_dev is NULL", fn); return false; }
  if (critic && !b->target_dev) { g_sac_err.set("%s: batch.target_dev is NULL", fn); return false; }
  const void* mem[6] = {b->obs_dev, b->act_dev, b->rwd_dev, b->next_obs_dev, b->boot_dev, b->live_dev};
  const char* names[6] = {"obs_dev", "act_dev", "rwd_dev", "next_obs_dev", "boot_dev", "live_dev"};
  for (int k = 0; k < 6; k++)
    if (!mem[k]) { g_sac_err.set("%s: batch.%s is NULL (a segment of the replay memory)", fn, names[k]); return false; }
  if (!b->idx_dev) { g_sac_err.set("%s: batch.idx_dev is NULL", fn); return false; }
  if (!b->work_dev) { g_sac_err.set("%s: batch.work_dev is NULL", fn); return false; }
  if (!b->state_dev) { g_sac_err.set("%s: batch.state_dev is NULL", fn); return false; }
  if (!sac_m_ok(fn, b->m)) return false;
  if (b->capacity < 1 || b->capacity > 0x7fffffffll) { g_sac_err.set("%s: batch.capacity = %lld: must lie in 1 .. 2^31 - 1", fn, (long long)b->capacity); return false; }
  if (critic && !(b->gamma >= 0.0 && b->gamma <= 1.0)) { g_sac_err.set("%s: batch.gamma = %g: must lie in [0, 1]", fn, b->gamma); return false; }
  if (!critic && !isfinite(b->target_entropy)) { g_sac_err.set("%s: batch.target_entropy = %g: must be finite", fn, b->target_entropy); return false; }
  return true;
}

// the double launches live in sac_f64.hip
template <> int sac_launch_tile<double>(int kernel, const SacArgs<double>& a, int grid, void* stream);
template <> int sac_launch_reduce<double>(const SacReduceArgs<double>& r, int blocks, double* norm_out, void* stream);
template <> int sac_launch_adam<double>(const Td3AdamArgs<double>& a, void* stream);
template <> int sac_launch_polyak<double>(const double* params, double* target, int n, double tau, void* stream);

template <typename real>
static int sac_adam_t(const bcn_sac_cfg* c, void* params, void* work, void* state, int which, const bcn_sac_adam_hyper* h, void* stream) {
  const SacWork w = sac_work_of(c, 1, work);
  const SacState s = sac_state_of(c, state);
  Td3AdamArgs<real> a;
  memset(&a, 0, sizeof(a));
  a.params = static_cast<real*>(params); a.grad = reinterpret_cast<const real*>(w.grad);
  a.m = reinterpret_cast<real*>(s.m); a.v = reinterpret_cast<real*>(s.v); a.step = reinterpret_cast<int32_t*>(s.step);
  a.norm = reinterpret_cast<const double*>(s.stats) + (which == BCN_SAC_OPT_CRITIC ? BCN_SAC_STAT_CRITIC_NORM : BCN_SAC_STAT_POLICY_NORM);
  const SacRanges rg = sac_ranges(c);
  a.e0 = which == BCN_SAC_OPT_POLICY ? 0 : (which == BCN_SAC_OPT_CRITIC ? rg.split : rg.la);
  a.e1 = which == BCN_SAC_OPT_POLICY ? rg.split : (which == BCN_SAC_OPT_CRITIC ? rg.la : rg.la + 1);
  a.which = which;
  a.lr = h->lr; a.beta1 = h->beta1; a.beta2 = h->beta2; a.eps = h->eps;
  a.max_grad_norm = which == BCN_SAC_OPT_ALPHA ? 0.0 : h->max_grad_norm;      // one element: no norm to clip by
  return sac_launch_adam<real>(a, stream);
}

static int sac_hip(const char* fn, int e) {
  if (e) { g_sac_err.set("%s: launch -> %s", fn, hipGetErrorString((hipError_t)e)); return BCN_SAC_ERR_HIP; }
  return BCN_SAC_OK;
}

extern "C" {

BCN_SAC_API const char* bcn_sac_last_error(void) { return g_sac_err.text; }

BCN_SAC_API int bcn_sac_params_layout(const bcn_sac_cfg* cfg, bcn_sac_seg* segs, int max_segs) {
  size_t bytes;
  return sac_cfg_ok(cfg, false) ? sac_params_lay(cfg, segs, max_segs, &bytes) : 0;
}
BCN_SAC_API size_t bcn_sac_params_bytes(const bcn_sac_cfg* cfg) {
  size_t bytes = 0;
  if (sac_cfg_ok(cfg, false)) sac_params_lay(cfg, nullptr, 0, &bytes);
  return bytes;
}
BCN_SAC_API int bcn_sac_state_layout(const bcn_sac_cfg* cfg, bcn_sac_seg* segs, int max_segs) {
  size_t bytes;
  return sac_cfg_ok(cfg, true) ? sac_state_lay(cfg, segs, max_segs, &bytes) : 0;
}
BCN_SAC_API size_t bcn_sac_state_bytes(const bcn_sac_cfg* cfg) {
  size_t bytes = 0;
  if (sac_cfg_ok(cfg, true)) sac_state_lay(cfg, nullptr, 0, &bytes);
  return bytes;
}
BCN_SAC_API int bcn_sac_work_layout(const bcn_sac_cfg* cfg, int64_t m, bcn_sac_seg* segs, int max_segs) {
  size_t bytes;
  return sac_cfg_ok(cfg, false) && sac_m_ok("bcn_sac_work_layout", m) ? sac_work_lay(cfg, m, segs, max_segs, &bytes) : 0;
}
BCN_SAC_API size_t bcn_sac_work_bytes(const bcn_sac_cfg* cfg, int64_t m) {
  size_t bytes = 0;
  if (sac_cfg_ok(cfg, false) && sac_m_ok("bcn_sac_work_bytes", m)) sac_work_lay(cfg, m, nullptr, 0, &bytes);
  return bytes;
}
BCN_SAC_API int bcn_sac_grid(const bcn_sac_cfg* cfg) { return sac_cfg_ok(cfg, false) ? sac_grid_of(cfg) : 0; }
BCN_SAC_API size_t bcn_sac_lds_bytes(const bcn_sac_cfg* cfg) { return sac_cfg_ok(cfg, false) ? sac_lds_of(cfg) : 0; }

BCN_SAC_API int bcn_sac_act(const bcn_sac_cfg* cfg, const void* params_dev, const void* obs_dev, const uint8_t* mask_dev, void* state_dev,
                            void* actions_dev, int mode, uint64_t seed, int64_t replica_offset, void* stream) {
  if (!sac_cfg_ok(cfg, true)) return BCN_SAC_ERR_ARG;
  if (!params_dev) { g_sac_err.set("bcn_sac_act: params_dev is NULL"); return BCN_SAC_ERR_ARG; }
  if (!obs_dev) { g_sac_err.set("bcn_sac_act: obs_dev is NULL"); return BCN_SAC_ERR_ARG; }
  if (!state_dev) { g_sac_err.set("bcn_sac_act: state_dev is NULL"); return BCN_SAC_ERR_ARG; }
  if (!actions_dev) { g_sac_err.set("bcn_sac_act: actions_dev is NULL"); return BCN_SAC_ERR_ARG; }
  if (mode < BCN_SAC_DETERMINISTIC || mode > BCN_SAC_UNIFORM) { g_sac_err.set("bcn_sac_act: mode = %d: must be 0 (deterministic), 1 (sample) or 2 (uniform)", mode); return BCN_SAC_ERR_ARG; }
  if (replica_offset < 0) { g_sac_err.set("bcn_sac_act: replica_offset = %lld: must be >= 0", (long long)replica_offset); return BCN_SAC_ERR_ARG; }
  return sac_hip("bcn_sac_act", cfg->dtype ? sac_act_t<double>(cfg, params_dev, obs_dev, mask_dev, state_dev, actions_dev, mode, seed, replica_offset, stream)
                                           : sac_act_t<float>(cfg, params_dev, obs_dev, mask_dev, state_dev, actions_dev, mode, seed, replica_offset, stream));
}

BCN_SAC_API int bcn_sac_critic_grad(const bcn_sac_cfg* cfg, const bcn_sac_batch* batch, void* stream) {
  if (!sac_batch_ok("bcn_sac_critic_grad", cfg, batch, true)) return BCN_SAC_ERR_ARG;
  return sac_hip("bcn_sac_critic_grad", cfg->dtype ? sac_grad_t<double>(cfg, batch, BCN_SAC_OPT_CRITIC, stream) : sac_grad_t<float>(cfg, batch, BCN_SAC_OPT_CRITIC, stream));
}

BCN_SAC_API int bcn_sac_actor_grad(const bcn_sac_cfg* cfg, const bcn_sac_batch* batch, void* stream) {
  if (!sac_batch_ok("bcn_sac_actor_grad", cfg, batch, false)) return BCN_SAC_ERR_ARG;
  return sac_hip("bcn_sac_actor_grad", cfg->dtype ? sac_grad_t<double>(cfg, batch, BCN_SAC_OPT_POLICY, stream) : sac_grad_t<float>(cfg, batch, BCN_SAC_OPT_POLICY, stream));
}

BCN_SAC_API int bcn_sac_adam(const bcn_sac_cfg* cfg, void* params_dev, void* work_dev, void* state_dev, int which,
                             const bcn_sac_adam_hyper* h, void* stream) {
  if (!sac_cfg_ok(cfg, true)) return BCN_SAC_ERR_ARG;
  if (!params_dev || !work_dev || !state_dev || !h) { g_sac_err.set("bcn_sac_adam: params_dev, work_dev, state_dev or hyper is NULL"); return BCN_SAC_ERR_ARG; }
  if (which != BCN_SAC_OPT_CRITIC && which != BCN_SAC_OPT_POLICY && which != BCN_SAC_OPT_ALPHA) {
    g_sac_err.set("bcn_sac_adam: which = %d: must be 0 (critic), 1 (policy) or 2 (alpha)", which);
    return BCN_SAC_ERR_ARG;
  }
  if (!(h->lr >= 0.0)) { g_sac_err.set("bcn_sac_adam: hyper.lr = %g: must be >= 0", h->lr); return BCN_SAC_ERR_ARG; }
  if (!(h->beta1 >= 0.0 && h->beta1 < 1.0) || !(h->beta2 >= 0.0 && h->beta2 < 1.0)) {
    g_sac_err.set("bcn_sac_adam: hyper.beta1 = %g, hyper.beta2 = %g: must lie in [0, 1)", h->beta1, h->beta2);
    return BCN_SAC_ERR_ARG;
  }
  if (!(h->eps >= 0.0)) { g_sac_err.set("bcn_sac_adam: hyper.eps = %g: must be >= 0", h->eps); return BCN_SAC_ERR_ARG; }
  return sac_hip("bcn_sac_adam", cfg->dtype ? sac_adam_t<double>(cfg, params_dev, work_dev, state_dev, which, h, stream)
                                            : sac_adam_t<float>(cfg, params_dev, work_dev, state_dev, which, h, stream));
}

BCN_SAC_API int bcn_sac_polyak(const bcn_sac_cfg* cfg, const void* params_dev, void* target_dev, double tau, void* stream) {
  if (!sac_cfg_ok(cfg, false)) return BCN_SAC_ERR_ARG;
  if (!params_dev || !target_dev) { g_sac_err.set("bcn_sac_polyak: params_dev or target_dev is NULL"); return BCN_SAC_ERR_ARG; }
  if (!(tau >= 0.0 && tau <= 1.0)) { g_sac_err.set("bcn_sac_polyak: tau = %g: must lie in [0, 1]", tau); return BCN_SAC_ERR_ARG; }
  const int n = (int)sac_n_elems(cfg);
  return sac_hip("bcn_sac_polyak", cfg->dtype ? sac_launch_polyak<double>(static_cast<const double*>(params_dev), static_cast<double*>(target_dev), n, tau, stream)
                                              : sac_launch_polyak<float>(static_cast<const float*>(params_dev), static_cast<float*>(target_dev), n, (float)tau, stream));
}

}  // extern "C"
