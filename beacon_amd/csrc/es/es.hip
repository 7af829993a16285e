// es.hip -- libbeacon_es.so (include/beacon_es.h): the C ABI, the layouts, the argument checks, and the float32 instantiation of the
// kernels of es_impl.h.  The float64 instantiation is es_f64.hip (built without FMA contraction).
#include <math.h>

#include "es_impl.h"

ES_DEFINE_LAUNCH(float)

static thread_local PolicyErr g_es_err;

// ---- cfg, geometry, layouts ------------------------------------------------------------------------------------------------------
static int es_n_out(const bcn_es_cfg* c) { return c->kind == BCN_ES_BOX ? c->act_dim : c->n_actions; }

static int es_nmax(const bcn_es_cfg* c) {
  int n = es_n_out(c);
  for (int l = 0; l < c->n_hidden; l++) n = c->hidden[l] > n ? c->hidden[l] : n;
  return n;
}

static int es_hp(const bcn_es_cfg* c) { return (es_nmax(c) + 3) & ~3; }

static size_t es_lds_at(const bcn_es_cfg* c, int G) {
  return c->dtype ? es_lds_bytes<double>(es_hp(c), es_nmax(c), G) : es_lds_bytes<float>(es_hp(c), es_nmax(c), G);
}

// the members per workgroup of the act launch (the header's rule); only for a cfg whose fields passed the range checks
static int es_group_of(const bcn_es_cfg* c) {
  if (c->group != 0) return c->group;
  const long long R = c->batch / c->members;
  long long g = BCN_ES_MAX_GROUP;
  if (BCN_ES_TILE_ROWS / R < g) g = BCN_ES_TILE_ROWS / R;
  if (c->members / 512 < g) g = c->members / 512;
  if (g < 1) g = 1;
  while (g > 1 && es_lds_at(c, (int)g) > (size_t)BCN_ES_LDS_LIMIT) g--;
  return (int)g;
}

// need_batch: with cfg.batch and cfg.members (everything but the parameter layout)
static bool es_cfg_ok(const bcn_es_cfg* c, bool need_batch) {
  PolicyErr* err = &g_es_err;
  if (!c) { err->set("cfg is NULL"); return false; }
  if (c->obs_dim < 1 || c->obs_dim > BCN_ES_MAX_OBS) { err->set("cfg.obs_dim = %d: must lie in 1 .. %d", c->obs_dim, BCN_ES_MAX_OBS); return false; }
  if (c->kind != BCN_ES_BOX && c->kind != BCN_ES_DISCRETE) { err->set("cfg.kind = %d: must be 0 (Box) or 1 (Discrete)", c->kind); return false; }
  if (c->kind == BCN_ES_BOX) {
    if (c->act_dim < 1 || c->act_dim > BCN_ES_MAX_ACT) { err->set("cfg.act_dim = %d: must lie in 1 .. %d", c->act_dim, BCN_ES_MAX_ACT); return false; }
    if (!(c->low <= c->high) || !isfinite(c->low) || !isfinite(c->high)) {
      err->set("cfg.low = %g, cfg.high = %g: need finite low <= high", c->low, c->high);
      return false;
    }
  } else if (c->n_actions < 2 || c->n_actions > BCN_ES_MAX_ACT) {
    err->set("cfg.n_actions = %d: must lie in 2 .. %d", c->n_actions, BCN_ES_MAX_ACT);
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
  if (c->group < 0 || c->group > BCN_ES_MAX_GROUP) { err->set("cfg.group = %d: must lie in 0 .. %d", c->group, BCN_ES_MAX_GROUP); return false; }
  if (!need_batch) return true;
  if (c->members < 2 || c->members > BCN_ES_MAX_MEMBERS || (c->members & 1)) {
    err->set("cfg.members = %d: must be even and lie in 2 .. %d (antithetic pairs)", c->members, BCN_ES_MAX_MEMBERS);
    return false;
  }
  if (c->batch < c->members || c->batch % c->members != 0) {
    err->set("cfg.batch = %d is no multiple of cfg.members = %d: every member runs the same number of replicas", c->batch, c->members);
    return false;
  }
  if (c->group > 1 && (long long)c->group * (c->batch / c->members) > BCN_ES_TILE_ROWS) {
    err->set("cfg.group = %d with %d replicas per member: the group's rows must fit a tile of %d", c->group, c->batch / c->members, BCN_ES_TILE_ROWS);
    return false;
  }
  const size_t lds = es_lds_at(c, es_group_of(c));
  if (lds > (size_t)BCN_ES_LDS_LIMIT) {
    err->set("cfg: the act launch needs %zu bytes of LDS for these widths and group = %d, the limit is %d", lds, es_group_of(c), BCN_ES_LDS_LIMIT);
    return false;
  }
  return true;
}

static size_t es_esz(const bcn_es_cfg* c) { return c->dtype ? 8 : 4; }

struct EsSegDesc { char name[16]; int elem; size_t n; };

static size_t es_lay(const EsSegDesc* d, int nd, size_t esz, bcn_es_seg* segs, int max_segs) {
  size_t off = 0;
  for (int k = 0; k < nd; k++) {
    off = (off + 15) & ~(size_t)15;
    if (segs && k < max_segs) {
      memset(&segs[k], 0, sizeof(segs[k]));
      strncpy(segs[k].name, d[k].name, sizeof(segs[k].name) - 1);
      segs[k].offset = off; segs[k].elem = d[k].elem; segs[k].planes = 0; segs[k].row_elems = (int64_t)d[k].n;
    }
    off += d[k].n * (d[k].elem == BCN_ES_REAL ? esz : d[k].elem == BCN_ES_F64 ? 8 : d[k].elem == BCN_ES_U8 ? 1 : 4);
  }
  return (off + 15) & ~(size_t)15;
}

static void es_desc(EsSegDesc* d, const char* name, int elem, size_t n) {
  memset(d, 0, sizeof(*d));
  strncpy(d->name, name, sizeof(d->name) - 1);
  d->elem = elem; d->n = n;
}

static int es_params_lay(const bcn_es_cfg* c, bcn_es_seg* segs, int max_segs, size_t* bytes) {
  EsSegDesc d[ES_MAX_PSEGS];
  int nd = 0;
  size_t in = (size_t)c->obs_dim;
  for (int l = 0; l <= c->n_hidden; l++) {
    const size_t out = l < c->n_hidden ? (size_t)c->hidden[l] : (size_t)es_n_out(c);
    char name[16];
    snprintf(name, sizeof(name), "pi_w%d", l);
    es_desc(&d[nd++], name, BCN_ES_REAL, out * in);
    snprintf(name, sizeof(name), "pi_b%d", l);
    es_desc(&d[nd++], name, BCN_ES_REAL, out);
    in = out;
  }
  *bytes = es_lay(d, nd, es_esz(c), segs, max_segs);
  return nd;
}

static size_t es_n_elems(const bcn_es_cfg* c) {
  size_t bytes;
  es_params_lay(c, nullptr, 0, &bytes);
  return bytes / es_esz(c);
}

static int es_chunks(const bcn_es_cfg* c) { return (c->members / 2 + BCN_ES_PAIR_CHUNK - 1) / BCN_ES_PAIR_CHUNK; }

#define ES_N_STATE 9
static int es_state_lay(const bcn_es_cfg* c, bcn_es_seg* segs, int max_segs, size_t* bytes) {
  EsSegDesc d[ES_N_STATE];
  const size_t n = es_n_elems(c), B = (size_t)c->batch, M = (size_t)c->members;
  es_desc(&d[0], "gen", BCN_ES_I32, 4);
  es_desc(&d[1], "fit", BCN_ES_F64, B);
  es_desc(&d[2], "len", BCN_ES_I32, B);
  es_desc(&d[3], "alive", BCN_ES_U8, B);
  es_desc(&d[4], "member_fit", BCN_ES_F64, M);
  es_desc(&d[5], "util", BCN_ES_F64, M);
  es_desc(&d[6], "stats", BCN_ES_F64, BCN_ES_N_STATS);
  es_desc(&d[7], "adam_m", BCN_ES_REAL, n);
  es_desc(&d[8], "adam_v", BCN_ES_REAL, n);
  *bytes = es_lay(d, ES_N_STATE, es_esz(c), segs, max_segs);
  return ES_N_STATE;
}

static int es_work_lay(const bcn_es_cfg* c, bcn_es_seg* segs, int max_segs, size_t* bytes) {
  EsSegDesc d[3];
  const size_t n = es_n_elems(c);
  es_desc(&d[0], "grad", BCN_ES_REAL, n);
  es_desc(&d[1], "norm2", BCN_ES_F64, (n + ES_NT - 1) / ES_NT);
  es_desc(&d[2], "partial", BCN_ES_F64, (size_t)es_chunks(c) * n);
  *bytes = es_lay(d, 3, es_esz(c), segs, max_segs);
  return 3;
}

static EsLayout es_layout_of(const bcn_es_cfg* c) {
  EsLayout L;
  memset(&L, 0, sizeof(L));
  bcn_es_seg s[ES_MAX_PSEGS];
  size_t bytes;
  L.n_segs = es_params_lay(c, s, ES_MAX_PSEGS, &bytes);
  for (int k = 0; k < L.n_segs; k++) {
    L.off[k] = (unsigned)(s[k].offset / es_esz(c));
    L.cnt[k] = (unsigned)s[k].row_elems;
  }
  L.E = (unsigned)(bytes / es_esz(c));
  return L;
}

struct EsState { char *gen, *fit, *len, *alive, *member_fit, *util, *stats, *m, *v; };
static EsState es_state_of(const bcn_es_cfg* c, void* state) {
  bcn_es_seg s[ES_N_STATE];
  size_t bytes;
  es_state_lay(c, s, ES_N_STATE, &bytes);
  char* p = static_cast<char*>(state);
  return EsState{p + s[0].offset, p + s[1].offset, p + s[2].offset, p + s[3].offset, p + s[4].offset,
                 p + s[5].offset, p + s[6].offset, p + s[7].offset, p + s[8].offset};
}

// ---- the argument blocks -----------------------------------------------------------------------------------------------------------
// the double launches live in es_f64.hip
template <> int es_launch_act<double>(const EsActArgs<double>& a, int grid, void* stream);
template <> int es_launch_begin<double>(const EsBeginArgs<double>& a, void* stream);
template <> int es_launch_observe<double>(long long B, double* fit, int32_t* len, uint8_t* alive, const double* rwd, const uint8_t* done,
                                          const uint8_t* trunc, void* stream);
template <> int es_launch_update<double>(const EsUpdateArgs<double>& a, void* stream);

template <typename real>
static int es_act_t(const bcn_es_cfg* c, const void* weights, int shared, const void* obs, const uint8_t* mask, void* actions, void* stream) {
  EsActArgs<real> A;
  memset(&A, 0, sizeof(A));
  A.weights = static_cast<const real*>(weights); A.obs = static_cast<const real*>(obs); A.mask = mask;
  A.actions = static_cast<real*>(actions); A.actions_i = static_cast<int32_t*>(actions);
  A.B = c->batch;
  A.M = shared ? 1 : c->members;
  A.R = shared ? (long long)c->batch : (long long)(c->batch / c->members);
  A.G = shared ? 1 : es_group_of(c);
  int grid;
  if (A.R > BCN_ES_TILE_ROWS) {
    A.G = 1;
    A.tiles = (A.R + BCN_ES_TILE_ROWS - 1) / BCN_ES_TILE_ROWS;
    long long split = (BCN_ES_WANT_GRID + A.M - 1) / A.M;
    split = split < A.tiles ? split : A.tiles;
    A.split = (int)split;
    grid = A.M * A.split;
  } else {
    A.tiles = 0; A.split = 1;
    grid = (A.M + A.G - 1) / A.G;
  }
  A.obs_dim = c->obs_dim; A.n_out = es_n_out(c); A.n_hidden = c->n_hidden; A.activation = c->activation; A.kind = c->kind;
  for (int l = 0; l < c->n_hidden; l++) A.hidden[l] = c->hidden[l];
  A.HP = es_hp(c); A.nmax = es_nmax(c);
  A.center = (real)((c->high + c->low) / 2.0); A.half = (real)((c->high - c->low) / 2.0);
  A.lay = es_layout_of(c);
  return es_launch_act<real>(A, grid, stream);
}

template <typename real>
static int es_begin_t(const bcn_es_cfg* c, const void* theta, void* pop, void* state, double sigma, uint64_t seed, void* stream) {
  const EsState s = es_state_of(c, state);
  EsBeginArgs<real> A;
  memset(&A, 0, sizeof(A));
  A.theta = static_cast<const real*>(theta); A.pop = static_cast<real*>(pop);
  A.gen = reinterpret_cast<const int32_t*>(s.gen); A.fit = reinterpret_cast<double*>(s.fit);
  A.len = reinterpret_cast<int32_t*>(s.len); A.alive = reinterpret_cast<uint8_t*>(s.alive);
  A.B = c->batch; A.M = c->members; A.sigma = (real)sigma;
  A.k0 = (uint32_t)(seed & 0xffffffffull); A.k1 = (uint32_t)(seed >> 32);
  A.lay = es_layout_of(c);
  return es_launch_begin<real>(A, stream);
}

template <typename real>
static int es_observe_t(const bcn_es_cfg* c, void* state, const void* rwd, const uint8_t* done, const uint8_t* trunc, void* stream) {
  const EsState s = es_state_of(c, state);
  return es_launch_observe<real>(c->batch, reinterpret_cast<double*>(s.fit), reinterpret_cast<int32_t*>(s.len), reinterpret_cast<uint8_t*>(s.alive),
                                 static_cast<const real*>(rwd), done, trunc, stream);
}

template <typename real>
static int es_update_t(const bcn_es_cfg* c, void* theta, void* state, void* work, const bcn_es_hyper* h, uint64_t seed, void* stream) {
  const EsState s = es_state_of(c, state);
  bcn_es_seg w[3];
  size_t bytes;
  es_work_lay(c, w, 3, &bytes);
  char* wp = static_cast<char*>(work);
  EsUpdateArgs<real> U;
  memset(&U, 0, sizeof(U));
  U.M = c->members; U.R = c->batch / c->members;
  U.fit = reinterpret_cast<const double*>(s.fit); U.member_fit = reinterpret_cast<double*>(s.member_fit);
  U.util = reinterpret_cast<double*>(s.util); U.stats = reinterpret_cast<double*>(s.stats);
  EsGradArgs<real>& g = U.g;
  g.theta = static_cast<real*>(theta); g.gen = reinterpret_cast<const int32_t*>(s.gen); g.util = U.util;
  g.grad = reinterpret_cast<real*>(wp + w[0].offset); g.norm2 = reinterpret_cast<double*>(wp + w[1].offset);
  g.partial = reinterpret_cast<double*>(wp + w[2].offset);
  g.M = c->members; g.chunks = es_chunks(c);
  g.denom = (double)c->members * (double)(real)h->sigma;
  g.weight_decay = (real)h->weight_decay;
  g.k0 = (uint32_t)(seed & 0xffffffffull); g.k1 = (uint32_t)(seed >> 32);
  g.lay = es_layout_of(c);
  Td3AdamArgs<real>& a = U.adam;
  a.params = static_cast<real*>(theta); a.grad = g.grad;
  a.m = reinterpret_cast<real*>(s.m); a.v = reinterpret_cast<real*>(s.v); a.step = reinterpret_cast<int32_t*>(s.gen);
  a.norm = U.stats + BCN_ES_STAT_GRAD_NORM;
  a.e0 = 0; a.e1 = (int)g.lay.E; a.which = 1;        // t = gen[1] + 1
  a.lr = h->lr; a.beta1 = h->beta1; a.beta2 = h->beta2; a.eps = h->eps; a.max_grad_norm = h->max_grad_norm;
  return es_launch_update<real>(U, stream);
}

static int es_hip(const char* fn, int e) {
  if (e) { g_es_err.set("%s: launch -> %s", fn, hipGetErrorString((hipError_t)e)); return BCN_ES_ERR_HIP; }
  return BCN_ES_OK;
}

static bool es_aligned(const char* fn, const char* name, const void* p) {
  if (!p) { g_es_err.set("%s: %s is NULL", fn, name); return false; }
  if (reinterpret_cast<uintptr_t>(p) & 15) { g_es_err.set("%s: %s is not 16-byte aligned", fn, name); return false; }
  return true;
}

extern "C" {

BCN_ES_API const char* bcn_es_last_error(void) { return g_es_err.text; }

BCN_ES_API int bcn_es_params_layout(const bcn_es_cfg* cfg, bcn_es_seg* segs, int max_segs) {
  size_t bytes;
  return es_cfg_ok(cfg, false) ? es_params_lay(cfg, segs, max_segs, &bytes) : 0;
}
BCN_ES_API size_t bcn_es_params_bytes(const bcn_es_cfg* cfg) {
  size_t bytes = 0;
  if (es_cfg_ok(cfg, false)) es_params_lay(cfg, nullptr, 0, &bytes);
  return bytes;
}
BCN_ES_API int bcn_es_state_layout(const bcn_es_cfg* cfg, bcn_es_seg* segs, int max_segs) {
  size_t bytes;
  return es_cfg_ok(cfg, true) ? es_state_lay(cfg, segs, max_segs, &bytes) : 0;
}
BCN_ES_API size_t bcn_es_state_bytes(const bcn_es_cfg* cfg) {
  size_t bytes = 0;
  if (es_cfg_ok(cfg, true)) es_state_lay(cfg, nullptr, 0, &bytes);
  return bytes;
}
BCN_ES_API int bcn_es_work_layout(const bcn_es_cfg* cfg, bcn_es_seg* segs, int max_segs) {
  size_t bytes;
  return es_cfg_ok(cfg, true) ? es_work_lay(cfg, segs, max_segs, &bytes) : 0;
}
BCN_ES_API size_t bcn_es_work_bytes(const bcn_es_cfg* cfg) {
  size_t bytes = 0;
  if (es_cfg_ok(cfg, true)) es_work_lay(cfg, nullptr, 0, &bytes);
  return bytes;
}
BCN_ES_API int bcn_es_group(const bcn_es_cfg* cfg) { return es_cfg_ok(cfg, true) ? es_group_of(cfg) : 0; }
BCN_ES_API size_t bcn_es_lds_bytes(const bcn_es_cfg* cfg) { return es_cfg_ok(cfg, true) ? es_lds_at(cfg, es_group_of(cfg)) : 0; }

BCN_ES_API int bcn_es_begin(const bcn_es_cfg* cfg, const void* theta_dev, void* pop_dev, void* state_dev, double sigma, uint64_t seed,
                            void* stream) {
  const char* fn = "bcn_es_begin";
  if (!es_cfg_ok(cfg, true)) return BCN_ES_ERR_ARG;
  if (!es_aligned(fn, "theta_dev", theta_dev) || !es_aligned(fn, "pop_dev", pop_dev) || !es_aligned(fn, "state_dev", state_dev)) return BCN_ES_ERR_ARG;
  if (!(sigma >= 0.0) || !isfinite(sigma)) { g_es_err.set("%s: sigma = %g: must be finite and >= 0", fn, sigma); return BCN_ES_ERR_ARG; }
  return es_hip(fn, cfg->dtype ? es_begin_t<double>(cfg, theta_dev, pop_dev, state_dev, sigma, seed, stream)
                               : es_begin_t<float>(cfg, theta_dev, pop_dev, state_dev, sigma, seed, stream));
}

BCN_ES_API int bcn_es_act(const bcn_es_cfg* cfg, const void* weights_dev, int shared, const void* obs_dev, const uint8_t* mask_dev,
                          void* actions_dev, void* stream) {
  const char* fn = "bcn_es_act";
  if (!es_cfg_ok(cfg, true)) return BCN_ES_ERR_ARG;
  if (!es_aligned(fn, "weights_dev", weights_dev)) return BCN_ES_ERR_ARG;
  if (shared != 0 && shared != 1) { g_es_err.set("%s: shared = %d: must be 0 or 1", fn, shared); return BCN_ES_ERR_ARG; }
  if (!obs_dev) { g_es_err.set("%s: obs_dev is NULL", fn); return BCN_ES_ERR_ARG; }
  if (!actions_dev) { g_es_err.set("%s: actions_dev is NULL", fn); return BCN_ES_ERR_ARG; }
  return es_hip(fn, cfg->dtype ? es_act_t<double>(cfg, weights_dev, shared, obs_dev, mask_dev, actions_dev, stream)
                               : es_act_t<float>(cfg, weights_dev, shared, obs_dev, mask_dev, actions_dev, stream));
}

BCN_ES_API int bcn_es_observe(const bcn_es_cfg* cfg, void* state_dev, const void* rwd_dev, const uint8_t* done_dev, const uint8_t* trunc_dev,
                              void* stream) {
  const char* fn = "bcn_es_observe";
  if (!es_cfg_ok(cfg, true)) return BCN_ES_ERR_ARG;
  if (!es_aligned(fn, "state_dev", state_dev)) return BCN_ES_ERR_ARG;
  if (!rwd_dev) { g_es_err.set("%s: rwd_dev is NULL", fn); return BCN_ES_ERR_ARG; }
  if (!done_dev) { g_es_err.set("%s: done_dev is NULL", fn); return BCN_ES_ERR_ARG; }
  if (!trunc_dev) { g_es_err.set("%s: trunc_dev is NULL", fn); return BCN_ES_ERR_ARG; }
  return es_hip(fn, cfg->dtype ? es_observe_t<double>(cfg, state_dev, rwd_dev, done_dev, trunc_dev, stream)
                               : es_observe_t<float>(cfg, state_dev, rwd_dev, done_dev, trunc_dev, stream));
}

BCN_ES_API int bcn_es_update(const bcn_es_cfg* cfg, void* theta_dev, void* state_dev, void* work_dev, const bcn_es_hyper* h, uint64_t seed,
                             void* stream) {
  const char* fn = "bcn_es_update";
  if (!es_cfg_ok(cfg, true)) return BCN_ES_ERR_ARG;
  if (!es_aligned(fn, "theta_dev", theta_dev) || !es_aligned(fn, "state_dev", state_dev) || !es_aligned(fn, "work_dev", work_dev)) return BCN_ES_ERR_ARG;
  if (!h) { g_es_err.set("%s: hyper is NULL", fn); return BCN_ES_ERR_ARG; }
  if (!(h->sigma > 0.0) || !isfinite(h->sigma) || (cfg->dtype == 0 && !((float)h->sigma > 0.0f))) {
    g_es_err.set("%s: hyper.sigma = %g: must be finite and > 0 (the gradient divides by it)", fn, h->sigma);
    return BCN_ES_ERR_ARG;
  }
  if (!(h->lr >= 0.0)) { g_es_err.set("%s: hyper.lr = %g: must be >= 0", fn, h->lr); return BCN_ES_ERR_ARG; }
  if (!(h->beta1 >= 0.0 && h->beta1 < 1.0) || !(h->beta2 >= 0.0 && h->beta2 < 1.0)) {
    g_es_err.set("%s: hyper.beta1 = %g, hyper.beta2 = %g: must lie in [0, 1)", fn, h->beta1, h->beta2);
    return BCN_ES_ERR_ARG;
  }
  // Adam runs over the gaps too, where grad = m = v = 0: with eps = 0 the step there would be 0 / 0
  if (!(h->eps > 0.0) || (cfg->dtype == 0 && !((float)h->eps > 0.0f))) { g_es_err.set("%s: hyper.eps = %g: must be > 0 (in real)", fn, h->eps); return BCN_ES_ERR_ARG; }
  if (!isfinite(h->max_grad_norm)) { g_es_err.set("%s: hyper.max_grad_norm = %g: must be finite (<= 0: off)", fn, h->max_grad_norm); return BCN_ES_ERR_ARG; }
  if (!(h->weight_decay >= 0.0) || !isfinite(h->weight_decay)) { g_es_err.set("%s: hyper.weight_decay = %g: must be finite and >= 0", fn, h->weight_decay); return BCN_ES_ERR_ARG; }
  return es_hip(fn, cfg->dtype ? es_update_t<double>(cfg, theta_dev, state_dev, work_dev, h, seed, stream)
                               : es_update_t<float>(cfg, theta_dev, state_dev, work_dev, h, seed, stream));
}

}  // extern "C"
