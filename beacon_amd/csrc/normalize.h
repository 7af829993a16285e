// normalize.h -- argument block of the running-normalisation kernels (normalize.hip; include/beacon_hip.h: bcn_normalize*).
//
// One packed normaliser buffer of the caller holds, for the handle's B replicas of n_obs observations, eleven segments (every
// start a multiple of 16 bytes):
//   obs_mean, obs_var float64 [n_obs], obs_count float64 [1]   the running statistics of every observation column
//   ret_mean, ret_var, ret_count float64 [1]                   those of the discounted return
//   ret float64 [B]                                            the discounted return of every replica
//   norm_obs real [B][n_obs], norm_rwd real [B], norm_final_obs real [B][n_obs]   the outputs
//   scratch                                                    private: a copy of the statistics in front of the update and the
//                                                              per-workgroup partials (count, mean, M2) of every column
// The kernels read the packed outputs of a step [obs | rwd | status | done | trunc] and, optionally, finished / final_obs of an
// episode buffer (episode.h).
#pragma once
#include "bcn_common.h"
#include "snapshot.h"

#define BCN_NRM_NT 256            // threads per workgroup
#define BCN_NRM_W 64              // columns a workgroup covers at most: rows longer than this are cut into chunks
#define BCN_NRM_MAXG 256          // replica slabs at most
#define BCN_NRM_NSEG 11
#define BCN_NRM_STEP 0            // kind
#define BCN_NRM_RESET 1

struct NormalizeArgs {
  // the step's outputs
  const void* obs;
  const void* rwd;
  const int32_t* status;
  const uint8_t* done;
  const uint8_t* trunc;
  const uint8_t* mask;            // NULL: every replica
  // of the episode buffer; NULL: no terminal observations
  const uint8_t* finished;
  const void* final_obs;
  // the normaliser buffer
  double* obs_mean;
  double* obs_var;
  double* obs_count;
  double* ret_mean;
  double* ret_var;
  double* ret_count;
  double* ret;
  void* norm_obs;
  void* norm_rwd;
  void* norm_final_obs;
  double* prev;                   // scratch: mean [n_obs + 1], var [n_obs + 1], count [2] in front of the update (column n_obs: the return)
  double* part;                   // scratch: [G][n_obs + 1][3] (count, mean, M2) of slab g and column c
  unsigned batch, n_obs;
  unsigned w;                     // columns per chunk: min(n_obs, BCN_NRM_W)
  unsigned R;                     // replicas a workgroup covers per trip: BCN_NRM_NT / w
  unsigned chunks;                // ceil(n_obs / w); workgroups [0, chunks) of a slab take observations, workgroup `chunks` the return
  unsigned S, G;                  // replicas per slab, slabs
  int f64;                        // the env's dtype
  int kind;                       // BCN_NRM_STEP / BCN_NRM_RESET
  int training;
  double gamma, eps, clip_obs, clip_rwd;
};

// What bcn_normalize_layout and the launch agree on: the shape of the decomposition for a batch and a row length.
struct NormalizeShape { unsigned w, R, chunks, S, G; };
inline NormalizeShape normalize_shape(size_t batch, size_t n_obs) {
  NormalizeShape s;
  s.w = (unsigned)(n_obs < BCN_NRM_W ? n_obs : BCN_NRM_W);
  s.R = BCN_NRM_NT / s.w;
  s.chunks = (unsigned)((n_obs + s.w - 1) / s.w);
  // slabs: no more than BCN_NRM_MAXG, no more than 8 R (so that the R lanes of a column merge at most 8 partials each), and at
  // least 4 R replicas in each
  size_t g = batch / (4 * (size_t)s.R);
  if (g > 8 * (size_t)s.R) g = 8 * (size_t)s.R;
  if (g > BCN_NRM_MAXG) g = BCN_NRM_MAXG;
  if (g < 1) g = 1;
  s.S = (unsigned)((batch + g - 1) / g);
  s.G = (unsigned)((batch + s.S - 1) / s.S);
  return s;
}

// The segments in buffer order: the host addresses them by these names, never by number.
enum { NRM_OBS_MEAN, NRM_OBS_VAR, NRM_OBS_COUNT, NRM_RET_MEAN, NRM_RET_VAR, NRM_RET_COUNT, NRM_RET, NRM_NORM_OBS, NRM_NORM_RWD,
       NRM_NORM_FINAL_OBS, NRM_SCRATCH, NRM_NSEG_ };
static_assert(NRM_NSEG_ == BCN_NRM_NSEG, "normalize.h: the enum and BCN_NRM_NSEG disagree");
inline void normalize_segs(size_t batch, size_t n_obs, SegDesc* d) {
  const size_t scratch = ((2 * (n_obs + 1) + 2) + (size_t)normalize_shape(batch, n_obs).G * (n_obs + 1) * 3) * 8;   // prev + part, in bytes
  d[NRM_OBS_MEAN] = {"obs_mean", BCN_SNAP_F64, 0, n_obs}; d[NRM_OBS_VAR] = {"obs_var", BCN_SNAP_F64, 0, n_obs};
  d[NRM_OBS_COUNT] = {"obs_count", BCN_SNAP_F64, 0, 1};   d[NRM_RET_MEAN] = {"ret_mean", BCN_SNAP_F64, 0, 1};
  d[NRM_RET_VAR] = {"ret_var", BCN_SNAP_F64, 0, 1};       d[NRM_RET_COUNT] = {"ret_count", BCN_SNAP_F64, 0, 1};
  d[NRM_RET] = {"ret", BCN_SNAP_F64, 1, 1};               d[NRM_NORM_OBS] = {"norm_obs", BCN_SNAP_REAL, 1, n_obs};
  d[NRM_NORM_RWD] = {"norm_rwd", BCN_SNAP_REAL, 1, 1};    d[NRM_NORM_FINAL_OBS] = {"norm_final_obs", BCN_SNAP_REAL, 1, n_obs};
  d[NRM_SCRATCH] = {"scratch", BCN_SNAP_U8, 0, scratch};
}

int normalize_launch(const NormalizeArgs& a, hipStream_t s);
