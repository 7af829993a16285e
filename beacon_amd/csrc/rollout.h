// rollout.h -- argument blocks of the rollout storage and GAE kernels (rollout.hip; include/beacon_hip.h: bcn_rollout_*).
//
// One packed rollout buffer of the caller holds, for T steps of the handle's B replicas, twelve segments (every start a multiple of
// 16 bytes; [T] stands for T planes of B rows one behind the other, as "fields" in a snapshot):
//   cursor int32 [4]                                  [0] steps recorded so far, [1] sticky overflow flag
//   obs real [T + 1][B][n_obs]                        obs[0]: what bcn_rollout_begin found; obs[t + 1]: what step t returned
//   act real [T][B][n_act] or int32 [T][B]            the actions handed to step t, in the element type the step takes
//   rwd real [T][B], status int32 [T][B], done, trunc, valid uint8 [T][B]
//   final_obs real [T][B][n_obs]   (BCN_RO_FINAL_OBS) the terminal observation of the replicas that finished in step t
//   rwd_jets real [T][B][n_jets]   (BCN_RO_JETS)      the per-jet rewards of step t
//   adv, ret real [T][B cols]                         written by bcn_rollout_gae; sized for cols = n_jets with BCN_RO_JETS, else 1
// A segment whose flag is off has rows of zero elements: the names and their order never change.
#pragma once
#include "bcn_common.h"
#include "snapshot.h"

#define BCN_RO_NT 256             // threads per workgroup
#define BCN_RO_UPL 4              // copy workgroups: units of the flattened [replica][unit] space per lane
#define BCN_RO_NSEG 12
#define BCN_RO_NJOB 4             // row copies of one record: obs, final_obs, act, rwd_jets
#define BCN_RO_GAE_AHEAD 4        // steps of the GAE recurrence whose loads are issued before the first of them is used

// The segments in buffer order: the host addresses them by these names, never by number.
enum { RO_CURSOR, RO_OBS, RO_ACT, RO_RWD, RO_STATUS, RO_DONE, RO_TRUNC, RO_VALID, RO_FINAL_OBS, RO_RWD_JETS, RO_ADV, RO_RET, RO_NSEG_ };
static_assert(RO_NSEG_ == BCN_RO_NSEG, "rollout.h: the enum and BCN_RO_NSEG disagree");
// act_elem: BCN_SNAP_REAL or BCN_SNAP_I32; n_jets: of a shkadov handle (used with BCN_RO_JETS only)
inline void rollout_segs(int T, size_t n_obs, int act_elem, size_t act_dim, size_t n_jets, int flags, SegDesc* d) {
  const size_t fo = (flags & BCN_RO_FINAL_OBS) ? n_obs : 0, nj = (flags & BCN_RO_JETS) ? n_jets : 0, cols = nj ? nj : 1;
  d[RO_CURSOR] = {"cursor", BCN_SNAP_I32, 0, 4};          d[RO_OBS] = {"obs", BCN_SNAP_REAL, T + 1, n_obs};
  d[RO_ACT] = {"act", act_elem, T, act_dim};              d[RO_RWD] = {"rwd", BCN_SNAP_REAL, T, 1};
  d[RO_STATUS] = {"status", BCN_SNAP_I32, T, 1};          d[RO_DONE] = {"done", BCN_SNAP_U8, T, 1};
  d[RO_TRUNC] = {"trunc", BCN_SNAP_U8, T, 1};             d[RO_VALID] = {"valid", BCN_SNAP_U8, T, 1};
  d[RO_FINAL_OBS] = {"final_obs", BCN_SNAP_REAL, T, fo};  d[RO_RWD_JETS] = {"rwd_jets", BCN_SNAP_REAL, T, nj};
  d[RO_ADV] = {"adv", BCN_SNAP_REAL, T, cols};            d[RO_RET] = {"ret", BCN_SNAP_REAL, T, cols};
}

// One row copy of a record: unit e of the flattened [replica][unit] space of the source goes to dst + slot * slot_bytes + e * unit.
enum { RO_COPY_ALWAYS, RO_COPY_FINISHED, RO_COPY_STEPPED };
struct RolloutJob {
  const char* src;                // RO_COPY_STEPPED: NULL writes zeros
  char* dst;                      // slot 0 of the segment
  unsigned long long slot_bytes;  // B * row bytes
  unsigned unit;                  // bytes one lane copies at a time: 16, 8 or 4, the largest that divides a row
  unsigned upr;                   // units per row
  unsigned total;                 // B * upr; 0: the job is off
  unsigned blk0;                  // its first copy workgroup (the jobs that are off carry the count of all copy workgroups)
  int when;                       // RO_COPY_*
  int slot_off;                   // obs: 1 (step t writes obs[t + 1])
};

struct RolloutRecordArgs {
  int32_t* cursor;
  // the step's outputs (rwd: the normaliser's norm_rwd when one is passed)
  const void* rwd;
  const int32_t* status;
  const uint8_t* done;
  const uint8_t* trunc;
  const uint8_t* mask;            // NULL: every replica
  const uint8_t* finished;        // of the episode buffer; NULL: no terminal observations
  // slot 0 of the [T][B] columns
  void* d_rwd;
  int32_t* d_status;
  uint8_t* d_done;
  uint8_t* d_trunc;
  uint8_t* d_valid;
  RolloutJob job[BCN_RO_NJOB];
  unsigned batch;
  unsigned nbk;                   // column workgroups: ceil(batch / BCN_RO_NT); the rest copy
  unsigned ncp;                   // copy workgroups
  int T;
  int f64;                        // the env's dtype
};

struct RolloutGaeArgs {
  const int32_t* cursor;
  const void* rwd;                // [T][ncols]: the rwd segment, or rwd_jets with cols = n_jets
  const uint8_t* done;            // [T][B]
  const uint8_t* trunc;
  const uint8_t* valid;
  const void* values;             // [T][ncols]
  const void* last_value;         // [ncols]
  const void* final_values;       // [T][ncols]; NULL: no bootstrap on truncation
  void* adv;                      // [T][ncols]
  void* ret;
  unsigned batch, cols, ncols;    // ncols = batch * cols
  int T;
  int f64;
  double gamma, lam;
};

// cursor = 0, overflow = 0, obs[0] <- src: ONE launch
int rollout_begin_launch(int32_t* cursor, const RolloutJob& obs, hipStream_t s);
// the record and, behind it, the one-lane launch that advances the cursor
int rollout_record_launch(const RolloutRecordArgs& a, hipStream_t s);
int rollout_gae_launch(const RolloutGaeArgs& a, hipStream_t s);
