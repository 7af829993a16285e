// episode.h -- argument block of the episode bookkeeping kernel (episode.hip; include/beacon_hip.h: bcn_episode_*).
//
// One packed episode buffer of the caller holds, for the handle's B replicas, nine segments (every start a multiple of 16 bytes):
//   ret real [B], len int32 [B]            the running return and length of the episode in progress
//   last_ret real [B], last_len int32 [B]  those of the last finished episode
//   count int32 [B], sum_ret float64 [B], sum_len int64 [B]   finished episodes and the sums of their returns and lengths
//   finished uint8 [B]                     1 where the step just tracked ended an episode: the mask of the reset that follows
//   final_obs real [B][n_obs]              the observation of the terminal step (rows of finished replicas only are written)
// The kernel reads the packed outputs of a step [obs | rwd | status | done | trunc] and updates the buffer in ONE launch.
#pragma once
#include "bcn_common.h"
#include "snapshot.h"

#define BCN_EP_NT 256             // threads per workgroup
#define BCN_EP_UPL 4              // copy workgroups: units of the flattened [replica][unit] space per lane
#define BCN_EP_NSEG 9

// The segments in buffer order: the host addresses them by these names, never by number.
enum { EP_RET, EP_LEN, EP_LAST_RET, EP_LAST_LEN, EP_COUNT, EP_SUM_RET, EP_SUM_LEN, EP_FINISHED, EP_FINAL_OBS, EP_NSEG_ };
static_assert(EP_NSEG_ == BCN_EP_NSEG, "episode.h: the enum and BCN_EP_NSEG disagree");
inline void episode_segs(size_t n_obs, SegDesc* d) {
  d[EP_RET] = {"ret", BCN_SNAP_REAL, 1, 1};           d[EP_LEN] = {"len", BCN_SNAP_I32, 1, 1};
  d[EP_LAST_RET] = {"last_ret", BCN_SNAP_REAL, 1, 1}; d[EP_LAST_LEN] = {"last_len", BCN_SNAP_I32, 1, 1};
  d[EP_COUNT] = {"count", BCN_SNAP_I32, 1, 1};        d[EP_SUM_RET] = {"sum_ret", BCN_SNAP_F64, 1, 1};
  d[EP_SUM_LEN] = {"sum_len", BCN_SNAP_I64, 1, 1};    d[EP_FINISHED] = {"finished", BCN_SNAP_U8, 1, 1};
  d[EP_FINAL_OBS] = {"final_obs", BCN_SNAP_REAL, 1, n_obs};
}

struct EpisodeArgs {
  // the step's outputs
  const char* obs;
  const void* rwd;
  const uint8_t* done;
  const uint8_t* trunc;
  const uint8_t* mask;            // NULL: every replica
  // the episode buffer
  void* ret;
  int32_t* len;
  void* last_ret;
  int32_t* last_len;
  int32_t* count;
  double* sum_ret;
  long long* sum_len;
  uint8_t* finished;
  char* final_obs;
  unsigned batch;
  unsigned nbk;                   // bookkeeping workgroups: ceil(batch / BCN_EP_NT); the rest copy
  unsigned unit;                  // bytes one lane copies at a time: 16, 8 or 4, the largest that divides a row
  unsigned upr;                   // units per observation row
  unsigned total;                 // batch * upr
  int f64;                        // the env's dtype
};

int episode_launch(const EpisodeArgs& a, hipStream_t s);
