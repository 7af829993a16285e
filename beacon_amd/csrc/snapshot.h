// snapshot.h -- segment table of the snapshot copy kernels (snapshot.hip; include/beacon_hip.h: bcn_snapshot_*).
//
// A snapshot is one device byte buffer holding, for n replicas, every array a handle reads in its next *_step plus the packed
// outputs of its last call.  The kernels move bytes only: ONE launch copies every segment, handle -> snapshot (save) or
// snapshot -> handle with a per-replica source index and mask (load).  The table travels by value in the kernel arguments.
#pragma once
#include "bcn_common.h"

#define BCN_SNAP_MAX_SEG 32       // table entries: one per plane of a named segment (vortex: 14 state columns + stp + 5 outputs)
#define BCN_SNAP_NT 256           // threads per workgroup
#define BCN_SNAP_TILE 16384u      // bytes of a long row one workgroup copies: 256 lanes x 4 x 16 B
#define BCN_SNAP_LONG_ROW 1024u   // rows of at least this many bytes get workgroups of their own (tiles); shorter ones share them

// One named segment of a packed device buffer -- a snapshot, or a bookkeeping buffer (episode.h, shkadov_jets.h, normalize.h): `planes`
// arrays of [replicas][row_elems] elements of kind `elem` (BCN_SNAP_*) one behind the other; planes = 0: ONE array of row_elems
// elements that does not scale with the replicas.  seg_layout (capi.hip) lays a table of these out.
struct SegDesc { const char* name; int elem; int planes; size_t row_elems; };

// One array of the handle: replica b's row is dev + b * row_bytes (rows are contiguous in every handle array), and
// snap_off + b * row_bytes in a snapshot.
struct SnapSeg {
  char* dev;
  unsigned long long snap_off;    // of row 0, for the replica count the table was built for
  unsigned row_bytes;
  unsigned blk0;                  // first workgroup of this entry
  unsigned bpr;                   // long rows: workgroups per row; 0: short rows, BCN_SNAP_NT * 4 units per workgroup
  unsigned unit;                  // short rows: bytes one lane copies at a time (16, 8, 4 or 1; divides row_bytes)
};

struct SnapTable {
  int nseg;
  int batch;                      // replicas of the handle
  int n_src;                      // replicas of the snapshot (load; == batch on save)
  unsigned nblk;                  // workgroups in all
  SnapSeg seg[BCN_SNAP_MAX_SEG];
};

// save: snap <- handle, every replica.  load: handle replica b <- snapshot replica src[b] (src NULL: b) where mask[b] != 0
// (mask NULL: all) and 0 <= src[b] < n_src; other replicas are left untouched.
int snapshot_launch(const SnapTable& t, bool load, char* snap, const int32_t* src, const uint8_t* mask, hipStream_t s);
