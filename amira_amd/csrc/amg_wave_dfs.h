// amg_wave_dfs.h — the bounded search for simple paths of the live graph (new_find_paths_between_nodes, reference
// construct_graph.py:2292-2342), executed COOPERATIVELY by one wave.  Control flow is uniform; stack level d lives in
// the registers of lane d (node, direction, row cursor, row limit, row offset), levels are read with v_readlane, and
// the "already on the path" test is one ballot.  (A one-lane search with its stack in LDS or scratch spends its time
// in dependent LDS/scratch round trips.)  A path follows the forward list of a node taken in direction +1, the
// backward list in direction -1, in list order.
//
// What happens at a node is the caller's: visit.enter(d, L, cur_node, cur_dir, my_node, my_dir) is called once per node
// entered, at depth d with L = d + 1 nodes on the path; (cur_node, cur_dir) is the node entered, wave-uniform, and
// (my_node, my_dir) is the CALLING LANE's own level, so lanes 0 .. L - 1 can write the path out at once.  It answers
//   WD_EXPAND   go on through the node's list,
//   WD_RETREAT  this node ends the path (accepted or too long): back to the level before,
//   WD_ABORT    the whole search ends here.
// Users: the re-threading (amg_gap_memo.hip: k_gap_dfs, k_gap_dfs_lanes; amg_gap_fast.hip: k_corr_gapped_fast) and the
// junction search (amg_bubbles.hip: k_bj_dfs).
#pragma once
#include "amg_device.h"

enum { WD_EXPAND = 0, WD_RETREAT = 1, WD_ABORT = 2 };

template <class Visit>
__device__ __forceinline__ void wave_dfs(const GView& g, int start, int start_dir, int lane, Visit& visit) {
  int my_node = 0, my_dir = 0, my_cur = 0, my_lim = 0, my_off = 0;
  if (lane == 0) {
    my_node = start;
    my_dir = start_dir;
  }
  int depth = 0;
  bool entering = true;
  // A row record carries the row's first entry {z, w} next to {offset, live count}: the row just entered needs no
  // load from lent for it.  This cannot change what is found: every writer of a row record stores lent[offset] and
  // {z, w} from the same values (k_lr_fill, k_lr_finish, k_lr_long, k_lr_patch in amg_live_rows.hip).
  int2 first_ent = make_int2(-1, 0);
  while (depth >= 0) {
    const int d = __builtin_amdgcn_readfirstlane(depth);
    if (entering) {
      entering = false;
      const int cur_node = __builtin_amdgcn_readlane(my_node, d);
      const int cur_dir = __builtin_amdgcn_readlane(my_dir, d);
      const int step = visit.enter(d, d + 1, cur_node, cur_dir, my_node, my_dir);
      if (step == WD_ABORT) break;
      if (step == WD_RETREAT) {
        --depth;
        first_ent.x = -1;
        continue;
      }
      const int4 rw = g.lrows[2ll * cur_node + (cur_dir == 1 ? 0 : 1)];  // uniform address
      if (lane == d) {
        my_cur = 0;
        my_lim = rw.y;
        my_off = rw.x;
      }
      first_ent = make_int2(rw.z, rw.w);
    }
    int c = __builtin_amdgcn_readlane(my_cur, d);
    const int lim = __builtin_amdgcn_readlane(my_lim, d);
    const int row_off = __builtin_amdgcn_readlane(my_off, d);
    bool pushed = false;
    while (c < lim) {
      int2 ent = first_ent;
      if (!(c == 0 && first_ent.x >= 0)) ent = g.lent[row_off + c];  // uniform address
      ++c;
      const int t = __builtin_amdgcn_readfirstlane(ent.x);
      const int td = __builtin_amdgcn_readfirstlane(ent.y);
      if (__ballot(lane <= d && my_node == t) != 0ull) continue;  // no node twice on a path (:2327)
      if (lane == d) my_cur = c;
      if (lane == d + 1) {
        my_node = t;
        my_dir = td;
      }
      ++depth;
      entering = true;
      pushed = true;
      break;
    }
    if (!pushed) {
      --depth;
      first_ent.x = -1;  // back in an older row: its first entry was consumed long ago
    }
  }
}
