// plan.h -- what render.hip and windows.hip need of the batch planner
// (plan.hip): the carved workspace and plan_all().
#pragma once
#include "gsky_device.h"
#include "render.h"
#include "render_common.h"

namespace gsky {

// The arrays of a planned batch inside the caller's workspace.
struct Carve {
  PairPlan *pairs; Xform *xforms; TilePlan *tplans; int32_t *order; int32_t *pair_tile;
  RowRec *rows; RowFix *rowfix; Leaf *pool; int32_t *counters; MinMax *minmax; int64_t *split_list; int32_t *complex_list;
  EntryD *entries;
  SepCol *sepcols;
  int pool_cap;
  int64_t total;
};

Carve carve(void *base, int n_tiles, int n_pairs, int max_h);

// Plans rc's batch into its workspace (async on rc.stream); cv: its arrays.
// fill_rgba: the RGBA output of a call whose pair-less tiles the planner
// launches may write (launch_render's eligibility test), else NULL.  *filled
// = true exactly when both fill-carrying launches were issued.
int plan_all(const RenderCall &rc, Carve &cv, uint8_t *fill_rgba = nullptr, bool *filled = nullptr);

}  // namespace gsky
