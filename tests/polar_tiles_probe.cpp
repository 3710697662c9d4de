// Test hook for csrc/polar_tiles.cpp (compiled by tests/test_polar_tiles_host.py into its own shared object with g++; the libraries export the C ABI only).
// A batch plan is built for cones of the given sides (off = 7 i, kind = i % 3, idx = 100 + i: the pass-through members) and handed out as raw arrays
// of the device descriptors; the caller sizes its buffers from polar_probe_sizes.
#include <string.h>
#include "polar_tiles.h"

extern "C" {

// nullptr: the planner refused the batch
void* polar_probe_batch(int n, const int* d, int ts96, int flat, int ragged, int pair, int sort) {
  std::vector<PolarBatchIn> in;
  for (int i = 0; i < n; ++i) in.push_back(PolarBatchIn{d[i], 7 * i, i % 3, 100 + i});
  PolarTileOpts o;
  o.ts96 = ts96; o.flat = flat; o.ragged = ragged; o.pair = pair; o.sort = sort;
  PolarBatchPlan* bp = new PolarBatchPlan();
  if (polar_plan_batch(in, o, *bp)) { delete bp; return nullptr; }
  return bp;
}
void polar_probe_free(void* plan) { delete static_cast<PolarBatchPlan*>(plan); }

// out = {cones, qtiles, nbtiles, nbtiles96, rtiles, items, pairs, df_ntiles, work}
void polar_probe_sizes(const void* plan, long long out[9]) {
  const PolarBatchPlan& bp = *static_cast<const PolarBatchPlan*>(plan);
  const long long v[9] = {(long long)bp.cones.size(), (long long)bp.qtiles.size(), bp.nbtiles, bp.nbtiles96, (long long)bp.rtiles.size(),
                          (long long)bp.items.size(), (long long)bp.pairs.size(), bp.df_ntiles, bp.work};
  memcpy(out, v, sizeof v);
}

// which: 0 BatchCone table, 1 quadrant list, 2 interleaved RTile list, 3 RTile items, 4 RPair items, 5 xoff[9], 6 cone_nt, 7 {flops performed, useful}
void polar_probe_copy(const void* plan, int which, void* dst) {
  const PolarBatchPlan& bp = *static_cast<const PolarBatchPlan*>(plan);
  const double flops[2] = {bp.flops_performed, bp.flops_useful};
  auto copy = [&](const void* src, size_t bytes) { if (bytes) memcpy(dst, src, bytes); };
  switch (which) {
    case 0: copy(bp.cones.data(), sizeof(BatchCone) * bp.cones.size()); break;
    case 1: copy(bp.qtiles.data(), sizeof(QTile) * bp.qtiles.size()); break;
    case 2: copy(bp.rtiles.data(), sizeof(RTile) * bp.rtiles.size()); break;
    case 3: copy(bp.items.data(), sizeof(RTile) * bp.items.size()); break;
    case 4: copy(bp.pairs.data(), sizeof(RPair) * bp.pairs.size()); break;
    case 5: copy(bp.xoff, sizeof bp.xoff); break;
    case 6: copy(bp.cone_nt.data(), sizeof(int) * bp.cone_nt.size()); break;
    case 7: copy(flops, sizeof flops); break;
  }
}

// out = {ts, sk, ld, skg, skc} of a large cone of side d
void polar_probe_large(int d, int streamk, int ts, int sk, long long skg, int out[5]) {
  PolarTileOpts o;
  o.streamk = streamk; o.ts = ts; o.sk = sk; o.skg = skg;
  PolarCone pc;
  memset(&pc, 0, sizeof pc);
  pc.d = d;
  polar_plan_large(o, pc);
  out[0] = pc.ts; out[1] = pc.sk; out[2] = pc.ld; out[3] = pc.skg; out[4] = pc.skc;
}

long long polar_probe_cost(int d, int ext) { return polar_tile_cost(d, ext); }

// replays verification results (1 = failed) on a LiftDepth; out[3 t ...] = {k, streak, patience} after result t
void polar_probe_lift(int k, int patience, int cap, int floor, int n, const int* failed, int* out) {
  LiftDepth dp{k, 0, patience};
  for (int t = 0; t < n; ++t) {
    if (failed[t]) dp.fail(cap); else dp.pass(floor);
    out[3 * t] = dp.k; out[3 * t + 1] = dp.streak; out[3 * t + 2] = dp.patience;
  }
}

int polar_probe_xcds() { return kPolarXcds; }

}  // extern "C"
