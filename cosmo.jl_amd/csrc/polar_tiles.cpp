// polar_tiles.cpp -- tile planning of the sign iteration: see polar_tiles.h
#include "polar_tiles.h"

void polar_plan_large(const PolarTileOpts& o, PolarCone& pc) {
  const int d = pc.d;
  // tile side: minimise (rounds of upper tiles over the 256 CUs) x (tile work)
  long long best = -1; pc.ts = 64;
  for (int ts : {64, 96}) {
    const long long nt = (d + ts - 1) / ts, tiles = nt * (nt + 1) / 2;
    const long long cost = ((tiles + 255) / 256) * (long long)ts * ts;
    if (best < 0 || cost < best) { best = cost; pc.ts = ts; }
  }
  if (o.ts == 64 || o.ts == 96) pc.ts = o.ts;
  pc.ld = ((d + pc.ts - 1) / pc.ts) * pc.ts;
  { const long long nt = pc.ld / pc.ts; pc.sk = (pc.ts == 96 && nt * (nt + 1) / 2 <= 256) ? 2 : 1; }
  if (o.sk == 1 || (o.sk == 2 && pc.ts == 96)) pc.sk = o.sk;
  pc.skg = 0; pc.skc = 8;
  if (o.streamk) {
    // stream-K: tiles of 96 whatever the count (quantisation no longer matters); 2 workgroups per CU when the cone has the work
    pc.ts = kPolarStreamKTile; pc.sk = 3;
    pc.ld = ((d + pc.ts - 1) / pc.ts) * pc.ts;
    const long long nt = pc.ld / pc.ts, tiles = nt * (nt + 1) / 2, nk = pc.ld / kPolarPanelK;
    pc.skc = tiles >= 64 ? 8 : 1;
    const long long units_min = (tiles / pc.skc) * nk;                 // units of the smallest class
    long long per = std::min<long long>(512 / pc.skc, std::max<long long>(1, units_min / 4));   // >= 4 panels per workgroup
    { const long long v = o.skg / pc.skc; if (v >= 1 && v <= 1024 / pc.skc) per = std::min(v, std::max<long long>(1, units_min)); }
    pc.skg = (int)(per * pc.skc);
  }
}

long long polar_tile_cost(int d, int ext) {
  const int ei = ext & 255, ej = (ext >> 8) & 255, dg = (ext >> 16) & 1;
  const int nblk = dg ? ei * (ei + 1) / 2 : ei * ej, slots = (nblk + 3) / 4;
  return (long long)((d + 15) / 16) * (10 * slots + 2) + 125;
}

namespace {

// XCD-aware order: workgroup b runs on XCD b % 8 and each XCD has its own L2, so all tiles of a cone go to ONE XCD (they share the cone's operand
// panels: 1.5-2.5x fewer HBM reads than tiles scattered over eight L2s).  The cones of `order` are dealt, one after the other, to the XCD with the
// least work so far; emit(cone, x) appends the cone's entries to the lists of XCD x and returns the work they add.
template <class Emit>
void deal_to_xcds(const std::vector<int>& order, Emit emit) {
  long long load[kPolarXcds] = {};
  for (int ci : order) {
    int x = 0;
    for (int t = 1; t < kPolarXcds; ++t) if (load[t] < load[x]) x = t;
    load[x] += emit(ci, x);
  }
}

// entry 8 * slot + x is the slot-th entry of XCD x; short lists end with `null`
template <class T>
std::vector<T> interleave_xcds(const std::vector<T> (&xl)[kPolarXcds], const T& null) {
  size_t maxlen = 0;
  for (const std::vector<T>& l : xl) maxlen = std::max(maxlen, l.size());
  std::vector<T> out(kPolarXcds * maxlen, null);
  for (int x = 0; x < kPolarXcds; ++x) for (size_t sl = 0; sl < xl[x].size(); ++sl) out[kPolarXcds * sl + x] = xl[x][sl];
  return out;
}

// the XCDs' lists one after the other; counts the entries of every cone
template <class T>
std::vector<T> concat_xcds(const std::vector<T> (&xl)[kPolarXcds], int (&xoff)[kPolarXcds + 1], std::vector<int>& cone_nt) {
  std::vector<T> out;
  for (int x = 0; x < kPolarXcds; ++x) { xoff[x] = (int)out.size(); for (const T& t : xl[x]) { out.push_back(t); cone_nt[(size_t)t.cone] += 1; } }
  xoff[kPolarXcds] = (int)out.size();
  return out;
}

// quadrant list of one tile class (the cones of `order` whose ts is `ts`)
std::vector<QTile> quadrant_class(const std::vector<BatchCone>& cones, const std::vector<int>& order, int ts, bool flat) {
  std::vector<int> mine;
  for (int ci : order) if (cones[ci].ts == ts) mine.push_back(ci);
  std::vector<QTile> xl[kPolarXcds];
  auto emit = [&](int ci, int x) {
    const int nt = cones[ci].ld / ts;
    for (int tj = 0; tj < nt; ++tj) for (int ti = 0; ti <= tj; ++ti) xl[x].push_back(QTile{ci, ti, tj, 0});
    return (long long)nt * (nt + 1) / 2 * cones[ci].ld;
  };
  if (flat) { for (int ci : mine) emit(ci, 0); return xl[0]; }
  deal_to_xcds(mine, emit);
  return interleave_xcds(xl, QTile{-1, 0, 0, 0});
}

// Ragged tiles (see k_symm_gemm_batch_r) and queue items of the cones, per XCD: a cone's side in blocks of 16 is cut into ceil(nb16 / 4) nearly equal parts
const char* ragged_lists(const PolarTileOpts& o, const std::vector<int>& order, PolarBatchPlan& out, std::vector<RTile> (&xl)[kPolarXcds],
                         std::vector<RPair> (&xp)[kPolarXcds]) {
  const char* err = nullptr;
  deal_to_xcds(order, [&](int ci, int x) {
    const BatchCone& bc = out.cones[ci];
    const int nb16 = (bc.d + 15) / 16, nt = (nb16 + 3) / 4;
    std::vector<int> start(nt + 1, 0);
    for (int t = 0; t < nt; ++t) start[t + 1] = start[t] + nb16 / nt + (t < nb16 % nt ? 1 : 0);   // larger parts first: i0 + 64 <= ld for every tile
    auto ext = [&](int a, int b) { return (start[a + 1] - start[a]) | ((start[b + 1] - start[b]) << 8) | ((a == b ? 1 : 0) << 16); };
    long long load = 0;
    for (int tj = 0; tj < nt; ++tj)
      for (int ti = 0; ti <= tj; ++ti) {
        const int ei = start[ti + 1] - start[ti], ej = start[tj + 1] - start[tj];
        RTile rt; rt.cone = ci; rt.i0 = 16 * start[ti]; rt.j0 = 16 * start[tj]; rt.ext = ext(ti, tj);
        rt.ld = bc.ld; rt.d = bc.d; rt.woff = bc.woff;
        if (rt.i0 + 64 > bc.ld || rt.j0 + 64 > bc.ld) err = "ragged tile exceeds the leading dimension";
        xl[x].push_back(rt);
        const int nblk = ti == tj ? ei * (ei + 1) / 2 : ei * ej, slots = (nblk + 3) / 4;
        load += (long long)slots * nb16;
        out.flops_performed += 2.0 * 256.0 * nblk * 16.0 * nb16;
      }
    // items: along block row ti the tiles (ti, ti), (ti, ti + 1), ... are taken two at a time -- diagonal + right neighbour, then off-diagonal neighbours;
    // an odd one is left single.  What is left lies in the last block column: pair == 3 takes those tiles two at a time as well (they share the
    // column's B panel).  pair == 2 (lab): every tile single, in the order of the tile list above
    auto item = [&](int ti, int tj, int ti1, int tj1) {      // tile (ti, tj) and, if ti1 >= 0, tile (ti1, tj1)
      RPair it; it.cone = ci; it.i0 = 16 * start[ti]; it.j0 = 16 * start[tj]; it.ld = bc.ld; it.d = bc.d; it.woff = bc.woff; it.pad = 0;
      it.ext0 = ext(ti, tj);
      it.i1 = ti1 >= 0 ? 16 * start[ti1] : it.i0; it.j1 = ti1 >= 0 ? 16 * start[tj1] : it.j0;
      it.ext1 = ti1 >= 0 ? ext(ti1, tj1) : 0;
      xp[x].push_back(it);
    };
    if (o.pair == 2) { for (int tj = 0; tj < nt; ++tj) for (int ti = 0; ti <= tj; ++ti) item(ti, tj, -1, -1); }
    else {
      int left = -1;                                         // a block row whose last tile waits for a partner in the last column
      for (int ti = 0; ti < nt; ++ti)
        for (int tj = ti; tj < nt; tj += 2) {
          if (tj + 1 < nt) item(ti, tj, ti, tj + 1);
          else if (o.pair != 3) item(ti, tj, -1, -1);
          else if (left < 0) left = ti;
          else { item(left, tj, ti, tj); left = -1; }
        }
      if (left >= 0) item(left, nt - 1, -1, -1);
    }
    return load;
  });
  return err;
}

}  // namespace

const char* polar_plan_batch(const std::vector<PolarBatchIn>& in, const PolarTileOpts& o, PolarBatchPlan& out) {
  out = PolarBatchPlan();
  for (const PolarBatchIn& c : in) {
    BatchCone bc;
    bc.off = c.off; bc.d = c.d; bc.kind = c.kind; bc.idx = c.idx;
    // tile side (opt-in): 96 x 96 tiles stream 1.5x fewer operand bytes per flop than 64 x 64 tiles (12 vs 8 flop per byte) and spend fewer barriers
    // per flop; they would be used where they do not cost padding: sides in (64, 96] (one tile instead of three) and in (128, 192] (three tiles
    // instead of six).  Everything else keeps 64 x 64 tiles.
    bc.ts = (o.ts96 && ((c.d > 64 && c.d <= 96) || (c.d > 128 && c.d <= 192))) ? 96 : 64;
    bc.ld = ((c.d + bc.ts - 1) / bc.ts) * bc.ts;
    bc.woff = out.work;
    out.work += 4LL * bc.ld * bc.ld;
    out.cones.push_back(bc);
    out.flops_useful += (double)bc.d * bc.d * (bc.d + 1.0);
  }
  // longest k first: the tiles of the biggest cones start at once, the small ones fill the tail
  std::vector<int> order(out.cones.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return out.cones[a].ld > out.cones[b].ld; });
  // one quadrant list per tile class (64, then 96): a product is one launch per class
  out.qtiles = quadrant_class(out.cones, order, 64, o.flat);
  out.nbtiles = (int)out.qtiles.size();
  { const std::vector<QTile> t96 = quadrant_class(out.cones, order, 96, o.flat);
    out.nbtiles96 = (int)t96.size();
    out.qtiles.insert(out.qtiles.end(), t96.begin(), t96.end()); }
  if (!o.ragged) {
    for (const BatchCone& bc : out.cones) { const long long nt = bc.ld / bc.ts; out.flops_performed += 2.0 * (double)(nt * (nt + 1) / 2) * bc.ts * bc.ts * (((bc.d + 31) / 32) * 32); }
    return nullptr;
  }
  std::vector<RTile> xl[kPolarXcds];
  std::vector<RPair> xp[kPolarXcds];       // the items of the persistent launch's 512-thread form
  if (const char* err = ragged_lists(o, order, out, xl, xp)) return err;
  // Launch order inside an XCD's list = decreasing modelled cost of a tile: the hardware hands the next workgroup to the first free slot, i.e. it runs
  // longest-processing-time-first list scheduling if the list is sorted -- with ~1.5 tiles per slot the order of the cones (by leading
  // dimension only) left expensive tiles for the tail.  35.8 -> 32.0 us per product on BASELINE config 5 (three alternating pairs of runs,
  // profiles/r03_cfg5_ragged.txt).  A cone's tiles of one shape stay adjacent (stable sort), so they still meet in the XCD's L2.
  if (o.sort) {
    auto cost = [](const RTile& t) { return polar_tile_cost(t.d, t.ext); };
    auto pcost = [](const RPair& it) {            // an item costs what its busier half costs
      const long long c0 = polar_tile_cost(it.d, it.ext0);
      return it.ext1 ? std::max(c0, polar_tile_cost(it.d, it.ext1)) : c0;
    };
    for (std::vector<RTile>& l : xl) std::stable_sort(l.begin(), l.end(), [&](const RTile& a, const RTile& b) { return cost(a) > cost(b); });
    for (std::vector<RPair>& l : xp) std::stable_sort(l.begin(), l.end(), [&](const RPair& a, const RPair& b) { return pcost(a) > pcost(b); });
  }
  out.rtiles = interleave_xcds(xl, RTile{-1, 0, 0, 0, 0, 0, 0});
  for (const std::vector<RTile>& l : xl) out.df_ntiles += (int)l.size();
  // the same per-XCD lists, contiguous, for the persistent dependency-driven launch of the main schedule
  out.cone_nt.assign(out.cones.size(), 0);
  if (o.pair) out.pairs = concat_xcds(xp, out.xoff, out.cone_nt);
  else out.items = concat_xcds(xl, out.xoff, out.cone_nt);
  return nullptr;
}
