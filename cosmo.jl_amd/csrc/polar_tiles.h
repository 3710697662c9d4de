// polar_tiles.h -- tile planning of the sign iteration (psd_polar.hip): the descriptors its kernels read and the integer planning that fills them
// (host code, integers only; no HIP headers, the same object in both libraries).  The kernels rely on what the lists promise -- every upper block of
// a cone in exactly one tile, 64-wide panel loads inside the leading dimension, a cone's tiles in one XCD's list, at most three distinct panels per
// queue item, per-cone item counts that match the queue -- and tests/test_polar_tiles_host.py checks those promises through tests/polar_tiles_probe.cpp.
#pragma once
#include <algorithm>
#include <vector>

constexpr int kPolarXcds = 8;   // tile lists of the batch: one per XCD (workgroup b runs on XCD b % 8, the kernels' `& 7`)
constexpr int kPolarPanelK = 16, kPolarStreamKTile = 96;   // k panel of the product kernels, tile side of the stream-K kernel (PK, SKG_TS of psd_polar.hip)

// ---- descriptors (device layouts) ----------------------------------------------------------------------------------------------------------------
struct PolarCone {
  int idx;            // index in PsdPlan::cones
  int off, d, kind;
  int ts;             // tile side of the products (64 or 96), chosen per cone
  int sk;             // 2: intra-workgroup split of k (8 waves), when the upper tiles give at most one tile per CU; 3: stream-K
  int skg, skc;       // stream-K: workgroups of a launch, ticket classes (8 = one tile range per XCD, 1 = a single range)
  int ld;             // d rounded up to ts
  long long woff;     // offset of this cone's 4 work matrices (doubles)
};

struct BatchCone { long long woff; int off, d, kind, ld, idx, ts; };   // a mid-size cone of the batched path (device table); ts = tile side of its products (64 | 96)

struct QTile { int cone, ti, tj, pad; };   // tile (ti <= tj) of the quadrant kernel, in tiles of the cone's ts; uploaded as the kernel's int4

// ragged tile: ext = ei | ej << 8 | diag << 16 (ei, ej in blocks of 16); see k_symm_gemm_batch_r
struct alignas(32) RTile { int cone; int i0, j0; int ext; int ld, d; long long woff; };

// queue item of the 512-thread persistent kernel: one ragged tile (ext1 == 0) or two that share a panel; see paired_item
struct alignas(16) RPair { int cone; int i0, j0, i1, j1; int ext0, ext1; int ld, d; int pad; long long woff; };

static_assert(sizeof(BatchCone) == 32 && sizeof(QTile) == 16 && sizeof(RTile) == 32 && sizeof(RPair) == 48, "device layouts of the tile descriptors");

// ---- planning --------------------------------------------------------------------------------------------------------------------------------------
struct PolarTileOpts {
  int ts96 = 0;       // batch: cones whose side fits 96 / 192 take 96 x 96 quadrant tiles (a second tile class)
  int flat = 0;       // batch, quadrant list: cone order, no XCD interleaving
  int ragged = 1;     // batch: build the ragged tile list and the queue items
  int pair = 3;       // queue items: 0 one RTile each; 1 RPairs along block rows; 3 and along the last block column; 2 RPairs, every tile single
  int sort = 1;       // ragged lists: decreasing modelled cost inside an XCD's list (0: cone order)
  int streamk = 0;    // large cones: stream-K geometry
  int ts = 0, sk = 0; // large cones: forced tile side (64 | 96) / k-split (1, or 2 with ts == 96); anything else: the planner's choice
  long long skg = 0;  // large cones, stream-K: requested workgroups per launch (<= 0: the planner's choice)
};

// ts, sk, ld, skg, skc of a large cone from its side d (the other members are left alone)
void polar_plan_large(const PolarTileOpts& o, PolarCone& pc);

struct PolarBatchIn { int d, off, kind, idx; };   // off, kind, idx are passed through to the BatchCone table
struct PolarBatchPlan {
  std::vector<BatchCone> cones;                 // in the order of the input
  long long work = 0;                           // reals of all cones' work matrices (4 ld^2 each, at woff)
  std::vector<QTile> qtiles;                    // quadrant list: the 64-class (nbtiles entries), then the 96-class (nbtiles96)
  int nbtiles = 0, nbtiles96 = 0;
  // the rest only with PolarTileOpts::ragged
  std::vector<RTile> rtiles;                    // entry 8 * slot + x is the slot-th tile of XCD x; short lists end with null tiles (cone == -1)
  std::vector<RTile> items;                     // pair == 0: the XCDs' lists one after the other, list x = [xoff[x], xoff[x + 1])
  std::vector<RPair> pairs;                     // pair != 0: the same as RPairs
  int xoff[kPolarXcds + 1] = {};
  std::vector<int> cone_nt;                     // queue items per cone: what a cone's completion counter gains per product
  int df_ntiles = 0;                            // ragged tiles per product
  double flops_performed = 0.0, flops_useful = 0.0;   // per product: 16 x 16 x 16 blocks actually issued; sum d^2 (d + 1)
};
// nullptr, or the reason why the batch cannot be planned (out is then incomplete)
const char* polar_plan_batch(const std::vector<PolarBatchIn>& in, const PolarTileOpts& o, PolarBatchPlan& out);

// ---- cone-local workgroup ids of the batch's populate-type kernels ---------------------------------------------------------------------------------
// The bpx workgroups of a cone share id % 8, i.e. (round-robin dispatch) one XCD and its L2: id = 8 * ((cone / 8) * bpx + bx) + cone % 8 on a 1-D grid of
// 8 * bpx * ceil(n / 8) workgroups; the ids of a short last group of cones decode to "none".  Placement is a matter of speed only.  constexpr: the
// kernels decode with the same code that tests/test_polar_passes_host.py checks on the CPU.
struct PolarWg { int cone, bx; };   // cone == -1: none
constexpr int polar_wg_grid(int n, int bpx) { return kPolarXcds * bpx * ((n + kPolarXcds - 1) / kPolarXcds); }
constexpr int polar_wg_id(int cone, int bx, int bpx) { return kPolarXcds * ((cone / kPolarXcds) * bpx + bx) + cone % kPolarXcds; }
constexpr PolarWg polar_wg_decode(int id, int n, int bpx) {
  const int xcd = id & (kPolarXcds - 1), slot = id / kPolarXcds;
  const int cone = kPolarXcds * (slot / bpx) + xcd;
  return (id < 0 || cone >= n) ? PolarWg{-1, 0} : PolarWg{cone, slot % bpx};
}

// modelled cost of a ragged tile of a cone of side d: k-panels x slots of its fullest wave, in units of a tenth of a slot, + a fixed part for prologue
// and epilogue
long long polar_tile_cost(int d, int ext);

// Lifting depth of one cone under the adaptive rule: one step deeper on a failed verification (and twice the patience, up to 96, before the next
// probe downwards), one step shallower after `patience` verified projections in a row.  Both return whether k changed.
struct LiftDepth {
  int k, streak, patience;
  bool fail(int cap) {
    const bool up = k < cap;
    if (up) k += 1;
    streak = 0;
    patience = std::min(96, 2 * patience);
    return up;
  }
  bool pass(int floor) {
    if (++streak < patience || k <= floor) return false;
    k -= 1; streak = 0;
    return true;
  }
};
