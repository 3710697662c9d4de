// batch_image.cpp -- see batch_image.h.  Host code: no HIP header, no getenv.  plan_batch_images at the end is the driver; every step above it says in
// one line what it promises, and tests/test_batch_image_host.py checks the promises on the finished plan.
#include "batch_image.h"
#include <string.h>
#include <algorithm>

typedef cosmo_hip_real real;
#ifdef COSMO_HIP_REAL_FLOAT
#define REAL_IS_FLOAT 1
#else
#define REAL_IS_FLOAT 0
#endif
#define R(x) ((real)(x))

void brow_blocks(const std::vector<int>& rowptr, int nrows, std::vector<int>& rb) {
  rb.clear(); rb.push_back(0);
  int r = 0;
  while (r < nrows) {
    int r1 = r; long long cnt = 0;
    while (r1 < nrows) {
      const long long rn = (long long)rowptr[r1 + 1] - rowptr[r1];
      if (r1 > r && (cnt + rn > kRowBlockNnz || r1 - r >= kRowBlockRows)) break;
      cnt += rn; ++r1;
      if (cnt > kRowBlockNnz) break;
    }
    rb.push_back(r1); r = r1;
  }
}

namespace {

long long up16(long long x) { return (x + 15) / 16 * 16; }

// the arrays of a row-major image
struct ImgArrays {
  real *Aval, *Pval; unsigned short *Arp, *Acol, *Trp, *Prp, *Pcol; uint32_t* Tpr;
  ImgArrays(std::vector<unsigned char>& im, const LdsHdr& h)
      : Aval(reinterpret_cast<real*>(im.data() + h.oAval)), Pval(reinterpret_cast<real*>(im.data() + h.oPval)),
        Arp(reinterpret_cast<unsigned short*>(im.data() + h.oArp)), Acol(reinterpret_cast<unsigned short*>(im.data() + h.oAcol)),
        Trp(reinterpret_cast<unsigned short*>(im.data() + h.oTrp)), Prp(reinterpret_cast<unsigned short*>(im.data() + h.oPrp)),
        Pcol(reinterpret_cast<unsigned short*>(im.data() + h.oPcol)), Tpr(reinterpret_cast<uint32_t*>(im.data() + h.oTpr)) {}
};

// Step 1.  The form of the batch from its sizes, cones and switches: workgroup size, register mode, the register-CG flags, long rows, whether a sliced
// image is wanted, whether P is diagonal everywhere.  false: no image at all (LDS = 0, or n / m beyond u16 indices).
bool choose_form(const BatchImageIn& in, const BatchImageOpts& o, BatchImagePlan& pl) {
  if (!o.lds) return false;
  const long long n = in.n, m = in.m;
  if (n > 65535 || m > 65535 || n + m == 0) return false;
  const bool ext = in.npsd > 0 || in.n3 > 0 || in.aa_on || o.ext;
  pl.bs = (o.bs == 256 || o.bs == 512 || o.bs == 1024) ? o.bs : 512;
  pl.force_ext = o.ext;     // measure the extended-cone instantiations on batches without such cones
  if (ext) pl.bs = 512;     // the extended-cone / accelerated instantiations of the LDS-image kernel exist for 512 threads
  // register-resident iterates (k_batch_admm_reg, 512 threads) when the vectors fit 1-2 (n) / 2-4 (m) elements per thread
  if (o.reg) {
    if (n <= 512 && m <= 1024) pl.reg_mode = 1; else if (n <= 1024 && m <= 2048) pl.reg_mode = 2;
    if (in.aa_on && (in.npsd > 0 || in.n3 > 0)) pl.reg_mode = 0;   // the accelerated register kernel is instantiated without the PSD / exp / pow code (registers): the LDS-image kernel takes such batches
    if (in.nmid > 0) pl.reg_mode = 0;         // the block-Jacobi code on top of ~200 live registers would spill: the LDS-image kernel (187 VGPRs) takes such batches
    if (pl.reg_mode) pl.bs = 512;
  }
  // sliced image (register kernel <512, 1, 2>, double precision; row_sliced): built next to the row-major one, used if every problem's fits
  pl.want_sliced = !REAL_IS_FLOAT && pl.reg_mode == 1 && o.sliced;
  pl.p_all_diag = true;                                                                      // P diagonal (or empty rows) in every problem: it moves into registers
  for (int k = 0; k < in.nprob && pl.p_all_diag; ++k) {
    const HostCsr& PT = (*in.PT)[k];
    for (long long j = 0; j < n && pl.p_all_diag; ++j) { const int len = PT.split[j] - PT.rowptr[j]; if (len > 1 || (len == 1 && PT.col[PT.rowptr[j]] != (int)j)) pl.p_all_diag = false; }
  }
  // rows / columns of A with >= LONG_ROW entries (a dense budget row, an epigraph variable): the register kernel <512, 1, 2> hands them to a whole wave in
  // its Krylov passes (LONG instantiations, row_long_or_pipe3); the sliced image would pad the 32 rows of such a row's slice to its length: not built then
  if (pl.reg_mode != 0 && o.long_rows) {
    for (int k = 0; k < in.nprob && !pl.long_rows; ++k) {
      const HostCsr &A = (*in.A)[k], &AT = (*in.AT)[k];
      for (long long i = 0; i < m && !pl.long_rows; ++i) if (A.rowptr[i + 1] - A.rowptr[i] >= LONG_ROW) pl.long_rows = true;
      for (long long j = 0; j < n && !pl.long_rows; ++j) if (AT.rowptr[j + 1] - AT.rowptr[j] >= LONG_ROW) pl.long_rows = true;
    }
    if (pl.long_rows) pl.want_sliced = false;
  }
  // LDS-image kernel, register-CG form of its reduced solve (batch_admm_body, RCG: the 512-thread instantiations with the extended cones): the compute
  // assignment sorted by length (D.permA / D.permT in that form's <2, 4>-slot layout) and, with it, the image STORED in that order (round 6)
  pl.rcg_form = pl.reg_mode == 0 && pl.bs == 512 && n <= 2 * 512 && m <= 4 * 512 && ext && o.ldscg;
  pl.rcg_sorted = pl.rcg_form && o.ldscg_sorted;
  pl.rcg_stored = pl.rcg_sorted && o.store_sorted;
  return true;
}

// Step 2.  ordA: the rows of A by decreasing length; ordT: the columns by decreasing length of [P | A'].  Stable: equal lengths stay in index order.
void length_order(const HostCsr& A, const HostCsr& PT, std::vector<int>& ordA, std::vector<int>& ordT) {
  ordA.resize((size_t)A.nrows); ordT.resize((size_t)PT.nrows);
  for (size_t i = 0; i < ordA.size(); ++i) ordA[i] = (int)i;
  for (size_t j = 0; j < ordT.size(); ++j) ordT[j] = (int)j;
  std::stable_sort(ordA.begin(), ordA.end(), [&](int x, int y) { return A.rowptr[x + 1] - A.rowptr[x] > A.rowptr[y + 1] - A.rowptr[y]; });
  std::stable_sort(ordT.begin(), ordT.end(), [&](int x, int y) { return PT.rowptr[x + 1] - PT.rowptr[x] > PT.rowptr[y + 1] - PT.rowptr[y]; });
}

// Step 3.  Sorted position q goes to slot q / 512 of thread q % 512 -- a wave-step covers 64 consecutive positions -- and with `serpentine` (the rows of
// A) odd slots run backwards, thread 511 - q % 512: the wave with the longest rows of one slot has the shortest of the next, so that the pass ends with
// its slowest wave.  perm: the member's table of slots * 512 entries, -1 where no position falls.
void assign_serpentine(const std::vector<int>& ord, bool serpentine, int* perm) {
  for (size_t q = 0; q < ord.size(); ++q) {
    const size_t sl = q / 512, t = (serpentine && (sl & 1)) ? 511 - q % 512 : q % 512;
    perm[sl * 512 + t] = ord[q];
  }
}

// row pointers of the rows of `rowptr` laid out in the order `ord`
std::vector<int> ordered_rowptr(const std::vector<int>& rowptr, const std::vector<int>& ord) {
  std::vector<int> out(ord.size() + 1, 0);
  for (size_t q = 0; q < ord.size(); ++q) out[q + 1] = out[q] + (rowptr[(size_t)ord[q] + 1] - rowptr[(size_t)ord[q]]);
  return out;
}

// Step 4.  The header of a row-major image from its counts: every array at a 16-byte offset behind the one before it, bytes = the end of the last.
LdsHdr layout(long long n, long long m, long long nnzA, long long nnzP, size_t nbA, size_t nbAT, size_t nbPT, bool with_ord) {
  LdsHdr h; memset(&h, 0, sizeof h);
  h.nnzA = (int)nnzA; h.nnzP = (int)nnzP; h.nbA = (int)nbA; h.nbAT = (int)nbAT; h.nbPT = (int)nbPT;
  long long o = up16(sizeof(LdsHdr));
  h.oAval = (int)o; o = up16(o + (long long)sizeof(real) * nnzA);
  h.oPval = (int)o; o = up16(o + (long long)sizeof(real) * nnzP);
  h.oRbA = (int)o; o = up16(o + 16LL * h.nbA);
  h.oRbAT = (int)o; o = up16(o + 16LL * h.nbAT);
  h.oRbPT = (int)o; o = up16(o + 16LL * h.nbPT);
  h.oArp = (int)o; o = up16(o + 2 * (m + 1));
  h.oAcol = (int)o; o = up16(o + 2 * nnzA);
  h.oTrp = (int)o; o = up16(o + 2 * (n + 1));
  h.oTpr = (int)o; o = up16(o + 4 * nnzA);
  h.oPrp = (int)o; o = up16(o + 2 * (n + 1));
  h.oPcol = (int)o; o = up16(o + 2 * nnzP);
  if (with_ord) { h.oAord = (int)o; o = up16(o + 2 * m); h.oTord = (int)o; o = up16(o + 2 * n); }
  h.bytes = (int)o;
  return h;
}

// the tile list at `off`: {first row, end row, first entry, end entry} of every block of r, entries counted on rowptr
void fill_rb(std::vector<unsigned char>& im, int off, const std::vector<int>& r, const std::vector<int>& rowptr) {
  int* d = reinterpret_cast<int*>(im.data() + off);
  for (size_t t = 0; t + 1 < r.size(); ++t) { d[4 * t] = r[t]; d[4 * t + 1] = r[t + 1]; d[4 * t + 2] = rowptr[r[t]]; d[4 * t + 3] = rowptr[r[t + 1]]; }
}

// Step 5.  The image in index order: A by rows, P by rows, every entry of A' as (its slot in Aval | its row << 16); srcA / srcP: the source of every slot
// of Aval / Pval (cosmo_hip_batch_stage_matrices), carried through every reordering next to the values.  false: A and A' disagree.
bool fill_index_order(const HostCsr& A, const HostCsr& AT, const HostCsr& PT, const std::vector<int32_t>& uA, const std::vector<int32_t>& uPT,
                      const ImgArrays& a, std::vector<int32_t>& srcA, std::vector<int32_t>& srcP) {
  const long long n = PT.nrows, m = A.nrows, nnzA = (long long)A.val.size();
  srcA.assign(uA.begin(), uA.end()); srcP.assign((size_t)(PT.val.size() - A.val.size()), -1);
  for (long long t = 0; t < nnzA; ++t) { a.Aval[t] = A.val[t]; a.Acol[t] = (unsigned short)A.col[t]; }
  for (long long i = 0; i <= m; ++i) a.Arp[i] = (unsigned short)A.rowptr[i];
  std::vector<int> cur(A.rowptr.begin(), A.rowptr.end() - 1);
  long long pp = 0;
  for (long long j = 0; j < n; ++j) {
    a.Trp[j] = (unsigned short)AT.rowptr[j]; a.Prp[j] = (unsigned short)pp;
    for (int t = PT.rowptr[j]; t < PT.split[j]; ++t) { a.Pval[pp] = PT.val[t]; a.Pcol[pp] = (unsigned short)PT.col[t]; srcP[(size_t)pp] = uPT[(size_t)t]; ++pp; }
    for (int t = AT.rowptr[j]; t < AT.rowptr[j + 1]; ++t) {
      const int i = AT.col[t]; const int p = cur[i]++;
      if (p >= A.rowptr[i + 1] || A.col[p] != (int)j || A.val[p] != AT.val[t]) return false;
      a.Tpr[t] = (uint32_t)p | ((uint32_t)i << 16);
    }
  }
  a.Trp[n] = (unsigned short)AT.rowptr[n]; a.Prp[n] = (unsigned short)pp;
  return true;
}

// Step 6.  The arrays filled in index order move to the order (ordA, ordT): the rows of A, the columns of A' and the rows of P lie in that order, Arp /
// Trp / Prp are indexed by POSITION, A' entries name the new slots; the source maps move with the values.  Same values, same order inside every row:
// every row sum keeps its bits.
void store_in_order(const std::vector<int>& ordA, const std::vector<int>& ordT, const LdsHdr& h, const ImgArrays& a, std::vector<int32_t>& srcA,
                    std::vector<int32_t>& srcP) {
  const size_t m = ordA.size(), n = ordT.size(), nnzA = (size_t)h.nnzA, nnzP = (size_t)h.nnzP;
  const std::vector<unsigned short> oArp(a.Arp, a.Arp + m + 1), oTrp(a.Trp, a.Trp + n + 1), oPrp(a.Prp, a.Prp + n + 1);
  std::vector<real> nAval(nnzA), nPval(nnzP);
  std::vector<unsigned short> nAcol(nnzA), nPcol(nnzP);
  std::vector<uint32_t> nTpr(nnzA);
  std::vector<int> newstart(m);
  std::vector<int32_t> nsrcA(nnzA), nsrcP(nnzP);
  size_t w = 0;
  for (size_t q = 0; q < m; ++q) {
    const size_t r = (size_t)ordA[q];
    a.Arp[q] = (unsigned short)w; newstart[r] = (int)w;
    for (size_t t = oArp[r]; t < oArp[r + 1]; ++t) { nAval[w] = a.Aval[t]; nAcol[w] = a.Acol[t]; nsrcA[w] = srcA[t]; ++w; }
  }
  a.Arp[m] = (unsigned short)w;
  size_t wt = 0, wp = 0;
  for (size_t q = 0; q < n; ++q) {
    const size_t c = (size_t)ordT[q];
    a.Trp[q] = (unsigned short)wt; a.Prp[q] = (unsigned short)wp;
    for (size_t t = oTrp[c]; t < oTrp[c + 1]; ++t) {
      const uint32_t pr = a.Tpr[t]; const uint32_t row = pr >> 16, pold = pr & 0xffffu;
      nTpr[wt++] = (uint32_t)(newstart[row] + (int)(pold - oArp[row])) | (row << 16);
    }
    for (size_t t = oPrp[c]; t < oPrp[c + 1]; ++t) { nPval[wp] = a.Pval[t]; nPcol[wp] = a.Pcol[t]; nsrcP[wp] = srcP[t]; ++wp; }
  }
  a.Trp[n] = (unsigned short)wt; a.Prp[n] = (unsigned short)wp;
  srcA.swap(nsrcA); srcP.swap(nsrcP);
  std::copy(nAval.begin(), nAval.end(), a.Aval); std::copy(nAcol.begin(), nAcol.end(), a.Acol); std::copy(nTpr.begin(), nTpr.end(), a.Tpr);
  std::copy(nPval.begin(), nPval.end(), a.Pval); std::copy(nPcol.begin(), nPcol.end(), a.Pcol);
}

// Greedy bank-pair assignment: entries by decreasing number of appearances, each to the bank pair that adds the fewest conflicts over the groups it
// appears in (capacity = slots of that residue), slots handed out in order.  pos: a permutation of 0 .. nent - 1.
void assign_positions(int nent, const std::vector<std::vector<int>>& groups, int* pos) {
  std::vector<std::vector<int>> where((size_t)nent);                 // entry -> groups it appears in
  for (size_t g = 0; g < groups.size(); ++g) for (int e : groups[g]) where[(size_t)e].push_back((int)g);
  std::vector<int> order((size_t)nent);
  for (int e = 0; e < nent; ++e) order[(size_t)e] = e;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return where[(size_t)x].size() > where[(size_t)y].size(); });
  std::vector<int> cap(32, 0), used(32, 0);
  for (int q = 0; q < nent; ++q) cap[q % 32] += 1;
  std::vector<unsigned char> cnt(groups.size() * 32, 0);
  for (int e : order) {
    int best = -1; long long bestc = 0;
    for (int bk = 0; bk < 32; ++bk) {
      if (used[bk] >= cap[bk]) continue;
      long long c = 0;
      for (int g : where[(size_t)e]) c += cnt[(size_t)g * 32 + bk];
      if (best < 0 || c < bestc || (c == bestc && used[bk] < used[best])) { best = bk; bestc = c; }
    }
    pos[e] = best + 32 * used[best];
    used[best] += 1;
    for (int g : where[(size_t)e]) cnt[(size_t)g * 32 + best] += 1;
  }
}

// Step 7.  Positions of the gathered vectors (register kernel <512, 1, 2>: permA of 2 slots, permT of 1).  A ds_read_b64 is served 32 lanes at a time and
// an 8-byte slot p lies in bank pair p mod 32: the 32 rows a half-wave works on in one step gather 32 entries, and every extra entry on a busy bank
// pair costs an LDS cycle (random indices: ~3.4 per group).  posN / posM: permutations that use every residue mod 32 to its capacity; the image's
// gather indices (Acol, Pcol, the row half of Tpr) become positions.
void colour_positions(const HostCsr& A, const HostCsr& AT, const HostCsr& PT, const int* permA, const int* permT, const LdsHdr& h, const ImgArrays& a,
                      int* posN, int* posM) {
  // one group per step st of a half-wave's 32 rows: the entries its lanes gather together
  std::vector<std::vector<int>> gN, gM;
  auto add_groups = [](const int* perm32, const std::vector<int>& first, const std::vector<int>& end, const std::vector<int>& col, std::vector<std::vector<int>>& out) {
    int maxlen = 0;
    for (int t = 0; t < 32; ++t) { const int r = perm32[t]; if (r >= 0) maxlen = std::max(maxlen, end[(size_t)r] - first[(size_t)r]); }
    for (int st = 0; st < maxlen; ++st) {
      std::vector<int> g;
      for (int t = 0; t < 32; ++t) { const int r = perm32[t]; if (r >= 0 && first[(size_t)r] + st < end[(size_t)r]) g.push_back(col[(size_t)(first[(size_t)r] + st)]); }
      if (g.size() > 1) out.push_back(g);
    }
  };
  const std::vector<int> Aend(A.rowptr.begin() + 1, A.rowptr.end()), Tend(AT.rowptr.begin() + 1, AT.rowptr.end());
  // the x-gathers: rows computed by a half-wave in one step of the A pass; columns of P gathered by a half-wave in the column pass
  for (int hw = 0; hw < 2 * 16; ++hw) add_groups(permA + 32 * hw, A.rowptr, Aend, A.col, gN);
  for (int hw = 0; hw < 16; ++hw) {
    add_groups(permT + 32 * hw, PT.rowptr, PT.split, PT.col, gN);
    add_groups(permT + 32 * hw, AT.rowptr, Tend, AT.col, gM);
  }
  assign_positions(PT.nrows, gN, posN);
  assign_positions(A.nrows, gM, posM);
  for (int t = 0; t < h.nnzA; ++t) { a.Acol[t] = (unsigned short)posN[a.Acol[t]]; a.Tpr[t] = (a.Tpr[t] & 0xffffu) | ((uint32_t)posM[a.Tpr[t] >> 16] << 16); }
  for (int t = 0; t < h.nnzP; ++t) a.Pcol[t] = (unsigned short)posN[a.Pcol[t]];
}

// Step 8.  The sliced image of a member (see row_sliced) from its final row-major arrays (stored in sorted order, gather indices = positions): the entry
// of trip tt of lane l of a 32-row slice at (slice offset + l) + 32 tt, a zero tail two trips past every wave's longest row, Acol in bytes, A' entries
// as (LDS byte address of the value | row position << 21); slA / slT: first entry | length << 16 of every thread's rows / column.  With a diagonal P
// the image has no P and the member's row of pdiag / pdiag_has / um_pd holds it.  false: the sliced image does not fit (nothing is written then).
bool slice_image(const BatchImageIn& in, int k, const LdsHdr& h, const ImgArrays& a, const std::vector<int32_t>& srcA, BatchImagePlan& pl) {
  const long long n = in.n, m = in.m, nnzA = h.nnzA, nnzP = h.nnzP;
  const HostCsr& PT = (*in.PT)[k];
  const bool p_all_diag = pl.p_all_diag;
  auto qA = [&](int j, int t) { return 512 * j + ((j & 1) ? 511 - t : t); };        // slot j of thread t computes the row at this sorted position
  long long offA[32], LA[32], offT[16], LT[16], curA = 0, curT = 0, needA = 0, needT = 0;
  for (int j = 0; j < 2; ++j) for (int sx = 0; sx < 16; ++sx) {
    long long L = 0;
    for (int l = 0; l < 32; ++l) { const int q = qA(j, 32 * sx + l); if (q < m) L = std::max<long long>(L, a.Arp[q + 1] - a.Arp[q]); }
    offA[j * 16 + sx] = curA; LA[j * 16 + sx] = L; curA += 32 * L;
  }
  for (int sx = 0; sx < 16; ++sx) {
    long long L = 0;
    for (int l = 0; l < 32; ++l) { const int q = 32 * sx + l; if (q < n) L = std::max<long long>(L, a.Trp[q + 1] - a.Trp[q]); }
    offT[sx] = curT; LT[sx] = L; curT += 32 * L;
  }
  // a lane runs to its WAVE's longest row and reads two trips ahead: into the slices behind its own, or into the zero tail sized here
  for (int j = 0; j < 2; ++j) for (int sx = 0; sx < 16; ++sx) needA = std::max(needA, offA[j * 16 + sx] + 32 * (std::max(LA[j * 16 + (sx & ~1)], LA[j * 16 + (sx | 1)]) + 2));
  for (int sx = 0; sx < 16; ++sx) needT = std::max(needT, offT[sx] + 32 * (std::max(LT[sx & ~1], LT[sx | 1]) + 2));
  const long long nS = std::max(curA, needA), nT = std::max(curT, needT);
  LdsHdr h2; memset(&h2, 0, sizeof h2);
  h2.nnzA = (int)nS; h2.nnzP = p_all_diag ? 0 : (int)nnzP;
  long long o2 = up16(sizeof(LdsHdr));
  h2.oAval = (int)o2; o2 = up16(o2 + (long long)sizeof(real) * nS);
  h2.oTpr = (int)o2; o2 = up16(o2 + 4 * nT);
  h2.oAcol = (int)o2; o2 = up16(o2 + 2 * nS);
  if (!p_all_diag) {
    h2.oPval = (int)o2; o2 = up16(o2 + (long long)sizeof(real) * nnzP);
    h2.oPrp = (int)o2; o2 = up16(o2 + 2 * (n + 1));
    h2.oPcol = (int)o2; o2 = up16(o2 + 2 * nnzP);
  }
  h2.bytes = (int)o2;
  if (nS > 65535 || nT > 65535 || SL_WS0 + o2 > in.max_lds || SL_WS0 + h2.oAval + (long long)sizeof(real) * nS >= (1LL << 18)) return false;
  if (pl.slA.empty()) {
    pl.slA.assign((size_t)in.nprob * 2 * 512, 0u); pl.slT.assign((size_t)in.nprob * 512, 0u);
    if (p_all_diag) { pl.pdiag.assign((size_t)in.nprob * n, R(0.0)); pl.pdiag_has.assign((size_t)in.nprob * n, 0); }
  }
  std::vector<unsigned char>& i2 = pl.imgs2[(size_t)k];
  i2.assign((size_t)o2, 0);
  memcpy(i2.data(), &h2, sizeof h2);
  real* Aval2 = reinterpret_cast<real*>(i2.data() + h2.oAval);
  unsigned short* Acol2 = reinterpret_cast<unsigned short*>(i2.data() + h2.oAcol);
  uint32_t* Tpr2 = reinterpret_cast<uint32_t*>(i2.data() + h2.oTpr);
  std::vector<long long> newpos((size_t)std::max<long long>(nnzA, 1), 0);
  std::vector<int32_t>& srcA2 = pl.um_imgA2[(size_t)k];
  srcA2.assign((size_t)nS, -1);                                                  // (the zero padding has no source)
  for (int j = 0; j < 2; ++j) for (int sx = 0; sx < 16; ++sx) for (int l = 0; l < 32; ++l) {
    const int t = 32 * sx + l, q = qA(j, t);
    const long long off = offA[j * 16 + sx] + l;
    const long long start = q < m ? a.Arp[q] : 0, len = q < m ? a.Arp[q + 1] - a.Arp[q] : 0;
    pl.slA[((size_t)k * 2 + (size_t)j) * 512 + (size_t)t] = (uint32_t)off | ((uint32_t)len << 16);
    for (long long tt = 0; tt < len; ++tt) {
      const long long e = off + 32 * tt;
      Aval2[e] = a.Aval[start + tt]; srcA2[(size_t)e] = srcA[(size_t)(start + tt)]; Acol2[e] = (unsigned short)(a.Acol[start + tt] * (unsigned)sizeof(real)); newpos[(size_t)(start + tt)] = e;
    }
  }
  for (int sx = 0; sx < 16; ++sx) for (int l = 0; l < 32; ++l) {
    const int q = 32 * sx + l;
    const long long off = offT[sx] + l;
    const long long start = q < n ? a.Trp[q] : 0, len = q < n ? a.Trp[q + 1] - a.Trp[q] : 0;
    pl.slT[(size_t)k * 512 + (size_t)q] = (uint32_t)off | ((uint32_t)len << 16);
    for (long long tt = 0; tt < len; ++tt) {
      const uint32_t pr = a.Tpr[start + tt];
      Tpr2[off + 32 * tt] = (uint32_t)(SL_WS0 + h2.oAval + (long long)sizeof(real) * newpos[(size_t)(pr & 0xffffu)]) | ((pr >> 16) << 21);
    }
  }
  if (!p_all_diag) {
    memcpy(i2.data() + h2.oPval, a.Pval, (size_t)nnzP * sizeof(real));
    memcpy(i2.data() + h2.oPrp, a.Prp, (size_t)(n + 1) * 2);
    memcpy(i2.data() + h2.oPcol, a.Pcol, (size_t)nnzP * 2);
  } else {
    const std::vector<int32_t>& uPT = (*in.um_PT)[(size_t)k];
    std::vector<int32_t>& pd = pl.um_pd[(size_t)k];
    pd.assign((size_t)n, -1);
    for (long long j = 0; j < n; ++j) if (PT.split[j] > PT.rowptr[j]) { pl.pdiag[(size_t)k * n + (size_t)j] = PT.val[PT.rowptr[j]]; pl.pdiag_has[(size_t)k * n + (size_t)j] = 1; pd[(size_t)j] = uPT[(size_t)PT.rowptr[j]]; }
  }
  pl.stride2 = std::max(pl.stride2, o2);
  return true;
}

}  // namespace

void plan_batch_images(const BatchImageIn& in, const BatchImageOpts& o, BatchImagePlan& pl) {
  pl = BatchImagePlan();
  const int nprob = in.nprob; const long long n = in.n, m = in.m;
  pl.um_imgA.resize((size_t)nprob); pl.um_imgA2.resize((size_t)nprob); pl.um_imgP.resize((size_t)nprob); pl.um_pd.resize((size_t)nprob);
  if (!choose_form(in, o, pl)) return;
  pl.imgs.resize((size_t)nprob); pl.imgs2.resize((size_t)nprob);
  const bool reg_sorted = pl.reg_mode == 1 && o.sorted;      // SORTED = 0: every thread of the register kernel computes the rows it owns (the form until round 3)
  if (pl.rcg_sorted) { pl.permA.assign((size_t)nprob * 4 * 512, -1); pl.permT.assign((size_t)nprob * 2 * 512, -1); }
  if (reg_sorted) { pl.permA.assign((size_t)nprob * 2 * 512, -1); pl.permT.assign((size_t)nprob * 512, -1); }
  for (int k = 0; k < nprob; ++k) {
    const HostCsr &A = (*in.A)[k], &AT = (*in.AT)[k], &PT = (*in.PT)[k];
    const long long nnzA = (long long)A.val.size(), nnzP = (long long)PT.val.size() - nnzA;
    if (nnzA > 65535 || nnzP > 65535) return;
    std::vector<int> ordA, ordT;
    if (pl.rcg_sorted || reg_sorted) length_order(A, PT, ordA, ordT);
    if (pl.rcg_sorted) {        // the register-CG form's <2, 4>-slot layout: rows serpentine, columns forwards
      assign_serpentine(ordA, true, pl.permA.data() + (size_t)k * 4 * 512);
      assign_serpentine(ordT, false, pl.permT.data() + (size_t)k * 2 * 512);
    }
    // the tile lists of the generic loops are cut on the row pointers of the order the image is stored in
    const std::vector<int> prA = pl.rcg_stored ? ordered_rowptr(A.rowptr, ordA) : A.rowptr, prT = pl.rcg_stored ? ordered_rowptr(AT.rowptr, ordT) : AT.rowptr,
                           prPT = pl.rcg_stored ? ordered_rowptr(PT.rowptr, ordT) : PT.rowptr;
    std::vector<int> rA, rAT, rPT;
    brow_blocks(prA, (int)m, rA); brow_blocks(prT, (int)n, rAT); brow_blocks(prPT, (int)n, rPT);
    const LdsHdr h = layout(n, m, nnzA, nnzP, rA.size() - 1, rAT.size() - 1, rPT.size() - 1, pl.rcg_stored);
    // fit: the image, the two gathered vectors and the block-sum slots (two per wave) within the workgroup's LDS
    if (h.bytes + (long long)sizeof(real) * (n + m) + (long long)sizeof(real) * 2 * (pl.bs / 64) > in.max_lds) return;
    std::vector<unsigned char>& im = pl.imgs[(size_t)k];
    im.assign((size_t)h.bytes, 0);
    memcpy(im.data(), &h, sizeof h);
    const ImgArrays a(im, h);
    std::vector<int32_t>& srcA = pl.um_imgA[(size_t)k]; std::vector<int32_t>& srcP = pl.um_imgP[(size_t)k];
    if (!fill_index_order(A, AT, PT, (*in.um_A)[(size_t)k], (*in.um_PT)[(size_t)k], a, srcA, srcP)) { pl.error = "LDS image: A / A' mismatch"; return; }
    fill_rb(im, h.oRbA, rA, prA); fill_rb(im, h.oRbAT, rAT, prT); fill_rb(im, h.oRbPT, rPT, prPT);
    pl.stride = std::max(pl.stride, (long long)h.bytes);
    if (pl.rcg_stored) {
      store_in_order(ordA, ordT, h, a, srcA, srcP);
      // the generic loops of the LDS-image kernel read the row / column stored at every position from the image
      unsigned short* Aord = reinterpret_cast<unsigned short*>(im.data() + h.oAord);
      unsigned short* Tord = reinterpret_cast<unsigned short*>(im.data() + h.oTord);
      for (long long q = 0; q < m; ++q) Aord[q] = (unsigned short)ordA[(size_t)q];
      for (long long q = 0; q < n; ++q) Tord[q] = (unsigned short)ordT[(size_t)q];
    }
    if (!reg_sorted) continue;
    // register kernel <512, 1, 2>: length-sorted compute assignment (see k_batch_admm_reg)
    int* permA = pl.permA.data() + (size_t)k * 2 * 512; int* permT = pl.permT.data() + (size_t)k * 512;
    assign_serpentine(ordA, true, permA);
    assign_serpentine(ordT, false, permT);
    // STORAGE ORDER of the image = the sorted order (round 5): the 64 rows a wave works on in one trip are NEIGHBOURS in the value / index arrays --
    // lane l reads at (start of its row) + t with starts about one row length apart: a constant-stride access, which the LDS serves at 4.1 (b64) /
    // 2.2 (u16) cycles per wave-read against 7.2 for the scattered reads that CSR order gives a length-sorted assignment (bench/lds_conflict_lab.hip)
    if (o.store_sorted) {
      store_in_order(ordA, ordT, h, a, srcA, srcP);
      // the register kernel derives the positions of its rows / columns from the thread index, and reads the position of the rows it OWNS from D.qposA
      if (pl.qposA.empty()) pl.qposA.assign((size_t)nprob * m, 0);
      for (long long q = 0; q < m; ++q) pl.qposA[(size_t)k * m + (size_t)ordA[(size_t)q]] = (int)q;
    }
    if (o.color) {
      if (pl.posN.empty()) { pl.posN.assign((size_t)nprob * n, 0); pl.posM.assign((size_t)nprob * m, 0); }
      colour_positions(A, AT, PT, permA, permT, h, a, pl.posN.data() + (size_t)k * n, pl.posM.data() + (size_t)k * m);
    }
    if (pl.qposA.empty()) pl.want_sliced = false;             // the sliced image needs the sorted storage order (Arp / Trp / Prp indexed by position)
    if (pl.want_sliced) pl.want_sliced = slice_image(in, k, h, a, srcA, pl);
  }
  pl.fits = true;
}
