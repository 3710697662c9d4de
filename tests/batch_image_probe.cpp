// Test hook for csrc/batch_image.cpp (compiled by tests/test_batch_image_host.py into its own shared object with g++, once per precision; the libraries
// export the C ABI only).  Members are staged from Julia-layout CSC arrays as cosmo_hip_batch_set_problem stages them (A, A', [P | A'] and the source maps
// of value_maps.h), the planner runs with the given switches and max_lds, and every array of the plan is handed out raw.
#include <string.h>
#include "batch_image.h"
#include "value_maps.h"

typedef cosmo_hip_real real;

namespace {
struct Probe {
  BatchImageIn in; BatchImagePlan pl;
  std::vector<HostCsr> A, AT, PT;
  std::vector<std::vector<int32_t>> um_A, um_PT;
};

// CSC (1-based) -> CSR of the transpose (the CSC arrays themselves) and of the matrix (columns ascending inside a row)
void stage(int64_t nr, int64_t nc, const int64_t* colptr, const int64_t* rowval, const real* nzval, HostCsr& Mt, HostCsr& M) {
  const int64_t nnz = colptr[nc] - 1;
  Mt.nrows = (int)nc; Mt.ncols = (int)nr; Mt.rowptr.resize(nc + 1); Mt.col.resize(nnz); Mt.val.assign(nzval, nzval + nnz);
  for (int64_t j = 0; j <= nc; ++j) Mt.rowptr[j] = (int)(colptr[j] - 1);
  M.nrows = (int)nr; M.ncols = (int)nc; M.rowptr.assign(nr + 1, 0); M.col.resize(nnz); M.val.resize(nnz);
  for (int64_t k = 0; k < nnz; ++k) { Mt.col[k] = (int)(rowval[k] - 1); M.rowptr[rowval[k]] += 1; }
  for (int64_t i = 0; i < nr; ++i) M.rowptr[i + 1] += M.rowptr[i];
  std::vector<int> pos(M.rowptr.begin(), M.rowptr.end() - 1);
  for (int64_t j = 0; j < nc; ++j)
    for (int k = Mt.rowptr[j]; k < Mt.rowptr[j + 1]; ++k) { const int p = pos[Mt.col[k]]++; M.col[p] = (int)j; M.val[p] = nzval[k]; }
}
}  // namespace

extern "C" {

void* bimg_probe_new(int nprob, long long n, long long m) {
  Probe* p = new Probe();
  p->in.nprob = nprob; p->in.n = n; p->in.m = m;
  p->A.resize(nprob); p->AT.resize(nprob); p->PT.resize(nprob); p->um_A.resize(nprob); p->um_PT.resize(nprob);
  return p;
}
void bimg_probe_free(void* h) { delete static_cast<Probe*>(h); }
int bimg_probe_real_bytes() { return (int)sizeof(real); }

// member k from the arrays cosmo_hip_batch_set_problem takes; returns 0, or -1 for a malformed pattern
int bimg_probe_set(void* h, int k, const int64_t* Pc, const int64_t* Pr, const real* Pv, const int64_t* Ac, const int64_t* Ar, const real* Av) {
  Probe& p = *static_cast<Probe*>(h);
  const int64_t n = p.in.n, m = p.in.m;
  HostCsr Pt, Pm;
  stage(n, n, Pc, Pr, Pv, Pt, Pm);
  stage(m, n, Ac, Ar, Av, p.AT[k], p.A[k]);
  HostCsr& PT = p.PT[k];
  PT.nrows = (int)n; PT.ncols = (int)(n + m); PT.rowptr.assign(n + 1, 0); PT.split.assign(n, 0);
  for (int64_t j = 0; j < n; ++j) {
    PT.rowptr[j] = (int)PT.col.size();
    for (int t = Pm.rowptr[j]; t < Pm.rowptr[j + 1]; ++t) { PT.col.push_back(Pm.col[t]); PT.val.push_back(Pm.val[t]); }
    PT.split[j] = (int)PT.col.size();
    for (int t = p.AT[k].rowptr[j]; t < p.AT[k].rowptr[j + 1]; ++t) { PT.col.push_back(p.AT[k].col[t] + (int)n); PT.val.push_back(p.AT[k].val[t]); }
  }
  PT.rowptr[n] = (int)PT.col.size();
  std::vector<int> prp, pmap, arp, amap, mrp, msp, mmap;
  if (value_map_csr(n, n, Pc, Pr, prp, pmap) || value_map_csr(m, n, Ac, Ar, arp, amap)) return -1;
  value_map_merged(n, prp, pmap, Ac, mrp, msp, mmap);
  const int32_t nnzP = (int32_t)pmap.size();
  p.um_A[k].resize(amap.size()); p.um_PT[k].resize(mmap.size());
  for (size_t t = 0; t < amap.size(); ++t) p.um_A[k][t] = nnzP + amap[t];
  for (int64_t j = 0; j < n; ++j) {
    for (int t = mrp[j]; t < msp[j]; ++t) p.um_PT[k][(size_t)t] = mmap[(size_t)t];
    for (int t = msp[j]; t < mrp[j + 1]; ++t) p.um_PT[k][(size_t)t] = nnzP + mmap[(size_t)t];
  }
  return 0;
}

// entry t of the staged A' of member k gets another value: the staged copies of A disagree from here on
void bimg_probe_corrupt(void* h, int k, int t) { Probe& p = *static_cast<Probe*>(h); p.AT[k].val[(size_t)t] += (real)1; }

// opts: the eleven switches in BatchImageOpts order; cones = {npsd, nmid, n3}.  Returns 0, 1 if the planner reports an error (bimg_probe_error)
int bimg_probe_plan(void* h, const int* opts, const int* cones, int aa_on, long long max_lds) {
  Probe& p = *static_cast<Probe*>(h);
  BatchImageOpts o;
  o.lds = opts[0]; o.bs = opts[1]; o.ext = opts[2]; o.reg = opts[3]; o.sliced = opts[4]; o.long_rows = opts[5]; o.ldscg = opts[6];
  o.ldscg_sorted = opts[7]; o.store_sorted = opts[8]; o.sorted = opts[9]; o.color = opts[10];
  p.in.A = &p.A; p.in.AT = &p.AT; p.in.PT = &p.PT; p.in.um_A = &p.um_A; p.in.um_PT = &p.um_PT;
  p.in.npsd = cones[0]; p.in.nmid = cones[1]; p.in.n3 = cones[2]; p.in.aa_on = aa_on != 0; p.in.max_lds = max_lds;
  plan_batch_images(p.in, o, p.pl);
  return p.pl.error.empty() ? 0 : 1;
}
const char* bimg_probe_error(const void* h) { return static_cast<const Probe*>(h)->pl.error.c_str(); }

// out = {fits, bs, reg_mode, long_rows, force_ext, want_sliced, p_all_diag, rcg_form, rcg_sorted, rcg_stored, stride, stride2}
void bimg_probe_flags(const void* h, long long out[12]) {
  const BatchImagePlan& pl = static_cast<const Probe*>(h)->pl;
  const long long v[12] = {pl.fits, pl.bs, pl.reg_mode, pl.long_rows, pl.force_ext, pl.want_sliced, pl.p_all_diag, pl.rcg_form, pl.rcg_sorted, pl.rcg_stored,
                           pl.stride, pl.stride2};
  memcpy(out, v, sizeof v);
}

// which: 0 row-major image of member k, 1 its sliced image, 2 permA, 3 permT, 4 posN, 5 posM, 6 qposA, 7 slA, 8 slT, 9 pdiag, 10 pdiag_has (whole batch),
// 11 um_imgA, 12 um_imgA2, 13 um_imgP, 14 um_pd of member k, 15 um_A, 16 um_PT of member k (the inputs).  dst = nullptr: the size in bytes only
long long bimg_probe_get(const void* h, int which, int k, void* dst) {
  const Probe& p = *static_cast<const Probe*>(h);
  const BatchImagePlan& pl = p.pl;
  const void* src = nullptr; size_t bytes = 0;
  auto take = [&](const auto& v) { src = v.data(); bytes = v.size() * sizeof(v[0]); };
  switch (which) {
    case 0: if ((size_t)k < pl.imgs.size()) take(pl.imgs[(size_t)k]); break;
    case 1: if ((size_t)k < pl.imgs2.size()) take(pl.imgs2[(size_t)k]); break;
    case 2: take(pl.permA); break;
    case 3: take(pl.permT); break;
    case 4: take(pl.posN); break;
    case 5: take(pl.posM); break;
    case 6: take(pl.qposA); break;
    case 7: take(pl.slA); break;
    case 8: take(pl.slT); break;
    case 9: take(pl.pdiag); break;
    case 10: take(pl.pdiag_has); break;
    case 11: if ((size_t)k < pl.um_imgA.size()) take(pl.um_imgA[(size_t)k]); break;
    case 12: if ((size_t)k < pl.um_imgA2.size()) take(pl.um_imgA2[(size_t)k]); break;
    case 13: if ((size_t)k < pl.um_imgP.size()) take(pl.um_imgP[(size_t)k]); break;
    case 14: if ((size_t)k < pl.um_pd.size()) take(pl.um_pd[(size_t)k]); break;
    case 15: take(p.um_A[(size_t)k]); break;
    case 16: take(p.um_PT[(size_t)k]); break;
  }
  if (dst && bytes) memcpy(dst, src, bytes);
  return (long long)bytes;
}

}  // extern "C"
