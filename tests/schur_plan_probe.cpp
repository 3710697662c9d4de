// schur_plan_probe.cpp -- test-only stand-alone program that walks the maps of the Schur-complement KKT solver's host plan (csrc/schur_plan.cpp,
// csrc/schur_plan.h).  tests/test_schur_plan_host.py compiles it together with schur_plan.cpp with -fsanitize=address,undefined and runs it as a program.
//
// stdin:  n m row_threshold, then the CSR of P (n + 1 row pointers, the columns) and of A (m + 1 row pointers, the columns), whitespace separated.
// The program checks that every index of every map is in range (exit status 2 with a message otherwise) and prints the plan:
//   figures nd ncomp largest sumsq nnz_w n_small n_wave
//   perm <n variables in block order>
//   block <k> <first position> <side> <offset>
//   entry <variable i> <variable j> <terms...>      one line per listed block entry; a term is S (sigma), P<k> or A<ka>:<kb>:<row>
//   ad <row of A> <src...>                          one line per long row: the CSR positions of its entries
//   adt <variable j> <kd:src ...>                   one line per variable that a long row touches
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "schur_plan.h"

static void fail(const char* what) {
  fprintf(stderr, "schur_plan_probe: %s\n", what);
  exit(2);
}
#define REQUIRE(cond) do { if (!(cond)) fail(#cond); } while (0)

static void read_ints(std::vector<int>& v, size_t count) {
  v.resize(count);
  for (size_t i = 0; i < count; ++i)
    if (scanf("%d", &v[i]) != 1) fail("short input");
}

int main() {
  long long n = 0, m = 0;
  int threshold = 0;
  if (scanf("%lld %lld %d", &n, &m, &threshold) != 3) fail("no header");
  std::vector<int> pp, pc, ap, ac;
  read_ints(pp, (size_t)n + 1); read_ints(pc, (size_t)pp[n]);
  read_ints(ap, (size_t)m + 1); read_ints(ac, (size_t)ap[m]);
  SchurPlan S;
  const char* err = nullptr;
  if (schur_analyze(n, m, pp, pc, ap, ac, threshold, S, &err) != 0) fail(err ? err : "analysis failed");
  const long long nnzP = pp[n], nnzA = ap[m];
  // the permutation and the blocks
  REQUIRE((long long)S.perm.size() == n && (long long)S.pos.size() == n && (long long)S.blk_of_pos.size() == n);
  REQUIRE((long long)S.comp_ptr.size() == S.ncomp + 1 && (long long)S.boff.size() == S.ncomp + 1);
  std::vector<char> seen((size_t)n, 0);
  for (long long p = 0; p < n; ++p) {
    REQUIRE(S.perm[p] >= 0 && S.perm[p] < n && !seen[S.perm[p]]);
    seen[S.perm[p]] = 1;
    REQUIRE(S.pos[S.perm[p]] == p);
    const int k = S.blk_of_pos[p];
    REQUIRE(k >= 0 && k < S.ncomp && S.comp_ptr[k] <= p && p < S.comp_ptr[k + 1]);
  }
  REQUIRE(S.comp_ptr[0] == 0 && S.comp_ptr[S.ncomp] == n && S.boff[0] == 0 && S.boff[S.ncomp] == S.sumsq);
  long long prev = 0;
  for (long long k = 0; k < S.ncomp; ++k) {
    const long long s = S.comp_ptr[k + 1] - S.comp_ptr[k];
    REQUIRE(s >= 1 && s >= prev && S.boff[k + 1] - S.boff[k] == s * s);       // ordered by size: equal sides are neighbours
    REQUIRE((k < S.n_small) == (s <= SCHUR_SMALL_MAX) && (k < S.n_wave) == (s <= SCHUR_WAVE_MAX));
    for (int p = S.comp_ptr[k] + 1; p < S.comp_ptr[k + 1]; ++p) REQUIRE(S.perm[p - 1] < S.perm[p]);
    prev = s;
  }
  printf("figures %lld %lld %lld %lld %lld %d %d\n", (long long)S.nd, (long long)S.ncomp, (long long)S.largest, (long long)S.sumsq, (long long)S.nnz_w, S.n_small, S.n_wave);
  printf("perm");
  for (long long p = 0; p < n; ++p) printf(" %d", S.perm[p]);
  printf("\n");
  for (long long k = 0; k < S.ncomp; ++k) printf("block %lld %d %d %lld\n", k, S.comp_ptr[k], S.comp_ptr[k + 1] - S.comp_ptr[k], (long long)S.boff[k]);
  // the refill map
  const size_t ne = S.epos.size();
  REQUIRE(S.eptr.size() == ne + 1 && S.eptr[0] == 0 && (size_t)S.eptr[ne] == S.ta.size() && S.tb.size() == S.ta.size() && S.trow.size() == S.ta.size());
  for (size_t e = 0; e < ne; ++e) {
    REQUIRE(S.epos[e] >= 0 && S.epos[e] < S.sumsq && (e == 0 || S.epos[e] > S.epos[e - 1]) && S.eptr[e + 1] > S.eptr[e]);
    // the block of the entry: the last one whose offset is <= epos
    long long lo = 0, hi = S.ncomp - 1;
    while (lo < hi) { const long long mid = (lo + hi + 1) / 2; if (S.boff[mid] <= S.epos[e]) lo = mid; else hi = mid - 1; }
    const long long s = S.comp_ptr[lo + 1] - S.comp_ptr[lo], off = S.epos[e] - S.boff[lo];
    printf("entry %d %d", S.perm[S.comp_ptr[lo] + off / s], S.perm[S.comp_ptr[lo] + off % s]);
    for (long long t = S.eptr[e]; t < S.eptr[e + 1]; ++t) {
      if (S.tb[t] == -2) printf(" S");
      else if (S.tb[t] == -1) { REQUIRE(S.ta[t] >= 0 && S.ta[t] < nnzP); printf(" P%d", S.ta[t]); }
      else {
        REQUIRE(S.ta[t] >= 0 && S.ta[t] < nnzA && S.tb[t] >= 0 && S.tb[t] < nnzA && S.trow[t] >= 0 && S.trow[t] < m);
        REQUIRE(ap[S.trow[t]] <= S.ta[t] && S.ta[t] < ap[S.trow[t] + 1] && ap[S.trow[t]] <= S.tb[t] && S.tb[t] < ap[S.trow[t] + 1]);
        printf(" A%d:%d:%d", S.ta[t], S.tb[t], S.trow[t]);
      }
    }
    printf("\n");
  }
  // the long rows and their transpose
  REQUIRE((long long)S.ad_row.size() == S.nd && (long long)S.ad_ptr.size() == S.nd + 1 && S.ad_col.size() == S.ad_src.size());
  REQUIRE((long long)S.adt_ptr.size() == n + 1 && S.adt_k.size() == S.ad_col.size() && S.adt_src.size() == S.ad_col.size());
  REQUIRE(S.ad_ptr[0] == 0 && (size_t)S.ad_ptr[S.nd] == S.ad_col.size() && S.adt_ptr[0] == 0 && (size_t)S.adt_ptr[n] == S.ad_col.size());
  for (long long kd = 0; kd < S.nd; ++kd) {
    const int i = S.ad_row[kd];
    REQUIRE(i >= 0 && i < m && S.ad_ptr[kd + 1] - S.ad_ptr[kd] == ap[i + 1] - ap[i]);
    printf("ad %d", i);
    for (int p = S.ad_ptr[kd]; p < S.ad_ptr[kd + 1]; ++p) {
      REQUIRE(S.ad_src[p] >= ap[i] && S.ad_src[p] < ap[i + 1] && S.ad_col[p] == ac[S.ad_src[p]]);
      printf(" %d", S.ad_src[p]);
    }
    printf("\n");
  }
  for (long long j = 0; j < n; ++j) {
    REQUIRE(S.adt_ptr[j + 1] >= S.adt_ptr[j]);
    if (S.adt_ptr[j + 1] == S.adt_ptr[j]) continue;
    printf("adt %lld", j);
    for (int p = S.adt_ptr[j]; p < S.adt_ptr[j + 1]; ++p) {
      REQUIRE(S.adt_k[p] >= 0 && S.adt_k[p] < S.nd && S.adt_src[p] >= 0 && S.adt_src[p] < nnzA && ac[S.adt_src[p]] == j);
      REQUIRE(p == S.adt_ptr[j] || S.adt_k[p - 1] <= S.adt_k[p]);
      printf(" %d:%d", S.adt_k[p], S.adt_src[p]);
    }
    printf("\n");
  }
  return 0;
}
