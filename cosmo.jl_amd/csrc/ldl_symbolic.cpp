// ldl_symbolic.cpp -- symbolic analysis of the direct KKT solver (COSMO_HIP_KKT_DIRECT), host only, pattern only (see ldl.h).
//
//   1. ordering: the rows of A with at most one nonzero are degree <= 1 nodes of K's graph and go first (no fill); the other nodes are ordered
//      by approximate minimum degree on the quotient graph (Amestoy, Davis, Duff, SIAM J. Matrix Anal. Appl. 17(4), 1996: elements formed by
//      elimination, element absorption, the approximate external degree bound of section 3).  Supervariables / mass elimination are left out.
//   2. elimination tree and column counts (Liu's row-subtree walk), a postorder of the tree (same fill, contiguous subtrees), the pattern of L;
//   3. maximal supernodes (fundamental ones without the single-child condition; no explicit zeros), the supernodal tree, its level schedule
//      and the left-looking update lists of ldl.hip.
#include "ldl.h"
#include "../../include/cosmo_hip.h"
#include <algorithm>
#include <chrono>
#include <string.h>

namespace {

struct Graph {   // symmetric adjacency without self loops
  std::vector<int64_t> ptr, adj;
};

Graph build_graph(int64_t N, const std::vector<std::pair<int64_t, int64_t>>& edges) {
  Graph G;
  G.ptr.assign(N + 1, 0);
  for (auto& e : edges) { G.ptr[e.first + 1] += 1; G.ptr[e.second + 1] += 1; }
  for (int64_t i = 0; i < N; ++i) G.ptr[i + 1] += G.ptr[i];
  G.adj.resize(G.ptr[N]);
  std::vector<int64_t> fill(G.ptr.begin(), G.ptr.end() - 1);
  for (auto& e : edges) { G.adj[fill[e.first]++] = e.second; G.adj[fill[e.second]++] = e.first; }
  // sort + unique every list
  std::vector<int64_t> np(N + 1, 0);
  int64_t w = 0;
  for (int64_t i = 0; i < N; ++i) {
    auto b = G.adj.begin() + G.ptr[i], e = G.adj.begin() + G.ptr[i + 1];
    std::sort(b, e);
    int64_t last = -1;
    np[i] = w;
    for (auto it = b; it != e; ++it) if (*it != last) { last = *it; G.adj[w++] = *it; }
  }
  np[N] = w;
  G.adj.resize(w);
  G.ptr.swap(np);
  return G;
}

// Approximate minimum degree on the subgraph of `nodes` (indices into G); appends the elimination order to `order`.
void amd_order(const Graph& G, const std::vector<int64_t>& nodes, std::vector<int64_t>& order) {
  const int64_t nn = (int64_t)nodes.size();
  if (nn == 0) return;
  std::vector<int64_t> loc(G.ptr.size() - 1, -1);
  for (int64_t k = 0; k < nn; ++k) loc[nodes[k]] = k;
  std::vector<std::vector<int64_t>> Av(nn), Ev(nn), Le(nn);
  for (int64_t k = 0; k < nn; ++k) {
    const int64_t g = nodes[k];
    for (int64_t q = G.ptr[g]; q < G.ptr[g + 1]; ++q) { const int64_t l = loc[G.adj[q]]; if (l >= 0) Av[k].push_back(l); }
  }
  std::vector<int8_t> state(nn, 0);             // 0 variable, 1 element, 2 absorbed element
  std::vector<int64_t> deg(nn), head(nn + 1, -1), nxt(nn, -1), prv(nn, -1);
  auto insert = [&](int64_t i) { const int64_t d = deg[i]; nxt[i] = head[d]; prv[i] = -1; if (head[d] >= 0) prv[head[d]] = i; head[d] = i; };
  auto remove = [&](int64_t i) {
    if (prv[i] >= 0) nxt[prv[i]] = nxt[i]; else head[deg[i]] = nxt[i];
    if (nxt[i] >= 0) prv[nxt[i]] = prv[i];
  };
  for (int64_t i = nn - 1; i >= 0; --i) { deg[i] = (int64_t)Av[i].size(); insert(i); }
  std::vector<int64_t> inLp(nn, -1), wst(nn, -1), wv(nn, 0), Lp;
  int64_t mindeg = 0;
  for (int64_t step = 0; step < nn; ++step) {
    while (head[mindeg] < 0) ++mindeg;
    const int64_t p = head[mindeg];
    remove(p);
    order.push_back(nodes[p]);
    // L_p = (A_p u (union of the elements of p)) \ {p}; the elements of p are absorbed into the new element p
    Lp.clear();
    inLp[p] = step;
    for (int64_t j : Av[p]) if (state[j] == 0 && inLp[j] != step) { inLp[j] = step; Lp.push_back(j); }
    for (int64_t e : Ev[p]) {
      if (state[e] != 1) continue;
      for (int64_t j : Le[e]) if (state[j] == 0 && inLp[j] != step) { inLp[j] = step; Lp.push_back(j); }
      state[e] = 2;
      std::vector<int64_t>().swap(Le[e]);
    }
    state[p] = 1;
    std::vector<int64_t>().swap(Av[p]);
    std::vector<int64_t>().swap(Ev[p]);
    const int64_t remaining = nn - step - 1;
    // prune the lists of the variables of L_p: dead elements out, p in; variables that are now reached through p out of A_i
    for (int64_t i : Lp) {
      remove(i);
      auto& E = Ev[i];
      int64_t w = 0;
      for (int64_t e : E) if (state[e] == 1) E[w++] = e;
      E.resize(w);
      E.push_back(p);
      auto& A = Av[i];
      w = 0;
      for (int64_t j : A) if (state[j] == 0 && inLp[j] != step) A[w++] = j;
      A.resize(w);
    }
    // |L_e \ L_p| for every other element adjacent to L_p
    for (int64_t i : Lp)
      for (int64_t e : Ev[i]) {
        if (e == p) continue;
        if (wst[e] != step) { wst[e] = step; wv[e] = (int64_t)Le[e].size(); }
        wv[e] -= 1;
      }
    const int64_t lp = (int64_t)Lp.size();
    for (int64_t i : Lp) {
      int64_t d = (int64_t)Av[i].size() + (lp - 1);
      for (int64_t e : Ev[i]) {
        if (e == p || state[e] != 1) continue;
        if (wv[e] == 0) { state[e] = 2; std::vector<int64_t>().swap(Le[e]); continue; }   // L_e inside L_p: absorbed
        d += wv[e];
      }
      d = std::min(d, std::min(remaining - 1, deg[i] + lp - 1));
      if (d < 0) d = 0;
      deg[i] = d;
      insert(i);
      if (d < mindeg) mindeg = d;
    }
    Le[p] = Lp;
  }
}

// Elimination tree of the permuted pattern (upper column k = permuted neighbours j < k) and the strictly lower counts of L's columns;
// optionally the row pattern of every column (rows ascending).
int64_t etree(int64_t N, const std::vector<int64_t>& up, const std::vector<int64_t>& ui, std::vector<int64_t>& parent, std::vector<int64_t>& cnt,
              std::vector<int64_t>* Lp, std::vector<int32_t>* Li) {
  parent.assign(N, -1); cnt.assign(N, 0);
  std::vector<int64_t> flag(N, -1);
  for (int64_t k = 0; k < N; ++k) {
    flag[k] = k;
    for (int64_t q = up[k]; q < up[k + 1]; ++q) {
      int64_t j = ui[q];
      while (flag[j] != k) {
        if (parent[j] == -1) parent[j] = k;
        cnt[j] += 1; flag[j] = k; j = parent[j];
      }
    }
  }
  int64_t nnz = 0;
  for (int64_t j = 0; j < N; ++j) nnz += cnt[j];
  if (Lp) {
    Lp->assign(N + 1, 0);
    for (int64_t j = 0; j < N; ++j) (*Lp)[j + 1] = (*Lp)[j] + cnt[j];
    Li->resize(nnz);
    std::vector<int64_t> fill(Lp->begin(), Lp->end() - 1);
    std::fill(flag.begin(), flag.end(), -1);
    for (int64_t k = 0; k < N; ++k) {
      flag[k] = k;
      for (int64_t q = up[k]; q < up[k + 1]; ++q) {
        int64_t j = ui[q];
        while (flag[j] != k) { (*Li)[fill[j]++] = (int32_t)k; flag[j] = k; j = parent[j]; }
      }
    }
  }
  return nnz;
}

// upper pattern of G[perm, perm]: column k holds the permuted neighbours j < k
void permuted_upper(const Graph& G, const std::vector<int64_t>& perm, const std::vector<int64_t>& iperm, std::vector<int64_t>& up,
                    std::vector<int64_t>& ui) {
  const int64_t N = (int64_t)perm.size();
  up.assign(N + 1, 0);
  for (int64_t k = 0; k < N; ++k) {
    const int64_t g = perm[k];
    int64_t c = 0;
    for (int64_t q = G.ptr[g]; q < G.ptr[g + 1]; ++q) c += (iperm[G.adj[q]] < k);
    up[k + 1] = up[k] + c;
  }
  ui.resize(up[N]);
  for (int64_t k = 0; k < N; ++k) {
    const int64_t g = perm[k];
    int64_t w = up[k];
    for (int64_t q = G.ptr[g]; q < G.ptr[g + 1]; ++q) { const int64_t j = iperm[G.adj[q]]; if (j < k) ui[w++] = j; }
  }
}

}  // namespace

int64_t LdlSymbolic::slot(int64_t i, int64_t j) const {
  int64_t a = iperm[i], b = iperm[j];
  if (a < b) std::swap(a, b);                     // lower triangle: row a >= column b
  const int64_t J = sn_of[b];
  const int64_t f = sn_first[J], w = sn_first[J + 1] - f, nr = sn_rp[J + 1] - sn_rp[J];
  int64_t r;
  if (a < f + w) {
    r = a - f;
  } else {
    const int32_t* rows = sn_rows.data() + sn_rp[J];
    const int32_t* pos = std::lower_bound(rows + w, rows + nr, (int32_t)a);
    if (pos == rows + nr || *pos != a) return -1;
    r = pos - rows;
  }
  return sn_poff[J] + (b - f) * nr + r;
}

int ldl_analyze(int64_t n, int64_t m, const std::vector<int64_t>& p_row, const std::vector<int64_t>& p_col, const std::vector<int64_t>& a_row,
                const std::vector<int64_t>& a_col, const int64_t* perm_in, LdlSymbolic& S, const char** err) {
  const auto t0 = std::chrono::steady_clock::now();
  const int64_t N = n + m;
  S = LdlSymbolic();
  S.n = n; S.m = m; S.N = N;
  if (N >= 2147483647LL) { *err = "n + m out of int32 range"; return -1; }
  std::vector<std::pair<int64_t, int64_t>> edges;
  edges.reserve(p_row.size() + a_row.size());
  for (size_t k = 0; k < p_row.size(); ++k) if (p_row[k] != p_col[k]) edges.emplace_back(p_row[k], p_col[k]);
  std::vector<int64_t> rowcnt(m, 0);
  for (size_t k = 0; k < a_row.size(); ++k) { edges.emplace_back(n + a_row[k], a_col[k]); rowcnt[a_row[k]] += 1; }
  const Graph G = build_graph(N, edges);
  std::vector<int64_t>().swap(rowcnt);
  std::vector<std::pair<int64_t, int64_t>>().swap(edges);

  // ---- ordering
  std::vector<int64_t> order;
  order.reserve(N);
  if (perm_in) {
    std::vector<char> seen(N, 0);
    for (int64_t k = 0; k < N; ++k) {
      const int64_t v = perm_in[k];
      if (v < 0 || v >= N || seen[v]) { *err = "perm is not a permutation of 0 .. n+m-1"; return -1; }
      seen[v] = 1;
      order.push_back(v);
    }
  } else {
    std::vector<int64_t> rest;
    for (int64_t i = 0; i < m; ++i) {
      const int64_t g = n + i;
      if (G.ptr[g + 1] - G.ptr[g] <= 1) order.push_back(g); else rest.push_back(g);
    }
    std::vector<int64_t> nodes;
    nodes.reserve(n + rest.size());
    for (int64_t j = 0; j < n; ++j) nodes.push_back(j);
    nodes.insert(nodes.end(), rest.begin(), rest.end());
    amd_order(G, nodes, order);
  }
  // ---- elimination tree of the ordering, then its postorder (children in ascending order): the same fill, subtrees contiguous
  std::vector<int64_t> iperm(N), up, ui, parent, cnt;
  for (int64_t k = 0; k < N; ++k) iperm[order[k]] = k;
  permuted_upper(G, order, iperm, up, ui);
  etree(N, up, ui, parent, cnt, nullptr, nullptr);
  {
    std::vector<int64_t> chead(N, -1), cnext(N, -1), post;
    post.reserve(N);
    for (int64_t j = N - 1; j >= 0; --j) if (parent[j] >= 0) { cnext[j] = chead[parent[j]]; chead[parent[j]] = j; }
    std::vector<int64_t> stack;
    for (int64_t r = 0; r < N; ++r) {
      if (parent[r] != -1) continue;
      stack.push_back(r);
      while (!stack.empty()) {            // iterative DFS: a node is emitted after all its children
        const int64_t v = stack.back();
        if (chead[v] >= 0) { const int64_t c = chead[v]; chead[v] = cnext[c]; stack.push_back(c); }
        else { post.push_back(v); stack.pop_back(); }
      }
    }
    std::vector<int64_t> o2(N);
    for (int64_t k = 0; k < N; ++k) o2[k] = order[post[k]];
    order.swap(o2);
  }
  for (int64_t k = 0; k < N; ++k) iperm[order[k]] = k;
  permuted_upper(G, order, iperm, up, ui);
  std::vector<int64_t> Lp;
  std::vector<int32_t> Li;
  S.nnz_L = etree(N, up, ui, parent, cnt, &Lp, &Li);
  S.perm = order; S.iperm = iperm;

  // ---- maximal supernodes: j + 1 joins the supernode of j when parent(j) = j + 1 and |L(:, j)| = |L(:, j+1)| + 1.  Unlike FUNDAMENTAL
  // supernodes, j need not be the only child of j + 1: the pattern of L(:, j) is still {j + 1} u pattern(L(:, j + 1)), so the columns share one
  // row structure and no explicit zero is stored; other children of j + 1 simply update a supernode whose first column is not j + 1.
  S.sn_of.assign(N, 0);
  S.sn_first.clear();
  for (int64_t j = 0; j < N; ++j) {
    if (j == 0 || !(parent[j - 1] == j && cnt[j - 1] == cnt[j] + 1)) S.sn_first.push_back(j);
    S.sn_of[j] = (int32_t)(S.sn_first.size() - 1);
  }
  S.ns = (int64_t)S.sn_first.size();
  S.sn_first.push_back(N);
  const int64_t ns = S.ns;
  S.sn_rp.assign(ns + 1, 0); S.sn_poff.assign(ns + 1, 0); S.sn_parent.assign(ns, -1);
  for (int64_t J = 0; J < ns; ++J) {
    const int64_t f = S.sn_first[J], l = S.sn_first[J + 1], w = l - f;
    const int64_t nr = w + cnt[l - 1];
    S.sn_rp[J + 1] = S.sn_rp[J] + nr;
    S.sn_poff[J + 1] = S.sn_poff[J] + nr * w;
    S.nnz_stored += nr * w - w * (w + 1) / 2;
    S.max_width = std::max(S.max_width, w);
    if (parent[l - 1] >= 0) S.sn_parent[J] = S.sn_of[parent[l - 1]];
  }
  S.panel_size = S.sn_poff[ns];
  S.sn_rows.resize(S.sn_rp[ns]);
  for (int64_t J = 0; J < ns; ++J) {
    const int64_t f = S.sn_first[J], l = S.sn_first[J + 1];
    int64_t w = S.sn_rp[J];
    for (int64_t c = f; c < l; ++c) S.sn_rows[w++] = (int32_t)c;
    for (int64_t q = Lp[l - 1]; q < Lp[l]; ++q) S.sn_rows[w++] = Li[q];
  }
  // ---- level schedule
  std::vector<int32_t> level(ns, 0);
  int32_t H = 0;
  for (int64_t J = 0; J < ns; ++J) {
    H = std::max(H, level[J] + 1);
    if (S.sn_parent[J] >= 0) level[S.sn_parent[J]] = std::max(level[S.sn_parent[J]], level[J] + 1);
  }
  S.height = H;
  S.lvl_ptr.assign(H + 1, 0);
  for (int64_t J = 0; J < ns; ++J) S.lvl_ptr[level[J] + 1] += 1;
  for (int32_t h = 0; h < H; ++h) S.lvl_ptr[h + 1] += S.lvl_ptr[h];
  S.lvl_sn.resize(ns);
  { std::vector<int32_t> fill(S.lvl_ptr.begin(), S.lvl_ptr.end() - 1);
    for (int64_t J = 0; J < ns; ++J) S.lvl_sn[fill[level[J]]++] = (int32_t)J; }
  // ---- left-looking update lists (descendants in ascending order)
  std::vector<int32_t> pairs;   // J, K, r0, r1
  for (int64_t K = 0; K < ns; ++K) {
    const int64_t w = S.sn_first[K + 1] - S.sn_first[K], b = S.sn_rp[K], nr = S.sn_rp[K + 1] - b;
    int64_t r = w;
    while (r < nr) {
      const int32_t J = S.sn_of[S.sn_rows[b + r]];
      int64_t r1 = r + 1;
      while (r1 < nr && S.sn_of[S.sn_rows[b + r1]] == J) ++r1;
      pairs.push_back(J); pairs.push_back((int32_t)K); pairs.push_back((int32_t)r); pairs.push_back((int32_t)r1);
      r = r1;
    }
  }
  const int64_t np = (int64_t)pairs.size() / 4;
  if (3 * np >= 2147483647LL) { *err = "left-looking update lists out of int32 range"; return -1; }
  S.desc_ptr.assign(ns + 1, 0);
  for (int64_t q = 0; q < np; ++q) S.desc_ptr[pairs[4 * q] + 1] += 1;
  for (int64_t J = 0; J < ns; ++J) S.desc_ptr[J + 1] += S.desc_ptr[J];
  S.desc.resize(3 * np);
  { std::vector<int32_t> fill(S.desc_ptr.begin(), S.desc_ptr.end() - 1);
    for (int64_t q = 0; q < np; ++q) {         // pairs are generated with K ascending: each list stays ascending
      const int32_t d = fill[pairs[4 * q]]++;
      S.desc[3 * d] = pairs[4 * q + 1]; S.desc[3 * d + 1] = pairs[4 * q + 2]; S.desc[3 * d + 2] = pairs[4 * q + 3];
    } }
  S.amalg_zeros = 0;
  S.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

// out = {nnz(L) without amalgamation zeros, strictly lower entries stored, supernodes, tree height in supernodes, widest supernode,
//        amalgamation zeros, panel values allocated on the device, left-looking update pairs}
extern "C" COSMO_HIP_API int32_t cosmo_hip_ldl_analyze(int64_t n, int64_t m, const int64_t* P_colptr, const int64_t* P_rowval, const int64_t* A_colptr,
                                                      const int64_t* A_rowval, const int64_t* perm, int64_t* out) {
  if (n < 0 || m < 0 || !P_colptr || !A_colptr || !out) return COSMO_HIP_ERR_INVALID;
  std::vector<int64_t> pr, pc, ar, ac;
  for (int64_t j = 0; j < n; ++j)
    for (int64_t q = P_colptr[j]; q < P_colptr[j + 1]; ++q) {
      const int64_t i = P_rowval[q];
      if (i < 0 || i >= n) return COSMO_HIP_ERR_INVALID;
      if (i < j) { pr.push_back(i); pc.push_back(j); }        // upper triangle of P (assemble_kkt_triangle, :U)
    }
  for (int64_t j = 0; j < n; ++j)
    for (int64_t q = A_colptr[j]; q < A_colptr[j + 1]; ++q) {
      const int64_t i = A_rowval[q];
      if (i < 0 || i >= m) return COSMO_HIP_ERR_INVALID;
      ar.push_back(i); ac.push_back(j);
    }
  LdlSymbolic S;
  const char* err = nullptr;
  if (ldl_analyze(n, m, pr, pc, ar, ac, perm, S, &err) != 0) return COSMO_HIP_ERR_INVALID;
  out[0] = S.nnz_L; out[1] = S.nnz_stored; out[2] = S.ns; out[3] = S.height; out[4] = S.max_width; out[5] = S.amalg_zeros;
  out[6] = S.panel_size; out[7] = (int64_t)S.desc.size() / 3;
  return COSMO_HIP_OK;
}
