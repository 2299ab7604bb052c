// grim_refresh.h -- EM on a fixed support: the graph's frequencies from M-step counts, on the device (gfx950, wave64;
// include/grim_hip.h, grim_graph_refresh*).
//
// Contract (every sum's order is part of it).
//   Inputs: a device graph g (V nodes, P populations, full_mask, node_key, node_mask, a_start, a_nbr, n_a_nbr, lab_start,
//     lab_nodes) and counts C, a partial map (haplotype key below bit GRIM_KEY_GRAPH_ORDER, population) -> double, that comes
//     through one of two doors: a grim_em accumulator, where its table lies (an entry exists when the slot of the key exists
//     and bit p of its popmask is set), or host arrays keys / pops / counts [n] in grim_em_export's order.
//   Full nodes: the nodes with node_mask == full_mask in node-id order f_0 < ... < f_{F-1}, i.e.
//     lab_nodes[lab_start[full_mask] .. lab_start[full_mask + 1]).  c[i][p] = C(node_key[f_i] & GRIM_EM_KEYMASK, p) when the
//     map holds that entry, else +0.0.  Counts of haplotypes that are not full nodes of g take no part anywhere (Plan-B joins,
//     everything on the spill list): the support is fixed.
//   Totals, with B = GRIM_REFRESH_BLOCK: s_b[p] = ((+0.0 + c[bB][p]) + c[bB+1][p]) + ... over the block's positions,
//     T_p = ((+0.0 + s_0[p]) + s_1[p]) + ... over the blocks in order; fp64, no fma (-ffp-contract=off).
//   New frequencies: new[f_i][p] = c[i][p] / T_p, one IEEE division.  For a partial node v (node_mask[v] != full_mask) with
//     the row R(v) = a_nbr[a_start[v] .. e(v)), e(v) = a_start[v + 1] for v < V - 1 and e(V - 1) = n_a_nbr (a_start[V] holds
//     the reference's sentinel quirk, not an end, and is never read as one):
//     new[v][p] = ((+0.0 + new[r_0][p]) + new[r_1][p]) + ... in the row's stored order, which is ascending full id.
//     The fht entry of key k gets f0 = new[n][0], n the highest-numbered full node of that key (what grim_graph_upload does
//     with a repeated name).
//   Refreshable graphs: decided on the host inside grim_graph_upload from the descriptor (refresh_check_rows, below the
//     kernels): the rows of the partial nodes, in node order with e(v) as above, tile a_nbr[0 .. n_a_nbr) without gap or
//     overlap; every row is non-empty; every entry is a full node; every entry's key cut to the slots of node_mask[v] equals
//     node_key[v].  The quirks of a_start make a node without rows alias its neighbour's, so the kernels trust the array no
//     further than this check; they still compare every a_nbr entry against V before it indexes anything.
//   Refusals answer -3 with a text, launch nothing that writes freq or fht and leave every bit of both as it was.  The new
//     values go to a shadow buffer; the totals are read before anything is committed.
//   Commit: the shadow is copied over freq IN PLACE (batches and streams hold DevGraph by value) and the fht entries are
//     patched.  The caller guarantees that no batch or stream of the graph is in flight.
//   Statistics: total[p] = T_p; delta = the largest |new - old| over the full nodes and populations (a max: exact, order-free);
//     matched = the (i, p) with an entry; zero_full = the full nodes whose new vector is all zero; n_full = F.
//   Not defined here: no floor, no pseudo-count, no new haplotypes, no merge of several devices' counts.
//
// Deliberately plain: no floating-point atomics, no inline assembly, integer atomics only for the statistics.
//   rf_lookup_kernel   one lane per (full node, population): c into a dense [F][P] array.  One routine (rf_count) behind both
//                      doors: a read-only probe of the EmTable (em_find_or_insert without the insert) or a binary search in
//                      the uploaded sorted records.
//   rf_blocksum_kernel one wave per block of B positions: 64 positions x P at a time come into LDS with coalesced loads, lanes
//                      p < P fold them in position order into a running register.
//   rf_total_kernel    ONE wave folds the <= F / B block sums in order.
//   rf_divide_kernel   one lane per full node: the P divisions into the shadow, delta and zero_full.
//   rf_short_kernel    partial nodes whose row has at most RF_SHORT_MAX entries: one lane per (node, population), so 64 / P rows
//                      share a wave and the P lanes of a row gather one contiguous frequency vector per entry.
//   rf_long_kernel     the other partial nodes, one wave each: the lanes gather 64 entries at a time into LDS and lanes p < P
//                      fold them in lane (= row) order, as mt_pair_kernel folds its chunks.
//   rf_fht_kernel      one lane per full node: writes f0 of its key's fht entry when the exact-name index maps the key to it.
#pragma once
#include "grim_em.h"

#define RF_SHORT_MAX 32u  // longest row rf_short_kernel takes
#define RF_CHUNK 64u      // entries / positions a wave folds per step
enum { RF_S_MATCHED = 0, RF_S_ZERO_FULL = 1, RF_S_DELTA = 2, RF_S_FAULT = 3, RF_S_COUNT = 4 };

// where the counts come from: the accumulator's table (records == 0) or sorted host records on the device
struct RfCounts {
  EmTable T;
  const unsigned long long *keys;  // [n] ascending in (key, pop)
  const uint32_t *pops;
  const double *counts;
  unsigned long long n;
  uint32_t records;
};

// C(key, pop): true and the count when the map holds the entry
__device__ __forceinline__ bool rf_count(const RfCounts &C, uint64_t key, uint32_t pop, double &out) {
  if (C.records) {
    unsigned long long lo = 0, hi = C.n;  // the first entry >= (key, pop)
    while (lo < hi) {
      const unsigned long long mid = lo + ((hi - lo) >> 1);
      const unsigned long long k = C.keys[mid];
      if (k < key || (k == key && C.pops[mid] < pop))
        lo = mid + 1;
      else
        hi = mid;
    }
    if (lo >= C.n || C.keys[lo] != key || C.pops[lo] != pop) return false;
    out = C.counts[lo];
    return true;
  }
  const unsigned long long word = key | GRIM_VALID;
  uint32_t s = (uint32_t)mix64(key) & C.T.mask;
  for (uint32_t turn = 0; turn <= C.T.mask; ++turn) {
    const unsigned long long cur = C.T.keys[s];
    if (cur == 0ull) return false;
    if (cur == word) {
      if (!((C.T.popmask[s] >> pop) & 1ull)) return false;
      out = C.T.counts[(uint64_t)s * C.T.P + pop];
      return true;
    }
    s = (s + 1u) & C.T.mask;
  }
  return false;
}

// full[i] = the i-th full node; c[i * P + p]
__global__ __launch_bounds__(256) void rf_lookup_kernel(const uint32_t *full, uint32_t F, uint32_t V, uint32_t P, const uint64_t *node_key,
                                                        RfCounts C, double *c, unsigned long long *stat) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  uint32_t hit = 0;
  if (t < (uint64_t)F * P) {
    const uint32_t i = (uint32_t)(t / P), p = (uint32_t)(t - (uint64_t)i * P);
    const uint32_t node = full[i];
    double v = 0.0;
    if (node < V)
      hit = rf_count(C, node_key[node] & GRIM_EM_KEYMASK, p, v) ? 1u : 0u;
    else
      atomicAdd(stat + RF_S_FAULT, 1ull);
    c[t] = hit ? v : 0.0;
  }
  const uint32_t n_hit = __popcll(__ballot(hit));
  if ((threadIdx.x & 63u) == 0 && n_hit) atomicAdd(stat + RF_S_MATCHED, (unsigned long long)n_hit);
}

// RF_CHUNK consecutive vectors of P doubles starting at src come into sh; lanes p < P add them to run in vector order.
// n_vec <= RF_CHUNK.  The workgroup is one wave.
__device__ __forceinline__ void rf_fold_staged(const double *sh, uint32_t n_vec, uint32_t P, uint32_t lane, double &run) {
  if (lane < P) {
    if (n_vec == RF_CHUNK) {
#pragma unroll 16
      for (uint32_t k = 0; k < RF_CHUNK; ++k) run = run + sh[k * P + lane];
    } else {
      for (uint32_t k = 0; k < n_vec; ++k) run = run + sh[k * P + lane];
    }
  }
}

// grid = blocks of GRIM_REFRESH_BLOCK positions, 64 threads; dynamic LDS: RF_CHUNK * P doubles
__global__ __launch_bounds__(64) void rf_blocksum_kernel(const double *c, uint32_t F, uint32_t P, double *bsum) {
  extern __shared__ double rf_sh[];
  const uint32_t b = blockIdx.x, lane = threadIdx.x;
  const uint32_t lo = b * GRIM_REFRESH_BLOCK;
  if (lo >= F) return;
  const uint32_t hi = F - lo < GRIM_REFRESH_BLOCK ? F : lo + GRIM_REFRESH_BLOCK;  // read once: every loop below runs to it
  double run = 0.0;
  for (uint32_t i0 = lo; i0 < hi; i0 += RF_CHUNK) {  // the same trip count on every lane
    const uint32_t n_vec = hi - i0 < RF_CHUNK ? hi - i0 : RF_CHUNK;
    const uint32_t words = n_vec * P;
    const double *src = c + (uint64_t)i0 * P;
    for (uint32_t w = lane; w < words; w += 64u) rf_sh[w] = src[w];
    __syncthreads();
    rf_fold_staged(rf_sh, n_vec, P, lane, run);
    __syncthreads();
  }
  if (lane < P) bsum[(uint64_t)b * P + lane] = run;
}

// one wave: T_p over the block sums in order
__global__ __launch_bounds__(64) void rf_total_kernel(const double *bsum, uint32_t n_blocks, uint32_t P, double *total) {
  const uint32_t lane = threadIdx.x;
  if (lane >= P) return;
  double run = 0.0;
  for (uint32_t b = 0; b < n_blocks; ++b) run = run + bsum[(uint64_t)b * P + lane];
  total[lane] = run;
}

// a double that is >= +0.0 or NaN as an integer that orders like it (NaN above everything)
__device__ __forceinline__ unsigned long long rf_abs_bits(double x) { return (unsigned long long)__double_as_longlong(x) & ~GRIM_VALID; }

// one lane per full node
__global__ __launch_bounds__(256) void rf_divide_kernel(const uint32_t *full, uint32_t F, uint32_t V, uint32_t P, const double *c,
                                                        const double *total, const double *old_freq, double *shadow,
                                                        unsigned long long *stat) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  unsigned long long dmax = 0;
  uint32_t zero = 0;
  if (i < F) {
    const uint32_t node = full[i];
    if (node < V) {
      zero = 1;
      for (uint32_t p = 0; p < P; ++p) {
        const double nv = c[(uint64_t)i * P + p] / total[p];
        const double d = nv - old_freq[(uint64_t)node * P + p];
        const unsigned long long bits = rf_abs_bits(d);
        if (bits > dmax) dmax = bits;
        if (nv != 0.0) zero = 0;
        shadow[(uint64_t)node * P + p] = nv;
      }
    }
  }
  // the statistics: one atomic per wave
  for (uint32_t off = 32u; off; off >>= 1) {
    const unsigned long long o = __shfl_xor(dmax, off);
    if (o > dmax) dmax = o;
  }
  const uint32_t n_zero = __popcll(__ballot(zero));
  if ((threadIdx.x & 63u) == 0) {
    if (dmax) atomicMax(stat + RF_S_DELTA, dmax);
    if (n_zero) atomicAdd(stat + RF_S_ZERO_FULL, (unsigned long long)n_zero);
  }
}

// the row of partial node v: [lo, lo + n), cut to the array
__device__ __forceinline__ void rf_row(const uint32_t *a_start, uint32_t v, uint32_t V, uint32_t n_a_nbr, uint32_t &lo, uint32_t &n) {
  lo = a_start[v];
  uint32_t hi = v + 1u < V ? a_start[v + 1u] : n_a_nbr;
  if (hi > n_a_nbr) hi = n_a_nbr;
  n = hi > lo ? hi - lo : 0u;
}

// list[k]: a partial node whose row has at most RF_SHORT_MAX entries; one lane per (k, p)
__global__ __launch_bounds__(256) void rf_short_kernel(const uint32_t *list, uint32_t n_list, uint32_t V, uint32_t P, const uint32_t *a_start,
                                                       const uint32_t *a_nbr, uint32_t n_a_nbr, double *shadow, unsigned long long *stat) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= (uint64_t)n_list * P) return;
  const uint32_t k = (uint32_t)(t / P), p = (uint32_t)(t - (uint64_t)k * P);
  const uint32_t v = list[k];
  if (v >= V) {
    atomicAdd(stat + RF_S_FAULT, 1ull);
    return;
  }
  uint32_t lo, n;  // read once: the loop below runs to n
  rf_row(a_start, v, V, n_a_nbr, lo, n);
  if (n > RF_SHORT_MAX) {
    atomicAdd(stat + RF_S_FAULT, 1ull);
    return;
  }
  double run = 0.0;
  bool bad = false;
  for (uint32_t e = 0; e < n; ++e) {
    const uint32_t r = a_nbr[lo + e];
    if (r < V)
      run = run + shadow[(uint64_t)r * P + p];
    else
      bad = true;
  }
  if (bad)
    atomicAdd(stat + RF_S_FAULT, 1ull);
  else
    shadow[(uint64_t)v * P + p] = run;
}

// list[blockIdx.x]: a partial node with a longer row; 64 threads; dynamic LDS: RF_CHUNK * P doubles, then RF_CHUNK node ids
__global__ __launch_bounds__(64) void rf_long_kernel(const uint32_t *list, uint32_t n_list, uint32_t V, uint32_t P, const uint32_t *a_start,
                                                     const uint32_t *a_nbr, uint32_t n_a_nbr, double *shadow, unsigned long long *stat) {
  extern __shared__ double rf_sh[];
  uint32_t *ids = (uint32_t *)(rf_sh + RF_CHUNK * P);
  const uint32_t lane = threadIdx.x;
  if (blockIdx.x >= n_list) return;
  const uint32_t v = list[blockIdx.x];
  if (v >= V) {
    if (lane == 0) atomicAdd(stat + RF_S_FAULT, 1ull);
    return;
  }
  uint32_t lo, n;  // read once: every loop below runs to n
  rf_row(a_start, v, V, n_a_nbr, lo, n);
  double run = 0.0;
  uint32_t bad = 0;
  for (uint32_t e0 = 0; e0 < n; e0 += RF_CHUNK) {  // the same trip count on every lane
    const uint32_t n_vec = n - e0 < RF_CHUNK ? n - e0 : RF_CHUNK;
    uint32_t r = GRIM_NONE;
    if (lane < n_vec) r = a_nbr[lo + e0 + lane];
    if (lane < n_vec && r >= V) {
      bad = 1;
      r = GRIM_NONE;
    }
    ids[lane] = r;
    __syncthreads();
    const uint32_t words = n_vec * P;
    for (uint32_t w = lane; w < words; w += 64u) {
      const uint32_t k = w / P, p = w - k * P;
      const uint32_t rk = ids[k];
      rf_sh[w] = rk != GRIM_NONE ? shadow[(uint64_t)rk * P + p] : 0.0;
    }
    __syncthreads();
    rf_fold_staged(rf_sh, n_vec, P, lane, run);
    __syncthreads();
  }
  const bool any_bad = __ballot(bad) != 0ull;
  if (any_bad) {
    if (lane == 0) atomicAdd(stat + RF_S_FAULT, 1ull);
    return;
  }
  if (lane < P) shadow[(uint64_t)v * P + lane] = run;
}

// one lane per full node: f0 of the fht entry of its key, when the exact-name index maps the key to this node
__global__ __launch_bounds__(256) void rf_fht_kernel(const uint32_t *full, uint32_t F, uint32_t V, uint32_t P, const uint64_t *node_key,
                                                     const HtEnt *ht, uint32_t ht_mask, FullEnt *fht, uint32_t fht_mask, const double *freq) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= F) return;
  const uint32_t node = full[i];
  if (node >= V) return;
  const uint64_t key = node_key[node];
  uint32_t h = (uint32_t)mix64(key) & ht_mask;
  bool mine = false;
  for (uint32_t turn = 0; turn <= ht_mask; ++turn) {
    const HtEnt e = ht[h];
    if (e.key == 0) break;
    if (e.key == key) {
      mine = e.val == node;
      break;
    }
    h = (h + 1u) & ht_mask;
  }
  if (!mine) return;
  uint32_t s = fht_hash(key) & fht_mask;
  for (uint32_t turn = 0; turn <= fht_mask; ++turn) {
    const uint64_t k = fht[s].key;
    if (k == 0) return;
    if (k == key) {
      fht[s].f0 = freq[(uint64_t)node * P];
      return;
    }
    s = (s + 1u) & fht_mask;
  }
}
