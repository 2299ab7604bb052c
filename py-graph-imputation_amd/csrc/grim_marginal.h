// grim_marginal.h -- marginal genotype tables on a subset of the loci, reduced on the device (gfx950, wave64) from the
// genotype rows a finished batch holds in HBM (include/grim_hip.h, grim_marginal_*).
//
// Contract.  Input: a set K of locus slots to keep (not empty) and, for every subject with status GRIM_ST_OK, its
// GRIM_T_UMUG rows k = 0..n-1 in rank order, row k = (a_k, b_k, p_k).
//   Reduced genotype of row k: for every slot s in K the UNORDERED pair {field_s(a_k), field_s(b_k)} of the slot's 12-bit key
//     fields.  Which haplotype of a row carries which allele is not canonical between rows (the formatter sorts each locus
//     pair when it prints), so rows are compared per slot on (min, max).  Bit GRIM_KEY_GRAPH_ORDER and every field outside
//     K are dropped; a field of 0 (locus not typed) is a value like any other; grouping never crosses subjects, so allele
//     ids private to a subject need no special case.
//   Group: the first row of a reduced genotype, in rank order, leads its group.  The group's sum is the left-to-right fp64
//     sum of the p_k of its rows in rank order, starting from the leader's own p: (p_i + p_j) + p_l ...  No floating-point
//     atomics, no tree sums.
//   Rank: groups by sum descending, ties in the leaders' order (a stable sort): rank of group g = the number of groups h
//     with sum_h > sum_g, or sum_h == sum_g and leader_h < leader_g.
//   Output per subject: the first min(groups, max_rows) groups in rank order as grim_row records (a = the leader's a masked
//     to K, b = the leader's b masked to K, prob = the sum, popa = popb = 0), and a grim_subject_result copy: status / plan /
//     reason copied, n_genotypes = groups, n_rows[GRIM_T_UMUG] = rows written, row_off[GRIM_T_UMUG] = the start of the
//     subject's region of the output rows, everything else 0.  A subject that is not GRIM_ST_OK, or has no UMUG rows,
//     produces no rows.
//   Not defined: a row whose a and b occupy different sets of slots (the formatter pairs the printed alleles by index: the
//     text would misalign).  Such subjects are counted (MG_S_UNDEFINED); the caller raises when the count is not 0.
//
// Deliberately plain: one wave per subject, quadratic grouping inside the subject, no hash table, no global sort.
//   mg_count_kernel    UMUG rows per subject (0 = skipped); em_scan_kernel (grim_em.h) turns them into region starts
//   mg_reduce_kernel   one 64-thread workgroup per subject; lanes stride over the rows:
//                      (a) canonical form and probability of every row into the staging area
//                      (b) leader[k] = the smallest j <= k with the same canonical form
//                      (c) every leader adds the p_j of its rows j = k+1.. in order
//                      (d) every leader counts the leaders that beat it and writes its row at region start + rank
//                      (e) one lane writes the result copy and the statistics
//                      The staging area is LDS when the subject has at most MG_LDS_ROWS rows and the subject's region of a
//                      global scratch otherwise: the same code, through pointers chosen once.
#pragma once
#include "grim_em.h"

#define MG_LDS_ROWS 256u
// per-call counters (device, u64)
// (every subject adds to them: MG_S_SLICES copies, one cache line each, taken by subject number, so that the adds of a big batch
// do not queue on one address; the host adds the slices up)
enum { MG_S_SUBJECTS = 0, MG_S_ROWS_IN = 1, MG_S_GROUPS = 2, MG_S_ROWS_OUT = 3, MG_S_UNDEFINED = 4, MG_S_COUNT = 8 };
#define MG_S_SLICES 64u

struct MgScratch {  // [rows of the batch]: a subject uses [region start, region start + its rows)
  uint64_t *lo, *hi;  // canonical form: per kept slot the smaller / the larger field
  double *prob, *sum;
  uint32_t *lead;
};

// never trust an offset: a subject whose rows do not lie inside the rows given is skipped, not read
__device__ __forceinline__ bool mg_skipped(const grim_subject_result &r, uint32_t rows_used) {
  if (r.status != GRIM_ST_OK) return true;
  const uint32_t n = r.n_rows[GRIM_T_UMUG], off = r.row_off[GRIM_T_UMUG];
  return n == 0 || off > rows_used || n > rows_used - off;
}

// rows per subject (0 = skipped) into cnt[0..n_subj)
__global__ __launch_bounds__(256) void mg_count_kernel(const grim_subject_result *res, uint32_t n_subj, uint32_t rows_used, uint32_t *cnt) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= n_subj) return;
  const grim_subject_result r = res[s];
  cnt[s] = mg_skipped(r, rows_used) ? 0u : r.n_rows[GRIM_T_UMUG];
}

// one workgroup of one wave per subject.  first[] = the scanned counts (first[n_subj] = their total); cap = rows the
// scratch and the output hold: a region that does not lie inside them is not touched.
__global__ __launch_bounds__(64) void mg_reduce_kernel(const grim_subject_result *res, const grim_row *rows, uint32_t n_subj,
                                                       uint32_t rows_used, const uint32_t *first, uint32_t cap, uint32_t keep_mask,
                                                       uint32_t max_rows, MgScratch G, grim_subject_result *ores, grim_row *orows,
                                                       unsigned long long *stat) {
  __shared__ uint64_t sh_lo[MG_LDS_ROWS], sh_hi[MG_LDS_ROWS];
  __shared__ double sh_prob[MG_LDS_ROWS], sh_sum[MG_LDS_ROWS];
  __shared__ uint32_t sh_lead[MG_LDS_ROWS];
  __shared__ uint32_t sh_cnt[3];  // groups, rows written, a row that is not defined
  const uint32_t s = blockIdx.x, lane = threadIdx.x;
  if (s >= n_subj) return;
  const grim_subject_result r = res[s];
  const uint32_t f = first[s];
  uint32_t n = first[s + 1] - f;  // the row count, read once: every loop below runs to it
  if (mg_skipped(r, rows_used) || n != r.n_rows[GRIM_T_UMUG] || f > cap || n > cap - f) n = 0;
  if (lane < 3u) sh_cnt[lane] = 0;
  uint64_t keep = 0;  // the key fields of K
  for (uint32_t q = 0; q < GRIM_MAXL; ++q)
    if ((keep_mask >> q) & 1u) keep |= 0xFFFull << (GRIM_ABITS * q);
  const bool in_lds = n <= MG_LDS_ROWS;
  uint64_t *lo = in_lds ? sh_lo : G.lo + f, *hi = in_lds ? sh_hi : G.hi + f;
  double *prob = in_lds ? sh_prob : G.prob + f, *sum = in_lds ? sh_sum : G.sum + f;
  uint32_t *lead = in_lds ? sh_lead : G.lead + f;
  const grim_row *R = rows + (n ? r.row_off[GRIM_T_UMUG] : 0u);
  __syncthreads();
  // (a) canonical form
  uint32_t undefined = 0;
  for (uint32_t k = lane; k < n; k += 64u) {
    const grim_row row = R[k];
    uint64_t l = 0, h = 0;
    for (uint32_t q = 0; q < GRIM_MAXL; ++q) {
      const uint64_t fa = (row.a >> (GRIM_ABITS * q)) & 0xFFFull, fb = (row.b >> (GRIM_ABITS * q)) & 0xFFFull;
      undefined |= (fa == 0) != (fb == 0);
      if ((keep_mask >> q) & 1u) {
        l |= (fa < fb ? fa : fb) << (GRIM_ABITS * q);
        h |= (fa < fb ? fb : fa) << (GRIM_ABITS * q);
      }
    }
    lo[k] = l;
    hi[k] = h;
    prob[k] = row.prob;
  }
  if (undefined) atomicOr(&sh_cnt[2], 1u);
  __threadfence_block();
  __syncthreads();
  // (b) leaders
  for (uint32_t k = lane; k < n; k += 64u) {
    const uint64_t l = lo[k], h = hi[k];
    uint32_t j = 0;
    while (j < k && (lo[j] != l || hi[j] != h)) ++j;
    lead[k] = j;
  }
  __threadfence_block();
  __syncthreads();
  // (c) sums, left to right
  uint32_t groups = 0;
  for (uint32_t k = lane; k < n; k += 64u) {
    if (lead[k] != k) continue;
    double acc = prob[k];
    for (uint32_t j = k + 1; j < n; ++j)
      if (lead[j] == k) acc = acc + prob[j];
    sum[k] = acc;
    ++groups;
  }
  if (groups) atomicAdd(&sh_cnt[0], groups);
  __threadfence_block();
  __syncthreads();
  // (d) ranks
  uint32_t written = 0;
  for (uint32_t k = lane; k < n; k += 64u) {
    if (lead[k] != k) continue;
    const double mine = sum[k];
    uint32_t rank = 0;
    for (uint32_t j = 0; j < n; ++j) {
      if (lead[j] != j) continue;
      const double other = sum[j];
      rank += (other > mine || (other == mine && j < k)) ? 1u : 0u;
    }
    if (rank < max_rows) {
      grim_row out;
      out.a = R[k].a & keep;
      out.b = R[k].b & keep;
      out.prob = mine;
      out.popa = out.popb = 0;
      orows[f + rank] = out;  // rank < groups <= n: inside the subject's region
      ++written;
    }
  }
  if (written) atomicAdd(&sh_cnt[1], written);
  __syncthreads();
  // (e) the result copy
  if (lane == 0) {
    const uint32_t n_groups = sh_cnt[0], n_out = sh_cnt[1];
    grim_subject_result o;
    memset(&o, 0, sizeof(o));  // the padding too: the copy is the same bytes every time
    o.status = r.status;
    o.plan = r.plan;
    o.reason = r.reason;
    o.n_genotypes = n_groups;
    o.row_off[GRIM_T_UMUG] = n_out ? f : 0u;
    o.n_rows[GRIM_T_UMUG] = n_out;
    ores[s] = o;
    if (n) {
      stat += (s % MG_S_SLICES) * MG_S_COUNT;
      atomicAdd(stat + MG_S_SUBJECTS, 1ull);
      atomicAdd(stat + MG_S_ROWS_IN, (unsigned long long)n);
      atomicAdd(stat + MG_S_GROUPS, (unsigned long long)n_groups);
      atomicAdd(stat + MG_S_ROWS_OUT, (unsigned long long)n_out);
      if (sh_cnt[2]) atomicAdd(stat + MG_S_UNDEFINED, 1ull);
    }
  }
}
