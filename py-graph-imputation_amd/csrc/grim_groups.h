// grim_groups.h -- allele groups: the genotype rows of a finished batch mapped to a chosen resolution (first field, two
// fields, P or G groups, any table) in front of the consumers' kernels, which stay as they are (gfx950, wave64;
// include/grim_hip.h, grim_groups_*).
//
// Contract.  A group map gives for every locus slot s a table T_s[0 .. n_alleles[s]] of uint16_t and a count n_groups[s]:
// T_s[0] == 0, 1 <= T_s[f] <= n_groups[s] for 1 <= f <= n_alleles[s], every group id used (checked on the host before any
// upload).  A row (a, b, prob, popa, popb) maps to (map(a), map(b), prob, popa, popb); the 12-bit field f of slot s becomes
//     0                                  if f == 0                      (untyped stays untyped)
//     T_s[f]                             if 1 <= f <= n_alleles[s]
//     n_groups[s] + (f - n_alleles[s])   if f > n_alleles[s]             (private to the subject: stays private, keeps its index)
// which is <= f <= 4095, so a field never overflows.  Key bits at GRIM_KEY_GRAPH_ORDER and above are copied.  No
// floating-point operation takes place: prob is moved as bits.
//
//   gp_map_kernel    row-wise, knows nothing of subjects: rows[0 .. rows_used) into a second buffer.  256 threads, a grid-stride
//                    loop, a row per thread as two 16-byte loads and two 16-byte stores (a wave moves 2 KB contiguous each
//                    way).  STAGED (the default, by measurement): the tables (at most 5 x 4096 x 2 B = 40 KB; only the
//                    entries there are get copied) go into LDS in every workgroup first; otherwise they are read where
//                    they lie.
//   gp_flag_kernel   the launch shape of mt_prepare_kernel, one wave per subject, four to a workgroup: flags[i] =
//                    GP_F_PRIVATE when the subject is readable (mg_skipped) and some UMUG row holds, in a slot of `mask`
//                    (kept and not an identity slot), a field above n_alleles; a skipped subject gets 0 and its rows are
//                    never read.
#pragma once
#include "grim_match.h"

#define GP_THREADS 256u
#define GP_MAX_BLOCKS 256u  // one workgroup a CU; more rows than 65 536 take further passes of the grid-stride loop
#define GP_MAX_ENTRIES (GRIM_MAXL * 4096u)
#define GP_F_PRIVATE 1u  // = GRIM_GROUPS_PRIVATE
#define GP_FIELDS ((1ull << (GRIM_ABITS * GRIM_MAXL)) - 1ull)

struct GpMap {
  const uint16_t *tab;            // the slots' tables back to back
  uint32_t off[GRIM_MAXL];        // where slot s begins in tab; off[s] + n_alleles[s] < total
  uint32_t n_alleles[GRIM_MAXL];  // the last index of a slot's table
  uint32_t n_groups[GRIM_MAXL];
  uint32_t total;                 // entries of tab, <= GP_MAX_ENTRIES
};

__device__ __forceinline__ uint64_t gp_map_key(uint64_t key, const uint16_t *tab, const GpMap &M) {
  uint64_t out = key & ~GP_FIELDS;
#pragma unroll
  for (uint32_t q = 0; q < GRIM_MAXL; ++q) {
    const uint32_t f = (uint32_t)(key >> (GRIM_ABITS * q)) & 0xFFFu, n = M.n_alleles[q];
    uint32_t g = 0;
    if (f > n)
      g = M.n_groups[q] + (f - n);  // n_groups <= n_alleles: at most f
    else if (f != 0u)
      g = tab[M.off[q] + f];  // f <= n_alleles[q]: inside the slot's table
    out |= (uint64_t)(g & 0xFFFu) << (GRIM_ABITS * q);
  }
  return out;
}

template <bool STAGED>
__global__ __launch_bounds__(GP_THREADS) void gp_map_kernel(const grim_row *__restrict__ rows, uint32_t rows_used, GpMap M,
                                                            grim_row *__restrict__ out) {
  __shared__ uint16_t sh_tab[STAGED ? GP_MAX_ENTRIES : 1u];
  const uint16_t *tab = M.tab;
  if (STAGED) {
    const uint32_t total = M.total < GP_MAX_ENTRIES ? M.total : GP_MAX_ENTRIES;  // read once; never past the LDS array
    for (uint32_t i = threadIdx.x; i < total; i += GP_THREADS) sh_tab[i] = M.tab[i];
    __syncthreads();
    tab = sh_tab;
  }
  const uint4 *in4 = reinterpret_cast<const uint4 *>(rows);
  uint4 *out4 = reinterpret_cast<uint4 *>(out);
  const uint32_t stride = gridDim.x * GP_THREADS;
  for (uint64_t k = (uint64_t)blockIdx.x * GP_THREADS + threadIdx.x; k < rows_used; k += stride) {
    const uint4 keys = in4[2 * k], rest = in4[2 * k + 1];  // (a, b) and (prob, popa, popb)
    const uint64_t a = gp_map_key(((uint64_t)keys.y << 32) | keys.x, tab, M), b = gp_map_key(((uint64_t)keys.w << 32) | keys.z, tab, M);
    out4[2 * k] = make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
    out4[2 * k + 1] = rest;
  }
}

// L: the dictionary sizes (a field above them is private); mask: the kept slots that are not identity slots
__global__ __launch_bounds__(256) void gp_flag_kernel(const grim_subject_result *res, const grim_row *rows, uint32_t n_subj,
                                                      uint32_t rows_used, EmLimits L, uint32_t mask, uint8_t *flags) {
  const uint32_t s = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (s >= n_subj) return;
  const grim_subject_result r = res[s];
  if (mg_skipped(r, rows_used)) {
    if (lane == 0) flags[s] = 0;
    return;
  }
  const uint32_t n = r.n_rows[GRIM_T_UMUG];  // the row count, read once; mg_skipped: off + n <= rows_used
  const grim_row *R = rows + r.row_off[GRIM_T_UMUG];
  uint32_t priv = 0;
  for (uint32_t k = lane; k < n; k += 64u) {
    const uint64_t a = R[k].a, b = R[k].b;
    for (uint32_t q = 0; q < GRIM_MAXL; ++q) {
      const uint32_t fa = (uint32_t)(a >> (GRIM_ABITS * q)) & 0xFFFu, fb = (uint32_t)(b >> (GRIM_ABITS * q)) & 0xFFFu;
      if ((mask >> q) & 1u) priv |= (fa > L.n_alleles[q]) | (fb > L.n_alleles[q]);
    }
  }
  const bool any_priv = __ballot(priv) != 0ull;
  if (lane == 0) flags[s] = any_priv ? (uint8_t)GP_F_PRIVATE : (uint8_t)0;
}
