// grim_match.h -- match probabilities between imputed subjects on a subset of the loci, computed on the device (gfx950,
// wave64) from the genotype rows finished batches hold in HBM, with a mismatch direction and, when graded, per-locus
// probabilities of exactly 0, 1 and 2 mismatches (include/grim_hip.h, grim_match_*).
//
// Contract.  Input: a set K of locus slots (keep_mask, not empty), the dictionary sizes n_alleles[GRIM_MAXL], a direction DIR,
// whether the records are GRADED, and two sides, patients and donors, each a set of grim_subject_result records plus grim_row
// records.  Of a subject only its GRIM_T_UMUG rows k = 0..n-1 in rank order are used, row k = (a_k, b_k, p_k).
//   Per subject (both sides), flags:
//     MT_F_VALID      status GRIM_ST_OK, n >= 1, row_off / n_rows inside the rows given (mg_skipped), and
//                     total = ((p_0 + p_1) + p_2) + ... (fp64, left to right) finite and > 0
//     MT_F_PRIVATE    some row holds, in a slot of K, a field f > n_alleles[s]: an allele id private to the subject (grim_em.h,
//                     the spill rule); its id means nothing outside that subject
//     MT_F_UNDEFINED  some row has a slot (any slot, as in mg_reduce_kernel) typed on one haplotype and 0 on the other
//     PRIVATE and UNDEFINED are looked for in every subject whose rows can be read (status, count and offsets as for VALID),
//     whatever its total.  Weights w_k = p_k / total.  Bit GRIM_KEY_GRAPH_ORDER and every field outside K are dropped.
//   Per row pair, patient row i = (a, b), donor row j = (c, d); for every slot s in K, with x1 = field_s(a), x2 = field_s(b),
//     y1 = field_s(c), y2 = field_s(d):
//       eq(x, y) = x == y and x != 0        (an untyped field equals nothing, not even another untyped field)
//       mm_s, the per-slot function, by DIR:
//         GRIM_MATCH_DIR_EITHER (0)  2 - max(eq(x1,y1) + eq(x2,y2), eq(x1,y2) + eq(x2,y1))                    (mt_mm)
//         GRIM_MATCH_DIR_GVH    (1)  !(eq(x1,y1) || eq(x1,y2)) + !(eq(x2,y1) || eq(x2,y2))                    (mt_lacking)
//                                    the patient's alleles the donor lacks: both copies are counted, an untyped field is
//                                    always lacking
//         GRIM_MATCH_DIR_HVG    (2)  the same with the roles of x and y exchanged: the donor's alleles the patient lacks
//         either == max(gvh, hvg) for all fields, 0 included.
//       M(i,j)   = sum over s in K of mm_s, in 0..2|K|
//   Per (patient, donor) pair one record of mm[2*GRIM_MAXL+1] and PER bins per locus slot:
//       ungraded  PER = 1, G = {0}        grim_match_rec { double mm[11]; double locus[GRIM_MAXL]; }, 16 doubles, 128 bytes
//       graded    PER = 3, G = {0, 1, 2}  grim_match_grade_rec { double mm[11]; double grade[GRIM_MAXL][3]; }, 26 doubles, 208 bytes
//   The order of every sum is part of the contract (w = the patient's weights, v = the donor's):
//       H[0..2|K|] = 0.0 ; L[s][g] = 0.0
//       for j = 0..n_d-1:                      donor rows, rank order
//           ph[*] = 0.0 ; pl[*][*] = 0.0
//           for i = 0..n_p-1:                  patient rows, rank order
//               t = w_i * v_j                  one multiply, no fma
//               ph[M(i,j)] = ph[M(i,j)] + t
//               for s in K: for g in G: if mm_s == g: pl[s][g] = pl[s][g] + t
//           H[m] = H[m] + ph[m] for every m ; L[s][g] = L[s][g] + pl[s][g] for every s in K, g in G
//       mm[m] = H[m] (0.0 for m > 2|K|) ; locus[s] = L[s][0], or grade[s][g] = L[s][g], for s in K, 0.0 elsewhere
//     The inner sum belongs to one donor row, so a lane owns it; the outer fold is sequential over the donor rows: equal inputs
//     give equal bits whatever the launch shape.  No partial is ever -0.0 (every sum starts from +0.0), so adding a 0.0 changes
//     no bit and "add t to bin M" may be written "add (M == m ? t : 0.0) to every bin m", and likewise (mm_s == g ? t : 0.0).
//     So the graded mm[] has the bits of the ungraded mm[] of the same direction, and grade[s][0] those of its locus[s].
//   A pair is computed iff both subjects are VALID and neither is PRIVATE; otherwise its record is all zero bytes.
//   Results are patient-major: out[p * n_donors + d].
//
// Deliberately plain: no floating-point atomics, no inline assembly, integer atomics only for the statistics.
//   mg_count_kernel (grim_marginal.h) + em_scan_kernel (grim_em.h)   rows per subject -> region starts of a side
//   mt_prepare_kernel   one wave per subject: the total (every lane the same serial sum), then lanes stride over the rows and
//                       write a & keep, b & keep, w_k into the side's packed arrays at region start + k; one lane writes the
//                       flags.  A subject whose rows do not lie inside the rows given is flagged 0 and never read.
//   mt_pair_kernel<DIR, GRADED>
//                       one 64-thread workgroup per (donor, patient) pair.  Donor rows go MT_CHUNK at a time: lane l owns donor
//                       row chunk * 64 + l and walks all patient rows in order (patient rows come from global memory: every
//                       donor of the launch reads them, they sit in L2), holding ph[11] and pg[5][PER] in registers (no indexed
//                       access); the lanes put their REC = 16 or 26 partials into LDS, a tile of 64 x (REC + 1) doubles (an
//                       odd row length: the rows start on different banks), and lanes 0..REC-1 fold one bin each over the
//                       chunk's rows in increasing j into a running register.  LDS use does not depend on the row counts.
#pragma once
#include "grim_marginal.h"

#define MT_F_VALID 1u      // = GRIM_MATCH_VALID
#define MT_F_PRIVATE 2u    // = GRIM_MATCH_PRIVATE
#define MT_F_UNDEFINED 4u  // = GRIM_MATCH_UNDEFINED
#define MT_DIR_EITHER 0    // = GRIM_MATCH_DIR_EITHER
#define MT_DIR_GVH 1       // = GRIM_MATCH_DIR_GVH
#define MT_DIR_HVG 2       // = GRIM_MATCH_DIR_HVG
#define MT_CHUNK 64u
#define MT_BINS (2 * GRIM_MAXL + 1)
#define MT_GRADES 3
#define MT_REC (MT_BINS + GRIM_MAXL)                    // doubles of a grim_match_rec
#define MT_GRADE_REC (MT_BINS + GRIM_MAXL * MT_GRADES)  // doubles of a grim_match_grade_rec
// per-call counters (device, u64), sliced like the marginal reducer's: MT_S_SLICES copies of MT_S_COUNT words, one cache line
// each, taken by subject or pair number (a run of 64 patients against 100 000 donors adds from 6.4 million workgroups); the
// host adds the slices up
#define MT_S_SLICES 256u
enum { MT_S_P_VALID = 0, MT_S_D_VALID = 1, MT_S_P_PRIVATE = 2, MT_S_D_PRIVATE = 3, MT_S_UNDEFINED = 4, MT_S_PAIRS = 5, MT_S_ROW_PAIRS = 6, MT_S_COUNT = 8 };

struct MtSide {  // a side's subjects as the pair kernel reads them
  const uint32_t *first;  // [n + 1] region starts (first[n] = rows of the side)
  const uint64_t *a, *b;  // [rows] keys masked to K
  const double *w;        // [rows] weights
  const uint8_t *flags;   // [n]
};

// one wave per subject, four to a workgroup.  side: 0 = patients, 1 = donors (which statistics the subject adds to);
// cap = rows the packed arrays hold: a region that does not lie inside them is not touched and its subject not valid.
__global__ __launch_bounds__(256) void mt_prepare_kernel(const grim_subject_result *res, const grim_row *rows, uint32_t n_subj,
                                                         uint32_t rows_used, const uint32_t *first, uint32_t cap, uint32_t keep_mask,
                                                         EmLimits L, uint32_t side, uint64_t *oa, uint64_t *ob, double *ow,
                                                         uint8_t *oflags, unsigned long long *stat) {
  const uint32_t s = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (s >= n_subj) return;
  const grim_subject_result r = res[s];
  const uint32_t f = first[s];
  uint32_t n = first[s + 1] - f;  // the row count, read once: every loop below runs to it
  if (mg_skipped(r, rows_used) || n != r.n_rows[GRIM_T_UMUG] || f > cap || n > cap - f) n = 0;
  if (n == 0) {
    if (lane == 0) oflags[s] = 0;
    return;
  }
  uint64_t keep = 0;  // the key fields of K
  for (uint32_t q = 0; q < GRIM_MAXL; ++q)
    if ((keep_mask >> q) & 1u) keep |= 0xFFFull << (GRIM_ABITS * q);
  const grim_row *R = rows + r.row_off[GRIM_T_UMUG];
  double total = R[0].prob;  // every lane: the same sequential sum
  for (uint32_t k = 1; k < n; ++k) total = total + R[k].prob;
  const bool valid = total > 0.0 && total <= 1.7976931348623157e308;  // finite and > 0 (false for a NaN)
  uint32_t priv = 0, undefined = 0;
  for (uint32_t k = lane; k < n; k += 64u) {
    const grim_row row = R[k];
    for (uint32_t q = 0; q < GRIM_MAXL; ++q) {
      const uint32_t fa = (uint32_t)(row.a >> (GRIM_ABITS * q)) & 0xFFFu, fb = (uint32_t)(row.b >> (GRIM_ABITS * q)) & 0xFFFu;
      undefined |= (fa == 0) != (fb == 0);
      if ((keep_mask >> q) & 1u) priv |= (fa > L.n_alleles[q]) | (fb > L.n_alleles[q]);
    }
    oa[f + k] = row.a & keep;  // k < n <= cap - f: inside the side's arrays
    ob[f + k] = row.b & keep;
    ow[f + k] = valid ? row.prob / total : 0.0;
  }
  const bool any_priv = __ballot(priv) != 0ull, any_undef = __ballot(undefined) != 0ull;
  if (lane == 0) {
    oflags[s] = (uint8_t)((valid ? MT_F_VALID : 0u) | (any_priv ? MT_F_PRIVATE : 0u) | (any_undef ? MT_F_UNDEFINED : 0u));
    stat += (s % MT_S_SLICES) * MT_S_COUNT;
    if (valid) atomicAdd(stat + MT_S_P_VALID + side, 1ull);
    if (any_priv) atomicAdd(stat + MT_S_P_PRIVATE + side, 1ull);
    if (any_undef) atomicAdd(stat + MT_S_UNDEFINED, 1ull);
  }
}

// mismatches of one locus slot in either direction: the 12-bit fields x1, x2 (patient) against y1, y2 (donor)
__device__ __forceinline__ uint32_t mt_mm(uint32_t x1, uint32_t x2, uint32_t y1, uint32_t y2) {
  const uint32_t straight = (uint32_t)(x1 == y1 && x1 != 0u) + (uint32_t)(x2 == y2 && x2 != 0u);
  const uint32_t crossed = (uint32_t)(x1 == y2 && x1 != 0u) + (uint32_t)(x2 == y1 && x2 != 0u);
  return 2u - (straight > crossed ? straight : crossed);
}

// alleles of (x1, x2) that (y1, y2) lacks
__device__ __forceinline__ uint32_t mt_lacking(uint32_t x1, uint32_t x2, uint32_t y1, uint32_t y2) {
  const bool has1 = (x1 == y1 || x1 == y2) && x1 != 0u, has2 = (x2 == y1 || x2 == y2) && x2 != 0u;
  return (uint32_t)!has1 + (uint32_t)!has2;
}

template <int DIR>
__device__ __forceinline__ uint32_t mt_mm_dir(uint32_t x1, uint32_t x2, uint32_t y1, uint32_t y2) {
  if (DIR == MT_DIR_GVH) return mt_lacking(x1, x2, y1, y2);
  if (DIR == MT_DIR_HVG) return mt_lacking(y1, y2, x1, x2);
  return mt_mm(x1, x2, y1, y2);
}

// grid (n_donors, patients of this launch); p0 = the first patient of the launch.  out (records of REC doubles) is cleared
// before the launch: a pair that is not computed writes nothing.
template <int DIR, bool GRADED>
__global__ __launch_bounds__(64) void mt_pair_kernel(MtSide P, uint32_t n_p, uint32_t p0, MtSide D, uint32_t n_d, uint32_t keep_mask,
                                                     double *out, unsigned long long *stat) {
  constexpr uint32_t PER = GRADED ? MT_GRADES : 1u;  // bins of a locus slot
  constexpr uint32_t REC = MT_BINS + GRIM_MAXL * PER;
  __shared__ double sh[MT_CHUNK][REC + 1];  // [donor row of the chunk][bin]; 17 or 27 doubles a row: the rows on different banks
  const uint32_t d = blockIdx.x, p = p0 + blockIdx.y, lane = threadIdx.x;
  if (d >= n_d || p >= n_p) return;
  if ((P.flags[p] & (MT_F_VALID | MT_F_PRIVATE)) != MT_F_VALID || (D.flags[d] & (MT_F_VALID | MT_F_PRIVATE)) != MT_F_VALID) return;
  const uint32_t pf = P.first[p], np = P.first[p + 1] - pf;  // the row counts, read once: every loop below runs to them
  const uint32_t df = D.first[d], nd = D.first[d + 1] - df;
  const uint64_t *pa = P.a + pf, *pb = P.b + pf;
  const double *pw = P.w + pf;
  double run = 0.0;  // lanes 0..REC-1: bin `lane` of the record, folded over the donor rows so far
  for (uint32_t c0 = 0; c0 < nd; c0 += MT_CHUNK) {  // the same trip count on every lane
    const uint32_t j = c0 + lane;
    double ph[MT_BINS], pg[GRIM_MAXL][PER];
#pragma unroll
    for (uint32_t m = 0; m < MT_BINS; ++m) ph[m] = 0.0;
#pragma unroll
    for (uint32_t q = 0; q < GRIM_MAXL; ++q)
#pragma unroll
      for (uint32_t g = 0; g < PER; ++g) pg[q][g] = 0.0;
    if (j < nd) {
      const uint64_t c = D.a[df + j], e = D.b[df + j];
      const double v = D.w[df + j];
      for (uint32_t i = 0; i < np; ++i) {
        const uint64_t a = pa[i], b = pb[i];
        const double t = pw[i] * v;
        uint32_t M = 0;
#pragma unroll
        for (uint32_t q = 0; q < GRIM_MAXL; ++q) {
          if (!((keep_mask >> q) & 1u)) continue;
          const uint32_t mm = mt_mm_dir<DIR>((uint32_t)(a >> (GRIM_ABITS * q)) & 0xFFFu, (uint32_t)(b >> (GRIM_ABITS * q)) & 0xFFFu,
                                             (uint32_t)(c >> (GRIM_ABITS * q)) & 0xFFFu, (uint32_t)(e >> (GRIM_ABITS * q)) & 0xFFFu);
          M += mm;
#pragma unroll
          for (uint32_t g = 0; g < PER; ++g) pg[q][g] = pg[q][g] + (mm == g ? t : 0.0);
        }
#pragma unroll
        for (uint32_t m = 0; m < MT_BINS; ++m) ph[m] = ph[m] + (M == m ? t : 0.0);  // registers, no indexed access
      }
    }
#pragma unroll
    for (uint32_t m = 0; m < MT_BINS; ++m) sh[lane][m] = ph[m];
#pragma unroll
    for (uint32_t q = 0; q < GRIM_MAXL; ++q)
#pragma unroll
      for (uint32_t g = 0; g < PER; ++g) sh[lane][MT_BINS + q * PER + g] = pg[q][g];
    __threadfence_block();
    __syncthreads();
    if (lane < REC) {
      const uint32_t in_chunk = nd - c0 < MT_CHUNK ? nd - c0 : MT_CHUNK;
      for (uint32_t k = 0; k < in_chunk; ++k) run = run + sh[k][lane];  // increasing j
    }
    __syncthreads();
  }
  const uint64_t at = ((uint64_t)p * n_d + d) * REC;
  if (lane < REC) out[at + lane] = run;
  if (lane == 0) {
    stat += ((d + p) % MT_S_SLICES) * MT_S_COUNT;
    atomicAdd(stat + MT_S_PAIRS, 1ull);
    atomicAdd(stat + MT_S_ROW_PAIRS, (unsigned long long)np * nd);
  }
}
