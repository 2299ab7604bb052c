// grim_match_grade.h -- the match probabilities of grim_match.h with a mismatch direction and, when graded, per-locus
// probabilities of exactly 0, 1 and 2 mismatches (include/grim_hip.h, grim_match_create_ex).
//
// Contract.  Everything of grim_match.h holds -- the flags, the weights, patient-major results, the donor-row outer fold, the
// patient-row inner fold, +0.0 starts, no fma, the statistics -- except the per-slot mismatch function and, when graded, the
// record.  With x1, x2 the patient's fields of a slot, y1, y2 the donor's and eq(x, y) = x == y and x != 0:
//   GRIM_MATCH_DIR_EITHER (0)  mm_s = 2 - max(eq(x1,y1) + eq(x2,y2), eq(x1,y2) + eq(x2,y1))                    (mt_mm)
//   GRIM_MATCH_DIR_GVH    (1)  mm_s = !(eq(x1,y1) || eq(x1,y2)) + !(eq(x2,y1) || eq(x2,y2))
//                              the patient's alleles the donor lacks: both copies are counted, an untyped field is always lacking
//   GRIM_MATCH_DIR_HVG    (2)  the same with the roles of x and y exchanged: the donor's alleles the patient lacks
//   either == max(gvh, hvg) for all fields, 0 included.
// Graded record: grim_match_grade_rec { double mm[2*GRIM_MAXL+1]; double grade[GRIM_MAXL][3]; }, 26 doubles.  grade[s][g] is
// the two-level fold of locus[s] with the condition mm_s == g in the place of mm_s == 0 (0.0 for s outside K): mm[] has the
// bits of the ungraded record of the same direction and grade[s][0] those of its locus[s].
//
// mt_pair_dir_kernel<DIR, GRADED> keeps the launch shape of mt_pair_kernel: one 64-thread workgroup per (donor, patient), donor
// rows MT_CHUNK at a time, lane l owns a donor row and walks the patient rows in order, the partials go to LDS and lanes
// 0..REC-1 fold one bin each over the chunk's rows in increasing j.  Graded, a lane holds ph[11] and pg[5][3] in registers
// (every update is `mm == g ? t : 0.0`, no indexed access) and the LDS tile is 64 x 27 doubles (an odd row length: the rows
// start on different banks).  mt_pair_kernel itself is not touched: (either, ungraded) launches it as before.
// Plain C++: no floating-point atomics, no inline assembly, integer atomics only for the statistics.
#pragma once
#include "grim_match.h"

#define MT_DIR_EITHER 0  // = GRIM_MATCH_DIR_EITHER
#define MT_DIR_GVH 1     // = GRIM_MATCH_DIR_GVH
#define MT_DIR_HVG 2     // = GRIM_MATCH_DIR_HVG
#define MT_GRADES 3
#define MT_GRADE_REC (MT_BINS + GRIM_MAXL * MT_GRADES)  // doubles of a grim_match_grade_rec

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
__global__ __launch_bounds__(64) void mt_pair_dir_kernel(MtSide P, uint32_t n_p, uint32_t p0, MtSide D, uint32_t n_d, uint32_t keep_mask,
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
