// grim_em.h -- the M-step of an EM iteration on the device (gfx950, wave64): per-population haplotype counts from the
// phased hap;pop rows a finished batch holds in HBM (include/grim_hip.h, grim_em_*).
//
// Contract.  A subject takes part when its status is GRIM_ST_OK, it has phased rows and they did not come from Plan C.
// With p_k the probability of its k-th phased row (rank order), total = ((p_0 + p_1) + p_2) + ..., w_k = p_k / total, the
// subject adds w_k to (haplotype a_k, population popa_k) and then to (b_k, popb_k).  Every (haplotype, population) counter
// is the left-to-right fp64 sum of its contributions in (subject, rank, side) order over the whole input, whatever the
// batch cuts: a batch's sums START from the counter the batches before it left.
//
// So no floating-point atomics.  Per batch:
//   em_count_kernel    rows each subject contributes (0 = skipped); em_scan_kernel turns them into positions
//   em_weight_kernel   one wave per subject: the total (sequential), then per row and side a contribution record at
//                      position 2 * (first row of the subject + rank) + side -- the buffer is in contract order.  The
//                      haplotype is found or inserted in an open-addressing table (64-bit compare-and-swap on the key word;
//                      slot numbers are arbitrary and never leave the device); the record's group is slot * P + population.
//   em_radix_*         a stable LSD radix sort of (group, position) by group, 8 bits a pass: groups become runs, each run
//                      still in contract order
//   em_gather_kernel   the weights in sorted order
//   em_sum_kernel      one lane per run: counter = ((counter + w) + w) + ...
// A haplotype that holds an allele the dictionary does not know (an id private to its subject, grim_hip.h grim_tokenize) can
// never equal a dictionary-only one; its contributions go to a spill list the host folds by allele TEXT.
//
// The sharded M-step: a contract of its own.  The promise above holds because a batch's sums start from the counters the
// batches before it left; accumulators that run at the same time (one per rank, grim/shard.py) cannot give that, so their
// tables are MERGED, and the order of every sum is stated anew:
//   the input is cut into chunks of chunk_lines lines, chunk c = global lines [c * chunk_lines, ...) (as chunk_offsets cuts it);
//   T_c = the table of chunk c alone: the M-step above over the chunk's lines into an EMPTY accumulator (the block cuts
//     inside a chunk stay invisible); S_c = the chunk's spilled counts, (population, haplotype text) -> count, folded in
//     the chunk's contract order;
//   count[k, p] = ((T_c0[k, p] + T_c1[k, p]) + T_c2[k, p]) + ...  fp64, no fma, over the chunks c0 < c1 < ... whose table
//     holds the entry (k, p), in ascending chunk number; the spilled counts fold the same way.  A first contribution may be
//     written +0.0 + x: every count is >= +0.0, so these are the same bits.
// The answer depends on chunk_lines.  It does not depend on the number of ranks, on which rank ran which chunk, on the order
// in which tables arrive (they are folded by chunk number), or on block_lines; with one chunk it is the M-step above, bit
// for bit.  The statistics (subjects used, skipped for Plan C, contributions, spill) are the sums over the chunks.
//
// Two merge doors add a table to an accumulator (dst.counts[k, p] = dst.counts[k, p] + x, through ONE device function):
//   em_merge_kernel          one lane per slot of the source accumulator's table, where both tables lie: for every set bit p
//                            of the slot's popmask the key is found or inserted in dst and the counter added
//   em_merge_records_kernel  one lane per entry of an exported table keys / pops / counts [n] (grim_em_export's order)
// Keys are unique within a source, (key, population) pairs within an exported table: each dst counter is written by exactly
// one lane of a call, so no floating-point atomics and no order inside a call; the order BETWEEN calls is the caller's (the
// fold above calls in chunk order).  The host makes room first by the accumulator's own rule (used + incoming keys <=
// cap / 2, em_rehash).  A merge is not a batch: spill records, their ordinals and the subject statistics do not move, and
// the source's spill list is not merged (the host folds it by text).
#pragma once
#include "grim_dev.h"

#define GRIM_EM_NONE 0xFFFFFFFFu
#define GRIM_EM_KEYMASK ((1ull << GRIM_KEY_GRAPH_ORDER) - 1ull)  // the alleles of a key: how the haplotype was spelled is dropped
#define GRIM_EM_CHUNK 2048u                                      // contributions one wave sorts per radix pass
// per-call and running counters (device, u64): the host reads the block after every call
enum { EM_S_USED = 0, EM_S_PLANC = 1, EM_S_UNSUPPORTED = 2, EM_S_SPILL = 3, EM_S_TABLE = 4, EM_S_ENTRIES = 5, EM_S_FAULT = 6, EM_S_COUNT = 8 };

struct EmTable {
  unsigned long long *keys;     // [cap] GRIM_VALID | key, 0 = empty
  unsigned long long *popmask;  // [cap] bit p: counts[slot * P + p] has been added to
  double *counts;               // [cap * P]
  uint32_t mask;                // cap - 1
  uint32_t P;
};

struct EmLimits {
  uint32_t n_alleles[GRIM_MAXL];  // dictionary size per locus slot: a key field above it is a private allele
};

__device__ __forceinline__ bool em_skipped(const grim_subject_result &r, uint32_t rows_used) {
  if (r.status != GRIM_ST_OK) return true;
  const uint32_t n = r.n_rows[GRIM_T_PMUG], off = r.row_off[GRIM_T_PMUG];
  if (n == 0 || off > rows_used || n > rows_used - off) return true;
  const uint8_t plan = r.plan_phased ? r.plan_phased : r.plan;
  return plan == 'c';
}

// rows per subject (0 = skipped) into cnt[0..n_subj); statistics
__global__ __launch_bounds__(256) void em_count_kernel(const grim_subject_result *res, uint32_t n_subj, uint32_t rows_used, uint32_t *cnt,
                                                       unsigned long long *stat) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  uint32_t used = 0, planc = 0, unsup = 0;
  if (s < n_subj) {
    const grim_subject_result r = res[s];
    const bool skip = em_skipped(r, rows_used);
    cnt[s] = skip ? 0u : r.n_rows[GRIM_T_PMUG];
    used = skip ? 0u : 1u;
    unsup = r.status == GRIM_ST_UNSUPPORTED;
    if (skip && r.status == GRIM_ST_OK && r.n_rows[GRIM_T_PMUG] != 0 && (r.plan_phased ? r.plan_phased : r.plan) == 'c') planc = 1;
  }
  const uint32_t n_used = __popcll(__ballot(used)), n_planc = __popcll(__ballot(planc)), n_unsup = __popcll(__ballot(unsup));
  if ((threadIdx.x & 63u) == 0) {
    if (n_used) atomicAdd(stat + EM_S_USED, (unsigned long long)n_used);
    if (n_planc) atomicAdd(stat + EM_S_PLANC, (unsigned long long)n_planc);
    if (n_unsup) atomicAdd(stat + EM_S_UNSUPPORTED, (unsigned long long)n_unsup);
  }
}

// exclusive scan of a[0..n) in place by ONE workgroup; a[n] = the total
__global__ __launch_bounds__(1024) void em_scan_kernel(uint32_t *a, uint32_t n) {
  __shared__ uint32_t sh[1024];
  const uint32_t tid = threadIdx.x;
  const uint32_t per = (n + 1023u) / 1024u;
  const uint32_t lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
  uint32_t s = 0;
  for (uint32_t i = lo; i < hi; ++i) s += a[i];
  sh[tid] = s;
  __syncthreads();
  for (uint32_t off = 1; off < 1024u; off <<= 1) {
    const uint32_t v = tid >= off ? sh[tid - off] : 0u;
    __syncthreads();
    sh[tid] += v;
    __syncthreads();
  }
  uint32_t run = sh[tid] - s;
  for (uint32_t i = lo; i < hi; ++i) {
    const uint32_t t = a[i];
    a[i] = run;
    run += t;
  }
  if (tid == 1023u) a[n] = sh[1023];
}

// slot of `key` in the table, inserted when new.  The caller has made room (used + inserts <= cap / 2), so a probe
// sequence ends; GRIM_EM_NONE after a full turn all the same.
__device__ __forceinline__ uint32_t em_find_or_insert(const EmTable &T, uint64_t key, unsigned long long *stat) {
  const unsigned long long word = key | GRIM_VALID;
  uint32_t s = (uint32_t)mix64(key) & T.mask;
  for (uint32_t turn = 0; turn <= T.mask; ++turn) {
    unsigned long long cur = __hip_atomic_load(T.keys + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == 0ull) {
      cur = atomicCAS(T.keys + s, 0ull, word);
      if (cur == 0ull) {
        atomicAdd(stat + EM_S_TABLE, 1ull);
        return s;
      }
    }
    if (cur == word) return s;
    s = (s + 1u) & T.mask;
  }
  return GRIM_EM_NONE;
}

struct EmSpill {  // = grim_em_spill_rec
  uint64_t key;
  double w;
  uint32_t batch, subject, row;
  uint16_t pop, side;
};

// one wave per subject
__global__ __launch_bounds__(256) void em_weight_kernel(const grim_subject_result *res, const grim_row *rows, uint32_t n_subj,
                                                        const uint32_t *first, EmTable T, EmLimits L, uint32_t batch_no,
                                                        uint32_t *grp, uint32_t *idx, double *w, EmSpill *spill, uint32_t spill_cap,
                                                        unsigned long long *stat) {
  const uint32_t s = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (s >= n_subj) return;
  const uint32_t f = first[s], n = first[s + 1] - f;
  if (n == 0) return;
  const grim_row *R = rows + res[s].row_off[GRIM_T_PMUG];
  double total = R[0].prob;  // every lane: the same sequential sum
  for (uint32_t k = 1; k < n; ++k) total = total + R[k].prob;
  for (uint32_t k = lane; k < n; k += 64u) {
    const grim_row r = R[k];
    const double wk = r.prob / total;
    for (uint32_t side = 0; side < 2u; ++side) {
      const uint64_t key = (side ? r.b : r.a) & GRIM_EM_KEYMASK;
      const uint32_t pop = side ? r.popb : r.popa;
      const uint32_t pos = 2u * (f + k) + side;
      bool priv = pop >= T.P;
      for (int q = 0; q < GRIM_MAXL; ++q) priv |= (uint32_t)((key >> (GRIM_ABITS * q)) & 0xFFFu) > L.n_alleles[q];
      uint32_t g = GRIM_EM_NONE;
      if (!priv) {
        const uint32_t slot = em_find_or_insert(T, key, stat);
        if (slot == GRIM_EM_NONE)
          atomicAdd(stat + EM_S_FAULT, 1ull);
        else
          g = slot * T.P + pop;
      } else {
        const unsigned long long at = atomicAdd(stat + EM_S_SPILL, 1ull);  // any order: the host sorts the records
        if (at < spill_cap) {
          EmSpill e;
          e.key = key;
          e.w = wk;
          e.batch = batch_no;
          e.subject = s;
          e.row = k;
          e.pop = (uint16_t)pop;
          e.side = (uint16_t)side;
          spill[at] = e;
        }
      }
      grp[pos] = g;
      idx[pos] = pos;
      w[pos] = wk;
    }
  }
}

// ---- stable LSD radix sort of (grp, idx) by grp: one wave per chunk of GRIM_EM_CHUNK records -----------------------------
// records without a group (GRIM_EM_NONE) have every digit 255 in every pass the host runs (it sorts one bit more than the
// largest group needs), so they end behind all groups
__global__ __launch_bounds__(64) void em_radix_hist_kernel(const uint32_t *kin, uint32_t n, uint32_t n_chunks, uint32_t shift, uint32_t *cnt) {
  __shared__ uint32_t hist[256];
  const uint32_t c = blockIdx.x, lane = threadIdx.x;
  for (uint32_t d = lane; d < 256u; d += 64u) hist[d] = 0;
  __syncthreads();
  const uint32_t lo = c * GRIM_EM_CHUNK, hi = lo + GRIM_EM_CHUNK < n ? lo + GRIM_EM_CHUNK : n;
  for (uint32_t i = lo + lane; i < hi; i += 64u) atomicAdd(&hist[(kin[i] >> shift) & 255u], 1u);
  __syncthreads();
  for (uint32_t d = lane; d < 256u; d += 64u) cnt[d * n_chunks + c] = hist[d];
}

__global__ __launch_bounds__(64) void em_radix_scatter_kernel(const uint32_t *kin, const uint32_t *vin, uint32_t *kout, uint32_t *vout,
                                                              uint32_t n, uint32_t n_chunks, uint32_t shift, const uint32_t *start) {
  __shared__ uint32_t base[256];
  const uint32_t c = blockIdx.x, lane = threadIdx.x;
  for (uint32_t d = lane; d < 256u; d += 64u) base[d] = start[d * n_chunks + c];
  __syncthreads();
  const uint32_t lo = c * GRIM_EM_CHUNK, hi = lo + GRIM_EM_CHUNK < n ? lo + GRIM_EM_CHUNK : n;
  for (uint32_t i0 = lo; i0 < hi; i0 += 64u) {  // the same trip count on every lane
    const uint32_t i = i0 + lane;
    const bool valid = i < hi;
    const uint32_t k = valid ? kin[i] : 0u, v = valid ? vin[i] : 0u;
    const uint32_t d = (k >> shift) & 255u;
    unsigned long long same = __ballot(valid);  // lanes of this step with my digit
    for (uint32_t bit = 0; bit < 8u; ++bit) {
      const unsigned long long b = __ballot((d >> bit) & 1u);
      same &= ((d >> bit) & 1u) ? b : ~b;
    }
    uint32_t pos = 0;
    if (valid) pos = base[d] + __popcll(same & ((1ull << lane) - 1ull));
    __syncthreads();
    if (valid && (same >> lane) == 1ull) base[d] += __popcll(same);  // the last lane of each digit moves its head
    __syncthreads();
    if (valid && pos < n) {
      kout[pos] = k;
      vout[pos] = v;
    }
  }
}

__global__ __launch_bounds__(256) void em_gather_kernel(const uint32_t *idx, const double *w, double *ws, uint32_t n) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j < n) ws[j] = w[idx[j]];
}

// one lane per run of equal groups: the carried counter plus the run's weights, left to right
__global__ __launch_bounds__(256) void em_sum_kernel(const uint32_t *grp, const double *ws, uint32_t n, EmTable T, unsigned long long *stat) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n) return;
  const uint32_t g = grp[j];
  if (g == GRIM_EM_NONE || (j > 0 && grp[j - 1] == g)) return;
  double c = T.counts[g];
  uint32_t k = j;
  do {
    c = c + ws[k];
    ++k;
  } while (k < n && grp[k] == g);
  T.counts[g] = c;
  const uint32_t slot = g / T.P, pop = g - slot * T.P;
  const unsigned long long bit = 1ull << pop;
  if (!(atomicOr(T.popmask + slot, bit) & bit)) atomicAdd(stat + EM_S_ENTRIES, 1ull);
}

// ---- merge: one accumulator's table, or an exported one, added to another ---------------------------------------------------
// the add both merge doors share: entry (slot t of D, population p) takes x.  Keys are unique within a source and the
// (key, population) pairs of an exported table are, so exactly one lane of a launch writes a counter: a plain read, one
// fp64 add, a plain write.  A counter that was never added to holds +0.0.
__device__ __forceinline__ void em_merge_add(const EmTable &D, uint32_t t, uint32_t p, double x, unsigned long long *stat) {
  const uint64_t at = (uint64_t)t * D.P + p;
  D.counts[at] = D.counts[at] + x;
  const unsigned long long bit = 1ull << p;
  if (!(atomicOr(D.popmask + t, bit) & bit)) atomicAdd(stat + EM_S_ENTRIES, 1ull);
}

// one lane per slot of S: every entry of the slot into D
__global__ __launch_bounds__(256) void em_merge_kernel(EmTable S, EmTable D, unsigned long long *stat) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s > S.mask) return;
  const unsigned long long word = S.keys[s];
  unsigned long long m = S.popmask[s];
  if (word == 0ull || m == 0ull) return;
  const uint32_t t = em_find_or_insert(D, word & ~GRIM_VALID, stat);
  if (t == GRIM_EM_NONE) {
    atomicAdd(stat + EM_S_FAULT, 1ull);
    return;
  }
  while (m) {
    const uint32_t p = (uint32_t)__ffsll(m) - 1u;
    m &= m - 1ull;
    if (p < S.P && p < D.P) em_merge_add(D, t, p, S.counts[(uint64_t)s * S.P + p], stat);
  }
}

// one lane per entry of keys / pops / counts [n] (the host has checked them): the entry into D
__global__ __launch_bounds__(256) void em_merge_records_kernel(const unsigned long long *keys, const uint32_t *pops, const double *counts,
                                                               uint32_t n, EmTable D, unsigned long long *stat) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = pops[i];
  if (p >= D.P) return;
  const uint32_t t = em_find_or_insert(D, keys[i], stat);
  if (t == GRIM_EM_NONE) {
    atomicAdd(stat + EM_S_FAULT, 1ull);
    return;
  }
  em_merge_add(D, t, p, counts[i], stat);
}

// every entry of `from` into `to` (twice the size, zeroed), counters carried
__global__ __launch_bounds__(256) void em_rehash_kernel(EmTable from, EmTable to, unsigned long long *stat) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s > from.mask) return;
  const unsigned long long word = from.keys[s];
  if (word == 0ull) return;
  const uint64_t key = word & ~GRIM_VALID;
  uint32_t t = (uint32_t)mix64(key) & to.mask;
  bool placed = false;
  for (uint32_t turn = 0; turn <= to.mask && !placed; ++turn) {
    if (atomicCAS(to.keys + t, 0ull, word) == 0ull)
      placed = true;
    else
      t = (t + 1u) & to.mask;
  }
  if (!placed) {
    atomicAdd(stat + EM_S_FAULT, 1ull);
    return;
  }
  to.popmask[t] = from.popmask[s];
  for (uint32_t p = 0; p < from.P; ++p) to.counts[(uint64_t)t * to.P + p] = from.counts[(uint64_t)s * from.P + p];
}
