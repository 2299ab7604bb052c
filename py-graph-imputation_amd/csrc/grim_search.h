// grim_search.h -- donor search: each patient's best N donors by match probability, selected on the device (gfx950, wave64)
// from the ungraded records mt_pair_kernel<DIR, false> leaves in the matcher's result buffer (include/grim_hip.h, grim_search_*).
//
// Contract.  Input: the inputs of grim_match.h (keep mask K, n_alleles, patients set once, donors in any number of runs), and
//   top_n   in 1..GRIM_SEARCH_MAX_N
//   min_p0  a double that is not NaN
//   ids     per run one uint32_t per donor, distinct over the whole search; they are the caller's
//   Candidates.  A pair (p, d) is a candidate iff it is computed under grim_match.h (both subjects MT_F_VALID, neither
//     MT_F_PRIVATE: decided from the two flag arrays, never from the record's bytes) and rec.mm[0] >= min_p0.  Every mm value of
//     a computed pair is finite and >= +0.0 (sums of products of weights that are finite and >= 0, started from +0.0), so plain
//     > and == on doubles are a total preorder on them: there is no NaN to handle and no -0.0 to tell from +0.0.
//   Order.  Candidate x comes before candidate y iff
//       x.mm[0] > y.mm[0], or
//       the mm[0] are equal and x.mm[1] > y.mm[1]   (mm[1] always exists: 2|K| >= 2), or
//       both are equal and x.id < y.id.
//     Ids are distinct, so the order is strict and the answer does not depend on how the selection is done: not on the tile, on
//     the block cuts or on the order of the runs.  No floating-point operation is added: the records are grim_match.h's.
//   Result per patient: a count n_hits <= top_n and top_n slots of grim_search_hit { donor, reserved = 0, rec } (136 bytes).  The
//     first n_hits slots hold the first candidates in that order over all runs since the patients were set or the search was
//     reset; the other slots are donor = 0xFFFFFFFF with a zero record.  Results are patient-major.
//   Statistics: grim_match.h's seven counters summed over the runs, and `candidates`, the pairs that passed the threshold,
//     counted as u64 on the device.
//   Merge (the merge door of include/grim_hip.h): n_lists hit lists in the layout of the results, in[(l * n_p + p) * top_n + k]
//     with counts in_cnt[l * n_p + p], each with this search's top_n slots per patient, n_lists <= SR_MERGE_MAX_LISTS.
//     Entries: the first in_cnt slots of list l and patient p are entries (donor, rec); later slots are not looked at.
//     Candidates: an entry is a candidate iff rec.mm[0] >= min_p0, the search's own threshold; a list made under a lower one
//       is filtered.  The patients' flags are not consulted: a hit is a record some search computed.
//     Selection: the patient's new running list is the first top_n, in the strict order, of (its running list so far) united
//       with (the candidates of all lists).  Records and ids are copied bit for bit, reserved = 0; unused slots are
//       donor = 0xFFFFFFFF with a zero record; no floating-point operation is added.  Runs and merges that follow see the
//       merged list as the running list.
//     Ids distinct over everything the search has seen stay the caller's duty; a repeat across lists is not detected: both
//       entries are kept and nothing faults.
//     Left alone: the eight summed statistics, the matcher and its flags and donors (they speak of the last run).  The two
//       times become the merge's device time.
//     The host refuses, before any upload: another number of patients, a null array with something to read, too many lists, a
//       count above top_n, an entry with donor = 0xFFFFFFFF or reserved != 0, an entry whose mm[0] or mm[1] is NaN, infinite
//       or < 0, and a list whose entries are not in the strict order (entry k + 1 after entry k under sr_before; this catches
//       an id repeated within a list).  So the kernels meet only finite values >= 0 here too.
//
// Deliberately plain: no floating-point atomics, no inline assembly, one integer atomic per level-0 tile for the statistic.
//   sr_import_kernel  grid (slots of all lists, patients): one thread per uploaded slot, coalesced over the slot index.  Reads
//                     mm[0], mm[1] and the id of its hit (stride 136 bytes) and its list's count (clamped to top_n) and writes
//                     one key entry into the key lists a merging level reads: a candidate with the source index SR_SRC_IN |
//                     (l * top_n + k), everything else as a sentinel; writes the per-list counts too.  The merging levels of
//                     a merge are sr_tile_kernel on those lists, with the running list as `extra`; at least one level runs.
//   sr_tile_kernel    grid (tiles, patients).  A workgroup takes one tile of a patient's candidate stream, builds one key entry
//                     per candidate in LDS (mm0, mm1, id, and a source index saying where the full record lies: 24 bytes an
//                     entry, 48 KB at SR_TILE), makes everything else, up to a power of two, a sentinel that sorts last, sorts
//                     the tile with a bitonic network under the strict order, and writes its first min(top_n, candidates)
//                     entries and their count.  Level 0 (keys == nullptr): the stream is the patient's donors of this run,
//                     `tile` at a time; mm[0] and mm[1] come straight out of the pair kernel's records (stride 128 bytes) and
//                     candidates are told by the two flag arrays.  Merging levels: the stream is the lists a level below wrote
//                     (top_n slots each, a count each), tile / top_n whole lists at a time; the patient's running list from the
//                     earlier runs enters the first merging level as one more list (`extra`).  Levels repeat until one list
//                     per patient is left; 2 top_n <= tile guarantees progress.
//   sr_gather_kernel  one workgroup per patient: copies the 128-byte records of the kept entries into the new running hit list,
//                     from this run's result buffer, from the previous running list or (SR_SRC_IN, a merge) from the uploaded
//                     hit lists as the source index says, writes the
//                     running list's keys for the next run, n_hits and the unused slots.  The running list is double-buffered:
//                     no kernel reads what it writes.
//   Every loop bound is a count read once; every index taken from device data (a list's count, a source index) is checked
//   against the buffer it goes into before it is used.
#pragma once
#include "grim_match.h"

#define SR_TILE 2048u              // entries of a tile, at most; = GRIM_SEARCH_TILE_MAX
#define SR_THREADS 256u
#define SR_SENTINEL 0xFFFFFFFFu    // source index of an entry that is no candidate
#define SR_SRC_PREV 0x80000000u    // source index: slot (low bits) of the patient's previous running list, not a donor of this run
#define SR_SRC_IN 0x40000000u      // source index: slot l * top_n + k (low bits) of the hit lists a merge uploaded; a run's donor
                                   // indices stay below 2^24
#define SR_NO_DONOR 0xFFFFFFFFu    // = GRIM_SEARCH_NO_DONOR
#define SR_MERGE_MAX_LISTS 4096u   // = GRIM_SEARCH_MERGE_MAX_LISTS: lists x top_n stays below 2^20

struct SrKey {  // 24 bytes
  double mm0, mm1;
  uint32_t id, src;
};

struct SrHit {  // = grim_search_hit
  uint32_t donor, reserved;
  double rec[MT_REC];
};

// the strict order; a sentinel (mm0 = mm1 = -1.0, id = 0xFFFFFFFF) comes after every candidate, whose mm0 is >= 0
__host__ __device__ __forceinline__ bool sr_before(double a0, double a1, uint32_t ai, double b0, double b1, uint32_t bi) {
  if (a0 > b0) return true;
  if (a0 == b0) {
    if (a1 > b1) return true;
    if (a1 == b1) return ai < bi;
  }
  return false;
}

// grid (tiles, patients of this launch); p0 = the first patient of the launch; block SR_THREADS.
//   level 0:  keys == nullptr.  rec = the pair kernel's records [n_p][n_d], ids[n_d], pflags[n_p], dflags[n_d]; tile t takes
//             donors [t * tile, (t + 1) * tile) of n_d.
//   merging:  keys[(p * n_lists + l) * top_n + k], counts[p * n_lists + l], l < n_lists; list n_lists, when extra is given, is
//             extra[p * top_n + k] with extra_cnt[p]; tile t takes lists [t * per, (t + 1) * per), per = tile / top_n.
//   out:      okeys[(p * gridDim.x + t) * top_n + k], ocounts[p * gridDim.x + t]
__global__ __launch_bounds__(SR_THREADS) void sr_tile_kernel(const double *rec, const uint32_t *ids, const uint8_t *pflags,
                                                             const uint8_t *dflags, uint32_t n_p, uint32_t p0, uint32_t n_d,
                                                             double min_p0, const SrKey *keys, const uint32_t *counts,
                                                             uint32_t n_lists, const SrKey *extra, const uint32_t *extra_cnt,
                                                             uint32_t tile, uint32_t top_n, SrKey *okeys, uint32_t *ocounts,
                                                             unsigned long long *candidates) {
  __shared__ double s0[SR_TILE], s1[SR_TILE];
  __shared__ uint32_t sid[SR_TILE], ssrc[SR_TILE];
  __shared__ uint32_t s_cnt;
  const uint32_t t = blockIdx.x, p = p0 + blockIdx.y, tid = threadIdx.x;
  if (p >= n_p || tile > SR_TILE || top_n == 0u || 2u * top_n > tile) return;
  uint32_t entries;  // of this tile's part of the stream, read once: every loop below runs to it or to n
  if (keys == nullptr) {
    const uint64_t lo = (uint64_t)t * tile;
    entries = lo >= n_d ? 0u : (n_d - lo < tile ? (uint32_t)(n_d - lo) : tile);
  } else {
    const uint32_t per = tile / top_n, total = n_lists + (extra ? 1u : 0u);
    const uint64_t lo = (uint64_t)t * per;
    entries = lo >= total ? 0u : (total - lo < per ? (uint32_t)(total - lo) : per) * top_n;
  }
  uint32_t n = 2u;  // the power of two the network sorts
  while (n < entries) n <<= 1;
  if (tid == 0) s_cnt = 0u;
  if (keys == nullptr) {
    const bool p_ready = (pflags[p] & (MT_F_VALID | MT_F_PRIVATE)) == MT_F_VALID;
    for (uint32_t e = tid; e < n; e += SR_THREADS) {
      double m0 = -1.0, m1 = -1.0;
      uint32_t id = 0xFFFFFFFFu, src = SR_SENTINEL;
      if (e < entries) {
        const uint32_t d = t * tile + e;  // < n_d
        if (p_ready && (dflags[d] & (MT_F_VALID | MT_F_PRIVATE)) == MT_F_VALID) {
          const double *r = rec + ((uint64_t)p * n_d + d) * MT_REC;
          const double x0 = r[0];
          if (x0 >= min_p0) {
            m0 = x0;
            m1 = r[1];
            id = ids[d];
            src = d;
          }
        }
      }
      s0[e] = m0;
      s1[e] = m1;
      sid[e] = id;
      ssrc[e] = src;
    }
  } else {
    const uint32_t per = tile / top_n;
    for (uint32_t e = tid; e < n; e += SR_THREADS) {
      double m0 = -1.0, m1 = -1.0;
      uint32_t id = 0xFFFFFFFFu, src = SR_SENTINEL;
      if (e < entries) {
        const uint32_t l = t * per + e / top_n, k = e % top_n;  // l < n_lists + (extra ? 1 : 0)
        const SrKey *list = l < n_lists ? keys + ((uint64_t)p * n_lists + l) * top_n : extra + (uint64_t)p * top_n;
        uint32_t cnt = l < n_lists ? counts[(uint64_t)p * n_lists + l] : extra_cnt[p];
        if (cnt > top_n) cnt = top_n;  // a list holds top_n slots
        if (k < cnt) {
          const SrKey key = list[k];
          if (key.src != SR_SENTINEL) {
            m0 = key.mm0;
            m1 = key.mm1;
            id = key.id;
            src = key.src;
          }
        }
      }
      s0[e] = m0;
      s1[e] = m1;
      sid[e] = id;
      ssrc[e] = src;
    }
  }
  __syncthreads();
  // bitonic network on n entries, n / 2 compare-exchanges a step; the first in the order ends at index 0
  for (uint32_t k = 2u; k <= n; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
      for (uint32_t x = tid; x < (n >> 1); x += SR_THREADS) {
        const uint32_t i = ((x & ~(j - 1u)) << 1) | (x & (j - 1u)), l = i | j;
        const double a0 = s0[i], a1 = s1[i], b0 = s0[l], b1 = s1[l];
        const uint32_t ai = sid[i], bi = sid[l];
        const bool up = (i & k) == 0u;
        if (up ? sr_before(b0, b1, bi, a0, a1, ai) : sr_before(a0, a1, ai, b0, b1, bi)) {
          const uint32_t as = ssrc[i], bs = ssrc[l];
          s0[i] = b0; s1[i] = b1; sid[i] = bi; ssrc[i] = bs;
          s0[l] = a0; s1[l] = a1; sid[l] = ai; ssrc[l] = as;
        }
      }
      __syncthreads();
    }
  }
  // the candidates stand first: their number is the index of the first sentinel (one thread finds the border)
  for (uint32_t e = tid; e < n; e += SR_THREADS)
    if (ssrc[e] != SR_SENTINEL && (e + 1u == n || ssrc[e + 1u] == SR_SENTINEL)) s_cnt = e + 1u;
  __syncthreads();
  const uint32_t found = s_cnt, keep = found < top_n ? found : top_n;
  const uint64_t at = (uint64_t)p * gridDim.x + t;
  for (uint32_t e = tid; e < keep; e += SR_THREADS) {
    SrKey key;
    key.mm0 = s0[e];
    key.mm1 = s1[e];
    key.id = sid[e];
    key.src = ssrc[e];
    okeys[at * top_n + e] = key;
  }
  if (tid == 0) {
    ocounts[at] = keep;
    if (keys == nullptr && found) atomicAdd(candidates, (unsigned long long)found);
  }
}

// grid (ceil(n_lists * top_n / SR_THREADS), patients of this launch); block SR_THREADS.  One thread per uploaded slot
// j = l * top_n + k of patient p: in[(l * n_p + p) * top_n + k], in_cnt[l * n_p + p] -> keys[(p * n_lists + l) * top_n + k],
// counts[p * n_lists + l] (the count clamped to top_n), the layout a merging level of sr_tile_kernel reads.  An entry (k below
// the count) with mm[0] >= min_p0 becomes a key with src = SR_SRC_IN | j; every other slot a sentinel.
__global__ __launch_bounds__(SR_THREADS) void sr_import_kernel(const SrHit *in, const uint32_t *in_cnt, uint32_t n_p, uint32_t p0,
                                                               uint32_t n_lists, uint32_t top_n, double min_p0, SrKey *keys,
                                                               uint32_t *counts) {
  const uint32_t p = p0 + blockIdx.y;
  const uint64_t j = (uint64_t)blockIdx.x * SR_THREADS + threadIdx.x;
  if (p >= n_p || top_n == 0u || n_lists > SR_MERGE_MAX_LISTS || j >= (uint64_t)n_lists * top_n) return;
  const uint32_t l = (uint32_t)(j / top_n), k = (uint32_t)(j % top_n);  // l < n_lists
  uint32_t cnt = in_cnt[(uint64_t)l * n_p + p];
  if (cnt > top_n) cnt = top_n;
  SrKey key = {-1.0, -1.0, 0xFFFFFFFFu, SR_SENTINEL};
  if (k < cnt) {
    const SrHit *h = in + ((uint64_t)l * n_p + p) * top_n + k;
    const double x0 = h->rec[0];
    if (x0 >= min_p0) {
      key.mm0 = x0;
      key.mm1 = h->rec[1];
      key.id = h->donor;
      key.src = SR_SRC_IN | (uint32_t)j;  // j < 2^20
    }
  }
  keys[((uint64_t)p * n_lists + l) * top_n + k] = key;
  if (k == 0u) counts[(uint64_t)p * n_lists + l] = cnt;
}

// grid (patients of this launch); block 64.  keys[p * stride * top_n + k], counts[p * stride]: the patient's one list left.
// rec = this run's records [n_p][n_d]; prev = the previous running list [n_p][top_n] (read only when a source index says so);
// in = the hit lists of a merge, in[(l * n_p + p) * top_n + k] for the source index SR_SRC_IN | (l * top_n + k), which must be
// below in_slots = n_lists * top_n (a run passes null / 0); out = the new one, okeys / ocnt its keys and count for the next run.
__global__ __launch_bounds__(64) void sr_gather_kernel(const SrKey *keys, const uint32_t *counts, uint32_t stride, const double *rec,
                                                       uint32_t n_p, uint32_t p0, uint32_t n_d, const SrHit *prev, uint32_t top_n,
                                                       SrHit *out, SrKey *okeys, uint32_t *ocnt, const SrHit *in,
                                                       uint32_t in_slots) {
  const uint32_t p = p0 + blockIdx.x, lane = threadIdx.x;
  if (p >= n_p) return;
  uint32_t cnt = counts[(uint64_t)p * stride];  // read once
  if (cnt > top_n) cnt = top_n;
  const SrKey *list = keys + (uint64_t)p * stride * top_n;
  uint32_t kept = 0;  // entries whose source index points into a buffer: all of them, unless something is broken
  for (uint32_t k = 0; k < top_n; ++k) {  // a record is 16 doubles: lanes 0..15 copy one each, lane 16 the id
    const uint64_t at = (uint64_t)p * top_n + kept;
    const double *from = nullptr;
    SrKey key = {-1.0, -1.0, SR_NO_DONOR, SR_SENTINEL};
    if (k < cnt) {
      key = list[k];
      if (key.src != SR_SENTINEL) {
        if (key.src & SR_SRC_PREV) {
          const uint32_t slot = key.src & ~SR_SRC_PREV;
          if (prev != nullptr && slot < top_n) from = prev[(uint64_t)p * top_n + slot].rec;
        } else if (in != nullptr && (key.src & SR_SRC_IN)) {
          const uint32_t j = key.src & ~SR_SRC_IN;
          if (j < in_slots) from = in[((uint64_t)(j / top_n) * n_p + p) * top_n + j % top_n].rec;
        } else if (key.src < n_d) {
          from = rec + ((uint64_t)p * n_d + key.src) * MT_REC;
        }
      }
    }
    if (from == nullptr) continue;  // the same on every lane
    if (lane < MT_REC) out[at].rec[lane] = from[lane];
    if (lane == MT_REC) {
      out[at].donor = key.id;
      out[at].reserved = 0u;
      key.src = SR_SRC_PREV | kept;
      okeys[at] = key;
    }
    ++kept;
  }
  for (uint32_t k = kept; k < top_n; ++k) {  // the unused slots
    const uint64_t at = (uint64_t)p * top_n + k;
    if (lane < MT_REC) out[at].rec[lane] = 0.0;
    if (lane == MT_REC) {
      out[at].donor = SR_NO_DONOR;
      out[at].reserved = 0u;
    }
  }
  if (lane == 0) ocnt[p] = kept;
}
