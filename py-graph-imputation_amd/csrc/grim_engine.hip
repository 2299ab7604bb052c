// grim_engine.hip -- libgrim_hip.so: kernels + the C-ABI of include/grim_hip.h (gfx950 only).
//
// Build: hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -fPIC -shared grim_engine.hip -o libgrim_hip.so
// (-ffp-contract=off is REQUIRED: an fma in P1*P2*prior would change the last bit and with it
//  rankings that the reference decides on exact ties).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "grim_plan_a.h"
#include "grim_plan_b.h"
#include "grim_small.h"
#include "grim_medium.h"
#include "grim_mid.h"
#include "grim_tables.h"
#include "grim_tokdev.h"
#include "grim_em.h"
#include "grim_refresh.h"
#include "grim_marginal.h"
#include "grim_match.h"
#include "grim_search.h"
#include "grim_groups.h"
#include "grim_engine_internal.h"
#include "grim_host_internal.h"
#include "grim_sdma.h"

// =================================================================================================
// Plan-A kernel: one workgroup per subject, pulled from a work counter.  Waves build the phase
// sides (one wave per side, wave64 ballots/prefix scans, LDS-staged running top-K); the whole
// workgroup then scores haplotype pairs, dedups, sums and ranks.
// =================================================================================================
__global__ __launch_bounds__(GRIM_WG, GRIM_WG_PER_CU) void grim_plan_a_kernel(DevArgs A) {
  __shared__ WgShared sh;
  __shared__ WaveTop wt[GRIM_NWAVE];
  const int tid = threadIdx.x;
  const int P = A.g.P;
  Slot S = make_slot(A, blockIdx.x);
  // hand-overs of the one-wave kernel (earlier in the stream): the heavier ones, at the back of its list, are
  // taken first, then this kernel's own subjects (heaviest first), then the light hand-overs
  const uint32_t n_bail = A.bail_list ? A.queue[GRIM_Q_BAIL] : 0, n_bail_heavy = A.bail_list ? A.queue[GRIM_Q_BAIL_HEAVY] : 0;
  // behind the mid-size kernel (grim_mid.h) this kernel only takes what that one handed over
  const uint32_t n_mid = A.mid_list ? A.queue[GRIM_Q_MID] : 0;
  if (tid < GRIM_NWAVE * 4) ((unsigned long long *)sh.wctr)[tid] = 0;
  wg_arena(sh, wt);
  __syncthreads();
  for (;;) {
    if (tid == 0) sh.bc[3] = atomicAdd(A.queue + GRIM_Q_GENERAL, 1u);
    __syncthreads();
    const uint32_t w = sh.bc[3];
    if (A.mid_list ? w >= n_mid : w >= A.n_work + n_bail + n_bail_heavy) break;
    uint32_t si;
    if (A.mid_list)
      si = A.mid_list[w];
    else if (w < n_bail_heavy)
      si = A.bail_list[A.n_medium - 1u - w];
    else if (w - n_bail_heavy < A.n_work)
      si = A.order[w - n_bail_heavy];
    else
      si = A.bail_list[w - n_bail_heavy - A.n_work];
    if (tid < 16) ((uint32_t *)&sh.subj)[tid] = ((const uint32_t *)&A.subj[si])[tid];
    if (tid < GRIM_SIDES) {
      sh.Tn[tid] = 0;
      sh.cand_any[tid] = 0;
    }
    if (tid < (int)(sizeof(grim_subject_result) / 4)) ((uint32_t *)&sh.out)[tid] = 0;
    __syncthreads();
    STAMP_BEGIN();
    const unsigned long long t_subject = STAMP_NOW();
    (void)t_subject;
    enumerate_phases(sh);
    const double *prior = A.priors + (uint64_t)sh.subj.prior_idx * P * P;
    const int nph = sh.nph;
    const bool fits = prepare_lists(A, sh, S);
    bool kept = false;
    // open_phases; when no phase has candidates on both sides the reference rewrites the '/'-lists
    // (known alleles only, then the 10 most frequent) and opens again (impute.py:1619-1627)
    for (int stage = 0; fits; ++stage) {
      // one scan of the label for all sides when that is cheaper than opening them one by one (high ambiguity on a big graph)
      bool done = false;
      if (stage == 0 && shared_scan_wanted(A, sh)) done = build_sides_shared_scan(A, sh, S, prior, wt);
      if (stage == 0) HIST(0, done ? 1 : 0, 1);  // (diagnostic build) subjects by opening: bucket 0 side by side, bucket 1 shared scan
      if (!done)
        for (int s = wave_id(); s < 2 * nph; s += GRIM_NWAVE) build_side_plan_a(A, sh, S, prior, wt[wave_id()], s >> 1, s & 1, s);
      __syncthreads();
      kept = false;
      for (int i = 0; i < nph; ++i) kept |= (sh.cand_any[2 * i] && sh.cand_any[2 * i + 1]);
      if (kept || stage == 2) break;
      if (stage == 0) reduce_lists(A, sh, S, prior);
      apply_stage(A, sh, stage + 1);
    }
    STAMP(8);
    const unsigned long long t_sides = STAMP_NOW();
    HIST(1, sh.ntok, (t_sides - t_subject) / 100);  // us in the sides by number of alleles in the GL string
    HIST(2, sh.ntok, 1);
    uint8_t status = GRIM_ST_MISS, reason = 0, plan = 'a';
    if (!fits) {
      status = GRIM_ST_UNSUPPORTED;  // more than GRIM_RTOK_CAP/3 alleles in one GL string
      reason = 5;
    } else if (!kept) {
      // no phase at all: the reference returns its placeholder result and trips over it while writing
      // the phased file (impute.py:1607-1609, 2090-2097)
      status = GRIM_ST_NOPHASE;
    } else {
      const uint32_t np = pair_offsets(sh);
      int e = A.prm.n_ladder;
      if (np > 0) e = ladder_first(A, sh, S, prior, np);
      STAMP(9);
      uint32_t nU = 0;
      double mx = 0.0;
      if (e < A.prm.n_ladder) {
        double eps = A.prm.ladder[e];
        bool first = true;
        if (eps > 0.0) {
          pair_pass(A, sh, S, prior, np, eps, false, &mx);
          STAMP(10);
          eps = mx / 100000.0;  // impute.py:1685
          first = false;
        }
        nU = pair_pass(A, sh, S, prior, np, eps, true, &mx, first);
        STAMP(11);
      }
      const unsigned long long t_pairs = STAMP_NOW();
      (void)t_pairs;
      HIST(3, nU, 1);
      HIST(4, np, 1);
      HIST(5, sh.poff[0] + [&]() { uint32_t e = 0; for (int s = 0; s < 2 * sh.nph; ++s) e += sh.Tn[s]; return e; }(), 1);
      HIST(6, nU, nU);
      HIST(7, nU, (t_pairs - t_subject) / 100);
      if (nU > 0) {
        emit_tables(A, sh, S, nU, sh.out, si);
        STAMP(12);
        status = GRIM_ST_OK;
        if (tid == 0) sh.out.max_prob = mx;
      } else if (A.prm.planb) {
        status = GRIM_ST_UNSUPPORTED;  // replaced by the plan-B kernel's verdict when it runs
        reason = 2;
        if (tid == 0 && A.next_list) push_next(A, si, sh.subj.n_loci <= GRIM_HEAVY_LOCI);
      }
    }
    __syncthreads();
    if (tid == 0) {
      sh.out.status = status;
      sh.out.reason = reason;
      sh.out.plan = plan;
      A.res[si] = sh.out;
    }
    __syncthreads();
  }
  if (tid == 0) {
    unsigned long long c0 = 0, c1 = 0, c2 = 0;
    for (int wv = 0; wv < GRIM_NWAVE; ++wv) {
      c0 += sh.wctr[wv][0];
      c1 += sh.wctr[wv][1];
      c2 += sh.wctr[wv][2];
    }
    atomicAdd(&A.counters[GRIM_C_PROBES], c0);
    atomicAdd(&A.counters[GRIM_C_NBR], c1);
    atomicAdd(&A.counters[GRIM_C_FREQ], c2);
  }
}


// The half-wave kernel writes a subject's rows at a fixed stride (no atomics on its hot path) into a staging region at
// the TOP of the row pool; most of that region stays empty (1 + ~1.3 of 11 rows per subject).  This kernel moves the
// rows that exist into the bump-allocated part of the pool -- one allocation per wave of 64 subjects -- and re-bases the
// subjects' row offsets, so that the batch's D2H copy carries ~75 instead of 352 bytes of rows per subject.
__global__ __launch_bounds__(64) void grim_small_compact_kernel(DevArgs A, const uint32_t *order_s, const SmallRec *recs, uint32_t n_small,
                                                                 uint32_t stage_base, uint32_t stride) {
  const uint32_t w = blockIdx.x * 64 + threadIdx.x;
  const int lane = lane_id();
  // a subject's staged rows are one run: [the row that is its .umug, .umug.pops and .pmug.pops row, its .pmug rows] from stage_base + w * stride
  uint32_t si = 0, cnt = 0;
  uint4 ro = make_uint4(0, 0, 0, 0), nr = make_uint4(0, 0, 0, 0);
  // record w's subject: from the class list (host-tokenised subjects), or from the record itself (device-tokenised
  // lines: GRIM_NONE where the line is not a device subject)
  if (w < n_small) si = order_s ? order_s[w] : recs[w].si;
  if (w < n_small && si != GRIM_NONE) {
    const uint32_t *r = (const uint32_t *)(A.res + si);  // dwords 3..6 row_off, 7..10 n_rows
    ro = make_uint4(r[3], r[4], r[5], r[6]);
    nr = make_uint4(r[7], r[8], r[9], r[10]);
    if ((nr.x | nr.y | nr.z | nr.w) != 0 && ro.z >= stage_base) cnt = GRIM_SMALL_ROWS_FIXED + nr.z;  // .z: GRIM_T_PMUG
  }
  uint32_t incl = cnt;  // inclusive prefix over the wave
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(incl, d);
    if (lane >= d) incl += o;
  }
  const uint32_t total = __shfl(incl, 63);
  if (total == 0) return;
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(A.row_head, total);
  base = __shfl(base, 0);
  if (base + total > stage_base) {  // the pool is full: reported like every other row overflow (the caller splits the batch)
    if (lane == 0) run_overflow(A);
    return;
  }
  if (cnt == 0) return;
  const uint32_t src = stage_base + w * stride, dst = base + incl - cnt;
  const uint4 *sp = (const uint4 *)(A.rows + src);
  uint4 *dp = (uint4 *)(A.rows + dst);
  uint32_t k = 0;
  for (; k + 2 <= cnt; k += 2) {  // two rows (four 16-byte loads) in flight
    const uint4 a0 = sp[2 * k], a1 = sp[2 * k + 1], a2 = sp[2 * k + 2], a3 = sp[2 * k + 3];
    dp[2 * k] = a0;
    dp[2 * k + 1] = a1;
    dp[2 * k + 2] = a2;
    dp[2 * k + 3] = a3;
  }
  if (k < cnt) {
    const uint4 a0 = sp[2 * k], a1 = sp[2 * k + 1];
    dp[2 * k] = a0;
    dp[2 * k + 1] = a1;
  }
  const uint32_t delta = dst - src;  // modulo 2^32: offsets move down
  uint32_t *r = (uint32_t *)(A.res + si);
  r[3] = ro.x + delta;
  r[4] = ro.y + delta;
  r[5] = ro.z + delta;
  r[6] = ro.w + delta;
}

// A finished batch's results, device arena -> pinned host memory, by a few workgroups instead of the DMA engine: the
// engine moves a 1.3 MB block (10 000 config-2 subjects) at ~20 GB/s, which made the D2H copy the slowest stage of the
// stream (62 us per chunk against 33 us of kernels); sixteen-byte stores from 32 workgroups fill the PCIe link without
// taking the chip from the kernels of the next batches (the runtime's own blit kernel, which rocprofv3 forces, does take
// it: the half-wave kernel beside it stretches from 11 to 49 us).  GRIM_EXPORT_KERNEL=0: hipMemcpyAsync as before.
__global__ __launch_bounds__(256) void grim_export_kernel(uint4 *__restrict__ dst, const uint4 *__restrict__ src, uint64_t n16) {
  const uint64_t step = (uint64_t)gridDim.x * 256u;
  uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  for (; i + 3 * step < n16; i += 4 * step) {  // four loads in flight per lane
    const uint4 a = src[i], b = src[i + step], c = src[i + 2 * step], d = src[i + 3 * step];
    dst[i] = a;
    dst[i + step] = b;
    dst[i + 2 * step] = c;
    dst[i + 3 * step] = d;
  }
  for (; i < n16; i += step) dst[i] = src[i];
}

// End of a stage: the run-state block (the GRIM_NCTR counter words, then the GRIM_NQ queue words: grim_dev.h) goes straight
// to the batch's pinned host copy, and -- unless a second stage follows (stage2_pending), which needs the heads as they
// are -- the device copy is reset for the next run.  One small kernel instead of a copy engine job now and a reset launch next time.
__global__ void grim_finish_kernel(unsigned long long *state, unsigned long long *host_state, uint32_t row_head0, int after_plan_b) {
  __shared__ uint32_t pending;
  if (threadIdx.x == 0) pending = after_plan_b ? 0u : stage2_pending((const uint32_t *)(state + GRIM_NCTR));
  for (int i = threadIdx.x; i < GRIM_STATE_WORDS; i += blockDim.x) host_state[i] = state[i];
  __syncthreads();
  if (pending) return;  // the second stage works on this state
  for (int i = threadIdx.x; i < GRIM_NCTR; i += blockDim.x) state[i] = 0;
  if (threadIdx.x < GRIM_NQ) ((uint32_t *)(state + GRIM_NCTR))[threadIdx.x] = threadIdx.x == GRIM_Q_ROWS ? row_head0 : 0u;
}

// =================================================================================================
// host side
// =================================================================================================
struct grim_ctx {
  int device;
  hipStream_t stream;
  hipStream_t copy_stream;  // D2H of a finished batch while the next batch's kernels run (engine_batch_fetch_issue)
  hipStream_t up_stream;    // H2D of the next batch's input while this batch's kernels run (engine_batch_load)
  GrimSdma *sdma;           // results D2H on an SDMA engine of its own (grim_sdma.h); nullptr: export kernel / hipMemcpyAsync
  int export_mode;          // 2 = grim_sdma, 1 = grim_export_kernel, 0 = hipMemcpyAsync on the copy stream
  // Two threads of a stream use one context at the same time (device thread: loads and launches; copy thread: waits,
  // second stages, D2H), so the error text is written and read under its own lock; grim_last_error hands out a
  // per-thread copy.  Everything else a context owns is either immutable after grim_create or guarded by run_mu.
  std::mutex err_mu;
  std::string err;
  std::mutex run_mu;        // binding the scratch block / launching a run's kernels: one thread at a time
  int n_cu;
  // per-workgroup scratch slots, kept across batches (13 GB at the default sizes: allocating them
  // per batch cost more than the kernels)
  void *scratch;
  uint64_t scratch_bytes;
  uint32_t *wctr;           // the table kernels' sliced work counters (grim_dev.h: slice_next), zeroed in front of every use
  // capacity batches a finished stream handed back: the next stream on this context takes them instead of
  // allocating (and pinning) a few hundred MB per slot again
  std::vector<grim_batch *> spare;
};

struct RefreshState;  // device buffers of grim_graph_refresh, made by the first refresh (below the M-step accumulator)

struct grim_graph {
  grim_ctx *ctx;
  DevGraph d;
  std::vector<void *> bufs;
  uint64_t bytes;
  uint32_t max_label;
  // grim_graph_refresh (grim_refresh.h): whether the descriptor's top-link rows can be trusted for it, and why not; the partial
  // nodes by row length (host copies: they go to the device with the first refresh)
  bool refreshable = false;
  std::string refresh_why;
  uint32_t n_a_nbr = 0, full_first = 0, n_full = 0;
  std::vector<uint32_t> rf_short, rf_long;
  RefreshState *rf = nullptr;
  double refresh_ms = 0.0;
};

// Timing mode: one entry per timed interval of a run.  Each has a start/stop event pair in its batch, and a row below with
// its public number (grim_batch_kernel_ms) and whether it counts into GRIM_MS_PLAN_A.  A new kernel of the run path is one
// entry, one row and one launch(...) line.
enum Phase { PH_HALF_WAVE, PH_ONE_WAVE, PH_MID, PH_GENERAL, PH_PLAN_B, PH_TABLES, PH_COMPACT, PH_TOKENIZER, PH_COUNT, PH_NONE = PH_COUNT };
struct PhaseRow {
  int which;
  bool plan_a;
};
static constexpr PhaseRow PHASES[PH_COUNT] = {
    {GRIM_MS_HALF_WAVE, true}, {GRIM_MS_ONE_WAVE, true}, {GRIM_MS_MID, true},      {GRIM_MS_GENERAL, true},
    {GRIM_MS_PLAN_B, false},   {GRIM_MS_TABLES, false},  {GRIM_MS_COMPACT, false}, {GRIM_MS_TOKENIZER, false},
};
// every per-kernel value of the header, GRIM_MS_PLAN_B .. GRIM_MS_MID, is the number of exactly one phase
static constexpr bool phases_match_header() {
  for (int w = GRIM_MS_PLAN_B; w <= GRIM_MS_MID; ++w) {
    int n = 0;
    for (int p = 0; p < PH_COUNT; ++p) n += PHASES[p].which == w;
    if (n != 1) return false;
  }
  return PH_COUNT == GRIM_MS_MID - GRIM_MS_PLAN_B + 1;
}
static_assert(phases_match_header(), "PHASES and the GRIM_MS_* values of grim_hip.h have drifted apart");
static_assert(GRIM_MS_TOTAL == 0 && GRIM_MS_PLAN_A == 1 && GRIM_MS_MID < GRIM_MS_MEAN && GRIM_MS_MEAN == 0x10, "the GRIM_MS_* values are frozen");

struct grim_batch {
  grim_ctx *ctx;
  const grim_graph *g;
  DevArgs a;
  // Three arenas, laid out per load (engine_batch_plan): what the next batch holds decides the offsets, so ONE copy
  // moves a batch's whole input to the device and ONE copy brings its results back.
  //   in   (device + pinned mirror): run state | subjects | half-wave records | three class lists | tokens
  //   work (device only)           : hand-over lists, per-wave counters
  //   out  (device + pinned mirror): result headers | row pool
  uint8_t *d_in, *h_in, *d_work, *d_out, *h_out;
  uint64_t in_cap, work_cap, out_cap, h_out_cap;
  double *d_priors, *h_priors;  // prior matrices: their own small buffers, uploaded only when the set changes
  uint8_t *d_pool;              // the table kernels' arena (device only; grows at load time): pair records, per-item state,
  uint64_t pool_cap, pool_bytes; // bucket starts, cells, work units, bucket order, groups, probabilities in cell order
  uint64_t pool_want;            // records the last run asked for when it ran out (the next load sizes the pool for it)
  uint64_t pool_asked;           // pair records the last run asked for
  EngineLoad last_load;          // what the last engine_batch_load was given (priors not kept): a run that outgrew the pair pool loads again
  bool in_retry;
  uint32_t priors_cap, priors_up;
  uint64_t row_limit;   // rows a run may use
  EnginePlan plan;      // what the arenas are laid out for
  uint64_t off_tok, off_rows;  // byte offsets inside in / out
  EngineHost h;         // pointers into the pinned arenas (valid until the next plan)
  uint32_t n_subj, n_slots;
  uint32_t n_small_waves;
  bool small_ctr_pending;  // the half-wave kernel's per-wave counts have not been added to `counters` yet
  unsigned long long *hstate;  // pinned: counters + work/row heads of the last run
  SmallRec *d_small;
  uint32_t *d_os, *d_om;
  // device tokenizer (plan.text_cap != 0)
  const grim_devdict *dict;
  LineRec *d_lines;
  uint8_t *d_text;
  SmallRec *d_dsmall;   // its half-wave records, one slot per line (work arena)
  uint64_t off_subj;    // the input arena up to here is all a run without host-tokenised subjects needs
  uint32_t dev_lo, dev_hi, n_dev_lines, n_irregular;
  uint32_t n_host_small_waves;
  uint32_t n_medium;
  uint32_t n_small, n_general, small_stride;
  uint64_t scratch_need;  // bytes of per-workgroup scratch this batch's runs need (bound at run time)
  hipEvent_t ev_copy;  // behind the D2H copy of engine_batch_fetch_issue
  int ct_slot = -1;    // GRIM_DEBUG_COPYTIME
  uint64_t sdma_job = 0;  // completion signal of grim_sdma copies (made on first use)
  bool fetch_hsa = false; // the copy in flight was issued through grim_sdma
  bool up_pending = false; // an input copy is on the upload stream and the launch stream has not been ordered behind it yet
  hipEvent_t ev_up;    // behind the H2D copy of engine_batch_load: the batch's kernels wait for it
  hipEvent_t ev_done;  // recorded behind the last kernel of a stage: what engine_batch_wait waits for (not the whole stream --
                       // the device thread may have queued the next chunk's kernels behind it already)
  bool enqueued;       // stage 1 is in flight (engine_batch_enqueue without its engine_batch_wait)
  hipEvent_t ev[PH_COUNT][2];  // timing mode: start/stop of every phase
  uint32_t launched;  // timing mode: bit p = phase p was launched with its events and has not been read back yet
  bool timing;       // GRIM_TIMING=1 or grim_batch_set_timing: direct launches with per-kernel events instead of the graph replay
  hipGraphExec_t gexec;
  int graph_state;  // 0 not tried, 1 captured, -1 direct launches
  float ms[PH_COUNT];       // timing mode: the phases of the last run
  double acc_ms[PH_COUNT];  // their sums over the timed runs since timing was switched on
  uint32_t n_timed;
  uint32_t rows_used;
  bool ran_ok = false;  // the last grim_batch_run finished and nothing was loaded since: res / rows hold its results (grim_em_accumulate)
  unsigned long long counters[GRIM_C_SLICE0];  // the last run's GRIM_C_* words, the slices folded in
};

static thread_local std::string g_err;

static void set_err(grim_ctx *c, const std::string &m) {
  g_err = m;
  if (c) {
    std::lock_guard<std::mutex> lk(c->err_mu);
    c->err = m;
  }
}

#define HIPCHK(call, ctxp, ret)                                                        \
  do {                                                                                 \
    hipError_t e_ = (call);                                                            \
    if (e_ != hipSuccess) {                                                            \
      set_err((ctxp), std::string(#call) + ": " + hipGetErrorString(e_));             \
      return ret;                                                                      \
    }                                                                                  \
  } while (0)

extern "C" int grim_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

extern "C" grim_ctx *grim_create(int device_id) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    g_err = "grim_create: no HIP device visible";
    return nullptr;
  }
  if (device_id < 0 || device_id >= n) {
    g_err = "grim_create: device id out of range";
    return nullptr;
  }
  grim_ctx *c = new grim_ctx();
  c->device = device_id;
  c->copy_stream = nullptr;
  c->up_stream = nullptr;
  if (hipSetDevice(device_id) != hipSuccess || hipStreamCreate(&c->stream) != hipSuccess ||
      hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&c->up_stream, hipStreamNonBlocking) != hipSuccess) {
    g_err = "grim_create: cannot initialise device";
    delete c;
    return nullptr;
  }
  hipDeviceProp_t prop;
  c->n_cu = 256;
  c->scratch = nullptr;
  c->scratch_bytes = 0;
  c->wctr = nullptr;
  if (hipMalloc((void **)&c->wctr, 4 * GRIM_WCTR_WORDS) != hipSuccess) {
    (void)hipGetLastError();
    g_err = "grim_create: cannot allocate the work counters";
    hipStreamDestroy(c->stream);
    hipStreamDestroy(c->copy_stream);
    hipStreamDestroy(c->up_stream);
    delete c;
    return nullptr;
  }
  if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) c->n_cu = prop.multiProcessorCount;
  // how a stream's results come down: GRIM_EXPORT=sdma|kernel|memcpy (GRIM_EXPORT_KERNEL=0/1 of round 3 still means
  // memcpy / kernel); default sdma when ROCr offers an engine besides the uploads', else the export kernel
  c->sdma = nullptr;
  c->export_mode = 1;
  {
    const char *e = getenv("GRIM_EXPORT");
    int want = 2;
    if (e && !strcmp(e, "kernel")) want = 1;
    else if (e && !strcmp(e, "memcpy")) want = 0;
    else if (!e && getenv("GRIM_EXPORT_KERNEL")) want = atoi(getenv("GRIM_EXPORT_KERNEL")) ? 1 : 0;
    if (want == 2) {
      char bdf[64] = {0};
      const char *why = nullptr;
      if (hipDeviceGetPCIBusId(bdf, (int)sizeof(bdf), device_id) != hipSuccess) bdf[0] = 0;
      c->sdma = grim_sdma_open(bdf[0] ? bdf : nullptr, device_id, &why);
      if (c->sdma) {
        // the engine by measurement (grim_sdma_pick: a chunk's worth of results down on every engine on offer, ~1 ms)
        const size_t probe = 1500000;
        void *hp = nullptr, *dp = nullptr;
        char report[256];
        uint32_t got = 0;
        if (hipHostMalloc(&hp, probe, hipHostMallocDefault) == hipSuccess && hipMalloc(&dp, probe) == hipSuccess &&
            hipMemset(dp, 0, probe) == hipSuccess && hipDeviceSynchronize() == hipSuccess)
          got = grim_sdma_pick(c->sdma, hp, dp, probe, report, sizeof(report));
        (void)hipGetLastError();
        if (dp) (void)hipFree(dp);
        if (hp) (void)hipHostFree(hp);
        if (getenv("GRIM_DEBUG_STREAM")) fprintf(stderr, "grim: SDMA engines for the downloads: %s -> 0x%x\n", got ? report : "none worked", got);
        if (!got) {
          why = "no SDMA engine completed a test copy";
          grim_sdma_close(c->sdma);
          c->sdma = nullptr;
        }
      }
      if (!c->sdma && e) fprintf(stderr, "grim: GRIM_EXPORT=sdma is not available (%s); using the export kernel\n", why ? why : "?");
      want = c->sdma ? 2 : 1;
    }
    c->export_mode = want;
  }
  return c;
}

extern "C" int grim_export_engine(grim_ctx *c) {
  if (!c) return -1;
  return c->export_mode == 2 ? (int)grim_sdma_engine(c->sdma) : c->export_mode == 1 ? 0 : -1;
}

static void batch_destroy(grim_batch *b);

extern "C" void grim_destroy(grim_ctx *c) {
  if (!c) return;
  hipSetDevice(c->device);
  for (grim_batch *b : c->spare) batch_destroy(b);
  c->spare.clear();
  if (c->scratch) hipFree(c->scratch);
  if (c->wctr) hipFree(c->wctr);
  if (c->sdma) grim_sdma_close(c->sdma);
  c->sdma = nullptr;
  hipStreamDestroy(c->stream);
  if (c->copy_stream) hipStreamDestroy(c->copy_stream);
  if (c->up_stream) hipStreamDestroy(c->up_stream);
  delete c;
}

extern "C" const char *grim_last_error(grim_ctx *c) {
  if (c) {  // a copy private to the calling thread: the context's text may be rewritten by another thread meanwhile
    std::lock_guard<std::mutex> lk(c->err_mu);
    g_err = c->err;
  }
  return g_err.c_str();
}

template <typename T>
static T *upload(grim_ctx *c, std::vector<void *> &bufs, const T *src, size_t n, uint64_t *bytes) {
  void *p = nullptr;
  size_t sz = (n ? n : 1) * sizeof(T);
  if (hipMalloc(&p, sz) != hipSuccess) return nullptr;
  bufs.push_back(p);
  if (n && src && hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
  if (bytes) *bytes += sz;
  return (T *)p;
}

static uint64_t host_mix64(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return x;
}

// Whether grim_graph_refresh may trust the descriptor's top-link rows (the conditions: grim_refresh.h), kept on the graph as a
// flag plus a reason text; the partial nodes go to the short-row or the long-row list on the way.  Reads the host arrays only.
static void refresh_check_rows(grim_graph *g, const grim_graph_desc *d) {
  const uint32_t V = d->n_nodes;
  auto no = [&](const std::string &why) {
    g->refreshable = false;
    g->refresh_why = why;
    g->rf_short.clear();
    g->rf_long.clear();
  };
  if (d->full_mask >= (1u << GRIM_MAXL)) return no("full_mask names a locus slot beyond GRIM_MAXL");
  if (d->n_a_nbr > 0xFFFFFFFFull) return no("more than 2^32 - 1 top links");
  const uint32_t n_a = (uint32_t)d->n_a_nbr;
  const uint32_t f_lo = d->lab_start[d->full_mask], f_hi = d->lab_start[d->full_mask + 1];
  if (f_lo > f_hi || f_hi > V) return no("lab_start does not lie inside the nodes");
  {  // the full nodes of lab_nodes are the full nodes, in node-id order
    uint32_t at = f_lo;
    for (uint32_t v = 0; v < V; ++v)
      if (d->node_mask[v] == d->full_mask) {
        if (at >= f_hi || d->lab_nodes[at] != v) return no("lab_nodes does not list the full nodes in node order");
        ++at;
      }
    if (at != f_hi) return no("lab_nodes does not list the full nodes in node order");
  }
  uint64_t slots[1u << GRIM_MAXL];  // the key fields of a label mask
  for (uint32_t m = 0; m < (1u << GRIM_MAXL); ++m) {
    slots[m] = 0;
    for (uint32_t q = 0; q < GRIM_MAXL; ++q)
      if ((m >> q) & 1u) slots[m] |= 0xFFFull << (GRIM_ABITS * q);
  }
  g->rf_short.clear();
  g->rf_long.clear();
  uint32_t pos = 0;
  for (uint32_t v = 0; v < V; ++v) {
    const uint32_t m = d->node_mask[v];
    if (m == d->full_mask) continue;
    const std::string node = "partial node " + std::to_string(v);
    if (m >= (1u << GRIM_MAXL)) return no(node + ": label mask beyond GRIM_MAXL");
    const uint32_t lo = d->a_start[v], hi = v + 1 < V ? d->a_start[v + 1] : n_a;
    if (lo != pos) return no(node + ": its top-link row does not begin where the row before it ends");
    if (hi <= lo) return no(node + ": empty top-link row");
    if (hi > n_a) return no(node + ": its top-link row ends beyond the links");
    for (uint32_t e = lo; e < hi; ++e) {
      const uint32_t r = d->a_nbr[e];
      if (r >= V || d->node_mask[r] != d->full_mask) return no(node + ": a top link that does not end at a full node");
      if ((d->node_key[r] & slots[m]) != d->node_key[v]) return no(node + ": a top link to a full haplotype that does not project onto it");
    }
    (hi - lo <= RF_SHORT_MAX ? g->rf_short : g->rf_long).push_back(v);
    pos = hi;
  }
  if (pos != n_a) return no("top links beyond the rows of the partial nodes");
  g->refreshable = true;
  g->refresh_why.clear();
  g->n_a_nbr = n_a;
  g->full_first = f_lo;
  g->n_full = f_hi - f_lo;
}

extern "C" grim_graph *grim_graph_upload(grim_ctx *c, const grim_graph_desc *d) {
  if (!c || !d) return nullptr;
  hipSetDevice(c->device);
  if (d->n_pops == 0 || d->n_pops > GRIM_MAXPOP) { set_err(c, "grim_graph_upload: population count out of range"); return nullptr; }
  if (d->n_loci == 0 || d->n_loci > GRIM_MAXL) { set_err(c, "grim_graph_upload: locus count out of range"); return nullptr; }
  if (d->n_nodes >= (1u << 23)) { set_err(c, "grim_graph_upload: more than 2^23 nodes"); return nullptr; }
  grim_graph *g = new grim_graph();
  g->ctx = c;
  g->bytes = 0;
  // exact-name index: open addressing over the 64-bit node keys
  // load <= 0.5; a graph whose index is far beyond the L2 anyway (every probe is a memory round trip, and the
  // rounds of linear probing are what a 64-lane wave waits for) gets load <= 0.25
  uint32_t cap = 64;
  static const int ht_factor = getenv("GRIM_HT_FACTOR") ? atoi(getenv("GRIM_HT_FACTOR")) : 0;
  while (cap < (uint64_t)(ht_factor > 1 ? ht_factor : (d->n_nodes > (1u << 18) ? 4 : 2)) * (uint64_t)d->n_nodes) cap <<= 1;
  std::vector<uint64_t> hk(cap, 0);
  std::vector<uint32_t> hv(cap, 0);
  bool unique_names = true;
  for (uint32_t i = 0; i < d->n_nodes; ++i) {
    uint64_t k = d->node_key[i];
    if (k == 0) { set_err(c, "grim_graph_upload: node with empty key"); delete g; return nullptr; }
    uint32_t h = (uint32_t)host_mix64(k) & (cap - 1);
    while (hk[h] != 0 && hk[h] != k) h = (h + 1) & (cap - 1);
    if (hk[h] == k) unique_names = false;
    hk[h] = k;  // a repeated name keeps the later row, like dict assignment (networkx_graph.py:53)
    hv[h] = i;
  }
  uint32_t max_deg = 0;
  for (uint32_t i = 0; i < d->n_nodes; ++i)
    if (d->a_start[i + 1] > d->a_start[i]) max_deg = std::max(max_deg, d->a_start[i + 1] - d->a_start[i]);
  uint32_t maxlab = 0;
  for (uint32_t m = 0; m < (1u << GRIM_MAXL); ++m) {
    uint32_t n = d->lab_start[m + 1] - d->lab_start[m];
    if (n > maxlab) maxlab = n;
  }
  g->max_label = maxlab;
  DevGraph &D = g->d;
  D.n_nodes = d->n_nodes;
  D.P = d->n_pops;
  D.n_loci = d->n_loci;
  D.full_mask = d->full_mask;
  D.ht_mask = cap - 1;
  D.n_conn = d->n_conn;
  D.node_key = upload(c, g->bufs, d->node_key, d->n_nodes, &g->bytes);
  D.node_mask = upload(c, g->bufs, d->node_mask, d->n_nodes, &g->bytes);
  D.freq = upload(c, g->bufs, d->freq, (size_t)d->n_nodes * d->n_pops, &g->bytes);
  D.a_start = upload(c, g->bufs, d->a_start, (size_t)d->n_nodes + 1, &g->bytes);
  D.a_nbr = upload(c, g->bufs, d->a_nbr, d->n_a_nbr, &g->bytes);
  D.b_conn = upload(c, g->bufs, d->b_conn, (size_t)d->n_nodes * GRIM_MAXL, &g->bytes);
  D.b_start = upload(c, g->bufs, d->b_start, (size_t)d->n_conn + 1, &g->bytes);
  D.b_nbr = upload(c, g->bufs, d->b_nbr, d->n_b_nbr, &g->bytes);
  D.lab_start = upload(c, g->bufs, d->lab_start, (1u << GRIM_MAXL) + 1, &g->bytes);
  D.lab_nodes = upload(c, g->bufs, d->lab_nodes, d->n_nodes, &g->bytes);
  {
    std::vector<uint64_t> lk(d->n_nodes);
    for (uint32_t i = 0; i < d->n_nodes; ++i) lk[i] = d->node_key[d->lab_nodes[i]];
    D.lab_key = upload(c, g->bufs, lk.data(), d->n_nodes, &g->bytes);
  }
  D.scan_ok = (unique_names && max_deg < (1u << 22) && d->n_pops <= 64) ? 1u : 0u;
  D.order_bad = d->label_order_bad;
  {
    std::vector<HtEnt> ht(cap);
    for (uint32_t i = 0; i < cap; ++i) {
      ht[i].key = hk[i];
      ht[i].val = hv[i];
      ht[i].pad = 0;
    }
    D.ht = upload(c, g->bufs, ht.data(), cap, &g->bytes);
  }
  {  // full-haplotype table
    uint32_t nfull = d->lab_start[d->full_mask + 1] - d->lab_start[d->full_mask];
    uint32_t fcap = 64;
    // load <= 1/8: every lane of a wave probes at once and the wave waits for its unluckiest lane, so the
    // number of linear-probing rounds matters more than the table's footprint (1 MB for the CAU graph);
    // measured on the bench kernel: 10.8 / 8.8 / 8.2 / 8.5 us at load 1/2, 1/4, 1/8, 1/16
    static const int fht_factor = getenv("GRIM_FHT_FACTOR") ? atoi(getenv("GRIM_FHT_FACTOR")) : 8;
    while (fcap < (uint64_t)(fht_factor > 1 ? fht_factor : 2) * (uint64_t)nfull) fcap <<= 1;
    std::vector<FullEnt> ft(fcap);
    memset(ft.data(), 0, sizeof(FullEnt) * fcap);
    for (uint32_t i = 0; i < d->n_nodes; ++i) {
      if (d->node_mask[i] != d->full_mask) continue;
      uint64_t k = d->node_key[i];
      uint32_t h = fht_hash(k) & (fcap - 1);
      while (ft[h].key != 0 && ft[h].key != k) h = (h + 1) & (fcap - 1);
      ft[h].key = k;
      ft[h].f0 = d->freq[(size_t)i * d->n_pops];
    }
    D.fht = upload(c, g->bufs, ft.data(), fcap, &g->bytes);
    D.fht_mask = fcap - 1;
  }
  if (!D.fht || !D.node_key || !D.node_mask || !D.freq || !D.a_start || !D.a_nbr || !D.b_conn || !D.b_start || !D.b_nbr ||
      !D.lab_start || !D.lab_nodes || !D.lab_key || !D.ht) {
    set_err(c, "grim_graph_upload: device allocation or copy failed");
    for (void *p : g->bufs) hipFree(p);
    delete g;
    return nullptr;
  }
  refresh_check_rows(g, d);
  return g;
}

static void refresh_state_free(RefreshState *rf);

extern "C" void grim_graph_free(grim_graph *g) {
  if (!g) return;
  hipSetDevice(g->ctx->device);
  refresh_state_free(g->rf);
  for (void *p : g->bufs) hipFree(p);
  delete g;
}

extern "C" uint64_t grim_graph_device_bytes(const grim_graph *g) { return g ? g->bytes : 0; }


static uint64_t align256(uint64_t x) { return (x + 255) & ~255ull; }

static thread_local int tl_device = -1;
static inline void use_device(int dev) {
  if (tl_device != dev) {
    hipSetDevice(dev);
    tl_device = dev;
  }
}

static int env_int(const char *name, int dflt) {
  const char *v = getenv(name);
  return v ? atoi(v) : dflt;
}

uint32_t engine_small_stride(const grim_params *p) { return GRIM_SMALL_ROWS_FIXED + (p->n_results < 16 ? p->n_results : 16); }

uint64_t engine_rows_per_subject(const grim_params *p, uint32_t P) {
  return 2ull * p->n_results + 2ull * (p->n_pop_results < (uint64_t)P * P ? p->n_pop_results : (uint64_t)P * P);
}

static bool dev_realloc(uint8_t *&ptr, uint64_t bytes) {
  if (ptr) hipFree(ptr);
  ptr = nullptr;
  return hipMalloc((void **)&ptr, bytes ? bytes : 256) == hipSuccess;
}
static bool pin_realloc(uint8_t *&ptr, uint64_t bytes) {
  if (ptr) hipHostFree(ptr);
  ptr = nullptr;
  return hipHostMalloc((void **)&ptr, bytes ? bytes : 256, hipHostMallocDefault) == hipSuccess;
}

static std::atomic<uint64_t> g_moved[2];

// lay the arenas out for a batch of at most pl.n_subj subjects and pl.tok_cap tokens; grows them when needed (what
// they held is lost then) and points the device arguments and the host-side pointers at the new places
static bool batch_plan(grim_batch *b, const EnginePlan &pl) {
  const uint64_t n = pl.n_subj ? pl.n_subj : 1;
  uint64_t o = 0;
  auto take = [&](uint64_t bytes) { uint64_t r = o; o = align256(o + bytes); return r; };
  const uint64_t o_state = take(8ull * GRIM_STATE_WORDS);
  // device tokenizer: line records and the chunk's text come first -- a run whose lines are all tokenised on the device
  // copies the arena only up to here
  const bool devtok = pl.text_cap != 0;
  const uint64_t o_lines = take(devtok ? sizeof(LineRec) * n : 0), o_text = take(devtok ? pl.text_cap + 64 : 0);
  const uint64_t o_subj = take(sizeof(grim_subject) * n);
  const uint64_t o_small = take(sizeof(SmallRec) * n);
  const uint64_t o_os = take(4 * n), o_om = take(4 * n), o_og = take(4 * n);
  const uint64_t o_tok = take(2 * ((pl.tok_cap ? pl.tok_cap : 1) + (devtok ? (uint64_t)TOK_LANES * n : 0)));  // device-written tokens behind the host's
  const uint64_t in_bytes = o;
  o = 0;
  const uint64_t small_waves = ((n + GRIM_WG / 32 - 1) / (GRIM_WG / 32)) * (GRIM_WG / 64);
  const uint64_t w_bail = take(4 * n), w_next = take(4 * n), w_ctr = take(4 * (4 * small_waves + 4));  // host- and device-tokenised launches
  const uint64_t w_mid = take(4 * n);
  const uint64_t w_dsmall = take(devtok ? sizeof(SmallRec) * n : 0);
  const uint64_t w_t1 = take(sizeof(TabWork) * 2 * n), w_t2 = take(sizeof(TabWork) * 2 * n);  // a subject queues at most two items
  const uint64_t work_bytes = o;
  o = 0;
  const uint64_t o_res = take(sizeof(grim_subject_result) * n);
  const uint64_t o_rows = take(sizeof(grim_row) * b->row_limit);
  const uint64_t out_bytes = o;
  bool ok = true;
  if (in_bytes > b->in_cap || !b->d_in) {
    const uint64_t want = in_bytes > b->in_cap ? in_bytes : b->in_cap;
    ok = ok && dev_realloc(b->d_in, want) && pin_realloc(b->h_in, want);
    b->in_cap = ok ? want : 0;
  }
  if (work_bytes > b->work_cap || !b->d_work) {
    const uint64_t want = work_bytes > b->work_cap ? work_bytes : b->work_cap;
    ok = ok && dev_realloc(b->d_work, want);
    b->work_cap = ok ? want : 0;
  }
  if (out_bytes > b->out_cap || !b->d_out) {
    const uint64_t want = out_bytes > b->out_cap ? out_bytes : b->out_cap;
    ok = ok && dev_realloc(b->d_out, want);
    b->out_cap = ok ? want : 0;
  }
  if (!ok) return false;
  b->plan = pl;
  b->off_tok = o_tok;
  b->off_rows = o_rows;
  DevArgs &A = b->a;
  A.counters = (unsigned long long *)(b->d_in + o_state);
  A.queue = (uint32_t *)(A.counters + GRIM_NCTR);
  A.row_head = A.queue + GRIM_Q_ROWS;
  A.next_count = A.queue + GRIM_Q_NEXT;
  A.subj = (const grim_subject *)(b->d_in + o_subj);
  b->d_small = (SmallRec *)(b->d_in + o_small);
  b->d_lines = devtok ? (LineRec *)(b->d_in + o_lines) : nullptr;
  b->d_text = devtok ? b->d_in + o_text : nullptr;
  b->d_dsmall = devtok ? (SmallRec *)(b->d_work + w_dsmall) : nullptr;
  b->off_subj = o_subj;
  b->h.lines = devtok ? (LineRec *)(b->h_in + o_lines) : nullptr;
  b->h.text = devtok ? b->h_in + o_text : nullptr;
  b->d_os = (uint32_t *)(b->d_in + o_os);
  b->d_om = (uint32_t *)(b->d_in + o_om);
  A.order = (const uint32_t *)(b->d_in + o_og);
  A.tok = (const uint16_t *)(b->d_in + o_tok);
  A.bail_list = (uint32_t *)(b->d_work + w_bail);
  A.next_list = (uint32_t *)(b->d_work + w_next);
  {
    // test switch: everything the mid-size kernel takes goes to the general kernel.  Read at every layout, like the other
    // switches: a process that runs with it on and off (the tests do) must get what it asked for each time.
    const int no_mid = env_int("GRIM_NO_MID", 0);
    A.mid_list = no_mid ? nullptr : (uint32_t *)(b->d_work + w_mid);
  }
  A.small_ctr = (uint32_t *)(b->d_work + w_ctr);
  A.t1_list = (TabWork *)(b->d_work + w_t1);
  A.t2_list = (TabWork *)(b->d_work + w_t2);
  A.res = (grim_subject_result *)(b->d_out + o_res);
  A.rows = (grim_row *)(b->d_out + o_rows);
  A.row_cap = (uint32_t)b->row_limit;
  A.priors = b->d_priors;
  A.next_cap = (uint32_t)n;
  b->h.subj = (grim_subject *)(b->h_in + o_subj);
  b->h.small = (SmallRec *)(b->h_in + o_small);
  b->h.order_s = (uint32_t *)(b->h_in + o_os);
  b->h.order_m = (uint32_t *)(b->h_in + o_om);
  b->h.order_g = (uint32_t *)(b->h_in + o_og);
  b->h.tok = (uint16_t *)(b->h_in + o_tok);
  b->h.res = (grim_subject_result *)b->h_out;            // set for real by the first fetch (the landing area grows on demand)
  b->h.rows = (grim_row *)(b->h_out ? b->h_out + o_rows : nullptr);
  return true;
}

// parameters, graph and the per-workgroup scratch layout of a batch (everything that is not a buffer)
static void batch_init_params(grim_batch *b, const grim_graph *g, const grim_params *p) {
  b->g = g;
  DevArgs &A = b->a;
  A.g = g->d;
  A.prm = *p;
  const uint32_t P = g->d.P;
  b->small_stride = engine_small_stride(p);
  // per-workgroup scratch layout (bytes per slot); the block itself belongs to the context and is bound at run time
  A.pair_cap = GRIM_MAXPH * p->top_n * p->top_n;
  uint32_t tab = 64;
  while (tab < 2 * A.pair_cap) tab <<= 1;
  A.tab_cap = tab;
  A.bset_cap = g->max_label;
  SlotLayout &L = A.lay;
  uint64_t o = 0;
  auto take = [&](uint64_t n) { uint64_t r = o; o = align256(o + n); return r; };
  L.Tp = take(8ull * GRIM_SIDES * GRIM_TOPCAP);
  L.Tm = take(8ull * GRIM_SIDES * GRIM_TOPCAP);
  L.Te = take(4ull * GRIM_SIDES * GRIM_TOPCAP);
  L.k0 = take(8ull * tab);
  L.k1 = take(8ull * tab);
  L.tmin = take(4ull * tab);
  L.tgid = take(4ull * tab);
  L.Useq = take(4ull * A.pair_cap);
  L.Uprob = take(8ull * A.pair_cap);
  L.Uslot = take(4ull * A.pair_cap);
  L.ska = take(8ull * A.pair_cap);
  L.skb = take(8ull * A.pair_cap);
  L.sva = take(4ull * A.pair_cap);
  L.svb = take(4ull * A.pair_cap);
  L.gsum = take(8ull * A.pair_cap);
  L.ghead = take(4ull * A.pair_cap);
  L.gstart = take(4ull * (A.pair_cap + 1));
  L.gcnt = take(4ull * (A.pair_cap > P * P ? A.pair_cap : P * P));
  L.qsum = take(8ull * P * P);
  L.qfirst = take(4ull * P * P);
  L.bset = take(4ull * GRIM_NWAVE * GRIM_MAXL * (uint64_t)A.bset_cap);
  L.comp = take(8ull * GRIM_COMP_CAP);
  {
    uint32_t pc = 64;
    while (pc < 2 * A.bset_cap) pc <<= 1;
    A.proj_cap = pc;
  }
  L.proj_k = take(8ull * GRIM_NWAVE * A.proj_cap);
  L.proj_p = take(4ull * GRIM_NWAVE * A.proj_cap);
  L.rtok = take(2ull * GRIM_RTOK_CAP);
  L.save = take(p->save_mode ? 8ull * GRIM_NWAVE * 2 * GRIM_SAVE_CAP * (P + 1) : 0);
  L.stride = align256(o);
  b->timing = env_int("GRIM_TIMING", 0) != 0;
  A.flags = (env_int("GRIM_TABLES_HBM", 0) ? GRIM_F_TABLES_HBM : 0u) | (env_int("GRIM_NO_NODUP", 0) ? GRIM_F_NO_NODUP : 0u) |
            (env_int("GRIM_NO_SIDEMASK", 0) ? GRIM_F_NO_SIDEMASK : 0u);
  memset(b->acc_ms, 0, sizeof(b->acc_ms));
  b->n_timed = 0;
  b->n_subj = b->n_small = b->n_medium = b->n_general = 0;
  b->rows_used = 0;
}

grim_batch *engine_batch_create(grim_ctx *c, const grim_graph *g, const grim_params *p, uint64_t row_limit, const EnginePlan *plan) {
  if (!c || !g || !p || !plan) return nullptr;
  use_device(c->device);
  if (p->top_n == 0 || p->top_n > GRIM_TOPCAP) { set_err(c, "grim_batch_upload: max_haplotypes_number_in_phase must be 1..128"); return nullptr; }
  if (p->n_ladder < 0 || p->n_ladder > GRIM_MAXLADDER) { set_err(c, "grim_batch_upload: epsilon ladder too long"); return nullptr; }
  if (row_limit > 0x7FFFFFF0ull) row_limit = 0x7FFFFFF0ull;
  if (row_limit < 64) row_limit = 64;
  grim_batch *b = nullptr;
  if (!c->spare.empty()) {  // a batch some earlier stream handed back: its arenas and events are reused
    b = c->spare.back();
    c->spare.pop_back();
    if (b->d_priors) hipFree(b->d_priors);  // sized in P x P units of the graph it served
    if (b->h_priors) hipHostFree(b->h_priors);
    b->d_priors = b->h_priors = nullptr;
    b->priors_cap = b->priors_up = 0;
  } else {
    b = new grim_batch();
    memset((void *)b, 0, sizeof(*b));
    b->ctx = c;
    bool ok = true;
    if (hipHostMalloc((void **)&b->hstate, 8 * GRIM_STATE_WORDS) != hipSuccess) {
      b->hstate = nullptr;
      ok = false;
    }
    for (auto &pair : b->ev)
      for (hipEvent_t &e : pair) ok = ok && hipEventCreate(&e) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&b->ev_done, hipEventDisableTiming | hipEventReleaseToSystem) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&b->ev_copy, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&b->ev_up, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
      set_err(c, "grim_batch: device or pinned-host allocation failed");
      batch_destroy(b);
      return nullptr;
    }
  }
  b->row_limit = row_limit;
  batch_init_params(b, g, p);
  if (!batch_plan(b, *plan)) {
    set_err(c, "grim_batch: device or pinned-host allocation failed");
    batch_destroy(b);
    return nullptr;
  }
  return b;
}

// hand a capacity batch back to its context for the next stream (at most 8 are kept)
void engine_batch_recycle(grim_batch *b) {
  if (!b) return;
  grim_ctx *c = b->ctx;
  use_device(c->device);
  hipStreamSynchronize(c->stream);
  if (b->gexec) {
    hipGraphExecDestroy(b->gexec);
    b->gexec = nullptr;
  }
  b->graph_state = 0;
  if (c->spare.size() >= 8) {
    batch_destroy(b);
    return;
  }
  c->spare.push_back(b);
}

int engine_batch_plan(grim_batch *b, const EnginePlan *plan) {
  if (!b || !plan) return -1;
  use_device(b->ctx->device);
  if (!batch_plan(b, *plan)) {
    set_err(b->ctx, "grim_batch: device or pinned-host allocation failed while growing a batch");
    return -1;
  }
  return 0;
}

void engine_set_error(grim_ctx *c, const char *msg) { set_err(c, msg); }
const EngineHost *engine_batch_host(grim_batch *b) { return b ? &b->h : nullptr; }
uint64_t engine_bytes_moved(const grim_batch *, int dir) { return g_moved[dir ? 1 : 0]; }

struct grim_devdict {
  grim_ctx *ctx;
  DevDict d;
  std::vector<void *> bufs;
};

static void pack_name(const char *p, size_t n, uint32_t (&w)[6]) {
  for (int i = 0; i < 6; ++i) w[i] = 0;
  for (size_t k = 0; k < n && k < GRIM_TOKNAME; ++k) w[k >> 2] |= (uint32_t)(uint8_t)p[k] << (24 - 8 * (k & 3));
}

extern "C" uint32_t grim_tokname_hash(const char *name, uint32_t len) {
  if (!name || len > GRIM_TOKNAME) return 0;
  uint32_t w[6];
  pack_name(name, len, w);
  return tokname_hash(w, len);
}

grim_devdict *engine_devdict_create(grim_ctx *c, const DictSnap *snap) {
  if (!c || !snap) return nullptr;
  use_device(c->device);
  grim_devdict *dd = new grim_devdict();
  dd->ctx = c;
  memset(&dd->d, 0, sizeof(dd->d));
  dd->d.n_loci = snap->n_loci;
  for (uint32_t s = 0; s < GRIM_MAXL; ++s) dd->d.locus_len[s] = 0xFFFFFFFFu;  // matches no name
  for (const DictSnap::Locus &L : snap->loci) {
    if (L.slot >= GRIM_MAXL || L.name.empty() || L.name.size() > 8) continue;  // (longer locus names: host tokenizer)
    uint64_t v = 0;
    for (size_t k = 0; k < L.name.size(); ++k) v |= (uint64_t)(uint8_t)L.name[k] << (56 - 8 * k);
    dd->d.locus[L.slot] = v;
    dd->d.locus_len[L.slot] = (uint32_t)L.name.size();
  }
  bool ok = true;
  for (uint32_t s = 0; s < snap->n_loci && s < GRIM_MAXL && ok; ++s) {
    const uint32_t cnt = snap->base[s];
    uint32_t cap = 16;
    while (cap < 4ull * cnt) cap <<= 1;  // load <= 1/4: a wave waits for its unluckiest lane
    std::vector<DictEnt> tab(cap);
    memset(tab.data(), 0, sizeof(DictEnt) * cap);
    for (uint32_t id = 0; id < cnt; ++id) {
      const sv nm = snap->name(s, id);
      if (nm.empty() || nm.size() > GRIM_TOKNAME) continue;  // never found on the device: such a line goes to the host tokenizer
      DictEnt e;
      pack_name(nm.data(), nm.size(), e.w);
      e.hash = tokname_hash(e.w, (uint32_t)nm.size());
      e.meta = 0x80000000u | ((uint32_t)nm.size() << 16) | (id & 0xFFFFu);
      uint32_t k = e.hash & (cap - 1);
      while (tab[k].meta >> 31) k = (k + 1) & (cap - 1);
      tab[k] = e;
    }
    DictEnt *dt = upload(c, dd->bufs, tab.data(), cap, nullptr);
    ok = dt != nullptr;
    dd->d.tab[s] = dt;
    dd->d.mask[s] = cap - 1;
  }
  if (!ok) {
    set_err(c, "engine_devdict_create: device allocation or copy failed");
    engine_devdict_free(dd);
    return nullptr;
  }
  return dd;
}

void engine_devdict_free(grim_devdict *d) {
  if (!d) return;
  use_device(d->ctx->device);
  for (void *p : d->bufs) hipFree(p);
  delete d;
}

void engine_batch_set_dict(grim_batch *b, const grim_devdict *d) {
  if (b) b->dict = d;
}

uint32_t engine_batch_irregular(const grim_batch *b) { return b ? b->n_irregular : 0; }
uint32_t engine_graph_order_bad(const grim_graph *g) { return g ? g->d.order_bad : 0; }

// After grim_batch_run returned -2: when the PAIR POOL was what ran out and the demand fits `max_records`, the next
// engine_batch_load sizes the pool for it (returns 1: load and run the same subjects again); 0: something else
// overflowed, or the demand is beyond the limit -- split the batch.
int engine_batch_grow_pool(grim_batch *b, uint64_t max_records) {
  if (!b || b->pool_asked <= b->a.ppool_cap) return 0;
  uint64_t want = b->pool_asked + b->pool_asked / 8 + 4096;
  if (want > max_records || want > 0x7FFFFFF0ull) return 0;
  if (want <= b->pool_want) return 0;  // already tried with that much
  b->pool_want = want;
  return 1;
}

// The ROW pool of a batch whose run ran out of rows (not of pairs, buckets or work units): twice as many, up to max_rows.
// 1: grown -- the caller runs the same subjects again (their inputs are still in the pinned arena); 0: not the row pool, or
// already at the bound (the caller halves the range).  engine_batch_hint_rows: the same lesson for a sibling batch of the
// stream before its next load.  Only ever called between runs of the batch.
static int batch_set_rows(grim_batch *b, uint64_t rows) {
  const uint64_t old = b->row_limit;
  b->row_limit = rows;
  const EnginePlan pl = b->plan;
  if (!batch_plan(b, pl)) {
    (void)hipGetLastError();
    b->row_limit = old;
    if (!batch_plan(b, pl)) set_err(b->ctx, "grim_batch: device allocation failed while growing the row pool");
    return 0;
  }
  return 1;
}
int engine_batch_grow_rows(grim_batch *b, uint64_t max_rows) {
  if (!b || b->rows_used < b->a.row_cap || b->row_limit >= max_rows) return 0;
  use_device(b->ctx->device);
  uint64_t want = b->row_limit * 2;
  if (want > max_rows) want = max_rows;
  if (want > 0x7FFFFFF0ull) want = 0x7FFFFFF0ull;
  if (want <= b->row_limit) return 0;
  return batch_set_rows(b, want);
}
uint64_t engine_batch_row_limit(const grim_batch *b) { return b ? b->row_limit : 0; }
void engine_batch_hint_rows(grim_batch *b, uint64_t rows) {
  if (!b || rows <= b->row_limit) return;
  use_device(b->ctx->device);
  (void)batch_set_rows(b, rows);
}

// what a batch learnt about its pair pool (0: the default sizing was enough) / the same lesson for a sibling batch of the
// same stream, which will see the same kind of chunks: its next load sizes the pool accordingly instead of finding out
uint64_t engine_batch_pool_want(const grim_batch *b) { return b ? b->pool_want : 0; }
void engine_batch_hint_pool(grim_batch *b, uint64_t records) {
  if (b && records > b->pool_want) b->pool_want = records;
}

int engine_batch_load(grim_batch *b, const EngineLoad *ld) {
  if (!b || !ld) return -1;
  grim_ctx *c = b->ctx;
  use_device(c->device);
  DevArgs &A = b->a;
  b->ran_ok = false;
  if (ld->n_subj > b->plan.n_subj || ld->tok_used > b->plan.tok_cap) {
    set_err(c, "engine_batch_load: beyond what the batch was planned for");
    return -1;
  }
  hipStream_t st = c->stream;
  const uint32_t P = b->g->d.P;
  const uint64_t PP = (uint64_t)P * P;
  // prior matrices + one all-ones matrix for Plan B's second level (impute.py:1696-1700): only when the set changed
  if (ld->priors && (ld->n_priors != b->priors_up || !b->d_priors)) {
    if (ld->n_priors + 1 > b->priors_cap || !b->d_priors) {
      const uint32_t want = ld->n_priors + 1 > 2 * b->priors_cap ? ld->n_priors + 1 : 2 * b->priors_cap;
      if (b->d_priors) hipFree(b->d_priors);
      if (b->h_priors) hipHostFree(b->h_priors);
      b->d_priors = b->h_priors = nullptr;
      if (hipMalloc((void **)&b->d_priors, 8 * (uint64_t)want * PP) != hipSuccess ||
          hipHostMalloc((void **)&b->h_priors, 8 * (uint64_t)want * PP, hipHostMallocDefault) != hipSuccess) {
        set_err(c, "engine_batch_load: allocation of the prior matrices failed");
        return -1;
      }
      b->priors_cap = want;
    }
    if (ld->n_priors) memcpy(b->h_priors, ld->priors, 8 * (uint64_t)ld->n_priors * PP);
    for (uint64_t k = 0; k < PP; ++k) b->h_priors[(uint64_t)ld->n_priors * PP + k] = 1.0;
    HIPCHK(hipMemcpyAsync(b->d_priors, b->h_priors, 8 * ((uint64_t)ld->n_priors + 1) * PP, hipMemcpyHostToDevice, st), c, -1);
    g_moved[0] += 8 * ((uint64_t)ld->n_priors + 1) * PP;
    b->priors_up = ld->n_priors;
  }
  A.priors = b->d_priors;
  A.ones_prior = b->priors_up;
  if (ld->dev_hi > ld->dev_lo && (!b->dict || !b->d_lines || ld->text_bytes > b->plan.text_cap || ld->dev_hi > ld->n_subj)) {
    set_err(c, "engine_batch_load: the batch was not planned for the device tokenizer");
    return -1;
  }
  b->dev_lo = ld->dev_lo;
  b->dev_hi = ld->dev_hi;
  b->n_dev_lines = ld->dev_hi > ld->dev_lo ? ld->dev_hi - ld->dev_lo : 0;  // record slots of the device tokenizer: one per line of the range
  b->n_irregular = 0;
  b->n_subj = ld->n_subj;
  b->n_small = ld->n_small;
  b->n_medium = ld->n_medium;
  b->n_general = ld->n_general;
  b->last_load = *ld;
  b->last_load.priors = nullptr;
  A.n_medium = ld->n_medium;
  A.n_work = ld->n_general;
  // the run state travels with the input: clean counters and work heads, rows of the half-wave kernel's fixed region taken
  unsigned long long *hs = (unsigned long long *)b->h_in;
  memset(hs, 0, 8 * GRIM_STATE_WORDS);
  // (rows are bump-allocated from 0; the half-wave kernel's staging region is the top of the pool)
  {
    const uint64_t staged = ((uint64_t)b->n_small + b->n_dev_lines) * b->small_stride;
    A.row_cap = (uint32_t)(b->row_limit - (staged <= b->row_limit ? staged : 0));
  }
  // everything up to the last token in use; a load without host-tokenised subjects ends with the chunk's text
  const bool host_subjects = ld->n_small + ld->n_medium + ld->n_general > 0;
  const uint64_t bytes = (!host_subjects && b->n_dev_lines) ? b->off_subj : b->off_tok + 2 * ld->tok_used;
  // the input goes up on the upload stream -- the copy of THIS batch overlaps the kernels of the batch before it -- and the
  // launch stream waits for it (the batch's buffers are its own: nothing else orders the two streams)
  HIPCHK(hipMemcpyAsync(b->d_in, b->h_in, bytes, hipMemcpyHostToDevice, c->up_stream), c, -1);
  HIPCHK(hipEventRecord(b->ev_up, c->up_stream), c, -1);
  b->up_pending = true;  // engine_batch_enqueue orders the launch stream behind it (or finds it done)
  g_moved[0] += bytes;
  {
    // arena of the table kernels: a pair pool of 512 records per subject that can reach them directly, a few for the
    // half-wave kernel's subjects (they get there through Plan B only), and the arrays of the three-kernel path sized by
    // it; running out of any of them is reported like a row-pool overflow
    uint64_t R = (1ull << 20) + 512ull * ((uint64_t)ld->n_medium + ld->n_general) + 16ull * ld->n_small;
    // subjects the host classified as heavy (high ambiguity) can accept tens of thousands of pairs each: half a subject's
    // worst case for the first 256 of them, so that a small batch of heavy subjects does not need a second run
    R += (uint64_t)(ld->n_general < 256u ? ld->n_general : 256u) * (A.pair_cap / 2);
    const char *env_pool = getenv("GRIM_PAIR_POOL");  // tests: start small so that the grow-and-run-again path is taken
    if (env_pool && atol(env_pool) > 0) R = (uint64_t)atol(env_pool);
    if (b->pool_want > R) R = b->pool_want;  // an earlier run of this batch ran out: it said how much it needed
    if (R > 0x7FFFFFF0ull) R = 0x7FFFFFF0ull;
    const uint64_t items = 2ull * ld->n_subj < R / 256 + 1 ? 2ull * ld->n_subj : R / 256 + 1;  // bigger work items at most
    // buckets: a table starts with fewer than n / 64 and the split kernels may re-deal it into twice as many up to three
    // times (n / 8 at most), two tables
    uint64_t cap_b = R / 4 + (items + 1) * ((uint64_t)P * P + 4), cap_u = R / 4 + items * 64 + 1024;
    if (cap_b > R + 4096) cap_b = R + 4096;
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { uint64_t r = o; o = align256(o + bytes); return r; };
    const uint64_t o_pool = take(sizeof(PairRec) * R), o_aux = take(sizeof(TabAux) * 2 * (uint64_t)(ld->n_subj ? ld->n_subj : 1)),
                   o_boff = take(4 * cap_b), o_cell = take(sizeof(CellRec) * cap_b), o_units = take(sizeof(TabUnit) * cap_u),
                   o_sort = take(4 * 3 * R), o_grp = take(sizeof(GrpRec) * 2 * R), o_prob = take(8 * R);
    if (o > b->pool_bytes || !b->d_pool) {
      HIPCHK(hipStreamSynchronize(st), c, -1);
      if (b->d_pool) hipFree(b->d_pool);
      b->d_pool = nullptr;
      b->pool_bytes = 0;
      if (hipMalloc((void **)&b->d_pool, o) != hipSuccess) {
        (void)hipGetLastError();
        set_err(c, "engine_batch_load: cannot allocate " + std::to_string((unsigned long long)(o >> 20)) + " MiB for the table kernels");
        return -1;
      }
      b->pool_bytes = o;
    }
    b->pool_cap = R;
    A.ppool = (PairRec *)(b->d_pool + o_pool);
    A.ppool_cap = (uint32_t)R;
    A.taux = (TabAux *)(b->d_pool + o_aux);
    A.tboff = (uint32_t *)(b->d_pool + o_boff);
    A.tcell = (CellRec *)(b->d_pool + o_cell);
    A.tboff_cap = (uint32_t)cap_b;
    A.tunits = (TabUnit *)(b->d_pool + o_units);
    A.tunits_cap = (uint32_t)cap_u;
    A.tstride = (uint32_t)R;
    A.psort = (uint32_t *)(b->d_pool + o_sort);
    A.pgrp = (GrpRec *)(b->d_pool + o_grp);
    A.pprob = (double *)(b->d_pool + o_prob);
  }
  const uint32_t per_block = GRIM_WG / 32;
  b->n_host_small_waves = ((b->n_small + per_block - 1) / per_block) * (GRIM_WG / 64);
  b->n_small_waves = b->n_host_small_waves + ((b->n_dev_lines + per_block - 1) / per_block) * (GRIM_WG / 64);
  uint32_t slots = (uint32_t)c->n_cu * GRIM_WG_PER_CU;
  static const int env_slots = env_int("GRIM_SLOTS", 0);
  if (env_slots > 0) slots = (uint32_t)env_slots;
  if (slots > ld->n_subj) slots = ld->n_subj;
  if (slots == 0) slots = 1;
  // (a device-tokenised subject can only ever reach the Plan-B kernel: it is the half-wave kernel's)
  b->n_slots = slots;
  b->scratch_need = (uint64_t)A.lay.stride * slots;
  if (b->gexec) {
    hipGraphExecDestroy(b->gexec);
    b->gexec = nullptr;
  }
  b->graph_state = 0;
  b->rows_used = 0;
  b->small_ctr_pending = false;
  return 0;
}

extern "C" grim_batch *grim_batch_upload(grim_ctx *c, const grim_graph *g, const grim_params *p, const grim_batch_desc *d) {
  if (!c || !g || !p || !d) return nullptr;
  use_device(c->device);
  const uint32_t P = g->d.P;
  // subject classes
  ClassRule rule;
  // (a loci_map that is not alphabetical -- DevGraph::order_bad -- goes through the general kernel only: its look-ups are
  // the ones that reproduce the reference's misses)
  rule.small_ok = (P == 1) && p->opt_threshold > 1 && !getenv("GRIM_NO_SMALL") && g->d.order_bad == 0;
  rule.medium_ok = !getenv("GRIM_NO_MEDIUM") && g->d.order_bad == 0;
  rule.medium_max_cost = getenv("GRIM_MEDIUM_MAXCOST") ? atof(getenv("GRIM_MEDIUM_MAXCOST")) : 0.0;
  rule.graph_loci = g->d.n_loci;
  rule.opt_threshold = p->opt_threshold;
  std::vector<uint32_t> os, om, og;
  for (uint32_t i = 0; i < d->n_subjects; ++i) {
    const int cls = grim_classify(rule, d->subjects[i]);
    (cls == GRIM_CLS_SMALL ? os : cls == GRIM_CLS_MEDIUM ? om : og).push_back(i);
  }
  {  // longest-processing-time-first; stable so equal-cost subjects stay in input order
    std::vector<double> cs(d->n_subjects);
    for (uint32_t i : og) cs[i] = grim_cost(d->subjects[i]);
    std::stable_sort(og.begin(), og.end(), [&](uint32_t a, uint32_t b2) { return cs[a] > cs[b2]; });
  }
  // rows: enough for every subject to fill all four tables (+ the gaps of the one-wave kernel's private row blocks:
  // at most as much again as its subjects use, plus one unfinished GRIM_ROW_GRAB block per resident wave)
  const uint64_t per = engine_rows_per_subject(p, P);
  uint64_t want = per * d->n_subjects + per * om.size() + 2ull * engine_small_stride(p) * os.size() + 1024 +
                  (uint64_t)GRIM_ROW_GRAB * c->n_cu * 32;
  const char *env_rows = getenv("GRIM_ROW_CAP");
  if (env_rows) want = strtoull(env_rows, nullptr, 10);
  if (want > 0x7FFFFFF0ull) want = 0x7FFFFFF0ull;
  EnginePlan plan{d->n_subjects ? d->n_subjects : 1u, d->n_tokens ? d->n_tokens : 1ull};
  grim_batch *b = engine_batch_create(c, g, p, want, &plan);
  if (!b) return nullptr;
  if (d->n_subjects) memcpy(b->h.subj, d->subjects, sizeof(grim_subject) * (size_t)d->n_subjects);
  if (d->n_tokens) memcpy(b->h.tok, d->tokens, 2 * (size_t)d->n_tokens);
  for (size_t k = 0; k < os.size(); ++k) {
    const grim_subject &sj = d->subjects[os[k]];
    grim_small_rec(sj, d->tokens + sj.tok_off, os[k], b->h.small[k]);
    b->h.order_s[k] = os[k];
  }
  if (!om.empty()) memcpy(b->h.order_m, om.data(), 4 * om.size());
  if (!og.empty()) memcpy(b->h.order_g, og.data(), 4 * og.size());
  std::vector<double> one_prior;
  const double *pri = d->priors;
  if (!d->n_priors) {  // no matrix given: subjects index matrix 0
    one_prior.assign((size_t)P * P, 1.0);
    pri = one_prior.data();
  }
  EngineLoad ld{d->n_subjects, (uint32_t)os.size(), (uint32_t)om.size(), (uint32_t)og.size(), d->n_tokens,
                d->n_priors ? d->n_priors : 1u, pri};
  const int lrc = engine_batch_load(b, &ld);  // sets the error text itself
  if (lrc != 0 || hipStreamSynchronize(c->stream) != hipSuccess) {
    if (lrc == 0) set_err(c, "grim_batch_upload: copy failed");
    grim_batch_free(b);
    return nullptr;
  }
  return b;
}

// the context's scratch block: bound when a run's kernels are launched (c->run_mu held).  Kernels use it only while they
// run -- nothing in it outlives a kernel -- and a context's kernels share one stream, so batches in flight at the same
// time may share the block; it is only ever replaced by a bigger one, after the stream has drained.
static int bind_scratch(grim_batch *b) {
  grim_ctx *c = b->ctx;
  if (b->scratch_need > c->scratch_bytes) {
    if (c->scratch) {
      hipStreamSynchronize(c->stream);
      hipFree(c->scratch);
    }
    c->scratch = nullptr;
    c->scratch_bytes = 0;
    if (hipMalloc(&c->scratch, b->scratch_need) != hipSuccess) {
      (void)hipGetLastError();
      set_err(c, "grim_batch_run: cannot allocate " + std::to_string((unsigned long long)(b->scratch_need >> 20)) + " MiB of scratch");
      return -1;
    }
    c->scratch_bytes = b->scratch_need;
  }
  b->a.scratch = (uint8_t *)c->scratch;
  b->a.wctr = c->wctr;
  return 0;
}

// Every kernel of a run is launched through here, on the context's stream.  Timing mode (b->timing) brackets the launch
// with its phase's events (hipExtLaunchKernelGGL) and notes the phase for engine_batch_wait to read back; otherwise, and
// for a kernel outside every timed interval (PH_NONE), it is a plain launch.  start/stop: an interval that spans several
// kernels gives its first one the start event only and its last one the stop event only.
template <typename... P, typename... Q>
static void launch_span(grim_batch *b, Phase ph, bool start, bool stop, void (*kernel)(P...), dim3 grid, dim3 block, Q &&...args) {
  if (b->timing && ph != PH_NONE) {
    b->launched |= 1u << ph;
    hipExtLaunchKernelGGL(kernel, grid, block, 0, b->ctx->stream, start ? b->ev[ph][0] : nullptr, stop ? b->ev[ph][1] : nullptr, 0,
                          static_cast<P>(args)...);
  } else {
    hipLaunchKernelGGL(kernel, grid, block, 0, b->ctx->stream, static_cast<P>(args)...);
  }
}
template <typename... P, typename... Q>
static void launch(grim_batch *b, Phase ph, void (*kernel)(P...), dim3 grid, dim3 block, Q &&...args) {
  launch_span(b, ph, true, true, kernel, grid, block, args...);
}

// The table kernels: the one-wave kernel for work items of up to GRIM_TAB_T1_MAX pairs; split, bucket and merge kernel
// for the rest.  All read their list lengths on the device (the kernels before them in the stream wrote them) and come
// back at once when there is nothing to do.  Timing mode: one interval around them all.
static void enqueue_tables(grim_batch *b) {
  grim_ctx *c = b->ctx;
  DevArgs &A = b->a;
  const uint32_t cand = b->n_subj;
  uint32_t g1 = (uint32_t)c->n_cu * 14u, g2 = (uint32_t)c->n_cu * GRIM_TAB_WG_PER_CU;
  if (g1 > cand) g1 = cand;
  if (g2 > b->n_slots) g2 = b->n_slots;  // one scratch slot per workgroup
  if (g1 == 0) g1 = 1;
  if (g2 == 0) g2 = 1;
  // resident waves of the bucket kernel (registers or LDS, whichever binds): its units are dealt round robin over the grid, a
  // block that had to wait for a free slot would run its share after everybody else's
  static int bucket_per_cu = 0;
  if (bucket_per_cu == 0) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, grim_tables_bucket_kernel, 64, 0) != hipSuccess || nb <= 0) {
      (void)hipGetLastError();
      nb = 8;
    }
    bucket_per_cu = nb > 32 ? 32 : nb;
  }
  const uint32_t g3 = (uint32_t)c->n_cu * (uint32_t)bucket_per_cu;
  // items of up to TW_MAXN pairs: a wave each, twelve split waves (LDS) / sixteen merge waves (registers) per CU
  uint32_t g4 = (uint32_t)c->n_cu * (160u * 1024u / (uint32_t)sizeof(SplitWave)), g5 = (uint32_t)c->n_cu * 16u;
  if (g4 > cand) g4 = cand;
  if (g5 > cand) g5 = cand;
  if (g4 == 0) g4 = 1;
  if (g5 == 0) g5 = 1;
  (void)hipMemsetAsync(c->wctr, 0, 4 * GRIM_WCTR_WORDS, c->stream);
  launch_span(b, PH_TABLES, true, false, grim_tables_wave_kernel, dim3(g1), dim3(64), A);
  launch(b, PH_NONE, grim_tables_split_wave_kernel, dim3(g4), dim3(64), A);
  launch(b, PH_NONE, grim_tables_split_kernel, dim3(g2), dim3(GRIM_WG), A);
  launch(b, PH_NONE, grim_tables_bucket_kernel, dim3(g3), dim3(64), A);
  launch(b, PH_NONE, grim_tables_merge_wave_kernel, dim3(g5), dim3(64), A);
  launch_span(b, PH_TABLES, false, true, grim_tables_merge_kernel, dim3(g2), dim3(GRIM_WG), A);
}

// The half-wave kernel over the `n` records at `recs`, and the compaction of its rows out of their fixed places in the staging
// region from `stage` on.  order: the records' subjects (host-tokenised), or nullptr (device-tokenised: one record slot per
// line).  Ak: the kernel's arguments (its slice of the per-wave counters).
static void enqueue_half_wave(grim_batch *b, bool timed, const DevArgs &Ak, const SmallRec *recs, const uint32_t *order, uint32_t n, uint32_t stage) {
  const uint32_t per_block = GRIM_WG / 32;
  launch(b, timed ? PH_HALF_WAVE : PH_NONE, grim_plan_a_small_kernel, dim3((n + per_block - 1) / per_block), dim3(GRIM_WG), Ak, recs, n, stage,
         b->small_stride);
  launch(b, timed ? PH_COMPACT : PH_NONE, grim_small_compact_kernel, dim3((n + 63) / 64), dim3(64), b->a, order, order ? nullptr : recs, n, stage,
         b->small_stride);
}

// Stage 1 of a run: half-wave kernel, one-wave kernel, general plan-A kernel, finish kernel (state to the pinned
// host copy, device copy reset for the next run).  Default: launched directly.  GRIM_GRAPH=1: captured once per batch and
// replayed as ONE hipGraph launch (no event nodes: they carry no timestamps when replayed on this runtime).
// Timing mode: launched directly, every kernel bracketed by its own start/stop events (launch).
static int enqueue_stage1(grim_batch *b) {
  grim_ctx *c = b->ctx;
  DevArgs &A = b->a;
  // staging region of the half-wave kernel's rows, at the top of the pool: host-tokenised subjects first, then one slot per
  // line of the device tokenizer
  const uint32_t stage0 = (uint32_t)b->row_limit - (b->n_small + b->n_dev_lines) * b->small_stride;
  // A run with both kinds launches the half-wave pair twice.  The half-wave and compaction times are then those of the
  // device-tokenised launch: the host-tokenised one goes out untimed (PH_NONE) rather than recording the same events first.
  if (b->n_small) enqueue_half_wave(b, b->n_dev_lines == 0, A, b->d_small, b->d_os, b->n_small, stage0);
  if (b->n_dev_lines) {
    // GL strings -> half-wave records on the device, then the half-wave kernel over one record slot per line
    DevTok T;
    T.text = b->d_text;
    T.lines = b->d_lines;
    T.lo = b->dev_lo;
    T.hi = b->dev_hi;
    T.dict = b->dict->d;
    T.dsmall = b->d_dsmall;
    T.subj = const_cast<grim_subject *>(A.subj);
    T.tok = const_cast<uint16_t *>(A.tok);
    T.tok_base = (uint32_t)(b->plan.tok_cap ? b->plan.tok_cap : 1);
    T.graph_loci = A.g.n_loci;
    const dim3 tgrid((b->n_dev_lines + (GRIM_WG / 64) * TOK_LINES_PER_WAVE - 1) / ((GRIM_WG / 64) * TOK_LINES_PER_WAVE));
    launch(b, PH_TOKENIZER, grim_tokenize_kernel, tgrid, dim3(GRIM_WG), A, T);
    DevArgs A2 = A;
    A2.small_ctr = A.small_ctr + 2 * b->n_host_small_waves;
    enqueue_half_wave(b, true, A2, b->d_dsmall, nullptr, b->n_dev_lines, stage0 + b->n_small * b->small_stride);
  }
  if (b->n_medium) {
    static const int waves_per_cu = env_int("GRIM_MEDIUM_WAVES", GRIM_MEDIUM_WAVES_PER_CU);
    uint32_t grid = (uint32_t)c->n_cu * (uint32_t)(waves_per_cu > 0 ? waves_per_cu : GRIM_MEDIUM_WAVES_PER_CU);
    if (grid > b->n_medium) grid = b->n_medium;
    launch(b, PH_ONE_WAVE, grim_plan_a_medium_kernel, dim3(grid), dim3(64), A, b->d_om, b->n_medium, A.bail_list);
  }
  if (A.mid_list && b->n_general + b->n_medium) {
    const uint32_t want = b->n_general + b->n_medium;
    uint32_t grid = (uint32_t)c->n_cu * GRIM_MID_WG_PER_CU;
    if (grid > want) grid = want;
    launch(b, PH_MID, grim_plan_a_mid_kernel, dim3(grid), dim3(GRIM_WG), A);
  }
  if (b->n_general + b->n_medium) {
    uint32_t want = b->n_general + b->n_medium;
    launch(b, PH_GENERAL, grim_plan_a_kernel, dim3(b->n_slots < want ? b->n_slots : want), dim3(GRIM_WG), A);
  }
  launch(b, PH_NONE, grim_finish_kernel, dim3(1), dim3(GRIM_WG), A.counters, b->hstate, 0u, 0);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int grim_batch_set_timing(grim_batch *b, int on) {
  if (!b) return -1;
  b->timing = on != 0;
  memset(b->acc_ms, 0, sizeof(b->acc_ms));
  b->n_timed = 0;
  return 0;
}

// A run in two halves, so that a caller can keep the device busy: engine_batch_enqueue launches stage 1 (half-wave, one-wave,
// general kernel, finish kernel) behind whatever the context's stream holds and returns at once; engine_batch_wait waits for
// that stage, launches stage 2 (Plan B / C, the table kernels) when the state block says subjects or accepted pairs are
// waiting, and returns what grim_batch_run returns.  The two may be called from different threads (one after the other).
// has the input copy of the last engine_batch_load arrived?  (any thread; never blocks)
int engine_batch_upload_done(grim_batch *b) {
  if (!b || !b->up_pending) return 1;
  use_device(b->ctx->device);
  if (hipEventQuery(b->ev_up) == hipSuccess) return 1;
  (void)hipGetLastError();
  return 0;
}

int engine_batch_enqueue(grim_batch *b) {
  if (!b) return -1;
  grim_ctx *c = b->ctx;
  use_device(c->device);
  if (((uint64_t)b->n_small + b->n_dev_lines) * b->small_stride > b->row_limit) {
    // the half-wave kernel's rows have fixed places in the staging region at the top of the pool: they must all exist
    b->rows_used = 0;
    set_err(c, "grim_batch_run: output row pool smaller than the half-wave kernel's fixed region");
    return -2;
  }
  memset(b->ms, 0, sizeof(b->ms));
  b->launched = 0;
  std::lock_guard<std::mutex> lk(c->run_mu);
  if (bind_scratch(b) != 0) return -1;
  if (b->up_pending) {
    // The batch's input went up on the upload stream.  A wait for its event in the launch stream costs the stream ~9 us
    // (a barrier packet on a signal of another queue: 46 -> 55 us per four 10-us kernels, profiles/r4_notes.md); when the
    // copy is over already -- the stream pipeline launches a chunk after it has sent the NEXT chunk's input up -- the
    // host has seen so and a launch from here on is ordered behind it without any packet.
    b->up_pending = false;
    if (hipEventQuery(b->ev_up) != hipSuccess) {
      (void)hipGetLastError();
      HIPCHK(hipStreamWaitEvent(c->stream, b->ev_up, 0), c, -1);
    }
  }
  if (b->timing) {
    if (enqueue_stage1(b) != 0) {
      set_err(c, "grim_batch_run: kernel launch failed");
      return -1;
    }
  } else {
    if (b->graph_state == 0) {
      b->graph_state = -1;
      // measured on MI355X / ROCm 7.2 (tools/step_time.py, 10k-subject batch): replaying the captured stage costs
      // 26.9 us per synchronous run, launching its two kernels directly 21.8 us -- so the replay is opt-in
      static const int use_graph = env_int("GRIM_GRAPH", 0);
      if (use_graph && hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
        int rc = enqueue_stage1(b);
        hipGraph_t gr = nullptr;
        hipError_t e = hipStreamEndCapture(c->stream, &gr);
        if (rc == 0 && e == hipSuccess && gr && hipGraphInstantiate(&b->gexec, gr, nullptr, nullptr, 0) == hipSuccess)
          b->graph_state = 1;
        if (gr) hipGraphDestroy(gr);
        (void)hipGetLastError();
      }
    }
    if (b->graph_state == 1) {
      HIPCHK(hipGraphLaunch(b->gexec, c->stream), c, -1);
    } else if (enqueue_stage1(b) != 0) {
      set_err(c, "grim_batch_run: kernel launch failed");
      return -1;
    }
  }
  HIPCHK(hipEventRecord(b->ev_done, c->stream), c, -1);
  b->enqueued = true;
  return 0;
}

// the times of the phases launched since the last call (timing mode; the caller has waited for the kernels)
static int read_phase_times(grim_batch *b) {
  for (int p = 0; p < PH_COUNT; ++p)
    if (b->launched >> p & 1) HIPCHK(hipEventElapsedTime(&b->ms[p], b->ev[p][0], b->ev[p][1]), b->ctx, -1);
  b->launched = 0;
  return 0;
}

// subjects the first stage left for the Plan-B kernel (q: the queue words of the run-state block)
static inline uint32_t planb_count(const uint32_t *q) { return q[GRIM_Q_NEXT] + q[GRIM_Q_NEXT_HEAVY]; }

int engine_batch_wait(grim_batch *b) {
  if (!b) return -1;
  grim_ctx *c = b->ctx;
  use_device(c->device);
  DevArgs &A = b->a;
  if (!b->enqueued) {
    set_err(c, "engine_batch_wait: nothing in flight");
    return -1;
  }
  b->enqueued = false;
  b->ran_ok = false;
  HIPCHK(hipEventSynchronize(b->ev_done), c, -1);
  if (read_phase_times(b) != 0) return -1;
  uint32_t q[GRIM_NQ];  // the queue words as the last finish kernel left them in the pinned block
  auto read_queue = [&] { memcpy(q, b->hstate + GRIM_NCTR, sizeof(q)); };
  read_queue();
  // ---- stage 2: Plan B / C when the first stage left subjects for it, then the table kernels ONCE over the accepted
  // pairs both stages queued (a round after each stage cost their tails twice) -------------------------------------
  const bool run_b = A.prm.planb && planb_count(q) > 0;
  if (run_b || stage2_pending(q) > 0) {
    {
      std::lock_guard<std::mutex> lk(c->run_mu);
      if (bind_scratch(b) != 0) return -1;
      if (run_b) {
        // the plan-A kernels leave the list of subjects in next_list/next_count
        uint32_t grid = b->n_slots < planb_count(q) ? b->n_slots : planb_count(q);
        launch(b, PH_PLAN_B, grim_plan_b_kernel, dim3(grid), dim3(GRIM_WG), A);
        if (hipGetLastError() != hipSuccess) {
          set_err(c, "grim_batch_run: plan-B launch failed");
          return -1;
        }
      }
      enqueue_tables(b);
      launch(b, PH_NONE, grim_finish_kernel, dim3(1), dim3(GRIM_WG), A.counters, b->hstate, 0u, 1);
      HIPCHK(hipGetLastError(), c, -1);
      HIPCHK(hipEventRecord(b->ev_done, c->stream), c, -1);
    }
    HIPCHK(hipEventSynchronize(b->ev_done), c, -1);
    if (read_phase_times(b) != 0) return -1;
    read_queue();
  }
  if (b->timing) {
    for (int p = 0; p < PH_COUNT; ++p) b->acc_ms[p] += b->ms[p];
    b->n_timed++;
  }
  static const int dbg_classes = env_int("GRIM_DEBUG_CLASSES", 0);
  if (dbg_classes)
    fprintf(stderr, "grim classes: mid-size kernel took %u, handed %u to the general kernel\n"
            "grim classes: small %u medium %u general %u | medium->general %u (+%u heavier), to plan B %u (+%u heavy) | table items %u one-wave, %u bigger (%u work units), %u pair records; workgroup merge: %u items (%u with an overflowed bucket), up to %u pairs; workgroup split: %u items | stage 1 %s\n",
            q[GRIM_Q_MID_WORK], q[GRIM_Q_MID], b->n_small, b->n_medium, b->n_general, q[GRIM_Q_BAIL], q[GRIM_Q_BAIL_HEAVY], q[GRIM_Q_NEXT], q[GRIM_Q_NEXT_HEAVY], q[GRIM_Q_T1], q[GRIM_Q_T2],
            q[GRIM_Q_TUNITS], q[GRIM_Q_POOL], q[GRIM_Q_DBG_MERGE_WG], q[GRIM_Q_DBG_MERGE_OVF], q[GRIM_Q_DBG_MERGE_MAX], q[GRIM_Q_DBG_SPLIT_WG],
            b->graph_state == 1 ? "replayed as a hipGraph" : "launched directly");
  memcpy(b->counters, b->hstate, sizeof(b->counters));
  b->small_ctr_pending = b->n_small + b->n_dev_lines > 0;
  for (int sh = 0; sh < GRIM_C_SLICES; ++sh)  // a slice: {probes, neighbour ids, frequency vectors, free}
    for (int k = GRIM_C_PROBES; k <= GRIM_C_FREQ; ++k) b->counters[k] += b->hstate[GRIM_C_SLICE0 + GRIM_C_SLICE_WORDS * sh + k];
  b->rows_used = q[GRIM_Q_ROWS];
  b->pool_asked = q[GRIM_Q_POOL];
  b->n_irregular = q[GRIM_Q_IRREGULAR];
#ifdef GRIM_STAMPS
  fprintf(stderr, "grim stamps (us):");
  for (int k = 0; k < 16; ++k) fprintf(stderr, " [%d]%.0f", k, b->hstate[GRIM_STAMP_BASE + k] / 100.0);
  fprintf(stderr, "\n");
  fprintf(stderr, "grim mid-size kernel stage us (setup, probes, rows, entries, lists, ladder, first pass, final pass, emit):");
  for (int k = 0; k < 9; ++k) fprintf(stderr, " %.0f", b->hstate[GRIM_MID_BASE + k] / 100.0);
  fprintf(stderr, "\ngrim mid-size kernel hand-overs (branch/candidates, hits, rows, entries, lists, pairs, dedup):");
  for (int k = 0; k < 7; ++k) fprintf(stderr, " %llu", b->hstate[GRIM_MID_BASE + 16 + k]);
  fprintf(stderr, "\n");
  static const char *hname[8] = {"0", "1", "2", "3 workgroup-merge items by pairs", "4 workgroup-split items by pairs",
                                 "5 workgroup-split us by pairs", "6 workgroup-merge items by genotype groups",
                                 "7 workgroup-merge us by pairs"};
  for (int h = 0; h < 8; ++h) {
    fprintf(stderr, "grim hist %s:", hname[h]);
    for (int k = 0; k < 24; ++k) fprintf(stderr, " %llu", b->hstate[GRIM_HIST_BASE + 24 * h + k]);
    fprintf(stderr, "\n");
  }
#endif
  if (b->counters[GRIM_C_OVERFLOW] != 0 || q[GRIM_Q_ROWS] > A.row_cap) {
    if (b->rows_used > A.row_cap) b->rows_used = A.row_cap;
    set_err(c, "grim_batch_run: output row pool exhausted (raise GRIM_ROW_CAP or lower the batch size)");
    return -2;
  }
  b->ran_ok = true;
  return 0;
}

extern "C" int grim_batch_run(grim_batch *b) {
  if (!b) return -1;
  int rc = engine_batch_enqueue(b);
  if (rc == 0) rc = engine_batch_wait(b);
  if (rc == -2 && !b->in_retry && engine_batch_grow_pool(b, 256ull << 20)) {
    // the accepted pairs outgrew the table kernels' pool: size it for what this run asked for and run again (the
    // inputs are still in the pinned arena; the prior matrices stay where they are)
    b->in_retry = true;
    EngineLoad ld = b->last_load;
    rc = engine_batch_load(b, &ld);
    if (rc == 0) rc = grim_batch_run(b);
    b->in_retry = false;
  }
  return rc;
}

extern "C" int grim_batch_run_repeat(grim_batch *b, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) {
    const int rc = grim_batch_run(b);
    if (rc != 0) return rc;
  }
  return 0;
}

extern "C" double grim_batch_kernel_ms(const grim_batch *b, int which) {
  if (!b) return 0.0;
  const bool mean = (which & GRIM_MS_MEAN) != 0;  // over the timed runs since grim_batch_set_timing(b, 1)
  const int w = which & ~GRIM_MS_MEAN;
  if (mean && !b->n_timed) return 0.0;
  double sum = 0.0;
  for (int p = 0; p < PH_COUNT; ++p)
    if (w == GRIM_MS_TOTAL || w == PHASES[p].which || (w == GRIM_MS_PLAN_A && PHASES[p].plan_a)) sum += mean ? b->acc_ms[p] : b->ms[p];
  return mean ? sum / b->n_timed : sum;
}

extern "C" int grim_batch_counters(const grim_batch *cb, uint64_t out[4]) {
  if (!cb) return -1;
  grim_batch *b = const_cast<grim_batch *>(cb);  // lazily folds the half-wave kernel's per-wave counts in
  if (b->small_ctr_pending) {
    grim_ctx *c = b->ctx;
    use_device(c->device);
    std::vector<uint32_t> h(2 * (size_t)b->n_small_waves);
    HIPCHK(hipMemcpy(h.data(), b->a.small_ctr, 4 * h.size(), hipMemcpyDeviceToHost), c, -1);
    for (size_t i = 0; i < h.size(); i += 2) {
      b->counters[GRIM_C_PROBES] += h[i];
      b->counters[GRIM_C_FREQ] += h[i + 1];
    }
    b->small_ctr_pending = false;
  }
  for (int k = GRIM_C_PROBES; k <= GRIM_C_FREQ; ++k) out[k] = b->counters[k];
  out[3] = b->rows_used;
  return 0;
}

extern "C" uint32_t grim_batch_total_rows(const grim_batch *b) { return b ? b->rows_used : 0; }

// D2H of result headers [res_lo, res_hi) and the rows into the pinned landing area (rows: or `rows_dst`) on stream `st`;
// wait: until the copies are over
static int batch_fetch_on(grim_batch *b, uint32_t res_lo, uint32_t res_hi, grim_row *rows_dst, hipStream_t st, bool wait) {
  if (!b) return -1;
  grim_ctx *c = b->ctx;
  use_device(c->device);
  b->fetch_hsa = false;
  if (res_hi > b->n_subj) res_hi = b->n_subj;
  // the pinned landing area mirrors the out arena as far as it is used; it grows on demand
  const uint64_t need = b->off_rows + sizeof(grim_row) * (uint64_t)(rows_dst ? 0 : b->rows_used);
  if (need > b->h_out_cap || !b->h_out) {
    uint64_t n = b->h_out_cap ? b->h_out_cap : (1u << 20);
    while (n < need) n *= 2;
    if (n > b->out_cap) n = b->out_cap;
    if (n < need) n = need;
    if (!pin_realloc(b->h_out, n)) {
      b->h_out_cap = 0;
      set_err(c, "engine_batch_fetch: pinned allocation failed");
      return -1;
    }
    b->h_out_cap = n;
  }
  b->h.res = (grim_subject_result *)b->h_out;
  b->h.rows = (grim_row *)(b->h_out + b->off_rows);
  const bool whole = res_lo == 0 && res_hi == b->n_subj && !rows_dst;
  if (whole && b->off_rows - sizeof(grim_subject_result) * (uint64_t)b->n_subj < 4096) {
    // headers and rows are (nearly) back to back: one copy
    const uint64_t bytes = b->rows_used ? b->off_rows + sizeof(grim_row) * (uint64_t)b->rows_used : sizeof(grim_subject_result) * (uint64_t)b->n_subj;
    const uint64_t n16 = (bytes + 15) / 16;  // (both arenas are 256-byte granular: the last sixteen bytes exist)
    if (bytes && !wait && c->export_mode == 2 && st == c->copy_stream) {
      // an SDMA engine of our own (grim_sdma.h); the caller has waited for the kernels that wrote the arena
      if (!b->sdma_job && grim_sdma_job_create(c->sdma, &b->sdma_job) != 0) b->sdma_job = 0;
      if (b->sdma_job && grim_sdma_d2h_issue(c->sdma, b->sdma_job, b->h_out, b->d_out, bytes) == 0) b->fetch_hsa = true;
    }
    const int by_kernel = c->export_mode == 1;
    if (b->fetch_hsa) {
    } else if (bytes && by_kernel && 16 * n16 <= b->h_out_cap && 16 * n16 <= b->out_cap) {
      uint32_t grid = (uint32_t)((n16 + 1023) / 1024);
      if (grid > 32) grid = 32;
      hipLaunchKernelGGL(grim_export_kernel, dim3(grid), dim3(256), 0, st, (uint4 *)b->h_out, (const uint4 *)b->d_out, n16);
      HIPCHK(hipGetLastError(), c, -1);
    } else if (bytes) {
      HIPCHK(hipMemcpyAsync(b->h_out, b->d_out, bytes, hipMemcpyDeviceToHost, st), c, -1);
    }
    g_moved[1] += bytes;
  } else {
    if (res_hi > res_lo) {
      const uint64_t o = sizeof(grim_subject_result) * (uint64_t)res_lo, n = sizeof(grim_subject_result) * (uint64_t)(res_hi - res_lo);
      HIPCHK(hipMemcpyAsync(b->h_out + o, b->d_out + o, n, hipMemcpyDeviceToHost, st), c, -1);
      g_moved[1] += n;
    }
    if (b->rows_used) {
      void *dst = rows_dst ? (void *)rows_dst : (void *)(b->h_out + b->off_rows);
      HIPCHK(hipMemcpyAsync(dst, b->d_out + b->off_rows, sizeof(grim_row) * (uint64_t)b->rows_used, hipMemcpyDeviceToHost, st), c, -1);
      g_moved[1] += sizeof(grim_row) * (uint64_t)b->rows_used;
    }
  }
  if (wait) HIPCHK(hipStreamSynchronize(st), c, -1);
  return 0;
}

int engine_batch_fetch(grim_batch *b, uint32_t res_lo, uint32_t res_hi, grim_row *rows_dst) {
  return b ? batch_fetch_on(b, res_lo, res_hi, rows_dst, b->ctx->stream, true) : -1;
}
// The whole batch's results over the context's copy stream: the caller has synchronised the kernels (engine_batch_wait
// returned) and may run the NEXT batch's kernels while this copy is in flight.  In two halves: the copy is queued on the
// copy stream with an event behind it (issue), another thread waits for that event (wait) -- so the thread that watches
// the kernels is not held up by a PCIe transfer.
// GRIM_DEBUG_COPYTIME (diagnostic): the D2H's own duration by a pair of timing events on the copy stream
static std::atomic<uint64_t> g_ct_ns, g_ct_n;
static hipEvent_t g_ct_ev[2][64];
static std::atomic<uint32_t> g_ct_k;
static int ct_on() {
  static const int on = [] {
    const int v = env_int("GRIM_DEBUG_COPYTIME", 0);
    if (v) {
      for (int i = 0; i < 64; ++i) { (void)hipEventCreate(&g_ct_ev[0][i]); (void)hipEventCreate(&g_ct_ev[1][i]); }
      atexit([] { if (g_ct_n.load()) fprintf(stderr, "grim: D2H on the copy stream: %.1f us average over %llu copies\n", g_ct_ns.load() / 1e3 / (double)g_ct_n.load(), (unsigned long long)g_ct_n.load()); });
    }
    return v;
  }();
  return on;
}
int engine_batch_fetch_issue(grim_batch *b) {
  if (!b) return -1;
  const bool ct = ct_on() != 0;
  if (ct) {
    b->ct_slot = (int)(g_ct_k.fetch_add(1) & 63);
    (void)hipEventRecord(g_ct_ev[0][b->ct_slot], b->ctx->copy_stream);
  }
  if (batch_fetch_on(b, 0, b->n_subj, nullptr, b->ctx->copy_stream, false) != 0) return -1;
  if (ct) (void)hipEventRecord(g_ct_ev[1][b->ct_slot], b->ctx->copy_stream);
  if (ct || !b->fetch_hsa) HIPCHK(hipEventRecord(b->ev_copy, b->ctx->copy_stream), b->ctx, -1);
  return 0;
}
int engine_batch_fetch_wait(grim_batch *b) {
  if (!b) return -1;
  use_device(b->ctx->device);
  if (b->fetch_hsa) {
    b->fetch_hsa = false;
    if (grim_sdma_wait(b->ctx->sdma, b->sdma_job) != 0) {
      set_err(b->ctx, "engine_batch_fetch: the SDMA copy of the results failed");
      return -1;
    }
    return 0;
  }
  HIPCHK(hipEventSynchronize(b->ev_copy), b->ctx, -1);
  if (ct_on() && b->ct_slot >= 0) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, g_ct_ev[0][b->ct_slot], g_ct_ev[1][b->ct_slot]) == hipSuccess) { g_ct_ns += (uint64_t)(ms * 1e6); ++g_ct_n; }
    b->ct_slot = -1;
  }
  return 0;
}
extern "C" int grim_batch_results(grim_batch *b, grim_subject_result *res, grim_row *rows) {
  if (!b) return -1;
  grim_ctx *c = b->ctx;
  use_device(c->device);
  if (b->n_subj) HIPCHK(hipMemcpy(res, b->a.res, sizeof(grim_subject_result) * (size_t)b->n_subj, hipMemcpyDeviceToHost), c, -1);
  if (b->rows_used) HIPCHK(hipMemcpy(rows, b->a.rows, sizeof(grim_row) * (size_t)b->rows_used, hipMemcpyDeviceToHost), c, -1);
  return 0;
}

extern "C" void grim_batch_free(grim_batch *b) { batch_destroy(b); }

static void batch_destroy(grim_batch *b) {
  if (!b) return;
  use_device(b->ctx->device);
  hipStreamSynchronize(b->ctx->stream);
  for (auto &pair : b->ev)
    for (hipEvent_t e : pair)
      if (e) hipEventDestroy(e);
  if (b->ev_done) hipEventDestroy(b->ev_done);
  if (b->ev_copy) hipEventDestroy(b->ev_copy);
  if (b->fetch_hsa && b->ctx->sdma) (void)grim_sdma_wait(b->ctx->sdma, b->sdma_job);  // (an abandoned stream: the copy still writes h_out)
  if (b->sdma_job && b->ctx->sdma) grim_sdma_job_destroy(b->ctx->sdma, b->sdma_job);
  if (b->ev_up) hipEventDestroy(b->ev_up);
  if (b->gexec) hipGraphExecDestroy(b->gexec);
  void *dev[] = {b->d_in, b->d_work, b->d_out, b->d_priors, b->d_pool};
  for (void *p : dev)
    if (p) hipFree(p);
  void *pin[] = {b->h_in, b->h_out, b->h_priors, b->hstate};
  for (void *p : pin)
    if (p) hipHostFree(p);
  delete b;
}

// =================================================================================================
// Shared pieces of the finished-batch consumers below (M-step, marginal tables, match probabilities, donor search): each
// consumer is a plain struct that holds these by value
// =================================================================================================
// A device array kept across calls and grown on demand.  Growing discards the contents; a failed grow leaves it empty
// (null, capacity 0), so that the next call tries again.  Kernels are handed these pointers even for a side without rows:
// a caller that must never pass null asks for one element more than it needs.
template <typename T>
struct DevBuf {
  T *p = nullptr;
  uint64_t cap = 0;  // elements
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) hipFree(p);
    p = nullptr;
    cap = 0;
  }
  // room for `need` elements; a grow allocates need + headroom
  bool reserve(uint64_t need, uint64_t headroom = 0) {
    if (need <= cap) return true;
    release();
    if (hipMalloc((void **)&p, sizeof(T) * (need + headroom)) != hipSuccess) {
      (void)hipGetLastError();
      p = nullptr;
      return false;
    }
    cap = need + headroom;
    return true;
  }
  operator T *() const { return p; }
};

// several buffers to one size; false if any of them fails
template <typename... B>
static bool reserve_all(uint64_t need, uint64_t headroom, B &...bufs) {
  return (bufs.reserve(need, headroom) && ...);
}

template <int N>
struct Events {
  hipEvent_t ev[N] = {};
  Events() = default;
  Events(const Events &) = delete;
  Events &operator=(const Events &) = delete;
  ~Events() {
    for (hipEvent_t e : ev)
      if (e) hipEventDestroy(e);
  }
  bool create() {
    for (hipEvent_t &e : ev)
      if (hipEventCreate(&e) != hipSuccess) return false;
    return true;
  }
  hipEvent_t operator[](int k) const { return ev[k]; }
};

static bool refuse(grim_ctx *c, const char *who, const char *why) {
  set_err(c, std::string(who) + ": " + why);
  return false;
}

// The door of a consumer that works on a finished batch where its rows lie.  n_pops == 0: the consumer needs genotype rows
// and keeps the locus slots of keep_mask; n_pops > 0: it needs phased rows that carry populations, n_pops of them.  The
// first check that fails sets the message; the caller returns -3.
static bool batch_door(grim_ctx *c, const char *who, const grim_batch *b, uint32_t keep_mask, uint32_t n_pops) {
  if (b->ctx != c) return refuse(c, who, "the batch belongs to another context");
  if (n_pops && (!b->a.prm.em_mr || !b->a.prm.out_haps))
    return refuse(c, who, "the batch was built without em_mr / out_haps: its phased rows carry no populations");
  if (!b->ran_ok) return refuse(c, who, "the batch holds no finished run (call grim_batch_run first)");
  if (n_pops) return b->g->d.P == n_pops || refuse(c, who, "the batch's graph has another number of populations");
  if (!b->a.prm.out_muug) return refuse(c, who, "the batch was built with out_muug off: it holds no genotype rows");
  if (keep_mask == 0 || b->g->d.n_loci > GRIM_MAXL || (keep_mask >> b->g->d.n_loci) != 0)
    return refuse(c, who, "keep_mask is empty or names a locus slot the graph does not have");
  return true;
}

// the door of a consumer that is given host records; the caller returns -3
static bool records_door(grim_ctx *c, const char *who, uint32_t keep_mask, const grim_subject_result *res, uint32_t n, const grim_row *rows,
                         uint64_t n_rows) {
  if (keep_mask == 0 || (keep_mask >> GRIM_MAXL) != 0) return refuse(c, who, "keep_mask is empty or names a locus slot beyond GRIM_MAXL");
  if ((n && !res) || (n_rows && !rows) || n_rows > 0x7FFFFFFFull) return refuse(c, who, "bad arguments");
  return true;
}

// host records on the device, kept and grown
struct RecordsUpload {
  DevBuf<grim_subject_result> res;
  DevBuf<grim_row> rows;
  // res[n], rows[n_rows] of the host into the buffers; the caller's arrays are free again on return
  int upload(grim_ctx *c, const char *who, const grim_subject_result *h_res, uint32_t n, const grim_row *h_rows, uint32_t n_rows) {
    if (!res.reserve((uint64_t)n + 1) || !rows.reserve((uint64_t)n_rows + 1)) {  // never an empty allocation
      set_err(c, std::string(who) + ": device allocation failed");
      return -1;
    }
    if (n) HIPCHK(hipMemcpyAsync(res, h_res, sizeof(grim_subject_result) * (uint64_t)n, hipMemcpyHostToDevice, c->stream), c, -1);
    if (n_rows) HIPCHK(hipMemcpyAsync(rows, h_rows, sizeof(grim_row) * (uint64_t)n_rows, hipMemcpyHostToDevice, c->stream), c, -1);
    HIPCHK(hipStreamSynchronize(c->stream), c, -1);
    return 0;
  }
};

// the door of a consumer that is given an exported table keys / pops / counts [n] in grim_em_export's order; `whose` names
// the owner of n_pops in the text ("the graph's").  n_alleles, when given, bounds the fields of a key.  *distinct, when
// given, takes the number of different keys.  The caller returns -3.
static bool counts_door(grim_ctx *c, const char *who, const char *whose, uint32_t n_pops, const uint32_t *n_alleles, const uint64_t *keys,
                        const uint32_t *pops, const double *counts, uint64_t n, uint64_t *distinct) {
  if (n && (!keys || !pops || !counts)) return refuse(c, who, "a null array with n > 0");
  uint64_t nd = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (pops[i] >= n_pops) return refuse(c, who, (std::string("a population at or above ") + whose + " number of populations").c_str());
    if (keys[i] >> GRIM_KEY_GRAPH_ORDER) return refuse(c, who, "a key with a bit at or above GRIM_KEY_GRAPH_ORDER");
    if (n_alleles)
      for (int q = 0; q < GRIM_MAXL; ++q)
        if ((uint32_t)((keys[i] >> (GRIM_ABITS * q)) & 0xFFFu) > n_alleles[q])
          return refuse(c, who, "a key with a field above n_alleles of its slot (an exported table never holds a private allele)");
    if (i && !(keys[i - 1] < keys[i] || (keys[i - 1] == keys[i] && pops[i - 1] < pops[i])))
      return refuse(c, who, "the entries are not strictly ascending in (key, pop)");
    if (!(counts[i] >= 0.0 && counts[i] <= 1.7976931348623157e308)) return refuse(c, who, "a count that is negative, NaN or infinite");
    nd += i == 0 || keys[i - 1] != keys[i];
  }
  if (distinct) *distinct = nd;
  return true;
}

// an exported table on the device, kept and grown
struct CountsUpload {
  DevBuf<unsigned long long> keys;
  DevBuf<uint32_t> pops;
  DevBuf<double> counts;
  int upload(grim_ctx *c, const char *who, const uint64_t *h_keys, const uint32_t *h_pops, const double *h_counts, uint64_t n) {
    if (!keys.reserve(n + 1) || !pops.reserve(n + 1) || !counts.reserve(n + 1)) {  // never an empty allocation
      set_err(c, std::string(who) + ": device allocation failed");
      return -1;
    }
    if (n) {
      HIPCHK(hipMemcpyAsync(keys, h_keys, 8 * n, hipMemcpyHostToDevice, c->stream), c, -1);
      HIPCHK(hipMemcpyAsync(pops, h_pops, 4 * n, hipMemcpyHostToDevice, c->stream), c, -1);
      HIPCHK(hipMemcpyAsync(counts, h_counts, 8 * n, hipMemcpyHostToDevice, c->stream), c, -1);
      HIPCHK(hipStreamSynchronize(c->stream), c, -1);
    }
    return 0;
  }
};

// a statistics block of the device (SLICES copies of COUNT words), slices added up; ends in a stream synchronise
template <uint32_t COUNT, uint32_t SLICES>
static int read_stat(grim_ctx *c, const unsigned long long *d_stat, uint64_t h[COUNT]) {
  unsigned long long hs[COUNT * SLICES];
  HIPCHK(hipMemcpyAsync(hs, d_stat, sizeof(hs), hipMemcpyDeviceToHost, c->stream), c, -1);
  HIPCHK(hipStreamSynchronize(c->stream), c, -1);
  for (uint32_t k = 0; k < COUNT; ++k) h[k] = 0;
  for (uint32_t k = 0; k < COUNT * SLICES; ++k) h[k % COUNT] += hs[k];
  return 0;
}

// the grid's second dimension ends at 65535: launch(p0, np) for every slab [p0, p0 + np) of n_p rows
template <typename F>
static void for_slabs(uint32_t n_p, F launch) {
  for (uint32_t p0 = 0; p0 < n_p; p0 += 65535u) launch(p0, n_p - p0 < 65535u ? n_p - p0 : 65535u);
}

// =================================================================================================
// M-step accumulator (grim_em.h): haplotype / population counts from the phased rows of finished batches
// =================================================================================================
static_assert(sizeof(EmSpill) == sizeof(grim_em_spill_rec) && sizeof(EmSpill) == 32, "spill record layout");

struct grim_em {
  grim_ctx *ctx;
  EmLimits lim;
  EmTable T;               // keys / popmask / counts in HBM
  uint64_t cap;            // slots (a power of two); at most half of them are ever used
  DevBuf<unsigned long long> d_stat;
  // per-batch buffers: positions per subject, (group, position) ping-pong, weights, radix counts, spill
  DevBuf<uint32_t> d_first, d_grp[2], d_idx[2], d_cnt;
  DevBuf<double> d_w, d_ws;
  DevBuf<EmSpill> d_spill;
  RecordsUpload in;            // the uploaded records of grim_em_accumulate_records
  CountsUpload merge_in;       // the uploaded table of grim_em_merge_records
  std::vector<EmSpill> spill;  // every batch's records, in contract order
  uint64_t table_used, entries, n_used, n_planc, n_contrib, n_rehash, last_unsupported;
  uint32_t batch_no;
  Events<8> ev;  // 0..3 a batch, 4..5 a rehash, 6..7 a merge
  double last_ms, merge_ms;
};

static void em_table_free(EmTable &T) {
  if (T.keys) hipFree(T.keys);
  if (T.popmask) hipFree(T.popmask);
  if (T.counts) hipFree(T.counts);
  T.keys = T.popmask = nullptr;
  T.counts = nullptr;
}

static bool em_table_alloc(grim_ctx *c, EmTable &T, uint64_t cap, uint32_t P) {
  T.keys = T.popmask = nullptr;
  T.counts = nullptr;
  T.mask = (uint32_t)(cap - 1);
  T.P = P;
  if (hipMalloc((void **)&T.keys, 8 * cap) != hipSuccess || hipMalloc((void **)&T.popmask, 8 * cap) != hipSuccess ||
      hipMalloc((void **)&T.counts, 8 * cap * P) != hipSuccess || hipMemsetAsync(T.keys, 0, 8 * cap, c->stream) != hipSuccess ||
      hipMemsetAsync(T.popmask, 0, 8 * cap, c->stream) != hipSuccess || hipMemsetAsync(T.counts, 0, 8 * cap * P, c->stream) != hipSuccess) {
    (void)hipGetLastError();
    em_table_free(T);
    return false;
  }
  return true;
}

extern "C" grim_em *grim_em_create(grim_ctx *c, const uint32_t n_alleles[GRIM_MAXL], uint32_t n_pops, uint64_t first_capacity) {
  if (!c || !n_alleles || n_pops == 0 || n_pops > GRIM_MAXPOP) {
    set_err(c, "grim_em_create: bad arguments");
    return nullptr;
  }
  use_device(c->device);
  uint64_t cap = 64;
  while (cap < first_capacity) cap *= 2;
  if (cap * n_pops > (1ull << 31)) {
    set_err(c, "grim_em_create: first_capacity times the populations is beyond 2^31 counters");
    return nullptr;
  }
  grim_em *e = new grim_em();
  e->ctx = c;
  for (int q = 0; q < GRIM_MAXL; ++q) e->lim.n_alleles[q] = n_alleles[q];
  e->cap = cap;
  bool ok = em_table_alloc(c, e->T, cap, n_pops);
  ok = ok && e->d_stat.reserve(EM_S_COUNT) && hipMemsetAsync(e->d_stat, 0, 8 * EM_S_COUNT, c->stream) == hipSuccess;
  ok = ok && e->ev.create() && hipStreamSynchronize(c->stream) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    set_err(c, "grim_em_create: device allocation failed");
    grim_em_free(e);
    return nullptr;
  }
  return e;
}

extern "C" void grim_em_free(grim_em *e) {
  if (!e) return;
  use_device(e->ctx->device);
  hipStreamSynchronize(e->ctx->stream);
  em_table_free(e->T);
  delete e;
}

// a table twice the size, the entries moved by a kernel with their counters; returns the kernel's milliseconds or < 0
static double em_rehash(grim_em *e, const std::string &name) {
  grim_ctx *c = e->ctx;
  if (e->cap * 2 * e->T.P > (1ull << 31)) {
    set_err(c, name + ": the table cannot grow beyond 2^31 counters");
    return -1.0;
  }
  EmTable to;
  if (!em_table_alloc(c, to, e->cap * 2, e->T.P)) {
    set_err(c, name + ": device allocation failed (rehash)");
    return -1.0;
  }
  float ms = 0;
  bool ok = hipEventRecord(e->ev[4], c->stream) == hipSuccess;
  hipLaunchKernelGGL(em_rehash_kernel, dim3((uint32_t)((e->cap + 255) / 256)), dim3(256), 0, c->stream, e->T, to, e->d_stat);
  ok = ok && hipGetLastError() == hipSuccess && hipEventRecord(e->ev[5], c->stream) == hipSuccess &&
       hipStreamSynchronize(c->stream) == hipSuccess && hipEventElapsedTime(&ms, e->ev[4], e->ev[5]) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    em_table_free(to);
    set_err(c, name + ": rehash failed");
    return -1.0;
  }
  em_table_free(e->T);
  e->T = to;
  e->cap *= 2;
  e->n_rehash++;
  return ms;
}

// the device sequence on n subjects whose phased rows lie in [0, rows_used) of `rows` (device arrays); one "batch" of batch_no
static int em_run(grim_em *e, const char *who, const grim_subject_result *res, const grim_row *rows, uint32_t n, uint32_t rows_used) {
  grim_ctx *c = e->ctx;
  hipStream_t st = c->stream;
  const std::string name(who);
  const uint32_t batch_no = e->batch_no++;
  if (n == 0) return 0;
  if (!e->d_first.reserve((uint64_t)n + 1)) {
    set_err(c, name + ": device allocation failed");
    return -1;
  }
  // ---- rows per subject -> positions ------------------------------------------------------------------------------
  HIPCHK(hipMemsetAsync(e->d_stat, 0, 8 * 4, st), c, -1);  // the per-call words
  HIPCHK(hipMemsetAsync(e->d_stat + EM_S_FAULT, 0, 8, st), c, -1);
  HIPCHK(hipEventRecord(e->ev[0], st), c, -1);
  hipLaunchKernelGGL(em_count_kernel, dim3((n + 255) / 256), dim3(256), 0, st, res, n, rows_used, e->d_first, e->d_stat);
  hipLaunchKernelGGL(em_scan_kernel, dim3(1), dim3(1024), 0, st, e->d_first, n);
  HIPCHK(hipGetLastError(), c, -1);
  HIPCHK(hipEventRecord(e->ev[1], st), c, -1);
  uint32_t n_rows = 0;
  HIPCHK(hipMemcpyAsync(&n_rows, e->d_first + n, 4, hipMemcpyDeviceToHost, st), c, -1);
  HIPCHK(hipStreamSynchronize(st), c, -1);
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, e->ev[0], e->ev[1]), c, -1);
  double total_ms = ms;
  if (n_rows > rows_used || n_rows > 0x3FFFFFFFu) {
    set_err(c, name + ": more phased rows than the batch holds");
    return -1;
  }
  const uint32_t C = 2 * n_rows;  // contributions
  if (C) {
    // ---- room first: C contributions insert at most C haplotypes -----------------------------------------------------
    while (e->table_used + C > e->cap / 2) {
      const double r = em_rehash(e, name);
      if (r < 0) return -1;
      total_ms += r;
    }
    const uint32_t n_chunks = (C + GRIM_EM_CHUNK - 1) / GRIM_EM_CHUNK;
    if (!reserve_all(C, C / 4, e->d_grp[0], e->d_grp[1], e->d_idx[0], e->d_idx[1], e->d_w, e->d_ws, e->d_spill) ||
        !e->d_cnt.reserve(256ull * n_chunks + 1)) {
      set_err(c, name + ": device allocation failed");
      return -1;
    }
    HIPCHK(hipEventRecord(e->ev[2], st), c, -1);
    hipLaunchKernelGGL(em_weight_kernel, dim3((n + 3) / 4), dim3(256), 0, st, res, rows, n, e->d_first, e->T, e->lim, batch_no,
                       e->d_grp[0], e->d_idx[0], e->d_w, e->d_spill, C, e->d_stat);
    // groups are < cap * P; one bit more sends the records without a group behind them
    uint32_t bits = 1;
    while ((1ull << bits) < e->cap * e->T.P) ++bits;
    int cur = 0;
    for (uint32_t shift = 0; shift < bits + 1; shift += 8) {
      hipLaunchKernelGGL(em_radix_hist_kernel, dim3(n_chunks), dim3(64), 0, st, e->d_grp[cur], C, n_chunks, shift, e->d_cnt);
      hipLaunchKernelGGL(em_scan_kernel, dim3(1), dim3(1024), 0, st, e->d_cnt, 256u * n_chunks);
      hipLaunchKernelGGL(em_radix_scatter_kernel, dim3(n_chunks), dim3(64), 0, st, e->d_grp[cur], e->d_idx[cur], e->d_grp[cur ^ 1],
                         e->d_idx[cur ^ 1], C, n_chunks, shift, e->d_cnt);
      cur ^= 1;
    }
    hipLaunchKernelGGL(em_gather_kernel, dim3((C + 255) / 256), dim3(256), 0, st, e->d_idx[cur], e->d_w, e->d_ws, C);
    hipLaunchKernelGGL(em_sum_kernel, dim3((C + 255) / 256), dim3(256), 0, st, e->d_grp[cur], e->d_ws, C, e->T, e->d_stat);
    HIPCHK(hipGetLastError(), c, -1);
    HIPCHK(hipEventRecord(e->ev[3], st), c, -1);
  }
  unsigned long long h[EM_S_COUNT];
  HIPCHK(hipMemcpyAsync(h, e->d_stat, sizeof(h), hipMemcpyDeviceToHost, st), c, -1);
  HIPCHK(hipStreamSynchronize(st), c, -1);
  if (C) {
    HIPCHK(hipEventElapsedTime(&ms, e->ev[2], e->ev[3]), c, -1);
    total_ms += ms;
  }
  e->last_ms = total_ms;
  e->last_unsupported = h[EM_S_UNSUPPORTED];
  if (h[EM_S_FAULT] || h[EM_S_SPILL] > C) {
    set_err(c, name + ": the haplotype table overflowed (internal)");
    return -1;
  }
  e->table_used = h[EM_S_TABLE];
  e->entries = h[EM_S_ENTRIES];
  e->n_used += h[EM_S_USED];
  e->n_planc += h[EM_S_PLANC];
  e->n_contrib += C;
  if (h[EM_S_SPILL]) {
    const size_t at = e->spill.size(), ns = (size_t)h[EM_S_SPILL];
    e->spill.resize(at + ns);
    HIPCHK(hipMemcpy(e->spill.data() + at, e->d_spill, sizeof(EmSpill) * ns, hipMemcpyDeviceToHost), c, -1);
    std::sort(e->spill.begin() + at, e->spill.end(), [](const EmSpill &x, const EmSpill &y) {
      if (x.subject != y.subject) return x.subject < y.subject;
      if (x.row != y.row) return x.row < y.row;
      return x.side < y.side;
    });
  }
  return 0;
}

extern "C" int grim_em_accumulate(grim_em *e, grim_batch *b) {
  if (!e || !b) return -1;
  grim_ctx *c = e->ctx;
  e->last_ms = 0.0;
  e->last_unsupported = 0;
  if (!batch_door(c, "grim_em_accumulate", b, 0, e->T.P)) return -3;
  use_device(c->device);
  return em_run(e, "grim_em_accumulate", b->a.res, b->a.rows, b->n_subj, b->rows_used);
}

extern "C" int grim_em_accumulate_records(grim_em *e, const grim_subject_result *res, uint32_t n_subjects, const grim_row *rows,
                                          uint64_t n_rows) {
  if (!e) return -1;
  grim_ctx *c = e->ctx;
  e->last_ms = 0.0;
  e->last_unsupported = 0;
  if (!records_door(c, "grim_em_accumulate_records", (1u << GRIM_MAXL) - 1u, res, n_subjects, rows, n_rows)) return -3;
  use_device(c->device);
  if (n_subjects && e->in.upload(c, "grim_em_accumulate_records", res, n_subjects, rows, (uint32_t)n_rows) != 0) return -1;
  return em_run(e, "grim_em_accumulate_records", e->in.res, e->in.rows, n_subjects, (uint32_t)n_rows);
}

// the launch behind both merge doors: room for `incoming` keys first, then one lane per slot of S (n == 0) or per entry of
// the uploaded table
static int em_merge_run(grim_em *e, const char *who, const EmTable *S, uint64_t incoming, uint32_t n) {
  grim_ctx *c = e->ctx;
  hipStream_t st = c->stream;
  const std::string name(who);
  double total_ms = 0.0;
  while (e->table_used + incoming > e->cap / 2) {
    const double r = em_rehash(e, name);
    if (r < 0) return -1;
    total_ms += r;
  }
  HIPCHK(hipMemsetAsync(e->d_stat + EM_S_FAULT, 0, 8, st), c, -1);
  HIPCHK(hipEventRecord(e->ev[6], st), c, -1);
  if (S)
    hipLaunchKernelGGL(em_merge_kernel, dim3((S->mask + 256u) / 256u), dim3(256), 0, st, *S, e->T, e->d_stat);
  else
    hipLaunchKernelGGL(em_merge_records_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, e->merge_in.keys, e->merge_in.pops,
                       e->merge_in.counts, n, e->T, e->d_stat);
  HIPCHK(hipGetLastError(), c, -1);
  HIPCHK(hipEventRecord(e->ev[7], st), c, -1);
  uint64_t h[EM_S_COUNT];
  if (read_stat<EM_S_COUNT, 1>(c, e->d_stat, h) != 0) return -1;
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, e->ev[6], e->ev[7]), c, -1);
  e->merge_ms = total_ms + ms;
  if (h[EM_S_FAULT]) {
    set_err(c, name + ": the haplotype table overflowed (internal)");
    return -1;
  }
  e->table_used = h[EM_S_TABLE];
  e->entries = h[EM_S_ENTRIES];
  return 0;
}

extern "C" int grim_em_merge(grim_em *dst, grim_em *src) {
  if (!dst || !src) return -1;
  grim_ctx *c = dst->ctx;
  const char *who = "grim_em_merge";
  dst->merge_ms = 0.0;
  if (src == dst) return refuse(c, who, "the source is the destination"), -3;
  if (src->ctx != c) return refuse(c, who, "the accumulator belongs to another context"), -3;
  if (src->T.P != dst->T.P) return refuse(c, who, "the accumulator has another number of populations"), -3;
  for (int q = 0; q < GRIM_MAXL; ++q)
    if (src->lim.n_alleles[q] != dst->lim.n_alleles[q]) return refuse(c, who, "the accumulator has another n_alleles"), -3;
  use_device(c->device);
  if (src->entries == 0) return 0;
  return em_merge_run(dst, who, &src->T, src->table_used, 0);
}

extern "C" int grim_em_merge_records(grim_em *e, const uint64_t *keys, const uint32_t *pops, const double *counts, uint64_t n) {
  if (!e) return -1;
  grim_ctx *c = e->ctx;
  const char *who = "grim_em_merge_records";
  e->merge_ms = 0.0;
  uint64_t distinct = 0;
  if (!counts_door(c, who, "the accumulator's", e->T.P, e->lim.n_alleles, keys, pops, counts, n, &distinct)) return -3;
  use_device(c->device);
  if (n == 0) return 0;
  if (n > 0x7FFFFFFFull) {  // strictly ascending entries of at most P populations a key: more than any table holds
    set_err(c, std::string(who) + ": the table cannot grow beyond 2^31 counters");
    return -1;
  }
  if (e->merge_in.upload(c, who, keys, pops, counts, n) != 0) return -1;
  return em_merge_run(e, who, nullptr, distinct, (uint32_t)n);
}

extern "C" double grim_em_merge_ms(const grim_em *e) { return e ? e->merge_ms : 0.0; }

extern "C" uint64_t grim_em_entries(const grim_em *e) { return e ? e->entries : 0; }
extern "C" uint64_t grim_em_spill_count(const grim_em *e) { return e ? e->spill.size() : 0; }
extern "C" uint64_t grim_em_last_unsupported(const grim_em *e) { return e ? e->last_unsupported : 0; }
extern "C" double grim_em_kernel_ms(const grim_em *e) { return e ? e->last_ms : 0.0; }

extern "C" int grim_em_spill(grim_em *e, uint64_t first, uint64_t n, grim_em_spill_rec *out) {
  if (!e || !out || first > e->spill.size() || n > e->spill.size() - first) return -1;
  if (n) memcpy(out, e->spill.data() + first, sizeof(EmSpill) * (size_t)n);
  return 0;
}

extern "C" int grim_em_stats(const grim_em *e, uint64_t out[4]) {
  if (!e || !out) return -1;
  out[0] = e->n_used;
  out[1] = e->n_planc;
  out[2] = e->n_contrib;
  out[3] = e->n_rehash;
  return 0;
}

extern "C" int grim_em_export(grim_em *e, uint64_t *keys, uint32_t *pops, double *counts) {
  if (!e) return -1;
  if (e->entries == 0) return 0;
  if (!keys || !pops || !counts) return -1;
  grim_ctx *c = e->ctx;
  use_device(c->device);
  const uint32_t P = e->T.P;
  std::vector<unsigned long long> hk(e->cap), hm(e->cap);
  std::vector<double> hc(e->cap * P);
  HIPCHK(hipMemcpy(hk.data(), e->T.keys, 8 * e->cap, hipMemcpyDeviceToHost), c, -1);
  HIPCHK(hipMemcpy(hm.data(), e->T.popmask, 8 * e->cap, hipMemcpyDeviceToHost), c, -1);
  HIPCHK(hipMemcpy(hc.data(), e->T.counts, 8 * e->cap * P, hipMemcpyDeviceToHost), c, -1);
  // slot numbers depend on which insert came first: the entries leave in (key, population) order
  std::vector<std::pair<uint64_t, uint64_t>> order;  // (key, slot)
  for (uint64_t s = 0; s < e->cap; ++s)
    if (hk[s] && hm[s]) order.emplace_back(hk[s] & ~GRIM_VALID, s);
  std::sort(order.begin(), order.end());
  uint64_t k = 0;
  for (const auto &o : order)
    for (uint32_t p = 0; p < P; ++p)
      if ((hm[o.second] >> p) & 1ull) {
        if (k >= e->entries) {
          set_err(c, "grim_em_export: more entries than counted (internal)");
          return -1;
        }
        keys[k] = o.first;
        pops[k] = p;
        counts[k] = hc[o.second * P + p];
        ++k;
      }
  if (k != e->entries) {
    set_err(c, "grim_em_export: fewer entries than counted (internal)");
    return -1;
  }
  return 0;
}

// =================================================================================================
// EM on a fixed support (grim_refresh.h): the graph's frequencies from M-step counts
// =================================================================================================
struct RefreshState {
  DevBuf<uint32_t> d_short, d_long;  // the partial nodes by row length
  DevBuf<double> d_c, d_bsum, d_total, d_shadow;
  DevBuf<unsigned long long> d_stat;
  CountsUpload in;  // the uploaded records of grim_graph_refresh_records
  Events<4> ev;
};

static void refresh_state_free(RefreshState *rf) { delete rf; }

// the graph's refresh state, made by the first refresh of a refreshable graph: every buffer whose size the graph fixes, and
// the two node lists on the device; null and a text on failure
static RefreshState *refresh_state(grim_graph *g, const char *who) {
  if (g->rf) return g->rf;
  const uint32_t V = g->d.n_nodes, P = g->d.P, F = g->n_full;
  const uint32_t n_short = (uint32_t)g->rf_short.size(), n_long = (uint32_t)g->rf_long.size();
  const uint32_t n_blocks = (F + GRIM_REFRESH_BLOCK - 1) / GRIM_REFRESH_BLOCK;
  RefreshState *rf = new RefreshState();
  bool ok = rf->ev.create() && rf->d_short.reserve((uint64_t)n_short + 1) && rf->d_long.reserve((uint64_t)n_long + 1) &&
            rf->d_c.reserve((uint64_t)F * P + 1) && rf->d_bsum.reserve((uint64_t)n_blocks * P + 1) && rf->d_total.reserve(GRIM_MAXPOP) &&
            rf->d_shadow.reserve((uint64_t)V * P + 1) && rf->d_stat.reserve(RF_S_COUNT);
  ok = ok && (!n_short || hipMemcpy(rf->d_short, g->rf_short.data(), 4ull * n_short, hipMemcpyHostToDevice) == hipSuccess) &&
       (!n_long || hipMemcpy(rf->d_long, g->rf_long.data(), 4ull * n_long, hipMemcpyHostToDevice) == hipSuccess);
  if (!ok) {
    (void)hipGetLastError();
    delete rf;
    set_err(g->ctx, std::string(who) + ": device allocation failed");
    return nullptr;
  }
  return g->rf = rf;
}

// the device sequence behind both doors; C.T or C.keys / pops / counts are device arrays
static int refresh_run(grim_graph *g, const char *who, RfCounts C, grim_refresh_stats *stats) {
  grim_ctx *c = g->ctx;
  hipStream_t st = c->stream;
  const std::string name(who);
  const DevGraph &D = g->d;
  const uint32_t V = D.n_nodes, P = D.P, F = g->n_full;
  const uint32_t n_short = (uint32_t)g->rf_short.size(), n_long = (uint32_t)g->rf_long.size();
  const uint32_t n_blocks = (F + GRIM_REFRESH_BLOCK - 1) / GRIM_REFRESH_BLOCK;
  grim_refresh_stats out;
  memset(&out, 0, sizeof(out));
  out.n_full = F;
  HIPCHK(hipStreamSynchronize(st), c, -1);
  if (!refresh_state(g, who)) return -1;
  RefreshState &R = *g->rf;
  const uint32_t *full = D.lab_nodes + g->full_first;
  const size_t lds = sizeof(double) * RF_CHUNK * P + sizeof(uint32_t) * RF_CHUNK;
  // ---- everything into the shadow ---------------------------------------------------------------------------------------
  HIPCHK(hipMemsetAsync(R.d_stat, 0, 8 * RF_S_COUNT, st), c, -1);
  HIPCHK(hipMemsetAsync(R.d_total, 0, 8 * GRIM_MAXPOP, st), c, -1);
  HIPCHK(hipEventRecord(R.ev[0], st), c, -1);
  if (F) {
    const uint32_t n_fp = (uint32_t)(((uint64_t)F * P + 255) / 256);
    hipLaunchKernelGGL(rf_lookup_kernel, dim3(n_fp), dim3(256), 0, st, full, F, V, P, D.node_key, C, R.d_c, R.d_stat);
    hipLaunchKernelGGL(rf_blocksum_kernel, dim3(n_blocks), dim3(64), lds, st, R.d_c, F, P, R.d_bsum);
    hipLaunchKernelGGL(rf_total_kernel, dim3(1), dim3(64), 0, st, R.d_bsum, n_blocks, P, R.d_total);
    hipLaunchKernelGGL(rf_divide_kernel, dim3((F + 255) / 256), dim3(256), 0, st, full, F, V, P, R.d_c, R.d_total, D.freq, R.d_shadow,
                       R.d_stat);
    if (n_short)
      hipLaunchKernelGGL(rf_short_kernel, dim3((uint32_t)(((uint64_t)n_short * P + 255) / 256)), dim3(256), 0, st, R.d_short, n_short, V, P,
                         D.a_start, D.a_nbr, g->n_a_nbr, R.d_shadow, R.d_stat);
    if (n_long)
      hipLaunchKernelGGL(rf_long_kernel, dim3(n_long), dim3(64), lds, st, R.d_long, n_long, V, P, D.a_start, D.a_nbr, g->n_a_nbr,
                         R.d_shadow, R.d_stat);
    HIPCHK(hipGetLastError(), c, -1);
  }
  HIPCHK(hipEventRecord(R.ev[1], st), c, -1);
  HIPCHK(hipMemcpyAsync(out.total, R.d_total, 8 * P, hipMemcpyDeviceToHost, st), c, -1);
  uint64_t h[RF_S_COUNT];
  if (read_stat<RF_S_COUNT, 1>(c, R.d_stat, h) != 0) return -1;
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, R.ev[0], R.ev[1]), c, -1);
  g->refresh_ms = ms;
  if (h[RF_S_FAULT]) {
    set_err(c, name + ": a top-link row or the full-node list does not lie inside the graph (internal)");
    return -1;
  }
  for (uint32_t p = 0; p < P; ++p)
    if (!(out.total[p] > 0.0 && out.total[p] <= 1.7976931348623157e308)) {  // finite and > 0 (false for a NaN)
      if (stats) *stats = out;
      set_err(c, name + ": population " + std::to_string(p) + " has no count inside the support (its total is not finite or not > 0)");
      return -3;
    }
  // ---- commit: in place, at the addresses every batch and stream of the graph holds ---------------------------------------
  HIPCHK(hipEventRecord(R.ev[2], st), c, -1);
  HIPCHK(hipMemcpyAsync(const_cast<double *>(D.freq), R.d_shadow, 8ull * V * P, hipMemcpyDeviceToDevice, st), c, -1);
  hipLaunchKernelGGL(rf_fht_kernel, dim3((F + 255) / 256), dim3(256), 0, st, full, F, V, P, D.node_key, D.ht, D.ht_mask,
                     const_cast<FullEnt *>(D.fht), D.fht_mask, D.freq);
  HIPCHK(hipGetLastError(), c, -1);
  HIPCHK(hipEventRecord(R.ev[3], st), c, -1);
  HIPCHK(hipStreamSynchronize(st), c, -1);
  HIPCHK(hipEventElapsedTime(&ms, R.ev[2], R.ev[3]), c, -1);
  g->refresh_ms += ms;
  out.matched = h[RF_S_MATCHED];
  out.zero_full = h[RF_S_ZERO_FULL];
  memcpy(&out.delta, &h[RF_S_DELTA], 8);
  if (stats) *stats = out;
  return 0;
}

extern "C" int grim_graph_refresh(grim_graph *g, grim_em *e, grim_refresh_stats *stats) {
  if (!g || !e) return -1;
  grim_ctx *c = g->ctx;
  const char *who = "grim_graph_refresh";
  if (stats) memset(stats, 0, sizeof(*stats));
  if (!g->refreshable) return refuse(c, who, ("the graph is not refreshable: " + g->refresh_why).c_str()), -3;
  if (e->ctx != c) return refuse(c, who, "the accumulator belongs to another context"), -3;
  if (e->T.P != g->d.P) return refuse(c, who, "the accumulator has another number of populations"), -3;
  use_device(c->device);
  RfCounts C;
  memset(&C, 0, sizeof(C));
  C.T = e->T;
  return refresh_run(g, who, C, stats);
}

extern "C" int grim_graph_refresh_records(grim_graph *g, const uint64_t *keys, const uint32_t *pops, const double *counts, uint64_t n,
                                          grim_refresh_stats *stats) {
  if (!g) return -1;
  grim_ctx *c = g->ctx;
  const char *who = "grim_graph_refresh_records";
  if (stats) memset(stats, 0, sizeof(*stats));
  if (!g->refreshable) return refuse(c, who, ("the graph is not refreshable: " + g->refresh_why).c_str()), -3;
  if (!counts_door(c, who, "the graph's", g->d.P, nullptr, keys, pops, counts, n, nullptr)) return -3;
  use_device(c->device);
  if (!refresh_state(g, who)) return -1;
  RefreshState &R = *g->rf;
  if (R.in.upload(c, who, keys, pops, counts, n) != 0) return -1;
  RfCounts C;
  memset(&C, 0, sizeof(C));
  C.records = 1;
  C.keys = R.in.keys;
  C.pops = R.in.pops;
  C.counts = R.in.counts;
  C.n = n;
  return refresh_run(g, who, C, stats);
}

extern "C" int grim_graph_freq(grim_graph *g, double *out) {
  if (!g || !out) return -1;
  grim_ctx *c = g->ctx;
  use_device(c->device);
  HIPCHK(hipStreamSynchronize(c->stream), c, -1);
  HIPCHK(hipMemcpy(out, g->d.freq, 8ull * g->d.n_nodes * g->d.P, hipMemcpyDeviceToHost), c, -1);
  return 0;
}

extern "C" double grim_graph_refresh_ms(const grim_graph *g) { return g ? g->refresh_ms : 0.0; }
extern "C" int grim_graph_refreshable(const grim_graph *g) { return g && g->refreshable ? 1 : 0; }

// =================================================================================================
// Allele groups (grim_groups.h): the rows mapped to a chosen resolution in front of the consumers below
// =================================================================================================
struct grim_groups {
  grim_ctx *ctx;
  GpMap M;  // M.tab = d_tab
  uint32_t watch_mask;
  bool staged;
  DevBuf<uint16_t> d_tab;
  DevBuf<grim_row> d_in, d_out;  // of grim_groups_map_records
  Events<2> ev;
  double last_ms;
};

// what a consumer keeps of a group map: its own copy of the tables (its lifetime does not depend on the grim_groups) and the
// buffer the mapped rows go to
struct GpAttach {
  bool on = false, staged = false;
  GpMap M = {};
  uint32_t watch_mask = 0;
  DevBuf<uint16_t> tab;
  DevBuf<grim_row> mapped;
  void detach() { on = false; }
  // the tables of g, device to device; ends in a stream synchronise
  int attach(grim_ctx *c, const char *who, const grim_groups *g) {
    on = false;
    if (!tab.reserve((uint64_t)g->M.total + 1)) {  // never an empty allocation
      set_err(c, std::string(who) + ": device allocation failed");
      return -1;
    }
    HIPCHK(hipMemcpyAsync(tab, g->d_tab, sizeof(uint16_t) * (uint64_t)g->M.total, hipMemcpyDeviceToDevice, c->stream), c, -1);
    HIPCHK(hipStreamSynchronize(c->stream), c, -1);
    M = g->M;
    M.tab = tab;
    watch_mask = g->watch_mask;
    staged = g->staged;
    on = true;
    return 0;
  }
  EmLimits limits() const {
    EmLimits L;
    for (int q = 0; q < GRIM_MAXL; ++q) L.n_alleles[q] = M.n_groups[q];
    return L;
  }
};

// rows[0 .. rows_used) through the map into out (device arrays of at least rows_used rows, 16-byte aligned); enqueues only
static bool gp_launch(hipStream_t st, const GpMap &M, bool staged, const grim_row *rows, uint32_t rows_used, grim_row *out) {
  if (rows_used == 0) return true;
  if (((uintptr_t)rows | (uintptr_t)out) & 15u) return false;
  const uint32_t need = (rows_used + GP_THREADS - 1) / GP_THREADS, blocks = need < GP_MAX_BLOCKS ? need : GP_MAX_BLOCKS;
  if (staged)
    hipLaunchKernelGGL(gp_map_kernel<true>, dim3(blocks), dim3(GP_THREADS), 0, st, rows, rows_used, M, out);
  else
    hipLaunchKernelGGL(gp_map_kernel<false>, dim3(blocks), dim3(GP_THREADS), 0, st, rows, rows_used, M, out);
  return true;
}

// a consumer's rows through its map into its own buffer; rows then names the mapped rows.  Reserves before it launches.
static int gp_map_rows(grim_ctx *c, const char *who, GpAttach &A, const grim_row *&rows, uint32_t rows_used) {
  if (!A.mapped.reserve((uint64_t)rows_used + 1, rows_used / 4)) {  // never an empty allocation
    set_err(c, std::string(who) + ": device allocation failed");
    return -1;
  }
  if (!gp_launch(c->stream, A.M, A.staged, rows, rows_used, A.mapped)) {
    set_err(c, std::string(who) + ": the rows are not 16-byte aligned (internal)");
    return -1;
  }
  HIPCHK(hipGetLastError(), c, -1);
  rows = A.mapped;
  return 0;
}

extern "C" grim_groups *grim_groups_create(grim_ctx *c, const uint16_t *table, const uint32_t n_alleles[GRIM_MAXL],
                                           const uint32_t n_groups[GRIM_MAXL]) {
  if (!c || !table || !n_alleles || !n_groups) {
    set_err(c, "grim_groups_create: bad arguments");
    return nullptr;
  }
  const std::string who = "grim_groups_create: slot ";
  GpMap M = {};
  uint32_t watch = 0;
  for (int q = 0; q < GRIM_MAXL; ++q) {  // the sizes first: nothing of a table is read before they are known to be sane
    if (n_alleles[q] > 4095u) {
      set_err(c, who + std::to_string(q) + ": n_alleles " + std::to_string(n_alleles[q]) + " is above 4095");
      return nullptr;
    }
    if (n_groups[q] > n_alleles[q]) {
      set_err(c, who + std::to_string(q) + ": n_groups " + std::to_string(n_groups[q]) + " is above n_alleles " + std::to_string(n_alleles[q]));
      return nullptr;
    }
    M.off[q] = M.total;
    M.n_alleles[q] = n_alleles[q];
    M.n_groups[q] = n_groups[q];
    M.total += n_alleles[q] + 1u;
  }
  for (int q = 0; q < GRIM_MAXL; ++q) {
    const uint16_t *T = table + M.off[q];
    if (T[0] != 0) {
      set_err(c, who + std::to_string(q) + ", entry 0: " + std::to_string(T[0]) + ", not 0 (untyped stays untyped)");
      return nullptr;
    }
    std::vector<uint8_t> used(n_groups[q] + 1u, 0);
    for (uint32_t f = 1; f <= n_alleles[q]; ++f) {
      if (T[f] == 0 || T[f] > n_groups[q]) {
        set_err(c, who + std::to_string(q) + ", entry " + std::to_string(f) + ": group " + std::to_string(T[f]) + " is not in 1.." +
                       std::to_string(n_groups[q]));
        return nullptr;
      }
      used[T[f]] = 1;
      if (T[f] != f) watch |= 1u << q;
    }
    for (uint32_t gid = 1; gid <= n_groups[q]; ++gid)
      if (!used[gid]) {
        set_err(c, who + std::to_string(q) + ": group " + std::to_string(gid) + " is used by no entry");
        return nullptr;
      }
  }
  bool staged = true;  // measured (profiles/groups_notes.md): every workgroup stages the tables in LDS
  if (const char *e = getenv("GRIM_GROUPS_LDS")) staged = e[0] != '0';  // for the bench: 0 reads the tables where they lie
  use_device(c->device);
  grim_groups *g = new grim_groups();
  g->ctx = c;
  g->M = M;
  g->watch_mask = watch;
  g->staged = staged;
  if (!g->d_tab.reserve((uint64_t)M.total + 1) || !g->ev.create()) {  // never an empty allocation
    (void)hipGetLastError();
    set_err(c, "grim_groups_create: device allocation failed");
    grim_groups_free(g);
    return nullptr;
  }
  g->M.tab = g->d_tab;
  if (hipMemcpyAsync(g->d_tab, table, sizeof(uint16_t) * (uint64_t)M.total, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess) {
    (void)hipGetLastError();
    set_err(c, "grim_groups_create: the upload of the tables failed");
    grim_groups_free(g);
    return nullptr;
  }
  return g;
}

extern "C" void grim_groups_free(grim_groups *g) {
  if (!g) return;
  use_device(g->ctx->device);
  hipStreamSynchronize(g->ctx->stream);
  delete g;
}

extern "C" uint32_t grim_groups_watch_mask(const grim_groups *g) { return g ? g->watch_mask : 0; }
extern "C" double grim_groups_kernel_ms(const grim_groups *g) { return g ? g->last_ms : 0.0; }

extern "C" int grim_groups_map_records(grim_groups *g, const grim_row *rows, uint64_t n_rows, grim_row *out) {
  if (!g) return -1;
  grim_ctx *c = g->ctx;
  g->last_ms = 0.0;
  if ((n_rows && (!rows || !out)) || n_rows > 0x7FFFFFFFull) {
    set_err(c, "grim_groups_map_records: bad arguments");
    return -3;
  }
  if (n_rows == 0) return 0;
  use_device(c->device);
  hipStream_t st = c->stream;
  if (!reserve_all(n_rows + 1, 0, g->d_in, g->d_out)) {  // never an empty allocation
    set_err(c, "grim_groups_map_records: device allocation failed");
    return -1;
  }
  HIPCHK(hipMemcpyAsync(g->d_in, rows, sizeof(grim_row) * n_rows, hipMemcpyHostToDevice, st), c, -1);
  HIPCHK(hipEventRecord(g->ev[0], st), c, -1);
  if (!gp_launch(st, g->M, g->staged, g->d_in, (uint32_t)n_rows, g->d_out)) return -1;
  HIPCHK(hipGetLastError(), c, -1);
  HIPCHK(hipEventRecord(g->ev[1], st), c, -1);
  HIPCHK(hipMemcpyAsync(out, g->d_out, sizeof(grim_row) * n_rows, hipMemcpyDeviceToHost, st), c, -1);
  HIPCHK(hipStreamSynchronize(st), c, -1);
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, g->ev[0], g->ev[1]), c, -1);
  g->last_ms = ms;
  return 0;
}

// =================================================================================================
// Marginal genotype tables (grim_marginal.h): the UMUG rows of a finished batch reduced to a subset of the loci
// =================================================================================================
struct grim_marginal {
  grim_ctx *ctx;
  uint32_t keep_mask, max_rows;
  DevBuf<unsigned long long> d_stat;
  // region starts per subject; scratch (MgScratch), output rows and result copies; the uploaded records of
  // grim_marginal_reduce_records
  DevBuf<uint32_t> d_first, g_lead;
  DevBuf<uint64_t> g_lo, g_hi;
  DevBuf<double> g_prob, g_sum;
  DevBuf<grim_row> d_orows;
  DevBuf<grim_subject_result> d_ores;
  RecordsUpload in;
  GpAttach gp;  // the group map attached (grim_marginal_set_groups) and the subjects' GRIM_GROUPS_PRIVATE flags
  DevBuf<uint8_t> d_flags;
  bool have_flags;  // the last reduce ran with a map attached
  // the last reduce
  uint32_t n_subj, n_rows;
  uint64_t stat[5];
  Events<2> ev;
  double last_ms;
};

extern "C" grim_marginal *grim_marginal_create(grim_ctx *c, uint32_t keep_mask, uint32_t max_rows) {
  if (!c || max_rows == 0) {
    set_err(c, "grim_marginal_create: bad arguments");
    return nullptr;
  }
  use_device(c->device);
  grim_marginal *m = new grim_marginal();
  m->ctx = c;
  m->keep_mask = keep_mask;
  m->max_rows = max_rows;
  if (!m->d_stat.reserve(MG_S_COUNT * MG_S_SLICES) || !m->ev.create()) {
    (void)hipGetLastError();
    set_err(c, "grim_marginal_create: device allocation failed");
    grim_marginal_free(m);
    return nullptr;
  }
  return m;
}

extern "C" void grim_marginal_free(grim_marginal *m) {
  if (!m) return;
  use_device(m->ctx->device);
  hipStreamSynchronize(m->ctx->stream);
  delete m;
}

static void mg_clear(grim_marginal *m) {
  m->n_subj = m->n_rows = 0;
  m->have_flags = false;
  for (uint64_t &x : m->stat) x = 0;
  m->last_ms = 0.0;
}

// the three launches on n subjects whose rows lie in [0, rows_used) of `rows` (device arrays)
static int mg_run(grim_marginal *m, const char *who, const grim_subject_result *res, const grim_row *rows, uint32_t n, uint32_t rows_used) {
  grim_ctx *c = m->ctx;
  hipStream_t st = c->stream;
  if (n == 0) return 0;
  if (!m->d_first.reserve((uint64_t)n + 1) || !m->d_ores.reserve(n) ||
      !reserve_all(rows_used, rows_used / 4, m->g_lo, m->g_hi, m->g_prob, m->g_sum, m->g_lead, m->d_orows)) {
    set_err(c, std::string(who) + ": device allocation failed");
    return -1;
  }
  const bool grouped = m->gp.on;
  if (grouped && (!m->d_flags.reserve((uint64_t)n + 1) || !m->gp.mapped.reserve((uint64_t)rows_used + 1, rows_used / 4))) {
    set_err(c, std::string(who) + ": device allocation failed");
    return -1;
  }
  const MgScratch G = {m->g_lo, m->g_hi, m->g_prob, m->g_sum, m->g_lead};
  HIPCHK(hipMemsetAsync(m->d_stat, 0, 8 * MG_S_COUNT * MG_S_SLICES, st), c, -1);
  if (rows_used) HIPCHK(hipMemsetAsync(m->d_orows, 0, sizeof(grim_row) * (uint64_t)rows_used, st), c, -1);  // what a region does not use reads as zeros
  HIPCHK(hipEventRecord(m->ev[0], st), c, -1);
  if (grouped) {  // the flags from the rows as they came, then the rows through the map: the kernels below see the mapped rows
    EmLimits L;
    for (int q = 0; q < GRIM_MAXL; ++q) L.n_alleles[q] = m->gp.M.n_alleles[q];
    hipLaunchKernelGGL(gp_flag_kernel, dim3((n + 3) / 4), dim3(256), 0, st, res, rows, n, rows_used, L, m->keep_mask & m->gp.watch_mask,
                       m->d_flags);
    if (gp_map_rows(c, who, m->gp, rows, rows_used) != 0) return -1;
  }
  hipLaunchKernelGGL(mg_count_kernel, dim3((n + 255) / 256), dim3(256), 0, st, res, n, rows_used, m->d_first);
  hipLaunchKernelGGL(em_scan_kernel, dim3(1), dim3(1024), 0, st, m->d_first, n);
  hipLaunchKernelGGL(mg_reduce_kernel, dim3(n), dim3(64), 0, st, res, rows, n, rows_used, m->d_first, rows_used, m->keep_mask, m->max_rows,
                     G, m->d_ores, m->d_orows, m->d_stat);
  HIPCHK(hipGetLastError(), c, -1);
  HIPCHK(hipEventRecord(m->ev[1], st), c, -1);
  uint32_t total = 0;
  uint64_t h[MG_S_COUNT];
  HIPCHK(hipMemcpyAsync(&total, m->d_first + n, 4, hipMemcpyDeviceToHost, st), c, -1);
  if (read_stat<MG_S_COUNT, MG_S_SLICES>(c, m->d_stat, h) != 0) return -1;
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, m->ev[0], m->ev[1]), c, -1);
  if (total > rows_used || h[MG_S_ROWS_IN] != total) {  // regions that overlap: the kernel left those that did not fit alone
    set_err(c, std::string(who) + ": the subjects' genotype rows overlap (more rows than there are)");
    return -1;
  }
  m->last_ms = ms;
  m->n_subj = n;
  m->n_rows = total;
  m->have_flags = grouped;
  for (int k = 0; k < 5; ++k) m->stat[k] = h[k];
  return 0;
}

extern "C" int grim_marginal_reduce(grim_marginal *m, grim_batch *b) {
  if (!m || !b) return -1;
  grim_ctx *c = m->ctx;
  mg_clear(m);
  if (!batch_door(c, "grim_marginal_reduce", b, m->keep_mask, 0)) return -3;
  use_device(c->device);
  return mg_run(m, "grim_marginal_reduce", b->a.res, b->a.rows, b->n_subj, b->rows_used);
}

extern "C" int grim_marginal_reduce_records(grim_marginal *m, const grim_subject_result *res, uint32_t n_subjects, const grim_row *rows,
                                            uint64_t n_rows) {
  if (!m) return -1;
  grim_ctx *c = m->ctx;
  mg_clear(m);
  if (!records_door(c, "grim_marginal_reduce_records", m->keep_mask, res, n_subjects, rows, n_rows)) return -3;
  use_device(c->device);
  if (n_subjects == 0) return 0;
  if (m->in.upload(c, "grim_marginal_reduce_records", res, n_subjects, rows, (uint32_t)n_rows) != 0) return -1;
  return mg_run(m, "grim_marginal_reduce_records", m->in.res, m->in.rows, n_subjects, (uint32_t)n_rows);
}

extern "C" uint32_t grim_marginal_subjects(const grim_marginal *m) { return m ? m->n_subj : 0; }
extern "C" uint32_t grim_marginal_total_rows(const grim_marginal *m) { return m ? m->n_rows : 0; }
extern "C" double grim_marginal_kernel_ms(const grim_marginal *m) { return m ? m->last_ms : 0.0; }

extern "C" int grim_marginal_results(grim_marginal *m, grim_subject_result *res, grim_row *rows) {
  if (!m || (m->n_subj && !res) || (m->n_rows && !rows)) return -1;
  grim_ctx *c = m->ctx;
  use_device(c->device);
  if (m->n_subj) HIPCHK(hipMemcpy(res, m->d_ores, sizeof(grim_subject_result) * (size_t)m->n_subj, hipMemcpyDeviceToHost), c, -1);
  if (m->n_rows) HIPCHK(hipMemcpy(rows, m->d_orows, sizeof(grim_row) * (size_t)m->n_rows, hipMemcpyDeviceToHost), c, -1);
  return 0;
}

extern "C" int grim_marginal_set_groups(grim_marginal *m, const grim_groups *g) {
  if (!m) return -1;
  grim_ctx *c = m->ctx;
  mg_clear(m);
  m->gp.detach();
  if (!g) return 0;
  if (g->ctx != c) {
    set_err(c, "grim_marginal_set_groups: the groups belong to another context");
    return -3;
  }
  use_device(c->device);
  return m->gp.attach(c, "grim_marginal_set_groups", g);
}

extern "C" int grim_marginal_flags(grim_marginal *m, uint8_t *out) {
  if (!m || (m->n_subj && !out)) return -1;
  grim_ctx *c = m->ctx;
  if (!m->n_subj) return 0;
  if (!m->have_flags) {
    memset(out, 0, m->n_subj);
    return 0;
  }
  use_device(c->device);
  HIPCHK(hipMemcpy(out, m->d_flags, m->n_subj, hipMemcpyDeviceToHost), c, -1);
  return 0;
}

extern "C" int grim_marginal_stats(const grim_marginal *m, uint64_t out[5]) {
  if (!m || !out) return -1;
  for (int k = 0; k < 5; ++k) out[k] = m->stat[k];
  return 0;
}

// =================================================================================================
// Match probabilities (grim_match.h): the UMUG rows of patients against those of a finished batch of donors
// =================================================================================================
struct MtBuf {  // one side on the device
  DevBuf<uint32_t> first;
  DevBuf<uint64_t> a, b;
  DevBuf<double> w;
  DevBuf<uint8_t> flags;
  uint32_t n;  // subjects of the side
  MtSide side() const { return {first, a, b, w, flags}; }
};

struct grim_match {
  grim_ctx *ctx;
  uint32_t keep_mask;
  uint32_t direction;  // GRIM_MATCH_DIR_*
  bool graded;         // records are grim_match_grade_rec
  EmLimits lim;
  DevBuf<unsigned long long> d_stat;
  MtBuf P, D;
  // the uploaded records of grim_match_set_patients and of grim_match_run_records (one pair of buffers: mt_prepare copies
  // what a side needs out of them); the result records
  RecordsUpload in;
  GpAttach gp;  // the group map attached (grim_match_set_groups): both sides' rows go through it before mt_prepare_kernel
  DevBuf<double> d_out;
  bool have_patients;
  uint64_t pstat[MT_S_COUNT];  // what preparing the patients counted
  // the last run
  uint32_t n_donors;
  uint64_t stat[8];
  Events<2> ev;
  double last_ms;
};

static_assert(MT_DIR_EITHER == GRIM_MATCH_DIR_EITHER && MT_DIR_GVH == GRIM_MATCH_DIR_GVH && MT_DIR_HVG == GRIM_MATCH_DIR_HVG,
              "the directions of grim_match.h and of grim_hip.h have drifted apart");
static_assert(sizeof(grim_match_rec) == 8 * MT_REC && sizeof(grim_match_grade_rec) == 8 * MT_GRADE_REC,
              "the match records and the kernels' bin counts have drifted apart");

extern "C" grim_match *grim_match_create_ex(grim_ctx *c, uint32_t keep_mask, const uint32_t n_alleles[GRIM_MAXL], uint32_t direction,
                                            int graded) {
  if (!c || !n_alleles) {
    set_err(c, "grim_match_create: bad arguments");
    return nullptr;
  }
  if (direction > GRIM_MATCH_DIR_HVG) {
    set_err(c, "grim_match_create: direction must be GRIM_MATCH_DIR_EITHER, _GVH or _HVG");
    return nullptr;
  }
  use_device(c->device);
  grim_match *m = new grim_match();
  m->ctx = c;
  m->keep_mask = keep_mask;
  m->direction = direction;
  m->graded = graded != 0;
  for (int q = 0; q < GRIM_MAXL; ++q) m->lim.n_alleles[q] = n_alleles[q];
  if (!m->d_stat.reserve(MT_S_COUNT * MT_S_SLICES) || !m->ev.create()) {
    (void)hipGetLastError();
    set_err(c, "grim_match_create: device allocation failed");
    grim_match_free(m);
    return nullptr;
  }
  return m;
}

extern "C" grim_match *grim_match_create(grim_ctx *c, uint32_t keep_mask, const uint32_t n_alleles[GRIM_MAXL]) {
  return grim_match_create_ex(c, keep_mask, n_alleles, GRIM_MATCH_DIR_EITHER, 0);
}

extern "C" uint32_t grim_match_direction(const grim_match *m) { return m ? m->direction : 0; }
extern "C" int grim_match_graded(const grim_match *m) { return m && m->graded ? 1 : 0; }

extern "C" void grim_match_free(grim_match *m) {
  if (!m) return;
  use_device(m->ctx->device);
  hipStreamSynchronize(m->ctx->stream);
  delete m;
}

// no results: what a refusal leaves behind (the patients stay as they are)
static void mt_clear(grim_match *m) {
  m->n_donors = 0;
  for (uint64_t &x : m->stat) x = 0;
  m->last_ms = 0.0;
}

static void mt_drop_patients(grim_match *m) {
  m->have_patients = false;
  m->P.n = 0;
  for (uint64_t &x : m->pstat) x = 0;
}

// count, scan, prepare: n subjects whose rows lie in [0, rows_used) of `rows` (device arrays) into side S; enqueues only
static int mt_prepare(grim_match *m, const char *who, MtBuf &S, uint32_t side, const grim_subject_result *res, const grim_row *rows,
                      uint32_t n, uint32_t rows_used) {
  grim_ctx *c = m->ctx;
  hipStream_t st = c->stream;
  if (!reserve_all((uint64_t)n + 1, 0, S.first, S.flags) ||
      !reserve_all((uint64_t)rows_used + 1, rows_used / 4, S.a, S.b, S.w)) {  // never an empty allocation
    set_err(c, std::string(who) + ": device allocation failed");
    return -1;
  }
  if (m->gp.on && gp_map_rows(c, who, m->gp, rows, rows_used) != 0) return -1;  // n_groups then stands where n_alleles stood
  hipLaunchKernelGGL(mg_count_kernel, dim3((n + 255) / 256), dim3(256), 0, st, res, n, rows_used, S.first);
  hipLaunchKernelGGL(em_scan_kernel, dim3(1), dim3(1024), 0, st, S.first, n);
  hipLaunchKernelGGL(mt_prepare_kernel, dim3((n + 3) / 4), dim3(256), 0, st, res, rows, n, rows_used, S.first, rows_used, m->keep_mask,
                     m->gp.on ? m->gp.limits() : m->lim, side, S.a, S.b, S.w, S.flags, m->d_stat);
  HIPCHK(hipGetLastError(), c, -1);
  return 0;
}

extern "C" int grim_match_set_patients(grim_match *m, const grim_subject_result *res, uint32_t n, const grim_row *rows, uint32_t n_rows) {
  if (!m) return -1;
  grim_ctx *c = m->ctx;
  mt_clear(m);
  mt_drop_patients(m);
  if (!records_door(c, "grim_match_set_patients", m->keep_mask, res, n, rows, n_rows)) return -3;
  if ((uint64_t)n > GRIM_MATCH_MAX_PAIRS) {
    set_err(c, "grim_match_set_patients: more patients than GRIM_MATCH_MAX_PAIRS");
    return -3;
  }
  use_device(c->device);
  if (n) {
    if (m->in.upload(c, "grim_match_set_patients", res, n, rows, n_rows) != 0) return -1;
    HIPCHK(hipMemsetAsync(m->d_stat, 0, 8 * MT_S_COUNT * MT_S_SLICES, c->stream), c, -1);
    if (mt_prepare(m, "grim_match_set_patients", m->P, 0u, m->in.res, m->in.rows, n, n_rows) != 0) return -1;
    uint32_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, m->P.first + n, 4, hipMemcpyDeviceToHost, c->stream), c, -1);
    if (read_stat<MT_S_COUNT, MT_S_SLICES>(c, m->d_stat, m->pstat) != 0) return -1;
    if (total > n_rows) {  // regions that overlap: the kernel left those that did not fit alone
      mt_drop_patients(m);
      set_err(c, "grim_match_set_patients: the subjects' genotype rows overlap (more rows than there are)");
      return -1;
    }
  }
  m->P.n = n;
  m->have_patients = true;
  return 0;
}

extern "C" int grim_match_set_groups(grim_match *m, const grim_groups *g) {
  if (!m) return -1;
  grim_ctx *c = m->ctx;
  mt_clear(m);
  mt_drop_patients(m);  // rows prepared at one resolution never meet donors at another
  m->gp.detach();
  if (!g) return 0;
  if (g->ctx != c) {
    set_err(c, "grim_match_set_groups: the groups belong to another context");
    return -3;
  }
  for (int q = 0; q < GRIM_MAXL; ++q)
    if (g->M.n_alleles[q] != m->lim.n_alleles[q]) {
      set_err(c, "grim_match_set_groups: slot " + std::to_string(q) + ": the groups' n_alleles differ from the ones given at create");
      return -3;
    }
  use_device(c->device);
  return m->gp.attach(c, "grim_match_set_groups", g);
}

// the pair kernel's six instances, at direction * 2 + graded (grim_match_create_ex refuses a direction above _HVG)
template <int DIR, bool GRADED>
static void mt_launch(hipStream_t st, const MtSide &P, uint32_t n_p, uint32_t p0, uint32_t np, const MtSide &D, uint32_t n,
                      uint32_t keep_mask, double *out, unsigned long long *stat) {
  hipLaunchKernelGGL((mt_pair_kernel<DIR, GRADED>), dim3(n, np), dim3(64), 0, st, P, n_p, p0, D, n, keep_mask, out, stat);
}
static constexpr decltype(&mt_launch<MT_DIR_EITHER, false>) MT_LAUNCH[] = {
    mt_launch<MT_DIR_EITHER, false>, mt_launch<MT_DIR_EITHER, true>, mt_launch<MT_DIR_GVH, false>,
    mt_launch<MT_DIR_GVH, true>,     mt_launch<MT_DIR_HVG, false>,   mt_launch<MT_DIR_HVG, true>};
static_assert(sizeof(MT_LAUNCH) / sizeof(MT_LAUNCH[0]) == 2 * (GRIM_MATCH_DIR_HVG + 1),
              "one instance for every direction grim_match_create_ex lets in, ungraded and graded");

static uint32_t mt_rec_doubles(const grim_match *m) { return m->graded ? MT_GRADE_REC : MT_REC; }

// donors (device arrays) against the patients set
static int mt_run(grim_match *m, const char *who, const grim_subject_result *res, const grim_row *rows, uint32_t n, uint32_t rows_used) {
  grim_ctx *c = m->ctx;
  hipStream_t st = c->stream;
  if (n == 0) return 0;
  const uint32_t n_p = m->P.n;
  const uint64_t pairs = (uint64_t)n_p * n;
  const uint64_t rec = mt_rec_doubles(m);
  if (!m->d_out.reserve((pairs + 1) * rec)) {  // never an empty allocation
    set_err(c, std::string(who) + ": device allocation failed");
    return -1;
  }
  HIPCHK(hipMemsetAsync(m->d_stat, 0, 8 * MT_S_COUNT * MT_S_SLICES, st), c, -1);
  HIPCHK(hipEventRecord(m->ev[0], st), c, -1);
  if (mt_prepare(m, who, m->D, 1u, res, rows, n, rows_used) != 0) return -1;
  if (pairs) {
    HIPCHK(hipMemsetAsync(m->d_out, 0, sizeof(double) * rec * pairs, st), c, -1);  // a pair that is not computed reads as zero bytes
    const MtSide P = m->P.side(), D = m->D.side();
    const auto launch = MT_LAUNCH[m->direction * 2u + (m->graded ? 1u : 0u)];
    for_slabs(n_p, [&](uint32_t p0, uint32_t np) {
      launch(st, P, n_p, p0, np, D, n, m->keep_mask, m->d_out, m->d_stat);
    });
    HIPCHK(hipGetLastError(), c, -1);
  }
  HIPCHK(hipEventRecord(m->ev[1], st), c, -1);
  uint32_t total = 0;
  uint64_t h[MT_S_COUNT];
  HIPCHK(hipMemcpyAsync(&total, m->D.first + n, 4, hipMemcpyDeviceToHost, st), c, -1);
  if (read_stat<MT_S_COUNT, MT_S_SLICES>(c, m->d_stat, h) != 0) return -1;
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, m->ev[0], m->ev[1]), c, -1);
  if (total > rows_used) {
    set_err(c, std::string(who) + ": the subjects' genotype rows overlap (more rows than there are)");
    return -1;
  }
  m->last_ms = ms;
  m->n_donors = n;
  for (int k = 0; k < 8; ++k) m->stat[k] = k < MT_S_COUNT ? h[k] + m->pstat[k] : 0;
  return 0;
}

static bool mt_pairs_ok(grim_match *m, const char *who, uint32_t n) {
  if (!m->have_patients) return refuse(m->ctx, who, "no patients set (call grim_match_set_patients first)");
  if ((uint64_t)m->P.n * n > GRIM_MATCH_MAX_PAIRS) return refuse(m->ctx, who, "patients x donors above GRIM_MATCH_MAX_PAIRS");
  return true;
}

extern "C" int grim_match_run(grim_match *m, grim_batch *b) {
  if (!m || !b) return -1;
  grim_ctx *c = m->ctx;
  mt_clear(m);
  if (!batch_door(c, "grim_match_run", b, m->keep_mask, 0)) return -3;
  if (!mt_pairs_ok(m, "grim_match_run", b->n_subj)) return -3;
  use_device(c->device);
  return mt_run(m, "grim_match_run", b->a.res, b->a.rows, b->n_subj, b->rows_used);
}

extern "C" int grim_match_run_records(grim_match *m, const grim_subject_result *res, uint32_t n, const grim_row *rows, uint32_t n_rows) {
  if (!m) return -1;
  mt_clear(m);
  if (!records_door(m->ctx, "grim_match_run_records", m->keep_mask, res, n, rows, n_rows)) return -3;
  if (!mt_pairs_ok(m, "grim_match_run_records", n)) return -3;
  use_device(m->ctx->device);
  if (n == 0) return 0;
  if (m->in.upload(m->ctx, "grim_match_run_records", res, n, rows, n_rows) != 0) return -1;
  return mt_run(m, "grim_match_run_records", m->in.res, m->in.rows, n, n_rows);
}

extern "C" uint32_t grim_match_patients(const grim_match *m) { return m ? m->P.n : 0; }
extern "C" uint32_t grim_match_donors(const grim_match *m) { return m ? m->n_donors : 0; }
extern "C" double grim_match_kernel_ms(const grim_match *m) { return m ? m->last_ms : 0.0; }

// the records (of `bytes` each) and the flags of the last run
static int mt_results(grim_match *m, void *out, size_t bytes, uint8_t *patient_flags, uint8_t *donor_flags) {
  grim_ctx *c = m->ctx;
  use_device(c->device);
  const uint64_t pairs = (uint64_t)m->P.n * m->n_donors;
  if (out && pairs) HIPCHK(hipMemcpy(out, m->d_out, bytes * pairs, hipMemcpyDeviceToHost), c, -1);
  if (patient_flags && m->P.n) HIPCHK(hipMemcpy(patient_flags, m->P.flags, m->P.n, hipMemcpyDeviceToHost), c, -1);
  if (donor_flags && m->n_donors) HIPCHK(hipMemcpy(donor_flags, m->D.flags, m->n_donors, hipMemcpyDeviceToHost), c, -1);
  return 0;
}

extern "C" int grim_match_results(grim_match *m, grim_match_rec *out, uint8_t *patient_flags, uint8_t *donor_flags) {
  if (!m) return -1;
  if (m->graded) {  // the buffer holds records of another size
    mt_clear(m);
    refuse(m->ctx, "grim_match_results", "the matcher is graded (call grim_match_results_graded)");
    return -3;
  }
  return mt_results(m, out, sizeof(grim_match_rec), patient_flags, donor_flags);
}

extern "C" int grim_match_results_graded(grim_match *m, grim_match_grade_rec *out, uint8_t *patient_flags, uint8_t *donor_flags) {
  if (!m) return -1;
  if (!m->graded) {
    mt_clear(m);
    refuse(m->ctx, "grim_match_results_graded", "the matcher is not graded (call grim_match_results)");
    return -3;
  }
  return mt_results(m, out, sizeof(grim_match_grade_rec), patient_flags, donor_flags);
}

extern "C" int grim_match_stats(const grim_match *m, uint64_t out[8]) {
  if (!m || !out) return -1;
  for (int k = 0; k < 8; ++k) out[k] = m->stat[k];
  return 0;
}

// =================================================================================================
// Donor search (grim_search.h): each patient's best top_n donors over any number of runs, selected on the device from the
// records the matcher's pair kernel leaves in its result buffer
// =================================================================================================
struct grim_search {
  grim_ctx *ctx;
  grim_match *m;  // owned; driven through the grim_match_* doors, whose behaviour is theirs
  uint32_t top_n, tile;
  double min_p0;
  DevBuf<uint32_t> d_ids;
  DevBuf<SrKey> d_keys[2];  // the lists of a level and of the next, in turns: top_n keys a list
  DevBuf<uint32_t> d_cnt[2];
  // the running list, double-buffered: run r reads [cur] and writes [cur ^ 1].  The six are reserved together, for the patients set.
  DevBuf<SrHit> d_hits[2];
  DevBuf<SrKey> d_run_keys[2];
  DevBuf<uint32_t> d_run_cnt[2];
  int cur;
  bool have_running;  // [cur] holds lists (false: every list is empty, nothing on the device says so)
  DevBuf<unsigned long long> d_cand;
  DevBuf<SrHit> d_in;  // the hit lists of a merge and their counts, as uploaded
  DevBuf<uint32_t> d_in_cnt;
  uint64_t sum[8];  // the matcher's seven counters summed over the runs, [7] candidates
  Events<2> ev;
  double select_ms, kernel_ms;  // of the last run
};

static void sr_empty(grim_search *s) {
  s->have_running = false;
  for (uint64_t &x : s->sum) x = 0;
  s->select_ms = s->kernel_ms = 0.0;
}

extern "C" grim_search *grim_search_create_ex(grim_ctx *c, uint32_t keep_mask, const uint32_t n_alleles[GRIM_MAXL], uint32_t top_n,
                                              double min_p0, uint32_t direction) {
  if (!c || !n_alleles) {
    set_err(c, "grim_search_create: bad arguments");
    return nullptr;
  }
  if (top_n == 0 || top_n > GRIM_SEARCH_MAX_N) {
    set_err(c, "grim_search_create: top_n must be 1.." + std::to_string(GRIM_SEARCH_MAX_N));
    return nullptr;
  }
  if (min_p0 != min_p0) {
    set_err(c, "grim_search_create: min_p0 is not a number");
    return nullptr;
  }
  uint32_t tile = SR_TILE;
  if (const char *e = getenv("GRIM_SEARCH_TILE")) {  // for tests: small tiles make deep trees on small inputs
    char *end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    if (end == e || *end != 0 || v == 0 || (v & (v - 1)) != 0 || v > SR_TILE || v < 2ull * top_n) {
      set_err(c, "grim_search_create: GRIM_SEARCH_TILE must be a power of two with 2 top_n <= tile <= " + std::to_string(SR_TILE));
      return nullptr;
    }
    tile = (uint32_t)v;
  }
  grim_match *m = grim_match_create_ex(c, keep_mask, n_alleles, direction, 0);  // ungraded: the selection reads 128-byte records
  if (!m) return nullptr;
  use_device(c->device);
  grim_search *s = new grim_search();
  s->ctx = c;
  s->m = m;
  s->top_n = top_n;
  s->tile = tile;
  s->min_p0 = min_p0;
  if (!s->d_cand.reserve(1) || !s->ev.create()) {
    (void)hipGetLastError();
    set_err(c, "grim_search_create: device allocation failed");
    grim_search_free(s);
    return nullptr;
  }
  return s;
}

extern "C" grim_search *grim_search_create(grim_ctx *c, uint32_t keep_mask, const uint32_t n_alleles[GRIM_MAXL], uint32_t top_n,
                                           double min_p0) {
  return grim_search_create_ex(c, keep_mask, n_alleles, top_n, min_p0, GRIM_MATCH_DIR_EITHER);
}

extern "C" void grim_search_free(grim_search *s) {
  if (!s) return;
  use_device(s->ctx->device);
  hipStreamSynchronize(s->ctx->stream);
  grim_match *m = s->m;
  delete s;  // its own buffers first
  grim_match_free(m);
}

extern "C" int grim_search_set_patients(grim_search *s, const grim_subject_result *res, uint32_t n, const grim_row *rows, uint32_t n_rows) {
  if (!s) return -1;
  sr_empty(s);
  return grim_match_set_patients(s->m, res, n, rows, n_rows);
}

extern "C" int grim_search_set_groups(grim_search *s, const grim_groups *g) {
  if (!s) return -1;
  sr_empty(s);  // a hit list computed at one resolution never meets another
  return grim_match_set_groups(s->m, g);
}

extern "C" int grim_search_reset(grim_search *s) {
  if (!s) return -1;
  sr_empty(s);
  return 0;
}

// the selection of one run: the matcher holds the records of n donors; ids on the host.  The running list changes hands only
// when everything has worked.
static int sr_select(grim_search *s, const char *who, const uint32_t *ids, uint32_t n) {
  grim_ctx *c = s->ctx;
  grim_match *m = s->m;
  hipStream_t st = c->stream;
  const uint32_t n_p = m->P.n, top_n = s->top_n, tile = s->tile, per = tile / top_n;
  if (n == 0 || n_p == 0) return 0;
  const uint32_t tiles0 = (n + tile - 1) / tile;
  const uint64_t lists0 = (uint64_t)n_p * (tiles0 + 1ull);  // every level writes fewer lists than level 0
  bool ok = s->d_ids.reserve((uint64_t)n + 1) && reserve_all(lists0, 0, s->d_cnt[0], s->d_cnt[1]) &&
            reserve_all(lists0 * top_n, 0, s->d_keys[0], s->d_keys[1]);
  if (ok && s->have_running && (uint64_t)n_p > s->d_run_cnt[0].cap) {  // cannot be: the patients have not changed since the lists were made
    set_err(c, std::string(who) + ": the running lists are smaller than the patients (internal)");  // growing would discard them
    return -1;
  }
  ok = ok && reserve_all((uint64_t)n_p * top_n, 0, s->d_hits[0], s->d_hits[1], s->d_run_keys[0], s->d_run_keys[1]) &&
       reserve_all(n_p, 0, s->d_run_cnt[0], s->d_run_cnt[1]);
  if (!ok) {
    set_err(c, std::string(who) + ": device allocation failed");
    return -1;
  }
  HIPCHK(hipMemcpyAsync(s->d_ids, ids, 4ull * n, hipMemcpyHostToDevice, st), c, -1);
  HIPCHK(hipMemsetAsync(s->d_cand, 0, 8, st), c, -1);
  HIPCHK(hipEventRecord(s->ev[0], st), c, -1);
  const int cur = s->cur, nxt = cur ^ 1;
  const SrKey *extra = s->have_running ? s->d_run_keys[cur].p : nullptr;
  const uint32_t *extra_cnt = s->have_running ? s->d_run_cnt[cur].p : nullptr;
  const SrHit *hits_were = s->have_running ? s->d_hits[cur].p : nullptr;
  int side = 0;  // d_keys[side] holds the lists of the level just written
  for_slabs(n_p, [&](uint32_t p0, uint32_t np) {
    hipLaunchKernelGGL(sr_tile_kernel, dim3(tiles0, np), dim3(SR_THREADS), 0, st, m->d_out, s->d_ids, m->P.flags, m->D.flags, n_p, p0, n,
                       s->min_p0, (const SrKey *)nullptr, (const uint32_t *)nullptr, 0u, (const SrKey *)nullptr,
                       (const uint32_t *)nullptr, tile, top_n, s->d_keys[0], s->d_cnt[0], s->d_cand);
  });
  uint32_t lists = tiles0;
  while (lists + (extra ? 1u : 0u) > 1u) {  // merging levels: per >= 2 lists become one
    const uint32_t out_lists = (lists + (extra ? 1u : 0u) + per - 1) / per;
    for_slabs(n_p, [&](uint32_t p0, uint32_t np) {
      hipLaunchKernelGGL(sr_tile_kernel, dim3(out_lists, np), dim3(SR_THREADS), 0, st, (const double *)nullptr, (const uint32_t *)nullptr,
                         (const uint8_t *)nullptr, (const uint8_t *)nullptr, n_p, p0, 0u, s->min_p0, s->d_keys[side], s->d_cnt[side], lists,
                         extra, extra_cnt, tile, top_n, s->d_keys[side ^ 1], s->d_cnt[side ^ 1], s->d_cand);
    });
    side ^= 1;
    lists = out_lists;
    extra = nullptr;
    extra_cnt = nullptr;
  }
  for_slabs(n_p, [&](uint32_t p0, uint32_t np) {
    hipLaunchKernelGGL(sr_gather_kernel, dim3(np), dim3(64), 0, st, s->d_keys[side], s->d_cnt[side], lists, m->d_out, n_p, p0, n, hits_were,
                       top_n, s->d_hits[nxt], s->d_run_keys[nxt], s->d_run_cnt[nxt], (const SrHit *)nullptr, 0u);
  });
  HIPCHK(hipGetLastError(), c, -1);
  HIPCHK(hipEventRecord(s->ev[1], st), c, -1);
  unsigned long long cand = 0;
  HIPCHK(hipMemcpyAsync(&cand, s->d_cand, 8, hipMemcpyDeviceToHost, st), c, -1);
  HIPCHK(hipStreamSynchronize(st), c, -1);
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]), c, -1);
  s->cur = nxt;
  s->have_running = true;
  for (int k = 0; k < 7; ++k) s->sum[k] += m->stat[k];
  s->sum[7] += cand;
  s->select_ms = ms;
  s->kernel_ms = m->last_ms + ms;
  return 0;
}

extern "C" int grim_search_run(grim_search *s, grim_batch *b, const uint32_t *donor_ids) {
  if (!s || !b) return -1;
  s->select_ms = s->kernel_ms = 0.0;
  if (b->n_subj && !donor_ids) {
    set_err(s->ctx, "grim_search_run: donor_ids is null");
    return -3;
  }
  const int rc = grim_match_run(s->m, b);
  if (rc != 0) return rc;
  return sr_select(s, "grim_search_run", donor_ids, s->m->n_donors);
}

extern "C" int grim_search_run_records(grim_search *s, const grim_subject_result *res, uint32_t n, const grim_row *rows, uint32_t n_rows,
                                       const uint32_t *donor_ids) {
  if (!s) return -1;
  s->select_ms = s->kernel_ms = 0.0;
  if (n && !donor_ids) {
    set_err(s->ctx, "grim_search_run_records: donor_ids is null");
    return -3;
  }
  const int rc = grim_match_run_records(s->m, res, n, rows, n_rows);
  if (rc != 0) return rc;
  return sr_select(s, "grim_search_run_records", donor_ids, s->m->n_donors);
}

static_assert(sizeof(SrHit) == sizeof(grim_search_hit) && sizeof(SrHit) == 136 && SR_MERGE_MAX_LISTS == GRIM_SEARCH_MERGE_MAX_LISTS,
              "hit layout and the bound of a merge");
static_assert((uint64_t)SR_MERGE_MAX_LISTS * GRIM_SEARCH_MAX_N <= SR_SRC_IN && (SR_SRC_IN & SR_SRC_PREV) == 0,
              "a slot index l * top_n + k of a merge stays below the SR_SRC_IN tag bit");

// the door of a merge: hit lists as the results are laid out, checked on the host before anything is uploaded; the caller
// returns -3
static bool hits_door(grim_ctx *c, const char *who, const grim_search_hit *hits, const uint32_t *n_hits, uint32_t n_p, uint32_t n_lists,
                      uint32_t top_n) {
  const uint64_t lists = (uint64_t)n_lists * n_p;
  if (lists && !n_hits) return refuse(c, who, "n_hits is null with lists to read");
  for (uint64_t at = 0; at < lists; ++at) {
    const uint32_t n = n_hits[at];
    if (n > top_n) return refuse(c, who, "a list with more hits than top_n");
    if (n && !hits) return refuse(c, who, "hits is null with hits to read");
    const grim_search_hit *h = hits + at * top_n;
    for (uint32_t k = 0; k < n; ++k) {
      if (h[k].donor == GRIM_SEARCH_NO_DONOR || h[k].reserved != 0)
        return refuse(c, who, "a hit whose donor is GRIM_SEARCH_NO_DONOR or whose reserved word is not 0");
      for (int q = 0; q < 2; ++q)
        if (!(h[k].rec.mm[q] >= 0.0 && h[k].rec.mm[q] <= 1.7976931348623157e308))
          return refuse(c, who, "a hit whose mm[0] or mm[1] is negative, NaN or infinite");
      if (k && !sr_before(h[k - 1].rec.mm[0], h[k - 1].rec.mm[1], h[k - 1].donor, h[k].rec.mm[0], h[k].rec.mm[1], h[k].donor))
        return refuse(c, who, "a list whose hits are not in the strict order (mm[0] down, mm[1] down, id up)");
    }
  }
  return true;
}

extern "C" int grim_search_merge_hits(grim_search *s, const grim_search_hit *hits, const uint32_t *n_hits, uint32_t n_patients,
                                      uint32_t n_lists) {
  if (!s) return -1;
  const char *who = "grim_search_merge_hits";
  grim_ctx *c = s->ctx;
  grim_match *m = s->m;
  s->select_ms = s->kernel_ms = 0.0;
  const uint32_t n_p = m->P.n, top_n = s->top_n, tile = s->tile, per = tile / top_n;
  if (n_patients != n_p) {
    refuse(c, who, "n_patients is not the number of patients set");
    return -3;
  }
  if (n_lists > GRIM_SEARCH_MERGE_MAX_LISTS) {
    refuse(c, who, "more lists than GRIM_SEARCH_MERGE_MAX_LISTS");
    return -3;
  }
  if (!hits_door(c, who, hits, n_hits, n_p, n_lists, top_n)) return -3;
  if (n_lists == 0 || n_p == 0) return 0;
  use_device(c->device);
  hipStream_t st = c->stream;
  const uint64_t in_lists = (uint64_t)n_lists * n_p, lists0 = (uint64_t)n_p * (n_lists + 1ull);
  bool ok = s->d_in.reserve(in_lists * top_n + 1) && s->d_in_cnt.reserve(in_lists + 1) &&  // never an empty allocation
            reserve_all(lists0, 0, s->d_cnt[0], s->d_cnt[1]) && reserve_all(lists0 * top_n, 0, s->d_keys[0], s->d_keys[1]);
  if (ok && s->have_running && (uint64_t)n_p > s->d_run_cnt[0].cap) {  // as in sr_select: growing would discard the lists
    set_err(c, std::string(who) + ": the running lists are smaller than the patients (internal)");
    return -1;
  }
  ok = ok && reserve_all((uint64_t)n_p * top_n, 0, s->d_hits[0], s->d_hits[1], s->d_run_keys[0], s->d_run_keys[1]) &&
       reserve_all(n_p, 0, s->d_run_cnt[0], s->d_run_cnt[1]);
  if (!ok) {
    set_err(c, std::string(who) + ": device allocation failed");
    return -1;
  }
  const int cur = s->cur, nxt = cur ^ 1;
  // everything that is queued: a failure in it must not return while a staged copy or a kernel is still in flight against
  // the caller's arrays or the scratch lists, so the stream is drained on that path too
  auto enqueue = [&]() -> int {
    // a hits array may be null when every count is 0: the import kernel then reads no hit
    if (hits) HIPCHK(hipMemcpyAsync(s->d_in, hits, sizeof(grim_search_hit) * in_lists * top_n, hipMemcpyHostToDevice, st), c, -1);
    HIPCHK(hipMemcpyAsync(s->d_in_cnt, n_hits, 4ull * in_lists, hipMemcpyHostToDevice, st), c, -1);
    HIPCHK(hipEventRecord(s->ev[0], st), c, -1);
    const SrKey *extra = s->have_running ? s->d_run_keys[cur].p : nullptr;
    const uint32_t *extra_cnt = s->have_running ? s->d_run_cnt[cur].p : nullptr;
    const SrHit *hits_were = s->have_running ? s->d_hits[cur].p : nullptr;
    const uint32_t in_slots = n_lists * top_n;  // <= 2^20
    for_slabs(n_p, [&](uint32_t p0, uint32_t np) {
      hipLaunchKernelGGL(sr_import_kernel, dim3((in_slots + SR_THREADS - 1) / SR_THREADS, np), dim3(SR_THREADS), 0, st, s->d_in, s->d_in_cnt, n_p,
                         p0, n_lists, top_n, s->min_p0, s->d_keys[0], s->d_cnt[0]);
    });
    int side = 0;  // d_keys[side] holds the lists of the level just written
    uint32_t lists = n_lists;
    do {  // merging levels, at least one: what the gather reads is one sorted list
      const uint32_t out_lists = (lists + (extra ? 1u : 0u) + per - 1) / per;
      for_slabs(n_p, [&](uint32_t p0, uint32_t np) {
        hipLaunchKernelGGL(sr_tile_kernel, dim3(out_lists, np), dim3(SR_THREADS), 0, st, (const double *)nullptr, (const uint32_t *)nullptr,
                           (const uint8_t *)nullptr, (const uint8_t *)nullptr, n_p, p0, 0u, s->min_p0, s->d_keys[side], s->d_cnt[side], lists,
                           extra, extra_cnt, tile, top_n, s->d_keys[side ^ 1], s->d_cnt[side ^ 1], s->d_cand);
      });
      side ^= 1;
      lists = out_lists;
      extra = nullptr;
      extra_cnt = nullptr;
    } while (lists > 1u);
    for_slabs(n_p, [&](uint32_t p0, uint32_t np) {
      hipLaunchKernelGGL(sr_gather_kernel, dim3(np), dim3(64), 0, st, s->d_keys[side], s->d_cnt[side], lists, (const double *)nullptr, n_p, p0,
                         0u, hits_were, top_n, s->d_hits[nxt], s->d_run_keys[nxt], s->d_run_cnt[nxt], s->d_in.p, in_slots);
    });
    HIPCHK(hipGetLastError(), c, -1);
    HIPCHK(hipEventRecord(s->ev[1], st), c, -1);
    return 0;
  };
  if (enqueue() != 0) {
    (void)hipStreamSynchronize(st);
    return -1;
  }
  HIPCHK(hipStreamSynchronize(st), c, -1);
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]), c, -1);
  s->cur = nxt;
  s->have_running = true;
  s->select_ms = s->kernel_ms = ms;
  return 0;
}

extern "C" int grim_search_results(grim_search *s, grim_search_hit *hits, uint32_t *n_hits) {
  if (!s) return -1;
  grim_ctx *c = s->ctx;
  use_device(c->device);
  const uint32_t n_p = s->m->P.n;
  const uint64_t slots = (uint64_t)n_p * s->top_n;
  if (!s->have_running) {  // empty lists
    if (hits)
      for (uint64_t k = 0; k < slots; ++k) {
        memset(&hits[k], 0, sizeof(grim_search_hit));
        hits[k].donor = GRIM_SEARCH_NO_DONOR;
      }
    if (n_hits)
      for (uint32_t p = 0; p < n_p; ++p) n_hits[p] = 0;
    return 0;
  }
  if (hits && slots) HIPCHK(hipMemcpy(hits, s->d_hits[s->cur], sizeof(grim_search_hit) * slots, hipMemcpyDeviceToHost), c, -1);
  if (n_hits && n_p) HIPCHK(hipMemcpy(n_hits, s->d_run_cnt[s->cur], 4ull * n_p, hipMemcpyDeviceToHost), c, -1);
  return 0;
}

extern "C" int grim_search_flags(grim_search *s, uint8_t *patient_flags, uint8_t *donor_flags) {
  if (!s) return -1;
  return grim_match_results(s->m, nullptr, patient_flags, donor_flags);
}

extern "C" uint32_t grim_search_patients(const grim_search *s) { return s ? s->m->P.n : 0; }
extern "C" uint32_t grim_search_donors(const grim_search *s) { return s ? s->m->n_donors : 0; }
extern "C" uint32_t grim_search_top_n(const grim_search *s) { return s ? s->top_n : 0; }
extern "C" double grim_search_kernel_ms(const grim_search *s) { return s ? s->kernel_ms : 0.0; }
extern "C" double grim_search_select_ms(const grim_search *s) { return s ? s->select_ms : 0.0; }

extern "C" int grim_search_stats(const grim_search *s, uint64_t out[8]) {
  if (!s || !out) return -1;
  for (int k = 0; k < 8; ++k) out[k] = s->sum[k];
  return 0;
}
