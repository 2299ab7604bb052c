/*
 * grim_hip.h -- C-ABI of libgrim_hip.so, the MI355X (gfx950) engine for the grim.impute hot path.
 *
 * The reference (nmdp-bioinformatics/py-graph-imputation) has no FFI for this path -- its only
 * native code is a 65-line Cython list helper (grim/imputation/cutils.pyx) -- so this ABI is the
 * build's own.  Each entry point names the reference interface it replaces (file:line under the
 * reference tree).  Plain pointers and sizes only; the library copies what it is given, owns
 * what it returns, and never calls back into the host language.
 *
 * Threading: one grim_ctx per GPU.  The block entry points (grim_batch_*) of a context are used by one host thread at
 * a time; a grim_stream runs its own threads on its context (one stream per context at a time).  Independent contexts
 * are independent.  grim_last_error returns a copy private to the calling thread.
 * Errors: functions return 0 on success, <0 on error (grim_last_error gives the text);
 * constructors return NULL on error.  Per-subject outcomes (miss / needs-fallback) are DATA in
 * grim_subject_result.status, never a call failure.
 */
#ifndef GRIM_HIP_H
#define GRIM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GRIM_MAXL 5        /* loci per haplotype (A,B,C,DQB1,DRB1)                         */
#define GRIM_ABITS 12      /* bits per locus in a 64-bit haplotype key: (allele_id+1)<<12*slot */
#define GRIM_KEY_GRAPH_ORDER 60 /* bit of a haplotype key in a result row: the haplotype is a graph node's NAME (alleles in
                                  loci_map index order), not a joined key (alleles sorted); matters to the phased writer only,
                                  and only under a loci_map that is not alphabetical */
#define GRIM_MAXPH 16      /* 2^(GRIM_MAXL-1) phases (impute.py:274-303)                     */
#define GRIM_MAXPOP 64     /* populations                                                    */
#define GRIM_TOPCAP 128    /* upper bound for max_haplotypes_number_in_phase (impute.py:436) */
#define GRIM_MAXLADDER 64  /* epsilon ladder entries (impute.py:1665-1687)                   */
#define GRIM_MAXROWS 8     /* Plan_B_Matrix rows                                             */

typedef struct grim_ctx grim_ctx;
typedef struct grim_graph grim_graph;
typedef struct grim_batch grim_batch;

/* ---- context ---------------------------------------------------------------------------- */
grim_ctx *grim_create(int device_id);
void grim_destroy(grim_ctx *ctx);
const char *grim_last_error(grim_ctx *ctx);
/* number of HIP devices this process can use, 0 when there is none or the runtime fails (never raises). */
int grim_device_count(void);
/* How a stream's results come from HBM to pinned host memory on this context: the bit of the SDMA engine the downloads are
 * pinned to (hsa_amd_sdma_engine_id_t, > 1: csrc/grim_sdma.h -- uploads stay on engine 0x1, so both directions of the link
 * run at once), 0 = a copy kernel (GRIM_EXPORT=kernel, or no second engine on offer), -1 = hipMemcpyAsync
 * (GRIM_EXPORT=memcpy).  The reference has no counterpart (its results are Python objects). */
int grim_export_engine(grim_ctx *ctx);

/* ---- graph: replaces Graph.build_graph's in-memory product (networkx_graph.py:42-213) ----
 * Integer-encoded: node = (label bitmask over locus slots, <=5 allele ids); a node NAME lookup
 * (Vertices_attributes[name], networkx_graph.py:260,290) becomes a 64-bit key probe.
 * a_start/a_nbr : plan-A CSR partial node -> full nodes, INCLUDING the reference's row-start
 *                 quirks (networkx_graph.py:157-198); a_start has n_nodes+1 entries.
 * b_conn        : [n_nodes][GRIM_MAXL] connector index of (child node, added locus slot), or
 *                 0xFFFFFFFF (the "parentLabel+childName" pseudo nodes, networkx_graph.py:103-130)
 * b_start/b_nbr : connector -> parent nodes CSR (n_conn+1 entries, quirks included).
 * lab_start/lab_nodes : node ids grouped by label mask in id order (haps_by_label,
 *                 networkx_graph.py:215-236); lab_start has (1<<GRIM_MAXL)+1 entries. */
typedef struct {
  uint32_t n_nodes, n_pops, n_loci, full_mask;
  const uint64_t *node_key;  /* [n_nodes] */
  const uint8_t *node_mask;  /* [n_nodes] */
  const double *freq;        /* [n_nodes][n_pops] */
  const uint32_t *a_start;   /* [n_nodes+1] */
  const uint32_t *a_nbr;     /* [n_a_nbr] */
  uint64_t n_a_nbr;
  const uint32_t *b_conn;    /* [n_nodes*GRIM_MAXL] */
  const uint32_t *b_start;   /* [n_conn+1] */
  const uint32_t *b_nbr;     /* [n_b_nbr] */
  uint32_t n_conn;
  uint64_t n_b_nbr;
  const uint32_t *lab_start; /* [(1<<GRIM_MAXL)+1] */
  const uint32_t *lab_nodes; /* [n_nodes] */
  /* bit m set: a haplotype NAME over the loci of label mask m built from a subject's alleles never equals a graph name --
   * the subject's alleles come in sorted STRING order (gl2haps, impute.py:271), graph names in loci_map index order
   * (generate_neo4j_multi_hpf.py:59-68), and for this locus set the two orders differ (a loci_map that is not alphabetical,
   * e.g. the reference's own default A 1, B 3, C 2: every set that holds both B and C).  0: the two orders agree everywhere. */
  uint32_t label_order_bad;
  uint32_t reserved;
} grim_graph_desc;

grim_graph *grim_graph_upload(grim_ctx *ctx, const grim_graph_desc *desc);
void grim_graph_free(grim_graph *g);
uint64_t grim_graph_device_bytes(const grim_graph *g);

/* ---- graph, host side (C++, no GPU) ------------------------------------------------------
 * grim_hostgraph_load_csv: nodes.csv / top_links.csv / edges.csv -> the arrays above, i.e. all of
 *   Graph.build_graph (networkx_graph.py:42-213; argument order nodes, top links, all edges as at
 *   :42); alleles are interned into `dict` in file order.  NULL + message in err on failure.
 * grim_graphgen_csv: hpf.csv -> the four graph CSVs, i.e. generate_graph
 *   (graph_generation/generate_neo4j_multi_hpf.py:209-486); cutoff[p] = freq_trim_threshold /
 *   population count as computed at :251-262; locus_names/locus_index = the conf's loci_map. */
typedef struct grim_hostgraph grim_hostgraph;
typedef struct grim_dict grim_dict;     /* per locus slot: allele string <-> dense id (see the host helpers below) */
grim_hostgraph *grim_hostgraph_load_csv(grim_dict *dict, const char *full_loci, const char *nodes_csv, const char *top_links_csv,
                                        const char *edges_csv, char *err, uint64_t err_cap);
int grim_hostgraph_desc(const grim_hostgraph *h, grim_graph_desc *out);
void grim_hostgraph_free(grim_hostgraph *h);
int grim_graphgen_csv(const char *hpf_csv, const char *const *pops, const double *cutoff, uint32_t n_pops,
                      const char *const *locus_names, const uint32_t *locus_index, uint32_t n_locus_names, const char *nodes_csv,
                      const char *edges_csv, const char *top_links_csv, const char *info_csv, char *err, uint64_t err_cap);
/* grim_hostgraph_from_hpf: both of the above in one call -- hpf.csv -> loaded arrays, the generator's texts handed to the
 *   loader in memory (graph_freqs + Graph.build_graph, grim/grim.py:53-87, without the four files in between).  Each CSV
 *   path may be NULL; a path that is given is written exactly as grim_graphgen_csv writes it. */
grim_hostgraph *grim_hostgraph_from_hpf(grim_dict *dict, const char *full_loci, const char *hpf_csv, const char *const *pops,
                                        const double *cutoff, uint32_t n_pops, const char *const *locus_names,
                                        const uint32_t *locus_index, uint32_t n_locus_names, const char *nodes_csv,
                                        const char *edges_csv, const char *top_links_csv, const char *info_csv, char *err,
                                        uint64_t err_cap);

/* ---- run parameters: the conf keys of run_impute_def.py:63-129 that reach the hot path ------ */
typedef struct {
  double ladder[GRIM_MAXLADDER]; /* eps values tried in order (impute.py:1665-1673), host-computed */
  int32_t n_ladder;
  uint32_t top_n;          /* max_haplotypes_number_in_phase */
  uint64_t opt_threshold;  /* number_of_options_threshold    */
  uint32_t n_results;      /* number_of_results              */
  uint32_t n_pop_results;  /* number_of_pop_results          */
  uint8_t out_muug, out_haps, planb, em_mr;
  uint8_t em;              /* impute_file(em=True): the phased pass never falls back to Plan C (impute.py:1649) */
  uint8_t save_mode;       /* save_space_mode: open_option_ keeps the 10 largest entries of either operand before the cross
                              product (impute.py:1048-1059) */
  uint8_t eps_nonpositive; /* conf epsilon <= 0: call_comp_phase_prob never runs a pass and returns its "NaN" sentinel
                              (impute.py:1663-1665); the writers raise on it, so every subject that has phases ends as its
                              raw line in .problem (formatter rule; the ladder is empty) */
  uint8_t pop_rank[GRIM_MAXPOP]; /* rank of each population NAME in sorted order (impute.py:535) */
  double factor_missing_pow[GRIM_MAXL + 1]; /* factor_missing_data ** k for k = 0..5, evaluated by the
                                               host exactly as the reference does (impute.py:1168) */
  /* Plan_B_Matrix: row r has planb_nblk[r] blocks; block b is a locus-slot bitmask */
  uint8_t planb_rows;
  uint8_t planb_nblk[GRIM_MAXROWS];
  uint8_t planb_blk[GRIM_MAXROWS][GRIM_MAXL];
} grim_params;

/* ---- subjects: the tokenised form of one input line (impute.py:2022-2036, 105-118, 246-272) --
 * Position k (0..n_loci-1) is the k-th locus in the subject's sorted order; slot[k] is its locus
 * slot.  tokens[tok_off ...] holds, for k = 0.., side 0 then side 1, cnt[k][side] allele ids
 * (first occurrences only; wid[k][side] keeps the original '/'-list length that the
 * number_of_options_threshold test uses, impute.py:926-932). */
typedef struct {
  uint32_t tok_off;
  uint16_t prior_idx; /* index into the batch's prior matrices (impute.py:1956-1975) */
  uint8_t n_loci;
  uint8_t flags;      /* bit k: position k keeps its side in every phase (phase mask, impute.py:277-290) */
  uint8_t slot[GRIM_MAXL];
  uint8_t pad[3];
  uint16_t cnt[GRIM_MAXL][2];
  uint16_t wid[GRIM_MAXL][2];
  uint32_t reserved[2];
} grim_subject; /* 64 bytes */

typedef struct {
  uint32_t n_subjects;
  const grim_subject *subjects;
  const uint16_t *tokens;
  uint64_t n_tokens;
  const double *priors; /* [n_priors][n_pops][n_pops] */
  uint32_t n_priors;
} grim_batch_desc;

/* status values */
enum {
  GRIM_ST_OK = 0,         /* results present                                                    */
  GRIM_ST_MISS = 1,       /* nothing found on any plan  (-> .miss, impute.py:2065-2068)          */
  GRIM_ST_UNSUPPORTED = 2,/* needs a reference path this build does not run on device yet       */
  GRIM_ST_NOPHASE = 3     /* open_phases stayed empty after both rewrites (impute.py:1619-1629): the
                             reference writes nothing for MUUG and raises while writing the phased
                             output -> raw line in .problem when output_haplotypes is on             */
};

/* one output row: a/b are 64-bit haplotype keys (genotype and haplotype-pair tables); popa/popb are the populations of a
 * haplotype-pair row and NAME the pair of a population-table row (a/b repeat them there -- except in the one row that
 * serves as a one-population subject's genotype row and both its population rows: read popa/popb). */
typedef struct {
  uint64_t a, b;
  double prob;
  uint32_t popa, popb;
} grim_row; /* 32 bytes */

/* table ids inside grim_subject_result */
enum { GRIM_T_UMUG = 0, GRIM_T_UMUG_POPS = 1, GRIM_T_PMUG = 2, GRIM_T_PMUG_POPS = 3, GRIM_T_COUNT = 4 };

typedef struct {
  uint8_t status;
  uint8_t plan;           /* 'a', 'b' or 'c' as in impute.py:216,1638,1702 */
  uint8_t reason;         /* for GRIM_ST_UNSUPPORTED */
  uint8_t plan_phased;    /* plan the .pmug/.pmug.pops rows came from when it differs from `plan` (the phased pass
                             after a MUUG Plan C starts over, impute.py:1645-1654); 0 = same as `plan` */
  uint32_t n_pairs;       /* len(res_haps["Haps"])  (impute.py:2074-2078) */
  uint32_t n_genotypes;   /* len(res_muugs["Haps"]) (impute.py:2108-2112) */
  uint32_t row_off[GRIM_T_COUNT];
  uint32_t n_rows[GRIM_T_COUNT];
  double max_prob;
} grim_subject_result; /* 56 bytes */

/* grim_batch_upload copies subjects/tokens/priors to HBM and allocates result + scratch buffers.
 * grim_batch_run enqueues the kernels on the context's stream and waits; it may be called
 * repeatedly on the same resident batch (bench.py does).  Replaces the per-subject loop
 * impute_file -> impute_one -> comp_cand -> call_comp_phase_prob (impute.py:2019-2059,
 * 1584-1724) for every subject of the batch at once. */
grim_batch *grim_batch_upload(grim_ctx *ctx, const grim_graph *g, const grim_params *p,
                              const grim_batch_desc *d);
int grim_batch_run(grim_batch *b);
/* n complete synchronous runs back to back (what a caller's loop around grim_batch_run does, without the
 * caller's per-iteration overhead); stops at the first failing run and returns its code */
int grim_batch_run_repeat(grim_batch *b, uint32_t n);
/* Timing mode (also GRIM_TIMING=1 in the environment): every kernel of a run is bracketed by its own start/stop
 * hipEvents on the launch stream (hipExtLaunchKernelGGL).  Off by default: a synchronous 10k-subject run costs
 * 22 us without, 29 us with the events. */
int grim_batch_set_timing(grim_batch *b, int on);
/* device time of the last grim_batch_run in timing mode (0 otherwise), each figure from the kernels' own start/stop
 * events.  `which` is one of the values below (frozen: callers pass them as plain integers too); TOTAL = PLAN_A + PLAN_B +
 * TABLES + COMPACT + TOKENIZER.  which | GRIM_MS_MEAN = the mean of that figure over all runs since timing was switched on;
 * any other value gives 0. */
enum {
  GRIM_MS_TOTAL = 0,     /* all kernels */
  GRIM_MS_PLAN_A = 1,    /* half-wave + one-wave + general + mid-size kernel */
  GRIM_MS_PLAN_B = 2,    /* plan-B/C kernel */
  GRIM_MS_HALF_WAVE = 3, /* half-wave kernel */
  GRIM_MS_GENERAL = 4,   /* general plan-A kernel */
  GRIM_MS_ONE_WAVE = 5,  /* one-wave kernel */
  GRIM_MS_TABLES = 6,    /* the table kernels */
  GRIM_MS_COMPACT = 7,   /* the half-wave kernel's row compaction */
  GRIM_MS_TOKENIZER = 8, /* the device tokenizer */
  GRIM_MS_MID = 9,       /* the mid-size kernel */
  GRIM_MS_MEAN = 0x10
};
double grim_batch_kernel_ms(const grim_batch *b, int which);
/* algorithmic byte counters of the last run: [0] probes, [1] CSR neighbour ids,
 * [2] frequency vectors gathered, [3] output rows */
int grim_batch_counters(const grim_batch *b, uint64_t out[4]);
uint32_t grim_batch_total_rows(const grim_batch *b);
/* copy results to host: res[n_subjects], rows[grim_batch_total_rows] */
int grim_batch_results(grim_batch *b, grim_subject_result *res, grim_row *rows);
void grim_batch_free(grim_batch *b);

/* ======================= host-side helpers (CPU, multi-threaded; no GPU needed) ====================
 * Allele dictionary, GL tokenizer and result formatter in C++ (csrc/grim_host.cpp).  They replace,
 * for whole files at a time, the reference's per-line Python: impute_file's line handling
 * (impute.py:2022-2036), clean_up_gl (:105-118), gl2haps (:246-272), the writers' text and the
 * .miss/.problem rules (:24-99, 2061-2118) including CPython's str(float). */
typedef struct grim_parsed grim_parsed; /* a tokenised block of input lines           */
typedef struct grim_text grim_text;     /* the six output texts                       */

grim_dict *grim_dict_create(uint32_t n_loci);
void grim_dict_free(grim_dict *d);
int grim_dict_set_locus(grim_dict *d, uint32_t slot, const char *locus_name);
int32_t grim_dict_intern(grim_dict *d, uint32_t slot, const char *allele); /* id, created if new; <0 = full */
int32_t grim_dict_find(const grim_dict *d, uint32_t slot, const char *allele);
const char *grim_dict_name(const grim_dict *d, uint32_t slot, uint32_t id);
uint32_t grim_dict_count(const grim_dict *d, uint32_t slot);

/* per-line outcome kinds; GRIM_K_UNSUPPORTED: more distinct alleles at one locus of one subject than a key field
 * holds (reported like a GRIM_ST_UNSUPPORTED subject, reason 5); GRIM_K_UNSUPPORTED_GL: a GL string that names a locus
 * twice or mixes loci inside one entry once each side's entries are sorted (reason 8) -- the reference checks no locus
 * and pairs the entries by index (gl2haps, grim/imputation/impute.py:246-272); such a subject is REPORTED, never
 * answered differently */
enum { GRIM_K_DEVICE = 0, GRIM_K_PROBLEM_ID = 1, GRIM_K_PROBLEM_RAW = 2, GRIM_K_MISS_NO_DEVICE = 3, GRIM_K_UNSUPPORTED = 4,
       GRIM_K_UNSUPPORTED_GL = 5 };

/* text: '\n'-separated input lines ("id,GL[,race1,race2]" or '%'-separated).  The dictionary is only READ:
 * alleles it does not know get ids from grim_dict_count(slot) upwards that are private to the subject that
 * brought them (grim_parsed_allele gives their text).  subjects[i].prior_idx = index of the line's
 * (race1, race2) pair in grim_parsed_race(); the caller supplies one prior matrix per pair in that order. */
grim_parsed *grim_tokenize(grim_dict *d, const char *text, uint64_t len, int planb, int n_threads);
void grim_parsed_free(grim_parsed *p);
uint32_t grim_parsed_lines(const grim_parsed *p);
uint32_t grim_parsed_subjects(const grim_parsed *p);
const grim_subject *grim_parsed_subject_array(const grim_parsed *p);
const uint16_t *grim_parsed_tokens(const grim_parsed *p, uint64_t *n_tokens);
const uint8_t *grim_parsed_kinds(const grim_parsed *p);      /* [lines]                      */
const int32_t *grim_parsed_dev_index(const grim_parsed *p);  /* [lines] subject index or -1  */
uint32_t grim_parsed_n_races(const grim_parsed *p);
const char *grim_parsed_race(const grim_parsed *p, uint32_t i, int which);
const char *grim_parsed_id(const grim_parsed *p, uint32_t line, uint32_t *len);
/* text (not NUL terminated) of allele `id` at locus slot `slot` as line `line` uses it; NULL if there is none */
const char *grim_parsed_allele(const grim_parsed *p, uint32_t line, uint32_t slot, uint32_t id, uint32_t *len);
/* host-language overrides: force a line's outcome kind; set a subject's `flags` = bitmask of positions
 * that must NOT switch sides when phases are enumerated (bin_imputation_in_file, impute.py:277-290) */
int grim_parsed_set_kind(grim_parsed *p, uint32_t line, uint8_t kind);
int grim_parsed_set_flags(grim_parsed *p, uint32_t line, uint8_t flags);

/* res/rows as returned by grim_batch_results for the subjects of `p`.  line_offset = global index
 * of the first line (multi-GPU shards); skip = optional [lines] mask of lines to leave out; subjects with
 * status GRIM_ST_UNSUPPORTED are left out of every text.
 * Texts: 0 .umug, 1 .umug.pops, 2 .pmug, 3 .pmug.pops, 4 .miss, 5 .problem. */
grim_text *grim_format(const grim_dict *d, const grim_parsed *p, const grim_params *prm, const char *const *pop_names,
                       uint32_t n_pops, const grim_subject_result *res, const grim_row *rows, uint64_t line_offset,
                       const uint8_t *skip, int n_threads);
const char *grim_text_get(const grim_text *t, int which, uint64_t *len);
void grim_text_free(grim_text *t);
int grim_format_double(double x, char *buf, int cap); /* CPython str(float) */

/* ---- prior matrices: calc_priority_matrix (impute.py:1844-1924) --------------------------------------------------
 * One P x P matrix per (race1, race2) pair of an input line: alpha/beta/gamma/delta/eta weights of the conf's
 * "priority", the UNK_priors base matrix ("MR" all ones, else identity) for lines without a known population,
 * population counts of pops_count_file (impute.py:205-212; NULL = all 1).  Every operation in the reference's
 * order: the matrices are bit-identical to numpy's. */
typedef struct {
  double alpha, eta, beta, gamma, delta;
  uint8_t unk_mr;
  const double *count_by_prob; /* [n_pops] or NULL */
} grim_prior_spec;
int grim_prior_matrix(const grim_prior_spec *spec, const char *const *pop_names, uint32_t n_pops, const char *race1,
                      const char *race2, double *out /* [n_pops * n_pops] */);

/* ======================= streaming pipeline: impute_file's loop (impute.py:2019-2144) =================================
 * Input text goes in as it comes (any split, lines may straddle calls); the library cuts it into chunks of
 * chunk_lines lines and runs, per chunk and overlapped between chunks:
 *     tokenizer threads -> pinned staging -> H2D -> kernels -> D2H -> formatter threads -> ordered output
 * on `n_threads` host threads plus one device thread.  Output: the six texts, appended to the files named in
 * out_path (parallel pwrite at offsets known from the chunk order) or kept in memory; optionally the per-subject
 * stdout lines of impute_file (text 6); optionally the raw result records of every chunk (grim_stream_next_records).
 * The row pool of a chunk is bounded; a chunk that overflows it is run again -- with twice the pool (up to every line's
 * worst case) when rows_per_chunk was left at 0, in halves, down to single subjects, when the caller fixed it -- so no
 * configuration needs a worst-case allocation up front.
 * One stream per grim_ctx at a time; the calling thread may block in grim_stream_write while `depth` chunks are in
 * flight. */
typedef struct grim_stream grim_stream;
typedef struct {
  uint32_t chunk_lines;     /* lines per device batch; 0 = 131072 */
  uint32_t depth;           /* chunks in flight; 0 = 4 */
  int32_t n_threads;        /* tokenizer / formatter threads; 0 = grim_default_threads() */
  uint64_t line_offset;     /* global index of the first line (multi-GPU shards keep the reference's line numbers) */
  uint64_t rows_per_chunk;  /* row pool of one chunk; 0 = 32 rows per line to begin with, growing on demand; a value fixes it (never less than one subject's worst case) */
  uint8_t want_text;        /* format the six output texts */
  uint8_t want_log;         /* also text 6: the lines impute_file prints per subject */
  uint8_t want_records;     /* hand every chunk's records to grim_stream_next_records (the caller must drain them) */
  uint8_t timing;           /* per-kernel HIP events (grim_batch_set_timing) */
  uint8_t rows_exact;       /* take rows_per_chunk as it is (no floor): the caller knows that one subject's rows fit */
  uint8_t placed;           /* the out_path files are shared with other writers (the ranks of grim/shard.py): opened without
                             * truncation, and nothing is written until the caller gives a segment its base offsets
                             * (grim_stream_segment_wait / grim_stream_segment_place) */
  const char *out_path[6];  /* per text: file to create and fill, or NULL = keep in memory (grim_stream_text) */
  /* bin_imputation_in_file phase masks (impute.py:2001-2005, 2030-2032): n_masks ids (NUL-terminated, back to back
   * in mask_ids) and per id the bitmask of positions that keep their side; an id missing from the table sends its
   * line to .problem.  NULL = no masks. */
  const char *mask_ids;
  const uint8_t *mask_fixed;
  uint32_t n_masks;
} grim_stream_opts;

typedef struct {
  uint64_t lines, subjects, chunks, reruns;          /* reruns: sub-batches run again after a row-pool overflow */
  uint64_t unsupported;                              /* subjects left out (grim_stream_unsupported) */
  double wall_s;                                     /* open -> finish */
  double tokenize_cpu_s, format_cpu_s, write_cpu_s;  /* summed over the worker threads */
  double device_s;                                   /* device thread busy: copies + kernels + waits */
  double kernel_ms[7];                               /* sums of grim_batch_kernel_ms over the chunks (timing mode): [GRIM_MS_TOTAL .. GRIM_MS_TABLES] */
  uint64_t counters[4];                              /* sums of grim_batch_counters */
  uint64_t text_bytes[7];
  uint64_t bytes_h2d, bytes_d2h;
} grim_stream_stats;

grim_stream *grim_stream_open(grim_ctx *ctx, const grim_graph *g, const grim_dict *dict, const grim_params *prm,
                              const grim_prior_spec *priors, const char *const *pop_names, uint32_t n_pops,
                              const grim_stream_opts *opts);
int grim_stream_write(grim_stream *s, const char *text, uint64_t len);
/* The same, but the caller LENDS the bytes instead of having them copied: they must stay valid and unchanged until
 * grim_stream_finish has returned (or the stream is freed).  Chunks that begin inside the buffer read their lines where
 * they lie ('\n' line ends only).  For a caller that holds its input in memory anyway (a mapped file, a buffer it owns):
 * the reference's counterpart is the file object impute_file reads from (impute.py:2019-2027). */
int grim_stream_write_borrowed(grim_stream *s, const char *text, uint64_t len);
/* the same with universal newlines, as Python's open(): "\r\n" and "\r" end a line too (a "\r\n" may straddle two calls) */
int grim_stream_write_text(grim_stream *s, const char *text, uint64_t len);
/* reads the file in blocks and feeds it through grim_stream_write_text */
int grim_stream_write_file(grim_stream *s, const char *path);
/* Input segments -- what a rank of grim/shard.py feeds: byte ranges of ONE file that are not adjacent (the chunks it pulled
 * from the job's counter; scripts/runfile_mp.py:109-148 gives every worker ONE contiguous range instead).  grim_stream_segment
 * ends the current segment -- the line being filled is complete, with or without its newline -- and starts the next one at
 * global line index next_line_offset.  After grim_stream_finish, grim_stream_segment_end(k) gives the cumulative bytes of
 * the seven texts up to the end of segment k (segment 0 starts at the stream's line_offset), i.e. where segment k's part of
 * every output file ends. */
int grim_stream_segment(grim_stream *s, uint64_t next_line_offset);
uint32_t grim_stream_n_segments(const grim_stream *s);
int grim_stream_segment_end(const grim_stream *s, uint32_t k, uint64_t out[7]);
/* Placed output (opts.placed) -- how the ranks of a sharded job write ONE set of output files without a merge copy (what
 * scripts/runfile_mp.py:143-148 leaves to `cat`): grim_stream_segment_wait blocks until every chunk of the closed segment k
 * is formatted and gives the bytes of its piece of each text; the caller adds up the pieces before it (other ranks') and
 * grim_stream_segment_place writes segment k's buffers at those offsets of the shared files (returns when written). */
int grim_stream_segment_wait(grim_stream *s, uint32_t k, uint64_t sizes[7]);
int grim_stream_segment_place(grim_stream *s, uint32_t k, const uint64_t base[6]);
/* byte offsets of every chunk_lines-th line start of a file, the file size last (universal newlines, as
 * grim_stream_write_text; what scripts/runfile_mp.py:113-124 does with `split -l`, without writing the pieces): the number of
 * entries or -1; *out is the library's, released with grim_free */
int64_t grim_chunk_offsets(const char *path, uint32_t chunk_lines, uint64_t **out);
void grim_free(void *p);
/* worker threads a stream starts when opts.n_threads is 0: cores of this process's affinity mask / ranks on this host
 * (LOCAL_WORLD_SIZE, else WORLD_SIZE), at most 32 */
uint32_t grim_default_threads(void);
/* end of input: processes the last partial chunk and waits until every chunk is written; 0 or <0 (grim_stream_error) */
int grim_stream_finish(grim_stream *s);
const char *grim_stream_error(const grim_stream *s);
/* in-memory texts after grim_stream_finish (which: 0..5 as grim_format, 6 = log) */
const char *grim_stream_text(grim_stream *s, int which, uint64_t *len);
int grim_stream_get_stats(const grim_stream *s, grim_stream_stats *out);
/* The device tokenizer's verdicts so far (complete after grim_stream_finish).  *offered: lines the host's line splitter
 * left to it -- a GL field of 1..144 bytes without '/', on a stream that has the device tokenizer on -- the sum of the
 * chunks' counts.  *handed_back: those of them it flagged and the host's tokenizer took in the fix-up pass.  Either way
 * the output is the same; the difference is a second pass.  Either pointer may be NULL.  0 or -1 (s is NULL). */
int grim_stream_devtok_lines(const grim_stream *s, uint64_t *offered, uint64_t *handed_back);
/* The hash the device dictionary tables are built and probed with: the name packed big-endian into six words, zero
 * padded, then hashed with its length; a name's home slot in a locus's table is hash & (capacity - 1), capacity the
 * smallest power of two >= max(16, 4 * alleles of the locus).  Host code, no GPU needed.  len <= 24, else 0. */
uint32_t grim_tokname_hash(const char *name, uint32_t len);
/* subjects the device could not resolve (GRIM_ST_UNSUPPORTED / GRIM_K_UNSUPPORTED): global line index, reason, id */
uint64_t grim_stream_n_unsupported(const grim_stream *s);
int grim_stream_unsupported(const grim_stream *s, uint64_t k, uint64_t *line, uint32_t *reason, const char **id, uint32_t *id_len);
/* records mode: blocks until the next chunk (in input order) is done; 1 = a chunk, 0 = end of stream, <0 = error.
 * kinds[n_lines]; the subject of line j (kind GRIM_K_DEVICE) is res[j]; its rows are rows[res[j].row_off[t] ...].
 * The pointers stay valid until grim_stream_release_records; the chunk's buffers are not reused before that, so a
 * caller that never releases stalls the stream after `depth` chunks. */
typedef struct {
  uint64_t first_line;
  uint32_t n_lines;
  const uint8_t *kinds;
  const grim_subject_result *res;
  const grim_row *rows;
  void *chunk;
} grim_stream_records;
int grim_stream_next_records(grim_stream *s, grim_stream_records *out);
int grim_stream_release_records(grim_stream *s, grim_stream_records *rec);
void grim_stream_free(grim_stream *s);

/* ======================= M-step of an EM iteration: haplotype / population counts (csrc/grim_em.h) ====================
 * The reference has no counterpart: its sibling EM package folds the rows write_best_hap_race_pairs prints
 * (impute.py:79-99, 2079-2088) on the host.  Here the fold runs on the rows a finished batch holds in HBM.
 * Per subject with status GRIM_ST_OK whose phased rows did not come from Plan C, rows k = 0.. in rank order with
 * probabilities p_k: total = ((p_0 + p_1) + p_2) + ..., w_k = p_k / total; (haplotype a_k, population popa_k) += w_k,
 * then (b_k, popb_k) += w_k.  Every counter is the left-to-right fp64 sum of its contributions in (subject, rank, side)
 * order over all batches in the order they were accumulated: bit for bit the same however the input was cut.
 * A haplotype is its alleles: bit GRIM_KEY_GRAPH_ORDER of a row's key is dropped.
 * n_alleles[slot] = grim_dict_count(slot) when the batches were tokenised: a haplotype that holds an allele id at or above
 * it (an allele private to its subject) is not counted on the device; its contributions come back as spill records, in
 * contract order, for the host to fold by allele text (grim_parsed_allele).
 * first_capacity: haplotype slots to begin with (rounded up to a power of two, at least 64); the table doubles on demand. */
typedef struct grim_em grim_em;
typedef struct {
  uint64_t key;   /* haplotype key, GRIM_KEY_GRAPH_ORDER cleared */
  double w;
  uint32_t batch; /* ordinal of the grim_em_accumulate call, from 0 */
  uint32_t subject, row; /* subject index inside that batch, rank of the row */
  uint16_t pop, side;    /* side 0 = a, 1 = b */
} grim_em_spill_rec; /* 32 bytes */
grim_em *grim_em_create(grim_ctx *ctx, const uint32_t n_alleles[GRIM_MAXL], uint32_t n_pops, uint64_t first_capacity);
/* after grim_batch_run, on a batch whose params have em_mr and out_haps and whose graph has n_pops populations (else -3
 * and a grim_last_error text, nothing launched); synchronous; reads the batch's device arrays, copies no result down */
int grim_em_accumulate(grim_em *em, grim_batch *b);
/* the same on host records as grim_batch_results / grim_stream_next_records hand them out: res[n_subjects], rows[n_rows] are
 * uploaded and run through the same kernels in the same order, the subjects' GRIM_T_PMUG row_off / n_rows read against
 * n_rows (a subject whose rows do not lie inside the rows given is skipped like one without rows).  The call counts as one
 * batch: spill records carry its ordinal, the statistics add up, grim_em_kernel_ms speaks of it.  -3 and a grim_last_error
 * text, nothing uploaded, launched or counted, when res is null with n_subjects > 0, rows is null with n_rows > 0, or
 * n_rows is above 2^31 - 1.  Not defined: a subject whose total is zero, not finite or NaN (the kernels divide by it). */
int grim_em_accumulate_records(grim_em *em, const grim_subject_result *res, uint32_t n_subjects, const grim_row *rows,
                               uint64_t n_rows);
uint64_t grim_em_entries(const grim_em *em); /* (haplotype, population) counters that were added to */
/* keys / pops / counts [grim_em_entries], in (key, population) order */
int grim_em_export(grim_em *em, uint64_t *keys, uint32_t *pops, double *counts);
uint64_t grim_em_spill_count(const grim_em *em);
int grim_em_spill(grim_em *em, uint64_t first, uint64_t n, grim_em_spill_rec *out);
/* [0] subjects used [1] subjects skipped because their phased rows came from Plan C [2] contributions [3] rehashes */
int grim_em_stats(const grim_em *em, uint64_t out[4]);
/* subjects with status GRIM_ST_UNSUPPORTED in the batch of the last grim_em_accumulate (the caller reports them) */
uint64_t grim_em_last_unsupported(const grim_em *em);
/* device time of the last grim_em_accumulate: its kernels between their own start/stop events */
double grim_em_kernel_ms(const grim_em *em);
/* ---- merging tables: the sharded M-step (csrc/grim_em.h has the same text) ----
 * grim_em_accumulate's promise needs a batch's sums to start from the counters the batches before it left.  Accumulators that
 * run at the same time -- one per rank -- cannot give that, so the sharded M-step has a contract of its own:
 *   the input is cut into chunks of chunk_lines lines, chunk c = global lines [c * chunk_lines, ...), as grim_chunk_offsets
 *     cuts it;
 *   T_c = the table of chunk c alone: the M-step above over the chunk's lines into an empty accumulator (batch cuts inside the
 *     chunk stay invisible); S_c = the chunk's spilled counts, (population, haplotype text) -> count, in the chunk's order;
 *   count[k, p] = ((T_c0[k, p] + T_c1[k, p]) + T_c2[k, p]) + ...  fp64, no fma, over the chunks c0 < c1 < ... whose table
 *     holds the entry (k, p), in ascending chunk number; the spilled counts fold the same way.  A first contribution may be
 *     written +0.0 + x: every count is >= +0.0, so these are the same bits.
 * The answer depends on chunk_lines.  It does not depend on the number of ranks, on which rank ran which chunk, on the order
 * in which the tables arrive, or on the batch cuts; with one chunk it is grim_em_accumulate's, bit for bit.  The statistics
 * are the sums over the chunks.  The caller folds: it calls one of the two doors below once per chunk, in chunk order.
 *
 * grim_em_merge(dst, src): every entry of src's table into dst where both lie, no host trip.  One lane per slot of src; for
 *   every set bit p of the slot's popmask the key is found or inserted in dst and dst.count[k, p] = dst.count[k, p] + src.count[k, p].
 * grim_em_merge_records(dst, keys, pops, counts, n): the same add for an exported table, host arrays in grim_em_export's
 *   order, uploaded, one lane per entry.  Both doors add through one device function.
 * Keys are unique within src and (key, pop) pairs within an exported table, so each counter of dst is written by exactly one
 * lane of a call: no floating-point atomics, no order inside a call.  Before the launch dst makes room by its own rule (keys
 * in use plus incoming keys <= capacity / 2), doubling as grim_em_accumulate does; the doublings count in grim_em_stats
 * out[3].  A probe that finds no slot all the same answers -1 ("the haplotype table overflowed").
 * Refusals answer -3 with a grim_last_error text, launch nothing and change no bit of dst (grim_em_merge_ms is cleared
 * first): src == dst; src belongs to another context, has another number of populations or another n_alleles; records
 * door: a null array with n > 0, pops[i] >= n_pops, a key with a bit at or above GRIM_KEY_GRAPH_ORDER, a key field above
 * n_alleles of its slot (an exported table never holds a private allele), entries not strictly ascending in (key, pop), a
 * count that is negative, NaN or infinite -- the checks and texts of grim_graph_refresh_records where they are the same.
 * A merge is not a batch: spill ordinals, grim_em_stats out[0..2], grim_em_last_unsupported and grim_em_kernel_ms do not
 * move.  src's spill list is NOT merged: the caller folds it by allele text, in chunk order.  src is not changed. */
int grim_em_merge(grim_em *dst, grim_em *src);
int grim_em_merge_records(grim_em *dst, const uint64_t *keys, const uint32_t *pops, const double *counts, uint64_t n);
/* device time of the last merge: its kernel, and the doublings before it, between their own start/stop events; 0.0 after a
 * refusal or a merge of nothing.  grim_em_kernel_ms keeps speaking of the last grim_em_accumulate. */
double grim_em_merge_ms(const grim_em *em);
void grim_em_free(grim_em *em);

/* ======================= EM on a fixed support: the graph's frequencies from M-step counts (csrc/grim_refresh.h) =======
 * The reference has no counterpart: after an M-step it writes POP.freqs.gz, regenerates the graph files and loads them again
 * (grim/em.py em_iteration does the same here).  When the support is kept only the numbers in freq change, so the refresh
 * recomputes them where they lie.  The operation, every sum's order included (csrc/grim_refresh.h has the full text):
 *   full nodes f_0 < ... < f_{F-1}: the nodes with node_mask == full_mask, in node-id order;
 *   c[i][p] = the count of (node_key[f_i] with bit GRIM_KEY_GRAPH_ORDER and above dropped, p) when the counts hold that entry,
 *     else +0.0; counts of haplotypes that are not full nodes of the graph take no part;
 *   s_b[p] = ((+0.0 + c[bB][p]) + c[bB+1][p]) + ... over block b of B = GRIM_REFRESH_BLOCK positions,
 *   T_p = ((+0.0 + s_0[p]) + s_1[p]) + ... over the blocks in order (fp64, no fma);
 *   new[f_i][p] = c[i][p] / T_p; for a partial node v, new[v][p] = ((+0.0 + new[r_0][p]) + new[r_1][p]) + ... over its top-link
 *     row a_nbr[a_start[v] .. e(v)) in stored order, e(v) = a_start[v + 1] for v < n_nodes - 1 and n_a_nbr for the last node;
 *   the full-haplotype table's inline frequency of a key becomes new[n][0], n the highest-numbered full node of that key.
 * A graph can be refreshed when, in the descriptor grim_graph_upload was given, the rows of the partial nodes in node order
 * tile a_nbr[0 .. n_a_nbr) without gap or overlap, every row is non-empty, every entry is a full node and every entry's key cut
 * to the slots of node_mask[v] equals node_key[v] (every graph grim_graphgen_csv makes).  grim_graph_upload decides that and
 * keeps the answer; what it returns and uploads does not change.
 * Refusals answer -3 with a grim_last_error text, launch nothing that writes and leave every bit of the graph's frequencies as
 * it was: the graph is not refreshable; the accumulator belongs to another context or has another number of populations;
 * records door: a null array with n > 0, pops[i] >= n_pops, a key with a bit at or above GRIM_KEY_GRAPH_ORDER, entries not
 * strictly ascending in (key, pop), a count that is negative, NaN or infinite; some T_p is not finite or not > 0.0 (a
 * population without any count inside the support; `stats` then holds the totals and n_full, everything else 0).
 * The new values are computed into a shadow buffer and committed in place, at the same device addresses, after the totals were
 * read.  The caller guarantees that no batch or stream of this graph is in flight; the call synchronises the context's stream
 * before its first launch and before it returns.  No floor, no pseudo-count, no new haplotypes.  The counts of several
 * devices come in as one table: their chunk tables folded in chunk order (grim_em_merge_records), then this call's records
 * door on every device. */
#define GRIM_REFRESH_BLOCK 4096 /* positions of one block of the totals' two-level fold */
typedef struct {
  double total[GRIM_MAXPOP]; /* T_p */
  double delta;              /* the largest |new - old| over the full nodes and populations */
  uint64_t matched;          /* (full node, population) pairs with an entry in the counts */
  uint64_t zero_full;        /* full nodes whose new vector is all zero */
  uint64_t n_full;           /* F */
} grim_refresh_stats;
/* the counts of an accumulator, where its table lies; stats may be NULL */
int grim_graph_refresh(grim_graph *g, grim_em *em, grim_refresh_stats *stats);
/* the counts as host arrays keys / pops / counts [n] in grim_em_export's order */
int grim_graph_refresh_records(grim_graph *g, const uint64_t *keys, const uint32_t *pops, const double *counts, uint64_t n,
                               grim_refresh_stats *stats);
/* out[n_nodes][n_pops]: the frequencies as they lie on the device */
int grim_graph_freq(grim_graph *g, double *out);
/* device time of the last refresh that launched: its kernels and the commit between their own start/stop events */
double grim_graph_refresh_ms(const grim_graph *g);
/* 1 when grim_graph_upload found the graph refreshable, else 0 */
int grim_graph_refreshable(const grim_graph *g);

/* ======================= marginal genotype tables on a subset of the loci (csrc/grim_marginal.h) ======================
 * What scripts/reduce_loci.py does to a printed .umug file -- drop a locus from every genotype, add the probabilities of
 * genotypes that became equal, sort again, keep the top rows -- on the genotype rows a finished batch holds in HBM, for any
 * set of kept loci.
 * keep_mask: bit s = locus slot s is kept.  Per subject with status GRIM_ST_OK, GRIM_T_UMUG rows k = 0.. in rank order,
 * row k = (a_k, b_k, p_k):
 *   reduced genotype of row k: for every kept slot the UNORDERED pair of the slot's 12-bit fields of a_k and b_k (compared
 *     on (min, max): which haplotype carries which allele is not canonical between rows); bit GRIM_KEY_GRAPH_ORDER and the
 *     fields outside keep_mask are dropped; a field of 0 (locus not typed) is a value like any other;
 *   group: the first row of a reduced genotype leads it; its sum = (p_leader + p_j) + p_l ... over its rows in rank order
 *     (left-to-right fp64, no atomics, no tree sums);
 *   rank: sums descending, ties in the leaders' order (stable): the number of groups with a larger sum, or an equal sum and
 *     an earlier leader;
 *   output: the first min(groups, max_rows) groups as grim_row records (a, b = the leader's keys masked to the kept slots,
 *     prob = the sum, popa = popb = 0) and a grim_subject_result copy (status / plan / reason copied, n_genotypes = groups,
 *     n_rows[GRIM_T_UMUG] = rows written, row_off[GRIM_T_UMUG] into the output rows, everything else 0).  Subjects that are
 *     not GRIM_ST_OK or have no GRIM_T_UMUG rows, or whose rows do not lie inside the rows given, produce no rows.
 * Not defined: a row whose a and b occupy different sets of slots (grim_format pairs the printed alleles by index); such
 * subjects are counted in the statistics and the caller decides.
 * The records print through grim_format with out_muug = 1, out_haps = 0 (text 0); every subject is independent, so the cuts
 * of the input into batches cannot show. */
typedef struct grim_marginal grim_marginal;
grim_marginal *grim_marginal_create(grim_ctx *ctx, uint32_t keep_mask, uint32_t max_rows);
/* after grim_batch_run; synchronous; reads the batch's device arrays, copies no result of the batch down.  -3 and a
 * grim_last_error text, nothing launched and the reducer left empty, when the batch belongs to another context, holds no
 * finished run, was built with out_muug off, or keep_mask is 0 or has bits outside the graph's loci */
int grim_marginal_reduce(grim_marginal *m, grim_batch *b);
/* the same on host records as grim_batch_results / grim_stream_next_records hand them out: res[n_subjects], rows[n_rows]
 * are uploaded and run through the same kernels (-3 when keep_mask is 0 or has bits from GRIM_MAXL up) */
int grim_marginal_reduce_records(grim_marginal *m, const grim_subject_result *res, uint32_t n_subjects, const grim_row *rows,
                                 uint64_t n_rows);
/* of the last reduce: result copies, and the extent of the output rows (subject regions lie apart: use row_off) */
uint32_t grim_marginal_subjects(const grim_marginal *m);
uint32_t grim_marginal_total_rows(const grim_marginal *m);
/* res[grim_marginal_subjects], rows[grim_marginal_total_rows]; rows no region uses are zero */
int grim_marginal_results(grim_marginal *m, grim_subject_result *res, grim_row *rows);
/* of the last reduce: [0] subjects reduced [1] rows in [2] groups [3] rows out [4] subjects with a row that is not defined */
int grim_marginal_stats(const grim_marginal *m, uint64_t out[5]);
/* device time of the last reduce: its kernels between their own start/stop events */
double grim_marginal_kernel_ms(const grim_marginal *m);
void grim_marginal_free(grim_marginal *m);

/* ======================= match probabilities between imputed subjects (csrc/grim_match.h) ==============================
 * For every (patient, donor) pair the probability of 0, 1, 2, ... allele mismatches over a set K of kept loci (a 10/10, a
 * 9/10, an 8/8 match) and the per-locus match probabilities, from the genotype rows the two sides' batches hold; the
 * reference stops at the printed .umug files.
 * keep_mask: bit s = locus slot s is in K.  n_alleles[slot] = the dictionary size when the sides were tokenised (as
 * grim_em_create takes it).  Of a subject its GRIM_T_UMUG rows k = 0..n-1 in rank order are used, row k = (a_k, b_k, p_k).
 *   flags per subject (both sides):
 *     GRIM_MATCH_VALID      status GRIM_ST_OK, n >= 1, row_off / n_rows inside the rows given, and
 *                           total = ((p_0 + p_1) + p_2) + ... (fp64, left to right) finite and > 0
 *     GRIM_MATCH_PRIVATE    a row holds, in a slot of K, a key field above n_alleles[slot]: an allele private to the subject
 *     GRIM_MATCH_UNDEFINED  a row has a slot (any) typed on one haplotype and 0 on the other
 *     (PRIVATE and UNDEFINED are looked for whenever the subject's rows can be read, whatever the total)
 *   weights w_k = p_k / total; bit GRIM_KEY_GRAPH_ORDER and the fields outside K are dropped;
 *   row pair, patient row i = (a, b), donor row j = (c, d), per slot s of K with the 12-bit fields x1, x2 of a, b and y1, y2
 *     of c, d: eq(x, y) = x == y and x != 0 (an untyped field equals nothing);
 *     mm_s = 2 - max(eq(x1,y1) + eq(x2,y2), eq(x1,y2) + eq(x2,y1)); M(i,j) = the sum of mm_s over K, in 0..2|K|;
 *   pair record, every sum in this order (w the patient's weights, v the donor's):
 *     H[*] = 0.0, L[*] = 0.0
 *     for j = 0..n_d-1 (donor rows, rank order):
 *       ph[*] = 0.0, pl[*] = 0.0
 *       for i = 0..n_p-1 (patient rows, rank order): t = w_i * v_j (one multiply, no fma); ph[M(i,j)] = ph[M(i,j)] + t;
 *                                                    for s in K with mm_s == 0: pl[s] = pl[s] + t
 *       H[m] = H[m] + ph[m] for every m, L[s] = L[s] + pl[s] for every s in K
 *     mm[m] = H[m] (0.0 for m > 2|K|), locus[s] = L[s] for s in K and 0.0 elsewhere: equal inputs give equal bits.
 *   A pair is computed iff both subjects are VALID and neither is PRIVATE; otherwise its record is all zero bytes (the caller
 *   matches pairs left out for PRIVATE by allele text, grim_parsed_allele).  Results are patient-major: out[p * donors + d]. */
#define GRIM_MATCH_MAX_PAIRS (1u << 24) /* patients x donors of one run: 2 GiB of result records */
#define GRIM_MATCH_VALID 1
#define GRIM_MATCH_PRIVATE 2
#define GRIM_MATCH_UNDEFINED 4
typedef struct {
  double mm[2 * GRIM_MAXL + 1]; /* mm[m]: probability of m mismatching alleles over K */
  double locus[GRIM_MAXL];      /* locus[s]: probability of no mismatch at slot s */
} grim_match_rec; /* 128 bytes */
typedef struct grim_match grim_match;
grim_match *grim_match_create(grim_ctx *ctx, uint32_t keep_mask, const uint32_t n_alleles[GRIM_MAXL]);
/* the patients as host records (grim_batch_results hands them out): uploaded, prepared on the device and kept across runs
 * until set again.  Every call below answers -3 with a grim_last_error text, launches nothing and leaves no results (donors
 * 0, statistics 0, kernel_ms 0; a refused grim_match_set_patients leaves no patients either) when it refuses:
 * keep_mask is 0 or has bits from GRIM_MAXL up (here and in grim_match_run_records) or bits outside the graph's loci
 * (grim_match_run); the batch belongs to another context, holds no finished run or was built with out_muug off; no patients
 * were set; patients x donors is above GRIM_MATCH_MAX_PAIRS. */
int grim_match_set_patients(grim_match *m, const grim_subject_result *res, uint32_t n, const grim_row *rows, uint32_t n_rows);
/* the subjects of a finished batch as donors, where their rows lie in HBM; synchronous; copies no result of the batch down */
int grim_match_run(grim_match *m, grim_batch *donors);
/* the same with donors given as host records */
int grim_match_run_records(grim_match *m, const grim_subject_result *res, uint32_t n, const grim_row *rows, uint32_t n_rows);
uint32_t grim_match_patients(const grim_match *m); /* as set */
uint32_t grim_match_donors(const grim_match *m);   /* of the last run */
/* of the last run: out[patients * donors], patient_flags[patients], donor_flags[donors]; a null pointer skips that part */
int grim_match_results(grim_match *m, grim_match_rec *out, uint8_t *patient_flags, uint8_t *donor_flags);
/* of the last run (all 0 when it had no donors): [0] patients valid [1] donors valid [2] patients private [3] donors private
 * [4] subjects of either side with a row that is not defined [5] pairs computed [6] row pairs evaluated [7] 0 */
int grim_match_stats(const grim_match *m, uint64_t out[8]);
/* device time of the last run: preparing the donors, clearing the records and the pair kernel between start/stop events */
double grim_match_kernel_ms(const grim_match *m);
void grim_match_free(grim_match *m);

/* Mismatch direction and per-locus grades (csrc/grim_match.h).  Everything of the block above holds -- the flags, the
 * weights, patient-major results, the donor-row outer fold, the patient-row inner fold, +0.0 starts, no fma, the statistics --
 * except the per-slot mismatch function and, when graded, the record.  With x1, x2 the patient's fields of a slot, y1, y2 the
 * donor's and eq(x, y) = x == y and x != 0:
 *   GRIM_MATCH_DIR_EITHER  mm_s as above
 *   GRIM_MATCH_DIR_GVH     mm_s = !(eq(x1,y1) || eq(x1,y2)) + !(eq(x2,y1) || eq(x2,y2)): the patient's alleles the donor lacks
 *                          (graft versus host); both copies are counted, an untyped field is always lacking
 *   GRIM_MATCH_DIR_HVG     the same with the roles of x and y exchanged: the donor's alleles the patient lacks (host versus graft)
 *   either == max(gvh, hvg) for all fields, 0 included; so the row pairs with M == 0 under either are among those under gvh
 *   (and under hvg), and, rounded addition being monotone, mm_gvh[0] >= mm_either[0] and mm_hvg[0] >= mm_either[0] exactly.
 * Graded record: grade[s][g] is the two-level fold of locus[s] with the condition mm_s == g in the place of mm_s == 0, 0.0 for
 * s outside K.  mm[] is bit-identical to the ungraded record of the same direction and grade[s][0] to its locus[s].  A pair
 * that is not computed is all zero bytes.  The result buffer is sized by the record in use; GRIM_MATCH_MAX_PAIRS is the same
 * for both: a full graded run is 3.25 GiB of result records. */
#define GRIM_MATCH_DIR_EITHER 0
#define GRIM_MATCH_DIR_GVH 1
#define GRIM_MATCH_DIR_HVG 2
typedef struct {
  double mm[2 * GRIM_MAXL + 1]; /* mm[m]: probability of m mismatching alleles over K */
  double grade[GRIM_MAXL][3];   /* grade[s][g]: probability of exactly g mismatches at slot s */
} grim_match_grade_rec; /* 208 bytes */
/* grim_match_create is this with (GRIM_MATCH_DIR_EITHER, 0): that matcher runs the kernel it always ran.  NULL with a
 * grim_last_error text when direction is above GRIM_MATCH_DIR_HVG.  graded: not 0 = the records are grim_match_grade_rec. */
grim_match *grim_match_create_ex(grim_ctx *ctx, uint32_t keep_mask, const uint32_t n_alleles[GRIM_MAXL], uint32_t direction,
                                 int graded);
/* grim_match_results of a graded matcher.  Each of the two answers -3 with a text on a matcher of the other kind, and as
 * every refusal leaves no results (donors 0, statistics 0, kernel_ms 0; the patients stay). */
int grim_match_results_graded(grim_match *m, grim_match_grade_rec *out, uint8_t *patient_flags, uint8_t *donor_flags);
uint32_t grim_match_direction(const grim_match *m); /* as created */
int grim_match_graded(const grim_match *m);         /* 1 or 0, as created */

/* ======================= donor search: each patient's best N donors (csrc/grim_search.h) ================================
 * The match records above, computed run by run, and on the device a selection of every patient's first top_n donors over all
 * runs: only patients x top_n hits come down, once, however many donor runs were streamed.
 * Inputs: those of the match block (keep_mask, n_alleles, patients set once, donors in any number of runs), and
 *   top_n in 1..GRIM_SEARCH_MAX_N; a threshold min_p0, a double that is not NaN; per run one uint32_t id per donor, distinct
 *   over the whole search and the caller's own.
 * Candidates: a pair (p, d) is a candidate iff it is computed (both subjects GRIM_MATCH_VALID, neither GRIM_MATCH_PRIVATE;
 *   decided from the flags, not from the record's bytes) and rec.mm[0] >= min_p0.  Every mm value of a computed pair is finite
 *   and >= +0.0, so plain > and == on doubles are a total preorder: there is no NaN to handle.
 * Order: candidate x comes before candidate y iff x.mm[0] > y.mm[0]; or the mm[0] are equal and x.mm[1] > y.mm[1] (mm[1]
 *   always exists, 2|K| >= 2); or both are equal and x.id < y.id.  Ids are distinct, so the order is strict: the answer does
 *   not depend on how the selection is done, on tile size, on block cuts or on the order of the runs.  No floating-point
 *   operation is added: the records are the match block's, bit for bit.
 * Result per patient: a count n_hits <= top_n and top_n slots of grim_search_hit.  The first n_hits slots hold the first
 *   candidates in that order over all runs since the patients were set or the search was reset; the other slots are donor =
 *   GRIM_SEARCH_NO_DONOR with a zero record.  Results are patient-major: hits[p * top_n + k].
 * Statistics: the match block's seven counters, each run's summed, and [7] candidates: the pairs that passed the threshold,
 *   counted as u64 on the device.
 * Environment, read when a search is created: GRIM_SEARCH_TILE=n, the entries a workgroup sorts at a time, a power of two with
 *   2 top_n <= n <= GRIM_SEARCH_TILE_MAX (the default); for tests: small tiles make deep reduction trees on small inputs. */
#define GRIM_SEARCH_MAX_N 256u
#define GRIM_SEARCH_TILE_MAX 2048u
#define GRIM_SEARCH_NO_DONOR 0xFFFFFFFFu
typedef struct {
  uint32_t donor;    /* the donor's id as the caller gave it */
  uint32_t reserved; /* 0 */
  grim_match_rec rec;
} grim_search_hit; /* 136 bytes */
typedef struct grim_search grim_search;
/* NULL with a grim_last_error text when top_n is 0 or above GRIM_SEARCH_MAX_N, min_p0 is NaN or GRIM_SEARCH_TILE is not as
 * above */
grim_search *grim_search_create(grim_ctx *ctx, uint32_t keep_mask, const uint32_t n_alleles[GRIM_MAXL], uint32_t top_n, double min_p0);
/* grim_search_create is this with GRIM_MATCH_DIR_EITHER.  The search owns an ungraded matcher of that direction (NULL with a
 * text when it is above GRIM_MATCH_DIR_HVG); candidates, threshold and order are the ones above on the directed mm[0] and
 * mm[1], and the hits hold the directed records.  The merge door cannot know the direction of a list it is given: lists of
 * one direction are the caller's duty, as distinct ids are. */
grim_search *grim_search_create_ex(grim_ctx *ctx, uint32_t keep_mask, const uint32_t n_alleles[GRIM_MAXL], uint32_t top_n,
                                   double min_p0, uint32_t direction);
/* as grim_match_set_patients; also empties the hit lists and the summed statistics */
int grim_search_set_patients(grim_search *s, const grim_subject_result *res, uint32_t n, const grim_row *rows, uint32_t n_rows);
/* empties the hit lists and the summed statistics; the patients stay */
int grim_search_reset(grim_search *s);
/* the subjects of a finished batch as donors, donor_ids[subjects of the batch] (host memory); synchronous.  Answers -3 with a
 * text when donor_ids is null with donors, and with the matcher's own text whenever the match block refuses.  A refused or
 * failed run adds nothing: the hit lists and the summed statistics are what they were before it. */
int grim_search_run(grim_search *s, grim_batch *donors, const uint32_t *donor_ids);
/* the same with donors given as host records, donor_ids[n] */
int grim_search_run_records(grim_search *s, const grim_subject_result *res, uint32_t n, const grim_row *rows, uint32_t n_rows,
                            const uint32_t *donor_ids);
/* The merge door: hit lists that another search produced (a rank's, a saved one, one folded on the host) become inputs of the
 * same selection.  hits[(l * n_patients + p) * top_n + k], n_hits[l * n_patients + p]: n_lists lists in the layout the results
 * call below writes, each with this search's own top_n slots per patient (host memory); synchronous.
 *   Entries: of list l and patient p the first n_hits slots are entries (donor, rec); later slots are not looked at.
 *   Candidates: an entry is a candidate iff rec.mm[0] >= min_p0, the search's own threshold; a list made under a lower
 *     threshold is filtered.  The patients' flags are not consulted: a hit is a record some search computed, on the device or on
 *     allele text.
 *   Selection: the new running list of patient p is the first top_n, in the strict order above, of (its running list so far)
 *     united with (the candidates of all lists).  Records and ids are copied bit for bit, reserved = 0; unused slots are
 *     GRIM_SEARCH_NO_DONOR with a zero record; no floating-point operation is added.  Runs and merges that follow see the merged
 *     list as the running list.
 *   Distinct ids over everything a search has seen remain the caller's duty, as for runs.  A repeat across lists is not
 *     detected: both entries are kept and nothing faults.
 *   Left alone: the eight summed statistics; the donors and flags calls still speak of the last run and the matcher is not
 *     touched.  The two device times become the merge's, between the search's own event pair.
 *   Answers -3 with a text, checked on the host before any upload and after the two times were cleared, the running lists and
 *     sums exactly as they were: n_patients is not the number of patients set; a null array with something to read; n_lists
 *     above GRIM_SEARCH_MERGE_MAX_LISTS; some n_hits above top_n; an entry with donor = GRIM_SEARCH_NO_DONOR or reserved != 0;
 *     an entry whose mm[0] or mm[1] is NaN, infinite or < 0; a list whose entries are not in the strict order for some patient
 *     (entry k + 1 must come after entry k; this also catches an id repeated within a list).
 *   Answers 0 and changes nothing when n_lists is 0 or there are no patients; -1 for a null handle, and for a failed device
 *     call or allocation, which changes nothing: the lists change hands only after everything has worked. */
#define GRIM_SEARCH_MERGE_MAX_LISTS 4096u
int grim_search_merge_hits(grim_search *s, const grim_search_hit *hits, const uint32_t *n_hits, uint32_t n_patients, uint32_t n_lists);
/* hits[patients * top_n], n_hits[patients], over all runs so far; a null pointer skips that part */
int grim_search_results(grim_search *s, grim_search_hit *hits, uint32_t *n_hits);
/* patient_flags[patients], donor_flags[donors of the last run]; a null pointer skips that part */
int grim_search_flags(grim_search *s, uint8_t *patient_flags, uint8_t *donor_flags);
uint32_t grim_search_patients(const grim_search *s); /* as set */
uint32_t grim_search_donors(const grim_search *s);   /* of the last run */
uint32_t grim_search_top_n(const grim_search *s);
int grim_search_stats(const grim_search *s, uint64_t out[8]);
/* device time of the last run: the match block's kernels plus the selection */
double grim_search_kernel_ms(const grim_search *s);
/* device time of the last run's selection kernels alone, between their own start/stop events */
double grim_search_select_ms(const grim_search *s);
void grim_search_free(grim_search *s);

/* ======================= allele groups: the consumers above at a chosen resolution (csrc/grim_groups.h) =================
 * The marginal tables, the match and the search compare alleles by dictionary id: at the resolution the graph was built at.
 * A group map puts a mapping pass in front of their kernels, which stay exactly as they are.
 * Group map: for every locus slot s a table T_s[0 .. n_alleles[s]] of uint16_t and a count n_groups[s].  T_s[0] == 0 (untyped
 *   stays untyped); 1 <= T_s[f] <= n_groups[s] for 1 <= f <= n_alleles[s]; every group id in 1..n_groups[s] occurs; hence
 *   n_groups[s] <= n_alleles[s] <= 4095.  A slot with T_s[f] = f is an identity slot; watch_mask = the slots that are not.
 * Mapped row: (a, b, prob, popa, popb) -> (map(a), map(b), prob, popa, popb); the 12-bit field f of slot s becomes
 *     0                                  if f == 0
 *     T_s[f]                             if 1 <= f <= n_alleles[s]
 *     n_groups[s] + (f - n_alleles[s])   if f > n_alleles[s]: an allele private to the subject stays private, distinct from
 *                                        every group and from the subject's other private alleles, and keeps its index;
 *   the result is <= f, so a field never overflows.  Key bits at GRIM_KEY_GRAPH_ORDER and above are copied.  No
 *   floating-point operation takes place.
 * Consumers on mapped rows: with a map attached a consumer runs its contract above on the mapped rows, n_groups in the place
 *   of n_alleles, every rule word for word: the marginal's leaders, left-to-right sums and ranks; the matcher's flags, eq,
 *   M(i,j) and fold order (GRIM_MATCH_PRIVATE: a field above n_groups[s] in a slot of K); the search's order.  With every slot
 *   an identity slot every output byte equals the call without a map.  Without a map a consumer executes exactly the launches
 *   it did before.
 * Private alleles are the host's: the device cannot know which group an unseen allele's text belongs to.  Match and search
 *   leave such pairs out as before (the caller folds them on group names).  The marginal flags a subject
 *   GRIM_GROUPS_PRIVATE when its rows can be read (status GRIM_ST_OK, rows inside the rows given) and some GRIM_T_UMUG row
 *   holds a private field in a slot of keep_mask & watch_mask; the caller folds those subjects on text.  Private alleles in
 *   identity slots need no special case.
 * Environment, read when a map is created: GRIM_GROUPS_LDS=0 makes the map kernel read the tables where they lie instead of
 *   staging them in LDS in every workgroup, the default (for measurements). */
#define GRIM_GROUPS_PRIVATE 1
typedef struct grim_groups grim_groups;
/* table: the slots' tables back to back, each of length n_alleles[s] + 1.  Every rule above is checked on the host before any
 * upload; a refusal returns NULL with a grim_last_error text that names the slot and the entry, and launches nothing */
grim_groups *grim_groups_create(grim_ctx *ctx, const uint16_t *table, const uint32_t n_alleles[GRIM_MAXL],
                                const uint32_t n_groups[GRIM_MAXL]);
void grim_groups_free(grim_groups *g);
uint32_t grim_groups_watch_mask(const grim_groups *g);
/* rows[n_rows] (host) uploaded, mapped, downloaded into out[n_rows]; synchronous.  n_rows == 0 answers 0 with no launch; -3
 * for a null array with rows or n_rows above 2^31 - 1 */
int grim_groups_map_records(grim_groups *g, const grim_row *rows, uint64_t n_rows, grim_row *out);
/* device time of the map kernel of the last grim_groups_map_records, between its own start/stop events (64 bytes move per
 * row) */
double grim_groups_kernel_ms(const grim_groups *g);
/* Attach a map to a consumer (g == NULL detaches).  The consumer copies the tables device to device into a buffer of its own:
 * g may be freed right after.  The last results are cleared first.  -3 with a text: g belongs to another context; for match
 * and search, g's n_alleles differ from the ones given at create.  On a matcher, setting or detaching drops the patients, as
 * grim_match_set_patients does first; on a search it also empties the hit lists and the summed statistics: rows prepared, or
 * hits computed, at one resolution never meet another.  From then on both doors of the consumer (and
 * grim_match_set_patients) map the rows into a buffer of the consumer's between its two event records -- kernel_ms includes
 * the pass -- and hand that buffer to the kernels in place of the rows.  grim_search_merge_hits is untouched. */
int grim_marginal_set_groups(grim_marginal *m, const grim_groups *g);
int grim_match_set_groups(grim_match *m, const grim_groups *g);
int grim_search_set_groups(grim_search *s, const grim_groups *g);
/* out[grim_marginal_subjects]: GRIM_GROUPS_PRIVATE or 0 per subject of the last reduce; all zero when it ran without a map */
int grim_marginal_flags(grim_marginal *m, uint8_t *out);

#ifdef __cplusplus
}
#endif
#endif
