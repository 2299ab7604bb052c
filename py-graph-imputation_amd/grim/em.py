"""
The M-step of an EM iteration over the imputation: per-population haplotype counts from the phased `hap;pop` rows.

The reference has no M-step of its own -- its sibling EM package folds the rows `write_best_hap_race_pairs` prints
(impute.py:79-99, 2079-2088).  The operation is defined here:

    for every subject, in input-line order, with phased rows k = 0..n-1 in rank order and probabilities p_k
        (a subject whose phased rows came from Plan C -- populations `all_pops` -- is skipped and counted):
      total = ((p_0 + p_1) + p_2) + ...
      w_k   = p_k / total
      count[pop a_k][hap a_k] += w_k, then count[pop b_k][hap b_k] += w_k          for k = 0, 1, ...

Every counter is the left-to-right fp64 sum of its contributions in (line, rank, side) order.

`m_step_counts` runs it on the device, on the rows a batch leaves in HBM (csrc/grim_em.h): no text is formatted, no row
is copied to the host.  `fold_pmug_text` is the same fold over `.pmug` text in plain Python floats, `fold_records` the same
over record arrays as `EmAccumulator.accumulate_records` takes them.  Device and twins agree bit for bit.  There is no CPU
fallback of `m_step_counts`.

`m_step_chunked` is the M-step by the sharded contract on one device: the input in chunks of `chunk_lines` lines,
each chunk's table built in an empty accumulator, the tables merged on the device in chunk order; `merge_tables` and
`fold_chunk_tables` are its CPU twins, `grim.shard.m_step_sharded` the same across ranks.
"""

import gzip
import os

import numpy as np

from . import _native as nat
from .blocks import Blocks, note_unsupported, read_lines

ALL_POPS = "all_pops"


def fold_pmug_text(text):
    """`.pmug` text in `id,hap;pop,hap;pop,p,rank` form -> ({pop: {haplotype: count}}, stats).  A subject is the run of rows
    from one rank 0 to the next; a subject with an `all_pops` row is skipped (stats["skipped_plan_c"])."""
    counts = {}
    stats = {"subjects_used": 0, "skipped_plan_c": 0, "contributions": 0}

    def flush(rows):
        if not rows:
            return
        if any(pa == ALL_POPS or pb == ALL_POPS for _, pa, _, pb, _ in rows):
            stats["skipped_plan_c"] += 1
            return
        total = rows[0][4]
        for r in rows[1:]:
            total = total + r[4]
        if not total > 0.0:
            raise ValueError("phased rows whose probabilities add up to %r" % total)
        for ha, pa, hb, pb, p in rows:
            w = p / total
            for hap, pop in ((ha, pa), (hb, pb)):
                d = counts.setdefault(pop, {})
                d[hap] = d[hap] + w if hap in d else w
        stats["subjects_used"] += 1
        stats["contributions"] += 2 * len(rows)

    rows, sid = [], None
    for line in text.splitlines():
        if not line:
            continue
        f = line.split(",")
        if len(f) != 5 or ";" not in f[1] or ";" not in f[2]:
            raise ValueError("not a hap;pop,hap;pop row: %r" % line)
        if int(f[4]) == 0 or f[0] != sid:
            flush(rows)
            rows, sid = [], f[0]
        if int(f[4]) != len(rows):
            raise ValueError("ranks of subject %s are not 0..n-1" % f[0])
        ha, pa = f[1].rsplit(";", 1)
        hb, pb = f[2].rsplit(";", 1)
        rows.append((ha, pa, hb, pb, float(f[3])))
    flush(rows)
    return counts, stats


def fold_records(res, rows, n_alleles, n_pops, batch=0, carry=None):
    """The fold on record arrays (nat.RESULT_DT[n], nat.ROW_DT[m]) as grim_em_accumulate_records defines it (the header
    comment of csrc/grim_em.h), in plain Python floats -> (keys u64, pops u32, counts f64, spill SPILL_DT, stats).

    A subject is skipped when its status is not OK, it has no phased (T_PMUG) rows, its rows do not lie inside `rows`, or its
    effective plan (`plan_phased` when non-zero, else `plan`) is `c`; the last is counted in stats["skipped_plan_c"] when the
    subject is OK and has rows, wherever they point.  total = ((p_0 + p_1) + p_2) ..., w_k = p_k / total (ValueError unless
    total > 0.0); row k adds w_k to (a_k & keymask, popa_k), then to (b_k & keymask, popb_k), keymask dropping bit 60 and
    above.  A contribution whose population is `n_pops` or more, or one of whose 12-bit fields is above `n_alleles[slot]`,
    goes to the spill list instead, in (subject, row, side) order with the fields of grim_em_spill_rec (`batch` as given,
    `pop` cut to 16 bits as the record holds it).  Entries leave in (key, population) order, as grim_em_export writes them.
    stats: subjects_used, skipped_plan_c, contributions (spilled ones included) and unsupported (subjects with status
    UNSUPPORTED), of this call.

    Cuts: fold every cut with one `carry` dict ((key, population) -> count; updated in place) and the call's ordinal as
    `batch`.  Each call returns the entries of the whole dict so far, and the spill list and stats of that call alone."""
    n_pops = int(n_pops)
    limits = [int(x) for x in n_alleles] + [0] * (nat.MAXL - len(n_alleles))
    keymask = (1 << 60) - 1
    table = {} if carry is None else carry
    m = len(rows)
    res = np.ascontiguousarray(res, dtype=nat.RESULT_DT)
    rows = np.ascontiguousarray(rows, dtype=nat.ROW_DT)
    A, B, PR = rows["a"].tolist(), rows["b"].tolist(), rows["prob"].tolist()
    PA, PB = rows["popa"].tolist(), rows["popb"].tolist()
    status, plan, plan_phased = res["status"].tolist(), res["plan"].tolist(), res["plan_phased"].tolist()
    offs, cnts = res["row_off"][:, nat.T_PMUG].tolist(), res["n_rows"][:, nat.T_PMUG].tolist()
    stats = {"subjects_used": 0, "skipped_plan_c": 0, "contributions": 0, "unsupported": 0}
    spill = []
    private = {}  # key -> whether one of its fields is above the dictionary
    used = []
    for s in range(len(res)):
        stats["unsupported"] += status[s] == nat.ST_UNSUPPORTED
        if status[s] != nat.ST_OK or cnts[s] == 0:
            continue
        if (plan_phased[s] or plan[s]) == ord("c"):
            stats["skipped_plan_c"] += 1
            continue
        if offs[s] > m or cnts[s] > m - offs[s]:
            continue
        used.append(s)
    if sum(cnts[s] for s in used) > m:
        raise ValueError("the subjects' phased rows overlap (more rows than there are)")
    for s in used:
        off, n = offs[s], cnts[s]
        total = PR[off]
        for k in range(1, n):
            total = total + PR[off + k]
        if not total > 0.0:
            raise ValueError("subject %d: phased rows whose probabilities add up to %r" % (s, total))
        for k in range(n):
            w = PR[off + k] / total
            for side, (key, pop) in enumerate(((A[off + k], PA[off + k]), (B[off + k], PB[off + k]))):
                key &= keymask
                priv = private.get(key)
                if priv is None:
                    priv = private[key] = any(((key >> (nat.ABITS * q)) & 0xFFF) > limits[q] for q in range(nat.MAXL))
                if priv or pop >= n_pops:
                    spill.append((key, w, batch, s, k, pop & 0xFFFF, side))
                else:
                    at = (key, pop)
                    table[at] = table[at] + w if at in table else w
        stats["subjects_used"] += 1
        stats["contributions"] += 2 * n
    order = sorted(table)
    keys = np.array([k for k, _ in order], dtype=np.uint64)
    pops = np.array([p for _, p in order], dtype=np.uint32)
    counts = np.array([table[at] for at in order], dtype=np.float64)
    return keys, pops, counts, np.array(spill, dtype=nat.SPILL_DT), stats


def _accumulate_blocks(imputation, shared, lines, block_lines, acc, first=0):
    """The block loop of the M-step: `lines` in blocks of `block_lines`, each tokenised, imputed as one device batch of
    `shared` (a Blocks) and added to the accumulator `acc` where its rows lie.  -> (spilled, kernel_ms, blocks); spilled:
    (pop index, haplotype text) -> count, the haplotypes that hold an allele the dictionary does not know.  Resets and fills
    imputation.unsupported; `first`: the input line `lines` begins at (unsupported subjects are reported by input line)."""
    n_slots = len(imputation.netGraph.full_loci)
    imputation.unsupported = []
    spilled = {}
    kernel_ms = 0.0
    n_blocks = 0
    cut = shared.cut(lines, max(1, int(block_lines)), first)
    try:
        for block in cut:
            bad = block.bad
            if block.batch is not None:
                seen = acc.spill_count()
                acc.accumulate(block.batch)
                kernel_ms += acc.kernel_ms()
                n_blocks += 1
                if acc.last_unsupported():
                    bad = bad + block.unsupported()
                for rec in acc.spill(seen):
                    line, key = int(block.line_of[int(rec["subject"])]), int(rec["key"])
                    fields = [(s, (key >> (nat.ABITS * s)) & 0xFFF) for s in range(n_slots)]
                    name = "~".join(block.parsed.allele(line, s, a - 1) for s, a in fields if a)
                    at = (int(rec["pop"]), name)
                    spilled[at] = spilled[at] + float(rec["w"]) if at in spilled else float(rec["w"])
            note_unsupported(imputation, bad)
    finally:
        cut.close()
    return spilled, kernel_ms, n_blocks


def _counts_by_name(hap_name, pops, table, spilled):
    """an exported table (keys, pops, counts) and the spilled counts -> {pop: {haplotype: count}}; hap_name: key -> the
    haplotype's name (Graph.key_to_name); a population index beyond `pops` is named by its number"""
    keys, kpops, vals = table
    counts = {}
    names = {}
    for key, p, v in zip(keys.tolist(), kpops.tolist(), vals.tolist()):
        name = names.get(key)
        if name is None:
            name = names[key] = hap_name(key)
        counts.setdefault(pops[p] if p < len(pops) else str(p), {})[name] = v
    for (p, name), v in spilled.items():
        counts.setdefault(pops[p] if p < len(pops) else str(p), {})[name] = v
    return counts


def m_step_counts(imputation, lines_or_path, config, block_lines=65536, planb=None, em=True, first_capacity=1 << 20):
    """The M-step on the device.  `lines_or_path`: input lines (a list) or the path of an input file; `config`: the
    configuration dict of `load_config`.  The input is cut into blocks of `block_lines` lines; each is tokenised, imputed
    as one device batch (em_mr on, phased output on, `em` as impute_file's) and its rows are added to the accumulator
    where they lie.  `output_MUUG` stays as the configuration has it: the reference's phased pass starts from what the MUUG
    pass left when that one ended in Plan C (impute.py:1637-1654), so the phased rows of some subjects differ with it off,
    and the counts are those of the rows the configured run prints.  -> ({pop: {haplotype: count}}, stats); the cuts do not show in any bit of a count.
    Subjects the device cannot answer follow `imputation.on_unsupported` as in `impute_lines_block`."""
    lines = read_lines(lines_or_path)
    g = imputation.netGraph
    pops = imputation.populations
    shared = Blocks(imputation, config, planb, True, em, output_haplotypes=True)
    n_slots = len(g.full_loci)
    acc = nat.EmAccumulator(shared.ctx, [g.adict.count(s) for s in range(n_slots)], len(pops), first_capacity)
    try:
        spilled, kernel_ms, n_blocks = _accumulate_blocks(imputation, shared, lines, block_lines, acc)
        counts = _counts_by_name(g.key_to_name, pops, acc.export(), spilled)
        stats = acc.stats()
        stats.update(entries=acc.entries(), spill=acc.spill_count(), blocks=n_blocks, kernel_ms=kernel_ms)
    finally:
        acc.close()
    return counts, stats


# ---- the sharded M-step: chunk tables folded in chunk order (the header comment of csrc/grim_em.h) -------------
def merge_tables(carry, keys, pops, counts, n_pops=None, n_alleles=None):
    """The CPU twin of grim_em_merge_records (and of grim_em_merge on the table the source would export) in plain Python
    floats: every entry of keys / pops / counts [n] (EmAccumulator.export's order) added to `carry`, a (key, pop) -> count
    dict that is updated in place and returned: carry[k, p] = carry[k, p] + x, a first contribution as +0.0 + x.  The
    refusals of the device call are raised as ValueError, before `carry` is touched; the checks on populations need
    `n_pops`, those on key fields `n_alleles` (the accumulator's), and are left out where that is None."""
    if keys is None or pops is None or counts is None:
        raise ValueError("a null array")
    K = [int(k) for k in np.asarray(keys).tolist()]
    Q = [int(q) for q in np.asarray(pops).tolist()]
    X = [float(x) for x in np.asarray(counts).tolist()]
    if not len(K) == len(Q) == len(X):
        raise ValueError("keys, pops and counts of different lengths")
    limits = None if n_alleles is None else [int(x) for x in n_alleles] + [0] * (nat.MAXL - len(n_alleles))
    for i in range(len(K)):
        k, q, x = K[i], Q[i], X[i]
        if q < 0 or (n_pops is not None and q >= int(n_pops)):
            raise ValueError("a population at or above the accumulator's number of populations")
        if k < 0 or k >> 60:
            raise ValueError("a key with a bit at or above bit 60")
        if limits is not None and any(((k >> (nat.ABITS * s)) & 0xFFF) > limits[s] for s in range(nat.MAXL)):
            raise ValueError("a key with a field above n_alleles of its slot")
        if i and not (K[i - 1], Q[i - 1]) < (k, q):
            raise ValueError("the entries are not strictly ascending in (key, pop)")
        if not (x >= 0.0 and x != float("inf")):
            raise ValueError("a count that is negative, NaN or infinite")
    for k, q, x in zip(K, Q, X):
        carry[(k, q)] = carry.get((k, q), 0.0) + x
    return carry


def table_arrays(table):
    """a (key, pop) -> count dict -> (keys u64, pops u32, counts f64) in EmAccumulator.export's order"""
    order = sorted(table)
    return (np.array([k for k, _ in order], dtype=np.uint64), np.array([p for _, p in order], dtype=np.uint32),
            np.array([table[at] for at in order], dtype=np.float64))


def fold_chunk_tables(tables, n_pops=None, n_alleles=None):
    """The chunk-ordered fold: `tables` is the list, in chunk order, of the chunks' exported tables (keys, pops, counts);
    count[k, p] = ((T_c0[k, p] + T_c1[k, p]) + T_c2[k, p]) + ... over the chunks that hold the entry -> (keys, pops, counts) in
    export order."""
    carry = {}
    for keys, pops, counts in tables:
        merge_tables(carry, keys, pops, counts, n_pops, n_alleles)
    return table_arrays(carry)


def fold_spilled(master, spilled):
    """a chunk's spilled counts (pop index, haplotype text) -> count added to `master` (in place), as the tables fold"""
    for at, v in spilled.items():
        master[at] = master[at] + v if at in master else v
    return master


CHUNK_STATS = ("subjects_used", "skipped_plan_c", "contributions", "rehashes", "spill", "blocks", "kernel_ms")


def chunk_table(imputation, shared, lines, line_offset, block_lines=65536, first_capacity=1 << 20):
    """The chunk-local part of the sharded M-step: today's M-step over one chunk's `lines` (the first is input line
    `line_offset`) into a fresh accumulator -> (the accumulator, open: the caller closes it; spilled; stats, the keys of
    CHUNK_STATS; the chunk's unsupported subjects)."""
    g = imputation.netGraph
    n_alleles = [g.adict.count(s) for s in range(len(g.full_loci))]
    acc = nat.EmAccumulator(shared.ctx, n_alleles, len(imputation.populations), first_capacity)
    try:
        spilled, kernel_ms, n_blocks = _accumulate_blocks(imputation, shared, lines, block_lines, acc, line_offset)
        stats = acc.stats()
        stats.update(spill=acc.spill_count(), blocks=n_blocks, kernel_ms=kernel_ms)
    except BaseException:
        acc.close()
        raise
    return acc, spilled, stats, list(imputation.unsupported)


def chunk_text_lines(raw):
    """a chunk's bytes -> its lines without line ends, as `read_lines` reads a file's"""
    import io

    return io.TextIOWrapper(io.BytesIO(raw), encoding="utf-8", newline=None).read().splitlines()


def read_chunk(fh, offs, c):
    """the bytes of chunk c of the file open (binary) as `fh`, `offs` being its chunk_offsets"""
    fh.seek(offs[c])
    return fh.read(offs[c + 1] - offs[c])


def input_chunks(lines_or_path, chunk_lines):
    """(first input line, lines) of every chunk of `chunk_lines` lines.  A file is cut where grim.shard.chunk_offsets cuts it
    for the sharded drivers, whose ranks read their chunks through the same `read_chunk`; a list by its index."""
    if isinstance(lines_or_path, (str, bytes, os.PathLike)):
        offs = nat.chunk_offsets(os.fspath(lines_or_path), chunk_lines)
        with open(lines_or_path, "rb") as fh:
            for c in range(len(offs) - 1):
                yield c * chunk_lines, chunk_text_lines(read_chunk(fh, offs, c))
    else:
        lines = read_lines(lines_or_path)
        for lo in range(0, len(lines), chunk_lines):
            yield lo, lines[lo:lo + chunk_lines]


def m_step_chunked(imputation, lines_or_path, config, chunk_lines, block_lines=65536, planb=None, em=True, first_capacity=1 << 20):
    """The sharded M-step's single-process definition, on one device: the input in chunks of `chunk_lines` lines, each
    chunk's M-step into a fresh accumulator (`chunk_table`), the chunks' tables merged on the device into a master
    accumulator in chunk order (EmAccumulator.merge), the spilled counts folded in chunk order.  -> (counts, stats, table):
    counts and stats shaped like `m_step_counts`' (stats are the sums over the chunks; `entries` the master's; `rehashes`
    the chunks' and the master's; plus `chunks` and `merge_ms`), table = the master's (keys, pops, counts) as
    Graph.refresh takes them.  The counts depend on chunk_lines and not on block_lines; with one chunk they are
    `m_step_counts`', bit for bit.  imputation.unsupported holds every chunk's subjects, by input line."""
    chunk_lines = max(1, int(chunk_lines))
    g = imputation.netGraph
    pops = imputation.populations
    shared = Blocks(imputation, config, planb, True, em, output_haplotypes=True)
    master = nat.EmAccumulator(shared.ctx, [g.adict.count(s) for s in range(len(g.full_loci))], len(pops), first_capacity)
    stats = dict.fromkeys(CHUNK_STATS, 0)
    stats.update(kernel_ms=0.0, merge_ms=0.0, chunks=0)
    spilled, unsupported = {}, []
    try:
        for lo, lines in input_chunks(lines_or_path, chunk_lines):
            acc, chunk_spilled, chunk_stats, bad = chunk_table(imputation, shared, lines, lo, block_lines, first_capacity)
            try:
                master.merge(acc)
            finally:
                acc.close()
            fold_spilled(spilled, chunk_spilled)
            for k in CHUNK_STATS:
                stats[k] += chunk_stats[k]
            stats["merge_ms"] += master.merge_ms()
            stats["chunks"] += 1
            unsupported += bad
        imputation.unsupported = unsupported
        table = master.export()
        stats["rehashes"] += master.stats()["rehashes"]
        stats["entries"] = master.entries()
    finally:
        master.close()
    return _counts_by_name(g.key_to_name, pops, table, spilled), stats, table


def write_freq_files(counts, freq_data_dir, pops):
    """One `POP.freqs.gz` per population in the format produce_hpf reads (generate_hpf.py:43-59): header
    `Haplo,Count,Freq`, rows sorted by haplotype, Freq = Count / T with T the left-to-right sum of the file's counts in row
    order, floats written with repr.  -> {pop: T}"""
    os.makedirs(freq_data_dir, exist_ok=True)
    totals = {}
    for pop in pops:
        rows = sorted(counts.get(pop, {}).items())
        total = 0.0
        for _, c in rows:
            total = total + c
        totals[pop] = total
        with gzip.open(os.path.join(freq_data_dir, pop + ".freqs.gz"), "wt", newline="") as fh:
            fh.write("Haplo,Count,Freq\n")
            for hap, c in rows:
                fh.write("%s,%r,%r\n" % (hap, c, c / total if total else 0.0))
    return totals


def em_iteration(conf_file, graph=None, block_lines=65536):
    """One EM iteration on the configuration's own files: the M-step over `imputation_in_file` on `graph` (built from the
    configuration's graph CSVs when None), new `POP.freqs.gz` into `freq_data_dir`, then produce_hpf and
    graph_freqs(for_em=True, em_pop=populations).  -> (the new Graph, counts).  Paths are taken as the configuration gives
    them, as everywhere in this package.  Whether and when the frequencies converge is the caller's business."""
    import json

    from graph_generation.generate_hpf import produce_hpf

    from .grim import graph_freqs, graph_instance
    from .imputation.impute import Imputation
    from .run_impute_def import load_config

    config, _ = load_config(conf_file)
    with open(conf_file) as fh:
        raw = json.load(fh)
    if graph is None:
        graph = graph_instance(config)
    imp = Imputation(graph, config)
    counts, stats = m_step_counts(imp, config["imputation_input_file"], config, block_lines=block_lines)
    write_freq_files(counts, raw["freq_data_dir"], config["pops"])
    produce_hpf(conf_file, quiet=True)
    graph_freqs(conf_file, for_em=True, em_pop=config["pops"])
    return graph_instance(config), counts


# ---- EM on a fixed support: the graph's frequencies from M-step counts (csrc/grim_refresh.h) ----------------
KEYMASK = (1 << 60) - 1  # GRIM_EM_KEYMASK: the alleles of a key


def refreshable_rows(arrays):
    """Whether the top-link rows of a graph's arrays can be trusted for a refresh, decided as grim_graph_upload decides it:
    the rows of the partial nodes, in node order, row of v = a_nbr[a_start[v] .. e(v)) with e(v) = a_start[v + 1] for
    v < V - 1 and e(V - 1) = len(a_nbr) (a_start[V] is the reference's sentinel quirk, not an end), tile a_nbr without gap
    or overlap; every row is non-empty; every entry is a full node whose key, cut to the slots of node_mask[v], is
    node_key[v].  -> (full node ids in node order, {partial node: (lo, hi)}) or raises ValueError with the reason."""
    V, full_mask = int(arrays["n_nodes"]), int(arrays["full_mask"])
    keys, masks = arrays["node_key"].tolist(), arrays["node_mask"].tolist()
    a_start, a_nbr = arrays["a_start"].tolist(), arrays["a_nbr"].tolist()
    lab_start, lab_nodes = arrays["lab_start"].tolist(), arrays["lab_nodes"].tolist()
    n_a = len(a_nbr)
    if full_mask >= 1 << nat.MAXL:
        raise ValueError("not refreshable: full_mask names a locus slot beyond MAXL")
    full = [v for v in range(V) if masks[v] == full_mask]
    f_lo, f_hi = lab_start[full_mask], lab_start[full_mask + 1]
    if f_lo > f_hi or f_hi > V or lab_nodes[f_lo:f_hi] != full:
        raise ValueError("not refreshable: lab_nodes does not list the full nodes in node order")
    slots = [sum(0xFFF << (nat.ABITS * q) for q in range(nat.MAXL) if (m >> q) & 1) for m in range(1 << nat.MAXL)]
    rows = {}
    pos = 0
    for v in range(V):
        m = masks[v]
        if m == full_mask:
            continue
        if m >= 1 << nat.MAXL:
            raise ValueError("not refreshable: partial node %d: label mask beyond MAXL" % v)
        lo, hi = a_start[v], a_start[v + 1] if v + 1 < V else n_a
        if lo != pos:
            raise ValueError("not refreshable: partial node %d: its top-link row does not begin where the row before it ends" % v)
        if hi <= lo:
            raise ValueError("not refreshable: partial node %d: empty top-link row" % v)
        if hi > n_a:
            raise ValueError("not refreshable: partial node %d: its top-link row ends beyond the links" % v)
        for e in range(lo, hi):
            r = a_nbr[e]
            if r >= V or masks[r] != full_mask:
                raise ValueError("not refreshable: partial node %d: a top link that does not end at a full node" % v)
            if keys[r] & slots[m] != keys[v]:
                raise ValueError("not refreshable: partial node %d: a top link to a full haplotype that does not project onto it" % v)
        rows[v] = (lo, hi)
        pos = hi
    if pos != n_a:
        raise ValueError("not refreshable: top links beyond the rows of the partial nodes")
    return full, rows


def refresh_freq_arrays(arrays, keys, pops, counts):
    """The CPU twin of grim_graph_refresh_records in plain Python floats, every sum in the contract's order (the header
    comment of csrc/grim_refresh.h): `arrays` as Graph.arrays holds them, keys / pops / counts [n] in EmAccumulator.export's
    order -> (freq f64 [n_nodes][n_pops], stats with total, delta, matched, zero_full, n_full).  The refusals of the device
    call are raised as ValueError; `arrays` is not changed."""
    V, P = int(arrays["n_nodes"]), int(arrays["n_pops"])
    full, rows = refreshable_rows(arrays)
    if keys is None or pops is None or counts is None:
        raise ValueError("a null array")
    K = np.asarray(keys).tolist()
    Q = np.asarray(pops).tolist()
    Cn = [float(x) for x in np.asarray(counts).tolist()]
    if not len(K) == len(Q) == len(Cn):
        raise ValueError("keys, pops and counts of different lengths")
    table = {}
    for i in range(len(K)):
        k, q, c = int(K[i]), int(Q[i]), Cn[i]
        if q < 0 or q >= P:
            raise ValueError("a population at or above the graph's number of populations")
        if k < 0 or k >> 60:
            raise ValueError("a key with a bit at or above bit 60")
        if i and not (int(K[i - 1]), int(Q[i - 1])) < (k, q):
            raise ValueError("the entries are not strictly ascending in (key, pop)")
        if not (c >= 0.0 and c != float("inf")):
            raise ValueError("a count that is negative, NaN or infinite")
        table[(k, q)] = c
    node_key = arrays["node_key"].tolist()
    old = arrays["freq"]
    F = len(full)
    matched = 0
    c = []
    for v in full:
        vec = []
        for p in range(P):
            x = table.get((node_key[v] & KEYMASK, p))
            matched += x is not None
            vec.append(0.0 if x is None else x)
        c.append(vec)
    B = nat.REFRESH_BLOCK
    total = []
    for p in range(P):
        t = 0.0
        for b in range(0, F, B):
            s = 0.0
            for i in range(b, min(b + B, F)):
                s = s + c[i][p]
            t = t + s
        total.append(t)
    for p in range(P):
        if not (total[p] > 0.0 and total[p] != float("inf")):
            raise ValueError("population %d has no count inside the support (its total is %r)" % (p, total[p]))
    new = [None] * V
    delta = 0.0
    zero_full = 0
    for i, v in enumerate(full):
        vec = [c[i][p] / total[p] for p in range(P)]
        new[v] = vec
        oldv = old[v].tolist()
        for p in range(P):
            d = abs(vec[p] - oldv[p])
            if d > delta:
                delta = d
        zero_full += all(x == 0.0 for x in vec)
    a_nbr = arrays["a_nbr"].tolist()
    for v, (lo, hi) in rows.items():
        vec = [0.0] * P
        for e in range(lo, hi):
            src = new[a_nbr[e]]
            for p in range(P):
                vec[p] = vec[p] + src[p]
        new[v] = vec
    freq = np.array(new, dtype=np.float64).reshape(V, P)
    return freq, {"total": total, "delta": delta, "matched": matched, "zero_full": zero_full, "n_full": F}


def em_fixed_support(imputation, lines_or_path, config, iterations, block_lines=65536, planb=None, em=True, tol=None):
    """EM on a fixed support: `iterations` times the M-step over the input (the block loop of `m_step_counts`, one
    accumulator per iteration) followed by Graph.refresh on the accumulator, all on the device: no frequency file, no graph
    regeneration, no upload.  -> a list of per-iteration dicts: the M-step statistics (subjects_used, skipped_plan_c,
    contributions, rehashes, entries, spill, blocks, kernel_ms) and of the refresh total, delta, matched, zero_full, n_full,
    outside = entries - matched (counters of haplotypes outside the support, which take no part) and refresh_ms.  Stops
    early when `tol` is given and an iteration's delta <= tol.  imputation.netGraph holds the last frequencies, on the
    device and in arrays["freq"]."""
    lines = read_lines(lines_or_path)
    g = imputation.netGraph
    n_slots = len(g.full_loci)
    out = []
    for _ in range(int(iterations)):
        shared = Blocks(imputation, config, planb, True, em, output_haplotypes=True)
        acc = nat.EmAccumulator(shared.ctx, [g.adict.count(s) for s in range(n_slots)], len(imputation.populations))
        try:
            _, kernel_ms, n_blocks = _accumulate_blocks(imputation, shared, lines, block_lines, acc)
            it = acc.stats()
            it.update(entries=acc.entries(), spill=acc.spill_count(), blocks=n_blocks, kernel_ms=kernel_ms)
            rs = g.refresh(shared.ctx, acc)
        finally:
            acc.close()
        it.update(total=rs["total"], delta=rs["delta"], matched=rs["matched"], zero_full=rs["zero_full"], n_full=rs["n_full"],
                  outside=it["entries"] - rs["matched"], refresh_ms=rs["kernel_ms"])
        out.append(it)
        if tol is not None and rs["delta"] <= tol:
            break
    return out
