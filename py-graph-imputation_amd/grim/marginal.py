"""
Marginal genotype tables: a subject's genotype (`.umug`) rows collapsed to a subset of the loci -- A~B~DRB1 for a 6/6
search, A~B~C~DRB1 for 8/8, one locus for a typing-resolution report.

The reference does this to a printed file with scripts/reduce_loci.py: drop one locus from every genotype, add the
probabilities of genotypes that became equal, sort again, write the top rows.  The operation is defined here for any set of
kept loci:

    for every subject, with genotype rows k = 0..n-1 in rank order and probabilities p_k:
      reduced genotype of row k = its kept loci (per locus the unordered allele pair)
      the first row of a reduced genotype leads its group; sum = (p_leader + p_j) + p_l ... over its rows in rank order
      groups by sum descending, ties in the leaders' order (a stable sort); the first max_rows of them are written

`marginal_umug` runs it on the device, on the rows a batch leaves in HBM (csrc/grim_marginal.h), and prints the reduced
records with the formatter every other text comes from.  `reduce_umug_text` is the same fold over `.umug` text in plain
Python floats, `reduce_records` the same over record arrays.  Device text and twin text agree byte for byte.  There is no CPU
fallback of `marginal_umug`.

Two deviations from reduce_loci.py, both on purpose: a subject is the run of rows from one rank 0 to the next (the script
merges every input line that shares an id, wherever it stands), and `max_rows` defaults to the configuration's
`number_of_results` (the script hard-codes 10).
"""

import numpy as np

from . import _native as nat
from .blocks import Blocks, note_unsupported, read_lines
from .groups import as_groups, regroup_umug_text


def keep_mask(locus_slot, keep_loci):
    """locus names -> bitmask of locus slots; `locus_slot`: name -> slot (Graph.locus_slot).  ValueError on an empty set or a
    name the configuration's loci_map does not have."""
    names = [keep_loci] if isinstance(keep_loci, str) else list(keep_loci)
    if not names:
        raise ValueError("keep_loci is empty")
    mask = 0
    for name in names:
        if name not in locus_slot:
            raise ValueError("unknown locus %r (the loci_map has %s)" % (name, ", ".join(sorted(locus_slot))))
        mask |= 1 << int(locus_slot[name])
    return mask


def _fold(rows, max_rows):
    """[(reduced genotype, p)] in rank order -> [(reduced genotype, sum)] in the new rank order, cut to max_rows"""
    sums = {}
    for g, p in rows:
        sums[g] = sums[g] + p if g in sums else p
    ranked = sorted(sums.items(), key=lambda kv: kv[1], reverse=True)  # stable: ties keep the leaders' order
    return ranked if max_rows is None else ranked[:max_rows]


def reduce_umug_text(text, keep_loci, max_rows=None, loci=None, groups=None):
    """`.umug` text in `id,genotype,p,rank` form -> the marginal text on `keep_loci` in the same form (rank from 0, floats
    written with repr).  A subject is the run of rows from one rank 0 to the next; a `^`-part of a genotype is kept when the
    text before its first `*` is one of the kept locus names; a subject whose kept loci are all untyped gets an empty
    genotype string.  `max_rows` None = every group; `loci`: the names that may be kept (an unknown one raises); `groups`: a
    group specification (grim.groups.GroupSpec or what it takes): the fold then runs on `regroup_umug_text(text, groups)`."""
    if groups is not None:
        text = regroup_umug_text(text, groups)
    keep = {keep_loci} if isinstance(keep_loci, str) else set(keep_loci)
    if not keep:
        raise ValueError("keep_loci is empty")
    if loci is not None:
        keep_mask({name: 0 for name in loci}, keep)
    if max_rows is not None and int(max_rows) < 1:
        raise ValueError("max_rows must be at least 1")
    out = []

    def flush(sid, rows):
        for k, (g, p) in enumerate(_fold(rows, max_rows)):
            out.append("%s,%s,%r,%d\n" % (sid, g, p, k))

    rows, sid = [], None
    for line in text.splitlines():
        if not line:
            continue
        f = line.split(",")
        if len(f) != 4:
            raise ValueError("not an id,genotype,probability,rank row: %r" % line)
        if int(f[3]) == 0 or f[0] != sid:
            flush(sid, rows)
            rows, sid = [], f[0]
        if int(f[3]) != len(rows):
            raise ValueError("ranks of subject %s are not 0..n-1" % f[0])
        g = "^".join(part for part in f[1].split("^") if part.split("*", 1)[0] in keep)
        rows.append((g, float(f[2])))
    flush(sid, rows)
    return "".join(out)


def reduce_records(res, rows, keep_mask, max_rows, groups=None):
    """The same fold on record arrays (nat.RESULT_DT[n], nat.ROW_DT[m]) as grim_marginal_reduce_records defines it
    (include/grim_hip.h) -> (result copies, output rows, stats), laid out as the device lays them out: subject i's region of
    the output rows starts at the sum of the row counts of the subjects before it; rows no region uses are zero.  `groups`: an
    AlleleGroups (grim.groups): the fold runs on the mapped rows, as the device's does with the map attached (the subjects
    the host folds on text are those of `groups.flags`)."""
    if groups is not None:
        rows = groups.map_records(rows)
    keep_mask, max_rows = int(keep_mask), int(max_rows)
    if keep_mask == 0 or keep_mask >> nat.MAXL:
        raise ValueError("keep_mask is empty or names a locus slot beyond %d" % nat.MAXL)
    if max_rows < 1:
        raise ValueError("max_rows must be at least 1")
    m = len(rows)
    counts = []
    for r in res:
        n, off = int(r["n_rows"][nat.T_UMUG]), int(r["row_off"][nat.T_UMUG])
        counts.append(0 if int(r["status"]) != nat.ST_OK or n == 0 or off > m or n > m - off else n)
    total = sum(counts)
    if total > m:
        raise ValueError("the subjects' genotype rows overlap (more rows than there are)")
    ores = np.zeros(len(res), dtype=nat.RESULT_DT)
    orows = np.zeros(total, dtype=nat.ROW_DT)
    stats = dict.fromkeys(nat.MARGINAL_STATS, 0)
    slots = [s for s in range(nat.MAXL) if (keep_mask >> s) & 1]
    keep_bits = sum(0xFFF << (nat.ABITS * s) for s in slots)
    first = 0
    for i, (r, n) in enumerate(zip(res, counts)):
        ores[i]["status"], ores[i]["plan"], ores[i]["reason"] = r["status"], r["plan"], r["reason"]
        if n == 0:
            continue
        off = int(r["row_off"][nat.T_UMUG])
        sub, undefined, lead = [], False, {}
        for k in range(n):
            a, b, p = int(rows[off + k]["a"]), int(rows[off + k]["b"]), float(rows[off + k]["prob"])
            fa = [(a >> (nat.ABITS * s)) & 0xFFF for s in range(nat.MAXL)]
            fb = [(b >> (nat.ABITS * s)) & 0xFFF for s in range(nat.MAXL)]
            undefined |= any((x == 0) != (y == 0) for x, y in zip(fa, fb))
            g = tuple((min(fa[s], fb[s]), max(fa[s], fb[s])) for s in slots)
            lead.setdefault(g, k)
            sub.append((g, p))
        ranked = _fold(sub, max_rows)
        for k, (g, p) in enumerate(ranked):
            src = rows[off + lead[g]]
            orows[first + k] = (int(src["a"]) & keep_bits, int(src["b"]) & keep_bits, p, 0, 0)
        ores[i]["n_genotypes"] = len(lead)
        ores[i]["n_rows"][nat.T_UMUG] = len(ranked)
        ores[i]["row_off"][nat.T_UMUG] = first
        stats["subjects"] += 1
        stats["rows_in"] += n
        stats["groups"] += len(lead)
        stats["rows_out"] += len(ranked)
        stats["undefined"] += 1 if undefined else 0
        first += n
    return ores, orows, stats


def _genotype(pairs):
    """[(allele name of haplotype a or None, of haplotype b or None)] per kept slot -> the genotype as the formatter prints it:
    each haplotype's names sorted, paired by position, each pair sorted, joined with '^'"""
    a, b = sorted(x for x, _ in pairs if x is not None), sorted(y for _, y in pairs if y is not None)
    return "^".join("+".join(sorted(xy)) for xy in zip(a, b))


def _grouped_text(imputation, block, mres, mrows, flags, groups, slots, max_rows, stats):
    """the marginal text of a block reduced with a group map attached, printed here: the device's rows carry group ids, whose
    names are `groups.names`; a subject flagged GROUPS_PRIVATE holds an allele the dictionary does not know in a grouped kept
    locus, and is folded here on group names from the block's own records"""
    g = imputation.netGraph
    parsed, n_alleles, n_groups = block.parsed, groups.n_alleles, groups.n_groups
    out = []
    for i in np.argsort(block.line_of[:len(mres)], kind="stable"):
        line = int(block.line_of[i])
        n = int(mres[i]["n_rows"][nat.T_UMUG])
        if int(mres[i]["status"]) != nat.ST_OK or n == 0:
            continue
        sid = parsed.subject_id(line)
        names = {}

        def own(s, f):  # dictionary id f of slot s, or the line's own allele, as text
            if (s, f) not in names:
                names[(s, f)] = parsed.allele(line, s, f - 1) if f > n_alleles[s] else g.key_alleles(f << (nat.ABITS * s))[s]
            return names[(s, f)]

        if flags[i]:
            res, rows = block.records()
            cnt, off = int(res[i]["n_rows"][nat.T_UMUG]), int(res[i]["row_off"][nat.T_UMUG])
            sub = []
            for k in range(cnt):
                a, b = int(rows[off + k]["a"]), int(rows[off + k]["b"])
                fields = [((a >> (nat.ABITS * s)) & 0xFFF, (b >> (nat.ABITS * s)) & 0xFFF, s) for s in slots]
                sub.append((_genotype([tuple(groups.spec.name(g.slot_locus[s], own(s, f)) if f else None for f in (fa, fb))
                                       for fa, fb, s in fields]), float(rows[off + k]["prob"])))
            every = _fold(sub, None)
            ranked = every[:max_rows]
            stats["host_subjects"] += 1
            stats["groups"] += len(every) - int(mres[i]["n_genotypes"])
            stats["rows_out"] += len(ranked) - n
        else:
            off = int(mres[i]["row_off"][nat.T_UMUG])
            ranked = []
            for k in range(n):
                a, b = int(mrows[off + k]["a"]), int(mrows[off + k]["b"])
                pairs = []
                for s in slots:
                    pair = []
                    for f in ((a >> (nat.ABITS * s)) & 0xFFF, (b >> (nat.ABITS * s)) & 0xFFF):
                        if f == 0:
                            pair.append(None)
                        elif f <= n_groups[s]:
                            pair.append(groups.names[s][f])
                        else:  # private, in a slot that is not grouped or not watched: its own text through the slot's rule
                            pair.append(groups.spec.name(g.slot_locus[s], own(s, f - n_groups[s] + n_alleles[s])))
                    pairs.append(tuple(pair))
                ranked.append((_genotype(pairs), float(mrows[off + k]["prob"])))
        for k, (geno, p) in enumerate(ranked):
            out.append("%s,%s,%r,%d\n" % (sid, geno, p, k))
    return "".join(out)


def marginal_umug(imputation, lines_or_path, config, keep_loci, max_rows=None, block_lines=65536, planb=None, em=False, groups=None):
    """The marginal `.umug` text of an input on the device.  `lines_or_path`: input lines (a list) or the path of an input
    file; `config`: the configuration dict of `load_config`; `keep_loci`: locus names of its loci_map; `max_rows`: rows kept
    per subject (None = the configuration's number_of_results).  The input is cut into blocks of `block_lines` lines; each
    is tokenised, imputed as one device batch (genotype output on, the rest as configured), reduced where its rows lie, and
    the reduced records are printed by the formatter of every other text.  -> (text, stats); the cuts do not show in any
    byte.  Subjects the device cannot answer follow `imputation.on_unsupported` as in `impute_lines_block`.
    `groups`: an AlleleGroups of the imputation's graph or a group specification (grim.groups): the rows are mapped to group
    ids on the device before they are reduced, subjects that hold an allele the dictionary does not know in a grouped kept
    locus are folded here on group names (`host_subjects` of the stats), and the text is printed here with the groups'
    names; it equals `reduce_umug_text(regroup_umug_text(umug text, spec), keep_loci)` byte for byte."""
    g = imputation.netGraph
    mask = keep_mask(g.locus_slot, keep_loci)
    groups = as_groups(g, groups)
    if max_rows is None:
        max_rows = int(config["number_of_results"])
    if int(max_rows) < 1:
        raise ValueError("max_rows must be at least 1")
    lines = read_lines(lines_or_path)
    shared = Blocks(imputation, config, planb, False, em, output_MUUG=True)
    fparams = nat.Params.from_buffer_copy(shared.params)  # what the formatter is told: genotype rows only
    fparams.out_muug, fparams.out_haps = 1, 0
    red = nat.MarginalReducer(shared.ctx, mask, max_rows)
    imputation.unsupported = []
    stats = dict.fromkeys(nat.MARGINAL_STATS, 0)
    stats.update(blocks=0, kernel_ms=0.0, host_subjects=0)
    out = []
    cut = shared.cut(lines, max(1, int(block_lines)))
    try:
        if groups is not None:
            dev_groups = nat.Groups.of(shared.ctx, groups)
            try:
                red.set_groups(dev_groups)  # the reducer keeps its own copy of the tables
            finally:
                dev_groups.close()
        for block in cut:
            bad = block.bad
            mres, mrows = np.zeros(0, dtype=nat.RESULT_DT), np.zeros(0, dtype=nat.ROW_DT)
            if block.batch is not None:
                red.reduce(block.batch)
                for k, v in red.stats().items():
                    stats[k] += v
                stats["kernel_ms"] += red.kernel_ms()
                stats["blocks"] += 1
                mres, mrows = red.results()
                bad = bad + block.unsupported(mres)  # the reduced records carry the batch's status and reason
            note_unsupported(imputation, bad)
            if stats["undefined"]:
                raise ValueError("%d subject(s) hold a genotype row whose haplotypes are typed at different loci: their "
                                 "marginal is not defined" % stats["undefined"])
            if groups is None:
                out.append(block.parsed.format(g.adict, fparams, imputation.populations, mres, mrows, block.lo, None)["umug"])
            elif block.batch is not None:
                slots = [s for s in range(nat.MAXL) if (mask >> s) & 1]
                flags = red.flags()
                late = mask & groups.rule_mask & ~groups.watch_mask  # a rule that merges no dictionary allele may still
                if late:                                             # send an unseen allele into a known group
                    flags = flags | groups.flags(*block.records(), mask, watch=late)
                out.append(_grouped_text(imputation, block, mres, mrows, flags, groups, slots, int(max_rows), stats))
    finally:
        cut.close()
        red.close()
    return "".join(out), stats


def reduce_file(conf_file, keep_loci, out_path, graph=None, max_rows=None, block_lines=65536, groups=None):
    """The configuration's input file -> one marginal `.umug`-format file at `out_path`, on `graph` (built from the
    configuration's graph CSVs when None).  Paths are taken as the configuration gives them.  `groups`: as `marginal_umug`.
    -> stats"""
    from .grim import graph_instance
    from .imputation.impute import Imputation
    from .run_impute_def import load_config

    config, _ = load_config(conf_file)
    if graph is None:
        graph = graph_instance(config)
    imp = Imputation(graph, config)
    text, stats = marginal_umug(imp, config["imputation_input_file"], config, keep_loci, max_rows=max_rows, block_lines=block_lines,
                                groups=groups)
    with open(out_path, "w") as fh:
        fh.write(text)
    return stats
