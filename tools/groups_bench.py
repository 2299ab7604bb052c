"""
Measure allele groups (grim/groups.py, csrc/grim_groups.h) on tools/match_bench.py's workload: the pop4 graph, 100 000 mixed
subjects of seed 3 as donors, MR priors, first-field groups at every locus.  One JSON line with medians over --steps steps
after --warmup:

  (a) map_pass          gp_map_kernel alone through grim_groups_kernel_ms, on the batch's rows and on those rows repeated up
                        to --map-rows: ms and GB/s against the 64 bytes a row moves, with the tables staged in LDS by every
                        workgroup (the default) and read where they lie (GRIM_GROUPS_LDS=0), for the graph's tables and for
                        the largest tables there can be (5 x 4096 entries)
  (b) match_kernel_ms / marginal_kernel_ms
                        grim_match_kernel_ms per patient count and grim_marginal_kernel_ms on that batch, without a map and
                        with the first-field map attached (the map pass lies between the consumer's two event records)
  (c) text_route_s      what a caller had before: regroup_umug_text on the printed .umug, then match_umug_text /
                        reduce_umug_text, wall time on the first --text-donors donors, scaled to all donors

    python tools/groups_bench.py [--subjects N] [--steps K] [--warmup W] [--keep A,B,DRB1] [--patients 8,64]
"""
import argparse
import json
import os
import statistics
import sys
import timeit

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import harness  # noqa: E402
import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subjects", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--keep", default="A,B,DRB1", help="locus names to keep, comma separated")
    ap.add_argument("--patients", default="8,64", help="patient counts, comma separated: the first N subjects")
    ap.add_argument("--rule", default="first_field")
    ap.add_argument("--map-rows", type=int, default=8000000, help="rows of the large map pass (the batch's rows repeated)")
    ap.add_argument("--text-donors", type=int, default=1000, help="donors of the text route (scaled to --subjects)")
    args = ap.parse_args()

    import __graft_entry__ as ge
    ge.build()
    from grim import _native as nat
    from grim.groups import AlleleGroups, regroup_umug_text
    from grim.imputation.impute import Imputation
    from grim.imputation.networkx_graph import Graph
    from grim.marginal import keep_mask, reduce_umug_text
    from grim.match import match_umug_text
    from grim.run_impute_def import load_config

    pops = harness.POPS["pop4"]
    work = harness.ensure_graph("pop4")
    conf = harness.base_conf(pops)
    conf["UNK_priors"] = "MR"
    lines = synth.SubjectGen(synth.read_freqs(synth.CAU_FREQS), 3, pops=pops).mixed(args.subjects)
    conf, cpath = harness._write_inputs(work, conf, lines[:1], "groups_bench")
    cwd = os.getcwd()
    os.chdir(work)
    try:
        cfg, _ = load_config(cpath)
        g = Graph(cfg).build_graph(cfg["node_file"], cfg["top_links_file"], cfg["edges_file"])
        imp = Imputation(g, cfg)
    finally:
        os.chdir(cwd)
    imp.on_unsupported = "skip"
    imp.quiet = True
    keep = [k for k in args.keep.split(",") if k]
    counts = [int(x) for x in args.patients.split(",") if x]
    mask = keep_mask(g.locus_slot, keep)
    max_rows = int(cfg["number_of_results"])
    groups = AlleleGroups(g, args.rule)
    ctx = nat.default_context(imp.device)
    params = imp._params(dict(cfg, output_MUUG=True), cfg["planb"], False, False)
    parsed = nat.Parsed(g.adict, ("\n".join(lines) + "\n").encode(), cfg["planb"])
    ps, keep_alive = nat.prior_spec(cfg["priority"], imp.unk_priors, imp.count_by_prob)
    priors = nat.prior_matrices(ps, pops, parsed.races())
    batch = nat.DeviceBatch(ctx, g.device(ctx), params, parsed.subjects(), parsed.tokens(), priors)
    n_alleles = [g.adict.count(s) for s in range(len(g.full_loci))]
    total = args.warmup + args.steps
    map_pass, match_ms, marginal_ms = {}, {}, {}
    lds_was = os.environ.get("GRIM_GROUPS_LDS")
    try:
        batch.run()
        res, rows = batch.results()
        big = np.tile(rows, max(1, -(-args.map_rows // max(1, len(rows)))))
        # the largest tables there can be (5 x 4096 entries, 40 KB): what staging costs at its worst
        full = AlleleGroups.from_names(g.slot_locus, [["%s*%02d:%04d" % (locus, f % 16, f) for f in range(1, 4096)] for locus in g.slot_locus],
                                       "first_field")
        # (a) the map pass alone
        for name, staged in (("tables_in_l2", "0"), ("tables_in_lds", "1")):
            os.environ["GRIM_GROUPS_LDS"] = staged  # read when the map is created
            for tables, which in (("", groups), ("/full_tables", full)):
                dev = nat.Groups.of(ctx, which)
                try:
                    for what, arr in (("batch_rows", rows), ("repeated_rows", big)):
                        ms = []
                        for step in range(total):
                            dev.map_records(arr)
                            if step >= args.warmup:
                                ms.append(dev.kernel_ms())
                        med = statistics.median(ms)
                        map_pass["%s/%s%s" % (name, what, tables)] = {"rows": len(arr), "ms": med, "min_ms": min(ms), "max_ms": max(ms),
                                                                     "GB_per_s": 64.0 * len(arr) / (med * 1e6)}
                finally:
                    dev.close()
        if lds_was is None:
            del os.environ["GRIM_GROUPS_LDS"]
        else:
            os.environ["GRIM_GROUPS_LDS"] = lds_was
        # (b) the consumers without a map and with it
        dev = nat.Groups.of(ctx, groups)
        matcher = nat.Matcher(ctx, mask, n_alleles)
        red = nat.MarginalReducer(ctx, mask, max_rows)
        try:
            for name, attach in (("no_map", None), ("with_map", dev)):
                matcher.set_groups(attach)
                red.set_groups(attach)
                mg = []
                mt = {n: [] for n in counts}
                for step in range(total):
                    red.reduce(batch)
                    if step >= args.warmup:
                        mg.append(red.kernel_ms())
                    for n in counts:
                        matcher.set_patients(res[:n], rows)
                        matcher.run(batch)
                        if step >= args.warmup:
                            mt[n].append(matcher.kernel_ms())
                marginal_ms[name] = {"ms": statistics.median(mg), "min_ms": min(mg), "max_ms": max(mg), "stats": red.stats()}
                match_ms[name] = {str(n): {"ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for n, v in mt.items()}
        finally:
            red.close()
            matcher.close()
            dev.close()
    finally:
        batch.close()
        parsed.close()
    # (c) the text route it replaces
    text = None
    if args.text_donors > 0:
        n_text = min(args.text_donors, len(lines))
        scale = args.subjects / n_text
        umug = imp.impute_lines_block(lines[:n_text], dict(cfg, output_MUUG=True))["umug"]
        t0 = timeit.default_timer()
        regrouped = regroup_umug_text(umug, args.rule)
        t_regroup = timeit.default_timer() - t0
        t0 = timeit.default_timer()
        reduce_umug_text(regrouped, keep, max_rows)
        t_reduce = timeit.default_timer() - t0
        subjects = []
        for line in regrouped.splitlines(keepends=True):
            if line.rstrip("\n").endswith(",0"):
                subjects.append("")
            subjects[-1] += line
        text = {"text_donors": n_text, "regroup_s_scaled": t_regroup * scale, "marginal_s_scaled": (t_regroup + t_reduce) * scale, "match_s_scaled": {}}
        for n in counts:
            t0 = timeit.default_timer()
            match_umug_text("".join(subjects[:n]), regrouped, keep)
            text["match_s_scaled"][str(n)] = (t_regroup + timeit.default_timer() - t0) * scale
    print(json.dumps({
        "workload": "pop4 graph, %d mixed subjects (seed 3) as donors, MR priors, keep %s, rule %s" % (args.subjects, "~".join(keep), args.rule),
        "steps": args.steps, "warmup": args.warmup, "batch_rows": int(len(rows)),
        "n_alleles": groups.n_alleles, "n_groups": groups.n_groups, "watch_mask": groups.watch_mask,
        "map_pass": map_pass, "marginal_kernel_ms": marginal_ms, "match_kernel_ms": match_ms, "text_route": text,
    }))


if __name__ == "__main__":
    main()
