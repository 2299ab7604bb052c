"""
Measure the device match probabilities (grim/match.py, csrc/grim_match.h) on bench.py's config-4-shaped workload as donors:
the pop4 graph, 100 000 mixed subjects of seed 3, MR priors; the first 8 and the first 64 subjects are the patients.  One
JSON line with medians over --steps steps after --warmup:

  (a) impute_kernel_ms   the donors' batch's kernels, grim_batch_kernel_ms(GRIM_MS_TOTAL) in timing mode
  (b) match_kernel_ms    grim_match_kernel_ms of the run on that batch, per patient count; with --direction / --graded one
                         leg per (direction, graded) in the same run, `legs`, the first leg being the one to compare with
                         (the default leg, either and ungraded, is the kernel every caller had before), and
                         `download_bytes`, the size of a leg's result records
  (c) text_route_s       what a caller had before: match_umug_text on the printed .umug of the patients and of the first
                         --text-donors donors, wall time, scaled to all donors (the fold is linear in the donors)

    python tools/match_bench.py [--subjects N] [--steps K] [--warmup W] [--keep A,B,C,DQB1,DRB1] [--patients 8,64]
                                [--direction either,gvh] [--graded off|on|both]
"""
import argparse
import json
import os
import statistics
import sys
import timeit

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
    ap.add_argument("--keep", default="A,B,C,DQB1,DRB1", help="locus names to keep, comma separated")
    ap.add_argument("--patients", default="8,64", help="patient counts, comma separated: the first N subjects")
    ap.add_argument("--text-donors", type=int, default=1000, help="donors of the text route (scaled to --subjects)")
    ap.add_argument("--direction", default="either", help="mismatch directions (either, gvh, hvg), comma separated")
    ap.add_argument("--graded", default="off", choices=["off", "on", "both"], help="ungraded records, graded ones, or a leg each")
    args = ap.parse_args()

    import __graft_entry__ as ge
    ge.build()
    from grim import _native as nat
    from grim.imputation.impute import Imputation
    from grim.imputation.networkx_graph import Graph
    from grim.marginal import keep_mask
    from grim.match import direction_code, match_umug_text
    from grim.run_impute_def import load_config

    pops = harness.POPS["pop4"]
    work = harness.ensure_graph("pop4")
    conf = harness.base_conf(pops)
    conf["UNK_priors"] = "MR"
    lines = synth.SubjectGen(synth.read_freqs(synth.CAU_FREQS), 3, pops=pops).mixed(args.subjects)
    conf, cpath = harness._write_inputs(work, conf, lines[:1], "match_bench")
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
    ctx = nat.default_context(imp.device)
    params = imp._params(dict(cfg, output_MUUG=True), cfg["planb"], False, False)
    parsed = nat.Parsed(g.adict, ("\n".join(lines) + "\n").encode(), cfg["planb"])
    ps, keep_alive = nat.prior_spec(cfg["priority"], imp.unk_priors, imp.count_by_prob)
    priors = nat.prior_matrices(ps, pops, parsed.races())
    batch = nat.DeviceBatch(ctx, g.device(ctx), params, parsed.subjects(), parsed.tokens(), priors)
    batch.set_timing(True)
    legs = [(d, gr) for gr in {"off": [False], "on": [True], "both": [False, True]}[args.graded]
            for d in [x for x in args.direction.split(",") if x]]
    n_alleles = [g.adict.count(s) for s in range(len(g.full_loci))]
    matchers = []
    a_ms, b_ms, stats = [], {leg: {n: [] for n in counts} for leg in legs}, {}
    try:
        for d, gr in legs:
            matchers.append(nat.Matcher(ctx, mask, n_alleles, direction_code(d), gr))
        batch.run()
        res, rows = batch.results()
        for step in range(args.warmup + args.steps):
            batch.run()
            if step >= args.warmup:
                a_ms.append(batch.kernel_ms(nat.MS_TOTAL))
            for n in counts:  # the first n device subjects, their rows where the batch has them
                for leg, matcher in zip(legs, matchers):  # the legs in turn within a step: drift hits them alike
                    matcher.set_patients(res[:n], rows)
                    matcher.run(batch)
                    if step >= args.warmup:
                        b_ms[leg][n].append(matcher.kernel_ms())
                    if leg == legs[0]:
                        stats[n] = matcher.stats()
    finally:
        for matcher in matchers:
            matcher.close()
        batch.close()
        parsed.close()
    c_s = None
    if args.text_donors > 0:
        n_text = min(args.text_donors, len(lines))
        umug = imp.impute_lines_block(lines[:n_text], dict(cfg, output_MUUG=True))["umug"]
        subjects = []
        for line in umug.splitlines(keepends=True):
            if line.rstrip("\n").endswith(",0"):
                subjects.append("")
            subjects[-1] += line
        c_s = {}
        for n in counts:
            t0 = timeit.default_timer()
            match_umug_text("".join(subjects[:n]), umug, keep)
            c_s[n] = (timeit.default_timer() - t0) * args.subjects / n_text
    print(json.dumps({
        "workload": "pop4 graph, %d mixed subjects (seed 3) as donors, MR priors, keep %s" % (args.subjects, "~".join(keep)),
        "steps": args.steps, "warmup": args.warmup,
        "impute_kernel_ms": statistics.median(a_ms),
        "match_kernel_ms": {str(n): statistics.median(v) for n, v in b_ms[legs[0]].items()},
        "legs": {"%s%s" % (d, "~graded" if gr else ""): {
            "match_kernel_ms": {str(n): statistics.median(v) for n, v in b_ms[(d, gr)].items()},
            "min_ms": {str(n): min(v) for n, v in b_ms[(d, gr)].items()},
            "download_bytes": {str(n): n * len(res) * (nat.MATCH_GRADE_DT if gr else nat.MATCH_DT).itemsize for n in counts}}
            for d, gr in legs},
        "text_route_s_scaled": {str(n): v for n, v in c_s.items()} if c_s else None, "text_donors": args.text_donors,
        "match_stats": {str(n): s for n, s in stats.items()},
    }))


if __name__ == "__main__":
    main()
