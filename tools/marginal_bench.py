"""
Measure the device marginal genotype tables (grim/marginal.py, csrc/grim_marginal.h) on bench.py's config-4-shaped
workload: the pop4 graph, 100 000 mixed subjects of seed 3, MR priors.  One JSON line with three medians over --steps steps
after --warmup:

  (a) impute_kernel_ms    the batch's kernels, grim_batch_kernel_ms(GRIM_MS_TOTAL) in timing mode
  (b) marginal_kernel_ms  grim_marginal_kernel_ms of the reduce call on that batch
  (c) text_route_s        what a caller had before: impute_lines_block text -> reduce_umug_text on its .umug, wall time

    python tools/marginal_bench.py [--subjects N] [--steps K] [--warmup W] [--keep A,B,DRB1]
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
    ap.add_argument("--keep", default="A,B,DRB1", help="locus names to keep, comma separated")
    ap.add_argument("--text-steps", type=int, default=3, help="steps of the text route (seconds each at 100k subjects)")
    args = ap.parse_args()

    import __graft_entry__ as ge
    ge.build()
    from grim import _native as nat
    from grim.imputation.impute import Imputation
    from grim.imputation.networkx_graph import Graph
    from grim.marginal import keep_mask, reduce_umug_text
    from grim.run_impute_def import load_config

    pops = harness.POPS["pop4"]
    work = harness.ensure_graph("pop4")
    conf = harness.base_conf(pops)
    conf["UNK_priors"] = "MR"
    lines = synth.SubjectGen(synth.read_freqs(synth.CAU_FREQS), 3, pops=pops).mixed(args.subjects)
    conf, cpath = harness._write_inputs(work, conf, lines[:1], "marginal_bench")
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
    mask = keep_mask(g.locus_slot, keep)
    max_rows = int(cfg["number_of_results"])
    ctx = nat.default_context(imp.device)
    params = imp._params(dict(cfg, output_MUUG=True), cfg["planb"], False, False)
    parsed = nat.Parsed(g.adict, ("\n".join(lines) + "\n").encode(), cfg["planb"])
    ps, keep_alive = nat.prior_spec(cfg["priority"], imp.unk_priors, imp.count_by_prob)
    priors = nat.prior_matrices(ps, pops, parsed.races())
    batch = nat.DeviceBatch(ctx, g.device(ctx), params, parsed.subjects(), parsed.tokens(), priors)
    batch.set_timing(True)
    red = nat.MarginalReducer(ctx, mask, max_rows)
    a_ms, b_ms, stats = [], [], None
    try:
        for step in range(args.warmup + args.steps):
            batch.run()
            red.reduce(batch)
            if step >= args.warmup:
                a_ms.append(batch.kernel_ms(nat.MS_TOTAL))
                b_ms.append(red.kernel_ms())
            stats = red.stats()
    finally:
        red.close()
        batch.close()
        parsed.close()
    c_s, text_rows = [], None
    for step in range(args.text_steps):
        t0 = timeit.default_timer()
        texts = imp.impute_lines_block(lines, dict(cfg, output_MUUG=True))
        text_rows = reduce_umug_text(texts["umug"], keep, max_rows).count("\n")
        c_s.append(timeit.default_timer() - t0)
    print(json.dumps({
        "workload": "pop4 graph, %d mixed subjects (seed 3), MR priors, keep %s" % (args.subjects, "~".join(keep)),
        "steps": args.steps, "warmup": args.warmup,
        "impute_kernel_ms": statistics.median(a_ms), "marginal_kernel_ms": statistics.median(b_ms),
        "text_route_s": statistics.median(c_s) if c_s else None, "text_steps": args.text_steps,
        "marginal_stats": stats, "text_rows": text_rows,
    }))


if __name__ == "__main__":
    main()
