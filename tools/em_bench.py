"""
Measure the device M-step (grim/em.py, csrc/grim_em.h) on bench.py's config-4-shaped workload: the pop4 graph, 100 000
mixed subjects of seed 3, MR priors, em_mr on.  One JSON line with medians over --steps steps after --warmup:

  (a) impute_kernel_ms   the batch's kernels, grim_batch_kernel_ms(GRIM_MS_TOTAL) in timing mode
  (b) em_kernel_ms       grim_em_kernel_ms of the accumulate call on that batch (a fresh accumulator every step)
  (c) text_route_s       what a caller had before: impute_lines_block text -> fold_pmug_text, wall time
  (d) merge_ms           the sharded M-step's fold of that batch taken as ONE chunk: grim_em_merge_ms of merging the step's
                         accumulator into an empty master where both tables lie (EmAccumulator.merge)
  (e) merge_records_ms   the same chunk through the records door (EmAccumulator.merge_records of the exported table): device
                         time, next to merge_records_wall_ms (check, upload and launch) and export_wall_ms (the sender's side)

    python tools/em_bench.py [--subjects N] [--steps K] [--warmup W]
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
    ap.add_argument("--text-steps", type=int, default=3, help="steps of the text route (tens of seconds each at 100k subjects)")
    args = ap.parse_args()

    import __graft_entry__ as ge
    ge.build()
    from grim import _native as nat
    from grim.em import fold_pmug_text
    from grim.imputation.impute import Imputation
    from grim.imputation.networkx_graph import Graph
    from grim.run_impute_def import load_config

    pops = harness.POPS["pop4"]
    work = harness.ensure_graph("pop4")
    conf = harness.base_conf(pops)
    conf["UNK_priors"] = "MR"
    lines = synth.SubjectGen(synth.read_freqs(synth.CAU_FREQS), 3, pops=pops).mixed(args.subjects)
    conf, cpath = harness._write_inputs(work, conf, lines[:1], "em_bench")
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
    P = len(pops)
    ctx = nat.default_context(imp.device)
    params = imp._params(dict(cfg, output_haplotypes=True), cfg["planb"], True, True)
    parsed = nat.Parsed(g.adict, ("\n".join(lines) + "\n").encode(), cfg["planb"])
    ps, keep = nat.prior_spec(cfg["priority"], imp.unk_priors, imp.count_by_prob)
    priors = nat.prior_matrices(ps, pops, parsed.races())
    batch = nat.DeviceBatch(ctx, g.device(ctx), params, parsed.subjects(), parsed.tokens(), priors)
    batch.set_timing(True)
    n_alleles = [g.adict.count(s) for s in range(len(g.full_loci))]
    a_ms, b_ms, stats, entries = [], [], None, 0
    d_ms, e_ms, e_wall, x_wall = [], [], [], []
    for step in range(args.warmup + args.steps):
        batch.run()
        acc = nat.EmAccumulator(ctx, n_alleles, P)
        try:
            acc.accumulate(batch)
            if step >= args.warmup:
                a_ms.append(batch.kernel_ms(nat.MS_TOTAL))
                b_ms.append(acc.kernel_ms())
            stats, entries = acc.stats(), acc.entries()
            master, by_records = nat.EmAccumulator(ctx, n_alleles, P), nat.EmAccumulator(ctx, n_alleles, P)
            try:
                master.merge(acc)
                t0 = timeit.default_timer()
                table = acc.export()
                t1 = timeit.default_timer()
                by_records.merge_records(*table)
                t2 = timeit.default_timer()
                if master.entries() != entries or by_records.entries() != entries:
                    raise RuntimeError("a merge into an empty accumulator holds another number of entries than its source")
                if step >= args.warmup:
                    d_ms.append(master.merge_ms())
                    e_ms.append(by_records.merge_ms())
                    x_wall.append(1e3 * (t1 - t0))
                    e_wall.append(1e3 * (t2 - t1))
            finally:
                master.close()
                by_records.close()
        finally:
            acc.close()
    batch.close()
    parsed.close()
    c_s = []
    for step in range(args.text_steps):
        t0 = timeit.default_timer()
        texts = imp.impute_lines_block(lines, dict(cfg, output_haplotypes=True), em_mr=True, em=True)
        counts, _ = fold_pmug_text(texts["pmug"])
        c_s.append(timeit.default_timer() - t0)
    print(json.dumps({
        "workload": "pop4 graph, %d mixed subjects (seed 3), MR priors, em_mr" % args.subjects, "steps": args.steps, "warmup": args.warmup,
        "impute_kernel_ms": statistics.median(a_ms), "em_kernel_ms": statistics.median(b_ms),
        "text_route_s": statistics.median(c_s) if c_s else None, "text_steps": args.text_steps,
        "merge_ms": statistics.median(d_ms), "merge_records_ms": statistics.median(e_ms),
        "merge_records_wall_ms": statistics.median(e_wall), "export_wall_ms": statistics.median(x_wall),
        "em_stats": stats, "entries": entries, "text_entries": sum(len(d) for d in counts.values()) if c_s else None,
    }))


if __name__ == "__main__":
    main()
