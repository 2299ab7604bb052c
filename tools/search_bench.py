"""
Measure the device donor search (grim/search.py, csrc/grim_search.h) on tools/match_bench.py's workload: the pop4 graph,
100 000 mixed subjects of seed 3 as donors, MR priors; the first 8 and the first 64 subjects are the patients, all five loci
kept; top_n 10 and 256.  One JSON line with medians over --steps steps after --warmup, per patient count (and top_n):

  (a) match_kernel_ms     the match part of a search run: grim_search_kernel_ms - grim_search_select_ms (preparing the
                          donors, clearing the records, the pair kernel)
  (b) select_ms           grim_search_select_ms: the selection kernels alone
  (c) search_bytes        what comes down: patients x top_n x 136, against match_bytes = patients x donors x 128 before
  (d) search_wall_s       wall time of one Searcher run plus results(), against match_wall_s: one Matcher run plus
                          results() on the same batch
  (e) merge               the merge door at the last patient count and the largest top_n: the donors dealt into --merge-lists
                          parts, each part's hit list made by a run, then merge_select_ms (grim_search_select_ms of one merge
                          of all lists into an empty search) and merge_wall_s (Searcher.merge, upload included), against
                          python_merge_s: the same merge by grim.search.merge_hit_lists, a Python loop over the hits

    python tools/search_bench.py [--subjects N] [--steps K] [--warmup W] [--keep A,B,C,DQB1,DRB1] [--patients 8,64] [--top-n 10,256]
                                 [--merge-lists 8]
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
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--keep", default="A,B,C,DQB1,DRB1", help="locus names to keep, comma separated")
    ap.add_argument("--patients", default="8,64", help="patient counts, comma separated: the first N subjects")
    ap.add_argument("--top-n", default="10,256", help="hits per patient, comma separated")
    ap.add_argument("--merge-lists", type=int, default=8, help="lists of the merge leg (0: no merge leg)")
    args = ap.parse_args()

    import numpy as np

    import __graft_entry__ as ge
    ge.build()
    from grim import _native as nat
    from grim.imputation.impute import Imputation
    from grim.imputation.networkx_graph import Graph
    from grim.marginal import keep_mask
    from grim.run_impute_def import load_config

    pops = harness.POPS["pop4"]
    work = harness.ensure_graph("pop4")
    conf = harness.base_conf(pops)
    conf["UNK_priors"] = "MR"
    lines = synth.SubjectGen(synth.read_freqs(synth.CAU_FREQS), 3, pops=pops).mixed(args.subjects)
    conf, cpath = harness._write_inputs(work, conf, lines[:1], "search_bench")
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
    tops = [int(x) for x in args.top_n.split(",") if x]
    mask = keep_mask(g.locus_slot, keep)
    ctx = nat.default_context(imp.device)
    params = imp._params(dict(cfg, output_MUUG=True), cfg["planb"], False, False)
    parsed = nat.Parsed(g.adict, ("\n".join(lines) + "\n").encode(), cfg["planb"])
    ps, keep_alive = nat.prior_spec(cfg["priority"], imp.unk_priors, imp.count_by_prob)
    priors = nat.prior_matrices(ps, pops, parsed.races())
    n_alleles = [g.adict.count(s) for s in range(len(g.full_loci))]
    batch = nat.DeviceBatch(ctx, g.device(ctx), params, parsed.subjects(), parsed.tokens(), priors)
    matcher = nat.Matcher(ctx, mask, n_alleles)
    searchers = {top: nat.Searcher(ctx, mask, n_alleles, top, 0.0) for top in tops}  # min_p0 0.0: every computed pair is a candidate
    out = {}
    merge = None
    try:
        batch.run()
        res, rows = batch.results()
        ids = np.arange(batch.n, dtype=np.uint32)
        for n in counts:
            rec = out[str(n)] = {"match_bytes": n * batch.n * nat.MATCH_DT.itemsize, "match_pair_kernel_ms": [], "match_wall_s": [],
                                 "top_n": {str(top): {"match_kernel_ms": [], "select_ms": [], "search_wall_s": [],
                                                      "search_bytes": n * top * nat.SEARCH_DT.itemsize} for top in tops}}
            matcher.set_patients(res[:n], rows)
            for sr in searchers.values():
                sr.set_patients(res[:n], rows)
            for step in range(args.warmup + args.steps):
                t0 = timeit.default_timer()
                matcher.run(batch)
                matcher.results()
                wall = timeit.default_timer() - t0
                if step >= args.warmup:
                    rec["match_wall_s"].append(wall)
                    rec["match_pair_kernel_ms"].append(matcher.kernel_ms())
                for top, sr in searchers.items():  # alternating with the matcher, on the same batch
                    sr.reset()
                    t0 = timeit.default_timer()
                    sr.run(batch, ids)
                    sr.results()
                    wall = timeit.default_timer() - t0
                    if step >= args.warmup:
                        at = rec["top_n"][str(top)]
                        at["search_wall_s"].append(wall)
                        at["select_ms"].append(sr.select_ms())
                        at["match_kernel_ms"].append(sr.kernel_ms() - sr.select_ms())
            for top, sr in searchers.items():
                rec["top_n"][str(top)]["stats"] = sr.stats()
                rec["top_n"][str(top)]["hits"] = int(sr.results()[1].sum())
        if args.merge_lists > 0:  # (e): the last patient count, the largest top_n; the searcher's patients are still set
            from grim.search import merge_hit_lists

            n, top = counts[-1], max(tops)
            sr = searchers[top]
            whole = sr.results()
            made = []
            for part in range(args.merge_lists):  # the donors dealt round-robin: every list is full
                sr.reset()
                sr.run_records(res[part::args.merge_lists], rows, ids[part::args.merge_lists])
                made.append(sr.results())
            lists = (np.stack([m[0] for m in made]), np.stack([m[1] for m in made]))
            leg = merge = {"lists": args.merge_lists, "patients": n, "top_n": top, "upload_bytes": lists[0].nbytes + lists[1].nbytes,
                           "merge_select_ms": [], "merge_wall_s": [], "python_merge_s": []}
            for step in range(args.warmup + args.steps):
                sr.reset()
                t0 = timeit.default_timer()
                sr.merge(*lists)
                wall = timeit.default_timer() - t0
                if step >= args.warmup:
                    leg["merge_wall_s"].append(wall)
                    leg["merge_select_ms"].append(sr.select_ms())
            got = sr.results()
            leg["equals_one_run"] = bool(got[0].tobytes() == whole[0].tobytes() and got[1].tobytes() == whole[1].tobytes())
            for step in range(min(3, args.steps)):  # the route it replaces: a Python loop over the hits (search_donors' last step)
                t0 = timeit.default_timer()
                twin = merge_hit_lists(made, top, 0.0)
                leg["python_merge_s"].append(timeit.default_timer() - t0)
            leg["python_equals_device"] = bool(twin[0].tobytes() == got[0].tobytes())
    finally:
        for sr in searchers.values():
            sr.close()
        matcher.close()
        batch.close()
        parsed.close()

    def med(d):
        for k, v in list(d.items()):
            if isinstance(v, list):
                d[k + "_spread"] = [min(v), max(v)]
                d[k] = statistics.median(v)
            elif isinstance(v, dict):
                med(v)

    med(out)
    if merge is not None:
        med(merge)
    print(json.dumps({
        "workload": "pop4 graph, %d mixed subjects (seed 3) as donors, MR priors, keep %s, min_p0 0.0" % (args.subjects, "~".join(keep)),
        "steps": args.steps, "warmup": args.warmup, "patients": out, "merge": merge,
    }))


if __name__ == "__main__":
    main()
