"""
Measure the fixed-support refresh (csrc/grim_refresh.h, Graph.refresh) against what it replaces, on one graph per process:

  (a) refresh_ms     grim_graph_refresh_ms of one refresh through the records door: its kernels and the in-place commit
                     between their own HIP events
  (b) refresh_wall_s the same call seen from Python: records up, kernels, commit (ends in a stream synchronise)
  (c) route_s        the route of grim.em.em_iteration on the same counts, wall time: write_freq_files + produce_hpf +
                     graph_from_freqs (generator and loader back to back in the library) + upload; its four parts are
                     listed too

    python tools/refresh_bench.py --graph pop4|wmda [--steps K] [--warmup W] [--route-steps R]

pop4 is bench.py's config-4 graph, wmda config 5's synthetic graph (tools/wmda_scale.py).  The two sides alternate: every
route step is followed by steps / route-steps refresh steps.  One JSON line: medians and spans (min, max).  The counts are
seeded and give every full haplotype a positive count in every population it has, so the regenerated graph keeps the size.
"""
import argparse
import atexit
import json
import os
import shutil
import statistics
import sys
import tempfile
import timeit

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import harness  # noqa: E402


def _span(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", choices=["pop4", "wmda"], default="pop4")
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--route-steps", type=int, default=3)
    args = ap.parse_args()

    import __graft_entry__ as ge
    ge.build()
    import numpy as np
    from graph_generation.generate_hpf import produce_hpf
    from grim import _native as nat
    from grim.em import write_freq_files
    from grim.grim import graph_from_freqs
    from grim.imputation.networkx_graph import Graph
    from grim.run_impute_def import load_config

    if args.graph == "pop4":
        pops = harness.POPS["pop4"]
        work = harness.ensure_graph("pop4")
        conf = harness.base_conf(pops)
    else:
        import wmda_scale

        pops = list(wmda_scale.POPS)
        work = wmda_scale.ensure()
        conf = wmda_scale.conf()
    tmp = tempfile.mkdtemp(prefix="refresh_bench_", dir=work)
    atexit.register(shutil.rmtree, tmp, True)
    conf = dict(conf, freq_data_dir=os.path.join(tmp, "freqs"), freq_file=os.path.join(tmp, "hpf.csv"),
                pops_count_file=os.path.join(tmp, "pop_counts_file.txt"))
    graph_conf = dict(conf, graph_files_path=os.path.join(work, "output", "csv") + "/", imputation_in_file=os.path.join(tmp, "none.csv"),
                      imputation_out_path=os.path.join(tmp, "out"))
    cpath = os.path.join(tmp, "conf.json")
    with open(cpath, "w") as fh:
        json.dump(graph_conf, fh)
    cfg, _ = load_config(cpath)
    g = Graph(cfg).build_graph(cfg["node_file"], cfg["top_links_file"], cfg["edges_file"])
    a = g.arrays
    V, P = int(a["n_nodes"]), int(a["n_pops"])
    full = np.flatnonzero(a["node_mask"] == a["full_mask"])
    # seeded counts: a positive count wherever the graph's haplotype has a frequency in that population
    rng = np.random.default_rng(17)
    has = a["freq"][full] > 0.0
    order = np.argsort(a["node_key"][full], kind="stable")
    fi, pi = np.nonzero(has[order])
    keys = np.ascontiguousarray(a["node_key"][full][order][fi], dtype=np.uint64)
    kpops = np.ascontiguousarray(pi, dtype=np.uint32)
    counts = rng.random(len(keys)) * 10.0 + 0.5
    names = {}
    by_name = {p: {} for p in pops}
    for k, p, c in zip(keys.tolist(), kpops.tolist(), counts.tolist()):
        name = names.get(k)
        if name is None:
            name = names[k] = g.key_to_name(k)
        by_name[pops[p]][name] = c

    ctx = nat.default_context(None)
    dg = g.device(ctx)
    assert dg.refreshable()
    ms, wall, route, parts, sizes = [], [], [], [], None
    per = max(1, args.steps // max(1, args.route_steps))

    def refresh_steps(n, keep):
        for _ in range(n):
            t0 = timeit.default_timer()
            st = dg.refresh_records(keys, kpops, counts)
            t1 = timeit.default_timer()
            if keep:
                ms.append(st["kernel_ms"])
                wall.append(t1 - t0)

    refresh_steps(args.warmup, False)
    for _ in range(args.route_steps):
        t0 = timeit.default_timer()
        write_freq_files(by_name, conf["freq_data_dir"], pops)
        t1 = timeit.default_timer()
        produce_hpf(cpath, quiet=True)
        t2 = timeit.default_timer()
        g2 = graph_from_freqs(cpath, for_em=True, em_pop=pops)
        t3 = timeit.default_timer()
        dg2 = nat.DeviceGraph(ctx, g2.arrays)
        t4 = timeit.default_timer()
        route.append(t4 - t0)
        parts.append((t1 - t0, t2 - t1, t3 - t2, t4 - t3))
        sizes = (int(g2.arrays["n_nodes"]), int(g2.arrays["a_nbr"].shape[0]))
        dg2.close()
        refresh_steps(per, True)
    print(json.dumps({
        "graph": args.graph, "nodes": V, "full": int(len(full)), "pops": P, "top_links": int(a["a_nbr"].shape[0]), "entries": int(len(keys)),
        "refresh_ms": _span(ms), "refresh_wall_s": _span(wall), "route_s": _span(route),
        "route_parts_s": {k: statistics.median(x[i] for x in parts)
                          for i, k in enumerate(("write_freq_files", "produce_hpf", "graph_from_freqs", "upload"))},
        "route_graph": {"nodes": sizes[0], "top_links": sizes[1]}, "warmup": args.warmup,
    }))


if __name__ == "__main__":
    main()
