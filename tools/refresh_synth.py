"""
Synthetic graphs and counts for the fixed-support refresh (csrc/grim_refresh.h): shared by tests/test_refresh_*.py and
tools/refresh_bench.py.  Everything is generated from a seed; nothing is read from outside the repository.
"""

import os

import numpy as np

LOCI_MAP = {"A": 1, "B": 2, "C": 3, "DQB1": 4, "DRB1": 5}
FULL_LOCI = "12345"  # as run_impute_def.load_config derives it from the loci_map
POP_NAMES = ["P0", "P1", "P2"]
# alleles per locus: A has one (node "A*01:01" has a top-link row of all F full haplotypes), B two, the others more
RADIX = (("B", 2), ("C", 7), ("DQB1", 30), ("DRB1", 40))
MAX_F = 2 * 7 * 30 * 40
SIZES = [1, 2, 63, 64, 65, 130, 4095, 4096, 4097, 8193]


def haplotype(i):
    """the i-th of MAX_F distinct five-locus haplotypes, alleles in loci_map order"""
    parts = ["A*01:01"]
    for locus, n in RADIX:
        parts.append("%s*%02d:01" % (locus, 1 + i % n))
        i //= n
    return "~".join(parts)


def write_hpf(path, F, P, seed=0):
    """`hap,pop,freq` lines of F distinct haplotypes in P populations; with P > 1 every third haplotype is present in one
    population only"""
    assert 1 <= F <= MAX_F and 1 <= P <= len(POP_NAMES)
    rng = np.random.default_rng(seed)
    with open(path, "w", newline="") as fh:
        fh.write("hap,pop,freq\r\n")
        for i in range(F):
            only = i % P if (P > 1 and i % 3 == 1) else None
            for p in range(P):
                if only is None or only == p:
                    fh.write("%s,%s,%r\r\n" % (haplotype(i), POP_NAMES[p], float(rng.integers(1, 1000)) / 1e6))


def synthetic_graph(workdir, F, P, seed=0):
    """-> a Graph (grim.imputation.networkx_graph) of F full haplotypes in P populations, loaded through
    Graph.build_graph_from_hpf"""
    from grim.imputation.networkx_graph import Graph

    os.makedirs(workdir, exist_ok=True)
    hpf = os.path.join(workdir, "hpf_%d_%d.csv" % (F, P))
    write_hpf(hpf, F, P, seed)
    g = Graph({"full_loci": FULL_LOCI, "loci_map": dict(LOCI_MAP)})
    return g.build_graph_from_hpf(hpf, POP_NAMES[:P], [0.0] * P, dict(LOCI_MAP))


def random_counts(arrays, seed, absent=0.2, zeros=0.1, outside=5, drop_pop=0.2):
    """seeded counts for a graph's arrays in EmAccumulator.export's order -> (keys u64, pops u32, counts f64): entries for
    the full haplotypes of the graph, of which a share `absent` has no entry at all, a share `drop_pop` of the others
    misses one population's entry (when there is more than one population) and a share `zeros` of the entries counts 0.0,
    plus `outside` keys that are no full node of the graph.  Every population keeps at least one positive count."""
    rng = np.random.default_rng(seed)
    P, full_mask = int(arrays["n_pops"]), int(arrays["full_mask"])
    full_keys = sorted(set(int(k) for k, m in zip(arrays["node_key"].tolist(), arrays["node_mask"].tolist()) if m == full_mask))
    table = {}
    for n, k in enumerate(full_keys):
        if n >= P and rng.random() < absent:
            continue
        skip = int(rng.integers(0, P)) if (P > 1 and n >= P and rng.random() < drop_pop) else None
        for p in range(P):
            if p == skip:
                continue
            c = 0.0 if (n >= P and rng.random() < zeros) else float(rng.random() * 10.0 + 1e-3)
            table[(k, p)] = c
    for p in range(P):  # a positive count per population whatever the draws
        table[(full_keys[min(p, len(full_keys) - 1)], p)] = float(rng.random() + 0.5)
    made = 0
    while made < outside:  # keys outside the support: an allele id no graph haplotype has at locus slot 0
        k = (4000 + made) | (int(rng.integers(1, 4000)) << 12)
        made += 1
        for p in range(P):
            table[(k, p)] = float(rng.random() * 3.0)
    order = sorted(table)
    return (np.array([k for k, _ in order], dtype=np.uint64), np.array([p for _, p in order], dtype=np.uint32),
            np.array([table[at] for at in order], dtype=np.float64))


def own_imputation(gname, conf, tag="refresh"):
    """-> an Imputation over a Graph of its OWN, loaded from the files of the harness graph `gname` under the configuration
    dict `conf` (a refresh changes the graph, so the harness's cached one is never used); quiet, unsupported subjects skipped"""
    import harness
    from grim.imputation.impute import Imputation
    from grim.imputation.networkx_graph import Graph
    from grim.run_impute_def import load_config

    work = harness.ensure_graph(gname)
    _, cpath = harness._write_inputs(work, conf, [], tag)
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
    return imp


def with_freq(imp, freq):
    """-> a second Imputation like `imp` over a second Graph object whose arrays are a copy of imp's graph's with `freq` in
    place of its frequencies, never uploaded yet: what a fresh upload of those numbers sees"""
    from grim.imputation.impute import Imputation
    from grim.imputation.networkx_graph import Graph

    cfg = imp.config
    g = Graph(cfg)
    g.arrays = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in imp.netGraph.arrays.items()}
    g.arrays["freq"] = np.ascontiguousarray(freq, dtype=np.float64).copy()
    # the same allele ids: the dictionary is filled in the order the first graph's was
    src = imp.netGraph.adict
    for s in range(len(g.full_loci)):
        for i in range(src.count(s)):
            assert g.adict.intern(s, src.name(s, i)) == i
    g.n_graph_alleles = list(imp.netGraph.n_graph_alleles)
    other = Imputation(g, cfg, count_by_prob=imp.count_by_prob)
    other.on_unsupported = imp.on_unsupported
    other.quiet = imp.quiet
    return other
