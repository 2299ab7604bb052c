"""The fixed-support refresh without a GPU: the CPU twin (grim.em.refresh_freq_arrays) against sums derived independently of
the top-link rows, its refusals, the row-end quirk of the last node, and the bridge to the file route (write_freq_files)."""
import gzip
import json
import os

import numpy as np
import pytest

import harness
import refresh_synth as rs

ABITS, MAXL, BLOCK = 12, 5, 4096
SYNTH = [(F, P) for F in rs.SIZES for P in (1, 3)]
GOLDEN = ["cau", "pop4"]


def golden_graph(name):
    """a Graph of its own over the golden graph files (never the harness's cached one)"""
    from grim.imputation.networkx_graph import Graph
    from grim.run_impute_def import load_config

    work = harness.ensure_graph(name)
    conf = harness.base_conf(harness.POPS[name])
    path = os.path.join(work, "conf_refresh.json")
    with open(path, "w") as fh:
        json.dump(conf, fh)
    cwd = os.getcwd()
    os.chdir(work)
    try:
        cfg, _ = load_config(path)
        return Graph(cfg).build_graph(cfg["node_file"], cfg["top_links_file"], cfg["edges_file"])
    finally:
        os.chdir(cwd)


_graphs = {}


def graph_of(case, tmp_root):
    if case not in _graphs:
        _graphs[case] = golden_graph(case) if isinstance(case, str) else rs.synthetic_graph(str(tmp_root), *case)
    return _graphs[case]


@pytest.fixture(scope="module")
def tmp_root(tmp_path_factory):
    return tmp_path_factory.mktemp("refresh_host")


def _hex(a):
    return [float(x).hex() for x in np.asarray(a).ravel().tolist()]


@pytest.mark.parametrize("case", SYNTH + GOLDEN, ids=lambda c: c if isinstance(c, str) else "F%d_P%d" % c)
def test_twin_equals_sums_by_key_projection(case, tmp_root):
    from grim.em import refresh_freq_arrays

    a = graph_of(case, tmp_root).arrays
    V, P, full_mask = a["n_nodes"], a["n_pops"], a["full_mask"]
    keys, pops, counts = rs.random_counts(a, seed=7)
    assert (counts == 0.0).any() or len(counts) < 40
    freq, stats = refresh_freq_arrays(a, keys, pops, counts)
    assert freq.shape == (V, P) and freq.dtype == np.float64
    table = {(k, p): c for k, p, c in zip(keys.tolist(), pops.tolist(), counts.tolist())}
    node_key, node_mask = a["node_key"].tolist(), a["node_mask"].tolist()
    full = [v for v in range(V) if node_mask[v] == full_mask]
    # the totals: the blocked fold over the full nodes in id order
    c = [[table.get((node_key[v], p), 0.0) for p in range(P)] for v in full]
    for p in range(P):
        t = 0.0
        for b in range(0, len(full), BLOCK):
            s = 0.0
            for i in range(b, min(b + BLOCK, len(full))):
                s = s + c[i][p]
            t = t + s
        assert t.hex() == stats["total"][p].hex()
    assert stats["n_full"] == len(full)
    assert stats["matched"] == sum((node_key[v], p) in table for v in full for p in range(P))
    # full nodes: one division
    new_full = [[c[i][p] / stats["total"][p] for p in range(P)] for i in range(len(full))]
    for i, v in enumerate(full):
        assert _hex(freq[v]) == _hex(new_full[i])
    assert stats["zero_full"] == sum(all(x == 0.0 for x in vec) for vec in new_full)
    assert stats["delta"] == max(abs(new_full[i][p] - float(a["freq"][v][p])) for i, v in enumerate(full) for p in range(P))
    # partial nodes: by projecting every full node's key onto every smaller label, in full-node id order
    slots = [sum(0xFFF << (ABITS * q) for q in range(MAXL) if (m >> q) & 1) for m in range(1 << MAXL)]
    labels = sorted(set(node_mask) - {full_mask})
    proj = {}
    for i, v in enumerate(full):
        for m in labels:
            k = node_key[v] & slots[m]
            vec = proj.get(k)
            if vec is None:
                vec = proj[k] = [0.0] * P
            for p in range(P):
                vec[p] = vec[p] + new_full[i][p]
    partial = [v for v in range(V) if node_mask[v] != full_mask]
    assert partial and len(set(node_key[v] for v in partial)) == len(partial)
    assert set(node_key[v] for v in partial) == set(proj)
    for v in partial:
        assert _hex(freq[v]) == _hex(proj[node_key[v]]), "node %d" % v


def test_last_node_row_ends_at_the_link_count(tmp_root):
    from grim.em import refresh_freq_arrays

    a = graph_of((130, 3), tmp_root).arrays
    V, n_a = a["n_nodes"], len(a["a_nbr"])
    assert a["node_mask"][V - 1] != a["full_mask"]
    assert int(a["a_start"][V]) == V and int(a["a_start"][V]) != n_a  # the sentinel quirk: not an end
    lo = int(a["a_start"][V - 1])
    assert lo < n_a and not lo < int(a["a_start"][V])  # read as an end, the sentinel would leave the last node no row
    keys, pops, counts = rs.random_counts(a, seed=3, absent=0.0, zeros=0.0)
    freq, _ = refresh_freq_arrays(a, keys, pops, counts)
    want = [0.0] * a["n_pops"]
    for r in a["a_nbr"][lo:n_a].tolist():
        for p in range(a["n_pops"]):
            want[p] = want[p] + float(freq[r][p])
    assert all(x > 0.0 for x in want)
    assert _hex(freq[V - 1]) == _hex(want)


def test_twin_refusals(tmp_root):
    from grim.em import refresh_freq_arrays, refreshable_rows

    a = graph_of((65, 3), tmp_root).arrays
    keys, pops, counts = rs.random_counts(a, seed=5)
    before = a["freq"].tobytes()
    refresh_freq_arrays(a, keys, pops, counts)

    def refused(k=keys, p=pops, c=counts, arrays=a, match=None):
        with pytest.raises(ValueError, match=match):
            refresh_freq_arrays(arrays, k, p, c)

    refused(k=None, match="null")
    bad = pops.copy()
    bad[3] = 3
    refused(p=bad, match="population")
    bad = keys.copy()
    bad[-1] |= np.uint64(1 << 60)
    refused(k=bad, match="bit")
    refused(k=keys[::-1].copy(), p=pops[::-1].copy(), c=counts[::-1].copy(), match="ascending")
    refused(k=np.concatenate([keys[:1], keys]), p=np.concatenate([pops[:1], pops]), c=np.concatenate([counts[:1], counts]), match="ascending")
    for v in (-1.0, float("nan"), float("inf")):
        bad = counts.copy()
        bad[2] = v
        refused(c=bad, match="count")
    only0 = pops == 0  # populations 1 and 2 without any count
    refused(k=keys[only0], p=pops[only0], c=counts[only0], match="no count inside the support")
    refused(k=keys[:0], p=pops[:0], c=counts[:0], match="no count inside the support")
    # graphs that cannot be refreshed: a full node given a row, an empty row, a link to a haplotype that does not project
    V, F = a["n_nodes"], 65
    hand = dict(a)
    hand["a_start"] = a["a_start"].copy()
    hand["a_start"][1:F + 1] = 1  # full node 0 now owns link 0: the first partial node's row no longer begins at 0
    refused(arrays=hand, match="not refreshable")
    hand = dict(a)
    hand["a_start"] = a["a_start"].copy()
    hand["a_start"][F + 1] = hand["a_start"][F]
    refused(arrays=hand, match="not refreshable.*empty")
    hand = dict(a)
    hand["a_nbr"] = a["a_nbr"].copy()
    hand["a_nbr"][0] = F  # a partial node
    refused(arrays=hand, match="not refreshable.*full node")
    hand = dict(a)
    hand["a_nbr"] = a["a_nbr"].copy()
    lo, hi = min(r for r in refreshable_rows(a)[1].values() if r[1] - r[0] < F)  # a node that does not collect every haplotype
    others = sorted(set(range(F)) - set(a["a_nbr"][lo:hi].tolist()))
    hand["a_nbr"][lo] = others[0]
    refused(arrays=hand, match="not refreshable.*project")
    assert a["freq"].tobytes() == before


def test_bridge_to_the_file_route(tmp_path):
    """On counts whose every haplotype is a full node of the graph, the twin's frequencies and the Freq column
    write_freq_files writes differ only in the order of one n-term sum.  cau_em_mr holds two subjects (of 40) whose phased
    rows carry Plan-B joins that are no graph node -- asserted below -- so the counts are folded from the other subjects."""
    from grim.em import fold_pmug_text, refresh_freq_arrays, write_freq_files

    gname, conf, lines, exp, _, hap_pop = harness.golden("cau_em_mr")
    assert hap_pop and gname == "cau"
    g = golden_graph("cau")
    a = g.arrays

    def inside(name):
        v = g.node_of_name(name)
        return v is not None and a["node_mask"][v] == a["full_mask"]

    rows_of = {}
    for line in exp["pmug"].splitlines():
        rows_of.setdefault(line.split(",")[0], []).append(line)
    with_outside = {sid for sid, rows in rows_of.items()
                    if not all(inside(part.rsplit(";", 1)[0]) for l in rows for part in l.split(",")[1:3])}
    assert 0 < len(with_outside) < len(rows_of) // 4, "the scenario's subjects with a counted haplotype outside the graph"
    counts, _ = fold_pmug_text("".join(l + "\n" for sid, rows in rows_of.items() if sid not in with_outside for l in rows))
    assert set(counts) == {"CAU"}
    node_of = {name: g.node_of_name(name) for name in counts["CAU"]}
    assert all(inside(name) for name in node_of)
    n = len(node_of)
    assert n > 50
    recs = sorted((int(a["node_key"][v]), 0, counts["CAU"][name]) for name, v in node_of.items())
    freq, stats = refresh_freq_arrays(a, [k for k, _, _ in recs], [p for _, p, _ in recs], [c for _, _, c in recs])
    assert stats["matched"] == n
    write_freq_files(counts, str(tmp_path), ["CAU"])
    with gzip.open(os.path.join(str(tmp_path), "CAU.freqs.gz"), "rt") as fh:
        rows = [l.rstrip("\n").split(",") for l in fh][1:]
    assert len(rows) == n
    worst = 0.0
    for name, _, f in rows:
        mine, theirs = float(freq[node_of[name]][0]), float(f)
        worst = max(worst, abs(mine - theirs) / theirs)
        assert abs(mine - theirs) <= n * 2.0 ** -52 * theirs, name
    print("bridge: %d counted haplotypes, worst relative difference %r, bound %r" % (n, worst, n * 2.0 ** -52))
    counted = set(node_of.values())
    full = [v for v in range(a["n_nodes"]) if a["node_mask"][v] == a["full_mask"]]
    assert len(full) > n
    assert all(float(freq[v][0]) == 0.0 for v in full if v not in counted)


def test_m_step_counts_keeps_its_signature():
    import inspect

    from grim.em import em_fixed_support, m_step_counts

    assert str(inspect.signature(m_step_counts)) == "(imputation, lines_or_path, config, block_lines=65536, planb=None, em=True, first_capacity=1048576)"
    assert str(inspect.signature(em_fixed_support)) == "(imputation, lines_or_path, config, iterations, block_lines=65536, planb=None, em=True, tol=None)"
