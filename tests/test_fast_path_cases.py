"""The constructed fast-path cases of tools/fastpath_cases.py are what they claim to be -- checked without a GPU and
without the product's device path, so that tests/test_fast_path_gpu.py can rely on them.

Behaviour classes are judged twice: by fastpath_cases.plan_a_by_rule, a short restatement of the ladder rule
(impute.py:1665-1687) on the frequency rows as they were written, and by the CPU oracle on the generated graph; the two have
to agree on the number of phased pairs of every Plan A class.

Not covered here: the verdict function against the product's HOST tokenizer.  tokenise_gl_fast's accept / reject is not
visible through a CPU entry point (grim_tokenize sends a line it rejects through the general tokenizer and reports the same
kind), so that comparison is left to the GPU file, where grim_stream_devtok_lines shows the device's verdicts."""
import os

import numpy as np
import pytest

import fastpath_cases as fc
import harness


@pytest.fixture(scope="module")
def toy_graph():
    return fc.ensure_toy_graph()


@pytest.fixture(scope="module")
def oracle_texts(toy_graph):
    """every behaviour class once through the oracle, number_of_results high enough to see every phased pair"""
    T = fc.toy()
    keys = sorted(T.subjects)
    lines = [fc.make_line(k, T.subjects[k]) for k in keys]
    texts, _ = harness.run_oracle(toy_graph, fc.toy_conf(number_of_results=1000), lines, tag="cases_orc")
    return texts


def _rows_of(text, sid):
    """-> [(text before the probability, probability)] of subject `sid` in an output text"""
    out = []
    for line in text.splitlines():
        f = line.split(",")
        if f[0] == sid:
            out.append((",".join(f[1:-2]), float(f[-2])))
    return out


def test_python_hash_equals_the_library_hash():
    from grim import _native as nat

    T = fc.toy()
    names = [n for n in T.names() if len(n) <= fc.TOKNAME]
    assert any(len(n) == fc.TOKNAME for n in names) and len(names) > 100
    rng = np.random.default_rng(11)
    blobs = [bytes(rng.integers(1, 256, size=int(rng.integers(1, fc.TOKNAME + 1))).astype(np.uint8)) for _ in range(400)]
    blobs += [bytes([255] * 24), b"A", b"A*01:01", b"A*01:01:01", b"A*01:01:01:01"]
    assert {len(b) for b in blobs} >= set(range(1, fc.TOKNAME + 1))
    for n in names + blobs:
        assert fc.tokname_hash(n) == nat.tokname_hash(n), n
    assert nat.tokname_hash(b"x" * 25) == 0  # longer than the device dictionary holds: no hash


def test_wrap_and_chain_names_have_the_home_slots_claimed(toy_graph):
    """the table size comes from the GRAPH's allele count (as engine_devdict_create takes it), the hash from the library"""
    from grim import _native as nat
    from grim.imputation.networkx_graph import Graph
    from grim.run_impute_def import load_config

    T = fc.toy()
    work = harness.ensure_graph(toy_graph)
    _, cpath = harness._write_inputs(work, fc.toy_conf(), [], "cases_cfg")
    cwd = os.getcwd()
    os.chdir(work)
    try:
        cfg, _ = load_config(cpath)
        g = Graph(cfg).build_graph(cfg["node_file"], cfg["top_links_file"], cfg["edges_file"])
    finally:
        os.chdir(cwd)
    for l in fc.LOCI:
        s = g.locus_slot[l]
        assert g.n_graph_alleles[s] == len(T.alleles[l]), l
        assert {g.adict.name(s, i) for i in range(g.n_graph_alleles[s])} == T.alleles[l]  # every designed row survived the trim
    cap = fc.table_capacity(g.n_graph_alleles[g.locus_slot["C"]])
    assert cap == T.capacity["C"]
    assert len(T.wrap_names) >= 3 and len(T.chain_names) >= 3
    for n in T.wrap_names:
        assert nat.tokname_hash(n) & (cap - 1) == cap - 1, n
    for n in T.chain_names:
        assert nat.tokname_hash(n) & (cap - 1) == T.chain_slot != cap - 1, n
    # and the tables the build rule gives: the wrap names spill over the end, the chain names sit in consecutive slots
    tab = {}
    for n in sorted(T.alleles["C"]):  # (any insertion order gives the same occupied set for these six)
        k = fc.tokname_hash(n) & (cap - 1)
        while k in tab:
            k = (k + 1) & (cap - 1)
        tab[k] = n
    where = {n: k for k, n in tab.items()}
    at = sorted(where[n] for n in T.wrap_names)
    assert at[-1] == cap - 1 and at[0] < 3 and at[1] < 3  # one in the last slot, two wrapped to the table's start
    assert max(where[n] for n in T.chain_names) >= T.chain_slot + 2


def test_name_and_field_lengths():
    T = fc.toy()
    assert len(T.n24a) == 24 and len(T.n24r) == 24 and len(T.n25) == 25
    assert len(T.subjects["gl144"]) == 144 and len(T.subjects["gl145"]) == 145
    assert all(len(a) <= 24 for p in T.subjects["gl144"].split("^") for a in p.split("+"))
    for l in fc.LOCI:
        assert {"%s*01:01" % l, "%s*01:01:01" % l, "%s*01:01:01:01" % l} <= T.alleles[l]
    assert len(T.rows) <= 300


def test_verdict_cases_hold_their_verdict():
    d = fc.toy().dictionary()
    cases = fc.verdict_cases()
    assert {v for _, v in cases.values()} == {fc.ACCEPTED, fc.HANDED_BACK, fc.NOT_OFFERED}
    for name, (gl, want) in cases.items():
        assert fc.device_tokenizer_verdict(gl, d) == want, name
        assert fc.device_tokenizer_verdict(gl, d, device_tokenizer=False) == fc.NOT_OFFERED
    # the edges of the rule, one step to either side
    assert fc.device_tokenizer_verdict(cases["gl144"][0], d) == fc.ACCEPTED and len(cases["gl144"][0]) == 144
    assert fc.device_tokenizer_verdict(cases["gl145"][0], d) == fc.NOT_OFFERED and len(cases["gl145"][0]) == 145
    assert fc.line_verdict("", d) == fc.NOT_OFFERED
    assert fc.line_verdict("id," + cases["step0"][0], d) == fc.ACCEPTED
    assert fc.line_verdict("id,%s,TOY" % cases["step0"][0], d) == fc.NOT_OFFERED  # three fields: a raw .problem line


@pytest.mark.parametrize("cls,step", [("step0", 0), ("mid", 3), ("last", 6), ("cube_t", 0), ("cube_d", 0), ("cut_drop", 0),
                                      ("cut_keep", 0), ("hom_a", 0), ("hom_drb1", 0), ("hom_all", 0)])
def test_first_accepting_step_by_the_ladder_rule(cls, step, oracle_texts):
    """judged by the restated ladder rule (default priors: one population, w = 1; epsilon 1e-3: seven steps, the last is 0)"""
    T = fc.toy()
    lad = fc.ladder_of(1e-3)
    assert len(lad) == 7 and lad[-1] == 0.0 and lad[-2] > 0.0
    got, final, _ = fc.plan_a_by_rule(T.subjects[cls], T.freq)
    assert got == step
    # the oracle on the generated graph keeps as many phased pairs
    assert len(_rows_of(oracle_texts["pmug"], cls)) == len(final) > 0


def test_ladder_lengths():
    assert [len(fc.ladder_of(e)) for e in (1e-3, 1e-2, 1e-1, 1.0, 1e31)] == [7, 8, 9, 10, 41]


def test_plan_b_subjects_have_no_plan_a_pair(toy_graph, oracle_texts):
    """by the rule (no candidate pair at any step) and by the oracle (it reports plan b, and a result)"""
    import grim_oracle as go

    T = fc.toy()
    work = harness.ensure_graph(toy_graph)
    conf, _ = harness._write_inputs(work, fc.toy_conf(), [], "cases_pb")
    cwd = os.getcwd()
    os.chdir(work)
    try:
        cfg = go.config_from_json(conf)
        g = go.OGraph(cfg["full_loci"]).load(cfg["node_file"], cfg["top_links_file"], cfg["edges_file"])
        imp = go.OracleImputer(g, cfg)
        for cls in ("planb", "planb2"):
            assert fc.plan_a_by_rule(T.subjects[cls], T.freq) == (None, [], [])
            imp.plan = "a"
            res_m, res_h = imp.impute_one(T.subjects[cls], fc.POP, fc.POP)
            assert imp.plan == "b" and len(res_h["Haps"]) > 0
            assert fc.device_tokenizer_verdict(T.subjects[cls], T.dictionary()) == fc.ACCEPTED
        imp.plan = "a"
        imp.impute_one(T.subjects["step0"], fc.POP, fc.POP)
        assert imp.plan == "a"
    finally:
        os.chdir(cwd)
    assert _rows_of(oracle_texts["pmug"], "planb")


def test_final_cut_twins_differ_by_the_weak_pair(oracle_texts):
    T = fc.toy()
    drop, keep = _rows_of(oracle_texts["pmug"], "cut_drop"), _rows_of(oracle_texts["pmug"], "cut_keep")
    assert len(drop) == 1 and len(keep) == 2
    assert drop[0][1] == keep[0][1] == 2 * 0.02 * 0.02
    assert keep[1][1] == 2 * 1e-4 * 1e-4
    assert keep[0][0].replace("*14:", "*13:") == drop[0][0]
    # by the rule: the weak pair is accepted at no step above the final cut, and only the twin's survives it
    for cls, n in (("cut_drop", 1), ("cut_keep", 2)):
        step, final, at_step = fc.plan_a_by_rule(T.subjects[cls], T.freq)
        assert (step, len(at_step), len(final)) == (0, 1, n)
    assert 2.5e-9 < 8e-4 / 100000 < 1e-8


def test_cube_t_has_sixteen_tied_pairs_and_cube_d_distinct_ones(oracle_texts):
    t = _rows_of(oracle_texts["pmug"], "cube_t")
    assert len(t) == 16 and len({p for _, p in t}) == 1 and len({h for h, _ in t}) == 16
    d = _rows_of(oracle_texts["pmug"], "cube_d")
    probs = [p for _, p in d]
    assert len(set(probs)) == len(probs) >= 10 and probs == sorted(probs, reverse=True)
    T = fc.toy()
    fd = [T.freq[fc.hap([T.cube_d[(c >> k) & 1][k] for k in range(5)])] for c in range(32)]
    assert len({fd[c] * fd[c ^ 31] for c in range(16)}) == 16
    assert max(fd) / min(fd) > 900


def test_placer_alignments_and_neighbours():
    T = fc.toy()
    P = fc.Placer(8)
    for gl in (T.subjects["gl144"], T.subjects["step0"]):
        P.add_all_alignments(gl)
    P.fill_to_last_of_chunk(T.subjects["mid"])
    P.add(T.subjects["gl144"], align=15)
    assert len(P.lines) % 8 == 0
    data = P.data()
    seen = set()
    for c in range(0, len(P.lines), 8):
        off = 0
        for line in P.lines[c:c + 8]:
            gl_off = off + line.index(",") + 1
            if "xx" in line or line.split(",")[1] != T.subjects["mid"]:
                seen.add((line.split(",")[1], gl_off % 16))
            off += len(line) + 1
    assert {a for gl, a in seen if gl == T.subjects["gl144"]} == set(range(16))
    assert {a for gl, a in seen if gl == T.subjects["step0"]} == set(range(16))
    assert data.endswith(b"\n") and not P.data(final_newline=False).endswith(b"\n")
    N = fc.neighbour_pairs(chunk_lines=64)
    n = len(fc.NEIGHBOUR_CLASSES)
    assert len(N.lines) == 2 * n * n
    pairs = {(N.lines[i].split(",")[1] if N.lines[i] else None, N.lines[i + 1].split(",")[1] if N.lines[i + 1] else None)
             for i in range(0, len(N.lines), 2)}
    assert len(pairs) == n * n
