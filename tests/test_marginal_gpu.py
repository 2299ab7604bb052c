"""The device marginal genotype tables (csrc/grim_marginal.h through grim/marginal.py): the goldens against the text twin,
whatever the batch cuts; exact shapes through the host-records door against the record twin, bit for bit; the refusals; the
existing block path next to a reducer."""
import os

import numpy as np
import pytest

import harness

pytestmark = pytest.mark.gpu

SCENARIOS = ["pop4_mixed", "cau_mixed", "cau_save", "cau_edge", "pop4_planc", "bc_cau_default_map", "cau_mr_res1000"]
KEEPS = [("A", "B", "DRB1"), ("DRB1",), ("A", "B", "C", "DQB1", "DRB1")]

_imps = {}


def _imputation(scenario):
    """-> (Imputation on the scenario's graph and configuration, input lines, golden texts, em flag); no run"""
    if scenario in _imps:
        return _imps[scenario]
    from grim.imputation.impute import Imputation
    from grim.imputation.networkx_graph import Graph
    from grim.run_impute_def import load_config

    gname, conf, lines, exp, _, _ = harness.golden(scenario)
    work = harness.ensure_graph(gname)
    em = bool(conf.get("_em"))
    conf, cpath = harness._write_inputs(work, conf, lines, "marg_" + scenario)
    cwd = os.getcwd()
    os.chdir(work)
    try:
        cfg, _ = load_config(cpath)
        g = harness._graph_cache.get(gname)
        if g is None:
            g = harness._graph_cache[gname] = Graph(cfg).build_graph(cfg["node_file"], cfg["top_links_file"], cfg["edges_file"])
        imp = Imputation(g, cfg)
    finally:
        os.chdir(cwd)
    imp.on_unsupported = "raise"
    imp.quiet = True
    _imps[scenario] = (imp, lines, exp, em)
    return _imps[scenario]


# ---- 1. goldens against the twin ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", KEEPS, ids=["~".join(k) for k in KEEPS])
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_golden_marginal_equals_the_twin(scenario, keep):
    from grim.marginal import marginal_umug, reduce_umug_text

    imp, lines, exp, em = _imputation(scenario)
    R = int(imp.config["number_of_results"])
    want = reduce_umug_text(exp["umug"], keep, R)
    if len(keep) < 5:
        assert want != exp["umug"]  # merges, reorderings, ties: the comparison is not vacuous
    else:
        assert want == exp["umug"]
    text, stats = marginal_umug(imp, lines, imp.config, keep, em=em)
    assert stats["undefined"] == 0
    assert text == want
    assert stats["rows_in"] == len(exp["umug"].splitlines())
    assert stats["rows_out"] == len(want.splitlines())
    assert stats["groups"] == len(reduce_umug_text(exp["umug"], keep).splitlines())
    assert stats["kernel_ms"] > 0.0


def test_max_rows_cuts_on_the_device():
    from grim.marginal import marginal_umug, reduce_umug_text

    imp, lines, exp, em = _imputation("cau_mr_res1000")
    for max_rows in (10, 2000):
        text, stats = marginal_umug(imp, lines, imp.config, ("A", "B", "DRB1"), max_rows=max_rows, em=em)
        assert text == reduce_umug_text(exp["umug"], ("A", "B", "DRB1"), max_rows), "max_rows=%d" % max_rows
    assert stats["rows_out"] == stats["groups"]


# ---- 2. batch cuts ------------------------------------------------------------------------------------------------------
def test_batch_cuts_are_invisible():
    from grim.marginal import marginal_umug, reduce_umug_text

    imp, lines, exp, em = _imputation("pop4_mixed")
    keep = ("A", "B", "DRB1")
    want = reduce_umug_text(exp["umug"], keep, int(imp.config["number_of_results"]))
    for block in (1, 7, 65536):
        text, stats = marginal_umug(imp, lines, imp.config, keep, block_lines=block, em=em)
        assert text == want, "block_lines=%d" % block
        assert stats["blocks"] <= -(-len(lines) // block)


# ---- 3. exact shapes through the host-records door ----------------------------------------------------------------------
SIZES = [1, 63, 64, 65, 128, 129, 256, 257, 1000]  # 256 / 257: the last subject staged in LDS, the first in the global scratch
CASES = ["one_group", "distinct", "interleaved_ties", "swapped"]
ABITS = 12


def _key(fields):
    k = 0
    for s, f in enumerate(fields):
        k |= int(f) << (ABITS * s)
    return k


def _subject(case, n):
    """n rows (a, b, p) of one subject; slots 0, 1, 4 are the ones the proper subsets keep"""
    rows = []
    for k in range(n):
        noise = (k % 4000) + 1
        p = [0.1, 0.2, 0.3][k % 3] * 10.0 ** -(k % 5)
        if case == "one_group":  # equal on slots 0, 1, 4; slots 2 and 3 tell the rows apart; slot 3 untyped in every third row
            q = 0 if k % 3 == 0 else noise
            fa, fb = [5, 6, noise, q, 7], [8, 9, 4001 - noise, q, 10]
        elif case == "distinct":
            fa, fb = [noise, 6, 3, 3, 7], [8, 9, 3, 3, 10]
        elif case == "interleaved_ties":  # 7 groups, leaders 0..6, rows dealt round; groups g and g + 3 add up the same numbers
            g = k % 7
            p = [0.1, 0.2, 0.3][g % 3] * 10.0 ** -((k // 7) % 5)
            fa, fb = [20 + g, 6, noise, 3, 7], [8, 9, 3, noise, 10 + g]
        else:  # swapped: rows 2i and 2i+1 are one genotype whose alleles at slot 0 (and at slot 4) changed haplotypes
            g = (k // 2) % 50
            fa, fb = [30 + g, 6, noise, 3, 7], [90 + g, 9, 3, noise, 10]
            if k % 2:
                fa[0], fb[0] = fb[0], fa[0]
                fa[4], fb[4] = fb[4], fa[4]
        rows.append((_key(fa) | ((k % 2) << 60), _key(fb) | (((k // 2) % 2) << 60), p))
    return rows


def _batch(subjects, extra_rows=0):
    """[(status, rows)] -> (res, rows) records, rows back to back"""
    from grim import _native as nat

    res = np.zeros(len(subjects), dtype=nat.RESULT_DT)
    flat = []
    for i, (status, rows) in enumerate(subjects):
        res[i]["status"], res[i]["plan"], res[i]["reason"] = status, ord("abc"[i % 3]), 2 if status == nat.ST_UNSUPPORTED else 0
        res[i]["row_off"][nat.T_UMUG], res[i]["n_rows"][nat.T_UMUG] = len(flat), len(rows)
        res[i]["n_genotypes"], res[i]["n_pairs"], res[i]["max_prob"] = len(rows), 5, 0.5
        res[i]["row_off"][nat.T_PMUG], res[i]["n_rows"][nat.T_PMUG] = len(flat), len(rows)
        flat += rows
    out = np.zeros(len(flat) + extra_rows, dtype=nat.ROW_DT)
    for k, (a, b, p) in enumerate(flat):
        out[k] = (a, b, p, 3, 4)
    return res, out


def _same(got, want):
    (gres, grows, gstats), (wres, wrows, wstats) = got, want
    assert gstats == wstats
    assert gres.tobytes() == wres.tobytes()
    assert len(grows) == len(wrows)
    assert [float(x).hex() for x in grows["prob"]] == [float(x).hex() for x in wrows["prob"]]
    assert grows.tobytes() == wrows.tobytes()


@pytest.fixture(scope="module")
def ctx():
    from grim import _native as nat

    return nat.default_context(None)


@pytest.fixture(scope="module")
def shapes():
    from grim import _native as nat

    subjects = [(nat.ST_OK, _subject(case, n)) for n in SIZES for case in CASES]
    subjects.insert(3, (nat.ST_MISS, _subject("distinct", 5)))
    subjects.insert(9, (nat.ST_OK, []))
    subjects.insert(20, (nat.ST_UNSUPPORTED, []))
    res, rows = _batch(subjects)
    m = len(rows)
    # two subjects whose offsets point past the rows given: skipped, not read
    bad = np.zeros(2, dtype=nat.RESULT_DT)
    bad["row_off"][:, nat.T_UMUG] = [m - 1, m + 7]
    bad["n_rows"][:, nat.T_UMUG] = [5, 1]
    res = np.concatenate([res[:11], bad[:1], res[11:], bad[1:]])
    return res, rows


@pytest.mark.parametrize("max_rows", [1, 10, 2000])
@pytest.mark.parametrize("mask", [0b10011, 0b10000, 0b11111])
def test_shapes_bit_for_bit(ctx, shapes, mask, max_rows):
    from grim import _native as nat
    from grim.marginal import reduce_records

    res, rows = shapes
    want = reduce_records(res, rows, mask, max_rows)
    if mask == 0b10011:  # what the cases were built for
        assert want[2]["groups"] < want[2]["rows_in"] and want[2]["undefined"] == 0 and want[2]["subjects"] == len(SIZES) * len(CASES)
    red = nat.MarginalReducer(ctx, mask, max_rows)
    try:
        red.reduce_records(res, rows)
        got = red.results() + (red.stats(),)
        assert red.kernel_ms() > 0.0
    finally:
        red.close()
    _same(got, want)


def test_shape_properties_of_the_twin():
    """the cases hold what their names say, so the comparison above covers it"""
    from grim.marginal import reduce_records
    from grim import _native as nat

    for n in (64, 129, 1000):
        for case, groups in (("one_group", 1), ("distinct", n), ("interleaved_ties", 7), ("swapped", min(n // 2 + n % 2, 50))):
            res, rows = _batch([(nat.ST_OK, _subject(case, n))])
            ores, orows, stats = reduce_records(res, rows, 0b10011, 2000)
            assert stats["groups"] == groups, (case, n)
            if case == "interleaved_ties":
                sums = [float(x) for x in orows["prob"][:7]]
                lead = [(int(x) & 0xFFF) - 20 for x in orows["a"][:7]]
                assert len(set(sums)) < 7  # exact ties ...
                assert all(sums[i] > sums[i + 1] or (sums[i] == sums[i + 1] and lead[i] < lead[i + 1]) for i in range(6))  # ... in leader order
            if case == "swapped" and n >= 2:
                assert int(rows["a"][0]) & 0xFFF != int(rows["a"][1]) & 0xFFF  # equal only after the per-slot swap


def test_one_subject_alone_and_reuse_of_a_reducer(ctx):
    from grim import _native as nat
    from grim.marginal import reduce_records

    red = nat.MarginalReducer(ctx, 0b10011, 3)
    try:
        for case, n in (("interleaved_ties", 65), ("swapped", 300), ("one_group", 1)):  # grows, then shrinks again
            res, rows = _batch([(nat.ST_OK, _subject(case, n))])
            red.reduce_records(res, rows)
            _same(red.results() + (red.stats(),), reduce_records(res, rows, 0b10011, 3))
        # nothing to reduce
        res, rows = _batch([(nat.ST_MISS, []), (nat.ST_OK, [])])
        red.reduce_records(res, rows)
        gres, grows = red.results()
        assert len(grows) == 0 and not gres["n_rows"].any() and list(gres["status"]) == [nat.ST_MISS, nat.ST_OK]
        assert red.stats() == dict.fromkeys(nat.MARGINAL_STATS, 0)
    finally:
        red.close()


def test_undefined_rows_are_counted(ctx):
    from grim import _native as nat
    from grim.marginal import reduce_records

    good = _subject("distinct", 70)
    bad = list(good)
    a, b, p = bad[66]
    bad[66] = (a & ~(0xFFF << (ABITS * 2)), b, p)  # slot 2 typed on one haplotype only
    res, rows = _batch([(nat.ST_OK, good), (nat.ST_OK, bad), (nat.ST_OK, good)])
    red = nat.MarginalReducer(ctx, 0b10011, 10)
    try:
        red.reduce_records(res, rows)
        got = red.results() + (red.stats(),)
    finally:
        red.close()
    assert got[2]["undefined"] == 1
    _same(got, reduce_records(res, rows, 0b10011, 10))


# ---- 4. refusals --------------------------------------------------------------------------------------------------------
def _empty(red):
    from grim import _native as nat

    return red.subjects() == 0 and red.total_rows() == 0 and red.kernel_ms() == 0.0 and red.stats() == dict.fromkeys(nat.MARGINAL_STATS, 0)


def test_refusals_leave_the_reducer_empty():
    from grim import _native as nat

    imp, lines, _, _ = _imputation("cau_edge")
    g = imp.netGraph
    ctx = nat.default_context(imp.device)
    L = nat.lib()
    parsed = nat.Parsed(g.adict, ("\n".join(lines) + "\n").encode(), True)
    red = nat.MarginalReducer(ctx, 0b10011, 10)
    none = nat.MarginalReducer(ctx, 0, 10)
    wide = nat.MarginalReducer(ctx, 1 << len(g.full_loci), 10)
    batches = []
    try:
        priors = np.ones((max(1, len(parsed.races())), 1, 1))
        on = nat.DeviceBatch(ctx, g.device(ctx), imp._params(imp.config, True, False), parsed.subjects(), parsed.tokens(), priors)
        off = nat.DeviceBatch(ctx, g.device(ctx), imp._params(dict(imp.config, output_MUUG=False), True, False), parsed.subjects(),
                              parsed.tokens(), priors)
        batches += [on, off]
        # a batch that has not run
        assert L.grim_marginal_reduce(red.h, on.h) < 0
        assert "no finished run" in ctx.error() and _empty(red)
        on.run()
        off.run()
        red.reduce(on)
        assert red.stats()["rows_in"] > 0 and not _empty(red)
        # a batch built with output_MUUG off, after a reduce that worked
        assert L.grim_marginal_reduce(red.h, off.h) < 0
        assert "out_muug" in ctx.error() and _empty(red)
        with pytest.raises(nat.NativeError):
            red.reduce(off)
        # a keep_mask of 0, and one beyond the graph's loci
        assert L.grim_marginal_reduce(none.h, on.h) < 0
        assert "keep_mask" in ctx.error() and _empty(none)
        assert L.grim_marginal_reduce(wide.h, on.h) < 0
        assert "keep_mask" in ctx.error() and _empty(wide)
        with pytest.raises(nat.NativeError):
            none.reduce_records(*_batch([(nat.ST_OK, _subject("distinct", 3))]))
        assert _empty(none)
    finally:
        for b in batches:
            b.close()
        for r in (red, none, wide):
            r.close()
        parsed.close()


# ---- 5. the existing path next to a reducer -----------------------------------------------------------------------------
def test_block_path_texts_unchanged_next_to_a_reducer():
    from grim.marginal import marginal_umug

    imp, lines, exp, em = _imputation("pop4_mixed")
    before = imp.impute_lines_block(lines, imp.config, em=em)
    marginal_umug(imp, lines, imp.config, ("A", "B", "DRB1"), em=em)
    after = imp.impute_lines_block(lines, imp.config, em=em)
    assert before == after
    assert before["umug"] == exp["umug"]


def test_unknown_locus_raises_before_anything_runs():
    from grim.marginal import marginal_umug

    imp, lines, _, em = _imputation("cau_edge")
    with pytest.raises(ValueError):
        marginal_umug(imp, lines, imp.config, ("A", "DPB1"), em=em)
    with pytest.raises(ValueError):
        marginal_umug(imp, lines, imp.config, (), em=em)
