"""The fixed-support refresh on the device (csrc/grim_refresh.h through grim/_native.py, Graph.refresh and grim/em.py) against
the CPU twin (grim.em.refresh_freq_arrays), bit for bit: both doors, both row kernels at their edges, the totals' block edges,
imputation on a refreshed graph against a fresh upload of the same numbers, the refusals, and the EM loop."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import harness
import refresh_synth as rs

pytestmark = pytest.mark.gpu

SYNTH = [(F, P) for F in rs.SIZES for P in (1, 3)]
GOLDEN = ["cau", "pop4"]
STAT_KEYS = ("matched", "zero_full", "n_full")
_graphs = {}


@pytest.fixture(scope="module")
def tmp_root(tmp_path_factory):
    return tmp_path_factory.mktemp("refresh_gpu")


def graph_of(case, tmp_root):
    """a Graph per case, its arrays never changed by a test (device copies are made per test)"""
    if case not in _graphs:
        if isinstance(case, str):
            _graphs[case] = rs.own_imputation(case, harness.base_conf(harness.POPS[case]), tag="refresh_g").netGraph
        else:
            _graphs[case] = rs.synthetic_graph(str(tmp_root), *case)
    return _graphs[case]


def _ctx():
    from grim import _native as nat

    return nat.default_context(None)


def _same_stats(got, want):
    assert [float(x).hex() for x in got["total"]] == [float(x).hex() for x in want["total"]]
    assert float(got["delta"]).hex() == float(want["delta"]).hex()
    assert {k: got[k] for k in STAT_KEYS} == {k: want[k] for k in STAT_KEYS}


# ---- 1. the records door against the twin -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SYNTH + GOLDEN, ids=lambda c: c if isinstance(c, str) else "F%d_P%d" % c)
def test_records_door_equals_twin(case, tmp_root):
    from grim import _native as nat
    from grim.em import refresh_freq_arrays

    a = graph_of(case, tmp_root).arrays
    keys, pops, counts = rs.random_counts(a, seed=7)  # absent haplotypes, keys outside the support, a population's entry missing
    want, wstats = refresh_freq_arrays(a, keys, pops, counts)
    dg = nat.DeviceGraph(_ctx(), a)
    try:
        assert dg.refreshable()
        assert dg.freq().tobytes() == a["freq"].tobytes()
        got = dg.refresh_records(keys, pops, counts)
        assert dg.freq().tobytes() == want.tobytes()
        _same_stats(got, wstats)
        assert got["kernel_ms"] > 0.0
    finally:
        dg.close()


# ---- 2. the accumulator door ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first_capacity", [1 << 20, 64])
@pytest.mark.parametrize("scenario", ["cau_em_mr", "pop4_em_mr"])
def test_accumulator_door_equals_twin(scenario, first_capacity):
    from grim import _native as nat
    from grim.blocks import Blocks
    from grim.em import _accumulate_blocks, refresh_freq_arrays

    gname, conf, lines, _, _, hap_pop = harness.golden(scenario)
    assert hap_pop
    imp = rs.own_imputation(gname, conf, tag="refresh_acc")
    g = imp.netGraph
    shared = Blocks(imp, imp.config, None, True, bool(conf.get("_em")), output_haplotypes=True)
    acc = nat.EmAccumulator(shared.ctx, [g.adict.count(s) for s in range(len(g.full_loci))], len(imp.populations), first_capacity)
    try:
        _accumulate_blocks(imp, shared, lines, 16, acc)
        assert (acc.stats()["rehashes"] > 0) == (first_capacity == 64)
        keys, pops, counts = acc.export()
        assert len(keys) > 40
        want, wstats = refresh_freq_arrays(g.arrays, keys, pops, counts)
        assert 0 < wstats["matched"] < len(keys)  # some counted haplotypes are no node of the graph
        got = shared.dgraph.refresh(acc)
        assert shared.dgraph.freq().tobytes() == want.tobytes()
        _same_stats(got, wstats)
    finally:
        acc.close()


# ---- 3. imputation after a refresh equals imputation on a fresh upload ------------------------------------------------------
@pytest.mark.parametrize("no_small", ["", "1"])
def test_imputation_after_refresh_cau_full(no_small):
    """fully typed subjects: the half-wave kernel reads the full-haplotype table's inline frequency, so a stale one shows here;
    with GRIM_NO_SMALL=1 the same subjects go through the other plan-A kernels.  The switch is read once: own processes."""
    env = dict(os.environ)
    env.pop("GRIM_NO_SMALL", None)
    if no_small:
        env["GRIM_NO_SMALL"] = no_small
    r = subprocess.run([sys.executable, os.path.join(harness.ROOT, "tools", "refresh_check.py"), "cau_full"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["same"] and out["changed"] and out["no_small"] == no_small and out["subjects"] == 64 and out["rows_after"] > 0


def test_imputation_after_refresh_pop4_mixed():
    from refresh_check import refreshed_pair

    gname, conf, lines, _, _, _ = harness.golden("pop4_mixed")
    imp = rs.own_imputation(gname, conf, tag="refresh_mixed")
    em = bool(conf.get("_em"))
    before = imp.impute_lines(lines, imp.config, em=em)
    stats, fresh = refreshed_pair(imp, seed=13)
    after = imp.impute_lines(lines, imp.config, em=em)
    want = fresh.impute_lines(lines, fresh.config, em=em)
    assert sorted(want) == sorted(after) and len(want) == 6
    for k in want:
        assert after[k] == want[k], k
    assert after["umug"] != before["umug"] and after["umug"]
    assert imp.unsupported == fresh.unsupported


# ---- 4. two refreshes in a row --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(130, 3), (4097, 1)], ids=lambda c: "F%d_P%d" % c)
def test_second_refresh_equals_twin_of_the_second_alone(case, tmp_root):
    from grim import _native as nat
    from grim.em import refresh_freq_arrays

    a = graph_of(case, tmp_root).arrays
    first = rs.random_counts(a, seed=1)
    second = rs.random_counts(a, seed=2, absent=0.5)
    f1, _ = refresh_freq_arrays(a, *first)
    after_first = dict(a, freq=f1)  # only delta looks at the frequencies before
    f2, s2 = refresh_freq_arrays(after_first, *second)
    f2_alone, _ = refresh_freq_arrays(a, *second)
    assert f2.tobytes() == f2_alone.tobytes() and f1.tobytes() != f2.tobytes()
    dg = nat.DeviceGraph(_ctx(), a)
    try:
        dg.refresh_records(*first)
        assert dg.freq().tobytes() == f1.tobytes()
        got = dg.refresh_records(*second)
        assert dg.freq().tobytes() == f2.tobytes()
        _same_stats(got, s2)
    finally:
        dg.close()


def test_graph_refresh_replaces_host_freq_and_drops_other_contexts(tmp_root):
    from grim import _native as nat
    from grim.em import refresh_freq_arrays

    g = rs.synthetic_graph(str(tmp_root), 130, 3)  # a Graph of this test's own: refresh changes it
    old = g.arrays["freq"]
    keys, pops, counts = rs.random_counts(g.arrays, seed=21)
    want, wstats = refresh_freq_arrays(g.arrays, keys, pops, counts)
    ctx = _ctx()
    ctx2 = nat.Context(ctx.device)
    on_ctx2 = []  # closed before their context
    try:
        dg, dg2 = g.device(ctx), g.device(ctx2)
        on_ctx2.append(dg2)
        got = g.refresh(ctx, (keys, pops, counts))
        _same_stats(got, wstats)
        assert g.arrays["freq"] is not old and g.arrays["freq"].tobytes() == want.tobytes()
        assert g._freqs(0) == [float(x) for x in want[0]]
        assert g.device(ctx) is dg and dg.freq().tobytes() == want.tobytes()
        again = g.device(ctx2)  # uploaded anew, from the new numbers
        on_ctx2.append(again)
        assert again is not dg2 and again.freq().tobytes() == want.tobytes()
    finally:
        for d in on_ctx2:
            d.close()
        g._dev = {}
        ctx2.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_bit(tmp_root):
    from grim import _native as nat

    ctx = _ctx()
    a = graph_of((65, 3), tmp_root).arrays
    keys, pops, counts = rs.random_counts(a, seed=5)
    L = nat._refresh_lib()
    dg = nat.DeviceGraph(ctx, a)
    others = []
    try:
        dg.refresh_records(keys, pops, counts)  # so that "before" is not what the upload left
        before = dg.freq().tobytes()
        assert before != a["freq"].tobytes()

        def refused(k, p, c, text, n=None):
            k = None if k is None else np.ascontiguousarray(k, dtype=np.uint64)
            p = None if p is None else np.ascontiguousarray(p, dtype=np.uint32)
            c = None if c is None else np.ascontiguousarray(c, dtype=np.float64)
            n = len(counts) if n is None else n
            st = nat.RefreshStats()
            rc = L.grim_graph_refresh_records(dg.h, None if k is None else nat._ptr(k), None if p is None else nat._ptr(p),
                                              None if c is None else nat._ptr(c), n, C.byref(st))
            assert rc == -3, text
            assert text in ctx.error(), ctx.error()
            assert dg.freq().tobytes() == before, text

        refused(None, pops, counts, "null array")
        refused(keys, None, counts, "null array")
        refused(keys, pops, None, "null array")
        bad = pops.copy()
        bad[3] = 3
        refused(keys, bad, counts, "population")
        bad = keys.copy()
        bad[-1] |= np.uint64(1 << 60)
        refused(bad, pops, counts, "GRIM_KEY_GRAPH_ORDER")
        refused(keys[::-1], pops[::-1], counts[::-1], "ascending")
        refused(np.concatenate([keys[:1], keys]), np.concatenate([pops[:1], pops]), np.concatenate([counts[:1], counts]), "ascending",
                n=len(counts) + 1)
        for v in (-1.0, float("nan"), float("inf")):
            bad = counts.copy()
            bad[2] = v
            refused(keys, pops, bad, "negative, NaN or infinite")
        only0 = pops == 0
        refused(keys[only0], pops[only0], counts[only0], "no count inside the support", n=int(only0.sum()))
        refused(None, None, None, "no count inside the support", n=0)
        with pytest.raises(nat.NativeError):
            dg.refresh_records(keys[only0], pops[only0], counts[only0])
        assert dg.freq().tobytes() == before
        # the accumulator door: another number of populations, another context
        n_alleles = [4000] * 5
        acc = nat.EmAccumulator(ctx, n_alleles, 2)
        others.append(acc)
        assert L.grim_graph_refresh(dg.h, acc.h, None) == -3 and "populations" in ctx.error()
        assert dg.freq().tobytes() == before
        ctx2 = nat.Context(ctx.device)
        others.append(ctx2)
        acc2 = nat.EmAccumulator(ctx2, n_alleles, 3)
        others.insert(0, acc2)  # closed before its context
        assert L.grim_graph_refresh(dg.h, acc2.h, None) == -3 and "another context" in ctx.error()
        assert dg.freq().tobytes() == before
        # an accumulator without counts: every total is 0
        acc3 = nat.EmAccumulator(ctx, n_alleles, 3)
        others.append(acc3)
        with pytest.raises(nat.NativeError, match="no count inside the support"):
            dg.refresh(acc3)
        assert dg.freq().tobytes() == before
    finally:
        for o in others:
            o.close()
        dg.close()


def test_graph_with_a_hand_made_row_is_not_refreshable():
    """a descriptor in which one full node's row was made non-empty by hand: upload succeeds and the graph imputes, it is not
    refreshable, refresh answers -3 and changes nothing -- an imputation run afterwards gives the texts of before"""
    from grim import _native as nat
    from grim.em import refresh_freq_arrays

    gname, conf, lines, _, _, _ = harness.golden("cau_mixed")
    imp = rs.own_imputation(gname, conf, tag="refresh_hand")
    g = imp.netGraph
    ctx = _ctx()
    assert g.device(ctx).refreshable()
    a = g.arrays
    F = int(a["lab_start"][a["full_mask"] + 1] - a["lab_start"][a["full_mask"]])
    assert all(a["node_mask"][:F] == a["full_mask"]) and a["node_mask"][F] != a["full_mask"] and int(a["a_start"][F]) == 0
    hand = a["a_start"].copy()
    hand[1:F + 1] = 1  # full node 0 now owns link 0; the rows of the partial nodes no longer cover it
    a["a_start"] = hand
    g._dev = {}
    keys, pops, counts = rs.random_counts(a, seed=9)
    with pytest.raises(ValueError, match="not refreshable"):
        refresh_freq_arrays(a, keys, pops, counts)
    dg = g.device(ctx)  # upload succeeds
    assert not dg.refreshable()
    texts = imp.impute_lines(lines, imp.config)
    assert texts["umug"]
    before = dg.freq().tobytes()
    assert before == a["freq"].tobytes()
    with pytest.raises(nat.NativeError, match="not refreshable"):
        g.refresh(ctx, (keys, pops, counts))
    st = nat.RefreshStats()
    assert nat._refresh_lib().grim_graph_refresh_records(dg.h, nat._ptr(keys), nat._ptr(pops), nat._ptr(counts), len(keys), C.byref(st)) == -3
    assert dg.freq().tobytes() == before and g.arrays["freq"].tobytes() == before
    assert imp.impute_lines(lines, imp.config) == texts


# ---- 6. the EM loop ---------------------------------------------------------------------------------------------------------
def test_em_fixed_support_equals_host_composition():
    from grim.em import em_fixed_support, m_step_counts, refresh_freq_arrays

    gname, conf, lines, _, _, hap_pop = harness.golden("pop4_em_mr")
    assert hap_pop
    em = bool(conf.get("_em"))
    imp = rs.own_imputation(gname, conf, tag="refresh_em")
    start = imp.netGraph.arrays["freq"].copy()
    pops = imp.populations
    # the host composition: a fresh Graph with the previous twin frequencies -> m_step_counts -> refresh_freq_arrays
    want = []
    freq = start
    for _ in range(3):
        host = rs.with_freq(imp, freq)
        g = host.netGraph
        counts, mstats = m_step_counts(host, lines, host.config, em=em)
        recs = []
        for pi, pop in enumerate(pops):
            for name, c in counts.get(pop, {}).items():
                v = g.node_of_name(name)
                if v is not None and g.arrays["node_mask"][v] == g.arrays["full_mask"]:
                    recs.append((int(g.arrays["node_key"][v]), pi, c))
        recs.sort()
        freq, rstats = refresh_freq_arrays(g.arrays, [r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs])
        assert rstats["matched"] == len(recs)
        want.append((mstats, rstats, freq))
    got = em_fixed_support(imp, lines, imp.config, 3, em=em)
    assert len(got) == 3
    for it, (mstats, rstats, _) in zip(got, want):
        for k in ("subjects_used", "skipped_plan_c", "contributions", "entries", "spill", "blocks"):
            assert it[k] == mstats[k], k
        _same_stats(it, rstats)
        assert it["outside"] == it["entries"] - rstats["matched"] and it["outside"] > 0
        assert it["kernel_ms"] > 0.0 and it["refresh_ms"] > 0.0
    assert imp.netGraph.arrays["freq"].tobytes() == want[-1][2].tobytes()
    assert imp.netGraph.device(_ctx()).freq().tobytes() == want[-1][2].tobytes()
    assert got[0]["delta"] > got[1]["delta"] > 0.0
    # tol at the recorded second delta stops after two iterations
    again = rs.with_freq(imp, start)
    short = em_fixed_support(again, lines, again.config, 3, em=em, tol=got[1]["delta"])
    assert len(short) == 2
    assert [float(x["delta"]).hex() for x in short] == [float(x["delta"]).hex() for x in got[:2]]
    assert again.netGraph.arrays["freq"].tobytes() == want[1][2].tobytes()
