"""The device M-step (csrc/grim_em.h through grim/em.py) against the fold of the reference's golden .pmug files, against the
fold of the product's own text whatever the batch cuts, through table growth, private alleles, the mass property and an
end-to-end EM iteration; then the kernels at chosen shapes through the host-records door, against the record twin
(grim.em.fold_records), every comparison bit for bit."""
import json
import math
import os
import shutil

import numpy as np
import pytest

import harness
import synth

pytestmark = pytest.mark.gpu

POP4 = harness.POPS["pop4"]


def _hex(counts):
    return {pop: {hap: float(c).hex() for hap, c in d.items()} for pop, d in counts.items()}


def _product(gname, conf, lines, tag):
    """the product's six texts with hap;pop rows, and the Imputation (graph + configuration) that made them"""
    got, _, imp = harness.run_product(gname, conf, lines, tag=tag, em_mr=True, on_unsupported="skip", quiet=True)
    return got, imp


@pytest.mark.parametrize("scenario", ["pop4_em_mr", "cau_em_mr", "pop4_planc_rerun_em"])
def test_counts_equal_fold_of_reference_pmug(scenario):
    from grim.em import fold_pmug_text, m_step_counts

    gname, conf, lines, exp, _, hap_pop = harness.golden(scenario)
    assert hap_pop
    _, imp = _product(gname, conf, lines, "em_" + scenario)
    counts, stats = m_step_counts(imp, lines, imp.config, em=bool(conf.get("_em")))
    want, wstats = fold_pmug_text(exp["pmug"])
    assert set(counts) == set(want) and all(set(counts[p]) == set(want[p]) for p in want)
    assert _hex(counts) == _hex(want)
    assert stats["subjects_used"] == wstats["subjects_used"] and stats["contributions"] == wstats["contributions"]


@pytest.fixture(scope="module")
def mixed3000():
    rows = synth.read_freqs(synth.CAU_FREQS)
    lines = synth.SubjectGen(rows, 31, pops=POP4).mixed(3000)
    conf = harness.base_conf(POP4)
    conf["UNK_priors"] = "MR"
    conf["_em"] = True
    got, imp = _product("pop4", conf, lines, "em_mixed")
    return lines, imp, got


def test_batch_cuts_are_invisible(mixed3000):
    from grim.em import fold_pmug_text, m_step_counts

    lines, imp, got = mixed3000
    want, _ = fold_pmug_text(got["pmug"])
    assert sum(len(d) for d in want.values()) > 1000
    for block in (1, 7, 1000, 65536):
        counts, stats = m_step_counts(imp, lines, imp.config, block_lines=block)
        assert _hex(counts) == _hex(want), "block_lines=%d" % block
        assert stats["blocks"] == -(-len(lines) // block)


def test_table_growth_keeps_every_bit(mixed3000):
    from grim.em import fold_pmug_text, m_step_counts

    lines, imp, got = mixed3000
    want, _ = fold_pmug_text(got["pmug"])
    for block in (250, 65536):
        counts, stats = m_step_counts(imp, lines, imp.config, block_lines=block, first_capacity=64)
        assert stats["rehashes"] > 0
        assert _hex(counts) == _hex(want)


def test_private_alleles_come_back_through_the_spill_list():
    from grim.em import fold_pmug_text, m_step_counts

    lines = synth.edge_cases("CAU")
    conf = harness.base_conf(["CAU"])
    conf["_em"] = True
    known = {a for hap, _, _ in synth.read_freqs(synth.CAU_FREQS) for a in synth.hap_alleles(hap).values()}
    otext, _ = harness.run_oracle("cau", conf, lines, tag="em_edge_orc", em_mr=True)
    phased = {a for l in otext["pmug"].splitlines() for part in l.split(",")[1:3] for a in part.split(";")[0].split("~")}
    assert phased - known, "no phased row of the oracle carries an allele absent from the graph"
    got, imp = _product("cau", conf, lines, "em_edge")
    assert got["pmug"] == otext["pmug"]
    counts, stats = m_step_counts(imp, lines, imp.config)
    want, _ = fold_pmug_text(got["pmug"])
    assert stats["spill"] > 0
    assert _hex(counts) == _hex(want)
    assert any(set(h.split("~")) - known for d in counts.values() for h in d)


def test_mass(mixed3000):
    from grim.em import m_step_counts

    lines, imp, got = mixed3000
    counts, stats = m_step_counts(imp, lines, imp.config, block_lines=1000)
    S, R = stats["subjects_used"], int(imp.config["number_of_results"])
    total = math.fsum(c for d in counts.values() for c in d.values())  # exactly rounded: the test adds no error of its own
    print("mass: sum %r, 2S %d, bound %r" % (total, 2 * S, 2 * S * R * 2.0 ** -52))
    assert abs(total - 2 * S) <= 2 * S * R * 2.0 ** -52
    with_rows = len({l.split(",")[0] for l in got["pmug"].splitlines()})
    assert S + stats["skipped_plan_c"] == with_rows
    assert stats["contributions"] == 2 * len(got["pmug"].splitlines())


def test_block_path_texts_unchanged_next_to_an_accumulator():
    from grim import _native as nat

    gname, conf, lines, exp, _, _ = harness.golden("pop4_em_mr")
    _, imp = _product(gname, conf, lines, "em_same")
    before = imp.impute_lines_block(lines, imp.config, em_mr=True)
    g = imp.netGraph
    acc = nat.EmAccumulator(nat.default_context(imp.device), [g.adict.count(s) for s in range(len(g.full_loci))], len(POP4))
    try:
        after = imp.impute_lines_block(lines, imp.config, em_mr=True)
    finally:
        acc.close()
    assert before == after
    assert before["pmug"] == exp["pmug"]


def test_em_iteration_end_to_end(tmp_path, monkeypatch):
    from grim.em import em_iteration, m_step_counts
    from grim.imputation.impute import Imputation

    work = harness.ensure_graph("cau")
    for sub in ("data", "output"):
        shutil.copytree(os.path.join(work, sub), os.path.join(tmp_path, sub))
    rows = synth.read_freqs(synth.CAU_FREQS)
    lines = synth.SubjectGen(rows, 41).mixed(500)
    conf = json.load(open(os.path.join(harness.GOLD, "cau_em_mr", "conf.json")))
    conf["imputation_in_file"] = "data/subjects/em.csv"
    conf["output_haplotypes"] = True
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("GRIM_QUIET", "1")
    monkeypatch.setenv("GRIM_ON_UNSUPPORTED", "raise")
    with open(conf["imputation_in_file"], "w") as fh:
        fh.write("\n".join(lines) + "\n")
    with open("conf.json", "w") as fh:
        json.dump(conf, fh)
    graph, counts = em_iteration("conf.json")
    assert set(counts) == {"CAU"} and len(counts["CAU"]) > 100
    from grim.run_impute_def import load_config

    cfg, _ = load_config("conf.json")
    imp = Imputation(graph, cfg)
    imp.on_unsupported = "raise"
    imp.quiet = True
    texts = imp.impute_lines(lines, cfg, em_mr=True, em=True)
    assert imp.unsupported == []
    assert texts["pmug"]
    counts2, stats = m_step_counts(imp, lines, cfg)
    S, R = stats["subjects_used"], int(cfg["number_of_results"])
    assert S > 0
    total = math.fsum(counts2["CAU"].values())
    assert abs(total - 2 * S) <= 2 * S * R * 2.0 ** -52


def test_accumulate_refuses_a_batch_without_em_mr():
    from grim import _native as nat

    gname, conf, lines, _, _, _ = harness.golden("cau_em_mr")
    _, imp = _product(gname, conf, lines, "em_refuse")
    g = imp.netGraph
    ctx = nat.default_context(imp.device)
    parsed = nat.Parsed(g.adict, ("\n".join(lines) + "\n").encode(), True)
    acc = nat.EmAccumulator(ctx, [g.adict.count(s) for s in range(len(g.full_loci))], 1)
    try:
        priors = np.ones((max(1, len(parsed.races())), 1, 1))
        params = imp._params(imp.config, True, False)  # em_mr off
        batch = nat.DeviceBatch(ctx, g.device(ctx), params, parsed.subjects(), parsed.tokens(), priors)
        batch.run()
        rc = nat.lib().grim_em_accumulate(acc.h, batch.h)
        assert rc < 0
        assert "em_mr" in ctx.error()
        with pytest.raises(nat.NativeError):
            acc.accumulate(batch)
        assert acc.entries() == 0 and acc.stats()["contributions"] == 0 and acc.kernel_ms() == 0.0
        batch.close()
    finally:
        acc.close()
        parsed.close()


# ---- exact shapes through the host-records door, against the record twin (grim.em.fold_records), bit for bit ---------------
EM_SIZES = [1, 2, 63, 64, 65, 128, 129, 1000]  # rows of a subject: the weight kernel walks them 64 at a time
EM_CASES = ["hot", "distinct", "shared", "private"]
N_ALLELES = [4000] * 5
N_POPS = 4
ABITS = 12
EM_STATS = ("subjects_used", "skipped_plan_c", "contributions")


def _key(fields):
    k = 0
    for s, f in enumerate(fields):
        k |= int(f) << (ABITS * s)
    return k


HOT1, HOT2 = _key([11, 12, 13, 14, 15]), _key([11, 12, 13, 14, 16])
POOL = [_key([100 + i, 200 + i % 7, 300 + i % 3, 5, 50 + i % 11]) for i in range(40)]


def em_subject(case, n, seed=0, size_no=0, P=N_POPS, top=N_ALLELES[0]):
    """n phased rows (a, b, p, popa, popb) of one subject; probabilities of mixed magnitude; bit 60 set on some keys
    hot       one haplotype, or two, in the last population: 64 lanes insert one key at once, one counter takes every term
    distinct  every row a haplotype no other row of any subject names ((seed, size_no) tell the subjects apart)
    shared    40 haplotypes that recur across rows, subjects and populations
    private   slot 2 untyped in every third row; slot 4 AT `top` (the last dictionary allele) in every row and slot 0 in
              some; slot 1 at top + 1 (private) in every fifth row; populations running past P on both sides"""
    rows = []
    for k in range(n):
        p = [0.1, 0.2, 0.3][k % 3] * 10.0 ** -(k % 5)
        if case == "hot":
            a, b = HOT1, HOT1 if (k + seed) % 3 else HOT2
            pa = pb = P - 1
        elif case == "distinct":
            a, b = _key([1 + k, 1 + seed, 1 + size_no, 7, 9]), _key([1 + k, 1 + seed, 1 + size_no, 7, 10])
            pa, pb = (k + seed) % P, (k // 2) % P
        elif case == "shared":
            a, b = POOL[(7 * k + seed) % 40], POOL[(11 * k + 3 * seed + n) % 40]
            pa, pb = (k + seed) % P, (k // 3 + seed) % P
        else:
            fa = [top if k % 5 == 1 else 500 + k % 13, 600 + (k + seed) % 5, 0 if k % 3 == 0 else 700, 3, top]
            fb = [500 + (k + seed) % 13, top + 1 if k % 5 == 0 else 600, 700, 3, 800 + k % 3]
            a, b = _key(fa), _key(fb)
            pa, pb = k % (P + 2), (k + seed) % (P + 1)
        rows.append((a | ((k % 2) << 60), b | (((k // 2) % 2) << 60), p, pa, pb))
    return rows


def shape_subjects(rounds=19, P=N_POPS, sizes=EM_SIZES):
    """[(status, plan, plan_phased or None, rows, claim)]: every size in every case, `rounds` times with another seed, and
    the subjects the M-step must pass over in between.  claim = (delta, n): the subject says it has n rows from delta past
    the end of the batch's rows (and owns none)."""
    from grim import _native as nat

    subs = [(nat.ST_OK, "ab"[(seed + i) % 2], None, em_subject(case, n, seed, i, P), None)
            for seed in range(rounds) for i, n in enumerate(sizes) for case in EM_CASES]
    extra = rounds + 1
    subs.insert(3, (nat.ST_MISS, "a", None, em_subject("shared", 5, extra, 0, P), None))
    subs.insert(9, (nat.ST_OK, "a", None, [], None))
    subs.insert(11, (nat.ST_OK, "a", None, [], (-1, 5)))
    subs.insert(20, (nat.ST_UNSUPPORTED, "a", None, [], None))
    subs.insert(33, (nat.ST_OK, "c", None, em_subject("shared", 70, extra, 1, P), None))
    subs.insert(40, (nat.ST_OK, "c", "a", em_subject("distinct", 66, extra, 2, P), None))   # phased rows from Plan A: used
    subs.insert(47, (nat.ST_OK, "a", "c", em_subject("distinct", 66, extra, 3, P), None))   # phased rows from Plan C: not used
    subs.append((nat.ST_OK, "b", None, [], (7, 1)))
    return subs


def em_records(subs):
    """subjects of shape_subjects -> (res, rows) records, rows back to back"""
    from grim import _native as nat

    flat = [r for _, _, _, rows, _ in subs for r in rows]
    res = np.zeros(len(subs), dtype=nat.RESULT_DT)
    at = 0
    for i, (status, plan, phased, rows, claim) in enumerate(subs):
        off, n = (at, len(rows)) if claim is None else (max(len(flat) + claim[0], 0), claim[1])
        res[i]["status"], res[i]["plan"], res[i]["plan_phased"] = status, ord(plan), ord(phased) if phased else 0
        res[i]["reason"] = 2 if status == nat.ST_UNSUPPORTED else 0
        res[i]["row_off"][nat.T_PMUG], res[i]["n_rows"][nat.T_PMUG], res[i]["n_pairs"], res[i]["max_prob"] = off, n, n, 0.5
        at += len(rows)
    return res, np.array(flat, dtype=nat.ROW_DT).reshape(-1)


def used_subjects(res, m):
    """indices of the subjects the M-step uses, of records with m rows"""
    from grim import _native as nat

    out = []
    for s, r in enumerate(res):
        off, n = int(r["row_off"][nat.T_PMUG]), int(r["n_rows"][nat.T_PMUG])
        plan = int(r["plan_phased"]) or int(r["plan"])
        if int(r["status"]) == nat.ST_OK and n > 0 and off + n <= m and plan != ord("c"):
            out.append(s)
    return out


def _got(acc):
    keys, pops, counts = acc.export()
    stats = acc.stats()
    assert acc.entries() == len(keys) and acc.spill_count() == len(acc.spill())
    return (keys.tolist(), pops.tolist(), [float(c).hex() for c in counts.tolist()], [tuple(x) for x in acc.spill().tolist()],
            [float(w).hex() for w in acc.spill()["w"].tolist()], {k: stats[k] for k in EM_STATS})


def _want(out, spill=None):
    keys, pops, counts, wspill, stats = out
    spill = wspill if spill is None else spill
    return (keys.tolist(), pops.tolist(), [float(c).hex() for c in counts.tolist()], [tuple(x) for x in spill.tolist()],
            [float(w).hex() for w in spill["w"].tolist()], {k: stats[k] for k in EM_STATS})


def _run_records(ctx, res, rows, n_pops=N_POPS, first_capacity=1 << 14):
    """one accumulator, one call -> (what it holds, its statistics, its last_unsupported, its kernel_ms)"""
    from grim import _native as nat

    acc = nat.EmAccumulator(ctx, N_ALLELES, n_pops, first_capacity)
    try:
        acc.accumulate_records(res, rows)
        return _got(acc), acc.stats(), acc.last_unsupported(), acc.kernel_ms()
    finally:
        acc.close()


@pytest.fixture(scope="module")
def ctx():
    from grim import _native as nat

    return nat.default_context(None)


@pytest.fixture(scope="module")
def shapes():
    from grim.em import fold_records

    subs = shape_subjects()
    res, rows = em_records(subs)
    return subs, res, rows, fold_records(res, rows, N_ALLELES, N_POPS)


def test_the_shape_set_holds_what_it_was_built_for(shapes):
    """read off the twin's result, so that the comparisons below cover it"""
    from grim import _native as nat

    subs, res, rows, (keys, pops, counts, spill, stats) = shapes
    assert len(subs) >= 600 and stats["contributions"] > 200000 and len(keys) > 30000
    terms = {}
    for s in used_subjects(res, len(rows)):
        off, n = int(res[s]["row_off"][nat.T_PMUG]), int(res[s]["n_rows"][nat.T_PMUG])
        for a, b, _, pa, pb in rows[off:off + n].tolist():
            for at in ((a & ((1 << 60) - 1), pa), (b & ((1 << 60) - 1), pb)):
                terms[at] = terms.get(at, 0) + 1
    assert stats["contributions"] == sum(terms.values())
    assert max(terms[at] for at in zip(keys.tolist(), pops.tolist())) > 10000
    assert len(spill) > 0 and (spill["pop"] >= N_POPS).any() and (spill["pop"] < N_POPS).any()
    top = N_ALLELES[0]
    fields = lambda key: [(key >> (ABITS * q)) & 0xFFF for q in range(5)]
    # a field equal to n_alleles is a dictionary allele: it is counted, and no spill record is owed to it
    assert any(top in fields(k) for k in keys.tolist())
    assert all(p >= N_POPS or max(fields(k)) > top for k, p in zip(spill["key"].tolist(), spill["pop"].tolist()))
    assert stats["skipped_plan_c"] == 2 and stats["unsupported"] == 1
    assert stats["subjects_used"] == len(subs) - 8 + 1 == len(used_subjects(res, len(rows)))


@pytest.mark.parametrize("first_capacity", [64, 1 << 20])
def test_shapes_bit_for_bit(ctx, shapes, first_capacity):
    _, res, rows, want = shapes
    got, stats, unsupported, ms = _run_records(ctx, res, rows, first_capacity=first_capacity)
    assert got == _want(want)
    assert unsupported == want[4]["unsupported"]
    assert ms > 0.0
    assert stats["rehashes"] >= 12 if first_capacity == 64 else stats["rehashes"] == 0


def test_cuts_of_records_are_invisible(ctx, shapes):
    from grim import _native as nat

    subs, res, rows, want = shapes
    wkeys, wpops, wcounts, wspill, wstats = want
    for step in (1, 7, 257, len(subs)):
        acc = nat.EmAccumulator(ctx, N_ALLELES, N_POPS)
        try:
            unsupported = 0
            for lo in range(0, len(subs), step):
                acc.accumulate_records(*em_records(subs[lo:lo + step]))  # rows re-based: every call's begin at 0
                unsupported += acc.last_unsupported()
            got = _got(acc)
        finally:
            acc.close()
        spill = wspill.copy()
        spill["batch"], spill["subject"] = wspill["subject"] // step, wspill["subject"] % step
        assert got == _want(want, spill), "calls of %d subjects" % step
        assert unsupported == wstats["unsupported"]


def _one_row_subjects(n):
    from grim import _native as nat

    return [(nat.ST_OK, "a", None, em_subject(EM_CASES[i % 4], 1, i % 50, i // 50), None) for i in range(n)]


EDGES = [("subjects", n, None) for n in (1, 255, 256, 257, 1023, 1024, 1025, 2049)] + \
        [("rows", n, case) for n in (1, 31, 32, 33, 1023, 1024, 1025, 2047, 2048, 2049, 2560) for case in ("private", "hot")]


@pytest.mark.parametrize("what,n,case", EDGES, ids=["%s-%d%s" % (w, n, "-" + c if c else "") for w, n, c in EDGES])
def test_edges_of_scan_chunk_and_lane_step(ctx, what, n, case):
    """subjects: n one-row subjects -- the count kernel's 256-subject block, the weight kernel's four subjects a block, and the
    scan's elements per thread going from 1 to 2 (1024 -> 1025) and from 2 to 3 (2048 -> 2049) over the subjects' row counts.
    rows: one subject of n rows -- 2 n contributions around the radix kernels' 64-lane step and 2048-record chunk, and five
    chunks (1280 radix counts: the scan's elements per thread going from 1 to 2)."""
    from grim import _native as nat
    from grim.em import fold_records

    subs = _one_row_subjects(n) if what == "subjects" else [(nat.ST_OK, "b", None, em_subject(case, n, 3, 1), None)]
    res, rows = em_records(subs)
    want = fold_records(res, rows, N_ALLELES, N_POPS)
    assert want[4]["subjects_used"] == len(subs) and want[4]["contributions"] == 2 * len(rows)
    assert _run_records(ctx, res, rows)[0] == _want(want)


def _passes(first_capacity, n_pops, rehashes):
    """radix passes of a call, by the host's own formula: one bit more than cap * P - 1 needs, 8 bits a pass"""
    cap = 64
    while cap < first_capacity:
        cap *= 2
    cap <<= rehashes
    bits = 1
    while (1 << bits) < cap * n_pops:
        bits += 1
    return -(-(bits + 1) // 8)


def test_every_radix_pass_count(ctx):
    from grim import _native as nat
    from grim.em import fold_records

    small = [(nat.ST_OK, "a", None, em_subject(case, n, 1, i, 1), None)
             for i, (case, n) in enumerate((("shared", 2), ("private", 5), ("distinct", 1), ("hot", 8)))]  # 16 rows: no growth from 64
    seen = set()
    for first_capacity, n_pops, subs in ((64, 1, small),
                                         (1 << 10, 4, shape_subjects(1, 4, [1, 63, 64, 65, 129])),
                                         (1 << 16, 4, shape_subjects(1, 4, [1, 63, 64, 65, 129, 1000])),
                                         (1 << 18, 64, shape_subjects(1, 64, [1, 63, 64, 65, 129, 1000]))):
        res, rows = em_records(subs)
        want = fold_records(res, rows, N_ALLELES, n_pops)
        assert len(want[3]) > 0  # records without a group ride through every pass
        got, stats, _, _ = _run_records(ctx, res, rows, n_pops, first_capacity)
        assert got == _want(want), "first_capacity %d, %d populations" % (first_capacity, n_pops)
        if n_pops == 64:
            assert 63 in want[1].tolist()  # popmask bit 63
        seen.add(_passes(first_capacity, n_pops, stats["rehashes"]))
    assert seen == {1, 2, 3, 4}


def test_records_and_batches_share_one_accumulator():
    from grim import _native as nat
    from grim.blocks import Blocks
    from grim.em import fold_records

    gname, conf, lines, _, _, _ = harness.golden("pop4_em_mr")
    _, imp = _product(gname, conf, lines, "em_door")
    g = imp.netGraph
    n_alleles = [g.adict.count(s) for s in range(len(g.full_loci))]
    shared = Blocks(imp, imp.config, None, True, bool(conf.get("_em")), output_haplotypes=True)
    block = shared.block(lines)
    by_batch = nat.EmAccumulator(shared.ctx, n_alleles, len(POP4))
    by_records = nat.EmAccumulator(shared.ctx, n_alleles, len(POP4))
    try:
        by_batch.accumulate(block.batch)
        res, rows = block.records()
        by_records.accumulate_records(res, rows)
        got = _got(by_records)
        assert got == _got(by_batch)
        assert by_records.stats() == by_batch.stats() and by_records.last_unsupported() == by_batch.last_unsupported()
        assert got[5]["contributions"] > 0 and len(got[0]) > 100
        assert got == _want(fold_records(res, rows, n_alleles, len(POP4)))
    finally:
        by_batch.close()
        by_records.close()
        block.close()


def _em_empty(acc):
    return (acc.entries() == 0 and acc.spill_count() == 0 and acc.kernel_ms() == 0.0 and acc.last_unsupported() == 0
            and acc.stats() == {"subjects_used": 0, "skipped_plan_c": 0, "contributions": 0, "rehashes": 0}
            and len(acc.export()[0]) == 0)


def test_records_door_refusals_leave_the_accumulator_empty(ctx):
    from grim import _native as nat
    from grim.em import fold_records

    L = nat._em_lib()
    res, rows = em_records(shape_subjects(1, N_POPS, [1, 65]))
    acc = nat.EmAccumulator(ctx, N_ALLELES, N_POPS, 1 << 12)
    try:
        for args in ((None, len(res), nat._ptr(rows), len(rows)),      # no subjects given, some counted
                     (nat._ptr(res), len(res), None, len(rows)),       # no rows given, some counted
                     (nat._ptr(res), len(res), nat._ptr(rows), 1 << 31)):  # more rows than a position holds
            assert L.grim_em_accumulate_records(acc.h, *args) == -3
            assert "grim_em_accumulate_records" in ctx.error() and _em_empty(acc)
        # 2^26 slots of 64 populations are 2^32 counters: refused at creation, nothing allocated
        with pytest.raises(nat.NativeError) as refused:
            nat.EmAccumulator(ctx, N_ALLELES, 64, 1 << 26)
        assert "2^31" in str(refused.value)
        # the accumulator works after the refusals, and they did not count as batches
        acc.accumulate_records(res, rows)
        want = fold_records(res, rows, N_ALLELES, N_POPS, batch=0)
        assert len(want[3]) > 0 and _got(acc) == _want(want)
        assert L.grim_em_accumulate_records(acc.h, None, 1, None, 0) == -3
        assert _got(acc) == _want(want) and acc.kernel_ms() == 0.0  # a refusal adds nothing to what is there
    finally:
        acc.close()
