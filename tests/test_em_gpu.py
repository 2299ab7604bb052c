"""The device M-step (csrc/grim_em.h through grim/em.py) against the fold of the reference's golden .pmug files, against the
fold of the product's own text whatever the batch cuts, through table growth, private alleles, the mass property and an
end-to-end EM iteration."""
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
