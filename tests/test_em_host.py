"""The M-step's host side (grim/em.py): the text fold against an independent fold of the reference's golden .pmug files,
side order and the double add on a hand-made text, the frequency files through the package's own produce_hpf; the record twin against the text fold, on hand-made records and
against exact rational sums.  No GPU."""
import csv
import gzip
import json
import os

import pytest

import harness

EM_SCENARIOS = ["pop4_em_mr", "cau_em_mr", "pop4_planc_rerun_em"]


def _hex(counts):
    return {pop: {hap: float(c).hex() for hap, c in d.items()} for pop, d in counts.items()}


def _independent_fold(text):
    """the contract written out once more, on its own: explicit ((c + w)) in file order"""
    subjects = []
    for line in text.splitlines():
        sid, a, b, p, rank = line.split(",")
        if rank == "0":
            subjects.append([])
        assert int(rank) == len(subjects[-1]), "ranks are 0..n-1"
        subjects[-1].append((a.split(";"), b.split(";"), float(p)))
    table = {}
    for rows in subjects:
        if any(a[1] == "all_pops" or b[1] == "all_pops" for a, b, _ in rows):
            continue
        total = 0.0
        for _, _, p in rows:
            total = (total + p)
        ws = [p / total for _, _, p in rows]
        assert abs(sum(ws) - 1.0) <= len(rows) * 2.0 ** -52
        for (a, b, _), w in zip(rows, ws):
            for hap, pop in (a, b):
                c = table.get((pop, hap))
                table[(pop, hap)] = w if c is None else (c + w)
    out = {}
    for (pop, hap), c in table.items():
        out.setdefault(pop, {})[hap] = c
    return out


@pytest.mark.parametrize("scenario", EM_SCENARIOS)
def test_fold_equals_independent_fold_of_reference_files(scenario):
    from grim.em import fold_pmug_text

    text = open(os.path.join(harness.GOLD, scenario, "don.pmug")).read()
    counts, stats = fold_pmug_text(text)
    exp = _independent_fold(text)
    assert _hex(counts) == _hex(exp)
    assert stats["subjects_used"] > 0 and sum(len(d) for d in counts.values()) > 0
    assert stats["contributions"] == 2 * len(text.splitlines())  # no Plan-C subject in these files


def test_side_order_and_double_add():
    from grim.em import fold_pmug_text

    text = ("S0,H1;CAU,H1;CAU,0.5,0\n"      # homozygous, one population: adds twice
            "S0,H1;CAU,H2;AFA,0.25,1\n"     # split over two populations
            "S0,H2;AFA,H3;CAU,0.125,2\n"
            "S0,H3;AFA,H1;AFA,0.125,3\n"
            "S1,H2;CAU,H1;CAU,3.0,0\n")
    counts, stats = fold_pmug_text(text)
    assert counts == {
        "CAU": {"H1": 0.5 + 0.5 + 0.25 + 1.0, "H3": 0.125, "H2": 1.0},
        "AFA": {"H2": 0.25 + 0.125, "H3": 0.125, "H1": 0.125},
    }
    # side a before side b: S0 row 0 creates CAU/H1 before anything else, S1 creates CAU/H2 before it adds to CAU/H1
    assert list(counts["CAU"]) == ["H1", "H3", "H2"]
    assert list(counts["AFA"]) == ["H2", "H3", "H1"]
    assert stats == {"subjects_used": 2, "skipped_plan_c": 0, "contributions": 10}


def test_all_pops_rows_are_skipped_and_counted():
    from grim.em import fold_pmug_text

    text = ("S0,H1;CAU,H2;CAU,0.5,0\n"
            "S1,H1;all_pops,H2;all_pops,0.25,0\n"
            "S1,H3;all_pops,H2;all_pops,0.25,1\n"
            "S2,H2;CAU,H2;CAU,0.125,0\n")
    counts, stats = fold_pmug_text(text)
    assert counts == {"CAU": {"H1": 1.0, "H2": 3.0}}
    assert stats == {"subjects_used": 2, "skipped_plan_c": 1, "contributions": 4}


def test_freq_files_round_trip_through_produce_hpf(tmp_path, monkeypatch):
    from graph_generation.generate_hpf import produce_hpf
    from grim.em import fold_pmug_text, write_freq_files

    pops = harness.POPS["pop4"]
    counts, _ = fold_pmug_text(open(os.path.join(harness.GOLD, "pop4_em_mr", "don.pmug")).read())
    assert set(counts) <= set(pops)
    conf = json.load(open(os.path.join(harness.GOLD, "pop4_em_mr", "conf.json")))
    monkeypatch.chdir(tmp_path)
    with open("conf.json", "w") as fh:
        json.dump(conf, fh)
    totals = write_freq_files(counts, conf["freq_data_dir"], pops)
    expect = {}
    for pop in pops:
        rows = sorted(counts.get(pop, {}).items())
        t = 0.0
        for _, c in rows:
            t = t + c
        assert totals[pop] == t
        with gzip.open(os.path.join(conf["freq_data_dir"], pop + ".freqs.gz"), "rt") as zf:
            got = [l.rstrip("\n").split(",") for l in zf]
        assert got[0] == ["Haplo", "Count", "Freq"]
        assert [r[0] for r in got[1:]] == [h for h, _ in rows]
        for (hap, c), r in zip(rows, got[1:]):
            assert float(r[1]).hex() == c.hex() and float(r[2]).hex() == (c / t).hex()
            expect[(hap, pop)] = c / t
    produce_hpf("conf.json", quiet=True)
    with open(conf["freq_file"], newline="") as fh:
        rd = list(csv.reader(fh))
    assert rd[0] == ["hap", "pop", "freq"]
    seen = {(r[0], r[1]): float(r[2]) for r in rd[1:]}
    assert {k: v.hex() for k, v in seen.items()} == {k: v.hex() for k, v in expect.items() if v != 0.0}
    ratios = [float(l.split(",")[2]) for l in open(conf["pops_count_file"])]
    assert len(ratios) == len(pops)
    assert abs(sum(ratios) - 1.0) <= len(pops) * 2.0 ** -52


# ---- the record twin (grim.em.fold_records) -------------------------------------------------------------------------------
SLOT = {"A": 0, "B": 1, "C": 2, "DQB1": 3, "DRB1": 4}
PLAN_C_TAIL = ("X1,A*01:01~B*08:01;all_pops,A*02:01~B*07:02;all_pops,0.5,0\n"
               "X1,A*01:01~B*08:01;all_pops,A*03:01~B*07:02;all_pops,0.25,1\n"
               "X2,A*01:01~B*08:01;CAU,A*02:01~B*07:02;CAU,0.5,0\n")


def _pmug_records(text):
    """.pmug text -> (res, rows, key -> haplotype name, populations, n_alleles): allele ids from a small table per locus slot,
    populations by index in first-seen order; bit 60 set on some keys; a subject with `all_pops` rows gets plan c"""
    import numpy as np

    from grim import _native as nat

    ids = [dict() for _ in SLOT]
    names, pops = {}, []
    res, rows = [], []

    def key_of(hap):
        key = 0
        for allele in hap.split("~"):
            s = SLOT[allele.split("*", 1)[0]]
            key |= ids[s].setdefault(allele, len(ids[s]) + 1) << (nat.ABITS * s)
        assert names.setdefault(key, hap) == hap
        return key

    def pop_of(pop):
        if pop == "all_pops":
            return 0
        if pop not in pops:
            pops.append(pop)
        return pops.index(pop)

    for line in text.splitlines():
        sid, a, b, p, rank = line.split(",")
        if rank == "0":
            res.append([len(rows), 0, ord("ab"[len(res) % 2])])
        res[-1][1] += 1
        (ha, pa), (hb, pb) = a.rsplit(";", 1), b.rsplit(";", 1)
        if "all_pops" in (pa, pb):
            res[-1][2] = ord("c")
        k = len(rows)
        rows.append((key_of(ha) | (k % 3 == 0) << 60, key_of(hb) | (k % 2) << 60, float(p), pop_of(pa), pop_of(pb)))
    r = np.zeros(len(res), dtype=nat.RESULT_DT)
    for i, (off, n, plan) in enumerate(res):
        r[i]["row_off"][nat.T_PMUG], r[i]["n_rows"][nat.T_PMUG], r[i]["n_pairs"], r[i]["plan"] = off, n, n, plan
    return r, np.array(rows, dtype=nat.ROW_DT), names, pops, [len(d) for d in ids]


def _named(keys, kpops, counts, names, pops):
    out = {}
    for key, p, c in zip(keys.tolist(), kpops.tolist(), counts.tolist()):
        assert names[key] not in out.setdefault(pops[p], {})
        out[pops[p]][names[key]] = c
    return out


@pytest.mark.parametrize("tail", ["", PLAN_C_TAIL], ids=["golden", "golden_and_plan_c"])
@pytest.mark.parametrize("scenario", EM_SCENARIOS)
def test_record_twin_equals_text_fold_of_reference_files(scenario, tail):
    from grim.em import fold_pmug_text, fold_records

    text = open(os.path.join(harness.GOLD, scenario, "don.pmug")).read() + tail
    want, wstats = fold_pmug_text(text)
    res, rows, names, pops, n_alleles = _pmug_records(text)
    assert (rows["a"] >> 60).any() and (rows["b"] >> 60).any()
    keys, kpops, counts, spill, stats = fold_records(res, rows, n_alleles, len(pops))
    assert len(spill) == 0 and stats.pop("unsupported") == 0
    assert _hex(_named(keys, kpops, counts, names, pops)) == _hex(want)
    assert stats == wstats
    assert stats["skipped_plan_c"] == (1 if tail else 0)
    # not vacuous: many counters, and some that add up several contributions
    assert len(keys) >= 100
    per_counter = {}
    for r in rows[:len(rows) - (3 if tail else 0)]:
        for side, pop in (("a", "popa"), ("b", "popb")):
            at = (int(r[side]) & ((1 << 60) - 1), int(r[pop]))
            per_counter[at] = per_counter.get(at, 0) + 1
    assert max(per_counter.values()) >= 2


def _recs(subjects, rows):
    """[(status, plan, plan_phased, row_off, n_rows)], [(a, b, p, popa, popb)] -> record arrays"""
    import numpy as np

    from grim import _native as nat

    res = np.zeros(len(subjects), dtype=nat.RESULT_DT)
    for i, (status, plan, phased, off, n) in enumerate(subjects):
        res[i]["status"], res[i]["plan"], res[i]["plan_phased"] = status, ord(plan), ord(phased) if phased else 0
        res[i]["row_off"][nat.T_PMUG], res[i]["n_rows"][nat.T_PMUG] = off, n
    return res, np.array(rows, dtype=nat.ROW_DT).reshape(-1)


def _entries(out):
    keys, kpops, counts = out[:3]
    return list(zip(keys.tolist(), kpops.tolist(), counts.tolist()))


def test_record_twin_side_order_double_add_and_graph_order_bit():
    from grim import _native as nat
    from grim.em import fold_records

    H1, H2, H3, G = 1, 2, 3, 1 << 60
    rows = [(H1, H1 | G, 0.5, 0, 0),     # homozygous, one population, two spellings: adds twice to one counter
            (H1 | G, H2, 0.25, 0, 1),
            (H2, H3, 0.125, 1, 0),
            (H3, H1, 0.125, 1, 1),
            (H2, H1 | G, 3.0, 0, 0)]
    res, rows = _recs([(nat.ST_OK, "a", None, 0, 4), (nat.ST_OK, "b", None, 4, 1)], rows)
    out = fold_records(res, rows, [3], 2)
    assert _entries(out) == [(H1, 0, 0.5 + 0.5 + 0.25 + 1.0), (H1, 1, 0.125), (H2, 0, 1.0), (H2, 1, 0.25 + 0.125), (H3, 0, 0.125),
                             (H3, 1, 0.125)]
    assert len(out[3]) == 0
    assert out[4] == {"subjects_used": 2, "skipped_plan_c": 0, "contributions": 10, "unsupported": 0}
    # the total is the left-to-right sum, the weight one division
    res, rows = _recs([(nat.ST_OK, "a", None, 0, 3)], [(H1, H2, 0.3, 0, 0), (H1, H2, 0.2, 0, 0), (H3, H3, 0.1, 0, 0)])
    total = (0.3 + 0.2) + 0.1
    assert total != 0.3 + (0.2 + 0.1)
    assert _entries(fold_records(res, rows, [3], 1)) == [(H1, 0, 0.3 / total + 0.2 / total), (H2, 0, 0.3 / total + 0.2 / total),
                                                         (H3, 0, 0.1 / total + 0.1 / total)]


def test_record_twin_skip_rule():
    from grim import _native as nat
    from grim.em import fold_records

    rows = [(k + 1, k + 1, 1.0, 0, 0) for k in range(8)]  # row k names haplotype k + 1 alone
    subjects = [
        (nat.ST_OK, "c", "a", 0, 1),           # plan_phased overrides plan: used
        (nat.ST_OK, "a", "c", 1, 1),           # ... both ways: skipped, counted
        (nat.ST_OK, "c", None, 2, 1),          # plan c: skipped, counted
        (nat.ST_OK, "c", None, 3, 0),          # plan c with zero rows: skipped, NOT counted as plan c
        (nat.ST_MISS, "a", None, 3, 1),        # a MISS subject with rows
        (nat.ST_UNSUPPORTED, "a", None, 4, 1),
        (nat.ST_NOPHASE, "a", None, 4, 1),
        (nat.ST_OK, "a", None, 7, 2),          # offsets past the rows
        (nat.ST_OK, "b", None, 9, 1),
        (nat.ST_OK, "b", None, 8, 0),          # no rows, offset at the end
        (nat.ST_OK, "b", None, 7, 1),          # the last row: used
    ]
    res, rows = _recs(subjects, rows)
    out = fold_records(res, rows, [8], 1)
    assert _entries(out) == [(1, 0, 2.0), (8, 0, 2.0)]
    assert out[4] == {"subjects_used": 2, "skipped_plan_c": 2, "contributions": 4, "unsupported": 1}
    # a plan-c subject whose rows lie outside is still counted as skipped-plan-c (the count kernel looks at the plan alone)
    res2, _ = _recs([(nat.ST_OK, "c", None, 100, 3)], [])
    assert fold_records(res2, rows, [8], 1)[4]["skipped_plan_c"] == 1
    with pytest.raises(ValueError):
        fold_records(*_recs([(nat.ST_OK, "a", None, 0, 2)], [(1, 1, 0.0, 0, 0), (1, 1, 0.0, 0, 0)]), [8], 1)
    with pytest.raises(ValueError):
        fold_records(*_recs([(nat.ST_OK, "a", None, 0, 1)], [(1, 1, float("nan"), 0, 0)]), [8], 1)
    with pytest.raises(ValueError):  # regions that overlap: more rows than there are
        fold_records(*_recs([(nat.ST_OK, "a", None, 0, 2), (nat.ST_OK, "a", None, 0, 2)], rows[:3]), [8], 1)


def test_record_twin_private_boundary_and_spill_fields():
    from grim import _native as nat
    from grim.em import fold_records

    n_alleles = [7, 5, 0, 0, 9]
    at = 7 | 5 << 12 | 9 << 48              # every field AT n_alleles: the last dictionary allele of its slot
    over0, over1, over4 = 8 | 5 << 12, 7 | 6 << 12, 7 | 10 << 48   # one field at n_alleles + 1: private
    untyped_slot_typed = 1 | 1 << 24        # slot 2 has no allele at all: any field there is private
    G = 1 << 60
    rows = [(at | G, over0, 0.5, 1, 0),
            (over1 | G, at, 0.25, 1, 1),
            (at, over4, 0.25, 2, 70000),     # pop == n_pops on side a; a population beyond 16 bits on side b
            (untyped_slot_typed, 1, 1.0, 0, 0)]
    res, rows = _recs([(nat.ST_OK, "a", None, 0, 3), (nat.ST_OK, "a", None, 3, 1)], rows)
    keys, kpops, counts, spill, stats = fold_records(res, rows, n_alleles, 2, batch=5)
    assert list(zip(keys.tolist(), kpops.tolist(), counts.tolist())) == [(1, 0, 1.0), (at, 1, 0.5 + 0.25)]
    assert spill.dtype == nat.SPILL_DT
    assert [tuple(x) for x in spill.tolist()] == [
        (over0, 0.5, 5, 0, 0, 0, 1), (over1, 0.25, 5, 0, 1, 1, 0), (at, 0.25, 5, 0, 2, 2, 0), (over4, 0.25, 5, 0, 2, 70000 & 0xFFFF, 1),
        (untyped_slot_typed, 1.0, 5, 1, 0, 0, 0)]
    assert stats == {"subjects_used": 2, "skipped_plan_c": 0, "contributions": 8, "unsupported": 0}


def test_record_twin_cuts_with_a_carried_dictionary():
    from grim.em import fold_records

    text = open(os.path.join(harness.GOLD, "pop4_em_mr", "don.pmug")).read()
    res, rows, _, pops, n_alleles = _pmug_records(text)
    n_alleles[4] -= 2  # some private haplotypes
    whole = fold_records(res, rows, n_alleles, len(pops) - 1)
    assert len(whole[3]) > 0
    for step in (1, 7):
        carry, spill, stats = {}, [], dict.fromkeys(whole[4], 0)
        for call, lo in enumerate(range(0, len(res), step)):
            part = res[lo:lo + step].copy()
            base = int(part["row_off"][0, 2])
            end = int(part["row_off"][-1, 2] + part["n_rows"][-1, 2])
            part["row_off"][:, 2] -= base
            out = fold_records(part, rows[base:end], n_alleles, len(pops) - 1, batch=call, carry=carry)
            assert (out[3]["batch"] == call).all() and (out[3]["subject"] < step).all()
            spill += [(x["key"], x["w"], lo + x["subject"], x["row"], x["pop"], x["side"]) for x in out[3]]
            for k in stats:
                stats[k] += out[4][k]
        assert [float(c).hex() for c in out[2]] == [float(c).hex() for c in whole[2]]
        assert out[0].tolist() == whole[0].tolist() and out[1].tolist() == whole[1].tolist()
        assert spill == [(x["key"], x["w"], x["subject"], x["row"], x["pop"], x["side"]) for x in whole[3]]
        assert stats == whole[4]


def test_record_twin_is_close_to_the_exact_sums():
    """Every counter of the twin against the exact rational sum of its contributions.  Recursive summation of m positive
    terms has a relative error of at most (m - 1) u (1 + O(mu)); each term p_k / total carries the error of an R-term total,
    (R - 1) u, and of one division, u; u = 2^-53.  So |count - exact| <= 1.01 (m + R + 1) u exact, m the counter's number
    of contributions and R the largest row count of a subject that contributes to it."""
    from fractions import Fraction

    import test_em_gpu as shapes

    from grim.em import fold_records

    res, rows = shapes.em_records(shapes.shape_subjects(rounds=3))
    keys, kpops, counts, spill, stats = fold_records(res, rows, shapes.N_ALLELES, shapes.N_POPS)
    exact, m, R = {}, {}, {}
    used = 0
    for s in shapes.used_subjects(res, len(rows)):
        off, n = int(res[s]["row_off"][2]), int(res[s]["n_rows"][2])
        sub = rows[off:off + n]
        probs = [Fraction(p) for p in sub["prob"].tolist()]
        total = sum(probs)
        used += 1
        for k, r in enumerate(sub.tolist()):
            for key, pop in ((r[0], r[3]), (r[1], r[4])):
                at = (key & ((1 << 60) - 1), pop)
                exact[at] = exact.get(at, 0) + probs[k] / total
                m[at] = m.get(at, 0) + 1
                R[at] = max(R.get(at, 0), n)
    assert used == stats["subjects_used"] and len(keys) > 1000
    worst = Fraction(0)
    for key, pop, c in zip(keys.tolist(), kpops.tolist(), counts.tolist()):
        at = (key, pop)
        err = abs(Fraction(c) - exact[at]) / exact[at]
        worst = max(worst, err / Fraction(2) ** -53)
        assert err <= Fraction(101, 100) * (m[at] + R[at] + 1) * Fraction(2) ** -53, (at, m[at], R[at], float(err))
    assert max(m[(k, p)] for k, p in zip(keys.tolist(), kpops.tolist())) > 5000
    print("worst counter: %.1f units of 2^-53 relative" % float(worst))
