"""The M-step's host side (grim/em.py): the text fold against an independent fold of the reference's golden .pmug files,
side order and the double add on a hand-made text, the frequency files through the package's own produce_hpf.  No GPU."""
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
