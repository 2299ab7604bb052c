"""The marginal genotype tables' host side (grim/marginal.py): the text twin on hand-written rows, on the golden .umug files
with every locus kept, against the record twin, and the argument checks.  No GPU."""
import os

import numpy as np
import pytest

import harness

SLOT = {"A": 0, "B": 1, "C": 2, "DQB1": 3, "DRB1": 4}
ALL5 = list(SLOT)
UMUG_SCENARIOS = [s for s in harness.scenarios() if os.path.exists(os.path.join(harness.GOLD, s, "don.umug"))
                  and os.path.getsize(os.path.join(harness.GOLD, s, "don.umug")) > 0]


def _umug(scenario):
    return open(os.path.join(harness.GOLD, scenario, "don.umug")).read()


def test_two_rows_merge():
    from grim.marginal import reduce_umug_text

    text = ("S,A*01:01+A*02:01^B*07:02+B*08:01^DRB1*03:01+DRB1*15:01,0.5,0\n"
            "S,A*01:01+A*02:01^B*07:02+B*08:01^DRB1*03:01+DRB1*15:02,0.25,1\n")
    assert reduce_umug_text(text, ["A", "B"]) == "S,A*01:01+A*02:01^B*07:02+B*08:01,0.75,0\n"
    assert reduce_umug_text(text, ["DRB1"]) == "S,DRB1*03:01+DRB1*15:01,0.5,0\nS,DRB1*03:01+DRB1*15:02,0.25,1\n"
    assert reduce_umug_text(text, "A") == "S,A*01:01+A*02:01,0.75,0\n"


def test_merge_overtakes_the_former_first_row():
    from grim.marginal import reduce_umug_text

    text = ("S,A*01:01+A*02:01^B*07:02+B*08:01,0.4,0\n"
            "S,A*01:01+A*03:01^B*07:02+B*08:01,0.3,1\n"
            "S,A*01:01+A*03:01^B*07:02+B*44:02,0.2,2\n")
    assert reduce_umug_text(text, ["A"]) == "S,A*01:01+A*03:01,0.5,0\nS,A*01:01+A*02:01,0.4,1\n"
    # the sum is the left-to-right sum in rank order
    three = text + "S,A*01:01+A*03:01^B*07:02+B*51:01,0.1,3\n"
    assert reduce_umug_text(three, ["A"]).splitlines()[0] == "S,A*01:01+A*03:01,%r,0" % ((0.3 + 0.2) + 0.1)
    assert (0.3 + 0.2) + 0.1 != 0.3 + (0.2 + 0.1)


def test_exact_tie_keeps_first_seen_order():
    from grim.marginal import reduce_umug_text

    text = ("S,A*01:01+A*02:01^B*07:02+B*08:01,0.25,0\n"
            "S,A*01:01+A*03:01^B*07:02+B*08:01,0.125,1\n"
            "S,A*01:01+A*11:01^B*07:02+B*08:01,0.125,2\n"
            "S,A*01:01+A*11:01^B*07:02+B*44:02,0.125,3\n"
            "S,A*01:01+A*03:01^B*07:02+B*44:02,0.125,4\n")
    assert reduce_umug_text(text, ["A"]) == ("S,A*01:01+A*02:01,0.25,0\n"
                                             "S,A*01:01+A*03:01,0.25,1\n"
                                             "S,A*01:01+A*11:01,0.25,2\n")


def test_max_rows_cuts_the_groups():
    from grim.marginal import reduce_umug_text

    text = "".join("S,A*01:01+A*%02d:01^B*07:02+B*08:01,%r,%d\n" % (k + 2, 0.5 / (k + 1), k) for k in range(6))
    full = reduce_umug_text(text, ["A"])
    assert len(full.splitlines()) == 6
    assert reduce_umug_text(text, ["A"], max_rows=4) == "".join(full.splitlines(keepends=True)[:4])
    assert reduce_umug_text(text, ["A"], max_rows=100) == full
    assert reduce_umug_text(text, ["B"], max_rows=1).count("\n") == 1


def test_kept_locus_that_is_untyped():
    from grim.marginal import reduce_umug_text

    text = ("S,A*01:01+A*02:01^B*07:02+B*08:01,0.5,0\n"
            "S,A*01:01+A*02:01^B*07:02+B*44:02,0.25,1\n"
            "T,A*01:01+A*02:01^DRB1*03:01+DRB1*15:01,0.5,0\n")
    # C is typed nowhere: every row of a subject falls into one group with an empty genotype
    assert reduce_umug_text(text, ["C"]) == "S,,0.75,0\nT,,0.5,0\n"
    assert reduce_umug_text(text, ["B", "C"]) == "S,B*07:02+B*08:01,0.5,0\nS,B*07:02+B*44:02,0.25,1\nT,,0.5,0\n"


def test_consecutive_subjects_with_one_id_stay_separate():
    from grim.marginal import reduce_umug_text

    text = ("S,A*01:01+A*02:01^B*07:02+B*08:01,0.5,0\n"
            "S,A*01:01+A*02:01^B*07:02+B*44:02,0.25,1\n"
            "S,A*01:01+A*02:01^B*07:02+B*08:01,0.125,0\n")
    assert reduce_umug_text(text, ["A"]) == "S,A*01:01+A*02:01,0.75,0\nS,A*01:01+A*02:01,0.125,0\n"


@pytest.mark.parametrize("scenario", UMUG_SCENARIOS)
def test_all_five_loci_return_the_golden_text(scenario):
    from grim.marginal import reduce_umug_text

    text = _umug(scenario)
    assert reduce_umug_text(text, ALL5) == text


def _records(text):
    """.umug text -> (res, rows, names): ids from a small table, slot by locus name; in every second row the alleles of its
    first locus change haplotypes, as they may between the rows of a batch"""
    from grim import _native as nat

    ids = [dict() for _ in SLOT]
    names = [dict() for _ in SLOT]
    res, rows = [], []
    for line in text.splitlines():
        sid, geno, p, rank = line.split(",")
        if rank == "0":
            res.append([len(rows), 0])
        res[-1][1] += 1
        a = b = 0
        for z, part in enumerate(geno.split("^")):
            s = SLOT[part.split("*", 1)[0]]
            x, y = (ids[s].setdefault(name, len(ids[s]) + 1) for name in part.split("+"))
            names[s][x], names[s][y] = part.split("+")
            if z == 0 and len(rows) % 2:
                x, y = y, x
            a |= x << (nat.ABITS * s)
            b |= y << (nat.ABITS * s)
        rows.append((a | (len(rows) % 3 == 0) << 60, b, float(p), 7, 9))
    r = np.zeros(len(res), dtype=nat.RESULT_DT)
    for i, (off, n) in enumerate(res):
        r[i]["row_off"][nat.T_UMUG], r[i]["n_rows"][nat.T_UMUG], r[i]["n_genotypes"], r[i]["plan"] = off, n, n, ord("a")
    return r, np.array(rows, dtype=nat.ROW_DT), names


def _print(sids, res, rows, names):
    from grim import _native as nat

    out = []
    for sid, r in zip(sids, res):
        for k in range(int(r["n_rows"][nat.T_UMUG])):
            row = rows[int(r["row_off"][nat.T_UMUG]) + k]
            parts = []
            for s in range(len(SLOT)):
                x, y = ((int(row[side]) >> (nat.ABITS * s)) & 0xFFF for side in ("a", "b"))
                if x and y:
                    parts.append("+".join(sorted((names[s][x], names[s][y]))))
            out.append("%s,%s,%r,%d\n" % (sid, "^".join(parts), float(row["prob"]), k))
    return "".join(out)


@pytest.mark.parametrize("keep", [["A", "B", "DRB1"], ["DRB1"], ALL5])
def test_record_twin_agrees_with_text_twin(keep):
    from grim import _native as nat
    from grim.marginal import keep_mask, reduce_records, reduce_umug_text

    text = _umug("cau_mixed")
    res, rows, names = _records(text)
    sids = [l.split(",")[0] for l in text.splitlines() if l.endswith(",0")]
    assert len(sids) == len(res)
    assert _print(sids, res, rows, names) == text
    for max_rows in (3, 10):
        ores, orows, stats = reduce_records(res, rows, keep_mask(SLOT, keep), max_rows)
        want = reduce_umug_text(text, keep, max_rows)
        assert _print(sids, ores, orows, names) == want
        assert stats["rows_in"] == len(rows) and stats["subjects"] == len(res) and stats["undefined"] == 0
        assert stats["rows_out"] == len(want.splitlines())
        assert stats["groups"] == len(reduce_umug_text(text, keep).splitlines())
        assert not orows["popa"].any() and not orows["popb"].any() and not ((orows["a"] | orows["b"]) >> np.uint64(60)).any()
        assert (ores["plan"] == ord("a")).all() and (ores["n_rows"][:, 1:] == 0).all()
    if len(keep) < 5:
        assert want != text


def test_record_twin_skips_what_is_not_ok_or_out_of_range():
    from grim import _native as nat
    from grim.marginal import reduce_records

    rows = np.zeros(4, dtype=nat.ROW_DT)
    rows["a"], rows["b"], rows["prob"] = [1, 2, 1, 1], [1, 1, 2, 1], [0.5, 0.25, 0.125, 1.0]
    res = np.zeros(5, dtype=nat.RESULT_DT)
    res["status"] = [nat.ST_OK, nat.ST_MISS, nat.ST_OK, nat.ST_OK, nat.ST_OK]
    res["row_off"][:, 0] = [0, 0, 3, 3, 5]
    res["n_rows"][:, 0] = [3, 3, 0, 2, 1]  # a MISS subject, one without rows, two that point past the rows
    ores, orows, stats = reduce_records(res, rows, 1, 10)
    assert list(ores["n_rows"][:, 0]) == [2, 0, 0, 0, 0] and list(ores["n_genotypes"]) == [2, 0, 0, 0, 0]
    assert list(ores["status"]) == list(res["status"])
    assert [(int(r["a"]), int(r["b"]), float(r["prob"])) for r in orows[:2]] == [(1, 1, 0.5), (2, 1, 0.375)]
    assert stats == {"subjects": 1, "rows_in": 3, "groups": 2, "rows_out": 2, "undefined": 0}
    # a haplotype typed where the other is not
    rows["b"][0] = 1 << nat.ABITS
    assert reduce_records(res, rows, 1, 10)[2]["undefined"] == 1


def test_keep_loci_must_be_known_and_not_empty():
    from grim.marginal import keep_mask, reduce_records, reduce_umug_text

    assert keep_mask(SLOT, ["A", "B", "DRB1"]) == 0b10011 and keep_mask(SLOT, "C") == 0b100
    with pytest.raises(ValueError):
        keep_mask(SLOT, [])
    with pytest.raises(ValueError):
        keep_mask(SLOT, ["A", "DPB1"])
    with pytest.raises(ValueError):
        reduce_umug_text("S,A*01:01+A*02:01,0.5,0\n", [])
    with pytest.raises(ValueError):
        reduce_umug_text("S,A*01:01+A*02:01,0.5,0\n", ["DPB1"], loci=ALL5)
    with pytest.raises(ValueError):
        reduce_records([], [], 0, 10)
