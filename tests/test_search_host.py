"""The donor search's CPU twins (grim/search.py): the order and the threshold on hand-written records, the independence of
the answer from how the donors are cut into runs, and the text twin against a sort written out here.  No GPU."""
import os

import numpy as np
import pytest

import harness

ABITS = 12
N_ALLELES = [4000] * 5  # dictionary sizes: an id above is private
MASK = 0b00011
NO_DONOR = 0xFFFFFFFF

G = ([5, 6, 7, 8, 9], [15, 16, 17, 18, 19])    # the patient's genotype
G1 = ([5, 6, 7, 8, 9], [15, 99, 17, 18, 19])   # one mismatch at slot 1
G2 = ([5, 98, 7, 8, 9], [15, 99, 17, 18, 19])  # two mismatches at slot 1
PRIV = ([5, 6, 7, 8, 9], [4001, 16, 17, 18, 19])


def _key(fields):
    k = 0
    for s, f in enumerate(fields):
        k |= int(f) << (ABITS * s)
    return k


def _side(subjects, status=None):
    """[[((a fields, b fields), p)]] -> (res, rows) records, rows back to back"""
    from grim import _native as nat

    res = np.zeros(len(subjects), dtype=nat.RESULT_DT)
    flat = []
    for i, rows in enumerate(subjects):
        res[i]["status"] = nat.ST_OK if status is None else status[i]
        res[i]["row_off"][nat.T_UMUG], res[i]["n_rows"][nat.T_UMUG] = len(flat), len(rows)
        flat += [(_key(a), _key(b), p, 0, 0) for (a, b), p in rows]
    return res, np.array(flat, dtype=nat.ROW_DT) if flat else np.zeros(0, dtype=nat.ROW_DT)


# mm0 / mm1 of the donors against the one-row patient G, over slots 0 and 1:
FULL = [(G, 1.0)]                  # 1.0 / 0.0
HALF_ONE = [(G, 0.5), (G1, 0.5)]   # 0.5 / 0.5
HALF_TWO = [(G, 0.5), (G2, 0.5)]   # 0.5 / 0.0
QUARTER = [(G, 0.25), (G2, 0.75)]  # 0.25 / 0.0


def _search(donors, ids, top_n, min_p0=0.0, patients=None, dstatus=None, pstatus=None):
    from grim.search import search_records

    pres, prows = _side(patients or [[(G, 1.0)]], pstatus)
    dres, drows = _side(donors, dstatus)
    return search_records(pres, prows, [(dres, drows, ids)], MASK, N_ALLELES, top_n, min_p0)


def _mm(hit):
    return [float(hit["rec"]["mm"][0]), float(hit["rec"]["mm"][1])]


# ---- 1. the order ---------------------------------------------------------------------------------------------------------
def test_equal_mm0_is_separated_by_mm1():
    hits, n, stats = _search([HALF_TWO, QUARTER, HALF_ONE, FULL], [1, 2, 3, 4], 4)
    assert list(n) == [4] and stats["candidates"] == 4 and stats["pairs"] == 4
    assert [int(h["donor"]) for h in hits[0]] == [4, 3, 1, 2]  # id 3 before id 1: its mm1 is larger
    assert [_mm(h) for h in hits[0]] == [[1.0, 0.0], [0.5, 0.5], [0.5, 0.0], [0.25, 0.0]]
    assert not hits["reserved"].any()


def test_equal_mm0_and_mm1_are_separated_by_id_whatever_the_order_given():
    hits, n, _ = _search([HALF_ONE, HALF_ONE, FULL, HALF_ONE, HALF_ONE], [40, 30, 20, 20 - 1, 7], 3)
    assert list(n) == [3] and [int(h["donor"]) for h in hits[0]] == [20, 7, 19]
    hits, n, _ = _search([HALF_ONE] * 4, [9, 9 - 1, 5, 0], 4)
    assert [int(h["donor"]) for h in hits[0]] == [0, 5, 8, 9]


def test_the_threshold_is_inclusive():
    donors, ids = [HALF_TWO, QUARTER, HALF_ONE, FULL], [1, 2, 3, 4]
    hits, n, stats = _search(donors, ids, 4, min_p0=0.5)
    assert list(n) == [3] and stats["candidates"] == 3 and stats["pairs"] == 4
    assert [int(h["donor"]) for h in hits[0]] == [4, 3, 1, NO_DONOR]
    hits, n, stats = _search(donors, ids, 4, min_p0=float(np.nextafter(0.5, 1.0)))
    assert list(n) == [1] and stats["candidates"] == 1 and int(hits[0, 0]["donor"]) == 4


def test_a_threshold_above_everything_gives_no_hits():
    hits, n, stats = _search([HALF_TWO, FULL], [1, 2], 2, min_p0=2.0)
    assert list(n) == [0] and stats["candidates"] == 0 and stats["pairs"] == 2
    assert list(hits[0]["donor"]) == [NO_DONOR] * 2 and not np.frombuffer(hits["rec"].tobytes(), dtype=np.uint8).any()


def test_fewer_candidates_than_top_n_leave_empty_slots():
    hits, n, _ = _search([HALF_ONE, FULL], [8, 3], 5)
    assert list(n) == [2] and list(hits[0]["donor"]) == [3, 8] + [NO_DONOR] * 3
    tail = hits[0, 2:]
    assert not np.frombuffer(tail["rec"].tobytes(), dtype=np.uint8).any() and not tail["reserved"].any()
    assert hits.dtype.itemsize == 136 and hits.shape == (1, 5)


def test_a_private_or_invalid_donor_is_never_a_hit():
    from grim import _native as nat

    donors = [FULL, [(PRIV, 1.0)], FULL, [], FULL, [(G, 0.0)]]
    status = [nat.ST_OK, nat.ST_OK, nat.ST_MISS, nat.ST_OK, nat.ST_OK, nat.ST_OK]
    hits, n, stats = _search(donors, [10, 11, 12, 13, 14, 15], 6, dstatus=status)
    assert list(n) == [2] and list(hits[0]["donor"][:2]) == [10, 14]
    assert stats["donors_private"] == 1 and stats["donors_valid"] == 3 and stats["pairs"] == 2 and stats["candidates"] == 2
    # a record of zeros passes a threshold of 0.0 by its bytes: it is the flags that decide
    hits, n, _ = _search(donors, [10, 11, 12, 13, 14, 15], 6, min_p0=-1.0, dstatus=status)
    assert list(n) == [2]


def test_an_invalid_or_private_patient_gets_no_hits():
    from grim import _native as nat

    patients = [[(G, 1.0)], [(G, 1.0)], [(PRIV, 1.0)], [(G1, 0.5), (G, 1.5)]]
    hits, n, stats = _search([FULL, HALF_ONE], [1, 0], 2, patients=patients, pstatus=[nat.ST_MISS, nat.ST_OK, nat.ST_OK, nat.ST_OK])
    assert list(n) == [0, 2, 0, 2] and stats["candidates"] == 4
    assert list(hits[0]["donor"]) == [NO_DONOR] * 2 and list(hits[2]["donor"]) == [NO_DONOR] * 2
    assert list(hits[1]["donor"]) == [1, 0] and list(hits[3]["donor"]) == [1, 0]
    assert _mm(hits[3, 0]) == [0.75, 0.25]


def test_arguments_are_checked():
    from grim.search import search_records, search_umug_text

    pres, prows = _side([[(G, 1.0)]])
    for top_n, min_p0 in ((0, 0.0), (257, 0.0), (1, float("nan"))):
        with pytest.raises(ValueError):
            search_records(pres, prows, [], MASK, N_ALLELES, top_n, min_p0)
        with pytest.raises(ValueError):
            search_umug_text("", "", ["A"], top_n, min_p0)
    with pytest.raises(ValueError):
        search_records(pres, prows, [(pres, prows, [1, 2])], MASK, N_ALLELES, 1, 0.0)
    hits, n, stats = search_records(pres, prows, [], MASK, N_ALLELES, 256, 0.0)
    assert hits.shape == (1, 256) and list(n) == [0] and not any(stats.values())


# ---- 2. runs ----------------------------------------------------------------------------------------------------------------
def test_the_cut_into_runs_and_their_order_do_not_show():
    from grim.search import search_records

    pool = [FULL, HALF_ONE, HALF_TWO, QUARTER, [(G1, 1.0)], [(PRIV, 1.0)], [(G2, 0.125), (G, 0.125), (G1, 0.25)]]
    donors = [pool[(i * 5) % 7] for i in range(23)]
    ids = [(i * 37) % 101 + 1000 for i in range(23)]  # distinct, not the positions
    assert len(set(ids)) == 23
    pres, prows = _side([[(G, 1.0)], [(G1, 0.25), (G, 0.75)], []])

    def runs(cuts):
        return [_side(donors[a:b]) + (ids[a:b],) for a, b in cuts]

    for top_n in (4, 30):
        whole = search_records(pres, prows, runs([(0, 23)]), MASK, N_ALLELES, top_n, 0.2)
        assert whole[1][0] > 3 and whole[1][1] > 3 and whole[1][2] == 0
        assert (top_n == 4) == (whole[2]["candidates"] > int(whole[1].sum()))  # 4 cuts the lists, 30 does not
        cut = search_records(pres, prows, runs([(0, 1), (1, 6), (6, 23)]), MASK, N_ALLELES, top_n, 0.2)
        back = search_records(pres, prows, runs([(6, 23), (1, 6), (0, 1)]), MASK, N_ALLELES, top_n, 0.2)
        for other in (cut, back):
            assert other[0].tobytes() == whole[0].tobytes() and list(other[1]) == list(whole[1])
            for k in ("candidates", "pairs", "row_pairs", "donors_valid", "donors_private"):
                assert other[2][k] == whole[2][k]


# ---- 3. the text twin against a sort written out here -----------------------------------------------------------------------
def _first_subjects(text, n):
    out, seen = [], 0
    for line in text.splitlines(keepends=True):
        seen += line.rstrip("\n").endswith(",0")
        if seen > n:
            break
        out.append(line)
    return "".join(out)


@pytest.mark.parametrize("scenario", ["pop4_mixed", "cau_edge", "pop4_planc"])
def test_text_twin_equals_a_sort_of_the_match_twin(scenario):
    from grim.match import match_umug_text
    from grim.search import search_umug_text

    text = open(os.path.join(harness.GOLD, scenario, "don.umug")).read()
    ptext = _first_subjects(text, 8)
    keep = ["A", "B", "DRB1"]
    pid, did, rec = match_umug_text(ptext, text, keep)
    mm0 = sorted({H[0] for line in rec for H, _ in line})
    for top_n, min_p0 in ((1, 0.0), (5, mm0[len(mm0) // 2]), (256, 0.0), (256, 2.0)):
        gpid, gdid, hits = search_umug_text(ptext, text, keep, top_n, min_p0)
        assert gpid == pid and gdid == did and len(hits) == len(pid) == 8
        for p, line in enumerate(rec):
            order = list(range(len(line)))  # a selection sort by pairwise comparison under the contract's three rules
            want = []
            while order and len(want) < top_n:
                best = order[0]
                for d in order[1:]:
                    x, y = line[d][0], line[best][0]
                    if x[0] > y[0] or (x[0] == y[0] and (x[1] > y[1] or (x[1] == y[1] and d < best))):
                        best = d
                order.remove(best)
                if line[best][0][0] >= min_p0:
                    want.append(best)
                else:
                    break
            assert [h[0] for h in hits[p]] == want
            assert [(h[1], h[2]) for h in hits[p]] == [line[d] for d in want]
            assert [[float(x).hex() for x in h[1]] for h in hits[p]] == [[float(x).hex() for x in line[d][0]] for d in want]
        if min_p0 == 2.0:
            assert all(h == [] for h in hits)
        if top_n == 5 and min_p0 > 0.0:
            assert any(0 < len(h) for h in hits)
