"""Mismatch direction and per-locus grades, the host side (grim/match.py): the integer function the twins use,
answers worked out by hand, an exact-arithmetic witness, graded against ungraded bytes, the record twin against the text twin,
and the defaults.  No GPU."""
import itertools
import os

import numpy as np
import pytest

import harness

SLOT = {"A": 0, "B": 1, "C": 2, "DQB1": 3, "DRB1": 4}
ALL5 = list(SLOT)
ABITS = 12
BIG = [4000] * 5  # dictionary sizes: no id below is private
DIRS = ["either", "gvh", "hvg"]


def _key(fields):
    k = 0
    for s, f in enumerate(fields):
        k |= int(f) << (ABITS * s)
    return k


def _side(subjects):
    """[[(a fields, b fields, p)]] -> (res, rows) records, rows back to back"""
    from grim import _native as nat

    res = np.zeros(len(subjects), dtype=nat.RESULT_DT)
    flat = []
    for i, rows in enumerate(subjects):
        res[i]["row_off"][nat.T_UMUG], res[i]["n_rows"][nat.T_UMUG] = len(flat), len(rows)
        flat += [(_key(a), _key(b), p, 0, 0) for a, b, p in rows]
    return res, np.array(flat, dtype=nat.ROW_DT) if flat else np.zeros(0, dtype=nat.ROW_DT)


def _one(patient, donor, mask, direction, graded=False):
    """the record of one patient against one donor -> (mm, locus), graded (mm, grade[5][3])"""
    from grim.match import match_records

    rec, pf, df, stats = match_records(*_side([patient]), *_side([donor]), mask, BIG, direction=direction, graded=graded)
    assert list(pf) == [1] and list(df) == [1] and stats["pairs"] == 1
    return [float(x) for x in rec[0, 0]["mm"]], rec[0, 0]["grade" if graded else "locus"].tolist()


def _hex(rec):
    return [float(x).hex() for x in np.frombuffer(rec.tobytes(), dtype="<f8")]


# ---- 1. the integer function --------------------------------------------------------------------------------------------
def test_either_is_the_larger_of_the_two_directions():
    from grim import _native as nat
    from grim.match import locus_mismatches

    fields = list(itertools.product(range(4), repeat=4))
    for x1, x2, y1, y2 in fields:
        e, g, h = (int(locus_mismatches(x1, x2, y1, y2, d)) for d in (nat.MATCH_DIR_EITHER, nat.MATCH_DIR_GVH, nat.MATCH_DIR_HVG))
        assert e == max(g, h) and 0 <= min(g, h), (x1, x2, y1, y2)
        assert h == int(locus_mismatches(y1, y2, x1, x2, nat.MATCH_DIR_GVH))  # hvg is gvh with the roles exchanged
    # and on arrays, as the fold calls it
    x1, x2, y1, y2 = (np.array(c, dtype=np.int64) for c in zip(*fields))
    e, g, h = (locus_mismatches(x1, x2, y1, y2, d) for d in (nat.MATCH_DIR_EITHER, nat.MATCH_DIR_GVH, nat.MATCH_DIR_HVG))
    assert (e == np.maximum(g, h)).all() and (g != h).any() and (e != g).any()
    with pytest.raises(ValueError):
        locus_mismatches(1, 2, 1, 2, 3)


# ---- 2. answers worked out by hand --------------------------------------------------------------------------------------
def test_a_homozygous_donor_is_a_mismatch_in_one_direction_only():
    a1, a2 = 5, 6  # A*01:01, A*02:01
    hom, het = [([a1], [a1], 1.0)], [([a1], [a2], 1.0)]
    tail = [0.0] * 8
    # patient A*01:01+A*02:01, donor A*01:01+A*01:01: the patient carries something the donor lacks
    assert _one(het, hom, 0b1, "gvh")[0] == [0.0, 1.0, 0.0] + tail
    assert _one(het, hom, 0b1, "hvg")[0] == [1.0, 0.0, 0.0] + tail
    assert _one(het, hom, 0b1, "either")[0] == [0.0, 1.0, 0.0] + tail
    # the reverse pair: the mirror
    assert _one(hom, het, 0b1, "gvh")[0] == [1.0, 0.0, 0.0] + tail
    assert _one(hom, het, 0b1, "hvg")[0] == [0.0, 1.0, 0.0] + tail
    assert _one(hom, het, 0b1, "either")[0] == [0.0, 1.0, 0.0] + tail
    # the grades say the same per locus
    mm, grade = _one(het, hom, 0b1, "gvh", graded=True)
    assert mm == [0.0, 1.0, 0.0] + tail and grade == [[0.0, 1.0, 0.0]] + [[0.0] * 3] * 4
    mm, grade = _one(het, hom, 0b1, "hvg", graded=True)
    assert mm == [1.0, 0.0, 0.0] + tail and grade == [[1.0, 0.0, 0.0]] + [[0.0] * 3] * 4


def test_two_untyped_genotypes_are_two_mismatches_in_every_direction():
    gap = [([0], [0], 1.0)]
    typed = [([5], [6], 1.0)]
    for direction in DIRS:
        for p, d in ((gap, gap), (gap, typed), (typed, gap)):
            # everything typed is lacking on the untyped side, and an untyped field is always lacking
            mm, grade = _one(p, d, 0b1, direction, graded=True)
            assert mm[2] == 1.0 and sum(mm) == 1.0 and grade[0] == [0.0, 0.0, 1.0], (direction, p, d)


def test_both_copies_are_counted():
    # patient 5+5 against donor 6+7: two of the patient's alleles are lacking, and two of the donor's
    for direction in DIRS:
        assert _one([([5], [5], 1.0)], [([6], [7], 1.0)], 0b1, direction)[0][2] == 1.0
    # patient 5+6 against donor 5+5: the donor's second copy of 5 is not lacking in the patient
    assert _one([([5], [6], 1.0)], [([5], [5], 1.0)], 0b1, "hvg")[0][0] == 1.0


# ---- 3. an exact-arithmetic witness -------------------------------------------------------------------------------------
def _exact_subjects():
    """subjects whose rows are 2 or 4 equal probabilities (powers of two): every weight, product and sum is exact"""
    a = [([5, 6, 7, 8, 9], [5, 16, 17, 8, 19], 0.125), ([5, 6, 7, 8, 9], [15, 6, 17, 18, 9], 0.125)]
    b = [([5, 16, 7, 0, 9], [15, 6, 27, 0, 9], 0.25), ([15, 16, 7, 8, 19], [15, 6, 7, 8, 19], 0.25),
         ([5, 6, 17, 18, 9], [5, 6, 17, 8, 9], 0.25), ([25, 6, 7, 8, 9], [5, 26, 7, 8, 9], 0.25)]
    c = [([5, 6, 7, 8, 9], [15, 16, 17, 18, 19], 0.5), ([15, 16, 17, 18, 19], [15, 16, 17, 18, 19], 0.5)]
    return [a, b, c]


@pytest.mark.parametrize("direction", DIRS)
@pytest.mark.parametrize("mask", [0b11111, 0b10011, 0b10000], ids=bin)
def test_the_grades_of_a_locus_add_up_to_the_histogram_exactly(mask, direction):
    from grim.match import match_records

    subjects = _exact_subjects()
    rec = match_records(*_side(subjects), *_side(subjects), mask, BIG, direction=direction, graded=True)[0]
    slots = [s for s in range(5) if (mask >> s) & 1]
    seen = set()
    for p in range(len(subjects)):
        for d in range(len(subjects)):
            mm, grade = rec[p, d]["mm"].tolist(), rec[p, d]["grade"].tolist()
            total = 0.0
            for m in range(2 * len(slots) + 1):
                total = total + mm[m]
            assert total == 1.0
            for s in range(5):
                if s in slots:
                    assert (grade[s][0] + grade[s][1]) + grade[s][2] == total, (p, d, s)
                    seen.update(g for g in range(3) if grade[s][g] > 0.0)
                else:
                    assert grade[s] == [0.0, 0.0, 0.0]
    assert seen == {0, 1, 2}


# ---- 4. graded against ungraded, records against text, the defaults -----------------------------------------------------
def _records(text):
    """.umug text -> (res, rows): ids from a table built from the text, slot by locus name; in every second row the alleles of
    its first locus change haplotypes"""
    from grim import _native as nat

    ids = [dict() for _ in SLOT]
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
            if z == 0 and len(rows) % 2:
                x, y = y, x
            a |= x << (nat.ABITS * s)
            b |= y << (nat.ABITS * s)
        rows.append((a, b, float(p), 7, 9))
    r = np.zeros(len(res), dtype=nat.RESULT_DT)
    for i, (off, n) in enumerate(res):
        r[i]["row_off"][nat.T_UMUG], r[i]["n_rows"][nat.T_UMUG] = off, n
    return r, np.array(rows, dtype=nat.ROW_DT)


def _first_subjects(text, n):
    out, seen = [], 0
    for line in text.splitlines(keepends=True):
        seen += line.rstrip("\n").endswith(",0")
        if seen > n:
            break
        out.append(line)
    return "".join(out)


@pytest.fixture(scope="module")
def golden():
    text = open(os.path.join(harness.GOLD, "cau_mixed", "don.umug")).read()
    return (text,) + _records(text)


@pytest.mark.parametrize("direction", DIRS)
def test_graded_records_hold_the_ungraded_bytes(golden, direction):
    from grim.match import match_records

    _, res, rows = golden
    mask = 0b10011
    plain = match_records(res[:6], rows, res, rows, mask, BIG, direction=direction)
    graded = match_records(res[:6], rows, res, rows, mask, BIG, direction=direction, graded=True)
    assert list(plain[1]) == list(graded[1]) and list(plain[2]) == list(graded[2]) and plain[3] == graded[3]
    assert graded[0]["mm"].tobytes() == plain[0]["mm"].tobytes()
    assert np.ascontiguousarray(graded[0]["grade"][:, :, :, 0]).tobytes() == plain[0]["locus"].tobytes()
    assert (graded[0]["grade"][:, :, :, 1] > 0.0).any() and (graded[0]["grade"][:, :, :, 2] > 0.0).any()
    either = match_records(res[:6], rows, res, rows, mask, BIG)[0]
    assert (plain[0]["mm"][:, :, 0] >= either["mm"][:, :, 0]).all()  # rounded addition is monotone
    if direction != "either":
        assert plain[0].tobytes() != either.tobytes()


def test_record_twin_equals_text_twin_under_gvh_graded(golden):
    from grim import _native as nat
    from grim.marginal import keep_mask
    from grim.match import match_records, match_umug_text, text_records_array

    text, res, rows = golden
    keep = ["A", "B", "DRB1"]
    got = match_records(res[:8], rows, res, rows, keep_mask(SLOT, keep), BIG, direction="gvh", graded=True)
    pid, did, want = match_umug_text(_first_subjects(text, 8), text, keep, loci=ALL5, direction="gvh", graded=True)
    want = text_records_array(want, SLOT, graded=True)
    assert got[0].dtype == nat.MATCH_GRADE_DT and want.dtype == nat.MATCH_GRADE_DT and nat.MATCH_GRADE_DT.itemsize == 208
    assert got[0].shape == want.shape == (8, len(res)) and got[3]["pairs"] == 8 * len(res)
    assert _hex(got[0]) == _hex(want)
    plain = match_records(res[:8], rows, res, rows, keep_mask(SLOT, keep), BIG)[0]
    assert got[0]["mm"].tobytes() != plain["mm"].tobytes()  # the direction shows on this golden


def test_the_defaults_are_the_calls_without_the_keywords(golden):
    from grim.match import match_records, match_umug_text
    from grim.search import search_records, search_umug_text

    text, res, rows = golden
    mask = 0b11111
    a = match_records(res[:4], rows, res, rows, mask, BIG)
    b = match_records(res[:4], rows, res, rows, mask, BIG, groups=None, direction="either", graded=False)
    assert a[0].dtype == b[0].dtype and a[0].tobytes() == b[0].tobytes() and list(a[1]) == list(b[1]) and a[3] == b[3]
    ptext = _first_subjects(text, 4)
    assert match_umug_text(ptext, text, ALL5) == match_umug_text(ptext, text, ALL5, direction="either", graded=False)
    ids = np.arange(len(res), dtype=np.uint32)
    sa = search_records(res[:4], rows, [(res, rows, ids)], mask, BIG, 5, 0.0)
    sb = search_records(res[:4], rows, [(res, rows, ids)], mask, BIG, 5, 0.0, direction="either")
    assert sa[0].tobytes() == sb[0].tobytes() and list(sa[1]) == list(sb[1]) and sa[2] == sb[2]
    assert search_umug_text(ptext, text, ALL5, 5) == search_umug_text(ptext, text, ALL5, 5, direction="either")
    for bad in ("GVH", "both", 3, None):
        with pytest.raises(ValueError):
            match_records(res[:1], rows, res[:1], rows, mask, BIG, direction=bad)


def test_search_twins_agree_under_a_direction(golden):
    from grim.marginal import keep_mask
    from grim.search import search_records, search_umug_text

    text, res, rows = golden
    keep = ["A", "B", "DRB1"]
    ids = np.arange(len(res), dtype=np.uint32)
    hits, n_hits, stats = search_records(res[:6], rows, [(res, rows, ids)], keep_mask(SLOT, keep), BIG, 4, 0.01, direction="hvg")
    pid, did, want = search_umug_text(_first_subjects(text, 6), text, keep, 4, 0.01, direction="hvg")
    for p in range(6):
        assert [int(h["donor"]) for h in hits[p, :int(n_hits[p])]] == [w[0] for w in want[p]]
        assert [[float(x) for x in h["rec"]["mm"][:7]] for h in hits[p, :int(n_hits[p])]] == [w[1] for w in want[p]]
