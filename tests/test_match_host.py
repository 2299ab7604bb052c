"""The match probabilities' host side (grim/match.py): the record twin on answers worked out by hand, the record twin against
the text twin on the golden .umug files, that those comparisons are not vacuous, and the argument checks.  No GPU."""
import os

import numpy as np
import pytest

import harness

SLOT = {"A": 0, "B": 1, "C": 2, "DQB1": 3, "DRB1": 4}
ALL5 = list(SLOT)
SCENARIOS = ["pop4_mixed", "cau_mixed", "bc_cau_default_map", "pop4_planc", "cau_edge"]
KEEPS = [ALL5, ["A", "B", "DRB1"], ["DRB1"]]
ABITS = 12
BIG = [4000] * 5  # dictionary sizes: no id below is private


def _umug(scenario):
    return open(os.path.join(harness.GOLD, scenario, "don.umug")).read()


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


def _one(patient, donor, mask):
    """the record of one patient against one donor"""
    from grim.match import match_records

    rec, pf, df, stats = match_records(*_side([patient]), *_side([donor]), mask, BIG)
    assert list(pf) == [1] and list(df) == [1] and stats["pairs"] == 1 and stats["row_pairs"] == len(patient) * len(donor)
    return [float(x) for x in rec[0, 0]["mm"]], [float(x) for x in rec[0, 0]["locus"]]


# ---- 1. known answers ---------------------------------------------------------------------------------------------------
def test_identical_one_row_subjects_match_everywhere():
    g = [([5, 6, 7, 8, 9], [15, 16, 17, 18, 19], 0.25)]
    mm, locus = _one(g, g, 0b11111)
    assert mm == [1.0] + [0.0] * 10 and locus == [1.0] * 5
    mm, locus = _one(g, g, 0b10011)
    assert mm == [1.0] + [0.0] * 10 and locus == [1.0, 1.0, 0.0, 0.0, 1.0]


def test_homozygous_against_heterozygous_is_one_mismatch():
    x, y = 5, 6
    mm, locus = _one([([x], [x], 1.0)], [([x], [y], 1.0)], 0b1)
    assert mm == [0.0, 1.0] + [0.0] * 9 and locus == [0.0] * 5
    mm, _ = _one([([x], [y], 1.0)], [([x], [x], 1.0)], 0b1)
    assert mm[1] == 1.0


def test_donor_alleles_swapped_between_haplotypes_still_match():
    p = [([5, 6, 7, 8, 9], [15, 16, 17, 18, 19], 0.5)]
    d = [([15, 6, 17, 8, 19], [5, 16, 7, 18, 9], 0.125)]
    mm, locus = _one(p, d, 0b11111)
    assert mm[0] == 1.0 and sum(mm) == 1.0 and locus == [1.0] * 5


def test_disjoint_alleles_mismatch_everywhere():
    p = [([5, 6, 7, 8, 9], [15, 16, 17, 18, 19], 0.5)]
    d = [([25, 26, 27, 28, 29], [35, 36, 37, 38, 39], 0.5)]
    for mask, nk in ((0b11111, 5), (0b10011, 3), (0b10000, 1)):
        mm, locus = _one(p, d, mask)
        assert mm[2 * nk] == 1.0 and sum(mm) == 1.0 and locus == [0.0] * 5


def test_an_untyped_kept_locus_counts_two_on_either_side():
    full = [([5, 6, 7, 8, 9], [15, 16, 17, 18, 19], 0.5)]
    gap = [([5, 6, 0, 8, 9], [15, 16, 0, 18, 19], 0.5)]
    for p, d in ((full, gap), (gap, full), (gap, gap)):  # not even two untyped fields are equal
        mm, locus = _one(p, d, 0b11111)
        assert mm[2] == 1.0 and sum(mm) == 1.0 and locus == [1.0, 1.0, 0.0, 1.0, 1.0]
        assert _one(p, d, 0b11011)[0][0] == 1.0  # outside K it does not count


def test_differences_outside_k_and_bit_60_are_ignored():
    from grim import _native as nat
    from grim.match import match_records

    p = [([5, 6, 7, 8, 9], [15, 16, 17, 18, 19], 0.5)]
    d = [([5, 6, 77, 88, 9], [15, 16, 17, 18, 19], 0.5)]
    assert _one(p, d, 0b10011)[0][0] == 1.0 and _one(p, d, 0b11111)[0][2] == 1.0
    pres, prows = _side([p])
    dres, drows = _side([p])
    drows["a"] |= np.uint64(1 << 60)
    rec = match_records(pres, prows, dres, drows, 0b11111, BIG)[0]
    assert float(rec[0, 0]["mm"][0]) == 1.0 and nat.MATCH_DT.itemsize == 128


def test_weights_are_the_normalised_probabilities():
    g0, g1 = ([5, 6, 7, 8, 9], [15, 16, 17, 18, 19]), ([5, 6, 7, 8, 9], [15, 16, 17, 18, 20])
    mm, locus = _one([g0 + (3e-7,), g1 + (1e-7,)], [g0 + (0.5,)], 0b11111)
    assert mm[0] == 0.75 and mm[1] == 0.25 and locus == [1.0, 1.0, 1.0, 1.0, 0.75]


def test_what_is_not_valid_or_private_gives_zero_records():
    from grim import _native as nat
    from grim.match import match_records

    g = ([5, 6, 7, 8, 9], [15, 16, 17, 18, 19])
    pres, prows = _side([[g + (0.5,)], [g + (0.0,)], [([5, 6, 7, 8, 4001], g[1], 0.5)], [([5, 6, 4001, 8, 9], g[1], 0.5)], [g + (0.5,)], []])
    pres["status"][4] = nat.ST_MISS
    dres, drows = _side([[g + (0.25,)], [(g[0], [15, 0, 17, 18, 19], 0.5)]])
    dres["n_rows"][1, nat.T_UMUG] = 5  # past the rows given: skipped, not read
    rec, pf, df, stats = match_records(pres, prows, dres, drows, 0b10011, BIG)
    V, P = nat.MATCH_VALID, nat.MATCH_PRIVATE
    assert list(pf) == [V, 0, V | P, V, 0, 0] and list(df) == [V, 0]
    assert rec.shape == (6, 2) and [bool(np.frombuffer(rec[p, 0].tobytes(), dtype=np.uint8).any()) for p in range(6)] == [True, False, False, True, False, False]
    assert not np.frombuffer(rec[:, 1].tobytes(), dtype=np.uint8).any()
    assert stats == {"patients_valid": 3, "donors_valid": 1, "patients_private": 1, "donors_private": 0, "undefined": 0, "pairs": 2, "row_pairs": 2}
    # a haplotype typed where the other is not
    dres["n_rows"][1, nat.T_UMUG] = 1
    _, _, df, stats = match_records(pres, prows, dres, drows, 0b10011, BIG)
    assert list(df) == [V, V | nat.MATCH_UNDEFINED] and stats["undefined"] == 1
    # no donors: nothing ran
    assert match_records(pres, prows, dres[:0], drows[:0], 0b10011, BIG)[3] == dict.fromkeys(nat.MATCH_STATS, 0)


# ---- 2. and 3. twin against twin on the goldens -----------------------------------------------------------------------------
def _records(text):
    """.umug text -> (res, rows): ids from a table built from the text, slot by locus name; in every second row the alleles of
    its first locus change haplotypes, and bit 60 is set here and there"""
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
        rows.append((a | (len(rows) % 3 == 0) << 60, b, float(p), 7, 9))
    r = np.zeros(len(res), dtype=nat.RESULT_DT)
    for i, (off, n) in enumerate(res):
        r[i]["row_off"][nat.T_UMUG], r[i]["n_rows"][nat.T_UMUG] = off, n
    return r, np.array(rows, dtype=nat.ROW_DT)


def _first_subjects(text, n):
    """the rows of the first n subjects of a .umug text"""
    out, seen = [], 0
    for line in text.splitlines(keepends=True):
        seen += line.rstrip("\n").endswith(",0")
        if seen > n:
            break
        out.append(line)
    return "".join(out)


_twins = {}


def _both(scenario, keep):
    """-> (record twin's records, text twin's records as an array): computed once, shared, left alone"""
    from grim.marginal import keep_mask
    from grim.match import match_records, match_umug_text, text_records_array

    at = (scenario, tuple(keep))
    if at not in _twins:
        text = _umug(scenario)
        res, rows = _records(text)
        got = match_records(res[:8], rows, res, rows, keep_mask(SLOT, keep), BIG)
        pid, did, want = match_umug_text(_first_subjects(text, 8), text, keep, loci=ALL5)
        assert len(pid) == 8 and len(did) == len(res) and got[3]["pairs"] == 8 * len(res) and got[3]["undefined"] == 0
        _twins[at] = (got[0], text_records_array(want, SLOT))
    return _twins[at]


def _hex(rec):
    return [float(x).hex() for x in np.frombuffer(rec.tobytes(), dtype="<f8")]


@pytest.mark.parametrize("keep", KEEPS, ids=["~".join(k) for k in KEEPS])
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_record_twin_equals_text_twin(scenario, keep):
    got, want = _both(scenario, keep)
    assert got.shape == want.shape
    assert _hex(got) == _hex(want)


@pytest.mark.parametrize("keep", KEEPS, ids=["~".join(k) for k in KEEPS])
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_goldens_are_not_vacuous(scenario, keep):
    got, _ = _both(scenario, keep)
    mm = got["mm"].reshape(-1, got["mm"].shape[-1])
    fractional = np.count_nonzero(((mm > 0.0) & (mm < 1.0)).any(axis=1))
    assert fractional >= 0.2 * len(mm), "%d of %d pairs" % (fractional, len(mm))
    # (n_p * n_d + n_d) roundings of 2^-53 at 1000 x 1000 rows is 1.1e-10; the goldens' subjects have at most 20 rows
    assert float(np.abs(mm.sum(axis=1) - 1.0).max()) <= 1e-9
    assert (mm[:, 2 * len(keep) + 1:] == 0.0).all()
    locus = got["locus"].reshape(-1, 5)
    assert (locus[:, [s for n, s in SLOT.items() if n not in keep]] == 0.0).all() and (locus <= 1.0 + 1e-9).all()


# ---- 4. refusals of the twins ---------------------------------------------------------------------------------------------
def test_keep_must_be_known_and_not_empty():
    from grim import _native as nat
    from grim.match import match_records, match_umug_text

    text = "S,A*01:01+A*02:01^B*07:02+B*08:01,0.5,0\n"
    res, rows = _side([[([5], [6], 0.5)]])
    with pytest.raises(ValueError):
        match_umug_text(text, text, [])
    with pytest.raises(ValueError):
        match_umug_text(text, text, ["A", "DPB1"], loci=ALL5)
    with pytest.raises(ValueError):
        match_records(res, rows, res, rows, 0, BIG)
    with pytest.raises(ValueError):
        match_records(res, rows, res, rows, 1 << nat.MAXL, BIG)
    with pytest.raises(ValueError):
        match_umug_text(text, "S,A*01:01+A*02:01,0.0,0\n", ["A"])  # weights that cannot be formed
    pid, did, rec = match_umug_text(text, text, "A")
    assert pid == ["S"] and did == ["S"] and rec[0][0] == ([1.0, 0.0, 0.0], {"A": 1.0})
    # a kept locus that a row lacks is untyped
    assert match_umug_text(text, text, ["A", "C"])[2][0][0] == ([0.0, 0.0, 1.0, 0.0, 0.0], {"A": 1.0, "C": 0.0})
