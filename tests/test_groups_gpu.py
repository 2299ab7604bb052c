"""Allele groups on the device (csrc/grim_groups.h through grim/groups.py, grim/marginal.py, grim/match.py, grim/search.py): the
map kernel through grim_groups_map_records against its CPU twin; what grim_groups_create refuses; the marginal, the match and
the search through their records doors with a map attached against the record twins; and the public functions on two goldens
against the text twins on regrouped text.  Everything is compared bit for bit."""
import os

import numpy as np
import pytest

import harness

pytestmark = pytest.mark.gpu

ABITS = 12
LOCI = ["A", "B", "C", "DQB1", "DRB1"]
N_ALLELES = [4050] * 5  # dictionary sizes of the synthetic subjects: ids above are private
PRIVATE_ID = 4060


@pytest.fixture(scope="module")
def ctx():
    from grim import _native as nat

    return nat.default_context(None)


def _key(fields):
    k = 0
    for s, f in enumerate(fields):
        k |= int(f) << (ABITS * s)
    return k


def _groups(kinds, n_alleles=N_ALLELES):
    """AlleleGroups over synthetic dictionaries.  kinds[s]: "id" (identity), "one" (every allele into one group) or an int G
    (allele f into group (f - 1) % G + 1): the alleles are named so that the first-field rule gives exactly that."""
    from grim.groups import AlleleGroups

    names, spec = [], {}
    for s, (kind, n) in enumerate(zip(kinds, n_alleles)):
        spec[LOCI[s]] = None if kind == "id" else "first_field"
        group = (lambda f: f) if kind == "id" else (lambda f: 1) if kind == "one" else (lambda f, G=kind: (f - 1) % G + 1)
        names.append(["%s*%04d:%04d" % (LOCI[s], group(f), f) for f in range(1, n + 1)])
    ag = AlleleGroups.from_names(LOCI, names, spec)
    for s, (kind, n) in enumerate(zip(kinds, n_alleles)):
        assert ag.n_groups[s] == (n if kind == "id" else min(n, 1) if kind == "one" else min(n, kind))
    return ag


MIXED = [16, "id", "one", "id", 7]  # what the consumer tests attach: watch_mask 0b10101


# ---- 1. the map kernel ------------------------------------------------------------------------------------------------------
ROW_COUNTS = [0, 1, 255, 256, 257, 70001]  # 70 001: more than one pass of the grid-stride loop (256 workgroups of 256 rows)
TABLES = {"identity": (["id"] * 5, N_ALLELES),
          "all_to_one": (["one"] * 5, N_ALLELES),
          "full_and_empty": ([16, "id", "one", 3, 7], [4095, 4095, 0, 4095, 1]),  # n_alleles 4095, and a slot with no alleles
          "mixed": (MIXED, N_ALLELES)}
_random_rows = {}


def _rows(n, n_alleles):
    """n seeded random rows: in every slot the fields 0, 1, n_alleles, n_alleles + 1, 4095 and random ones, bit 60 mixed"""
    from grim import _native as nat

    at = (n, tuple(n_alleles))
    if at not in _random_rows:
        rng = np.random.default_rng(1234 + n)
        rows = np.zeros(n, dtype=nat.ROW_DT)
        for side in ("a", "b"):
            key = rng.integers(0, 2, n).astype(np.uint64) << np.uint64(60)
            for s in range(5):
                edge = np.array([0, 1, n_alleles[s], min(n_alleles[s] + 1, 4095), 4095], dtype=np.uint64)
                f = np.where(rng.integers(0, 3, n) == 0, edge[rng.integers(0, 5, n)], rng.integers(0, 4096, n).astype(np.uint64))
                key |= f.astype(np.uint64) << np.uint64(ABITS * s)
            rows[side] = key
        rows["prob"] = np.frombuffer(rng.integers(0, 1 << 63, n).astype(np.uint64).tobytes(), dtype="<f8")  # any bits: prob is moved, not computed
        rows["popa"], rows["popb"] = rng.integers(0, 1 << 32, n), rng.integers(0, 1 << 32, n)
        _random_rows[at] = rows
    return _random_rows[at]


@pytest.mark.parametrize("staged", ["0", "1"], ids=["tables_in_l2", "tables_in_lds"])
@pytest.mark.parametrize("table", list(TABLES))
def test_map_kernel_bit_for_bit(ctx, monkeypatch, table, staged):
    from grim import _native as nat

    monkeypatch.setenv("GRIM_GROUPS_LDS", staged)  # read when the map is created
    kinds, n_alleles = TABLES[table]
    ag = _groups(kinds, n_alleles)
    dev = nat.Groups.of(ctx, ag)
    try:
        assert dev.watch_mask() == ag.watch_mask
        for n in ROW_COUNTS:
            rows = _rows(n, n_alleles)
            want = ag.map_records(rows)
            got = dev.map_records(rows)
            assert got.tobytes() == want.tobytes(), "%d rows" % n
            assert (dev.kernel_ms() > 0.0) == (n > 0)  # no rows: no launch
            if table == "identity":
                assert got.tobytes() == rows.tobytes()
            elif n >= 255:
                assert got.tobytes() != rows.tobytes()
    finally:
        dev.close()


def test_create_refusals(ctx):
    from grim import _native as nat

    na, ng = [3, 2, 0, 0, 0], [2, 2, 0, 0, 0]
    good = [0, 1, 2, 1, 0, 1, 2, 0, 0, 0]
    nat.Groups(ctx, good, na, ng).close()

    def refused(table, n_alleles=na, n_groups=ng):
        with pytest.raises(nat.NativeError) as e:
            nat.Groups(ctx, table, n_alleles, n_groups)
        return str(e.value)

    assert "slot 0, entry 0" in refused([1, 1, 2, 1, 0, 1, 2, 0, 0, 0])   # T[0] != 0
    assert "slot 1, entry 0" in refused([0, 1, 2, 1, 7, 1, 2, 0, 0, 0])
    assert "slot 0, entry 2" in refused([0, 1, 0, 2, 0, 1, 2, 0, 0, 0])   # an entry 0
    assert "slot 1, entry 1" in refused([0, 1, 2, 1, 0, 3, 2, 0, 0, 0])   # an entry above n_groups
    assert "slot 0" in refused([0, 1, 1, 1, 0, 1, 2, 0, 0, 0]) and "group 2" in refused([0, 1, 1, 1, 0, 1, 2, 0, 0, 0])  # an unused id
    assert "slot 3" in refused([0] * 4200, [0, 0, 0, 4096, 0], [0, 0, 0, 1, 0])  # n_alleles above 4095
    assert "slot 1" in refused(good, na, [2, 3, 0, 0, 0])  # more groups than alleles
    nat.Groups(ctx, good, na, ng).close()  # a refusal leaves the context usable


# ---- synthetic subjects (the builders of tests/test_marginal_gpu.py and tests/test_match_gpu.py, restated) -----------------
def _mg_subject(case, n):
    """n rows (a, b, p) of one subject of the marginal cases; slots 0, 1, 4 are the ones the proper subset keeps"""
    rows = []
    for k in range(n):
        noise = (k % 4000) + 1
        p = [0.1, 0.2, 0.3][k % 3] * 10.0 ** -(k % 5)
        if case == "one_group":
            q = 0 if k % 3 == 0 else noise
            fa, fb = [5, 6, noise, q, 7], [8, 9, 4001 - noise, q, 10]
        elif case == "distinct":
            fa, fb = [noise, 6, 3, 3, 7], [8, 9, 3, 3, 10]
        elif case == "interleaved_ties":
            g = k % 7
            p = [0.1, 0.2, 0.3][g % 3] * 10.0 ** -((k // 7) % 5)
            fa, fb = [20 + g, 6, noise, 3, 7], [8, 9, 3, noise, 10 + g]
        else:  # swapped
            g = (k // 2) % 50
            fa, fb = [30 + g, 6, noise, 3, 7], [90 + g, 9, 3, noise, 10]
            if k % 2:
                fa[0], fb[0] = fb[0], fa[0]
                fa[4], fb[4] = fb[4], fa[4]
        rows.append((_key(fa) | ((k % 2) << 60), _key(fb) | (((k // 2) % 2) << 60), p))
    return rows


def _mt_subject(case, n, shift=0):
    """n rows (a, b, p) of one subject of the match cases over a small pool of alleles"""
    rows = []
    for k in range(n):
        noise = (k + shift) % 6 + 20
        p = [0.1, 0.2, 0.3][k % 3] * 10.0 ** -((k * 7) % 20)
        fa, fb = [5, 6, noise, 3, 7], [8, 9, 3, noise, 10]
        if case == "same":
            pass
        elif case == "distinct":
            fa[0], fb[4] = 30 + (k + shift) % 4000, 40 + k % 3
        elif case == "swapped":
            fa[0], fb[1] = 30 + ((k // 2) + shift) % 5, 9 + (k // 2) % 2
            if k % 2:
                fa[0], fb[0] = fb[0], fa[0]
                fa[4], fb[4] = fb[4], fa[4]
        elif case == "homhet":
            if k % 2 == 0:
                fb[0] = fa[0]
            if k % 3 == 0:
                fa[4] = fb[4]
        else:  # untyped
            if k % 3 == 0:
                fa[4] = fb[4] = 0
            if k % 4 == 0:
                fa[2] = fb[2] = 0
        rows.append((_key(fa) | ((k % 2) << 60), _key(fb) | (((k // 2) % 2) << 60), p))
    return rows


MT_CASES = ["same", "distinct", "swapped", "homhet", "untyped"]


def _batch(subjects):
    """[(status, rows)] -> (res, rows) records, rows back to back"""
    from grim import _native as nat

    res = np.zeros(len(subjects), dtype=nat.RESULT_DT)
    flat = []
    for i, (status, rows) in enumerate(subjects):
        res[i]["status"], res[i]["plan"] = status, ord("abc"[i % 3])
        res[i]["row_off"][nat.T_UMUG], res[i]["n_rows"][nat.T_UMUG] = len(flat), len(rows)
        res[i]["n_genotypes"] = len(rows)
        flat += rows
    out = np.zeros(len(flat), dtype=nat.ROW_DT)
    for k, (a, b, p) in enumerate(flat):
        out[k] = (a, b, p, 3, 4)
    return res, out


def _with_private(rows, slot, at=-1):
    rows = list(rows)
    a, b, p = rows[at]
    rows[at] = ((a & ~(0xFFF << (ABITS * slot))) | (PRIVATE_ID << (ABITS * slot)), b, p)
    return rows


def _past_the_rows(res, rows):
    """two more subjects whose offsets point past the rows given: skipped, never read"""
    from grim import _native as nat

    bad = np.zeros(2, dtype=nat.RESULT_DT)
    bad["row_off"][:, nat.T_UMUG] = [len(rows) - 1, len(rows) + 7]
    bad["n_rows"][:, nat.T_UMUG] = [5, 1]
    return np.concatenate([res[:2], bad[:1], res[2:], bad[1:]])


# ---- 2. the marginal through the records door ---------------------------------------------------------------------------------
MG_SIZES = [1, 64, 65, 256, 257]  # either side of MG_LDS_ROWS
MG_CASES = ["one_group", "distinct", "interleaved_ties", "swapped"]


@pytest.fixture(scope="module")
def mg_shapes():
    from grim import _native as nat

    subjects = [(nat.ST_OK, _mg_subject(MG_CASES[(i + j) % 4], n)) for i, n in enumerate(MG_SIZES) for j in range(2)]
    subjects.insert(1, (nat.ST_OK, _with_private(_mg_subject("distinct", 70), 0, at=66)))  # private in a watched kept slot
    subjects.insert(3, (nat.ST_OK, _with_private(_mg_subject("swapped", 9), 1)))           # private in an identity slot
    subjects.insert(4, (nat.ST_MISS, _with_private(_mg_subject("distinct", 5), 0)))        # private, but the status is not OK
    subjects.insert(6, (nat.ST_OK, []))
    subjects.insert(7, (nat.ST_OK, _with_private(_mg_subject("distinct", 3), 2)))          # private in a watched slot that is not kept
    res, rows = _batch(subjects)
    return _past_the_rows(res, rows), rows


def _same_marginal(got, want):
    (gres, grows, gstats), (wres, wrows, wstats) = got, want
    assert gstats == wstats
    assert gres.tobytes() == wres.tobytes()
    assert [float(x).hex() for x in grows["prob"]] == [float(x).hex() for x in wrows["prob"]]
    assert grows.tobytes() == wrows.tobytes()


def _reduce(red, res, rows):
    red.reduce_records(res, rows)
    assert red.kernel_ms() > 0.0
    return red.results() + (red.stats(),)


@pytest.mark.parametrize("max_rows", [1, 2000])
def test_marginal_with_groups_bit_for_bit(ctx, mg_shapes, max_rows):
    from grim import _native as nat
    from grim.marginal import reduce_records

    res, rows = mg_shapes
    mask = 0b10011
    ag = _groups(MIXED)
    plain = reduce_records(res, rows, mask, max_rows)
    want = reduce_records(res, rows, mask, max_rows, groups=ag)
    assert want[2]["groups"] < plain[2]["groups"] and want[2]["rows_in"] == plain[2]["rows_in"]  # the map merges rows
    flags = ag.flags(res, rows, mask)
    assert list(np.flatnonzero(flags)) == [1]  # the private field in slot 0; not the one in slot 1, the MISS, the unkept slot 2
    red = nat.MarginalReducer(ctx, mask, max_rows)
    dev = nat.Groups.of(ctx, ag)
    try:
        _same_marginal(_reduce(red, res, rows), plain)
        assert not red.flags().any()  # no map attached
        red.set_groups(dev)
        assert red.subjects() == 0 and red.kernel_ms() == 0.0  # attaching clears the last results
        dev.close()  # the reducer holds its own copy of the tables
        _same_marginal(_reduce(red, res, rows), want)
        assert list(red.flags()) == list(flags)
        _same_marginal(_reduce(red, res[:3], rows), reduce_records(res[:3], rows, mask, max_rows, groups=ag))  # shrinks; reuse
        red.set_groups(None)
        _same_marginal(_reduce(red, res, rows), plain)  # detached: ungrouped again
        assert not red.flags().any()
    finally:
        dev.close()
        red.close()


def test_marginal_all_to_one_nothing_merged_and_identity(ctx):
    from grim import _native as nat
    from grim.marginal import reduce_records

    res, rows = _batch([(nat.ST_OK, _mg_subject("distinct", n)) for n in MG_SIZES] + [(nat.ST_OK, _mg_subject("swapped", 65))])
    mask = 0b11111
    plain = reduce_records(res, rows, mask, 2000)
    red = nat.MarginalReducer(ctx, mask, 2000)
    try:
        for kinds, groups_want in ((["one"] * 5, len(res)),           # every row of a subject falls into one group
                                   ([2025] * 5, plain[2]["groups"]),  # not the identity, yet none of these alleles share a group
                                   (["id"] * 5, plain[2]["groups"])):
            ag = _groups(kinds)
            dev = nat.Groups.of(ctx, ag)
            try:
                red.set_groups(dev)
            finally:
                dev.close()
            want = reduce_records(res, rows, mask, 2000, groups=ag)
            assert want[2]["groups"] == groups_want
            got = _reduce(red, res, rows)
            _same_marginal(got, want)
            if kinds[0] == "id":
                assert ag.watch_mask == 0
                _same_marginal(got, plain)  # identity groups: the bytes of the ungrouped reduce
            else:
                assert ag.watch_mask == 0b11111 and (got[1].tobytes() != plain[1].tobytes()) == (kinds[0] == "one")
            assert not red.flags().any()
    finally:
        red.close()


def test_marginal_refuses_groups_of_another_context(ctx):
    from grim import _native as nat

    other = nat.Context(ctx.device)
    red = nat.MarginalReducer(ctx, 0b10011, 10)
    dev = nat.Groups.of(other, _groups(MIXED))
    try:
        with pytest.raises(nat.NativeError, match=r"\(-3\).*another context"):
            red.set_groups(dev)
    finally:
        dev.close()
        red.close()
        other.close()


# ---- 3. the match through the records door ------------------------------------------------------------------------------------
PATIENT_SIZES = [1, 2, 65]
DONOR_SIZES = [1, 64, 65, 129]


def _mt_specials(nat, subjects):
    subjects = list(subjects)
    subjects.insert(1, (nat.ST_MISS, _mt_subject("distinct", 5)))
    subjects.insert(3, (nat.ST_OK, []))
    subjects.insert(4, (nat.ST_OK, _with_private(_mt_subject("same", 3), 1)))      # a private id in a kept slot: left out
    subjects.insert(6, (nat.ST_OK, _with_private(_mt_subject("swapped", 66), 2)))  # outside 0b10011: still computed
    subjects.insert(7, (nat.ST_OK, [(_key([5, 6, 7, 8, 9]), _key([5, 6, 7, 8, 9]), 0.0)]))  # a total of 0: not valid
    res, rows = _batch(subjects)
    return _past_the_rows(res, rows), rows


@pytest.fixture(scope="module")
def mt_shapes():
    from grim import _native as nat

    patients = [(nat.ST_OK, _mt_subject(MT_CASES[(i + 1) % 5], n)) for i, n in enumerate(PATIENT_SIZES)]
    patients += [(nat.ST_OK, _mt_subject(case, 3, shift=1)) for case in MT_CASES]
    donors = [(nat.ST_OK, _mt_subject(MT_CASES[i % 5], n, shift=2)) for i, n in enumerate(DONOR_SIZES)]
    donors += [(nat.ST_OK, _mt_subject(case, n)) for case, n in zip(MT_CASES, (65, 1, 64, 2, 63))]
    return _mt_specials(nat, patients) + _mt_specials(nat, donors)


def _hex(a):
    return [float(x).hex() for x in np.frombuffer(a.tobytes(), dtype="<f8")]


def _same_match(got, want):
    (grec, gpf, gdf, gstats), (wrec, wpf, wdf, wstats) = got, want
    assert list(gpf) == list(wpf) and list(gdf) == list(wdf)
    assert gstats == wstats
    assert grec.shape == wrec.shape and _hex(grec) == _hex(wrec)
    assert grec.tobytes() == wrec.tobytes()


@pytest.mark.parametrize("mask", [0b10011, 0b11111], ids=["0b10011", "0b11111"])
def test_match_with_groups_bit_for_bit(ctx, mt_shapes, mask):
    from grim import _native as nat
    from grim.match import match_records

    ag = _groups(MIXED)
    plain = match_records(*mt_shapes, mask, N_ALLELES)
    want = match_records(*mt_shapes, mask, N_ALLELES, groups=ag)
    assert want[3]["pairs"] == plain[3]["pairs"] and want[0].tobytes() != plain[0].tobytes()
    assert list(want[1]) == list(plain[1]) and list(want[2]) == list(plain[2])  # private stays private, valid stays valid
    mt = nat.Matcher(ctx, mask, N_ALLELES)
    dev = nat.Groups.of(ctx, ag)
    try:
        mt.set_groups(dev)
        dev.close()
        mt.set_patients(*mt_shapes[:2])
        mt.run_records(*mt_shapes[2:])
        assert mt.kernel_ms() > 0.0
        _same_match(mt.results() + (mt.stats(),), want)
        mt.set_groups(None)  # detach: the patients are dropped with it
        assert mt.patients() == 0 and mt.donors() == 0
        mt.set_patients(*mt_shapes[:2])
        mt.run_records(*mt_shapes[2:])
        _same_match(mt.results() + (mt.stats(),), plain)
    finally:
        dev.close()
        mt.close()


def test_match_moves_mass_from_two_mismatches_to_none(ctx):
    from grim import _native as nat
    from grim.match import match_records

    # slot 0 groups allele f with f + 16: (5, 8) against (21, 24) differs in both alleles and is equal at group level
    pres, prows = _batch([(nat.ST_OK, [(_key([5, 6, 1, 1, 7]), _key([8, 9, 1, 1, 10]), 0.5)])])
    dres, drows = _batch([(nat.ST_OK, [(_key([24, 6, 2, 2, 7]), _key([21, 9, 2, 2, 10]), 0.25)])])
    ag = _groups(MIXED)
    mt = nat.Matcher(ctx, 0b10011, N_ALLELES)
    dev = nat.Groups.of(ctx, ag)
    try:
        mt.set_patients(pres, prows)
        mt.run_records(dres, drows)
        rec = mt.results()[0][0, 0]
        assert list(rec["mm"][:3]) == [0.0, 0.0, 1.0] and rec["locus"][0] == 0.0
        _same_match(mt.results() + (mt.stats(),), match_records(pres, prows, dres, drows, 0b10011, N_ALLELES))
        mt.set_groups(dev)
        with pytest.raises(nat.NativeError, match=r"\(-3\).*no patients"):  # set_groups dropped the patients
            mt.run_records(dres, drows)
        assert mt.donors() == 0 and mt.kernel_ms() == 0.0
        mt.set_patients(pres, prows)
        mt.run_records(dres, drows)
        rec = mt.results()[0][0, 0]
        assert list(rec["mm"][:3]) == [1.0, 0.0, 0.0] and rec["locus"][0] == 1.0
        _same_match(mt.results() + (mt.stats(),), match_records(pres, prows, dres, drows, 0b10011, N_ALLELES, groups=ag))
    finally:
        dev.close()
        mt.close()


def test_match_and_search_refuse_foreign_or_mismatched_groups(ctx):
    from grim import _native as nat

    other = nat.Context(ctx.device)
    mt = nat.Matcher(ctx, 0b10011, N_ALLELES)
    sr = nat.Searcher(ctx, 0b10011, N_ALLELES, 8)
    foreign = nat.Groups.of(other, _groups(MIXED))
    smaller = nat.Groups.of(ctx, _groups(MIXED, [4050, 4050, 4050, 4050, 4049]))
    pres, prows = _batch([(nat.ST_OK, _mt_subject("same", 2))])
    try:
        for obj in (mt, sr):
            obj.set_patients(pres, prows)
            with pytest.raises(nat.NativeError, match=r"\(-3\).*another context"):
                obj.set_groups(foreign)
            assert obj.patients() == 0  # clearing comes before checking
            with pytest.raises(nat.NativeError, match=r"\(-3\).*slot 4.*n_alleles"):
                obj.set_groups(smaller)
    finally:
        foreign.close()
        smaller.close()
        sr.close()
        mt.close()
        other.close()


# ---- 4. the search --------------------------------------------------------------------------------------------------------------
def _donors(n):
    """n donors of 1-3 rows cycling over a pool of 5 genotypes (thousands of ties), the specials among them; the ids are a fixed
    permutation of 32-bit numbers"""
    from grim import _native as nat

    pool = [_mt_subject(MT_CASES[j], 1 + j % 3, shift=j) for j in range(5)]
    # every second donor carries, in slot 0, the alleles 16 ids further on: other alleles, the same groups under MIXED
    far = [[(a + (16 if a & 0xFFF else 0), b + (16 if b & 0xFFF else 0), p) for a, b, p in rows] for rows in pool]
    res, rows = _mt_specials(nat, [(nat.ST_OK, (far if i % 2 else pool)[(i * 3) % 5]) for i in range(n - 7)])
    assert len(res) == n
    return res, rows, ((np.arange(n, dtype=np.uint64) * 2654435761 + 12345) % (1 << 32)).astype(np.uint32)


def test_search_with_groups_bit_for_bit(ctx, monkeypatch):
    from grim import _native as nat
    from grim.search import search_records

    monkeypatch.setenv("GRIM_SEARCH_TILE", "64")  # read when a search is created: 600 donors are three levels
    top_n, mask = 8, 0b10011
    ag = _groups(MIXED)
    pres, prows = _mt_specials(nat, [(nat.ST_OK, _mt_subject("same", 3)), (nat.ST_OK, _mt_subject("homhet", 66, shift=1))])
    run = _donors(600)
    want = search_records(pres, prows, [run], mask, N_ALLELES, top_n, 0.0, groups=ag)
    plain = search_records(pres, prows, [run], mask, N_ALLELES, top_n, 0.0)
    assert want[2]["candidates"] > top_n and want[0].tobytes() != plain[0].tobytes()
    sr = nat.Searcher(ctx, mask, N_ALLELES, top_n)
    dev = nat.Groups.of(ctx, ag)
    try:
        sr.set_groups(dev)
        sr.set_patients(pres, prows)
        sr.run_records(*run)
        hits, n_hits = sr.results()
        assert list(n_hits) == list(want[1]) and hits["donor"].tolist() == want[0]["donor"].tolist()
        assert _hex(hits["rec"]) == _hex(want[0]["rec"]) and hits.tobytes() == want[0].tobytes() and sr.stats() == want[2]
        # a hit list computed at one resolution never meets another: set_groups empties the running lists and the sums
        sr.set_groups(None)
        assert sr.patients() == 0 and sr.stats() == dict.fromkeys(nat.SEARCH_STATS, 0)
        sr.set_patients(pres, prows)
        hits, n_hits = sr.results()
        assert not n_hits.any() and (hits["donor"] == nat.SEARCH_NO_DONOR).all()
        sr.run_records(*run)
        hits, n_hits = sr.results()
        assert hits.tobytes() == plain[0].tobytes() and list(n_hits) == list(plain[1]) and sr.stats() == plain[2]
    finally:
        dev.close()
        sr.close()


# ---- 5. end to end on the goldens -----------------------------------------------------------------------------------------------
_imps, _graphs = {}, {}


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
    conf, cpath = harness._write_inputs(work, conf, lines, "groups_" + scenario)
    cwd = os.getcwd()
    os.chdir(work)
    try:
        cfg, _ = load_config(cpath)
        # a graph of this module's own: other modules' runs intern alleles they meet into a shared graph's dictionary, and
        # the cases below are about alleles the dictionary does not know
        g = _graphs.get(gname)
        if g is None:
            g = _graphs[gname] = Graph(cfg).build_graph(cfg["node_file"], cfg["top_links_file"], cfg["edges_file"])
        imp = Imputation(g, cfg)
    finally:
        os.chdir(cwd)
    imp.on_unsupported = "raise"
    imp.quiet = True
    _imps[scenario] = (imp, lines, exp, em)
    return _imps[scenario]


def _subjects_of(text):
    out = []
    for line in text.splitlines(keepends=True):
        if line.rstrip("\n").endswith(",0"):
            out.append([line.split(",")[0], ""])
        out[-1][1] += line
    return out


def _a02_table(graph):
    """a table specification: every A*02:... allele of the dictionary, and A*98:01, which no graph here has seen, into A*02"""
    s = graph.locus_slot["A"]
    table = {name: "A*02" for name in (graph.adict.name(s, i) for i in range(graph.adict.count(s))) if name.startswith("A*02:")}
    assert table and "A*98:01" not in table
    table["A*98:01"] = "A*02"
    assert "A*98:01" not in [graph.adict.name(s, i) for i in range(graph.adict.count(s))]  # unseen: private to its subjects
    return {"A": table}


def _check_marginal(scenario, spec, keep, blocks):
    from grim.groups import regroup_umug_text
    from grim.marginal import marginal_umug, reduce_umug_text

    imp, lines, exp, em = _imputation(scenario)
    R = int(imp.config["number_of_results"])
    want = reduce_umug_text(regroup_umug_text(exp["umug"], spec), keep, R)
    assert want != reduce_umug_text(exp["umug"], keep, R)
    stats = None
    for block in blocks:
        text, stats = marginal_umug(imp, lines, imp.config, keep, block_lines=block, em=em, groups=spec)
        assert text == want, "block_lines=%d" % block
        assert stats["undefined"] == 0 and stats["kernel_ms"] > 0.0 and stats["rows_in"] == len(exp["umug"].splitlines())
        assert stats["rows_out"] == len(want.splitlines())
        assert stats["groups"] == len(reduce_umug_text(regroup_umug_text(exp["umug"], spec), keep).splitlines())
    return stats


def _check_match(scenario, spec, keep, blocks):
    from grim.groups import regroup_umug_text
    from grim.match import match_probabilities, match_umug_text, text_records_array

    imp, lines, exp, em = _imputation(scenario)
    subjects = _subjects_of(regroup_umug_text(exp["umug"], spec))
    stats = None
    for block in blocks:
        pok, dok, rec, stats = match_probabilities(imp, lines[:8], lines, imp.config, keep, block_lines=block, em=em, groups=spec)
        assert int(dok.sum()) == len(subjects) and list(pok) == list(dok[:8]) and stats["undefined"] == 0
        patient_text = "".join(t for _, t in subjects[:int(pok.sum())])
        want = text_records_array(match_umug_text(patient_text, "".join(t for _, t in subjects), keep)[2], imp.netGraph.locus_slot)
        got = rec[np.flatnonzero(pok)][:, np.flatnonzero(dok)]
        assert got.shape == want.shape and _hex(got) == _hex(want), "block_lines=%d" % block
        assert stats["pairs"] + stats["host_pairs"] == int(pok.sum()) * len(subjects)
    return stats


def test_pop4_mixed_first_field_marginal_whatever_the_cuts():
    stats = _check_marginal("pop4_mixed", "first_field", ("A", "B", "DRB1"), (65536, 7, 1))
    assert stats["host_subjects"] == 0


def test_pop4_mixed_first_field_match_whatever_the_cuts():
    _check_match("pop4_mixed", {"A": "first_field", "B": "first_field"}, ("A", "B", "DRB1"), (65536, 7, 1))


def test_pop4_planc_first_field_folds_the_unseen_allele_on_the_host():
    """pop4_planc prints A*98:01, which its graph has never seen: with A kept, that subject's marginal and its pairs are the
    host's"""
    stats = _check_marginal("pop4_planc", "first_field", ("A", "B", "DRB1"), (65536, 7))
    assert stats["host_subjects"] > 0
    stats = _check_match("pop4_planc", "first_field", ("A", "B", "DRB1"), (65536,))
    assert stats["host_pairs"] > 0
    assert _check_marginal("pop4_planc", "first_field", ("DRB1",), (65536,))["host_subjects"] == 0  # every DRB1 allele is known


def test_pop4_planc_unseen_allele_into_a_group_the_dictionary_knows():
    """a table sends A*98:01 and every A*02 allele to A*02: the private allele falls into a known group, which the device alone
    would keep apart"""
    imp, lines, exp, em = _imputation("pop4_planc")
    spec = _a02_table(imp.netGraph)
    assert "A*98:01" in exp["umug"]
    stats = _check_marginal("pop4_planc", spec, ("A", "B", "DRB1"), (65536,))
    assert stats["host_subjects"] > 0
    stats = _check_match("pop4_planc", spec, ("A", "B", "DRB1"), (65536,))
    assert stats["host_pairs"] > 0


def test_search_donors_with_groups_equals_the_text_twin():
    from grim.groups import regroup_umug_text
    from grim.match import line_id
    from grim.search import search_donors, search_umug_text

    imp, lines, exp, em = _imputation("pop4_planc")
    keep, top_n, spec = ("A", "B", "DRB1"), 5, "first_field"
    pok, hits, n_hits, stats = search_donors(imp, lines[:8], lines, imp.config, keep, top_n, em=em, groups=spec)
    subjects = _subjects_of(exp["umug"])
    patient_text = "".join(t for _, t in subjects[:int(pok.sum())])
    pid, did, want = search_umug_text(patient_text, exp["umug"], keep, top_n, groups=spec)
    assert pid == [line_id(lines[i]) for i in np.flatnonzero(pok)] and stats["host_pairs"] > 0
    with_rows = []  # donor position in the text -> line: the subjects come in line order
    for i, l in enumerate(lines):
        if len(with_rows) < len(did) and line_id(l) == did[len(with_rows)]:
            with_rows.append(i)
    assert len(with_rows) == len(did) == len(subjects)
    for p, line in enumerate(np.flatnonzero(pok)):
        got = [(int(h["donor"]), [float(x) for x in h["rec"]["mm"][:2 * len(keep) + 1]]) for h in hits[line, :int(n_hits[line])]]
        assert [(with_rows[d], [float(x) for x in H]) for d, H, _ in want[p]] == got
