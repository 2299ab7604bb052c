"""Allele groups, host side (grim/groups.py and the `groups=` keyword of the twins in grim/marginal.py, grim/match.py,
grim/search.py): the text rules, the tables on the CAU graph, the CPU twin of the map kernel on hand-written keys, a merge
worked out by hand, the record twins against the text twins on regrouped goldens, the identity specification, the exported
symbols.  No GPU."""
import json
import os

import numpy as np
import pytest

import harness

SLOT = {"A": 0, "B": 1, "C": 2, "DQB1": 3, "DRB1": 4}
ALL5 = list(SLOT)
ABITS = 12
GOLDENS = ["pop4_mixed", "cau_edge", "pop4_planc"]
KEEPS = [ALL5, ["A", "B", "DRB1"], ["A"]]
# group specifications, given the allele names per slot: one rule, rules for some loci, and a table (every A*02 allele into one
# group under a name of its own, as a P-group table would)
SPECS = {"first_field": lambda alleles: "first_field",
         "ab_first": lambda alleles: {"A": "first_field", "B": "first_field"},
         "a02_table": lambda alleles: {a: "A*02:01P" for a in alleles[0] if a.startswith("A*02:")}}


def _umug(scenario):
    return open(os.path.join(harness.GOLD, scenario, "don.umug")).read()


def _key(fields):
    k = 0
    for s, f in enumerate(fields):
        k |= int(f) << (ABITS * s)
    return k


# ---- 1. GroupSpec ---------------------------------------------------------------------------------------------------------
def test_rules_on_allele_text(tmp_path):
    from grim.groups import GroupSpec

    ff, tf = GroupSpec("first_field"), GroupSpec("two_field")
    assert ff.name("A", "A*02") == "A*02" and tf.name("A", "A*02") == "A*02"                    # no colon
    assert ff.name("A", "A*02:01") == "A*02" and tf.name("A", "A*02:01") == "A*02:01"           # two fields
    assert ff.name("DRB1", "DRB1*15:01:01") == "DRB1*15" and tf.name("DRB1", "DRB1*15:01:01") == "DRB1*15:01"  # three
    assert tf.name("C", "C*07:02:01:03") == "C*07:02"
    assert GroupSpec(None).name("A", "A*02:01") == "A*02:01"
    per = GroupSpec({"A": "first_field", "DRB1": None})
    assert per.name("A", "A*02:01") == "A*02" and per.name("B", "B*07:02") == "B*07:02" and per.name("DRB1", "DRB1*15:01") == "DRB1*15:01"
    assert per.is_identity("B") and not per.is_identity("A")
    table = GroupSpec({"A*02:01": "A*02:01P", "A*02:09": "A*02:01P"})  # one table for all loci; alleles not listed stay
    assert table.name("A", "A*02:09") == "A*02:01P" and table.name("A", "A*03:01") == "A*03:01" and table.name("B", "B*07:02") == "B*07:02"
    path = tmp_path / "groups.csv"
    path.write_text("allele,group\nA*02:01,A*02:01P\nA*02:09,A*02:01P\n")
    for spec in (GroupSpec(str(path)), GroupSpec({"A": str(path)})):
        assert spec.name("A", "A*02:09") == "A*02:01P" and spec.name("A", "A*24:02") == "A*24:02"


def test_a_group_that_crosses_loci_raises(tmp_path):
    from grim.groups import GroupSpec

    with pytest.raises(ValueError):
        GroupSpec({"A*02:01": "B*02"})
    with pytest.raises(ValueError):
        GroupSpec({"A": {"A*02:01": "B*02"}})
    path = tmp_path / "bad.csv"
    path.write_text("A*02:01,C*02\n")
    with pytest.raises(ValueError):
        GroupSpec(str(path))
    with pytest.raises(ValueError):
        GroupSpec({"A": {"B*07:02": "B*07"}}).name("A", "B*07:02")  # a B table asked about locus A
    with pytest.raises(ValueError):
        GroupSpec(7)


# ---- 2. AlleleGroups on the CAU graph ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cau():
    from grim.imputation.networkx_graph import Graph
    from grim.run_impute_def import load_config

    work = harness.ensure_graph("cau")
    path = os.path.join(work, "conf_groups_host.json")
    json.dump(harness.base_conf(harness.POPS["cau"]), open(path, "w"))
    cwd = os.getcwd()
    os.chdir(work)
    try:
        cfg, _ = load_config(path)
        return Graph(cfg).build_graph(cfg["node_file"], cfg["top_links_file"], cfg["edges_file"])
    finally:
        os.chdir(cwd)


def test_first_field_tables_on_the_cau_graph(cau):
    from grim import _native as nat
    from grim.groups import AlleleGroups

    ag = AlleleGroups(cau, "first_field")
    assert ag.spec.name("A", "A*02:01") == "A*02"
    merged = 0
    for s, locus in enumerate(cau.slot_locus):
        n = cau.adict.count(s)
        assert ag.n_alleles[s] == n and len(ag.table[s]) == n + 1 and ag.table[s].dtype == np.uint16
        assert ag.table[s][0] == 0 and ag.names[s][0] == ""
        want, seen = [], {}
        for f in range(1, n + 1):  # ids in the order of first appearance over the allele ids
            name = cau.key_alleles(f << (nat.ABITS * s))[s].split(":")[0]
            want.append(seen.setdefault(name, len(seen) + 1))
            assert ag.names[s][ag.table[s][f]] == name  # names round-trips
        assert list(ag.table[s][1:]) == want
        assert sorted(set(want)) == list(range(1, ag.n_groups[s] + 1)) and len(ag.names[s]) == ag.n_groups[s] + 1  # every id used
        assert bool((ag.watch_mask >> s) & 1) == (want != list(range(1, n + 1)))
        merged += ag.n_groups[s] < n
    assert merged >= 3 and ag.watch_mask != 0  # the CAU dictionary holds several two-field alleles of one first field
    assert len(ag.flat()) == sum(ag.n_alleles) + nat.MAXL
    for spec in (None, {}, {"A": None}):
        ident = AlleleGroups(cau, spec)
        assert ident.watch_mask == 0 and ident.n_groups == ident.n_alleles
        assert all(list(t) == list(range(len(t))) for t in ident.table)
    only_a = AlleleGroups(cau, {"A": "first_field"})
    assert only_a.watch_mask == 1 << cau.locus_slot["A"]


# ---- 3. map_records on hand-written keys --------------------------------------------------------------------------------------
def test_map_records_by_hand():
    from grim import _native as nat
    from grim.groups import AlleleGroups

    names = [["A*01:01", "A*02:01", "A*02:06", "A*03:01"], ["B*07:02", "B*08:01"], [], ["DQB1*02:01"], ["DRB1*15:01", "DRB1*15:02", "DRB1*03:01"]]
    ag = AlleleGroups.from_names(ALL5, names, {"A": "first_field", "DRB1": "first_field"})
    assert list(ag.table[0]) == [0, 1, 2, 2, 3] and ag.n_groups == [3, 2, 0, 1, 2] and ag.watch_mask == 0b10001
    assert list(ag.table[4]) == [0, 1, 1, 2] and ag.names[4] == ["", "DRB1*15", "DRB1*03"]
    rows = np.zeros(4, dtype=nat.ROW_DT)
    # slot 0: field 0, 1, n_alleles (4), n_alleles + 1 (5: private), 4095; bit 60 set on some
    rows["a"] = [_key([0, 1, 0, 1, 3]), _key([1, 2, 0, 0, 2]) | 1 << 60, _key([4, 3, 5, 1, 4]), _key([4095, 4095, 4095, 4095, 4095]) | 1 << 60]
    rows["b"] = [_key([5, 2, 1, 2, 1]), _key([3, 0, 0, 0, 0]), _key([2, 1, 0, 0, 0]) | 1 << 60, 0]
    rows["prob"], rows["popa"], rows["popb"] = [0.5, 0.25, 1e-300, float("inf")], [1, 2, 3, 0xFFFFFFFF], [9, 8, 7, 6]
    got = ag.map_records(rows)
    # private: n_groups + (f - n_alleles); slot 2 has no alleles, so every field there is private and stays what it is
    assert [int(x) for x in got["a"]] == [_key([0, 1, 0, 1, 2]), _key([1, 2, 0, 0, 1]) | 1 << 60, _key([3, 3, 5, 1, 3]),
                                         _key([4094, 4095, 4095, 4095, 4094]) | 1 << 60]
    assert [int(x) for x in got["b"]] == [_key([4, 2, 1, 2, 1]), _key([2, 0, 0, 0, 0]), _key([2, 1, 0, 0, 0]) | 1 << 60, 0]
    for field in ("prob", "popa", "popb"):
        assert got[field].tobytes() == rows[field].tobytes()
    assert got.dtype == nat.ROW_DT and rows["a"][0] == _key([0, 1, 0, 1, 3])  # the input is left alone
    for s in range(5):
        for f in (0, 1, ag.n_alleles[s], ag.n_alleles[s] + 1, 4095):
            assert ag.map_field(s, f) == (int(ag.map_keys(np.array([f << (ABITS * s)], dtype=np.uint64))[0]) >> (ABITS * s)) & 0xFFF <= f


# ---- 4. a merge worked out by hand ---------------------------------------------------------------------------------------------
THREE = ("S,A*02:01+A*03:01,0.5,0\n"
         "S,A*02:06+A*03:01,0.3,1\n"
         "S,A*01:01+A*03:01,0.2,2\n")


def test_first_field_merges_rows():
    from grim import _native as nat
    from grim.marginal import reduce_records, reduce_umug_text

    want = "S,A*02+A*03,%r,0\nS,A*01+A*03,0.2,1\n" % (0.5 + 0.3)
    assert reduce_umug_text(THREE, ["A"]) == THREE  # nothing merges at the allele level
    assert reduce_umug_text(THREE, ["A"], groups="first_field") == want  # (0.5 + 0.3, in that order), then 0.2
    from grim.groups import AlleleGroups, regroup_umug_text

    assert regroup_umug_text(THREE, "first_field") == "S,A*02+A*03,0.5,0\nS,A*02+A*03,0.3,1\nS,A*01+A*03,0.2,2\n"
    ag = AlleleGroups.from_names(["A"], [["A*02:01", "A*03:01", "A*02:06", "A*01:01"]], "first_field")
    assert ag.names[0] == ["", "A*02", "A*03", "A*01"]
    rows = np.zeros(3, dtype=nat.ROW_DT)
    rows["a"], rows["b"], rows["prob"] = [1, 2, 4], [2, 3, 2], [0.5, 0.3, 0.2]  # the second row carries A*03:01 on haplotype a
    res = np.zeros(1, dtype=nat.RESULT_DT)
    res["n_rows"][0, nat.T_UMUG] = 3
    ores, orows, stats = reduce_records(res, rows, 1, 10, groups=ag)
    assert stats == {"subjects": 1, "rows_in": 3, "groups": 2, "rows_out": 2, "undefined": 0}
    assert [(int(r["a"]), int(r["b"]), float(r["prob"]).hex()) for r in orows[:2]] == [(1, 2, (0.5 + 0.3).hex()), (3, 2, (0.2).hex())]
    assert reduce_records(res, rows, 1, 10)[2]["groups"] == 3


def test_first_field_turns_a_mismatch_into_a_match():
    from grim.match import match_umug_text

    patient = "P,A*02:01+A*03:01,1.0,0\n"
    donor = "D,A*02:06+A*03:01,1.0,0\n"
    (H, L), = match_umug_text(patient, donor, ["A"])[2][0]
    assert H == [0.0, 1.0, 0.0] and L == {"A": 0.0}
    (H, L), = match_umug_text(patient, donor, ["A"], groups={"A": "first_field"})[2][0]
    assert H == [1.0, 0.0, 0.0] and L == {"A": 1.0}


# ---- 5. record twins against text twins on regrouped goldens ---------------------------------------------------------------
def _records(text):
    """.umug text -> (res, rows, allele names per slot in id order): ids from a table built from the text, slot by locus name;
    in every second row the alleles of its first locus change haplotypes, and bit 60 is set here and there"""
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
    return r, np.array(rows, dtype=nat.ROW_DT), [list(d) for d in ids]


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


_parsed = {}


def _golden(scenario):
    if scenario not in _parsed:
        text = _umug(scenario)
        _parsed[scenario] = (text,) + _records(text) + ([l.split(",")[0] for l in text.splitlines() if l.endswith(",0")],)
    return _parsed[scenario]


def _hex(rec):
    return [float(x).hex() for x in np.frombuffer(rec.tobytes(), dtype="<f8")]


def _first_subjects(text, n):
    out, seen = [], 0
    for line in text.splitlines(keepends=True):
        seen += line.rstrip("\n").endswith(",0")
        if seen > n:
            break
        out.append(line)
    return "".join(out)


@pytest.mark.parametrize("spec", list(SPECS))
@pytest.mark.parametrize("scenario", GOLDENS)
def test_reduce_records_with_groups_equals_the_text_twin_on_regrouped_text(scenario, spec):
    from grim.groups import AlleleGroups, regroup_umug_text
    from grim.marginal import keep_mask, reduce_records, reduce_umug_text

    text, res, rows, alleles, sids = _golden(scenario)
    which, spec = spec, SPECS[spec](alleles)
    ag = AlleleGroups.from_names(ALL5, alleles, spec)
    regrouped = regroup_umug_text(text, spec)
    assert regrouped != text and len(regrouped.splitlines()) == len(text.splitlines())
    merged = False
    for keep in KEEPS:
        ores, orows, stats = reduce_records(res, rows, keep_mask(SLOT, keep), 10, groups=ag)
        want = reduce_umug_text(regrouped, keep, 10)
        assert _print(sids, ores, orows, ag.names) == want == reduce_umug_text(text, keep, 10, groups=spec)
        assert stats["rows_in"] == len(rows) and stats["undefined"] == 0
        merged |= stats["groups"] < reduce_records(res, rows, keep_mask(SLOT, keep), 10)[2]["groups"]
    if which == "first_field":  # not vacuous: some rows fell together that the allele level keeps apart
        assert merged


@pytest.mark.parametrize("spec", ["first_field", "a02_table"])
@pytest.mark.parametrize("scenario", GOLDENS)
def test_match_records_with_groups_equals_the_text_twin_on_regrouped_text(scenario, spec):
    from grim.groups import AlleleGroups, regroup_umug_text
    from grim.marginal import keep_mask
    from grim.match import match_records, match_umug_text, text_records_array

    text, res, rows, alleles, sids = _golden(scenario)
    which, spec = spec, SPECS[spec](alleles)
    ag = AlleleGroups.from_names(ALL5, alleles, spec)
    keep = ["A", "B", "DRB1"]
    mask = keep_mask(SLOT, keep)
    got = match_records(res[:6], rows, res, rows, mask, ag.n_alleles, groups=ag)
    regrouped = regroup_umug_text(text, spec)
    pid, did, want = match_umug_text(_first_subjects(regrouped, 6), regrouped, keep, loci=ALL5)
    assert len(pid) == 6 and len(did) == len(res) and got[3]["pairs"] == 6 * len(res) and got[3]["undefined"] == 0
    assert _hex(got[0]) == _hex(text_records_array(want, SLOT))
    assert _hex(text_records_array(match_umug_text(_first_subjects(text, 6), text, keep, groups=spec)[2], SLOT)) == _hex(got[0])
    plain = match_records(res[:6], rows, res, rows, mask, ag.n_alleles)
    if which == "first_field":  # not vacuous: probability mass moved towards fewer mismatches
        assert float(got[0]["mm"][:, :, :3].sum()) > float(plain[0]["mm"][:, :, :3].sum())
    with pytest.raises(ValueError):
        match_records(res[:6], rows, res, rows, mask, [4000] * 5, groups=ag)  # another dictionary than the groups'


@pytest.mark.parametrize("scenario", GOLDENS)
def test_identity_groups_reproduce_the_ungrouped_twins(scenario):
    from grim.groups import AlleleGroups, regroup_umug_text
    from grim.marginal import keep_mask, reduce_records, reduce_umug_text
    from grim.match import match_records, match_umug_text
    from grim.search import search_records, search_umug_text

    text, res, rows, alleles, sids = _golden(scenario)
    assert regroup_umug_text(text, None) == text
    for spec in (None, {}, {"A": None}):
        ag = AlleleGroups.from_names(ALL5, alleles, spec)
        assert ag.watch_mask == 0 and ag.map_records(rows).tobytes() == rows.tobytes()
    mask = keep_mask(SLOT, ["A", "B", "DRB1"])
    a, b = reduce_records(res, rows, mask, 10, groups=ag), reduce_records(res, rows, mask, 10)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
    assert reduce_umug_text(text, ["A", "B"], groups={}) == reduce_umug_text(text, ["A", "B"])
    a, b = match_records(res[:4], rows, res, rows, mask, ag.n_alleles, groups=ag), match_records(res[:4], rows, res, rows, mask, ag.n_alleles)
    assert a[0].tobytes() == b[0].tobytes() and list(a[1]) == list(b[1]) and list(a[2]) == list(b[2]) and a[3] == b[3]
    few = _first_subjects(text, 4)
    assert match_umug_text(few, text, ["A", "B"], groups={}) == match_umug_text(few, text, ["A", "B"])
    runs = [(res, rows, np.arange(len(res), dtype=np.uint32))]
    a = search_records(res[:4], rows, runs, mask, ag.n_alleles, 5, 0.0, groups=ag)
    b = search_records(res[:4], rows, runs, mask, ag.n_alleles, 5, 0.0)
    assert a[0].tobytes() == b[0].tobytes() and list(a[1]) == list(b[1]) and a[2] == b[2]
    assert search_umug_text(few, text, ["A", "B"], 5, groups={}) == search_umug_text(few, text, ["A", "B"], 5)


def test_flags_twin():
    from grim import _native as nat
    from grim.groups import AlleleGroups

    ag = AlleleGroups.from_names(ALL5, [["A*02:01", "A*02:06"], ["B*07:02"], [], [], ["DRB1*15:01"]], {"A": "first_field"})
    assert ag.watch_mask == 1
    rows = np.zeros(5, dtype=nat.ROW_DT)
    rows["a"] = [_key([1, 1, 0, 0, 1]), _key([3, 1, 0, 0, 1]), _key([1, 2, 0, 0, 1]), _key([3, 1, 0, 0, 1]), _key([3, 1, 0, 0, 1])]
    rows["b"] = rows["a"]
    res = np.zeros(5, dtype=nat.RESULT_DT)
    res["row_off"][:, 0], res["n_rows"][:, 0] = [0, 1, 2, 3, 4], [1, 1, 1, 1, 7]
    res["status"][3] = nat.ST_MISS
    # known alleles; private in the watched slot; private in an identity slot; private but not OK; private but past the rows
    assert list(ag.flags(res, rows, 0b10011)) == [0, nat.GROUPS_PRIVATE, 0, 0, 0]
    assert list(ag.flags(res, rows, 0b10010)) == [0, 0, 0, 0, 0]  # slot 0 is not kept


# ---- 6. the library -----------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_new_symbols():
    import __graft_entry__ as ge
    from grim import _native

    ge.build()
    L = _native.lib()
    for name in ("grim_groups_create", "grim_groups_free", "grim_groups_map_records", "grim_groups_kernel_ms", "grim_marginal_set_groups",
                 "grim_match_set_groups", "grim_search_set_groups", "grim_marginal_flags"):
        assert name in _native.EXPORTS and getattr(L, name) is not None
