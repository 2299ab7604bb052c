"""Mismatch direction and per-locus grades on the device (csrc/grim_match.h through grim/match.py and grim/search.py,
DESIGN 4.12): the smallest shapes at which the pair kernel can go wrong, through the host-records door against the record
twin, bit for bit; what the directions and the graded record owe each other; reuse; refusals; a group map; the search; one
golden end to end against the text twin."""
import os

import numpy as np
import pytest

import harness

pytestmark = pytest.mark.gpu

LOCI = ["A", "B", "C", "DQB1", "DRB1"]
MASKS = [0b10000, 0b10011, 0b11111]
COMBOS = [("gvh", False), ("hvg", False), ("either", True), ("gvh", True), ("hvg", True)]
ABITS = 12
N_ALLELES = [4050] * 5  # dictionary sizes of the synthetic subjects: ids above are private
PRIVATE_ID = 4060
DONOR_SIZES = [1, 63, 64, 65, 129]  # one chunk of 64 donor rows, the chunk's edge, a second partial chunk
PATIENT_SIZES = [1, 2, 65]
CASES = ["homhet", "untyped", "swapped", "distinct"]


def _key(fields):
    k = 0
    for s, f in enumerate(fields):
        k |= int(f) << (ABITS * s)
    return k


def _subject(case, n, shift=0):
    """n rows (a, b, p) of one subject over a small pool of alleles: rows of different subjects share some alleles and not
    others, so that a locus has 0, 1 and 2 mismatches and the two directions differ; probabilities span 1e-1 to 1e-20"""
    rows = []
    for k in range(n):
        z = k + shift
        p = [0.1, 0.2, 0.3][k % 3] * 10.0 ** -((k * 7) % 20)
        fa, fb = [5, 6, 20 + z % 6, 3, 7], [8, 9, 3, 20 + z % 5, 10]
        if case == "homhet":  # homozygous and heterozygous rows in turn, at slots 0, 1 and 4
            if z % 2 == 0:
                fb[0] = fa[0]
            if z % 3 == 0:
                fa[4] = fb[4]
            if z % 5 == 0:
                fb[1] = fa[1]
        elif case == "untyped":  # kept slots untyped in some rows, homozygous in others
            if z % 3 == 0:
                fa[4] = fb[4] = 0
            if z % 4 == 1:
                fa[0] = fb[0] = 0
            if z % 5 == 2:
                fb[4] = fa[4]
        elif case == "swapped":  # rows 2i and 2i+1: one genotype whose alleles at slots 0 and 4 changed haplotypes
            fa[0], fb[1] = 30 + (z // 2) % 3, 9 + (z // 2) % 2
            if z % 2:
                fa[0], fb[0] = fb[0], fa[0]
                fa[4], fb[4] = fb[4], fa[4]
        else:  # distinct
            fa[0], fb[4] = 30 + z % 7, 40 + z % 3
        rows.append((_key(fa) | ((k % 2) << 60), _key(fb), p))
    return rows


def _batch(subjects):
    """[(status, rows)] -> (res, rows) records, rows back to back"""
    from grim import _native as nat

    res = np.zeros(len(subjects), dtype=nat.RESULT_DT)
    flat = []
    for i, (status, rows) in enumerate(subjects):
        res[i]["status"], res[i]["plan"] = status, ord("abc"[i % 3])
        res[i]["row_off"][nat.T_UMUG], res[i]["n_rows"][nat.T_UMUG] = len(flat), len(rows)
        flat += rows
    out = np.zeros(len(flat), dtype=nat.ROW_DT)
    for k, (a, b, p) in enumerate(flat):
        out[k] = (a, b, p, 3, 4)
    return res, out


def _specials(nat, subjects):
    """among the others: a subject with a private id in a slot every mask keeps, one whose status is not OK, one whose
    probabilities add up to 0"""
    a, b, p = _subject("homhet", 3)[-1]
    private = _subject("homhet", 3)[:-1] + [((a & ~(0xFFF << (ABITS * 4))) | (PRIVATE_ID << (ABITS * 4)), b, p)]
    subjects.insert(1, (nat.ST_OK, private))
    subjects.insert(3, (nat.ST_MISS, _subject("distinct", 5)))
    subjects.insert(4, (nat.ST_OK, [(_key([5, 6, 7, 8, 9]), _key([5, 6, 7, 8, 9]), 0.0)]))
    return subjects


@pytest.fixture(scope="module")
def shapes():
    from grim import _native as nat

    patients = [(nat.ST_OK, _subject(CASES[i % 4], n, shift=1)) for i, n in enumerate(PATIENT_SIZES)]
    patients += [(nat.ST_OK, _subject(case, 3, shift=2)) for case in CASES]
    donors = [(nat.ST_OK, _subject(CASES[i % 4], n)) for i, n in enumerate(DONOR_SIZES)]
    donors += [(nat.ST_OK, _subject(case, n, shift=3)) for case, n in zip(CASES, (65, 2, 64, 1))]
    return _batch(_specials(nat, patients)) + _batch(_specials(nat, donors))


@pytest.fixture(scope="module")
def ctx():
    from grim import _native as nat

    return nat.default_context(None)


_want, _got = {}, {}


def _twin(shapes, mask, direction, graded):
    """the record twin's answer, computed once, shared and left alone"""
    from grim.match import match_records

    at = (mask, direction, graded)
    if at not in _want:
        _want[at] = match_records(*shapes, mask, N_ALLELES, direction=direction, graded=graded)
    return _want[at]


def _run(ctx, pres, prows, dres, drows, mask, direction, graded, groups=None):
    from grim import _native as nat
    from grim.match import direction_code

    mt = nat.Matcher(ctx, mask, N_ALLELES, direction_code(direction), graded)
    try:
        assert mt.direction() == direction_code(direction) and mt.graded() == graded
        if groups is not None:
            dev = nat.Groups.of(ctx, groups)
            try:
                mt.set_groups(dev)
            finally:
                dev.close()
        mt.set_patients(pres, prows)
        mt.run_records(dres, drows)
        assert mt.kernel_ms() > 0.0
        return (mt.results_graded() if graded else mt.results()) + (mt.stats(),)
    finally:
        mt.close()


def _device(ctx, shapes, mask, direction, graded):
    """the device's answer, computed once, shared and left alone"""
    at = (mask, direction, graded)
    if at not in _got:
        _got[at] = _run(ctx, *shapes, mask, direction, graded)
    return _got[at]


def _hex(rec):
    return [float(x).hex() for x in np.frombuffer(rec.tobytes(), dtype="<f8")]


def _same(got, want):
    (grec, gpf, gdf, gstats), (wrec, wpf, wdf, wstats) = got, want
    assert list(gpf) == list(wpf) and list(gdf) == list(wdf)
    assert gstats == wstats
    assert grec.shape == wrec.shape and grec.dtype == wrec.dtype
    assert _hex(grec) == _hex(wrec)
    assert grec.tobytes() == wrec.tobytes()


# ---- 1. exact shapes through the host-records door ----------------------------------------------------------------------
@pytest.mark.parametrize("direction,graded", COMBOS, ids=["%s%s" % (d, "~graded" if g else "") for d, g in COMBOS])
@pytest.mark.parametrize("mask", MASKS, ids=[bin(m) for m in MASKS])
def test_shapes_bit_for_bit(ctx, shapes, mask, direction, graded):
    from grim import _native as nat

    want = _twin(shapes, mask, direction, graded)
    assert want[0].dtype == (nat.MATCH_GRADE_DT if graded else nat.MATCH_DT)
    V, P = nat.MATCH_VALID, nat.MATCH_PRIVATE
    assert list(want[1][:5]) == [V, V | P, V, 0, 0] and list(want[2][:5]) == [V, V | P, V, 0, 0]  # ok, private, ok, MISS, total 0
    n_p, n_d = len(PATIENT_SIZES) + 4, len(DONOR_SIZES) + 4
    assert want[3]["pairs"] == n_p * n_d and want[3]["patients_private"] == 1 and want[3]["donors_private"] == 1
    _same(_device(ctx, shapes, mask, direction, graded), want)


@pytest.mark.parametrize("mask", MASKS, ids=[bin(m) for m in MASKS])
def test_the_shapes_are_not_vacuous(shapes, mask):
    """on the twin: the directions differ from each other and from `either`, and every grade occurs"""
    either, gvh, hvg = (_twin(shapes, mask, d, False)[0] for d in ("either", "gvh", "hvg"))
    n_p, n_d = either.shape
    assert any(gvh[p, d].tobytes() != either[p, d].tobytes() for p in range(n_p) for d in range(n_d))
    assert any(gvh[p, d].tobytes() != hvg[p, d].tobytes() for p in range(n_p) for d in range(n_d))
    for direction in ("either", "gvh", "hvg"):
        grade = _twin(shapes, mask, direction, True)[0]["grade"]
        assert (grade[:, :, :, 1] != 0.0).any() and (grade[:, :, :, 2] != 0.0).any()
        assert ((grade > 0.0) & (grade < 1.0)).any()  # and not only whole subjects: sums of several rows' products


@pytest.mark.parametrize("mask", MASKS, ids=[bin(m) for m in MASKS])
def test_what_the_device_results_owe_each_other(ctx, shapes, mask):
    """on the device's own records: the directed mm[0] is never below either's, exactly; graded records hold the ungraded
    bytes.  (either, ungraded) is the matcher grim_match_create makes: one of the six instances of mt_pair_kernel."""
    either = _device(ctx, shapes, mask, "either", False)[0]
    _same(_device(ctx, shapes, mask, "either", False), _twin(shapes, mask, "either", False))
    for direction in ("either", "gvh", "hvg"):
        plain, graded = _device(ctx, shapes, mask, direction, False)[0], _device(ctx, shapes, mask, direction, True)[0]
        assert (plain["mm"][:, :, 0] >= either["mm"][:, :, 0]).all()
        assert graded["mm"].tobytes() == plain["mm"].tobytes()
        assert np.ascontiguousarray(graded["grade"][:, :, :, 0]).tobytes() == plain["locus"].tobytes()


# ---- 2. reuse -----------------------------------------------------------------------------------------------------------
def test_reuse_of_a_graded_matcher(ctx):
    from grim import _native as nat

    mask = 0b10011
    mt = nat.Matcher(ctx, mask, N_ALLELES, nat.MATCH_DIR_GVH, True)
    try:
        pres, prows = _batch([(nat.ST_OK, _subject("swapped", 5)), (nat.ST_OK, _subject("homhet", 66, shift=1))])
        mt.set_patients(pres, prows)
        assert mt.patients() == 2 and mt.donors() == 0
        for sizes in ((130, 2, 65, 9), (3,)):  # a larger run, then a smaller one in the same buffers; the patients stay set
            dres, drows = _batch([(nat.ST_OK, _subject(CASES[(i + n) % 4], n, shift=i)) for i, n in enumerate(sizes)])
            mt.run_records(dres, drows)
            assert mt.donors() == len(sizes)
            _same(mt.results_graded() + (mt.stats(),), _run(ctx, pres, prows, dres, drows, mask, "gvh", True))
        pres, prows = _batch([(nat.ST_OK, _subject("untyped", 65)), (nat.ST_MISS, []), (nat.ST_OK, _subject("homhet", 1))])
        mt.set_patients(pres, prows)
        assert mt.patients() == 3 and mt.donors() == 0 and mt.stats() == dict.fromkeys(nat.MATCH_STATS, 0)
        mt.run_records(dres, drows)
        _same(mt.results_graded() + (mt.stats(),), _run(ctx, pres, prows, dres, drows, mask, "gvh", True))
    finally:
        mt.close()


# ---- 3. refusals --------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_matcher_empty(ctx):
    from grim import _native as nat

    pres, prows = _batch([(nat.ST_OK, _subject("homhet", 3)), (nat.ST_OK, _subject("untyped", 4))])
    dres, drows = _batch([(nat.ST_OK, _subject("swapped", 5, shift=1))])
    zero = dict.fromkeys(nat.MATCH_STATS, 0)
    graded = nat.Matcher(ctx, 0b10011, N_ALLELES, nat.MATCH_DIR_HVG, True)
    plain = nat.Matcher(ctx, 0b10011, N_ALLELES, nat.MATCH_DIR_HVG)
    try:
        for mt, right, wrong, text in ((graded, graded.results_graded, graded.results, "is graded"),
                                       (plain, plain.results, plain.results_graded, "is not graded")):
            mt.set_patients(pres, prows)
            mt.run_records(dres, drows)
            assert mt.donors() == 1 and mt.stats()["pairs"] == 2 and right()[0].shape == (2, 1)
            with pytest.raises(nat.NativeError, match=text):
                wrong()
            assert mt.donors() == 0 and mt.kernel_ms() == 0.0 and mt.stats() == zero and right()[0].size == 0
            assert mt.patients() == 2  # the patients stay
            mt.run_records(dres, drows)  # and the matcher still works
            assert mt.stats()["pairs"] == 2
    finally:
        graded.close()
        plain.close()
    with pytest.raises(nat.NativeError, match="direction"):
        nat.Matcher(ctx, 0b10011, N_ALLELES, 3)
    with pytest.raises(nat.NativeError, match="direction"):
        nat.Searcher(ctx, 0b10011, N_ALLELES, 4, 0.0, 3)
    nat.Matcher(ctx, 0b10011, N_ALLELES, 2, True).close()  # a refusal leaves the context usable


# ---- 4. a group map in front --------------------------------------------------------------------------------------------
def test_groups_compose_with_direction_and_grades(ctx, shapes):
    from grim.groups import AlleleGroups
    from grim.match import match_records

    names, spec = [], {}
    for s, G in enumerate([16, None, 1, None, 7]):  # allele f into group (f - 1) % G + 1; None: the alleles as they are
        spec[LOCI[s]] = None if G is None else "first_field"
        names.append(["%s*%04d:%04d" % (LOCI[s], f if G is None else (f - 1) % G + 1, f) for f in range(1, N_ALLELES[s] + 1)])
    ag = AlleleGroups.from_names(LOCI, names, spec)
    mask = 0b11111
    want = match_records(*shapes, mask, N_ALLELES, groups=ag, direction="hvg", graded=True)
    assert want[0].tobytes() != _twin(shapes, mask, "hvg", True)[0].tobytes() and want[3]["pairs"] > 0
    _same(_run(ctx, *shapes, mask, "hvg", True, groups=ag), want)


# ---- 5. the search ------------------------------------------------------------------------------------------------------
def test_search_under_a_direction(ctx, monkeypatch):
    from grim import _native as nat
    from grim.search import search_records

    monkeypatch.setenv("GRIM_SEARCH_TILE", "64")  # read when a search is created: 600 donors are three levels
    mask, top_n, min_p0 = 0b10011, 8, 1e-6
    pres, prows = _batch(_specials(nat, [(nat.ST_OK, _subject(CASES[i % 4], (1, 2, 65, 3, 2, 4)[i], shift=1)) for i in range(6)]))
    donors = []
    for i in range(597):  # most donors have a few rows; every 50th has one of the chunk-edge sizes
        n = DONOR_SIZES[1 + (i // 50) % 4] if i % 50 == 7 else 1 + i % 4
        donors.append((nat.ST_OK, _subject(CASES[(i + i // 4) % 4], n, shift=i % 11)))
    dres, drows = _batch(_specials(nat, donors))
    assert len(pres) == 9 and len(dres) == 600
    ids = (np.arange(600, dtype=np.uint32) * 7 + 3) % 600 + 1000  # distinct, not in donor order
    want = search_records(pres, prows, [(dres, drows, ids)], mask, N_ALLELES, top_n, min_p0, direction="gvh")
    either = search_records(pres, prows, [(dres, drows, ids)], mask, N_ALLELES, top_n, min_p0)
    assert any(want[0][p].tobytes() != either[0][p].tobytes() for p in range(9))
    assert want[2]["candidates"] > 9 * top_n and int(want[1].max()) == top_n
    sr = nat.Searcher(ctx, mask, N_ALLELES, top_n, min_p0, nat.MATCH_DIR_GVH)
    try:
        sr.set_patients(pres, prows)
        sr.run_records(dres, drows, ids)
        hits, n_hits = sr.results()
        assert list(n_hits) == list(want[1]) and sr.stats() == want[2]
        assert _hex(hits["rec"]) == _hex(want[0]["rec"])
        assert hits.tobytes() == want[0].tobytes()
    finally:
        sr.close()


# ---- 6. one golden end to end against the text twin ---------------------------------------------------------------------
def _imputation(scenario):
    """-> (Imputation on the scenario's graph and configuration, input lines, golden texts, em flag); no run"""
    from grim.imputation.impute import Imputation
    from grim.imputation.networkx_graph import Graph
    from grim.run_impute_def import load_config

    gname, conf, lines, exp, _, _ = harness.golden(scenario)
    work = harness.ensure_graph(gname)
    em = bool(conf.get("_em"))
    conf, cpath = harness._write_inputs(work, conf, lines, "match_dir_" + scenario)
    cwd = os.getcwd()
    os.chdir(work)
    try:
        cfg, _ = load_config(cpath)
        g = harness._graph_cache.get(gname)
        if g is None:
            g = harness._graph_cache[gname] = Graph(cfg).build_graph(cfg["node_file"], cfg["top_links_file"], cfg["edges_file"])
        imp = Imputation(g, cfg)
    finally:
        os.chdir(cwd)
    imp.on_unsupported = "raise"
    imp.quiet = True
    return imp, lines, exp, em


def _subjects_of(text):
    """.umug text -> [(id, its rows as text)]: a subject is the run of rows from one rank 0 to the next"""
    out = []
    for line in text.splitlines(keepends=True):
        if line.rstrip("\n").endswith(",0"):
            out.append([line.split(",")[0], ""])
        out[-1][1] += line
    return out


@pytest.fixture(scope="module")
def pop4():
    return _imputation("pop4_mixed")


@pytest.mark.parametrize("keep", [("A", "B", "C", "DQB1", "DRB1"), ("A", "B", "DRB1")], ids=["all5", "A~B~DRB1"])
def test_golden_match_equals_the_text_twin(pop4, keep):
    from grim import _native as nat
    from grim.match import match_probabilities, match_umug_text, text_records_array

    imp, lines, exp, em = pop4
    pok, dok, rec, stats = match_probabilities(imp, lines[:8], lines, imp.config, keep, em=em, direction="hvg", graded=True)
    subjects = _subjects_of(exp["umug"])
    assert rec.dtype == nat.MATCH_GRADE_DT and rec.shape == (8, len(lines)) and int(dok.sum()) == len(subjects)
    assert stats["undefined"] == 0 and stats["kernel_ms"] > 0.0 and stats["pairs"] + stats["host_pairs"] == int(pok.sum()) * len(subjects)
    patient_text = "".join(t for _, t in subjects[:int(pok.sum())])
    want = match_umug_text(patient_text, exp["umug"], keep, direction="hvg", graded=True)[2]
    want = text_records_array(want, imp.netGraph.locus_slot, graded=True)
    got = rec[np.flatnonzero(pok)][:, np.flatnonzero(dok)]
    assert got.shape == want.shape
    assert _hex(got) == _hex(want)
    plain = text_records_array(match_umug_text(patient_text, exp["umug"], keep)[2], imp.netGraph.locus_slot)
    assert want["mm"].tobytes() != plain["mm"].tobytes() and (want["grade"][:, :, :, 1] > 0.0).any()
