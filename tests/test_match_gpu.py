"""The device match probabilities (csrc/grim_match.h through grim/match.py): exact shapes through the host-records door
against the record twin, bit for bit; reuse of a matcher; the goldens against the text twin, whatever the batch cuts; the
refusals; the existing block path next to a matcher."""
import os

import numpy as np
import pytest

import harness

pytestmark = pytest.mark.gpu

SCENARIOS = ["pop4_mixed", "cau_mixed", "bc_cau_default_map", "pop4_planc", "cau_edge", "cau_mr_res1000"]
KEEPS = [("A", "B", "C", "DQB1", "DRB1"), ("A", "B", "DRB1"), ("DRB1",)]
MASKS = [0b10011, 0b10000, 0b11111]
ABITS = 12
N_ALLELES = [4050] * 5  # dictionary sizes of the synthetic subjects: ids above are private
PRIVATE_ID = 4060

_imps = {}


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
    conf, cpath = harness._write_inputs(work, conf, lines, "match_" + scenario)
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
    _imps[scenario] = (imp, lines, exp, em)
    return _imps[scenario]


# ---- 1. exact shapes through the host-records door ----------------------------------------------------------------------
DONOR_SIZES = [1, 63, 64, 65, 128, 129, 257, 1000]  # one chunk of 64 donor rows, the chunk boundary, many chunks
PATIENT_SIZES = [1, 2, 65, 257]
CASES = ["same", "distinct", "swapped", "homhet", "untyped"]


def _key(fields):
    k = 0
    for s, f in enumerate(fields):
        k |= int(f) << (ABITS * s)
    return k


def _subject(case, n, shift=0):
    """n rows (a, b, p) of one subject over a small pool of alleles, so that rows of different subjects match at some loci and
    not at others; slots 0, 1, 4 are the ones the proper subsets keep; probabilities span 1e-1 to 1e-20"""
    rows = []
    for k in range(n):
        noise = (k + shift) % 6 + 20
        p = [0.1, 0.2, 0.3][k % 3] * 10.0 ** -((k * 7) % 20)
        fa, fb = [5, 6, noise, 3, 7], [8, 9, 3, noise, 10]
        if case == "same":  # one genotype on slots 0, 1, 4 throughout
            pass
        elif case == "distinct":
            fa[0], fb[4] = 30 + (k + shift) % 4000, 40 + k % 3
        elif case == "swapped":  # rows 2i and 2i+1: one genotype whose alleles at slot 0 (and at slot 4) changed haplotypes
            fa[0], fb[1] = 30 + ((k // 2) + shift) % 5, 9 + (k // 2) % 2
            if k % 2:
                fa[0], fb[0] = fb[0], fa[0]
                fa[4], fb[4] = fb[4], fa[4]
        elif case == "homhet":  # homozygous and heterozygous rows in turn, at slot 0 and at slot 4
            if k % 2 == 0:
                fb[0] = fa[0]
            if k % 3 == 0:
                fa[4] = fb[4]
        else:  # untyped: slot 4 (kept) untyped in every third row, slot 2 (outside the proper subsets) in every fourth
            if k % 3 == 0:
                fa[4] = fb[4] = 0
            if k % 4 == 0:
                fa[2] = fb[2] = 0
        rows.append((_key(fa) | ((k % 2) << 60), _key(fb) | (((k // 2) % 2) << 60), p))
    return rows


def _batch(subjects, extra_rows=0):
    """[(status, rows)] -> (res, rows) records, rows back to back"""
    from grim import _native as nat

    res = np.zeros(len(subjects), dtype=nat.RESULT_DT)
    flat = []
    for i, (status, rows) in enumerate(subjects):
        res[i]["status"], res[i]["plan"] = status, ord("abc"[i % 3])
        res[i]["row_off"][nat.T_UMUG], res[i]["n_rows"][nat.T_UMUG] = len(flat), len(rows)
        res[i]["row_off"][nat.T_PMUG], res[i]["n_rows"][nat.T_PMUG] = len(flat), len(rows)
        flat += rows
    out = np.zeros(len(flat) + extra_rows, dtype=nat.ROW_DT)
    for k, (a, b, p) in enumerate(flat):
        out[k] = (a, b, p, 3, 4)
    return res, out


def _with_private(rows, slot):
    a, b, p = rows[-1]
    return rows[:-1] + [((a & ~(0xFFF << (ABITS * slot))) | (PRIVATE_ID << (ABITS * slot)), b, p)]


def _specials(nat, subjects):
    """the subjects that take no part, or only with some masks, among the others"""
    subjects.insert(1, (nat.ST_MISS, _subject("distinct", 5)))
    subjects.insert(3, (nat.ST_OK, []))
    subjects.insert(4, (nat.ST_OK, _with_private(_subject("same", 3), 1)))      # a private id in a kept slot: left out
    subjects.insert(6, (nat.ST_OK, _with_private(_subject("swapped", 66), 2)))  # outside 0b10011 and 0b10000: still computed
    subjects.insert(7, (nat.ST_OK, [(_key([5, 6, 7, 8, 9]), _key([5, 6, 7, 8, 9]), 0.0)]))  # a total of 0: not valid
    res, rows = _batch(subjects)
    m = len(rows)
    bad = np.zeros(2, dtype=nat.RESULT_DT)  # two subjects whose offsets point past the rows given: skipped, not read
    bad["row_off"][:, nat.T_UMUG] = [m - 1, m + 7]
    bad["n_rows"][:, nat.T_UMUG] = [5, 1]
    return np.concatenate([res[:2], bad[:1], res[2:], bad[1:]]), rows


@pytest.fixture(scope="module")
def shapes():
    from grim import _native as nat

    patients = [(nat.ST_OK, _subject(CASES[(i + 1) % 5], n)) for i, n in enumerate(PATIENT_SIZES)]
    patients += [(nat.ST_OK, _subject(case, 3, shift=1)) for case in CASES]
    donors = [(nat.ST_OK, _subject(CASES[i % 5], n, shift=2)) for i, n in enumerate(DONOR_SIZES)]
    donors += [(nat.ST_OK, _subject(case, n)) for case, n in zip(CASES, (65, 1, 64, 2, 63))]
    return _specials(nat, patients) + _specials(nat, donors)


@pytest.fixture(scope="module")
def ctx():
    from grim import _native as nat

    return nat.default_context(None)


_want = {}


def _twin(shapes, mask):
    """the record twin's answer, computed once per mask, shared and left alone"""
    from grim.match import match_records

    if mask not in _want:
        _want[mask] = match_records(*shapes, mask, N_ALLELES)
    return _want[mask]


def _same(got, want):
    (grec, gpf, gdf, gstats), (wrec, wpf, wdf, wstats) = got, want
    assert list(gpf) == list(wpf) and list(gdf) == list(wdf)
    assert gstats == wstats
    assert grec.shape == wrec.shape
    assert [float(x).hex() for x in np.frombuffer(grec.tobytes(), dtype="<f8")] == [float(x).hex() for x in np.frombuffer(wrec.tobytes(), dtype="<f8")]
    assert grec.tobytes() == wrec.tobytes()


def _run_records(ctx, pres, prows, dres, drows, mask):
    from grim import _native as nat

    mt = nat.Matcher(ctx, mask, N_ALLELES)
    try:
        mt.set_patients(pres, prows)
        mt.run_records(dres, drows)
        assert mt.kernel_ms() > 0.0
        return mt.results() + (mt.stats(),)
    finally:
        mt.close()


@pytest.mark.parametrize("mask", MASKS, ids=[bin(m) for m in MASKS])
def test_shapes_bit_for_bit(ctx, shapes, mask):
    from grim import _native as nat

    want = _twin(shapes, mask)
    V, P = nat.MATCH_VALID, nat.MATCH_PRIVATE
    n_p, n_d = len(PATIENT_SIZES) + 5, len(DONOR_SIZES) + 5
    if mask == 0b10011:  # what the subjects were built for
        assert want[3]["patients_valid"] == n_p + 2 and want[3]["donors_valid"] == n_d + 2
        assert want[3]["patients_private"] == 1 and want[3]["donors_private"] == 1 and want[3]["undefined"] == 0
        assert want[3]["pairs"] == (n_p + 1) * (n_d + 1)
        assert list(want[1][:9]) == [V, 0, 0, V, 0, V | P, V, V, 0]  # ok, MISS, past the rows, ok, no rows, private, private outside K, ok, total 0
        mm = want[0]["mm"].reshape(-1, 11)
        assert np.count_nonzero(((mm > 0.0) & (mm < 1.0)).any(axis=1)) >= len(mm) // 4  # zero records included
    if mask == 0b11111:
        assert want[3]["patients_private"] == 2 and want[3]["pairs"] == n_p * n_d
    _same(_run_records(ctx, *shapes, mask), want)


def test_an_undefined_row_is_flagged_and_counted(ctx):
    from grim import _native as nat
    from grim.match import match_records

    good = _subject("distinct", 70)
    bad = list(good)
    a, b, p = bad[66]
    bad[66] = (a & ~(0xFFF << (ABITS * 2)), b, p)  # slot 2 typed on one haplotype only
    pres, prows = _batch([(nat.ST_OK, good), (nat.ST_OK, bad)])
    dres, drows = _batch([(nat.ST_OK, bad), (nat.ST_OK, good), (nat.ST_OK, bad)])
    want = match_records(pres, prows, dres, drows, 0b10011, N_ALLELES)
    assert want[3]["undefined"] == 3 and list(want[2]) == [nat.MATCH_VALID | nat.MATCH_UNDEFINED, nat.MATCH_VALID, nat.MATCH_VALID | nat.MATCH_UNDEFINED]
    _same(_run_records(ctx, pres, prows, dres, drows, 0b10011), want)


# ---- 2. reuse -----------------------------------------------------------------------------------------------------------
def test_reuse_of_a_matcher(ctx):
    from grim import _native as nat
    from grim.match import match_records

    mask = 0b10011
    mt = nat.Matcher(ctx, mask, N_ALLELES)
    try:
        pres, prows = _batch([(nat.ST_OK, _subject("swapped", 5)), (nat.ST_OK, _subject("homhet", 70))])
        mt.set_patients(pres, prows)
        assert mt.patients() == 2 and mt.donors() == 0
        for sizes in ((3,), (130, 2, 65, 9), (1, 1)):  # grows, then shrinks again; the patients stay set
            dres, drows = _batch([(nat.ST_OK, _subject(CASES[(i + n) % 5], n, shift=i)) for i, n in enumerate(sizes)])
            mt.run_records(dres, drows)
            assert mt.donors() == len(sizes)
            _same(mt.results() + (mt.stats(),), match_records(pres, prows, dres, drows, mask, N_ALLELES))
        pres, prows = _batch([(nat.ST_OK, _subject("untyped", 66)), (nat.ST_MISS, []), (nat.ST_OK, _subject("same", 1))])
        mt.set_patients(pres, prows)
        assert mt.patients() == 3 and mt.donors() == 0 and mt.stats() == dict.fromkeys(nat.MATCH_STATS, 0)
        mt.run_records(dres, drows)
        _same(mt.results() + (mt.stats(),), match_records(pres, prows, dres, drows, mask, N_ALLELES))
        # no donors: nothing runs
        mt.run_records(dres[:0], drows[:0])
        rec, pf, df = mt.results()
        assert mt.donors() == 0 and rec.shape == (3, 0) and len(df) == 0 and mt.patients() == 3
        assert mt.stats() == dict.fromkeys(nat.MATCH_STATS, 0) and mt.kernel_ms() == 0.0
        assert list(pf) == list(match_records(pres, prows, dres[:0], drows[:0], mask, N_ALLELES)[1])
    finally:
        mt.close()


# ---- 3. goldens against the text twin -----------------------------------------------------------------------------------
def _subjects_of(text):
    """.umug text -> [(id, its rows as text)]: a subject is the run of rows from one rank 0 to the next"""
    out = []
    for line in text.splitlines(keepends=True):
        if line.rstrip("\n").endswith(",0"):
            out.append([line.split(",")[0], ""])
        out[-1][1] += line
    return out


@pytest.mark.parametrize("keep", KEEPS, ids=["~".join(k) for k in KEEPS])
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_golden_match_equals_the_text_twin(scenario, keep):
    from grim.match import line_id, match_probabilities, match_umug_text, text_records_array

    imp, lines, exp, em = _imputation(scenario)
    pok, dok, rec, stats = match_probabilities(imp, lines[:8], lines, imp.config, keep, em=em)
    subjects = _subjects_of(exp["umug"])
    assert rec.shape == (8, len(lines)) and len(pok) == 8 and len(dok) == len(lines)
    assert int(dok.sum()) == len(subjects) and list(pok) == list(dok[:8])
    assert [line_id(lines[i]) for i in np.flatnonzero(dok)] == [sid for sid, _ in subjects]
    assert stats["undefined"] == 0 and stats["kernel_ms"] > 0.0
    assert stats["donors_valid"] == len(subjects) and stats["patients_valid"] == int(pok.sum())
    patient_text = "".join(t for _, t in subjects[:int(pok.sum())])
    pid, did, want = match_umug_text(patient_text, exp["umug"], keep)
    want = text_records_array(want, imp.netGraph.locus_slot)
    got = rec[np.flatnonzero(pok)][:, np.flatnonzero(dok)]
    assert got.shape == want.shape
    assert [float(x).hex() for x in np.frombuffer(got.tobytes(), dtype="<f8")] == [float(x).hex() for x in np.frombuffer(want.tobytes(), dtype="<f8")]
    # lines without genotype rows: zero records
    assert not np.frombuffer(rec[~pok].tobytes(), dtype=np.uint8).any() and not np.frombuffer(rec[:, ~dok].tobytes(), dtype=np.uint8).any()
    assert stats["pairs"] + stats["host_pairs"] == int(pok.sum()) * len(subjects)
    if scenario == "pop4_planc" and "A" in keep:  # its genotype rows print alleles the graph has never seen (A*98:01)
        assert stats["host_pairs"] > 0 and stats["donors_private"] > 0


# ---- 4. batch cuts ------------------------------------------------------------------------------------------------------
def test_batch_cuts_are_invisible():
    from grim.match import match_probabilities

    imp, lines, exp, em = _imputation("pop4_mixed")
    keep = ("A", "B", "DRB1")
    whole = match_probabilities(imp, lines[:8], lines, imp.config, keep, block_lines=65536, em=em)
    assert whole[3]["blocks"] == 1
    for block in (1, 7):
        pok, dok, rec, stats = match_probabilities(imp, lines[:8], lines, imp.config, keep, block_lines=block, em=em)
        assert rec.tobytes() == whole[2].tobytes(), "block_lines=%d" % block
        assert list(pok) == list(whole[0]) and list(dok) == list(whole[1])
        assert 1 < stats["blocks"] <= -(-len(lines) // block)
        assert {k: stats[k] for k in ("pairs", "row_pairs", "donors_valid", "patients_valid")} == {k: whole[3][k] for k in ("pairs", "row_pairs", "donors_valid", "patients_valid")}


# ---- 5. refusals --------------------------------------------------------------------------------------------------------
def _empty(mt):
    from grim import _native as nat

    return mt.donors() == 0 and mt.kernel_ms() == 0.0 and mt.stats() == dict.fromkeys(nat.MATCH_STATS, 0) and mt.results()[0].size == 0


def test_refusals_leave_the_matcher_empty():
    from grim import _native as nat

    imp, lines, _, _ = _imputation("cau_edge")
    g = imp.netGraph
    ctx = nat.default_context(imp.device)
    L = nat.lib()
    n_alleles = [g.adict.count(s) for s in range(len(g.full_loci))]
    parsed = nat.Parsed(g.adict, ("\n".join(lines) + "\n").encode(), True)
    other = nat.Context(ctx.device)
    mt = nat.Matcher(ctx, 0b10011, n_alleles)
    none = nat.Matcher(ctx, 0, n_alleles)
    wide = nat.Matcher(ctx, 1 << len(g.full_loci), n_alleles)
    foreign = nat.Matcher(other, 0b10011, n_alleles)
    batches = []
    pres, prows = _batch([(nat.ST_OK, _subject("same", 3)), (nat.ST_OK, _subject("homhet", 4))])
    ptr = lambda a: a.ctypes.data_as(nat.C.c_void_p)
    try:
        priors = np.ones((max(1, len(parsed.races())), 1, 1))
        on = nat.DeviceBatch(ctx, g.device(ctx), imp._params(imp.config, True, False), parsed.subjects(), parsed.tokens(), priors)
        off = nat.DeviceBatch(ctx, g.device(ctx), imp._params(dict(imp.config, output_MUUG=False), True, False), parsed.subjects(),
                              parsed.tokens(), priors)
        batches += [on, off]
        on.run()
        off.run()
        # a run before any patients were set, through both doors
        assert L.grim_match_run(mt.h, on.h) < 0
        assert "no patients set" in ctx.error() and _empty(mt)
        assert L.grim_match_run_records(mt.h, ptr(pres), len(pres), ptr(prows), len(prows)) < 0
        assert "no patients set" in ctx.error() and _empty(mt)
        mt.set_patients(pres, prows)
        mt.run(on)
        assert mt.stats()["pairs"] > 0 and mt.donors() == on.n and not _empty(mt)
        # a batch built with output_MUUG off, after a run that worked
        assert L.grim_match_run(mt.h, off.h) < 0
        assert "out_muug" in ctx.error() and _empty(mt) and mt.patients() == 2
        with pytest.raises(nat.NativeError):
            mt.run(off)
        # a batch that has not run
        fresh = nat.DeviceBatch(ctx, g.device(ctx), imp._params(imp.config, True, False), parsed.subjects(), parsed.tokens(), priors)
        batches.append(fresh)
        mt.run(on)
        assert L.grim_match_run(mt.h, fresh.h) < 0
        assert "no finished run" in ctx.error() and _empty(mt)
        # a batch of another context
        assert L.grim_match_run(foreign.h, on.h) < 0
        assert "another context" in other.error() and _empty(foreign)
        # a keep_mask of 0, and one beyond the loci: the batch door, the records doors
        for bad in (none, wide):
            assert L.grim_match_run(bad.h, on.h) < 0
            assert "keep_mask" in ctx.error() and _empty(bad)
            assert L.grim_match_set_patients(bad.h, ptr(pres), len(pres), ptr(prows), len(prows)) < 0
            assert "keep_mask" in ctx.error() and _empty(bad) and bad.patients() == 0
            assert L.grim_match_run_records(bad.h, ptr(pres), len(pres), ptr(prows), len(prows)) < 0
            assert "keep_mask" in ctx.error() and _empty(bad)
        # patients x donors above GRIM_MATCH_MAX_PAIRS, after a run that worked
        mt.run(on)
        assert not _empty(mt)
        many = np.zeros(nat.MATCH_MAX_PAIRS // 2 + 1, dtype=nat.RESULT_DT)
        many["status"] = nat.ST_MISS
        assert L.grim_match_run_records(mt.h, ptr(many), len(many), None, 0) < 0
        assert "GRIM_MATCH_MAX_PAIRS" in ctx.error() and _empty(mt) and mt.patients() == 2
        mt.run(on)  # and the matcher still works
        assert mt.stats()["pairs"] > 0
    finally:
        for b in batches:
            b.close()
        for m in (mt, none, wide, foreign):
            m.close()
        other.close()
        parsed.close()


def test_unknown_locus_and_too_many_patients_raise_before_anything_runs():
    from grim import _native as nat
    from grim.match import match_probabilities

    imp, lines, _, em = _imputation("cau_edge")
    with pytest.raises(ValueError):
        match_probabilities(imp, lines[:2], lines, imp.config, ("A", "DPB1"), em=em)
    with pytest.raises(ValueError):
        match_probabilities(imp, lines[:2], lines, imp.config, (), em=em)
    with pytest.raises(ValueError):
        match_probabilities(imp, [lines[0]] * (nat.MATCH_MAX_PAIRS + 1), lines, imp.config, ("A",), em=em)


# ---- 6. the existing path next to a matcher -----------------------------------------------------------------------------
def test_block_path_texts_unchanged_next_to_a_matcher():
    from grim.match import match_probabilities

    imp, lines, exp, em = _imputation("pop4_mixed")
    before = imp.impute_lines_block(lines, imp.config, em=em)
    match_probabilities(imp, lines[:8], lines, imp.config, ("A", "B", "DRB1"), em=em)
    after = imp.impute_lines_block(lines, imp.config, em=em)
    assert before == after
    assert before["umug"] == exp["umug"]


def test_match_file_writes_the_computed_pairs(tmp_path):
    from grim.match import line_id, match_file, match_umug_text

    imp, lines, exp, em = _imputation("cau_edge")
    work = harness.ensure_graph(harness.golden("cau_edge")[0])  # where _imputation wrote the configuration and the input
    ppath = os.path.join(str(tmp_path), "patients.csv")
    with open(ppath, "w") as fh:
        fh.write("\n".join(lines[:3]) + "\n")
    out = os.path.join(str(tmp_path), "match.csv")
    cwd = os.getcwd()
    os.chdir(work)
    try:
        stats = match_file(os.path.join(work, "conf_match_cau_edge.json"), ppath, ("A", "B", "DRB1"), out, graph=imp.netGraph)
    finally:
        os.chdir(cwd)
    got = open(out).read().splitlines()
    assert got[0] == "patient_id,donor_id,mm0,mm1,mm2,mm3,mm4,mm5,mm6,A,B,DRB1"
    subjects = _subjects_of(exp["umug"])
    ids = [line_id(l) for l in lines[:3]]
    ptext = "".join(t for sid, t in subjects if sid in ids)
    pid, did, want = match_umug_text(ptext, exp["umug"], ("A", "B", "DRB1"))
    lines_want = ["%s,%s,%s" % (p, d, ",".join(repr(v) for v in H + [L[n] for n in ("A", "B", "DRB1")]))
                  for p, row in zip(pid, want) for d, (H, L) in zip(did, row)]
    assert got[1:] == lines_want and stats["pairs"] + stats["host_pairs"] == len(lines_want)
