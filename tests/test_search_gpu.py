"""The device donor search (csrc/grim_search.h through grim/search.py): shapes through the host-records door at the real tile
and, in a child process, at a tile of 64 (deep reduction trees), against the record twin, bit for bit; accumulation over runs;
the threshold; the public function against the text twin on the goldens, whatever the block cuts; the refusals; the existing
paths next to a search.

Run as a program (`--child <file>`) it is the child of the deep-tree test: it runs the deep cases on the device with whatever
GRIM_SEARCH_TILE its environment holds and writes the bytes it got to <file>."""
import os
import subprocess
import sys

import numpy as np
import pytest

import harness

pytestmark = pytest.mark.gpu

ABITS = 12
N_ALLELES = [4050] * 5  # dictionary sizes of the synthetic subjects: ids above are private
PRIVATE_ID = 4060
CASES = ["same", "distinct", "swapped", "homhet", "untyped"]
TILE = 2048
MASKS = [0b10011, 0b11111]


# ---- synthetic subjects (the builders of tests/test_match_gpu.py) ---------------------------------------------------------
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


N_SPECIALS = 7


def _specials(nat, subjects):
    """the subjects that take no part, or only with some masks, among the others: MISS, no rows, private in K, private outside
    0b10011, a total of 0, and two whose offsets point past the rows given"""
    subjects = list(subjects)
    subjects.insert(1, (nat.ST_MISS, _subject("distinct", 5)))
    subjects.insert(3, (nat.ST_OK, []))
    subjects.insert(4, (nat.ST_OK, _with_private(_subject("same", 3), 1)))
    subjects.insert(6, (nat.ST_OK, _with_private(_subject("swapped", 66), 2)))
    subjects.insert(7, (nat.ST_OK, [(_key([5, 6, 7, 8, 9]), _key([5, 6, 7, 8, 9]), 0.0)]))
    res, rows = _batch(subjects)
    m = len(rows)
    bad = np.zeros(2, dtype=nat.RESULT_DT)
    bad["row_off"][:, nat.T_UMUG] = [m - 1, m + 7]
    bad["n_rows"][:, nat.T_UMUG] = [5, 1]
    return np.concatenate([res[:2], bad[:1], res[2:], bad[1:]]), rows


def _patients():
    """2 patients with 3 and 66 rows, and the specials among them"""
    from grim import _native as nat

    return _specials(nat, [(nat.ST_OK, _subject("same", 3)), (nat.ST_OK, _subject("homhet", 66, shift=1))])


def _other_patients():
    from grim import _native as nat

    return _batch([(nat.ST_OK, _subject("untyped", 4)), (nat.ST_MISS, []), (nat.ST_OK, _subject("same", 2, shift=3))])


def _donors(n):
    """n donors in all -> (res, rows, ids): donors of 1-3 rows cycling over a pool of 5 genotypes, so that thousands of keys tie
    and ties cross tile boundaries, the specials among them (from 12 donors on); the ids are a fixed permutation of 32-bit
    numbers, not the positions"""
    from grim import _native as nat

    pool = [_subject(CASES[j], 1 + j % 3, shift=j) for j in range(5)]
    plain = n - N_SPECIALS if n >= 12 else n
    subjects = [(nat.ST_OK, pool[(i * 3) % 5]) for i in range(plain)]
    res, rows = _specials(nat, subjects) if plain < n else _batch(subjects)
    assert len(res) == n
    ids = ((np.arange(n, dtype=np.uint64) * 2654435761 + 12345) % (1 << 32)).astype(np.uint32)  # odd multiplier: a bijection
    return res, rows, ids


_twins = {}


def _twin(n, mask, top_n, min_p0=0.0):
    """the record twin's answer for the first-kind shapes, computed once per case, shared and left alone"""
    from grim.search import search_records

    at = (n, mask, top_n, min_p0)
    if at not in _twins:
        pres, prows = _patients()
        _twins[at] = search_records(pres, prows, [_donors(n)], mask, N_ALLELES, top_n, min_p0)
    return _twins[at]


def _hex(a):
    return [float(x).hex() for x in np.frombuffer(a.tobytes(), dtype="<f8")]


def _same(got, want):
    (ghits, gn, gstats), (whits, wn, wstats) = got, want
    assert list(gn) == list(wn)
    assert ghits.shape == whits.shape
    assert ghits["donor"].tolist() == whits["donor"].tolist()
    assert _hex(ghits["rec"]) == _hex(whits["rec"])
    assert ghits.tobytes() == whits.tobytes()
    if gstats is not None:
        assert gstats == wstats


def _device(ctx, patients, runs, mask, top_n, min_p0=0.0):
    from grim import _native as nat

    sr = nat.Searcher(ctx, mask, N_ALLELES, top_n, min_p0)
    try:
        sr.set_patients(*patients)
        for res, rows, ids in runs:
            sr.run_records(res, rows, ids)
        assert sr.select_ms() > 0.0 and sr.kernel_ms() > sr.select_ms()
        return sr.results() + (sr.stats(),)
    finally:
        sr.close()


@pytest.fixture(scope="module")
def ctx():
    from grim import _native as nat

    return nat.default_context(None)


# ---- 2. deep trees: the child runs first, before this process touches the GPU ------------------------------------------------
DEEP_TILE = 64
DEEP = [(top_n, n) for top_n in (8, 32) for n in (63, 64, 65, 129, 600)]  # 600 donors at a tile of 64: three levels
_deep = {}


def _child(path):
    from grim import _native as nat

    ctx = nat.default_context(None)
    tile = int(os.environ.get("GRIM_SEARCH_TILE", TILE))
    out = {}
    try:  # the tile is in force: 2 top_n must fit into it
        nat.Searcher(ctx, 0b10011, N_ALLELES, tile // 2 + 1).close()
        out["refused"] = np.zeros(1, dtype=np.uint8)
    except nat.NativeError as e:
        out["refused"] = np.ones(1, dtype=np.uint8) if "GRIM_SEARCH_TILE" in str(e) else np.zeros(1, dtype=np.uint8)
    for top_n, n in DEEP:
        hits, n_hits, stats = _device(ctx, _patients(), [_donors(n)], 0b10011, top_n)
        out["hits_%d_%d" % (top_n, n)] = np.frombuffer(hits.tobytes(), dtype=np.uint8)
        out["n_%d_%d" % (top_n, n)] = n_hits
        out["stats_%d_%d" % (top_n, n)] = np.array([stats[k] for k in nat.SEARCH_STATS], dtype=np.uint64)
    np.savez(path, **out)


@pytest.fixture(scope="module")
def deep(tmp_path_factory):
    """what a fresh child process with GRIM_SEARCH_TILE=64 got (the tile is read when a search is created)"""
    if not _deep:
        path = str(tmp_path_factory.mktemp("search_deep") / "deep.npz")
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        paths = [os.path.join(root, "tools"), os.path.join(root, "py-graph-imputation_amd"), os.environ.get("PYTHONPATH", "")]
        env = dict(os.environ, GRIM_SEARCH_TILE=str(DEEP_TILE), PYTHONPATH=os.pathsep.join(p for p in paths if p))
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=env, timeout=300,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert done.returncode == 0, done.stdout[-4000:]
        _deep.update(np.load(path))
    return _deep


@pytest.mark.parametrize("top_n,n", DEEP, ids=["top%d-D%d" % c for c in DEEP])
def test_deep_trees_bit_for_bit(deep, top_n, n):
    from grim import _native as nat

    assert deep["refused"][0] == 1
    want = _twin(n, 0b10011, top_n)
    hits = np.frombuffer(deep["hits_%d_%d" % (top_n, n)].tobytes(), dtype=nat.SEARCH_DT).reshape(-1, top_n)
    stats = {k: int(v) for k, v in zip(nat.SEARCH_STATS, deep["stats_%d_%d" % (top_n, n)])}
    assert want[2]["candidates"] > top_n
    _same((hits, deep["n_%d_%d" % (top_n, n)], stats), want)


# ---- 1. shapes at the real tile ---------------------------------------------------------------------------------------------
def _sizes(top_n):
    return [1, top_n - 1, top_n, top_n + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]


SHAPES = [(100, n) for n in _sizes(100)] + [(top_n, TILE + 1) for top_n in (1, 2, 256)]


@pytest.mark.parametrize("mask", MASKS, ids=[bin(m) for m in MASKS])
@pytest.mark.parametrize("top_n,n", SHAPES, ids=["top%d-D%d" % c for c in SHAPES])
def test_shapes_bit_for_bit(ctx, top_n, n, mask):
    from grim import _native as nat

    assert nat.SEARCH_TILE == TILE and nat.SEARCH_MAX_N == 256 and os.environ.get("GRIM_SEARCH_TILE") is None
    want = _twin(n, mask, top_n)
    if n >= 12:  # the specials are among the donors and the patients
        computed_p = 3 if mask == 0b10011 else 2  # the patient that is private outside 0b10011 takes part with it only
        assert want[2]["patients_private"] == (1 if mask == 0b10011 else 2) and want[2]["donors_private"] == (1 if mask == 0b10011 else 2)
        assert want[2]["pairs"] == computed_p * (n - N_SPECIALS + (1 if mask == 0b10011 else 0))
        assert want[2]["candidates"] == want[2]["pairs"]  # a threshold of 0.0 keeps every computed pair
        assert sorted(int(x) for x in want[1]) == [0] * (len(want[1]) - computed_p) + [min(top_n, want[2]["pairs"] // computed_p)] * computed_p
    got = _device(ctx, _patients(), [_donors(n)], mask, top_n)
    _same(got, want)
    if n > TILE:  # ties: hits whose mm[0] and mm[1] are those of the hit before them, in the order of their ids
        h = got[0][0][:int(got[1][0])]
        tied = [k for k in range(1, len(h)) if _hex(h[k]["rec"]["mm"][:2]) == _hex(h[k - 1]["rec"]["mm"][:2])]
        assert top_n < 3 or (tied and all(h[k]["donor"] > h[k - 1]["donor"] for k in tied))


# ---- 3. accumulation --------------------------------------------------------------------------------------------------------
def test_runs_accumulate_reset_and_new_patients(ctx):
    from grim import _native as nat
    from grim.search import search_records

    mask, top_n, n = 0b10011, 100, 2 * TILE + 1
    want = _twin(n, mask, top_n)
    res, rows, ids = _donors(n)
    cuts = [(0, 1), (1, TILE + 2), (TILE + 2, n)]
    sr = nat.Searcher(ctx, mask, N_ALLELES, top_n, 0.0)
    try:
        sr.set_patients(*_patients())
        empty = sr.results()
        assert not empty[1].any() and (empty[0]["donor"] == nat.SEARCH_NO_DONOR).all() and not any(sr.stats().values())
        sr.run_records(res, rows, ids)
        _same(sr.results() + (sr.stats(),), want)
        sr.reset()
        assert not sr.results()[1].any() and not any(sr.stats().values()) and sr.patients() == len(_patients()[0])
        for a, b in cuts:  # the rows stay one array: a run's subjects point into it
            sr.run_records(res[a:b], rows, ids[a:b])
            assert sr.donors() == b - a
        got = sr.results() + (sr.stats(),)
        _same(got[:2] + (None,), want)
        for k in ("donors_valid", "donors_private", "pairs", "row_pairs", "candidates"):
            assert got[2][k] == want[2][k]
        # a run with no donors changes nothing
        sr.run_records(res[:0], rows[:0], ids[:0])
        assert sr.donors() == 0 and sr.select_ms() == 0.0
        again = sr.results() + (sr.stats(),)
        assert again[0].tobytes() == got[0].tobytes() and list(again[1]) == list(got[1]) and again[2] == got[2]
        # the runs in another order, after a reset
        sr.reset()
        for a, b in reversed(cuts):
            sr.run_records(res[a:b], rows, ids[a:b])
        _same(sr.results() + (None,), want)
        # other patients: the lists start empty, the answer is theirs
        pres, prows = _other_patients()
        small = _donors(101)
        sr.set_patients(pres, prows)
        assert sr.patients() == 3 and not sr.results()[1].any() and not any(sr.stats().values())
        sr.run_records(*small)
        other = search_records(pres, prows, [small], mask, N_ALLELES, top_n, 0.0)
        assert list(other[1]) == [95, 0, 95]
        _same(sr.results() + (sr.stats(),), other)
    finally:
        sr.close()


# ---- 4. the threshold on the device -----------------------------------------------------------------------------------------
def test_threshold_on_the_device(ctx):
    mask, top_n, n = 0b10011, 100, 101
    base = _twin(n, mask, top_n)
    shown = sorted({float(h["rec"]["mm"][0]) for p in range(len(base[1])) for h in base[0][p, :int(base[1][p])]})
    assert shown[0] == 0.0 and len(shown) > 3
    present = shown[1]  # an mm0 the twin shows to be present: the smallest above 0.0
    counts = []
    for min_p0 in (present, float(np.nextafter(present, np.inf)), 2.0):
        want = _twin(n, mask, top_n, min_p0)
        got = _device(ctx, _patients(), [_donors(n)], mask, top_n, min_p0)
        assert got[2]["candidates"] == want[2]["candidates"]
        _same(got, want)
        counts.append(want[2]["candidates"])
    assert base[2]["candidates"] > counts[0] > counts[1] > counts[2] == 0


# ---- 5. the public function against the text twin ---------------------------------------------------------------------------
SCENARIOS = ["pop4_mixed", "cau_mixed", "pop4_planc"]
KEEPS = [("A", "B", "C", "DQB1", "DRB1"), ("A", "B", "DRB1")]
_imps = {}
_oks = {}


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
    conf, cpath = harness._write_inputs(work, conf, lines, "search_" + scenario)
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


def _ok_lines(scenario):
    """which lines have genotype rows, from match_probabilities: (patient_ok of lines[:8], donor_ok)"""
    from grim.match import match_probabilities

    if scenario not in _oks:
        imp, lines, exp, em = _imputation(scenario)
        pok, dok, _, _ = match_probabilities(imp, lines[:8], lines, imp.config, ("A", "B", "DRB1"), em=em)
        _oks[scenario] = (pok, dok)
    return _oks[scenario]


def _subjects_of(text):
    """.umug text -> [(id, its rows as text)]: a subject is the run of rows from one rank 0 to the next"""
    out = []
    for line in text.splitlines(keepends=True):
        if line.rstrip("\n").endswith(",0"):
            out.append([line.split(",")[0], ""])
        out[-1][1] += line
    return out


def _text_hits(scenario, keep, top_n, n_patients=8, min_p0=0.0):
    """the text twin's hits as the public function lays them out: SEARCH_DT[n_patients][top_n] by patient line, donor line
    numbers through donor_ok -> (hits, n_hits)"""
    from grim import _native as nat
    from grim.search import search_umug_text

    imp, lines, exp, em = _imputation(scenario)
    pok, dok = _ok_lines(scenario)
    subjects = _subjects_of(exp["umug"])
    assert int(dok.sum()) == len(subjects)
    ptext = "".join(t for _, t in subjects[:int(pok[:n_patients].sum())])
    pid, did, found = search_umug_text(ptext, exp["umug"], keep, top_n, min_p0)
    line_of_donor = np.flatnonzero(dok)
    slot = imp.netGraph.locus_slot
    hits = np.zeros((n_patients, top_n), dtype=nat.SEARCH_DT)
    hits["donor"] = nat.SEARCH_NO_DONOR
    n_hits = np.zeros(n_patients, dtype=np.uint32)
    for line, mine in zip(np.flatnonzero(pok[:n_patients]), found):
        n_hits[line] = len(mine)
        for k, (d, H, L) in enumerate(mine):
            hits[line, k]["donor"] = line_of_donor[d]
            hits[line, k]["rec"]["mm"][:len(H)] = H
            for name, v in L.items():
                hits[line, k]["rec"]["locus"][int(slot[name])] = v
    return hits, n_hits


@pytest.mark.parametrize("top_n", [1, 5, 256])
@pytest.mark.parametrize("keep", KEEPS, ids=["~".join(k) for k in KEEPS])
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_search_donors_equals_the_text_twin(scenario, keep, top_n):
    from grim.search import search_donors

    imp, lines, exp, em = _imputation(scenario)
    pok, hits, n_hits, stats = search_donors(imp, lines[:8], lines, imp.config, keep, top_n, em=em)
    want_hits, want_n = _text_hits(scenario, keep, top_n)
    assert list(pok) == list(_ok_lines(scenario)[0]) and hits.shape == (8, top_n)
    _same((hits, n_hits, None), (want_hits, want_n, None))
    n_donors = int(_ok_lines(scenario)[1].sum())
    assert stats["blocks"] == 1 and stats["kernel_ms"] > stats["select_ms"] > 0.0 and stats["undefined"] == 0
    assert stats["donors_valid"] == n_donors and stats["patients_valid"] == int(pok.sum())
    assert stats["pairs"] + stats["host_pairs"] == int(pok.sum()) * n_donors == stats["candidates"]
    assert stats["download_bytes"] % (top_n * 136 + 4) == 0 and int(pok.sum()) <= stats["download_bytes"] // (top_n * 136 + 4) <= 8
    if scenario == "pop4_planc" and "A" in keep:  # its genotype rows print alleles the graph has never seen (A*98:01)
        assert stats["host_pairs"] > 0 and stats["donors_private"] > 0
        if top_n == 256:
            # host-folded pairs among the hits, with lines[:8] as patients: the scenario has fewer donors than top_n and the
            # threshold is 0.0, so every patient's hits are all of its pairs, the host-folded ones among them
            assert n_donors < top_n and int(n_hits.sum()) == stats["pairs"] + stats["host_pairs"]
            assert list(n_hits[pok]) == [n_donors] * int(pok.sum())


def test_search_donors_threshold_and_arguments():
    from grim.search import search_donors

    imp, lines, exp, em = _imputation("pop4_planc")
    keep = ("A", "B", "DRB1")
    whole = _text_hits("pop4_planc", keep, 256)
    shown = sorted({float(h["rec"]["mm"][0]) for p in range(8) for h in whole[0][p, :int(whole[1][p])]})
    assert shown[0] == 0.0 and len(shown) > 2
    present = shown[1]  # the smallest mm0 above 0.0 that the twin shows: most of these pairs are folded on the host
    pok, hits, n_hits, stats = search_donors(imp, lines[:8], lines, imp.config, keep, 5, min_p0=present, em=em)
    _same((hits, n_hits, None), _text_hits("pop4_planc", keep, 5, min_p0=present) + (None,))
    assert stats["candidates"] < stats["pairs"] + stats["host_pairs"]
    for bad in (dict(top_n=0), dict(top_n=257), dict(top_n=1, min_p0=float("nan"))):
        with pytest.raises(ValueError):
            search_donors(imp, lines[:2], lines, imp.config, keep, em=em, **bad)
    with pytest.raises(ValueError):
        search_donors(imp, lines[:2], lines, imp.config, ("A", "DPB1"), 1, em=em)


# ---- 6. cuts are invisible --------------------------------------------------------------------------------------------------
def test_block_cuts_are_invisible():
    from grim.search import search_donors

    imp, lines, exp, em = _imputation("pop4_mixed")
    keep = ("A", "B", "DRB1")
    whole = search_donors(imp, lines[:8], lines, imp.config, keep, 5, block_lines=65536, em=em)
    assert whole[3]["blocks"] == 1 and whole[2].any()
    for block in (1, 7):
        pok, hits, n_hits, stats = search_donors(imp, lines[:8], lines, imp.config, keep, 5, block_lines=block, em=em)
        assert hits.tobytes() == whole[1].tobytes(), "block_lines=%d" % block
        assert list(n_hits) == list(whole[2]) and list(pok) == list(whole[0])
        assert 1 < stats["blocks"] <= -(-len(lines) // block)
        assert stats["download_bytes"] == whole[3]["download_bytes"]  # once, after the last block
        for k in ("pairs", "row_pairs", "donors_valid", "patients_valid", "candidates", "host_pairs"):
            assert stats[k] == whole[3][k]


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_add_nothing():
    from grim import _native as nat

    imp, lines, _, _ = _imputation("cau_edge")
    g = imp.netGraph
    ctx = nat.default_context(imp.device)
    L = nat._search_lib()
    n_alleles = [g.adict.count(s) for s in range(len(g.full_loci))]
    arr = (nat.C.c_uint32 * nat.MAXL)(*(n_alleles + [0] * (nat.MAXL - len(n_alleles))))
    ptr = lambda a: a.ctypes.data_as(nat.C.c_void_p)
    for top_n, min_p0, text in ((0, 0.0, "top_n"), (257, 0.0, "top_n"), (5, float("nan"), "min_p0")):
        assert not L.grim_search_create(ctx.h, 0b10011, arr, top_n, min_p0)
        assert text in ctx.error()
        with pytest.raises(nat.NativeError):
            nat.Searcher(ctx, 0b10011, n_alleles, top_n, min_p0)
    parsed = nat.Parsed(g.adict, ("\n".join(lines) + "\n").encode(), True)
    sr = nat.Searcher(ctx, 0b10011, n_alleles, 5, 0.0)
    batches = []
    pres, prows = _batch([(nat.ST_OK, _subject("same", 3)), (nat.ST_OK, _subject("homhet", 4))])
    try:
        priors = np.ones((max(1, len(parsed.races())), 1, 1))
        on = nat.DeviceBatch(ctx, g.device(ctx), imp._params(imp.config, True, False), parsed.subjects(), parsed.tokens(), priors)
        off = nat.DeviceBatch(ctx, g.device(ctx), imp._params(dict(imp.config, output_MUUG=False), True, False), parsed.subjects(),
                              parsed.tokens(), priors)
        batches += [on, off]
        on.run()
        off.run()
        ids = np.arange(on.n, dtype=np.uint32) + 1000
        # a run before any patients were set, through both doors
        assert L.grim_search_run(sr.h, on.h, ptr(ids)) == -3 and "no patients set" in ctx.error()
        assert L.grim_search_run_records(sr.h, ptr(pres), len(pres), ptr(prows), len(prows), ptr(ids)) == -3
        assert "no patients set" in ctx.error() and sr.patients() == 0 and sr.results()[0].shape == (0, 5)
        # the patients of the batch itself, and a run that works
        sr.set_patients(*on.results())
        sr.run(on, ids)
        before = sr.results() + (sr.stats(),)
        assert before[1].any() and before[2]["candidates"] > 0 and sr.donors() == on.n and sr.top_n() == 5
        assert set(before[0]["donor"][before[0]["donor"] != nat.SEARCH_NO_DONOR].tolist()) <= set(ids.tolist())

        def unchanged():
            now = sr.results() + (sr.stats(),)
            return now[0].tobytes() == before[0].tobytes() and list(now[1]) == list(before[1]) and now[2] == before[2]

        # no ids, through both doors
        assert L.grim_search_run(sr.h, on.h, None) == -3 and "donor_ids" in ctx.error() and unchanged()
        dres, drows = on.results()
        assert L.grim_search_run_records(sr.h, ptr(dres), len(dres), ptr(drows), len(drows), None) == -3
        assert "donor_ids" in ctx.error() and unchanged()
        # a batch built with output_MUUG off, after a run that worked: the matcher's refusal with its own text
        assert L.grim_search_run(sr.h, off.h, ptr(ids)) == -3 and "out_muug" in ctx.error() and unchanged()
        with pytest.raises(nat.NativeError):
            sr.run(off, ids)
        assert unchanged() and sr.patients() == on.n
        # the searcher still works: the same donors under other ids join the lists
        sr.run(on, ids + 5000)
        after = sr.results() + (sr.stats(),)
        assert after[2]["candidates"] == 2 * before[2]["candidates"] and (after[1] >= before[1]).all()
        assert (after[0]["donor"][after[0]["donor"] != nat.SEARCH_NO_DONOR] >= 5000).any()
    finally:
        for b in batches:
            b.close()
        sr.close()
        parsed.close()


# ---- 8. neighbours ----------------------------------------------------------------------------------------------------------
def test_match_and_block_paths_unchanged_next_to_a_search():
    from grim.match import match_probabilities
    from grim.search import search_donors

    imp, lines, exp, em = _imputation("pop4_mixed")
    keep = ("A", "B", "DRB1")
    texts = imp.impute_lines_block(lines, imp.config, em=em)
    before = match_probabilities(imp, lines[:8], lines, imp.config, keep, em=em)
    search_donors(imp, lines[:8], lines, imp.config, keep, 5, em=em)
    after = match_probabilities(imp, lines[:8], lines, imp.config, keep, em=em)
    assert before[2].tobytes() == after[2].tobytes() and list(before[0]) == list(after[0]) and list(before[1]) == list(after[1])
    assert imp.impute_lines_block(lines, imp.config, em=em) == texts
    assert texts["umug"] == exp["umug"]


# ---- 9. search_file ---------------------------------------------------------------------------------------------------------
def test_search_file_writes_the_hits(tmp_path):
    from grim.match import line_id
    from grim.search import search_file, search_umug_text

    imp, lines, exp, em = _imputation("cau_edge")
    work = harness.ensure_graph(harness.golden("cau_edge")[0])  # where _imputation wrote the configuration and the input
    ppath = os.path.join(str(tmp_path), "patients.csv")
    with open(ppath, "w") as fh:
        fh.write("\n".join(lines[:3]) + "\n")
    out = os.path.join(str(tmp_path), "search.csv")
    cwd = os.getcwd()
    os.chdir(work)
    try:
        stats = search_file(os.path.join(work, "conf_search_cau_edge.json"), ppath, ("A", "B", "DRB1"), out, 4, graph=imp.netGraph)
    finally:
        os.chdir(cwd)
    got = open(out).read().splitlines()
    assert got[0] == "patient_id,rank,donor_id,mm0,mm1,mm2,mm3,mm4,mm5,mm6,A,B,DRB1"
    subjects = _subjects_of(exp["umug"])
    ids = [line_id(l) for l in lines[:3]]
    ptext = "".join(t for sid, t in subjects if sid in ids)
    pid, did, hits = search_umug_text(ptext, exp["umug"], ("A", "B", "DRB1"), 4)
    want = ["%s,%d,%s,%s" % (p, k, did[d], ",".join(repr(v) for v in H + [L[n] for n in ("A", "B", "DRB1")]))
            for p, mine in zip(pid, hits) for k, (d, H, L) in enumerate(mine)]
    assert got[1:] == want and len(want) == 4 * len(pid) and stats["candidates"] == stats["pairs"] + stats["host_pairs"]


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        _child(sys.argv[2])
    else:
        sys.exit("usage: test_search_gpu.py --child <file>")
