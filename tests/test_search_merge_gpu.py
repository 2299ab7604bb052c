"""The merge door of the device search (grim_search_merge_hits, csrc/grim_search.h: sr_import_kernel, the merging levels, the
third source of sr_gather_kernel) against its plain-Python twin (grim.search.merge_hit_lists), bit for bit: shapes at the real
tile and, in a child process, at a tile of 64; 4096 lists; runs and merges in turn; a list fetched from another device search;
the threshold; every refusal; what a merge leaves alone; DonorSearch fed in pieces and given another search's hits.

Run as a program (`--child <file>`) it is the child of the deep test: it runs the deep cases on the device with whatever
GRIM_SEARCH_TILE its environment holds and writes the bytes it got to <file>."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_search_gpu import N_ALLELES, SCENARIOS, TILE, _batch, _donors, _imputation, _patients, _same, _subject

pytestmark = pytest.mark.gpu

MASK = 0b10011
RUN_N = 40  # donors of the run that makes a running list before a merge; the specials are among them
_material = {}


def _case(top_n, L):
    """the material of one shape, made once, shared and left alone: RUN_N + L * each donors; the first RUN_N are a run, the
    others are dealt round-robin into L parts whose lists `search_records` makes; every list is full where top_n allows
    -> dict(run=(res, rows, ids), lists=(hits[L][P][top_n], n_hits[L][P]), alone=the twin's merge of the lists,
    after=the twin's merge with the run's list as the running list)"""
    from grim.search import merge_hit_lists, search_records

    at = (top_n, L)
    if at not in _material:
        each = max(3, top_n + top_n // 4)
        pres, prows = _patients()
        res, rows, ids = _donors(RUN_N + L * each)
        run = (res[:RUN_N], rows, ids[:RUN_N])
        parts = [np.arange(RUN_N + l, len(res), L) for l in range(L)]
        made = [search_records(pres, prows, [(res[i], rows, ids[i])], MASK, N_ALLELES, top_n, 0.0)[:2] for i in parts]
        lists = (np.stack([m[0] for m in made]), np.stack([m[1] for m in made]))
        running = search_records(pres, prows, [run], MASK, N_ALLELES, top_n, 0.0)[:2]
        alone = merge_hit_lists(made, top_n, 0.0)
        after = merge_hit_lists(made, top_n, 0.0, running=running)
        assert int(lists[1].max()) == min(top_n, each) and running[1].any()
        if L > 1:  # something is dropped, and the run's hits are among the kept ones or the test says nothing about `extra`
            assert int(lists[1].sum(axis=0).max()) > top_n
        assert top_n < 8 or after[0].tobytes() != alone[0].tobytes()
        _material[at] = dict(run=run, lists=lists, alone=alone, after=after)
    return _material[at]


def _merged(ctx, top_n, L, with_run):
    """the device's answer -> (hits, n_hits, None)"""
    from grim import _native as nat

    case = _case(top_n, L)
    sr = nat.Searcher(ctx, MASK, N_ALLELES, top_n, 0.0)
    try:
        sr.set_patients(*_patients())
        if with_run:
            sr.run_records(*case["run"])
        sr.merge(*case["lists"])
        assert sr.select_ms() > 0.0 and sr.kernel_ms() == sr.select_ms()
        return sr.results() + (None,)
    finally:
        sr.close()


@pytest.fixture(scope="module")
def ctx():
    from grim import _native as nat

    return nat.default_context(None)


# ---- 2. deep trees: the child runs first, before this process touches the GPU ------------------------------------------------
DEEP_TILE = 64
DEEP = [(8, L) for L in (1, 7, 8, 9, 64, 65)] + [(32, L) for L in (1, 2, 3, 5)]
_deep = {}


def _child(path):
    from grim import _native as nat

    ctx = nat.default_context(None)
    out = {}
    try:  # the tile is in force: 2 top_n must fit into it
        nat.Searcher(ctx, MASK, N_ALLELES, DEEP_TILE // 2 + 1).close()
        out["refused"] = np.zeros(1, dtype=np.uint8)
    except nat.NativeError as e:
        out["refused"] = np.ones(1, dtype=np.uint8) if "GRIM_SEARCH_TILE" in str(e) else np.zeros(1, dtype=np.uint8)
    for top_n, L in DEEP:
        for with_run in (0, 1):
            hits, n_hits, _ = _merged(ctx, top_n, L, with_run)
            out["hits_%d_%d_%d" % (top_n, L, with_run)] = np.frombuffer(hits.tobytes(), dtype=np.uint8)
            out["n_%d_%d_%d" % (top_n, L, with_run)] = n_hits
    np.savez(path, **out)


@pytest.fixture(scope="module")
def deep(tmp_path_factory):
    """what a fresh child process with GRIM_SEARCH_TILE=64 got (the tile is read when a search is created)"""
    if not _deep:
        path = str(tmp_path_factory.mktemp("merge_deep") / "deep.npz")
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        paths = [os.path.join(root, "tools"), os.path.join(root, "py-graph-imputation_amd"), os.environ.get("PYTHONPATH", "")]
        env = dict(os.environ, GRIM_SEARCH_TILE=str(DEEP_TILE), PYTHONPATH=os.pathsep.join(p for p in paths if p))
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=env, timeout=300,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert done.returncode == 0, done.stdout[-4000:]
        _deep.update(np.load(path))
    return _deep


@pytest.mark.parametrize("with_run", [0, 1], ids=["alone", "after-a-run"])
@pytest.mark.parametrize("top_n,L", DEEP, ids=["top%d-L%d" % c for c in DEEP])
def test_deep_merges_bit_for_bit(deep, top_n, L, with_run):
    from grim import _native as nat

    assert deep["refused"][0] == 1
    want = _case(top_n, L)["after" if with_run else "alone"]
    hits = np.frombuffer(deep["hits_%d_%d_%d" % (top_n, L, with_run)].tobytes(), dtype=nat.SEARCH_DT).reshape(-1, top_n)
    _same((hits, deep["n_%d_%d_%d" % (top_n, L, with_run)], None), want + (None,))


# ---- 1. shapes at the real tile ---------------------------------------------------------------------------------------------
SHAPES = [(256, L) for L in (1, 7, 8, 9)] + [(100, L) for L in (19, 20, 21)] + [(1, 3), (2, 3)]


@pytest.mark.parametrize("with_run", [0, 1], ids=["alone", "after-a-run"])
@pytest.mark.parametrize("top_n,L", SHAPES, ids=["top%d-L%d" % c for c in SHAPES])
def test_shapes_bit_for_bit(ctx, top_n, L, with_run):
    from grim import _native as nat

    assert nat.SEARCH_TILE == TILE and os.environ.get("GRIM_SEARCH_TILE") is None
    want = _case(top_n, L)["after" if with_run else "alone"]
    _same(_merged(ctx, top_n, L, with_run), want + (None,))


# ---- 3. the bound on the lists ----------------------------------------------------------------------------------------------
def test_4096_lists_are_merged_and_4097_refused(ctx):
    from grim import _native as nat
    from grim.search import merge_hit_lists

    n = nat.SEARCH_MERGE_MAX_LISTS + 1
    assert n == 4097
    hits = np.zeros((n, 1, 1), dtype=nat.SEARCH_DT)
    hits["donor"][:, 0, 0] = (np.arange(n, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32)
    hits["rec"]["mm"][:, 0, 0, 0] = ((np.arange(n) * 37) % 101) / 128.0  # ties in mm0 ...
    hits["rec"]["mm"][:, 0, 0, 1] = ((np.arange(n) * 11) % 7) / 16.0     # ... and in mm1: the id decides
    hits["rec"]["locus"][:, 0, 0, :] = np.arange(n)[:, None] + 0.5         # which record was copied shows
    n_hits = np.ones((n, 1), dtype=np.uint32)
    n_hits[5::9] = 0
    want = merge_hit_lists((hits[:-1], n_hits[:-1]), 1, 0.0)
    assert list(want[1]) == [1]
    sr = nat.Searcher(ctx, MASK, N_ALLELES, 1, 0.0)
    try:
        sr.set_patients(*_batch([(nat.ST_OK, _subject("same", 3))]))
        with pytest.raises(nat.NativeError) as e:
            sr.merge(hits, n_hits)
        assert "grim_search_merge_hits" in str(e.value) and "(-3)" in str(e.value) and not sr.results()[1].any()
        sr.merge(hits[:-1], n_hits[:-1])
        _same(sr.results() + (None,), want + (None,))
    finally:
        sr.close()


# ---- 4. runs and merges in turn ---------------------------------------------------------------------------------------------
def test_runs_and_merges_in_turn(ctx):
    from grim import _native as nat
    from grim.search import search_records

    top_n, each = 100, 150
    pres, prows = _patients()
    res, rows, ids = _donors(3 * each)
    A, B, C = [(res[k * each:(k + 1) * each], rows, ids[k * each:(k + 1) * each]) for k in range(3)]
    want = search_records(pres, prows, [A, B, C], MASK, N_ALLELES, top_n, 0.0)
    list_b = search_records(pres, prows, [B], MASK, N_ALLELES, top_n, 0.0)
    runs = search_records(pres, prows, [A, C], MASK, N_ALLELES, top_n, 0.0)
    sr = nat.Searcher(ctx, MASK, N_ALLELES, top_n, 0.0)
    try:
        sr.set_patients(pres, prows)
        sr.run_records(*A)
        sr.merge(list_b[0], list_b[1])  # [P][top_n]: one list
        after_b = sr.results()
        _same(after_b + (None,), search_records(pres, prows, [A, B], MASK, N_ALLELES, top_n, 0.0)[:2] + (None,))
        sr.run_records(*C)  # A's and B's hits are slots of the running list now
        before = sr.results()
        sr.merge(np.zeros((2, len(pres), top_n), dtype=nat.SEARCH_DT), np.zeros((2, len(pres)), dtype=np.uint32))  # nothing to add
        assert sr.select_ms() > 0.0
        got = sr.results()
        assert got[0].tobytes() == before[0].tobytes() and list(got[1]) == list(before[1])
        _same(got + (None,), want[:2] + (None,))
        for k in ("donors_valid", "donors_private", "pairs", "row_pairs", "candidates"):  # the sums are the runs'
            assert sr.stats()[k] == runs[2][k]
        kept = set(got[0]["donor"][got[0]["donor"] != nat.SEARCH_NO_DONOR].tolist())
        assert all(kept & set(part[2].tolist()) for part in (A, B, C))
    finally:
        sr.close()


def test_a_list_from_one_device_search_merged_into_another(ctx):
    from grim import _native as nat
    from grim.search import search_records

    top_n, n = 100, 400
    pres, prows = _patients()
    res, rows, ids = _donors(n)
    want = search_records(pres, prows, [(res, rows, ids)], MASK, N_ALLELES, top_n, 0.0)
    one, two = nat.Searcher(ctx, MASK, N_ALLELES, top_n, 0.0), nat.Searcher(ctx, MASK, N_ALLELES, top_n, 0.0)
    try:
        for sr, part in ((one, slice(0, n, 2)), (two, slice(1, n, 2))):
            sr.set_patients(pres, prows)
            sr.run_records(res[part], rows, ids[part])
        before = dict(stats=two.stats(), donors=two.donors(), flags=two.flags())
        two.merge(*one.results())
        _same(two.results() + (None,), want[:2] + (None,))
        # what a good merge leaves alone
        assert two.stats() == before["stats"] and two.donors() == before["donors"] == n // 2
        for now, was in zip(two.flags(), before["flags"]):
            assert now.tobytes() == was.tobytes()
        assert two.select_ms() > 0.0 and two.kernel_ms() == two.select_ms()
    finally:
        one.close()
        two.close()


# ---- 5. the threshold on the device -----------------------------------------------------------------------------------------
def test_threshold_on_the_device(ctx):
    from grim import _native as nat
    from grim.search import merge_hit_lists, search_records

    top_n, n = 100, 101
    pres, prows = _patients()
    res, rows, ids = _donors(n)
    made = [search_records(pres, prows, [(res[r::3], rows, ids[r::3])], MASK, N_ALLELES, top_n, 0.0)[:2] for r in range(3)]
    lists = (np.stack([m[0] for m in made]), np.stack([m[1] for m in made]))
    shown = sorted({float(h["rec"]["mm"][0]) for m in made for p in range(len(m[1])) for h in m[0][p, :int(m[1][p])]})
    assert len(shown) > 3
    present = shown[len(shown) // 2]  # an mm0 some hits reach and others do not
    counts = []
    for min_p0 in (present, float(np.nextafter(present, np.inf)), 2.0):
        want = search_records(pres, prows, [(res, rows, ids)], MASK, N_ALLELES, top_n, min_p0)[:2]
        assert merge_hit_lists(made, top_n, min_p0)[0].tobytes() == want[0].tobytes()
        sr = nat.Searcher(ctx, MASK, N_ALLELES, top_n, min_p0)
        try:
            sr.set_patients(pres, prows)
            sr.merge(*lists)
            _same(sr.results() + (None,), want + (None,))
        finally:
            sr.close()
        counts.append(int(want[1].sum()))
    assert int(lists[1].sum()) > counts[0] > counts[1] > counts[2] == 0


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(ctx):
    from grim import _native as nat

    top_n = 4
    pres, prows = _patients()
    n_p = len(pres)
    L = nat._search_lib()
    ptr = lambda a: a.ctypes.data_as(nat.C.c_void_p)

    def hand(entries, p=0):
        hits = np.zeros((1, n_p, top_n), dtype=nat.SEARCH_DT)
        hits["donor"] = nat.SEARCH_NO_DONOR
        n_hits = np.zeros((1, n_p), dtype=np.uint32)
        for k, (donor, mm0, mm1) in enumerate(entries):
            hits[0, p, k]["donor"] = donor
            hits[0, p, k]["rec"]["mm"][:2] = (mm0, mm1)
        n_hits[0, p] = len(entries)
        return hits, n_hits

    good = hand([(5, 0.5, 0.25), (3, 0.5, 0.125), (4, 0.5, 0.125)])
    reserved = hand([(1, 0.5, 0.25)])
    reserved[0][0, 0, 0]["reserved"] = 1
    too_many = (good[0], good[1].copy())
    too_many[1][0, 2] = top_n + 1
    bad = {
        "a count above top_n": too_many,
        "the donor of an unused slot": hand([(nat.SEARCH_NO_DONOR, 0.5, 0.25)]),
        "reserved is not 0": reserved,
        "mm0 is NaN": hand([(1, float("nan"), 0.25)]),
        "mm1 is NaN": hand([(1, 0.5, float("nan"))], p=3),
        "mm0 is infinite": hand([(1, float("inf"), 0.25)]),
        "mm1 is infinite": hand([(1, 0.5, float("inf"))]),
        "mm0 is negative": hand([(1, -0.5, 0.25)]),
        "mm1 is negative": hand([(1, 0.5, -1e-300)]),
        "mm0 goes up": hand([(1, 0.25, 0.0), (2, 0.5, 0.0)]),
        "mm1 goes up": hand([(1, 0.5, 0.0), (2, 0.5, 0.25)], p=n_p - 1),
        "the id goes down": hand([(2, 0.5, 0.25), (1, 0.5, 0.25)]),
        "an id twice": hand([(7, 0.75, 0.0), (2, 0.5, 0.25), (2, 0.5, 0.25)]),
    }
    sr = nat.Searcher(ctx, MASK, N_ALLELES, top_n, 0.0)
    try:
        assert L.grim_search_merge_hits(None, ptr(good[0]), ptr(good[1]), n_p, 1) == -1
        sr.set_patients(pres, prows)
        sr.run_records(*_donors(50))
        before = sr.results() + (sr.stats(),)
        assert before[1].any() and sr.select_ms() > 0.0

        def refused(rc, why):
            now = sr.results() + (sr.stats(),)
            assert rc == -3 and "grim_search_merge_hits: " in ctx.error(), why
            assert now[0].tobytes() == before[0].tobytes() and list(now[1]) == list(before[1]) and now[2] == before[2], why
            assert sr.select_ms() == 0.0 and sr.kernel_ms() == 0.0, why
            return True

        for why, (hits, n_hits) in bad.items():
            assert refused(L.grim_search_merge_hits(sr.h, ptr(hits), ptr(n_hits), n_p, 1), why)
            two = (np.concatenate([good[0], hits]), np.concatenate([good[1], n_hits]))  # after a good list
            assert refused(L.grim_search_merge_hits(sr.h, ptr(two[0]), ptr(two[1]), n_p, 2), why)
            with pytest.raises(nat.NativeError):
                sr.merge(hits, n_hits)
        assert refused(L.grim_search_merge_hits(sr.h, ptr(good[0]), ptr(good[1]), n_p - 1, 1), "fewer patients")
        assert refused(L.grim_search_merge_hits(sr.h, ptr(good[0]), ptr(good[1]), n_p + 1, 1), "more patients")
        assert refused(L.grim_search_merge_hits(sr.h, None, ptr(good[1]), n_p, 1), "no hits with counts above 0")
        assert refused(L.grim_search_merge_hits(sr.h, ptr(good[0]), None, n_p, 1), "no counts")
        assert refused(L.grim_search_merge_hits(sr.h, ptr(good[0]), ptr(good[1]), n_p, nat.SEARCH_MERGE_MAX_LISTS + 1), "too many lists")
        with pytest.raises(ValueError):
            sr.merge(good[0][:, :, :3], good[1])
        with pytest.raises(ValueError):
            sr.merge(good[0], good[1][:, :3])
        # no lists: 0, and nothing changes; null arrays are fine when nothing is read
        assert L.grim_search_merge_hits(sr.h, None, None, n_p, 0) == 0 and sr.select_ms() == 0.0
        now = sr.results()
        assert now[0].tobytes() == before[0].tobytes()
        empty = np.zeros((1, n_p), dtype=np.uint32)
        assert L.grim_search_merge_hits(sr.h, None, ptr(empty), n_p, 1) == 0 and sr.select_ms() > 0.0
        assert sr.results()[0].tobytes() == before[0].tobytes()
        # a good merge afterwards still works
        sr.merge(*good)
        after = sr.results()
        assert sr.stats() == before[2]
        was = [int(d) for d in before[0][0, :int(before[1][0])]["donor"]]
        keys = sorted([(-float(h["rec"]["mm"][0]), -float(h["rec"]["mm"][1]), int(h["donor"])) for h in before[0][0, :int(before[1][0])]]
                      + [(-0.5, -0.25, 5), (-0.5, -0.125, 3), (-0.5, -0.125, 4)])[:top_n]
        assert [int(d) for d in after[0][0, :int(after[1][0])]["donor"]] == [k[2] for k in keys] and len(was) <= top_n
        assert after[0][1:].tobytes() == before[0][1:].tobytes() and list(after[1][1:]) == list(before[1][1:])
        # the flags are not consulted: patient 1 takes no part in any run (its status is a miss) and takes a hit all the same
        assert int(before[1][1]) == 0
        sr.merge(*hand([(9, 0.5, 0.0)], p=1))
        flagless = sr.results()
        assert int(flagless[1][1]) == 1 and flagless[0][1]["donor"].tolist() == [9] + [nat.SEARCH_NO_DONOR] * 3
        # a repeat across lists is not detected: both entries are kept
        sr.reset()
        sr.merge(np.concatenate([good[0], good[0]]), np.concatenate([good[1], good[1]]))
        twice = sr.results()
        assert list(twice[1][:1]) == [4] and twice[0][0]["donor"].tolist() == [5, 5, 3, 3]
    finally:
        sr.close()


def test_merge_without_patients(ctx):
    from grim import _native as nat

    sr = nat.Searcher(ctx, MASK, N_ALLELES, 4, 0.0)
    try:
        sr.merge(np.zeros((3, 0, 4), dtype=nat.SEARCH_DT), np.zeros((3, 0), dtype=np.uint32))
        assert sr.select_ms() == 0.0 and sr.results()[0].shape == (0, 4)
        with pytest.raises(nat.NativeError):
            sr.merge(np.zeros((1, 2, 4), dtype=nat.SEARCH_DT), np.zeros((1, 2), dtype=np.uint32))
    finally:
        sr.close()


# ---- 7. DonorSearch ---------------------------------------------------------------------------------------------------------
KEEP = ("A", "B", "DRB1")


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_donor_search_fed_in_pieces_and_merged(scenario):
    from grim.search import DonorSearch, search_donors

    imp, lines, exp, em = _imputation(scenario)
    top_n, half = 5, len(lines) // 2
    whole = search_donors(imp, lines[:8], lines, imp.config, KEEP, top_n, em=em)
    assert whole[2].any()
    if scenario == "pop4_planc":  # alleles the graph has never seen: pairs folded on the host are among the hits
        assert whole[3]["host_pairs"] > 0

    def same(got):
        assert list(got[0]) == list(whole[0])
        _same(got[1:3] + (None,), whole[1:3] + (None,))
        for k in ("pairs", "row_pairs", "donors_valid", "donors_private", "patients_valid", "patients_private", "host_pairs"):
            assert got[3][k] == whole[3][k], k

    fed = DonorSearch(imp, lines[:8], imp.config, KEEP, top_n, em=em)
    try:
        fed.feed(lines[half:], first=half)  # the later lines first: the order of the pieces does not show
        fed.feed(lines[:half])
        got = fed.hits()
        same(got)
        assert got[3]["candidates"] == whole[3]["candidates"] and got[3]["blocks"] == 2 and sorted(got[3]) == sorted(whole[3])
    finally:
        fed.close()

    first, second = DonorSearch(imp, lines[:8], imp.config, KEEP, top_n, em=em), DonorSearch(imp, lines[:8], imp.config, KEEP, top_n, em=em)
    try:
        first.feed(lines[:half])
        second.feed(lines[half:], first=half)
        part = second.hits()
        assert part[2].any() and part[1].tobytes() != whole[1].tobytes()
        first.merge(part[1], part[2])
        assert first.merge_ms > 0.0
        got = first.hits()
        assert list(got[0]) == list(whole[0])
        _same(got[1:3] + (None,), whole[1:3] + (None,))
        with pytest.raises(ValueError):
            first.merge(part[1][:, :3], part[2])
        with pytest.raises(ValueError):
            first.feed(lines[:1], first=0xFFFFFFFF - 1)
    finally:
        first.close()
        second.close()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        _child(sys.argv[2])
    else:
        sys.exit("usage: test_search_merge_gpu.py --child <file>")
