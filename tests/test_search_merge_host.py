"""The merge door's CPU twin (grim.search.merge_hit_lists): the lists `search_records` gives for the parts of a donor set,
merged, equal `search_records` over the whole set, however the donors are cut; the threshold filters lists made under a lower
one; a running list takes part; every refusal of the contract (include/grim_hip.h, the merge door).  No GPU."""
import numpy as np
import pytest

from test_search_gpu import N_ALLELES, _donors, _patients

MASKS = [0b10011, 0b11111]
_wholes = {}


def _whole(n, mask, top_n, min_p0=0.0):
    """search_records over all of _donors(n), computed once per case, shared and left alone"""
    from grim.search import search_records

    at = (n, mask, top_n, min_p0)
    if at not in _wholes:
        pres, prows = _patients()
        _wholes[at] = search_records(pres, prows, [_donors(n)], mask, N_ALLELES, top_n, min_p0)
    return _wholes[at]


def _parts(n, R, how):
    """index arrays of R pieces of range(n): contiguous (the last ones may be empty) or round-robin"""
    idx = np.arange(n)
    if how == "contiguous":
        step = -(-n // R)
        return [idx[r * step:(r + 1) * step] for r in range(R)]
    return [idx[r::R] for r in range(R)]


def _lists(n, mask, top_n, R, how, min_p0=0.0):
    """the (hits, n_hits) search_records gives for each part; the rows stay one array: a part's subjects point into it"""
    from grim.search import search_records

    pres, prows = _patients()
    res, rows, ids = _donors(n)
    return [search_records(pres, prows, [(res[i], rows, ids[i])], mask, N_ALLELES, top_n, min_p0)[:2] for i in _parts(n, R, how)]


def _equal(got, want):
    assert list(got[1]) == list(want[1])
    assert got[0]["donor"].tolist() == want[0]["donor"].tolist()
    assert got[0].tobytes() == want[0].tobytes()


SIZES = [(top_n, n) for top_n in (1, 8, 256) for n in sorted({1, top_n - 1, top_n, top_n + 1, 600} - {0})]


@pytest.mark.parametrize("how", ["contiguous", "round-robin"])
@pytest.mark.parametrize("R", [1, 2, 3, 8])
@pytest.mark.parametrize("mask", MASKS, ids=[bin(m) for m in MASKS])
@pytest.mark.parametrize("top_n,n", SIZES, ids=["top%d-D%d" % c for c in SIZES])
def test_parts_merged_equal_the_whole(top_n, n, mask, R, how):
    from grim.search import merge_hit_lists

    want = _whole(n, mask, top_n)
    lists = _lists(n, mask, top_n, R, how)
    got = merge_hit_lists(lists, top_n, 0.0)
    _equal(got, want)
    assert not got[0]["reserved"].any()
    if n == 600:
        # 593 plain donors, every one a candidate of each computed patient at a threshold of 0.0: more than any top_n, so
        # the merge drops something
        assert want[2]["candidates"] // int(np.count_nonzero(want[1])) > top_n
        p = int(np.flatnonzero(want[1])[0])
        assert int(want[1][p]) == top_n
        if R >= 2:  # and the lists themselves hold more entries than the answer has slots
            assert sum(int(l[1][p]) for l in lists) > top_n
        if R >= 2 and top_n >= 2:  # a single kept hit comes from a single list; from two hits on, no list may be ignored
            kept = set(got[0][p]["donor"].tolist())
            sources = [r for r, l in enumerate(lists) if kept & set(l[0][p, :int(l[1][p])]["donor"].tolist())]
            assert len(sources) >= 2


@pytest.mark.parametrize("R", [2, 3, 8])
def test_no_list_is_ignored_at_top_n_1(R):
    """one kept hit has one source, so the test above cannot tell at top_n 1 whether a list was ignored: here the list that
    holds a patient's winner is put at every position in turn, and the answer must stay the whole's"""
    from grim.search import merge_hit_lists

    mask, n = 0b10011, 600
    want = _whole(n, mask, 1)
    lists = _lists(n, mask, 1, R, "round-robin")
    p = int(np.flatnonzero(want[1])[0])
    winner = int(want[0][p, 0]["donor"])
    holds = [r for r, l in enumerate(lists) if int(l[1][p]) and int(l[0][p, 0]["donor"]) == winner]
    assert len(holds) == 1  # ids are distinct: the winner is the head of exactly one list
    seen = set()
    for shift in range(R):
        turned = lists[shift:] + lists[:shift]
        seen.add((holds[0] - shift) % R)
        _equal(merge_hit_lists(turned, 1, 0.0), want)
    assert seen == set(range(R))  # the winner's list has stood at every position


@pytest.mark.parametrize("mask", MASKS, ids=[bin(m) for m in MASKS])
def test_one_array_of_lists_is_the_same_as_a_sequence(mask):
    from grim.search import merge_hit_lists

    lists = _lists(600, mask, 8, 3, "round-robin")
    stacked = (np.stack([l[0] for l in lists]), np.stack([l[1] for l in lists]))
    _equal(merge_hit_lists(stacked, 8, 0.0), _whole(600, mask, 8))


def test_the_threshold_filters_lists_made_under_a_lower_one():
    from grim.search import merge_hit_lists

    mask, top_n, n = 0b10011, 100, 101
    base = _whole(n, mask, top_n)
    shown = sorted({float(h["rec"]["mm"][0]) for p in range(len(base[1])) for h in base[0][p, :int(base[1][p])]})
    assert len(shown) > 3
    present = shown[len(shown) // 2]  # an mm0 some hits reach and others do not
    lists = _lists(n, mask, top_n, 3, "round-robin")  # made at 0.0
    counts = []
    for min_p0 in (present, float(np.nextafter(present, np.inf))):
        want = _whole(n, mask, top_n, min_p0)
        _equal(merge_hit_lists(lists, top_n, min_p0), want)
        counts.append(int(want[1].sum()))
    assert int(base[1].sum()) > counts[0] > counts[1] > 0
    got = merge_hit_lists(lists, top_n, 2.0)
    assert not got[1].any() and (got[0]["donor"] == 0xFFFFFFFF).all() and not np.frombuffer(got[0]["rec"].tobytes(), dtype=np.uint8).any()


def test_a_running_list_takes_part_and_empty_lists_change_nothing():
    from grim import _native as nat
    from grim.search import merge_hit_lists

    mask, top_n, n = 0b10011, 8, 600
    want = _whole(n, mask, top_n)
    lists = _lists(n, mask, top_n, 3, "contiguous")
    got = merge_hit_lists(lists[1:], top_n, 0.0, running=lists[0])
    _equal(got, want)
    step = merge_hit_lists([lists[2]], top_n, 0.0, running=merge_hit_lists([lists[1]], top_n, 0.0, running=lists[0]))
    _equal(step, want)
    # the running list is taken as it is: a threshold above its hits does not filter it
    kept = merge_hit_lists([], top_n, 2.0, running=lists[0])
    _equal(kept, lists[0])
    # lists with n_hits = 0 everywhere: their slots are not looked at, whatever they hold
    empty = (np.zeros((len(want[1]), top_n), dtype=nat.SEARCH_DT), np.zeros(len(want[1]), dtype=np.uint32))
    empty[0]["reserved"] = 7
    _equal(merge_hit_lists([empty, empty], top_n, 0.0, running=want[:2]), want)
    nothing = merge_hit_lists([empty], top_n, 0.0)
    assert not nothing[1].any() and (nothing[0]["donor"] == nat.SEARCH_NO_DONOR).all() and not nothing[0]["reserved"].any()


def _hand(entries, top_n, n_p=1):
    """[(donor, mm0, mm1)] as patient 0's list of n_p patients -> (hits, n_hits)"""
    from grim import _native as nat

    hits = np.zeros((n_p, top_n), dtype=nat.SEARCH_DT)
    hits["donor"] = nat.SEARCH_NO_DONOR
    for k, (donor, mm0, mm1) in enumerate(entries):
        hits[0, k]["donor"] = donor
        hits[0, k]["rec"]["mm"][:2] = (mm0, mm1)
    n_hits = np.zeros(n_p, dtype=np.uint32)
    n_hits[0] = len(entries)
    return hits, n_hits


def test_every_refusal_of_the_contract():
    from grim import _native as nat
    from grim.search import merge_hit_lists

    good = _hand([(5, 0.5, 0.25), (3, 0.5, 0.125), (4, 0.5, 0.125)], 4)
    hits, n_hits = merge_hit_lists([good], 4, 0.0)
    assert list(n_hits) == [3] and hits[0]["donor"].tolist() == [5, 3, 4, nat.SEARCH_NO_DONOR]
    bad = {
        "another number of patients": [good, _hand([(9, 0.5, 0.25)], 4, n_p=2)],
        "a count above top_n": [(good[0], np.array([5], dtype=np.uint32))],
        "the donor of an unused slot": [_hand([(nat.SEARCH_NO_DONOR, 0.5, 0.25)], 4)],
        "mm0 is NaN": [_hand([(1, float("nan"), 0.25)], 4)],
        "mm1 is NaN": [_hand([(1, 0.5, float("nan"))], 4)],
        "mm0 is infinite": [_hand([(1, float("inf"), 0.25)], 4)],
        "mm1 is infinite": [_hand([(1, 0.5, float("inf"))], 4)],
        "mm0 is negative": [_hand([(1, -0.5, 0.25)], 4)],
        "mm1 is negative": [_hand([(1, 0.5, -1e-300)], 4)],
        "mm0 goes up": [_hand([(1, 0.25, 0.0), (2, 0.5, 0.0)], 4)],
        "mm1 goes up": [_hand([(1, 0.5, 0.0), (2, 0.5, 0.25)], 4)],
        "the id goes down": [_hand([(2, 0.5, 0.25), (1, 0.5, 0.25)], 4)],
        "an id twice": [_hand([(2, 0.5, 0.25), (2, 0.5, 0.25)], 4)],
        "other slots": [_hand([(1, 0.5, 0.25)], 5)],
    }
    for why, lists in bad.items():
        with pytest.raises(ValueError):  # after a good list, and alone
            merge_hit_lists([good] + lists, 4, 0.0)
            pytest.fail(why)
        with pytest.raises(ValueError):
            merge_hit_lists(lists, 4, 0.0)
            pytest.fail(why)
    reserved = _hand([(1, 0.5, 0.25)], 4)
    reserved[0][0, 0]["reserved"] = 1
    with pytest.raises(ValueError):
        merge_hit_lists([reserved], 4, 0.0)
    # a refused entry below the threshold is refused all the same: the check comes before the selection
    with pytest.raises(ValueError):
        merge_hit_lists([_hand([(1, 0.5, 0.25), (2, float("nan"), 0.0)], 4)], 4, 0.75)
    for top_n, min_p0 in ((0, 0.0), (257, 0.0), (4, float("nan"))):
        with pytest.raises(ValueError):
            merge_hit_lists([good], top_n, min_p0)
    with pytest.raises(ValueError):
        merge_hit_lists([], 4, 0.0)
    one = _hand([(1, 0.5, 0.25)], 1)
    many = [_hand([(k, 0.5, 0.25)], 1) for k in range(nat.SEARCH_MERGE_MAX_LISTS + 1)]
    assert merge_hit_lists(many[:-1], 1, 0.0)[0][0, 0]["donor"] == 0
    with pytest.raises(ValueError):
        merge_hit_lists(many, 1, 0.0)
    # a repeat across lists is not detected: both entries are kept
    twice = merge_hit_lists([one, one], 1, 0.0)
    assert list(twice[1]) == [1] and int(twice[0][0, 0]["donor"]) == 1
    both = merge_hit_lists([_hand([(1, 0.5, 0.25)], 4), _hand([(1, 0.5, 0.25)], 4)], 4, 0.0)
    assert list(both[1]) == [2] and both[0][0]["donor"].tolist()[:2] == [1, 1]
