"""`direction=` through the sharded donor search's driver (grim/shard.py search_sharded), on CPU and alone.  The injected
per-chunk `compute(config, patient_lines, donor_lines, first)` of tests/test_search_sharded.py is not told the direction, so
the seam used here is the other one: the driver's own DonorSearch is replaced by a stand-in that answers from the lines' text
through `search_umug_text` under the direction it was opened with.  What is under test is that the keyword reaches the search
and that the driver hands back the search's answer, whatever the chunk size."""
import os

import numpy as np
import pytest

import harness

ALLELES = {"A": ["A*01:01", "A*02:01", "A*03:01"], "B": ["B*07:02", "B*08:01"]}
TOP_N, MIN_P0, KEEP = 6, 0.5, ("A", "B")


def _line(i, tag):
    """an input line that is one unambiguous genotype; homozygous and heterozygous at A in turn, so that the directions differ"""
    a = ALLELES["A"]
    a1, a2 = a[i % 3], a[(i + (i // 3) % 3) % 3]
    b1, b2 = ALLELES["B"][i % 2], ALLELES["B"][(i // 2) % 2]
    return "%s%d,%s+%s^%s+%s" % (tag, i, a1, a2, b1, b2)


def _umug(lines):
    """the lines as .umug text: every line one genotype row of probability 1"""
    return "".join("%s,%s,1.0,0\n" % tuple(line.split(",")) for line in lines)


def _as_hits(lists, n_patients):
    from grim import _native as nat

    hits = np.zeros((n_patients, TOP_N), dtype=nat.SEARCH_DT)
    hits["donor"] = nat.SEARCH_NO_DONOR
    n_hits = np.zeros(n_patients, dtype=np.uint32)
    for p, found in enumerate(lists):
        n_hits[p] = len(found)
        for k, (d, H, L) in enumerate(found):
            hits[p, k]["donor"] = d
            hits[p, k]["rec"]["mm"][:len(H)] = H
            hits[p, k]["rec"]["locus"][:2] = [L["A"], L["B"]]
    return hits, n_hits


class _TextSearch:
    """DonorSearch as the driver uses it, answering from the lines' text"""

    opened = []

    def __init__(self, imputation, patient_lines, config, keep_loci, top_n, min_p0=0.0, block_lines=65536, planb=None, em=False,
                 groups=None, direction="either"):
        self.plines, self.keep, self.top_n, self.min_p0, self.direction = patient_lines, keep_loci, top_n, min_p0, direction
        self.fed = []
        _TextSearch.opened.append(self)

    def feed(self, donor_lines, first=0):
        assert first == len(self.fed)  # alone, the chunks come in order
        self.fed += donor_lines

    def hits(self):
        from grim import _native as nat
        from grim.search import search_umug_text

        lists = search_umug_text(_umug(self.plines), _umug(self.fed), self.keep, self.top_n, self.min_p0, direction=self.direction)[2]
        stats = dict.fromkeys(nat.SEARCH_STATS, 0)
        stats.update(blocks=1, kernel_ms=0.0, select_ms=0.0, host_pairs=0, download_bytes=0)
        return (np.ones(len(self.plines), dtype=bool),) + _as_hits(lists, len(self.plines)) + (stats,)

    def close(self):
        pass


def test_the_direction_reaches_the_search_and_the_answer_is_the_text_twins(monkeypatch):
    from grim import _native as nat
    from grim import search, shard

    work = harness.ensure_graph("cau")
    dlines, plines = [_line(i, "D") for i in range(40)], [_line(i, "P") for i in range(4)]
    conf, cpath = harness._write_inputs(work, harness.base_conf(["CAU"]), dlines, "srdir")
    ppath = os.path.join(work, "patients_srdir.csv")
    with open(ppath, "w") as fh:
        fh.write("".join(l + "\n" for l in plines))
    monkeypatch.setattr(search, "DonorSearch", _TextSearch)
    monkeypatch.setattr(shard._Job, "imputation", lambda job, config, graph=None: type("Imp", (), {"unsupported": []})())
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.chdir(work)
    answers = {}
    for direction in ("either", "gvh", "hvg"):
        want = _as_hits(search.search_umug_text(_umug(plines), _umug(dlines), KEEP, TOP_N, MIN_P0, direction=direction)[2], len(plines))
        for chunk in (7, 1000):
            _TextSearch.opened = []
            ok, hits, n_hits, stats = shard.search_sharded(cpath, ppath, KEEP, TOP_N, min_p0=MIN_P0, chunk_lines=chunk, timeout_s=60,
                                                           direction=direction)
            assert [s.direction for s in _TextSearch.opened] == [nat.__dict__["MATCH_DIR_" + direction.upper()]]
            assert hits.tobytes() == want[0].tobytes() and list(n_hits) == list(want[1]) and ok.all()
            assert stats["chunks"] == -(-len(dlines) // chunk)
        answers[direction] = want[0].tobytes()
    assert len(set(answers.values())) == 3  # the lines were chosen so that the direction shows
    # the default is `either`, and what is no direction is refused before any job is opened
    _TextSearch.opened = []
    hits = shard.search_sharded(cpath, ppath, KEEP, TOP_N, min_p0=MIN_P0, chunk_lines=7, timeout_s=60)[1]
    assert hits.tobytes() == answers["either"] and _TextSearch.opened[0].direction == nat.MATCH_DIR_EITHER
    _TextSearch.opened = []
    with pytest.raises(ValueError):
        shard.search_sharded(cpath, ppath, KEEP, TOP_N, direction="both")
    with pytest.raises(ValueError):
        shard.search_file_sharded(cpath, ppath, KEEP, os.path.join(work, "never.csv"), TOP_N, direction="both")
    assert _TextSearch.opened == []
