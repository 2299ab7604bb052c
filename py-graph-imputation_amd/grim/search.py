"""
Donor search: each patient's best N donors out of a registry, ranked by the probability of a full match.

The records are those of `grim.match`, bit for bit; what is new is the selection and its order:

    a pair (patient, donor) is a candidate iff its record is computed and mm[0] >= min_p0;
    candidate x comes before candidate y iff  x.mm[0] > y.mm[0],
                                          or  the mm[0] are equal and x.mm[1] > y.mm[1],
                                          or  both are equal and x.id < y.id        (as a Python key: (-mm0, -mm1, id));
    per patient: the first top_n candidates in that order over all donors, n_hits of them, in top_n slots of nat.SEARCH_DT
    (donor id, 0, record); the unused slots are donor = 0xFFFFFFFF with a zero record.

Every mm value of a computed pair is finite and >= +0.0 and the ids are distinct, so the order is strict and the answer does
not depend on how the donors are cut into runs or in which order the runs come.

`search_donors` runs it on the device (csrc/grim_search.h): the donors are streamed block by block, the selection stays in
HBM, and patients x top_n hits come down once, after the last block.  `search_records` is the same selection over record
arrays in plain Python, laid out as the device lays it out; `search_umug_text` the same over `.umug` text.  The three agree
bit for bit.  There is no CPU fallback of the device functions.

The first N of a union are among the first N of each part, so hit lists that other searches produced are inputs of the same
selection: `DonorSearch` is `search_donors` opened once, fed its donors piece by piece and given such lists through the
device's merge door (`nat.Searcher.merge`); `merge_hit_lists` is that door's twin in plain Python.

`direction` ("either", "gvh", "hvg") chooses the records' mismatch function: candidates, threshold and order are
the ones above on the directed mm[0] and mm[1].  A hit list does not say under which direction it was made: merging lists of
one direction only is the caller's duty.
"""

import math

import numpy as np

from . import _native as nat
from .blocks import read_lines
from .match import _Pairing, _keep_mask, _slots_of, _store, direction_code, line_id, match_records, match_umug_text


def _check(top_n, min_p0):
    top_n, min_p0 = int(top_n), float(min_p0)
    if not 1 <= top_n <= nat.SEARCH_MAX_N:
        raise ValueError("top_n must be 1..%d" % nat.SEARCH_MAX_N)
    if math.isnan(min_p0):
        raise ValueError("min_p0 is not a number")
    return top_n, min_p0


def _empty_hits(n, top_n):
    hits = np.zeros((n, top_n), dtype=nat.SEARCH_DT)
    hits["donor"] = nat.SEARCH_NO_DONOR
    return hits


def search_records(pres, prows, donor_runs, keep_mask, n_alleles, top_n, min_p0, groups=None, direction="either"):
    """The selection on record arrays as grim_search_run_records defines it (include/grim_hip.h).  `donor_runs`: a list of
    (res, rows, ids), nat.RESULT_DT / nat.ROW_DT arrays and one id per donor, distinct over all runs.  Runs `match_records`
    per run, keeps the computed pairs with mm[0] >= min_p0 and sorts them -> (hits nat.SEARCH_DT[P][top_n], n_hits u32[P],
    stats), laid out as the device lays them out: stats are each run's match statistics summed, and `candidates`.  `groups`,
    `direction`: as `match_records`."""
    top_n, min_p0 = _check(top_n, min_p0)
    direction = direction_code(direction)
    ready = nat.MATCH_VALID | nat.MATCH_PRIVATE
    stats = dict.fromkeys(nat.SEARCH_STATS, 0)
    found = [[] for _ in range(len(pres))]  # per patient: (-mm0, -mm1, id, record)
    for res, rows, ids in donor_runs:
        if len(ids) != len(res):
            raise ValueError("%d donors but %d ids" % (len(res), len(ids)))
        rec, pf, df, run = match_records(pres, prows, res, rows, keep_mask, n_alleles, groups, direction)
        for k in nat.MATCH_STATS:
            stats[k] += run[k]
        for p in np.flatnonzero((pf & ready) == nat.MATCH_VALID):
            for d in np.flatnonzero((df & ready) == nat.MATCH_VALID):
                mm0 = float(rec[p, d]["mm"][0])
                if mm0 >= min_p0:
                    found[p].append((-mm0, -float(rec[p, d]["mm"][1]), int(ids[d]), rec[p, d]))
                    stats["candidates"] += 1
    hits = _empty_hits(len(pres), top_n)
    n_hits = np.zeros(len(pres), dtype=np.uint32)
    for p, cands in enumerate(found):
        cands.sort(key=lambda c: c[:3])
        n_hits[p] = min(top_n, len(cands))
        for k, (_, _, donor, rec) in enumerate(cands[:top_n]):
            hits[p, k]["donor"] = donor
            hits[p, k]["rec"] = rec
    return hits, n_hits, stats


def _as_lists(lists, top_n):
    """`lists` of merge_hit_lists -> [(hits SEARCH_DT[P][top_n], n_hits u32[P])]"""
    if isinstance(lists, tuple) and len(lists) == 2 and isinstance(lists[0], np.ndarray) and lists[0].ndim == 3:
        lists = list(zip(lists[0], lists[1]))  # (hits[L][P][top_n], n_hits[L][P])
    out = []
    for hits, n_hits in lists:
        hits, n_hits = np.asarray(hits), np.asarray(n_hits)
        if hits.dtype != nat.SEARCH_DT or hits.ndim != 2 or hits.shape[1] != top_n or n_hits.shape != hits.shape[:1]:
            raise ValueError("a list is not (nat.SEARCH_DT[patients][top_n = %d], one count a patient)" % top_n)
        out.append((hits, n_hits))
    return out


def merge_hit_lists(lists, top_n, min_p0, running=None):
    """The merge door of the device search (grim_search_merge_hits, include/grim_hip.h) in plain Python.  `lists`: a sequence
    of (hits nat.SEARCH_DT[P][top_n], n_hits[P]) as `search_records`, `Searcher.results` or `DonorSearch.hits` give them, or
    one pair of arrays (hits[L][P][top_n], n_hits[L][P]); `running`: the (hits, n_hits) the search holds so far, taken as it
    is (None: empty lists).  Of every list and patient the first n_hits slots are entries; an entry is a candidate iff its
    mm[0] >= min_p0; the answer per patient is the first top_n of running + candidates in the search's order ->
    (hits nat.SEARCH_DT[P][top_n], n_hits u32[P]), laid out as the device lays them out.  The refusals of the door are
    ValueErrors here: lists for another number of patients, more than nat.SEARCH_MERGE_MAX_LISTS lists, a count above top_n,
    an entry with donor = nat.SEARCH_NO_DONOR or reserved != 0, an entry whose mm[0] or mm[1] is NaN, infinite or < 0, a list
    whose entries are not in the strict order."""
    top_n, min_p0 = _check(top_n, min_p0)
    lists = _as_lists(lists, top_n)
    if running is not None:
        running = _as_lists([running], top_n)[0]
    if not lists and running is None:
        raise ValueError("neither lists nor a running list: the number of patients is not known")
    n_p = len(running[1]) if running is not None else len(lists[0][1])
    if len(lists) > nat.SEARCH_MERGE_MAX_LISTS:
        raise ValueError("%d lists: more than %d" % (len(lists), nat.SEARCH_MERGE_MAX_LISTS))
    found = [[] for _ in range(n_p)]  # per patient: ((-mm0, -mm1, id), hit)
    for l, (hits, n_hits) in enumerate(lists):
        if len(n_hits) != n_p:
            raise ValueError("list %d is of %d patients, not %d" % (l, len(n_hits), n_p))
        if len(n_hits) and int(n_hits.max()) > top_n:
            raise ValueError("list %d holds a count above top_n" % l)
        for p in np.flatnonzero(n_hits):
            before = None
            for h in hits[p, :int(n_hits[p])]:
                mm0, mm1, donor = float(h["rec"]["mm"][0]), float(h["rec"]["mm"][1]), int(h["donor"])
                if donor == nat.SEARCH_NO_DONOR or int(h["reserved"]) != 0:
                    raise ValueError("list %d, patient %d: a hit whose donor is SEARCH_NO_DONOR or whose reserved word is not 0" % (l, p))
                if not (0.0 <= mm0 < math.inf and 0.0 <= mm1 < math.inf):
                    raise ValueError("list %d, patient %d: a hit whose mm[0] or mm[1] is negative, NaN or infinite" % (l, p))
                key = (-mm0, -mm1, donor)
                if before is not None and not before < key:
                    raise ValueError("list %d, patient %d: the hits are not in the strict order (mm[0] down, mm[1] down, id up)" % (l, p))
                before = key
                if mm0 >= min_p0:
                    found[p].append((key, h))
    out = _empty_hits(n_p, top_n)
    n_out = np.zeros(n_p, dtype=np.uint32)
    for p, cands in enumerate(found):
        if running is not None:
            cands += [((-float(h["rec"]["mm"][0]), -float(h["rec"]["mm"][1]), int(h["donor"])), h)
                      for h in running[0][p, :min(top_n, int(running[1][p]))]]
        cands.sort(key=lambda c: c[0])
        n_out[p] = min(top_n, len(cands))
        for k, (key, h) in enumerate(cands[:top_n]):
            out[p, k]["donor"] = key[2]
            out[p, k]["rec"] = h["rec"]
    return out, n_out


def search_umug_text(patient_text, donor_text, keep_loci, top_n, min_p0=0.0, groups=None, direction="either"):
    """The selection on `.umug` text through `match_umug_text`; a donor's id is its position in the donor text -> (patient ids,
    donor ids, hits): hits[p] is the list of (donor position, mm[0..2|K|], {locus name: probability of no mismatch}) of the
    patient's first top_n donors with mm[0] >= min_p0, in order.  `groups`: a group specification, `direction`: as `match_umug_text`."""
    top_n, min_p0 = _check(top_n, min_p0)
    pid, did, records = match_umug_text(patient_text, donor_text, keep_loci, groups=groups, direction=direction)
    hits = []
    for line in records:
        cands = [(-H[0], -H[1], d) for d, (H, _) in enumerate(line) if H[0] >= min_p0]
        cands.sort()
        hits.append([(d,) + line[d] for _, _, d in cands[:top_n]])
    return pid, did, hits


class DonorSearch:
    """`search_donors` opened once: the patients are imputed as one device batch and set at construction; `feed` streams donor
    lines through the device, any number of times; `merge` takes hit lists that another search of the same patients produced;
    `hits` is the answer over everything fed and merged so far; `close` releases the device objects.  Arguments as
    `search_donors`, without the donors."""

    def __init__(self, imputation, patient_lines, config, keep_loci, top_n, min_p0=0.0, block_lines=65536, planb=None, em=False,
                 groups=None, direction="either"):
        self.top_n, self.min_p0 = _check(top_n, min_p0)
        self.pairing = pairing = _Pairing(imputation, patient_lines, None, config, keep_loci, block_lines, planb, em, groups, direction)
        self.searcher = None
        self.stats = dict.fromkeys(nat.SEARCH_STATS, 0)
        self.stats.update(blocks=0, kernel_ms=0.0, select_ms=0.0, host_pairs=0, download_bytes=0)
        self.merge_ms = 0.0  # device time of the merges
        self.host = {}   # patient -> [((-mm0, -mm1, id), H, L)] of the pairs folded here, at most top_n after a block
        try:
            self.searcher = nat.Searcher(pairing.ctx, pairing.mask, pairing.n_alleles, self.top_n, self.min_p0, pairing.direction)
            pairing.set_patients(self.searcher, lambda: self.searcher.flags()[0], self.stats)
        except BaseException:
            self.close()
            raise

    def feed(self, donor_lines, first=0):
        """donor lines (a list, or the path of an input file) that begin at line `first` of the donor input: cut into blocks,
        each imputed as one device batch and selected on the device into the running lists; a donor's id is `first` + its
        position in `donor_lines`"""
        pairing, searcher, stats, top_n = self.pairing, self.searcher, self.stats, self.top_n
        dlines = read_lines(donor_lines)
        first = int(first)
        if first < 0 or first + len(dlines) >= nat.SEARCH_NO_DONOR:
            raise ValueError("donor lines %d..%d: a line number must fit a hit's donor field" % (first, first + len(dlines)))
        pf, host = pairing.pf, self.host
        for block in pairing.donor_blocks(dlines, first):
            if block.batch is None or not len(pf):
                pairing.check(block, np.zeros(0, dtype=np.uint8))
                continue
            ids = block.lo + block.line_of
            searcher.run(block.batch, ids.astype(np.uint32))
            df = searcher.flags()[1]
            for p, d, H, L in pairing.host_pairs(block, df):
                stats["host_pairs"] += 1
                if H[0] >= self.min_p0:
                    host.setdefault(int(p), []).append(((-H[0], -H[1], int(ids[d])), H, L))
                    stats["candidates"] += 1
            for p in host:
                host[p].sort(key=lambda c: c[0])
                del host[p][top_n:]
            stats["donors_valid"] += int(np.count_nonzero(df & nat.MATCH_VALID))
            stats["donors_private"] += int(np.count_nonzero(df & nat.MATCH_PRIVATE))
            stats["kernel_ms"] += searcher.kernel_ms()
            stats["select_ms"] += searcher.select_ms()
            stats["blocks"] += 1

    def merge(self, hits, n_hits):
        """hit lists by patient *line*, as `hits` returns them: nat.SEARCH_DT[L][lines][top_n] or [lines][top_n] with matching
        n_hits, of searches of the same patients over other donors (ids distinct from everything seen here).  The lines that
        are patients on the device go through the device's merge door; the other lines have no hits."""
        hits = np.asarray(hits)
        n_hits = np.asarray(n_hits, dtype=np.uint32)
        if hits.ndim == 2:
            hits, n_hits = hits[None], n_hits[None]
        lines = len(self.pairing.plines)
        if hits.dtype != nat.SEARCH_DT or hits.shape[1:] != (lines, self.top_n) or n_hits.shape != hits.shape[:2]:
            raise ValueError("not nat.SEARCH_DT[lists][%d patient lines][top_n = %d] with one count a list and line" % (lines, self.top_n))
        if not len(self.pairing.pf):
            if n_hits.any():
                raise ValueError("hits of patient lines that are no patients on the device")
            return
        line_of = self.pairing.pblock.line_of
        off = np.ones(lines, dtype=bool)
        off[line_of] = False
        if n_hits[:, off].any():
            raise ValueError("hits of patient lines that are no patients on the device")
        self.searcher.merge(hits[:, line_of], n_hits[:, line_of])
        self.merge_ms += self.searcher.select_ms()

    def hits(self):
        """-> (patient_ok, hits, n_hits, stats) as `search_donors` returns them, over everything fed and merged so far: the
        device's lists fetched and merged with the pairs folded on the host under the same order"""
        pairing, top_n = self.pairing, self.top_n
        plines, slots, pf, pblock, host = pairing.plines, pairing.slots, pairing.pf, pairing.pblock, self.host
        stats = dict(self.stats)
        hits = _empty_hits(len(plines), top_n)
        n_hits = np.zeros(len(plines), dtype=np.uint32)
        if len(pf):
            dev_hits, dev_n = self.searcher.results()
            stats["download_bytes"] = dev_hits.nbytes + dev_n.nbytes
            total = self.searcher.stats()
            stats["pairs"], stats["row_pairs"] = total["pairs"], total["row_pairs"]
            stats["candidates"] += total["candidates"]
            for p in range(len(pf)):
                line = int(pblock.line_of[p])
                if p not in host:
                    hits[line], n_hits[line] = dev_hits[p], dev_n[p]
                    continue
                merged = [((-float(h["rec"]["mm"][0]), -float(h["rec"]["mm"][1]), int(h["donor"])), h) for h in dev_hits[p, :int(dev_n[p])]]
                merged += [(key, (H, L)) for key, H, L in host[p]]
                merged.sort(key=lambda c: c[0])
                n_hits[line] = min(top_n, len(merged))
                for k, (key, what) in enumerate(merged[:top_n]):
                    hits[line, k]["donor"] = key[2]
                    if isinstance(what, tuple):
                        _store(hits[line, k]["rec"], slots, *what)
                    else:
                        hits[line, k]["rec"] = what["rec"]
        return pairing.patient_ok, hits, n_hits, stats

    def close(self):
        self.pairing.close()
        if self.searcher is not None:
            self.searcher.close()


def search_donors(imputation, patient_lines, donor_lines_or_path, config, keep_loci, top_n, min_p0=0.0, block_lines=65536, planb=None,
                  em=False, groups=None, direction="either"):
    """Every patient's first `top_n` donors on the device.  Arguments as `match_probabilities`: `patient_lines`: input lines;
    `donor_lines_or_path`: input lines (a list) or the path of an input file; `config`: the configuration dict of
    `load_config`; `keep_loci`: locus names of its loci_map.  The patients are imputed as one device batch and set once; the
    donors are cut into blocks of `block_lines` lines exactly as `match_probabilities` cuts them, each tokenised, imputed as
    one device batch and matched where its rows lie, and the selection of every block is merged on the device with what the
    earlier blocks left; a donor's id is its line number in the donor input.  The hits are fetched once, after the last block.
    Pairs the device leaves out because a subject holds an allele the dictionary does not know are folded here on allele
    text, thresholded, kept in a per-patient list trimmed to `top_n` and merged with the device's hits at the end under the
    same order (the first N of a union are among the first N of each part, so the merge is exact).  A patient with such an
    allele at a kept locus is therefore searched entirely on the host: slow, and correct.
    -> (patient_ok, hits, n_hits, stats): hits is nat.SEARCH_DT[len(patient_lines)][top_n], hits["donor"] donor line numbers,
    n_hits u32[len(patient_lines)]; patient_ok says which lines have genotype rows (the others have no hits); stats are the
    match statistics as `match_probabilities` sums them, `candidates` (device and host), and `blocks`, `kernel_ms`,
    `select_ms`, `host_pairs` (pairs folded on text) and `download_bytes` (hits and counts fetched from the device).  The cuts
    do not show in any byte.  Subjects the device cannot answer follow `imputation.on_unsupported` as in
    `impute_lines_block`.  `groups`, `direction`: as `match_probabilities`."""
    top_n, min_p0 = _check(top_n, min_p0)
    search = DonorSearch(imputation, patient_lines, config, keep_loci, top_n, min_p0, block_lines, planb, em, groups, direction)
    try:
        search.feed(donor_lines_or_path)
        return search.hits()
    finally:
        search.close()


def write_hits_csv(out_path, graph, keep_loci, plines, dlines, pok, hits, n_hits):
    """the CSV of `search_file`: the header, then per patient line with genotype rows its hits in order"""
    slots = _slots_of(_keep_mask(graph.locus_slot, keep_loci))
    nb = 2 * len(slots) + 1
    with open(out_path, "w") as fh:
        fh.write(",".join(["patient_id", "rank", "donor_id"] + ["mm%d" % m for m in range(nb)] + [graph.slot_locus[s] for s in slots]) + "\n")
        for p in np.flatnonzero(pok):
            for k in range(int(n_hits[p])):
                r = hits[p, k]["rec"]
                vals = [float(x) for x in r["mm"][:nb]] + [float(r["locus"][s]) for s in slots]
                fh.write("%s,%d,%s,%s\n" % (line_id(plines[p]), k, line_id(dlines[int(hits[p, k]["donor"])]), ",".join(repr(v) for v in vals)))


def search_file(conf_file, patients_path, keep_loci, out_path, top_n, min_p0=0.0, graph=None, block_lines=65536, groups=None,
                direction="either"):
    """The configuration's input file as donors against the input file `patients_path`, on `graph` (built from the
    configuration's graph CSVs when None) -> a CSV at `out_path`: a header `patient_id,rank,donor_id,mm0,...,mm{2|K|},<kept
    locus names>`, then per patient its hits in order, ranks from 0, patient-major, floats written with repr.  Paths are
    taken as the configuration gives them.  `groups`, `direction`: as `search_donors`.  -> stats"""
    from .grim import graph_instance
    from .imputation.impute import Imputation
    from .run_impute_def import load_config

    config, _ = load_config(conf_file)
    if graph is None:
        graph = graph_instance(config)
    imp = Imputation(graph, config)
    plines, dlines = read_lines(patients_path), read_lines(config["imputation_input_file"])
    pok, hits, n_hits, stats = search_donors(imp, plines, dlines, config, keep_loci, top_n, min_p0=min_p0, block_lines=block_lines,
                                             groups=groups, direction=direction)
    write_hits_csv(out_path, graph, keep_loci, plines, dlines, pok, hits, n_hits)
    return stats
