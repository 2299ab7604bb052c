"""
Match probabilities between imputed subjects: for a patient and a donor, the probability that their genotypes differ in
0, 1, 2, ... alleles over a set K of kept loci (a 10/10, a 9/10, an 8/8 match), and per locus the probability of no mismatch.

The reference ends at the printed `.umug` files; the operation is defined here:

    per subject, genotype rows k = 0..n-1 in rank order with probabilities p_k:
      total = ((p_0 + p_1) + p_2) + ...,  w_k = p_k / total
    per row pair (patient row i, donor row j), per kept locus with the patient's alleles x1, x2 and the donor's y1, y2:
      eq(x, y) = x == y and x is typed          (an untyped locus equals nothing)
      mm = 2 - max(eq(x1,y1) + eq(x2,y2), eq(x1,y2) + eq(x2,y1));   M(i,j) = the sum of mm over the kept loci
    per (patient, donor) pair, with w the patient's weights and v the donor's:
      for j (donor rows, rank order):
          ph[*] = 0.0, pl[*] = 0.0
          for i (patient rows, rank order):  t = w_i * v_j;  ph[M(i,j)] += t;  pl[locus] += t for every locus with mm == 0
          H[m] += ph[m],  L[locus] += pl[locus]
      mm[m] = H[m],  locus[s] = L[s]

Two keywords change what is counted, not how it is summed.  `direction`: "either" is the mm above; "gvh" counts
the patient's alleles the donor lacks, mm = !(eq(x1,y1) or eq(x1,y2)) + !(eq(x2,y1) or eq(x2,y2)), an untyped allele always
lacking; "hvg" the donor's alleles the patient lacks; either = max(gvh, hvg).  `graded`: the record holds, in the place of
locus[s], grade[s][g] for g = 0, 1, 2: the same fold with `mm == g` for `mm == 0` (nat.MATCH_GRADE_DT).

`match_probabilities` runs it on the device, on the rows the donors' batches leave in HBM (csrc/grim_match.h).  Pairs in
which a subject holds an allele the dictionary does not know are left out by the device (the allele's id is private to the
subject) and folded here on allele text.  `match_records` is the same fold over record arrays in plain Python floats, laid
out as the device lays it out; `match_umug_text` the same over `.umug` text.  The three agree bit for bit.  There is no CPU
fallback of the device functions.
"""

import math

import numpy as np

from . import _native as nat
from .blocks import Blocks, note_unsupported, read_lines
from .groups import as_groups, regroup_umug_text
from .marginal import keep_mask as _keep_mask


DIRECTIONS = {"either": nat.MATCH_DIR_EITHER, "gvh": nat.MATCH_DIR_GVH, "hvg": nat.MATCH_DIR_HVG}


def direction_code(direction):
    """one of "either", "gvh", "hvg" (or its nat.MATCH_DIR_* number) -> the number"""
    if isinstance(direction, str) and direction in DIRECTIONS:
        return DIRECTIONS[direction]
    if isinstance(direction, (int, np.integer)) and not isinstance(direction, bool) and int(direction) in DIRECTIONS.values():
        return int(direction)
    raise ValueError("direction must be one of %s, not %r" % (", ".join(sorted(DIRECTIONS)), direction))


def locus_mismatches(x1, x2, y1, y2, direction=nat.MATCH_DIR_EITHER):
    """mm_s of DESIGN 4.7 / 4.12 on allele numbers (0 = untyped), integers or integer arrays that broadcast: the patient's
    x1, x2 against the donor's y1, y2.  either: 2 - the better pairing; gvh: the patient's alleles the donor lacks; hvg: the
    donor's alleles the patient lacks."""
    def eq(x, y):
        return (x == y) & (x != 0)

    if direction == nat.MATCH_DIR_EITHER:
        straight = eq(x1, y1) * 1 + eq(x2, y2) * 1
        crossed = eq(x1, y2) * 1 + eq(x2, y1) * 1
        return 2 - np.maximum(straight, crossed)
    if direction == nat.MATCH_DIR_HVG:
        x1, x2, y1, y2 = y1, y2, x1, x2
    elif direction != nat.MATCH_DIR_GVH:
        raise ValueError("not a direction: %r" % (direction,))
    return 2 - ((eq(x1, y1) | eq(x1, y2)) * 1 + (eq(x2, y1) | eq(x2, y2)) * 1)


class _Folder:
    """the pair fold on row genotypes: a row genotype is a tuple with one (x, y) allele pair per kept locus (None = untyped);
    alleles compare with ==.  Alleles are numbered (0 = untyped) so that the mismatch COUNTS of all row pairs come from integer
    array compares; every floating-point operation is a plain Python one, in the contract's order."""

    def __init__(self, nk):
        self.nk = nk
        self.ids = {None: 0}

    def pack(self, genos):
        """[row genotype] -> (x[nk][rows], y[nk][rows]) allele numbers"""
        ids = self.ids
        x = np.zeros((self.nk, len(genos)), dtype=np.int64)
        y = np.zeros((self.nk, len(genos)), dtype=np.int64)
        for r, geno in enumerate(genos):
            for k, (a, b) in enumerate(geno):
                x[k, r] = ids.setdefault(a, len(ids))
                y[k, r] = ids.setdefault(b, len(ids))
        return x, y

    def fold(self, pg, pw, dg, dv, direction=nat.MATCH_DIR_EITHER, graded=False):
        """patient rows (packed genotypes pg, weights pw) against donor rows (dg, dv) under `direction` (a nat.MATCH_DIR_*)
        -> (H[2 nk + 1], L[nk]); graded: (H, G[nk][3]), G[k][g] the fold of L[k] with `mm == g` in the place of `mm == 0`"""
        nk = self.nk
        nb = 2 * nk + 1
        grades = (0, 1, 2) if graded else (0,)
        n_p, n_d = len(pw), len(dv)
        M = np.zeros((n_d, n_p), dtype=np.int64)  # M[j][i]
        at = []  # per kept locus and grade, per donor row: the patient rows with that many mismatches there, ascending
        for k in range(nk):
            mm = locus_mismatches(pg[0][k][None, :], pg[1][k][None, :], dg[0][k][:, None], dg[1][k][:, None], direction)
            M += mm
            per = []
            for g in grades:
                jj, ii = np.nonzero(mm == g)
                per.append((np.searchsorted(jj, np.arange(n_d + 1)).tolist(), ii.tolist()))
            at.append(per)
        M = M.tolist()
        H, G = [0.0] * nb, [[0.0] * len(grades) for _ in range(nk)]
        for j in range(n_d):
            v = dv[j]
            ts = [w * v for w in pw]
            ph = [0.0] * nb
            for m, t in zip(M[j], ts):
                ph[m] = ph[m] + t
            for m in range(nb):
                H[m] = H[m] + ph[m]
            for k in range(nk):
                for g, (bounds, ii) in enumerate(at[k]):
                    pl = 0.0
                    for i in ii[bounds[j]:bounds[j + 1]]:
                        pl = pl + ts[i]
                    G[k][g] = G[k][g] + pl
        return H, (G if graded else [row[0] for row in G])


def _total(ps):
    total = ps[0]
    for p in ps[1:]:
        total = total + p
    return total


def _slots_of(keep_mask):
    keep_mask = int(keep_mask)
    if keep_mask <= 0 or keep_mask >> nat.MAXL:
        raise ValueError("keep_mask is empty or names a locus slot beyond %d" % nat.MAXL)
    return [s for s in range(nat.MAXL) if (keep_mask >> s) & 1]


def _store(rec, slots, H, L):
    """H, L of a pair into one nat.MATCH_DT record, or H, G into one nat.MATCH_GRADE_DT record"""
    rec["mm"][:len(H)] = H
    field = "grade" if "grade" in rec.dtype.names else "locus"
    for k, s in enumerate(slots):
        rec[field][s] = L[k]


def _side(res, rows, slots, n_alleles, folder):
    """one side's subjects as the device prepares them -> (flags, [(packed genotypes, weights) or None])"""
    m = len(rows)
    flags = np.zeros(len(res), dtype=np.uint8)
    subs = []
    used = 0
    for i, r in enumerate(res):
        n, off = int(r["n_rows"][nat.T_UMUG]), int(r["row_off"][nat.T_UMUG])
        if int(r["status"]) != nat.ST_OK or n == 0 or off > m or n > m - off:
            subs.append(None)
            continue
        used += n
        ps = [float(rows[off + k]["prob"]) for k in range(n)]
        total = _total(ps)
        valid = math.isfinite(total) and total > 0.0
        private = undefined = False
        genos = []
        for k in range(n):
            a, b = int(rows[off + k]["a"]), int(rows[off + k]["b"])
            fa = [(a >> (nat.ABITS * s)) & 0xFFF for s in range(nat.MAXL)]
            fb = [(b >> (nat.ABITS * s)) & 0xFFF for s in range(nat.MAXL)]
            undefined |= any((x == 0) != (y == 0) for x, y in zip(fa, fb))
            private |= any(fa[s] > n_alleles[s] or fb[s] > n_alleles[s] for s in slots)
            genos.append(tuple((fa[s] or None, fb[s] or None) for s in slots))
        flags[i] = (nat.MATCH_VALID if valid else 0) | (nat.MATCH_PRIVATE if private else 0) | (nat.MATCH_UNDEFINED if undefined else 0)
        subs.append((folder.pack(genos), [p / total for p in ps]) if valid else None)
    if used > m:
        raise ValueError("the subjects' genotype rows overlap (more rows than there are)")
    return flags, subs


def match_records(pres, prows, dres, drows, keep_mask, n_alleles, groups=None, direction="either", graded=False):
    """The fold on record arrays (nat.RESULT_DT / nat.ROW_DT of the patients and of the donors) as grim_match_run_records
    defines it (include/grim_hip.h) -> (records nat.MATCH_DT[P][D], patient flags, donor flags, stats), laid out as the device
    lays them out: a pair that is not computed is a record of zeros; without donors every statistic is 0.  `groups`: an
    AlleleGroups (grim.groups) whose n_alleles are the ones given: both sides' rows are mapped first and n_groups stands in
    the place of n_alleles, as on the device with the map attached.  `direction`: "either", "gvh" (the patient's alleles the
    donor lacks) or "hvg" (the donor's alleles the patient lacks), the per-locus mismatch function; `graded`:
    the records are nat.MATCH_GRADE_DT, per locus the probabilities of exactly 0, 1 and 2 mismatches."""
    slots = _slots_of(keep_mask)
    direction = direction_code(direction)
    n_alleles = [int(x) for x in n_alleles] + [0] * (nat.MAXL - len(n_alleles))
    if groups is not None:
        if list(groups.n_alleles) != n_alleles:
            raise ValueError("the groups' n_alleles differ from the ones given")
        prows, drows, n_alleles = groups.map_records(prows), groups.map_records(drows), list(groups.n_groups)
    folder = _Folder(len(slots))
    pflags, psubs = _side(pres, prows, slots, n_alleles, folder)
    dflags, dsubs = _side(dres, drows, slots, n_alleles, folder)
    out = np.zeros((len(pres), len(dres)), dtype=nat.MATCH_GRADE_DT if graded else nat.MATCH_DT)
    stats = dict.fromkeys(nat.MATCH_STATS, 0)
    if len(dres) == 0:
        return out, pflags, dflags, stats
    for side, flags in (("patients", pflags), ("donors", dflags)):
        stats[side + "_valid"] = int(np.count_nonzero(flags & nat.MATCH_VALID))
        stats[side + "_private"] = int(np.count_nonzero(flags & nat.MATCH_PRIVATE))
        stats["undefined"] += int(np.count_nonzero(flags & nat.MATCH_UNDEFINED))
    ready = nat.MATCH_VALID | nat.MATCH_PRIVATE
    for p, ps in enumerate(psubs):
        if (pflags[p] & ready) != nat.MATCH_VALID:
            continue
        for d, ds in enumerate(dsubs):
            if (dflags[d] & ready) != nat.MATCH_VALID:
                continue
            H, L = folder.fold(ps[0], ps[1], ds[0], ds[1], direction, graded)
            _store(out[p, d], slots, H, L)
            stats["pairs"] += 1
            stats["row_pairs"] += len(ps[1]) * len(ds[1])
    return out, pflags, dflags, stats


def _text_subjects(text, keep):
    """`.umug` text -> [(id, [({locus: (x, y)}, p)])]: a subject is the run of rows from one rank 0 to the next"""
    subs = []
    sid = None
    for line in text.splitlines():
        if not line:
            continue
        f = line.split(",")
        if len(f) != 4:
            raise ValueError("not an id,genotype,probability,rank row: %r" % line)
        if int(f[3]) == 0 or f[0] != sid:
            sid = f[0]
            subs.append((sid, []))
        if int(f[3]) != len(subs[-1][1]):
            raise ValueError("ranks of subject %s are not 0..n-1" % f[0])
        geno = {}
        for part in f[1].split("^"):
            if not part:
                continue
            name = part.split("*", 1)[0]
            if name not in keep:
                continue
            pair = part.split("+")
            if len(pair) != 2:
                raise ValueError("not two alleles at locus %s: %r" % (name, line))
            geno[name] = (pair[0], pair[1])
        subs[-1][1].append((geno, float(f[2])))
    return subs


def match_umug_text(patient_text, donor_text, keep_loci, loci=None, groups=None, direction="either", graded=False):
    """The fold on `.umug` text in `id,genotype,p,rank` form -> (patient ids, donor ids, records[P][D]); a record is
    (mm[0..2|K|], {locus name: probability of no mismatch}).  A subject is the run of rows from one rank 0 to the next; a
    `^`-part of a genotype belongs to the locus named before its first `*`, its two alleles are the `+`-separated texts; a
    kept locus a row lacks is untyped; two alleles are equal when their texts are.  `loci`: the names that may be kept (an
    unknown one raises); `groups`: a group specification (grim.groups.GroupSpec or what it takes): both texts go through
    `regroup_umug_text` first.  `direction`: as `match_records`; `graded`: a record is (mm[0..2|K|], {locus name: [the
    probabilities of exactly 0, 1 and 2 mismatches]})."""
    direction = direction_code(direction)
    if groups is not None:
        patient_text, donor_text = regroup_umug_text(patient_text, groups), regroup_umug_text(donor_text, groups)
    keep = [keep_loci] if isinstance(keep_loci, str) else list(dict.fromkeys(keep_loci))
    if not keep:
        raise ValueError("keep_loci is empty")
    if loci is not None:
        _keep_mask({name: 0 for name in loci}, keep)
    folder = _Folder(len(keep))
    sides = []
    for text in (patient_text, donor_text):
        side = []
        for sid, rows in _text_subjects(text, set(keep)):
            total = _total([p for _, p in rows])
            if not (math.isfinite(total) and total > 0.0):
                raise ValueError("genotype rows of subject %s whose probabilities add up to %r" % (sid, total))
            genos = folder.pack([tuple(g.get(name, (None, None)) for name in keep) for g, _ in rows])
            side.append((sid, genos, [p / total for _, p in rows]))
        sides.append(side)
    records = []
    for _, pg, pw in sides[0]:
        line = []
        for _, dg, dv in sides[1]:
            H, L = folder.fold(pg, pw, dg, dv, direction, graded)
            line.append((H, dict(zip(keep, L))))
        records.append(line)
    return [s[0] for s in sides[0]], [s[0] for s in sides[1]], records


def text_records_array(records, locus_slot, graded=False):
    """records of match_umug_text -> nat.MATCH_DT[P][D] (nat.MATCH_GRADE_DT of its graded records); `locus_slot`: name -> slot
    (Graph.locus_slot)"""
    out = np.zeros((len(records), len(records[0]) if records else 0), dtype=nat.MATCH_GRADE_DT if graded else nat.MATCH_DT)
    field = "grade" if graded else "locus"
    for p, line in enumerate(records):
        for d, (H, L) in enumerate(line):
            out[p, d]["mm"][:len(H)] = H
            for name, v in L.items():
                out[p, d][field][int(locus_slot[name])] = v
    return out


class _Pairing:
    """What match_probabilities and search_donors share: the patients imputed as one block and set on the device object (a
    Matcher or a Searcher), the donors cut into blocks, the check of a block's flags, and the host fold of the pairs the
    device leaves out.  The callers run each donor block themselves and do what they like with the pairs."""

    def __init__(self, imputation, patient_lines, donor_lines_or_path, config, keep_loci, block_lines, planb, em, groups=None,
                 direction="either", graded=False):
        self.imputation = imputation
        self.direction, self.graded = direction_code(direction), bool(graded)  # of the text route, as of the device object
        self.g = g = imputation.netGraph
        self.groups = as_groups(g, groups)  # None: alleles compare as the dictionary has them
        self.mask = _keep_mask(g.locus_slot, keep_loci)
        self.slots = _slots_of(self.mask)
        self.dlines = [] if donor_lines_or_path is None else read_lines(donor_lines_or_path)  # None: given per donor_blocks call
        self.plines = [l.rstrip("\n") for l in patient_lines]
        if len(self.plines) > nat.MATCH_MAX_PAIRS:
            raise ValueError("%d patients: more than %d pairs with a single donor" % (len(self.plines), nat.MATCH_MAX_PAIRS))
        self.block_lines = max(1, min(int(block_lines), nat.MATCH_MAX_PAIRS // max(1, len(self.plines))))
        self.blocks = Blocks(imputation, config, planb, False, em, output_MUUG=True)
        self.ctx = self.blocks.ctx
        self.n_alleles = [g.adict.count(s) for s in range(len(g.full_loci))] + [0] * (nat.MAXL - len(g.full_loci))
        self.folder = _Folder(len(self.slots))  # of the text route
        self.patient_ok = np.zeros(len(self.plines), dtype=bool)
        self.pblock = self._cut = None
        self.pf = np.zeros(0, dtype=np.uint8)
        self.ptext = {}  # patient -> its rows on allele text
        imputation.unsupported = []

    def set_patients(self, dev, patient_flags, stats):
        """the patients as one block onto `dev`; `patient_flags`: () -> their flags on the device.  Their batch is closed as
        soon as they are set: the records are on the host, the patients prepared on the device; the tokenised lines stay for
        the text route.  The group map, when there is one, is attached first (that drops whatever patients `dev` held)."""
        if self.groups is not None:
            dev_groups = nat.Groups.of(self.ctx, self.groups)
            try:
                dev.set_groups(dev_groups)  # `dev` keeps its own copy of the tables
            finally:
                dev_groups.close()
        self.pblock = self.blocks.block(self.plines)
        if self.pblock.batch is not None:
            dev.set_patients(*self.pblock.records())
            self.pf = patient_flags()
            self.pblock.batch.close()
        self.check(self.pblock, self.pf)
        self.patient_ok[self.pblock.line_of[np.flatnonzero(self.pf & nat.MATCH_VALID)]] = True
        stats["patients_valid"] = int(np.count_nonzero(self.pf & nat.MATCH_VALID))
        stats["patients_private"] = int(np.count_nonzero(self.pf & nat.MATCH_PRIVATE))

    def donor_blocks(self, lines=None, first=0):
        """the blocks of the donor lines given at construction, or of `lines`, which begin at line `first` of the donor input
        (a consumer that is fed its donors piece by piece); the cut before it is closed"""
        if self._cut is not None:
            self._cut.close()
        self._cut = self.blocks.cut(self.dlines if lines is None else lines, self.block_lines, first)
        return self._cut

    def check(self, block, flags):
        """a block after its run: its unsupported subjects noted (the records are fetched for them only when some subject
        has no flag at all), and no subject's match undefined"""
        note_unsupported(self.imputation, block.bad + (block.unsupported() if block.batch is not None and not flags.all() else []))
        if np.count_nonzero(flags & nat.MATCH_UNDEFINED):
            raise ValueError("%d subject(s) hold a genotype row whose haplotypes are typed at different loci: their match is "
                             "not defined" % np.count_nonzero(flags & nat.MATCH_UNDEFINED))

    def host_pairs(self, block, df):
        """a donor block after its run, `df` its flags: checks it, then yields (p, d, H, L) for every pair of valid subjects
        the device left out for a private allele: the same fold on allele text (L is G[nk][3] when graded)"""
        self.check(block, df)
        ready = nat.MATCH_VALID | nat.MATCH_PRIVATE
        pf, ptext, dtext = self.pf, self.ptext, {}
        for p in np.flatnonzero(pf & nat.MATCH_VALID):
            for d in np.flatnonzero(df & nat.MATCH_VALID):
                if (pf[p] & ready) == nat.MATCH_VALID and (df[d] & ready) == nat.MATCH_VALID:
                    continue
                if p not in ptext:
                    ptext[p] = self._text_subject(self.pblock, int(p))
                if d not in dtext:
                    dtext[d] = self._text_subject(block, int(d))
                H, L = self.folder.fold(ptext[p][0], ptext[p][1], dtext[d][0], dtext[d][1], self.direction, self.graded)
                yield p, d, H, L

    def _text_subject(self, block, i):
        """device subject i of `block`: its rows on allele text -> (packed genotypes, weights)"""
        res, rows = block.records()
        n, off = int(res[i]["n_rows"][nat.T_UMUG]), int(res[i]["row_off"][nat.T_UMUG])
        line = int(block.line_of[i])
        names = {}

        def text(s, f):
            if f == 0:
                return None
            if (s, f) not in names:  # an id above the dictionary's is the line's own
                name = block.parsed.allele(line, s, f - 1) if f > self.n_alleles[s] else self.g.key_alleles(f << (nat.ABITS * s))[s]
                names[(s, f)] = name if self.groups is None else self.groups.spec.name(self.g.slot_locus[s], name)
            return names[(s, f)]

        ps = [float(rows[off + k]["prob"]) for k in range(n)]
        total = _total(ps)
        genos = []
        for k in range(n):
            a, b = int(rows[off + k]["a"]), int(rows[off + k]["b"])
            genos.append(tuple((text(s, (a >> (nat.ABITS * s)) & 0xFFF), text(s, (b >> (nat.ABITS * s)) & 0xFFF)) for s in self.slots))
        return self.folder.pack(genos), [p / total for p in ps]

    def close(self):
        if self._cut is not None:
            self._cut.close()
        if self.pblock is not None:
            self.pblock.close()


def match_probabilities(imputation, patient_lines, donor_lines_or_path, config, keep_loci, block_lines=65536, planb=None, em=False,
                        groups=None, direction="either", graded=False):
    """Match probabilities of every patient against every donor on the device.  `patient_lines`: input lines;
    `donor_lines_or_path`: input lines (a list) or the path of an input file; `config`: the configuration dict of
    `load_config`; `keep_loci`: locus names of its loci_map.  The patients are imputed as one device batch, their records
    fetched and set once; the donors are cut into blocks of `block_lines` lines (lowered so that patients x block stays within
    GRIM_MATCH_MAX_PAIRS), each tokenised, imputed as one device batch (genotype output on, the rest as configured) and matched
    where its rows lie.  Pairs the device leaves out because a subject holds an allele the dictionary does not know are folded
    here on allele text.  -> (patient_ok, donor_ok, records, stats): records is nat.MATCH_DT[len(patient_lines)][len(donor
    lines)], zero for lines without genotype rows; *_ok say which lines have them; stats adds `blocks`, `kernel_ms` and
    `host_pairs` (pairs folded on text).  The cuts do not show in any byte.  Subjects the device cannot answer follow
    `imputation.on_unsupported` as in `impute_lines_block`.  `groups`: an AlleleGroups of the imputation's graph or a group
    specification (grim.groups): alleles are equal when their groups are -- on the device by group id, in the pairs folded
    here by group name -- and the result equals `match_umug_text` on the regrouped text.  `direction`, `graded`: as
    `match_records`, on the device (csrc/grim_match.h) and in the pairs folded here; graded, records is
    nat.MATCH_GRADE_DT."""
    pairing = _Pairing(imputation, patient_lines, donor_lines_or_path, config, keep_loci, block_lines, planb, em, groups, direction,
                       graded)
    graded = pairing.graded
    matcher = nat.Matcher(pairing.ctx, pairing.mask, pairing.n_alleles, pairing.direction, graded)
    results = matcher.results_graded if graded else matcher.results
    stats = dict.fromkeys(nat.MATCH_STATS, 0)
    stats.update(blocks=0, kernel_ms=0.0, host_pairs=0)
    out = np.zeros((len(pairing.plines), len(pairing.dlines)), dtype=nat.MATCH_GRADE_DT if graded else nat.MATCH_DT)
    donor_ok = np.zeros(len(pairing.dlines), dtype=bool)
    try:
        pairing.set_patients(matcher, lambda: results()[1], stats)
        for block in pairing.donor_blocks():
            if block.batch is None:
                pairing.check(block, np.zeros(0, dtype=np.uint8))
                continue
            matcher.run(block.batch)
            rec, _, df = results()
            run = matcher.stats()
            for p, d, H, L in pairing.host_pairs(block, df):
                _store(rec[p, d], pairing.slots, H, L)
                stats["host_pairs"] += 1
            for k in ("donors_valid", "donors_private", "pairs", "row_pairs"):
                stats[k] += run[k]
            stats["kernel_ms"] += matcher.kernel_ms()
            stats["blocks"] += 1
            donor_ok[block.lo + block.line_of[np.flatnonzero(df & nat.MATCH_VALID)]] = True
            if len(pairing.pf):
                out[pairing.pblock.line_of[:, None], block.lo + block.line_of[None, :]] = rec
    finally:
        pairing.close()
        matcher.close()
    return pairing.patient_ok, donor_ok, out, stats


def line_id(line):
    """the subject id of an input line as the tokenizer takes it: the field before the first ',' when the line has one, else
    before the first '%' (impute.py:2024-2027)"""
    return line.split("," if "," in line else "%", 1)[0]


def match_file(conf_file, patients_path, keep_loci, out_path, graph=None, min_p0=0.0, block_lines=65536, groups=None,
               direction="either", graded=False):
    """The configuration's input file as donors against the input file `patients_path`, on `graph` (built from the
    configuration's graph CSVs when None) -> a CSV at `out_path`: a header `patient_id,donor_id,mm0,...,mm{2|K|},<kept locus
    names>`, then one line per computed pair with mm0 >= min_p0, patient-major, floats written with repr.  Paths are taken
    as the configuration gives them.  `groups`, `direction`: as `match_probabilities`.  `graded`: after the kept locus names
    (the probability of no mismatch there) come `<locus>_mm1,<locus>_mm2` for every kept locus, the probabilities of exactly
    one and of two mismatches.  -> stats"""
    from .grim import graph_instance
    from .imputation.impute import Imputation
    from .run_impute_def import load_config

    config, _ = load_config(conf_file)
    if graph is None:
        graph = graph_instance(config)
    imp = Imputation(graph, config)
    plines, dlines = read_lines(patients_path), read_lines(config["imputation_input_file"])
    pok, dok, rec, stats = match_probabilities(imp, plines, dlines, config, keep_loci, block_lines=block_lines, groups=groups,
                                               direction=direction, graded=graded)
    slots = _slots_of(_keep_mask(graph.locus_slot, keep_loci))
    nb = 2 * len(slots) + 1
    pid, did = [line_id(l) for l in plines], [line_id(l) for l in dlines]
    with open(out_path, "w") as fh:
        more = ["%s_mm%d" % (graph.slot_locus[s], g) for s in slots for g in (1, 2)] if graded else []
        fh.write(",".join(["patient_id", "donor_id"] + ["mm%d" % m for m in range(nb)] + [graph.slot_locus[s] for s in slots] + more) + "\n")
        for p in np.flatnonzero(pok):
            for d in np.flatnonzero(dok):
                r = rec[p, d]
                if float(r["mm"][0]) >= min_p0:
                    if graded:
                        vals = [float(x) for x in r["mm"][:nb]] + [float(r["grade"][s][0]) for s in slots]
                        vals += [float(r["grade"][s][g]) for s in slots for g in (1, 2)]
                    else:
                        vals = [float(x) for x in r["mm"][:nb]] + [float(r["locus"][s]) for s in slots]
                    fh.write("%s,%s,%s\n" % (pid[p], did[d], ",".join(repr(v) for v in vals)))
    return stats
