"""
Allele groups: the marginal tables (grim.marginal), the match (grim.match) and the search (grim.search) at a chosen
resolution -- antigen level (`A*02`), two fields, P or G groups, any table -- instead of the resolution the graph was built at
(DESIGN 4.11).

A *group map* gives for every locus slot s a table T_s[0 .. n_alleles[s]] and a count n_groups[s]: T_s[0] == 0, and a
dictionary allele id f in 1..n_alleles[s] belongs to group T_s[f] in 1..n_groups[s].  A key's 12-bit field f becomes

    0                                 if f == 0                    untyped stays untyped
    T_s[f]                            if 1 <= f <= n_alleles[s]
    n_groups[s] + (f - n_alleles[s])  if f > n_alleles[s]           private to the subject: stays private, keeps its index

and the consumers run their contracts on the mapped rows, n_groups in the place of n_alleles.  The device cannot know which
group an allele it has never seen belongs to: those subjects and pairs are folded here on group *names*.

`GroupSpec` is the text function allele name -> group name and needs no graph; `AlleleGroups` are the device's tables, built
from a graph's dictionary through a GroupSpec; `regroup_umug_text` rewrites `.umug` text allele by allele, so that the grouped
text twins are, by definition, the existing twins applied to regrouped text.  No table is shipped with the package.
"""

import csv
import os

import numpy as np

from . import _native as nat

RULES = ("first_field", "two_field")


def _fields(allele, n):
    """the text up to the n-th ':'; unchanged with n fields or fewer"""
    parts = allele.split(":")
    return allele if len(parts) <= n else ":".join(parts[:n])


def _locus_of(name):
    return name.split("*", 1)[0]


def _read_csv(path):
    table = {}
    with open(path, newline="") as fh:
        for row in csv.reader(fh):
            if not row or (len(row) == 1 and not row[0].strip()):
                continue
            if len(row) != 2:
                raise ValueError("%s: not an allele,group row: %r" % (path, row))
            allele, group = row[0].strip(), row[1].strip()
            if (allele, group) == ("allele", "group"):
                continue
            table[allele] = group
    return table


def _rule(rule):
    """a rule as given -> None, one of RULES, or a dict allele -> group (checked: a group stays inside its allele's locus)"""
    if rule is None or rule in RULES:
        return rule
    if isinstance(rule, (str, bytes, os.PathLike)):
        rule = _read_csv(rule)
    if not isinstance(rule, dict):
        raise ValueError("not a rule: %r (one of %s, None, a dict allele -> group, or the path of an allele,group CSV)" % (rule, ", ".join(RULES)))
    for allele, group in rule.items():
        if _locus_of(group) != _locus_of(allele):
            raise ValueError("group %r of allele %r names another locus" % (group, allele))
    return dict(rule)


class GroupSpec:
    """The text function `name(locus, allele) -> group name`.  `spec`: one rule for all loci, or a dict locus -> rule (loci not
    named are identity).  A rule is "first_field" (the text up to the first ':'; unchanged when there is none), "two_field" (the
    text up to the second ':'; unchanged with two fields or fewer), None (identity), a dict allele -> group, or the path of a
    two-column `allele,group` CSV (alleles not listed map to themselves).  A top-level dict whose keys hold a '*' is one table
    for all loci.  A group name whose text before '*' is not the locus raises ValueError."""

    def __init__(self, spec):
        if isinstance(spec, GroupSpec):
            self.default, self.by_locus = spec.default, dict(spec.by_locus)
            return
        self.default, self.by_locus = None, {}
        if isinstance(spec, dict) and not any("*" in str(k) for k in spec):
            self.by_locus = {str(locus): _rule(rule) for locus, rule in spec.items()}
        else:
            self.default = _rule(spec)

    def rule(self, locus):
        return self.by_locus.get(locus, self.default)

    def is_identity(self, locus):
        return self.rule(locus) is None

    def name(self, locus, allele):
        rule = self.rule(locus)
        if rule is None:
            return allele
        if rule == "first_field":
            group = _fields(allele, 1)
        elif rule == "two_field":
            group = _fields(allele, 2)
        else:
            group = rule.get(allele, allele)
        if _locus_of(group) != locus:
            raise ValueError("group %r of allele %r is not of locus %s" % (group, allele, locus))
        return group


class AlleleGroups:
    """The device's tables of a GroupSpec on a graph's allele dictionary (`graph.adict`, ids as `graph.key_alleles` reads
    them).  Group ids per slot are 1, 2, ... in the order of first appearance over the allele ids 1..n_alleles[s].
    `table[s]`: uint16[n_alleles[s] + 1] with table[s][0] == 0; `names[s][gid]` the group's name, names[s][0] == "";
    `n_alleles`, `n_groups`: one count per slot up to nat.MAXL; `watch_mask`: the slots whose table is not the identity;
    `spec`: the GroupSpec."""

    def __init__(self, graph, spec):
        adict = graph.adict
        alleles = [[adict.name(s, i) for i in range(adict.count(s))] for s in range(len(graph.slot_locus))]
        self._build(list(graph.slot_locus), alleles, spec)

    @classmethod
    def from_names(cls, slot_locus, alleles, spec):
        """`alleles[s]`: the names of slot s's allele ids 1, 2, ... in id order (a dictionary without a graph)"""
        self = cls.__new__(cls)
        self._build(list(slot_locus), [list(a) for a in alleles], spec)
        return self

    def _build(self, slot_locus, alleles, spec):
        if len(slot_locus) > nat.MAXL:
            raise ValueError("more than %d loci" % nat.MAXL)
        self.spec = spec if isinstance(spec, GroupSpec) else GroupSpec(spec)
        self.slot_locus = slot_locus + [None] * (nat.MAXL - len(slot_locus))
        self.table, self.names, self.n_alleles, self.n_groups = [], [], [], []
        self.watch_mask = 0
        self.rule_mask = sum(1 << s for s, locus in enumerate(slot_locus) if not self.spec.is_identity(locus))  # slots with a rule
        for s in range(nat.MAXL):
            own = alleles[s] if s < len(alleles) else []
            if len(own) > 4095:
                raise ValueError("more than 4095 alleles at locus slot %d" % s)
            ids, names = {}, [""]
            table = np.zeros(len(own) + 1, dtype=np.uint16)
            for f, allele in enumerate(own, 1):
                group = self.spec.name(self.slot_locus[s], allele)
                if group not in ids:
                    ids[group] = len(names)
                    names.append(group)
                table[f] = ids[group]
            if (table != np.arange(len(table))).any():
                self.watch_mask |= 1 << s
            self.table.append(table)
            self.names.append(names)
            self.n_alleles.append(len(own))
            self.n_groups.append(len(names) - 1)

    def flat(self):
        """the slots' tables back to back, as grim_groups_create takes them"""
        return np.ascontiguousarray(np.concatenate(self.table), dtype=np.uint16)

    def map_field(self, s, f):
        f, n = int(f), self.n_alleles[s]
        return 0 if f == 0 else int(self.table[s][f]) if f <= n else self.n_groups[s] + (f - n)

    def map_keys(self, keys):
        """uint64 keys -> mapped keys (bits at 60 and above copied)"""
        keys = np.asarray(keys, dtype=np.uint64)
        out = keys & ~np.uint64((1 << (nat.ABITS * nat.MAXL)) - 1)
        for s in range(nat.MAXL):
            f = ((keys >> np.uint64(nat.ABITS * s)) & np.uint64(0xFFF)).astype(np.int64)
            n, ng = self.n_alleles[s], self.n_groups[s]
            known = self.table[s][np.minimum(f, n)].astype(np.int64)
            g = np.where(f > n, ng + (f - n), known)
            out |= g.astype(np.uint64) << np.uint64(nat.ABITS * s)
        return out

    def map_records(self, rows):
        """the CPU twin of gp_map_kernel: nat.ROW_DT rows -> mapped rows (prob, popa, popb untouched)"""
        rows = np.ascontiguousarray(rows, dtype=nat.ROW_DT)
        out = rows.copy()
        out["a"], out["b"] = self.map_keys(rows["a"]), self.map_keys(rows["b"])
        return out

    def flags(self, res, rows, keep_mask, watch=None):
        """the twin of gp_flag_kernel: per subject nat.GROUPS_PRIVATE when its rows can be read and some UMUG row holds a
        private field in a kept slot that is not an identity slot (`watch`: another set of slots than watch_mask)"""
        m = len(rows)
        mask = int(keep_mask) & (self.watch_mask if watch is None else int(watch))
        out = np.zeros(len(res), dtype=np.uint8)
        for i, r in enumerate(res):
            n, off = int(r["n_rows"][nat.T_UMUG]), int(r["row_off"][nat.T_UMUG])
            if int(r["status"]) != nat.ST_OK or n == 0 or off > m or n > m - off:
                continue
            for s in range(nat.MAXL):
                if (mask >> s) & 1:
                    for side in ("a", "b"):
                        f = (rows[side][off:off + n] >> np.uint64(nat.ABITS * s)) & np.uint64(0xFFF)
                        if (f > np.uint64(self.n_alleles[s])).any():
                            out[i] = nat.GROUPS_PRIVATE
        return out


def as_groups(graph, groups):
    """what a device function or a record twin is given as `groups` -> AlleleGroups (None stays None)"""
    if groups is None or isinstance(groups, AlleleGroups):
        return groups
    return AlleleGroups(graph, groups)


def regroup_umug_text(text, spec):
    """`.umug` text in `id,genotype,p,rank` form with every allele replaced by its group's name; each locus pair is sorted
    again as strings; no rows are merged and no number is touched"""
    spec = spec if isinstance(spec, GroupSpec) else GroupSpec(spec)
    out = []
    for line in text.splitlines():
        if not line:
            continue
        f = line.split(",")
        if len(f) != 4:
            raise ValueError("not an id,genotype,probability,rank row: %r" % line)
        parts = []
        for part in f[1].split("^"):
            if part:
                locus = _locus_of(part)
                part = "+".join(sorted(spec.name(locus, allele) for allele in part.split("+")))
            parts.append(part)
        f[1] = "^".join(parts)
        out.append(",".join(f) + "\n")
    return "".join(out)
