"""
Constructed cases for the chunk fast path: device tokenizer (csrc/grim_tokdev.h) -> half-wave kernel (csrc/grim_small.h)
-> row compaction.  A designed one-population graph ("toy", population TOY, loci A B C DQB1 DRB1) whose frequency rows
are written by hand, a plain restatement of the device tokenizer's acceptance rule, one input line per verdict class with
the expected verdict attached, and helpers that place a line at a given 16-byte alignment or next to a given wave
neighbour.  Pure Python and numpy; reads nothing outside the repository.  tests/test_fast_path_cases.py checks that every
case is what it claims to be (without a GPU), tests/test_fast_path_gpu.py runs them.
"""

import gzip
import itertools
import json
import os

import numpy as np

import harness

LOCI = ["A", "B", "C", "DQB1", "DRB1"]
POP = "TOY"
GRAPH = "toy"
TOKNAME = 24   # GRIM_TOKNAME: longest allele name of the device dictionary
TOK_MAXGL = 144  # GRIM_TOK_MAXGL: longest GL field the host offers to the device tokenizer
TRIM = 1e-12   # freq_trim_threshold of the toy graph: cut-off = TRIM / rows, far below every designed row

ACCEPTED, HANDED_BACK, NOT_OFFERED = "accepted", "handed_back", "not_offered"


# ---- the hash of csrc/grim_tok.h, restated ---------------------------------------------------------------------------------
def tokname_hash(name):
    b = name.encode() if isinstance(name, str) else bytes(name)
    assert 0 < len(b) <= TOKNAME
    w = [0] * 6
    for k, c in enumerate(b):
        w[k >> 2] |= c << (24 - 8 * (k & 3))
    m = 0xFFFFFFFF
    h = (len(b) * 0x9E3779B1) & m
    for x in w:
        h ^= x
        h = (h * 0x85EBCA6B) & m
        h ^= h >> 15
    h = (h * 0xC2B2AE35) & m
    h ^= h >> 16
    return h


def table_capacity(n_alleles):
    """engine_devdict_create: the smallest power of two >= max(16, 4 * alleles of the locus)"""
    cap = 16
    while cap < 4 * n_alleles:
        cap <<= 1
    return cap


# ---- names -----------------------------------------------------------------------------------------------------------------
def nm(locus, tag, k):
    return "%s*%02d:%02d" % (locus, tag, k)


def long_name(locus, tag, n):
    """a name of exactly n bytes: digits and colons only (no 'g', 'L', 'U', '/')"""
    s = "%s*%02d" % (locus, tag)
    while len(s) + 3 <= n:
        s += ":01"
    return s + "7" * (n - len(s))


def hap(names):
    """names by locus (dict or list in LOCI order) -> the haplotype string of a frequency row"""
    if isinstance(names, dict):
        names = [names[l] for l in LOCI]
    return "~".join(names)


def gl_of(h1, h2):
    """the fully typed GL of the two haplotypes (lists in LOCI order): side 0 = h1, side 1 = h2"""
    return "^".join("%s+%s" % (a, b) for a, b in zip(h1, h2))


def tagged(tag, k, **over):
    names = [nm(l, tag, k) for l in LOCI]
    for l, v in over.items():
        names[LOCI.index(l)] = v
    return names


# ---- the designed rows -----------------------------------------------------------------------------------------------------
class Toy:
    """the rows of the toy graph and what the cases need to know about them"""

    def __init__(self):
        self.rows = []       # (haplotype string, frequency)
        self.freq = {}       # haplotype string -> frequency
        self.subjects = {}   # behaviour class -> GL
        self._build()
        self.alleles = {l: set() for l in LOCI}
        for h, _ in self.rows:
            for l, a in zip(LOCI, h.split("~")):
                self.alleles[l].add(a)
        self.capacity = {l: table_capacity(len(self.alleles[l])) for l in LOCI}
        self._check_slots()

    def add(self, names, f):
        h = hap(names)
        assert h not in self.freq, h
        self.freq[h] = f
        self.rows.append((h, f))
        return list(names)

    def _build(self):
        S = self.subjects
        # cube T: all 32 haplotypes over two alleles per locus at one frequency -> 16 accepted phases, all tied
        self.cube_t = [[nm(l, 1, 1) for l in LOCI], [nm(l, 2, 1) for l in LOCI]]
        for c in range(32):
            self.add([self.cube_t[(c >> k) & 1][k] for k in range(5)], 0.02)
        S["cube_t"] = gl_of(*self.cube_t)
        # cube D: 32 distinct frequencies over about three decades, pair products pairwise distinct
        self.cube_d = [[nm(l, 3, 1) for l in LOCI], [nm(l, 4, 1) for l in LOCI]]
        order = np.random.default_rng(5).permutation(32)
        fd = [float("%.6g" % (0.03 * 10.0 ** (-3.0 * int(order[c]) / 31.0))) for c in range(32)]
        for c in range(32):
            self.add([self.cube_d[(c >> k) & 1][k] for k in range(5)], fd[c])
        prods = [fd[c] * fd[c ^ 31] for c in range(16)]
        assert len(set(prods)) == 16 and len(set(fd)) == 32, "cube D: pair products must be pairwise distinct"
        assert max(fd) / min(fd) > 900.0
        S["cube_d"] = gl_of(*self.cube_d)
        # one haplotype pair, by the ladder step that first accepts it (epsilon 1e-3: steps 1e-4 ... 1e-9, 0)
        for cls, tag, f in (("step0", 10, 0.02), ("mid", 11, 5e-4), ("last", 12, 1e-5)):
            h1, h2 = self.add(tagged(tag, 1), f), self.add(tagged(tag, 2), f)
            S[cls] = gl_of(h1, h2)
        # fully typed, every allele known, no haplotype pair: loci A B C of one pair, DQB1 DRB1 of another -> Plan B
        S["planb"] = gl_of(tagged(10, 1)[:3] + tagged(11, 1)[3:], tagged(10, 2)[:3] + tagged(11, 2)[3:])
        S["planb2"] = gl_of(tagged(11, 1)[:3] + tagged(12, 1)[3:], tagged(11, 2)[:3] + tagged(12, 2)[3:])
        # final cut (eps = MaxProb / 100000): a dominant pair P+Q (2 * 0.02 * 0.02 = 8e-4 -> eps 8e-9) and a weak pair R+S
        # of the other phase, below the cut (5e-5 * 5e-5 = 2.5e-9) and, in the twin, just above it (1e-4 * 1e-4 = 1e-8)
        for cls, tag, weak in (("cut_drop", 13, 5e-5), ("cut_keep", 14, 1e-4)):
            p, q = self.add(tagged(tag, 1), 0.02), self.add(tagged(tag, 2), 0.02)
            self.add(tagged(tag, 1, A=nm("A", tag, 2)), weak)
            self.add(tagged(tag, 2, A=nm("A", tag, 1)), weak)
            S[cls] = gl_of(p, q)
        # homozygous positions: one (A), the last locus alone (the locus-5 rule), all five
        self.add(tagged(10, 2, A=nm("A", 10, 1)), 0.02)
        S["hom_a"] = gl_of(tagged(10, 1), tagged(10, 2, A=nm("A", 10, 1)))
        self.add(tagged(10, 2, DRB1=nm("DRB1", 10, 1)), 0.02)
        S["hom_drb1"] = gl_of(tagged(10, 1), tagged(10, 2, DRB1=nm("DRB1", 10, 1)))
        S["hom_all"] = gl_of(tagged(10, 1), tagged(10, 1))
        # names of exactly 24 bytes (side 0 at A; side 1 at DRB1) and of 25 bytes
        self.n24a, self.n24r, self.n25 = long_name("A", 30, 24), long_name("DRB1", 32, 24), long_name("A", 31, 25)
        h1, h2 = self.add(tagged(30, 1, A=self.n24a), 0.02), self.add(tagged(30, 2), 0.02)
        S["name24_side0"] = gl_of(h1, h2)
        h1, h2 = self.add(tagged(32, 1), 0.02), self.add(tagged(32, 2, DRB1=self.n24r), 0.02)
        S["name24_side1"] = gl_of(h1, h2)
        h1, h2 = self.add(tagged(31, 1, A=self.n25), 0.02), self.add(tagged(31, 2), 0.02)
        S["name25"] = gl_of(h1, h2)
        # names that are prefixes of one another: X*01:01 (cube T), X*01:01:01, X*01:01:01:01
        pf1, pf2 = [nm(l, 1, 1) + ":01" for l in LOCI], [nm(l, 1, 1) + ":01:01" for l in LOCI]
        self.add(pf1, 0.02)
        self.add(pf2, 0.02)
        S["prefix_12"] = gl_of(self.cube_t[0], pf1)
        S["prefix_23"] = gl_of(pf1, pf2)
        S["prefix_13"] = gl_of(self.cube_t[0], pf2)
        # a graph allele that ends with 'U': on side 1 clean_up_gl drops the position, on side 0 nothing happens
        self.name_u = "DRB1*50:01U"
        h1, h2 = self.add(tagged(50, 1, DRB1=self.name_u), 0.02), self.add(tagged(50, 2), 0.02)
        S["u_end_side0"] = gl_of(h1, h2)
        S["u_end_side1"] = gl_of(h2, h1)
        # ten long names: a GL field of exactly 144 bytes (five of 13 bytes + five of 14 + nine separators), and one of 145
        l13 = [long_name(l, 60, 13) for l in LOCI]
        l14 = [long_name(l, 61, 14) for l in LOCI]
        l14b = [long_name("A", 62, 14)] + l13[1:]
        self.add(l13, 0.02)
        self.add(l14, 0.02)
        self.add(l14b, 0.02)
        S["gl144"] = gl_of(l13, l14)
        S["gl145"] = gl_of(l14b, l14)
        assert len(S["gl144"]) == TOK_MAXGL and len(S["gl145"]) == TOK_MAXGL + 1
        # locus C: names found by brute force whose home slot is the table's last (probes wrap) or one shared other slot (a
        # chain).  The allele count of C -- and so the table size -- is fixed before the search: six names are added.
        n_c = len({h.split("~")[2] for h, _ in self.rows}) + 1 + 6  # + C*40:02 below
        cap = table_capacity(n_c)
        by_slot = {}
        for t, k in itertools.product(range(40, 100), range(3, 100)):
            by_slot.setdefault(tokname_hash(nm("C", t, k)) & (cap - 1), []).append(nm("C", t, k))
        self.wrap_names = by_slot[cap - 1][:3]
        self.chain_slot = next(s for s in sorted(by_slot) if s not in (0, 1, 2, cap - 1) and len(by_slot[s]) >= 3)
        self.chain_names = by_slot[self.chain_slot][:3]
        assert len(self.wrap_names) == 3
        partner = self.add(tagged(40, 2), 0.02)
        for i, c in enumerate(self.wrap_names + self.chain_names):
            h1 = self.add(tagged(40, 1, C=c), 0.02)
            S[("wrap%d" % i) if i < 3 else ("chain%d" % (i - 3))] = gl_of(h1, partner)
        assert len({h.split("~")[2] for h, _ in self.rows}) == n_c
        assert len(self.rows) <= 300

    def _check_slots(self):
        mask = self.capacity["C"] - 1
        assert all(tokname_hash(n) & mask == mask for n in self.wrap_names)
        assert all(tokname_hash(n) & mask == self.chain_slot for n in self.chain_names)

    def dictionary(self):
        """locus -> the allele names of the graph"""
        return {l: set(v) for l, v in self.alleles.items()}

    def names(self):
        return sorted(a for v in self.alleles.values() for a in v)


_toy = None


def toy():
    global _toy
    if _toy is None:
        _toy = Toy()
    return _toy


def ensure_toy_graph():
    """builds the toy graph with the product's generator into tests/_work/toy (as harness.ensure_graph does for the committed
    frequency files) and registers it with the harness; -> the graph's name"""
    from graph_generation.generate_hpf import produce_hpf
    from graph_generation.generate_neo4j_multi_hpf import generate_graph

    harness.POPS[GRAPH] = [POP]
    harness.GRAPH_OVERRIDES[GRAPH] = {"freq_trim_threshold": TRIM}
    work = os.path.join(harness.WORK, GRAPH)
    T = toy()
    stamp = os.path.join(work, "rows.json")
    want = json.dumps(T.rows)
    marker = os.path.join(work, "output", "csv", "info_node.csv")
    if os.path.exists(marker) and os.path.exists(stamp) and open(stamp).read() == want:
        return GRAPH
    if os.path.exists(marker):
        os.remove(marker)
    os.makedirs(os.path.join(work, "data", "freqs"), exist_ok=True)
    os.makedirs(os.path.join(work, "data", "subjects"), exist_ok=True)
    with gzip.open(os.path.join(work, "data", "freqs", POP + ".freqs.gz"), "wt") as fh:
        for h, f in T.rows:
            fh.write("%s,1,%r\n" % (h, f))
    for stale in ("output/pop_counts_file.txt",):
        if os.path.exists(os.path.join(work, stale)):
            os.remove(os.path.join(work, stale))
    conf = toy_conf()
    with open(os.path.join(work, "graph_conf.json"), "w") as fh:
        json.dump(conf, fh)
    cwd = os.getcwd()
    os.chdir(work)
    try:
        produce_hpf("graph_conf.json", quiet=True)
        generate_graph("graph_conf.json", quiet=True)
    finally:
        os.chdir(cwd)
    with open(stamp, "w") as fh:
        fh.write(want)
    harness._graph_cache.pop(GRAPH, None)
    harness._ograph_cache.pop(GRAPH, None)
    return GRAPH


def toy_conf(**over):
    conf = harness.base_conf([POP])
    conf["freq_trim_threshold"] = TRIM
    conf.update(over)
    return conf


# ---- the acceptance rule of the device tokenizer, restated -----------------------------------------------------------------
def device_tokenizer_verdict(gl, dictionary, device_tokenizer=True):
    """-> NOT_OFFERED, ACCEPTED or HANDED_BACK for the GL field of an input line.  `dictionary`: locus name -> set of the
    graph's allele names.  From the header comment of csrc/grim_tokdev.h and from what tokenise_gl_fast (csrc/grim_host.cpp)
    accepts for a line with one allele per side."""
    if not device_tokenizer or not gl or len(gl.encode()) > TOK_MAXGL or "/" in gl:
        return NOT_OFFERED
    if "g" in gl or "L" in gl:
        return HANDED_BACK  # clean_up_gl would delete characters
    positions = gl.split("^")
    if len(positions) != 5:
        return HANDED_BACK
    sides = [p.split("+") for p in positions]
    if any(len(s) != 2 for s in sides):
        return HANDED_BACK  # (with nine separators in all, this is "'+' and '^' alternate, '+' first")
    loci = []
    for s0, s1 in sides:
        for a in (s0, s1):
            if not 1 <= len(a.encode()) <= TOKNAME:
                return HANDED_BACK
        if s0.startswith("U") or s1.endswith("U"):
            return HANDED_BACK  # clean_up_gl drops the position
        pre = []
        for a in (s0, s1):
            star = a.find("*")
            if star < 0:
                star = len(a)
            if star > 8 or a[:star] not in dictionary:
                return HANDED_BACK
            pre.append(a[:star])
        if pre[0] != pre[1]:
            return HANDED_BACK
        loci.append(pre[0])
    for side in (0, 1):
        col = [s[side].encode() for s in sides]
        if any(not col[k] < col[k + 1] for k in range(4)):
            return HANDED_BACK  # gl2haps would sort the side into another order (or two names are equal)
    if len(set(loci)) != 5 or set(loci) != set(dictionary):
        return HANDED_BACK
    for (s0, s1), l in zip(sides, loci):
        if s0 not in dictionary[l] or s1 not in dictionary[l]:
            return HANDED_BACK
    return ACCEPTED


def line_verdict(line, dictionary, device_tokenizer=True):
    """the verdict for a whole input line: the host offers the second field of a line of two, or of four and more, fields"""
    line = line.rstrip()
    sep = "," if "," in line else "%"
    f = line.split(sep)
    if len(f) < 2 or len(f) == 3:
        return NOT_OFFERED
    return device_tokenizer_verdict(f[1], dictionary, device_tokenizer)


def count_verdicts(lines, dictionary, device_tokenizer=True):
    """-> (offered, handed_back) as grim_stream_devtok_lines reports them"""
    v = [line_verdict(l, dictionary, device_tokenizer) for l in lines]
    return sum(x != NOT_OFFERED for x in v), sum(x == HANDED_BACK for x in v)


# ---- case lists ------------------------------------------------------------------------------------------------------------
def _swap(gl, i, j):
    p = gl.split("^")
    p[i], p[j] = p[j], p[i]
    return "^".join(p)


def verdict_cases():
    """-> {class name: (GL, expected verdict)}: one line per class"""
    T = toy()
    S = T.subjects
    base = S["step0"]
    pos = base.split("^")
    out = {}
    for k in ("step0", "mid", "last", "planb", "cube_t", "cube_d", "cut_drop", "cut_keep", "hom_a", "hom_drb1", "hom_all",
              "name24_side0", "name24_side1", "prefix_12", "prefix_23", "prefix_13", "u_end_side0", "gl144",
              "wrap0", "wrap1", "wrap2", "chain0", "chain1", "chain2"):
        out[k] = (S[k], ACCEPTED)
    hb = {
        "g_suffix": base.replace("A*10:01", "A*10:01g", 1),
        "l_suffix": base.replace("C*10:02", "C*10:02L", 1),
        "uuuu_side0": base.replace("B*10:01", "B*UUUU", 1),
        "uuuu_side1": base.replace("B*10:02", "B*UUUU", 1),
        "u_end_side1": S["u_end_side1"],
        "unknown_allele": base.replace("A*10:01", "A*99:99", 1),
        "loci_out_of_order": _swap(base, 1, 3),
        "sides_sort_differently": "^".join([pos[0], "B*10:01+C*10:02", "C*10:01+B*10:02"] + pos[3:]),
        "locus_twice": "^".join([pos[0], pos[1], S["mid"].split("^")[1]] + pos[3:]),
        "four_positions": "^".join(pos[:4]),
        "six_positions": "^".join(pos + [S["mid"].split("^")[4]]),  # (on a five-locus graph: a locus twice as well)
        "caret_for_plus": base.replace("+", "^", 1),
        "empty_allele": base.replace("A*10:01+A*10:02", "+", 1),
        "name25": S["name25"],
        # (the same odd name on both sides: an entry that mixes two locus names is a line of the locus-twice kind)
        "no_star": base.replace("A*10:01+A*10:02", "A10:01+A10:01", 1),
        "locus_prefix_9": base.replace("A*10:01+A*10:02", "ABCDEFGHI*10:01+ABCDEFGHI*10:02", 1),
    }
    for k, gl in hb.items():
        out[k] = (gl, HANDED_BACK)
    out["slash_list"] = (base.replace("A*10:01", "A*10:01/A*11:01", 1), NOT_OFFERED)
    out["empty_gl"] = ("", NOT_OFFERED)
    out["gl145"] = (S["gl145"], NOT_OFFERED)
    return out


# classes whose lines name a locus twice: the product reports them (reason 8) and answers every other line
LOCUS_TWICE_CLASSES = ("locus_twice", "six_positions")


# ---- placement -------------------------------------------------------------------------------------------------------------
def make_line(sid, gl):
    return "%s,%s,%s,%s" % (sid, gl, POP, POP)


class Placer:
    """Builds the lines of a stream so that chosen GL fields start at chosen offsets modulo 16 of their chunk's text (the
    device tokenizer loads a 160-byte window from the 16-byte boundary before the field).  A chunk is `chunk_lines` lines;
    its text starts at its first line."""

    def __init__(self, chunk_lines, prefix="s"):
        self.chunk_lines = chunk_lines
        self.prefix = prefix
        self.lines = []
        self.off = 0  # bytes of the current chunk's text before the next line

    def add(self, gl, align=None, raw=None):
        """appends a line for `gl` (or the raw text `raw`, e.g. a blank line); -> its subject id"""
        if len(self.lines) % self.chunk_lines == 0:
            self.off = 0
        if raw is not None:
            self.lines.append(raw)
            self.off += len(raw) + 1
            return None
        sid = "%s%d" % (self.prefix, len(self.lines))
        if align is not None:
            sid += "x" * ((align - (self.off + len(sid) + 1)) % 16)
            assert (self.off + len(sid) + 1) % 16 == align
        line = make_line(sid, gl)
        self.lines.append(line)
        self.off += len(line) + 1
        return sid

    def add_all_alignments(self, gl):
        return [self.add(gl, align=a) for a in range(16)]

    def fill_to_last_of_chunk(self, filler_gl):
        """fillers until the NEXT line added is the last of its chunk"""
        while len(self.lines) % self.chunk_lines != self.chunk_lines - 1:
            self.add(filler_gl)

    def data(self, final_newline=True):
        return ("\n".join(self.lines) + ("\n" if final_newline else "")).encode()


# ---- wave neighbours -------------------------------------------------------------------------------------------------------
NEIGHBOUR_CLASSES = ["step0", "mid", "last", "planb", "handed_back", "slash_list", "blank"]
# with the device tokenizer off only lines the host classifies as small get record slots of the half-wave kernel
SMALL_CLASSES = ["step0", "mid", "last", "planb"]


def neighbour_gl(cls):
    T = toy()
    if cls == "handed_back":
        return verdict_cases()["g_suffix"][0]
    if cls == "slash_list":
        return verdict_cases()["slash_list"][0]
    if cls == "blank":
        return None
    return T.subjects[cls]


def neighbour_pairs(classes=None, chunk_lines=256, extra=()):
    """-> Placer holding, for every ordered pair (X, Y) of behaviour classes, the two lines next to each other, X at an even
    line index of its chunk: record slot k of the device tokenizer is line lo + k, the half-wave kernel gives wave w the slots
    2w and 2w + 1, so the two share a wave.  `extra`: further GLs treated as classes of their own."""
    classes = list(classes or NEIGHBOUR_CLASSES)
    gls = {c: neighbour_gl(c) for c in classes}
    for k, gl in enumerate(extra):
        gls["extra%d" % k] = gl
    P = Placer(chunk_lines, prefix="n")
    for x, y in itertools.product(list(gls), repeat=2):
        assert len(P.lines) % chunk_lines % 2 == 0
        for c in (x, y):
            if gls[c] is None:
                P.add(None, raw="")
            else:
                P.add(gls[c])
    return P


# ---- the ladder rule, restated (impute.py:1665-1687 with one population: every prior is the same number w) -------------------
def ladder_of(epsilon):
    out = []
    eps = epsilon
    while eps > 0:
        eps /= 10
        if eps < 1.0e-9:
            eps = 0.0
        out.append(eps)
    return out


def plan_a_by_rule(gl, freq, epsilon=1e-3, w=1.0):
    """A fully typed, unambiguous GL against the haplotype table `freq` (haplotype string in LOCI order -> frequency).
    -> (index of the first ladder step that accepts a pair or None, [(hap1, hap2, probability)] after the final cut,
    [(hap1, hap2, probability)] accepted at the deciding step)"""
    sides = [p.split("+") for p in gl.split("^")]
    cand, seen = [], set()
    for i in range(16):
        pick = [(i >> k) & 1 for k in range(5)]
        h1 = "~".join(sides[k][pick[k]] for k in range(5))
        h2 = "~".join(sides[k][1 - pick[k]] for k in range(5))
        if frozenset((h1, h2)) in seen:
            continue
        seen.add(frozenset((h1, h2)))
        if freq.get(h1, 0) > 0 and freq.get(h2, 0) > 0:
            cand.append((h1, h2, freq[h1], freq[h2]))

    def accepted(eps):
        out = []
        for h1, h2, p1, p2 in cand:
            x = eps / p1
            if not p2 >= x:
                continue
            if (h1 != h2 and w * p2 >= x) or (h1 == h2 and w * p2 >= x * 2):
                out.append((h1, h2, p1 * p2 * w * (2 if h1 != h2 else 1)))
        return out

    for idx, eps in enumerate(ladder_of(epsilon)):
        acc = accepted(eps)
        if acc:
            if eps > 0:
                return idx, accepted(max(p for _, _, p in acc) / 100000), acc
            return idx, acc, acc
    return None, [], []
