"""The chunk fast path -- device tokenizer (csrc/grim_tokdev.h), half-wave kernel (csrc/grim_small.h), row compaction --
on the constructed cases of tools/fastpath_cases.py: a designed one-population graph whose subjects reach the limits and
branches that random subjects of the CAU graph do not (names of 24 bytes, a 144-byte GL field at every 16-byte alignment,
dictionary probes that chain and wrap, ladders longer than the eight steps kept in registers, wave neighbours that decide at
different steps, ties, truncation and the final cut).

Every comparison is of the six output texts, byte for byte, with the CPU oracle; the device tokenizer's verdicts are read
through grim_stream_devtok_lines and held against fastpath_cases.device_tokenizer_verdict, line by line.  Every run asserts
that no chunk ran twice and that nothing is reported unsupported, except lines that name a locus twice (reason 8)."""
import os

import pytest

import fastpath_cases as fc
import harness
import synth

pytestmark = pytest.mark.gpu

SWITCHES = ("GRIM_DEVICE_TOKENIZER", "GRIM_NO_SMALL", "GRIM_NO_MEDIUM", "GRIM_NO_MID", "GRIM_CHUNK_LINES")


@pytest.fixture(scope="module")
def toy_graph():
    return fc.ensure_toy_graph()


def _imp(gname, conf):
    from grim.imputation.impute import Imputation
    from grim.imputation.networkx_graph import Graph
    from grim.run_impute_def import load_config

    work = harness.ensure_graph(gname)
    _, cpath = harness._write_inputs(work, conf, [], "fp_cfg")
    cwd = os.getcwd()
    os.chdir(work)
    try:
        cfg, _ = load_config(cpath)
        g = harness._graph_cache.get(gname)
        if g is None:
            g = Graph(cfg).build_graph(cfg["node_file"], cfg["top_links_file"], cfg["edges_file"])
            harness._graph_cache[gname] = g
        imp = Imputation(g, cfg)
    finally:
        os.chdir(cwd)
    imp.quiet = True
    imp.on_unsupported = "skip"
    return imp, cfg


def _product(monkeypatch, gname, conf, data, **switches):
    """the six texts of the input bytes `data` through the product's stream, with the given switches and no others"""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in switches.items():
        assert k in SWITCHES
        monkeypatch.setenv(k, str(v))
    imp, cfg = _imp(gname, conf)
    texts = imp._stream_run(cfg, None, False, False, data=data)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return texts, imp


def _lines_of(data):
    lines = data.decode().split("\n")
    return lines[:-1] if lines[-1] == "" else lines


_oracle_cache = {}


def _oracle(gname, conf, lines):
    """computed once per (graph, configuration, input) and shared; never modified"""
    key = (gname, repr(sorted(conf.items(), key=lambda kv: kv[0])), tuple(lines))
    if key not in _oracle_cache:
        _oracle_cache[key] = harness.run_oracle(gname, conf, list(lines), tag="fp_orc")[0]
    return dict(_oracle_cache[key])


def _assert_equal_to(texts, exp, imp, what, twice=()):
    """`twice`: ids of lines that name a locus twice -- reported (reason 8) and left out of both sides; nothing else may be"""
    assert imp.last_stats["reruns"] == 0, what
    assert sorted((sid, r) for _, sid, r in imp.unsupported) == sorted((sid, 8) for sid in twice), what
    if twice:
        exp = harness.drop_subjects(exp, list(twice))
        texts = harness.drop_subjects(texts, list(twice))
    for k in exp:
        assert texts[k] == exp[k], "%s: %s differs" % (what, k)


# ---- verdict and answer, by class -------------------------------------------------------------------------------------------
_CASES = fc.verdict_cases()
_NAMES = list(_CASES)
_GROUPS = [_NAMES[i:i + 6] for i in range(0, len(_NAMES), 6)]


@pytest.mark.parametrize("group", _GROUPS, ids=["-".join(g) for g in _GROUPS])
def test_verdict_and_answer_by_class(group, toy_graph, monkeypatch):
    """each class line at all 16 alignments of its GL field, chunks of 32 lines: the device tokenizer's counts are the sums of
    the verdict function, the texts those of a host-tokenised run and of the oracle"""
    d = fc.toy().dictionary()
    conf = fc.toy_conf()
    P = fc.Placer(32)
    twice = []
    for name in group:
        ids = P.add_all_alignments(_CASES[name][0])
        if name in fc.LOCUS_TWICE_CLASSES:
            twice += ids
    data = P.data()
    lines = _lines_of(data)
    assert lines == P.lines and len(lines) == 16 * len(group)
    exp = _oracle(toy_graph, conf, lines)
    dev, imp = _product(monkeypatch, toy_graph, conf, data, GRIM_CHUNK_LINES=32)
    assert imp.last_stats["chunks"] == (len(lines) + 31) // 32
    want = fc.count_verdicts(lines, d)
    assert want[0] == 16 * sum(_CASES[n][1] != fc.NOT_OFFERED for n in group)
    assert want[1] == 16 * sum(_CASES[n][1] == fc.HANDED_BACK for n in group)
    assert imp.last_stats["devtok_lines"] == want, group
    _assert_equal_to(dev, exp, imp, "device tokenizer", twice)
    host, imp = _product(monkeypatch, toy_graph, conf, data, GRIM_CHUNK_LINES=32, GRIM_DEVICE_TOKENIZER=0)
    assert imp.last_stats["devtok_lines"] == (0, 0)
    _assert_equal_to(host, exp, imp, "host tokenizer", twice)
    for k in dev:
        assert dev[k] == host[k], k


@pytest.mark.parametrize("final_newline", [True, False])
def test_chunks_handed_back_whole_and_the_longest_line_last(final_newline, toy_graph, monkeypatch):
    """a chunk in which every line is handed back, a chunk in which exactly one is, and the 144-byte GL field at alignment 15
    as the last line of its chunk and of the input (its 160-byte window ends at the text's last byte), with and without a
    final newline"""
    T = fc.toy()
    d = T.dictionary()
    conf = fc.toy_conf()
    P = fc.Placer(16)
    P.add_all_alignments(_CASES["g_suffix"][0])            # chunk 0: all sixteen come back
    for k in range(16):                                    # chunk 1: one does
        P.add(_CASES["unknown_allele"][0] if k == 9 else T.subjects[("step0", "mid", "last", "cube_d")[k % 4]], align=(5 * k) % 16)
    for k in range(16):                                    # chunk 2: none
        P.add(T.subjects[("cube_t", "planb", "cut_keep", "hom_all")[k % 4]])
    P.fill_to_last_of_chunk(T.subjects["gl144"])           # chunk 3: the long lines
    P.add(T.subjects["gl144"], align=15)
    data = P.data(final_newline=final_newline)
    lines = _lines_of(data)
    assert len(lines) == 64 and data.endswith(b"\n") == final_newline
    assert fc.count_verdicts(lines[:16], d) == (16, 16) and fc.count_verdicts(lines[16:32], d) == (16, 1)
    exp = _oracle(toy_graph, conf, lines)
    dev, imp = _product(monkeypatch, toy_graph, conf, data, GRIM_CHUNK_LINES=16)
    assert imp.last_stats["chunks"] == 4
    assert imp.last_stats["devtok_lines"] == (64, 17)
    _assert_equal_to(dev, exp, imp, "device tokenizer")


# ---- grid tails ------------------------------------------------------------------------------------------------------------
_TAIL_CLASSES = ("step0", "mid", "cube_d", "last", "planb", "cut_keep", "cube_t", "hom_drb1", "name24_side1", "chain2", "wrap1")


@pytest.mark.parametrize("n", [1, 5, 6, 7, 23, 24, 25, 63, 64, 65, 129])
def test_grid_tails(n, toy_graph, monkeypatch):
    """n accepted lines in one chunk -- the tokenizer takes 6 lines per wave and 24 per workgroup, the half-wave kernel 2
    subjects per wave and 8 per workgroup, compaction 64 per wave -- and the same with every third line handed back"""
    T = fc.toy()
    d = T.dictionary()
    conf = fc.toy_conf()
    for third in (False, True):
        P = fc.Placer(4096, prefix="t")
        for k in range(n):
            P.add(_CASES["l_suffix"][0] if third and k % 3 == 2 else T.subjects[_TAIL_CLASSES[k % len(_TAIL_CLASSES)]])
        data = P.data()
        exp = _oracle(toy_graph, conf, P.lines)
        got, imp = _product(monkeypatch, toy_graph, conf, data)
        assert imp.last_stats["chunks"] == 1
        assert imp.last_stats["devtok_lines"] == (n, n // 3 if third else 0) == fc.count_verdicts(P.lines, d)
        _assert_equal_to(got, exp, imp, "n=%d third=%s" % (n, third))


# ---- wave neighbours ---------------------------------------------------------------------------------------------------------
def _neighbours(classes=None):
    T = fc.toy()
    return fc.neighbour_pairs(classes, chunk_lines=4096, extra=(T.subjects["cube_d"], T.subjects["cut_keep"], T.subjects["cube_t"]))


def test_wave_neighbours_device_tokenised(toy_graph, monkeypatch):
    """every ordered pair of behaviour classes as the two subjects of one wave of the half-wave kernel: against the oracle
    and against a run without the half-wave kernel"""
    conf = fc.toy_conf()
    P = _neighbours()
    exp = _oracle(toy_graph, conf, P.lines)
    got, imp = _product(monkeypatch, toy_graph, conf, P.data())
    assert imp.last_stats["chunks"] == 1
    assert imp.last_stats["devtok_lines"] == fc.count_verdicts(P.lines, fc.toy().dictionary())
    _assert_equal_to(got, exp, imp, "half-wave kernel")
    slow, imp = _product(monkeypatch, toy_graph, conf, P.data(), GRIM_NO_SMALL=1)
    _assert_equal_to(slow, exp, imp, "GRIM_NO_SMALL")
    for k in got:
        assert got[k] == slow[k], k


def test_wave_neighbours_host_tokenised(toy_graph, monkeypatch):
    """the same with the host's tokenizer: only lines it classifies as small get record slots, so the set is built from those"""
    conf = fc.toy_conf()
    P = _neighbours(fc.SMALL_CLASSES)
    d = fc.toy().dictionary()
    assert all(fc.line_verdict(l, d) == fc.ACCEPTED for l in P.lines)
    exp = _oracle(toy_graph, conf, P.lines)
    got, imp = _product(monkeypatch, toy_graph, conf, P.data(), GRIM_DEVICE_TOKENIZER=0)
    assert imp.last_stats["devtok_lines"] == (0, 0)
    _assert_equal_to(got, exp, imp, "half-wave kernel, host tokenizer")
    slow, imp = _product(monkeypatch, toy_graph, conf, P.data(), GRIM_NO_SMALL=1)
    _assert_equal_to(slow, exp, imp, "GRIM_NO_SMALL")


# ---- ladder length -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epsilon,steps", [(1e-3, 7), (1e-2, 8), (1e-1, 9), (1.0, 10), (1e31, 41)])
def test_ladder_length_on_the_half_wave_kernel(epsilon, steps, toy_graph, monkeypatch):
    """the kernel keeps eight steps in registers and reads the rest in a loop of its own: the wave-neighbour set and both
    cubes on ladders of 7, 8, 9, 10 and 41 steps.  Also without Plan B: a subject whose only accepting step is the last
    (epsilon 0) and is missed there gets the SAME answer from Plan B's first row (one block of all five loci), so only a run
    without Plan B shows a ladder that stops short on 9 or 10 steps"""
    for planb in (True, False):
        conf = fc.toy_conf(epsilon=epsilon, planb=planb)
        imp, cfg = _imp(toy_graph, conf)
        assert imp._params(cfg, cfg["planb"], False, False).n_ladder == steps == len(fc.ladder_of(epsilon))
        P = _neighbours()
        exp = _oracle(toy_graph, conf, P.lines)
        got, imp = _product(monkeypatch, toy_graph, conf, P.data())
        assert imp.last_stats["devtok_lines"] == fc.count_verdicts(P.lines, fc.toy().dictionary())
        _assert_equal_to(got, exp, imp, "epsilon %g planb %s" % (epsilon, planb))


# ---- ranking and truncation --------------------------------------------------------------------------------------------------
def _cube_lines():
    T = fc.toy()
    S = T.subjects
    P = fc.Placer(4096, prefix="c")
    for a, b in (("cube_t", "cube_d"), ("cube_d", "cube_t"), ("cube_t", "cube_t"), ("cube_d", "cube_d"), ("hom_a", "hom_drb1"),
                 ("cut_keep", "cut_drop"), ("hom_all", "cube_t"), ("cube_d", "last")):
        P.add(S[a])
        P.add(S[b])
    return P


@pytest.mark.parametrize("over", [{"number_of_results": 1}, {"number_of_results": 10}, {"number_of_results": 15},
                                  {"number_of_results": 16}, {"number_of_results": 1000}, {"output_MUUG": False},
                                  {"output_haplotypes": False}, {"number_of_pop_results": 0}, {"number_of_pop_results": 1}],
                         ids=lambda o: "-".join("%s=%s" % kv for kv in o.items()))
def test_ranking_and_truncation(over, toy_graph, monkeypatch):
    """cube T (16 tied phases: the order is 'earlier phase first') and cube D (distinct probabilities, one under the final
    cut) at result counts below, at and above the number of accepted phases, and with each output switched off"""
    conf = fc.toy_conf(**over)
    P = _cube_lines()
    exp = _oracle(toy_graph, conf, P.lines)
    if conf["output_haplotypes"] and conf["number_of_results"] >= 16:
        sid = P.lines[0].split(",")[0]
        probs = [l.split(",")[-2] for l in exp["pmug"].splitlines() if l.split(",")[0] == sid]
        assert len(probs) == 16 and len(set(probs)) == 1  # cube T: all tied
    got, imp = _product(monkeypatch, toy_graph, conf, P.data())
    assert imp.last_stats["devtok_lines"] == (len(P.lines), 0)
    _assert_equal_to(got, exp, imp, str(over))


# ---- long ladders in the other kernels -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname", ["cau", "pop4"])
@pytest.mark.parametrize("epsilon,steps", [(0.5, 9), (1e31, 41)])
def test_long_ladders_in_the_other_kernels(gname, epsilon, steps, monkeypatch):
    """mixed subjects (ambiguity, missing loci, recombinants) on ladders of more than eight steps: the default kernels, and
    the general kernel alone (no half-wave, one-wave or mid-size kernel), against the oracle"""
    pops = harness.POPS[gname]
    rows = synth.read_freqs(synth.CAU_FREQS)
    lines = synth.SubjectGen(rows, 97, pops=pops).mixed(200)
    conf = harness.base_conf(pops)
    conf["epsilon"] = epsilon
    if len(pops) > 1:
        conf["UNK_priors"] = "MR"
    imp, cfg = _imp(gname, conf)
    assert imp._params(cfg, cfg["planb"], False, False).n_ladder == steps
    data = ("\n".join(lines) + "\n").encode()
    exp = _oracle(gname, conf, lines)
    got, imp = _product(monkeypatch, gname, conf, data)
    _assert_equal_to(got, exp, imp, "default kernels")
    got, imp = _product(monkeypatch, gname, conf, data, GRIM_NO_SMALL=1, GRIM_NO_MEDIUM=1, GRIM_NO_MID=1)
    _assert_equal_to(got, exp, imp, "general kernel")
