"""The sharded donor search with its DEFAULT compute (the HIP engine) under a real process group: two ranks, both on the one
GPU of the test box, donor chunks pulled from the job's store, rank 1's hit lists merged into rank 0's through the device's
merge door.  Against the single-process functions (grim.search.search_donors, search_file) in this process, byte for
byte."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import harness
from test_search_gpu import _imputation

pytestmark = pytest.mark.gpu

CHUNK = 50
TOP_N = 10
KEEP = ("A", "B", "DRB1")
PAIR_COUNTERS = ("donors_valid", "donors_private", "pairs", "row_pairs", "candidates", "host_pairs")
WORKER = r'''
import json, os, sys
import numpy as np
os.environ["GRIM_QUIET"] = "1"
os.environ["GRIM_ON_UNSUPPORTED"] = "skip"
os.chdir(WORK)
from grim import shard
from grim.imputation.networkx_graph import Graph
from grim.run_impute_def import load_config
rank = int(os.environ["RANK"])
cfg, _ = load_config(CONF)
g = Graph(cfg).build_graph(cfg["node_file"], cfg["top_links_file"], cfg["edges_file"])
ok, hits, n_hits, stats = shard.search_sharded(CONF, PATIENTS, KEEP, TOP_N, chunk_lines=CHUNK, graph=g, timeout_s=300)
np.save(OUT + ".hits%d.npy" % rank, np.frombuffer(hits.tobytes(), dtype=np.uint8))
file_stats = shard.search_file_sharded(CONF, PATIENTS, KEEP, OUT + ".csv", TOP_N, chunk_lines=CHUNK, graph=g, timeout_s=300)
assert os.path.exists(OUT + ".csv")  # every rank returns when rank 0 has written it
json.dump({"ok": ok.tolist(), "n_hits": n_hits.tolist(), "stats": stats, "file_stats": file_stats}, open(OUT + ".rank%d" % rank, "w"))
'''


def _own(monkeypatch):
    """an Imputation of this process on the scenario's graph that skips unsupported subjects, as the workers do"""
    from grim.imputation.impute import Imputation

    imp, lines, _, _ = _imputation("pop4_mixed")
    monkeypatch.setenv("GRIM_ON_UNSUPPORTED", "skip")
    monkeypatch.setenv("GRIM_QUIET", "1")
    monkeypatch.chdir(harness.ensure_graph(harness.golden("pop4_mixed")[0]))  # the configuration's paths are relative to it
    return Imputation(imp.netGraph, imp.config), lines


def test_two_ranks_equal_the_single_process(tmp_path, monkeypatch):
    from grim.search import search_donors, search_file

    mine, lines = _own(monkeypatch)
    gname, conf = harness.golden("pop4_mixed")[:2]
    work = harness.ensure_graph(gname)
    conf, cpath = harness._write_inputs(work, conf, lines, "srsg")
    usable = search_donors(mine, lines[:24], lines[:1], mine.config, KEEP, 1)[0]  # which of the first lines have genotype rows
    plines = [lines[i] for i in np.flatnonzero(usable)[:8]]
    assert len(plines) == 8
    ppath = str(tmp_path / "patients.csv")
    with open(ppath, "w") as fh:
        fh.write("\n".join(plines) + "\n")
    out = str(tmp_path / "out")
    script = tmp_path / "worker.py"
    script.write_text("WORK=%r\nCONF=%r\nPATIENTS=%r\nOUT=%r\nCHUNK=%d\nTOP_N=%d\nKEEP=%r\n" % (work, cpath, ppath, out, CHUNK, TOP_N, KEEP) + WORKER)
    env = dict(os.environ, PYTHONPATH=harness.PKG, MASTER_ADDR="127.0.0.1")
    # a parent and two children, once: a non-zero exit is the failure
    subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                           "--master-addr", "127.0.0.1", "--master-port", "29591", str(script)], env=env, timeout=600)
    ranks = [json.load(open(out + ".rank%d" % r)) for r in range(2)]
    got_hits = [np.load(out + ".hits%d.npy" % r).tobytes() for r in range(2)]
    assert len(lines) > 2 * CHUNK  # more chunks than ranks
    ok, hits, n_hits, stats = search_donors(mine, plines, lines, mine.config, KEEP, TOP_N)
    assert ok.all() and n_hits.all() and stats["candidates"] > 8 * TOP_N
    assert ranks[0] == ranks[1] and got_hits[0] == got_hits[1]
    got = ranks[0]
    assert got_hits[0] == hits.tobytes() and got["n_hits"] == n_hits.tolist() and got["ok"] == ok.tolist()
    for k in PAIR_COUNTERS + ("patients_valid", "patients_private"):
        assert got["stats"][k] == stats[k], k
    assert got["stats"]["chunks"] == -(-len(lines) // CHUNK) and 0 < got["stats"]["blocks"] <= got["stats"]["chunks"]
    assert got["stats"]["merge_ms"] > 0.0 and got["stats"]["kernel_ms"] > got["stats"]["select_ms"] > 0.0
    assert [tuple(u) for u in got["stats"]["unsupported"]] == sorted(tuple(u) for u in mine.unsupported)
    # the file
    want_csv = str(tmp_path / "single.csv")
    cwd = os.getcwd()
    os.chdir(work)
    try:
        file_stats = search_file(cpath, ppath, KEEP, want_csv, TOP_N, graph=mine.netGraph)
    finally:
        os.chdir(cwd)
    text = open(want_csv).read()
    assert open(out + ".csv").read() == text and text.count("\n") == 1 + int(n_hits.sum())
    for k in PAIR_COUNTERS:
        assert got["file_stats"][k] == file_stats[k], k
