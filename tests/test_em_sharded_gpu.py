"""The sharded M-step and the sharded fixed-support EM with their DEFAULT compute (the HIP engine) under a real process
group: two ranks, both on the one GPU of the test box, chunks pulled from the job's store, tables folded by rank 0 through
the records door.  Against the single-process definition (grim.em.m_step_chunked, then Graph.refresh through the records
door) in this process, bit for bit: floats are compared as hex, frequencies as bytes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import harness
import refresh_synth as rs

pytestmark = pytest.mark.gpu

CHUNK = 50
WORKER = r'''
import json, os, sys
import numpy as np
os.environ["GRIM_QUIET"] = "1"
os.environ["GRIM_ON_UNSUPPORTED"] = "skip"
os.chdir(WORK)
from grim import shard
rank = int(os.environ["RANK"])
counts, stats, (keys, pops, vals) = shard.m_step_sharded(CONF, chunk_lines=CHUNK, timeout_s=300)
from grim import _native as nat
from grim.imputation.networkx_graph import Graph
from grim.run_impute_def import load_config
cfg, _ = load_config(CONF)
g = Graph(cfg).build_graph(cfg["node_file"], cfg["top_links_file"], cfg["edges_file"])
its = shard.em_fixed_support_sharded(CONF, 2, chunk_lines=CHUNK, graph=g, timeout_s=300)
ctx = nat.default_context(int(os.environ["LOCAL_RANK"]) % max(1, nat.lib().grim_device_count()))
freq = g.device(ctx).freq()  # as they lie on this rank's device
assert freq.tobytes() == g.arrays["freq"].tobytes()
np.save(OUT + ".freq%d.npy" % rank, freq)
short = shard.em_fixed_support_sharded(CONF, 3, chunk_lines=CHUNK, tol=float("inf"), timeout_s=300)  # rank 0 says stop
json.dump({"keys": keys.tolist(), "pops": pops.tolist(), "vals": [float(v).hex() for v in vals.tolist()], "stats": stats,
           "counts": {p: {h: float(v).hex() for h, v in d.items()} for p, d in counts.items()}, "short": len(short),
           "its": [{k: ([float(x).hex() for x in v] if k == "total" else float(v).hex() if isinstance(v, float) else v)
                    for k, v in it.items()} for it in its]}, open(OUT + ".rank%d" % rank, "w"))
'''


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("em_sharded_gpu")
    gname, conf, lines, _, _, _ = harness.golden("pop4_mixed")
    work = harness.ensure_graph(gname)
    conf, cpath = harness._write_inputs(work, conf, lines, "emsg")
    out = str(tmp / "out")
    script = tmp / "worker.py"
    script.write_text("WORK=%r\nCONF=%r\nOUT=%r\nCHUNK=%d\n" % (work, cpath, out, CHUNK) + WORKER)
    env = dict(os.environ, PYTHONPATH=harness.PKG, MASTER_ADDR="127.0.0.1")
    subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                           "--master-addr", "127.0.0.1", "--master-port", "29561", str(script)], env=env, timeout=600)
    ranks = [json.load(open(out + ".rank%d" % r)) for r in range(2)]
    freqs = [np.load(out + ".freq%d.npy" % r) for r in range(2)]
    return conf, lines, ranks, freqs


def test_m_step_sharded_equals_m_step_chunked(job):
    from grim.em import m_step_chunked

    conf, lines, ranks, _ = job
    imp = rs.own_imputation("pop4", conf, tag="emsg_single")
    counts, stats, (keys, pops, vals) = m_step_chunked(imp, lines, imp.config, CHUNK)
    assert len(keys) > 200 and stats["chunks"] == 6
    for r, got in enumerate(ranks):
        assert got["keys"] == keys.tolist() and got["pops"] == pops.tolist(), "rank %d" % r
        assert got["vals"] == [float(v).hex() for v in vals.tolist()], "rank %d" % r
        assert got["counts"] == {p: {h: float(v).hex() for h, v in d.items()} for p, d in counts.items()}, "rank %d" % r
        for k in ("subjects_used", "skipped_plan_c", "contributions", "spill", "blocks", "chunks", "entries"):
            assert got["stats"][k] == stats[k], k
        assert [tuple(u) for u in got["stats"]["unsupported"]] == sorted(tuple(u) for u in imp.unsupported)
    assert ranks[0]["stats"] == ranks[1]["stats"]


def test_em_fixed_support_sharded_equals_the_single_process_composition(job):
    from grim import _native as nat
    from grim.em import m_step_chunked

    conf, lines, ranks, freqs = job
    assert freqs[0].tobytes() == freqs[1].tobytes()
    imp = rs.own_imputation("pop4", conf, tag="emsg_em")
    ctx = nat.default_context(imp.device)
    start = imp.netGraph.arrays["freq"].tobytes()
    want = []
    for _ in range(2):
        _, mstats, table = m_step_chunked(imp, lines, imp.config, CHUNK)
        rstats = imp.netGraph.refresh(ctx, table)
        want.append((mstats, rstats))
    final = imp.netGraph.device(ctx).freq()
    assert final.tobytes() != start
    assert freqs[0].tobytes() == final.tobytes()
    for got in ranks:
        assert len(got["its"]) == 2 and got["short"] == 1  # any delta is <= an infinite tol: one iteration, on every rank
        for it, (mstats, rstats) in zip(got["its"], want):
            for k in ("subjects_used", "skipped_plan_c", "contributions", "spill", "blocks", "chunks", "entries"):
                assert it[k] == mstats[k], k
            assert it["total"] == [float(x).hex() for x in rstats["total"]] and it["delta"] == float(rstats["delta"]).hex()
            for k in ("matched", "zero_full", "n_full"):
                assert it[k] == rstats[k], k
            assert it["outside"] == it["entries"] - rstats["matched"]
