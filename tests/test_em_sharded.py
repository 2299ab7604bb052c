"""The sharded M-step's driver (grim/shard.py m_step_sharded) on CPU: gloo jobs of two and three ranks and the lone process,
chunks pulled from the job's store, every chunk's table published on the store and folded by rank 0 in chunk order.  The
per-chunk compute is injected -- a deterministic table derived from the chunk's line ids, keys overlapping across chunks --
so what is under test is the driver: the answer is the same bytes on every rank and in every world, and equal to
grim.em.fold_chunk_tables.  The default (HIP) compute under a process group is tests/test_em_sharded_gpu.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import harness

COMPUTE = r'''
import numpy as np
def chunk_result(lines, offset, big=0):
    """(keys, pops, counts, spilled, stats) of a chunk from its line ids: keys recur across chunks, every sum left to right"""
    table, spilled = {}, {}
    for j, line in enumerate(lines):
        gid = int(line.split(",")[0][1:])
        assert gid == offset + j, "the chunk does not begin at its line offset"
        x = [0.1, 0.2, 0.3][gid % 3] * 10.0 ** -(gid % 6)
        at = ((1 + gid % 37) | (1 + gid % 5) << 12 | 1 << 24 | 1 << 36 | 1 << 48, gid % 3)
        table[at] = table[at] + x if at in table else x
        if gid % 4 == 0:
            sp = (gid % 2, "PRIV*%d" % (gid % 3))
            spilled[sp] = spilled[sp] + x if sp in spilled else x
    order = sorted(table)
    keys = np.array([k for k, _ in order], dtype=np.uint64)
    pops = np.array([p for _, p in order], dtype=np.uint32)
    counts = np.array([table[at] for at in order], dtype=np.float64)
    if big:  # entries below every key of the small table (no field in slots 3, 4), ascending; counts that differ by chunk
        more = np.arange(big, dtype=np.uint64)
        f0, f1 = more % np.uint64(4000) + np.uint64(1), more // np.uint64(4000) + np.uint64(1)
        keys = np.concatenate([f0 | f1 << np.uint64(12) | np.uint64(7 << 24), keys])
        pops = np.concatenate([np.full(big, 2, dtype=np.uint32), pops])
        counts = np.concatenate([(more % np.uint64(1000) + np.uint64(1)).astype(np.float64) / 7.0 * (1 + offset), counts])
    stats = {"subjects_used": len(lines), "skipped_plan_c": offset % 2, "contributions": 2 * len(lines), "rehashes": 0,
             "spill": len(spilled), "blocks": 1, "kernel_ms": 0.0}
    return keys, pops, counts, spilled, stats
'''
exec(COMPUTE)  # chunk_result: the test's own copy of what the workers compute

WORKER = r'''
import json, os, sys, time
import torch.distributed as dist
from grim import shard
dist.init_process_group(backend="gloo")
os.chdir(WORK)
published = []  # every store key this rank's jobs set through the one publish routine: pieces and head keys
def publish(job, name, blob, _publish=shard._Job.publish):
    keys = _publish(job, name, blob)
    published.extend(keys)
    return keys
shard._Job.publish = publish
def compute(cfg, lines, offset):
    if FAIL_LINE >= 0 and offset <= FAIL_LINE < offset + len(lines):
        raise ValueError("boom in the chunk of line %d" % FAIL_LINE)
    return chunk_result(lines, offset, BIG)
t0 = time.monotonic()
try:
    counts, stats, (keys, pops, vals) = shard.m_step_sharded(CONF, chunk_lines=CHUNK, compute=compute, timeout_s=TIMEOUT)
    json.dump({"keys": keys.tolist(), "pops": pops.tolist(), "vals": [float(v).hex() for v in vals.tolist()], "stats": stats,
               "counts": {p: {h: float(v).hex() for h, v in d.items()} for p, d in counts.items()}},
              open(OUT + ".rank%d" % dist.get_rank(), "w"))
except Exception as e:
    open(OUT + ".err%d" % dist.get_rank(), "w").write("%.1f %s: %s" % (time.monotonic() - t0, type(e).__name__, e))
dist.barrier()
store = dist.distributed_c10d._get_default_store()
json.dump({"published": published, "left": [k for k in published if store.check([k])]}, open(OUT + ".keys%d" % dist.get_rank(), "w"))
dist.barrier(); dist.destroy_process_group()
'''

N_LINES = 95


def _inputs(tag):
    work = harness.ensure_graph("cau")
    lines = ["D%d,A*01:01+A*02:01^B*07:02+B*08:01" % i for i in range(N_LINES)]
    conf, cpath = harness._write_inputs(work, harness.base_conf(["CAU"]), lines, tag)
    return work, lines, cpath


def _launch(tmp_path, world, chunk, port, tag, fail_line=-1, big=0, timeout_s=120):
    work, lines, cpath = _inputs(tag)
    out = str(tmp_path / "out")
    script = tmp_path / "worker.py"
    script.write_text("WORK=%r\nCONF=%r\nOUT=%r\nCHUNK=%d\nFAIL_LINE=%d\nBIG=%d\nTIMEOUT=%d\n" % (
        work, cpath, out, chunk, fail_line, big, timeout_s) + COMPUTE + WORKER)
    env = dict(os.environ, PYTHONPATH=harness.PKG, MASTER_ADDR="127.0.0.1")
    subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
                           "--master-addr", "127.0.0.1", "--master-port", str(port), str(script)], env=env, timeout=300)
    return lines, out


def _store_keys(out, rank):
    """{"published": the store keys the rank's job set through its publish routine, "left": those of them still on the store
    after the job and a barrier}"""
    return json.load(open(out + ".keys%d" % rank))


def _want(lines, chunk, big=0):
    """the contract on the test's side: the chunks' tables folded in chunk order, the spilled counts the same way, the
    statistics summed"""
    from grim.em import fold_chunk_tables

    parts = [chunk_result(lines[lo:lo + chunk], lo, big) for lo in range(0, len(lines), chunk)]
    keys, pops, vals = fold_chunk_tables([p[:3] for p in parts])
    spilled = {}
    for p in parts:
        for at, v in p[3].items():
            spilled[at] = spilled[at] + v if at in spilled else v
    stats = {k: sum(p[4][k] for p in parts) for k in parts[0][4]}
    return keys, pops, vals, spilled, stats, len(parts)


def _check(got, want):
    keys, pops, vals, spilled, stats, n_chunks = want
    assert got["keys"] == keys.tolist() and got["pops"] == pops.tolist()
    assert got["vals"] == [float(v).hex() for v in vals.tolist()]
    for k, v in stats.items():
        assert got["stats"][k] == v, k
    assert got["stats"]["chunks"] == n_chunks and got["stats"]["entries"] == len(keys) and got["stats"]["unsupported"] == []
    named = {}
    for k, p, v in zip(keys.tolist(), pops.tolist(), vals.tolist()):
        named.setdefault("CAU" if p == 0 else str(p), {})[str(k)] = float(v).hex()
    for (p, name), v in spilled.items():
        named.setdefault("CAU" if p == 0 else str(p), {})[name] = float(v).hex()
    assert got["counts"] == named


def test_alone_equals_the_fold():
    from grim import shard

    work, lines, cpath = _inputs("ems1")
    cwd, env_world = os.getcwd(), os.environ.pop("WORLD_SIZE", None)
    os.chdir(work)
    try:
        for chunk in (13, 1000):
            counts, stats, (keys, pops, vals) = shard.m_step_sharded(cpath, chunk_lines=chunk, timeout_s=60,
                                                                     compute=lambda cfg, ls, off: chunk_result(ls, off))
            got = {"keys": keys.tolist(), "pops": pops.tolist(), "vals": [float(v).hex() for v in vals.tolist()], "stats": stats,
                   "counts": {p: {h: float(v).hex() for h, v in d.items()} for p, d in counts.items()}}
            _check(got, _want(lines, chunk))
    finally:
        os.chdir(cwd)
        if env_world is not None:
            os.environ["WORLD_SIZE"] = env_world


@pytest.mark.parametrize("world,chunk,port", [(2, 13, 29551), (3, 50, 29553)], ids=["world2", "world3_two_chunks"])
def test_every_rank_of_every_world_gives_the_same_bytes(tmp_path, world, chunk, port):
    """eight chunks for two ranks; two chunks for three (one rank gets no chunk at all): every rank returns the same bytes,
    those of the chunk-ordered fold -- which test_alone_equals_the_fold finds in the lone process too"""
    lines, out = _launch(tmp_path, world, chunk, port, "ems%d" % world)
    ranks = [open(out + ".rank%d" % r).read() for r in range(world)]
    assert all(r == ranks[0] for r in ranks)
    _check(json.loads(ranks[0]), _want(lines, chunk))


def test_a_failing_chunk_ends_every_rank_well_inside_the_timeout(tmp_path):
    """the compute of one chunk raises on whichever rank pulled it: that rank leaves with its own exception, the others with the
    report of it, none of them by running into timeout_s"""
    lines, out = _launch(tmp_path, 3, 5, 29555, "emsf", fail_line=42, timeout_s=120)
    errs = [open(out + ".err%d" % r).read().split(" ", 1) for r in range(3)]
    assert not [f for f in os.listdir(tmp_path) if ".rank" in f]
    assert sum(e.startswith("ValueError: boom in the chunk of line 42") for _, e in errs) == 1
    assert all(e.startswith("ValueError: boom") or "failed" in e for _, e in errs)
    assert all(float(t) < 60.0 for t, _ in errs)
    # the tables the surviving ranks published are collected by nobody: none of them outlives the job all the same
    assert [_store_keys(out, r)["left"] for r in range(3)] == [[], [], []]


def test_a_table_above_the_piece_size_survives_the_trip(tmp_path):
    from grim import shard

    big = 230000
    assert 20 * big > shard.PIECE_BYTES  # a chunk's table, and the final one, travel as more than one piece
    lines, out = _launch(tmp_path, 2, 48, 29557, "emsb", big=big)
    ranks = [json.load(open(out + ".rank%d" % r)) for r in range(2)]
    assert ranks[0] == ranks[1]
    keys, pops, vals, _, _, n_chunks = _want(lines, 48, big)
    assert n_chunks == 2 and len(keys) > big
    assert ranks[0]["keys"] == keys.tolist() and ranks[0]["pops"] == pops.tolist()
    assert ranks[0]["vals"] == [float(v).hex() for v in np.asarray(vals).tolist()]
    keys = [_store_keys(out, r) for r in range(2)]
    assert len(keys[0]["published"]) > 2  # rank 0: the final table's pieces and its head key
    assert [k["left"] for k in keys] == [[], []]  # no blob outlives its job
