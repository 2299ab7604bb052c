"""The sharded donor search's driver (grim/shard.py search_sharded) on CPU: gloo jobs of two and three ranks and the lone
process, donor chunks pulled from the job's store, every rank's hit lists published on the store and merged by rank 0.  The
per-chunk compute is injected -- deterministic records derived from the donor lines' text, with ties in mm[0] and mm[1] --
so what is under test is the driver: the answer is the same bytes on every rank, in every world and at every chunk size, and
equal to grim.search.merge_hit_lists over all lines.  The default (HIP) compute under a process group is
tests/test_search_sharded_gpu.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import harness

COMPUTE = r'''
import numpy as np
def chunk_hits(patient_lines, lines, first, top_n):
    """(hits, n_hits, stats) of a chunk of donor lines against the patients, made at a threshold of 0.0: a donor's id is its
    line number, read from its text; a record's values follow from the two line numbers"""
    from grim import _native as nat
    gid = np.array([int(line.split(",")[0][1:]) for line in lines], dtype=np.int64)
    assert gid.tolist() == list(range(first, first + len(lines))), "the chunk does not begin at its first line"
    P = len(patient_lines)
    hits = np.zeros((P, top_n), dtype=nat.SEARCH_DT)
    hits["donor"] = nat.SEARCH_NO_DONOR
    n_hits = np.zeros(P, dtype=np.uint32)
    for p in range(P):
        mm0 = ((gid * 7 + p * 3) % 11) / 16.0
        mm1 = ((gid * 5 + p) % 4) / 8.0
        order = np.lexsort((gid, -mm1, -mm0))[:top_n]
        n = len(order)
        n_hits[p] = n
        hits["donor"][p, :n] = gid[order]
        hits["rec"]["mm"][p, :n, 0] = mm0[order]
        hits["rec"]["mm"][p, :n, 1] = mm1[order]
        hits["rec"]["mm"][p, :n, 2] = 1.0 / (1 + gid[order] + p)
        hits["rec"]["locus"][p, :n, :] = (gid[order] * 1000 + p)[:, None] + np.arange(hits["rec"]["locus"].shape[2]) / 8.0
    stats = {"donors_valid": len(lines), "donors_private": first % 2, "pairs": P * len(lines), "row_pairs": 3 * P * len(lines),
             "candidates": P * len(lines), "host_pairs": len(lines) % 3, "kernel_ms": 0.5, "select_ms": 0.25, "blocks": 1,
             "download_bytes": 0}
    return hits, n_hits, stats
'''
exec(COMPUTE)  # chunk_hits: the test's own copy of what the workers compute

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
def compute(cfg, plines, lines, first):
    if FAIL_LINE >= 0 and first <= FAIL_LINE < first + len(lines):
        raise ValueError("boom in the chunk of line %d" % FAIL_LINE)
    return chunk_hits(plines, lines, first, TOP_N)
for chunk in CHUNKS:
    t0 = time.monotonic()
    try:
        ok, hits, n_hits, stats = shard.search_sharded(CONF, PATIENTS, ("A", "B"), TOP_N, min_p0=MIN_P0, chunk_lines=chunk, compute=compute,
                                                       timeout_s=TIMEOUT)
        np.save(OUT + ".hits%d.rank%d.npy" % (chunk, dist.get_rank()), np.frombuffer(hits.tobytes(), dtype=np.uint8))
        json.dump({"ok": ok.tolist(), "n_hits": n_hits.tolist(), "stats": stats}, open(OUT + ".c%d.rank%d" % (chunk, dist.get_rank()), "w"))
    except Exception as e:
        open(OUT + ".err%d" % dist.get_rank(), "w").write("%.1f %s: %s" % (time.monotonic() - t0, type(e).__name__, e))
dist.barrier()
store = dist.distributed_c10d._get_default_store()
json.dump({"published": published, "left": [k for k in published if store.check([k])]}, open(OUT + ".keys%d" % dist.get_rank(), "w"))
dist.barrier(); dist.destroy_process_group()
'''

N_LINES = 95


def _inputs(tag, n_patients):
    work = harness.ensure_graph("cau")
    lines = ["D%d,A*01:01+A*02:01^B*07:02+B*08:01" % i for i in range(N_LINES)]
    conf, cpath = harness._write_inputs(work, harness.base_conf(["CAU"]), lines, tag)
    ppath = os.path.join(work, "patients_%s.csv" % tag)
    with open(ppath, "w") as fh:
        fh.write("".join("P%d,A*01:01+A*02:01^B*07:02+B*08:01\n" % i for i in range(n_patients)))
    return work, lines, cpath, ppath


def _launch(tmp_path, world, chunks, port, tag, n_patients=5, top_n=20, min_p0=0.0, fail_line=-1, timeout_s=120):
    work, lines, cpath, ppath = _inputs(tag, n_patients)
    out = str(tmp_path / "out")
    script = tmp_path / "worker.py"
    script.write_text("WORK=%r\nCONF=%r\nPATIENTS=%r\nOUT=%r\nCHUNKS=%r\nTOP_N=%d\nMIN_P0=%r\nFAIL_LINE=%d\nTIMEOUT=%d\n" % (
        work, cpath, ppath, out, list(chunks), top_n, min_p0, fail_line, timeout_s) + COMPUTE + WORKER)
    env = dict(os.environ, PYTHONPATH=harness.PKG, MASTER_ADDR="127.0.0.1")
    subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
                           "--master-addr", "127.0.0.1", "--master-port", str(port), str(script)], env=env, timeout=300)
    return lines, out


def _store_keys(out, rank):
    """{"published": the store keys the rank's jobs set through their publish routine, "left": those of them still on the
    store after the jobs and a barrier}"""
    return json.load(open(out + ".keys%d" % rank))


def _want(lines, chunk, n_patients, top_n, min_p0):
    """the contract on the test's side: the twin over all lines at once, and the chunks' statistics summed"""
    from grim.search import merge_hit_lists

    plines = ["P%d" % i for i in range(n_patients)]
    whole = chunk_hits(plines, lines, 0, top_n)
    hits, n_hits = merge_hit_lists([whole[:2]], top_n, min_p0)
    parts = [chunk_hits(plines, lines[lo:lo + chunk], lo, top_n)[2] for lo in range(0, len(lines), chunk)]
    return hits, n_hits, {k: sum(p[k] for p in parts) for k in parts[0]}, len(parts)


def _check(hits_bytes, rest, want, n_patients):
    hits, n_hits, stats, n_chunks = want
    assert rest["n_hits"] == n_hits.tolist() and rest["ok"] == [True] * n_patients
    assert hits_bytes == hits.tobytes()
    for k, v in stats.items():
        assert rest["stats"][k] == v, k
    assert rest["stats"]["chunks"] == n_chunks and rest["stats"]["merge_ms"] == 0.0
    assert list(rest["stats"]["unsupported"]) == [] and list(rest["stats"]["patients_unsupported"]) == []


MIN_P0 = 9 / 16.0  # 8 or 9 donors hold each mm0 value k / 16, k < 11: the first 20 reach down to 8 / 16, the threshold cuts them


def test_alone_equals_the_twin_over_all_lines():
    from grim import shard

    work, lines, cpath, ppath = _inputs("srs1", 5)
    cwd, env_world = os.getcwd(), os.environ.pop("WORLD_SIZE", None)
    os.chdir(work)
    try:
        answers = set()
        for chunk in (13, 1000):
            for min_p0 in (0.0, MIN_P0):
                ok, hits, n_hits, stats = shard.search_sharded(cpath, ppath, ("A", "B"), 20, min_p0=min_p0, chunk_lines=chunk, timeout_s=60,
                                                               compute=lambda cfg, pl, ls, first: chunk_hits(pl, ls, first, 20))
                want = _want(lines, chunk, 5, 20, min_p0)
                _check(hits.tobytes(), {"ok": ok.tolist(), "n_hits": n_hits.tolist(), "stats": stats}, want, 5)
                assert hits.shape == (5, 20) and n_hits.all()
                answers.add(hits.tobytes())
        assert len(answers) == 2  # the threshold shows, the chunk size does not
    finally:
        os.chdir(cwd)
        if env_world is not None:
            os.environ["WORLD_SIZE"] = env_world


@pytest.mark.parametrize("world,port", [(2, 29571), (3, 29573)], ids=["world2", "world3"])
def test_every_rank_of_every_world_gives_the_same_bytes(tmp_path, world, port):
    """chunks of 13 lines (eight chunks) and of 50 (two: with three ranks one gets no chunk at all): every rank returns the
    same bytes, those of the twin over all lines, which test_alone_equals_the_twin_over_all_lines finds in the lone process"""
    chunks = (13, 50)
    lines, out = _launch(tmp_path, world, chunks, port, "srs%d" % world, min_p0=MIN_P0)
    assert not [f for f in os.listdir(tmp_path) if ".err" in f]
    for chunk in chunks:
        want = _want(lines, chunk, 5, 20, MIN_P0)
        hits = [np.load(out + ".hits%d.rank%d.npy" % (chunk, r)).tobytes() for r in range(world)]
        rest = [open(out + ".c%d.rank%d" % (chunk, r)).read() for r in range(world)]
        assert all(h == hits[0] for h in hits) and all(r == rest[0] for r in rest)
        _check(hits[0], json.loads(rest[0]), want, 5)
    assert want[3] == 2 and 0 < int(want[1].sum()) < 5 * 20


def test_a_failing_chunk_ends_every_rank_well_inside_the_timeout(tmp_path):
    """the compute of one chunk raises on whichever rank pulled it: that rank leaves with its own exception, the others with the
    report of it, none of them by running into timeout_s"""
    lines, out = _launch(tmp_path, 3, (5,), 29575, "srsf", fail_line=42, timeout_s=120)
    errs = [open(out + ".err%d" % r).read().split(" ", 1) for r in range(3)]
    assert not [f for f in os.listdir(tmp_path) if ".rank" in f]
    assert sum(e.startswith("ValueError: boom in the chunk of line 42") for _, e in errs) == 1
    assert all(e.startswith("ValueError: boom") or "failed" in e for _, e in errs)
    assert all(float(t) < 60.0 for t, _ in errs)
    # a surviving rank other than 0 has published its lists, and nobody collects them: none outlives the job all the same
    keys = [_store_keys(out, r) for r in range(3)]
    assert sum(len(k["published"]) for k in keys) > 0
    assert [k["left"] for k in keys] == [[], [], []]


def test_hit_lists_above_the_piece_size_survive_the_trip(tmp_path):
    from grim import shard

    n_patients, top_n = 130, 256
    assert 136 * n_patients * top_n > shard.PIECE_BYTES  # a rank's lists, and the final ones, travel as more than one piece
    lines, out = _launch(tmp_path, 2, (48,), 29577, "srsb", n_patients=n_patients, top_n=top_n)
    want = _want(lines, 48, n_patients, top_n, 0.0)
    hits = [np.load(out + ".hits48.rank%d.npy" % r).tobytes() for r in range(2)]
    rest = [json.load(open(out + ".c48.rank%d" % r)) for r in range(2)]
    assert hits[0] == hits[1] and rest[0] == rest[1]
    _check(hits[0], rest[0], want, n_patients)
    assert want[3] == 2 and want[1].tolist() == [N_LINES] * n_patients
    keys = [_store_keys(out, r) for r in range(2)]
    assert all(len(k["published"]) > 2 for k in keys)  # rank 1's lists and rank 0's final ones: pieces and a head key each
    assert [k["left"] for k in keys] == [[], []]  # no blob outlives its job
