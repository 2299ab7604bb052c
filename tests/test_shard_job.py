"""What the sharded drivers of grim/shard.py share, on CPU: the blob frame (`_pack` / `_unpack` and its two callers, in this
process) and `_Job.agree` (two ranks, gloo).  The job protocol's failure path is driven through the drivers:
tests/test_multi_rank.py, tests/test_em_sharded.py, tests/test_search_sharded.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import harness


def _table(n):
    keys = np.arange(1, n + 1, dtype=np.uint64) << np.uint64(12) | np.uint64(1)
    return keys, np.arange(n, dtype=np.uint32) % 3, (np.arange(n, dtype=np.float64) + 1.0) / 7.0


@pytest.mark.parametrize("n", [0, 1])
def test_a_table_comes_back_bit_for_bit(n):
    from grim import shard

    keys, pops, counts = _table(n)
    x = 0.1 + 0.2  # no finite decimal writes this double exactly: it travels as hex
    spilled = {(1, "A*01:01~B*07:02"): x, (0, "PRIV*1"): 1.0 / 3.0}
    stats = {"subjects_used": n, "kernel_ms": 0.25}
    blob = shard._pack_table(keys, pops, counts, spilled, stats, [(3, "D3", "why")])
    k, p, c, sp, st, bad = shard._unpack_table(blob)
    assert (k.dtype, p.dtype, c.dtype) == (np.dtype("<u8"), np.dtype("<u4"), np.dtype("<f8"))
    assert k.tobytes() == keys.tobytes() and p.tobytes() == pops.tobytes() and c.tobytes() == counts.tobytes()
    assert list(sp) == list(spilled) and [v.hex() for v in sp.values()] == [v.hex() for v in spilled.values()]
    assert st == stats and bad == [(3, "D3", "why")]
    assert all(a.flags.owndata and a.flags.writeable for a in (k, p, c))  # copies, not views of the blob


@pytest.mark.parametrize("shape", [(0, 4), (3, 1)])
def test_hit_lists_come_back_bit_for_bit(shape):
    from grim import _native as nat
    from grim import shard
    from grim.search import _empty_hits

    hits = _empty_hits(*shape)
    hits["donor"][:, :1] = np.arange(shape[0], dtype=hits["donor"].dtype)[:, None]
    hits["rec"]["mm"][:, :, 0] = 1.0 / 3.0
    n_hits = np.ones(shape[0], dtype=np.uint32)
    ok = np.array([True, False, True][:shape[0]], dtype=bool)
    stats = {"pairs": 12, "kernel_ms": 0.1 + 0.2}
    got_ok, got_hits, got_n, got_stats, bad = shard._unpack_hits(shard._pack_hits(ok, hits, n_hits, stats, [(7, "D7", "why")]))
    assert got_hits.shape == shape and got_hits.dtype == nat.SEARCH_DT and got_hits.tobytes() == hits.tobytes()
    assert got_n.dtype == np.dtype("<u4") and got_n.tobytes() == n_hits.tobytes()
    assert got_ok.dtype == bool and got_ok.tolist() == ok.tolist()
    assert got_stats["kernel_ms"].hex() == stats["kernel_ms"].hex() and got_stats == stats and bad == [(7, "D7", "why")]
    assert got_hits.flags.writeable and got_n.flags.owndata


@pytest.mark.parametrize("n", [0, 1, 5])
def test_a_blob_of_the_wrong_size_is_refused(n):
    from grim import shard

    specs = [("<u8", lambda h: h["n"]), ("<f8", lambda h: h["n"])]
    arrays = [np.arange(n, dtype="<u8"), np.arange(n, dtype="<f8")]
    blob = shard._pack({"n": n, "note": "x"}, arrays)
    head, (a, b) = shard._unpack(blob, specs, "the_caller")
    assert head == {"n": n, "note": "x"} and a.tobytes() == arrays[0].tobytes() and b.tobytes() == arrays[1].tobytes()
    for bad in (blob[:-1], blob + b"\0"):
        with pytest.raises(RuntimeError, match="the_caller"):
            shard._unpack(bad, specs, "the_caller")


WORKER = r'''
import json, os
import torch.distributed as dist
from grim import shard
dist.init_process_group(backend="gloo")
store = dist.distributed_c10d._get_default_store()
shared = []  # the keys rank 0's values travel under
def share(ctl, key, make, _share=shard._Control.share):
    shared.append(key)
    return _share(ctl, key, make)
shard._Control.share = share
rank = dist.get_rank()
job = shard._Job("test_agree", 60)
del shared[:]  # (the job's tag travelled the same way)
got = [job.agree(lambda: "first from rank %d" % rank)]
dist.barrier()  # (rank 0 removes the key once it is past agree's own barrier)
left =[store.check([k]) for k in shared]
got.append(job.agree(lambda: "second from rank %d" % rank))
other = shard._Job("test_agree", 60)
got.append(other.agree(lambda: "another job's from rank %d" % rank))
dist.barrier()
json.dump({"got": got, "keys": shared, "left_after_first": left, "left": [k for k in shared if store.check([k])]},
          open(OUT + ".rank%d" % rank, "w"))
dist.barrier(); dist.destroy_process_group()
'''


def test_agree_is_rank_0s_text_on_every_rank_and_leaves_no_key(tmp_path):
    out = str(tmp_path / "out")
    script = tmp_path / "worker.py"
    script.write_text("OUT=%r\n" % out + WORKER)
    env = dict(os.environ, PYTHONPATH=harness.PKG, MASTER_ADDR="127.0.0.1")
    subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                           "--master-addr", "127.0.0.1", "--master-port", "29581", str(script)], env=env, timeout=120)
    ranks = [json.load(open(out + ".rank%d" % r)) for r in range(2)]
    for r in ranks:
        assert r["got"] == ["first from rank 0", "second from rank 0", "another job's from rank 0"]
        # one key per decision (and one for the second job's tag), none of them the first one's again
        assert len(set(r["keys"])) == len(r["keys"]) == 4
        assert r["left_after_first"] == [False]
        assert [k for k in r["left"] if "grim_job_" not in k] == []
    assert ranks[0]["keys"] == ranks[1]["keys"]
