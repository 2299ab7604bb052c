"""
Multi-GPU drivers: one process per GPU, the subject file cut into fixed-size chunks of lines that the ranks PULL from a
shared counter, graph replicated per GPU, NO collective on the data path.

This is the split the reference's scripts/runfile_mp.py:109-148 intends (`split -l` + one worker per chunk + `cat` of the
per-chunk outputs), with three differences: workers are GPU ranks; chunks are handed out dynamically (a subject's cost
varies by more than 1000x with its ambiguity, so equal line counts are not equal work -- SURVEY 8e); `.miss/.problem`
keep the GLOBAL line index (the reference's per-chunk runs restart at 0).

THE PROTOCOL (`_Job`, once for every driver).  The only communication is the control plane on the job's rendezvous
store, and every key of a job carries the job's tag, a fresh id that rank 0 publishes:
  - chunks: an atomic fetch-add on the store hands out the next chunk number (`_Job.chunks`); a chunk is a byte range of
    the input file (`chunk_offsets`), read by the rank that pulled it;
  - waits are POLLED and look at the other ranks' error slots (`_Control.wait_bytes`): a rank that waits for something
    of a rank that failed stops with `_PeerFailed` instead of waiting for ever, or for the job's `timeout_s`;
  - the body of the job runs guarded (`_Job.body`): whatever it raises is kept, the rank's own error is reported in its
    error slot, the caller's clean-up runs;
  - then every rank, failed or not, reaches the first barrier and reads the error slots (`_Job.closing`): it raises its
    own error, else "<fn>: rank(s) [...] failed:" with the first report, else the peer failure it met; only when nobody
    failed does rank 0's epilogue run;
  - a second barrier ends the job on every path -- nobody leaves while another rank still reads the store -- and after it
    every rank removes the blobs it published, collected or not;
  - data on the store (`publish` / `collect` / `from_rank0`): bytes in pieces of at most PIECE_BYTES a key, framed by
    `_pack` / `_unpack`; `from_rank0` is "rank 0 computes, every rank decodes the same bytes";
  - `agree`: a short decision of rank 0's for every rank, its key removed once all have read it.

WHAT EACH DRIVER ADDS
`impute_sharded`: ONE long-lived streaming pipeline per rank (grim_stream: tokenizer threads -> device -> formatter
threads) for the whole job.  A pulled chunk's raw bytes go to the stream as one input SEGMENT (grim_stream_segment carries
the chunk's global line index), so chunk k+1 is tokenised while chunk k is on the device -- no per-chunk stream, no Python
line splitting.  Outputs are written ONCE, straight into the six final files, by every rank (no part files, no `cat`): as
soon as a chunk is formatted its rank publishes the SIZES of its six pieces on the store; where chunk c's pieces begin is
the sum of the sizes of the chunks before it, so only sizes wait for sizes -- a rank's placer thread picks them up and the
stream's worker threads pwrite the formatted buffers at their final offsets (grim_stream_segment_wait / _place) while the
pipeline is already busy with later chunks.  Rank 0 makes the files first ("ok" / "failed" under the job's files key) and
its epilogue checks their sizes and gathers the ranks' unsupported subjects.  Its waits have no deadline.

`m_step_sharded`, `em_fixed_support_sharded`: each chunk's count table is built in a fresh accumulator on the
rank's GPU and published as bytes, rank 0 folds the tables in CHUNK order (EmAccumulator.merge_records) and every rank
decodes the one result; the EM refreshes every rank's graph from it and agrees on when to stop.

`search_sharded`, `search_file_sharded`: a rank's device accumulates hit lists across its chunks, ranks other
than 0 publish theirs, rank 0 merges them on the device and every rank decodes the one answer; the file variant agrees on
the outcome of rank 0's CSV.

Launch:  torchrun --nproc-per-node N --master-addr 127.0.0.1 your_script.py   ->  impute_sharded(conf)
(a driver joins the job itself -- gloo, control plane only -- when the caller has not initialised torch.distributed;
alone, without WORLD_SIZE > 1, it runs every chunk in this process and touches no store).
"""

import contextlib
import json
import os
import pathlib
import queue
import struct
import threading
import time
import traceback
import uuid

OUTPUT_KEYS = ("umug", "umug_pops", "pmug", "pmug_pops", "miss", "problem")
DEFAULT_CHUNK_LINES = 65536
PIECE_BYTES = 4 << 20  # the most one store key carries: the store's own value limit has not been measured


def shard_range(n, rank, world):
    """[begin, end) of rank's contiguous block of ceil(n/world) lines (the static split of runfile_mp.py:113-124)."""
    per = -(-n // world) if world > 0 else n
    return min(n, rank * per), min(n, (rank + 1) * per)


def chunk_offsets(path, chunk_lines):
    """byte offset of every chunk_lines-th line start of the file, plus the file size: chunk c = bytes [off[c], off[c+1]).
    Lines end the way Python's universal-newline open() -- and the library's grim_stream_write_text -- ends them: at "\\n",
    at "\\r\\n" (one end, after the "\\n") and at a lone "\\r".  A last line without its line end counts as a line.
    (The library scans the file: grim_chunk_offsets, csrc/grim_stream.cpp.)"""
    from . import _native as nat

    return nat.chunk_offsets(path, chunk_lines)


class _PeerFailed(RuntimeError):
    """another rank reported an error while this one was waiting for something of its: this rank stops, the failure is the
    other rank's"""


class _Control:
    """the job's control plane: chunk counter, shared values, error slots, final barrier"""

    def __init__(self, timeout_s=None):
        """timeout_s: every wait_key / wait_bytes / share of this control plane ends with a TimeoutError that many seconds
        from now (None: a wait ends when its key is set or a peer reports an error)"""
        self.rank, self.world, self.dist, self.store = 0, 1, None, None
        self.local = 0
        self.deadline = None if timeout_s is None else time.monotonic() + float(timeout_s)
        world_env = int(os.environ.get("WORLD_SIZE", "1"))
        try:
            import torch.distributed as dist
        except ImportError:
            dist = None
        if dist is not None and dist.is_available():
            if not dist.is_initialized() and world_env > 1:
                # the caller did not join the job: do it here (control plane only, so gloo; the GPU work needs no
                # process group at all)
                os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
                dist.init_process_group(backend="gloo")
            if dist.is_initialized():
                self.dist = dist
                self.rank, self.world = dist.get_rank(), dist.get_world_size()
                from torch.distributed import distributed_c10d as c10d

                self.store = c10d._get_default_store()
        if self.dist is None and world_env > 1:
            raise RuntimeError("WORLD_SIZE=%d but torch.distributed is not available: every rank would impute the whole "
                               "file and write the same output files" % world_env)
        self.local = int(os.environ.get("LOCAL_RANK", self.rank))
        self._next = 0

    def next_chunk(self, tag):
        if self.store is None:
            c = self._next
            self._next += 1
            return c
        return int(self.store.add("grim_chunk_" + tag, 1)) - 1

    def share(self, key, make):
        """rank 0's make() for every rank (the store's get() blocks until rank 0 has set the key)"""
        if self.store is None:
            return make()
        if self.rank == 0:
            v = make()
            self.store.set(key, v)
            return v
        if self.deadline is not None:
            return self.wait_key(key, None)
        return self.store.get(key).decode()

    def set(self, key, value):
        if self.store is not None:
            self.store.set(key, value)

    def wait_key(self, key, tag, poll=0.0005):
        """the value of a key some rank will set -- POLLED (a blocking get would hold the store client, and with it this
        rank's chunk counter, for as long as it waits); raises when a rank has reported an error meanwhile (`tag` None:
        the job has no id yet, so no error slot either), or when the control plane's deadline has passed"""
        return self.wait_bytes(key, tag, poll).decode()

    def wait_bytes(self, key, tag, poll=0.0005):
        """wait_key, the value as the bytes the store holds"""
        last_look = 0.0
        while True:
            if self._has(key):
                return self.store.get(key)
            now = time.monotonic()
            if now - last_look > 0.05:
                last_look = now
                for r in range(self.world):
                    if tag is not None and r != self.rank and self._has("grim_err_%s_%d" % (tag, r)):
                        raise _PeerFailed("rank %d failed while this rank was waiting for %s" % (r, key))
                if self.deadline is not None and now > self.deadline:
                    raise TimeoutError("no rank has set %s within the job's timeout" % key)
            time.sleep(poll)

    def delete(self, key):
        if self.store is not None:
            try:
                self.store.delete_key(key)
            except Exception:  # a store that cannot delete keeps the key: it carries the job's id and is never read again
                pass

    def report_error(self, tag, text):
        if self.store is not None:
            self.store.set("grim_err_%s_%d" % (tag, self.rank), text)

    def barrier_and_errors(self, tag):
        """-> list of (rank, text) of the ranks that failed (every rank gets the same list)"""
        if self.dist is None:
            return []
        self.store.set("grim_done_%s_%d" % (tag, self.rank), "1")
        self.barrier()
        out = []
        for r in range(self.world):
            key = "grim_err_%s_%d" % (tag, r)
            if self.store.num_keys() and self._has(key):
                out.append((r, self.store.get(key).decode()))
        return out

    def barrier(self):
        if self.dist is None:
            return
        if self.dist.get_backend() == "nccl":  # RCCL wants the rank's device selected before its first collective
            import torch

            n = torch.cuda.device_count()
            if n > 0:
                torch.cuda.set_device(self.local % n)
        self.dist.barrier()

    def _has(self, key):
        try:
            return bool(self.store.check([key]))
        except Exception:  # older stores: no check()
            return False


class _Job:
    """One sharded call, on every rank: the protocol of the module docstring.  A driver is

        job = _Job("<fn>", timeout_s, chunk_lines)
        with job.body():        # this rank's work; job.cleanup takes what has to be closed whatever happens
            for c, first_line, raw in job.chunks(in_path): ...
        with job.closing():     # first barrier, raise if any rank failed ... last barrier, blobs removed
            ...                 # what rank 0 does once every rank has done its work (job.close() when there is nothing)
    """

    def __init__(self, fn, timeout_s=None, chunk_lines=None):
        """fn: the driver's name, for error texts; timeout_s: as `_Control`'s (None: waits without a deadline)"""
        self.fn = fn
        self.ctl = _Control(timeout_s)
        self.rank, self.world = self.ctl.rank, self.ctl.world
        self.chunk_lines = int(chunk_lines or os.environ.get("GRIM_SHARD_LINES", DEFAULT_CHUNK_LINES))
        # the job's id: unique per call and per job, published by rank 0 (keys of an earlier job on the same store never match)
        self.tag = self.ctl.share("grim_job_%d" % _next_call(), lambda: uuid.uuid4().hex[:12])
        self.n_chunks = 0  # (known once `chunks` has begun)
        self.cleanup = contextlib.ExitStack()  # runs when the body ends, however it ends
        self.error = self.peer_failed = None
        self.published = []  # every store key of this rank's blobs
        self.agreed = 0

    # ---- the guarded stages ---------------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def body(self):
        """the rank's work: the other ranks must not wait for this one forever, so nothing it raises leaves here -- it is
        kept for `closing`, and the rank's own error goes into its error slot"""
        try:
            with self.cleanup:
                yield
        except BaseException as e:  # noqa: B902  (raised again by `closing`, behind the barrier)
            if isinstance(e, _PeerFailed):
                self.peer_failed = e  # not this rank's failure: the barrier's error list names the rank whose it is
            else:
                self.error = e
                self.ctl.report_error(self.tag, "%s: %s\n%s" % (type(e).__name__, e, traceback.format_exc()))

    @contextlib.contextmanager
    def closing(self):
        """the barrier every rank reaches, then: this rank's own error, else the report of the ranks that failed, else the
        peer failure it met, else the `with` block (the epilogue).  One more barrier on every path: nobody leaves while
        another rank still reads the store; after it the rank's blobs go"""
        try:
            failed = self.ctl.barrier_and_errors(self.tag)
            if self.error is not None:
                raise self.error
            if failed:
                raise RuntimeError("%s: rank(s) %s failed:\n%s" % (self.fn, [r for r, _ in failed], failed[0][1]))
            if self.peer_failed is not None:
                raise self.peer_failed
            yield
        finally:
            self.ctl.barrier()
            for key in self.published:  # (collected or not: after a failure nobody will ask for them)
                self.ctl.delete(key)

    def close(self):
        with self.closing():
            pass

    # ---- chunks and the rank's device ------------------------------------------------------------------------------------
    def chunks(self, in_path):
        """(c, first line, raw bytes) of every chunk of the file this rank pulls from the job's counter"""
        from .em import read_chunk

        offs = chunk_offsets(in_path, self.chunk_lines)
        self.n_chunks = len(offs) - 1
        with open(in_path, "rb") as fh:
            while True:
                c = self.ctl.next_chunk(self.tag)
                if c >= self.n_chunks:
                    return
                yield c, c * self.chunk_lines, read_chunk(fh, offs, c)

    def imputation(self, config, graph=None):
        """the rank's Imputation on device LOCAL_RANK % device count; the graph is built from the configuration's files
        when none is given"""
        from . import _native as nat
        from .imputation.impute import Imputation
        from .imputation.networkx_graph import Graph

        if graph is None:
            graph = Graph(config).build_graph(config["node_file"], config["top_links_file"], config["edges_file"])
        return Imputation(graph, config, device=self.ctl.local % max(1, nat.lib().grim_device_count()))

    # ---- data on the store ---------------------------------------------------------------------------------------------
    def publish(self, name, blob):
        """blob under `name`: pieces of at most PIECE_BYTES, then the head key that says how many (set last: who sees it
        finds every piece).  -> the store keys it set"""
        n = max(1, -(-len(blob) // PIECE_BYTES))
        keys = ["%s_%d" % (name, i) for i in range(n)] + [name]
        self.published += keys
        for i, key in enumerate(keys[:n]):
            self.ctl.set(key, blob[i * PIECE_BYTES:(i + 1) * PIECE_BYTES])
        self.ctl.set(name, str(n))
        return keys

    def collect(self, name, delete):
        """the blob some rank publishes under `name`; delete: nobody else will ask for it"""
        n = int(self.ctl.wait_key(name, self.tag))
        blob = b"".join(self.ctl.wait_bytes("%s_%d" % (name, i), self.tag) for i in range(n))
        if delete:
            for i in range(n):
                self.ctl.delete("%s_%d" % (name, i))
            self.ctl.delete(name)
        return blob

    def from_rank0(self, name, make_blob):
        """rank 0's make_blob() on every rank, so that all decode the same bytes (alone: no store traffic)"""
        if self.rank != 0:
            return self.collect(name, False)
        blob = make_blob()
        if self.world > 1:
            self.publish(name, blob)
        return blob

    def agree(self, make_text):
        """rank 0's make_text() on every rank: a short decision.  Its key is removed once every rank has read it"""
        self.agreed += 1
        key = "grim_agree_%s_%d" % (self.tag, self.agreed)
        text = self.ctl.share(key, make_text)
        self.ctl.barrier()  # every rank has read the key
        if self.rank == 0:
            self.ctl.delete(key)
        return text


# ---- the blob frame: a <Q head length, the JSON head, the arrays' bytes in order --------------------------------------------
def _pack(head, arrays):
    head = json.dumps(head).encode()
    return struct.pack("<Q", len(head)) + head + b"".join(a.tobytes() for a in arrays)


def _unpack(blob, specs, who):
    """-> (head, arrays as copies); specs: per array (dtype, its number of items as a function of the head); who: the
    driver named by the RuntimeError a blob of the wrong size ends in"""
    import numpy as np

    try:
        (n_head,) = struct.unpack_from("<Q", blob, 0)
        head = json.loads(blob[8:8 + n_head].decode())
        shapes = [(np.dtype(dtype), int(count(head))) for dtype, count in specs]
        size = 8 + n_head + sum(dtype.itemsize * n for dtype, n in shapes)
    except (struct.error, ValueError, LookupError, TypeError):  # (cut inside the head, or not a head of this kind)
        size = None
    if size != len(blob):
        raise RuntimeError("%s: a blob of %d bytes whose head asks for %s" % (who, len(blob), size))
    arrays, at = [], 8 + n_head
    for dtype, n in shapes:
        arrays.append(np.frombuffer(blob, dtype=dtype, count=n, offset=at).copy())
        at += dtype.itemsize * n
    return head, arrays


def _pack_table(keys, pops, counts, spilled, stats, unsupported):
    """a chunk's (or the job's) count table as bytes; floats of the head as hex: every bit travels"""
    import numpy as np

    arrays = [np.ascontiguousarray(a, dtype=dt) for a, dt in ((keys, "<u8"), (pops, "<u4"), (counts, "<f8"))]
    return _pack({"n": int(arrays[0].shape[0]), "stats": stats, "unsupported": [list(u) for u in unsupported],
                  "spilled": [[int(p), name, float(v).hex()] for (p, name), v in spilled.items()]}, arrays)


def _unpack_table(blob):
    head, (keys, pops, counts) = _unpack(blob, [(dt, lambda h: h["n"]) for dt in ("<u8", "<u4", "<f8")], "m_step_sharded")
    spilled = {(int(p), name): float.fromhex(v) for p, name, v in head["spilled"]}  # (insertion order = the sender's)
    return keys, pops, counts, spilled, head["stats"], [tuple(u) for u in head["unsupported"]]


def _pack_hits(patient_ok, hits, n_hits, stats, unsupported):
    """a rank's (or the job's) hit lists as bytes (Python writes a float of the head so that it reads back the same)"""
    import numpy as np

    from . import _native as nat

    hits = np.ascontiguousarray(hits, dtype=nat.SEARCH_DT)
    return _pack({"patients": int(hits.shape[0]), "top_n": int(hits.shape[1]), "ok": [int(x) for x in patient_ok], "stats": stats,
                  "unsupported": [list(u) for u in unsupported]}, [hits, np.ascontiguousarray(n_hits, dtype="<u4")])


def _unpack_hits(blob):
    import numpy as np

    from . import _native as nat

    head, (hits, n_hits) = _unpack(blob, [(nat.SEARCH_DT, lambda h: h["patients"] * h["top_n"]), ("<u4", lambda h: h["patients"])],
                                   "search_sharded")
    return (np.array(head["ok"], dtype=bool), hits.reshape(head["patients"], head["top_n"]), n_hits, head["stats"],
            [tuple(u) for u in head["unsupported"]])


# ---- impute: one stream per rank, every rank writes its pieces into the six final files ------------------------------------
class _Placement:
    """where chunk c's piece of each output file begins: the sum of the sizes of the chunks before it, whoever ran them.
    Sizes travel through the job's store (one key per chunk, set once); a rank asks in increasing chunk order, so its
    running prefix only ever moves forward."""

    def __init__(self, job):
        self.ctl, self.tag = job.ctl, job.tag
        self.own = {}
        self.upto, self.prefix = 0, [0] * 6

    def publish(self, c, sizes):
        sizes = [int(x) for x in sizes[:6]]
        self.own[c] = sizes
        self.ctl.set("grim_sz_%s_%d" % (self.tag, c), ",".join(str(x) for x in sizes))

    def base(self, c):
        while self.upto < c:
            sz = self.own.get(self.upto)
            if sz is None:
                sz = [int(x) for x in self.ctl.wait_key("grim_sz_%s_%d" % (self.tag, self.upto), self.tag).split(",")]
            self.prefix = [a + b for a, b in zip(self.prefix, sz)]
            self.upto += 1
        return list(self.prefix)


class _StreamSink:
    """a rank's data path: one grim_stream for the whole job, a chunk = one input segment.  Alone: the stream appends to the
    six output files.  In a job: `placement` says where a segment's pieces go in the SHARED files, a placer thread asks for
    it segment by segment while the main thread keeps feeding."""

    def __init__(self, imp, config, hap_pop_pair, out_paths, flags, placement=None):
        from . import _native as nat

        self.nat = nat
        planb = config["planb"]
        params = imp._params(config, planb, hap_pop_pair, False)
        ps, keep = nat.prior_spec(config["priority"], imp.unk_priors, imp.count_by_prob)
        ctx = nat.default_context(imp.device)
        paths = {k: out_paths[k] for k in OUTPUT_KEYS if flags[k]}
        self._keep = (params, ps, keep)
        self.imp = imp
        self.placement = placement
        self.st = nat.Stream(ctx, imp.netGraph.device(ctx), imp.netGraph.adict, params, ps, imp.populations,
                             out_paths=paths, want_log=False, masks=imp._phase_masks(config), placed=placement is not None)
        self.first = True
        self.seg = 0
        self.placer_error = None
        self.todo = queue.Queue()
        self.placer = None
        if placement is not None:
            self.placer = threading.Thread(target=self._place_loop, name="grim-placer", daemon=True)
            self.placer.start()

    def _place_loop(self):
        try:
            while True:
                item = self.todo.get()
                if item is None:
                    return
                c, seg = item
                sizes = self.st.segment_wait(seg)  # (returns once the segment is closed -- the next feed, or finish -- and formatted)
                self.placement.publish(c, sizes)
                self.st.segment_place(seg, self.placement.base(c))
        except BaseException as e:  # noqa: B902  (handed to the main thread: feed / finish raise it)
            self.placer_error = e

    def feed(self, raw, line_offset, chunk_no):
        if self.placer_error is not None:
            raise self.placer_error
        if not self.first or line_offset:
            self.st.segment(line_offset)  # (the first chunk is segment 0 unless it does not start at line 0)
            self.seg += 1
        self.first = False
        self.st.write_text(raw)
        if self.placer is not None:
            self.todo.put((chunk_no, self.seg))

    def finish(self):
        try:
            self.st.finish()  # end of input: the last segment is closed; returns when every chunk is formatted (placed
            #                   output) resp. written (alone)
            if self.placer is not None:
                self.todo.put(None)
                self.placer.join()
                self.placer = None
                if self.placer_error is not None:
                    raise self.placer_error
            self.imp.unsupported = self.st.unsupported()
        finally:
            self.abort()

    def abort(self):
        try:
            if self.placer is not None:
                self.todo.put(None)
                self.st.close()  # (fails the waits of the placer thread)
                self.placer.join(timeout=5)
                self.placer = None
            else:
                self.st.close()
        except Exception:
            pass


class _ComputeSink:
    """the same layout from an injected per-chunk compute(config, lines, line_offset) -> texts (tests: the oracle)"""

    def __init__(self, compute, config, out_paths, flags, placement=None):
        self.compute, self.config = compute, config
        self.placement = placement
        self.unsupported = []
        if placement is None:
            self.fh = {k: open(out_paths[k], "wb") for k in OUTPUT_KEYS if flags[k]}
        else:
            self.fd = {k: os.open(out_paths[k], os.O_WRONLY) for k in OUTPUT_KEYS if flags[k]}

    def feed(self, raw, line_offset, chunk_no):
        import io

        # universal newlines, as the product path's grim_stream_write_text
        text = io.TextIOWrapper(io.BytesIO(raw), encoding="utf-8", newline=None).read()
        lines = [l + "\n" for l in text.split("\n")]
        if text.endswith("\n") or not text:
            lines.pop()  # the text ended with a line end: what follows it is not a line
        texts = self.compute(self.config, lines, line_offset)
        data = {}
        for k in OUTPUT_KEYS:
            d = texts.get(k, "")
            data[k] = d if isinstance(d, bytes) else d.encode()
        if self.placement is None:
            for k in OUTPUT_KEYS:
                if data[k] and k in self.fh:
                    self.fh[k].write(data[k])
            return
        self.placement.publish(chunk_no, [len(data[k]) if k in self.fd else 0 for k in OUTPUT_KEYS])
        base = self.placement.base(chunk_no)
        for ki, k in enumerate(OUTPUT_KEYS):
            if data[k] and k in self.fd:
                os.pwrite(self.fd[k], data[k], base[ki])

    def finish(self):
        self.abort()

    def abort(self):
        for fh in getattr(self, "fh", {}).values():
            try:
                fh.close()
            except Exception:
                pass
        for fd in getattr(self, "fd", {}).values():
            try:
                os.close(fd)
            except Exception:
                pass
        self.fh, self.fd = {}, {}


def impute_sharded(conf_file, hap_pop_pair=False, graph=None, compute=None, project_dir_graph="",
                   project_dir_in_file="", chunk_lines=None, return_texts=False):
    """Run `impute` across the ranks of the torch.distributed job (or alone if there is none).  `compute(config, lines,
    line_offset) -> texts` can be injected (tests); the default runs the HIP engine on this rank's GPU (LOCAL_RANK) as one
    stream per rank.  Rank 0 returns {key: path of the final file} (the texts themselves with return_texts=True: a test
    convenience -- the product path never reads its outputs back) plus "unsupported": the subjects of ALL ranks the device
    could not take, as (global line, id, reason), when GRIM_ON_UNSUPPORTED=skip let the job go on without them; the other
    ranks return None.  Every rank raises when any rank failed -- a rank that met unsupported subjects in the default
    `raise` mode included, exactly as the single-GPU impute_file does."""
    from .run_impute_def import load_config
    from .imputation.impute import Imputation as _I, UnsupportedSubjects

    job = _Job("impute_sharded", None, chunk_lines)  # (waits without a deadline)
    ctl, tag = job.ctl, job.tag
    names = {key: (path_key, flag) for key, path_key, flag in _I._OUT_FILES}
    alone = job.world == 1  # the one rank's stream appends to the output files: nothing to place
    files_key = "grim_files_" + tag
    files_announced = False
    placement = None if alone else _Placement(job)
    unsupported = []
    result = None

    def files_failed():  # (the other ranks wait for files_key)
        if job.rank == 0 and not alone and not files_announced:
            ctl.set(files_key, "failed")

    with job.body():
        job.cleanup.callback(files_failed)
        config, out_dir = load_config(conf_file, project_dir_graph, project_dir_in_file)
        flags = {k: (names[k][1] is None or bool(config[names[k][1]])) for k in OUTPUT_KEYS}
        out_paths = {k: config[names[k][0]] for k in OUTPUT_KEYS}
        if job.rank == 0:
            pathlib.Path(out_dir).mkdir(parents=False, exist_ok=True)
            if not alone:
                # the shared output files: made by rank 0 before any rank opens them for its pieces.  An earlier run's file
                # is moved aside and unlinked by a helper thread while the job runs -- truncating hundreds of megabytes of
                # cached pages costs tens of milliseconds, and every other rank would be waiting for it
                stale = []
                for k in OUTPUT_KEYS:
                    if flags[k]:
                        if os.path.isfile(out_paths[k]) and os.path.getsize(out_paths[k]) > (1 << 20):
                            old = "%s.grim_old.%s" % (out_paths[k], tag)
                            os.rename(out_paths[k], old)
                            stale.append(old)
                        os.close(os.open(out_paths[k], os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644))
                ctl.set(files_key, "ok")
                files_announced = True
                if stale:
                    unlinker = threading.Thread(target=lambda: [os.unlink(f) for f in stale], name="grim-unlink", daemon=True)
                    unlinker.start()
                    job.cleanup.callback(unlinker.join)
        elif ctl.wait_key(files_key, tag) != "ok":
            raise RuntimeError("impute_sharded: rank 0 could not create the output files")
        if compute is None:
            imp = job.imputation(config, graph)
            sink = _StreamSink(imp, config, hap_pop_pair, out_paths, flags, placement)
        else:
            imp = None
            sink = _ComputeSink(compute, config, out_paths, flags, placement)
        job.cleanup.callback(sink.abort)
        for c, first, raw in job.chunks(config["imputation_input_file"]):
            sink.feed(raw, first, c)
        sink.finish()
        # subjects the device could not take: the single-GPU path raises unless told to skip them, so does every rank here
        unsupported = list(imp.unsupported) if imp is not None else []
        if unsupported and imp.on_unsupported == "raise":
            raise UnsupportedSubjects(unsupported)
        ctl.set("grim_unsup_%s_%d" % (tag, job.rank), json.dumps(unsupported))
    with job.closing():
        if job.rank == 0:
            if not alone:
                total = placement.base(job.n_chunks)  # every size is on the store by now
                for ki, k in enumerate(OUTPUT_KEYS):
                    if flags[k] and os.path.getsize(out_paths[k]) != total[ki]:
                        raise RuntimeError("impute_sharded: %s holds %d bytes, the chunks add up to %d" % (
                            out_paths[k], os.path.getsize(out_paths[k]), total[ki]))
                for r in range(1, job.world):
                    unsupported += [tuple(u) for u in json.loads(ctl.wait_key("grim_unsup_%s_%d" % (tag, r), tag))]
                unsupported.sort(key=lambda u: u[0])
            result = {"unsupported": [tuple(u) for u in unsupported]}
            for k in OUTPUT_KEYS:
                if not flags[k]:
                    result[k] = "" if return_texts else None
                elif not return_texts:
                    result[k] = out_paths[k]
    if result is not None and return_texts:
        for k in OUTPUT_KEYS:
            if flags[k]:
                with open(out_paths[k]) as fh:
                    result[k] = fh.read()
    return result


# ---- the sharded M-step: every chunk's table onto the store, folded by rank 0 in chunk order ---------------------
def m_step_sharded(conf_file, chunk_lines=None, graph=None, compute=None, timeout_s=1800, block_lines=65536):
    """The M-step across the ranks of the torch.distributed job (or alone if there is none), by the chunk-ordered contract
    of DESIGN 4.5: the input is cut into chunks of `chunk_lines` lines as `impute_sharded` cuts it, the ranks pull chunk
    numbers from the job's counter, each runs a chunk's M-step on its own GPU into a fresh accumulator (grim.em.chunk_table)
    and publishes the chunk's exported table, spilled counts, statistics and unsupported subjects on the job's store; rank 0
    folds the tables in CHUNK order through EmAccumulator.merge_records into a master accumulator and publishes the result.
    -> (counts, stats, table) on EVERY rank, the same bytes: counts {pop: {haplotype: count}} and stats as
    grim.em.m_step_chunked returns them (plus stats["unsupported"]: the subjects of all ranks, by input line, that
    GRIM_ON_UNSUPPORTED=skip let the job go on without), table = (keys, pops, counts) as Graph.refresh takes them.  The
    answer depends on chunk_lines; not on the world size, on which rank ran which chunk, on the order the tables arrive in,
    or on block_lines.  Alone it equals m_step_chunked.

    `compute(config, lines, line_offset) -> (keys, pops, counts, spilled, stats)` can be injected (tests); the fold then
    runs through grim.em.fold_chunk_tables and haplotypes are named by their key.  Every wait ends `timeout_s` seconds
    after the call began at the latest, or when a peer reports an error; every rank raises when any rank failed."""
    return _m_step_sharded(_Job("m_step_sharded", timeout_s, chunk_lines), conf_file, graph, compute, block_lines, {})


def _m_step_sharded(job, conf_file, graph, compute, block_lines, state):
    """m_step_sharded as `job`; `state`: a dict that keeps the rank's Imputation (and with it its device graph) from call to
    call"""
    from . import em
    from .run_impute_def import load_config

    result = None
    with job.body():
        config, _ = load_config(conf_file)
        imp = shared = None
        pop_names, hap_name = list(config.get("pops") or []), str
        if compute is None:
            from . import _native as nat
            from .blocks import Blocks

            imp = state.get("imp")
            if imp is None:
                imp = state["imp"] = job.imputation(config, graph)
            shared = Blocks(imp, config, None, True, True, output_haplotypes=True)
            pop_names, hap_name = list(imp.populations), imp.netGraph.key_to_name
        own = {}  # rank 0 keeps its chunks' tables, the other ranks publish theirs
        for c, first, raw in job.chunks(config["imputation_input_file"]):
            lines = em.chunk_text_lines(raw)
            if compute is None:
                acc, spilled, stats, bad = em.chunk_table(imp, shared, lines, first, block_lines)
                try:
                    keys, pops, counts = acc.export()
                finally:
                    acc.close()
            else:
                keys, pops, counts, spilled, stats = compute(config, lines, first)
                bad = []
            if job.rank == 0:
                own[c] = (keys, pops, counts, spilled, stats, bad)
            else:
                job.publish("grim_emt_%s_%d" % (job.tag, c), _pack_table(keys, pops, counts, spilled, stats, bad))

        def fold():  # rank 0: the chunks' tables in chunk order -> the job's result as bytes
            stats = dict.fromkeys(em.CHUNK_STATS, 0)
            stats.update(kernel_ms=0.0, merge_ms=0.0, chunks=job.n_chunks)
            spilled, unsupported, tables, master = {}, [], [], None
            if compute is None:
                g = imp.netGraph
                master = nat.EmAccumulator(shared.ctx, [g.adict.count(s) for s in range(len(g.full_loci))], len(pop_names))
                job.cleanup.callback(master.close)
            for c in range(job.n_chunks):
                part = own.pop(c, None)
                if part is None:
                    part = _unpack_table(job.collect("grim_emt_%s_%d" % (job.tag, c), True))
                keys, pops, counts, chunk_spilled, chunk_stats, bad = part
                if master is not None:
                    master.merge_records(keys, pops, counts)
                    stats["merge_ms"] += master.merge_ms()
                else:
                    tables.append((keys, pops, counts))
                em.fold_spilled(spilled, chunk_spilled)
                for k in em.CHUNK_STATS:
                    stats[k] += chunk_stats.get(k, 0)
                unsupported += bad
            if master is not None:
                table = master.export()
                stats["rehashes"] += master.stats()["rehashes"]
            else:
                table = em.fold_chunk_tables(tables)
            stats["entries"] = int(table[0].shape[0])
            return _pack_table(table[0], table[1], table[2], spilled, stats, sorted(unsupported))

        keys, pops, counts, spilled, stats, unsupported = _unpack_table(job.from_rank0("grim_emf_" + job.tag, fold))
        stats["unsupported"] = unsupported
        result = (em._counts_by_name(hap_name, pop_names, (keys, pops, counts), spilled), stats, (keys, pops, counts))
    job.close()
    return result


def em_fixed_support_sharded(conf_file, iterations, chunk_lines=None, tol=None, graph=None, timeout_s=1800, block_lines=65536):
    """EM on a fixed support across the ranks of the job: per iteration `m_step_sharded`, then EVERY rank refreshes its own
    device graph with Graph.refresh(ctx, (keys, pops, counts)) through the records door from the one published table --
    rank 0 too, so that all ranks run the same code on the same numbers and hold the same frequencies, bit for bit.  The
    decision to stop (`tol` given and the iteration's delta <= tol) is rank 0's, shared through the store.  -> the list of
    per-iteration dicts of grim.em.em_fixed_support (kernel_ms etc. summed over the chunks) plus `chunks`, `merge_ms` and
    `unsupported`, the same on every rank apart from `refresh_ms`."""
    from . import _native as nat

    state = {}  # one Imputation, and with it one device graph, for every iteration
    out = []
    for _ in range(int(iterations)):
        job = _Job("m_step_sharded", timeout_s, chunk_lines)
        _, it, table = _m_step_sharded(job, conf_file, graph, None, block_lines, state)
        imp = state["imp"]
        rs = imp.netGraph.refresh(nat.default_context(imp.device), table)
        it.update(total=rs["total"], delta=rs["delta"], matched=rs["matched"], zero_full=rs["zero_full"], n_full=rs["n_full"],
                  outside=it["entries"] - rs["matched"], refresh_ms=rs["kernel_ms"])
        out.append(it)
        if job.agree(lambda: "1" if tol is not None and rs["delta"] <= tol else "0") == "1":
            break
    return out


# ---- the sharded donor search: every rank's hit lists onto the store, merged by rank 0 on the device ----------------
SEARCH_SUMS = ("donors_valid", "donors_private", "pairs", "row_pairs", "candidates", "host_pairs", "kernel_ms", "select_ms", "blocks",
               "download_bytes")


def search_sharded(conf_file, patients_path, keep_loci, top_n, min_p0=0.0, chunk_lines=None, graph=None, compute=None, timeout_s=1800,
                   block_lines=65536, direction="either"):
    """The donor search (grim.search.search_donors) across the ranks of the torch.distributed job, or alone if there is none:
    the configuration's input file as donors against the input file `patients_path`.  Every rank builds its graph and opens
    one grim.search.DonorSearch over all patients; the ranks pull donor chunks of `chunk_lines` lines from the job's counter
    as `impute_sharded` cuts them and feed each with its first line's number, so a donor's id is its line in the input file
    and the device accumulates across a rank's chunks.  Ranks other than 0 publish their hit lists on the job's store; rank 0
    merges them into its own through the device's merge door (DonorSearch.merge, one call), takes the answer and publishes it.
    -> (patient_ok, hits, n_hits, stats) on EVERY rank, decoded from the same bytes, as `search_donors` returns them: hits
    and n_hits do not depend on chunk_lines, on the world size, on which rank ran which chunk, or on block_lines; alone it
    equals `search_donors`.  In stats the pair counters (donors_valid, donors_private, pairs, row_pairs, candidates,
    host_pairs) are sums over the ranks and equal `search_donors`'; patients_* and undefined are rank 0's; kernel_ms,
    select_ms, blocks and download_bytes are summed; `chunks`, `merge_ms` (device time of rank 0's merge) and `unsupported`
    (the donor subjects of all ranks, by input line, that GRIM_ON_UNSUPPORTED=skip let the job go on without) are added, and
    `patients_unsupported`, the same of the patients' file.  `direction`: as `search_donors`, the same on every rank: every
    rank's DonorSearch is opened with it, so the lists rank 0 merges are of one direction.

    `compute(config, patient_lines, donor_lines, first) -> (hits, n_hits, stats)` can be injected (tests): a rank then folds
    its chunks' lists, and rank 0 the ranks' lists, with grim.search.merge_hit_lists (the direction is then the one `compute`
    folds under; the keyword is only checked).  Every wait ends `timeout_s` seconds
    after the call began at the latest, or when a peer reports an error; every rank raises when any rank failed."""
    from .match import direction_code
    from .search import _check

    top_n, min_p0 = _check(top_n, min_p0)
    return _search_sharded(_Job("search_sharded", timeout_s, chunk_lines), conf_file, patients_path, keep_loci, top_n, min_p0, graph,
                           compute, block_lines, direction_code(direction))


def _search_sharded(job, conf_file, patients_path, keep_loci, top_n, min_p0, graph, compute, block_lines, direction=0):
    """search_sharded as `job`, top_n, min_p0 and direction checked"""
    import numpy as np

    from .blocks import read_lines
    from .em import chunk_text_lines
    from .run_impute_def import load_config
    from .search import _empty_hits, merge_hit_lists

    result = None
    with job.body():
        config, _ = load_config(conf_file)
        plines = read_lines(patients_path)
        patients_bad = []
        if compute is None:
            from .search import DonorSearch

            imp = job.imputation(config, graph)
            search = DonorSearch(imp, plines, config, keep_loci, top_n, min_p0, block_lines, direction=direction)
            job.cleanup.callback(search.close)
            patients_bad = list(imp.unsupported)
        else:
            running = (_empty_hits(len(plines), top_n), np.zeros(len(plines), dtype=np.uint32))
            sums = dict.fromkeys(SEARCH_SUMS, 0)
        for c, first, raw in job.chunks(config["imputation_input_file"]):
            lines = chunk_text_lines(raw)
            if compute is None:
                search.feed(lines, first=first)
            else:
                hits, n_hits, chunk_stats = compute(config, plines, lines, first)
                running = merge_hit_lists([(hits, n_hits)], top_n, min_p0, running=running)
                for k in SEARCH_SUMS:
                    sums[k] += chunk_stats.get(k, 0)

        def mine():
            if compute is None:
                ok, hits, n_hits, stats = search.hits()
                return ok, hits, n_hits, stats, imp.unsupported[len(patients_bad):]
            return np.ones(len(plines), dtype=bool), running[0], running[1], dict(sums), []

        def merged():  # rank 0: the other ranks' lists merged into its own -> the job's answer as bytes
            others = [_unpack_hits(job.collect("grim_srl_%s_%d" % (job.tag, r), True)) for r in range(1, job.world)]
            for r, part in enumerate(others):
                if part[1].shape != (len(plines), top_n):
                    raise RuntimeError("search_sharded: rank %d sent lists of shape %r" % (r + 1, part[1].shape))
            merge_ms = 0.0
            if compute is None:
                if others:
                    search.merge(np.stack([part[1] for part in others]), np.stack([part[2] for part in others]))
                    merge_ms = search.merge_ms
                ok, hits, n_hits, stats, unsupported = mine()
            else:
                ok, hits, n_hits, stats, unsupported = mine()
                hits, n_hits = merge_hit_lists([part[1:3] for part in others], top_n, min_p0, running=(hits, n_hits))
            unsupported = list(unsupported)
            for part in others:
                for k in SEARCH_SUMS:
                    stats[k] = stats.get(k, 0) + part[3].get(k, 0)
                unsupported += part[4]
            stats.update(chunks=job.n_chunks, merge_ms=merge_ms, patients_unsupported=[list(u) for u in patients_bad])
            return _pack_hits(ok, hits, n_hits, stats, sorted(unsupported))

        if job.rank != 0:
            job.publish("grim_srl_%s_%d" % (job.tag, job.rank), _pack_hits(*mine()))
        ok, hits, n_hits, stats, unsupported = _unpack_hits(job.from_rank0("grim_srf_" + job.tag, merged))
        stats["unsupported"] = unsupported
        stats["patients_unsupported"] = [tuple(u) for u in stats["patients_unsupported"]]
        result = (ok, hits, n_hits, stats)
    job.close()
    return result


def search_file_sharded(conf_file, patients_path, keep_loci, out_path, top_n, min_p0=0.0, chunk_lines=None, graph=None, timeout_s=1800,
                        block_lines=65536, direction="either"):
    """grim.search.search_file across the ranks of the job through `search_sharded`: rank 0 writes the CSV at `out_path`, byte
    for byte the file `search_file` writes; every rank returns when it is written, and every rank raises when rank 0 could
    not write it.  `direction`: as `search_sharded`.  -> stats, the same on every rank"""
    from .blocks import read_lines
    from .match import direction_code
    from .imputation.networkx_graph import Graph
    from .run_impute_def import load_config
    from .search import _check, write_hits_csv

    top_n, min_p0 = _check(top_n, min_p0)
    direction = direction_code(direction)
    config, _ = load_config(conf_file)
    if graph is None:  # (the CSV's rows need it too)
        graph = Graph(config).build_graph(config["node_file"], config["top_links_file"], config["edges_file"])
    job = _Job("search_sharded", timeout_s, chunk_lines)
    ok, hits, n_hits, stats = _search_sharded(job, conf_file, patients_path, keep_loci, top_n, min_p0, graph, None, block_lines, direction)
    failure = []

    def write():  # on rank 0 (or alone) -> what the other ranks learn: "ok" or the error's text
        try:
            write_hits_csv(out_path, graph, keep_loci, read_lines(patients_path), read_lines(config["imputation_input_file"]), ok, hits,
                           n_hits)
            return "ok"
        except Exception as e:
            failure.append(e)
            return "%s: %s" % (type(e).__name__, e)

    text = job.agree(write)
    if failure:
        raise failure[0]
    if text != "ok":
        raise RuntimeError("search_file_sharded: rank 0 could not write %s: %s" % (out_path, text))
    return stats


_call_counter = [0]


def _next_call():
    _call_counter[0] += 1
    return _call_counter[0]
