"""
Multi-GPU driver: one process per GPU, the subject file cut into fixed-size chunks of lines that the ranks PULL from a
shared counter, graph replicated per GPU, NO collective on the data path.

This is the split the reference's scripts/runfile_mp.py:109-148 intends (`split -l` + one worker per chunk + `cat` of the
per-chunk outputs), with three differences: workers are GPU ranks; chunks are handed out dynamically (a subject's cost
varies by more than 1000x with its ambiguity, so equal line counts are not equal work -- SURVEY 8e); `.miss/.problem`
keep the GLOBAL line index (the reference's per-chunk runs restart at 0).

Data path of a rank: ONE long-lived streaming pipeline (grim_stream: tokenizer threads -> device -> formatter threads)
for the whole job.  A pulled chunk is a byte range of the input file; its raw bytes go to the stream as one input SEGMENT
(grim_stream_segment carries the chunk's global line index), so chunk k+1 is tokenised while chunk k is on the device -- no
per-chunk stream, no Python line splitting.

Outputs are written ONCE, straight into the six final files, by every rank (no part files, no `cat`): as soon as a chunk
is formatted its rank publishes the SIZES of its six pieces on the job's store; where chunk c's pieces begin is the sum of
the sizes of the chunks before it, so only sizes wait for sizes -- a rank's placer thread picks them up and the stream's
worker threads pwrite the formatted buffers at their final offsets (grim_stream_segment_wait / _place) while the pipeline
is already busy with later chunks.

The only communication is the control plane: an atomic fetch-add on the job's rendezvous store (the next chunk number),
the job's id, six sizes per chunk, one barrier at the end, and an error slot per rank so that a rank that fails does not
leave the others waiting.

The M-step and the fixed-support EM shard the same way (`m_step_sharded`, `em_fixed_support_sharded`): ranks
pull chunks, each chunk's count table is built in a fresh accumulator on the rank's GPU and published on the store as bytes,
rank 0 folds the tables in CHUNK order (EmAccumulator.merge_records) and publishes the one result every rank returns.

Launch:  torchrun --nproc-per-node N --master-addr 127.0.0.1 your_script.py   ->  impute_sharded(conf)
(`impute_sharded` joins the job itself -- gloo, control plane only -- when the caller has not initialised
torch.distributed; alone, without WORLD_SIZE > 1, it runs every chunk in this process).
"""

import json
import os
import pathlib
import queue
import threading
import time
import traceback
import uuid

OUTPUT_KEYS = ("umug", "umug_pops", "pmug", "pmug_pops", "miss", "problem")
DEFAULT_CHUNK_LINES = 65536


def shard_range(n, rank, world):
    """[begin, end) of rank's contiguous block of ceil(n/world) lines (the static split of runfile_mp.py:113-124)."""
    per = -(-n // world) if world > 0 else n
    return min(n, rank * per), min(n, (rank + 1) * per)


def merge_texts(per_rank):
    """per_rank: list (rank order) of dicts of output texts -> one dict, rank order preserved."""
    return {k: "".join(t.get(k, "") for t in per_rank) for k in OUTPUT_KEYS}


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
                self._own_group = True
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


class _Placement:
    """where chunk c's piece of each output file begins: the sum of the sizes of the chunks before it, whoever ran them.
    Sizes travel through the job's store (one key per chunk, set once); a rank asks in increasing chunk order, so its
    running prefix only ever moves forward."""

    def __init__(self, ctl, tag):
        self.ctl, self.tag = ctl, tag
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

    ctl = _Control()
    chunk_lines = int(chunk_lines or os.environ.get("GRIM_SHARD_LINES", DEFAULT_CHUNK_LINES))
    names = {key: (path_key, flag) for key, path_key, flag in _I._OUT_FILES}
    error = peer_failed = None
    sink = unlinker = None
    files_announced = False
    alone = ctl.world == 1  # the one rank's stream appends to the output files: nothing to place
    # the job's id: unique per call and per job, published by rank 0 (keys of an earlier job on the same store never match)
    tag = ctl.share("grim_job_%d" % _next_call(), lambda: uuid.uuid4().hex[:12])
    files_key = "grim_files_" + tag
    config = flags = None
    n_chunks = 0
    placement = None if alone else _Placement(ctl, tag)
    unsupported = []
    try:
        config, out_dir = load_config(conf_file, project_dir_graph, project_dir_in_file)
        in_path = config["imputation_input_file"]
        flags = {k: (names[k][1] is None or bool(config[names[k][1]])) for k in OUTPUT_KEYS}
        out_paths = {k: config[names[k][0]] for k in OUTPUT_KEYS}
        if ctl.rank == 0:
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
        elif ctl.wait_key(files_key, tag) != "ok":
            raise RuntimeError("impute_sharded: rank 0 could not create the output files")
        offs = chunk_offsets(in_path, chunk_lines)
        n_chunks = len(offs) - 1
        if compute is None:
            from .imputation.networkx_graph import Graph
            from . import _native as nat

            if graph is None:
                graph = Graph(config).build_graph(config["node_file"], config["top_links_file"], config["edges_file"])
            n_dev = max(1, nat.lib().grim_device_count())
            imp = _I(graph, config, device=ctl.local % n_dev)
            sink = _StreamSink(imp, config, hap_pop_pair, out_paths, flags, placement)
        else:
            imp = None
            sink = _ComputeSink(compute, config, out_paths, flags, placement)
        with open(in_path, "rb") as fh:
            while True:
                c = ctl.next_chunk(tag)
                if c >= n_chunks:
                    break
                fh.seek(offs[c])
                sink.feed(fh.read(offs[c + 1] - offs[c]), c * chunk_lines, c)
        sink.finish()
        sink = None
        # subjects the device could not take: the single-GPU path raises unless told to skip them, so does every rank here
        unsupported = list(imp.unsupported) if imp is not None else []
        if unsupported and imp.on_unsupported == "raise":
            raise UnsupportedSubjects(unsupported)
        ctl.set("grim_unsup_%s_%d" % (tag, ctl.rank), json.dumps(unsupported))
    except BaseException as e:  # the other ranks must not wait for this one forever: report, reach the barrier, raise
        if sink is not None:
            sink.abort()
        if isinstance(e, _PeerFailed):
            peer_failed = e  # not this rank's failure: the barrier's error list names the rank whose it is
        else:
            error = e
            ctl.report_error(tag, "%s: %s\n%s" % (type(e).__name__, e, traceback.format_exc()))
        if ctl.rank == 0 and not alone and not files_announced:
            ctl.set(files_key, "failed")
    failed = ctl.barrier_and_errors(tag)
    result = None
    try:
        if error is not None:
            raise error
        if failed:
            raise RuntimeError("impute_sharded: rank(s) %s failed:\n%s" % ([r for r, _ in failed], failed[0][1]))
        if peer_failed is not None:
            raise peer_failed
        if ctl.rank == 0:
            if not alone:
                total = placement.base(n_chunks)  # every size is on the store by now
                for ki, k in enumerate(OUTPUT_KEYS):
                    if flags[k] and os.path.getsize(out_paths[k]) != total[ki]:
                        raise RuntimeError("impute_sharded: %s holds %d bytes, the chunks add up to %d" % (
                            out_paths[k], os.path.getsize(out_paths[k]), total[ki]))
                for r in range(1, ctl.world):
                    unsupported += [tuple(u) for u in json.loads(ctl.wait_key("grim_unsup_%s_%d" % (tag, r), tag))]
                unsupported.sort(key=lambda u: u[0])
            result = {"unsupported": [tuple(u) for u in unsupported]}
            for k in OUTPUT_KEYS:
                path_key, _ = names[k]
                if not flags[k]:
                    result[k] = "" if return_texts else None
                elif not return_texts:
                    result[k] = config[path_key]
    finally:
        if unlinker is not None:
            unlinker.join()
        ctl.barrier()  # one barrier at the end on every path: nobody leaves while another rank still reads the store
    if ctl.rank == 0 and return_texts and result is not None:
        for k in OUTPUT_KEYS:
            if flags[k]:
                with open(config[names[k][0]]) as fh:
                    result[k] = fh.read()
    return result


# ---- the sharded M-step: every chunk's table onto the store, folded by rank 0 in chunk order ---------------------
PIECE_BYTES = 4 << 20  # the most one store key carries: the store's own value limit has not been measured


def _pack_table(keys, pops, counts, spilled, stats, unsupported):
    """a chunk's (or the job's) result as bytes: a JSON head (floats as hex: every bit travels) and the three arrays"""
    import struct

    import numpy as np

    keys = np.ascontiguousarray(keys, dtype="<u8")
    pops = np.ascontiguousarray(pops, dtype="<u4")
    counts = np.ascontiguousarray(counts, dtype="<f8")
    head = json.dumps({"n": int(keys.shape[0]), "stats": stats, "unsupported": [list(u) for u in unsupported],
                       "spilled": [[int(p), name, float(v).hex()] for (p, name), v in spilled.items()]}).encode()
    return struct.pack("<Q", len(head)) + head + keys.tobytes() + pops.tobytes() + counts.tobytes()


def _unpack_table(blob):
    import struct

    import numpy as np

    (n_head,) = struct.unpack_from("<Q", blob, 0)
    head = json.loads(blob[8:8 + n_head].decode())
    n, at = head["n"], 8 + n_head
    if len(blob) != at + 20 * n:
        raise RuntimeError("m_step_sharded: a table of %d entries in %d bytes" % (n, len(blob) - at))
    keys = np.frombuffer(blob, dtype="<u8", count=n, offset=at).copy()
    pops = np.frombuffer(blob, dtype="<u4", count=n, offset=at + 8 * n).copy()
    counts = np.frombuffer(blob, dtype="<f8", count=n, offset=at + 12 * n).copy()
    spilled = {(int(p), name): float.fromhex(v) for p, name, v in head["spilled"]}  # (insertion order = the sender's)
    return keys, pops, counts, spilled, head["stats"], [tuple(u) for u in head["unsupported"]]


def _publish(ctl, name, blob):
    """blob under `name`: pieces of at most PIECE_BYTES, then the head key that says how many (set last: who sees it finds
    every piece)"""
    n = max(1, -(-len(blob) // PIECE_BYTES))
    for i in range(n):
        ctl.set("%s_%d" % (name, i), blob[i * PIECE_BYTES:(i + 1) * PIECE_BYTES])
    ctl.set(name, str(n))


def _collect(ctl, name, tag, delete):
    n = int(ctl.wait_key(name, tag))
    blob = b"".join(ctl.wait_bytes("%s_%d" % (name, i), tag) for i in range(n))
    if delete:
        for i in range(n):
            ctl.delete("%s_%d" % (name, i))
        ctl.delete(name)
    return blob


def _names_of(keys, pops, counts, spilled, pop_names, hap_name):
    out = {}
    names = {}
    for key, p, v in zip(keys.tolist(), pops.tolist(), counts.tolist()):
        name = names.get(key)
        if name is None:
            name = names[key] = hap_name(key)
        out.setdefault(pop_names[p] if p < len(pop_names) else str(p), {})[name] = v
    for (p, name), v in spilled.items():
        out.setdefault(pop_names[p] if p < len(pop_names) else str(p), {})[name] = v
    return out


M_STEP_SUMS = ("subjects_used", "skipped_plan_c", "contributions", "rehashes", "spill", "blocks", "kernel_ms")


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
    return _m_step_sharded(conf_file, chunk_lines, graph, compute, timeout_s, block_lines, None)


def _m_step_sharded(conf_file, chunk_lines, graph, compute, timeout_s, block_lines, _state):
    """m_step_sharded; `_state`: a dict that keeps the rank's Imputation (and with it its device graph) from call to call"""
    from .em import chunk_text_lines
    from .run_impute_def import load_config

    ctl = _Control(timeout_s)
    chunk_lines = int(chunk_lines or os.environ.get("GRIM_SHARD_LINES", DEFAULT_CHUNK_LINES))
    error = peer_failed = None
    result = None
    tag = ctl.share("grim_job_%d" % _next_call(), lambda: uuid.uuid4().hex[:12])
    master = None
    try:
        config, _ = load_config(conf_file)
        in_path = config["imputation_input_file"]
        offs = chunk_offsets(in_path, chunk_lines)
        n_chunks = len(offs) - 1
        imp = shared = None
        if compute is None:
            from . import _native as nat
            from .blocks import Blocks
            from .em import chunk_table
            from .imputation.impute import Imputation as _I
            from .imputation.networkx_graph import Graph

            if _state is not None and _state.get("imp") is not None:
                imp = _state["imp"]
            else:
                if graph is None:
                    graph = Graph(config).build_graph(config["node_file"], config["top_links_file"], config["edges_file"])
                n_dev = max(1, nat.lib().grim_device_count())
                imp = _I(graph, config, device=ctl.local % n_dev)
                if _state is not None:
                    _state["imp"] = imp
            shared = Blocks(imp, config, None, True, True, output_haplotypes=True)
            pop_names = list(imp.populations)
            hap_name = imp.netGraph.key_to_name
        else:
            pop_names = list(config.get("pops") or [])
            hap_name = str
        # ---- this rank's chunks ----------------------------------------------------------------------------------------
        own = {}
        with open(in_path, "rb") as fh:
            while True:
                c = ctl.next_chunk(tag)
                if c >= n_chunks:
                    break
                fh.seek(offs[c])
                lines = chunk_text_lines(fh.read(offs[c + 1] - offs[c]))
                if compute is None:
                    acc, spilled, stats, bad = chunk_table(imp, shared, lines, c * chunk_lines, block_lines)
                    try:
                        keys, pops, counts = acc.export()
                    finally:
                        acc.close()
                else:
                    keys, pops, counts, spilled, stats = compute(config, lines, c * chunk_lines)
                    bad = []
                if ctl.rank == 0:
                    own[c] = (keys, pops, counts, spilled, stats, bad)
                else:
                    _publish(ctl, "grim_emt_%s_%d" % (tag, c), _pack_table(keys, pops, counts, spilled, stats, bad))
        # ---- rank 0: the fold, in chunk order --------------------------------------------------------------------------
        final = "grim_emf_" + tag
        if ctl.rank == 0:
            from .em import fold_chunk_tables, fold_spilled

            stats = dict.fromkeys(M_STEP_SUMS, 0)
            stats.update(kernel_ms=0.0, merge_ms=0.0, chunks=n_chunks)
            spilled, unsupported, tables = {}, [], []
            if compute is None:
                g = imp.netGraph
                master = nat.EmAccumulator(shared.ctx, [g.adict.count(s) for s in range(len(g.full_loci))], len(pop_names))
            for c in range(n_chunks):
                part = own.pop(c, None)
                if part is None:
                    part = _unpack_table(_collect(ctl, "grim_emt_%s_%d" % (tag, c), tag, True))
                keys, pops, counts, chunk_spilled, chunk_stats, bad = part
                if master is not None:
                    master.merge_records(keys, pops, counts)
                    stats["merge_ms"] += master.merge_ms()
                else:
                    tables.append((keys, pops, counts))
                fold_spilled(spilled, chunk_spilled)
                for k in M_STEP_SUMS:
                    stats[k] += chunk_stats.get(k, 0)
                unsupported += bad
            if master is not None:
                table = master.export()
                stats["rehashes"] += master.stats()["rehashes"]
            else:
                table = fold_chunk_tables(tables)
            stats["entries"] = int(table[0].shape[0])
            blob = _pack_table(table[0], table[1], table[2], spilled, stats, sorted(unsupported))
            if ctl.world > 1:
                _publish(ctl, final, blob)
        else:
            blob = _collect(ctl, final, tag, False)
        keys, pops, counts, spilled, stats, unsupported = _unpack_table(blob)  # every rank reads the same bytes
        stats["unsupported"] = unsupported
        result = (_names_of(keys, pops, counts, spilled, pop_names, hap_name), stats, (keys, pops, counts))
    except BaseException as e:  # the other ranks must not wait for this one: report, reach the barrier, raise
        if isinstance(e, _PeerFailed):
            peer_failed = e
        else:
            error = e
            ctl.report_error(tag, "%s: %s\n%s" % (type(e).__name__, e, traceback.format_exc()))
    finally:
        if master is not None:
            master.close()
    failed = ctl.barrier_and_errors(tag)
    try:
        if error is not None:
            raise error
        if failed:
            raise RuntimeError("m_step_sharded: rank(s) %s failed:\n%s" % ([r for r, _ in failed], failed[0][1]))
        if peer_failed is not None:
            raise peer_failed
    finally:
        ctl.barrier()  # nobody leaves while another rank still reads the store
        if ctl.rank == 0 and ctl.world > 1 and result is not None:
            n = max(1, -(-len(blob) // PIECE_BYTES))
            for i in range(n):
                ctl.delete("grim_emf_%s_%d" % (tag, i))
            ctl.delete("grim_emf_" + tag)
    return result


def em_fixed_support_sharded(conf_file, iterations, chunk_lines=None, tol=None, graph=None, timeout_s=1800, block_lines=65536):
    """EM on a fixed support across the ranks of the job: per iteration `m_step_sharded`, then EVERY rank refreshes its own
    device graph with Graph.refresh(ctx, (keys, pops, counts)) through the records door from the one published table --
    rank 0 too, so that all ranks run the same code on the same numbers and hold the same frequencies, bit for bit.  The
    decision to stop (`tol` given and the iteration's delta <= tol) is rank 0's, shared through the store.  -> the list of
    per-iteration dicts of grim.em.em_fixed_support (kernel_ms etc. summed over the chunks) plus `chunks`, `merge_ms` and
    `unsupported`, the same on every rank apart from `refresh_ms`."""
    from . import _native as nat

    state = {"imp": None}  # one Imputation, and with it one device graph, for every iteration
    out = []
    for _ in range(int(iterations)):
        _, it, table = _m_step_sharded(conf_file, chunk_lines, graph, None, timeout_s, block_lines, state)
        ctl, imp = _Control(timeout_s), state["imp"]
        rs = imp.netGraph.refresh(nat.default_context(imp.device), table)
        it.update(total=rs["total"], delta=rs["delta"], matched=rs["matched"], zero_full=rs["zero_full"], n_full=rs["n_full"],
                  outside=it["entries"] - rs["matched"], refresh_ms=rs["kernel_ms"])
        out.append(it)
        stop = ctl.share("grim_emstop_%d" % _next_call(), lambda: "1" if tol is not None and rs["delta"] <= tol else "0")
        if stop == "1":
            break
    return out


# ---- the sharded donor search: every rank's hit lists onto the store, merged by rank 0 on the device ----------------
SEARCH_SUMS = ("donors_valid", "donors_private", "pairs", "row_pairs", "candidates", "host_pairs", "kernel_ms", "select_ms", "blocks",
               "download_bytes")


def _pack_hits(patient_ok, hits, n_hits, stats, unsupported):
    """a rank's (or the job's) hit lists as bytes: a JSON head (Python writes a float so that it reads back the same) and the
    raw hits / n_hits bytes"""
    import struct

    import numpy as np

    from . import _native as nat

    hits = np.ascontiguousarray(hits, dtype=nat.SEARCH_DT)
    n_hits = np.ascontiguousarray(n_hits, dtype="<u4")
    head = json.dumps({"patients": int(hits.shape[0]), "top_n": int(hits.shape[1]), "ok": [int(x) for x in patient_ok], "stats": stats,
                       "unsupported": [list(u) for u in unsupported]}).encode()
    return struct.pack("<Q", len(head)) + head + hits.tobytes() + n_hits.tobytes()


def _unpack_hits(blob):
    import struct

    import numpy as np

    from . import _native as nat

    (n_head,) = struct.unpack_from("<Q", blob, 0)
    head = json.loads(blob[8:8 + n_head].decode())
    n_p, top_n, at = head["patients"], head["top_n"], 8 + n_head
    size = nat.SEARCH_DT.itemsize * n_p * top_n
    if len(blob) != at + size + 4 * n_p:
        raise RuntimeError("search_sharded: hit lists of %d patients x %d in %d bytes" % (n_p, top_n, len(blob) - at))
    hits = np.frombuffer(blob, dtype=nat.SEARCH_DT, count=n_p * top_n, offset=at).reshape(n_p, top_n).copy()
    n_hits = np.frombuffer(blob, dtype="<u4", count=n_p, offset=at + size).copy()
    return np.array(head["ok"], dtype=bool), hits, n_hits, head["stats"], [tuple(u) for u in head["unsupported"]]


def search_sharded(conf_file, patients_path, keep_loci, top_n, min_p0=0.0, chunk_lines=None, graph=None, compute=None, timeout_s=1800,
                   block_lines=65536):
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
    `patients_unsupported`, the same of the patients' file.

    `compute(config, patient_lines, donor_lines, first) -> (hits, n_hits, stats)` can be injected (tests): a rank then folds
    its chunks' lists, and rank 0 the ranks' lists, with grim.search.merge_hit_lists.  Every wait ends `timeout_s` seconds
    after the call began at the latest, or when a peer reports an error; every rank raises when any rank failed."""
    import numpy as np

    from .blocks import read_lines
    from .em import chunk_text_lines
    from .run_impute_def import load_config
    from .search import _check, _empty_hits, merge_hit_lists

    top_n, min_p0 = _check(top_n, min_p0)
    ctl = _Control(timeout_s)
    chunk_lines = int(chunk_lines or os.environ.get("GRIM_SHARD_LINES", DEFAULT_CHUNK_LINES))
    error = peer_failed = None
    result = blob = None
    tag = ctl.share("grim_job_%d" % _next_call(), lambda: uuid.uuid4().hex[:12])
    search = None
    try:
        config, _ = load_config(conf_file)
        in_path = config["imputation_input_file"]
        offs = chunk_offsets(in_path, chunk_lines)
        n_chunks = len(offs) - 1
        plines = read_lines(patients_path)
        imp = None
        patients_bad = []
        if compute is None:
            from . import _native as nat
            from .imputation.impute import Imputation as _I
            from .imputation.networkx_graph import Graph
            from .search import DonorSearch

            if graph is None:
                graph = Graph(config).build_graph(config["node_file"], config["top_links_file"], config["edges_file"])
            n_dev = max(1, nat.lib().grim_device_count())
            imp = _I(graph, config, device=ctl.local % n_dev)
            search = DonorSearch(imp, plines, config, keep_loci, top_n, min_p0, block_lines)
            patients_bad = list(imp.unsupported)
        else:
            running = (_empty_hits(len(plines), top_n), np.zeros(len(plines), dtype=np.uint32))
            sums = dict.fromkeys(SEARCH_SUMS, 0)
        # ---- this rank's chunks ----------------------------------------------------------------------------------------
        with open(in_path, "rb") as fh:
            while True:
                c = ctl.next_chunk(tag)
                if c >= n_chunks:
                    break
                fh.seek(offs[c])
                lines = chunk_text_lines(fh.read(offs[c + 1] - offs[c]))
                if compute is None:
                    search.feed(lines, first=c * chunk_lines)
                else:
                    hits, n_hits, chunk_stats = compute(config, plines, lines, c * chunk_lines)
                    running = merge_hit_lists([(hits, n_hits)], top_n, min_p0, running=running)
                    for k in SEARCH_SUMS:
                        sums[k] += chunk_stats.get(k, 0)

        def mine():
            if compute is None:
                ok, hits, n_hits, stats = search.hits()
                return ok, hits, n_hits, stats, imp.unsupported[len(patients_bad):]
            return np.ones(len(plines), dtype=bool), running[0], running[1], dict(sums), []

        # ---- ranks other than 0 publish their lists; rank 0 merges them into its own -----------------------------------
        final = "grim_srf_" + tag
        if ctl.rank != 0:
            _publish(ctl, "grim_srl_%s_%d" % (tag, ctl.rank), _pack_hits(*mine()))
            blob = _collect(ctl, final, tag, False)
        else:
            others = [_unpack_hits(_collect(ctl, "grim_srl_%s_%d" % (tag, r), tag, True)) for r in range(1, ctl.world)]
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
            stats.update(chunks=n_chunks, merge_ms=merge_ms, patients_unsupported=[list(u) for u in patients_bad])
            blob = _pack_hits(ok, hits, n_hits, stats, sorted(unsupported))
            if ctl.world > 1:
                _publish(ctl, final, blob)
        ok, hits, n_hits, stats, unsupported = _unpack_hits(blob)  # every rank reads the same bytes
        stats["unsupported"] = unsupported
        stats["patients_unsupported"] = [tuple(u) for u in stats["patients_unsupported"]]
        result = (ok, hits, n_hits, stats)
    except BaseException as e:  # the other ranks must not wait for this one: report, reach the barrier, raise
        if isinstance(e, _PeerFailed):
            peer_failed = e
        else:
            error = e
            ctl.report_error(tag, "%s: %s\n%s" % (type(e).__name__, e, traceback.format_exc()))
    finally:
        if search is not None:
            search.close()
    failed = ctl.barrier_and_errors(tag)
    try:
        if error is not None:
            raise error
        if failed:
            raise RuntimeError("search_sharded: rank(s) %s failed:\n%s" % ([r for r, _ in failed], failed[0][1]))
        if peer_failed is not None:
            raise peer_failed
    finally:
        ctl.barrier()  # nobody leaves while another rank still reads the store
        if ctl.rank == 0 and ctl.world > 1:
            _discard(ctl, "grim_srf_" + tag)
            for r in range(1, ctl.world):  # lists a rank published before the job failed: nobody will collect them
                _discard(ctl, "grim_srl_%s_%d" % (tag, r))
    return result


def _discard(ctl, name):
    """best effort: the pieces and the head key of a blob published under `name`, if its head key is there"""
    try:
        if ctl._has(name):
            for i in range(int(ctl.store.get(name))):
                ctl.delete("%s_%d" % (name, i))
            ctl.delete(name)
    except Exception:
        pass


def search_file_sharded(conf_file, patients_path, keep_loci, out_path, top_n, min_p0=0.0, chunk_lines=None, graph=None, timeout_s=1800,
                        block_lines=65536):
    """grim.search.search_file across the ranks of the job through `search_sharded`: rank 0 writes the CSV at `out_path`, byte
    for byte the file `search_file` writes; every rank returns when it is written, and every rank raises when rank 0 could
    not write it.  -> stats, the same on every rank"""
    from .blocks import read_lines
    from .imputation.networkx_graph import Graph
    from .run_impute_def import load_config
    from .search import write_hits_csv

    config, _ = load_config(conf_file)
    if graph is None:
        graph = Graph(config).build_graph(config["node_file"], config["top_links_file"], config["edges_file"])
    ok, hits, n_hits, stats = search_sharded(conf_file, patients_path, keep_loci, top_n, min_p0=min_p0, chunk_lines=chunk_lines, graph=graph,
                                             timeout_s=timeout_s, block_lines=block_lines)
    ctl = _Control(timeout_s)
    failure = []

    def write():  # on rank 0 (or alone) -> what the other ranks learn: "ok" or the error's text
        try:
            write_hits_csv(out_path, graph, keep_loci, read_lines(patients_path), read_lines(config["imputation_input_file"]), ok, hits,
                           n_hits)
            return "ok"
        except Exception as e:
            failure.append(e)
            return "%s: %s" % (type(e).__name__, e)

    key = "grim_srcsv_%d" % _next_call()
    text = ctl.share(key, write)
    ctl.barrier()  # every rank has read the key
    if ctl.rank == 0:
        ctl.delete(key)
    if failure:
        raise failure[0]
    if text != "ok":
        raise RuntimeError("search_file_sharded: rank 0 could not write %s: %s" % (out_path, text))
    return stats


_call_counter = [0]


def _next_call():
    _call_counter[0] += 1
    return _call_counter[0]
