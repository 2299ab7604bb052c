"""
ctypes binding of libgrim_hip.so (include/grim_hip.h).  There is no CPU fallback: if the
library is missing or no HIP device is visible, every compute entry point raises.
"""

import ctypes as C
import os

import numpy as np

MAXL = 5
ABITS = 12
MAXPH = 16
MAXPOP = 64
TOPCAP = 128
MAXLADDER = 64
MAXROWS = 8

ST_OK, ST_MISS, ST_UNSUPPORTED, ST_NOPHASE = 0, 1, 2, 3
T_UMUG, T_UMUG_POPS, T_PMUG, T_PMUG_POPS = 0, 1, 2, 3
# `which` of DeviceBatch.kernel_ms (GRIM_MS_* in grim_hip.h); MS_MEAN | x = the mean of x over the timed runs
(MS_TOTAL, MS_PLAN_A, MS_PLAN_B, MS_HALF_WAVE, MS_GENERAL, MS_ONE_WAVE, MS_TABLES, MS_COMPACT, MS_TOKENIZER,
 MS_MID) = range(10)
MS_MEAN = 0x10

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GRIM_LIB") or os.path.join(os.path.dirname(_HERE), "libgrim_hip.so")


class GraphDesc(C.Structure):
    _fields_ = [
        ("n_nodes", C.c_uint32), ("n_pops", C.c_uint32), ("n_loci", C.c_uint32), ("full_mask", C.c_uint32),
        ("node_key", C.c_void_p), ("node_mask", C.c_void_p), ("freq", C.c_void_p),
        ("a_start", C.c_void_p), ("a_nbr", C.c_void_p), ("n_a_nbr", C.c_uint64),
        ("b_conn", C.c_void_p), ("b_start", C.c_void_p), ("b_nbr", C.c_void_p),
        ("n_conn", C.c_uint32), ("n_b_nbr", C.c_uint64),
        ("lab_start", C.c_void_p), ("lab_nodes", C.c_void_p), ("label_order_bad", C.c_uint32), ("reserved", C.c_uint32),
    ]


class Params(C.Structure):
    _fields_ = [
        ("ladder", C.c_double * MAXLADDER), ("n_ladder", C.c_int32), ("top_n", C.c_uint32),
        ("opt_threshold", C.c_uint64), ("n_results", C.c_uint32), ("n_pop_results", C.c_uint32),
        ("out_muug", C.c_uint8), ("out_haps", C.c_uint8), ("planb", C.c_uint8), ("em_mr", C.c_uint8), ("em", C.c_uint8),
        ("save_mode", C.c_uint8), ("eps_nonpositive", C.c_uint8),
        ("pop_rank", C.c_uint8 * MAXPOP), ("factor_missing_pow", C.c_double * (MAXL + 1)),
        ("planb_rows", C.c_uint8), ("planb_nblk", C.c_uint8 * MAXROWS),
        ("planb_blk", (C.c_uint8 * MAXL) * MAXROWS),
    ]


class BatchDesc(C.Structure):
    _fields_ = [
        ("n_subjects", C.c_uint32), ("subjects", C.c_void_p), ("tokens", C.c_void_p), ("n_tokens", C.c_uint64),
        ("priors", C.c_void_p), ("n_priors", C.c_uint32),
    ]


# numpy mirrors of the plain-data structs
SUBJECT_DT = np.dtype([
    ("tok_off", "<u4"), ("prior_idx", "<u2"), ("n_loci", "u1"), ("flags", "u1"),
    ("slot", "u1", (MAXL,)), ("pad", "u1", (3,)),
    ("cnt", "<u2", (MAXL, 2)), ("wid", "<u2", (MAXL, 2)), ("reserved", "<u4", (2,)),
], align=False)
assert SUBJECT_DT.itemsize == 64

RESULT_DT = np.dtype([
    ("status", "u1"), ("plan", "u1"), ("reason", "u1"), ("plan_phased", "u1"),
    ("n_pairs", "<u4"), ("n_genotypes", "<u4"),
    ("row_off", "<u4", (4,)), ("n_rows", "<u4", (4,)), ("pad2", "<u4"), ("max_prob", "<f8"),
], align=False)
assert RESULT_DT.itemsize == 56

ROW_DT = np.dtype([("a", "<u8"), ("b", "<u8"), ("prob", "<f8"), ("popa", "<u4"), ("popb", "<u4")])
assert ROW_DT.itemsize == 32

_lib = None


class NativeError(RuntimeError):
    pass


def _share_hip_runtime_with_torch():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so.  Two HIP runtimes in one process do not
    work (whoever comes second sees no GPU), and torch.distributed's RCCL backend needs torch's, so
    when a torch wheel is installed its runtime is loaded first and this library binds to it.
    GRIM_HIP_RUNTIME=system keeps the system runtime (then do not use torch.cuda in the process)."""
    if os.environ.get("GRIM_HIP_RUNTIME") == "system":
        return
    try:
        import importlib.util

        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass


def lib():
    """Load the shared library (once).  Raises NativeError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(
            "libgrim_hip.so not found at %s -- build it with `python __graft_entry__.py` "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
    _share_hip_runtime_with_torch()
    L = C.CDLL(LIB_PATH)
    L.grim_create.restype = C.c_void_p
    L.grim_create.argtypes = [C.c_int]
    L.grim_export_engine.restype = C.c_int
    L.grim_export_engine.argtypes = [C.c_void_p]
    L.grim_destroy.argtypes = [C.c_void_p]
    L.grim_last_error.restype = C.c_char_p
    L.grim_last_error.argtypes = [C.c_void_p]
    L.grim_device_count.restype = C.c_int
    L.grim_graph_upload.restype = C.c_void_p
    L.grim_graph_upload.argtypes = [C.c_void_p, C.POINTER(GraphDesc)]
    L.grim_graph_free.argtypes = [C.c_void_p]
    L.grim_graph_device_bytes.restype = C.c_uint64
    L.grim_graph_device_bytes.argtypes = [C.c_void_p]
    L.grim_batch_upload.restype = C.c_void_p
    L.grim_batch_upload.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Params), C.POINTER(BatchDesc)]
    L.grim_batch_run.restype = C.c_int
    L.grim_batch_run.argtypes = [C.c_void_p]
    L.grim_batch_kernel_ms.restype = C.c_double
    L.grim_batch_kernel_ms.argtypes = [C.c_void_p, C.c_int]
    L.grim_batch_counters.restype = C.c_int
    L.grim_batch_counters.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.grim_batch_total_rows.restype = C.c_uint32
    L.grim_batch_total_rows.argtypes = [C.c_void_p]
    L.grim_batch_results.restype = C.c_int
    L.grim_batch_results.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.grim_batch_free.argtypes = [C.c_void_p]
    L.grim_batch_run_repeat.restype = C.c_int
    L.grim_batch_run_repeat.argtypes = [C.c_void_p, C.c_uint32]
    L.grim_batch_set_timing.restype = C.c_int
    L.grim_batch_set_timing.argtypes = [C.c_void_p, C.c_int]
    _lib = L
    return L


EXPORTS = [
    "grim_create", "grim_destroy", "grim_last_error", "grim_device_count", "grim_export_engine", "grim_graph_upload", "grim_graph_free",
    "grim_graph_device_bytes", "grim_batch_upload", "grim_batch_run", "grim_batch_kernel_ms", "grim_batch_counters",
    "grim_batch_total_rows", "grim_batch_results", "grim_batch_free", "grim_batch_set_timing", "grim_batch_run_repeat",
]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _per_slot(counts):
    """per-slot counts (n_alleles, n_groups), padded with 0 to MAXL -> the uint32[GRIM_MAXL] a create call takes"""
    return (C.c_uint32 * MAXL)(*([int(x) for x in counts] + [0] * (MAXL - len(counts))))


def _records(res, rows):
    """host records -> (res RESULT_DT[n], rows ROW_DT[m], the four C arguments res, n, rows, m); the caller keeps the arrays
    alive across the call"""
    res = np.ascontiguousarray(res, dtype=RESULT_DT)
    rows = np.ascontiguousarray(rows, dtype=ROW_DT)
    return res, rows, (_ptr(res) if res.size else None, res.shape[0], _ptr(rows) if rows.size else None, rows.shape[0])


class _Handle:
    """an object of the library behind `h`, freed once by the function named `_free`; `ctx` holds its error text"""

    _free = None
    h = None

    def _check(self, rc, name, code=True):
        if rc != 0:
            raise NativeError("%s failed%s: %s" % (name, " (%d)" % rc if code else "", self.ctx.error()))

    def close(self):
        if self.h:
            getattr(lib(), self._free)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context(_Handle):
    """One per GPU (grim_ctx)."""

    _free = "grim_destroy"

    def __init__(self, device=0):
        L = lib()
        self.device = device
        self.h = L.grim_create(device)
        if not self.h:
            raise NativeError("grim_create(%d) failed: %s" % (device, L.grim_last_error(None).decode()))

    def error(self):
        return lib().grim_last_error(self.h).decode()

    def export_engine(self):
        """SDMA engine bit of the result downloads (> 1), 0 = copy kernel, -1 = hipMemcpyAsync (grim_export_engine)"""
        return int(lib().grim_export_engine(self.h))


_contexts = {}


def default_context(device=None):
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0")) if os.environ.get("GRIM_DEVICE") is None else int(os.environ["GRIM_DEVICE"])
        n = lib().grim_device_count()
        if n > 0:
            device %= n
    if device not in _contexts:
        _contexts[device] = Context(device)
    return _contexts[device]


class DeviceGraph(_Handle):
    """Device-resident graph (grim_graph)."""

    _free = "grim_graph_free"

    def __init__(self, ctx, arrays):
        L = lib()
        self.ctx = ctx
        d = GraphDesc()
        self._keep = arrays  # host arrays must outlive the upload call only, kept for debugging
        d.n_nodes = arrays["n_nodes"]
        d.n_pops = arrays["n_pops"]
        d.n_loci = arrays["n_loci"]
        d.full_mask = arrays["full_mask"]
        for k in ("node_key", "node_mask", "freq", "a_start", "a_nbr", "b_conn", "b_start", "b_nbr", "lab_start", "lab_nodes"):
            setattr(d, k, _ptr(arrays[k]))
        d.n_a_nbr = arrays["a_nbr"].shape[0]
        d.n_conn = arrays["b_start"].shape[0] - 1
        d.n_b_nbr = arrays["b_nbr"].shape[0]
        d.label_order_bad = int(arrays.get("label_order_bad", 0))
        self.h = L.grim_graph_upload(ctx.h, C.byref(d))
        if not self.h:
            raise NativeError("grim_graph_upload failed: " + ctx.error())

    def device_bytes(self):
        return int(lib().grim_graph_device_bytes(self.h))

    # ---- EM on a fixed support (grim_graph_refresh*, include/grim_hip.h): the frequencies from M-step counts ----
    def refreshable(self):
        return bool(_refresh_lib().grim_graph_refreshable(self.h))

    def _refreshed(self, rc, name, st):
        self._check(rc, name)
        P = int(self._keep["n_pops"])
        return {"total": [float(x) for x in st.total[:P]], "delta": float(st.delta), "matched": int(st.matched),
                "zero_full": int(st.zero_full), "n_full": int(st.n_full), "kernel_ms": self.refresh_ms()}

    def refresh(self, acc):
        """new frequencies from the counts of an EmAccumulator, where its table lies -> the statistics (a dict); synchronous.
        The caller guarantees that no batch or stream of this graph is in flight."""
        st = RefreshStats()
        return self._refreshed(_refresh_lib().grim_graph_refresh(self.h, acc.h, C.byref(st)), "grim_graph_refresh", st)

    def refresh_records(self, keys, pops, counts):
        """the same from host arrays keys u64 / pops u32 / counts f64 in EmAccumulator.export's order"""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        pops = np.ascontiguousarray(pops, dtype=np.uint32)
        counts = np.ascontiguousarray(counts, dtype=np.float64)
        if not (keys.ndim == 1 and keys.shape == pops.shape == counts.shape):
            raise ValueError("keys, pops and counts must be one-dimensional and of one length")
        n = keys.shape[0]
        st = RefreshStats()
        rc = _refresh_lib().grim_graph_refresh_records(self.h, _ptr(keys) if n else None, _ptr(pops) if n else None,
                                                       _ptr(counts) if n else None, n, C.byref(st))
        return self._refreshed(rc, "grim_graph_refresh_records", st)

    def freq(self):
        """the frequencies as they lie on the device -> f64 [n_nodes][n_pops]"""
        out = np.zeros((int(self._keep["n_nodes"]), int(self._keep["n_pops"])), dtype=np.float64)
        self._check(_refresh_lib().grim_graph_freq(self.h, _ptr(out)), "grim_graph_freq")
        return out

    def refresh_ms(self):
        return float(_refresh_lib().grim_graph_refresh_ms(self.h))


EXPORTS += ["grim_graph_refresh", "grim_graph_refresh_records", "grim_graph_freq", "grim_graph_refresh_ms", "grim_graph_refreshable"]

REFRESH_BLOCK = 4096


class RefreshStats(C.Structure):
    _fields_ = [("total", C.c_double * MAXPOP), ("delta", C.c_double), ("matched", C.c_uint64), ("zero_full", C.c_uint64),
                ("n_full", C.c_uint64)]


_refresh_ready = False


def _refresh_lib():
    global _refresh_ready
    L = lib()
    if not _refresh_ready:
        L.grim_graph_refresh.restype = C.c_int
        L.grim_graph_refresh.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(RefreshStats)]
        L.grim_graph_refresh_records.restype = C.c_int
        L.grim_graph_refresh_records.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(RefreshStats)]
        L.grim_graph_freq.restype = C.c_int
        L.grim_graph_freq.argtypes = [C.c_void_p, C.c_void_p]
        L.grim_graph_refresh_ms.restype = C.c_double
        L.grim_graph_refresh_ms.argtypes = [C.c_void_p]
        L.grim_graph_refreshable.restype = C.c_int
        L.grim_graph_refreshable.argtypes = [C.c_void_p]
        _refresh_ready = True
    return L


class DeviceBatch(_Handle):
    """Subjects resident in HBM + result/scratch buffers (grim_batch)."""

    _free = "grim_batch_free"

    def __init__(self, ctx, dgraph, params, subjects, tokens, priors):
        L = lib()
        self.ctx = ctx
        self.n = int(subjects.shape[0])
        d = BatchDesc()
        tokens = np.ascontiguousarray(tokens, dtype=np.uint16)
        priors = np.ascontiguousarray(priors, dtype=np.float64)
        subjects = np.ascontiguousarray(subjects)
        d.n_subjects = self.n
        d.subjects = _ptr(subjects)
        d.tokens = _ptr(tokens)
        d.n_tokens = tokens.shape[0]
        d.priors = _ptr(priors)
        d.n_priors = priors.shape[0]
        self._keep = (subjects, tokens, priors)
        self.h = L.grim_batch_upload(ctx.h, dgraph.h, C.byref(params), C.byref(d))
        if not self.h:
            raise NativeError("grim_batch_upload failed: " + ctx.error())

    def run(self):
        self._check(lib().grim_batch_run(self.h), "grim_batch_run")

    def run_repeat(self, n):
        self._check(lib().grim_batch_run_repeat(self.h, int(n)), "grim_batch_run")

    def set_timing(self, on=True):
        """start/stop hipEvents around every kernel of a run (resets the accumulated means); see grim_batch_set_timing"""
        lib().grim_batch_set_timing(self.h, 1 if on else 0)

    def kernel_ms(self, which=MS_TOTAL):
        """device time of the last run in timing mode: which = one of MS_*, | MS_MEAN for the mean over the timed runs"""
        return float(lib().grim_batch_kernel_ms(self.h, which))

    def counters(self):
        out = (C.c_uint64 * 4)()
        lib().grim_batch_counters(self.h, out)
        return [int(x) for x in out]

    def results(self):
        L = lib()
        nrows = int(L.grim_batch_total_rows(self.h))
        res = np.zeros(self.n, dtype=RESULT_DT)
        rows = np.zeros(max(nrows, 1), dtype=ROW_DT)
        self._check(L.grim_batch_results(self.h, _ptr(res), _ptr(rows)), "grim_batch_results", code=False)
        return res, rows[:nrows]


# ---- M-step accumulator (grim_em_*): haplotype / population counts from the phased rows of finished batches ----
EXPORTS += [
    "grim_em_create", "grim_em_accumulate", "grim_em_accumulate_records", "grim_em_entries", "grim_em_export", "grim_em_spill_count",
    "grim_em_spill", "grim_em_stats", "grim_em_last_unsupported", "grim_em_kernel_ms", "grim_em_free",
    "grim_em_merge", "grim_em_merge_records", "grim_em_merge_ms",
]

SPILL_DT = np.dtype([("key", "<u8"), ("w", "<f8"), ("batch", "<u4"), ("subject", "<u4"), ("row", "<u4"), ("pop", "<u2"), ("side", "<u2")])
assert SPILL_DT.itemsize == 32

_em_ready = False


def _em_lib():
    global _em_ready
    L = lib()
    if not _em_ready:
        L.grim_em_create.restype = C.c_void_p
        L.grim_em_create.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint64]
        L.grim_em_accumulate.restype = C.c_int
        L.grim_em_accumulate.argtypes = [C.c_void_p, C.c_void_p]
        L.grim_em_accumulate_records.restype = C.c_int
        L.grim_em_accumulate_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]
        L.grim_em_entries.restype = C.c_uint64
        L.grim_em_entries.argtypes = [C.c_void_p]
        L.grim_em_export.restype = C.c_int
        L.grim_em_export.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.grim_em_spill_count.restype = C.c_uint64
        L.grim_em_spill_count.argtypes = [C.c_void_p]
        L.grim_em_spill.restype = C.c_int
        L.grim_em_spill.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        L.grim_em_stats.restype = C.c_int
        L.grim_em_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.grim_em_last_unsupported.restype = C.c_uint64
        L.grim_em_last_unsupported.argtypes = [C.c_void_p]
        L.grim_em_kernel_ms.restype = C.c_double
        L.grim_em_kernel_ms.argtypes = [C.c_void_p]
        L.grim_em_free.argtypes = [C.c_void_p]
        L.grim_em_merge.restype = C.c_int
        L.grim_em_merge.argtypes = [C.c_void_p, C.c_void_p]
        L.grim_em_merge_records.restype = C.c_int
        L.grim_em_merge_records.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.grim_em_merge_ms.restype = C.c_double
        L.grim_em_merge_ms.argtypes = [C.c_void_p]
        _em_ready = True
    return L


class EmAccumulator(_Handle):
    """grim_em: per-population haplotype counts summed on the device from the phased rows of finished batches, in input
    order and bit for bit independent of the batch cuts (include/grim_hip.h, the grim_em_* block)."""

    _free = "grim_em_free"

    def __init__(self, ctx, n_alleles, n_pops, first_capacity=1 << 20):
        L = _em_lib()
        self.ctx = ctx
        arr = _per_slot(n_alleles)
        self.h = L.grim_em_create(ctx.h, arr, int(n_pops), int(first_capacity))
        if not self.h:
            raise NativeError("grim_em_create failed: " + ctx.error())

    def accumulate(self, batch):
        """the counts of one DeviceBatch after its run(); synchronous"""
        self._check(_em_lib().grim_em_accumulate(self.h, batch.h), "grim_em_accumulate")

    def accumulate_records(self, res, rows):
        """host records (RESULT_DT[n], ROW_DT[m]) through the same kernels; the call counts as one batch"""
        res, rows, args = _records(res, rows)
        self._check(_em_lib().grim_em_accumulate_records(self.h, *args), "grim_em_accumulate_records")

    def entries(self):
        return int(_em_lib().grim_em_entries(self.h))

    def export(self):
        """-> (keys u64, pops u32, counts f64), one element per (haplotype, population) counter, in (key, population) order"""
        n = self.entries()
        keys, pops, counts = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.float64)
        if n:
            self._check(_em_lib().grim_em_export(self.h, _ptr(keys), _ptr(pops), _ptr(counts)), "grim_em_export", code=False)
        return keys, pops, counts

    def spill_count(self):
        return int(_em_lib().grim_em_spill_count(self.h))

    def spill(self, first=0, n=None):
        """spill records [first, first + n): contributions of haplotypes that hold an allele private to their subject"""
        if n is None:
            n = self.spill_count() - first
        out = np.zeros(max(int(n), 0), dtype=SPILL_DT)
        if n > 0 and _em_lib().grim_em_spill(self.h, int(first), int(n), _ptr(out)) != 0:
            raise NativeError("grim_em_spill: range outside the list")
        return out

    def stats(self):
        out = (C.c_uint64 * 4)()
        _em_lib().grim_em_stats(self.h, out)
        return {"subjects_used": int(out[0]), "skipped_plan_c": int(out[1]), "contributions": int(out[2]), "rehashes": int(out[3])}

    def last_unsupported(self):
        return int(_em_lib().grim_em_last_unsupported(self.h))

    def kernel_ms(self):
        return float(_em_lib().grim_em_kernel_ms(self.h))

    def merge(self, other):
        """every entry of `other`'s table added to this one's on the device (grim_em_merge); `other` is not changed, its spill
        list is not merged.  The caller merges in chunk order: count = (count + other's), one add per entry."""
        self._check(_em_lib().grim_em_merge(self.h, other.h), "grim_em_merge")

    def merge_records(self, keys, pops, counts):
        """the same add for an exported table: host arrays keys u64 / pops u32 / counts f64 in export()'s order"""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        pops = np.ascontiguousarray(pops, dtype=np.uint32)
        counts = np.ascontiguousarray(counts, dtype=np.float64)
        if not (keys.ndim == 1 and keys.shape == pops.shape == counts.shape):
            raise ValueError("keys, pops and counts must be one-dimensional and of one length")
        n = keys.shape[0]
        self._check(_em_lib().grim_em_merge_records(self.h, _ptr(keys) if n else None, _ptr(pops) if n else None,
                                                    _ptr(counts) if n else None, n), "grim_em_merge_records")

    def merge_ms(self):
        """device time of the last merge (kernel_ms keeps speaking of the last accumulate)"""
        return float(_em_lib().grim_em_merge_ms(self.h))


# ---- allele groups (grim_groups_*): the rows of the three consumers below mapped to a chosen resolution first ----
EXPORTS += [
    "grim_groups_create", "grim_groups_free", "grim_groups_watch_mask", "grim_groups_map_records", "grim_groups_kernel_ms",
    "grim_marginal_set_groups", "grim_match_set_groups", "grim_search_set_groups", "grim_marginal_flags",
]

GROUPS_PRIVATE = 1

_groups_ready = False


def _groups_lib():
    global _groups_ready
    L = lib()
    if not _groups_ready:
        L.grim_groups_create.restype = C.c_void_p
        L.grim_groups_create.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.grim_groups_free.argtypes = [C.c_void_p]
        L.grim_groups_watch_mask.restype = C.c_uint32
        L.grim_groups_watch_mask.argtypes = [C.c_void_p]
        L.grim_groups_map_records.restype = C.c_int
        L.grim_groups_map_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.grim_groups_kernel_ms.restype = C.c_double
        L.grim_groups_kernel_ms.argtypes = [C.c_void_p]
        for name in ("grim_marginal_set_groups", "grim_match_set_groups", "grim_search_set_groups", "grim_marginal_flags"):
            getattr(L, name).restype = C.c_int
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p]
        _groups_ready = True
    return L


class Groups(_Handle):
    """grim_groups: a group map on the device (include/grim_hip.h, the grim_groups_* block).  `table`: the slots' uint16 tables
    back to back, each of length n_alleles[s] + 1 (AlleleGroups.flat()); a map the library refuses raises NativeError with its
    text.  A consumer copies the tables when the map is attached, so the map may be closed right after."""

    _free = "grim_groups_free"

    def __init__(self, ctx, table, n_alleles, n_groups):
        L = _groups_lib()
        self.ctx = ctx
        na, ng = _per_slot(n_alleles), _per_slot(n_groups)
        table = np.ascontiguousarray(table, dtype=np.uint16)
        need = sum(min(x, 4095) + 1 for x in na)  # the library reads no table before it has checked the sizes
        if table.ndim != 1 or len(table) < need:
            raise ValueError("the table holds %d entries, the slots need %d" % (table.size, need))
        self.h = L.grim_groups_create(ctx.h, _ptr(table), na, ng)
        if not self.h:
            raise NativeError("grim_groups_create failed: " + ctx.error())

    @classmethod
    def of(cls, ctx, groups):
        """an AlleleGroups (grim.groups) on the device"""
        return cls(ctx, groups.flat(), groups.n_alleles, groups.n_groups)

    def watch_mask(self):
        return int(_groups_lib().grim_groups_watch_mask(self.h))

    def map_records(self, rows):
        """ROW_DT rows through gp_map_kernel -> the mapped rows"""
        rows = np.ascontiguousarray(rows, dtype=ROW_DT)
        out = np.zeros(max(len(rows), 1), dtype=ROW_DT)
        self._check(_groups_lib().grim_groups_map_records(self.h, _ptr(rows) if rows.size else None, len(rows), _ptr(out)),
                    "grim_groups_map_records")
        return out[:len(rows)]

    def kernel_ms(self):
        return float(_groups_lib().grim_groups_kernel_ms(self.h))


def _set_groups(obj, name, groups):
    obj._check(getattr(_groups_lib(), name)(obj.h, groups.h if groups is not None else None), name)


# ---- marginal genotype tables (grim_marginal_*): the UMUG rows of finished batches reduced to a subset of the loci ----
EXPORTS += [
    "grim_marginal_create", "grim_marginal_reduce", "grim_marginal_reduce_records", "grim_marginal_subjects",
    "grim_marginal_total_rows", "grim_marginal_results", "grim_marginal_stats", "grim_marginal_kernel_ms", "grim_marginal_free",
]

_marginal_ready = False


def _marginal_lib():
    global _marginal_ready
    L = lib()
    if not _marginal_ready:
        L.grim_marginal_create.restype = C.c_void_p
        L.grim_marginal_create.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        L.grim_marginal_reduce.restype = C.c_int
        L.grim_marginal_reduce.argtypes = [C.c_void_p, C.c_void_p]
        L.grim_marginal_reduce_records.restype = C.c_int
        L.grim_marginal_reduce_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]
        L.grim_marginal_subjects.restype = C.c_uint32
        L.grim_marginal_subjects.argtypes = [C.c_void_p]
        L.grim_marginal_total_rows.restype = C.c_uint32
        L.grim_marginal_total_rows.argtypes = [C.c_void_p]
        L.grim_marginal_results.restype = C.c_int
        L.grim_marginal_results.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.grim_marginal_stats.restype = C.c_int
        L.grim_marginal_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.grim_marginal_kernel_ms.restype = C.c_double
        L.grim_marginal_kernel_ms.argtypes = [C.c_void_p]
        L.grim_marginal_free.argtypes = [C.c_void_p]
        _marginal_ready = True
    return L


MARGINAL_STATS = ("subjects", "rows_in", "groups", "rows_out", "undefined")


class MarginalReducer(_Handle):
    """grim_marginal: the genotype rows of a finished batch (or of host records) grouped on the kept locus slots, summed in
    rank order and ranked again, per subject, on the device (include/grim_hip.h, the grim_marginal_* block).  results(),
    stats() and kernel_ms() speak of the last reduce."""

    _free = "grim_marginal_free"

    def __init__(self, ctx, keep_mask, max_rows):
        L = _marginal_lib()
        self.ctx = ctx
        self.h = L.grim_marginal_create(ctx.h, int(keep_mask), int(max_rows))
        if not self.h:
            raise NativeError("grim_marginal_create failed: " + ctx.error())

    def reduce(self, batch):
        """one DeviceBatch after its run(), where its rows lie; synchronous"""
        self._check(_marginal_lib().grim_marginal_reduce(self.h, batch.h), "grim_marginal_reduce")

    def reduce_records(self, res, rows):
        """host records (RESULT_DT[n], ROW_DT[m]) through the same kernels"""
        res, rows, args = _records(res, rows)
        self._check(_marginal_lib().grim_marginal_reduce_records(self.h, *args), "grim_marginal_reduce_records")

    def set_groups(self, groups):
        """a Groups map for every reduce that follows (None detaches); the last results are cleared"""
        _set_groups(self, "grim_marginal_set_groups", groups)

    def flags(self):
        """-> u8[subjects] of the last reduce: GROUPS_PRIVATE where the host has to fold the subject on text; zeros without a map"""
        out = np.zeros(max(self.subjects(), 1), dtype=np.uint8)
        self._check(_groups_lib().grim_marginal_flags(self.h, _ptr(out)), "grim_marginal_flags", code=False)
        return out[:self.subjects()]

    def subjects(self):
        return int(_marginal_lib().grim_marginal_subjects(self.h))

    def total_rows(self):
        return int(_marginal_lib().grim_marginal_total_rows(self.h))

    def results(self):
        """-> (res RESULT_DT[subjects], rows ROW_DT[total_rows]): subject i's rows are rows[res[i].row_off[0]:][:res[i].n_rows[0]]"""
        L = _marginal_lib()
        n, m = self.subjects(), self.total_rows()
        res = np.zeros(n, dtype=RESULT_DT)
        rows = np.zeros(max(m, 1), dtype=ROW_DT)
        self._check(L.grim_marginal_results(self.h, _ptr(res), _ptr(rows)), "grim_marginal_results", code=False)
        return res, rows[:m]

    def stats(self):
        out = (C.c_uint64 * 5)()
        _marginal_lib().grim_marginal_stats(self.h, out)
        return {k: int(v) for k, v in zip(MARGINAL_STATS, out)}

    def kernel_ms(self):
        return float(_marginal_lib().grim_marginal_kernel_ms(self.h))


# ---- match probabilities (grim_match_*): the UMUG rows of patients against those of finished batches of donors ----
EXPORTS += [
    "grim_match_create", "grim_match_set_patients", "grim_match_run", "grim_match_run_records", "grim_match_patients",
    "grim_match_donors", "grim_match_results", "grim_match_stats", "grim_match_kernel_ms", "grim_match_free",
    "grim_match_create_ex", "grim_match_results_graded", "grim_match_direction", "grim_match_graded",
]

MATCH_DT = np.dtype([("mm", "<f8", (2 * MAXL + 1,)), ("locus", "<f8", (MAXL,))])
assert MATCH_DT.itemsize == 128
MATCH_GRADE_DT = np.dtype([("mm", "<f8", (2 * MAXL + 1,)), ("grade", "<f8", (MAXL, 3))])  # grim_match_grade_rec
assert MATCH_GRADE_DT.itemsize == 208
MATCH_DIR_EITHER, MATCH_DIR_GVH, MATCH_DIR_HVG = 0, 1, 2
MATCH_STATS = ("patients_valid", "donors_valid", "patients_private", "donors_private", "undefined", "pairs", "row_pairs")
MATCH_VALID, MATCH_PRIVATE, MATCH_UNDEFINED = 1, 2, 4
MATCH_MAX_PAIRS = 1 << 24

_match_ready = False


def _match_lib():
    global _match_ready
    L = lib()
    if not _match_ready:
        L.grim_match_create.restype = C.c_void_p
        L.grim_match_create.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        L.grim_match_set_patients.restype = C.c_int
        L.grim_match_set_patients.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        L.grim_match_run.restype = C.c_int
        L.grim_match_run.argtypes = [C.c_void_p, C.c_void_p]
        L.grim_match_run_records.restype = C.c_int
        L.grim_match_run_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        L.grim_match_patients.restype = C.c_uint32
        L.grim_match_patients.argtypes = [C.c_void_p]
        L.grim_match_donors.restype = C.c_uint32
        L.grim_match_donors.argtypes = [C.c_void_p]
        L.grim_match_results.restype = C.c_int
        L.grim_match_results.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.grim_match_stats.restype = C.c_int
        L.grim_match_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.grim_match_kernel_ms.restype = C.c_double
        L.grim_match_kernel_ms.argtypes = [C.c_void_p]
        L.grim_match_free.argtypes = [C.c_void_p]
        L.grim_match_create_ex.restype = C.c_void_p
        L.grim_match_create_ex.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_int]
        L.grim_match_results_graded.restype = C.c_int
        L.grim_match_results_graded.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.grim_match_direction.restype = C.c_uint32
        L.grim_match_direction.argtypes = [C.c_void_p]
        L.grim_match_graded.restype = C.c_int
        L.grim_match_graded.argtypes = [C.c_void_p]
        _match_ready = True
    return L


class Matcher(_Handle):
    """grim_match: for every (patient, donor) pair the probabilities of 0, 1, 2, ... mismatching alleles over the kept locus
    slots and the per-locus match probabilities, on the device (include/grim_hip.h, the grim_match_* block).  The patients
    stay set across runs; results(), stats() and kernel_ms() speak of the last run.  `direction`: MATCH_DIR_EITHER, _GVH or
    _HVG, the per-locus mismatch function; `graded`: the records are MATCH_GRADE_DT and come from results_graded()."""

    _free = "grim_match_free"

    def __init__(self, ctx, keep_mask, n_alleles, direction=0, graded=False):
        L = _match_lib()
        self.ctx = ctx
        arr = _per_slot(n_alleles)
        direction = int(direction)
        if not 0 <= direction < 1 << 32:
            raise ValueError("direction out of range")
        self.h = L.grim_match_create_ex(ctx.h, int(keep_mask), arr, direction, 1 if graded else 0)
        if not self.h:
            raise NativeError("grim_match_create failed: " + ctx.error())

    def direction(self):
        return int(_match_lib().grim_match_direction(self.h))

    def graded(self):
        return bool(_match_lib().grim_match_graded(self.h))

    def set_groups(self, groups):
        """a Groups map for everything that follows (None detaches); drops the patients and the last results"""
        _set_groups(self, "grim_match_set_groups", groups)

    def set_patients(self, res, rows):
        """host records (RESULT_DT[n], ROW_DT[m]) as the patients of every run that follows"""
        res, rows, args = _records(res, rows)
        self._check(_match_lib().grim_match_set_patients(self.h, *args), "grim_match_set_patients")

    def run(self, batch):
        """one DeviceBatch after its run() as donors, where its rows lie; synchronous"""
        self._check(_match_lib().grim_match_run(self.h, batch.h), "grim_match_run")

    def run_records(self, res, rows):
        """host records as donors, through the same kernels"""
        res, rows, args = _records(res, rows)
        self._check(_match_lib().grim_match_run_records(self.h, *args), "grim_match_run_records")

    def patients(self):
        return int(_match_lib().grim_match_patients(self.h))

    def donors(self):
        return int(_match_lib().grim_match_donors(self.h))

    def _results(self, name, dtype):
        n_p, n_d = self.patients(), self.donors()
        out = np.zeros((n_p, n_d), dtype=dtype)
        pf, df = np.zeros(n_p, dtype=np.uint8), np.zeros(n_d, dtype=np.uint8)
        self._check(getattr(_match_lib(), name)(self.h, _ptr(out) if out.size else None, _ptr(pf) if n_p else None,
                                                _ptr(df) if n_d else None), name, code=False)
        return out, pf, df

    def results(self):
        """-> (records MATCH_DT[patients][donors], patient flags u8[patients], donor flags u8[donors])"""
        return self._results("grim_match_results", MATCH_DT)

    def results_graded(self):
        """of a graded matcher -> (records MATCH_GRADE_DT[patients][donors], patient flags, donor flags)"""
        return self._results("grim_match_results_graded", MATCH_GRADE_DT)

    def stats(self):
        out = (C.c_uint64 * 8)()
        _match_lib().grim_match_stats(self.h, out)
        return {k: int(v) for k, v in zip(MATCH_STATS, out)}

    def kernel_ms(self):
        return float(_match_lib().grim_match_kernel_ms(self.h))


# ---- donor search (grim_search_*): each patient's best top_n donors over any number of runs, selected on the device ----
EXPORTS += [
    "grim_search_create", "grim_search_set_patients", "grim_search_reset", "grim_search_run", "grim_search_run_records",
    "grim_search_results", "grim_search_flags", "grim_search_patients", "grim_search_donors", "grim_search_top_n",
    "grim_search_stats", "grim_search_kernel_ms", "grim_search_select_ms", "grim_search_free", "grim_search_merge_hits",
    "grim_search_create_ex",
]

SEARCH_DT = np.dtype([("donor", "<u4"), ("reserved", "<u4"), ("rec", MATCH_DT)])
assert SEARCH_DT.itemsize == 136
SEARCH_MAX_N = 256
SEARCH_TILE = 2048  # entries a workgroup sorts at a time (GRIM_SEARCH_TILE lowers it, for tests)
SEARCH_NO_DONOR = 0xFFFFFFFF
SEARCH_MERGE_MAX_LISTS = 4096
SEARCH_STATS = MATCH_STATS + ("candidates",)

_search_ready = False


def _search_lib():
    global _search_ready
    L = lib()
    if not _search_ready:
        L.grim_search_create.restype = C.c_void_p
        L.grim_search_create.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_double]
        L.grim_search_set_patients.restype = C.c_int
        L.grim_search_set_patients.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        L.grim_search_reset.restype = C.c_int
        L.grim_search_reset.argtypes = [C.c_void_p]
        L.grim_search_run.restype = C.c_int
        L.grim_search_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.grim_search_run_records.restype = C.c_int
        L.grim_search_run_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
        L.grim_search_results.restype = C.c_int
        L.grim_search_results.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.grim_search_flags.restype = C.c_int
        L.grim_search_flags.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        for name in ("grim_search_patients", "grim_search_donors", "grim_search_top_n"):
            getattr(L, name).restype = C.c_uint32
            getattr(L, name).argtypes = [C.c_void_p]
        L.grim_search_stats.restype = C.c_int
        L.grim_search_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        for name in ("grim_search_kernel_ms", "grim_search_select_ms"):
            getattr(L, name).restype = C.c_double
            getattr(L, name).argtypes = [C.c_void_p]
        L.grim_search_free.argtypes = [C.c_void_p]
        L.grim_search_merge_hits.restype = C.c_int
        L.grim_search_merge_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        L.grim_search_create_ex.restype = C.c_void_p
        L.grim_search_create_ex.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_double, C.c_uint32]
        _search_ready = True
    return L


class Searcher(_Handle):
    """grim_search: every patient's first top_n donors by match probability (mm[0] down, then mm[1] down, then id up) among the
    pairs with mm[0] >= min_p0, over all runs since the patients were set or the search was reset, selected on the device
    (include/grim_hip.h, the grim_search_* block).  results() and stats() speak of all runs so far; flags(), donors(),
    kernel_ms() and select_ms() of the last one.  `direction`: as Matcher; order and threshold are on the directed mm[0], mm[1]."""

    _free = "grim_search_free"

    def __init__(self, ctx, keep_mask, n_alleles, top_n, min_p0=0.0, direction=0):
        L = _search_lib()
        self.ctx = ctx
        arr = _per_slot(n_alleles)
        top_n = int(top_n)
        if not 0 <= top_n < 1 << 32:
            raise ValueError("top_n out of range")
        direction = int(direction)
        if not 0 <= direction < 1 << 32:
            raise ValueError("direction out of range")
        self.h = L.grim_search_create_ex(ctx.h, int(keep_mask), arr, top_n, float(min_p0), direction)
        if not self.h:
            raise NativeError("grim_search_create failed: " + ctx.error())

    @staticmethod
    def _ids(ids, n):
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        if ids.shape != (n,):
            raise ValueError("%d donors but ids of shape %r" % (n, ids.shape))
        return ids

    def set_groups(self, groups):
        """a Groups map for everything that follows (None detaches); drops the patients, empties the hit lists and the sums"""
        _set_groups(self, "grim_search_set_groups", groups)

    def set_patients(self, res, rows):
        """host records (RESULT_DT[n], ROW_DT[m]) as the patients of every run that follows; empties the hit lists"""
        res, rows, args = _records(res, rows)
        self._check(_search_lib().grim_search_set_patients(self.h, *args), "grim_search_set_patients")

    def reset(self):
        """empties the hit lists and the summed statistics; the patients stay"""
        self._check(_search_lib().grim_search_reset(self.h), "grim_search_reset", code=False)

    def run(self, batch, ids):
        """one DeviceBatch after its run() as donors, where its rows lie; ids: one uint32 per subject of the batch"""
        ids = self._ids(ids, batch.n)
        self._check(_search_lib().grim_search_run(self.h, batch.h, _ptr(ids) if ids.size else None), "grim_search_run")

    def run_records(self, res, rows, ids):
        """host records as donors, through the same kernels"""
        res, rows, args = _records(res, rows)
        ids = self._ids(ids, res.shape[0])
        self._check(_search_lib().grim_search_run_records(self.h, *args, _ptr(ids) if ids.size else None), "grim_search_run_records")

    def merge(self, hits, n_hits):
        """hit lists that another search produced into the running lists (grim_search_merge_hits): hits SEARCH_DT[L][P][top_n]
        or [P][top_n], n_hits u32[L][P] or [P], P and top_n this search's; results() speaks of them from now on, stats(),
        flags() and donors() do not; kernel_ms() and select_ms() become the merge's device time"""
        hits = np.ascontiguousarray(hits, dtype=SEARCH_DT)
        n_hits = np.ascontiguousarray(n_hits, dtype=np.uint32)
        if hits.ndim == 2:
            hits, n_hits = hits[None], n_hits[None]
        if hits.ndim != 3 or hits.shape[2] != self.top_n() or n_hits.shape != hits.shape[:2]:
            raise ValueError("hits of shape %r with n_hits of shape %r: not [lists][patients][top_n = %d] with one count a list"
                             % (hits.shape, n_hits.shape, self.top_n()))
        self._check(_search_lib().grim_search_merge_hits(self.h, _ptr(hits) if hits.size else None, _ptr(n_hits) if n_hits.size else None,
                                                         hits.shape[1], hits.shape[0]), "grim_search_merge_hits")

    def patients(self):
        return int(_search_lib().grim_search_patients(self.h))

    def donors(self):
        return int(_search_lib().grim_search_donors(self.h))

    def top_n(self):
        return int(_search_lib().grim_search_top_n(self.h))

    def results(self):
        """-> (hits SEARCH_DT[patients][top_n], n_hits u32[patients])"""
        n_p, top_n = self.patients(), self.top_n()
        hits = np.zeros((n_p, top_n), dtype=SEARCH_DT)
        n_hits = np.zeros(n_p, dtype=np.uint32)
        self._check(_search_lib().grim_search_results(self.h, _ptr(hits) if hits.size else None, _ptr(n_hits) if n_p else None),
                    "grim_search_results", code=False)
        return hits, n_hits

    def flags(self):
        """-> (patient flags u8[patients], donor flags u8[donors of the last run])"""
        n_p, n_d = self.patients(), self.donors()
        pf, df = np.zeros(n_p, dtype=np.uint8), np.zeros(n_d, dtype=np.uint8)
        self._check(_search_lib().grim_search_flags(self.h, _ptr(pf) if n_p else None, _ptr(df) if n_d else None), "grim_search_flags",
                    code=False)
        return pf, df

    def stats(self):
        out = (C.c_uint64 * 8)()
        _search_lib().grim_search_stats(self.h, out)
        return {k: int(v) for k, v in zip(SEARCH_STATS, out)}

    def kernel_ms(self):
        return float(_search_lib().grim_search_kernel_ms(self.h))

    def select_ms(self):
        return float(_search_lib().grim_search_select_ms(self.h))


# ======================================================================================================
# host-side helpers of the library (C++: allele dictionary, tokenizer, formatter) -- no GPU needed
# ======================================================================================================
K_DEVICE, K_PROBLEM_ID, K_PROBLEM_RAW, K_MISS_NO_DEVICE, K_UNSUPPORTED, K_UNSUPPORTED_GL = 0, 1, 2, 3, 4, 5

EXPORTS += [
    "grim_dict_create", "grim_dict_free", "grim_dict_set_locus", "grim_dict_intern", "grim_dict_find", "grim_dict_name",
    "grim_dict_count", "grim_tokenize", "grim_parsed_free", "grim_parsed_lines", "grim_parsed_subjects",
    "grim_parsed_subject_array", "grim_parsed_tokens", "grim_parsed_kinds", "grim_parsed_dev_index",
    "grim_parsed_n_races", "grim_parsed_race", "grim_parsed_id", "grim_parsed_set_kind", "grim_parsed_set_flags", "grim_format", "grim_text_get", "grim_text_free",
    "grim_format_double", "grim_hostgraph_load_csv", "grim_hostgraph_desc", "grim_hostgraph_free", "grim_graphgen_csv", "grim_hostgraph_from_hpf",
    "grim_parsed_allele", "grim_prior_matrix", "grim_stream_open", "grim_stream_write", "grim_stream_write_borrowed", "grim_stream_write_file", "grim_stream_finish",
    "grim_stream_error", "grim_stream_text", "grim_stream_get_stats", "grim_stream_n_unsupported", "grim_stream_unsupported",
    "grim_stream_next_records", "grim_stream_release_records", "grim_stream_free", "grim_stream_write_text",
    "grim_stream_segment", "grim_stream_n_segments", "grim_stream_segment_end", "grim_stream_segment_wait", "grim_stream_segment_place", "grim_default_threads", "grim_chunk_offsets", "grim_free",
    "grim_stream_devtok_lines", "grim_tokname_hash",
]


class PriorSpec(C.Structure):
    _fields_ = [("alpha", C.c_double), ("eta", C.c_double), ("beta", C.c_double), ("gamma", C.c_double), ("delta", C.c_double),
                ("unk_mr", C.c_uint8), ("count_by_prob", C.POINTER(C.c_double))]


class StreamOpts(C.Structure):
    _fields_ = [("chunk_lines", C.c_uint32), ("depth", C.c_uint32), ("n_threads", C.c_int32), ("line_offset", C.c_uint64),
                ("rows_per_chunk", C.c_uint64), ("want_text", C.c_uint8), ("want_log", C.c_uint8), ("want_records", C.c_uint8),
                ("timing", C.c_uint8), ("rows_exact", C.c_uint8), ("placed", C.c_uint8), ("out_path", C.c_char_p * 6), ("mask_ids", C.c_char_p), ("mask_fixed", C.c_void_p),
                ("n_masks", C.c_uint32)]


class StreamStats(C.Structure):
    _fields_ = [("lines", C.c_uint64), ("subjects", C.c_uint64), ("chunks", C.c_uint64), ("reruns", C.c_uint64),
                ("unsupported", C.c_uint64), ("wall_s", C.c_double), ("tokenize_cpu_s", C.c_double), ("format_cpu_s", C.c_double),
                ("write_cpu_s", C.c_double), ("device_s", C.c_double), ("kernel_ms", C.c_double * 7), ("counters", C.c_uint64 * 4),
                ("text_bytes", C.c_uint64 * 7), ("bytes_h2d", C.c_uint64), ("bytes_d2h", C.c_uint64)]


class StreamRecords(C.Structure):
    _fields_ = [("first_line", C.c_uint64), ("n_lines", C.c_uint32), ("kinds", C.c_void_p), ("res", C.c_void_p),
                ("rows", C.c_void_p), ("chunk", C.c_void_p)]


_host_ready = False


def host_lib():
    global _host_ready
    L = lib()
    if _host_ready:
        return L
    L.grim_dict_create.restype = C.c_void_p
    L.grim_dict_create.argtypes = [C.c_uint32]
    L.grim_dict_free.argtypes = [C.c_void_p]
    L.grim_dict_set_locus.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p]
    L.grim_dict_intern.restype = C.c_int32
    L.grim_dict_intern.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p]
    L.grim_dict_find.restype = C.c_int32
    L.grim_dict_find.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p]
    L.grim_dict_name.restype = C.c_char_p
    L.grim_dict_name.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    L.grim_dict_count.restype = C.c_uint32
    L.grim_dict_count.argtypes = [C.c_void_p, C.c_uint32]
    L.grim_tokenize.restype = C.c_void_p
    L.grim_tokenize.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_int, C.c_int]
    L.grim_parsed_free.argtypes = [C.c_void_p]
    L.grim_parsed_lines.restype = C.c_uint32
    L.grim_parsed_lines.argtypes = [C.c_void_p]
    L.grim_parsed_subjects.restype = C.c_uint32
    L.grim_parsed_subjects.argtypes = [C.c_void_p]
    L.grim_parsed_subject_array.restype = C.c_void_p
    L.grim_parsed_subject_array.argtypes = [C.c_void_p]
    L.grim_parsed_tokens.restype = C.c_void_p
    L.grim_parsed_tokens.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.grim_parsed_kinds.restype = C.c_void_p
    L.grim_parsed_kinds.argtypes = [C.c_void_p]
    L.grim_parsed_dev_index.restype = C.c_void_p
    L.grim_parsed_dev_index.argtypes = [C.c_void_p]
    L.grim_parsed_n_races.restype = C.c_uint32
    L.grim_parsed_n_races.argtypes = [C.c_void_p]
    L.grim_parsed_race.restype = C.c_char_p
    L.grim_parsed_race.argtypes = [C.c_void_p, C.c_uint32, C.c_int]
    L.grim_parsed_id.restype = C.c_void_p
    L.grim_parsed_id.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.grim_parsed_set_kind.argtypes = [C.c_void_p, C.c_uint32, C.c_uint8]
    L.grim_parsed_set_flags.argtypes = [C.c_void_p, C.c_uint32, C.c_uint8]
    L.grim_format.restype = C.c_void_p
    L.grim_format.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Params), C.POINTER(C.c_char_p), C.c_uint32, C.c_void_p,
                              C.c_void_p, C.c_uint64, C.c_void_p, C.c_int]
    L.grim_text_get.restype = C.c_void_p
    L.grim_text_get.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
    L.grim_text_free.argtypes = [C.c_void_p]
    L.grim_format_double.restype = C.c_int
    L.grim_format_double.argtypes = [C.c_double, C.c_char_p, C.c_int]
    L.grim_hostgraph_load_csv.restype = C.c_void_p
    L.grim_hostgraph_load_csv.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint64]
    L.grim_hostgraph_desc.restype = C.c_int
    L.grim_hostgraph_desc.argtypes = [C.c_void_p, C.POINTER(GraphDesc)]
    L.grim_hostgraph_free.argtypes = [C.c_void_p]
    L.grim_graphgen_csv.restype = C.c_int
    L.grim_graphgen_csv.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_char_p),
                                    C.POINTER(C.c_uint32), C.c_uint32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p,
                                    C.c_char_p, C.c_uint64]
    L.grim_hostgraph_from_hpf.restype = C.c_void_p
    L.grim_hostgraph_from_hpf.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.c_uint32,
                                          C.POINTER(C.c_char_p), C.POINTER(C.c_uint32), C.c_uint32, C.c_char_p, C.c_char_p, C.c_char_p,
                                          C.c_char_p, C.c_char_p, C.c_uint64]
    L.grim_parsed_allele.restype = C.c_void_p
    L.grim_parsed_allele.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    L.grim_prior_matrix.restype = C.c_int
    L.grim_prior_matrix.argtypes = [C.POINTER(PriorSpec), C.POINTER(C.c_char_p), C.c_uint32, C.c_char_p, C.c_char_p, C.c_void_p]
    L.grim_stream_open.restype = C.c_void_p
    L.grim_stream_open.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Params), C.POINTER(PriorSpec), C.POINTER(C.c_char_p),
                                   C.c_uint32, C.POINTER(StreamOpts)]
    L.grim_stream_write.restype = C.c_int
    L.grim_stream_write.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64]
    L.grim_stream_write_borrowed.restype = C.c_int
    L.grim_stream_write_borrowed.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64]
    L.grim_stream_write_file.restype = C.c_int
    L.grim_stream_write_file.argtypes = [C.c_void_p, C.c_char_p]
    L.grim_stream_finish.restype = C.c_int
    L.grim_stream_finish.argtypes = [C.c_void_p]
    L.grim_stream_error.restype = C.c_char_p
    L.grim_stream_error.argtypes = [C.c_void_p]
    L.grim_stream_text.restype = C.c_void_p
    L.grim_stream_text.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
    L.grim_stream_get_stats.restype = C.c_int
    L.grim_stream_get_stats.argtypes = [C.c_void_p, C.POINTER(StreamStats)]
    L.grim_stream_n_unsupported.restype = C.c_uint64
    L.grim_stream_n_unsupported.argtypes = [C.c_void_p]
    L.grim_stream_unsupported.restype = C.c_int
    L.grim_stream_unsupported.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_void_p),
                                          C.POINTER(C.c_uint32)]
    L.grim_stream_next_records.restype = C.c_int
    L.grim_stream_next_records.argtypes = [C.c_void_p, C.POINTER(StreamRecords)]
    L.grim_stream_release_records.restype = C.c_int
    L.grim_stream_release_records.argtypes = [C.c_void_p, C.POINTER(StreamRecords)]
    L.grim_stream_free.argtypes = [C.c_void_p]
    L.grim_stream_write_text.restype = C.c_int
    L.grim_stream_write_text.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64]
    L.grim_stream_segment.restype = C.c_int
    L.grim_stream_segment.argtypes = [C.c_void_p, C.c_uint64]
    L.grim_stream_n_segments.restype = C.c_uint32
    L.grim_stream_n_segments.argtypes = [C.c_void_p]
    L.grim_stream_segment_end.restype = C.c_int
    L.grim_stream_segment_end.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]
    L.grim_stream_segment_wait.restype = C.c_int
    L.grim_stream_segment_wait.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]
    L.grim_stream_segment_place.restype = C.c_int
    L.grim_stream_segment_place.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]
    L.grim_stream_devtok_lines.restype = C.c_int
    L.grim_stream_devtok_lines.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.grim_tokname_hash.restype = C.c_uint32
    L.grim_tokname_hash.argtypes = [C.c_char_p, C.c_uint32]
    L.grim_default_threads.restype = C.c_uint32
    L.grim_chunk_offsets.restype = C.c_int64
    L.grim_chunk_offsets.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.POINTER(C.c_uint64))]
    L.grim_free.argtypes = [C.c_void_p]
    _host_ready = True
    return L


def tokname_hash(name):
    """grim_tokname_hash of an allele name (bytes or str, at most 24 bytes)"""
    b = name.encode() if isinstance(name, str) else bytes(name)
    return int(host_lib().grim_tokname_hash(b, len(b)))


def host_threads():
    n = int(os.environ.get("GRIM_HOST_THREADS", "0"))
    if n <= 0:
        n = min(16, os.cpu_count() or 1)
    return n


class AlleleDict:
    """grim_dict: the one allele dictionary shared by the graph loader, the tokenizer and the formatter."""

    def __init__(self, slot_locus):
        L = host_lib()
        self.n = len(slot_locus)
        self.h = L.grim_dict_create(self.n)
        if not self.h:
            raise NativeError("grim_dict_create failed")
        for s, name in enumerate(slot_locus):
            L.grim_dict_set_locus(self.h, s, name.encode())
        self._cache = [dict() for _ in slot_locus]

    def intern(self, slot, allele):
        i = self._cache[slot].get(allele)
        if i is None:
            i = host_lib().grim_dict_intern(self.h, slot, allele.encode())
            if i < 0:
                raise OverflowError("more than %d alleles at locus slot %d" % ((1 << ABITS) - 2, slot))
            self._cache[slot][allele] = i
        return i

    def name(self, slot, idx):
        s = host_lib().grim_dict_name(self.h, slot, idx)
        return None if s is None else s.decode()

    def count(self, slot):
        return int(host_lib().grim_dict_count(self.h, slot))

    def __del__(self):
        try:
            if self.h:
                host_lib().grim_dict_free(self.h)
                self.h = None
        except Exception:
            pass


class Parsed(_Handle):
    """grim_parsed: a block of input lines tokenised by the library."""

    _free = "grim_parsed_free"

    def __init__(self, adict, text_bytes, planb):
        L = host_lib()
        self.h = L.grim_tokenize(adict.h, text_bytes, len(text_bytes), 1 if planb else 0, host_threads())
        if not self.h:
            raise NativeError("grim_tokenize failed")
        self.n_lines = int(L.grim_parsed_lines(self.h))
        self.n_subjects = int(L.grim_parsed_subjects(self.h))

    def _array(self, ptr, dtype, n):
        if n == 0:
            return np.zeros(0, dtype=dtype)
        buf = (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr)
        return np.frombuffer(buf, dtype=dtype, count=n).copy()

    def subjects(self):
        return self._array(host_lib().grim_parsed_subject_array(self.h), SUBJECT_DT, self.n_subjects)

    def tokens(self):
        n = C.c_uint64(0)
        ptr = host_lib().grim_parsed_tokens(self.h, C.byref(n))
        return self._array(ptr, np.uint16, int(n.value))

    def kinds(self):
        return self._array(host_lib().grim_parsed_kinds(self.h), np.uint8, self.n_lines)

    def dev_index(self):
        return self._array(host_lib().grim_parsed_dev_index(self.h), np.int32, self.n_lines)

    def races(self):
        L = host_lib()
        return [(L.grim_parsed_race(self.h, i, 0).decode(), L.grim_parsed_race(self.h, i, 1).decode())
                for i in range(int(L.grim_parsed_n_races(self.h)))]

    def set_kind(self, line, kind):
        host_lib().grim_parsed_set_kind(self.h, line, kind)

    def set_flags(self, line, flags):
        host_lib().grim_parsed_set_flags(self.h, line, flags)

    def subject_id(self, line):
        n = C.c_uint32(0)
        ptr = host_lib().grim_parsed_id(self.h, line, C.byref(n))
        return C.string_at(ptr, n.value).decode() if ptr else None

    def allele(self, line, slot, idx):
        """text of allele `idx` at locus slot `slot` as line `line` uses it (dictionary allele or the line's own)"""
        n = C.c_uint32(0)
        ptr = host_lib().grim_parsed_allele(self.h, line, slot, idx, C.byref(n))
        return C.string_at(ptr, n.value).decode() if ptr else None

    def format(self, adict, params, pops, res, rows, line_offset=0, skip=None, as_bytes=False):
        L = host_lib()
        names = (C.c_char_p * len(pops))(*[p.encode() for p in pops])
        res = np.ascontiguousarray(res)
        rows = np.ascontiguousarray(rows)
        skip_p = None
        if skip is not None:
            skip = np.ascontiguousarray(skip, dtype=np.uint8)
            skip_p = _ptr(skip)
        t = L.grim_format(adict.h, self.h, C.byref(params), names, len(pops), _ptr(res) if res.size else None,
                          _ptr(rows) if rows.size else None, line_offset, skip_p, host_threads())
        if not t:
            raise NativeError("grim_format failed")
        out = {}
        for k, key in enumerate(("umug", "umug_pops", "pmug", "pmug_pops", "miss", "problem")):
            n = C.c_uint64(0)
            ptr = L.grim_text_get(t, k, C.byref(n))
            if as_bytes:
                out[key] = C.string_at(ptr, n.value) if n.value else b""
            else:
                out[key] = C.string_at(ptr, n.value).decode() if n.value else ""
        L.grim_text_free(t)
        return out


def chunk_offsets(path, chunk_lines):
    """grim_chunk_offsets: byte offsets of every chunk_lines-th line start of the file, the file size last"""
    L = host_lib()
    out = C.POINTER(C.c_uint64)()
    n = L.grim_chunk_offsets(os.fsencode(path), int(chunk_lines), C.byref(out))
    if n < 0:
        raise OSError("grim_chunk_offsets(%s) failed" % path)
    try:
        return [int(out[i]) for i in range(n)]
    finally:
        L.grim_free(out)


def format_double(x):
    buf = C.create_string_buffer(48)
    n = host_lib().grim_format_double(float(x), buf, 48)
    return buf.value[:n].decode()


def load_graph_csv(adict, full_loci, nodes_csv, top_links_csv, edges_csv):
    """grim_hostgraph_load_csv: the three graph CSVs -> dict of numpy arrays (same keys as the Python loader
    builds; the arrays are copies, the C object is freed before returning)."""
    L = host_lib()
    err = C.create_string_buffer(512)
    h = L.grim_hostgraph_load_csv(adict.h, full_loci.encode(), os.fsencode(nodes_csv), os.fsencode(top_links_csv),
                                  os.fsencode(edges_csv), err, len(err))
    return _hostgraph_arrays(h, err)


def _hostgraph_arrays(h, err):
    """a grim_hostgraph handle -> dict of numpy arrays (copies); frees the handle"""
    L = host_lib()
    if not h:
        msg = err.value.decode()
        if msg.startswith("graph: the highest-numbered vertex"):
            raise IndexError(msg)
        raise ValueError(msg)
    try:
        d = GraphDesc()
        L.grim_hostgraph_desc(h, C.byref(d))

        def arr(ptr, dtype, n):
            if n == 0:
                return np.zeros(0, dtype=dtype)
            buf = (C.c_char * (int(n) * np.dtype(dtype).itemsize)).from_address(ptr)
            return np.frombuffer(buf, dtype=dtype, count=int(n)).copy()

        V, P = int(d.n_nodes), int(d.n_pops)
        return {
            "n_nodes": V, "n_pops": P, "n_loci": int(d.n_loci), "full_mask": int(d.full_mask),
            "node_key": arr(d.node_key, np.uint64, V), "node_mask": arr(d.node_mask, np.uint8, V),
            "freq": arr(d.freq, np.float64, V * P).reshape(V, P),
            "a_start": arr(d.a_start, np.uint32, V + 1), "a_nbr": arr(d.a_nbr, np.uint32, d.n_a_nbr),
            "b_conn": arr(d.b_conn, np.uint32, V * MAXL), "b_start": arr(d.b_start, np.uint32, int(d.n_conn) + 1),
            "b_nbr": arr(d.b_nbr, np.uint32, d.n_b_nbr),
            "lab_start": arr(d.lab_start, np.uint32, (1 << MAXL) + 1), "lab_nodes": arr(d.lab_nodes, np.uint32, V),
        }
    finally:
        L.grim_hostgraph_free(h)


def graphgen_csv(hpf_csv, pops, cutoffs, loci_map, nodes_csv, edges_csv, top_links_csv, info_csv):
    """grim_graphgen_csv: hpf.csv -> nodes.csv, edges.csv, top_links.csv, info_node.csv."""
    L = host_lib()
    err = C.create_string_buffer(512)
    pop_arr = (C.c_char_p * len(pops))(*[p.encode() for p in pops])
    cut_arr = (C.c_double * len(pops))(*[float(c) for c in cutoffs])
    names = list(loci_map.keys())
    name_arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
    idx_arr = (C.c_uint32 * len(names))(*[int(loci_map[n]) for n in names])
    rc = L.grim_graphgen_csv(os.fsencode(hpf_csv), pop_arr, cut_arr, len(pops), name_arr, idx_arr, len(names),
                             os.fsencode(nodes_csv), os.fsencode(edges_csv), os.fsencode(top_links_csv), os.fsencode(info_csv),
                             err, len(err))
    if rc != 0:
        raise ValueError(err.value.decode())


def graph_from_hpf(adict, full_loci, hpf_csv, pops, cutoffs, loci_map, csv_paths=None):
    """grim_hostgraph_from_hpf: hpf.csv -> the loader's arrays, generator and loader back to back in memory.
    csv_paths: optional (nodes, edges, top_links, info_node) paths to ALSO write the four CSVs (None entries are skipped)."""
    L = host_lib()
    err = C.create_string_buffer(512)
    pop_arr = (C.c_char_p * len(pops))(*[p.encode() for p in pops])
    cut_arr = (C.c_double * len(pops))(*[float(c) for c in cutoffs])
    names = list(loci_map.keys())
    name_arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
    idx_arr = (C.c_uint32 * len(names))(*[int(loci_map[n]) for n in names])
    paths = [os.fsencode(p) if p else None for p in (csv_paths or (None, None, None, None))]
    h = L.grim_hostgraph_from_hpf(adict.h, full_loci.encode(), os.fsencode(hpf_csv), pop_arr, cut_arr, len(pops), name_arr, idx_arr,
                                  len(names), paths[0], paths[1], paths[2], paths[3], err, len(err))
    return _hostgraph_arrays(h, err)


def prior_spec(priority, unk_priors, count_by_prob=None):
    """grim_prior_spec from the conf's "priority" dict, UNK_priors and the population counts (kept alive by the caller)"""
    ps = PriorSpec()
    ps.alpha, ps.eta, ps.beta, ps.gamma, ps.delta = (float(priority[k]) for k in ("alpha", "eta", "beta", "gamma", "delta"))
    ps.unk_mr = 1 if unk_priors == "MR" else 0
    keep = None
    if count_by_prob is not None:
        keep = np.ascontiguousarray(count_by_prob, dtype=np.float64)
        ps.count_by_prob = keep.ctypes.data_as(C.POINTER(C.c_double))
    return ps, keep


def prior_matrix(ps, pops, race1, race2):
    """calc_priority_matrix in the library (grim_prior_matrix) -> P x P float64"""
    names = (C.c_char_p * len(pops))(*[p.encode() for p in pops])
    out = np.zeros((len(pops), len(pops)), dtype=np.float64)
    rc = host_lib().grim_prior_matrix(C.byref(ps), names, len(pops), (race1 or "").encode(), (race2 or "").encode(), _ptr(out))
    if rc != 0:
        raise NativeError("grim_prior_matrix failed")
    return out


def prior_matrices(ps, pops, races):
    """one prior matrix per race pair of `races` (Parsed.races()) -> float64[max(1, len(races))][P][P]; without a race pair
    one matrix of ones"""
    priors = np.ones((max(1, len(races)), len(pops), len(pops)))
    for k, (r1, r2) in enumerate(races):
        priors[k] = prior_matrix(ps, pops, r1, r2)
    return priors


TEXT_KEYS = ("umug", "umug_pops", "pmug", "pmug_pops", "miss", "problem")


class Stream:
    """grim_stream: the chunked tokenizer -> device -> formatter pipeline (impute_file's loop)."""

    def __init__(self, ctx, dgraph, adict, params, ps, pops, out_paths=None, want_text=True, want_log=False, want_records=False,
                 chunk_lines=0, depth=0, n_threads=0, line_offset=0, rows_per_chunk=0, timing=False, masks=None, rows_exact=False,
                 placed=False):
        L = host_lib()
        self.ctx = ctx
        o = StreamOpts()
        o.chunk_lines = int(chunk_lines or int(os.environ.get("GRIM_CHUNK_LINES", "0")))
        o.depth = int(depth or int(os.environ.get("GRIM_STREAM_DEPTH", "0")))
        o.n_threads = int(n_threads or int(os.environ.get("GRIM_HOST_THREADS", "0")))
        o.line_offset = int(line_offset)
        o.rows_per_chunk = int(rows_per_chunk or int(os.environ.get("GRIM_ROWS_PER_CHUNK", "0")))
        o.want_text = 1 if want_text else 0
        o.want_log = 1 if want_log else 0
        o.want_records = 1 if want_records else 0
        o.timing = 1 if timing else 0
        o.rows_exact = 1 if rows_exact else 0
        o.placed = 1 if placed else 0
        self._keep = [params, ps]
        if out_paths:
            for k, key in enumerate(TEXT_KEYS):
                if out_paths.get(key):
                    o.out_path[k] = os.fsencode(out_paths[key])
        if masks is not None:
            ids = b"".join(str(k).encode() + b"\0" for k in masks.keys())
            fixed = np.array([int(v) for v in masks.values()], dtype=np.uint8)
            self._keep += [ids, fixed]
            o.mask_ids = ids if len(masks) else b"\0"
            o.mask_fixed = _ptr(fixed) if len(masks) else None
            o.n_masks = len(masks)
        names = (C.c_char_p * len(pops))(*[p.encode() for p in pops])
        self.line_offset = int(line_offset)
        self._lent = []  # buffers lent to the stream (write(..., borrowed=True)): alive until close()
        self.h = L.grim_stream_open(ctx.h, dgraph.h, adict.h, C.byref(params), C.byref(ps), names, len(pops), C.byref(o))
        if not self.h:
            raise NativeError("grim_stream_open failed: " + ctx.error())

    def _check(self, rc):
        if rc < 0:
            raise NativeError("grim_stream: " + host_lib().grim_stream_error(self.h).decode())

    def write(self, data, borrowed=False):
        """feed bytes; `borrowed`: the stream reads them where they are (grim_stream_write_borrowed) -- this object keeps
        `data` alive until finish() / close()"""
        if borrowed:
            if not isinstance(data, bytes):
                raise TypeError("a borrowed buffer must be a bytes object")
            self._lent.append(data)
            self._check(host_lib().grim_stream_write_borrowed(self.h, data, len(data)))
        else:
            self._check(host_lib().grim_stream_write(self.h, data, len(data)))

    def write_text(self, data):
        """universal newlines, as Python's open(): "\r\n" and "\r" end a line too"""
        self._check(host_lib().grim_stream_write_text(self.h, data, len(data)))

    def segment(self, next_line_offset):
        """end the current input segment; the next byte written starts the line with this global index"""
        self._check(host_lib().grim_stream_segment(self.h, int(next_line_offset)))

    def segment_ends(self):
        """after finish(): per segment the cumulative bytes of the seven texts up to its end"""
        L = host_lib()
        out = []
        for k in range(int(L.grim_stream_n_segments(self.h))):
            v = (C.c_uint64 * 7)()
            L.grim_stream_segment_end(self.h, k, v)
            out.append([int(x) for x in v])
        return out

    def segment_wait(self, k):
        """placed output: blocks until the (closed) segment k is formatted; -> bytes of its piece of the seven texts"""
        v = (C.c_uint64 * 7)()
        self._check(host_lib().grim_stream_segment_wait(self.h, int(k), v))
        return [int(x) for x in v]

    def segment_place(self, k, base):
        """placed output: writes segment k's piece of every output file at base[t]; returns when the bytes are written"""
        v = (C.c_uint64 * 6)(*[int(x) for x in base])
        self._check(host_lib().grim_stream_segment_place(self.h, int(k), v))

    def write_file(self, path):
        self._check(host_lib().grim_stream_write_file(self.h, os.fsencode(path)))

    def finish(self):
        self._check(host_lib().grim_stream_finish(self.h))

    def text(self, which, as_bytes=False):
        n = C.c_uint64(0)
        ptr = host_lib().grim_stream_text(self.h, which, C.byref(n))
        data = C.string_at(ptr, n.value) if n.value else b""
        return data if as_bytes else data.decode()

    def stats(self):
        st = StreamStats()
        host_lib().grim_stream_get_stats(self.h, C.byref(st))
        return st

    def devtok_lines(self):
        """-> (offered, handed_back): lines left to the device tokenizer, and those of them it gave back to the host's"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._check(host_lib().grim_stream_devtok_lines(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def unsupported(self):
        L = host_lib()
        out = []
        for k in range(int(L.grim_stream_n_unsupported(self.h))):
            line, reason, ptr, n = C.c_uint64(0), C.c_uint32(0), C.c_void_p(0), C.c_uint32(0)
            L.grim_stream_unsupported(self.h, k, C.byref(line), C.byref(reason), C.byref(ptr), C.byref(n))
            out.append((int(line.value), C.string_at(ptr.value, n.value).decode() if n.value else "", int(reason.value)))
        return out

    def next_records(self):
        """records mode: -> (first_line, kinds, res, rows_base_address, handle) of the next chunk, or None at the end.
        The arrays are VIEWS of the chunk's pinned buffers: copy what you keep, then release(handle)."""
        rec = StreamRecords()
        rc = host_lib().grim_stream_next_records(self.h, C.byref(rec))
        self._check(rc)
        if rc == 0:
            return None
        n = int(rec.n_lines)
        kinds = np.frombuffer((C.c_char * n).from_address(rec.kinds), dtype=np.uint8, count=n)
        res = np.frombuffer((C.c_char * (n * RESULT_DT.itemsize)).from_address(rec.res), dtype=RESULT_DT, count=n)
        return int(rec.first_line), kinds, res, rec.rows, rec

    def release(self, rec):
        host_lib().grim_stream_release_records(self.h, C.byref(rec))

    def close(self):
        if self.h:
            host_lib().grim_stream_free(self.h)
            self.h = None
        self._lent = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
