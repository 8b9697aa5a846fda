"""ctypes binding of include/niqki_hip.h (libniqki_hip.so).

Fails loudly when the shared library is missing or cannot be loaded: there is
no CPU fallback for any entry point.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "lib", "libniqki_hip.so")

MEM_HOST, MEM_DEVICE = 0, 1
SEQ_PAD = 64
KC_SKETCH, KC_DENSIFY, KC_GATHER, KC_HITS, KC_BUILD, KC_INGEST, KC_EXCHANGE, KC_INFLATE = 0, 1, 2, 3, 4, 5, 6, 7
E_GZIP = 7
FILE_GZIP = 0x80
GROUP_ID_BYTES = 128
E_CAPACITY = 4
TAXON_NONE = 0xFFFFFFFF
# NIQKI_CONTAIN_*: what the share of niqki_query_contained is a share of, and the share of 1
CONTAIN_QUERY, CONTAIN_GENOME, CONTAIN_MAX = 0, 1, 2
CONTAIN_ONE = 0xFFFFFFFF
# NIQKI_AUDIT_*: the verdicts of niqki_audit, named in the order of their values (the rule is the kernel's alone)
AUDIT_ALONE, AUDIT_AGREES, AUDIT_TIED, AUDIT_MISPLACED, AUDIT_STRAY = 0, 1, 2, 3, 4
AUDIT_VERDICTS = ("alone", "agrees", "tied", "misplaced", "stray")


class NiqkiError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("niqki status %d: %s" % (code, msg))
        self.code = code


class Params(C.Structure):
    _fields_ = [("K", C.c_uint32), ("S", C.c_uint32), ("W", C.c_uint32), ("H", C.c_uint32),
                ("min_score", C.c_uint32), ("slot_begin", C.c_uint32), ("slot_end", C.c_uint32),
                ("device", C.c_int32), ("tile_genomes", C.c_uint32), ("resident_mib", C.c_uint32),
                ("top_k", C.c_uint32), ("reserved", C.c_uint32 * 1)]


class RawBatch(C.Structure):
    _fields_ = [("raw", C.c_void_p), ("file_ptr", C.c_void_p), ("file_off", C.c_void_p), ("file_type", C.c_void_p),
                ("n_files", C.c_uint32), ("lines", C.c_uint32), ("final", C.c_uint32),
                ("max_entries", C.c_uint32), ("file_status", C.c_void_p)]


class GroupPlan(C.Structure):
    _fields_ = [("sparse", C.c_uint32), ("cand_threshold", C.c_uint32), ("surv_threshold", C.c_uint32),
                ("slice_slots", C.c_uint32), ("slice_bytes", C.c_uint64), ("cand_blob_bytes", C.c_uint64),
                ("sum_words", C.c_uint64), ("row_stride", C.c_uint64)]


class StageInfo(C.Structure):
    _fields_ = [("n_entry", C.c_uint32), ("n_rec", C.c_uint32), ("consumed", C.c_uint64),
                ("seq_bytes", C.c_uint64)]


class TallyTotals(C.Structure):
    _fields_ = [("queries", C.c_uint64), ("classified", C.c_uint64), ("no_hit", C.c_uint64), ("no_common", C.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


def lib_path():
    return _LIB


def build_native(force=False):
    """Compile libniqki_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    src = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-C", src, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", src, "-j4"], stdout=subprocess.DEVNULL)
    return _LIB


# every symbol include/niqki_hip.h declares: (name, restype, argtypes)
_vp, _u32, _u64, _i32, _i64, _int, _dbl = (C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32,
                                         C.c_int64, C.c_int, C.c_double)
ABI = [
    ("niqki_abi_version", _int, []),
    ("niqki_status_string", C.c_char_p, [_int]),
    ("niqki_min_score", _u32, [_dbl, _u32]),
    ("niqki_create", _int, [C.POINTER(Params), C.POINTER(_vp)]),
    ("niqki_destroy", None, [_vp]),
    ("niqki_last_error", C.c_char_p, [_vp]),
    ("niqki_get_params", _int, [_vp, C.POINTER(Params)]),
    ("niqki_select_best_H", _int, [_vp, _dbl, C.POINTER(C.c_uint32)]),
    ("niqki_set_stream", _int, [_vp, _vp]),
    ("niqki_get_stream", _vp, [_vp]),
    ("niqki_synchronize", _int, [_vp]),
    ("niqki_set_option", _int, [_vp, C.c_char_p, _i64]),
    ("niqki_reserve", _int, [_vp, _u32]),
    ("niqki_sketch", _int, [_vp, _vp, _vp, _u32, _vp, _u32, _vp, _int]),
    ("niqki_densify", _int, [_vp, _vp, _u32, _int]),
    ("niqki_insert", _int, [_vp, _vp, _u32, _int]),
    ("niqki_genome_count", _u32, [_vp]),
    ("niqki_build", _int, [_vp]),
    ("niqki_query_counts", _int, [_vp, _vp, _u32, _vp, _u64, _int]),
    ("niqki_query_counts32", _int, [_vp, _vp, _u32, _vp, _u64, _int]),
    ("niqki_hits_from_counts", _int, [_vp, _vp, _u32, _u64, _u32, _u32, _vp, _vp, _vp, _u64, _int]),
    ("niqki_candidates_from_counts", _int, [_vp, _vp, _u32, _u64, _u32, _u32, _u32, _vp, _vp, _int]),
    ("niqki_query_counts_candidates", _int, [_vp, _vp, _u32, _vp, _u64, _u32, _u32, _vp, _vp, _int]),
    ("niqki_query", _int, [_vp, _vp, _u32, _vp, _vp, _vp, _u64, _int]),
    ("niqki_sketch_shared", _int, [_vp, _vp, _u64, _vp]),
    ("niqki_insert_shared", _int, [_vp, _vp, C.POINTER(_u32)]),
    ("niqki_query_shared", _int, [_vp, _vp, C.POINTER(_u64), _vp, _vp, _u64]),
    ("niqki_query_sequence_shared", _int, [_vp, _vp, _u64, C.POINTER(_u64), _vp, _vp, _u64]),
    ("niqki_shared_stats", _int, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    ("niqki_query_survivors", _int, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _int]),
    ("niqki_survivor_counts", _int, [_vp, _vp, _u32, _vp, _u32, _vp, _vp, _u32, _vp, _int]),
    ("niqki_hits_from_candidates", _int, [_vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _u64, _int]),
    ("niqki_query_sequences", _int, [_vp, _vp, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _u64, _int]),
    ("niqki_sketch_ahead", _int, [_vp, _vp, _vp, _u32, _vp, _u32, _int]),
    ("niqki_query_ahead", _int, [_vp, C.POINTER(_u32), _vp, _vp, _vp, _u64, _vp, _int]),
    ("niqki_stage_raw", _int, [_vp, C.POINTER(RawBatch), _int, C.POINTER(StageInfo), _vp]),
    ("niqki_stage_raw_prefetch", _int, [_vp, C.POINTER(RawBatch)]),
    ("niqki_staged_sketch", _int, [_vp, _vp, _int]),
    ("niqki_staged_insert", _int, [_vp]),
    ("niqki_staged_query", _int, [_vp, _vp, _vp, _vp, _u64, _int]),
    ("niqki_staged_records", _int, [_vp, _vp, _vp, _vp, _vp]),
    ("niqki_pack_bound", C.c_size_t, [C.c_size_t]),
    ("niqki_pack_fasta", C.c_size_t, [_vp, C.c_size_t, _vp, C.c_size_t]),
    ("niqki_unpack_fasta", _int, [_vp, C.c_size_t, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("niqki_host_alloc", _vp, [C.c_size_t]),
    ("niqki_host_free", None, [_vp]),
    ("niqki_matrix_range", _int, [_vp, _u32, _u32, _vp, _u64, _int]),
    ("niqki_neighbors_range", _int, [_vp, _u32, _u32, _vp, _vp, _vp, _u64, _int]),
    ("niqki_cluster", _int, [_vp, _u32, _vp, C.POINTER(_u32), _int]),
    ("niqki_dereplicate", _int, [_vp, _u32, _vp, _vp, C.POINTER(_u32), _int]),
    ("niqki_dereplicate_from", _int, [_vp, _u32, _u32, _vp, _vp, C.POINTER(_u32), _int]),
    ("niqki_linkage", _int, [_vp, _u32, _vp, _vp, _vp, _vp, _vp, C.POINTER(_u32), _int]),
    ("niqki_audit", _int, [_vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int]),
    ("niqki_cover", _int, [_vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _u64, _int]),
    ("niqki_staged_cover", _int, [_vp, _u32, _vp, _vp, _vp, _vp, _u64, _int]),
    ("niqki_set_labels", _int, [_vp, _vp, _u32, _int]),
    ("niqki_query_collapsed", _int, [_vp, _vp, _u32, _vp, _vp, _vp, _vp, _u64, _int]),
    ("niqki_staged_query_collapsed", _int, [_vp, _vp, _vp, _vp, _vp, _u64, _int]),
    ("niqki_set_sizes", _int, [_vp, _vp, _u32, _int]),
    ("niqki_query_contained", _int, [_vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _u64, _int]),
    ("niqki_staged_query_contained", _int, [_vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _u64, _int]),
    ("niqki_set_taxonomy", _int, [_vp, _vp, _u32, _vp, _u32, _int]),
    ("niqki_query_lca", _int, [_vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _int]),
    ("niqki_staged_query_lca", _int, [_vp, _u32, _vp, _vp, _vp, _vp, _int]),
    ("niqki_tally_begin", _int, [_vp]),
    ("niqki_tally_add", _int, [_vp, _vp, _vp, _vp, _u32, _int]),
    ("niqki_tally_read", _int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(TallyTotals), _int]),
    ("niqki_tally_end", _int, [_vp]),
    ("niqki_retain", _int, [_vp, _vp, _vp, C.POINTER(_u32), _int]),
    ("niqki_unite", _int, [_vp, _vp, _u32, _vp, C.POINTER(_u32), _int]),
    ("niqki_registers", _int, [_vp, _u32, _u32, _vp, _int]),
    ("niqki_sketch_registers", _int, [_vp, _vp, _u32, _vp, _int]),
    ("niqki_staged_registers", _int, [_vp, _vp, _int]),
    ("niqki_export_dump", _int, [_vp, _vp, _u64, C.POINTER(_u64)]),
    ("niqki_import_dump", _int, [C.POINTER(Params), _vp, _u64, C.POINTER(_u64), C.POINTER(_vp)]),
    ("niqki_export_dump_header", _int, [_vp, _vp]),
    ("niqki_export_dump_layout", _int, [_vp, _vp]),
    ("niqki_export_dump_slots", _int, [_vp, _u32, _u32, _vp, _u64, C.POINTER(_u64)]),
    ("niqki_import_begin", _int, [C.POINTER(Params), _vp, C.POINTER(_vp)]),
    ("niqki_import_slots", _int, [_vp, _u32, _u32, _vp, _u64, C.POINTER(_u64)]),
    ("niqki_append_begin", _int, [_vp, _vp]),
    ("niqki_append_slots", _int, [_vp, _u32, _u32, _vp, _u64, C.POINTER(_u64)]),
    ("niqki_append_cancel", _int, [_vp]),
    ("niqki_append_dump", _int, [_vp, _vp, _u64, C.POINTER(_u64)]),
    ("niqki_get_sketches", _int, [_vp, _u32, _u32, _vp, _int]),
    ("niqki_query_gathered", _int, [_vp, _vp, _u32, _vp, _int]),
    ("niqki_group_slot_range", None, [_u32, _u32, _u32, C.POINTER(_u32), C.POINTER(_u32)]),
    ("niqki_group_new_id", _int, [_vp]),
    ("niqki_group_plan_batch", _int, [_u32, _u32, _u32, _int, _u32, _u32, _u32, C.POINTER(GroupPlan)]),
    ("niqki_group_create", _int, [_vp, _u32, _u32, _u32, _vp, C.POINTER(_vp)]),
    ("niqki_group_destroy", None, [_vp]),
    ("niqki_group_last_error", C.c_char_p, [_vp]),
    ("niqki_group_set_option", _int, [_vp, C.c_char_p, _i64]),
    ("niqki_group_get_stat", _int, [_vp, C.c_char_p, C.POINTER(_u64)]),
    ("niqki_group_insert", _int, [_vp, _vp, _u32, _u32]),
    ("niqki_group_query", _int, [_vp, _vp, _u32, _vp, _vp, _vp, _u64, _int]),
    ("niqki_group_query_begin", _int, [_vp, _vp, _u32, _vp, _vp, _vp, _u64, _int]),
    ("niqki_group_query_end", _int, [_vp]),
    ("niqki_group_staged_insert", _int, [_vp, _u32, _vp]),
    ("niqki_group_staged_query", _int, [_vp, _u32, _vp, _vp, _vp, _vp, _u64, _int]),
    ("niqki_get_stat", _int, [_vp, C.c_char_p, C.POINTER(_u64)]),
    ("niqki_profile_enable", _int, [_vp, _int]),
    ("niqki_profile_reset", _int, [_vp]),
    ("niqki_profile_read", _int, [_vp, _int, C.POINTER(_dbl), C.POINTER(_u64)]),
    ("niqki_synth_genomes", _int, [_vp, _u64, _vp, _vp, _vp, _u32, _u64, _u64, _vp, _int]),
    ("niqki_synth_genome_host", None, [_u64, _u32, _u32, _u32, _u64, _vp]),
    ("niqki_synth_reads", _int, [_vp, _u64, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u64, _vp, _int]),
    ("niqki_measure_alu", _int, [_vp, _int, _dbl, C.POINTER(_dbl)]),
    ("niqki_gunzip", _int, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, C.POINTER(_u64)]),
    ("niqki_gunzip_stats", _int, [_vp, _vp]),
]

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB):
            raise ImportError("%s is missing: run __graft_entry__.build() (make -C niqki_amd/csrc); "
                              "there is no fallback path" % _LIB)
        # libniqki_hip.so binds to the HIP runtime by soname (libamdhip64.so.7).
        # PyTorch wheels ship their own copy under the same soname; when both are
        # used in one process PyTorch's must be loaded first, otherwise the process
        # ends up with two runtimes and the second one to initialise finds no
        # device.  (The C++ host program never loads PyTorch.)
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(_LIB)
        for name, res, args in ABI:
            f = getattr(L, name)  # AttributeError if the library lacks a declared symbol
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def cut_linkage(merge_into, merge_count, t):
    """labels of Engine.cluster(t) from Engine.linkage(floor)'s hierarchy, t >= floor: from every genome follow
    merge_into while merge_count >= t.  (merge_count descends strictly along a chain, so the walk stops at the first
    genome below t, or at a root.)"""
    into = np.asarray(merge_into, dtype=np.int64)
    cnt = np.asarray(merge_count, dtype=np.int64)
    ids = np.arange(into.size, dtype=np.int64)
    up = np.where((cnt >= t) & (into != ids), into, ids)     # one step, or none
    while True:
        nxt = up[up]
        if np.array_equal(nxt, up):
            return up.astype(np.uint32)
        up = nxt


def row_stride(n):
    """NIQKI_ROW_STRIDE of the header: counter rows that start on 128-byte lines."""
    return (int(n) + 63) & ~63


def min_score(J, S):
    return lib().niqki_min_score(J, S)


def pack_fasta(data):
    """niqki_pack_fasta: the packed container of a FASTA file's bytes (np.uint8 array), or None when the file is not
    worth packing (hand it over raw).  Host code: no GPU needed."""
    raw = np.frombuffer(bytes(data), dtype=np.uint8)
    out = np.empty(lib().niqki_pack_bound(raw.size), dtype=np.uint8)
    n = lib().niqki_pack_fasta(raw.ctypes.data if raw.size else None, raw.size, out.ctypes.data, out.size)
    return out[:n].copy() if n else None


def unpack_fasta(container):
    """niqki_unpack_fasta: the file's bytes back (the host restatement of the device pass)."""
    c = np.ascontiguousarray(container, dtype=np.uint8)
    n = C.c_size_t(0)
    rc = lib().niqki_unpack_fasta(c.ctypes.data, c.size, None, 0, C.byref(n))
    if rc:
        raise NiqkiError(rc, "niqki_unpack_fasta: not a well-formed container")
    out = np.empty(max(n.value, 1), dtype=np.uint8)
    rc = lib().niqki_unpack_fasta(c.ctypes.data, c.size, out.ctypes.data, out.size, C.byref(n))
    if rc:
        raise NiqkiError(rc, "niqki_unpack_fasta failed")
    return out[:n.value]


def synth_genome_host(seed, family, member, rate14, length):
    out = np.empty(length, dtype=np.uint8)
    lib().niqki_synth_genome_host(seed, family, member, rate14, length, out.ctypes.data)
    return out


def _p(x):
    """numpy array / torch tensor / int / None -> raw address."""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    if isinstance(x, int):
        return x
    return x.data_ptr()  # torch tensor


class Engine:
    """One handle = one GPU (or one slot shard of an index)."""

    def __init__(self, K=31, S=15, W=12, H=4, J=0.0, min_score_value=None, device=-1,
                 slot_begin=0, slot_end=0, tile_genomes=0, resident_mib=0, top_k=0, _handle=None):
        self.L = lib()
        if _handle is not None:
            self.h = _handle
        else:
            ms = self.L.niqki_min_score(J, S) if min_score_value is None else min_score_value
            p = Params(K, S, W, H, ms, slot_begin, slot_end, device, tile_genomes, resident_mib, top_k)
            h = _vp()
            rc = self.L.niqki_create(C.byref(p), C.byref(h))
            if rc:
                raise NiqkiError(rc, "%s (%s)" % (self.L.niqki_status_string(rc).decode(),
                                                  self.L.niqki_last_error(None).decode()))
            self.h = h
        q = Params()
        self.L.niqki_get_params(self.h, C.byref(q))
        self.K, self.S, self.W, self.H, self.min_score = q.K, q.S, q.W, q.H, q.min_score
        self.slot_begin, self.slot_end, self.device = q.slot_begin, q.slot_end, q.device
        self.top_k = q.top_k
        self.F = 1 << self.S

    def close(self):
        if getattr(self, "h", None):
            self.L.niqki_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, allow=()):
        if rc and rc not in allow:
            raise NiqkiError(rc, "%s (%s)" % (self.L.niqki_status_string(rc).decode(),
                                              self.L.niqki_last_error(self.h).decode()))
        return rc

    # -- plumbing
    def set_stream(self, stream_ptr):
        self._ck(self.L.niqki_set_stream(self.h, stream_ptr))

    # -- many host threads on one handle (niqki_*_shared: callers are combined into batches)
    def sketch_shared(self, seq):
        s = np.ascontiguousarray(seq, dtype=np.uint8)
        out = np.empty(self.F, dtype=np.int32)
        self._ck(self.L.niqki_sketch_shared(self.h, _p(s), s.size, _p(out)))
        return out

    def insert_shared(self, sketch):
        sk = np.ascontiguousarray(sketch, dtype=np.int32)
        gid = _u32(0)
        self._ck(self.L.niqki_insert_shared(self.h, _p(sk), C.byref(gid)))
        return gid.value

    def query_shared(self, sketch, capacity=1024):
        sk = np.ascontiguousarray(sketch, dtype=np.int32)
        n = _u64(0)
        hc, hg = np.empty(capacity, np.uint32), np.empty(capacity, np.uint32)
        self._ck(self.L.niqki_query_shared(self.h, _p(sk), C.byref(n), _p(hc), _p(hg), capacity))
        if n.value > capacity:
            return self.query_shared(sketch, int(n.value))
        return hc[:n.value].copy(), hg[:n.value].copy()

    def query_sequence_shared(self, seq, capacity=1024):
        s = np.ascontiguousarray(seq, dtype=np.uint8)
        n = _u64(0)
        hc, hg = np.empty(capacity, np.uint32), np.empty(capacity, np.uint32)
        self._ck(self.L.niqki_query_sequence_shared(self.h, _p(s), s.size, C.byref(n), _p(hc), _p(hg), capacity))
        if n.value > capacity:
            return self.query_sequence_shared(seq, int(n.value))
        return hc[:n.value].copy(), hg[:n.value].copy()

    def shared_stats(self):
        b, r, m = _u64(0), _u64(0), _u64(0)
        self._ck(self.L.niqki_shared_stats(self.h, C.byref(b), C.byref(r), C.byref(m)))
        return {"batches": b.value, "requests": r.value, "largest_batch": m.value}

    def get_stream(self):
        """The hipStream_t the handle enqueues on (an int, for torch.cuda.ExternalStream)."""
        return int(self.L.niqki_get_stream(self.h) or 0)

    def synchronize(self):
        self._ck(self.L.niqki_synchronize(self.h))

    def set_option(self, key, value):
        self._ck(self.L.niqki_set_option(self.h, key.encode(), int(value)))

    def reserve(self, n):
        self._ck(self.L.niqki_reserve(self.h, n))

    def select_best_H(self, genome_size):
        """Index::select_best_H (-G): src/niqki_index.cpp:126-138."""
        H = C.c_uint32(0)
        self._ck(self.L.niqki_select_best_H(self.h, float(genome_size), C.byref(H)))
        self.H = H.value
        return self.H

    @property
    def n_genomes(self):
        return self.L.niqki_genome_count(self.h)

    def stat(self, key):
        v = _u64(0)
        self._ck(self.L.niqki_get_stat(self.h, key.encode(), C.byref(v)))
        return v.value

    def tile_genomes(self):
        q = Params()
        self.L.niqki_get_params(self.h, C.byref(q))
        return q.tile_genomes

    # -- host-memory convenience (numpy in / numpy out)
    @staticmethod
    def pack_records(records):
        """list of bytes/str/uint8 arrays -> (seqs uint8, rec_off uint64)."""
        arrs = []
        for r in records:
            if isinstance(r, str):
                r = r.encode()
            if isinstance(r, (bytes, bytearray)):
                r = np.frombuffer(bytes(r), dtype=np.uint8)
            arrs.append(np.ascontiguousarray(r, dtype=np.uint8))
        off = np.zeros(len(arrs) + 1, dtype=np.uint64)
        if arrs:
            off[1:] = np.cumsum([a.size for a in arrs], dtype=np.uint64)
        seqs = np.concatenate(arrs) if arrs else np.zeros(0, dtype=np.uint8)
        return np.ascontiguousarray(seqs), off

    def sketch(self, records, entry_rec=None):
        seqs, off = self.pack_records(records)
        n_rec = off.size - 1
        if entry_rec is None:
            n_entry, er = n_rec, None
        else:
            er = np.ascontiguousarray(entry_rec, dtype=np.uint32)
            n_entry = er.size - 1
        out = np.empty((n_entry, self.F), dtype=np.int32)
        self._ck(self.L.niqki_sketch(self.h, _p(seqs) if seqs.size else _p(np.zeros(1, np.uint8)),
                                     _p(off), n_rec, _p(er), n_entry, _p(out), MEM_HOST))
        return out

    def densify(self, sketches):
        sk = np.ascontiguousarray(sketches, dtype=np.int32).copy()
        sk2 = sk.reshape(-1, self.F)
        self._ck(self.L.niqki_densify(self.h, _p(sk2), sk2.shape[0], MEM_HOST))
        return sk

    def insert(self, sketches):
        sk = np.ascontiguousarray(sketches, dtype=np.int32).reshape(-1, self.F)
        self._ck(self.L.niqki_insert(self.h, _p(sk), sk.shape[0], MEM_HOST))

    def build(self):
        self._ck(self.L.niqki_build(self.h))

    def query_counts(self, sketches):
        sk = np.ascontiguousarray(sketches, dtype=np.int32).reshape(-1, self.F)
        n = self.n_genomes
        stride = row_stride(n)
        out = np.zeros((sk.shape[0], max(stride, 2)), dtype=np.uint16)
        self._ck(self.L.niqki_query_counts(self.h, _p(sk), sk.shape[0], _p(out), out.shape[1], MEM_HOST))
        return out[:, :n]

    def query_counts32(self, sketches):
        sk = np.ascontiguousarray(sketches, dtype=np.int32).reshape(-1, self.F)
        n = self.n_genomes
        stride = row_stride(n)
        out = np.zeros((sk.shape[0], max(stride, 2)), dtype=np.uint32)
        self._ck(self.L.niqki_query_counts32(self.h, _p(sk), sk.shape[0], _p(out), out.shape[1], MEM_HOST))
        return out[:, :n]

    def _hits(self, call, nq, capacity):
        off = np.zeros(nq + 1, dtype=np.uint64)
        while True:
            hc = np.empty(max(capacity, 1), dtype=np.uint32)
            hg = np.empty(max(capacity, 1), dtype=np.uint32)
            rc = call(off, hc, hg, capacity)
            self._ck(rc, allow=(E_CAPACITY,))
            if rc == 0:
                tot = int(off[nq])
                return off, hc[:tot], hg[:tot]
            capacity = int(off[nq])

    def query(self, sketches, capacity=None):
        sk = np.ascontiguousarray(sketches, dtype=np.int32).reshape(-1, self.F)
        nq = sk.shape[0]
        cap = capacity if capacity is not None else max(1024, nq * 64)
        return self._hits(lambda off, hc, hg, c: self.L.niqki_query(
            self.h, _p(sk), nq, _p(off), _p(hc), _p(hg), c, MEM_HOST), nq, cap)

    def hits_from_counts(self, counts, gid_begin=0, n_gids=None, capacity=None):
        ct = np.ascontiguousarray(counts, dtype=np.uint16)
        nq, stride = ct.shape
        ng = stride - gid_begin if n_gids is None else n_gids
        cap = capacity if capacity is not None else max(1024, nq * 64)
        return self._hits(lambda off, hc, hg, c: self.L.niqki_hits_from_counts(
            self.h, _p(ct), nq, stride, gid_begin, ng, _p(off), _p(hc), _p(hg), c, MEM_HOST), nq, cap)

    def query_sequences(self, records, capacity=None):
        seqs, off = self.pack_records(records)
        nq = off.size - 1
        cap = capacity if capacity is not None else max(1024, nq * 64)
        return self._hits(lambda ho, hc, hg, c: self.L.niqki_query_sequences(
            self.h, _p(seqs), _p(off), nq, None, nq, _p(ho), _p(hc), _p(hg), c, MEM_HOST), nq, cap)

    # -- raw file bytes, framed on the GPU (niqki_stage_raw and friends)
    def stage_raw(self, files, types=None, lines=False, final=True, max_entries=16384, scattered=False, prefetch=None):
        """files: list of bytes-like (the gunzipped content of each file).  Returns
        (StageInfo, entry_hdr) -- entry_hdr: raw offset of each entry's header line (lines mode).
        scattered: hand the files over as separate buffers (file_ptr) instead of one.
        prefetch (with scattered): "this" = niqki_stage_raw_prefetch of this very batch first,
        "only" = just the prefetch, nothing staged (the buffers stay alive on the object), "take" =
        stage the batch of the last "only" call from those very buffers."""
        blobs = [np.frombuffer(bytes(f), dtype=np.uint8) for f in files]
        off = np.zeros(len(blobs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([b.size for b in blobs], dtype=np.uint64)
        raw = np.concatenate(blobs + [np.zeros(0, np.uint8)]) if blobs else np.zeros(0, np.uint8)
        ty = np.array([ord(t) if isinstance(t, str) else int(t) for t in (types if types else "A" * len(blobs))], dtype=np.uint8)
        if ty.size == 0:
            ty = np.zeros(1, np.uint8)
        self.file_status = np.zeros(max(len(blobs), 1), dtype=np.uint8)   # (why a gzip file was refused, after E_GZIP)
        ptrs = None
        if prefetch == "take":      # the buffers an earlier prefetch="only" call handed over
            keep, ptrs, off, ty = self._pre_keep
        elif scattered:
            keep = [np.ascontiguousarray(x).copy() for x in blobs]
            ptrs = (C.c_void_p * max(len(keep), 1))(*[k.ctypes.data for k in keep])
        b = RawBatch(None if scattered or not raw.size else _p(raw), C.cast(ptrs, C.c_void_p) if scattered else None,
                     _p(off), _p(ty), len(blobs), int(bool(lines)), int(bool(final)), max_entries, _p(self.file_status))
        info = StageInfo()
        hdr = np.zeros(max(max_entries, 1), dtype=np.uint64)
        if prefetch in ("this", "only"):
            self._ck(self.L.niqki_stage_raw_prefetch(self.h, C.byref(b)))
            if prefetch == "only":
                self._pre_keep = (keep, ptrs, off, ty)
                return None, None
        self._ck(self.L.niqki_stage_raw(self.h, C.byref(b), MEM_HOST, C.byref(info), _p(hdr) if lines else None))
        self._staged = info
        return info, hdr[:info.n_entry] if lines else None

    def gunzip(self, files, sizes, check_outside=True):
        """The device inflate alone (niqki_gunzip): files = gzip files as bytes, sizes = the length each is expected
        to inflate to.  Returns (list of bytes, status, produced, members, outside)."""
        blobs = [np.frombuffer(bytes(f), dtype=np.uint8) for f in files]
        goff = np.zeros(len(blobs) + 1, dtype=np.uint64)
        goff[1:] = np.cumsum([b.size for b in blobs], dtype=np.uint64)
        roff = np.zeros(len(blobs) + 1, dtype=np.uint64)
        roff[1:] = np.cumsum(list(sizes), dtype=np.uint64)
        gz = np.concatenate(blobs + [np.zeros(8, np.uint8)])
        raw = np.zeros(int(roff[-1]) + 8, dtype=np.uint8)
        n = len(blobs)
        status, produced, members = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint32)
        outside = C.c_uint64(0)
        self._ck(self.L.niqki_gunzip(self.h, _p(gz), _p(goff), n, _p(roff), _p(raw), _p(status), _p(produced), _p(members),
                                     C.byref(outside) if check_outside else None))
        out = [raw[int(roff[i]):int(roff[i]) + int(min(produced[i], roff[i + 1] - roff[i]))].tobytes() for i in range(n)]
        return out, status[:n], produced[:n], members[:n], int(outside.value)

    def gunzip_stats(self):
        """{rounds, round_bytes, serial_tokens, blocks} of the last device inflate (summed over its files)"""
        o = np.zeros(4, dtype=np.uint64)
        self._ck(self.L.niqki_gunzip_stats(self.h, _p(o)))
        return dict(zip(("rounds", "round_bytes", "serial_tokens", "blocks"), (int(x) for x in o)))

    def staged_records(self):
        """(records as list of bytes, entry_rec, hdr_pos) of the staged batch."""
        st = self._staged
        rec_off = np.zeros(st.n_rec + 1, dtype=np.uint64)
        seqs = np.zeros(max(st.seq_bytes, 1), dtype=np.uint8)
        entry_rec = np.zeros(st.n_entry + 1, dtype=np.uint32)
        hdr_pos = np.zeros(max(st.n_rec, 1), dtype=np.uint64)
        self._ck(self.L.niqki_staged_records(self.h, _p(rec_off), _p(seqs), _p(entry_rec), _p(hdr_pos)))
        recs = [seqs[int(rec_off[i]):int(rec_off[i + 1])].tobytes() for i in range(st.n_rec)]
        return recs, entry_rec, hdr_pos[:st.n_rec]

    def staged_sketch(self):
        out = np.empty((self._staged.n_entry, self.F), dtype=np.int32)
        self._ck(self.L.niqki_staged_sketch(self.h, _p(out), MEM_HOST))
        return out

    def staged_insert(self):
        self._ck(self.L.niqki_staged_insert(self.h))

    def staged_query(self, capacity=None):
        nq = self._staged.n_entry
        cap = capacity if capacity is not None else max(1024, nq * 64)
        return self._hits(lambda ho, hc, hg, c: self.L.niqki_staged_query(
            self.h, _p(ho), _p(hc), _p(hg), c, MEM_HOST), nq, cap)

    def matrix_range(self, begin, end):
        n = self.n_genomes
        stride = max(row_stride(n), 2)
        out = np.zeros((end - begin, stride), dtype=np.uint16)
        self._ck(self.L.niqki_matrix_range(self.h, begin, end, _p(out), stride, MEM_HOST))
        return out[:, :n]

    def neighbors_range(self, begin, end, capacity=None):
        """The hits of the STORED sketches of genomes [begin, end): what query(get_sketches(begin, end - begin))
        returns, without the sketches leaving the device.  Same return shape as query."""
        nq = max(end - begin, 0)
        cap = capacity if capacity is not None else max(1024, nq * 64)
        return self._hits(lambda off, hc, hg, c: self.L.niqki_neighbors_range(
            self.h, begin, end, _p(off), _p(hc), _p(hg), c, MEM_HOST), nq, cap)

    def cluster(self, threshold):
        """Single-linkage clusters at co-occurrence count >= threshold: (labels, n_clusters), labels[g] = the
        smallest genome id of g's cluster."""
        labels = np.empty(self.n_genomes, dtype=np.uint32)
        n = _u32(0)
        self._ck(self.L.niqki_cluster(self.h, int(threshold), _p(labels), C.byref(n), MEM_HOST))
        return labels, int(n.value)

    def dereplicate(self, threshold, counts=False):
        """Greedy representatives in index order at co-occurrence count >= threshold: genome t is a representative
        iff no representative below it is linked to it; labels[g] = g, or the linked representative with the largest
        count (ties: the smallest).  (labels, n_representatives), or with counts=True
        (labels, label_counts, n_representatives), label_counts[g] = count(g, labels[g]), 0 for a representative."""
        labels = np.empty(self.n_genomes, dtype=np.uint32)
        lc = np.empty(self.n_genomes, dtype=np.uint32) if counts else None
        n = _u32(0)
        self._ck(self.L.niqki_dereplicate(self.h, int(threshold), _p(labels), _p(lc) if counts else None, C.byref(n), MEM_HOST))
        return (labels, lc, int(n.value)) if counts else (labels, int(n.value))

    def dereplicate_from(self, first, threshold, counts=False):
        """dereplicate with the genomes below `first` given: all of them are representatives (labels[g] = g, count 0),
        a genome from `first` on is one iff no representative below it, given or new, is linked to it.  Same returns
        as dereplicate; first=0 is dereplicate."""
        labels = np.empty(self.n_genomes, dtype=np.uint32)
        lc = np.empty(self.n_genomes, dtype=np.uint32) if counts else None
        n = _u32(0)
        self._ck(self.L.niqki_dereplicate_from(self.h, int(first), int(threshold), _p(labels), _p(lc) if counts else None,
                                               C.byref(n), MEM_HOST))
        return (labels, lc, int(n.value)) if counts else (labels, int(n.value))

    def linkage(self, floor, edges=True):
        """The complete single-linkage hierarchy at co-occurrence counts >= floor, in one self-join:
        (merge_into, merge_count, (edge_lo, edge_hi, edge_count) | None, n_roots).  merge_count[g] is the largest
        threshold at which genome g is not the smallest id of its cluster, merge_into[g] its cluster's label there
        (g and 0 for a genome that is one down to the floor): cut_linkage reads the labels of cluster(t) off the two
        for any t >= floor.  The edges are the maximum spanning forest in edge order (larger count, then smaller lo,
        then smaller hi), N - n_roots of them."""
        n_g = self.n_genomes
        into = np.empty(n_g, dtype=np.uint32)
        cnt = np.empty(n_g, dtype=np.uint32)
        e3 = [np.zeros(n_g, dtype=np.uint32) for _ in range(3)] if edges else None
        n = _u32(0)
        ep = [_p(a) for a in e3] if edges else [None, None, None]
        self._ck(self.L.niqki_linkage(self.h, int(floor), _p(into), _p(cnt), ep[0], ep[1], ep[2], C.byref(n), MEM_HOST))
        n_edges = n_g - int(n.value)
        return into, cnt, (tuple(a[:n_edges].copy() for a in e3) if edges else None), int(n.value)

    def audit(self, threshold, k=1):
        """niqki_audit: every indexed genome's leave-one-out neighbours at co-occurrence count >= max(threshold, 1)
        against the labelling of set_labels, in one self-join: (verdict, own_count, own_gid, other_count, other_gid,
        vote_gid, vote_n), uint32 arrays of one entry per genome.  own / other: the nearest other genome under the
        genome's label and under another one (0 and 0xFFFFFFFF: none); vote: the label most frequent among the k
        nearest, as its first member there and its number of members; verdict: AUDIT_* (AUDIT_VERDICTS names them)."""
        out = tuple(np.empty(self.n_genomes, dtype=np.uint32) for _ in range(7))
        self._ck(self.L.niqki_audit(self.h, int(threshold), int(k), *[_p(a) for a in out], MEM_HOST))
        return out

    def _cover(self, call, nq, capacity, totals):
        off = np.zeros(nq + 1, dtype=np.uint64)
        while True:
            hc, hg, ht = (np.empty(max(capacity, 1), dtype=np.uint32) for _ in range(3))
            rc = call(off, hc, hg, ht if totals else None, capacity)
            self._ck(rc, allow=(E_CAPACITY,))
            if rc == 0:
                tot = int(off[nq])
                return (off, hc[:tot], hg[:tot], ht[:tot]) if totals else (off, hc[:tot], hg[:tot])
            capacity = int(off[nq])

    def cover(self, sketches, max_picks=0, capacity=None, totals=False):
        """niqki_cover: the greedy cover of each query sketch, (off, counts, gids[, totals]) shaped like query's
        result.  A query's picks are in pick order; counts = the slots a pick newly explains, totals = the genome's
        plain count.  max_picks = 0: no limit."""
        sk = np.ascontiguousarray(sketches, dtype=np.int32).reshape(-1, self.F)
        nq = sk.shape[0]
        cap = capacity if capacity is not None else (nq * max_picks if max_picks else max(1024, nq * 8))
        return self._cover(lambda off, hc, hg, ht, c: self.L.niqki_cover(
            self.h, _p(sk), nq, int(max_picks), _p(off), _p(hc), _p(hg), _p(ht), c, MEM_HOST), nq, cap, totals)

    def staged_cover(self, max_picks=0, capacity=None, totals=False):
        """niqki_staged_cover: cover of the staged batch's sketches; the staged batch stays usable."""
        nq = self._staged.n_entry
        cap = capacity if capacity is not None else (nq * max_picks if max_picks else max(1024, nq * 8))
        return self._cover(lambda off, hc, hg, ht, c: self.L.niqki_staged_cover(
            self.h, int(max_picks), _p(off), _p(hc), _p(hg), _p(ht), c, MEM_HOST), nq, cap, totals)

    def set_labels(self, labels):
        """niqki_set_labels: a uint32 label per indexed genome (a numpy array, or a device tensor of dtype int32 /
        uint32 holding the same bits), None to remove the labelling.  Labels need not be dense; the labelling lasts
        until genomes are added or dropped."""
        if labels is None:
            self._ck(self.L.niqki_set_labels(self.h, None, 0, MEM_HOST))
        elif hasattr(labels, "data_ptr"):
            if labels.element_size() != 4 or not labels.is_contiguous():
                raise ValueError("set_labels: a device tensor must be contiguous and hold 32-bit labels")
            self._ck(self.L.niqki_set_labels(self.h, _p(labels), int(labels.numel()), MEM_DEVICE))
        else:
            lab = np.ascontiguousarray(labels, dtype=np.uint32).reshape(-1)
            self._ck(self.L.niqki_set_labels(self.h, _p(lab) if lab.size else None, lab.size, MEM_HOST))

    def query_collapsed(self, sketches, capacity=None, members=False):
        """niqki_query_collapsed: per query the best hit of every label, (off, counts, gids[, members]) shaped like
        query's result.  A query's entries are the first of their label in its full ordered hit list, in that order;
        members = the label's entries in the full list.  The handle's top_k bounds the labels."""
        sk = np.ascontiguousarray(sketches, dtype=np.int32).reshape(-1, self.F)
        nq = sk.shape[0]
        cap = capacity if capacity is not None else max(1024, nq * 8)
        return self._cover(lambda off, hc, hg, hm, c: self.L.niqki_query_collapsed(
            self.h, _p(sk), nq, _p(off), _p(hc), _p(hg), _p(hm), c, MEM_HOST), nq, cap, members)

    def staged_query_collapsed(self, capacity=None, members=False):
        """niqki_staged_query_collapsed: query_collapsed of the staged batch's sketches; the staged batch stays usable."""
        nq = self._staged.n_entry
        cap = capacity if capacity is not None else max(1024, nq * 8)
        return self._cover(lambda off, hc, hg, hm, c: self.L.niqki_staged_query_collapsed(
            self.h, _p(off), _p(hc), _p(hg), _p(hm), c, MEM_HOST), nq, cap, members)

    def set_sizes(self, sizes):
        """niqki_set_sizes: a uint64 size (distinct k-mers, below 2^40; 0 = none) per indexed genome (a numpy array, or
        a device tensor of 64-bit elements), None to remove the sizes.  They last until genomes are added or dropped."""
        if sizes is None:
            self._ck(self.L.niqki_set_sizes(self.h, None, 0, MEM_HOST))
        elif hasattr(sizes, "data_ptr"):
            if sizes.element_size() != 8 or not sizes.is_contiguous():
                raise ValueError("set_sizes: a device tensor must be contiguous and hold 64-bit sizes")
            self._ck(self.L.niqki_set_sizes(self.h, _p(sizes), int(sizes.numel()), MEM_DEVICE))
        else:
            sz = np.ascontiguousarray(sizes, dtype=np.uint64).reshape(-1)
            self._ck(self.L.niqki_set_sizes(self.h, _p(sz) if sz.size else None, sz.size, MEM_HOST))

    def _contained(self, call, nq, capacity, unsized):
        off = np.zeros(nq + 1, dtype=np.uint64)
        nu = np.zeros(nq, dtype=np.uint32)
        while True:
            hs, hc, hg = (np.empty(max(capacity, 1), dtype=np.uint32) for _ in range(3))
            rc = call(off, hs, hc, hg, nu if unsized else None, capacity)
            self._ck(rc, allow=(E_CAPACITY,))
            if rc == 0:
                tot = int(off[nq])
                return (off, hs[:tot], hc[:tot], hg[:tot]) + ((nu,) if unsized else ())
            capacity = int(off[nq])

    def query_contained(self, sketches, qsizes, mode=0, min_share=0, unsized=False, capacity=None):
        """niqki_query_contained: per query the hits with a size whose share (CONTAIN_QUERY / _GENOME / _MAX of the
        sizes of set_sizes and qsizes, a uint64 per query) reaches min_share (CONTAIN_ONE = 1), ordered by share with
        ties in the full list's order: (off, shares, counts, gids[, n_unsized]).  The handle's min_score is the floor,
        its top_k the cut."""
        sk = np.ascontiguousarray(sketches, dtype=np.int32).reshape(-1, self.F)
        nq = sk.shape[0]
        qs = np.ascontiguousarray(qsizes, dtype=np.uint64).reshape(-1)
        if qs.size != nq:
            raise ValueError("query_contained: %d sizes for %d queries" % (qs.size, nq))
        cap = capacity if capacity is not None else max(1024, nq * 8)
        return self._contained(lambda off, hs, hc, hg, nu, c: self.L.niqki_query_contained(
            self.h, _p(sk), _p(qs), nq, int(mode), int(min_share), _p(off), _p(hs), _p(hc), _p(hg), _p(nu), c, MEM_HOST),
            nq, cap, unsized)

    def staged_query_contained(self, qsizes, mode=0, min_share=0, unsized=False, capacity=None):
        """niqki_staged_query_contained: query_contained of the staged batch's sketches (qsizes: one per staged
        entry); the staged batch stays usable."""
        nq = self._staged.n_entry
        qs = np.ascontiguousarray(qsizes, dtype=np.uint64).reshape(-1)
        if qs.size != nq:
            raise ValueError("staged_query_contained: %d sizes for %d staged entries" % (qs.size, nq))
        cap = capacity if capacity is not None else max(1024, nq * 8)
        return self._contained(lambda off, hs, hc, hg, nu, c: self.L.niqki_staged_query_contained(
            self.h, _p(qs), int(mode), int(min_share), _p(off), _p(hs), _p(hc), _p(hg), _p(nu), c, MEM_HOST),
            nq, cap, unsized)

    def set_taxonomy(self, genome_taxon, parent):
        """niqki_set_taxonomy: genome_taxon[g] = the taxon of indexed genome g, parent[t] = the parent of taxon t (a
        root is its own parent); numpy arrays, or two device tensors of 32-bit elements.  None for either removes the
        taxonomy.  It lasts until genomes are added or dropped."""
        if genome_taxon is None or parent is None:
            self._ck(self.L.niqki_set_taxonomy(self.h, None, 0, None, 0, MEM_HOST))
        elif hasattr(genome_taxon, "data_ptr") or hasattr(parent, "data_ptr"):
            for t in (genome_taxon, parent):
                if not hasattr(t, "data_ptr") or t.element_size() != 4 or not t.is_contiguous():
                    raise ValueError("set_taxonomy: device tensors must both be contiguous and hold 32-bit ids")
            self._ck(self.L.niqki_set_taxonomy(self.h, _p(genome_taxon), int(genome_taxon.numel()), _p(parent),
                                               int(parent.numel()), MEM_DEVICE))
        else:
            gt = np.ascontiguousarray(genome_taxon, dtype=np.uint32).reshape(-1)
            par = np.ascontiguousarray(parent, dtype=np.uint32).reshape(-1)
            spare = np.zeros(1, dtype=np.uint32)   # (an empty index has no genome taxa, and NULL would remove the taxonomy)
            self._ck(self.L.niqki_set_taxonomy(self.h, _p(gt) if gt.size else _p(spare), gt.size,
                                               _p(par) if par.size else None, par.size, MEM_HOST))

    def _lca(self, call, nq, details):
        outs = [np.empty(nq, dtype=np.uint32) for _ in range(4 if details else 1)]
        ptrs = [_p(a) if nq else None for a in outs] + [None] * (4 - len(outs))
        if nq == 0:
            ptrs[0] = _p(np.empty(1, dtype=np.uint32))
        self._ck(call(*ptrs))
        return tuple(outs) if details else outs[0]

    def query_lca(self, sketches, top_permille=0, details=False):
        """niqki_query_lca: per query the deepest taxon that holds every hit within top_permille of its best hit
        (TAXON_NONE: no hit, or hits in two trees), as a uint32 array; with details (taxon, best_count, best_gid,
        considered)."""
        sk = np.ascontiguousarray(sketches, dtype=np.int32).reshape(-1, self.F)
        nq = sk.shape[0]
        return self._lca(lambda t, bc, bg, co: self.L.niqki_query_lca(
            self.h, _p(sk) if nq else None, nq, int(top_permille), t, bc, bg, co, MEM_HOST), nq, details)

    def staged_query_lca(self, top_permille=0, details=False):
        """niqki_staged_query_lca: query_lca of the staged batch's sketches; the staged batch stays usable."""
        return self._lca(lambda t, bc, bg, co: self.L.niqki_staged_query_lca(
            self.h, int(top_permille), t, bc, bg, co, MEM_HOST), self._staged.n_entry, details)

    def tally_begin(self):
        """niqki_tally_begin: opens (or clears and reopens) the handle's taxon tally; it needs a taxonomy.  While it is
        open every query_lca / staged_query_lca adds the rows it returns."""
        self._ck(self.L.niqki_tally_begin(self.h))

    def tally_add(self, taxon, best_count=None, considered=None):
        """niqki_tally_add: rows (taxon, best_count, considered) as numpy arrays into the open tally; best_count None
        counts as zeros, considered None counts every TAXON_NONE row as a row without a hit."""
        t = np.ascontiguousarray(taxon, dtype=np.uint32).reshape(-1)
        rest = [None if x is None else np.ascontiguousarray(x, dtype=np.uint32).reshape(-1) for x in (best_count, considered)]
        if any(x is not None and x.size != t.size for x in rest):
            raise ValueError("tally_add: the arrays differ in length")
        self._ck(self.L.niqki_tally_add(self.h, _p(t) if t.size else None, *[_p(x) if t.size else None for x in rest], t.size, MEM_HOST))

    def tally_read(self):
        """niqki_tally_read: (direct, clade, direct_best, clade_best, totals), four uint64 arrays of one entry per taxon
        and totals as a dict (queries, classified, no_hit, no_common).  The tally stays open."""
        n = self.stat("taxa")
        outs = [np.zeros(n, dtype=np.uint64) for _ in range(4)]
        totals = TallyTotals()
        self._ck(self.L.niqki_tally_read(self.h, *[_p(a) if n else None for a in outs], C.byref(totals), MEM_HOST))
        return outs[0], outs[1], outs[2], outs[3], totals.as_dict()

    def tally_end(self):
        """niqki_tally_end: discards the tally; fine when none is open."""
        self._ck(self.L.niqki_tally_end(self.h))

    def retain(self, keep):
        """Drops the genomes whose keep flag (bool or uint8 array, one per genome) is zero: (n_kept, new_ids),
        new_ids[g] = the new id of old genome g (the kept genomes below it), 0xFFFFFFFF for a dropped one.  The handle
        then equals a fresh one holding the kept genomes in their old order."""
        k = np.ascontiguousarray(np.asarray(keep) != 0, dtype=np.uint8).reshape(-1)
        if k.size != self.n_genomes:
            raise ValueError("retain: %d keep flags for %d genomes" % (k.size, self.n_genomes))
        ids = np.empty(k.size, dtype=np.uint32)
        n = _u32(0)
        self._ck(self.L.niqki_retain(self.h, _p(k) if k.size else None, _p(ids) if k.size else None, C.byref(n), MEM_HOST))
        return int(n.value), ids

    def unite(self, labels):
        """niqki_unite: one entry per label, its sketch the per-slot minimum of the members' valid cells: (n_labels,
        new_ids), new_ids[g] = the number of g's label, labels numbered by first appearance.  labels: a uint32 per
        indexed genome as a numpy array, or a device tensor of 32-bit elements as in set_labels; new_ids is then a
        device tensor (int32, holding the same bits).  The handle then equals a fresh one holding the labels' sketches."""
        n = _u32(0)
        if hasattr(labels, "data_ptr"):
            if labels.element_size() != 4 or not labels.is_contiguous():
                raise ValueError("unite: a device tensor must be contiguous and hold 32-bit labels")
            import torch
            ids = torch.empty(int(labels.numel()), dtype=torch.int32, device=labels.device)
            self._ck(self.L.niqki_unite(self.h, _p(labels), int(labels.numel()), _p(ids), C.byref(n), MEM_DEVICE))
            return int(n.value), ids
        lab = np.ascontiguousarray(labels, dtype=np.uint32).reshape(-1)
        ids = np.empty(lab.size, dtype=np.uint32)
        self._ck(self.L.niqki_unite(self.h, _p(lab) if lab.size else None, lab.size, _p(ids) if lab.size else None,
                                    C.byref(n), MEM_HOST))
        return int(n.value), ids

    @property
    def register_bins(self):
        """NIQKI_REGISTER_BINS(H): 2^H register values and one bin for the cells that are not valid."""
        return (1 << self.H) + 1

    def registers(self, begin=0, end=None):
        """niqki_registers: the register histograms of genomes [begin, end) (end None: all), uint32 (end - begin,
        2^H + 1): column r counts the genome's valid cells whose top H bits are r, the last one its cells that are not
        valid.  size_estimate.estimate() turns a row into a number of distinct k-mers."""
        end = self.n_genomes if end is None else end
        out = np.zeros((max(end - begin, 0), self.register_bins), dtype=np.uint32)
        self._ck(self.L.niqki_registers(self.h, begin, end, _p(out) if out.size else None, MEM_HOST))
        return out

    def sketch_registers(self, sketches):
        """niqki_sketch_registers: the same histograms of the sketches given, int32 (n, 2^S)."""
        sk = np.ascontiguousarray(sketches, dtype=np.int32).reshape(-1, self.F)
        out = np.zeros((sk.shape[0], self.register_bins), dtype=np.uint32)
        self._ck(self.L.niqki_sketch_registers(self.h, _p(sk) if sk.size else None, sk.shape[0], _p(out) if out.size else None,
                                               MEM_HOST))
        return out

    def staged_registers(self):
        """niqki_staged_registers: the same histograms of the staged batch's sketches; the batch stays usable."""
        out = np.zeros((self._staged.n_entry, self.register_bins), dtype=np.uint32)
        self._ck(self.L.niqki_staged_registers(self.h, _p(out) if out.size else None, MEM_HOST))
        return out

    def registers_dev(self, hist, begin=0, end=None, sketches=None, n=None, staged=False):
        """The three register calls on device arrays, written in stream order.  hist: 32-bit elements, rows x (2^H + 1).
        sketches (with n): niqki_sketch_registers; staged: niqki_staged_registers; else niqki_registers of [begin, end)."""
        if sketches is not None:
            self._ck(self.L.niqki_sketch_registers(self.h, _p(sketches), int(n), _p(hist), MEM_DEVICE))
        elif staged:
            self._ck(self.L.niqki_staged_registers(self.h, _p(hist), MEM_DEVICE))
        else:
            self._ck(self.L.niqki_registers(self.h, begin, self.n_genomes if end is None else end, _p(hist), MEM_DEVICE))

    def get_sketches(self, begin, n):
        out = np.empty((n, self.F), dtype=np.int32)
        self._ck(self.L.niqki_get_sketches(self.h, begin, n, _p(out), MEM_HOST))
        return out

    def gathered(self, sketches):
        sk = np.ascontiguousarray(sketches, dtype=np.int32).reshape(-1, self.F)
        out = np.zeros(sk.shape[0], dtype=np.uint64)
        self._ck(self.L.niqki_query_gathered(self.h, _p(sk), sk.shape[0], _p(out), MEM_HOST))
        return out

    def export_dump(self):
        size = _u64(0)
        self._ck(self.L.niqki_export_dump(self.h, None, 0, C.byref(size)))
        buf = np.empty(size.value, dtype=np.uint8)
        self._ck(self.L.niqki_export_dump(self.h, _p(buf), buf.size, C.byref(size)))
        return buf.tobytes()

    def append_dump(self, data):
        """Appends the genomes of a dump (export_dump's bytes, names may follow) behind the handle's own: genome g of
        the dump becomes id n_genomes + g.  Returns the offset of the first name byte."""
        buf = np.frombuffer(data, dtype=np.uint8)
        consumed = _u64(0)
        self._ck(self.L.niqki_append_dump(self.h, _p(buf), buf.size, C.byref(consumed)))
        return consumed.value

    def append_begin(self, header):
        """Streaming append: the dump's 24-byte header; then append_slots in slot order (the last slot commits)."""
        hdr = np.frombuffer(bytes(header[:24]), dtype=np.uint8)
        self._ck(self.L.niqki_append_begin(self.h, _p(hdr)))

    def append_slots(self, slot_begin, slot_end, data):
        """The payload bytes of whole slots [slot_begin, slot_end); returns the bytes used."""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        used = _u64(0)
        self._ck(self.L.niqki_append_slots(self.h, slot_begin, slot_end, _p(buf) if buf.size else None, buf.size, C.byref(used)))
        return used.value

    def append_cancel(self):
        self._ck(self.L.niqki_append_cancel(self.h))

    @classmethod
    def import_dump(cls, data, device=-1, tile_genomes=0, resident_mib=0, top_k=0):
        L = lib()
        buf = np.frombuffer(data, dtype=np.uint8)
        p = Params(31, 15, 12, 4, 0, 0, 0, device, tile_genomes, resident_mib, top_k)
        h = _vp()
        consumed = _u64(0)
        rc = L.niqki_import_dump(C.byref(p), _p(buf), buf.size, C.byref(consumed), C.byref(h))
        if rc:
            raise NiqkiError(rc, L.niqki_status_string(rc).decode())
        e = cls(_handle=h)
        e.names_offset = consumed.value
        return e

    # -- profiling
    def profile(self, on=True):
        self._ck(self.L.niqki_profile_enable(self.h, 1 if on else 0))

    def profile_reset(self):
        self._ck(self.L.niqki_profile_reset(self.h))

    def profile_read(self, kc):
        ms, n = _dbl(0), _u64(0)
        self._ck(self.L.niqki_profile_read(self.h, kc, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # -- raw device-pointer calls (torch tensors or addresses)
    def synth_dev(self, seed, family, member, rate14, n, length, stride, out):
        self._ck(self.L.niqki_synth_genomes(self.h, seed, _p(family), _p(member), _p(rate14), n,
                                            length, stride, _p(out), MEM_DEVICE))

    def synth_reads_dev(self, seed, family, member, rate14, offset, read_id, read_rate14, n, length, stride, out):
        self._ck(self.L.niqki_synth_reads(self.h, seed, _p(family), _p(member), _p(rate14), _p(offset), _p(read_id),
                                          read_rate14, n, length, stride, _p(out), MEM_DEVICE))

    def synth_reads_host(self, seed, family, member, rate14, offset, read_id, read_rate14, length):
        a = [np.ascontiguousarray(x, dtype=np.uint32) for x in (family, member, rate14, read_id)]
        off = np.ascontiguousarray(offset, dtype=np.uint64)
        out = np.empty((a[0].size, length), dtype=np.uint8)
        self._ck(self.L.niqki_synth_reads(self.h, seed, _p(a[0]), _p(a[1]), _p(a[2]), _p(off), _p(a[3]), read_rate14,
                                          a[0].size, length, length, _p(out), MEM_HOST))
        return out

    def measure_alu(self, what, ms=20.0):
        r = _dbl(0)
        self._ck(self.L.niqki_measure_alu(self.h, what, ms, C.byref(r)))
        return r.value

    def stage_raw_dev(self, raw, file_off, types, lines=False, final=True, max_entries=16384):
        """raw: device bytes (torch tensor / address); file_off, types: host numpy arrays."""
        off = np.ascontiguousarray(file_off, dtype=np.uint64)
        ty = np.ascontiguousarray(types, dtype=np.uint8)
        b = RawBatch(_p(raw), None, _p(off), _p(ty), off.size - 1, int(bool(lines)), int(bool(final)), max_entries)
        info = StageInfo()
        hdr = np.zeros(max(max_entries, 1), dtype=np.uint64)
        self._ck(self.L.niqki_stage_raw(self.h, C.byref(b), MEM_DEVICE, C.byref(info), _p(hdr) if lines else None))
        self._staged = info
        return info, hdr[:info.n_entry] if lines else None

    def sketch_dev(self, seqs, rec_off, n_rec, sketches, entry_rec=None, n_entry=None):
        self._ck(self.L.niqki_sketch(self.h, _p(seqs), _p(rec_off), n_rec, _p(entry_rec),
                                     n_rec if n_entry is None else n_entry, _p(sketches), MEM_DEVICE))

    def densify_dev(self, sketches, n):
        """niqki_densify in place on n rows of device memory (on the handle's stream)."""
        self._ck(self.L.niqki_densify(self.h, _p(sketches), n, MEM_DEVICE))

    def insert_dev(self, sketches, n):
        self._ck(self.L.niqki_insert(self.h, _p(sketches), n, MEM_DEVICE))

    def query_counts_dev(self, sketches, nq, counts, stride):
        self._ck(self.L.niqki_query_counts(self.h, _p(sketches), nq, _p(counts), stride, MEM_DEVICE))

    def hits_from_counts_dev(self, counts, nq, stride, gid_begin, n_gids, hit_off, hc, hg, capacity):
        self._ck(self.L.niqki_hits_from_counts(self.h, _p(counts), nq, stride, gid_begin, n_gids,
                                               _p(hit_off), _p(hc), _p(hg), capacity, MEM_DEVICE))

    def candidates_dev(self, counts, nq, stride, n_gids, threshold, cap, cand, n_cand):
        self._ck(self.L.niqki_candidates_from_counts(self.h, _p(counts), nq, stride, n_gids, threshold, cap,
                                                     _p(cand), _p(n_cand), MEM_DEVICE))

    def query_counts_candidates_dev(self, sketches, nq, counts, stride, threshold, cap, cand, n_cand):
        self._ck(self.L.niqki_query_counts_candidates(self.h, _p(sketches), nq, _p(counts), stride, threshold, cap,
                                                      _p(cand), _p(n_cand), MEM_DEVICE))

    def query_survivors_dev(self, sketches, nq, cand_thr, surv_thr, cand_cap, surv_cap, cand, n_cand, surv, n_surv):
        self._ck(self.L.niqki_query_survivors(self.h, _p(sketches), nq, cand_thr, surv_thr, cand_cap, surv_cap, _p(cand),
                                              _p(n_cand), _p(surv), _p(n_surv), MEM_DEVICE))

    def survivor_counts_dev(self, sketches, nq, ids, m, surv, n_surv, surv_cap, counts):
        self._ck(self.L.niqki_survivor_counts(self.h, _p(sketches), nq, _p(ids), m, _p(surv), _p(n_surv), surv_cap,
                                              _p(counts), MEM_DEVICE))

    def hits_from_candidates_dev(self, ids, totals, nq, m, hit_off, hc, hg, capacity):
        self._ck(self.L.niqki_hits_from_candidates(self.h, _p(ids), _p(totals), nq, m, _p(hit_off), _p(hc), _p(hg),
                                                   capacity, MEM_DEVICE))

    def query_dev(self, sketches, nq, hit_off, hc, hg, capacity):
        self._ck(self.L.niqki_query(self.h, _p(sketches), nq, _p(hit_off), _p(hc), _p(hg), capacity,
                                    MEM_DEVICE))

    def cover_dev(self, sketches, nq, max_picks, hit_off, hc, hg, ht, capacity):
        """niqki_cover on device arrays (ht may be None); returns the status: 0, or E_CAPACITY with the true total in
        hit_off[nq] and nothing else written."""
        return self._ck(self.L.niqki_cover(self.h, _p(sketches), nq, int(max_picks), _p(hit_off), _p(hc), _p(hg), _p(ht),
                                           capacity, MEM_DEVICE), allow=(E_CAPACITY,))

    def query_collapsed_dev(self, sketches, nq, hit_off, hc, hg, hm, capacity):
        """niqki_query_collapsed on device arrays (hm may be None); returns the status: 0, or E_CAPACITY with the true
        total in hit_off[nq] and nothing else written."""
        return self._ck(self.L.niqki_query_collapsed(self.h, _p(sketches), nq, _p(hit_off), _p(hc), _p(hg), _p(hm),
                                                     capacity, MEM_DEVICE), allow=(E_CAPACITY,))

    def query_contained_dev(self, sketches, qsizes, nq, mode, min_share, hit_off, hs, hc, hg, nu, capacity):
        """niqki_query_contained on device arrays (qsizes: 64-bit elements; nu may be None); returns the status: 0, or
        E_CAPACITY with the true total in hit_off[nq]."""
        return self._ck(self.L.niqki_query_contained(self.h, _p(sketches), _p(qsizes), nq, int(mode), int(min_share), _p(hit_off),
                                                     _p(hs), _p(hc), _p(hg), _p(nu), capacity, MEM_DEVICE), allow=(E_CAPACITY,))

    def query_lca_dev(self, sketches, nq, top_permille, taxon, best_count=None, best_gid=None, considered=None):
        """niqki_query_lca on device arrays (each of the last three may be None), written in stream order."""
        self._ck(self.L.niqki_query_lca(self.h, _p(sketches), nq, int(top_permille), _p(taxon), _p(best_count), _p(best_gid),
                                        _p(considered), MEM_DEVICE))

    def audit_dev(self, threshold, k, verdict=None, own_count=None, own_gid=None, other_count=None, other_gid=None,
                  vote_gid=None, vote_n=None):
        """niqki_audit on device arrays of n_genomes 32-bit elements (each may be None), written in stream order."""
        self._ck(self.L.niqki_audit(self.h, int(threshold), int(k), _p(verdict), _p(own_count), _p(own_gid), _p(other_count),
                                    _p(other_gid), _p(vote_gid), _p(vote_n), MEM_DEVICE))

    def tally_add_dev(self, taxon, best_count, considered, n):
        """niqki_tally_add on device arrays of 32-bit elements (the last two may be None), read in stream order; bad
        rows among them are reported by the next read."""
        self._ck(self.L.niqki_tally_add(self.h, _p(taxon), _p(best_count), _p(considered), n, MEM_DEVICE))

    def tally_read_dev(self, direct=None, clade=None, direct_best=None, clade_best=None):
        """niqki_tally_read into device tensors of 64-bit elements, one per taxon (each may be None); returns totals."""
        totals = TallyTotals()
        self._ck(self.L.niqki_tally_read(self.h, _p(direct), _p(clade), _p(direct_best), _p(clade_best), C.byref(totals), MEM_DEVICE))
        return totals.as_dict()

    def query_sequences_dev(self, seqs, rec_off, n, hit_off, hc, hg, capacity):
        self._ck(self.L.niqki_query_sequences(self.h, _p(seqs), _p(rec_off), n, None, n, _p(hit_off),
                                              _p(hc), _p(hg), capacity, MEM_DEVICE))

    def sketch_ahead_dev(self, seqs, rec_off, n_rec, entry_rec=None, n_entry=None):
        """niqki_sketch_ahead: the batch's sketch kernel on the handle's sketch lane, beside what its stream runs."""
        self._ck(self.L.niqki_sketch_ahead(self.h, _p(seqs), _p(rec_off), n_rec, _p(entry_rec),
                                           n_rec if n_entry is None else n_entry, MEM_DEVICE))

    def query_ahead_dev(self, hit_off, hc, hg, capacity, sketches=None):
        """niqki_query_ahead with device outputs: the oldest batch sketched ahead; returns its entry count."""
        n = _u32(0)
        self._ck(self.L.niqki_query_ahead(self.h, C.byref(n), _p(hit_off), _p(hc), _p(hg), capacity, _p(sketches), MEM_DEVICE))
        return n.value

    def query_ahead(self, n_entry, capacity=None, want_sketches=False):
        """niqki_query_ahead with host outputs: (off, counts, gids[, sketches]) of the oldest batch sketched ahead
        (n_entry: its entry count, as given to sketch_ahead_dev)."""
        n = _u32(0)
        cap = capacity if capacity is not None else max(1024, n_entry * 64)
        while True:
            off = np.zeros(n_entry + 1, dtype=np.uint64)
            hc, hg = np.empty(max(cap, 1), dtype=np.uint32), np.empty(max(cap, 1), dtype=np.uint32)
            sk = np.empty((n_entry, self.F), dtype=np.int32) if want_sketches else None
            rc = self.L.niqki_query_ahead(self.h, C.byref(n), _p(off), _p(hc), _p(hg), cap, _p(sk), MEM_HOST)
            self._ck(rc, allow=(E_CAPACITY,))
            if rc == 0:
                tot = int(off[n.value])
                res = (off[:n.value + 1], hc[:tot], hg[:tot])
                return res + (sk[:n.value],) if want_sketches else res
            cap = int(off[n.value])

    def gathered_dev(self, sketches, nq):
        out = np.zeros(nq, dtype=np.uint64)
        self._ck(self.L.niqki_query_gathered(self.h, _p(sketches), nq, _p(out), MEM_DEVICE))
        return out


def group_slot_range(rank, world, S):
    b, e = _u32(0), _u32(0)
    lib().niqki_group_slot_range(rank, world, S, C.byref(b), C.byref(e))
    return b.value, e.value


def group_plan(world, S, min_score, exchange_option, per, n_genomes, cand_cap):
    """niqki_group_plan_batch: the decisions and sizes of one query batch of a group (pure arithmetic: no GPU)."""
    p = GroupPlan()
    rc = lib().niqki_group_plan_batch(world, S, min_score, exchange_option, per, n_genomes, cand_cap, C.byref(p))
    if rc:
        raise NiqkiError(rc, "niqki_group_plan_batch: invalid arguments")
    return p


def group_new_id():
    """128 opaque bytes naming a group about to be formed (rank 0 makes them, the caller carries
    them to the other processes)."""
    buf = np.zeros(GROUP_ID_BYTES, dtype=np.uint8)
    rc = lib().niqki_group_new_id(buf.ctypes.data)
    if rc:
        raise NiqkiError(rc, "niqki_group_new_id: " + lib().niqki_status_string(rc).decode())
    return buf


class Group:
    """The ranks of a slot-sharded index that live in this process (niqki_group_*):
    engines[i] is rank first_rank + i, created with group_slot_range(rank, world, S)."""

    def __init__(self, engines, first_rank=0, world=None, group_id=None):
        self.L = lib()
        self.engines = list(engines)
        self.n_local = len(self.engines)
        self.first = first_rank
        self.world = self.n_local if world is None else world
        hs = (_vp * self.n_local)(*[e.h for e in self.engines])
        idp = None if group_id is None else np.ascontiguousarray(group_id, dtype=np.uint8).ctypes.data
        g = _vp()
        rc = self.L.niqki_group_create(C.cast(hs, _vp), self.n_local, first_rank, self.world, idp, C.byref(g))
        if rc:
            raise NiqkiError(rc, "%s (%s)" % (self.L.niqki_status_string(rc).decode(),
                                              self.L.niqki_last_error(self.engines[0].h).decode()))
        self.g = g

    def close(self):
        if getattr(self, "g", None):
            self.L.niqki_group_destroy(self.g)
            self.g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, allow=()):
        if rc and rc not in allow:
            raise NiqkiError(rc, "%s (%s)" % (self.L.niqki_status_string(rc).decode(),
                                              self.L.niqki_group_last_error(self.g).decode()))
        return rc

    def set_option(self, key, value):
        self._ck(self.L.niqki_group_set_option(self.g, key.encode(), int(value)))

    def stat(self, key):
        v = _u64(0)
        self._ck(self.L.niqki_group_get_stat(self.g, key.encode(), C.byref(v)))
        return v.value

    def _ptrs(self, xs):
        return C.cast((_vp * self.n_local)(*[_p(x) for x in xs]), _vp)

    def insert_dev(self, local_sketches, per, n_total):
        """local_sketches: per local rank a device tensor / address of per x F int32."""
        self._ck(self.L.niqki_group_insert(self.g, self._ptrs(local_sketches), per, n_total))

    def query_dev(self, local_sketches, per, hit_off, hit_counts, hit_gids, capacity):
        """Per-rank device outputs (torch tensors / addresses): hit_off[i] int64 [per+1]."""
        self._ck(self.L.niqki_group_query(self.g, self._ptrs(local_sketches), per, self._ptrs(hit_off),
                                          self._ptrs(hit_counts), self._ptrs(hit_gids), capacity, MEM_DEVICE))

    def query_begin_dev(self, local_sketches, per, hit_off, hit_counts, hit_gids, capacity):
        """niqki_group_query_begin with device outputs: returns without waiting for the device."""
        self._ck(self.L.niqki_group_query_begin(self.g, self._ptrs(local_sketches), per, self._ptrs(hit_off),
                                                self._ptrs(hit_counts), self._ptrs(hit_gids), capacity, MEM_DEVICE))

    def query_end(self):
        self._ck(self.L.niqki_group_query_end(self.g))

    def query(self, local_sketches, per, capacity=None):
        """Device sketches in, numpy hits out: list of (off, counts, gids) per local rank."""
        cap = capacity if capacity is not None else max(1024, per * 64)
        while True:
            off = [np.zeros(per + 1, dtype=np.uint64) for _ in range(self.n_local)]
            hc = [np.empty(max(cap, 1), dtype=np.uint32) for _ in range(self.n_local)]
            hg = [np.empty(max(cap, 1), dtype=np.uint32) for _ in range(self.n_local)]
            rc = self.L.niqki_group_query(self.g, self._ptrs(local_sketches), per, self._ptrs(off), self._ptrs(hc),
                                          self._ptrs(hg), cap, MEM_HOST)
            self._ck(rc, allow=(E_CAPACITY,))
            if rc == 0:
                return [(o, c[:int(o[per])], g_[:int(o[per])]) for o, c, g_ in zip(off, hc, hg)]
            cap = max(int(o[per]) for o in off)
