"""GPU: every key niqki_get_stat knows answers on a fresh handle, the per-call stats with 0, and a key it does not know
is refused -- a prefix of a real key included.  The list is typed out here, not read from the library."""
import ctypes as C

import pytest

from test_gpu_cluster import S, W

pytestmark = pytest.mark.gpu

E_INVALID = 1

HANDLE_KEYS = [
    "store_bytes", "index_bytes", "delta_genomes", "tiles", "class_mask", "last_gather_form", "last_gather_kernel", "last_densify_form",
    "bucket_align_log2", "last_hits_form", "labels", "taxa", "taxonomy_depth", "retain_us_rank", "retain_us_compact",
    "inflate_files_in_flight", "inflate_files_in_flight_8k", "page_slots", "pages",
]

CALL_KEYS = [
    "cluster_splits", "cluster_us_read", "cluster_us_hits", "cluster_us_link", "cluster_us_flatten", "cluster_pairs",
    "derep_rounds", "derep_splits", "derep_us_read", "derep_us_hits", "derep_us_decide", "derep_us_assign", "derep_pairs",
    "linkage_rounds", "linkage_splits", "linkage_us_read", "linkage_us_hits", "linkage_us_forest", "linkage_us_finish",
    "linkage_pairs",
    "cover_rounds", "cover_picks", "cover_recount_mismatches", "cover_us_hits", "cover_us_pick", "cover_us_compact",
    "cover_us_finish",
    "collapse_splits", "collapse_long_lists", "collapse_us_hits", "collapse_us_first", "collapse_us_emit",
    "lca_splits", "lca_long_lists", "lca_no_common", "lca_us_hits", "lca_us_fold",
]


def test_every_stat_key_answers_on_a_fresh_handle(native):
    assert len(set(HANDLE_KEYS + CALL_KEYS)) == len(HANDLE_KEYS) + len(CALL_KEYS) == 56
    e = native.Engine(K=31, S=S, W=W, H=3, min_score_value=50, tile_genomes=0, resident_mib=0, top_k=0)
    v = C.c_uint64(0)
    for key in HANDLE_KEYS + CALL_KEYS:
        v.value = 0xDEAD
        assert e.L.niqki_get_stat(e.h, key.encode(), C.byref(v)) == 0, key
        assert v.value != 0xDEAD, key                  # (written)
        if key in CALL_KEYS or key in ("labels", "taxa", "taxonomy_depth"):
            assert v.value == 0, key
    for key in ("no_such_key", "cluster_split", ""):
        v.value = 0xDEAD
        assert e.L.niqki_get_stat(e.h, key.encode(), C.byref(v)) == E_INVALID, key
        assert v.value == 0xDEAD
    e.close()
