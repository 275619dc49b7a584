"""What every entry point of the C ABI that takes a context (ku_ctx *) or a group (ku_mgpu *) first does while batches of
ku_classify_batch_rle_enqueue are in flight on that context -- or, for a group, on any of its rank contexts.

  refuse   KU_ESTATE with no side effect: the run's state is unchanged, no buffer is freed, reallocated or written
  wait     returns only once all of the context's work is complete, on every one of its streams
  allowed  a query (or the two steps themselves) that stays correct while batches run

A plain module, not a fixture file: tests/test_abi_host.py holds it against include/krakenuniq_amd.h (every such prototype
has exactly one row, every row names a prototype), tests/test_gpu_inflight.py against the library.  A new entry point fails
the CPU suite until its row is written here."""

REFUSE, WAIT, ALLOWED = "refuse", "wait", "allowed"

# name -> (behaviour, one-line reason)
CONTRACT = {
    # ---- context: database and taxonomy (they free and rebuild what running kernels read)
    "ku_ctx_load_db": (REFUSE, "frees the resident shard and the taxonomy"),
    "ku_ctx_adopt_db": (REFUSE, "frees the resident shard and the taxonomy"),
    "ku_ctx_add_db": (REFUSE, "appends a store the kernels would search"),
    "ku_ctx_set_taxonomy": (REFUSE, "replaces the slot tables and the per-taxon state"),
    "ku_ctx_swap_shard": (REFUSE, "frees the resident shard"),
    "ku_ctx_prefetch_shard": (REFUSE, "a chunk swap cannot follow while batches run; same rule as swap_shard"),
    # ---- context: per-taxon state
    "ku_ctx_enable_exact": (REFUSE, "reallocates the exact set"),
    "ku_counts_export_exact": (REFUSE, "reads counters the batches still write"),
    "ku_ctx_reset_counts": (REFUSE, "zeroes counters the batches still write"),
    "ku_counts_export": (REFUSE, "reads counters the batches still write"),
    "ku_ctx_merge_state": (REFUSE, "either side: src's counters are still written, dst's too"),
    "ku_ctx_report": (REFUSE, "reads the state and closes the open work unit"),
    "ku_ctx_report_cols": (REFUSE, "reads the state and closes the open work unit"),
    "ku_ctx_replace_calls": (REFUSE, "moves read counts of the batch finished last"),
    # ---- context: sparse-sketch emulation
    "ku_ctx_enable_sparse": (REFUSE, "reallocates the emulation's tables"),
    "ku_ctx_disable_sparse": (REFUSE, "frees the emulation's tables"),
    "ku_sparse_close_unit": (REFUSE, "closes the unit the batches in flight continue"),
    "ku_sparse_export": (REFUSE, "closes the open unit and reads the run-wide set"),
    "ku_ctx_sparse_state": (ALLOWED, "a host flag"),
    # ---- context: classification on host buffers
    "ku_classify_batch": (REFUSE, "shares the context's scratch and the open work unit"),
    "ku_classify_batch_rle": (REFUSE, "shares the context's scratch and the open work unit"),
    "ku_classify_batch_rle_reserve": (REFUSE, "grows the jobs' buffers and runs warm-up batches"),
    "ku_classify_batch_rle_enqueue": (ALLOWED, "the first step itself (KU_ESTATE only past KU_RLE_MAX_IN_FLIGHT)"),
    "ku_classify_batch_rle_finish": (ALLOWED, "the second step itself"),
    "ku_classify_batch_rle_copied": (ALLOWED, "a host counter of the batch finished last"),
    "ku_classify_batch_rle_in_flight": (ALLOWED, "a host counter"),
    "ku_fetch_runs": (ALLOWED, "the runs of the batch finished last, as documented"),
    # ---- context: device-buffer and staged entry points
    "ku_classify_batch_device": (REFUSE, "writes the per-taxon state and the context's scratch"),
    "ku_classify_batch_device_rle": (REFUSE, "writes the per-taxon state"),
    "ku_device_rle_runs_cap": (ALLOWED, "arithmetic on the arguments"),
    "ku_lookup_device": (REFUSE, "writes the per-taxon state"),
    "ku_resolve_device": (REFUSE, "writes the read counts"),
    "ku_lookup_stats_device": (REFUSE, "uses the context's scalars"),
    # ---- context: out-of-core runs
    "ku_batch_create": (REFUSE, "uploads on the context's stream for a run that swaps shards"),
    "ku_batch_lookup": (REFUSE, "writes the per-taxon state"),
    "ku_batch_finish": (REFUSE, "writes the per-taxon state and the context's scratch"),
    "ku_batch_absorb": (REFUSE, "uses the context's scratch"),
    "ku_ctx_mem_info": (ALLOWED, "hipMemGetInfo"),
    # ---- context: queries
    "ku_ctx_db_layout": (ALLOWED, "host fields"),
    "ku_ctx_db_values": (ALLOWED, "host copy of the shard's values"),
    "ku_ctx_count_taxons": (ALLOWED, "reads the database only, which the batches do not write"),
    "ku_ctx_count_taxons_db": (ALLOWED, "reads the database only, which the batches do not write"),
    "ku_counts_dims_get": (ALLOWED, "host fields"),
    "ku_counts_device_ptrs": (ALLOWED, "pointers only"),
    # ---- context: life cycle
    "ku_ctx_synchronize": (WAIT, "every stream of the context; _finish still settles each batch"),
    "ku_ctx_destroy": (WAIT, "every stream of the context before anything is freed"),
    # ---- group (checked over every rank context before any rank starts)
    "ku_mgpu_destroy": (WAIT, "through ku_ctx_synchronize / ku_ctx_destroy of every rank"),
    "ku_mgpu_load": (REFUSE, "loads every rank"),
    "ku_mgpu_load_dbs": (REFUSE, "loads every rank"),
    "ku_mgpu_set_taxonomy": (REFUSE, "sets every rank's taxonomy"),
    "ku_mgpu_enable_sparse": (REFUSE, "enables the emulation on every rank"),
    "ku_mgpu_sparse_close_unit": (REFUSE, "closes a rank's open unit"),
    "ku_mgpu_enable_exact": (REFUSE, "reallocates every rank's exact set"),
    "ku_mgpu_classify_batch_rle": (REFUSE, "classifies on every rank"),
    "ku_mgpu_step_device": (REFUSE, "classifies on every rank"),
    "ku_mgpu_reduce_state": (REFUSE, "reduces the ranks' counters in place"),
    "ku_mgpu_ctx": (ALLOWED, "a pointer"),
    "ku_mgpu_uses_rccl": (ALLOWED, "a host flag"),
    "ku_mgpu_uses_routing": (ALLOWED, "a host flag"),
    "ku_mgpu_set_timing": (ALLOWED, "a host flag for later steps"),
    "ku_mgpu_step_times": (ALLOWED, "events of the group's last step"),
    "ku_mgpu_sparse_state": (ALLOWED, "host flags"),
    "ku_mgpu_fetch_runs": (ALLOWED, "the runs of the group's last batch"),
    "ku_mgpu_count_taxons": (ALLOWED, "ku_ctx_count_taxons summed"),
}


def rows(behaviour):
    return sorted(n for n, (b, _) in CONTRACT.items() if b == behaviour)
