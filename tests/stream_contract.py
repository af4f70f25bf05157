"""The stream contract of the QGTC surface, one line per public name ("Streams and graph capture"). Every name is in
exactly one class, decided by reading the binding (qgtc_torch.cpp), tiled.py and the C entries behind them, not by trying it:

  ASYNC  enqueues on ``torch.cuda.current_stream()`` of the operands' device and returns; no host read, no other stream. After ONE
         warm-up call (kernel handles, the dynamic-LDS opt-in, the violation record's first-use allocation, lazy adjacency caches)
         it can be captured into a graph.
  FORKS  asynchronous too, but records an event on the current stream, launches on the binding's per-device pool streams and makes the
         current stream wait for them. Never inside a capture.
  HOST   synchronises with the host: reads a result back (``.item()``, ``.cpu()``, hipMemcpy, hipEventSynchronize,
         hipStreamSynchronize) or uploads from pageable memory. Never capturable.
  PURE   host only: switches, counters, constants, attribute reads, constructors that only check and keep references.

tests/test_stream_contract.py (no GPU) fails when a name the extension or the Python layer exports is missing here, or when this table
names something that is gone. tests/stream_cases.py holds the cases of the GPU tests and is keyed by these names, so an ASYNC or FORKS
entry cannot exist without an ordering probe (and, ASYNC, a capture test).
"""
ASYNC, FORKS, HOST, PURE = "async", "forks", "host", "pure"

# name -> (class, why).  "QGTC.x": the module's names; "QGTC.C.m": a class's; "ext._x": the private entries tiled.py wraps.
CONTRACT = {
    # ---- the reference's eight operators, their checked (pybind11) twins and aliases -------------------------------------------------
    "QGTC.val2bit": (ASYNC, "lean path: hipMemsetAsync + atomic-OR kernel (rows) or one kernel (cols), both on the current stream"),
    "QGTC.checked_val2bit": (ASYNC, "the pybind11 path of val2bit: device guard, then the same entry on current_stream(input)"),
    "QGTC.bit_qnt": (ASYNC, "alias of val2bit"),
    "QGTC.bit2val": (ASYNC, "one kernel on current_stream(input)"),
    "QGTC.bitMM2Bit": (ASYNC, "lean path: qgtc_bitmm2bit on getCurrentHIPStream(current device)"),
    "QGTC.bitMM2Bit_col": (ASYNC, "lean path, QGTC_OUT_COLS"),
    "QGTC.bitMM2Int": (ASYNC, "lean path: qgtc_bitmm2int"),
    "QGTC.checked_bitMM2Bit": (ASYNC, "mm2bit_impl: device guard, current_stream(bit_X1)"),
    "QGTC.checked_bitMM2Bit_col": (ASYNC, "mm2bit_impl with cols"),
    "QGTC.checked_bitMM2Int": (ASYNC, "pybind11 bitMM2Int: device guard, current_stream(bit_X1)"),
    "QGTC.mm_v1": (ASYNC, "alias of bitMM2Bit"),
    "QGTC.mm_v2": (ASYNC, "alias of bitMM2Int"),
    "QGTC.bitMM2Bit_profile": (HOST, "hipEventSynchronize around 200 launches"),
    "QGTC.bitMM2Bit_base_cnt": (HOST, "tile_counters: buf.cpu()"),
    "QGTC.bitMM2Bit_zerojump_cnt": (HOST, "tile_counters: buf.cpu()"),
    # ---- additive operators ----------------------------------------------------------------------------------------------------------
    "QGTC.bitMM2Bit_enqueue": (ASYNC, "reps launches into a caller's buffer on current_stream(bit_X1)"),
    "QGTC.bitMM2Bit_enqueue_streams": (FORKS, "event fork / join over side_streams(device, len(outs))"),
    "QGTC.gcn_layer": (ASYNC, "two mm launches on the current stream"),
    "QGTC.val2bit_many": (ASYNC, "one kernel (jobs passed by value) on current_stream(inputs[0])"),
    "QGTC.i8gemm": (ASYNC, "one kernel on current_stream(A)"),
    "QGTC.tile_occupancy": (ASYNC, "one kernel on current_stream(x); the bitmap stays on the device"),
    "QGTC.tiledMM2Bit": (ASYNC, "ext._tiled_mm / _tiled_mm_t on a warmed adjacency"),
    "QGTC.tiledMM2Int": (ASYNC, "ext._tiled_mm / _tiled_mm_t, to_float"),
    "QGTC.tiledMMFloat": (ASYNC, "ext._tiled_mm_f32 / _t / _src / _t_src"),
    "QGTC.tiledAggregate": (ASYNC, "tiledMMFloat forward; the backward is tiledMMFloat on adj.T (built on first use, on the stream "
                                   "autograd runs the backward on)"),
    "QGTC.profile": (HOST, "hipEventSynchronize"),
    "QGTC.i8gemm_profile": (HOST, "hipEventSynchronize"),
    "QGTC.host_parts": (HOST, "hipDeviceSynchronize between its timed pieces"),
    "QGTC.tile_counters": (HOST, "buf.cpu()"),
    "QGTC.last_batched_violation": (HOST, "hipStreamSynchronize + hipMemcpy of the violation record"),
    "QGTC.pack_edges": (HOST, "validate: bad.item(); nbits > 1: min / max .item() and unique. (validate=False, nbits=1 is asynchronous "
                              "on the current stream: probed through qgtc_pack_edge_list's sibling qgtc_pack_edges in the raw-entry tests)"),
    "QGTC.pack_edges_tiled": (HOST, "ext._tiled_pack reads the tile count back"),
    "QGTC.reorder_nodes": (HOST, "ext._reorder_nodes: validate reads bad_index back"),
    "QGTC.add_self_loops": (HOST, "boolean-mask indexing: torch reads the kept count back"),
    # ---- switches, counters, constants -----------------------------------------------------------------------------------------------
    "QGTC.set_engine": (PURE, "atomic switch"), "QGTC.get_engine": (PURE, "atomic switch"),
    "QGTC.set_zero_skip": (PURE, "atomic switch"), "QGTC.get_zero_skip": (PURE, "atomic switch"),
    "QGTC.get_counters": (PURE, "host counters"), "QGTC.reset_counters": (PURE, "host counters"),
    "QGTC.last_profile_ms": (PURE, "host value"), "QGTC.abi_version": (PURE, "constant"),
    "QGTC.SRC_A": (PURE, "constant"), "QGTC.SRC_X": (PURE, "constant"), "QGTC.SRC_XR": (PURE, "constant"),
    "QGTC.SRC_XC": (PURE, "constant"), "QGTC.SRC_AT": (PURE, "constant"), "QGTC.SRC_WEIGHT": (PURE, "constant"),
    "QGTC.SRC_STAGE": (PURE, "constant"), "QGTC.DIM_NODES": (PURE, "constant"), "QGTC.CHAIN_DISCARD": (PURE, "constant"),
    # ---- BatchedGemm -----------------------------------------------------------------------------------------------------------------
    "QGTC.BatchedGemm": (HOST, "the constructor uploads the descriptors from pageable host memory (host.to(dev))"),
    "QGTC.BatchedGemm.run": (ASYNC, "qgtc_bitmm_batched on current_stream(descs)"),
    "QGTC.BatchedGemm.run_per_problem": (FORKS, "event fork / join over side_streams(device, n_streams)"),
    "QGTC.BatchedGemm.occupied_fraction": (HOST, "stats.cpu()"),
    "QGTC.BatchedGemm.zero_jump": (HOST, "occupied_fraction"),
    "QGTC.BatchedGemm.outs": (PURE, "attribute"), "QGTC.BatchedGemm.occs": (PURE, "attribute"), "QGTC.BatchedGemm.count": (PURE, "attribute"),
    # ---- FusedLayer, ChainedPair -----------------------------------------------------------------------------------------------------
    "QGTC.FusedLayer": (PURE, "the constructor checks host copies of the descriptors"),
    "QGTC.FusedLayer.run": (ASYNC, "qgtc_gcn_layer_batched on current_stream(descs)"),
    "QGTC.FusedLayer.outs": (PURE, "attribute"),
    "QGTC.ChainedPair": (PURE, "the constructor checks host copies of the descriptors"),
    "QGTC.ChainedPair.run": (ASYNC, "qgtc_gcn_chain_batched on current_stream(descs)"),
    "QGTC.ChainedPair.outs": (PURE, "attribute"), "QGTC.ChainedPair.discard": (PURE, "attribute"),
    # ---- EpochPlan -------------------------------------------------------------------------------------------------------------------
    "QGTC.EpochPlan": (HOST, "the constructor uploads the batch table from pageable memory and reads the occupancy count back"),
    "QGTC.EpochPlan.load": (HOST, "reads the occupied-tile count (and bad_index) back"),
    "QGTC.EpochPlan.bind": (ASYNC, "qgtc_expand_weights + qgtc_epoch_plan_fill (arguments by value) on the current stream; the first "
                                   "bind of a process allocates the violation record (hipMalloc + hipMemcpy): the warm-up"),
    "QGTC.EpochPlan.run": (ASYNC, "every launch of the plan on current_stream(descs)"),
    "QGTC.EpochPlan.run_launch": (ASYNC, "one launch of the plan on current_stream(descs)"),
    "QGTC.EpochPlan.run_checked": (HOST, "qgtc_last_batched_violation"),
    "QGTC.EpochPlan.outs": (HOST, "the first call after a bind reads the fill kernel's violation record"),
    "QGTC.EpochPlan.format_of": (PURE, "a non-owning view"),
    "QGTC.EpochPlan.As": (PURE, "views"), "QGTC.EpochPlan.Xs": (PURE, "views"), "QGTC.EpochPlan.Xrs": (PURE, "views"),
    "QGTC.EpochPlan.count": (PURE, "attribute"), "QGTC.EpochPlan.zero_jump": (PURE, "attribute"), "QGTC.EpochPlan.x_chain": (PURE, "attribute"),
    "QGTC.EpochPlan.a_tiles": (PURE, "attribute"), "QGTC.EpochPlan.occupied_fraction": (PURE, "read back by the constructor"),
    "QGTC.EpochPlan.n_launches": (PURE, "attribute"),
    # ---- TiledAdjacency (tiled.py) ---------------------------------------------------------------------------------------------------
    "QGTC.TiledAdjacency": (PURE, "the constructor keeps references"),
    "QGTC.TiledAdjacency.T": (ASYNC, "first use: ext._tiled_colindex on the current stream, cached; later uses are attribute reads"),
    "QGTC.TiledAdjacency.degrees": (ASYNC, "first use: ext._tiled_degrees on the current stream, cached for both views"),
    "QGTC.TiledAdjacency.mean_scale": (ASYNC, "the same cache as degrees()"),
    "QGTC.TiledAdjacency.sym_scale": (ASYNC, "first use: degrees, then ext._tiled_inv_sqrt_degree twice on the current stream, cached"),
    "QGTC.TiledAdjacency.to_new": (ASYNC, "index_select on the current stream"),
    "QGTC.TiledAdjacency.to_old": (ASYNC, "index_select on the current stream"),
    "QGTC.TiledAdjacency.to_old_packed": (ASYNC, "clone + index_select on the current stream"),
    "QGTC.TiledAdjacency.to_rows": (HOST, "repeat_interleave with tensor repeats reads their sum back (a test aid)"),
    "QGTC.TiledAdjacency.max_block_tiles": (HOST, ".item() on first use"),
    "QGTC.TiledAdjacency.n_tiles": (PURE, "shape"), "QGTC.TiledAdjacency.device": (PURE, "attribute"),
    "QGTC.TiledAdjacency.nbytes": (PURE, "shapes"),
    # ---- the private entries behind tiled.py -----------------------------------------------------------------------------------------
    "ext._tiled_pack": (HOST, "row_ptr[nrb].item(): the tile count sizes the allocation"),
    "ext._reorder_nodes": (HOST, "validate reads bad_index back"),
    "ext._tiled_mm": (ASYNC, "one kernel on current_stream(bit_X)"),
    "ext._tiled_mm_t": (ASYNC, "one kernel on current_stream(bit_X)"),
    "ext._tiled_mm_f32": (ASYNC, "one kernel on current_stream(X)"),
    "ext._tiled_mm_f32_t": (ASYNC, "one kernel on current_stream(X)"),
    "ext._tiled_mm_f32_src": (ASYNC, "one kernel on current_stream(X)"),
    "ext._tiled_mm_f32_t_src": (ASYNC, "one kernel on current_stream(X)"),
    "ext._tiled_degrees": (ASYNC, "hipMemsetAsync + kernels on current_stream(row_ptr)"),
    "ext._tiled_colindex": (ASYNC, "hipMemsetAsync + count / scan / fill kernels on current_stream(row_ptr)"),
    "ext._tiled_inv_sqrt_degree": (ASYNC, "one kernel on current_stream(deg)"),
}

# aliases: the same function object under another name (tests/test_stream_contract.py asserts the identity), covered by their target
ALIASES = {"QGTC.bit_qnt": "QGTC.val2bit", "QGTC.mm_v1": "QGTC.bitMM2Bit", "QGTC.mm_v2": "QGTC.bitMM2Int"}

CLASSES = ("BatchedGemm", "FusedLayer", "ChainedPair", "EpochPlan", "TiledAdjacency")


def names_of(cls):
    """The table's names of one class, aliases left out (they are their targets), sorted."""
    return sorted(k for k, (c, _) in CONTRACT.items() if c == cls and k not in ALIASES)


def exported_names():
    """What the build exports today, in the table's spelling. Needs the built extension, no GPU."""
    import QGTC
    import qgtc_ppopp22_amd

    ext = qgtc_ppopp22_amd.load_ext()
    names = {"QGTC." + k for k in dir(QGTC) if not k.startswith("_") and k != "torch"}
    names |= {"QGTC." + k for k in dir(ext) if not k.startswith("_") and k != "torch"}
    names |= {"ext." + k for k in dir(ext) if k.startswith("_") and not k.startswith("__")}
    for c in CLASSES:
        names |= {f"QGTC.{c}.{k}" for k in dir(getattr(QGTC, c)) if not k.startswith("_")}
    return names
