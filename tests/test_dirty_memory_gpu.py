"""Every operator on recycled, poisoned device memory (tests/dirty_memory.py; DESIGN.md, "Dirty memory").

Each case creates its operands, then runs under ``dirty`` once per pattern: the adjacency is packed INSIDE it, so packing, reordering,
``.T``, the degree caches, the edge-value index and every output, saved tensor and scratch buffer come from blocks whose words are
0x7FC00000 (a NaN) or 0xA5A5A5A5 (a small negative number). The result must equal the exact models bit for bit (a NaN only where the
model has one), and the two patterns' results must equal each other bit for bit.

a. the registry: every non-raw case of tests/stream_cases.py (``REGISTRY``; ``EXCLUDED`` states the two rules of what is left out);
b. directed skip-path cases on the tiled surface (``DIRECTED`` x ``GRAPHS``): graphs without a tile, with row blocks and k-quads
   without one, ragged last blocks, masks that remove whole blocks, dropout that empties rows;
c. whole modules: one training step of every layer of conv.py on ``islands200`` (``MODULES``);
d. tests/test_dirty_memory.py (no GPU) holds ``DIRECTED`` and ``MODULES`` against ``tiled.__all__`` and conv.py.

A new operator adds a function to ``DIRECTED`` (or a layer to ``MODULES``) that names it in ``covers``.

The harness itself is shown to bite by two fake operators that use no project kernel (test_an_unwritten_row_fails_under_both_patterns,
test_a_row_left_at_zero_passes_clean_and_fails_dirty), and its two error conditions by test_fresh_memory_and_a_written_operand_are_errors."""
import functools

import numpy as np
import pytest

import dirty_memory as dm
import stream_cases as sc

pytestmark = pytest.mark.gpu

MODULE = "tests/test_dirty_memory_gpu.py"


# ---------------------------------------------------------------------------------------------------------------------------------------
# a. the registry
# ---------------------------------------------------------------------------------------------------------------------------------------
_BIG_GRAPHS = tuple(f"enqueue-graph-{d[0]}x{d[1]}x{d[2]}-" for d in sc.ENQUEUE_BIG)


def excluded_why(case):
    """None for a case that runs dirty, else the rule that leaves it out: raw cases prefill their own outputs; the headline-sized graph
    cases take too long."""
    if case.raw:
        return "raw: the case prefills its own outputs with NaN words and canaries"
    if case.id.startswith(_BIG_GRAPHS):
        return "enqueue-graph on an ENQUEUE_BIG shape: run time"
    return None


REGISTRY = [c for c in sc.CASES if excluded_why(c) is None]
EXCLUDED = {c.id: excluded_why(c) for c in sc.CASES if excluded_why(c) is not None}


@pytest.fixture(scope="module")
def env(qgtc, oracle):
    import torch

    e = sc.env_of(qgtc, oracle, torch)
    from qgtc_ppopp22_amd import tiled

    e.tiled = tiled
    a = torch.ones(64, 32, device=e.dev)
    torch.mm(a, a.t())                 # the BLAS handle and its workspace exist before any case counts the driver's allocations
    torch.cuda.synchronize(e.dev)
    return e


def _under_both_patterns(env, what, inputs, run, check, sizes=()):
    """run() under each pattern; check(got, label) on each result; the two results bit for bit. Returns the first result."""
    torch, results = env.torch, []
    for pattern in dm.PATTERNS:
        with dm.dirty(torch, env.dev, pattern, inputs=inputs, sizes=sizes) as d:
            dm.announce(MODULE, d)
            got = [t.detach().cpu() for t in run()]
        check(got, f"{what} on memory poisoned with {pattern:#010x}")
        results.append(got)
    dm.same_bits(results[0], results[1], f"{what}: {dm.PATTERNS[0]:#010x} against {dm.PATTERNS[1]:#010x}")
    return results[0]


@pytest.mark.parametrize("case", [pytest.param(c, id=c.id) for c in REGISTRY])
def test_registry_case_on_dirty_memory(env, case):
    torch = env.torch
    live = case.build(env)
    what = f"{'/'.join(case.entries)} [{case.id}]"
    with torch.cuda.device(env.dev), sc.switches(env.Q, live):
        live.load(1)                   # the buffers hold content 1 before `dirty` records the operands' bits
        torch.cuda.synchronize(env.dev)

        def run():
            live.load(1)
            return live.outputs(live.run())

        _under_both_patterns(env, what, live.bufs, run, lambda got, label: sc.check(got, live.expected[1], label),
                             sizes=[np.asarray(e).nbytes for e in live.expected[1]])


# the cases whose plan objects allocate in their constructors and in bind(): occupancy bitmaps, statistics, descriptors, pools, weight codes
BUILT_DIRTY = [c for c in REGISTRY if any(e.split(".")[1] in ("BatchedGemm", "FusedLayer", "ChainedPair", "EpochPlan") for e in c.entries)]


@pytest.mark.parametrize("case", [pytest.param(c, id=c.id) for c in BUILT_DIRTY])
def test_plan_built_and_run_on_dirty_memory(env, case):
    """The registry builds its cases before `dirty`, so what BatchedGemm, FusedLayer, ChainedPair and EpochPlan allocate in their
    constructors and in bind() is clean there. Here the whole case is built INSIDE the poisoned region, then run on content 1."""
    torch = env.torch
    what = f"{'/'.join(case.entries)} [{case.id}], built on dirty memory"

    def run():
        live = case.build(env)
        with sc.switches(env.Q, live):
            live.load(1)
            out = live.outputs(live.run())
            torch.cuda.synchronize(env.dev)
        run.expected = live.expected[1]
        return out

    with torch.cuda.device(env.dev):
        _under_both_patterns(env, what, [], run, lambda got, label: sc.check(got, run.expected, label))


# ---------------------------------------------------------------------------------------------------------------------------------------
# b. the graphs
# ---------------------------------------------------------------------------------------------------------------------------------------
GRAPHS = ("void1", "void129", "islands200", "g300", "g300r")


class Graph:
    """An edge list in its own numbering (src, dst) and in the adjacency's (s, d: through the model's rank under reorder), NumPy."""

    def __init__(self, name):
        from reorder_model import reorder_model
        from tiled_esoftmax_model import graph_edges

        self.name, self.reorder = name, name.endswith("r")
        empty = np.zeros(0, dtype=np.int64)
        if name == "void1":
            self.n, self.src, self.dst = 1, empty, empty
        elif name == "void129":
            self.n, self.src, self.dst = 129, empty, empty
        elif name == "islands200":
            rng = np.random.default_rng(200)
            self.n = 200
            self.src = np.concatenate([rng.integers(0, 20, size=60), [199, 199]]).astype(np.int64)
            self.dst = np.concatenate([rng.integers(0, 20, size=60), [150, 199]]).astype(np.int64)
        else:
            self.n = 300
            self.src, self.dst = (np.asarray(a, dtype=np.int64) for a in graph_edges(300))      # test_tiled_esoftmax_gpu.graph(300)
        n = self.n
        self.perm = self.rank = None
        self.s, self.d = self.src, self.dst
        if self.reorder:
            self.perm, self.rank = reorder_model(self.src, self.dst, n)
            self.s, self.d = self.rank[self.src], self.rank[self.dst]

    def device(self, env):
        t = env.torch
        return t.from_numpy(self.src).to(env.dev), t.from_numpy(self.dst).to(env.dev)

    def pack(self, env, dsrc, ddst, **kw):
        return env.Q.pack_edges_tiled(dsrc, ddst, self.n, reorder=self.reorder, **kw)


@functools.lru_cache(maxsize=None)
def graph(name):
    return Graph(name)


def _dev(env, a, grad=False):
    t = env.torch.from_numpy(np.ascontiguousarray(a)).to(env.dev)
    return t.requires_grad_(True) if grad else t


def _rng(g, salt):
    return np.random.default_rng([g.n, len(g.src), salt])


def _normal(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


def _grad(env, y, wrt, dY):
    return list(env.torch.autograd.grad(y, wrt, dY))


# ---------------------------------------------------------------------------------------------------------------------------------------
# b. the directed cases: prepare(env, g) -> (inputs, run, want). `inputs` exist before `dirty`; run() packs and computes inside it.
# ---------------------------------------------------------------------------------------------------------------------------------------
def bit_shapes():
    """The two smallest (N, w, ob) of tests/test_tiled_variants_gpu.py's POISON rows."""
    from test_tiled_variants_gpu import POISON

    return sorted({(N, w, ob) for _, N, w, ob, _ in POISON})[:2]


def case_bits(env, g):
    """tiledMM2Bit / tiledMM2Int, plain and with mean_scale(), both views: the whole word array, pad rows and pad words included."""
    from qgtc_ppopp22_amd.shapes import rows_shape
    from tiled_model import aggregate, expected_bits, expected_floats
    from tiled_scaled_model import degrees, expected_bits_scaled, mean_scale, scaled

    n, rng, shapes = g.n, _rng(g, 1), bit_shapes()
    Xq = [rng.integers(0, 2 ** w, size=(n, N)) for N, w, _ in shapes]
    dX = [_dev(env, x.astype(np.float32)) for x in Xq]
    dsrc, ddst = g.device(env)
    o_deg, i_deg = degrees(g.s, g.d, n)
    want = []
    for T in (False, True):
        r = mean_scale(i_deg if T else o_deg)
        for x, (N, w, ob) in zip(Xq, shapes):
            C = aggregate(g.s, g.d, n, x, T)
            y = scaled(C, r)
            shape = rows_shape(n, N, ob)          # the models give the words flat
            want += [expected_bits(env.O, C, ob).reshape(shape), expected_floats(C), expected_bits_scaled(env.O, y, ob).reshape(shape), y]

    def run():
        adj, Q, out = g.pack(env, dsrc, ddst), env.Q, []
        for view in (adj, adj.T):
            ms = view.mean_scale()
            for x, (N, w, ob) in zip(dX, shapes):
                bx = Q.val2bit(x, w, True, False)
                out += [Q.tiledMM2Bit(view, bx, N, w, ob), Q.tiledMM2Int(view, bx, N, w), Q.tiledMM2Bit(view, bx, N, w, ob, ms),
                        Q.tiledMM2Int(view, bx, N, w, ms)]
        return out
    return dX + [dsrc, ddst], run, want


def _case_float(N):
    def prepare(env, g):
        """tiledMMFloat / tiledAggregate: plain, sym, max and min with their winners, attention with its statistics for one head and for
        three, edge weights - forward and every gradient, both views."""
        import tiled_attn_heads_model as ahm
        import tiled_edge_model as em
        from tiled_attn_model import attention_f32, attention_grads_f32
        from tiled_float_model import aggregate_f32
        from tiled_max_model import MAX, MIN, extremum_f32, select_f32
        from tiled_scaled_model import degrees
        from tiled_sym_model import aggregate_f32_src, inv_sqrt_degree

        n, s, d, rng, Q = g.n, g.s, g.d, _rng(g, 10 + N), env.Q
        nnz = em.slot_cells(s, d, n)[0].size
        X, dY, X3, dY3 = _normal(rng, n, N), _normal(rng, n, N), _normal(rng, n, 3 * N), _normal(rng, n, 3 * N)
        p, q, P3, Q3, vals = _normal(rng, n), _normal(rng, n), _normal(rng, n, 3), _normal(rng, n, 3), _normal(rng, nnz)
        o_deg, i_deg = degrees(s, d, n)
        dsrc, ddst = g.device(env)
        t = {k: _dev(env, v, grad=k not in ("dY", "dY3")) for k, v in
             dict(X=X, dY=dY, X3=X3, dY3=dY3, p=p, q=q, P3=P3, Q3=Q3, vals=vals).items()}
        want = []
        for T in (False, True):
            r, c = (inv_sqrt_degree(i_deg), inv_sqrt_degree(o_deg)) if T else (inv_sqrt_degree(o_deg), inv_sqrt_degree(i_deg))
            y = aggregate_f32(s, d, n, X, T)
            want += [y, y, aggregate_f32(s, d, n, dY, not T)]
            want += [aggregate_f32_src(s, d, n, X, T, r, c), aggregate_f32_src(s, d, n, dY, not T, c, r)]
            for op in (MAX, MIN):
                out, arg = extremum_f32(s, d, n, X, T, op)
                want += [out, arg, out, select_f32(s, d, n, dY, arg, not T)]
            Y, m, inv = attention_f32(s, d, n, X, p, q, 0.2, T)
            want += [Y, m, inv, Y] + list(attention_grads_f32(s, d, n, X, p, q, dY, Y, m, inv, 0.2, T)[:3])
            Y, m, inv = ahm.attention_heads_f32(s, d, n, X3, P3, Q3, 0.2, T)
            want += [Y, m, inv, Y] + list(ahm.attention_grads_heads_f32(s, d, n, X3, P3, Q3, dY3, Y, m, inv, 0.2, T)[:3])
            want += [em.weighted_f32(s, d, n, X, vals, T), em.weighted_f32(s, d, n, X, vals, T), em.weighted_f32(s, d, n, dY, vals, not T),
                     em.sddmm_f32(s, d, n, dY, X, T)]

        def run():
            adj, out = g.pack(env, dsrc, ddst), []
            for view in (adj, adj.T):
                y = Q.tiledAggregate(view, t["X"])
                out += [Q.tiledMMFloat(view, t["X"].detach()), y] + _grad(env, y, [t["X"]], t["dY"])
                y = Q.tiledAggregate(view, t["X"], view.sym_scale(), view.T.sym_scale())
                out += [y] + _grad(env, y, [t["X"]], t["dY"])
                for op in ("max", "min"):
                    y = Q.tiledAggregate(view, t["X"], reduce=op)
                    out += list(Q.tiledMMFloat(view, t["X"].detach(), reduce=op, return_arg=True)) + [y] + _grad(env, y, [t["X"]], t["dY"])
                for x, a, b, g_ in ((t["X"], t["p"], t["q"], t["dY"]), (t["X3"], t["P3"], t["Q3"], t["dY3"])):
                    y = Q.tiledAggregate(view, x, attn=(a, b))
                    out += list(Q.tiledMMFloat(view, x.detach(), attn=(a.detach(), b.detach()), return_stats=True)) + [y] + _grad(env, y, [x, a, b], g_)
                y = Q.tiledAggregate(view, t["X"], edge_weight=t["vals"])
                out += [Q.tiledMMFloat(view, t["X"].detach(), edge_weight=t["vals"].detach()), y] + _grad(env, y, [t["X"], t["vals"]], t["dY"])
            return out
        return list(t.values()) + [dsrc, ddst], run, want
    return prepare


def mask_flags(g, T):
    """(row flags without block 0 of the view - 32 rows on adj, 128 on adj.T -, neighbour flags without every neighbour of the first row
    of the view that has any, that row or None) from the model's lists."""
    from tiled_float_model import neighbour_lists

    n = g.n
    rows = np.ones(n, dtype=bool)
    rows[: 128 if T else 32] = False
    nbrs = np.ones(n, dtype=bool)
    out_row, nb, deg = neighbour_lists(g.s, g.d, n, T)
    live = np.flatnonzero(deg > 0)
    row = int(live[-1]) if live.size else None          # the LAST such row: it survives the row mask on the graphs with edges
    if row is not None:
        nbrs[nb[out_row == row]] = False
    return rows, nbrs, row


def drop_seed(g):
    """(seed, rows of adj that have neighbours and lose all of them at rate 0.9 under it) - the first seed for which the model shows one."""
    from tiled_drop_model import kept_edges, threshold
    from tiled_float_model import neighbour_lists

    deg = neighbour_lists(g.s, g.d, g.n, False)[2]
    for seed in range(1, 65):
        ks, kd = kept_edges(g.s, g.d, g.n, threshold(0.9), seed)
        lost = np.flatnonzero((deg > 0) & (neighbour_lists(ks, kd, g.n, False)[2] == 0))
        if lost.size and ks.size:
            return seed, lost
    raise AssertionError("no seed in 1 .. 64 empties a row and keeps an edge")


def case_masks(env, g):
    """Forward and every gradient of the sum, the maximum (with its winners), the attention and the attention with three heads (with
    their statistics), and degrees() / mean_scale() / sym_scale(), under a row mask that removes block 0 whole, a neighbour mask that
    empties a live row and both together; the four operators also under edge_drop=(0.9, seed), with a seed that empties rows where the
    graph has an edge. The gradients are the models' on the kept edges: the select with an arg of -1 for masked and emptied rows, the
    attention's three gradients with m, inv and D of rows without a kept neighbour."""
    import tiled_attn_heads_model as ahm
    from tiled_attn_model import attention_f32, attention_grads_f32
    from tiled_drop_model import kept_edges, threshold
    from tiled_float_model import aggregate_f32, neighbour_lists
    from tiled_max_model import MAX, extremum_f32, select_f32
    from tiled_nodes_model import induced_edges
    from tiled_scaled_model import mean_scale
    from tiled_sym_model import inv_sqrt_degree

    n, s, d, rng, Q, N = g.n, g.s, g.d, _rng(g, 3), env.Q, 5
    X, dY, p, q = _normal(rng, n, N), _normal(rng, n, N), _normal(rng, n), _normal(rng, n)
    X3, dY3, P3, Q3 = _normal(rng, n, 3 * N), _normal(rng, n, 3 * N), _normal(rng, n, 3), _normal(rng, n, 3)
    t = {k: _dev(env, v, grad=not k.startswith("dY")) for k, v in dict(X=X, dY=dY, p=p, q=q, X3=X3, dY3=dY3, P3=P3, Q3=Q3).items()}
    dsrc, ddst = g.device(env)

    def model(ks, kd, T):
        y = aggregate_f32(ks, kd, n, X, T)
        out, arg = extremum_f32(ks, kd, n, X, T, MAX)
        want = [y, aggregate_f32(ks, kd, n, dY, not T), out, arg, out, select_f32(ks, kd, n, dY, arg, not T)]
        Y, m, inv = attention_f32(ks, kd, n, X, p, q, 0.2, T)
        want += [Y, m, inv, Y] + list(attention_grads_f32(ks, kd, n, X, p, q, dY, Y, m, inv, 0.2, T)[:3])
        Y, m, inv = ahm.attention_heads_f32(ks, kd, n, X3, P3, Q3, 0.2, T)
        return want + [Y, m, inv, Y] + list(ahm.attention_grads_heads_f32(ks, kd, n, X3, P3, Q3, dY3, Y, m, inv, 0.2, T)[:3])

    def device(view, **kw):
        y = Q.tiledAggregate(view, t["X"], **kw)
        out = [y] + _grad(env, y, [t["X"]], t["dY"])
        y = Q.tiledAggregate(view, t["X"], reduce="max", **kw)
        out += list(Q.tiledMMFloat(view, t["X"].detach(), reduce="max", return_arg=True, **kw)) + [y] + _grad(env, y, [t["X"]], t["dY"])
        for x, a, b, g_ in ((t["X"], t["p"], t["q"], t["dY"]), (t["X3"], t["P3"], t["Q3"], t["dY3"])):
            y = Q.tiledAggregate(view, x, attn=(a, b), **kw)
            out += list(Q.tiledMMFloat(view, x.detach(), attn=(a.detach(), b.detach()), return_stats=True, **kw)) + [y] + _grad(env, y, [x, a, b], g_)
        return out

    want, flags, combos = [], {}, (("row", True, False), ("nbr", False, True), ("both", True, True))
    for T in (False, True):
        rows, nbrs, row = mask_flags(g, T)
        flags[T] = (_dev(env, rows), _dev(env, nbrs))
        if row is not None:
            kept = neighbour_lists(*induced_edges(s, d, n, None, nbrs, T), n, T)[2]
            assert kept[row] == 0 and neighbour_lists(s, d, n, T)[2][row] > 0, "the neighbour mask empties a live row"
            if g.name == "islands200":
                assert rows[row], "the emptied row survives the row mask"
        for _, use_r, use_n in combos:
            ks, kd = induced_edges(s, d, n, rows if use_r else None, nbrs if use_n else None, T)
            deg = neighbour_lists(ks, kd, n, T)[2].astype(np.int32)
            want += model(ks, kd, T) + [deg, mean_scale(deg), inv_sqrt_degree(deg)]
    seed = 1                                  # without an edge any seed does: the _drop entries run on an adjacency without a tile
    if g.src.size:
        seed, lost = drop_seed(g)
        assert lost.size >= 1, "the model shows a row with neighbours that loses all of them"
    ks, kd = kept_edges(s, d, n, threshold(0.9), seed)
    for T in (False, True):
        want += model(ks, kd, T)

    def run():
        adj, out = g.pack(env, dsrc, ddst), []
        for T, view in ((False, adj), (True, adj.T)):
            rm, nm = (env.tiled.node_bitmap(f, n) for f in flags[T])
            for _, use_r, use_n in combos:
                kw = {"row_mask": rm if use_r else None, "nbr_mask": nm if use_n else None}
                out += device(view, **kw) + [view.degrees(**kw), view.mean_scale(**kw), view.sym_scale(**kw)]
        for view in (adj, adj.T):
            out += device(view, edge_drop=(0.9, seed))
        return out
    return list(t.values()) + list(flags[False]) + list(flags[True]) + [dsrc, ddst], run, want


def _case_edge(H, dh):
    def prepare(env, g):
        """The edge-value surface with H heads of dh columns: SDDMM, edge scores, edge softmax with statistics, edge attention, the
        additive score and its attention - forward and every gradient, both views -, and edge_values / edge_slots / edge_endpoints."""
        import tiled_addscore_model as am
        import tiled_edge_model as em
        import tiled_heads_model as hm
        from tiled_model import set_cells

        n, s, d, rng, tl, N = g.n, g.s, g.d, _rng(g, 100 * H + dh), env.tiled, H * dh
        row, col = em.slot_cells(s, d, n)
        nnz = row.size
        A, B, V, dY, att = _normal(rng, n, N), _normal(rng, n, N), _normal(rng, n, N), _normal(rng, n, N), _normal(rng, H, dh)
        logits, ge = (3 * _normal(rng, nnz, H)), _normal(rng, nnz, H)
        cells = set_cells(g.src, g.dst, n)                     # every stored cell once, in the edge list's numbering
        es, ed = cells // n, cells % n
        ew = _normal(rng, es.size)
        qs = np.concatenate([g.src, [-1, n, 0, 0]]).astype(np.int64)          # the raw list (doubled edges are not stored) and ids out of range
        qd = np.concatenate([g.dst, [0, 0, n + 5, 0]]).astype(np.int64)
        old_to_new = (lambda a: np.where((a >= 0) & (a < n), g.rank[np.clip(a, 0, n - 1)], a)) if g.reorder else (lambda a: a)
        flat = (lambda a: a.reshape(-1)) if H == 1 else (lambda a: a)          # one head: [nnz] vectors and [n] statistics
        stat = (lambda a: a[:, 0]) if H == 1 else (lambda a: a)
        t = {k: _dev(env, v, grad=k in ("A", "B", "V", "att", "logits")) for k, v in
             dict(A=A, B=B, V=V, dY=dY, att=att if H > 1 else att.reshape(-1), logits=flat(logits), ge=flat(ge), es=es, ed=ed, ew=ew, qs=qs,
                  qd=qd).items()}
        dsrc, ddst = g.device(env)
        want = []
        for T in (False, True):
            want += [flat(hm.sddmm_heads_f32(s, d, n, A, B, H, T))]
            want += [flat(hm.sddmm_heads_f32(s, d, n, A, B, H, T)), hm.weighted_heads_f32(s, d, n, B, ge, T), hm.weighted_heads_f32(s, d, n, A, ge, not T)]
            alpha, m, inv = hm.edge_softmax_heads_f32(s, d, n, logits, T)
            want += [flat(alpha), stat(m), stat(inv), flat(hm.edge_softmax_grad_heads_f32(s, d, n, alpha, ge, T))]
            want += [hm.edge_attention_heads_f32(s, d, n, A, B, V, H, None, T)] + list(hm.edge_attention_grads_heads_f32(s, d, n, A, B, V, H, dY, None, T))
            want += [flat(am.addscore_heads_f32(s, d, n, A, B, att, 0.2, H, T))]
            d_own, _ = am.addscore_grad_heads_f32(s, d, n, A, B, att, 0.2, ge, H, T)
            d_nbr, _ = am.addscore_grad_heads_f32(s, d, n, B, A, att, 0.2, ge, H, not T)
            want += [d_own, d_nbr, None]                                       # att's gradient is torch.sum of P: no exact model
            d_own, d_nbr, dV, _ = am.additive_attention_grads_heads_f32(s, d, n, A, B, V, att, 0.2, H, dY, T)
            want += [am.additive_attention_heads_f32(s, d, n, A, B, V, att, 0.2, H, T)[0], d_own, d_nbr, dV, None]
        slots = em.edge_slots(s, d, n, old_to_new(es), old_to_new(ed))
        assert (slots >= 0).all() and np.unique(slots).size == nnz, "the stored cells name every slot once"
        values = np.zeros(nnz, dtype=np.float32)
        values[slots] = ew
        want += [values, em.edge_slots(s, d, n, old_to_new(qs), old_to_new(qd)), row.astype(np.int32), col.astype(np.int32)]

        def run():
            adj, out = g.pack(env, dsrc, ddst), []
            for view in (adj, adj.T):
                out += [tl.tiledSDDMM(view, t["A"].detach(), t["B"].detach(), heads=H)]
                y = tl.tiledEdgeScores(view, t["A"], t["B"], heads=H)
                out += [y] + _grad(env, y, [t["A"], t["B"]], t["ge"])
                alpha, m, inv = tl.tiledEdgeSoftmax(view, t["logits"], return_stats=True)
                out += [alpha, m, inv] + _grad(env, alpha, [t["logits"]], t["ge"])
                y = tl.tiledEdgeAttention(view, t["A"], t["B"], t["V"], heads=H)
                out += [y] + _grad(env, y, [t["A"], t["B"], t["V"]], t["dY"])
                y = tl.tiledEdgeAdditiveScores(view, t["A"], t["B"], t["att"], 0.2, heads=H)
                out += [y] + _grad(env, y, [t["A"], t["B"], t["att"]], t["ge"])
                y = tl.tiledEdgeAdditiveAttention(view, t["A"], t["B"], t["V"], t["att"], 0.2, heads=H)
                out += [y] + _grad(env, y, [t["A"], t["B"], t["V"], t["att"]], t["dY"])
            out += [tl.edge_values(adj.T, t["es"], t["ed"], t["ew"]), tl.edge_slots(adj, t["qs"], t["qd"])] + list(tl.edge_endpoints(adj.T))
            return out
        return list(t.values()) + [dsrc, ddst], run, want
    return prepare


def case_adjacency(env, g):
    """pack_edges_tiled and reorder_nodes with validate on and off, the column index, node_bitmap with its pad bits, degrees, mean_scale
    and sym_scale of both views, to_rows, add_self_loops."""
    from oracle.qgtc_oracle import np_pack_edges
    from qgtc_ppopp22_amd.shapes import rows_shape
    from reorder_model import reorder_model
    from tiled_model import np_colindex, np_tiled
    from tiled_nodes_model import bitmap
    from tiled_scaled_model import degrees, mean_scale
    from tiled_sym_model import add_self_loops, inv_sqrt_degree

    n, s, d, rng, Q, tl = g.n, g.s, g.d, _rng(g, 4), env.Q, env.tiled
    flags = rng.random(n) < 0.4
    ids = np.flatnonzero(flags)[::-1].copy()
    ids = np.concatenate([ids, ids[:3]]).astype(np.int64)                     # any order, duplicates allowed
    dflags, dids = _dev(env, flags), _dev(env, ids)
    dsrc, ddst = g.device(env)
    rp, kq, tiles = np_tiled(s, d, n)
    o_deg, i_deg = degrees(s, d, n)
    perm, rank = reorder_model(g.src, g.dst, n)
    ls, ld = add_self_loops(g.src, g.dst, n)
    packed = [rp, kq, tiles] + ([g.perm, g.rank] if g.reorder else [])
    want = packed + packed + [perm, perm] + list(np_colindex(rp, kq, n)) + [bitmap(flags), bitmap(flags)]
    want += [o_deg, i_deg, mean_scale(o_deg), mean_scale(i_deg), inv_sqrt_degree(o_deg), inv_sqrt_degree(i_deg)]
    dense = rows_shape(n, n, 1)
    want += [np_pack_edges(s, d, n, n, 1).reshape(dense), np_pack_edges(d, s, n, n, 1).reshape(dense), ls, ld] + list(np_tiled(ls, ld, n))

    def parts(adj):
        return [adj.row_ptr, adj.kquad, adj.tiles] + ([adj.perm, adj.rank] if g.reorder else [])

    def run():
        adj = g.pack(env, dsrc, ddst, validate=True)
        out = parts(adj) + parts(g.pack(env, dsrc, ddst, validate=False))
        out += [Q.reorder_nodes(dsrc, ddst, n, validate=True), Q.reorder_nodes(dsrc, ddst, n, validate=False)]
        at = adj.T
        out += [at.col_ptr, at.col_tile, at.col_rb, tl.node_bitmap(dflags, n), tl.node_bitmap(dids, n)]
        out += [adj.degrees(), at.degrees(), adj.mean_scale(), at.mean_scale(), adj.sym_scale(), at.sym_scale(), adj.to_rows(), at.to_rows()]
        loops = Q.add_self_loops(dsrc, ddst, n)
        looped = Q.pack_edges_tiled(loops[0], loops[1], n)
        return out + list(loops) + [looped.row_ptr, looped.kquad, looped.tiles]
    return [dflags, dids, dsrc, ddst], run, want


_EDGE_NAMES = ("tiledSDDMM", "tiledEdgeScores", "tiledEdgeSoftmax", "tiledEdgeAttention", "tiledEdgeAdditiveScores",
               "tiledEdgeAdditiveAttention", "edge_values", "edge_slots", "edge_endpoints")
# case id -> (prepare, covers: the names of tiled.__all__ it runs dirty)
DIRECTED = {
    "bits": (case_bits, ("tiledMM2Bit", "tiledMM2Int", "pack_edges_tiled", "TiledAdjacency")),
    "float-N1": (_case_float(1), ("tiledMMFloat", "tiledAggregate")),
    "float-N5": (_case_float(5), ("tiledMMFloat", "tiledAggregate")),
    "float-N40": (_case_float(40), ("tiledMMFloat", "tiledAggregate")),
    "masks": (case_masks, ("tiledMMFloat", "tiledAggregate", "node_bitmap")),
    "edge-1x5": (_case_edge(1, 5), _EDGE_NAMES),
    "edge-3x5": (_case_edge(3, 5), _EDGE_NAMES),
    "edge-2x100": (_case_edge(2, 100), _EDGE_NAMES),
    "adjacency": (case_adjacency, ("pack_edges_tiled", "reorder_nodes", "node_bitmap", "TiledAdjacency", "add_self_loops")),
}


@pytest.mark.parametrize("name", GRAPHS)
@pytest.mark.parametrize("case", sorted(DIRECTED))
def test_directed_case_on_dirty_memory(env, case, name):
    g = graph(name)
    inputs, run, want = DIRECTED[case][0](env, g)
    _under_both_patterns(env, f"{case} on {name}", inputs, run, lambda got, label: dm.same_as_model(got, want, label),
                         sizes=(g.n * 4, g.n * 40 * 4))


# ---------------------------------------------------------------------------------------------------------------------------------------
# c. whole modules: one training step on islands200
# ---------------------------------------------------------------------------------------------------------------------------------------
F_IN, HIDDEN, OUT = 12, 20, 7
DROP = (0.5, 0x0123456789ABCDEF)


def _gcn(**kw):
    def make(conv):
        return conv.GCNConv(F_IN, HIDDEN, OUT, **kw), ("W_in", "W_out"), OUT, {}
    return make


def _gat(conv):
    return conv.GATConv(F_IN, OUT, heads=2, edge_drop=DROP[0]), ("W", "a_dst", "a_src"), 2 * OUT, {"edge_seed": DROP[1]}


def _transformer(conv):
    return conv.TransformerConv(F_IN, OUT, heads=2), ("W_q", "W_k", "W_v"), 2 * OUT, {}


def _gatv2(conv):
    return conv.GATv2Conv(F_IN, OUT, heads=2), ("W_l", "W_r", "att"), 2 * OUT, {}


def _reference(name, g, t, dtype):
    """The dense definition of the layer on the graph: {"Y", "dX", "d<parameter>"}."""
    import gatv2_reference as G2
    import layers_reference as R
    import transformer_reference as TR

    a = (g.src, g.dst, g.n, t["X"])
    if name.startswith("GCNConv"):
        kw = {"norm": "sym"} if name.endswith("sym") else {"aggr": "max"}
        return R.gcn_layer(*a, t["W_in"], t["W_out"], t["dY"], dtype=dtype, **kw)
    if name == "GATConv":
        return R.gat_layer(*a, t["W"], t["a_dst"], t["a_src"], t["dY"], heads=2, edge_drop=(DROP[0], DROP[1], None), dtype=dtype)
    if name == "TransformerConv":
        return TR.transformer_layer(*a, t["W_q"], t["W_k"], t["W_v"], t["dY"], heads=2, dtype=dtype)
    return G2.gatv2_layer(*a, t["W_l"], t["W_r"], t["att"], t["dY"], heads=2, dtype=dtype)


# module case -> (constructor, the torch.nn.Module of conv.py it steps)
MODULES = {
    "GCNConv-sym": (_gcn(norm="sym"), "GCNConv"),
    "GCNConv-max": (_gcn(aggr="max"), "GCNConv"),
    "GATConv": (_gat, "GATConv"),
    "TransformerConv": (_transformer, "TransformerConv"),
    "GATv2Conv": (_gatv2, "GATv2Conv"),
}
QNT_MODES = {"sum": {}, "mean": {"aggr": "mean"}, "float_out": {"aggr": "mean", "float_out": True}}       # conv.GCNConv_Qnt, forward only


@pytest.mark.parametrize("name", sorted(MODULES))
def test_training_step_on_dirty_memory(env, name):
    """forward, loss, backward and every parameter gradient: the bits of the same step on clean memory under either pattern, and within
    layers_reference.tolerances of the dense float64 definition."""
    import layers_reference as R
    from qgtc_ppopp22_amd import conv

    torch, g = env.torch, graph("islands200")
    with torch.random.fork_rng(devices=[]):          # the parameters' draw leaves the process's generator where it was
        torch.manual_seed(7)
        layer, params, width, fwd = MODULES[name][0](conv)
    layer = layer.to(env.dev).train()
    rng = _rng(g, 5)
    X, dY = _dev(env, _normal(rng, g.n, F_IN), grad=True), _dev(env, _normal(rng, g.n, width))
    dsrc, ddst = g.device(env)

    def step():
        adj = g.pack(env, dsrc, ddst)
        Y = layer(adj, X, **fwd)
        loss = (Y * dY).sum()
        grads = torch.autograd.grad(loss, [X] + [getattr(layer, p) for p in params])
        return [Y] + list(grads)

    clean = [t.detach().cpu() for t in step()]
    t = {p: getattr(layer, p).detach().cpu().numpy() for p in params}
    t.update(X=X.detach().cpu().numpy(), dY=dY.cpu().numpy())
    ref64, ref32 = _reference(name, g, t, torch.float64), _reference(name, g, t, torch.float32)
    tol = R.tolerances(ref64, ref32)
    keys = ["Y", "dX"] + ["d" + p for p in params]
    assert set(keys) == set(ref64)

    def check(got, label):
        dm.same_bits(got, clean, f"{label}, against the same step on clean memory")
        for k, t_ in zip(keys, got):
            err = float((t_.to(torch.float64) - ref64[k]).abs().max())
            assert tol[k] > 0 and err <= tol[k], f"{label}: {k} is {err:.3e} from the float64 definition, tolerance {tol[k]:.3e}"

    check(clean, f"{name} on clean memory")
    _under_both_patterns(env, f"{name} training step on islands200", [X, dY, dsrc, ddst] + [getattr(layer, p) for p in params], step, check)


@pytest.mark.parametrize("mode", sorted(QNT_MODES))
def test_quantised_forward_on_dirty_memory(env, mode):
    """conv.GCNConv_Qnt on the tiled adjacency: the bits of the same forward on clean memory under either pattern."""
    from qgtc_ppopp22_amd import conv

    torch, g = env.torch, graph("islands200")
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(8)
        layer = conv.GCNConv_Qnt(F_IN, HIDDEN, OUT, **QNT_MODES[mode]).to(env.dev)
    X = _dev(env, np.abs(_normal(_rng(g, 6), g.n, F_IN)) * 3)
    dsrc, ddst = g.device(env)

    def forward():
        layer.bit_W_in = None          # the weights are packed again, on whatever memory the allocator hands out
        with torch.no_grad():
            return [layer(g.pack(env, dsrc, ddst), X)]

    clean = [t.cpu() for t in forward()]
    assert clean[0].shape == (g.n, OUT) and bool(torch.isfinite(clean[0]).all()) and bool((clean[0] != 0).any())
    _under_both_patterns(env, f"GCNConv_Qnt {mode} on islands200", [X, dsrc, ddst, layer.W_in, layer.W_out], forward,
                         lambda got, label: dm.same_bits(got, clean, f"{label}, against the same forward on clean memory"))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the harness bites: two fake operators, plain torch, no project kernel
# ---------------------------------------------------------------------------------------------------------------------------------------
def _fake_rows(torch, X, leave_last_row):
    """X + 1 into a torch.empty result; the defect: the last row is never written."""
    out = torch.empty_like(X)
    rows = X.size(0) - 1 if leave_last_row else X.size(0)
    out[:rows] = X[:rows] + 1
    return out


@pytest.mark.parametrize("pattern", dm.PATTERNS)
def test_an_unwritten_row_fails_under_both_patterns(env, pattern):
    """A fake operator that leaves the last row of its torch.empty result unwritten: the comparison with the reference fails under each
    pattern, on exactly that row; the complete operator passes."""
    torch = env.torch
    X = _dev(env, _normal(np.random.default_rng(1), 37, 5))
    want = [X.cpu().numpy() + np.float32(1)]
    with dm.dirty(torch, env.dev, pattern, inputs=[X]):
        whole = [_fake_rows(torch, X, False).cpu()]
    with dm.dirty(torch, env.dev, pattern, inputs=[X]):      # poisoned again: the block the complete fake just freed holds its result
        holed = [_fake_rows(torch, X, True).cpu()]
    dm.same_as_model(whole, want, "the complete fake")
    with pytest.raises(AssertionError, match="differs from the model in 5 of 185"):
        dm.same_as_model(holed, want, "the incomplete fake")
    assert bool((dm.bits_of(holed[0][-1]) == pattern).all()), "the unwritten row reads back as the pattern"


def test_a_row_left_at_zero_passes_clean_and_fails_dirty(env):
    """A fake whose reference has +0 in the last row and which never writes it: on memory that holds zeros - what a short process sees -
    it passes; under both patterns it fails. The all-zero word is the harness's own `clean` pattern."""
    torch = env.torch
    X = _dev(env, _normal(np.random.default_rng(2), 37, 5))
    want = X.cpu().numpy() + np.float32(1)
    want[-1] = 0.0
    with dm.dirty(torch, env.dev, 0x00000000, inputs=[X]):
        clean = [_fake_rows(torch, X, True).cpu()]
    dm.same_as_model(clean, [want], "the fake on zeroed memory")
    for pattern in dm.PATTERNS:
        with dm.dirty(torch, env.dev, pattern, inputs=[X]):
            got = [_fake_rows(torch, X, True).cpu()]
        with pytest.raises(AssertionError, match="differs from the model in 5 of 185"):
            dm.same_as_model(got, [want], "the fake on poisoned memory")
        with pytest.raises(AssertionError, match="differs in 5 of 185"):
            dm.same_bits(got, clean, "the fake, poisoned against zeroed")


def test_fresh_memory_and_a_written_operand_are_errors(env):
    """The two conditions of the harness raise: a body that outgrows the poisoned pool (the allocator goes to the driver), and an
    operator that writes to an operand."""
    torch = env.torch
    X = _dev(env, _normal(np.random.default_rng(3), 8, 8))
    with pytest.raises(dm.DirtyMemoryError, match="FRESH memory"):
        with dm.dirty(torch, env.dev, dm.NAN_WORD, inputs=[X], large_bytes=32 * dm.MIB, small_bytes=2 * dm.MIB) as d:
            torch.empty(d.nbytes + 16 * dm.MIB, dtype=torch.uint8, device=env.dev)      # more than everything the cache holds
    with pytest.raises(AssertionError, match="no operator writes to an operand"):
        with dm.dirty(torch, env.dev, dm.NAN_WORD, inputs=[X]):
            X.add_(1)
