"""Helpers and cases of the stream tests (tests/test_streams_gpu.py, tests/test_stream_abi_gpu.py, tests/test_multistream_gpu.py, and
the stream test of every later tiled operator, which builds its own LIVE object next to the test).

A CASE names the entries of tests/stream_contract.py it exercises and builds a LIVE object on the GPU: static device buffers, four
seeded CONTENTS for them (pinned host tensors), the EXPECTED results of every content from the CPU oracle or the NumPy models, and
``run()``, which calls the operator on the buffers and returns its outputs. Two drivers use a live case:

``ordering_probe``     content 0 in the buffers, synchronise; then on a fresh side stream: a head start of filler work (plain torch.mm,
                       ``Filler``), the copy of content 1 into the buffers, the operator, the read-back. The result must be content 1's.
                       An operator that went to another stream runs while the filler still occupies the side stream, reads content 0 and
                       gives content 0's result: "ran ahead of its stream".
``capture_and_replay`` one warm-up call on a side stream, one call captured into a graph, three replays with contents 1, 2, 3 copied into
                       the buffers before each: every replay gives that content's result and the bits of an eager call. A launch that
                       was not captured raises at capture time or leaves a stale result. Outputs a case lists in ``refill`` are
                       filled with -1 before each replay.

Everything is compared bit for bit. Importing this module needs neither a GPU nor the built extension (test_stream_contract.py reads
CASES on the CPU).
"""
import contextlib
import types

import numpy as np

from helpers import (QgtcLoaderBatch, QgtcProblem, edge_floats, kernel_behind, oracle_chain, rand_q)
from qgtc_ppopp22_amd import cabi
from qgtc_ppopp22_amd.shapes import cols_shape, rows_shape

FILLER_MIN_MS = 5.0          # the head start of a probe: filler work on the side stream, timed with HIP events once per device
NAN_WORD = 0x7FC00000        # float32 quiet NaN, the prefill of raw-entry outputs
CANARY = 0x5A5A5A5A


# ---------------------------------------------------------------------------------------------------------------------------------------
# the head start
# ---------------------------------------------------------------------------------------------------------------------------------------
class Filler:
    """`reps` float32 torch.mm of 4096 x 4096 scratch matrices into a preallocated result: nothing of this project. `reps` is doubled
    until the whole run takes at least FILLER_MIN_MS by HIP events; `ms` is the measured time of the final setting."""

    def __init__(self, torch, device):
        self.torch = torch
        with torch.cuda.device(device):
            g = torch.Generator(device="cpu").manual_seed(1)
            self.a = torch.rand(4096, 4096, generator=g).to(device)
            self.b = torch.rand(4096, 4096, generator=g).to(device)
            self.c = torch.empty(4096, 4096, device=device)
            self.reps = 1
            self()                                   # rocBLAS picks and loads its kernel
            torch.cuda.synchronize(device)
            while True:
                self.ms = self._time(device)
                if self.ms >= FILLER_MIN_MS:
                    break
                self.reps = max(self.reps * 2, int(self.reps * FILLER_MIN_MS / max(self.ms, 1e-3)) + 1)
            print(f"[stream probes] head start on {device}: {self.reps} x torch.mm(4096^2 float32) = {self.ms:.2f} ms by HIP events")

    def _time(self, device):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def __call__(self, scale=1):
        for _ in range(self.reps * scale):
            self.torch.mm(self.a, self.b, out=self.c)


_FILLERS = {}


def filler_for(torch, device):
    key = str(device)
    if key not in _FILLERS:
        _FILLERS[key] = Filler(torch, device)
    return _FILLERS[key]


def head_start(torch, device, scale=1):
    """Queue the filler on the current stream and return an event recorded behind it: while `event.query()` is False the filler still
    occupies the stream, so whatever the host has queued by then waits behind it."""
    filler_for(torch, device)(scale)
    ev = torch.cuda.Event()
    ev.record()
    return ev


def until_sensitive(attempt):
    """attempt(scale) -> (the head start was still running when the operator had been queued, result). A probe whose head start ran out
    first - a slow host, a first-use initialisation inside the call - could not have seen a mis-streamed launch: it is repeated with
    a longer head start, whatever its result was."""
    for scale in (1, 2, 4):
        busy, got = attempt(scale)
        if busy:
            return got
    raise AssertionError("three times the head start ended before the operator was queued: the probe cannot see a mis-streamed launch here")


PROBE_ROUNDS = 3


def probe_rounds(attempt, verify):
    """The probe on PROBE_ROUNDS fresh side streams in a row, each result verified. A process has few hardware queues (four by default) and
    its streams share them: a launch that went to the WRONG stream is still ordered behind the head start when that stream happens to sit
    on the side stream's hardware queue. torch hands out its pool streams in turn, so consecutive side streams sit on different queues
    and at most one of them can hide the defect."""
    for r in range(PROBE_ROUNDS):
        verify(until_sensitive(attempt), f"side stream {r + 1} of {PROBE_ROUNDS}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# comparing bits
# ---------------------------------------------------------------------------------------------------------------------------------------
def bits_of(x):
    """Any array or CPU tensor as a flat array of unsigned words of its element size: NaNs and signed zeros compare as bits."""
    a = np.ascontiguousarray(x.numpy() if hasattr(x, "numpy") else x)
    return a.reshape(-1).view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    a, b = bits_of(a), bits_of(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a == b).all())


def check(got, want, what, old=None, old_means="ran ahead of its stream"):
    """got[i] == want[i] bit for bit; when it equals old[i] instead (the result of the content the buffers held BEFORE), say so."""
    assert len(got) == len(want), f"{what}: {len(got)} outputs, {len(want)} expected"
    for i, (g, w) in enumerate(zip(got, want)):
        if same(g, w):
            continue
        gb, wb = bits_of(g), bits_of(w)
        if old is not None and same(g, old[i]):
            raise AssertionError(f"{what}: output {i} is the result of the PREVIOUS content of the buffers: the operator {old_means}")
        if gb.shape != wb.shape or gb.dtype != wb.dtype:
            raise AssertionError(f"{what}: output {i} has {gb.size} x {gb.dtype} words, expected {wb.size} x {wb.dtype}")
        bad = np.flatnonzero(gb != wb)
        raise AssertionError(f"{what}: output {i} differs in {bad.size} of {gb.size} words (first at {bad[0]}: got {gb[bad[0]]:#x}, "
                             f"expected {wb[bad[0]]:#x}); it is not the previous content's result either")


# ---------------------------------------------------------------------------------------------------------------------------------------
# a live case
# ---------------------------------------------------------------------------------------------------------------------------------------
class Live:
    """bufs: static device tensors; contents[k]: one host array per buffer; expected[k]: one array per output; run(): the operator on
    bufs -> list of output tensors (or a callable giving them: outputs that only exist once a capture has ended). engine / zero_skip:
    the switches the case runs under. raw(stream_ptr) -> rc, for the C entries: writes into `outs`. refill: indices of outputs that do
    not depend on the contents (a sample's thresholds); they are filled with -1 before every replay, so a replay that did not write them
    shows."""

    def __init__(self, torch, bufs, contents, expected, run=None, raw=None, outs=None, engine="auto", zero_skip=True, keep=None, refill=()):
        assert len(contents) == len(expected) == 4 and all(len(c) == len(bufs) for c in contents)
        self.torch, self.bufs, self.expected, self.run, self.raw, self.outs = torch, bufs, expected, run, raw, outs
        self.engine, self.zero_skip, self.keep, self.refill = engine, zero_skip, keep, tuple(refill)
        self.contents = []
        for c in contents:
            row = []
            for b, h in zip(bufs, c):
                h = np.ascontiguousarray(h)
                h = h.view({np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(h.dtype, h.dtype))
                t = torch.from_numpy(h)
                t = t.view(b.dtype) if t.dtype != b.dtype and t.element_size() == b.element_size() else t
                assert t.numel() == b.numel() and t.dtype == b.dtype, (t.shape, t.dtype, b.shape, b.dtype)
                row.append(t.reshape(b.shape).pin_memory())
            self.contents.append(row)
        for k in range(3):     # a stale result must be visible: consecutive contents give different results
            assert any(not same(x, y) for x, y in zip(expected[k], expected[k + 1])), f"contents {k} and {k + 1} expect the same result"

    def load(self, k):
        """Queue the copies of content k into the buffers on the current stream (asynchronous: the host tensors are pinned)."""
        with self.torch.no_grad():
            for b, h in zip(self.bufs, self.contents[k]):
                b.copy_(h, non_blocking=True)

    def outputs(self, r):
        return list(r() if callable(r) else r)


def eager_results(torch, bufs, contents, run):
    """The `expected` of a case whose reference is the operator's own eager result: run() on every content in turn, on the current
    (default) stream before any probe, as CPU tensors."""
    want = []
    for c in contents:
        with torch.no_grad():
            for b, h in zip(bufs, c):
                b.copy_(torch.from_numpy(np.ascontiguousarray(h)))
        want.append([o.detach().cpu() for o in run()])
    return want


@contextlib.contextmanager
def switches(qgtc, live):
    prev = (qgtc.get_engine(), qgtc.get_zero_skip())
    qgtc.set_engine(live.engine)
    qgtc.set_zero_skip(live.zero_skip)
    try:
        yield
    finally:
        qgtc.set_engine(prev[0])
        qgtc.set_zero_skip(prev[1])


def ordering_probe(torch, qgtc, live, what):
    """The eager probe on a fresh side stream (module docstring). One call on content 0 comes first, so that nothing the first call of a
    kernel does on the host (loading its code object) eats the head start. For a raw C entry the current stream stays the default one
    and the entry gets the side stream's handle; its outputs are prefilled with NaN on the side stream first."""
    dev = live.bufs[0].device

    def attempt(scale):
        live.load(0)
        if live.raw is None:
            live.outputs(live.run())
        else:
            assert live.raw(torch.cuda.current_stream(dev).cuda_stream) == 0
        torch.cuda.synchronize(dev)
        s = torch.cuda.Stream(dev)
        if live.raw is None:
            with torch.cuda.stream(s):
                ev = head_start(torch, dev, scale)
                live.load(1)
                r = live.run()
                busy = not ev.query()
                got = [o.cpu() for o in live.outputs(r)]          # copies on s and waits for s only
        else:
            with torch.cuda.stream(s):
                ev = head_start(torch, dev, scale)
                live.load(1)
                for o in live.outs:
                    o.view(torch.int32).fill_(NAN_WORD)
                    if hasattr(o, "_canary"):
                        o._canary.fill_(CANARY)
            assert torch.cuda.current_stream(dev) != s
            rc = live.raw(s.cuda_stream)
            busy = not ev.query()
            assert rc == 0, f"{what}: rc {rc}"
            with torch.cuda.stream(s):
                got = [o.cpu() for o in live.outs] + [o._canary.cpu() for o in live.outs if hasattr(o, "_canary")]
        torch.cuda.synchronize(dev)
        return busy, got

    want = list(live.expected[1]) + ([np.full(o._canary.numel(), CANARY, np.uint32) for o in live.outs if hasattr(o, "_canary")] if live.raw else [])
    old = list(live.expected[0]) + want[len(live.expected[0]):]
    with torch.cuda.device(dev), switches(qgtc, live):
        probe_rounds(attempt, lambda got, which: check(got, want, f"{what}, {which}", old=old))


def capture_and_replay(torch, qgtc, live, what, replays=(1, 2, 3)):
    dev = live.bufs[0].device
    with torch.cuda.device(dev), switches(qgtc, live):
        cur = torch.cuda.current_stream(dev)

        def call():
            if live.raw is None:
                return live.run()
            rc = live.raw(torch.cuda.current_stream(dev).cuda_stream)
            assert rc == 0, f"{what}: rc {rc}"
            return live.outs

        side = torch.cuda.Stream(dev)
        side.wait_stream(cur)
        with torch.cuda.stream(side):          # the warm-up: kernel handles, LDS opt-in, first-use allocations, lazy caches
            live.load(0)
            call()
        cur.wait_stream(side)
        torch.cuda.synchronize(dev)
        captured = torch.cuda.CUDAGraph()
        with torch.cuda.graph(captured):
            r = call()
        outs = live.outputs(r)
        for k in replays:
            live.load(k)
            for i in live.refill:
                outs[i].fill_(-1)
            captured.replay()
            got = [o.clone() for o in outs]
            torch.cuda.synchronize(dev)
            check([g.cpu() for g in got], live.expected[k], f"{what}, replay with content {k}", old=live.expected[k - 1],
                  old_means="was not captured (a stale result)")
            eager = live.outputs(call())
            torch.cuda.synchronize(dev)
            check([e.cpu() for e in eager], [g.cpu() for g in got], f"{what}, eager call on content {k} against the replay")
        del captured


# ---------------------------------------------------------------------------------------------------------------------------------------
# the registry
# ---------------------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, id, entries, build, capture=True, probe=True, raw=False):
        self.id, self.entries, self.build, self.capture, self.probe, self.raw = id, tuple(entries), build, capture, probe, raw

    def __repr__(self):
        return self.id


CASES = []


def case(id, entries, **kw):
    def deco(fn):
        CASES.append(Case(id, entries, fn, **kw))
        return fn
    return deco


def cases_of(entry):
    return [c for c in CASES if entry in c.entries]


def env_of(qgtc, oracle, torch, device="cuda:0"):
    import qgtc_ppopp22_amd

    return types.SimpleNamespace(Q=qgtc, O=oracle, torch=torch, dev=torch.device(device), ext=qgtc_ppopp22_amd.load_ext())


def empty(env, shape, dtype):
    return env.torch.empty(shape, dtype=dtype, device=env.dev)


def _i32(env, shape):
    return empty(env, shape, env.torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# val2bit, bit2val, val2bit_many, i8gemm, tile_occupancy
# ---------------------------------------------------------------------------------------------------------------------------------------
def _val2bit_inputs(H, W, nbits, seed):
    xs = []
    for k in range(4):
        rng = np.random.default_rng(seed * 16 + k)
        if nbits <= 8:
            xs.append(edge_floats(rng, H, W, nbits))
        else:                                             # as tests/test_gpu_parity.py::test_val2bit_wide
            x = (rng.uniform(0, 1, size=(H, W)) * 2.0 ** nbits).astype(np.float32)
            x[0, :8] = [np.nan, -1, 2.0 ** nbits, 2.0 ** nbits * 2, 0.5, 1.5, 2.0 ** 31, 2.0 ** 32]
            xs.append(x)
    return xs


def _val2bit_case(name, H, W, nbits, cm, ol, seed):
    def build(env):
        xs = _val2bit_inputs(H, W, nbits, seed)
        buf = empty(env, (H, W), env.torch.float32)
        fn = getattr(env.Q, name)
        return Live(env.torch, [buf], [[x] for x in xs], [[env.O.val2bit(x, nbits, cm, ol)] for x in xs],
                    run=lambda: [fn(buf, nbits, cm, ol)])
    return build


for _name in ("val2bit", "checked_val2bit"):
    for _tag, _a in (("rows", (37, 130, 3, False, False)), ("cols", (130, 37, 2, True, False)), ("output_layer", (257, 300, 4, True, True)),
                     ("rows17", (40, 70, 17, False, False))):
        CASES.append(Case(f"{_name}-{_tag}", ["QGTC." + _name], _val2bit_case(_name, *_a, seed=len(CASES) + 1)))


@case("bit2val", ["QGTC.bit2val"])
def _bit2val(env):
    H, W, nbits = 37, 130, 3
    qs = [rand_q(np.random.default_rng(40 + k), H, W, nbits) for k in range(4)]
    buf = _i32(env, rows_shape(H, W, nbits))
    return Live(env.torch, [buf], [[env.O.pack(q, nbits, False)] for q in qs], [[q] for q in qs],
                run=lambda: [env.Q.bit2val(buf, nbits, H, W, False, False)])


@case("val2bit_many", ["QGTC.val2bit_many"])
def _val2bit_many(env):
    shapes, nbits, cm, ol = [(50, 64), (64, 64), (64, 10), (64, 10)], 2, [True, True, True, False], [False, False, True, False]
    xs = [[edge_floats(np.random.default_rng(50 + 4 * k + i), h, w, nbits) for i, (h, w) in enumerate(shapes)] for k in range(4)]
    bufs = [empty(env, s, env.torch.float32) for s in shapes]
    return Live(env.torch, bufs, xs, [[env.O.val2bit(x, nbits, c, o) for x, c, o in zip(row, cm, ol)] for row in xs],
                run=lambda: env.Q.val2bit_many(bufs, nbits, cm, ol))


@case("i8gemm", ["QGTC.i8gemm"])
def _i8gemm(env):
    from oracle.qgtc_oracle import np_i8gemm

    M, K, N = 100, 256, 48
    ab = [[np.random.default_rng(60 + k).integers(-128, 128, size=s, dtype=np.int8) for s in ((M, K), (N, K))] for k in range(4)]
    bufs = [empty(env, (M, K), env.torch.int8), empty(env, (N, K), env.torch.int8)]
    return Live(env.torch, bufs, ab, [[np_i8gemm(a, b)] for a, b in ab], run=lambda: [env.Q.i8gemm(bufs[0], bufs[1])])


@case("tile_occupancy", ["QGTC.tile_occupancy"])
def _tile_occupancy(env):
    from oracle.qgtc_oracle import np_tile_occupancy

    M, K, a = 300, 1000, 1
    Xs = [env.O.pack(rand_q(np.random.default_rng(70 + k), M, K, a, 1.5e-4), a, False) for k in range(4)]
    buf = _i32(env, rows_shape(M, K, a))
    return Live(env.torch, [buf], [[x] for x in Xs], [[np_tile_occupancy(x, M, K, a)] for x in Xs],
                run=lambda: [env.Q.tile_occupancy(buf, M, K, a)])


# ---------------------------------------------------------------------------------------------------------------------------------------
# the three bitMM operators: one shape per kernel family (the family is asserted, so a routing change cannot quietly drop one)
# ---------------------------------------------------------------------------------------------------------------------------------------
MM_FAMILIES = [
    # tag, (M, K, N, a, w, ob) from tests/test_gpu_parity.py::MM_CASES (wide: its own), engine, the kernel behind it
    ("fp4_one", (1213, 1213, 128, 1, 2, 2), "auto", "k_bitmm_fp4_one"),
    ("rows_single", (129, 513, 100, 3, 2, 5), "auto", "k_bitmm_fp4_rows_single"),
    ("stream", (257, 9000, 40, 1, 1, 3), "mfma", "k_bitmm_fp4_stream"),
    ("skinny", (257, 9000, 40, 1, 1, 3), "auto", "k_bitmm_fp4_skinny"),
    ("wide", (1024, 1024, 1030, 1, 2, 2), "auto", "k_bitmm_fp4_wide"),
    ("int8", (77, 259, 40, 8, 8, 8), "mfma", "k_bitmm_mfma"),
    ("planes", (20, 300, 40, 9, 12, 4), "auto", "k_bitmm_planes"),
    ("popcount", (100, 1000, 64, 1, 1, 1), "popcount", "k_bitmm"),
]


def _small_q(rng, H, W, bits, density, rare):
    """Quantised values of `bits` planes whose sums stay readable: two-bit values at the given density, and a few full-range ones (one in
    `rare`) so that the upper planes are not empty."""
    q = rand_q(rng, H, W, min(bits, 2), density)
    if bits > 2:
        big = rng.random((H, W)) < 1.0 / rare
        q = np.where(big, rand_q(rng, H, W, bits), q).astype(np.int32)
    return q


def _mm_operands(O, M, K, N, a, w, seed, pad128=True, ob=None):
    """Packed operands of one product. The left operand is sparse and the values are small, so the sums spread over 0 .. 2^ob instead of
    all running into requant's clamp (a saturated result is the same for every content: a stale one could not be told from a fresh one)."""
    rng = np.random.default_rng(seed)
    mean = lambda b: 0.5 if b == 1 else 1.5   # noqa: E731
    density = min(1.0, 2.0 ** ((ob or 4) - 1) / (K * mean(a) * mean(w)))
    X = O.pack(_small_q(rng, M, K, a, density, 4 * K), a, False)
    Wt = O.pack(_small_q(rng, K, N, w, None, 4 * K), w, True, output_layer=not pad128)
    return X, Wt


def _mm_case(name, dims, engine, kernel, zero_skip=True, pad128=True, seed=0):
    M, K, N, a, w, ob = dims
    mode = 2 if name.endswith("Int") else 1 if name.endswith("_col") else 0

    def build(env):
        assert kernel_behind(M, K, N, a, w, ob, mode, engine) == kernel, "the routing moved: pick another shape for this family"
        ops = [_mm_operands(env.O, M, K, N, a, w, seed * 16 + k, pad128 or mode != 2, ob) for k in range(4)]
        bufs = [_i32(env, rows_shape(M, K, a)), _i32(env, cols_shape(K, N, w, mode == 2 and not pad128))]
        fn = getattr(env.Q, name)
        if mode == 2:
            want = [[env.O.bitmm2int(X, Wt, M, K, N, a, w, pad128)] for X, Wt in ops]
            run = lambda: [fn(bufs[0], bufs[1], M, K, N, a, w, pad128)]            # noqa: E731
        else:
            want = [[env.O.bitmm2bit(X, Wt, M, K, N, a, w, ob, col=(mode == 1))] for X, Wt in ops]
            run = lambda: [fn(bufs[0], bufs[1], M, K, N, a, w, ob)]                # noqa: E731
        return Live(env.torch, bufs, [list(o) for o in ops], want, run=run, engine=engine, zero_skip=zero_skip)
    return build


for _tag, _dims, _eng, _kern in MM_FAMILIES:      # lean and checked path of bitMM2Bit on every family
    for _name in ("bitMM2Bit", "checked_bitMM2Bit"):
        CASES.append(Case(f"{_name}-{_tag}", ["QGTC." + _name], _mm_case(_name, _dims, _eng, _kern, seed=len(CASES) + 1)))
for _name in ("bitMM2Bit_col", "checked_bitMM2Bit_col", "bitMM2Int", "checked_bitMM2Int"):
    for _tag, _dims, _eng, _kern in (MM_FAMILIES[0], MM_FAMILIES[1], MM_FAMILIES[7]):
        CASES.append(Case(f"{_name}-{_tag}", ["QGTC." + _name], _mm_case(_name, _dims, _eng, _kern, seed=len(CASES) + 1)))
for _name in ("bitMM2Bit", "checked_bitMM2Bit", "bitMM2Int"):       # zero-tile skipping off; bitMM2Int with PAD8 weight lines
    CASES.append(Case(f"{_name}-fp4_one-noskip", ["QGTC." + _name], _mm_case(_name, MM_FAMILIES[0][1], "auto", "k_bitmm_fp4_one", zero_skip=False,
                                                                              seed=len(CASES) + 1)))
    CASES.append(Case(f"{_name}-popcount-noskip", ["QGTC." + _name], _mm_case(_name, MM_FAMILIES[7][1], "popcount", "k_bitmm", zero_skip=False,
                                                                               pad128=False, seed=len(CASES) + 1)))


@case("gcn_layer-bits", ["QGTC.gcn_layer"])
def _gcn_layer_bits(env):
    return _gcn_layer(env, False)


@case("gcn_layer-float", ["QGTC.gcn_layer"])
def _gcn_layer_float(env):
    return _gcn_layer(env, True)


def _gcn_layer(env, output):
    n, f_in, f_out, act, wb = 300, 50, 64, 2, 2
    O, contents, want = env.O, [], []
    for k in range(4):
        rng = np.random.default_rng(90 + k)
        A = O.pack((rng.random((n, n)) < 1.5 / n).astype(np.int32), 1, False)           # sparse everywhere: nothing saturates
        X, W = O.pack(rand_q(rng, n, f_in, act, 3.0 / f_in), act, False), O.pack(rand_q(rng, f_in, f_out, wb, 1.0 / 6), wb, True)
        T = O.bitmm2bit(X, W, n, f_in, f_out, act, wb, act, col=True)
        contents.append([A, X, W])
        want.append([O.bitmm2int(A, T, n, n, f_out, 1, act, True) if output else O.bitmm2bit(A, T, n, n, f_out, 1, act, act)])
    bufs = [_i32(env, rows_shape(n, n, 1)), _i32(env, rows_shape(n, f_in, act)), _i32(env, cols_shape(f_in, f_out, wb))]
    return Live(env.torch, bufs, contents, want, run=lambda: [env.Q.gcn_layer(bufs[0], bufs[1], bufs[2], n, f_in, f_out, 1, act, wb, output)])


# ---------------------------------------------------------------------------------------------------------------------------------------
# bitMM2Bit_enqueue: a preallocated output with a canary tail behind the words the launch needs
# ---------------------------------------------------------------------------------------------------------------------------------------
_BIG = {}


def big_operands(O, M, K, N, w, k):
    """Seeded operands of a headline-sized product (M, K multiples of 128: every packed word is payload, so the words are drawn
    directly) and the oracle's rows- and cols-layout results; cached for the session."""
    key = (M, K, N, w, k)
    if key not in _BIG:
        rng = np.random.default_rng(1000 + 10 * w + k)
        words = int(np.prod(rows_shape(M, K, 1)))          # about 2^(w-1) / mean(w) set bits a row: the sums stay around the clamp 2^w
        X = np.zeros(words, dtype=np.uint32)
        n_set = int(M * max(1.0, 2.0 ** (w - 1) / max(0.5, (2.0 ** w - 1) / 2)) * 2)
        where = rng.integers(0, words * 32, size=n_set)
        np.bitwise_or.at(X, where // 32, (np.uint32(1) << (where % 32).astype(np.uint32)))
        Wt = O.pack(rand_q(rng, K, N, w), w, True)
        _BIG[key] = (X, Wt, O.bitmm2bit(X, Wt, M, K, N, 1, w, w), O.bitmm2bit(X, Wt, M, K, N, 1, w, w, col=True))
    return _BIG[key]


def enqueue_live(env, M, K, N, a, w, ob, reps, cols, seed=0):
    O, torch = env.O, env.torch
    if M % 128 == 0 and K % 128 == 0 and a == 1 and ob == w:
        ops = [big_operands(O, M, K, N, w, k) for k in range(4)]
        contents, words = [[x, wt] for x, wt, _, _ in ops], [r[3] if cols else r[2] for r in ops]
    else:
        ops = [_mm_operands(O, M, K, N, a, w, 3000 + seed * 16 + k, ob=ob) for k in range(4)]
        contents, words = [list(o) for o in ops], [O.bitmm2bit(X, Wt, M, K, N, a, w, ob, col=cols) for X, Wt in ops]
    need = words[0].size
    whole = torch.full((need + 64,), CANARY, dtype=torch.int32, device=env.dev)
    out, tail = whole[:need], whole[need:]
    bufs = [_i32(env, rows_shape(M, K, a)), _i32(env, cols_shape(K, N, w))]
    canary = np.full(64, CANARY, np.uint32)

    def run():
        env.Q.bitMM2Bit_enqueue(out, bufs[0], bufs[1], M, K, N, a, w, ob, reps, cols)
        return [out, tail]
    live = Live(torch, bufs, contents, [[wd, canary] for wd in words], run=run)
    live.out, live.args = out, (M, K, N, a, w, ob, reps, cols)
    return live


ENQUEUE_SMALL = [(129, 513, 100, 3, 2, 5), (300, 300, 128, 1, 8, 8)]
ENQUEUE_BIG = [(4096, 4096, 64, 1, w, w) for w in (1, 2, 4, 8)]
for _dims in ENQUEUE_SMALL:
    for _reps in (1, 3):
        for _cols in (False, True):
            CASES.append(Case(f"enqueue-{_dims[0]}x{_dims[1]}x{_dims[2]}-reps{_reps}-{'cols' if _cols else 'rows'}", ["QGTC.bitMM2Bit_enqueue"],
                              (lambda env, d=_dims, r=_reps, c=_cols: enqueue_live(env, *d, r, c)), capture=False))
for _dims in ENQUEUE_BIG + ENQUEUE_SMALL:          # the graphs `bench.py --issue graph` builds, and two small shapes
    for _reps in (1, 3, 200):
        for _cols in (False, True):
            CASES.append(Case(f"enqueue-graph-{_dims[0]}x{_dims[1]}x{_dims[2]}-w{_dims[4]}-reps{_reps}-{'cols' if _cols else 'rows'}",
                              ["QGTC.bitMM2Bit_enqueue"], (lambda env, d=_dims, r=_reps, c=_cols: enqueue_live(env, *d, r, c)), probe=False))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the tiled products on a warmed adjacency
# ---------------------------------------------------------------------------------------------------------------------------------------
def graph(n, seed):
    from tiled_model import random_edges

    return random_edges(np.random.default_rng(seed), n, 4 * n)


def warm_adjacency(env, src, dst, n, reorder=False):
    t = env.torch
    adj = env.Q.pack_edges_tiled(t.from_numpy(src).to(env.dev), t.from_numpy(dst).to(env.dev), n, reorder=reorder)
    adj.T, adj.mean_scale(), adj.sym_scale(), adj.T.sym_scale()        # every lazy cache, before any probe or capture
    t.cuda.synchronize(env.dev)
    return adj


def _scales(src, dst, n, transposed, kind):
    """(row_scale, src_scale) of the model for a view: kind None / "mean" / "sym" / "src" (a source scale alone)."""
    from tiled_scaled_model import degrees, mean_scale
    from tiled_sym_model import inv_sqrt_degree

    out_deg, in_deg = degrees(src, dst, n)
    r, c = (in_deg, out_deg) if transposed else (out_deg, in_deg)
    return {None: (None, None), "mean": (mean_scale(r), None), "sym": (inv_sqrt_degree(r), inv_sqrt_degree(c)),
            "src": (None, inv_sqrt_degree(c))}[kind]


def _dev_scales(adj, kind):
    return {None: (None, None), "mean": (adj.mean_scale(), None), "sym": (adj.sym_scale(), adj.T.sym_scale()),
            "src": (None, adj.T.sym_scale())}[kind]


def _tiled_bits_case(to_float, transposed, scaled, N, bit2, ob, seed):
    def build(env):
        from tiled_model import aggregate, expected_bits, expected_floats
        from tiled_scaled_model import expected_bits_scaled, scaled as scale_rows

        n = 600
        src, dst = graph(n, seed)
        adj = warm_adjacency(env, src, dst, n)
        view = adj.T if transposed else adj
        r, _ = _scales(src, dst, n, transposed, "mean" if scaled else None)
        dr = view.mean_scale() if scaled else None
        contents, want = [], []
        for k in range(4):
            Xq = rand_q(np.random.default_rng(seed * 16 + k), n, N, bit2)
            C = aggregate(src, dst, n, Xq, transposed)
            contents.append([env.O.pack(Xq, bit2, True)])
            if scaled:
                y = scale_rows(C, r)
                want.append([y if to_float else expected_bits_scaled(env.O, y, ob)])
            else:
                want.append([expected_floats(C) if to_float else expected_bits(env.O, C, ob)])
        buf = _i32(env, cols_shape(n, N, bit2))
        if to_float:
            run = lambda: [env.Q.tiledMM2Int(view, buf, N, bit2, dr)]            # noqa: E731
        else:
            run = lambda: [env.Q.tiledMM2Bit(view, buf, N, bit2, ob, dr)]        # noqa: E731
        return Live(env.torch, [buf], contents, want, run=run, keep=adj)
    return build


for _tf, _name in ((False, "tiledMM2Bit"), (True, "tiledMM2Int")):
    for _tr in (False, True):
        for _sc in (False, True):
            _N = {(False, False): 16, (False, True): 40, (True, False): 64, (True, True): 100}[(_tr, _sc)]
            CASES.append(Case(f"{_name}-{'adjT' if _tr else 'adj'}{'-scaled' if _sc else ''}-N{_N}",
                              ["QGTC." + _name, "ext._tiled_mm_t" if _tr else "ext._tiled_mm"],
                              _tiled_bits_case(_tf, _tr, _sc, _N, 3, 4, seed=len(CASES) + 1)))


def _tiled_float_case(transposed, kind, N, seed, aggregate_op=False):
    def build(env):
        from tiled_sym_model import aggregate_f32_src

        n = 600
        src, dst = graph(n, seed)
        adj = warm_adjacency(env, src, dst, n)
        view = adj.T if transposed else adj
        r, c = _scales(src, dst, n, transposed, kind)
        dr, dc = _dev_scales(view, kind)
        torch = env.torch
        contents, want = [], []
        for k in range(4):
            rng = np.random.default_rng(seed * 16 + k)
            X = rng.normal(size=(n, N)).astype(np.float32)
            y = aggregate_f32_src(src, dst, n, X, transposed, r, c)
            if aggregate_op:        # forward and the gradient for X of sum(Y * G): the product on the other view, scales swapped
                G = rng.normal(size=(n, N)).astype(np.float32)
                contents.append([X, G])
                want.append([y, aggregate_f32_src(src, dst, n, G, not transposed, c, r)])
            else:
                contents.append([X])
                want.append([y])
        if aggregate_op:
            bufs = [empty(env, (n, N), torch.float32).requires_grad_(True), empty(env, (n, N), torch.float32)]

            def run():
                y = env.Q.tiledAggregate(view, bufs[0], dr, dc)
                return [y.detach(), torch.autograd.grad(y, bufs[0], bufs[1])[0]]
        else:
            bufs = [empty(env, (n, N), torch.float32)]
            run = lambda: [env.Q.tiledMMFloat(view, bufs[0], dr, dc)]            # noqa: E731
        return Live(torch, bufs, contents, want, run=run, keep=adj)
    return build


# one N per variant of FLOAT_FORWARD_VARIANTS (N <= 16, 32, 64, 128, beyond) and of FLOAT_TRANSPOSED_VARIANTS (N <= 16, 32, beyond)
FLOAT_CASES = [(False, None, 16), (False, "mean", 32), (False, "sym", 64), (False, "src", 128), (False, "sym", 200),
               (True, None, 16), (True, "sym", 32), (True, "mean", 64), (True, "src", 40)]
for _tr, _kind, _N in FLOAT_CASES:
    _e = "ext._tiled_mm_f32" + ("_t" if _tr else "") + ("_src" if _kind in ("sym", "src") else "")
    CASES.append(Case(f"tiledMMFloat-{'adjT' if _tr else 'adj'}-{_kind or 'plain'}-N{_N}", ["QGTC.tiledMMFloat", _e],
                      _tiled_float_case(_tr, _kind, _N, seed=len(CASES) + 1)))
for _tr, _kind, _N in ((False, "sym", 24), (True, "sym", 70), (False, None, 16)):
    CASES.append(Case(f"tiledAggregate-{'adjT' if _tr else 'adj'}-{_kind or 'plain'}-N{_N}", ["QGTC.tiledAggregate"],
                      _tiled_float_case(_tr, _kind, _N, seed=len(CASES) + 1, aggregate_op=True)))


@case("reordered-adjacency", ["QGTC.TiledAdjacency.to_new", "QGTC.TiledAdjacency.to_old", "QGTC.TiledAdjacency.to_old_packed"])
def _reordered(env):
    """A reordered adjacency: X goes to its numbering, the results come back. The features are small integers, so every float add is
    exact and the order the new ids impose does not show."""
    from tiled_model import aggregate, expected_bits

    n, N, bit2, ob = 600, 24, 2, 4
    src, dst = graph(n, 77)
    adj = warm_adjacency(env, src, dst, n, reorder=True)
    assert adj.perm is not None
    contents, want = [], []
    for k in range(4):
        Xq = rand_q(np.random.default_rng(770 + k), n, N, bit2)
        assert np.array_equal(env.O.quantize(Xq.astype(np.float32), bit2), Xq)         # val2bit keeps these values
        C = aggregate(src, dst, n, Xq)
        contents.append([Xq.astype(np.float32)])
        want.append([C.astype(np.float32), expected_bits(env.O, C, ob)])
    buf = empty(env, (n, N), env.torch.float32)

    def run():
        Xn = adj.to_new(buf)
        words = env.Q.tiledMM2Bit(adj, env.Q.val2bit(Xn, bit2, True, False), N, bit2, ob)
        return [adj.to_old(env.Q.tiledMMFloat(adj, Xn)), adj.to_old_packed(words, ob)]
    return Live(env.torch, [buf], contents, want, run=run, keep=adj)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the lazy caches of a TiledAdjacency and the entries that build them. The adjacency's own tensors are the static buffers: the four
# contents are images of one graph under maps that keep every row block's tile count (so row_ptr and T are the same) and change the
# k-quads and the bits.
# ---------------------------------------------------------------------------------------------------------------------------------------
CACHE_N = 1280      # a multiple of 128: the maps below stay in range


def cache_graphs():
    """[(src, dst, (row_ptr, kquad, tiles))] x 4. The base graph has three occupied tiles in every 32-row block (so most k-quads of a
    block are empty and the maps move them); content k rotates every cell's k-quad by k and its place inside the tile."""
    from tiled_model import np_tiled

    n, nq = CACHE_N, CACHE_N // 128
    rng = np.random.default_rng(5)
    s0, d0 = [], []
    for rb in range(n // 32):
        for q in rng.choice(nq, size=3, replace=False):
            s0.append(rb * 32 + rng.integers(0, 32, size=40))
            d0.append(q * 128 + rng.integers(0, 128, size=40))
    s0, d0 = np.concatenate(s0).astype(np.int64), np.concatenate(d0).astype(np.int64)
    s0, d0 = np.concatenate([s0, s0[::9], s0[::18]]), np.concatenate([d0, d0[::9], d0[::18]])       # multiplicities 2 and 3
    out = []
    for k in range(4):
        s = (s0 // 32) * 32 + (s0 % 32 + 3 * k) % 32
        d = ((d0 // 128 + k) % nq) * 128 + (d0 % 128 + 11 * k) % 128
        out.append((s, d, np_tiled(s, d, n)))
    assert all(np.array_equal(g[2][0], out[0][2][0]) for g in out)
    assert all(not np.array_equal(a[2][1], b[2][1]) for a, b in zip(out, out[1:]))
    return out


def _adjacency_buffers(env, graphs):
    t = env.torch
    rp, kq, tl = graphs[0][2]
    return [empty(env, rp.shape, t.int64), _i32(env, kq.shape), _i32(env, tl.shape)]


@case("ext._tiled_colindex", ["ext._tiled_colindex"])
def _colindex(env):
    from tiled_model import np_colindex

    gs = cache_graphs()
    bufs = _adjacency_buffers(env, gs)[:2]
    return Live(env.torch, bufs, [[g[2][0], g[2][1]] for g in gs], [list(np_colindex(g[2][0], g[2][1], CACHE_N)) for g in gs],
                run=lambda: env.ext._tiled_colindex(bufs[0], bufs[1], CACHE_N))


@case("ext._tiled_degrees", ["ext._tiled_degrees"])
def _degrees(env):
    from tiled_scaled_model import degrees, mean_scale

    gs = cache_graphs()
    bufs = _adjacency_buffers(env, gs)
    want = []
    for s, d, _ in gs:
        o, i = degrees(s, d, CACHE_N)
        want.append([o, i, mean_scale(o), mean_scale(i)])
    return Live(env.torch, bufs, [list(g[2]) for g in gs], want, run=lambda: env.ext._tiled_degrees(bufs[0], bufs[1], bufs[2], CACHE_N))


@case("ext._tiled_inv_sqrt_degree", ["ext._tiled_inv_sqrt_degree"])
def _inv_sqrt(env):
    from tiled_sym_model import inv_sqrt_degree

    degs = [np.random.default_rng(80 + k).integers(0, 50, size=1000).astype(np.int32) for k in range(4)]
    buf = _i32(env, (1000,))
    return Live(env.torch, [buf], [[d] for d in degs], [[inv_sqrt_degree(d)] for d in degs], run=lambda: [env.ext._tiled_inv_sqrt_degree(buf)])


def cache_expected(src, dst, X):
    """What `cache_run` returns for one graph and X: products through every lazy cache, and the caches themselves."""
    from tiled_model import np_colindex, np_tiled
    from tiled_scaled_model import degrees, mean_scale
    from tiled_sym_model import aggregate_f32_src, inv_sqrt_degree

    n = CACHE_N
    o, i = degrees(src, dst, n)
    rp, kq, _ = np_tiled(src, dst, n)
    return [aggregate_f32_src(src, dst, n, X, True, mean_scale(i), None),
            aggregate_f32_src(src, dst, n, X, False, inv_sqrt_degree(o), inv_sqrt_degree(i)),
            aggregate_f32_src(src, dst, n, X, True, inv_sqrt_degree(i), inv_sqrt_degree(o)),
            o, i] + list(np_colindex(rp, kq, n))


def cache_run(Q, adj, X):
    """First touches of adj.T, mean_scale() and sym_scale() with the products right behind them, on whatever stream is current."""
    t = adj.T
    return [Q.tiledMMFloat(t, X, t.mean_scale()), Q.tiledMMFloat(adj, X, adj.sym_scale(), t.sym_scale()),
            Q.tiledMMFloat(t, X, t.sym_scale(), adj.sym_scale()), adj.degrees(), t.degrees(), t.col_ptr, t.col_tile, t.col_rb]


@case("lazy-caches", ["QGTC.TiledAdjacency.T", "QGTC.TiledAdjacency.degrees", "QGTC.TiledAdjacency.mean_scale", "QGTC.TiledAdjacency.sym_scale"])
def _lazy(env):
    """A FRESH TiledAdjacency over the static buffers in every call: each call builds every cache again, on the stream it runs on."""
    gs = cache_graphs()
    bufs = _adjacency_buffers(env, gs) + [empty(env, (CACHE_N, 24), env.torch.float32)]
    Xs = [np.random.default_rng(85 + k).normal(size=(CACHE_N, 24)).astype(np.float32) for k in range(4)]
    return Live(env.torch, bufs, [list(g[2]) + [x] for g, x in zip(gs, Xs)], [cache_expected(g[0], g[1], x) for g, x in zip(gs, Xs)],
                run=lambda: cache_run(env.Q, env.Q.TiledAdjacency(CACHE_N, bufs[0], bufs[1], bufs[2]), bufs[3]))


# ---------------------------------------------------------------------------------------------------------------------------------------
# grouped launches: BatchedGemm / FusedLayer / ChainedPair through driver.BatchedEpoch, EpochPlan through driver.PlannedEpoch
# ---------------------------------------------------------------------------------------------------------------------------------------
def grouped_inputs(O, ns, F, H, C, b, seed, random_weights=False):
    """Four contents of ragged cluster batches (the adjacencies stay, X changes; with random_weights the weights change too) in the
    form helpers.oracle_chain reads. Adjacency, features and weights are all sparse: with the driver's all-ones weights every X . W
    runs into requant's clamp and the epoch's output no longer depends on X at all."""
    rng = np.random.default_rng(seed)
    As = [(rng.random((n, n)) < 1.5 / n).astype(np.float32) for n in ns]
    bitA = [O.val2bit(A, 1, False, False) for A in As]
    m = 2.0 ** b / 2.0

    def weights(rw):
        ws = [rand_q(rw, F, H, b, min(1.0, 2.0 ** (b - 1) / (3.0 * m * m))), rand_q(rw, H, H, b, 1.5 / (H * 0.5)), rand_q(rw, H, C, b, 1.5 / (H * 0.5))]
        ws = [w.astype(np.float32) for w in ws]
        return {"W1": O.val2bit(ws[0], b, True, False), "W2": O.val2bit(ws[1], b, True, False), "W3": O.val2bit(ws[2], b, True, True),
                "W3h": O.val2bit(ws[2], b, True, False), "hidden": H, "classes": C}
    fixed = weights(np.random.default_rng(seed + 1))
    contents = []
    for k in range(4):
        rk = np.random.default_rng(seed * 16 + k)
        Xs = [rand_q(rk, n, F, b, 3.0 / F).astype(np.float32) for n in ns]
        bis = [{"n": n, "F": F, "A": A, "X": X, "bit_A": a, "bit_X": O.val2bit(X, b, True, False), "bit_X_rows": O.val2bit(X, b, False, False)}
               for n, A, X, a in zip(ns, As, Xs, bitA)]
        contents.append((bis, weights(rk) if random_weights else fixed))
    return contents


def _grouped_live(env, chain, gin, planned, fuse=True, chain_stages=True, rebind=False, by_launch=False, b=2, seed=0):
    from qgtc_ppopp22_amd import driver
    from qgtc_ppopp22_amd.sampler import ClusterTensor

    torch, O, Q = env.torch, env.O, env.Q
    ns, F, H, C = [150, 333, 40], 50, 64, 10
    data = grouped_inputs(O, ns, F, H, C, b, 500 + seed, random_weights=rebind)
    bitA = [torch.from_numpy(bi["bit_A"].view(np.int32).reshape(rows_shape(n, n, 1))).to(env.dev) for n, bi in zip(ns, data[0][0])]
    Xc = [_i32(env, cols_shape(n, F, b)) for n in ns]
    Xr = [_i32(env, rows_shape(n, F, b)) for n in ns]
    Wd = {"W1": _i32(env, cols_shape(F, H, b)), "W2": _i32(env, cols_shape(H, H, b)), "W3": _i32(env, cols_shape(H, C, b, True)),
          "W3h": _i32(env, cols_shape(H, C, b)), "hidden": H, "classes": C, "feat": F}
    wkeys = ("W1", "W2", "W3", "W3h")
    bufs = Xc + Xr + [Wd[k] for k in wkeys]
    contents = [[bi["bit_X"] for bi in bis] + [bi["bit_X_rows"] for bi in bis] + [W[k] for k in wkeys] for bis, W in data]
    want = [[oracle_chain(O, bi, W, b, chain, gin)[-1] for bi in bis] for bis, W in data]
    params = [(n, n, n, F) for n in ns]
    for buf, h in zip(bufs, contents[0]):          # the plans are built from content 0 (occupancy bitmaps: of the adjacencies only)
        buf.copy_(torch.from_numpy(h.view(np.int32)).reshape(buf.shape))
    torch.cuda.synchronize(env.dev)
    if not planned:
        cts = [ClusterTensor(a, xc, xr) for a, xc, xr in zip(bitA, Xc, Xr)]
        plan = driver.BatchedEpoch(Q, cts, params, Wd, b, chain, gin, fuse=fuse, chain_stages=chain_stages)
        run = lambda: list(plan.run())             # noqa: E731
    else:
        ep = Q.EpochPlan(bitA, Xc, Xr, ns, 1, True, 0, F, False)
        plan = driver.PlannedEpoch(Q, ep, params, Wd, b, chain, gin, fuse=fuse, chain_stages=chain_stages)
        views = plan.outs                          # (reads the fill kernel's record once, here: never inside a probe or a capture)
        if rebind:
            def run():
                plan._bind()
                ep.run()
                return lambda: plan.outs           # the new pool's views exist once the bind has run: read after the capture has ended
        elif by_launch:
            def run():
                for i in range(plan.n_launches):
                    ep.run_launch(i)
                return views
        else:
            def run():
                ep.run()
                return views
    live = Live(torch, bufs, contents, want, run=run, keep=(plan, bitA))
    live.plan = plan
    return live


@case("BatchedGemm.run-reference-gcn", ["QGTC.BatchedGemm.run"])
def _bg_ref(env):
    live = _grouped_live(env, "reference", False, planned=False, seed=1)
    assert all(type(g).__name__ == "BatchedGemm" for g in live.plan.launches) and len(live.plan.launches) == 6
    return live


@case("BatchedGemm.run-reference-gin-4bit", ["QGTC.BatchedGemm.run"])
def _bg_gin(env):
    return _grouped_live(env, "reference", True, planned=False, b=4, seed=2)


@case("FusedLayer.run-correct-gcn", ["QGTC.FusedLayer.run"])
def _fused(env):
    live = _grouped_live(env, "correct", False, planned=False, chain_stages=False, seed=3)
    assert [type(g).__name__ for g in live.plan.launches] == ["FusedLayer"] * 3
    return live


@case("ChainedPair.run-correct-gcn", ["QGTC.ChainedPair.run"])
def _chained(env):
    live = _grouped_live(env, "correct", False, planned=False, seed=4)
    assert [type(g).__name__ for g in live.plan.launches] == ["BatchedGemm", "ChainedPair", "ChainedPair", "BatchedGemm"]
    return live


@case("ChainedPair.run-correct-gin-4bit", ["QGTC.ChainedPair.run"])
def _chained_gin(env):
    live = _grouped_live(env, "correct", True, planned=False, b=4, seed=5)
    assert [type(g).__name__ for g in live.plan.launches] == ["ChainedPair"] * 3
    return live


@case("EpochPlan.run-reference-gcn", ["QGTC.EpochPlan.run"])
def _plan_ref(env):
    live = _grouped_live(env, "reference", False, planned=True, seed=6)
    assert live.plan.n_launches == 6
    return live


@case("EpochPlan.run-correct-gcn-chain-entries", ["QGTC.EpochPlan.run"])
def _plan_chain(env):
    live = _grouped_live(env, "correct", False, planned=True, seed=7)
    assert live.plan.n_launches == 4               # qgtc_chain_transform + three qgtc_chain_aggregate
    return live


@case("EpochPlan.run-correct-gcn-layer-entries", ["QGTC.EpochPlan.run"])
def _plan_layers(env):
    live = _grouped_live(env, "correct", False, planned=True, chain_stages=False, seed=8)
    assert live.plan.n_launches == 3               # qgtc_gcn_layer_batched
    return live


@case("EpochPlan.run_launch-correct-gcn", ["QGTC.EpochPlan.run_launch"])
def _plan_by_launch(env):
    return _grouped_live(env, "correct", False, planned=True, by_launch=True, seed=9)


@case("EpochPlan.bind-correct-gcn-random-weights", ["QGTC.EpochPlan.bind"])
def _plan_bind(env):
    """bind() expands the weights of the chain entries (qgtc_expand_weights): the weights change with the content, so a bind that ran
    ahead of the copy expands the old ones."""
    live = _grouped_live(env, "correct", False, planned=True, rebind=True, seed=10)
    assert live.plan.n_launches == 4
    return live


# ---------------------------------------------------------------------------------------------------------------------------------------
# C entries with an explicit stream handle (ctypes, raw device pointers): the current stream stays the default one
# ---------------------------------------------------------------------------------------------------------------------------------------
def _out(env, n, dtype):
    """A caller-owned output of n elements with a 64-word canary behind it."""
    t = env.torch
    whole = t.empty(n * (2 if dtype == t.int64 else 1) + 64, dtype=t.int32, device=env.dev)
    out = whole[: n * (2 if dtype == t.int64 else 1)].view(dtype)
    out._canary = whole[n * (2 if dtype == t.int64 else 1):]
    return out


def raw_case(id, entry):
    return case(id, ["C." + entry], raw=True)


@raw_case("qgtc_val2bit-rows", "qgtc_val2bit")
def _raw_val2bit(env, H=37, W=130, nbits=3, cm=0):
    L, xs = cabi.load(), _val2bit_inputs(37, 130, 3, 201)
    buf, out = empty(env, (H, W), env.torch.float32), _out(env, int(L.qgtc_rows_words(H, W, nbits)), env.torch.int32)
    return Live(env.torch, [buf], [[x] for x in xs], [[env.O.val2bit(x, nbits, False, False)] for x in xs], outs=[out],
                raw=lambda st: L.qgtc_val2bit(buf.data_ptr(), H, W, nbits, 0, 0, out.data_ptr(), out.numel(), st))


@raw_case("qgtc_val2bit-cols", "qgtc_val2bit")
def _raw_val2bit_cols(env):
    H, W, nbits = 130, 37, 2
    L, xs = cabi.load(), _val2bit_inputs(H, W, nbits, 202)
    buf, out = empty(env, (H, W), env.torch.float32), _out(env, int(L.qgtc_cols_words(H, W, nbits, 0)), env.torch.int32)
    return Live(env.torch, [buf], [[x] for x in xs], [[env.O.val2bit(x, nbits, True, False)] for x in xs], outs=[out],
                raw=lambda st: L.qgtc_val2bit(buf.data_ptr(), H, W, nbits, 1, 0, out.data_ptr(), out.numel(), st))


def _raw_mm(entry, dims, flags, cols=False):
    M, K, N, a, w, ob = dims

    def build(env):
        L, O, t = cabi.load(), env.O, env.torch
        ops = [_mm_operands(O, M, K, N, a, w, 210 + k, ob=ob) for k in range(4)]
        bufs = [_i32(env, rows_shape(M, K, a)), _i32(env, cols_shape(K, N, w))]
        if entry == "qgtc_bitmm2int":
            out = _out(env, M * N, t.float32)
            want = [[O.bitmm2int(X, Wt, M, K, N, a, w, True)] for X, Wt in ops]
            raw = lambda st: L.qgtc_bitmm2int(bufs[0].data_ptr(), bufs[0].numel(), bufs[1].data_ptr(), bufs[1].numel(), M, K, N, a, w, 1,   # noqa: E731
                                              out.data_ptr(), out.numel(), flags, st)
        else:
            want = [[O.bitmm2bit(X, Wt, M, K, N, a, w, ob, col=cols)] for X, Wt in ops]
            out = _out(env, want[0][0].size, t.int32)
            raw = lambda st: L.qgtc_bitmm2bit(bufs[0].data_ptr(), bufs[0].numel(), bufs[1].data_ptr(), bufs[1].numel(), M, K, N, a, w, ob,  # noqa: E731
                                              out.data_ptr(), out.numel(), flags | (1 if cols else 0), st)
        return Live(t, bufs, [list(o) for o in ops], want, outs=[out], raw=raw)
    return build


CASES.append(Case("qgtc_bitmm2bit-auto", ["C.qgtc_bitmm2bit"], _raw_mm("qgtc_bitmm2bit", (300, 300, 64, 1, 2, 2), 0x10), raw=True))
CASES.append(Case("qgtc_bitmm2bit-popcount-cols", ["C.qgtc_bitmm2bit"], _raw_mm("qgtc_bitmm2bit", (129, 1000, 40, 2, 2, 3), 0x0, cols=True), raw=True))
CASES.append(Case("qgtc_bitmm2int-auto", ["C.qgtc_bitmm2int"], _raw_mm("qgtc_bitmm2int", (300, 300, 64, 1, 2, 2), 0x10), raw=True))
CASES.append(Case("qgtc_bitmm2int-mfma", ["C.qgtc_bitmm2int"], _raw_mm("qgtc_bitmm2int", (77, 500, 130, 3, 5, 4), 0x8), raw=True))


@raw_case("qgtc_pack_edges-3bit", "qgtc_pack_edges")
def _raw_pack_edges(env):
    """Sorted unique cells with their multiplicities (what QGTC.pack_edges hands over for nbits > 1): hipMemsetAsync, then atomic ORs.
    The four contents have the same number of distinct cells."""
    from oracle.qgtc_oracle import np_pack_edges

    L, H, W, nbits, n_cells = cabi.load(), 200, 333, 3, 900
    contents, want = [], []
    for k in range(4):
        rng = np.random.default_rng(220 + k)
        cells = np.sort(rng.choice(H * W, size=n_cells, replace=False)).astype(np.int64)
        counts = rng.integers(1, 10, size=n_cells).astype(np.int32)
        contents.append([cells, counts])
        want.append([np_pack_edges(np.repeat(cells // W, counts), np.repeat(cells % W, counts), H, W, nbits)])
    bufs = [empty(env, (n_cells,), env.torch.int64), _i32(env, (n_cells,))]
    out = _out(env, int(L.qgtc_rows_words(H, W, nbits)), env.torch.int32)
    return Live(env.torch, bufs, contents, want, outs=[out],
                raw=lambda st: L.qgtc_pack_edges(bufs[0].data_ptr(), bufs[1].data_ptr(), n_cells, H, W, nbits, out.data_ptr(), out.numel(), st))


@raw_case("qgtc_pack_edge_list", "qgtc_pack_edge_list")
def _raw_pack_edge_list(env):
    """The raw edge list behind QGTC.pack_edges(..., nbits=1, validate=False): three cleared bitmaps, atomic ORs, one finishing pass."""
    from oracle.qgtc_oracle import np_pack_edges

    L, H, W, n_edges = cabi.load(), 300, 333, 2000
    contents, want = [], []
    for k in range(4):
        rng = np.random.default_rng(225 + k)
        r, c = rng.integers(0, H, n_edges).astype(np.int64), rng.integers(0, W, n_edges).astype(np.int64)
        r[:60], c[:60] = np.tile(r[60:80], 3), np.tile(c[60:80], 3)          # multiplicities 2, 3 and 4
        r[20:40], c[20:40] = r[60:80], c[60:80]
        contents.append([r, c])
        want.append([np_pack_edges(r, c, H, W, 1)])
    words = int(L.qgtc_rows_words(H, W, 1))
    bufs = [empty(env, (n_edges,), env.torch.int64), empty(env, (n_edges,), env.torch.int64)]
    out, scratch = _out(env, words, env.torch.int32), _i32(env, (2 * words,))
    return Live(env.torch, bufs, contents, want, outs=[out], keep=scratch,
                raw=lambda st: L.qgtc_pack_edge_list(bufs[0].data_ptr(), bufs[1].data_ptr(), n_edges, H, W, out.data_ptr(), words, scratch.data_ptr(),
                                                     2 * words, None, st))


@raw_case("qgtc_tiled_colindex", "qgtc_tiled_colindex")
def _raw_colindex(env):
    from tiled_model import np_colindex

    L, gs, t = cabi.load(), cache_graphs(), env.torch
    bufs = _adjacency_buffers(env, gs)[:2]
    T, nq = int(bufs[1].numel()), CACHE_N // 128
    outs = [_out(env, nq + 1, t.int64), _out(env, T, t.int64), _out(env, T, t.int32)]
    ww = int(L.qgtc_tiled_colindex_work_words(T))
    work = _i32(env, (max(ww, 4),))
    return Live(t, bufs, [[g[2][0], g[2][1]] for g in gs], [list(np_colindex(g[2][0], g[2][1], CACHE_N)) for g in gs], outs=outs, keep=work,
                raw=lambda st: L.qgtc_tiled_colindex(bufs[0].data_ptr(), bufs[1].data_ptr(), T, CACHE_N, outs[0].data_ptr(), outs[1].data_ptr(),
                                                     outs[2].data_ptr(), work.data_ptr(), ww, st))


@raw_case("qgtc_tiled_degrees", "qgtc_tiled_degrees")
def _raw_degrees(env):
    from tiled_scaled_model import degrees, mean_scale

    L, gs, t, n = cabi.load(), cache_graphs(), env.torch, CACHE_N
    bufs = _adjacency_buffers(env, gs)
    T = int(bufs[1].numel())
    outs = [_out(env, n, t.int32), _out(env, n, t.int32), _out(env, n, t.float32), _out(env, n, t.float32)]
    want = []
    for s, d, _ in gs:
        o, i = degrees(s, d, n)
        want.append([o, i, mean_scale(o), mean_scale(i)])
    return Live(t, bufs, [list(g[2]) for g in gs], want, outs=outs,
                raw=lambda st: L.qgtc_tiled_degrees(bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), T, n, *[o.data_ptr() for o in outs], st))


def _raw_tiled_product(entry):
    """The transposed bit product and the two source-scaled float products on the cache graphs: tiles (and k-quads) AND X change."""
    def build(env):
        from tiled_model import aggregate, expected_bits, np_colindex
        from tiled_scaled_model import degrees
        from tiled_sym_model import aggregate_f32_src, inv_sqrt_degree

        L, gs, t, n, O = cabi.load(), cache_graphs(), env.torch, CACHE_N, env.O
        N, bit2, ob = 40, 2, 3
        adj = _adjacency_buffers(env, gs)
        T = int(adj[1].numel())
        transposed = entry != "qgtc_tiledmm_f32_src"
        contents, want = [], []
        for k, (s, d, (rp, kq, tl)) in enumerate(gs):
            rng = np.random.default_rng(230 + k)
            index = list(np_colindex(rp, kq, n)) if transposed else [rp, kq]
            if entry == "qgtc_tiledmm2bit_t":
                Xq = rand_q(rng, n, N, bit2)
                contents.append(index + [tl, O.pack(Xq, bit2, True)])
                want.append([expected_bits(O, aggregate(s, d, n, Xq, True), ob)])
            else:
                o, i = degrees(s, d, n)
                r, c = (inv_sqrt_degree(i), inv_sqrt_degree(o)) if transposed else (inv_sqrt_degree(o), inv_sqrt_degree(i))
                X = rng.normal(size=(n, N)).astype(np.float32)
                contents.append(index + [tl, X, r, c])
                want.append([aggregate_f32_src(s, d, n, X, transposed, r, c)])
        index_bufs = [empty(env, (n // 128 + 1,), t.int64), empty(env, (T,), t.int64), _i32(env, (T,))] if transposed else adj[:2]
        if entry == "qgtc_tiledmm2bit_t":
            X = _i32(env, cols_shape(n, N, bit2))
            out = _out(env, want[0][0].size, t.int32)
            bufs = index_bufs + [adj[2], X]
            raw = lambda st: L.qgtc_tiledmm2bit_t(*[b.data_ptr() for b in index_bufs], adj[2].data_ptr(), T, n, X.data_ptr(), X.numel(), N, bit2, ob,   # noqa: E731
                                                  out.data_ptr(), out.numel(), st)
        else:
            X, r, c = empty(env, (n, N), t.float32), empty(env, (n,), t.float32), empty(env, (n,), t.float32)
            out = _out(env, n * N, t.float32)
            bufs = index_bufs + [adj[2], X, r, c]
            fn = getattr(L, entry)
            raw = lambda st: fn(*[b.data_ptr() for b in index_bufs], adj[2].data_ptr(), T, n, X.data_ptr(), X.numel(), N, r.data_ptr(), c.data_ptr(),   # noqa: E731
                                out.data_ptr(), out.numel(), st)
        return Live(t, bufs, contents, want, outs=[out], raw=raw)
    return build


for _entry in ("qgtc_tiledmm2bit_t", "qgtc_tiledmm_f32_src", "qgtc_tiledmm_f32_t_src"):
    CASES.append(Case(_entry, ["C." + _entry], _raw_tiled_product(_entry), raw=True))


@raw_case("qgtc_gcn_chain_batched-auto", "qgtc_gcn_chain_batched")
def _raw_chain(env, flags=0x10):
    """As tests/test_abi_gpu.py::test_chain_entry_with_raw_descriptors: host-written descriptors; T (the aggregation's right operand)
    and the next layer's weight change with the content."""
    L, O, t = cabi.load(), env.O, env.torch
    act, wb, f1, f2, ns = 2, 2, 128, 96, [150, 333, 40]
    rng = np.random.default_rng(240)
    As = [O.pack((rng.random((n, n)) < 1.5 / n).astype(np.int32), 1, False) for n in ns]     # sparse: the sums stay below the clamp
    dA = [t.from_numpy(A.view(np.int32)).to(env.dev) for A in As]
    dT = [_i32(env, (int(L.qgtc_cols_words(n, f1, act, 0)),)) for n in ns]
    dW = _i32(env, (int(L.qgtc_cols_words(f1, f2, wb, 0)),))
    outs = [_out(env, int(L.qgtc_rows_words(n, f1, act)), t.int32) for n in ns] + [_out(env, int(L.qgtc_cols_words(n, f2, act, 0)), t.int32) for n in ns]
    contents, want = [], []
    for k in range(4):
        rk = np.random.default_rng(241 + k)
        Ts = [O.pack(rand_q(rk, n, f1, act), act, True) for n in ns]
        W2 = O.pack(rand_q(rk, f1, f2, wb, 0.01), wb, True)
        agg = [O.bitmm2bit(A, T, n, n, f1, 1, act, act) for A, T, n in zip(As, Ts, ns)]
        contents.append(Ts + [W2])
        want.append(agg + [O.bitmm2bit(a, W2, n, f1, f2, act, wb, act, col=True) for a, n in zip(agg, ns)])
    P128 = lambda x: (x + 127) // 128 * 128   # noqa: E731
    count = len(ns)
    sa = [QgtcProblem(dA[i].data_ptr(), dT[i].data_ptr(), outs[i].data_ptr(), dA[i].numel(), dT[i].numel(), n, n, f1, P128(f1), 0, None) for i, n in enumerate(ns)]
    sx = [QgtcProblem(outs[i].data_ptr(), dW.data_ptr(), outs[count + i].data_ptr(), outs[i].numel(), dW.numel(), n, f1, f2, P128(f2), 0, None)
          for i, n in enumerate(ns)]
    descs = t.frombuffer(bytearray(bytes((QgtcProblem * (2 * count))(*(sa + sx)))), dtype=t.uint8).to(env.dev)
    return Live(t, dT + [dW], contents, want, outs=outs, keep=(dA, descs),
                raw=lambda st: L.qgtc_gcn_chain_batched(descs.data_ptr(), descs.data_ptr() + 72 * count, count, max(ns), max(ns), f1, f2, 1, act, act, wb,
                                                        act, 1, flags, st))


def _raw_load_batches(with_work):
    """As tests/test_loader_gpu.py::test_load_batches_through_the_raw_abi: the features change with the content, and the edges move
    inside their batches (the same edge counts). Without a work buffer the entry clears `zero` itself (hipMemsetAsync) and ORs into it."""
    def build(env):
        L, O, t = cabi.load(), env.O, env.torch
        sizes, F, bits = [70, 257, 5], 20, 2
        rng = np.random.default_rng(250)
        ecounts = [int(rng.integers(n, 8 * n)) for n in sizes]
        a_words = [int(L.qgtc_rows_words(n, n, 1)) for n in sizes]
        x_words = [int(L.qgtc_cols_words(n, F, bits, 0)) for n in sizes]
        contents, want = [], []
        for k in range(4):
            rk = np.random.default_rng(251 + k)
            rows = [rk.integers(0, n, ne).astype(np.int64) for n, ne in zip(sizes, ecounts)]
            cols = [rk.integers(0, n, ne).astype(np.int64) for n, ne in zip(sizes, ecounts)]
            feats = [(rk.normal(size=(n, F)) * 2.0).astype(np.float32) for n in sizes]
            contents.append([np.concatenate(rows), np.concatenate(cols), np.concatenate(feats)])
            dense = []
            for n, r, c in zip(sizes, rows, cols):
                A = np.zeros((n, n), dtype=np.float32)
                np.add.at(A, (r, c), 1.0)
                dense.append(O.val2bit(A, 1))
            want.append([np.concatenate(dense), np.concatenate([O.val2bit(x, bits, True) for x in feats])])
        src, dst = empty(env, (sum(ecounts),), t.int64), empty(env, (sum(ecounts),), t.int64)
        X = empty(env, (sum(sizes), F), t.float32)
        # [A of every batch | stats (4 words) | scratch]: the first sum(a_words) words are the output, the rest is the entry's own
        zero = _i32(env, (3 * sum(a_words) + 4,))
        out_a = zero[: sum(a_words)]
        out_x = _out(env, sum(x_words), t.int32)
        table, e0, f0, a0, x0 = [], 0, 0, 0, 0
        for n, ne, aw, xw in zip(sizes, ecounts, a_words, x_words):
            table.append(QgtcLoaderBatch(e0, ne, f0, n, 0, zero.data_ptr() + 4 * a0, None if with_work else zero.data_ptr() + 4 * (sum(a_words) + 4 + 2 * a0),
                                         None, None, out_x.data_ptr() + 4 * x0, None, None))
            e0, f0, a0, x0 = e0 + ne, f0 + n, a0 + aw, x0 + xw
        dev_table = t.frombuffer(bytearray(bytes((QgtcLoaderBatch * len(sizes))(*table))), dtype=t.uint8).to(env.dev)
        stats_ptr = zero.data_ptr() + 4 * sum(a_words)
        ww = int(L.qgtc_load_work_words(len(sizes), max(sizes), sum(ecounts)))
        work = _i32(env, (max(ww, 4),))
        assert ww > 0, "the bucketed route is switched off (QGTC_NO_LOAD_SORT)"
        if with_work:
            raw = lambda st: L.qgtc_load_batches(dev_table.data_ptr(), len(sizes), max(sizes), max(ecounts), src.data_ptr(), dst.data_ptr(), X.data_ptr(),   # noqa: E731
                                                 F, bits, stats_ptr, 16, stats_ptr, None, 0, work.data_ptr(), ww, st)
        else:
            raw = lambda st: L.qgtc_load_batches(dev_table.data_ptr(), len(sizes), max(sizes), max(ecounts), src.data_ptr(), dst.data_ptr(), X.data_ptr(),   # noqa: E731
                                                 F, bits, zero.data_ptr(), zero.numel() * 4, stats_ptr, None, 0, None, 0, st)
        return Live(t, [src, dst, X], contents, want, outs=[out_a, out_x], raw=raw, keep=(zero, dev_table, work))
    return build


CASES.append(Case("qgtc_load_batches-bitmaps", ["C.qgtc_load_batches"], _raw_load_batches(False), raw=True))
CASES.append(Case("qgtc_load_batches-buckets", ["C.qgtc_load_batches"], _raw_load_batches(True), raw=True))

# the C entries the issue of this test suite names: each has at least one raw case (tests/test_stream_contract.py)
RAW_ENTRIES = ("qgtc_val2bit", "qgtc_bitmm2bit", "qgtc_bitmm2int", "qgtc_pack_edges", "qgtc_tiledmm2bit_t", "qgtc_tiledmm_f32_src",
               "qgtc_tiledmm_f32_t_src", "qgtc_tiled_degrees", "qgtc_tiled_colindex", "qgtc_gcn_chain_batched", "qgtc_load_batches")
