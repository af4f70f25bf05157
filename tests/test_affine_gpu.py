"""Affine quantisation on the GPU (qgtc_ppopp22_amd/affine.py over include/qgtc_affine.h) against tests/affine_model.py, bit for bit:
the range launch, the fused quantise + pack with its code sums, the dequantising epilogue, ``linear``, ``aggregate`` and the layer, and the
refusals. ``linear`` and the layer are also held to float64 (the first-order bound; 8 bits closer than 4). The shapes are the smallest
that reach each path: the float4 and the general packer, more than one 256-column chunk, more than one workgroup of range partials, every
row slice of the per-column range, and code sums of lines shorter and longer than a wave's 64 words. (The 64-bit index branches are
launch-uniform and need more than 2^31 units: no test has that size.)"""
import types

import numpy as np
import pytest

import affine_model as am
import tiled_nodes_model as nm
from dirty_memory import same_as_model
from tiled_model import random_edges

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def env(qgtc, oracle):
    import torch
    from qgtc_ppopp22_amd import affine

    return types.SimpleNamespace(torch=torch, Q=qgtc, O=oracle, af=affine, dev=torch.device("cuda:0"))


def up(env, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return env.torch.from_numpy(a).to(env.dev)


def up_off4(env, a):
    """a on the device at a base 4 bytes past a 16-byte boundary: contiguous, but no float4 may be read from it"""
    torch = env.torch
    buf = torch.empty(a.size + 1, dtype=torch.float32, device=env.dev)
    v = buf[1:].view(a.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def values(rng, H, W, kind=0):
    x = rng.normal(size=(H, W)) * (10.0 ** rng.integers(-2, 3)) + (0.0, 2.5, -40.0)[kind % 3]
    return (x * 2.0 ** rng.integers(-3, 4, size=(1, W))).astype(F32)


SPECIAL = {
    "negative": np.array([-3.0, -1.5, -0.25, -7.0], F32), "positive": np.array([0.5, 2.0, 7.0, 1.0], F32), "zero": np.zeros(4, F32),
    "signed zeros": np.array([-0.0, 0.0, -0.0, 0.0], F32), "constant": np.full(4, 2.5, F32),
    "nothing finite": np.array([np.nan, np.inf, -np.inf, np.nan], F32), "nan and inf": np.array([np.nan, -2.0, np.inf, 6.0], F32),
    "tiny": np.array([0.0, 2.0 ** -110, 0.0, 2.0 ** -120], F32), "tiny negative": np.array([-(2.0 ** -110), 0.0, 0.0, 0.0], F32)}


# ----------------------------------------------------------------------------------------------------------------------------------
# qparams
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (7, 9), (1, 64), (5, 13), (257, 1), (70, 131)], ids=str)   # H W = 1, 63, 64, 65, 257; 9170 = 3 workgroups
def test_qparams_per_tensor(env, shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    for k, bits in enumerate((1, 2, 4, 8)):
        x = values(rng, *shape, kind=k)
        x[rng.integers(0, shape[0]), rng.integers(0, shape[1])] = (np.nan, np.inf, -np.inf, 1.0)[k]
        for move in (up, up_off4):
            got = env.af.qparams(move(env, x), bits)
            same_as_model([got.cpu()], [am.qparams(x, bits)], f"qparams {shape} {bits} bits {move.__name__}")


@pytest.mark.parametrize("shape", [(1, 1), (33, 5), (257, 64), (40, 130), (2100, 3)], ids=str)   # (2100, 3): every one of the 64 row slices
def test_qparams_per_column(env, shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1] + 1)
    for k, bits in enumerate((1, 2, 4, 8)):
        x = values(rng, *shape, kind=k)
        x[rng.integers(0, shape[0]), rng.integers(0, shape[1])] = (np.nan, np.inf, -np.inf, 1.0)[k]
        got = env.af.qparams(up(env, x), bits, per_column=True)
        same_as_model([got.cpu()], [am.qparams(x, bits, True)], f"qparams per column {shape} {bits} bits")


@pytest.mark.parametrize("bits", (1, 2, 4, 8))
def test_qparams_on_the_special_ranges(env, bits):
    for name, v in SPECIAL.items():
        x = v.reshape(2, 2)
        same_as_model([env.af.qparams(up(env, x), bits).cpu()], [am.qparams(x, bits)], f"qparams {name} {bits} bits")
    x = np.stack(list(SPECIAL.values()), axis=1)      # one special range per column
    same_as_model([env.af.qparams(up(env, x), bits, True).cpu()], [am.qparams(x, bits, True)], f"qparams per column, special, {bits} bits")
    x = am.tie_inputs(bits)
    same_as_model([env.af.qparams(up(env, x), bits).cpu()], [am.qparams(x, bits)], f"qparams ties {bits} bits")


# ----------------------------------------------------------------------------------------------------------------------------------
# val2bit_affine
# ----------------------------------------------------------------------------------------------------------------------------------
def check_pack(env, x, bits, qp, col_major, what, move=up):
    q = am.quantise(x, qp, bits)
    want = env.O.pack(q, bits, col_major, False).view(np.int32)
    dx, dq = move(env, x), up(env, qp)
    words, sums = env.af.val2bit_affine(dx, bits, dq, col_major)
    H, W = x.shape
    rows = (bits * ((H + 127) // 128) * 4, (W + 127) // 128 * 128) if col_major else (bits * ((H + 7) // 8 * 8), (W + 127) // 128 * 4)
    assert tuple(words.shape) == rows and words.dtype == env.torch.int32, what
    same_as_model([words.reshape(-1).cpu(), sums.cpu()], [want, am.sums(q, col_major)], what)
    words, none = env.af.val2bit_affine(dx, bits, dq, col_major, return_sums=False)
    assert none is None
    same_as_model([words.reshape(-1).cpu()], [want], what + ", without sums")


@pytest.mark.parametrize("col_major", [False, True], ids=["rows", "cols"])
# (3, 2100) and (2100, 3): a line of more than 64 words, whose code sum takes a whole workgroup
@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (33, 130), (100, 260), (37, 256), (3, 2100), (2100, 3)], ids=str)
def test_val2bit_affine(env, shape, col_major):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1] + 2 + col_major)
    for k, bits in enumerate((1, 2, 3, 4, 8)):
        x = values(rng, *shape, kind=k)
        for per_column in (False, True):
            check_pack(env, x, bits, am.qparams(x, bits, per_column), col_major, f"val2bit_affine {shape} {bits} bits per_column={per_column}")
        if shape[1] % 4 == 0:    # off the float4 alignment: the general packer at a W the fast one would take
            check_pack(env, x, bits, am.qparams(x, bits), col_major, f"val2bit_affine {shape} {bits} bits, base + 4 bytes", move=up_off4)


@pytest.mark.parametrize("col_major", [False, True], ids=["rows", "cols"])
def test_val2bit_affine_on_nan_inf_and_ties(env, col_major):
    rng = np.random.default_rng(9)
    for shape in ((33, 130), (37, 256)):
        x = values(rng, *shape)
        bad = rng.random(shape)
        x[bad < 0.05] = np.nan
        x[(bad > 0.05) & (bad < 0.1)] = np.inf
        x[(bad > 0.1) & (bad < 0.15)] = -np.inf
        x[:, 3] = np.nan                       # a group without a finite element
        for bits in (1, 4, 8):
            for per_column in (False, True):
                check_pack(env, x, bits, am.qparams(x, bits, per_column), col_major, f"val2bit_affine NaN / inf {shape} {bits} bits {per_column}")
    for bits in (2, 4, 8):
        x = am.tie_inputs(bits)
        check_pack(env, x, bits, am.qparams(x, bits), col_major, f"val2bit_affine ties {bits} bits")
        check_pack(env, np.ascontiguousarray(x.T), bits, am.qparams(x, bits), col_major, f"val2bit_affine ties as a column {bits} bits")
        x4 = np.ascontiguousarray(np.tile(x, (3, 4))[:, : x.shape[1] * 4 // 4 * 4])       # the float4 path in the rows layout
        check_pack(env, x4, bits, am.qparams(x4, bits), col_major, f"val2bit_affine ties, W % 4 == 0, {bits} bits")


# ----------------------------------------------------------------------------------------------------------------------------------
# dequant
# ----------------------------------------------------------------------------------------------------------------------------------
def qrow(rng, n, bits=8):
    s = (rng.random(n) * 0.1 + 0.001).astype(F32)
    z = rng.integers(0, 2 ** bits, size=n).astype(F32)
    return np.stack([s, z, (F32(1) / s).astype(F32), np.zeros(n, F32)], axis=1).astype(F32)


@pytest.mark.parametrize("shape", [(1, 1), (33, 7), (100, 64), (130, 130)], ids=str)
def test_dequant(env, shape):
    M, N = shape
    rng = np.random.default_rng(M * 1000 + N)
    K = int(rng.integers(1, 500))
    acc = rng.integers(0, 2 ** 22, size=shape).astype(F32)
    qa = qrow(rng, 1)
    rs, cs = rng.integers(0, 255 * K + 1, size=M).astype(np.int32), rng.integers(0, 255 * K + 1, size=N).astype(np.int32)
    scale, bias = rng.normal(size=M).astype(F32), rng.normal(size=N).astype(F32) * F32(100)
    d = {k: up(env, v) for k, v in dict(acc=acc, qa=qa, rs=rs, cs=cs, scale=scale, bias=bias).items()}
    for groups in (1, N):
        qb = qrow(rng, groups)
        dqb = up(env, qb)
        for mask in range(8):
            for drop in range(4):
                if drop and mask not in (0, 7):
                    continue
                use_s, use_b, relu = bool(mask & 1), bool(mask & 2), bool(mask & 4)
                no_rs, no_cs = bool(drop & 1), bool(drop & 2)
                want = am.dequant(acc, K, qa, None if no_rs else rs, qb, None if no_cs else cs, scale if use_s else None,
                                  bias if use_b else None, relu)
                got = env.af.dequant(d["acc"], K, d["qa"], None if no_rs else d["rs"], dqb, None if no_cs else d["cs"],
                                     d["scale"] if use_s else None, d["bias"] if use_b else None, relu)
                what = f"dequant {shape} groups {groups} row_scale={use_s} bias={use_b} relu={relu} row_sums={not no_rs} col_sums={not no_cs}"
                assert got.data_ptr() != d["acc"].data_ptr()
                same_as_model([got.cpu()], [want], what)
        # in place
        mine = d["acc"].clone()
        got = env.af.dequant(mine, K, d["qa"], d["rs"], dqb, d["cs"], d["scale"], d["bias"], True, out=mine)
        assert got is mine
        same_as_model([mine.cpu()], [am.dequant(acc, K, qa, rs, qb, cs, scale, bias, True)], f"dequant {shape} in place")


def test_dequant_needs_its_64_bits(env):
    """an accumulator at 2^24 - 1 with K za zb far beyond 2^31, and sums that bring t back"""
    rng = np.random.default_rng(3)
    M, N, K = 5, 6, 2 ** 31 - 1
    acc = np.full((M, N), 2.0 ** 24 - 1, F32)
    acc[1:] = rng.integers(0, 2 ** 24, size=(M - 1, N)).astype(F32)
    qa = np.array([[0.5, 255, 2, 0]], F32)
    qb = qrow(rng, N)
    qb[0, 1], qb[1, 1] = 255, 0
    rs = rng.integers(2 ** 30, 2 ** 31 - 1, size=M).astype(np.int32)
    cs = rng.integers(2 ** 30, 2 ** 31 - 1, size=N).astype(np.int32)
    t = am.dequant_t(acc, K, qa, rs, qb, cs)
    assert int(np.abs(t).max()) > 2 ** 40 and int(t[0, 0]) == 2 ** 24 - 1 + K * 255 * 255 - 255 * int(rs[0]) - 255 * int(cs[0])
    for args in ((rs, cs), (None, None), (rs, None)):
        got = env.af.dequant(up(env, acc), K, up(env, qa), None if args[0] is None else up(env, args[0]), up(env, qb),
                             None if args[1] is None else up(env, args[1]))
        same_as_model([got.cpu()], [am.dequant(acc, K, qa, args[0], qb, args[1])], "dequant beyond 32 bits")


# ----------------------------------------------------------------------------------------------------------------------------------
# linear
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_column", [True, False], ids=["per column", "per tensor"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (33, 20, 7), (100, 130, 64)], ids=str)
def test_linear(env, shape, per_column):
    M, K, N = shape
    rng = np.random.default_rng(M + K + N)
    X, W = values(rng, M, K, 1), values(rng, K, N)
    scale, bias = (rng.random(M) + 0.5).astype(F32), rng.normal(size=N).astype(F32)
    dX, dW = up(env, X), up(env, W)
    for a_bits, w_bits in ((8, 8), (8, 4), (4, 2), (1, 1)):
        what = f"linear {shape} a{a_bits} w{w_bits} per_column={per_column}"
        got = env.af.linear(dX, dW, a_bits, w_bits, per_column)
        want = am.linear(X, W, a_bits, w_bits, per_column)
        same_as_model([got.cpu()], [want], what)
        qa, _, qb, _, _ = am.linear_parts(X, W, a_bits, w_bits, per_column)
        err = np.abs(got.cpu().numpy().astype(np.float64) - X.astype(np.float64) @ W.astype(np.float64))
        assert (err <= am.linear_bound(X, W, qa, qb, want)).all(), what
        got = env.af.linear(dX, dW, a_bits, w_bits, per_column, up(env, scale), up(env, bias), True)
        same_as_model([got.cpu()], [am.linear(X, W, a_bits, w_bits, per_column, scale, bias, True)], what + ", epilogue")
    assert not got.requires_grad


# ----------------------------------------------------------------------------------------------------------------------------------
# aggregate
# ----------------------------------------------------------------------------------------------------------------------------------
def graph(n, seed=0):
    src, dst = (np.asarray(a, dtype=np.int64) for a in random_edges(np.random.default_rng(seed + n), n, 3 * n))
    return src, dst


@pytest.fixture(scope="module")
def graphs(env):
    out = {}
    for n in (100, 300):
        src, dst = graph(n)
        s, d = up(env, src), up(env, dst)
        out[n] = (src, dst, env.Q.pack_edges_tiled(s, d, n), env.Q.pack_edges_tiled(s, d, n, reorder=True))
    return out


@pytest.mark.parametrize("reorder", [False, True], ids=["plain", "reordered"])
@pytest.mark.parametrize("transposed", [False, True], ids=["adj", "adjT"])
@pytest.mark.parametrize("n", [100, 300])
def test_aggregate(env, graphs, n, transposed, reorder):
    src, dst, plain, reordered = graphs[n]
    base = reordered if reorder else plain
    adj = base.T if transposed else base
    A = am.dense_view(src, dst, n, transposed)
    assert (A[32:64].sum() == 0) if not transposed else (A[:, 32:64].sum() == 0)      # random_edges leaves row block 1 of the adjacency empty
    rng = np.random.default_rng(n + 2 * transposed + reorder)
    R, S = rng.random(n) < 0.5, rng.random(n) < 0.5
    to_new = (lambda f: f[base.perm.cpu().numpy()]) if reorder else (lambda f: f)
    rm, sm = up(env, nm.bitmap(to_new(R))), up(env, nm.bitmap(to_new(S)))
    for N in (5, 40):
        T = values(rng, n, N, N % 3)
        dT = adj.to_new(up(env, T)).contiguous()
        for bits in (2, 8):
            what = f"aggregate n={n} N={N} {bits} bits transposed={transposed} reorder={reorder}"
            got = adj.to_old(env.af.aggregate(adj, dT, bits))
            same_as_model([got.cpu()], [am.aggregate(A, T, bits)], what)
            got = adj.to_old(env.af.aggregate(adj, dT, bits, adj.mean_scale()))
            same_as_model([got.cpu()], [am.aggregate(A, T, bits, am.inv_degree(A.sum(axis=1)))], what + ", mean")
            got = adj.to_old(env.af.aggregate(adj, dT, bits, row_mask=rm, nbr_mask=sm))
            want = am.aggregate(A, T, bits, None, R, S)
            same_as_model([got.cpu()], [want], what + ", masks")
            dead = am.masked_view(A, R, S).sum(axis=1) == 0
            assert (~R).any() and (got.cpu().numpy()[dead].view(np.uint32) == 0).all(), what      # +0 outside row_mask and without live neighbours
            scale = adj.mean_scale(row_mask=rm, nbr_mask=sm)
            got = adj.to_old(env.af.aggregate(adj, dT, bits, scale, row_mask=rm, nbr_mask=sm))
            same_as_model([got.cpu()], [am.aggregate(A, T, bits, am.inv_degree(am.masked_view(A, R, S).sum(axis=1)), R, S)], what + ", masked mean")


# ----------------------------------------------------------------------------------------------------------------------------------
# the layer
# ----------------------------------------------------------------------------------------------------------------------------------
DIMS = (12, 20, 7)


def layer_inputs(n, seed=0):
    rng = np.random.default_rng(seed)
    F, H, C = DIMS
    return tuple(rng.normal(size=s).astype(F32) for s in ((n, F), (F, H), (H, C))) + (rng.random(n) < 0.6,)


@pytest.mark.parametrize("reorder", [False, True], ids=["plain", "reordered"])
@pytest.mark.parametrize("transposed", [False, True], ids=["adj", "adjT"])
@pytest.mark.parametrize("norm", [None, "mean", "sym"])
def test_the_layer_is_the_model_composed(env, graphs, norm, transposed, reorder):
    torch, n = env.torch, 300
    src, dst, plain, reordered = graphs[n]
    base = reordered if reorder else plain
    adj = base.T if transposed else base
    A = am.dense_view(src, dst, n, transposed)
    X, W_in, W_out, nodes = layer_inputs(n)
    for w_bit, act_bit in ((4, 8), (8, 8)):
        layer = env.af.GCNConv_Affine(*DIMS, w_bit=w_bit, act_bit=act_bit, norm=norm).to(env.dev)
        with torch.no_grad():
            layer.W_in.copy_(up(env, W_in))
            layer.W_out.copy_(up(env, W_out))
        what = f"GCNConv_Affine norm={norm} w{w_bit} a{act_bit} transposed={transposed} reorder={reorder}"
        got = layer(adj, up(env, X))
        assert not got.requires_grad and tuple(got.shape) == (n, DIMS[2])
        same_as_model([got.cpu()], [am.gcn(A, X, W_in, W_out, w_bit, act_bit, norm)], what)
        got = layer(adj, up(env, X), nodes=up(env, nodes))
        want = am.gcn(A, X, W_in, W_out, w_bit, act_bit, norm, nodes)
        same_as_model([got.cpu()], [want], what + ", nodes")
        assert (got.cpu().numpy()[~nodes].view(np.uint32) == 0).all(), what


@pytest.mark.parametrize("norm", [None, "mean", "sym"])
def test_from_float_follows_the_float_layer(env, graphs, norm):
    """(8, 8) reproduces the float layer more closely than (4, 4): the model on the CPU says so at these seeds
    (tests/test_affine_model.py, the composition), and the errors here are the model's"""
    from qgtc_ppopp22_amd import conv

    torch, n = env.torch, 300
    src, dst, adj, _ = graphs[n]
    X, W_in, W_out, _ = layer_inputs(n)
    torch.manual_seed(0)
    ref = conv.GCNConv(*DIMS, norm=norm).to(env.dev)
    with torch.no_grad():
        ref.W_in.copy_(up(env, W_in))
        ref.W_out.copy_(up(env, W_out))
        want = ref(adj, up(env, X)).double().cpu().numpy()
    errs = {}
    for bits in (4, 8):
        q = env.af.GCNConv_Affine.from_float(ref, bits, bits)
        assert q.norm == norm and q.W_in is not ref.W_in and torch.equal(q.W_in, ref.W_in) and torch.equal(q.W_out, ref.W_out)
        errs[bits] = am.rel_error(q(adj, up(env, X)).double().cpu().numpy(), want)
    print(f"norm={norm}: relative error against the float layer {errs}")
    assert errs[8] < errs[4] and errs[8] < 0.1


# ----------------------------------------------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------------------------------------------
def test_the_refusals(env, graphs):
    from qgtc_ppopp22_amd import conv

    torch, af = env.torch, env.af
    x = up(env, np.ones((8, 6), F32))
    qp = af.qparams(x, 4)
    for bits in (0, 9, -1):
        with pytest.raises(ValueError, match="bits"):
            af.qparams(x, bits)
        with pytest.raises(ValueError, match="bits"):
            af.val2bit_affine(x, bits, qp)
        with pytest.raises(ValueError, match="a_bits"):
            af.linear(x, x.t().contiguous(), bits, 4)
        with pytest.raises(ValueError, match="w_bits"):
            af.linear(x, x.t().contiguous(), 4, bits)
    with pytest.raises(TypeError, match="bits"):
        af.qparams(x, 4.0)
    for bad, exc in ((x.double(), TypeError), (x.to(torch.int32), TypeError), (x.t(), ValueError), (x.cpu(), ValueError), (x[0], ValueError),
                     ([1.0], TypeError)):
        with pytest.raises(exc, match="x"):
            af.qparams(bad, 4)
        with pytest.raises(exc, match="x"):
            af.val2bit_affine(bad, 4, qp)
        with pytest.raises(exc, match="acc"):
            af.dequant(bad, 3, qp, None, qp, None)
    for bad in (up(env, np.ones((2, 4), F32)), up(env, np.ones((1, 3), F32)), up(env, np.ones((4,), F32)), up(env, np.ones((8, 4), F32))):
        with pytest.raises(ValueError, match="qp"):       # groups other than 1 or W = 6
            af.val2bit_affine(x, 4, bad)
        with pytest.raises(ValueError, match="qb"):
            af.dequant(x, 3, qp, None, bad, None)
    with pytest.raises(ValueError, match="qa"):
        af.dequant(x, 3, af.qparams(x, 4, True), None, qp, None)
    with pytest.raises(TypeError, match="qp"):
        af.val2bit_affine(x, 4, qp.double())
    with pytest.raises(ValueError, match="qp"):
        af.val2bit_affine(x, 4, qp.cpu())
    with pytest.raises(TypeError, match="row_sums"):
        af.dequant(x, 3, qp, torch.zeros(8, device=env.dev), qp, None)
    with pytest.raises(ValueError, match="col_sums"):
        af.dequant(x, 3, qp, None, qp, torch.zeros(5, dtype=torch.int32, device=env.dev))
    with pytest.raises(ValueError, match="K"):
        af.dequant(x, 0, qp, None, qp, None)
    with pytest.raises(ValueError, match="W"):
        af.linear(x, x, 4, 4)
    with pytest.raises(ValueError, match="2\\^24"):
        af.linear(up(env, np.ones((2, 300), F32)), up(env, np.ones((300, 2), F32)), 8, 8)
    adj = graphs[100][2]
    with pytest.raises(TypeError, match="TiledAdjacency"):
        af.aggregate(x, x, 4)
    with pytest.raises(ValueError, match="T"):
        af.aggregate(adj, x, 4)
    layer = af.GCNConv_Affine(6, 5, 3).to(env.dev)
    with pytest.raises(NotImplementedError, match="TiledAdjacency"):
        layer(torch.ones(8, 8, device=env.dev), x)
    with pytest.raises(ValueError, match="norm"):
        af.GCNConv_Affine(6, 5, 3, norm="max")
    with pytest.raises(ValueError, match="w_bit"):
        af.GCNConv_Affine(6, 5, 3, w_bit=9)
    with pytest.raises(ValueError, match="aggr"):
        af.GCNConv_Affine.from_float(conv.GCNConv(6, 5, 3, aggr="max"), 4, 8)
    with pytest.raises(ValueError, match="edge_drop"):
        af.GCNConv_Affine.from_float(conv.GCNConv(6, 5, 3, edge_drop=0.5), 4, 8)
    with pytest.raises(TypeError, match="GCNConv"):
        af.GCNConv_Affine.from_float(layer, 4, 8)
