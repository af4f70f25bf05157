"""Every layer of qgtc_ppopp22_amd/conv.py and sage.py as a long-lived object (the rows of tests/module_state_cases.py): a layer always
computes with the values its parameters and hyper-parameters hold at the call, however they were written; it survives copies and
checkpoints with its bits; it draws from torch's CPU generator only in ``train()`` with sampling active and no seed given; and it keeps
nothing from one graph to the next.

The comparison object is the FRESH TWIN: a newly constructed layer of the same class and hyper-parameters whose parameters are set by
``copy_`` under ``no_grad`` from the values the tested layer now holds, and which is called once. A fresh layer has no warm cache, so it
cannot be stale. Every comparison with a twin is bit for bit, on the output and on every parameter gradient.

A twin is the project's own code, so each row is also ANCHORED once per property to its independent definition (``mc.reference``): the
layer's output, at the parameter values it holds then, equals the dense float64 definition (the integer chain for GCNConv_Qnt) - bit for
bit on the dyadic graph with integer data where the definition is exact in float32, within layers_reference.tolerances on the random
graph otherwise - on ``adj`` and on the transposed view of the reordered adjacency."""
import copy
import io

import numpy as np
import pytest

import layers_reference as R
import module_state_cases as mc

pytestmark = pytest.mark.gpu

SEED, OTHER_SEED = mc.SEED, mc.OTHER_SEED
_CACHE = {}


class _Env:
    pass


@pytest.fixture(scope="module")
def env(qgtc, oracle):
    import torch

    e = _Env()
    e.torch, e.Q, e.O = torch, qgtc, oracle
    e.forms = {graph: mc.forms(torch, qgtc, graph) for graph in mc.GRAPHS}
    return e


def _dev(env, a):
    return env.torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _X(env, row, n):
    key = ("X", row.name, n)
    if key not in _CACHE:
        _CACHE[key] = _dev(env, mc.features(row, n))
    return _CACHE[key]


def _dY(env, shape):
    key = ("dY", tuple(shape))
    if key not in _CACHE:
        _CACHE[key] = _dev(env, np.random.default_rng(len(shape) + 31 * int(np.prod(shape))).standard_normal(tuple(shape)).astype(np.float32))
    return _CACHE[key]


def _named(layer, row):
    named = dict(layer.named_parameters())
    return {name: named[name] for name in row.params}


def _snapshot(layer, row):
    return {name: p.detach().cpu().numpy().copy() for name, p in _named(layer, row).items()}


def _start(env, row, which="new", **hyper):
    """A layer on the device in ``train()`` holding mc.old_values / mc.new_values, written through ``.data``: the parameters of the
    quantised layer stay at version 0, as in a layer that was only ever initialised the old way."""
    layer = row.make(**hyper).cuda().train()
    values = mc.old_values(row, layer) if which == "old" else mc.new_values(row, layer)
    for name, p in _named(layer, row).items():
        p.data.copy_(_dev(env, values[name]))
    if row.quantised:
        assert all(p._version == 0 for p in layer.parameters())
    return layer


def _twin(env, row, layer, training=None, **hyper):
    """The fresh twin of ``layer`` (with ``hyper`` over the row's): new object, parameters by copy_ under no_grad, never called."""
    twin = row.make(**hyper).cuda()
    twin.train(layer.training if training is None else training)
    ours = _named(layer, row)
    with env.torch.no_grad():
        for name, p in _named(twin, row).items():
            p.copy_(ours[name].detach())
    return twin


def _run(env, row, layer, A, seed=SEED):
    """(Y, {name: gradient}): one forward on the form ``A`` and, for the trainable layers, one backward."""
    for p in layer.parameters():
        p.grad = None
    Y = row.call(layer, A, _X(env, row, A.n), seed)
    grads = {}
    if not row.quantised:
        Y.backward(_dY(env, Y.shape))
        grads = {name: p.grad.detach().clone() for name, p in _named(layer, row).items()}
        assert all(g is not None for g in grads.values())
    return Y.detach().clone(), grads


def _bits(env, t):
    return t.contiguous().view(env.torch.int32)


def _differences(env, got, want, label):
    """The tensors of ``got`` that are not ``want``'s bits."""
    (Y, g), (Yw, gw) = got, want
    assert set(g) == set(gw) and Y.shape == Yw.shape and Y.dtype == Yw.dtype == env.torch.float32, label
    bad = []
    for name, a, b in [("Y", Y, Yw)] + [("d" + k, g[k], gw[k]) for k in sorted(g)]:
        diff = _bits(env, a) != _bits(env, b)
        if bool(diff.any()):
            bad.append(f"{label} {name}: {int(diff.sum())} of {diff.numel()} elements differ")
    return bad


def _against_twins(env, row, layer, forms, seed=SEED, label="", training=None, **hyper):
    """[(Y, grads)] of ``layer`` on every form, each held against a fresh twin's single call."""
    outs, bad = [], []
    for A in forms:
        got = _run(env, row, layer, A, seed)
        bad += _differences(env, got, _run(env, row, _twin(env, row, layer, training, **hyper), A, seed), f"{label} {A}")
        outs.append(got)
    assert not bad, "\n".join(bad)
    return outs


def _warm(env, row, layer):
    """Two forwards and one backward on ``adj`` and on ``adj.T``; the first view's output."""
    first = None
    for A in env.forms[row.graph][:2]:
        row.call(layer, A, _X(env, row, A.n), SEED)
        Y, _ = _run(env, row, layer, A)
        first = Y if first is None else first
    return first


def _exact(row, hyper):
    """The row's definition is exact in float32 on the dyadic graph with integer data under these hyper-parameters: a sum rescaled by a
    keep_scale that is no power of two is not."""
    o = dict(row.hyper, **hyper)
    if row.exact and row.cls == "GCNConv":
        return o.get("aggr", "sum") != "sum" or o.get("edge_drop", 0.0) in (0.0, 0.5)
    return row.exact


def _anchor(env, row, layer, seed=SEED, **hyper):
    """The layer's output at the values it holds now against the row's independent definition under ``hyper`` (module docstring)."""
    torch = env.torch
    exact = _exact(row, hyper)
    forms = env.forms["dyadic" if exact else "random"]
    values = _snapshot(layer, row)
    lines = []
    for A in (forms[0], forms[3]):
        X = mc.features(row, A.n, k=1, integer=exact)
        with torch.no_grad():
            got = row.call(layer, A, _dev(env, X), seed)
        assert got.dtype == torch.float32
        got = got.cpu().numpy().astype(np.float64)
        if row.how == "block":
            got = got[mc.batch_flags(A.n)]
        want = mc.reference(row, A, X, values, hyper, seed, oracle=env.O)
        assert got.shape == want.shape and np.abs(want).max() > 0, (row, A)
        if exact:
            wrong = got != want
            if wrong.any():
                lines.append(f"{row} {A}: {int(wrong.sum())} of {wrong.size} elements are not the definition's")
        else:
            low = mc.reference(row, A, X, values, hyper, seed, "float32", oracle=env.O)
            tol = R.tolerances({"Y": torch.from_numpy(want)}, {"Y": torch.from_numpy(low)})["Y"]
            err = float(np.abs(got - want).max()) if np.isfinite(got).all() else float("inf")
            print(f"ratio {row} | {A} | {err / tol:.3f} | tol {tol:.3e}")
            if not err <= tol:
                lines.append(f"{row} {A}: |Y - Y_f64| = {err:.3e} above the tolerance {tol:.3e}")
    assert not lines, "\n".join(lines)


# ---- 1. every write reaches the next forward -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", mc.WRITE_ROUTES, ids=repr)
@pytest.mark.parametrize("row", mc.ROWS, ids=repr)
def test_every_write_reaches_the_next_forward(env, row, route):
    torch = env.torch
    layer = _start(env, row, "old")
    stale = _warm(env, row, layer)
    old, new = _snapshot(layer, row), mc.new_values(row, layer)
    assert route.write(layer, new) is layer
    now = _snapshot(layer, row)
    for name in row.params:
        assert now[name].dtype == np.float32 and not np.array_equal(now[name], old[name]), f"{route} left {name} as it was"
        if route.given:
            assert np.array_equal(now[name], new[name]), name
        if row.quantised:   # values that quantise differently: most of the packed codes must change
            changed = float((mc.codes(now[name], mc.W_BIT) != mc.codes(old[name], mc.W_BIT)).mean())
            assert changed > 0.5, f"{route}: only {changed:.2f} of the codes of {name} changed"
    outs = _against_twins(env, row, layer, env.forms[row.graph], label=f"after {route}:")
    assert not torch.equal(outs[0][0], stale), "the test is blind: the output does not depend on the parameters"
    if route is mc.WRITE_ROUTES[0]:
        _anchor(env, row, layer)


# ---- 2. re-configuration is coherent or refused ----------------------------------------------------------------------------------------

RECONFIGURATIONS = [(row, attr, value) for row in mc.ROWS for attr, values in row.reconfigure.items() for value in values]


@pytest.mark.parametrize("row,attr,value", RECONFIGURATIONS, ids=lambda v: v if isinstance(v, str) else repr(v))
def test_reconfiguration_is_coherent_or_refused(env, row, attr, value):
    """``layer.attr = value`` after the warm-up: the next forward is the fresh twin's built with that value, or the assignment or the
    forward raises. Where the twin itself cannot be built or called (no such layer), the live layer must raise the same error."""
    forms = env.forms[row.graph]
    layer = _start(env, row)
    _warm(env, row, layer)
    assert getattr(layer, attr) != value or type(getattr(layer, attr)) is not type(value)
    refusal = None
    try:
        for A in forms:
            _run(env, row, _twin(env, row, layer, **{attr: value}), A)
    except (ValueError, TypeError, NotImplementedError) as err:
        refusal = err
    if refusal is not None:
        with pytest.raises(type(refusal)):
            setattr(layer, attr, value)
            for A in forms:
                _run(env, row, layer, A)
        return
    try:
        setattr(layer, attr, value)
        for A in forms:
            row.call(layer, A, _X(env, row, A.n), SEED)
    except (ValueError, TypeError, NotImplementedError, AttributeError):
        return   # refused
    assert getattr(layer, attr) == value
    _against_twins(env, row, layer, forms, label=f"{attr} = {value!r}:", **{attr: value})
    twin = _twin(env, row, layer, **{attr: value})
    for name, (kind, _) in row.attributes.items():
        if kind == "derived":     # (tests/test_module_state.py holds that the class assigns every name of the table)
            assert getattr(layer, name, None) == getattr(twin, name, None), f"{name} did not follow {attr}"
    _anchor(env, row, layer, **{attr: value})


# ---- 3. copies and checkpoints ---------------------------------------------------------------------------------------------------------

def _pickled(env, obj):
    buf = io.BytesIO()
    env.torch.save(obj, buf)
    buf.seek(0)
    return env.torch.load(buf, weights_only=False)


def _through_state_dict(env, row, layer):
    fresh = row.make().cuda().train(layer.training)
    fresh.load_state_dict(layer.state_dict())
    return fresh


COPIES = {"deepcopy": lambda env, row, layer: copy.deepcopy(layer), "pickle": lambda env, row, layer: _pickled(env, layer),
          "state_dict": _through_state_dict}


@pytest.mark.parametrize("how", list(COPIES))
@pytest.mark.parametrize("row", mc.ROWS, ids=repr)
def test_a_copy_gives_the_twins_bits(env, row, how):
    layer = _start(env, row)
    _warm(env, row, layer)
    other = COPIES[how](env, row, layer)
    assert other is not layer and other.training and type(other) is type(layer)
    for name, p in _named(other, row).items():
        assert p is not _named(layer, row)[name] and p.data_ptr() != _named(layer, row)[name].data_ptr() and p.requires_grad
    if row.hyper.get("share_weights"):
        assert other.W_r is other.W_l and "W_r" not in dict(other.named_parameters())
    _against_twins(env, row, other, env.forms[row.graph], label=f"{how}:")
    if how == "deepcopy":
        _anchor(env, row, other)


def _cache_tensors(env, layer, row):
    found = []

    def walk(v):
        if isinstance(v, env.torch.Tensor):
            found.append(v)
        elif isinstance(v, (tuple, list)):
            for x in v:
                walk(x)

    for name, (kind, _) in row.attributes.items():
        if kind == "cache":
            walk(getattr(layer, name))
    return found


@pytest.mark.parametrize("how", ["deepcopy", "pickle"])
@pytest.mark.parametrize("row", mc.ROWS, ids=repr)
def test_a_copy_is_independent(env, row, how):
    """Writing the copy's parameters (through ``.data`` and under ``no_grad``) leaves the original's next output unchanged, and the
    reverse; no cache tensor is shared."""
    A = env.forms[row.graph][0]
    layer = _start(env, row)
    _warm(env, row, layer)
    other = COPIES[how](env, row, layer)
    mine = _run(env, row, layer, A)
    by_route = {r.name: r for r in mc.WRITE_ROUTES}
    for k, name in ((2, "data.copy_"), (3, "no_grad")):
        by_route[name].write(other, mc.new_values(row, other, k))
        theirs = _run(env, row, other, A)
        assert not env.torch.equal(theirs[0], mine[0])
        assert not _differences(env, _run(env, row, layer, A), mine, f"the original after {name} on the copy")
    for k, name in ((4, "data.copy_"), (5, "no_grad")):
        by_route[name].write(layer, mc.new_values(row, layer, k))
        assert not env.torch.equal(_run(env, row, layer, A)[0], mine[0])
        assert not _differences(env, _run(env, row, other, A), theirs, f"the copy after {name} on the original")
    ptrs = {t.data_ptr() for t in _cache_tensors(env, layer, row)}
    assert not ptrs & {t.data_ptr() for t in _cache_tensors(env, other, row)}
    if row.cls in ("GCNConv_Qnt",) or row.name == "gcn-None-drop":
        assert ptrs, "the warm layer holds its cache"


def test_gatv2_never_drops_one_of_two_differing_matrices(env):
    torch = env.torch
    shared_row, plain_row = mc.BY_NAME["gatv2-shared"], mc.BY_NAME["gatv2"]
    forms = env.forms["random"][:2]
    shared, plain = _start(env, shared_row), _start(env, plain_row)
    _warm(env, shared_row, shared)
    assert not torch.equal(plain.W_l, plain.W_r)
    before = _snapshot(shared, shared_row)
    with pytest.raises(RuntimeError):
        shared.load_state_dict(plain.state_dict())
    assert shared.W_r is shared.W_l
    # a shared layer's checkpoint into a layer with two matrices: the twin's bits, or an error
    target = _start(env, plain_row, "old")
    try:
        target.load_state_dict(shared.state_dict())
    except RuntimeError:
        pass
    else:
        assert torch.equal(target.W_l, target.W_r)
        _against_twins(env, plain_row, target, forms, label="a shared checkpoint in a plain layer:")
    # assign=True leaves flag and parameters in agreement, on both kinds
    state = {k: v.detach().clone() + 0.125 for k, v in shared.state_dict().items()}
    shared.load_state_dict(state, assign=True)
    assert shared.W_r is shared.W_l and [n for n, _ in shared.named_parameters()] == ["W_l", "att"]
    assert not np.array_equal(_snapshot(shared, shared_row)["W_l"], before["W_l"])
    _against_twins(env, shared_row, shared, forms, label="assign=True on the shared layer:")
    plain.load_state_dict({k: v.detach().clone() + 0.125 for k, v in plain.state_dict().items()}, assign=True)
    assert plain.W_r is not plain.W_l
    _against_twins(env, plain_row, plain, forms, label="assign=True on the plain layer:")
    _anchor(env, shared_row, shared)


def _warm_adjacency(adj):
    from qgtc_ppopp22_amd import tiled

    for view in (adj, adj.T):
        view.degrees(), view.mean_scale(), view.sym_scale(), view.max_block_tiles
        tiled.edge_endpoints(view)


@pytest.mark.parametrize("how", ["deepcopy", "pickle"])
@pytest.mark.parametrize("reorder", [False, True], ids=["plain", "reordered"])
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_an_adjacency_survives_a_copy(env, warm, reorder, how):
    """A TiledAdjacency, cold or with every lazy cache warm: the copy aggregates to the original's bits on both views, is its own pair of
    views and shares no tensor with the original."""
    torch = env.torch
    src, dst, n = mc.GRAPHS["second"]
    adj = env.Q.pack_edges_tiled(_dev(env, src), _dev(env, dst), n, reorder=reorder)
    if warm:
        _warm_adjacency(adj)
    X = _dev(env, np.random.default_rng(5).standard_normal((n, 9)).astype(np.float32))
    for original in (adj, adj.T):
        other = copy.deepcopy(original) if how == "deepcopy" else _pickled(env, original)
        assert other is not original and other.transposed == original.transposed and other.n == n
        assert other.T.T is other and other.T is not original.T and other.T is not original and other.T.transposed != other.transposed
        assert other.tiles.data_ptr() != original.tiles.data_ptr() and other.T.tiles.data_ptr() == other.tiles.data_ptr()
        assert (other.perm is None) == (original.perm is None)
        for a, b in ((other, original), (other.T, original.T)):
            assert torch.equal(env.Q.tiledAggregate(a, a.to_new(X)), env.Q.tiledAggregate(b, b.to_new(X)))
            assert torch.equal(env.Q.tiledAggregate(a, a.to_new(X), a.sym_scale(), a.T.sym_scale()),
                               env.Q.tiledAggregate(b, b.to_new(X), b.sym_scale(), b.T.sym_scale()))
            assert torch.equal(a.mean_scale(), b.mean_scale()) and a.mean_scale().data_ptr() != b.mean_scale().data_ptr()


@pytest.mark.parametrize("how", ["deepcopy", "pickle"])
def test_a_sample_and_a_block_survive_a_copy(env, how):
    """A FanoutSample and a Block travel with their view: the copy aggregates to the original's bits on its own adjacency, and is refused
    on the original's - by tiledAggregate for the sample, by SAGEConv with today's ValueError for the block."""
    from qgtc_ppopp22_amd.fanout import sample_fanout

    torch = env.torch
    row = mc.BY_NAME["sage-block"]
    dup = (lambda o: copy.deepcopy(o)) if how == "deepcopy" else (lambda o: _pickled(env, o))
    for A in (env.forms["random"][1], env.forms["random"][2]):
        X = _X(env, row, A.n)
        sample = sample_fanout(A.adj, 3, SEED)
        other = dup(sample)
        assert other.view is not A.adj and other.view.transposed == A.adj.transposed and (other.k, other.seed) == (3, SEED)
        assert torch.equal(other.thr, sample.thr) and other.thr.data_ptr() != sample.thr.data_ptr()
        assert torch.equal(env.Q.tiledAggregate(other.view, X, fanout=other), env.Q.tiledAggregate(A.adj, X, fanout=sample))
        assert torch.equal(env.Q.tiledAggregate(other.view.T, X, fanout=other), env.Q.tiledAggregate(A.adj.T, X, fanout=sample))
        with pytest.raises(ValueError, match="another adjacency"):
            env.Q.tiledAggregate(A.adj, X, fanout=other)
        block, layer = mc.block_of(A), _start(env, row)
        away = dup(block)
        assert type(away) is type(block) and away.sample.view is not A.adj
        assert torch.equal(away.rows, block.rows) and torch.equal(away.inputs, block.inputs) and torch.equal(away.sample.counts, block.sample.counts)
        assert torch.equal(layer(away.sample.view, X, block=away), layer(A.adj, X, block=block))
        with pytest.raises(ValueError, match="another view"):
            layer(A.adj, X, block=away)


# ---- 4. modes and the generator --------------------------------------------------------------------------------------------------------

def _off(row):
    return {row.sampling: 0.0 if row.sampling == "edge_drop" else None} if row.sampling else {}


@pytest.mark.parametrize("row", mc.ROWS, ids=repr)
def test_eval_is_the_layer_without_sampling_and_draws_nothing(env, row):
    torch = env.torch
    layer = _start(env, row)
    _warm(env, row, layer)
    layer.eval()
    state = torch.get_rng_state()
    for A in env.forms[row.graph]:
        _run(env, row, layer, A, None)
    assert torch.equal(torch.get_rng_state(), state), "eval() drew from torch's generator"
    # (a twin's constructor draws its initial parameters: the generator is compared before any is built)
    _against_twins(env, row, layer, env.forms[row.graph], seed=None, label="eval():", training=True, **_off(row))
    _anchor(env, row, layer, seed=None, **_off(row))


@pytest.mark.parametrize("row", mc.ROWS, ids=repr)
def test_train_with_a_seed_repeats_and_draws_nothing(env, row):
    torch = env.torch
    A = env.forms[row.graph][2]
    layer = _start(env, row)
    state = torch.get_rng_state()
    first = _run(env, row, layer, A, SEED)
    assert not _differences(env, _run(env, row, layer, A, SEED), first, "the same seed again")
    if row.sampling:
        assert not torch.equal(_run(env, row, layer, A, OTHER_SEED)[0], first[0]), "the seed does not reach the sample"
    assert torch.equal(torch.get_rng_state(), state), "a seeded forward drew from torch's generator"


@pytest.mark.parametrize("row", [r for r in mc.ROWS if r.sampling], ids=repr)
def test_train_without_a_seed_draws_two_words_a_forward(env, row):
    """Two forwards differ; torch.manual_seed brings both back; each consumed exactly the two 32-bit draws of conv._draw_edge_seed's
    docstring, high word first - drawn again here from a copy of the generator's state."""
    torch = env.torch
    A = env.forms[row.graph][1]
    layer = _start(env, row)
    torch.manual_seed(20221)
    states = [torch.get_rng_state()]
    outs = []
    for _ in range(2):
        outs.append(_run(env, row, layer, A, None))
        states.append(torch.get_rng_state())
    assert not torch.equal(outs[0][0], outs[1][0])
    torch.manual_seed(20221)
    for k in range(2):
        assert not _differences(env, _run(env, row, layer, A, None), outs[k], f"forward {k} after manual_seed")
    g = torch.Generator()
    for k in range(2):
        g.set_state(states[k])
        hi, lo = torch.randint(0, 1 << 32, (2,), dtype=torch.int64, generator=g).tolist()
        assert torch.equal(g.get_state(), states[k + 1]), "a forward consumes exactly two 32-bit draws"
        assert not _differences(env, _run(env, row, layer, A, (hi << 32) | lo), outs[k], f"forward {k} with the seed drawn here")


@pytest.mark.parametrize("row", mc.ROWS, ids=repr)
def test_nothing_is_drawn_without_sampling(env, row):
    """train() with rate 0, with fanout=None, with block=, and every layer that has no sampling at all."""
    torch = env.torch
    layer = _start(env, row, **_off(row))
    assert layer.training
    state = torch.get_rng_state()
    for A in env.forms[row.graph][:2]:
        _run(env, row, layer, A, None)
    assert torch.equal(torch.get_rng_state(), state)


# ---- 5. one layer, many graphs ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", mc.ROWS, ids=repr)
def test_one_layer_many_graphs(env, row):
    """G1 on adj; G2 with another n; G3 with G1's n and other edges; G1 reordered; G1.T; G1 again: every call is its twin's, the last the
    first's."""
    g1, g2, g3 = env.forms["random"], env.forms["second"], env.forms["dyadic"]
    assert g1[0].n == g3[0].n != g2[0].n
    layer = _start(env, row)
    outs = _against_twins(env, row, layer, [g1[0], g2[0], g3[0], g1[2], g1[1], g1[0]], label="in turn:")
    assert not _differences(env, outs[-1], outs[0], "G1 again")
    assert not env.torch.equal(outs[0][0], outs[2][0]) and not env.torch.equal(outs[0][0], outs[4][0])
    _anchor(env, row, layer)
