"""The autograd contract of every differentiable call of tests/autograd_cases.py, on ``adj`` and ``adj.T``: what the
``torch.autograd.Function`` classes of qgtc_ppopp22_amd/tiled.py promise beyond their kernels' bits.

P1  gradients of any subset of the leaves are the all-leaves run's bits, the other leaves get none; without a leaf to differentiate, and
    under ``no_grad``, the output carries no graph and the same bits.
P2  a strided, a stride-0 and an offset ``dY`` give the bits of a contiguous clone (not run on the rows of
    ``autograd_cases.DY_MEETS_TORCH_FIRST``, where no layout of ``dY`` reaches a Function of the package).
P3  two backward passes over a retained graph give the same bits and ``.grad`` holds exactly twice the first.
P4  the second derivative: the sum rows give d<dX, R>/d(dY) as the forward on R, bit for bit (the layers on them within the dense
    float64 definition's tolerance); every other row raises, naming ``once_differentiable``. Nothing returns another value or "does not
    require grad".
P5  a tensor edited in place between forward and backward either raises autograd's "modified by an inplace operation" or - where the
    backward does not read it - leaves the gradients' bits alone. Gradients of the edited values are the defect.
P6  a context keeps no tensor outside ``save_for_backward`` (the adjacency's own, constant by contract, excepted).
P7  ``torch.utils.checkpoint`` (non-reentrant) gives the direct call's bits, the drawn edge seed of ``GCNConv(edge_drop>0)`` included.

Everything is compared bit for bit (``assert_floats_identical``) except the layers' second derivative."""
import itertools
import zlib

import numpy as np
import pytest

import autograd_cases as ac
import layers_reference as R
from test_tiled_float_gpu import assert_floats_identical

pytestmark = pytest.mark.gpu

PAIRS = [(c, v) for c in ac.DIFFERENTIABLE for v in ac.VIEWS]
IDS = [f"{c.name}-{v}" for c, v in PAIRS]
OTHER_THRESHOLD = 1 << 30          # keeps about three cells in four: neither the sample's thresholds nor "all" nor "none"
_BASELINES = {}


def _np(t):
    return t.detach().cpu().numpy()


def _live(qgtc, case, view):
    import torch

    live = case.build(ac.Env(torch, qgtc, case, view))
    assert tuple(live.leaves) == case.leaves and set(live.sides) == set(case.sides), (case, tuple(live.leaves), tuple(live.sides))
    return live


def _dy(case, view, shape, key="dY"):
    import torch

    rng = np.random.default_rng([zlib.crc32(case.name.encode()), zlib.crc32(key.encode()), ac.VIEWS.index(view)])
    return torch.from_numpy(rng.standard_normal(tuple(shape)).astype(np.float32)).cuda()


def _backward(live, case, view, requires=None, dY=None):
    """(out, {leaf: .grad or None}) of one forward and ``out.backward(dY)`` with the leaves of ``requires`` (all by default)."""
    t = live.tensors(case.leaves if requires is None else requires)
    out = live.run(t)
    out.backward(_dy(case, view, out.shape) if dY is None else dY)
    return out, {k: v.grad for k, v in t.items()}


def _baseline(qgtc, case, view):
    """(output, {leaf: gradient}) as numpy, of the all-leaves run with a contiguous dY: computed once per case and view, never changed."""
    key = (case.name, view)
    if key not in _BASELINES:
        out, grads = _backward(_live(qgtc, case, view), case, view)
        assert all(g is not None for g in grads.values()), (case, grads)
        _BASELINES[key] = (_np(out), {k: _np(g) for k, g in grads.items()})
        for a in (_BASELINES[key][0],) + tuple(_BASELINES[key][1].values()):
            a.setflags(write=False)
            assert np.isfinite(a).all() and a.any(), case
    return _BASELINES[key]


def _assert_grads(got, want, what):
    for name, w in want.items():
        assert got[name] is not None, f"{what}: no gradient for {name}"
        assert_floats_identical(_np(got[name]), w, f"{what}: gradient for {name}")


# ---- P1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,view", PAIRS, ids=IDS)
def test_p1_any_subset_of_the_leaves(qgtc, case, view):
    import torch

    want_out, want = _baseline(qgtc, case, view)
    live = _live(qgtc, case, view)
    for r in range(1, len(case.leaves)):
        for subset in itertools.combinations(case.leaves, r):
            out, grads = _backward(live, case, view, subset)
            assert_floats_identical(_np(out), want_out, f"{case} {view} {subset}: output")
            _assert_grads(grads, {k: want[k] for k in subset}, f"{case} {view} {subset}")
            assert all(grads[k] is None for k in case.leaves if k not in subset), f"{case} {view} {subset}: a gradient nobody asked for"
    out = live.run(live.tensors(()))
    assert out.grad_fn is None and not out.requires_grad, "no leaf requires a gradient: no graph"
    assert_floats_identical(_np(out), want_out, f"{case} {view}: output without a graph")
    with torch.no_grad():
        out = live.run(live.tensors(case.leaves))
    assert out.grad_fn is None and not out.requires_grad, "no_grad: no graph"
    assert_floats_identical(_np(out), want_out, f"{case} {view}: output under no_grad")


# ---- P2 ---------------------------------------------------------------------------------------------------------------------------------
_P2 = [(c, v) for c, v in PAIRS if c.name not in ac.DY_MEETS_TORCH_FIRST]


@pytest.mark.parametrize("case,view", _P2, ids=[f"{c.name}-{v}" for c, v in _P2])
def test_p2_forms_of_dy(qgtc, case, view):
    import torch

    want_out, want = _baseline(qgtc, case, view)
    live = _live(qgtc, case, view)
    dY = _dy(case, view, want_out.shape)
    wide = torch.zeros(tuple(dY.shape[:-1]) + (2 * dY.shape[-1],), device="cuda")
    strided = wide[..., ::2]
    strided.copy_(dY)
    flat = torch.zeros(dY.numel() + 1, device="cuda")
    offset = flat[1:1 + dY.numel()].view(dY.shape)
    offset.copy_(dY)
    assert not strided.is_contiguous() and offset.is_contiguous() and offset.storage_offset() == 1
    for what, form in (("every second column of a wider buffer", strided), ("a 4-byte storage offset", offset)):
        _, grads = _backward(live, case, view, dY=form)
        _assert_grads(grads, want, f"{case} {view} dY = {what}")
    # stride 0: the gradient of out.sum() is an expanded scalar
    _, ones = _backward(live, case, view, dY=torch.ones(dY.shape, device="cuda"))
    t = live.tensors(case.leaves)
    live.run(t).sum().backward()
    _assert_grads({k: v.grad for k, v in t.items()}, {k: _np(g) for k, g in ones.items()}, f"{case} {view} dY = an expanded one")


# ---- P3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,view", PAIRS, ids=IDS)
def test_p3_backward_twice(qgtc, case, view):
    import torch

    want_out, want = _baseline(qgtc, case, view)
    live = _live(qgtc, case, view)
    dY = _dy(case, view, want_out.shape)
    t = live.tensors(case.leaves)
    out = live.run(t)
    leaves = [t[k] for k in case.leaves]
    for time in ("first", "second"):
        grads = torch.autograd.grad(out, leaves, dY, retain_graph=True)
        _assert_grads(dict(zip(case.leaves, grads)), want, f"{case} {view} the {time} pass")
    out.backward(dY, retain_graph=True)
    out.backward(dY, retain_graph=True)
    for name in case.leaves:     # x + x is exact in float32
        assert_floats_identical(_np(t[name].grad), want[name] + want[name], f"{case} {view}: .grad of {name} after two passes")


# ---- P4 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,view", PAIRS, ids=IDS)
def test_p4_second_derivative(qgtc, case, view):
    import torch

    want_out, _ = _baseline(qgtc, case, view)
    live = _live(qgtc, case, view)
    t = live.tensors(case.leaves)
    X = t[case.leaves[0]]
    Rm = _dy(case, view, X.shape, "R")
    U = _dy(case, view, want_out.shape).requires_grad_(True)
    out = live.run(t)
    try:
        g, = torch.autograd.grad(out, X, U, create_graph=True)
        # .backward(), not autograd.grad(..., U): once_differentiable hangs its error node on detached copies, so a pass pruned to the
        # paths that reach U would never run it and torch would only report U as unused
        (g * Rm).sum().backward()
        v = U.grad
    except RuntimeError as e:
        assert "once_differentiable" in str(e), f"{case} {view}: differentiating the backward neither works nor says why: {e}"
        assert case.second == "raises", f"{case} {view}: the call is linear in X and must be twice differentiable, but: {e}"
        return
    assert case.second != "raises", f"{case} {view}: a once_differentiable backward returned a second derivative"
    assert v is not None and v.shape == U.shape, f"{case} {view}: the second pass never reached dY"
    if case.second == "value":
        assert_floats_identical(_np(v), _np(live.second(Rm)), f"{case} {view}: d<dX, R>/d(dY) is tiledMMFloat on R")
        return
    want, want32 = live.dense(Rm, torch.float64), live.dense(Rm, torch.float32)
    tol = R.tolerances({"v": want}, {"v": want32})["v"]
    err = float((v.detach().cpu().to(torch.float64) - want).abs().max())
    print(f"ratio {case.name} | {view} | d<dX, R>/d(dY) | {err / tol:.3f} | tol {tol:.3e}")
    assert tol > 0 and float(want.abs().max()) > 0 and err <= tol, (case, view, err, tol)


# ---- the graph of a call -----------------------------------------------------------------------------------------------------------------
def _nodes(out):
    """The nodes of this package's Functions in the graph of ``out``, in a fixed order."""
    import torch

    seen, stack, found = set(), [out.grad_fn], []
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if isinstance(fn, torch.autograd.function.BackwardCFunction):
            found.append(fn)
        stack.extend(f for f, _ in fn.next_functions)
    return found


def _attribute_tensors(node):
    """(path, tensor) of every tensor among the plain attributes of a context: through tuples, lists and dicts, and one level into a
    FanoutSample. An adjacency is not entered."""
    import torch

    from qgtc_ppopp22_amd.fanout import FanoutSample

    def walk(path, v):
        if isinstance(v, torch.Tensor):
            yield path, v
        elif isinstance(v, (tuple, list)):
            for i, x in enumerate(v):
                yield from walk(f"{path}[{i}]", x)
        elif isinstance(v, dict):
            for k, x in v.items():
                yield from walk(f"{path}[{k!r}]", x)
        elif isinstance(v, FanoutSample):
            for k, x in vars(v).items():
                if isinstance(x, torch.Tensor):
                    yield f"{path}.{k}", x

    for name, value in sorted(vars(node).items()):
        yield from walk(name, value)


def _adjacency_pointers(adj):
    """data_ptr of every tensor the adjacency and its other view own, caches included."""
    import torch

    ptrs = set()

    def add(v):
        if isinstance(v, torch.Tensor):
            ptrs.add(v.data_ptr())
        elif isinstance(v, (tuple, list)):
            for x in v:
                add(x)

    for a in (adj, adj.T):
        for v in vars(a).values():
            add(v)
    return ptrs


def _saved(node):
    return [s for s in node.saved_tensors if s is not None]


# ---- P6 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,view", PAIRS, ids=IDS)
def test_p6_nothing_unversioned_on_the_context(qgtc, case, view):
    import torch

    live = _live(qgtc, case, view)
    out = live.run(live.tensors(case.leaves))
    nodes = _nodes(out)
    assert {type(n).__name__[:-len("Backward")] for n in nodes} == set(case.functions), (case, [type(n).__name__ for n in nodes])
    constant = _adjacency_pointers(ac.Env(torch, qgtc, case, view).adj)
    loose = []
    for node in nodes:
        saved = {s.data_ptr() for s in _saved(node)}
        loose += [f"{type(node).__name__}.{path}" for path, t in _attribute_tensors(node)
                  if t.data_ptr() not in saved and t.data_ptr() not in constant]
    assert not loose, f"{case} {view}: tensors kept on the context outside save_for_backward, where no version check sees an edit: {loose}"


# ---- P5 ---------------------------------------------------------------------------------------------------------------------------------
def _edit(label, t):
    """The in-place edit of the design: floats doubled, bitmaps and counts cleared, thresholds set to another one."""
    import torch

    with torch.no_grad():
        if t.is_floating_point():
            t.mul_(2)
        elif label.endswith("thr"):
            t.fill_(OTHER_THRESHOLD)
        else:
            t.zero_()


def _targets(live, case, t, out, constant):
    """{label: tensor}: the leaves, the side tensors, the output where a Function saved it, and whatever else the contexts of the graph
    hold or saved (``arg`` of max / min, the softmax statistics, intermediates of a layer) - the adjacency's own excepted."""
    targets = {f"leaf {k}": t[k] for k in case.leaves}
    targets.update({f"side {k}": v for k, v in live.sides.items()})
    known = {v.data_ptr() for v in targets.values()} | constant
    for i, node in enumerate(_nodes(out)):
        found = [(f"saved[{j}]", s) for j, s in enumerate(node.saved_tensors) if s is not None] + list(_attribute_tensors(node))
        for path, s in found:
            if s.data_ptr() == out.data_ptr():
                targets["output"] = out
            elif s.data_ptr() not in known:
                known.add(s.data_ptr())
                targets[f"{i}:{type(node).__name__}.{path}"] = s
    return targets


@pytest.mark.parametrize("case,view", PAIRS, ids=IDS)
def test_p5_in_place_edits_between_forward_and_backward(qgtc, case, view):
    import torch

    want_out, want = _baseline(qgtc, case, view)
    dY = _dy(case, view, want_out.shape)
    constant = _adjacency_pointers(ac.Env(torch, qgtc, case, view).adj)
    # not vacuous: the call does depend on every side tensor's contents
    for name in case.sides:
        live = _live(qgtc, case, view)
        _edit(name, live.sides[name])
        _, grads = _backward(live, case, view)
        assert any((_np(grads[k]).view(np.uint32) != want[k].view(np.uint32)).any() for k in case.leaves), \
            f"{case} {view}: editing {name} before the forward changes no gradient"
    live = _live(qgtc, case, view)
    t = live.tensors(case.leaves)
    labels = list(_targets(live, case, t, live.run(t), constant))
    raised, unread, bad = [], [], []
    for label in labels:
        live = _live(qgtc, case, view)           # a fresh case: an edit does not outlive its turn
        t = live.tensors(case.leaves)
        out = live.run(t)
        _edit(label, _targets(live, case, t, out, constant)[label])
        try:
            grads = torch.autograd.grad(out, [t[k] for k in case.leaves], dY)
        except RuntimeError as e:
            assert "modified by an inplace operation" in str(e), f"{case} {view} after editing {label}: {e}"
            raised.append(label)
            continue
        differs = [k for k, g in zip(case.leaves, grads) if (_np(g).view(np.uint32) != want[k].view(np.uint32)).any()]
        if differs:
            bad.append(f"{label} (gradients of {differs})")
        else:
            unread.append(label)
    print(f"edits {case.name} | {view} | raised: {raised} | not read by the backward: {unread}")
    assert not bad, f"{case} {view}: an in-place edit after the forward silently changed the gradients: {bad}"
    assert all(f"side {k}" in raised + unread for k in case.sides)


# ---- P7 ---------------------------------------------------------------------------------------------------------------------------------
def _checkpointed(live, case, view, run, dY):
    from torch.utils.checkpoint import checkpoint

    t = live.tensors(case.leaves)
    out = checkpoint(lambda *ts: run(dict(zip(case.leaves, ts))), *[t[k] for k in case.leaves], use_reentrant=False)
    out.backward(dY)
    return out, {k: v.grad for k, v in t.items()}


@pytest.mark.parametrize("case,view", PAIRS, ids=IDS)
def test_p7_checkpointing(qgtc, case, view):
    want_out, want = _baseline(qgtc, case, view)
    live = _live(qgtc, case, view)
    out, grads = _checkpointed(live, case, view, live.run, _dy(case, view, want_out.shape))
    assert_floats_identical(_np(out), want_out, f"{case} {view}: the checkpointed output")
    _assert_grads(grads, want, f"{case} {view} checkpointed")


@pytest.mark.parametrize("view", ac.VIEWS)
def test_p7_checkpointing_replays_the_drawn_edge_seed(qgtc, view):
    """GCNConv(edge_drop>0).train() with edge_seed=None draws its seed from torch's CPU generator: the recompute must draw it again."""
    import torch

    case = next(c for c in ac.CASES if c.name == "layer-gcn-sym-edge_drop")
    live = _live(qgtc, case, view)
    dY = _dy(case, view, _baseline(qgtc, case, view)[0].shape)

    def direct(seed):
        torch.manual_seed(seed)
        t = live.tensors(case.leaves)
        out = live.drawn(t)
        out.backward(dY)
        return _np(out), {k: _np(v.grad) for k, v in t.items()}

    want_out, want = direct(77)
    other_out, _ = direct(78)
    assert (want_out.view(np.uint32) != other_out.view(np.uint32)).any(), "the drawn seed decides the subgraph"
    torch.manual_seed(77)
    out, grads = _checkpointed(live, case, view, live.drawn, dY)
    assert_floats_identical(_np(out), want_out, f"{view}: the checkpointed output")
    _assert_grads(grads, want, f"{view} checkpointed, seed drawn")


# ---- the inference-only row -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", ac.VIEWS)
def test_the_quantised_layer_is_inference_only(qgtc, view):
    """Aggregation_Qnt: its inputs are packed words, so no graph reaches it, and its backward raises when called."""
    import torch

    from qgtc_ppopp22_amd.conv import Aggregation_Qnt

    case = next(c for c in ac.CASES if c.second == "inference")
    live = _live(qgtc, case, view)
    out = live.run(live.tensors(case.leaves))
    assert out.grad_fn is None and not out.requires_grad and bool(torch.isfinite(out).all())
    with pytest.raises(RuntimeError, match="does not require grad"):
        out.sum().backward()
    with pytest.raises(NotImplementedError, match="inference-only"):
        Aggregation_Qnt.backward(None, out)
