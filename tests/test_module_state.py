"""The table of tests/module_state_cases.py is complete, and the torch facts its design rests on hold. No GPU; the package is read with
``ast``, as tests/test_autograd_contract.py reads it.

Completeness: every class of qgtc_ppopp22_amd/conv.py and sage.py whose bases name ``Module`` has a row; every ``self.<name> = ...`` of
the class (in ``__init__`` or any other method) and every property that is not a Parameter or a sub-module is classified in the row's
``attributes``; every parameter is in some row's ``params``. A new cache or hyper-parameter without a classification fails here.

The torch facts: for each WRITE_ROUTE, on a plain ``torch.nn.Linear`` on the CPU, whether ``weight._version`` changes and whether the
Parameter object is replaced. Five routes change neither - which is why GCNConv_Qnt cannot key its packed weights on ``_version`` and
packs them in every forward; a torch upgrade that changes a flag is noticed here.

Shared parameters: one Parameter registered under two names takes the LAST of two differing tensors of a state dict and raises nothing.
That is torch's behaviour on a stand-in module; conv.GATv2Conv(share_weights=True) therefore registers its matrix once."""
import ast
import os

import numpy as np
import pytest
import torch

import module_state_cases as mc

PACKAGE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qgtc_ppopp22_amd")


def _tree(stem):
    with open(os.path.join(PACKAGE, stem + ".py")) as f:
        return ast.parse(f.read())


def _self_names(target):
    """The names n of ``self.n`` among an assignment's targets (tuples unpacked)."""
    if isinstance(target, (ast.Tuple, ast.List)):
        return [n for t in target.elts for n in _self_names(t)]
    if isinstance(target, ast.Attribute) and isinstance(target.value, ast.Name) and target.value.id == "self":
        return [target.attr]
    return []


def _mentions(node, word):
    return any((isinstance(n, ast.Attribute) and n.attr == word) or (isinstance(n, ast.Name) and n.id == word) for n in ast.walk(node))


def _is_module_call(value):
    """``torch.nn.<Class>(...)`` other than Parameter: a sub-module."""
    return (isinstance(value, ast.Call) and ast.unparse(value.func).startswith("torch.nn.") and not ast.unparse(value.func).endswith("Parameter"))


def module_classes(trees=None):
    """{class: {"file", "params", "modules", "attributes"}} of every class whose bases name ``Module``: the names assigned on ``self``
    anywhere in the class, split into Parameters (the value mentions ``Parameter``; ``setattr(self, name, Parameter)`` in a loop over a
    literal tuple counts), sub-modules (a ``torch.nn`` constructor) and the rest, to which the class's properties are added."""
    found = {}
    for stem, tree in trees if trees is not None else [(s, _tree(s)) for s in ("conv", "sage")]:
        for cls in ast.walk(tree):
            if not (isinstance(cls, ast.ClassDef) and any(ast.unparse(b).split(".")[-1] == "Module" for b in cls.bases)):
                continue
            params, modules, rest = set(), set(), set()
            for node in ast.walk(cls):
                if isinstance(node, ast.Assign):
                    names = [n for t in node.targets for n in _self_names(t)]
                    if _mentions(node.value, "Parameter"):
                        params.update(names)
                    elif _is_module_call(node.value):
                        modules.update(names)
                    else:
                        rest.update(names)
                elif isinstance(node, (ast.AugAssign, ast.AnnAssign)):
                    rest.update(_self_names(node.target))
                elif isinstance(node, ast.For) and isinstance(node.iter, (ast.Tuple, ast.List)) and isinstance(node.target, ast.Name):
                    for call in ast.walk(node):
                        if (isinstance(call, ast.Call) and ast.unparse(call.func) == "setattr" and len(call.args) == 3
                                and ast.unparse(call.args[0]) == "self" and ast.unparse(call.args[1]) == node.target.id):
                            names = [ast.literal_eval(e) for e in node.iter.elts]
                            (params if _mentions(call.args[2], "Parameter") else rest).update(names)
                elif isinstance(node, ast.FunctionDef) and any(ast.unparse(d).split(".")[0] == "property" or ast.unparse(d).endswith(".setter")
                                                               for d in node.decorator_list):
                    rest.add(node.name)
            found[cls.name] = {"file": stem, "params": params, "modules": modules, "attributes": rest - params - modules}
    return found


def _problems(classes, rows, attributes):
    """What the table lacks, and what it names that the package no longer has."""
    out = []
    for name, c in classes.items():
        mine = [r for r in rows if r.cls == name]
        if not mine:
            out.append(f"{name}: no row")
            continue
        table = attributes.get(name, {})
        out += [f"{name}.{a}: not classified" for a in sorted(c["attributes"] - set(table))]
        out += [f"{name}.{a}: classified, but the class no longer assigns it" for a in sorted(set(table) - c["attributes"])]
        listed = set().union(*(r.params for r in mine))
        out += [f"{name}.{p}: a parameter in no row's params" for p in sorted(c["params"] - listed)]
        out += [f"{name}.{p}: in params, but no parameter or sub-module of the class" for p in sorted(listed)
                if p.split(".")[0] not in c["params"] | c["modules"]]
        out += [f"{name}.{m}: a sub-module without a parameter in params" for m in sorted(c["modules"])
                if not any(p.startswith(m + ".") for p in listed)]
    out += [f"{r.name}: names the class {r.cls}, which does not exist" for r in rows if r.cls not in classes]
    return out


def test_the_package_has_the_modules_the_table_was_written_for():
    classes = module_classes()
    assert {k: v["file"] for k, v in classes.items()} == mc.FILES, classes


def test_every_module_parameter_and_attribute_has_its_row():
    problems = _problems(module_classes(), mc.ROWS, mc.ATTRIBUTES)
    assert not problems, "\n".join(problems)


def test_the_check_notices_a_new_module_a_new_cache_and_a_new_parameter():
    classes = module_classes()
    extra = ast.parse("import torch\nclass New(torch.nn.Module):\n    def __init__(self):\n        self.w = torch.nn.Parameter(torch.zeros(1))\n"
                      "class Not(torch.autograd.Function):\n    pass\n")
    assert _problems(dict(classes, **module_classes([("new", extra)])), mc.ROWS, mc.ATTRIBUTES) == ["New: no row"]
    grown = ast.parse("import torch\nclass SAGEConv(torch.nn.Module):\n    def __init__(self):\n        self.aggr, self.fanout = 1, 2\n"
                      "        self.lin_self = torch.nn.Linear(1, 1)\n        self.lin_nbr = torch.nn.Linear(1, 1)\n"
                      "        self.scale = torch.nn.Parameter(torch.zeros(1))\n"
                      "    def forward(self, x):\n        self._last_n = x.size(0)\n"
                      "    @property\n    def rate(self):\n        return 1\n")
    got = _problems(dict(classes, **module_classes([("sage", grown)])), mc.ROWS, mc.ATTRIBUTES)
    assert got == ["SAGEConv._last_n: not classified", "SAGEConv.rate: not classified", "SAGEConv.scale: a parameter in no row's params"], got
    without = {k: {a: v for a, v in t.items() if a != "_keep_vector"} for k, t in mc.ATTRIBUTES.items()}
    assert _problems(classes, mc.ROWS, without) == ["GCNConv._keep_vector: not classified"]
    assert _problems(classes, [r for r in mc.ROWS if r.cls != "TransformerConv"], mc.ATTRIBUTES) == ["TransformerConv: no row"]
    stale = dict(mc.ATTRIBUTES, GATConv=dict(mc.ATTRIBUTES["GATConv"], _packed=("cache", "x")))
    assert _problems(classes, mc.ROWS, stale) == ["GATConv._packed: classified, but the class no longer assigns it"]


def test_the_table_is_well_formed():
    for cls, table in mc.ATTRIBUTES.items():
        for name, (kind, note) in table.items():
            assert kind in mc.KINDS, (cls, name)
            assert kind not in ("cache", "derived") or note, f"{cls}.{name}: a {kind} attribute names its key or its source"
    names = [r.name for r in mc.ROWS]
    # the rows the issue lists
    for prefix, count in (("qnt-", 4), ("gcn-", 3), ("gat", 4), ("gat-drop", 1), ("gatv2", 2), ("transformer", 1), ("sage-", 2)):
        assert sum(n.startswith(prefix) for n in names) == count, prefix
    for r in mc.ROWS:
        hyper = {a for a, (kind, _) in r.attributes.items() if kind == "hyper"}
        assert set(r.reconfigure) == hyper, f"{r.name}: property 2 needs a value for every hyper attribute, and for those only"
        assert r.reference and set(r.hyper) <= set(r.attributes), r.name
        if r.cls == "GCNConv":
            assert r.hyper["edge_drop"] == 0.25
    assert len(mc.WRITE_ROUTES) == 10 and len(mc.UNSEEN) == 5


def test_values_of_the_quantised_rows_change_their_codes():
    """The old values change 60 % of their codes under float16 (the ties), and every element of the new values has another code."""
    row = mc.BY_NAME["qnt-dense"]
    layer = row.make()
    old, new = mc.old_values(row, layer), mc.new_values(row, layer)
    for name in row.params:
        before = mc.codes(old[name], mc.W_BIT)
        halved = mc.codes(old[name].astype(np.float16).astype(np.float32), mc.W_BIT)
        assert (before != halved).mean() > 0.5, name
        assert (mc.codes(new[name], mc.W_BIT) != before).all(), name


@pytest.mark.parametrize("route", mc.WRITE_ROUTES, ids=repr)
def test_what_torchs_version_counter_sees(route):
    """On a plain Linear: does the route change ``weight._version``, does it replace the Parameter - as the table says."""
    lin = torch.nn.Linear(3, 2)
    for name in ("weight", "bias"):     # Linear initialises in place; the layers here hold Parameter(torch.randn(..)), at version 0
        setattr(lin, name, torch.nn.Parameter(getattr(lin, name).detach().clone()))
    assert lin.weight._version == 0
    new = {"weight": np.full((2, 3), 0.3, dtype=np.float32), "bias": np.full((2,), 1.3, dtype=np.float32)}
    before = lin.weight
    version, values = before._version, before.detach().clone()
    assert route.write(lin, new) is lin
    after = lin.weight
    assert not torch.equal(after.detach(), values), "the route must change the values"
    assert (after is not before) == route.replaces, f"{route}: replaces the Parameter: {after is not before}"
    assert (after._version != version) == route.bumps, f"{route}: _version {version} -> {after._version}"
    assert after.requires_grad and after.dtype == torch.float32
    if route.given:
        assert torch.equal(after.detach(), torch.from_numpy(new["weight"]))


def test_the_routes_the_version_counter_misses():
    assert mc.UNSEEN == ["load_state_dict-assign", "data.copy_", "data=", "vector_to_parameters", "half-float"]


class _TwoNames(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Parameter(torch.zeros(2))
        self.b = self.a


def test_one_parameter_under_two_names_keeps_the_last_tensor_loaded():
    m = _TwoNames()
    assert sorted(m.state_dict()) == ["a", "b"] and len(list(m.parameters())) == 1
    m.load_state_dict({"a": torch.tensor([1.0, 1.0]), "b": torch.tensor([2.0, 2.0])})       # raises nothing
    assert m.a is m.b and m.a.tolist() == [2.0, 2.0]
    m.load_state_dict({"a": torch.tensor([1.0, 1.0]), "b": torch.tensor([2.0, 2.0])}, assign=True)
    assert m.a is not m.b, "assign=True un-shares the two names"


def test_gatv2_registers_a_shared_matrix_once():
    """What property 3c rests on, without a device: the shared layer has no second key, its W_r is its W_l however W_l is replaced, and a
    state dict whose W_l and W_r differ is refused; one whose W_r equals W_l (a checkpoint of a shared layer from before) still loads."""
    from qgtc_ppopp22_amd.conv import GATv2Conv

    shared, plain = GATv2Conv(4, 3, heads=2, share_weights=True), GATv2Conv(4, 3, heads=2)
    assert sorted(shared.state_dict()) == ["W_l", "att"] and sorted(plain.state_dict()) == ["W_l", "W_r", "att"]
    assert shared.W_r is shared.W_l and plain.W_r is not plain.W_l
    with pytest.raises(RuntimeError, match="W_r"):
        shared.load_state_dict(plain.state_dict())
    with pytest.raises(RuntimeError, match="W_r"):
        plain.load_state_dict(shared.state_dict())
    old = dict(plain.state_dict(), W_r=plain.W_l.detach().clone())
    shared.load_state_dict(old)
    assert torch.equal(shared.W_l, plain.W_l) and shared.W_r is shared.W_l
    shared.load_state_dict({k: v.clone() for k, v in shared.state_dict().items()}, assign=True)
    assert shared.W_r is shared.W_l and sorted(n for n, _ in shared.named_parameters()) == ["W_l", "att"]
