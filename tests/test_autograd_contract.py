"""The table of tests/autograd_cases.py is complete: every ``torch.autograd.Function`` of qgtc_ppopp22_amd is crossed by a case, no case
names a class that is gone, and every parameter of ``tiledAggregate`` that can hold a tensor is a leaf or a side tensor of some case. A
new Function or a new keyword without a case fails here. The package is read with ``ast``: nothing is imported that needs the device."""
import ast
import glob
import os

import autograd_cases as ac

PACKAGE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qgtc_ppopp22_amd")


def _trees():
    for path in sorted(glob.glob(os.path.join(PACKAGE, "*.py"))):
        with open(path) as f:
            yield os.path.basename(path), ast.parse(f.read())


def function_classes(trees=None):
    """{class name: file} of every class whose bases name ``torch.autograd.Function`` (or ``autograd.Function`` / ``Function``)."""
    found = {}
    for name, tree in trees if trees is not None else _trees():
        for node in ast.walk(tree):
            if isinstance(node, ast.ClassDef) and any(ast.unparse(b).split(".")[-2:] in (["autograd", "Function"], ["Function"])
                                                      for b in node.bases):
                found[node.name] = name
    return found


def aggregate_parameters():
    """The parameter names of ``tiled.tiledAggregate``."""
    tree = dict(_trees())["tiled.py"]
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "tiledAggregate")
    return [a.arg for a in fn.args.posonlyargs + fn.args.args + fn.args.kwonlyargs]


def _uncovered_functions(cases, classes):
    named = {f for c in cases for f in c.functions}
    return sorted(set(classes) - named), sorted(named - set(classes))


def _uncovered_keywords(cases, parameters):
    held = set().union(*(c.keywords for c in cases))
    return sorted(p for p in parameters if p not in ac.NOT_TENSORS and p not in held)


def test_the_package_has_the_functions_the_table_was_written_for():
    classes = function_classes()
    assert classes == {"_TiledAggregate": "tiled.py", "_TiledWeighted": "tiled.py", "_TiledExtremum": "tiled.py",
                       "_TiledAttention": "tiled.py", "_TiledEdgeSoftmax": "tiled.py", "_TiledEdgeScores": "tiled.py",
                       "_TiledEdgeAdditiveScores": "tiled.py", "Aggregation_Qnt": "conv.py"}, classes


def test_every_function_has_a_case_and_every_case_a_function():
    missing, stale = _uncovered_functions(ac.CASES, function_classes())
    assert not missing, f"no case of tests/autograd_cases.py crosses {missing}"
    assert not stale, f"tests/autograd_cases.py names classes that do not exist: {stale}"


def test_every_tensor_keyword_of_tiledaggregate_has_a_case():
    parameters = aggregate_parameters()
    assert parameters[:2] == ["adj", "X"] and set(ac.NOT_TENSORS) <= set(parameters), parameters
    missing = _uncovered_keywords(ac.CASES, parameters)
    assert not missing, f"no case of tests/autograd_cases.py passes a tensor in {missing} (or name them in NOT_TENSORS, with the reason)"


def test_the_checks_notice_a_removed_case_a_new_function_and_a_new_keyword():
    """The three checks above on a table with a case taken out, on a package with one more Function, on a signature with one more keyword."""
    classes, parameters = function_classes(), aggregate_parameters()
    without = [c for c in ac.CASES if "_TiledExtremum" not in c.functions]
    assert _uncovered_functions(without, classes) == (["_TiledExtremum"], [])
    gone = {k: v for k, v in classes.items() if k != "_TiledExtremum"}
    assert _uncovered_functions(ac.CASES, gone) == ([], ["_TiledExtremum"])
    extra = ast.parse("import torch\nclass _New(torch.autograd.Function):\n    pass\nclass _Not(torch.nn.Module):\n    pass\n")
    assert _uncovered_functions(ac.CASES, function_classes([("new.py", extra)])) == (["_New"], sorted({f for c in ac.CASES for f in c.functions}))
    assert _uncovered_keywords(ac.CASES, parameters + ["edge_bias"]) == ["edge_bias"]
    assert _uncovered_keywords([c for c in ac.CASES if "src_scale" not in c.keywords], parameters) == ["src_scale"]


def test_the_table_is_well_formed():
    names = [c.name for c in ac.CASES]
    assert len(names) == len(set(names))
    for c in ac.CASES:
        assert c.second in ac.SECONDS and c.spec and callable(c.build) and not set(c.leaves) & set(c.sides), c
        assert (c.second == "value") == (c.functions == ("_TiledAggregate",) and not c.name.startswith("layer-")), c
    assert [c.name for c in ac.CASES if c.second == "inference"] == ["layer-gcn-qnt"]
    # the rows the design lists
    for prefix, count in (("sum-", 8), ("max-", 4), ("min-", 4), ("attn-", 7), ("edge_weight", 3), ("edge_", 10), ("layer-", 7)):
        assert sum(n.startswith(prefix) for n in names) == count, prefix
