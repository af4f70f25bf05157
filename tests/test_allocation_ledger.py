"""tests/allocation_ledger.py names, for every uninitialised allocation of the binding and the Python layer, who defines its elements.
No GPU: the sites are found in the sources by regular expression and held against the ledger, both ways."""
import re

import allocation_ledger as L


def test_every_site_has_its_row_and_every_row_its_site():
    missing, stale, malformed = L.check()
    assert not missing, f"allocation sites without a verdict per site in tests/allocation_ledger.py (read who writes them): {missing}"
    assert not stale, f"rows of tests/allocation_ledger.py whose site is gone: {stale}"
    assert not malformed, f"verdicts that are none of {L.VERDICTS}: {malformed}"
    assert set(L.NEVER_READ) <= set(L.LEDGER)


def test_the_search_finds_what_a_plain_count_finds():
    """The routing of sites to (function, tensor) loses none: per file, as many sites as the pattern has matches outside comments and
    strings; no site fell outside a function or an assignment."""
    counts = {}
    for name, path in L.FILES.items():
        cpp = path.suffix == ".cpp"
        text = "\n".join((L._strip_cpp if cpp else L._strip_py)(ln) for ln in path.read_text().split("\n"))
        counts[name] = len((L._CPP_SITE if cpp else L._PY_SITE).findall(text))
        assert counts[name] == sum(L.find_sites(name).values()), name
    assert counts["qgtc_torch.cpp"] >= 60 and counts["tiled.py"] >= 20 and counts["dist.py"] == 4
    assert counts["sampler.py"] == 0 and counts["driver.py"] == 0, "a new site in sampler.py / driver.py needs its row"
    for file, fn, tensor in L.all_sites():
        assert not fn.startswith("<") and not tensor.startswith("<"), (file, fn, tensor)
    # the scopes are real: every function or struct named exists in its file under that name
    for file, fn, _ in L.LEDGER:
        src = L.FILES[file].read_text()
        assert re.search(rf"\b(?:def|struct)\s+{fn}\b|\b{fn}\s*\(", src), (file, fn)


def test_a_zero_filled_allocation_needs_the_header_behind_it():
    """The contract of the binding's header: outputs come from torch::empty and the entries write every word. A torch::zeros in the
    binding hides a skipped write from the dirty-memory tests, so each one must be listed in ZERO_FILLED with the sentence of
    include/qgtc.h that makes the caller responsible for clearing that argument - and that sentence must stand in the header."""
    raw = L.FILES["qgtc_torch.cpp"].read_text().split("\n")
    lines = [L._strip_cpp(ln) for ln in raw]
    found = set()
    for i, line in enumerate(lines):
        for m in re.finditer(r"torch::zeros(?:_like)?\s*\(", line):
            found.add((L._cpp_function(raw, i), L._tensor(line[: m.start()], m.start())))
    assert found == set(L.ZERO_FILLED), f"zero-filled allocations of the binding against tests/allocation_ledger.py's ZERO_FILLED: {found}"
    header = " ".join((L.ROOT / "include" / "qgtc.h").read_text().split())
    for key, sentence in L.ZERO_FILLED.items():
        assert " ".join(sentence.split()) in header, f"{key}: include/qgtc.h does not say the caller clears it"


def test_the_extractor_on_a_small_sample(tmp_path):
    sample = tmp_path / "sample.cpp"
    sample.write_text('// torch::empty (a comment)\nstruct Plan {\n    void bind() {\n        pool = torch::empty({4}, opts);\n    }\n};\n'
                      'torch::Tensor f(int n,\n                int m) {\n    torch::Tensor out = n\n        ? torch::empty({n}, o)\n'
                      '        : torch::empty({m}, o);\n    auto a = torch::empty({n}, o), b = torch::empty_like(a);\n'
                      '    m.def("x", "uses torch::empty(");\n    return out;\n}\n')
    L.FILES["sample.cpp"] = sample
    try:
        got = dict(L.find_sites("sample.cpp"))
    finally:
        del L.FILES["sample.cpp"]
    assert got == {("sample.cpp", "Plan", "pool"): 1, ("sample.cpp", "f", "out"): 2, ("sample.cpp", "f", "a"): 1, ("sample.cpp", "f", "b"): 1}
