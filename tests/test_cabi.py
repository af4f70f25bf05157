"""qgtc_ppopp22_amd.cabi derives every entry's ctypes signature from include/qgtc.h, so the header is the one place a signature is
written. This file is the second statement of the ABI that the hand-written lists of the tests used to be: tests/golden/qgtc_abi.txt
lists every entry at calling-convention level, and the widths whose loss truncates silently are pinned by hand. No GPU."""
import ctypes
import os
import subprocess
import sys

import pytest

from qgtc_ppopp22_amd import cabi
from test_abi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the golden file's word for a ctypes class: the first that is that class. uint32_t is `unsigned` and uint64_t is `size_t` where they are
# one class (LP64): the same register, the same call
WORDS = (("int", ctypes.c_int), ("unsigned", ctypes.c_uint), ("float", ctypes.c_float), ("size_t", ctypes.c_size_t), ("int64", ctypes.c_int64),
         ("uint64", ctypes.c_uint64), ("uint32", ctypes.c_uint32), ("ptr", ctypes.c_void_p), ("str", ctypes.c_char_p))


def _word(cls):
    return next(w for w, c in WORDS if c is cls)


def _lines(sig):
    return [f"{_word(ret)} {name}({', '.join(_word(a) for a in args)})" for name, (ret, args) in sig.items()]


def test_the_derived_signatures_are_the_golden_ones():
    golden = open(os.path.join(ROOT, "tests", "golden", "qgtc_abi.txt")).read().splitlines()
    derived = _lines(cabi.signatures())
    n = next((i for i, (got, want) in enumerate(zip(derived, golden)) if got != want), min(len(derived), len(golden)))
    got, want = (lines[n] if n < len(lines) else "nothing" for lines in (derived, golden))
    assert derived == golden, (f"entry {n} of include/qgtc.h is `{got}`, line {n + 1} of tests/golden/qgtc_abi.txt is `{want}`. A changed line is an "
                               "ABI break: bump QGTC_ABI_VERSION and say so. An added entry adds a line to the golden file and breaks nothing")


def test_every_declared_name_has_a_signature():
    """test_abi_symbols.declared_symbols() finds names with its own regex (comments included): the two cannot drift apart."""
    sig = cabi.signatures()
    assert sorted(sig) == declared_symbols()
    assert list(sig)[:3] == ["qgtc_abi_version", "qgtc_strerror", "qgtc_last_hip_error"]   # header order


def test_load_needs_no_torch_and_is_lazy():
    code = ("import sys\n"
            "from qgtc_ppopp22_amd import cabi\n"
            "assert cabi._lib is None, 'importing cabi opened the library'\n"
            "L = cabi.load()\n"
            "assert L.qgtc_abi_version() == 11 and L.qgtc_strerror(0) == b'ok'\n"
            "assert 'torch' not in sys.modules, 'cabi.load() imported torch'\n"
            "assert 'qgtc_ppopp22_amd.QGTC' not in sys.modules, 'cabi.load() imported the extension'\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-800:]


def test_load_returns_one_handle_with_every_entry_bound():
    L = cabi.load()
    assert cabi.load() is L
    for name, (ret, args) in cabi.signatures().items():
        fn = getattr(L, name)
        assert fn.restype is ret and list(fn.argtypes) == args, name


@pytest.mark.parametrize("text,entry,kind", [
    ("int qgtc_new_entry(const float *x, double scale, void *stream);", "qgtc_new_entry", "double scale"),
    ("int qgtc_new_entry(const float *x, long n);", "qgtc_new_entry", "long n"),
    ("int qgtc_ok(int n);\nint64_t qgtc_new_size(void);", "qgtc_new_size", "int64_t"),
    ("int qgtc_new_entry(int);", "qgtc_new_entry", "int"),          # an unnamed parameter: the type cannot be told from the name
], ids=["double", "long", "return", "unnamed"])
def test_a_type_outside_the_vocabulary_is_an_error(text, entry, kind):
    with pytest.raises(ValueError) as e:
        cabi.signatures("/* a comment with qgtc_in_a_comment(double x); */\n" + text)
    assert entry in str(e.value) and f"'{kind}'" in str(e.value)


def test_the_parser_reads_a_string():
    sig = cabi.signatures("size_t qgtc_a(void);  // qgtc_not_this(int x);\nconst char *qgtc_b(unsigned flags,\n   const qgtc_problem *p, uint32_t t);\n")
    assert sig == {"qgtc_a": (ctypes.c_size_t, []), "qgtc_b": (ctypes.c_char_p, [ctypes.c_uint, ctypes.c_void_p, ctypes.c_uint32])}


def test_the_widths_that_truncate_when_wrong():
    """By hand and independent of the golden file: a c_int in one of these places passes every small test and cuts a large value."""
    sig = cabi.signatures()
    assert sig["qgtc_tiledmm_f32"][1][3] is ctypes.c_int64 and ctypes.sizeof(ctypes.c_int64) == 8                                   # n_tiles
    assert sig["qgtc_tiledmm_f32"][1][6] is ctypes.c_size_t and ctypes.sizeof(ctypes.c_size_t) == ctypes.sizeof(ctypes.c_void_p)    # x_elems
    assert sig["qgtc_tiledmm_f32_drop"][1][13] is ctypes.c_uint64 and ctypes.sizeof(ctypes.c_uint64) == 8                           # seed
    assert sig["qgtc_tiledatt_f32"][1][10] is ctypes.c_float                                                                        # negative_slope
    assert sig["qgtc_rows_words"][0] is ctypes.c_size_t
    assert sig["qgtc_strerror"][0] is ctypes.c_char_p
