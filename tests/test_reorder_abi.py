"""C-ABI of the node reordering (include/qgtc.h, qgtc_reorder_*): exported, and bad arguments are refused before any device work (no
GPU needed); and the rule itself, in its NumPy model (tests/reorder_model.py), brings a shuffled graph's tile count back to about
what block-local ids give. The signatures come from the header (cabi.load())."""
import ctypes

import numpy as np
import pytest

from reorder_model import mix32, reorder_model, shuffled_sbm, tile_count

EINVAL = 1


@pytest.fixture(scope="module")
def lib():
    from qgtc_ppopp22_amd import cabi

    return cabi.load()


def _buf(words):
    b = (ctypes.c_uint32 * (words + 64))()
    addr = ctypes.addressof(b)
    return b, (addr + 255) & ~255   # keep the buffer alive; 256-byte aligned address inside it


def test_entries_are_exported(lib):
    for name in ("qgtc_reorder_work_words", "qgtc_reorder_nodes"):
        assert hasattr(lib, name)


def test_reorder_refuses_bad_arguments(lib):
    keep, p = _buf(4096)
    call = lib.qgtc_reorder_nodes
    assert call(p, p, 10, 0, 20, 128, p, p, p, 4096, None, None) == EINVAL              # n < 1
    assert call(p, p, 10, (1 << 23) + 1, 20, 128, p, p, p, 4096, None, None) == EINVAL  # n > 2^23
    assert call(p, p, 10, 100, -1, 128, p, p, p, 4096, None, None) == EINVAL            # sweeps < 0
    assert call(p, p, 10, 100, 65, 128, p, p, p, 4096, None, None) == EINVAL            # sweeps > 64
    assert call(p, p, 10, 100, 20, 0, p, p, p, 4096, None, None) == EINVAL              # cap < 1
    assert call(None, p, 10, 100, 20, 128, p, p, p, 4096, None, None) == EINVAL         # edges without src
    assert call(p, None, 10, 100, 20, 128, p, p, p, 4096, None, None) == EINVAL         # edges without dst
    assert call(p, p, 10, 100, 20, 128, None, p, p, 4096, None, None) == EINVAL         # no perm
    assert call(p, p, 10, 100, 20, 128, p, p, None, 0, None, None) == EINVAL            # edges without a work buffer
    assert call(None, None, 0, 0, 20, 128, p, None, None, 0, None, None) == EINVAL      # n < 1 without edges


def test_work_words_domain(lib):
    assert lib.qgtc_reorder_work_words(0, 0) == 0
    assert lib.qgtc_reorder_work_words(-5, 100) == 0
    assert lib.qgtc_reorder_work_words((1 << 23) + 1, 0) == 0
    # the size query asks rocPRIM, which may need the current device: 0 where it fails, else at least the fixed part of the layout
    # (keys a and b, 64-bit; offsets; order, label, proposal; two size arrays). The GPU test checks that it grows with n and edges.
    for n, e in ((1000, 0), (1, 0), (1000, 5000)):
        w = lib.qgtc_reorder_work_words(n, e)
        assert w == 0 or w >= n * (2 + 2 + 2 + 1 + 1 + 1 + 2) + 2 * e * (4 + 1)


def test_mix32_is_lowbias32():
    x = np.array([0, 1, 0x9E3779B9, 0xFFFFFFFF], dtype=np.uint32)
    ref = []
    for v in x.tolist():
        v ^= v >> 16
        v = (v * 0x7FEB352D) & 0xFFFFFFFF
        v ^= v >> 15
        v = (v * 0x846CA68B) & 0xFFFFFFFF
        v ^= v >> 16
        ref.append(v)
    np.testing.assert_array_equal(mix32(x), np.array(ref, dtype=np.uint32))


def test_model_identity_and_permutation():
    rng = np.random.default_rng(5)
    n = 300
    src, dst = rng.integers(0, n, 2000), rng.integers(0, n, 2000)
    perm, rank = reorder_model(src, dst, n, sweeps=0)
    np.testing.assert_array_equal(perm, np.arange(n))
    np.testing.assert_array_equal(rank, np.arange(n))
    perm, rank = reorder_model(np.array([], dtype=np.int64), np.array([], dtype=np.int64), n)
    np.testing.assert_array_equal(perm, np.arange(n))
    perm, rank = reorder_model(src, dst, n, sweeps=20, cap=16)
    assert sorted(perm.tolist()) == list(range(n))
    np.testing.assert_array_equal(perm[rank], np.arange(n))


def test_model_brings_a_shuffled_sbm_back_to_block_local_tiles():
    n = 20000
    s, d, ss, dd = shuffled_sbm(n)
    t_local, t_shuffled = tile_count(s, d, n), tile_count(ss, dd, n)
    perm, rank, ran = reorder_model(ss, dd, n, return_sweeps=True)
    t_reordered = tile_count(rank[ss], rank[dd], n)
    assert t_reordered <= 1.1 * t_local
    assert t_reordered <= 0.25 * t_shuffled
    assert 1 <= ran <= 20
