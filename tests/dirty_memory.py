"""Recycled, poisoned device memory for the operators under test ("Dirty memory").

Every output, every tensor kept for backward and every scratch buffer of this project comes from ``torch.empty``: its words are whatever
the caching allocator's block held last. In a short test that is fresh memory, or the same test's own result; in a training loop it is
last step's gradients. :func:`dirty` makes the allocator hand out blocks whose every 32-bit word is a chosen pattern, so a row an entry
skipped, a statistic it did not write or a flag it did not clear shows in a bit-for-bit comparison.

    with dirty(torch, device, NAN_WORD, inputs=[X, src, dst]) as d:
        adj = QGTC.pack_edges_tiled(src, dst, n)       # packed on dirty memory too
        got = [t.cpu() for t in op(adj, X)]
    same_bits(got, want, "op")

How it works, in plain ``torch.cuda`` calls (no environment variable, no allocator setting, nothing preloaded):

1. collect garbage, synchronise, ``torch.cuda.empty_cache()``: the cache keeps only the segments that live tensors share;
2. every free block those segments still hold is allocated (``torch.cuda.memory_snapshot`` lists them), then ``large_bytes`` in one
   block of the large pool and ``small_bytes`` in 1 MiB blocks of the small pool (the two pools split at 1 MiB requests);
3. all of it is filled with the pattern on the current stream and freed: the cache now holds poisoned blocks only;
4. CONTROL: ``torch.empty`` at sizes on both sides of the pool boundary, and at the sizes the caller names, must read back as the pattern
   everywhere, else :class:`DirtyMemoryError`;
5. the body runs; afterwards ``num_device_alloc`` of ``torch.cuda.memory_stats`` must be what it was after step 3 - an allocation that
   went to the driver was fresh memory, and the case proved nothing: :class:`DirtyMemoryError` says so -, and the ``inputs`` must hold
   the bits they held before: no operator writes to an operand.

The harness never skips. Patterns: :data:`NAN_WORD` is a quiet NaN as a float and a large positive integer; :data:`SMALL_WORD` is about
-2.9e-16 as a float, a plausible small number that a maximum or a sum swallows where a NaN would show, and a negative integer. Any
other 32-bit word works too; 0 imitates the fresh memory a short process usually sees.
"""
from __future__ import annotations

import contextlib
import gc

import numpy as np

NAN_WORD = 0x7FC00000
SMALL_WORD = 0xA5A5A5A5
PATTERNS = (NAN_WORD, SMALL_WORD)

MIB = 1 << 20
SMALL_LIMIT = MIB            # requests up to 1 MiB are served from the small pool (2 MiB segments), larger ones from the large pool
LARGE_BYTES = 256 * MIB      # one poisoned block of the large pool: every larger allocation of a case is split from it
SMALL_BYTES = 32 * MIB       # sixteen poisoned segments of the small pool
CONTROL_SIZES = (512, 4096, 65536, MIB - 512, MIB, MIB + 512, 4 * MIB, 24 * MIB)     # bytes, both sides of the pool boundary

_announced = set()


class DirtyMemoryError(RuntimeError):
    """The harness could not do what it promises: the control read something else than the pattern, or the body got fresh memory."""


def signed(pattern: int) -> int:
    """The 32-bit word as the int32 value ``fill_`` takes."""
    pattern &= 0xFFFFFFFF
    return pattern - (1 << 32) if pattern >= (1 << 31) else pattern


def bits_of(x):
    """A CPU tensor or an array as a flat array of unsigned words of its element size: NaNs and signed zeros compare as bits."""
    if hasattr(x, "detach"):
        x = x.detach().contiguous()
        x = x.view(_int_dtype(x)).cpu().numpy()
    a = np.ascontiguousarray(x)
    return a.reshape(-1).view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _int_dtype(t):
    import torch

    return {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]


def same_bits(got, want, what):
    """got[i] equals want[i] bit for bit (a NaN equals a NaN only where both have the same one); otherwise an AssertionError that names
    the output, the number of differing words and the first of them."""
    got, want = list(got), list(want)
    assert len(got) == len(want), f"{what}: {len(got)} outputs, {len(want)} expected"
    for i, (g, w) in enumerate(zip(got, want)):
        shape_g, shape_w = tuple(g.shape), tuple(w.shape)
        gb, wb = bits_of(g), bits_of(w)
        assert shape_g == shape_w and gb.dtype == wb.dtype, f"{what}: output {i} is {shape_g} x {gb.dtype}, expected {shape_w} x {wb.dtype}"
        bad = np.flatnonzero(gb != wb)
        if bad.size:
            poison = {int(p): int((gb[bad] == p).sum()) for p in PATTERNS if gb.dtype == np.uint32}
            raise AssertionError(f"{what}: output {i} differs in {bad.size} of {gb.size} words (first at {int(bad[0])}: got {int(gb[bad[0]]):#x}, "
                                 f"expected {int(wb[bad[0]]):#x}); of these {poison} hold a poison pattern")


def same_as_model(got, want, what):
    """got[i] (CPU tensors) equals the model's want[i] (arrays) in shape and in value: integers and packed words bit for bit; float32 bit
    for bit too, except that a NaN equals a NaN wherever the model has one (the models do not specify a NaN's payload) - and nowhere
    else. A want of None has no exact model (a torch reduction): it is left to the comparison of the two patterns."""
    got, want = list(got), list(want)
    assert len(got) == len(want), f"{what}: {len(got)} outputs, {len(want)} expected"
    for i, (g, w) in enumerate(zip(got, want)):
        if w is None:
            continue
        g = g.detach().cpu().numpy() if hasattr(g, "detach") else np.asarray(g)
        w = np.asarray(w)
        assert g.dtype.itemsize == w.dtype.itemsize and g.dtype.kind in ("f" if w.dtype.kind == "f" else "iub"), \
            f"{what}: output {i} is {g.dtype}, the model's {w.dtype}"
        assert g.shape == w.shape, f"{what}: output {i} is {g.shape}, the model's {w.shape}"
        gb, wb = bits_of(g), bits_of(w)
        bad = gb != wb
        if w.dtype.kind == "f":
            gn, wn = np.isnan(g).reshape(-1), np.isnan(w).reshape(-1)
            bad = (gn != wn) | (bad & ~wn)
        bad = np.flatnonzero(bad)
        if bad.size:
            k = int(bad[0])
            poison = {f"{p:#010x}": int((gb[bad] == p).sum()) for p in PATTERNS} if gb.dtype == np.uint32 else {}
            raise AssertionError(f"{what}: output {i} {g.shape} differs from the model in {bad.size} of {gb.size} elements (first at flat index "
                                 f"{k}: got {int(gb[k]):#x}, the model has {int(wb[k]):#x}); poison words among them: {poison}")


class Poisoned:
    """What :func:`dirty` yields: the pattern and the bytes it poisoned."""

    def __init__(self, pattern, nbytes, recycled, device_allocs):
        self.pattern, self.nbytes, self.recycled, self.device_allocs = pattern, nbytes, recycled, device_allocs


def _device_allocs(torch, device) -> int:
    return int(torch.cuda.memory_stats(device)["num_device_alloc"])


def _free_blocks(torch, device):
    """(bytes, small pool?) of every free block the cache holds on the device."""
    index = torch.device(device).index
    index = torch.cuda.current_device() if index is None else index
    out = []
    for seg in torch.cuda.memory_snapshot():
        if seg["device"] != index:
            continue
        for b in seg["blocks"]:
            if b["state"] == "inactive":
                out.append((int(b["size"]), seg["segment_type"] == "small"))
    return out


def _take(torch, device, nbytes):
    return torch.empty(nbytes // 4, dtype=torch.int32, device=device)


def _poison(torch, device, pattern, large_bytes, small_bytes):
    """Steps 2 and 3 of the module docstring; (bytes poisoned, of which recycled from segments that live tensors share)."""
    held, recycled = [], 0
    for _ in range(64):      # every pass takes each free block whole, or its first MiB: a few passes empty any segment
        free = _free_blocks(torch, device)
        if not free:
            break
        for size, small in sorted(free):
            take = min(size, SMALL_LIMIT) if small else size
            held.append(_take(torch, device, take))
            recycled += take
    else:
        raise DirtyMemoryError("the cache still holds free blocks after 64 passes over it")
    assert large_bytes % (2 * MIB) == 0 and large_bytes >= 20 * MIB and small_bytes % (2 * MIB) == 0
    held.append(_take(torch, device, large_bytes))                      # a segment of its own, exactly this large
    held += [_take(torch, device, MIB) for _ in range(small_bytes // MIB)]    # two to a 2 MiB segment
    left = _free_blocks(torch, device)
    if left:
        raise DirtyMemoryError(f"{len(left)} free blocks ({sum(s for s, _ in left)} bytes) escaped the poisoning")
    for t in held:
        t.fill_(signed(pattern))
    nbytes = sum(t.numel() * 4 for t in held)
    del held, t
    return nbytes, recycled


def _control(torch, device, pattern, sizes):
    for nbytes in sizes:
        nbytes = max(4, (int(nbytes) + 3) // 4 * 4)
        t = _take(torch, device, nbytes)
        clean = int((t.cpu().numpy() != signed(pattern)).sum())      # compared on the host: a device temporary would overwrite poison
        del t
        if clean:
            raise DirtyMemoryError(f"control: torch.empty of {nbytes} bytes right after poisoning has {clean} words that are not "
                                   f"{pattern:#010x}: the allocator did not serve it from the poisoned blocks")


def _snapshot(inputs):
    return [bits_of(t).copy() for t in inputs]


@contextlib.contextmanager
def dirty(torch, device, pattern, inputs=(), sizes=(), large_bytes=LARGE_BYTES, small_bytes=SMALL_BYTES):
    """The context manager of the module docstring. ``inputs``: the operands of the case, compared bit for bit before and after;
    ``sizes``: byte sizes the case is about to request, added to the control's. Poisoning and body run on the current stream."""
    device = torch.device(device)
    inputs = list(inputs)
    with torch.cuda.device(device):
        gc.collect()                     # tensors that only a reference cycle keeps (autograd contexts of an earlier case) go back now,
        torch.cuda.synchronize(device)   # not in the middle of the poisoning, where their blocks would join the cache unpoisoned
        before = _snapshot(inputs)
        torch.cuda.empty_cache()
        nbytes, recycled = _poison(torch, device, pattern, large_bytes, small_bytes)
        allocs = _device_allocs(torch, device)
        _control(torch, device, pattern, tuple(CONTROL_SIZES) + tuple(sizes))
        if _device_allocs(torch, device) != allocs:
            raise DirtyMemoryError("the control itself went to the driver for memory: the poisoned pool is too small for its sizes")
        yield Poisoned(pattern, nbytes, recycled, allocs)
        torch.cuda.synchronize(device)
        fresh = _device_allocs(torch, device) - allocs
        if fresh:
            raise DirtyMemoryError(f"the body made the allocator ask the driver for memory {fresh} time(s): some buffer was FRESH memory, "
                                   f"not a poisoned block, and this case proved nothing. Raise large_bytes / small_bytes "
                                   f"(now {large_bytes} / {small_bytes}).")
        for i, (b, t) in enumerate(zip(before, inputs)):
            now = bits_of(t)
            if now.shape != b.shape or bool((now != b).any()):
                raise AssertionError(f"input {i} {tuple(t.shape)} changed under the operator: no operator writes to an operand")


def announce(module: str, poisoned: Poisoned) -> None:
    """Print the bytes a case poisons, once per test module."""
    if module not in _announced:
        _announced.add(module)
        print(f"[dirty memory] {module}: every case poisons {poisoned.nbytes} bytes ({poisoned.nbytes / MIB:.1f} MiB; "
              f"{poisoned.recycled} of them recycled from segments that live tensors share) with each of "
              f"{', '.join(f'{p:#010x}' for p in PATTERNS)}")
