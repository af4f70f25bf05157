"""The cases behind the ledger of bit-GEMM routes x output layouts x requantiser branches (test_bitmm_clamp_ledger.py on the CPU,
test_bitmm_clamp_gpu.py on the device), their operands and their independent NumPy reference. No GPU code, no library, no oracle.

The rule (kernel.h:31-37 as called at :350), written out ONCE here (`requant`): an int32 sum c becomes 1 if c < 0, 2^ob - 1 if c > 2^ob,
else c, and only the low ob bits are stored - so c == 2^ob is kept by the clamp and packs as 0.

Every case puts chosen sums next to that clamp (the staircase block) and random sums on both sides of it (the rest). The operands are
dense: no case skips or jumps a zero tile (see FORMS)."""
import collections
import math

import numpy as np

Case = collections.namedtuple("Case", "form engine zero_skip M K N a w mode ob route")
# one launch / QGTC.BatchedGemm with zero_jump off / on. "grouped_jump" covers the route decision under QGTC_ZERO_JUMP and the kernels'
# bitmap-carrying instantiations; it does NOT jump: these left operands have no empty 32-row x 128-bit tile, so the binding's occupancy
# pass clears the bitmaps (more than a quarter occupied). Jumping itself is tests/test_gpu_extras.py's (sparse block-diagonal operands).
FORMS = ("single", "grouped", "grouped_jump")
OB_CLASSES = ("1", "2", "4", "8", "rt", "hi")    # the compile-time widths, the run-time width (3, 5, 6, 7), and 9 .. 23
SINGLE_ROUTES = ("k_bitmm", "k_bitmm_planes", "k_bitmm_mfma", "k_bitmm_fp4_one", "k_bitmm_fp4_skinny", "k_bitmm_fp4_stream",
                 "k_bitmm_fp4_rows_single", "k_bitmm_fp4_wide")
GROUPED_ROUTES = ("k_bitmm_batched", "k_bitmm_mfma_batched", "k_bitmm_fp4_rows", "k_bitmm_fp4_xw_rows")
ENGINE_FLAGS = {"popcount": 0x0, "mfma": 0x8, "auto": 0x10}
NO_ZERO_SKIP, ZERO_JUMP = 0x2, 0x4               # include/qgtc.h


def ob_class(ob):
    if ob in (1, 2, 4, 8):
        return str(ob)
    if ob in (3, 5, 6, 7):
        return "rt"
    if 9 <= ob <= 23:
        return "hi"
    raise ValueError(f"ob = {ob} is outside the ledger (ob >= 24: tests/test_edge_domain_gpu.py)")


def max_sum(K, a, w):
    return K * ((1 << a) - 1) * ((1 << w) - 1)


def ob_hi(K, a, w):
    """The largest ob in 9 .. 23 whose boundary sums 2^ob - 1 .. 2^ob + 2 a K-long product of a-bit and w-bit values can reach."""
    obs = [ob for ob in range(9, 24) if (1 << ob) + 2 <= max_sum(K, a, w)]
    if not obs:
        raise ValueError(f"K = {K} at {a} x {w} bits is too short for ob >= 9")
    return obs[-1]


def case_id(c):
    return f"{c.route}-{c.form}-{c.engine}-zs{int(c.zero_skip)}-{c.M}x{c.K}x{c.N}-{c.a}x{c.w}-m{c.mode}-ob{c.ob}"


def route_flags(c):
    """The flags the binding passes for this case (qgtc_torch.cpp: mm_flags, BatchedGemm.run)."""
    return ENGINE_FLAGS[c.engine] | (0 if c.zero_skip else NO_ZERO_SKIP) | (ZERO_JUMP if c.form == "grouped_jump" else 0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# The table. One block per kernel; a row of a block is (mode or None for both, ob or "hi", form, zero_skip, M, K, N, a, w). Shapes are the
# smallest the route query admits with M, N no multiple of 32 (one interior 32 x 32 tile and a ragged last one), K no multiple of 128,
# and K long enough for the ob of the row; the plane counts are chosen so that a compile-time OB instantiation is hit where a kernel has
# one (the row-block kernels in cols layout: ob == the right operand's planes).
# ---------------------------------------------------------------------------------------------------------------------------------------
S, G, J = FORMS
_BLOCKS = [
    # AND + popcount, every plane count up to 8 x 8 on a single launch (engine "popcount"): requant() of bitmm_popcount.hip.h
    ("k_bitmm", "popcount", [
        (None, 1, S, True, 37, 515, 35, 1, 1), (None, 2, S, False, 37, 515, 35, 1, 2), (None, 4, S, True, 37, 515, 35, 2, 2),
        (None, 8, S, False, 37, 515, 35, 1, 8), (None, 5, S, True, 37, 515, 35, 3, 5), (None, "hi", S, True, 37, 515, 35, 4, 4),
        (0, "hi", S, False, 37, 515, 35, 1, 1), (1, 3, S, True, 37, 130, 35, 1, 4)]),
    # more than eight left-hand planes with zero-skip on: K > 1024 (more than one chunk of 8 k-quads staged) at 9 planes, and 32 planes
    # with 8 * 32 * STEP128(K) > 1024 (the census loop's second trip)
    ("k_bitmm_planes", "popcount", [
        (None, 1, S, True, 37, 515, 35, 32, 1), (None, 2, S, True, 37, 1100, 35, 9, 1), (None, 4, S, True, 37, 515, 35, 32, 1),
        (None, 8, S, True, 37, 515, 35, 32, 1), (None, 7, S, True, 37, 1100, 35, 9, 2), (None, "hi", S, True, 37, 1100, 35, 9, 1),
        (0, 8, S, True, 37, 1100, 35, 12, 3)]),
    # 128 x 128 tiles on the matrix cores (engine "mfma"): what no FP4 kernel takes - more than 256 columns at three planes, and
    # 8 x 8 bits with K 255 255 >= 2^24 (the int8 form, int32 sums)
    ("k_bitmm_mfma", "mfma", [
        (None, 1, S, True, 37, 515, 261, 3, 1), (None, 2, S, False, 37, 515, 35, 8, 8), (None, 4, S, True, 37, 515, 261, 3, 1),
        (None, 8, S, True, 37, 515, 35, 8, 8), (None, 6, S, True, 37, 515, 261, 3, 1), (None, "hi", S, True, 37, 515, 35, 8, 8),
        (None, "hi", S, False, 37, 515, 261, 3, 1)]),
    # the headline kernel (the default engine): the byte path below plane 8 and the qhi path for planes 8 .. 22
    ("k_bitmm_fp4_one", "auto", [
        (None, 1, S, True, 37, 515, 35, 1, 1), (None, 2, S, False, 37, 515, 35, 2, 2), (None, 4, S, True, 37, 515, 35, 1, 4),
        (None, 8, S, True, 37, 515, 35, 2, 8), (None, 3, S, True, 37, 515, 35, 1, 2), (None, 7, S, False, 37, 515, 35, 2, 4),
        (None, "hi", S, True, 37, 4095, 35, 1, 1), (None, "hi", S, True, 37, 515, 35, 2, 8), (None, "hi", S, False, 37, 515, 35, 1, 1)]),
    # the same operands beyond K = 4096
    ("k_bitmm_fp4_skinny", "auto", [
        (None, 1, S, True, 37, 4225, 35, 1, 1), (None, 2, S, False, 37, 4225, 35, 1, 2), (None, 4, S, True, 37, 4225, 35, 2, 2),
        (None, 8, S, True, 37, 4225, 35, 1, 8), (None, 6, S, False, 37, 4225, 35, 2, 4), (None, "hi", S, True, 37, 4225, 35, 1, 1),
        (None, "hi", S, True, 37, 4225, 35, 2, 8)]),
    # the long-K kernel: one-plane operands, 64-row tiles
    ("k_bitmm_fp4_stream", "mfma", [
        (None, 1, S, True, 70, 4225, 33, 1, 1), (None, 2, S, False, 70, 4225, 33, 1, 1), (None, 4, S, True, 70, 4225, 33, 1, 1),
        (None, 8, S, True, 70, 4225, 33, 1, 1), (None, 5, S, False, 70, 4225, 33, 1, 1), (None, "hi", S, True, 70, 4225, 33, 1, 1)]),
    # single launches with three to eight left-hand planes: requant_pack16<OB> at OB = 4 (4 x 4, 4 x 8 planes) and 8 (8 x 8) against <0>
    ("k_bitmm_fp4_rows_single", "mfma", [
        (None, 1, S, True, 37, 515, 35, 4, 4), (None, 2, S, True, 37, 515, 35, 3, 2), (None, 4, S, True, 37, 515, 35, 4, 4),
        (None, 4, S, True, 37, 515, 35, 4, 8), (None, 8, S, True, 37, 200, 35, 8, 8), (None, 8, S, True, 37, 515, 35, 4, 4),
        (None, 3, S, True, 37, 515, 35, 3, 3), (None, "hi", S, True, 37, 515, 35, 4, 4), (None, "hi", S, True, 37, 200, 35, 8, 8)]),
    # wide right operands (engine "mfma", more than 256 columns). The kernel has TWO bit epilogues, chosen with the fragments per wave
    # (launch_wide.hip.h: nl / nr = the planes of the operand that supplies the output lines / the output bits - a / w in rows layout,
    # w / a in cols layout): 4 x 2 fragments end in the `ob <= 4` / `ob > 4` branches, 2 x 4 and 4 x 4 in requant_pack16<1 / 2 / 0>.
    # The plane counts below FORCE the fragments, whatever wide_plan's cost model says: `if (nr == 8) rf = 4, cf = 2` and
    # `if (nl >= 4) rf = 2, cf = 4`. Every ob class runs on both epilogues in both layouts (wide_epilogue() below; the ledger asserts it).
    ("k_bitmm_fp4_wide", "mfma", [
        # 4 x 2 fragments (nr == 8): ob 1, 2, 3, 4 take `ob <= 4`; ob 5, 6, 8, hi take `ob > 4`
        (0, 1, S, True, 37, 515, 261, 1, 8), (0, 2, S, True, 37, 515, 261, 2, 8), (0, 4, S, True, 37, 515, 261, 1, 8),
        (0, 8, S, True, 37, 515, 261, 2, 8), (0, 3, S, True, 37, 515, 261, 1, 8), (0, 5, S, True, 37, 515, 261, 2, 8),
        (0, "hi", S, True, 37, 515, 261, 2, 8),
        (1, 1, S, True, 37, 515, 261, 8, 1), (1, 2, S, True, 37, 515, 261, 8, 2), (1, 4, S, True, 37, 515, 261, 8, 1),
        (1, 8, S, True, 37, 515, 261, 8, 2), (1, 3, S, True, 37, 515, 261, 8, 1), (1, 6, S, True, 37, 515, 261, 8, 2),
        (1, "hi", S, True, 37, 515, 261, 8, 2),
        # 2 x 4 fragments (nl >= 4): requant_pack16<1> at ob 1, <2> at ob 2, <0> for every other width
        (0, 1, S, True, 37, 515, 261, 4, 1), (0, 2, S, True, 37, 515, 261, 4, 2), (0, 4, S, True, 37, 515, 261, 8, 1),
        (0, 8, S, True, 37, 515, 261, 4, 2), (0, 7, S, True, 37, 515, 261, 4, 1), (0, "hi", S, True, 37, 515, 261, 4, 2),
        (1, 1, S, True, 37, 515, 261, 1, 4), (1, 2, S, True, 37, 515, 261, 2, 4), (1, 4, S, True, 37, 515, 261, 1, 8),
        (1, 8, S, True, 37, 515, 261, 2, 4), (1, 5, S, True, 37, 515, 261, 1, 4), (1, "hi", S, True, 37, 515, 261, 2, 4),
        # one and two planes on both sides: the fragments are the cost model's choice (today 4 x 4 / 2 x 4, requant_pack16 as above)
        (None, 1, S, True, 37, 515, 261, 1, 1), (None, 2, S, True, 37, 515, 261, 2, 2), (None, "hi", S, True, 37, 515, 261, 1, 1)]),
    # grouped AND + popcount (engine "popcount"), nine left-hand planes included (8 x 8 plane blocks)
    ("k_bitmm_batched", "popcount", [
        (None, 1, G, True, 37, 515, 35, 1, 1), (None, 2, J, True, 37, 515, 35, 2, 2), (None, 4, G, False, 37, 515, 35, 1, 4),
        (None, 8, J, True, 37, 515, 35, 9, 1), (None, 6, G, True, 37, 515, 35, 3, 3), (None, "hi", J, True, 37, 515, 35, 4, 4),
        (None, "hi", G, True, 37, 515, 35, 1, 1)]),
    # grouped 128 x 128 tiles: rows / float stages wider than 64 columns with K > 256 and no bitmaps; cols stages the row blocks cannot
    # take (more than 256 columns, or 8 x 8 bits with inexact float32 sums - those with bitmaps too)
    ("k_bitmm_mfma_batched", "mfma", [
        (0, 1, G, True, 37, 515, 70, 1, 1), (0, 2, G, True, 37, 515, 70, 2, 2), (0, 4, G, True, 37, 515, 70, 1, 4),
        (0, 8, J, True, 37, 515, 35, 8, 8), (0, 7, G, True, 37, 515, 70, 3, 3), (0, "hi", G, True, 37, 515, 70, 1, 1),
        (0, "hi", J, True, 37, 515, 35, 8, 8),
        (1, 1, G, True, 37, 515, 261, 1, 1), (1, 2, G, True, 37, 515, 261, 2, 2), (1, 4, J, True, 37, 515, 35, 8, 8),
        (1, 8, G, True, 37, 515, 261, 1, 8), (1, 3, G, True, 37, 515, 261, 3, 3), (1, "hi", G, True, 37, 515, 261, 1, 1),
        (1, "hi", J, True, 37, 515, 35, 8, 8)]),
    # grouped row blocks: OB = 1 / 2 / 4 / 8 against the run-time width in rows layout; in cols layout OB = the right operand's planes
    ("k_bitmm_fp4_rows", "auto", [
        (0, 1, G, True, 37, 515, 35, 1, 1), (0, 2, J, True, 37, 515, 35, 1, 2), (0, 2, G, True, 37, 515, 35, 2, 2),
        (0, 4, G, True, 37, 515, 35, 4, 4), (0, 8, J, True, 37, 515, 35, 1, 8), (0, 8, G, True, 37, 200, 35, 8, 8),
        (0, 5, G, True, 37, 515, 35, 4, 8), (0, "hi", J, True, 37, 515, 35, 4, 4), (0, "hi", G, True, 37, 515, 35, 1, 1),
        (1, 1, G, True, 37, 515, 35, 1, 1), (1, 2, G, True, 37, 515, 35, 2, 2), (1, 2, J, True, 37, 515, 35, 1, 1),
        (1, 4, G, True, 37, 515, 35, 4, 4), (1, 8, G, True, 37, 200, 35, 8, 8), (1, 8, G, True, 37, 515, 35, 1, 8),
        (1, 6, G, True, 37, 515, 35, 2, 2), (1, "hi", G, True, 37, 515, 35, 4, 4), (1, "hi", J, True, 37, 200, 35, 8, 8)]),
    # grouped X . W stages of one k-quad: the two instantiations <2, 2, 2> and <4, 4, 4>
    ("k_bitmm_fp4_xw_rows", "auto", [
        (1, 2, G, True, 37, 100, 35, 2, 2), (1, 2, G, True, 37, 100, 35, 1, 2), (1, 4, G, True, 37, 100, 35, 4, 4),
        (1, 4, J, True, 37, 100, 35, 3, 2)]),
]


def _expand():
    out = []
    for route, engine, rows in _BLOCKS:
        for mode, ob, form, zs, M, K, N, a, w in rows:
            for m in ((0, 1) if mode is None else (mode,)):
                out.append(Case(form, engine, zs, M, K, N, a, w, m, ob_hi(K, a, w) if ob == "hi" else ob, route))
    assert len({case_id(c) for c in out}) == len(out)
    return out


CLAMP_CASES = _expand()

# cells of {route} x {mode 0, mode 1} x {ob class} that no call can reach, each with the rule that says so (launch_common.hip.h,
# qgtc_hip.hip: batched_route)
UNREACHABLE = {
    **{("k_bitmm_fp4_xw_rows", 0, c): "batched_route: `engine && mode == 1 && xw_rows_ok(...)` - mode 0 never takes k_bitmm_fp4_xw_rows"
       for c in OB_CLASSES},
    **{("k_bitmm_fp4_xw_rows", 1, c): "xw_rows_ok: `(a <= 2 && w <= 2 && ob == 2) || (a <= 4 && w <= 4 && ob == 4)` - ob 2 and 4 only"
       for c in ("1", "8", "rt", "hi")},
}


def wide_epilogue(c):
    """Which of k_bitmm_fp4_wide's two bit epilogues the plane counts of a case force (launch_wide.hip.h: `if (nl >= 4) rf = 2, cf = 4;
    if (nr == 8) rf = 4, cf = 2;`): "4x2" = the `ob <= 4` / `ob > 4` branches, "2x4" = requant_pack16<OB>, None = the cost model decides."""
    nl, nr = (c.w, c.a) if c.mode == 1 else (c.a, c.w)
    return "4x2" if nr == 8 else "2x4" if nl >= 4 else None


# ---------------------------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------------------------
def targets(c):
    """The sums the staircase places: both ends, the four next to the clamp, one far above it (where the shape reaches it) and the
    largest the shape allows."""
    top = max_sum(c.K, c.a, c.w)
    t = [0, 1, (1 << c.ob) - 1, 1 << c.ob, (1 << c.ob) + 1, (1 << c.ob) + 2, 1 << (c.ob + 1), top]
    return [v for v in t if v <= top]


def staircase_rows(c):
    return list(range(16)) + ([c.M - 1] if c.M % 32 else [])


def staircase_cols(c):
    return list(range(8)) + ([c.N - 1] if c.N % 32 else [])


def _spans(c):
    """Per target below the largest sum: (the values of the first span, t2); and KA, where the second span starts in every row.
    The first span is t1 ones where that fits K; where it does not (many-plane operands on a short K), the same t1 as
    t1 // (2^a - 1) largest values and one entry with the remainder."""
    maxa = (1 << c.a) - 1
    P = maxa * ((1 << c.w) - 1)
    tt = [(t % P, t // P) for t in targets(c)[:-1]]
    most2 = max(t2 for _, t2 in tt)
    for first in (lambda t1: [1] * t1, lambda t1: [maxa] * (t1 // maxa) + ([t1 % maxa] if t1 % maxa else [])):
        sp = [(first(t1), t2) for t1, t2 in tt]
        KA = max(len(f) for f, _ in sp)
        if KA + most2 <= c.K:
            return sp, KA
    raise ValueError(f"{case_id(c)}: the staircase does not fit K")


def _rest_values(rng, shape, bits, density, mix):
    """Entries set with probability `density`: the largest `bits`-bit value, but for a fraction `mix` of them a uniform one."""
    vmax = (1 << bits) - 1
    v = np.where(rng.random(shape) < mix, rng.integers(1, vmax + 1, size=shape), vmax)
    return (v * (rng.random(shape) < density)).astype(np.int64)


def operands(c):
    """qx [M, K], qw [K, N] as int64 in [0, 2^a) and [0, 2^w), a function of the case alone.

    Staircase rows (the first 16, and the last one of a ragged tile) hold t1 ones from k = 0 and t2 largest values from k = KA. KA is one
    per case, the largest t1, so in the shorter rows the ones are followed by zeros up to KA (_spans: what happens when K is too short).
    Staircase columns (the first 8, and the last one of a ragged tile) are 1 below KA and 2^w - 1 from KA on. A staircase row times a
    staircase column is then exactly t1 + t2 (2^a - 1)(2^w - 1). Row 15 is all 2^a - 1 and column 7 all 2^w - 1: their product is the
    largest sum the shape allows. The targets cycle over the rows.

    Everything else is random. Set entries hold vmax = 2^ra - 1 (2^rw - 1 in qw), ra <= a and rw <= w the widest that leave room under
    the clamp: pr = (2^ra - 1)(2^rw - 1) <= 2^ob / 4. A fraction `mix` of the set entries holds a uniform value in 1 .. vmax instead, so
    a set entry is mean * vmax on average with mean = (1 - mix) + mix (1 + 1 / vmax) / 2. Both operands are set with probability d, so
    the expected sum is K d^2 pr mean mean_w; d solves that for 2^ob. Where even d = 1 falls short of it (`need`, the share of full
    products wanted, above 0.7) every set entry is vmax (mix = 0)."""
    rng = np.random.default_rng([c.M, c.K, c.N, c.a, c.w, c.mode, c.ob, FORMS.index(c.form), sum(map(ord, c.route))])
    maxa, maxw = (1 << c.a) - 1, (1 << c.w) - 1
    ra, rw = c.a, c.w
    while ((1 << ra) - 1) * ((1 << rw) - 1) > max(1, (1 << c.ob) // 4) and (ra > 1 or rw > 1):
        if ra >= rw:
            ra -= 1
        else:
            rw -= 1
    pr = ((1 << ra) - 1) * ((1 << rw) - 1)
    need = (1 << c.ob) / (c.K * pr)
    mix = 0.125 if need <= 0.7 else 0.0
    mean = (1.0 - mix) + mix * 0.5 * (1.0 + 1.0 / max(((1 << ra) - 1), 1))
    mean_w = (1.0 - mix) + mix * 0.5 * (1.0 + 1.0 / max(((1 << rw) - 1), 1))
    d = min(1.0, math.sqrt(need / (mean * mean_w)))
    qx = _rest_values(rng, (c.M, c.K), ra, d, mix)
    qw = _rest_values(rng, (c.K, c.N), rw, d, mix)
    sp, KA = _spans(c)
    rows, cols = staircase_rows(c), staircase_cols(c)
    for i, m in enumerate(rows):
        first, t2 = sp[i % len(sp)]
        qx[m] = 0
        qx[m, :len(first)] = first
        qx[m, KA:KA + t2] = maxa
    qx[15] = maxa
    for n in cols:
        qw[:KA, n] = 1
        qw[KA:, n] = maxw
    qw[:, 7] = maxw
    return qx, qw


def as_int32(q):
    """The int32 view oracle.pack takes (a 32-plane value with its top bit set is negative there)."""
    return (np.asarray(q, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the independent definition
# ---------------------------------------------------------------------------------------------------------------------------------------
def sums(c):
    """The int32 accumulator of every output: the integer product, wrapped to 32 bits as the plane-by-plane shift-accumulate wraps it
    (only 32-plane operands get there)."""
    qx, qw = operands(c)
    s = (qx.astype(np.int64) @ qw.astype(np.int64)) & 0xFFFFFFFF
    return np.where(s >= 1 << 31, s - (1 << 32), s)


def requant(s, ob):
    """THE rule. s: int64 array of int32 sums."""
    lim = np.int64(1) << ob
    return np.where(s < 0, 1, np.where(s > lim, lim - 1, s)) & (lim - 1)


def reference(c):
    """What bit2val of the case's output must give, element for element."""
    return requant(sums(c), c.ob).astype(np.int64)
