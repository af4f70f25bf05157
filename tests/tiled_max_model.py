"""Exact NumPy model of the extremum tiled products (include/qgtc.h, "Extremum tiled products"; QGTC.tiledMMFloat(reduce="max" | "min")
on adj and adj.T, and the select that is their gradient), on tests/tiled_float_model.py's neighbour lists: the fold over each row's
neighbours in ASCENDING id order, all rows at once. Nothing is rounded in the forward and the order of the select's adds is the
contract, so both are compared with the device's bit for bit. No GPU."""
import numpy as np

from tiled_float_model import neighbour_lists

MAX, MIN = 0, 1

# (lanes per output row, columns per lane) of the launchers by output width N: the row view takes the float product's variants for both
# kernels (tiled_max_kernels.hip.h, tiled_red_f32_launch, through tiled_float_kernels.hip.h's tiled_row_width_switch), the column view's
# extremum stops at 32 columns a workgroup (two words of LDS state a column) and its select goes to 64 like the float product
# (tiled_max_t_kernels.hip.h, tiled_red_f32_launch: tiled_col_width_switch with WIDEST 32 / 64). These tables are a hand-kept copy of
# those two switches, as tiled_float_model.py's are: whoever changes a width there changes it here, or the sweep's coverage claim goes
# stale.
MAX_FORWARD_VARIANTS = ((16, 1), (16, 2), (16, 4), (32, 4), (64, 4))
MAX_TRANSPOSED_VARIANTS = ((16, 1), (16, 2))
SELECT_FORWARD_VARIANTS = MAX_FORWARD_VARIANTS
SELECT_TRANSPOSED_VARIANTS = ((16, 1), (16, 2), (16, 4))


def max_variant(N, transposed, select=False):
    """The template variant the launcher picks at output width N."""
    if transposed:
        v = SELECT_TRANSPOSED_VARIANTS if select else MAX_TRANSPOSED_VARIANTS
        return v[0 if N <= 16 else 1 if N <= 32 else len(v) - 1]
    return MAX_FORWARD_VARIANTS[0 if N <= 16 else 1 if N <= 32 else 2 if N <= 64 else 3 if N <= 128 else 4]


def max_chunks(N, transposed, select=False):
    """Workgroups along the output width (grid.y)."""
    lpr, cpl = max_variant(N, transposed, select)
    return (N + lpr * cpl - 1) // (lpr * cpl)


def extremum_f32(src, dst, n, X, transposed=False, op=MAX, highest_id=False, ignore_nan=False):
    """(out float32 [n, N], arg int32 [n, N]): a row without neighbours gives (+0, -1); otherwise (s, a) start as the first neighbour's
    (X[v_1], v_1) and neighbour v_k with x = X[v_k] replaces them when s is not a NaN and (x is a NaN or x > s [min: x < s]).
    `highest_id` (ties go to the highest id: >= for >) and `ignore_nan` (a NaN never wins or blocks, np.fmax's rule) are WRONG rules, test
    aids that show the inputs tell them apart."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    assert X.ndim == 2 and X.shape[0] == n and op in (MAX, MIN)
    out_row, nb, deg = neighbour_lists(src, dst, n, transposed)
    start = np.concatenate([[0], np.cumsum(deg)[:-1]])
    out = np.zeros((n, X.shape[1]), dtype=np.float32)
    arg = np.full((n, X.shape[1]), -1, dtype=np.int32)
    with np.errstate(invalid="ignore"):
        for k in range(int(deg.max()) if deg.size else 0):
            rows = np.flatnonzero(deg > k)
            v = nb[start[rows] + k]
            x, s = X[v], out[rows]
            if k == 0:
                take = np.ones(x.shape, bool)
            else:
                if highest_id:
                    better = (x <= s) if op == MIN else (x >= s)
                else:
                    better = (x < s) if op == MIN else (x > s)
                if ignore_nan:
                    take = (np.isnan(s) & ~np.isnan(x)) | better
                else:
                    take = ~np.isnan(s) & (np.isnan(x) | better)
            out[rows] = np.where(take, x, s)
            arg[rows] = np.where(take, v[:, None].astype(np.int32), arg[rows])
    return out, arg


def select_f32(src, dst, n, dY, arg, transposed=False):
    """float32 [n, N]: s = +0; s = fl32(s + dY[r_k]) over the neighbours r_1 < r_2 < ... of row v where arg[r_k] == v, one np.float32 add
    each; an unselected term adds +0 (the same bits as skipping it: a sum that starts at +0 is never -0). `arg` is any int32 data."""
    dY = np.ascontiguousarray(dY, dtype=np.float32)
    arg = np.ascontiguousarray(arg, dtype=np.int32)
    assert dY.ndim == 2 and dY.shape[0] == n and arg.shape == dY.shape
    out_row, nb, deg = neighbour_lists(src, dst, n, transposed)
    start = np.concatenate([[0], np.cumsum(deg)[:-1]])
    out = np.zeros(dY.shape, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for k in range(int(deg.max()) if deg.size else 0):
            rows = np.flatnonzero(deg > k)
            r = nb[start[rows] + k]
            out[rows] = out[rows] + np.where(arg[r] == rows[:, None], dY[r], np.float32(0.0))
    assert out.dtype == np.float32
    return out
