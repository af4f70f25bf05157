"""Dense definition of conv.GATv2Conv, written from its docstring as plain torch on the CPU: an n x n matrix built from the raw edge
list in the edge list's own numbering, matrix products, a masked row softmax. No call into the library, no tiled format. float64 is the
reference; the same code in float32 only sizes the tolerance (layers_reference.tolerances). The gradients for a given dY come from
torch.autograd on the dense definition (tests/test_gatv2_reference.py holds them against central differences).

The leaky relu has a kink at u = hr_i + hl_j = 0, where a float32 evaluation could take the other branch than the definition. Every
case therefore ASSERTS, in ``Case.reference``, that the smallest |u_f64| over all edges of the view and all columns is at least
KINK_MARGIN = 64 times the case's largest |u_f32 - u_f64|: no float32 evaluation order can then flip a branch (64 covers a device
``mm`` whose summation order differs from the CPU's). A case that fails the condition gets another seed in CASES; none is skipped.

``WRONG`` names plausible mistakes; ``wrong=`` evaluates the definition with one of them. They are test aids: the CPU test shows that
the inputs of the GPU test tell each mistake from the definition.

``CASES`` are the inputs shared by tests/test_gatv2_reference.py (CPU) and tests/test_gatv2_dense_gpu.py (the real layer): the graph,
forms and head cases of tests/transformer_reference.py, and one case with shared weights."""
import numpy as np
import torch

import layers_reference as R

N_NODES, F_IN, OUT = R.N_NODES, R.F_IN, 7
SLOPE = 0.2
KINK_MARGIN = 64.0
WRONG = ("softmax_over_other_end",   # the weights of edge (i, j) are normalised over the edges into j instead of those out of row i
         "static_attention",         # GAT's logit: the leaky relu after the reduction with att
         "ends_swapped")             # u = hl_i + hr_j: the receiving node transformed by W_l
VIEWS = R.VIEWS
GRAPH = R.GRAPHS["random"]


def _u(src, dst, n, X, W_l, W_r, view, dtype):
    """u[i, j, c] = hr[i, c] + hl[j, c] on the edges of the view, as a [E, N] tensor"""
    X, W_l, W_r = (torch.as_tensor(np.asarray(t), dtype=dtype) for t in (X, W_l, W_r))
    i, j = np.nonzero(R.dense_adjacency(src, dst, n, view))
    return (X @ W_r)[i] + (X @ W_l)[j]


def kink_margin(src, dst, n, X, W_l, W_r, view):
    """(the smallest |u_f64|, the largest |u_f32 - u_f64|) over the edges of the view and all columns"""
    u64, u32 = _u(src, dst, n, X, W_l, W_r, view, torch.float64), _u(src, dst, n, X, W_l, W_r, view, torch.float32)
    return float(u64.abs().min()), float((u32.to(torch.float64) - u64).abs().max())


def gatv2_layer(src, dst, n, X, W_l, W_r, att, dY, view="adj", heads=1, concat=True, slope=SLOPE, shared=False, dtype=torch.float64,
                wrong=None):
    """{"Y", "dX", "dW_l", "dW_r", "datt"} (shared: no "dW_r", and "dW_l" is the gradient of the one matrix): hl = X W_l, hr = X W_r;
    per head, on its block of columns, e[i, j] = att . leaky_relu(hr_i + hl_j), alpha = softmax of e over the neighbours j of row i of
    the view, out[i] = sum_j alpha[i, j] hl_j; a row without neighbours gives 0. The heads are concatenated or averaged."""
    assert wrong in (None,) + WRONG
    X, W_l, W_r, att = (torch.as_tensor(np.asarray(t), dtype=dtype).clone().requires_grad_(True) for t in (X, W_l, W_r, att))
    dY = torch.as_tensor(np.asarray(dY), dtype=dtype)
    C = W_l.shape[1] // heads
    m = torch.from_numpy(R.dense_adjacency(src, dst, n, view))
    a = torch.tensor(slope, dtype=torch.float64).to(torch.float32).to(dtype)   # the layer passes a float32
    hl = X @ W_l
    hr = hl if shared else X @ W_r
    if wrong == "ends_swapped":
        hl_s, hr_s = hr, hl
    else:
        hl_s, hr_s = hl, hr
    axis = 0 if wrong == "softmax_over_other_end" else 1
    has = m.any(dim=axis, keepdim=True)
    outs = []
    for h in range(heads):
        cols = slice(h * C, (h + 1) * C)
        u = hr_s[:, None, cols] + hl_s[None, :, cols]   # [n, n, C]
        if wrong == "static_attention":
            S = (u * att[h]).sum(dim=2)
            S = torch.where(S > 0, S, a * S)
        else:
            S = (torch.where(u > 0, u, a * u) * att[h]).sum(dim=2)
        top = torch.where(has, S.masked_fill(~m, float("-inf")).max(dim=axis, keepdim=True).values, torch.zeros((), dtype=dtype)).detach()
        w = torch.where(m, torch.exp(S - top), torch.zeros((), dtype=dtype))
        den = w.sum(dim=axis, keepdim=True)
        alpha = w / torch.where(has, den, torch.ones_like(den))
        outs.append(alpha @ hl[:, cols])
    Y = torch.cat(outs, dim=1) if concat else torch.stack(outs).mean(dim=0)
    if shared:
        dX, dl, da = torch.autograd.grad(Y, (X, W_l, att), dY)
        return {"Y": Y.detach(), "dX": dX, "dW_l": dl, "datt": da}
    dX, dl, dr, da = torch.autograd.grad(Y, (X, W_l, W_r, att), dY)
    return {"Y": Y.detach(), "dX": dX, "dW_l": dl, "dW_r": dr, "datt": da}


class Case:
    def __init__(self, name, heads, concat, shared=False, seed=0):
        self.name, self.heads, self.concat, self.shared, self.seed = name, heads, concat, shared, seed

    def __repr__(self):
        return self.name

    def inputs(self):
        """dict of float64 arrays, the same on every call: X, dY and the parameters, scaled as the constructor scales them"""
        rng = np.random.default_rng([29, [c.name for c in CASES].index(self.name), self.seed])
        width = self.heads * OUT
        t = {"X": rng.standard_normal((N_NODES, F_IN)), "dY": rng.standard_normal((N_NODES, width if self.concat else OUT))}
        for name in ("W_l", "W_r"):
            t[name] = rng.standard_normal((F_IN, width)) / F_IN ** 0.5
        if self.shared:
            t["W_r"] = t["W_l"]
        t["att"] = rng.standard_normal((self.heads, OUT)) / OUT ** 0.5
        return t

    def margin(self, view):
        src, dst, _ = GRAPH
        t = self.inputs()
        return kink_margin(src, dst, N_NODES, t["X"], t["W_l"], t["W_r"], view)

    def reference(self, view, dtype=torch.float64, wrong=None):
        src, dst, _ = GRAPH
        t = self.inputs()
        least, err = self.margin(view)
        assert least >= KINK_MARGIN * err, f"{self.name} on {view}: min |u| {least:.3e} is below 64 x {err:.3e}: give the case another seed"
        return gatv2_layer(src, dst, N_NODES, t["X"], t["W_l"], t["W_r"], t["att"], t["dY"], view=view, heads=self.heads,
                           concat=self.concat, shared=self.shared, dtype=dtype, wrong=wrong)


CASES = []
# the seeds: the first of 0, 1, 2, ... at which the case holds the kink condition on both views
CASES.extend([Case("gatv2-h1-concat", 1, True, seed=0), Case("gatv2-h3-concat", 3, True, seed=10), Case("gatv2-h3-mean", 3, False, seed=6),
              Case("gatv2-h3-shared", 3, True, shared=True, seed=2)])
tolerances = R.tolerances
