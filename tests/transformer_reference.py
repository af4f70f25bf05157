"""Dense definition of conv.TransformerConv, written from its docstring as plain torch on the CPU: an n x n matrix built from the raw
edge list in the edge list's own numbering, matrix products, a masked row softmax. No call into the library, no tiled format. float64
is the reference; the same code in float32 only sizes the tolerance (layers_reference.tolerances). The gradients for a given dY come
from torch.autograd on the dense definition (tests/test_transformer_reference.py holds them against central differences).

``WRONG`` names plausible mistakes; ``wrong=`` evaluates the definition with one of them. They are test aids: the CPU test shows that
the inputs of the GPU test tell each mistake from the definition.

``CASES`` are the inputs shared by tests/test_transformer_reference.py (CPU) and tests/test_transformer_dense_gpu.py (the real layer)."""
import numpy as np
import torch

import layers_reference as R

N_NODES, F_IN, OUT = R.N_NODES, R.F_IN, 7
WRONG = ("softmax_over_other_end",   # the weights of edge (i, j) are normalised over the edges into j instead of those out of row i
         "no_scale")                 # the logits are not divided by sqrt(output_dim)
VIEWS = R.VIEWS
GRAPH = R.GRAPHS["random"]


def transformer_layer(src, dst, n, X, W_q, W_k, W_v, dY, view="adj", heads=1, concat=True, dtype=torch.float64, wrong=None):
    """{"Y", "dX", "dW_q", "dW_k", "dW_v"}: q = X W_q, k = X W_k, v = X W_v; per head, on its block of columns,
    alpha = softmax over the neighbours j of row i of the view of q_i . k_j / sqrt(C), out[i] = sum_j alpha[i, j] v_j; a row without
    neighbours gives 0. The heads are concatenated or averaged."""
    assert wrong in (None,) + WRONG
    X, W_q, W_k, W_v = (torch.as_tensor(np.asarray(t), dtype=dtype).clone().requires_grad_(True) for t in (X, W_q, W_k, W_v))
    dY = torch.as_tensor(np.asarray(dY), dtype=dtype)
    C = W_q.shape[1] // heads
    m = torch.from_numpy(R.dense_adjacency(src, dst, n, view))
    scale = torch.tensor(1.0 / np.sqrt(C), dtype=torch.float64).to(torch.float32).to(dtype)   # the layer multiplies by a float32
    if wrong == "no_scale":
        scale = torch.ones((), dtype=dtype)
    q, k, v = X @ W_q, X @ W_k, X @ W_v
    axis = 0 if wrong == "softmax_over_other_end" else 1
    has = m.any(dim=axis, keepdim=True)
    outs = []
    for h in range(heads):
        cols = slice(h * C, (h + 1) * C)
        S = (q[:, cols] @ k[:, cols].T) * scale
        top = torch.where(has, S.masked_fill(~m, float("-inf")).max(dim=axis, keepdim=True).values, torch.zeros((), dtype=dtype)).detach()
        w = torch.where(m, torch.exp(S - top), torch.zeros((), dtype=dtype))
        den = w.sum(dim=axis, keepdim=True)
        alpha = w / torch.where(has, den, torch.ones_like(den))
        outs.append(alpha @ v[:, cols])
    Y = torch.cat(outs, dim=1) if concat else torch.stack(outs).mean(dim=0)
    dX, dq, dk, dv = torch.autograd.grad(Y, (X, W_q, W_k, W_v), dY)
    return {"Y": Y.detach(), "dX": dX, "dW_q": dq, "dW_k": dk, "dW_v": dv}


class Case:
    def __init__(self, name, heads, concat):
        self.name, self.heads, self.concat = name, heads, concat

    def __repr__(self):
        return self.name

    def inputs(self):
        """dict of float64 arrays, the same on every call: X, dY and the parameters, scaled as the constructor scales them"""
        rng = np.random.default_rng([23, [c.name for c in CASES].index(self.name)])
        width = self.heads * OUT
        t = {"X": rng.standard_normal((N_NODES, F_IN)), "dY": rng.standard_normal((N_NODES, width if self.concat else OUT))}
        for name in ("W_q", "W_k", "W_v"):
            t[name] = rng.standard_normal((F_IN, width)) / F_IN ** 0.5
        return t

    def reference(self, view, dtype=torch.float64, wrong=None):
        src, dst, _ = GRAPH
        t = self.inputs()
        return transformer_layer(src, dst, N_NODES, t["X"], t["W_q"], t["W_k"], t["W_v"], t["dY"], view=view, heads=self.heads,
                                 concat=self.concat, dtype=dtype, wrong=wrong)


CASES = []
CASES.extend([Case("transformer-h1-concat", 1, True), Case("transformer-h3-concat", 3, True), Case("transformer-h3-mean", 3, False)])
tolerances = R.tolerances
