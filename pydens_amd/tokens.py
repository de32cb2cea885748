""" The two tokens user equations are written with: `D` (differentiate) and `V` (trainable variable).
Same names, call signatures and meaning as the reference (pydens/model_torch.py:174-188). """
from contextvars import ContextVar

import torch
from torch import nn

from . import trace

current_model = ContextVar("current_model")          # reference model_torch.py:15


# how often D had to differentiate by torch autograd (create_graph) instead of picking a kernel stream: the solver never records a step
# as a launch graph in which that happens (Solver._graph_step)
AUTOGRAD_FALLBACKS = [0]


def D(y, x):
    """ Differentiation token: per-sample dy/dx with y, x of shape [N,1] (reference model_torch.py:174-178).

    The reference runs a nested reverse sweep through the network for every call. Here the derivatives of the
    solution approximation are *streams* computed by the HIP kernels in the forward pass, so
      * `D(f, x)` / `D(D(f, x), x)` on the field (or on a stream) just picks the stream;
      * `D(expr, x)` of an expression of streams and inputs applies the chain rule
        d expr/dx = (d expr/dx)|explicit + sum_a (d expr/d stream_a) * stream_{a + e_x}, the partials by torch
        autograd over the few pointwise ops of `expr` (never through the network);
      * anything unrelated to the field falls back to the reference's plain autograd formula.
    """
    if isinstance(y, trace.Sym) or isinstance(x, trace.Sym):
        return trace.sym_D(y, x)
    alpha = getattr(y, '_pinn_alpha', None)
    col = getattr(x, '_pinn_col', None)
    sc = trace.active_streams.get()
    if alpha is not None and y._pinn_ctx.args is not None:
        # the value (or a derivative stream) of a model call a CONSTRAINT made at points of its own: `x` is one of the tensors the model
        # was called with, and the derivative is the kernel stream along that column -- picked, not differentiated
        ctx = y._pinn_ctx
        cols = ctx.columns_of(x)
        if cols is None:
            ctx.refuse_unrelated(x)
        return ctx.derivative_along(alpha, cols)
    if alpha is not None and col is not None:
        return y._pinn_ctx.derivative(alpha, col)
    # an expression of streams: chain rule over the streams of every context `x` is a column of -- the equation's one context, or, inside a
    # constraint, the context of EVERY model call the constraint has made so far (`D(f(a, t) - f(b, t), t)`: both calls' streams)
    pairs = []
    if sc is not None and sc.args is not None:
        pairs = [(c, c.columns_of(x)) for c in (sc.group if sc.group is not None else [sc])]
        pairs = [(c, cols) for c, cols in pairs if cols is not None]
    elif sc is not None and col is not None:
        pairs = [(sc, (col, ))]
    if pairs and y.requires_grad:
        for c, _ in pairs:
            c.used_autograd_fallback = True
        AUTOGRAD_FALLBACKS[0] += 1
        items = [(c, cols, a, t) for c, cols in pairs for a, t in c.stream_tensors() if t.requires_grad]
        # (x itself is always asked: the explicit partial derivative of `D(x * f(x, t), x)`. The batch columns a differentiating constraint
        #  gets are leaves that require grad for this -- Solver._generic_step)
        wrt = [x] + [t for _, _, _, t in items]
        grads = list(torch.autograd.grad(y.sum(), wrt, retain_graph=True, create_graph=True, allow_unused=True))
        explicit = grads.pop(0)
        total = explicit if explicit is not None else torch.zeros_like(x)
        for (c, cols, a, _), g in zip(items, grads):
            if g is not None:
                total = total + g * c.derivative_along(a, cols)
        return total
    if sc is not None:
        sc.used_autograd_fallback = True
    AUTOGRAD_FALLBACKS[0] += 1
    return torch.autograd.grad(y.sum(), x, retain_graph=True, create_graph=True)[0]


def V(name, *args, **kwargs):
    """ Token for a trainable variable (reference model_torch.py:180-188): created on first use and registered on
    the model of the current context, fetched afterwards. The storage lives in the model's flat parameter buffer
    so that the HIP Adam kernel updates it together with the network. """
    model = current_model.get()
    if not hasattr(model, name):
        param = nn.Parameter(*args, **kwargs)
        register = getattr(model, 'register_variable', None)
        setattr(model, name, register(name, param) if register is not None else param)
    param = getattr(model, name)
    lookup = trace._variable_slot.get()
    if lookup is not None:
        # symbolic trace of the equation (trace.symbolic): a scalar variable is a register of the residual program, so
        # that expressions of variables alone (`0.1 * V('a') * V('b')`) stay symbolic as well
        slot = lookup(param)
        if slot is not None and slot < trace.MAX_VARS:
            return trace.Sym('var', col=slot)
    return param
