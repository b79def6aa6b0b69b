"""PDE layer: equation strings -> residuals (mirrors src/pde.py:12-151 of the reference).

Same public surface as the reference ``PDELayer``: ``add_equation``, ``update_forward_method``, ``eval``,
``__call__(x, return_residue=True)``, ``eqn_num``, ``eqn_names`` and the attributes ``in_vars, out_vars, n_in,
n_out, all_vars, eqns_raw, eqns_fn, forward_method``.

Two evaluation strategies:

* generic (reference semantics, any forward function): every ``dif(a, b)`` is one reverse sweep
  ``torch.autograd.grad(a, b, ones_like(a), create_graph=True, allow_unused=True)`` (reference :8-9);
* jets (hot path): at ``add_equation`` time the expression is rewritten with sympy -- every output symbol becomes
  an applied function of the inputs and each nested ``dif`` is expanded with ``sympy.diff`` -- into an algebraic
  expression of the "jet atoms" u, du/dx, d2u/dx2, ...  ``__call__`` then asks the forward method for those
  derivatives in ONE pass (``local_implicit_grid.jet_context``); if the forward method is the HIP local-implicit-
  grid query it answers with forward-mode jets computed by the CDNA4 kernels, and the residual is plain
  elementwise algebra on them.  If the forward method is anything else (or post-processes the query result) the
  generic strategy is used, exactly like the reference.

Functions (beyond the reference's lambdify defaults): Max / Min of any arity, sign, Heaviside (H(0) = 1/2), Abs under a ``dif``
(``dif(Abs(f), x)`` = sign(f) f_x), real and expression powers, tan sinh cosh asin acos atan atan2 evaluate elementwise on tensors
on every strategy with torch's conventions (ties halve the cotangent, NaN propagates, sign' = H' = 0), and compile into the device
residual program (``_compile_residual_program(..., extended=True)``, opcodes TAN .. STEP of the one table ``_RES_OPS``); DESIGN
section 9 has the envelope.
So do ``Piecewise`` with conditions made of the six relationals, ``And`` / ``Or`` / ``Not`` (a chain of torch.where: every branch
is evaluated, the selected one takes the cotangent, the others exactly 0, nothing reaches a condition; NaN where no condition
holds), ``Heaviside(a, h0)`` and the constants pi, E, EulerGamma, GoldenRatio, Catalan (opcodes LT .. STEPC of
``_RES_OPS``, compiled with ``extended=True, conditional=True``, which PDELayer passes).

Coefficients (an extension of the reference surface): ``PDELayer(in_vars, out_vars, param_vars='nu')`` declares symbols whose
values are tensors handed over with ``update_parameters`` -- one value for all points or one per batch element, optionally
requiring grad (inverse problems, mixed-regime batches).  Both torch strategies take them.  With the HIP jets the residual
algebra of such a layer is by default evaluated by the lambdified torch functions (counted and reported once as
``residual_torch_fallbacks``).  ``PDELayer(..., device_params=True)`` hands it to the HIP residual evaluator instead: a
coefficient compiles to a late-bound CONST (no new opcode: ``_compile_residual_program(..., coef_slots=)``), the kernels
``k_residual_coef_fwd`` / ``_bwd`` read the tensors when they run -- an in-place update is seen by the next call and by the next
replay of a ``train_step.GraphedStep`` -- and the backward sums the coefficient gradients inside its one launch (long
accumulators in deterministic mode).  A coefficient computed from a leaf (``nu = exp(log_nu)``) works through autograd.  The
torch functions still take over, counted as before, for more than 8 coefficients, a coefficient that is not fp32, query points
that are not [B, N, n_in], and a program beyond 192 instructions.
"""
import ctypes as C

import numpy as np
import sympy
import torch
from sympy.core.function import AppliedUndef
from sympy.parsing.sympy_parser import parse_expr
from sympy.printing.pycode import PythonCodePrinter
from torch.autograd import grad

from . import _lib
from . import local_implicit_grid as _lig


def torch_diff(y, x):
    """``dif(y, x)``: d(sum y)/dx keeping the graph (reference pde.py:8-9)."""
    return grad(y, x, grad_outputs=torch.ones_like(y), create_graph=True, allow_unused=True)[0]


def _tensor_args(args):
    """Numbers among the arguments of a two-tensor torch function (``Max(u, 0)``, ``atan2(u, 1)``) as 0-d tensors of the
    dtype and device of the first tensor argument."""
    ref = next((a for a in args if torch.is_tensor(a)), None)
    if ref is None:
        return [torch.as_tensor(float(a)) for a in args]
    return [a if torch.is_tensor(a) else torch.as_tensor(float(a), dtype=ref.dtype, device=ref.device) for a in args]


def _t_max(*args):
    """``Max(a, b, ...)``: a chain of torch.maximum (NaN propagates, a tie halves the cotangent) from left to right."""
    args = _tensor_args(args)
    r = args[0]
    for a in args[1:]:
        r = torch.maximum(r, a)
    return r


def _t_min(*args):
    args = _tensor_args(args)
    r = args[0]
    for a in args[1:]:
        r = torch.minimum(r, a)
    return r


def _t_sign(a):
    """torch.sign (sign(0) = 0, gradient 0) with sign(NaN) = NaN: torch's own gives 0 there."""
    a, = _tensor_args([a])
    return torch.where(a != a, a.detach(), torch.sign(a))


def _t_heaviside(a, h0=0.5):
    """sympy's Heaviside: 1, 0, H(0) = h0 (1/2 by default: the tie rule of Max / Min), NaN for NaN; gradient 0."""
    a, = _tensor_args([a])
    s = _t_sign(a)
    return torch.where(a == 0, torch.as_tensor(float(h0), dtype=a.dtype, device=a.device), 0.5 * (s + 1.0))


def _t_atan2(a, b):
    return torch.atan2(*_tensor_args([a, b]))


def _t_rel(op):
    """A relational as a bool tensor: IEEE comparisons, a NaN operand gives False except for ``!=``."""
    def rel(a, b):
        return op(*_tensor_args([a, b]))
    return rel


def _t_and(*args):
    r = args[0]
    for a in args[1:]:
        r = torch.logical_and(torch.as_tensor(r), torch.as_tensor(a))
    return r


def _t_or(*args):
    r = args[0]
    for a in args[1:]:
        r = torch.logical_or(torch.as_tensor(r), torch.as_tensor(a))
    return r


def _t_not(a):
    return torch.logical_not(torch.as_tensor(a))


def _t_piecewise(like, *pairs):
    """``Piecewise((e1, c1), ..., (en, cn))``: the right-nested torch.where(c1, e1, where(c2, e2, ...)).  Every branch is evaluated;
    the selected one takes the cotangent and the others exactly 0 (torch.where's autograd).  A condition that is the constant
    True ends the chain; without one the chain ends in NaN, sympy's value where no condition holds.  Branches that are plain
    numbers become 0-d tensors of the dtype and device of ``like`` (a symbol of the expression) and broadcast."""
    def val(e):
        return e if torch.is_tensor(e) else torch.as_tensor(float(e), dtype=like.dtype, device=like.device)

    chain, r = [], None
    for e, c in pairs:
        if c is True:
            r = val(e)
            break
        if c is not False:
            chain.append((val(e), c))
    if r is None:
        r = val(float("nan"))
    for e, c in reversed(chain):
        r = torch.where(c, e, r)
    return r


_TORCH_FUNCS = {"sin": torch.sin, "cos": torch.cos, "tan": torch.tan, "exp": torch.exp, "log": torch.log,
                "sqrt": torch.sqrt, "tanh": torch.tanh, "sinh": torch.sinh, "cosh": torch.cosh, "Abs": torch.abs,
                "asin": torch.asin, "acos": torch.acos, "atan": torch.atan, "atan2": _t_atan2, "Max": _t_max, "Min": _t_min,
                "sign": _t_sign, "Heaviside": _t_heaviside, "Piecewise": _t_piecewise, "And": _t_and, "Or": _t_or, "Not": _t_not,
                "StrictLessThan": _t_rel(torch.lt), "LessThan": _t_rel(torch.le), "StrictGreaterThan": _t_rel(torch.gt),
                "GreaterThan": _t_rel(torch.ge), "Equality": _t_rel(torch.eq), "Unequality": _t_rel(torch.ne)}


class _TorchPrinter(PythonCodePrinter):
    """The printer sympy.lambdify picks for these modules, except that Max, Min, sign, Heaviside, Piecewise, And / Or / Not and
    the six relationals print as calls of the elementwise functions above: as Python conditionals and comparisons chained with
    ``and`` / ``or`` (the stock printer) they cannot take tensors."""

    def _call(self, e):
        return "%s(%s)" % (e.func.__name__, ", ".join(self._print(a) for a in e.args))

    _print_Max = _print_Min = _print_sign = _print_Heaviside = _print_And = _print_Or = _print_Not = _call
    _print_Relational = _call

    def _print_Piecewise(self, e):
        like = min(e.free_symbols, key=lambda s: (s.name, getattr(s, "dummy_index", 0)))
        pairs = ", ".join("(%s, %s)" % (self._print(v), self._print(c)) for v, c in e.args)
        return "Piecewise(%s, %s)" % (self._print(like), pairs)


def _lambdify(args, expr, extra=None):
    """sympy.lambdify onto the torch functions (and ``extra``, e.g. dif), with the settings lambdify gives its own printer."""
    modules = ([extra] if extra else []) + [_TORCH_FUNCS]
    names = {k: k for m in modules for k in m}
    printer = _TorchPrinter({'fully_qualified_modules': False, 'inline': True, 'allow_unknown_functions': True,
                             'user_functions': names})
    return sympy.lambdify(args, expr, modules, printer=printer)


class _RealSign(sympy.Function):
    """sign of a real argument while PDELayer._compile_jet differentiates: derivative 0, as torch.sign's."""
    nargs = 1

    def fdiff(self, argindex=1):
        return sympy.S.Zero


class _RealAbs(sympy.Function):
    """Abs of a real argument while PDELayer._compile_jet differentiates: d|f| = sign(f) df."""
    nargs = 1

    def fdiff(self, argindex=1):
        return _RealSign(self.args[0])


class _JetProgram:
    """Residual as a function of input columns and jet atoms."""

    def __init__(self, fn, atoms, expr=None, syms=None):
        self.fn = fn          # callable(*in_cols, *atom_tensors)
        self.atoms = atoms    # list of (out_index, multi_index tuple sorted)  e.g. (2, ()) / (2, (1,)) / (2, (1, 1))
        self.expr = expr      # sympy expression in the atom symbols (kept for the combined-stream rewrite)
        self.syms = syms      # {atom key: sympy Dummy}


# ---- residual programs for the HIP evaluator (stpde_residual_fwd / _bwd) ---------------------------------------
# The opcodes, numbered in the order of the STPDE_RES_* enum of include/stpde_hip.h.  JET .. OUT are what every program may hold;
# TAN .. STEP only programs compiled with extended=True; LT .. STEPC only those compiled with extended=True, conditional=True:
# masks (1.0 / 0.0) of relationals and logic, the three-operand select of a Piecewise chain -- a = mask, b = then | else << 16 --
# and Heaviside with H(0) = c.
_RES_OPS = {name: k for k, name in enumerate(
    "JET X CONST ADD SUB MUL DIV NEG POWI SIN COS EXP LOG SQRT TANH ABS OUT "
    "TAN SINH COSH ASIN ACOS ATAN ATAN2 POWC POW MIN MAX SIGN STEP "
    "LT LE EQ NE AND OR NOT SEL STEPC".split())}
_RES_UNARY = {sympy.sin: "SIN", sympy.cos: "COS", sympy.exp: "EXP", sympy.log: "LOG", sympy.tanh: "TANH",
              sympy.Abs: "ABS"}
_RES_UNARY_EXT = {sympy.tan: "TAN", sympy.sinh: "SINH", sympy.cosh: "COSH", sympy.asin: "ASIN", sympy.acos: "ACOS",
                  sympy.atan: "ATAN", sympy.sign: "SIGN"}
_RES_REL = {sympy.StrictLessThan: ("LT", False), sympy.LessThan: ("LE", False), sympy.StrictGreaterThan: ("LT", True),
            sympy.GreaterThan: ("LE", True), sympy.Equality: ("EQ", False), sympy.Unequality: ("NE", False)}   # (opcode, swap)
_RES_NUMBER_SYMBOLS = (sympy.pi, sympy.E, sympy.EulerGamma, sympy.GoldenRatio, sympy.Catalan)
_RES_MAX_INS = 192      # STPDE_RES_MAX_INS
_RES_DT = np.dtype([("op", "<i4"), ("a", "<i4"), ("b", "<i4"), ("c", "<f4")])   # = stpde_res_ins


class _Unsupported(Exception):
    pass


def _compile_residual_program(exprs, in_vars, sym_to_slot, extended=False, conditional=False, coef_slots=None):
    """Straight-line SSA program (common sub-expressions shared) for a list of sympy expressions.

    sym_to_slot: {sympy symbol: (stream, channel)} for the jet atoms.  Returns (numpy program, uses_x) or None when
    an expression contains something the device evaluator does not implement.  extended: also use the opcodes
    TAN .. STEP of _RES_OPS, for what the 17 up to OUT cannot express (Max / Min as a chain, sign, Heaviside with H(0) = 1/2, real
    and expression exponents, tan sinh cosh asin acos atan atan2).  conditional (with extended): also use LT .. STEPC,
    for what extended alone rejects (Piecewise over relationals joined by And / Or / Not as a chain of selects on float masks;
    Heaviside with another H(0); pi, E, EulerGamma, GoldenRatio and Catalan as fp32 constants, as an exponent too).  What
    compiles without a switch compiles to the same bytes with it.

    coef_slots: {sympy symbol: k} for coefficients whose values the device reads from tensors (stpde_residual_coef_fwd / _bwd).
    Such a symbol compiles to ONE late-bound CONST (a = k, b = 1, c = 0; every other CONST has a = b = 0), and the return value
    becomes (program, uses_x, the sorted k the program reads).  None: nothing changes."""
    ins, memo, uses_x, used_coefs = [], {}, [False], set()

    def emit(op, a=0, b=0, c=0.0):
        ins.append((_RES_OPS[op], int(a), int(b), float(c)))
        return len(ins) - 1

    def number_symbol(e):
        return float(np.float32(float(e.evalf(30))))

    def cond(c):
        """A Piecewise condition as a float mask, 1.0 or 0.0."""
        if c in memo:
            return memo[c]
        if type(c) in _RES_REL:
            op, swap = _RES_REL[type(c)]
            a, b = rec(c.args[0]), rec(c.args[1])
            idx = emit(op, b, a) if swap else emit(op, a, b)
        elif isinstance(c, (sympy.And, sympy.Or)):
            op = "AND" if isinstance(c, sympy.And) else "OR"
            idx = cond(c.args[0])
            for t in c.args[1:]:
                idx = emit(op, idx, cond(t))
        elif isinstance(c, sympy.Not):
            idx = emit("NOT", cond(c.args[0]))
        else:
            raise _Unsupported(c)
        memo[c] = idx
        return idx

    def rec_ext(e):
        """What only the extended opcodes express."""
        if conditional and e in _RES_NUMBER_SYMBOLS:
            return emit("CONST", c=number_symbol(e))
        if conditional and e.is_Piecewise:
            # SEL(mask, then, else) from the last branch backwards; every branch is evaluated, as torch.where's are
            pairs = list(e.args)
            if pairs[-1][1] == sympy.true:
                idx = rec(pairs.pop()[0])
            else:
                idx = emit("CONST", c=float("nan"))                 # no condition holds: sympy's nan
            for ex, c in reversed(pairs):
                idx = emit("SEL", cond(c), rec(ex) | idx << 16)
            return idx
        if e.is_Pow:
            base, ex = e.args
            if ex.is_Float and float(ex).is_integer():
                return emit("POWI", rec(base), int(ex))             # u**2.0: the exact integer power
            if ex.is_Number:
                if not (ex.is_real and ex.is_finite):
                    raise _Unsupported(e)
                return emit("POWC", rec(base), c=float(ex))
            if conditional and ex in _RES_NUMBER_SYMBOLS:
                return emit("POWC", rec(base), c=number_symbol(ex))
            return emit("POW", rec(base), rec(ex))
        if e.func in (sympy.Max, sympy.Min):
            op = "MAX" if e.func is sympy.Max else "MIN"
            idx = rec(e.args[0])
            for t in e.args[1:]:
                idx = emit(op, idx, rec(t))
            return idx
        if e.func is sympy.Heaviside and (len(e.args) == 1 or e.args[1] == sympy.Rational(1, 2)):
            return emit("STEP", rec(e.args[0]))
        if conditional and e.func is sympy.Heaviside and e.args[1].is_Number and e.args[1].is_real and e.args[1].is_finite:
            return emit("STEPC", rec(e.args[0]), c=float(e.args[1]))    # (STEP's c is 0 and means 1/2)
        if e.func is sympy.atan2:
            return emit("ATAN2", rec(e.args[0]), rec(e.args[1]))
        if e.func in _RES_UNARY_EXT and len(e.args) == 1:
            return emit(_RES_UNARY_EXT[e.func], rec(e.args[0]))
        raise _Unsupported(e)

    def rec(e):
        if e in memo:
            return memo[e]
        if e.is_Symbol:
            if e in sym_to_slot:
                idx = emit("JET", *sym_to_slot[e])
            elif e in in_vars:
                uses_x[0] = True
                idx = emit("X", in_vars.index(e))
            elif coef_slots is not None and e in coef_slots:
                used_coefs.add(int(coef_slots[e]))
                idx = emit("CONST", coef_slots[e], 1)
            else:
                raise _Unsupported(e)
        elif e.is_Number:
            if not e.is_real or not e.is_finite:
                raise _Unsupported(e)
            idx = emit("CONST", c=float(e))
        elif e.is_Add:
            terms = list(e.args)
            pos = [t for t in terms if not t.could_extract_minus_sign()] or [terms[0]]
            first = pos[0]
            idx = rec(first)
            for t in terms:
                if t is first:
                    continue
                if t.could_extract_minus_sign():
                    idx = emit("SUB", idx, rec(-t))
                else:
                    idx = emit("ADD", idx, rec(t))
        elif e.is_Mul:
            c, rest = e.as_coeff_Mul()
            if c == -1:
                idx = emit("NEG", rec(rest))
            else:
                num, den = [], []
                for f in e.args:
                    if f.is_Pow and f.args[1].is_Integer and f.args[1] < 0:
                        den.append(sympy.Pow(f.args[0], -f.args[1]))
                    else:
                        num.append(f)
                idx = rec(num[0]) if num else emit("CONST", c=1.0)
                for f in num[1:]:
                    idx = emit("MUL", idx, rec(f))
                for f in den:
                    idx = emit("DIV", idx, rec(f))
        elif e.is_Pow:
            base, ex = e.args
            if ex.is_Integer:
                idx = emit("POWI", rec(base), int(ex))
            elif ex == sympy.Rational(1, 2):
                idx = emit("SQRT", rec(base))
            elif ex == -sympy.Rational(1, 2):
                idx = emit("DIV", emit("CONST", c=1.0), emit("SQRT", rec(base)))
            elif extended:
                idx = rec_ext(e)
            else:
                raise _Unsupported(e)
        elif e.func in _RES_UNARY and len(e.args) == 1:
            idx = emit(_RES_UNARY[e.func], rec(e.args[0]))
        elif extended:
            idx = rec_ext(e)
        else:
            raise _Unsupported(e)
        memo[e] = idx
        return idx

    try:
        for k, e in enumerate(exprs):
            emit("OUT", rec(sympy.sympify(e)), k)
    except _Unsupported:
        return None
    if len(ins) > _RES_MAX_INS:
        return None
    if coef_slots is not None:
        return np.array(ins, dtype=_RES_DT), uses_x[0], sorted(used_coefs)
    return np.array(ins, dtype=_RES_DT), uses_x[0]


_warned = set()


def _note_fallback(counter, message):
    """Count (``local_implicit_grid.stats[counter]``) and report ONCE per kind that a slower strategy was taken; results
    are the same either way (nothing logged that the HIP residual program was not used)."""
    _lig.stats[counter] = _lig.stats.get(counter, 0) + 1
    if counter not in _warned:
        _warned.add(counter)
        import warnings
        warnings.warn("space_time_pde_amd.pde: " + message, RuntimeWarning, stacklevel=3)


class _ResidualHip(torch.autograd.Function):
    """res[n_eq, P] = program(jets[S, n_out, P], x[P, 3]); backward returns d loss / d jets."""

    @staticmethod
    @_lib.guarded
    def forward(ctx, jets, x2d, prog_t, nins, n_eq):
        L = _lib.lib()
        P, n_out = jets.shape[2], jets.shape[1]
        # as it is when its rows are unit-stride and neither rows nor streams overlap (dense, or a slice of padded rows)
        if not (jets.stride(2) == 1 and jets.stride(1) >= P and jets.stride(0) >= (n_out - 1) * jets.stride(1) + P):
            jets = jets.contiguous()
        res = torch.empty(n_eq, P, device=jets.device, dtype=torch.float32)
        _lib.check(L.stpde_residual_fwd(_lib.ptr(prog_t), nins, n_eq, n_out, P, _lib.ptr(jets), jets.stride(0),
                                        jets.stride(1), _lib.ptr(x2d), _lib.ptr(res), _lib.stream_ptr()))
        ctx.save_for_backward(jets, x2d, prog_t)
        ctx.meta = (nins, n_eq)
        return res

    @staticmethod
    @torch.autograd.function.once_differentiable
    @_lib.guarded
    def backward(ctx, gres):
        L = _lib.lib()
        jets, x2d, prog_t = ctx.saved_tensors
        nins, n_eq = ctx.meta
        P, n_out = jets.shape[2], jets.shape[1]
        jbar = _jets_bar_like(jets)
        _lib.check(L.stpde_residual_bwd(_lib.ptr(prog_t), nins, n_eq, n_out, P, _lib.ptr(jets), jets.stride(0),
                                        jets.stride(1), _lib.ptr(x2d), _lib.ptr(gres.contiguous()), _lib.ptr(jbar),
                                        _lib.stream_ptr()))
        return jbar, None, None, None, None


def _jets_bar_like(jets):
    """The zero-filled jets_bar of a residual backward.  jets may be the slice [:, :, :P] of a buffer whose rows are padded
    (lig_jet.lig_jets at an odd point count), and the kernels address jets_bar with the strides of jets: one zero-filled block of
    that extent, viewed the same way (zeros_like would return dense strides for such a slice)."""
    extent = (jets.shape[0] - 1) * jets.stride(0) + (jets.shape[1] - 1) * jets.stride(1) + jets.shape[2]
    return torch.zeros(extent, device=jets.device, dtype=jets.dtype).as_strided(jets.shape, jets.stride())


class _ResidualCoefHip(torch.autograd.Function):
    """_ResidualHip for a program with late-bound CONSTs: ``coefs`` are the tensors the program reads (fp32, contiguous, on the
    device of the jets, [] / [1] / [B]), ``ks`` their coefficient indices.  backward returns d loss / d jets and, for every
    coefficient that wants one, its gradient in the tensor's own shape -- summed over the points inside the kernel."""

    @staticmethod
    def _record(coefs, ks, n_batch, P, bars=None):
        rec = _lib.ResCoefs()
        rec.n = max(ks) + 1
        rec.n_per_batch = P // n_batch
        rec.det = 1 if (bars is not None and _lib.deterministic) else 0
        for j, (k, t) in enumerate(zip(ks, coefs)):
            rec.per_batch[k] = 1 if t.numel() != 1 else 0
            rec.value[k] = t.data_ptr()
            if bars is not None and bars[j] is not None:
                rec.bar[k] = bars[j].data_ptr()
        for k in range(rec.n):          # an index the program does not read: any valid address (it is never dereferenced per point)
            if not rec.value[k]:
                rec.value[k] = coefs[0].data_ptr()
        return rec

    @staticmethod
    @_lib.guarded
    def forward(ctx, jets, x2d, prog_t, nins, n_eq, n_batch, ks, *coefs):
        L = _lib.lib()
        P, n_out = jets.shape[2], jets.shape[1]
        if not (jets.stride(2) == 1 and jets.stride(1) >= P and jets.stride(0) >= (n_out - 1) * jets.stride(1) + P):
            jets = jets.contiguous()
        res = torch.empty(n_eq, P, device=jets.device, dtype=torch.float32)
        rec = _ResidualCoefHip._record(coefs, ks, n_batch, P)
        _lib.check(L.stpde_residual_coef_fwd(_lib.ptr(prog_t), nins, n_eq, n_out, P, _lib.ptr(jets), jets.stride(0),
                                             jets.stride(1), _lib.ptr(x2d), _lib.ptr(res), C.byref(rec), _lib.stream_ptr()))
        ctx.save_for_backward(jets, x2d, prog_t, *coefs)
        ctx.meta = (nins, n_eq, n_batch, ks)
        return res

    @staticmethod
    @torch.autograd.function.once_differentiable
    @_lib.guarded
    def backward(ctx, gres):
        L = _lib.lib()
        jets, x2d, prog_t = ctx.saved_tensors[:3]
        coefs = ctx.saved_tensors[3:]
        nins, n_eq, n_batch, ks = ctx.meta
        P, n_out = jets.shape[2], jets.shape[1]
        jbar = _jets_bar_like(jets)
        want = ctx.needs_input_grad[7:]
        det = _lib.deterministic
        per = 2 * _lib.DET_K if det else 1            # floats of storage per gradient element
        sizes = [t.numel() if w else 0 for t, w in zip(coefs, want)]
        acc = torch.zeros(max(1, sum(sizes)) * per, device=jets.device, dtype=torch.float32)
        bars, o = [], 0
        for n in sizes:
            bars.append(acc[o * per:(o + n) * per] if n else None)
            o += n
        rec = _ResidualCoefHip._record(coefs, ks, n_batch, P, bars)
        _lib.check(L.stpde_residual_coef_bwd(_lib.ptr(prog_t), nins, n_eq, n_out, P, _lib.ptr(jets), jets.stride(0),
                                             jets.stride(1), _lib.ptr(x2d), _lib.ptr(gres.contiguous()), _lib.ptr(jbar),
                                             C.byref(rec), _lib.stream_ptr()))
        if det and o:       # the long accumulators -> fp32 (train_step._LossSumHip's pattern)
            out = torch.empty(o, device=jets.device, dtype=torch.float32)
            _lib.check(L.stpde_det_finalize(_lib.ptr(acc), o, _lib.ptr(out), _lib.stream_ptr()))
            acc, per = out, 1
        grads, o = [], 0
        for t, n in zip(coefs, sizes):
            grads.append(acc[o:o + n].reshape(t.shape) if n else None)
            o += n
        return (jbar, None, None, None, None, None, None) + tuple(grads)


class PDELayer(object):
    """PDE Layer for querying values and computing PDE residues."""

    def __init__(self, in_vars, out_vars, param_vars='', device_params=False):
        """in_vars / out_vars: strings of variable names, e.g. 'x, y, t' and 'u, v, p'; param_vars: names of coefficient
        symbols (e.g. 'nu' or 'Ra, Pr') whose values ``update_parameters`` sets; device_params: with the HIP jets, evaluate the
        residuals of a layer with coefficients in the HIP residual kernels too, which then read the coefficient tensors (off: the
        lambdified torch functions evaluate them)."""
        self.device_params = bool(device_params)
        self.in_vars = sympy.symbols(in_vars)
        self.out_vars = sympy.symbols(out_vars)
        self.param_vars = sympy.symbols(param_vars) if param_vars.strip() else ()
        if not isinstance(self.in_vars, tuple):
            self.in_vars = (self.in_vars,)
        if not isinstance(self.out_vars, tuple):
            self.out_vars = (self.out_vars,)
        if not isinstance(self.param_vars, tuple):
            self.param_vars = (self.param_vars,)
        self.params = {}     # {name: tensor} set by update_parameters
        self.n_in = len(self.in_vars)
        self.n_out = len(self.out_vars)
        self.all_vars = list(self.in_vars) + list(self.out_vars)
        self.eqns_raw = {}   # raw string equations
        self.eqns_fn = {}    # lambda functions (generic autograd strategy)
        self.eqns_jet = {}   # _JetProgram or None per equation
        self._combo = False  # lazily built combined-second-order plan (False = not built yet)
        self._res_progs = {}  # {(stream layout key): compiled device residual program or None}
        self._res_coefs = {}  # {(stream layout key): the coefficient indices that program reads}
        self.forward_method = None

    # ------------------------------------------------------------------------------------------------
    def add_equation(self, eqn_str, eqn_name='', subs_dict=None):
        """Add the residue expression of one equation; ``dif(y,x)`` denotes dy/dx (reference :37-86).

        Raises ValueError when the expression uses symbols outside in_vars/out_vars/param_vars.
        """
        if not eqn_name:
            # the reference formats 'eqn_{i}' with a positional argument and therefore raises KeyError here
            # (quirk a-Q5); the documented intent -- a default name eqn_<index> -- is implemented instead.
            eqn_name = 'eqn_{}'.format(len(self.eqns_raw.keys()))
        expr = parse_expr(eqn_str)
        if subs_dict:
            for key, val in subs_dict.items():   # sequential substitution, as the reference
                expr = expr.subs(key, val)
        valid_var = expr.free_symbols <= (set(self.in_vars) | set(self.out_vars) | set(self.param_vars))
        if not valid_var:
            raise ValueError('Variables in the eqn_str ({}) does not match that of '
                             'in_vars ({}), out_vars ({}) and param_vars ({})'.format(
                                 expr.free_symbols, set(self.in_vars), set(self.out_vars), set(self.param_vars)))
        fn = _lambdify(self.all_vars + list(self.param_vars), expr, {'dif': torch_diff})
        self.eqns_raw.update({eqn_name: eqn_str})
        self.eqns_fn.update({eqn_name: fn})
        self.eqns_jet.update({eqn_name: self._compile_jet(expr)})
        self._combo = False   # combined-second-order plan is rebuilt lazily
        self._res_progs = {}
        self._res_coefs = {}

    def _combo_plan(self):
        """If every equation is LINEAR in the second derivatives and uses them only through one common combination
        L y_c = sum_p alpha_p d2y_c/dq_a dq_b (same alpha for all channels and equations, e.g. the anisotropic Laplacian
        nu_x^2 d_xx + nu_z^2 d_zz of the Rayleigh-Benard set), the network only has to carry ONE second-order stream.
        Returns dict(alpha={pair: float}, progs={name: _JetProgram}) or None."""
        if self._combo is not False:
            return self._combo
        self._combo = None
        progs = self.eqns_jet
        if not progs or any(p is None for p in progs.values()):
            return None
        try:
            groups = {}
            for name, prog in progs.items():
                s2 = {k: v for k, v in prog.syms.items() if len(k[1]) == 2}
                # a Piecewise condition is not differentiated below: a second derivative in one is not linear use
                if s2 and any(c.has(*s2.values()) for pw in prog.expr.atoms(sympy.Piecewise) for _, c in pw.args):
                    return None
                for key, sym in s2.items():
                    coeff = sympy.diff(prog.expr, sym)
                    if any(coeff.has(t) for t in s2.values()):
                        return None                        # non-linear in the second derivatives
                    groups.setdefault((name, key[0]), {})[key[1]] = coeff
            if not groups:
                return None
            pairs = sorted({p for g in groups.values() for p in g})
            if len(pairs) < 2:
                return None                                # a single pair is already one stream
            ref = pairs[0]
            alpha = {ref: 1.0}
            for g in groups.values():
                if ref not in g or g[ref] == 0:
                    return None
                for p in pairs[1:]:
                    ratio = sympy.simplify(g.get(p, sympy.Integer(0)) / g[ref])
                    if not ratio.is_number:
                        return None
                    r = float(ratio)
                    if p in alpha:
                        if abs(alpha[p] - r) > 1e-9 * max(1.0, abs(r)):
                            return None
                    else:
                        alpha[p] = r
            new = {}
            for name, prog in progs.items():
                repl, lam = {}, {}
                for key, sym in prog.syms.items():
                    if len(key[1]) == 2:
                        if key[1] == ref:
                            lam[key[0]] = sympy.Dummy("L%d" % key[0])
                            repl[sym] = lam[key[0]]
                        else:
                            repl[sym] = sympy.Integer(0)
                e = prog.expr.xreplace(repl)
                atoms = [(k, v) for k, v in prog.syms.items() if len(k[1]) < 2] + \
                        [((c, ("L",)), v) for c, v in lam.items()]
                atoms.sort(key=lambda a: (a[0][0], len(a[0][1]), str(a[0][1])))
                fn = _lambdify(list(self.in_vars) + list(self.param_vars) + [a[1] for a in atoms], e)
                new[name] = _JetProgram(fn, [a[0] for a in atoms], e, {a[0]: a[1] for a in atoms})
            self._combo = dict(alpha=alpha, progs=new)
        except Exception as exc:   # any sympy corner case -> one stream per pair (never wrong, only slower)
            _note_fallback("combo_plan_errors", "combined second-order stream analysis failed (%r): one stream per pair" % (exc,))
            self._combo = None
        return self._combo

    def _compile_jet(self, expr):
        """Expand nested ``dif`` symbolically; returns a _JetProgram or None (not expressible with order<=2 jets)."""
        try:
            funcs = {v: sympy.Function(v.name)(*self.in_vars) for v in self.out_vars}
            e = expr.subs(funcs, simultaneous=True)
            dif = sympy.Function('dif')
            e = e.replace(lambda t: isinstance(t, AppliedUndef) and t.func == dif and len(t.args) == 2,
                          lambda t: sympy.Derivative(t.args[0], t.args[1]))
            # Abs, sign and Heaviside differentiate as the real functions torch's autograd sees (|f|' = sign(f) f', sign' = H' = 0):
            # sympy expands the derivative of an Abs whose argument is not known to be real into re / im terms
            real = e.has(sympy.Abs, sympy.sign)
            if real:
                e = e.replace(sympy.Abs, _RealAbs).replace(sympy.sign, _RealSign)
            e = e.doit()
            if real:
                e = e.replace(_RealAbs, sympy.Abs).replace(_RealSign, sympy.sign)
            if e.has(sympy.DiracDelta):
                e = e.replace(lambda t: isinstance(t, sympy.DiracDelta), lambda t: sympy.S.Zero)
            if e.has(dif) or e.has(sympy.Subs):
                return None
            fout = {f: i for i, f in enumerate(funcs.values())}
            ivar = {v: i for i, v in enumerate(self.in_vars)}
            atoms, repl = [], {}
            for dv in e.atoms(sympy.Derivative):
                if dv.expr not in fout:
                    return None
                mi = []
                for v, cnt in dv.variable_count:
                    if v not in ivar:
                        return None
                    mi += [ivar[v]] * int(cnt)
                if len(mi) > 2:
                    return None
                key = (fout[dv.expr], tuple(sorted(mi)))
                repl[dv] = sympy.Dummy("j%d_%s" % (key[0], "".join(map(str, key[1]))))
                atoms.append((key, repl[dv]))
            e = e.xreplace(repl)
            for f, i in fout.items():
                if e.has(f):
                    s = sympy.Dummy("j%d_" % i)
                    e = e.xreplace({f: s})
                    atoms.append(((i, ()), s))
            if e.atoms(AppliedUndef):
                return None
            atoms.sort(key=lambda a: (a[0][0], len(a[0][1]), a[0][1]))
            fn = _lambdify(list(self.in_vars) + list(self.param_vars) + [a[1] for a in atoms], e)
            return _JetProgram(fn, [a[0] for a in atoms], e, {a[0]: a[1] for a in atoms})
        except Exception as exc:  # any sympy corner case -> generic strategy (never wrong, only slower)
            _note_fallback("jet_compile_errors", "equation %s could not be expanded into jets (%r): reverse-sweep strategy"
                           % (expr, exc))
            return None

    # ------------------------------------------------------------------------------------------------
    def update_forward_method(self, forward_method):
        """forward_method: y = forward_method(x), x (..., n_in) -> y (..., n_out)."""
        self.forward_method = forward_method

    def update_parameters(self, values):
        """values: {name: tensor} for names of ``param_vars``; fp32 of shape [], [1] (one value for all points) or [B] (one
        per batch element of the query points [B, N, n_in]).  A value may require grad: the residuals are differentiable
        w.r.t. it on every strategy.  The tensors are kept, not copied: an in-place update is seen by the next call."""
        names = {s.name for s in self.param_vars}
        for name, t in values.items():
            if name not in names:
                raise ValueError('{} is not one of the declared param_vars ({})'.format(name, sorted(names)))
            if not (torch.is_tensor(t) and t.dtype == torch.float32):
                raise ValueError('parameter {} must be a float32 tensor'.format(name))
            if t.dim() > 1:
                raise ValueError('parameter {} has shape {}: expected [], [1] or [B]'.format(name, tuple(t.shape)))
        self.params.update(values)

    def _param_values(self, x):
        """The coefficient tensors in the order of param_vars, checked against the batch size of the query points x."""
        vals = []
        for s in self.param_vars:
            if s.name not in self.params:
                raise RuntimeError('parameter {} has not been set. Run update_parameters first.'.format(s.name))
            t = self.params[s.name]
            if t.numel() != 1 and t.shape[0] != x.shape[0]:
                raise ValueError('parameter {} has {} values, the query points have batch size {}'.format(
                    s.name, t.shape[0], x.shape[0]))
            vals.append(t)
        return vals

    def _param_broadcast(self, x):
        """[B, 1, ...] / [1, 1, ...] views of the coefficients, broadcastable against the columns of x."""
        return [t.reshape((-1,) + (1,) * (x.dim() - 1)) for t in self._param_values(x)]

    def eval(self, x):
        """Evaluate the output values using forward_method (reference :97-113)."""
        if not self.forward_method:
            raise RuntimeError('forward_method has not been defined.'
                               'Run update_forward_method first.')
        y = self.forward_method(x)
        if not ((x.shape[-1] == self.n_in) and (y.shape[-1] == self.n_out)):
            raise ValueError('Input/output dimensions ({}/{}) not equal to the dimensions of '
                             'defined variables ({}/{}).'.format(x.shape[-1], y.shape[-1], self.n_in, self.n_out))
        return y

    def _jet_request(self, x):
        if not (self.eqns_jet and all(p is not None for p in self.eqns_jet.values())):
            return None
        if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 3):
            return None
        nd = self.n_in in _lig.lig_jet.ND_JET_DIMS
        if nd:
            # 1- and 2-d problems (opt-in, ``lig_jet.nd_jets``): the HIP jets there serve forward passes that need no
            # gradient, so a request is made with grad mode off only -- with it on the forward would be evaluated for the
            # request, find it unserved and be evaluated again by the reverse sweeps -- unless their training backward is
            # switched on as well (``lig_jet.nd_jet_backward``)
            if not (_lig.lig_jet.nd_jets and (not torch.is_grad_enabled() or _lig.lig_jet.nd_jet_backward)):
                return None
        elif self.n_in == 4:
            # (t, x, y, z) problems (opt-in, ``lig_jet.nd4_jets``): forward passes that need no gradient only -- there is no
            # training backward through these derivatives, so grad mode on keeps the reverse sweeps
            if not _lig.lig_jet.nd4_jets or torch.is_grad_enabled():
                return None
        elif self.n_in != 3:
            return None
        if x.requires_grad and torch.is_grad_enabled():
            return None   # the caller wants autograd through the coordinates: only the generic strategy provides it
        # (the combined second-order stream is dim = 3 only: pairs everywhere else)
        plan = None if (nd or self.n_in == 4) else self._combo_plan()
        if plan is not None:
            return _lig.JetRequest(x, True, [], combo=plan["alpha"])
        first, pairs = False, set()
        for prog in self.eqns_jet.values():
            for _, mi in prog.atoms:
                if len(mi) == 1:
                    first = True
                elif len(mi) == 2:
                    pairs.add(mi)
        return _lig.JetRequest(x, first or bool(pairs), sorted(pairs))

    def _residues_from_jets(self, x, req):
        jets, pairs = req.jets, req.pairs_out
        shape = x.shape[:-1] + (1,)
        nfirst = 4 if self.n_in == 4 else 3     # first-order streams of the jets tensor (four inputs: 1 .. 4, pairs from 5)
        stream_of = {(): 0}
        for d in range(nfirst):
            stream_of[(d,)] = 1 + d
        progs = self.eqns_jet
        if pairs == ["combo"]:
            stream_of[("L",)] = 4
            progs = self._combo_plan()["progs"]
        else:
            for k, p in enumerate(pairs):
                stream_of.setdefault(tuple(p), 1 + nfirst + k)
        hip = self._residues_hip(x, jets, progs, stream_of, shape)
        if hip is not None:
            return hip
        if jets.is_cuda:
            _note_fallback("residual_torch_fallbacks", "an equation uses an expression the HIP residual evaluator does not "
                           "implement: residuals evaluated with the lambdified torch functions")
        cols = [x[..., i:i + 1] for i in range(self.n_in)] + [t.to(jets.device) for t in self._param_broadcast(x)]
        cache = {}

        def atom(key):
            if key not in cache:
                cache[key] = jets[stream_of[key[1]], key[0]].reshape(shape)
            return cache[key]

        return {name: prog.fn(*(cols + [atom(k) for k in prog.atoms])) for name, prog in progs.items()}

    def _coef_slots(self):
        """{coefficient symbol: k} for the device programs of a layer with ``device_params``; None when the layer has none to
        offer (the flag is off, or more coefficients than the kernels stage)."""
        if not (self.device_params and self.param_vars) or len(self.param_vars) > _lib.RES_MAX_COEF:
            return None
        return {s: k for k, s in enumerate(self.param_vars)}

    def _res_program(self, progs, stream_of, device):
        """The device program of these equations for this stream layout, compiled once and kept on ``device``: (program tensor,
        instructions, uses_x) or None when the device evaluator cannot take them; the coefficient indices it reads are kept
        beside it in ``_res_coefs``."""
        key = (tuple(sorted((str(k), v) for k, v in stream_of.items())), str(device))
        ent = self._res_progs.get(key, False)
        if ent is False:
            slots = {}
            for prog in progs.values():
                for akey, sym in prog.syms.items():
                    slots[sym] = (stream_of[akey[1]], akey[0])
            comp = _compile_residual_program([p.expr for p in progs.values()], list(self.in_vars), slots, extended=True,
                                             conditional=True, coef_slots=self._coef_slots())
            ent = None
            if comp is not None:
                arr, uses_x = comp[:2]
                ent = (torch.from_numpy(arr.view(np.uint8).copy()).to(device), len(arr), uses_x)
                self._res_coefs[key] = tuple(comp[2]) if len(comp) > 2 else ()
            self._res_progs[key] = ent
        return ent if ent is None else ent + (self._res_coefs[key],)

    def device_program_compiles(self, device="cpu"):
        """Whether the HIP residual evaluator takes this layer's equations, coefficients included (``device_params``), in the
        stream layout its own jet request asks for."""
        progs = self.eqns_jet
        if not (progs and all(p is not None and p.expr is not None for p in progs.values())):
            return False
        nfirst = 4 if self.n_in == 4 else 3
        stream_of = {(): 0}
        stream_of.update({(d,): 1 + d for d in range(nfirst)})
        plan = self._combo_plan() if self.n_in == 3 else None
        if plan is not None:
            stream_of[("L",)] = 4
            progs = plan["progs"]
        else:
            pairs = sorted({mi for p in progs.values() for _, mi in p.atoms if len(mi) == 2})
            for k, pr in enumerate(pairs):
                stream_of[pr] = 1 + nfirst + k
        ent = self._res_program(progs, stream_of, device)
        # (the evaluator addresses coordinates as [P][3]: a program on four inputs that names one is not taken)
        return ent is not None and not (self.n_in == 4 and ent[2])

    def _residues_hip(self, x, jets, progs, stream_of, shape):
        """All residuals of all equations in ONE HIP kernel (and one for the backward) instead of ~100 elementwise
        torch kernels; None when an equation uses something the device evaluator does not implement."""
        if not (jets.is_cuda and jets.dtype == torch.float32 and all(p.expr is not None for p in progs.values())):
            return None
        if self.param_vars and not (self.device_params and x.dim() == 3):
            return None     # coefficients in tensors: the device evaluator reads them for a layer with device_params only
        ent = self._res_program(progs, stream_of, jets.device)
        if ent is None:
            return None
        prog_t, nins, uses_x, ks = ent
        if uses_x and self.n_in > 3:
            return None     # the evaluator addresses coordinates as [P][3]: the lambdified functions do this layer's algebra
        coefs = []
        if ks:
            vals = self._param_values(x)
            coefs = [vals[k].to(jets.device) for k in ks]
            if not all(t.dtype == torch.float32 for t in coefs):
                return None
            coefs = [t.contiguous() for t in coefs]
        x2d = x.detach().reshape(-1, self.n_in).contiguous().float() if uses_x else None
        if x2d is not None and self.n_in < 3:      # the evaluator addresses x as [P][3]
            x2d = torch.nn.functional.pad(x2d, (0, 3 - self.n_in)).contiguous()
        if ks:      # (a declared coefficient that no equation uses is not handed over: its .grad stays None)
            res = _ResidualCoefHip.apply(jets, x2d, prog_t, nins, len(progs), x.shape[0], ks, *coefs)
        else:
            res = _ResidualHip.apply(jets, x2d, prog_t, nins, len(progs))
        return {name: res[k].reshape(shape) for k, name in enumerate(progs)}

    def __call__(self, x, return_residue=True):
        """y = forward(x) and, optionally, the residue of every equation (reference :115-143)."""
        if not return_residue:
            return self.eval(x)
        req = self._jet_request(x)
        if req is not None:
            with _lig.jet_context(req):
                y = self.eval(x)
            if req.jets is not None and req.y is y:
                return y, self._residues_from_jets(x, req)
        # generic strategy: split into columns that require grad, re-assemble, differentiate by reverse sweeps
        inputs = [x[..., i:i + 1] for i in range(x.shape[-1])]
        for xx in inputs:
            if not xx.requires_grad:
                xx.requires_grad = True
        x_ = torch.cat(inputs, axis=-1)
        y = self.eval(x_)
        outputs = [y[..., i:i + 1] for i in range(y.shape[-1])]
        inputs_outputs = inputs + outputs
        residues = {}
        inputs_outputs = inputs_outputs + self._param_broadcast(x)
        for key, fn in self.eqns_fn.items():
            residues.update({key: fn(*inputs_outputs)})
        return y, residues

    @property
    def eqn_num(self):
        return len(self.eqns_raw)

    @property
    def eqn_names(self):
        return list(self.eqns_raw.keys())
