"""Host model of the residual evaluator and the loss kernels of csrc/residual.hip (k_residual_fwd, k_residual_bwd, k_loss_sum,
k_loss_grad), shared by tests/test_residual_program.py, tests/test_residual_model_host.py and tests/test_gpu_residual_ops.py.
Built once, shared, never modified.

``run(prog, jets, x, dtype)``                interprets an stpde_res_ins program (pde._RES_DT) for all points at once.  With
                                             dtype = float32 every instruction is the kernel's own IEEE operation in the kernel's
                                             order (POWI: the same square-and-multiply loop, 1 / r for negative exponents); with
                                             float64 it is the reference.
``adjoint(prog, jets, x, res_bar, dtype)``   the reverse sweep of k_residual_bwd, rule for rule in the same expression order
                                             (``(gi * v[i]) / v[b]`` for the divisor, ``(gi * 0.5) / v[i]`` for the square root,
                                             ``(gi * float(n)) * x^(n-1)`` for the integer power), every adjoint register starting
                                             at +0 and added into, like the kernel's.
``torch_program(prog, jets, x)``             the same program as a torch graph made of torch's own operators (``**``, ``/``,
                                             torch.sqrt, torch.abs, ...), so that torch.autograd differentiates it: the adjoint
                                             rules are checked against it, not against a second copy of themselves.

The library is built with -ffp-contract=off and without fast-math, and HIP's fp32 divide and square root are correctly rounded, so
the eleven opcodes JET X CONST ADD SUB MUL DIV NEG ABS SQRT OUT and POWI are fixed sequences of IEEE operations: the device must
reproduce the float32 model bit for bit (``same_bits``).  SIN COS EXP LOG TANH go through the device's math library; they are held
to the fp64 model in ulps (``ulp_err``) for values and in units of 2^-24 of the sum of the absolute values of the adjoint's terms
(``TRANS[name].terms``) for adjoints.

An OUT instruction is never an operand of a later one (pde._compile_residual_program memoises the operand, not the OUT), and the
kernel's adjoint of OUT ignores the OUT's own adjoint register; so does this model.

Losses: ``loss_elem`` / ``loss_grad`` are the expressions of the kernels in float32 (or float64: the reference), and
``loss_sum_bound`` is the relative bound the structure of k_loss_sum gives for a sum of non-negative terms.
"""
import numpy as np

F = np.float32
U = 2.0 ** -24
OPS = {"JET": 0, "X": 1, "CONST": 2, "ADD": 3, "SUB": 4, "MUL": 5, "DIV": 6, "NEG": 7, "POWI": 8, "SIN": 9, "COS": 10,
       "EXP": 11, "LOG": 12, "SQRT": 13, "TANH": 14, "ABS": 15, "OUT": 16}          # = pde._RES_OPS (asserted by the host tests)
NAMES = {v: k for k, v in OPS.items()}
DT = np.dtype([("op", "<i4"), ("a", "<i4"), ("b", "<i4"), ("c", "<f4")])             # = pde._RES_DT
_UNARY = {"SIN": np.sin, "COS": np.cos, "EXP": np.exp, "LOG": np.log, "SQRT": np.sqrt, "TANH": np.tanh, "ABS": np.abs}
EDGES = (0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan)


def program(*ins):
    """[(name, a, b, c) with trailing fields optional] -> a pde._RES_DT array."""
    rows = []
    for i in ins:
        i = tuple(i) + (0, 0, 0.0)[len(i) - 1:]
        rows.append((OPS[i[0]], int(i[1]), int(i[2]), float(i[3])))
    return np.array(rows, dtype=DT)


def _powi(base, n, dtype):
    """res_eval's STPDE_RES_POWI: square-and-multiply on |n|, then 1 / r when n < 0."""
    base = base.copy()
    r = np.ones_like(base)
    e = -n if n < 0 else n
    while e:
        if e & 1:
            r = r * base
        base = base * base
        e >>= 1
    return dtype(1) / r if n < 0 else r


def _values(prog, jets, x, dtype):
    jets = np.asarray(jets, dtype=dtype)
    x = None if x is None else np.asarray(x, dtype=dtype)
    P = jets.shape[2]
    v = []
    with np.errstate(all="ignore"):
        for op, a, b, c in prog.tolist():
            name = NAMES[op]
            if name == "JET":
                r = jets[a, b]
            elif name == "X":
                r = x[:, a]
            elif name == "CONST":
                r = np.full(P, F(c), dtype=dtype)        # the program holds fp32 constants
            elif name == "ADD":
                r = v[a] + v[b]
            elif name == "SUB":
                r = v[a] - v[b]
            elif name == "MUL":
                r = v[a] * v[b]
            elif name == "DIV":
                r = v[a] / v[b]
            elif name == "NEG":
                r = -v[a]
            elif name == "POWI":
                r = _powi(v[a], b, dtype)
            elif name == "OUT":
                r = v[a]
            else:
                r = _UNARY[name](v[a])
            assert r.dtype == dtype, (name, r.dtype)
            v.append(r)
    return v


def run(prog, jets, x, dtype=np.float64):
    """The residuals [n_eq] of P points: jets [S, n_out, P], x [P, 3] or None.  Returned in the order of the OUT indices."""
    v = _values(prog, jets, x, dtype)
    out = {int(b): v[i] for i, (op, a, b, c) in enumerate(prog.tolist()) if NAMES[op] == "OUT"}
    return [out[k] for k in sorted(out)]


def adjoint(prog, jets, x, res_bar, dtype=np.float64):
    """d (sum res * res_bar) / d jets, the sweep of k_residual_bwd: res_bar [n_eq, P] -> jets_bar [S, n_out, P]."""
    v = _values(prog, jets, x, dtype)
    res_bar = np.asarray(res_bar, dtype=dtype)
    P = np.shape(jets)[2]
    g = [np.zeros(P, dtype=dtype) for _ in v]
    jets_bar = np.zeros(np.shape(jets), dtype=dtype)
    half, one, zero = dtype(0.5), dtype(1), dtype(0)
    with np.errstate(all="ignore"):
        for i in range(len(v) - 1, -1, -1):
            op, a, b, c = prog[i].tolist()
            name, gi = NAMES[op], g[i]
            if name == "OUT":
                g[a] = g[a] + res_bar[b]
            elif name == "JET":
                jets_bar[a, b] = jets_bar[a, b] + gi
            elif name == "ADD":
                g[a] = g[a] + gi
                g[b] = g[b] + gi
            elif name == "SUB":
                g[a] = g[a] + gi
                g[b] = g[b] - gi
            elif name == "MUL":
                g[a] = g[a] + gi * v[b]
                g[b] = g[b] + gi * v[a]
            elif name == "DIV":
                g[a] = g[a] + gi / v[b]
                g[b] = g[b] - (gi * v[i]) / v[b]
            elif name == "NEG":
                g[a] = g[a] - gi
            elif name == "POWI":
                if b != 0:
                    g[a] = g[a] + (gi * dtype(b)) * _powi(v[a], b - 1, dtype)
            elif name == "SIN":
                g[a] = g[a] + gi * np.cos(v[a])
            elif name == "COS":
                g[a] = g[a] - gi * np.sin(v[a])
            elif name == "EXP":
                g[a] = g[a] + gi * v[i]
            elif name == "LOG":
                g[a] = g[a] + gi / v[a]
            elif name == "SQRT":
                g[a] = g[a] + (gi * half) / v[i]
            elif name == "TANH":
                g[a] = g[a] + gi * (one - v[i] * v[i])
            elif name == "ABS":
                g[a] = g[a] + np.where(v[a] > zero, gi, np.where(v[a] < zero, -gi, zero))
            # X, CONST: the coordinates are not differentiated on this path
    assert jets_bar.dtype == dtype
    return jets_bar


def torch_program(prog, jets, x):
    """The program as a torch graph over the tensor jets [S, n_out, P] (x [P, 3] or None) -> residuals [n_eq] of [P]."""
    import torch
    un = {"SIN": torch.sin, "COS": torch.cos, "EXP": torch.exp, "LOG": torch.log, "SQRT": torch.sqrt, "TANH": torch.tanh,
          "ABS": torch.abs}
    v, out = [], {}
    for op, a, b, c in prog.tolist():
        name = NAMES[op]
        if name == "JET":
            r = jets[a, b]
        elif name == "X":
            r = x[:, a]
        elif name == "CONST":
            r = torch.full((jets.shape[2],), float(F(c)), dtype=jets.dtype)
        elif name == "ADD":
            r = v[a] + v[b]
        elif name == "SUB":
            r = v[a] - v[b]
        elif name == "MUL":
            r = v[a] * v[b]
        elif name == "DIV":
            r = v[a] / v[b]
        elif name == "NEG":
            r = -v[a]
        elif name == "POWI":
            r = v[a] ** b
        elif name == "OUT":
            r = v[a]
            out[b] = r
        else:
            r = un[name](v[a])
        v.append(r)
    return [out[k] for k in sorted(out)]


# ---- comparisons ----------------------------------------------------------------------------------------------------------
def same_bits(got, want):
    """Element-wise: bit-equal where ``want`` is not NaN (this covers the finite values, the sign of a zero and the sign of an
    infinity), NaN exactly where ``want`` is NaN (the payload is not compared)."""
    got, want = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(want, dtype=F)
    nan = np.isnan(want)
    return np.where(nan, np.isnan(got), got.view(np.int32) == want.view(np.int32))


def bit_mismatches(got, want, limit=5):
    """Text for an assertion message: how many elements differ and the first few of them."""
    bad = np.argwhere(~same_bits(got, want))
    got, want = np.asarray(got), np.asarray(want)
    return "%d of %d differ; first: %s" % (len(bad), want.size, [(tuple(int(k) for k in i), float(got[tuple(i)]), float(want[tuple(i)]))
                                                                  for i in bad[:limit]])


def ulp_of(ref64):
    """The spacing of float32 at |ref64| (2^-149 at and below the subnormals)."""
    _, e = np.frexp(np.abs(np.asarray(ref64, dtype=np.float64)))
    return np.maximum(np.ldexp(1.0, e.astype(np.int64) - 24), 2.0 ** -149)


def units_err(got, ref64, unit):
    """|got - ref64| / unit element by element; 0 where both are the same infinity or both NaN, inf where only one is not
    finite, 0 where got == ref64 (so that a unit of 0 under an exact result does not matter)."""
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    fin = np.isfinite(got) & np.isfinite(ref64)
    with np.errstate(all="ignore"):
        err = np.where(got == ref64, 0.0, np.abs(got - ref64) / unit)
    same = (np.isnan(got) & np.isnan(ref64)) | (~fin & (got == ref64))
    return np.where(fin, err, np.where(same, 0.0, np.inf))


def ulp_err(got, ref64):
    """The error of a float32 result in float32 ulps of the fp64 reference, element by element."""
    return units_err(got, ref64, ulp_of(ref64))


# ---- input sweeps ---------------------------------------------------------------------------------------------------------
_cache = {}


def _frozen(key, make):
    if key not in _cache:
        a = make()
        a.setflags(write=False)
        _cache[key] = a
    return _cache[key]


def normal_operands(n=4096, seed=0):
    """n float32 values, random sign, magnitude log-uniform in [1e-3, 1e3]."""
    def make():
        rng = np.random.default_rng(1000 + seed)
        return (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3, 3, n)).astype(F)
    return _frozen(("normal", n, seed), make)


def unary_inputs(seed=0):
    """4096 normal-range values, then the seven edge values: [4103]."""
    return _frozen(("unary", seed), lambda: np.concatenate([normal_operands(4096, seed), np.array(EDGES, dtype=F)]))


def binary_inputs():
    """Two operands [4145]: 4096 independent normal-range pairs, then every pair of the seven edge values."""
    def make():
        e = np.array(EDGES, dtype=F)
        return np.stack([np.concatenate([normal_operands(4096, 0), np.repeat(e, 7)]),
                         np.concatenate([normal_operands(4096, 1), np.tile(e, 7)])])
    return _frozen(("binary",), make)


def cotangent(n, seed=7):
    return _frozen(("cot", n, seed), lambda: np.random.default_rng(2000 + seed).standard_normal(n).astype(F))


SWEEP_N = 32768


class _Trans:
    def __init__(self, lo, hi, fn, dfn, terms, log_uniform=False):
        self.lo, self.hi, self.fn, self.dfn, self.terms, self.log_uniform = lo, hi, fn, dfn, terms, log_uniform


# terms(x, g) = the fp64 sum of the absolute values of the terms of the adjoint expression of k_residual_bwd
TRANS = {
    "SIN": _Trans(-8.0, 8.0, np.sin, np.cos, lambda x, g: np.abs(g * np.cos(x))),
    "COS": _Trans(-8.0, 8.0, np.cos, lambda x: -np.sin(x), lambda x, g: np.abs(g * np.sin(x))),
    "EXP": _Trans(-20.0, 20.0, np.exp, np.exp, lambda x, g: np.abs(g * np.exp(x))),
    "LOG": _Trans(1e-3, 1e3, np.log, lambda x: 1.0 / x, lambda x, g: np.abs(g / x), log_uniform=True),
    "TANH": _Trans(-10.0, 10.0, np.tanh, lambda x: 1.0 - np.tanh(x) ** 2,
                   lambda x, g: np.abs(g) * (1.0 + np.tanh(x) ** 2)),          # g * (1 - t * t): the terms g and g t t
}


def sweep(name):
    """32,768 float32 arguments of a transcendental opcode: both ends of its interval (for tanh also +-0 and the first saturated
    arguments), then a seeded fill, uniform (log-uniform for log)."""
    def make():
        t = TRANS[name]
        head = [t.lo, t.hi]
        if name == "TANH":
            head += [0.0, -0.0, 9.0, -9.0, 9.5, -9.5, 1e-30, -1e-30, 1e-4, -1e-4]
        rng = np.random.default_rng(3000 + OPS[name])
        n = SWEEP_N - len(head)
        fill = np.exp(rng.uniform(np.log(t.lo), np.log(t.hi), n)) if t.log_uniform else rng.uniform(t.lo, t.hi, n)
        a = np.concatenate([np.array(head), fill]).astype(F)
        return np.clip(a, F(t.lo), F(t.hi)) if t.log_uniform else a
    return _frozen(("sweep", name), make)


def trans_reference(name):
    """(x32, cot32, value64, adjoint64, unit of the adjoint) of the sweep of one transcendental opcode: the fp64 model of the
    program JET, op, OUT and of its adjoint; unit = 2^-24 * terms."""
    x, g = sweep(name), cotangent(SWEEP_N, OPS[name])
    prog = program(("JET", 0, 0), (name, 0), ("OUT", 1, 0))
    val, = run(prog, x[None, None].astype(np.float64), None, np.float64)
    adj = adjoint(prog, x[None, None].astype(np.float64), None, g[None].astype(np.float64), np.float64)[0, 0]
    return x, g, val, adj, U * TRANS[name].terms(x.astype(np.float64), g.astype(np.float64))


def trans_yardstick(name):
    """The maximum error of torch's own float32 CPU evaluation of the opcode (value in ulps, autograd adjoint in adjoint units) on
    the same sweep against the same fp64 reference: (value, adjoint)."""
    import torch
    x, g, val, adj, unit = trans_reference(name)
    fn = {"SIN": torch.sin, "COS": torch.cos, "EXP": torch.exp, "LOG": torch.log, "TANH": torch.tanh}[name]
    xt = torch.from_numpy(np.array(x)).requires_grad_(True)
    y = fn(xt)
    y.backward(torch.from_numpy(np.array(g)))
    return float(ulp_err(y.detach().numpy(), val).max()), float(units_err(xt.grad.numpy(), adj, unit).max())


def trans_bound(yardstick):
    """What the device may reach: 4 x max(1, yardstick) -- the margin tests/act_jet_model.py gives a correctly rounded
    transcription."""
    return 4.0 * max(1.0, yardstick)


# ---- the all-opcode equation set ------------------------------------------------------------------------------------------
ALL_OPS_VARS = ("x, y, t", "c, u, v, w, p")
ALL_OPS_EQUATIONS = (
    ("exp(-u**2)*cos(v) - tanh(w)/(2 + sin(c))", "transcendental"),
    ("Abs(dif(u,x)) - log(1 + c**2)", "abs_log"),
    ("-dif(v,y) - dif(w,t)", "all_negative"),
    ("1/sqrt(2 + u**2) + p**-2 + x*dif(p,x)", "rsqrt_negpow"),
    ("-u", "neg"),
)


def all_ops_layer():
    from space_time_pde_amd import pde
    layer = pde.PDELayer(*ALL_OPS_VARS)
    for eq, name in ALL_OPS_EQUATIONS:
        layer.add_equation(eq, name)
    return layer


def all_ops_streams(layer):
    """{multi-index: stream} the way PDELayer._residues_from_jets numbers the streams."""
    req_pairs = sorted({mi for prog in layer.eqns_jet.values() for _, mi in prog.atoms if len(mi) == 2})
    stream_of = {(): 0, (0,): 1, (1,): 2, (2,): 3}
    for k, pr in enumerate(req_pairs):
        stream_of[pr] = 4 + k
    return stream_of


def all_ops_program(layer):
    """(program, uses_x, stream_of) of the layer's equations, compiled the way PDELayer._residues_hip compiles them."""
    from space_time_pde_amd import pde
    progs = layer.eqns_jet
    assert all(p is not None for p in progs.values())
    stream_of = all_ops_streams(layer)
    slots = {sym: (stream_of[k[1]], k[0]) for p in progs.values() for k, sym in p.syms.items()}
    comp = pde._compile_residual_program([p.expr for p in progs.values()], list(layer.in_vars), slots)
    assert comp is not None
    return comp[0], comp[1], stream_of


# ---- loss kernels ---------------------------------------------------------------------------------------------------------
LOSS_KINDS = ("l1", "l2", "huber")


def loss_diff(a, b, dtype=F):
    a = np.asarray(a, dtype=dtype)
    return a - (dtype(0) if b is None else np.asarray(b, dtype=dtype))


def loss_elem(kind, d):
    """loss_elem of csrc/residual.hip in the dtype of d."""
    t = d.dtype.type
    with np.errstate(all="ignore"):
        ad = np.abs(d)
        if kind == "l1":
            return ad
        if kind == "l2":
            return d * d
        return np.where(ad < t(1), t(0.5) * d * d, ad - t(0.5))


def loss_grad(kind, d, g):
    """k_loss_grad: g * f'(d) in the dtype of d.  f'(NaN) is 0 for l1 (torch's sign) and NaN for l2 and huber."""
    t = d.dtype.type
    with np.errstate(all="ignore"):
        if kind == "l1":
            f = np.where(d > t(0), t(1), np.where(d < t(0), t(-1), t(0)))
        elif kind == "l2":
            f = t(2) * d
        else:
            f = np.where(d >= t(1), t(1), np.where(d <= t(-1), t(-1), d))
        return t(g) * f


def loss_blocks(n, cap=1024):
    return min((n + 1023) // 1024, cap)


def loss_sum_bound(n, det):
    """Relative bound of k_loss_sum on a sum of non-negative terms: every thread chains ceil(n / (256 blocks)) additions, the wave
    and block tree adds 6 + 2 levels, and every block adds its sum with one fp32 atomic (blocks more roundings) -- or, in
    deterministic mode, exactly into the long accumulator, which is rounded to fp32 once."""
    blocks = loss_blocks(n)
    chain = -(-n // (256 * blocks))
    return (chain + 9) * U if det else (chain + 8 + blocks) * U


# ---- one small program per exact opcode -------------------------------------------------------------------------------------
POWI_EXPONENTS = (-3, -1, 0, 1, 2, 3, 7)
CONSTS = (0.1, -2.5, 0.0, -0.0, 1e-30, 3e38)
EXACT_CASES = ("JET", "X", "CONST", "ADD", "SUB", "MUL", "DIV", "NEG", "ABS", "SQRT", "OUT") + \
    tuple("POWI_%d" % n for n in POWI_EXPONENTS)
N_EDGE1, N_EDGE2 = len(EDGES), len(EDGES) ** 2


def edge_index(a, b=None):
    """The offset, from the end of unary_inputs() / binary_inputs(), of the edge row with operand a (and b): compare with
    ``is`` semantics for the two zeros and NaN."""
    def pos(v):
        for k, e in enumerate(EDGES):
            if (np.isnan(v) and np.isnan(e)) or (v == e and np.signbit(v) == np.signbit(e)):
                return k
        raise KeyError(v)
    return 4096 + (pos(a) if b is None else 7 * pos(a) + pos(b))


def exact_case(name):
    """(prog, jets [1, n_out, P] float32, x [P, 3] float32 or None, res_bar [n_eq, P] float32) of one exact opcode: 4096
    normal-range rows with a random cotangent, then the edge rows with cotangent 1."""
    def cot(n_eq, P, n_edge):
        c = np.array(cotangent(n_eq * P, 11).reshape(n_eq, P))
        c[:, P - n_edge:] = 1.0
        return c

    un, bi = unary_inputs(0), binary_inputs()
    x = None
    if name in ("ADD", "SUB", "MUL", "DIV"):
        prog = program(("JET", 0, 0), ("JET", 0, 1), (name, 0, 1), ("OUT", 2, 0), (name, 1, 1), ("OUT", 4, 1))
        jets, n_edge = bi[None], N_EDGE2
    elif name == "JET":
        prog = program(("JET", 0, 1), ("JET", 0, 0), ("OUT", 0, 0), ("OUT", 1, 1))
        jets, n_edge = bi[None], N_EDGE2
    elif name == "X":
        prog = program(("JET", 0, 0), ("X", 2), ("X", 0), ("X", 1), ("OUT", 1, 0), ("OUT", 2, 1), ("OUT", 3, 2))
        jets, n_edge = un[None, None], N_EDGE1
        x = np.ascontiguousarray(np.stack([unary_inputs(k) for k in (1, 2, 3)], 1))
    elif name == "CONST":
        ins = [("JET", 0, 0)] + [("CONST", 0, 0, c) for c in CONSTS] + [("OUT", 1 + k, k) for k in range(len(CONSTS))]
        prog = program(*ins)
        jets, n_edge = un[None, None], N_EDGE1
    elif name == "OUT":
        prog = program(("JET", 0, 0), ("OUT", 0, 1), ("OUT", 0, 0))
        jets, n_edge = un[None, None], N_EDGE1
    elif name.startswith("POWI_"):
        prog = program(("JET", 0, 0), ("POWI", 0, int(name[5:])), ("OUT", 1, 0))
        jets, n_edge = un[None, None], N_EDGE1
    else:
        prog = program(("JET", 0, 0), (name, 0), ("OUT", 1, 0))
        jets, n_edge = un[None, None], N_EDGE1
        if name == "SQRT":                      # positive normal-range arguments; the edge rows keep their signs
            jets = np.concatenate([np.abs(jets[..., :4096]), jets[..., 4096:]], -1)
    n_eq = int((prog["op"] == OPS["OUT"]).sum())
    P = jets.shape[2]
    return prog, np.ascontiguousarray(jets, dtype=F), x, cot(n_eq, P, n_edge)


def chain_program(nins=192):
    """A program of exactly nins exact-opcode instructions: two jets and a constant, then a chain that keeps its values in
    range (every round halves, takes a root and divides), an OUT every 37 instructions and at the end."""
    ins = [("JET", 0, 0), ("JET", 1, 0), ("CONST", 0, 0, 1.5)]
    t, k, n_eq = 0, 0, 0
    steps = [lambda t: ("ADD", t, 0), lambda t: ("MUL", t, 2), lambda t: ("SUB", t, 1), lambda t: ("ABS", t),
             lambda t: ("SQRT", t), lambda t: ("DIV", t, 2), lambda t: ("NEG", t), lambda t: ("POWI", t, 2),
             lambda t: ("ADD", t, 1), lambda t: ("POWI", t, -1), lambda t: ("MUL", t, 0), lambda t: ("POWI", t, 3),
             lambda t: ("ABS", t), lambda t: ("SQRT", t)]
    while len(ins) < nins - 1:
        if len(ins) % 37 == 36:
            ins.append(("OUT", t, n_eq))
            n_eq += 1
        else:
            ins.append(steps[k % len(steps)](t))
            t = len(ins) - 1
            k += 1
    ins.append(("OUT", t, n_eq))
    assert len(ins) == nins
    return program(*ins), n_eq + 1
