"""The chunk buffers of the LIG jet path without a device: what the four chunk drivers of lig_jet allocate, what they hand to
the library in which pointer slot, and what the memory plan counts -- all three from one table (lig_jet._forward_buffers /
_backward_buffers / _dlatent_buffers / _two_phase_buffers).

The drivers run on CPU tensors against a library stub that records every entry point with its arguments and launches nothing,
with ``lig_jet.torch`` replaced by a proxy that records every ``empty`` / ``zeros``.  ``trace()`` knows nothing of the table:
the recording in tests/golden/lig_chunk_trace.json was made with it at the commit before the table existed, when every driver
still called torch.empty itself, and pins launches, scalar arguments, pointer slots and the order of the allocations (per case
the entry-point names and a digest of the whole record: ``_write_fixture``)."""
import ctypes as C
import hashlib
import itertools
import json
import os

import pytest
import torch

from space_time_pde_amd import _lib, lig_jet

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lig_chunk_trace.json")
COMBO = {(1, 1): 1.0, (2, 2): 0.25}
GRIDS = {1: (6,), 2: (5, 6), 3: (4, 5, 6), 4: (3, 4, 5, 6)}
CIN = {1: 32, 2: 32, 3: 32, 4: 31}        # (dim + cin + 1 <= 36: 31 is the widest latent of a 4-d grid)
# stream sets of the dim = 3 matrix: (first, pairs, combo) -> value only, (3, 0), (3, 1) with the combined stream, (3, 6)
STREAMS = {"value": (False, (), None), "first": (True, (), None), "combo": (True, (), COMBO),
           "six": (True, tuple(lig_jet.CANON_PAIRS), None)}
ND_PAIRS = {1: ((0, 0),), 2: ((0, 0), (0, 1), (1, 1))}
DEFAULTS = dict(deterministic_dlatent=True, value_tiles=True, tan0_rowsum=True, wgrad_split=True, packed_stash=True,
                fused_tail=True, use_pipeline=True, nd_backward=False, nd_jets=False, force_recompute=False, profile=None,
                memory_budget=None, sync_hooks=None, expect_two_phase=False)


def SORT_TMP_BYTES(n, nodes):
    """the stub's stpde_lig_sort_tmp_bytes"""
    return 1024 + 16 * n + 4 * nodes


def cases():
    """The matrix.  kind: "train" (forward with a stash, then the backward), "two_phase" (... with the d latent hook on the last
    chunk), "no_dlatent" (... for the weights alone), "fwd" (no gradient), "jets" (dim = 1, 2 derivative request, no gradient)."""
    out = []
    sw = list(itertools.product(("fp32", "bf16", "fp32x3"), (True, False), (True, False), (True, False), (True, False)))
    for prec, tan0, tail, det, pipe in sw:
        base = dict(precision=prec, tan0_rowsum=tan0, fused_tail=tail, deterministic_dlatent=det, use_pipeline=pipe)
        for streams in STREAMS:
            for kind in ("train", "two_phase", "no_dlatent"):
                out.append(dict(base, dim=3, streams=streams, kind=kind))
        for dim in (1, 2, 4):
            out.append(dict(base, dim=dim, streams="value", kind="fwd"))
            for kind in ("train", "two_phase", "no_dlatent"):
                out.append(dict(base, dim=dim, streams="value", kind=kind, nd_backward=True))
        for dim in (1, 2):
            for streams in ("first", "pairs"):
                out.append(dict(base, dim=dim, streams=streams, kind="jets", nd_jets=True))
    return out


def case_id(c):
    return "d%d-%s-%s-%s-rowsum%d-tail%d-det%d-pipe%d" % (c["dim"], c["kind"], c["streams"], c["precision"], c["tan0_rowsum"],
                                                         c["fused_tail"], c["deterministic_dlatent"], c["use_pipeline"])


def make_call(c, monkeypatch):
    """The call record of a case at the smallest legal size -- chunk = call.mult points, two chunks -- or None where
    JetCall.make refuses the combination (lig_jets' own refusals are kept out of the matrix by ``cases``)."""
    for name, default in DEFAULTS.items():
        monkeypatch.setattr(lig_jet, name, c.get(name, default))
    monkeypatch.setattr(_lib, "deterministic", False)
    monkeypatch.setenv("STPDE_FC1_FUSED", "1")
    monkeypatch.delenv("STPDE_S34", raising=False)
    dim = c["dim"]
    first, pairs, combo = (True, ND_PAIRS[dim], None) if c["streams"] == "pairs" else STREAMS[c["streams"]]
    plan = lig_jet.ImNetPlan.get(dim, CIN[dim], 4, 32)
    box = lig_jet.box_constants(GRIDS[dim], 0., 1.)
    need_grad = c["kind"] in ("train", "two_phase", "no_dlatent")
    try:
        mult = lig_jet.JetCall.make(plan, "softplus", 0.0, first, pairs, combo, c["precision"], GRIDS[dim], box).mult
        return lig_jet.JetCall.make(plan, "softplus", 0.0, first, pairs, combo, c["precision"], GRIDS[dim], box, None, 1,
                                    2 * mult, mult, need_grad)
    except NotImplementedError:
        return None


class _Recorder:
    """Library stub + torch proxy + pointer book of one case."""

    def __init__(self):
        self.on = False
        self.phase = None
        self.allocs = []        # (phase, numel, dtype name, first byte, bytes)
        self.keep = []          # every recorded tensor stays alive: no address is handed out twice
        self.inputs = []        # (name, first byte, bytes)
        self.calls = []         # [entry point, encoded arguments]

    # ---- torch proxy
    def __getattr__(self, name):
        return getattr(torch, name)

    def _made(self, t):
        if self.on:
            self.allocs.append((self.phase, t.numel(), str(t.dtype).split(".")[1], t.data_ptr(), t.numel() * t.element_size()))
            self.keep.append(t)
        return t

    def empty(self, *a, **kw):
        return self._made(torch.empty(*a, **kw))

    def zeros(self, *a, **kw):
        return self._made(torch.zeros(*a, **kw))

    # ---- pointers
    def add_input(self, name, t):
        self.inputs.append((name, t.data_ptr(), t.numel() * t.element_size()))
        return t

    def where(self, addr):
        if not addr:
            return "NULL"
        for k, (_, _, _, base, nbytes) in enumerate(self.allocs):
            if base <= addr < base + nbytes:
                return "alloc %d (%d B) + %d" % (k, nbytes, addr - base)
        for name, base, nbytes in self.inputs:
            if base <= addr < base + nbytes:
                return "input %s + %d" % (name, addr - base)
        raise AssertionError("pointer %#x is neither an input nor a recorded allocation" % addr)

    def encode(self, v):
        if v is None:
            return "NULL"
        if isinstance(v, C.c_void_p):
            return self.where(v.value)
        if isinstance(v, (bool, int, float)):
            return v
        if isinstance(v, C.Structure):
            out = {}
            for name, typ in v._fields_:
                x = getattr(v, name)
                if typ is C.c_void_p:
                    out[name] = self.where(x)
                elif issubclass(typ, C.Array):
                    out[name] = [self.where(e) for e in x] if typ._type_ is C.c_void_p else list(x)
                else:
                    out[name] = self.encode(x)
            return out
        if isinstance(v, C.Array):
            return [self.where(e) for e in v] if v._type_ is C.c_void_p else list(v)
        if hasattr(v, "_obj"):          # ctypes.byref(...)
            return self.encode(v._obj)
        raise AssertionError("argument of a type the recording does not know: %r" % (v,))

    # ---- library stub
    def entry(self, name):
        def call(*args):
            self.calls.append([name, [self.encode(a) for a in args]])
            if name == "stpde_jet_fc1_bwd_supported":
                return 1
            if name == "stpde_lig_sort_tmp_bytes":
                return SORT_TMP_BYTES(*args)
            return 0
        return call


class _Stub:
    def __init__(self, rec):
        self._rec = rec

    def __getattr__(self, name):
        return self._rec.entry(name)


_PACKS = {}


def _packs(plan, nsplit):
    """weight packs of a plan (zeros: only their addresses matter), made once per plan and operand mode"""
    key = (plan.dim, nsplit)
    if key not in _PACKS:
        params = []
        for lay in plan.layers:
            params += [torch.zeros(lay["M"], lay["Kin"]), torch.zeros(lay["M"])]
        packs = plan.pack(params)
        _PACKS[key] = (packs, plan.pack_bf16(packs, nsplit) if nsplit else None)
    return _PACKS[key]


def trace(c, monkeypatch):
    """Run the chunk drivers of a case: a forward without a stash over the first chunk, then -- a call that trains -- both
    chunks forward with a stash and backward, the last one with the d latent hook of the two-phase order where the case asks
    for it.  Returns (call, recorder), or None for a refused combination."""
    call = make_call(c, monkeypatch)
    if call is None:
        return None
    rec = _Recorder()
    plan, P = call.plan, call.B * call.N
    packs, packs16 = _packs(plan, call.nsplit if call.bf16 else 0)
    rec.add_input("packs", packs)
    for (l, name), t in sorted((packs16 or {}).items()):
        rec.add_input("packs16[%d, %s]" % (l, name), t)
    g = torch.Generator().manual_seed(1)
    latent = rec.add_input("latent", torch.rand(call.B, *call.grid_shape, plan.cin, generator=g))
    pts = rec.add_input("pts", torch.rand(P, plan.dim, generator=g))
    jets = rec.add_input("jets", torch.zeros(call.S_out, plan.cout, P))
    jets_bar = rec.add_input("jets_bar", torch.ones(call.S_out, plan.cout, P))
    train = c["kind"] in ("train", "two_phase", "no_dlatent")
    dw_flat = rec.add_input("dw_flat", torch.empty(lig_jet._AW(call) * plan.n_dw))
    dlatent = rec.add_input("dlatent", torch.zeros_like(latent)) if c["kind"] != "no_dlatent" else None
    pbar = rec.add_input("pbar", torch.zeros(_lib.PBAR_SLOTS))
    monkeypatch.setattr(lig_jet._lib, "lib", lambda: _Stub(rec))
    monkeypatch.setattr(lig_jet, "stream_ptr", lambda: None)
    monkeypatch.setattr(lig_jet, "torch", rec)
    rec.on = True
    chunks = lig_jet._chunk_ranges(call, P)
    assert chunks == [(0, call.mult), (call.mult, call.mult)]
    rec.phase = "forward, no stash"
    lig_jet._forward_chunk(call, packs, packs16, latent, pts[:call.mult], jets, 0, False)
    if train:
        saved = []
        for k, (p0, n) in enumerate(chunks):
            rec.phase = "forward %d" % k
            saved.append(lig_jet._forward_chunk(call, packs, packs16, latent, pts[p0:p0 + n], jets, p0, True))
        for k, s in enumerate(saved):
            rec.phase = "backward %d" % k
            hook = (lambda: rec.calls.append(["after_dlatent", []])) if (c["kind"] == "two_phase" and k == 1) else None
            lig_jet._backward_chunk(call, packs, packs16, s, jets_bar, dw_flat, dlatent, pbar, hook)
    rec.on = False
    monkeypatch.undo()
    return call, rec


def recording(rec):
    """The record of a case: the allocations in order and the calls.  -> (entry-point names, digest of the whole record)"""
    whole = json.dumps(dict(allocs=["%s: %d %s" % a[:3] for a in rec.allocs], calls=rec.calls), sort_keys=True)
    return [c[0] for c in rec.calls], hashlib.sha256(whole.encode()).hexdigest()[:16], whole


def _write_fixture():
    """Record every case with the drivers of the working tree.  The file is kept small: the entry-point names of a case are
    held readably (``names``, and ``sequences`` of their numbers), its whole record -- allocations, scalars, pointer slots --
    as a digest; records repeat from case to case, so each distinct one is held once and ``cases`` numbers them in the order
    of ``cases()``, -1 for a refused combination.  To see WHAT differs in a case, print its record at both commits:
    ``PYTHONPATH=. python tests/test_lig_chunk_buffers_host.py CASE_ID``."""
    mp = pytest.MonkeyPatch()
    names, seqs, records, order = {}, {}, {}, []
    for c in cases():
        got = trace(c, mp)
        if got is None:
            order.append(-1)
            continue
        seq, digest, _ = recording(got[1])
        k = seqs.setdefault(json.dumps([names.setdefault(n, len(names)) for n in seq]), len(seqs))
        order.append(records.setdefault((k, digest), len(records)))

    def rows(items, per):
        items = [json.dumps(x, separators=(",", ":")) for x in items]
        return "[\n  " + ",\n  ".join(", ".join(items[i:i + per]) for i in range(0, len(items), per)) + "\n ]"

    with open(FIXTURE, "w") as f:
        f.write('{\n "names": %s,\n "sequences": %s,\n "records": %s,\n "cases": %s\n}\n'
                % (rows(list(names), 4), rows([json.loads(q) for q in seqs], 1), rows([list(r) for r in records], 6),
                   rows(order, 32)))
    print("%d cases, %d records, %d sequences, %d bytes" % (len(order), len(records), len(seqs), os.path.getsize(FIXTURE)))


def load_fixture():
    """{case id: (entry-point names, digest)} of the recorded cases"""
    with open(FIXTURE) as f:
        fx = json.load(f)
    assert len(fx["cases"]) == len(cases())
    out = {}
    for c, r in zip(cases(), fx["cases"]):
        if r >= 0:
            k, digest = fx["records"][r]
            out[case_id(c)] = ([fx["names"][n] for n in fx["sequences"][k]], digest)
    return out


SWITCH_ROWS = sorted({case_id(c).split("-", 3)[3] for c in cases()})
_TRACES = {}


def traced(switches):
    """[(case, call, recorder)] of the cases under one setting of the switches that JetCall.make accepts, run once"""
    if switches not in _TRACES:
        rows = []
        for c in cases():
            if case_id(c).endswith("-" + switches):
                with pytest.MonkeyPatch.context() as mp:
                    got = trace(c, mp)
                rows.append((c, None, None) if got is None else (c,) + got)
        _TRACES[switches] = rows
    return _TRACES[switches]


@pytest.fixture(scope="module")
def parent_recording():
    return load_fixture()


@pytest.mark.parametrize("switches", SWITCH_ROWS)
def test_drivers_reproduce_the_recorded_allocations_and_launches(switches, parent_recording):
    """(a) the same allocations in the same order, the same entry points in the same order with the same scalars, and in every
    pointer slot the same input or allocation as in the recording."""
    seen = 0
    for c, call, rec in traced(switches):
        assert (call is None) == (case_id(c) not in parent_recording), case_id(c)
        if call is None:
            continue
        names, digest, _ = recording(rec)
        assert names == parent_recording[case_id(c)][0], case_id(c)
        assert digest == parent_recording[case_id(c)][1], "%s: an allocation, a scalar or a pointer slot differs" % case_id(c)
        seen += 1
    assert seen >= 8


def _sizes(table, skip=()):
    return sorted((n, str(dtype).split(".")[1]) for name, n, dtype in table if name not in skip)


def _nbytes(sizes):
    return sum(n * {"float32": 4, "int32": 4, "uint8": 1}[dt] for n, dt in sizes)


@pytest.mark.parametrize("switches", SWITCH_ROWS)
def test_tables_are_what_is_allocated_and_what_the_plan_counts(switches, monkeypatch):
    """(b) what the proxy saw a forward / backward chunk allocate is the chunk's table, no more and no less.  (c) the plan's
    bytes per point times the chunk's points are the bytes ALLOCATED for a whole-tile chunk, but for ``start`` (one int per
    grid node, not per point: never in the plan) and the sort's temporary storage (the plan's 24 B per point)."""
    monkeypatch.setattr(_lib, "lib", lambda: _Stub(_Recorder()))
    for c, call, rec in traced(switches):
        if call is None:
            continue
        cid, m = case_id(c), call.mult
        got = {ph: [] for ph in ("forward, no stash",) + (("forward 0", "forward 1", "backward 0", "backward 1")
                                                          if c["kind"] not in ("fwd", "jets") else ())}
        for phase, n, dt, _, _ in rec.allocs:
            got[phase].append((n, dt))
        got = {k: sorted(v) for k, v in got.items()}
        assert got.pop("forward, no stash") == _sizes(lig_jet._forward_buffers(call, m, False)), cid
        if c["kind"] in ("fwd", "jets"):
            assert not got, cid
            continue
        fwd = _sizes(lig_jet._forward_buffers(call, m, True))
        bwd = lig_jet._backward_buffers(call, m) + (lig_jet._dlatent_buffers(call, m) if c["kind"] != "no_dlatent" else [])
        # (the dgrad-first order is the one-call driver's, for the stream sets of the fused chain with tangent row sums)
        two = lig_jet._two_phase_buffers(call, m) if (c["kind"] == "two_phase" and call.pipeline and call.tail
                                                      and call.tan0_rowsum) else []
        assert got == {"forward 0": fwd, "forward 1": fwd, "backward 0": _sizes(bwd), "backward 1": _sizes(bwd + two)}, cid
        # ---- (c)
        plan_fwd, plan_bwd = lig_jet._per_point_bytes(call)
        assert plan_fwd * m == _nbytes(got["forward 0"]), cid
        assert lig_jet._two_phase_bytes(call) * m == _nbytes(_sizes(lig_jet._two_phase_buffers(call, m))), cid
        if two:
            assert lig_jet._two_phase_bytes(call) * m == _nbytes(got["backward 1"]) - _nbytes(got["backward 0"]), cid
        if c["kind"] == "train":
            scratch = lig_jet._dlatent_buffers(call, m)
            est = lig_jet.SORT_TMP_PLAN_BYTES * m if scratch else 0
            assert est == _nbytes(_sizes(lig_jet._dlatent_buffers(call, m, True), skip=("xrows", "perm", "start", "cell")))
            uncounted = _nbytes(_sizes([b for b in scratch if b[0] in ("start", "sort_tmp")]))
            assert plan_bwd * m == _nbytes(got["backward 0"]) - uncounted + est, cid
            if not call.tan0_rowsum and call.SP0 == 4:
                # the full layer-0 adjoint: 4 streams x 32 column tiles x 256 floats per row tile, 65,536 B per point
                full = call.SP0 * call.plan.layers[0]["MT"] * 256 * (m // 2)
                assert (full, "float32") in got["backward 0"] and plan_bwd >= 4 * full // m == 65536, cid


def _call(dim, prec="fp32", first=False, pairs=(), combo=None, need_grad=True):
    plan = lig_jet.ImNetPlan.get(dim, CIN[dim], 4, 32)
    return lig_jet.JetCall.make(plan, "softplus", 0.0, first, pairs, combo, prec, GRIDS[dim],
                                lig_jet.box_constants(GRIDS[dim], 0., 1.), chunk_points=1 << 20, need_grad=need_grad)


def test_plan_numbers_of_the_default_switches(monkeypatch):
    """The plan's figures for the reference width (ImNetPlan.get(dim, 32, 4, 32); dim = 4: 31 channels), softplus,
    chunk_points = 2^20, literally.  The forward figures and every figure of a call with gradient streams are those of the
    hand-written formulas this table replaced.  The backward figure of a VALUE-ONLY call (every dim = 1, 2, 4 call that
    trains) is smaller than theirs by the layer-0 tangent row sums -- 32 * 48 floats per row tile: 768 / 1536 / 3072 / 6144 B
    per point for dim = 1 / 2 / 3 / 4 -- which they counted and a call without tangent streams never allocates."""
    for name, default in DEFAULTS.items():
        monkeypatch.setattr(lig_jet, name, default)
    monkeypatch.setattr(_lib, "deterministic", False)
    both = {(1, 1): 1.0, (2, 2): 1.0}
    per, two = lig_jet._per_point_bytes, lig_jet._two_phase_bytes
    assert (per(_call(3, "fp32", True, (), both)), two(_call(3, "fp32", True, (), both))) == ((97380, 34844), 57344)
    assert (per(_call(3, "bf16", True, (), both)), two(_call(3, "bf16", True, (), both))) == ((66660, 50716), 0)
    assert per(_call(3)) == (33860, 10268 - 3072)
    monkeypatch.setattr(lig_jet, "_free_bytes", lambda device: 1 << 34)         # (16 GiB: the n-D default chunk is cut down)
    nd = {1: ((8456, 2592 - 768), 1 << 20), 2: ((16912, 5152 - 1536), 1 << 19), 4: ((67648, 20512 - 6144), 1 << 17)}
    for on in (False, True):
        monkeypatch.setattr(lig_jet, "nd_backward", on)
        for dim, (want, chunk) in nd.items():
            call = _call(dim, need_grad=on)
            assert (per(call), two(call)) == (want, 24576), (dim, on)
            # (a call that trains allocates z0 as well, 32 KiB per row tile on top of 34,880 B: half the chunk)
            assert lig_jet._nd_chunk_points(call, None) == (chunk // 2 if on else chunk), (dim, on)
    monkeypatch.setattr(lig_jet, "nd_jets", True)
    for dim, want, chunk in ((1, (28360, 10272), 1 << 18), (2, (56656, 20512), 1 << 17)):
        call = _call(dim, "fp32", True, ((0, 0),), need_grad=False)
        assert (per(call), two(call), lig_jet._nd_chunk_points(call, None)) == (want, 65536, chunk), dim


if __name__ == "__main__":
    import sys
    if len(sys.argv) > 1:       # the whole record of one case, to compare between two commits
        case = [c for c in cases() if case_id(c) == sys.argv[1]][0]
        print(json.dumps(json.loads(recording(trace(case, pytest.MonkeyPatch())[1])[2]), indent=1, sort_keys=True))
    else:
        _write_fixture()
