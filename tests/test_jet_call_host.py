"""The call record of the LIG jet path (lig_jet.JetCall) and the per-node deterministic mode of the U-Net, without a device:
every per-call switch is read once, when the call is made, and nothing a later stage computes from the record moves when the
switches do."""
import pytest
import torch

from space_time_pde_amd import _lib, lig_jet, unet3d

GRID = (4, 5, 6)
COMBO = {(1, 1): 1.0, (2, 2): 0.25}
# (module attribute, default); the environment switch and the process-wide deterministic mode are handled beside them
SWITCHES = [("deterministic_dlatent", True), ("value_tiles", True), ("tan0_rowsum", True), ("wgrad_split", True),
            ("packed_stash", True), ("fused_tail", True), ("use_pipeline", True), ("nd_backward", False), ("profile", None)]


def _make(precision="bf16", first=True, pairs=(), combo=COMBO, nf=32, act="softplus", **kw):
    plan = lig_jet.ImNetPlan.get(3, 32, 4, nf)
    return lig_jet.JetCall.make(plan, act, 0.0, first, pairs, combo, precision, GRID, lig_jet.box_constants(GRID, 0., 1.), **kw)


def _set_all(monkeypatch, flipped):
    """every switch at its default (flipped = False) or at the opposite"""
    for name, default in SWITCHES:
        if name == "profile":
            monkeypatch.setattr(lig_jet, name, {} if flipped else None)
        else:
            monkeypatch.setattr(lig_jet, name, default != flipped)
    monkeypatch.setenv("STPDE_FC1_FUSED", "0" if flipped else "1")
    monkeypatch.setattr(_lib, "deterministic", bool(flipped))


def _decisions(call):
    lay = call.plan.layers[2]
    return dict(flags=lig_jet._flags(call, True), flags_fwd=lig_jet._flags(call, False, False), aw=lig_jet._AW(call),
                det=lig_jet._layer_desc(call, 4, lay, call.cfg, False).det, per_point=lig_jet._per_point_bytes(call),
                two_phase=lig_jet._two_phase_bytes(call), tail=call.tail, split0=call.split0, pipeline=call.pipeline,
                dw1=lig_jet._dw_slice(call, torch.zeros(lig_jet._AW(call) * call.plan.n_dw), 1).numel())


@pytest.mark.parametrize("start_flipped", [False, True])
def test_switches_are_frozen_when_the_call_is_made(monkeypatch, start_flipped):
    """Sizes and flags only, no launch.  start_flipped = False is the direction "forward non-deterministic, backward
    deterministic": _AW, the descriptor's det and F_DET stay what the buffers of the call were sized for."""
    _set_all(monkeypatch, start_flipped)
    call = _make()
    before = _decisions(call)
    assert before["aw"] == (2 * _lib.DET_K if start_flipped else 1) and before["det"] == int(start_flipped)
    assert bool(before["flags"] & _lib.F_DET) == start_flipped
    assert call.packed_mask == (0 if start_flipped else 31)
    assert before["dw1"] == before["aw"] * call.plan.dw_off[1][1] * call.plan.dw_off[1][2]
    _set_all(monkeypatch, not start_flipped)
    assert _decisions(call) == before
    other = _decisions(_make())                 # (the switches do steer the NEXT call)
    for key in ("flags", "aw", "det", "per_point", "two_phase", "tail", "split0", "pipeline", "dw1"):
        assert other[key] != before[key], key
    with pytest.raises(AttributeError):         # frozen: no stage writes a field ...
        call.det = not call.det
    call.plan_chunk(4096)                       # ... but the memory plan, through its one method
    assert call.chunk == 4096


def test_flag_table(monkeypatch):
    """_flags for the default settings and for each single switch flipped, from the STPDE_F_* constants."""
    L = _lib
    base = L.F_STASH | L.F_VALUE_TILES | L.F_FUSED_TAIL | L.F_TAN0_ROWSUM | L.F_DETERMINISTIC | L.F_WGRAD
    assert base == 63 and (L.F_WGRAD_FP32, L.F_NO_FC1_FUSED, L.F_DET) == (64, 512, 1024)
    table = {"deterministic_dlatent": base & ~L.F_DETERMINISTIC, "value_tiles": base & ~L.F_VALUE_TILES,
             "tan0_rowsum": base & ~L.F_TAN0_ROWSUM, "wgrad_split": base | L.F_WGRAD_FP32, "packed_stash": base,
             "fused_tail": base & ~L.F_FUSED_TAIL, "use_pipeline": base, "nd_backward": base, "profile": base}
    _set_all(monkeypatch, False)
    call = _make("fp32")
    assert lig_jet._flags(call, True) == base
    assert lig_jet._flags(call, False) == base & ~L.F_STASH
    assert lig_jet._flags(call, True, False) == base & ~L.F_WGRAD
    for name, default in SWITCHES:
        _set_all(monkeypatch, False)
        monkeypatch.setattr(lig_jet, name, {} if name == "profile" else (not default))
        assert lig_jet._flags(_make("fp32"), True) == table[name], name
    _set_all(monkeypatch, False)
    monkeypatch.setenv("STPDE_FC1_FUSED", "0")
    assert lig_jet._flags(_make("fp32"), True) == base | L.F_NO_FC1_FUSED
    _set_all(monkeypatch, False)
    monkeypatch.setattr(_lib, "deterministic", True)
    assert lig_jet._flags(_make("fp32"), True) == base | L.F_DET


# (S1, S2, combined second-order stream) -> the fused fc3 -> fc5 kernels serve the stream set, at nf = 16 / 32 with the switch on
TAIL_TABLE = {(0, 0, False): True, (3, 0, False): True, (3, 1, True): True, (3, 1, False): False, (3, 2, False): True,
              (3, 4, False): True, (3, 6, False): False}


def test_tail_predicate_table(monkeypatch):
    """ONE predicate for what used to be spelled four times: the per-kernel forward (with its value-tile variant) and backward,
    the two-phase order of the one-call backward (which adds ``tan0_rowsum`` and SP0 in (1, 4) -- true of every served set) and
    the packed-buffer decision (which adds S1 == 3)."""
    assert set((a, b) for a, b, _ in TAIL_TABLE) == set(lig_jet.TAIL_SETS) | {(3, 6)}
    for nf in (16, 32, 48):
        for fused in (True, False):
            for (s1, s2, combo), served in TAIL_TABLE.items():
                cfg = _lib.JetCfg()
                cfg.S1, cfg.S2, cfg.combo = s1, s2, int(combo)
                want = served and fused and nf in (16, 32)
                assert lig_jet._tail_applies(fused, nf, cfg, int(combo)) is want, (nf, fused, s1, s2, combo)
                assert (1 + s1 in (1, 4)) or not want
                # the value-tile pass of a forward-only value query: every stream set of such a call
                assert lig_jet._tail_applies(fused, nf, cfg, int(combo), True) is (fused and nf in (16, 32))
    # the record, for every request make_cfg can produce: (first, pairs, combo) -> (S1, S2).  NOT the whole table: make_cfg
    # never yields S2 == 1 without a combined stream, so (3, 1, False) is checked through _tail_applies alone, above.
    requests = {(0, 0, False): (False, (), None), (3, 0, False): (True, (), None), (3, 1, True): (True, (), COMBO),
                (3, 2, False): (True, [(0, 0), (1, 1)], None), (3, 4, False): (True, [(0, 0), (1, 1), (2, 2), (1, 2)], None),
                (3, 6, False): (True, lig_jet.CANON_PAIRS, None)}
    for nf in (16, 32, 48):
        for fused in (True, False):
            for rowsum in (True, False):
                _set_all(monkeypatch, False)
                monkeypatch.setattr(lig_jet, "fused_tail", fused)
                monkeypatch.setattr(lig_jet, "tan0_rowsum", rowsum)
                for (s1, s2, combo), (first, pairs, cmb) in requests.items():
                    call = _make("bf16", first, pairs, cmb, nf)
                    assert (call.cfg.S1, call.cfg.S2, bool(call.cfg_out.combo)) == (s1, s2, combo)
                    want = TAIL_TABLE[(s1, s2, combo)] and fused and nf in (16, 32)
                    assert call.tail is want
                    assert (call.SP0, call.split0) == (1 + s1, s1 == 3 and rowsum)
                    packed = want and nf == 32 and s1 == 3 and call.S <= 6 and rowsum
                    assert call.packed_mask == (31 if packed else 0), (nf, fused, rowsum, s1, s2)
    # a piecewise-linear activation carries (3, 0) through the network whatever second derivatives are asked for
    _set_all(monkeypatch, False)
    call = _make("fp32", True, lig_jet.CANON_PAIRS, None, act="leakyrelu")
    assert (call.cfg.S1, call.cfg.S2, call.cfg_out.S2) == (3, 0, 6) and call.tail


@pytest.mark.parametrize("flag", [False, True])
def test_unet_accumulators_are_sized_by_the_mode_they_are_given(monkeypatch, flag):
    monkeypatch.setattr(_lib, "deterministic", flag)
    assert unet3d._acc_zeros(7, device="cpu", det=0).numel() == 7
    assert unet3d._acc_zeros(7, device="cpu", det=1).numel() == 7 * 2 * _lib.DET_K
    acc = unet3d._acc_zeros(7, device="cpu", det=0)
    assert unet3d._acc_value(acc, 7, 0) is acc
    x = torch.zeros(1, 2, 2, 2, 16)
    assert unet3d._desc(x, 16, 16, 1, 0, 0).det == 0 and unet3d._desc(x, 16, 16, 1, 0, 1).det == 1
    assert unet3d._desc(x, 16, 16, 1).det == int(flag)        # (no mode given: the caller's own forward-time reading)


@pytest.mark.parametrize("flag", [False, True])
def test_unet_step_record_carries_the_step_and_leaves_the_modules_alone(monkeypatch, flag):
    """UNet3d._prepare_step returns the per-forward record (unet3d._UNetStep): one reading of the mode, the _ConvStep of every
    convolution (same packs as the stand-alone constructor, disjoint slices that tile the step's gradient buffer), each
    BatchNorm's scratch handed out once -- and no ``_stpde*`` attribute on any module, after it or after a forward."""
    monkeypatch.setattr(_lib, "deterministic", flag)
    torch.manual_seed(0)
    net = unet3d.UNet3d(in_features=4, out_features=32, igres=(4, 16, 16), nf=16, mf=64).train()
    cpu, det = torch.device("cpu"), int(flag)
    step = net._prepare_step(cpu)
    monkeypatch.setattr(_lib, "deterministic", not flag)          # (what the step read is what it keeps)
    convs = [m for m in net.modules() if isinstance(m, torch.nn.Conv3d)]
    assert step.det == det and len(convs) == 40 and set(step.convs) == set(convs)
    spans = []
    for conv in convs:
        cs, alone = step.convs[conv], unet3d._ConvStep.alone(conv.weight, cpu, det)
        assert torch.equal(cs.fpack, alone.fpack) and torch.equal(cs.bpack, alone.bpack)
        assert cs.det == det and cs.defer is None and (alone.dw, alone.defer) == (None, None)
        co, ci, k = conv.weight.shape[:3]
        assert cs.dw.numel() == unet3d._acc_w(det) * k ** 3 * co * ((ci + 15) // 16 * 16)
        assert cs.dw.is_contiguous() and not cs.dw.any()
        spans.append((cs.dw.storage_offset(), cs.dw.storage_offset() + cs.dw.numel()))
    spans.sort()
    total = step.convs[convs[0]].dw.untyped_storage().nbytes() // 4
    assert spans[0][0] == 0 and spans[-1][1] == total == unet3d._acc_w(det) * 451072
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))    # pairwise disjoint, and together the whole buffer
    assert len({cs.dw.untyped_storage().data_ptr() for cs in step.convs.values()}) == 1
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm3d)]
    assert step.counted and all(int(bn.num_batches_tracked) == 1 for bn in bns)
    for bn in bns:
        sc = step.take_scratch(bn)
        assert sc.numel() == 6 * _lib.BN_REP * bn.num_features and not sc.any()
        assert step.take_scratch(bn) is None                      # once per BatchNorm and step: then "bring your own"

    def stray():
        return [(name, a) for name, m in net.named_modules() for a in vars(m) if a.startswith("_stpde")]

    assert stray() == []
    net(torch.randn(2, 4, 4, 16, 16))
    assert stray() == []
