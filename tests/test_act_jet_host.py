"""Host side of the element-wise activation-jet tests (tests/act_jet_model.py; the GPU side is tests/test_gpu_act_jets.py): the
bounds leave the fp32 model a margin of 4, the fp64 oracle agrees with torch's own activations differentiated three times, and
the bounds are tight enough to see a relative change of 2^-14 in any single derivative, a halved softplus threshold and a halved
log1p seam."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from oracle.jet_ref import act_derivs
from tests import act_jet_model as A


def test_sweep_is_what_the_bounds_were_measured_on():
    a = A.sweep()
    assert a.shape == (256, 128) and a.dtype == np.float32 and np.isfinite(a).all()
    flat = a.reshape(-1)
    assert flat[0] == 0 and flat[1] == 0 and not np.signbit(flat[0]) and np.signbit(flat[1])
    assert np.count_nonzero(flat == 0) == 2                      # nothing else on the kink of ReLU / LeakyReLU / ELU
    for v in (np.nextafter(np.float32(20), np.float32(0)), 20.0, np.nextafter(np.float32(20), np.float32(40)), 6.93, 6.94, 87.3,
              88.8, 104.0, 1e4, 1e-30, np.nextafter(np.float32(2.0 ** -10), np.float32(0))):
        assert (flat[:64] == np.float32(v)).any() and (flat[:64] == -np.float32(v)).any(), v
    # both sides of every branch of common.h are populated: series / log of log1p, the softplus select, exp underflow
    e = np.exp(-np.abs(flat.astype(np.float64)))
    assert (e < 2.0 ** -10).sum() > 1000 and ((e >= 2.0 ** -10) & (e < 2.0 ** -9)).sum() > 100
    assert (flat > 20).sum() > 1000 and (np.abs(flat) > 104).sum() > 100 and (np.abs(flat) < 1e-2).sum() > 3000


@pytest.mark.parametrize("act", A.ACTS)
def test_model_stays_within_a_quarter_of_every_bound(act):
    mx = A.model_maxima(act)
    for direction in ("fwd", "adj"):
        for order in range(3):
            assert mx[direction][order] <= A.BOUNDS[act][direction][order] / 4.0, (act, direction, order, mx)
    if act == "swish":
        for S1, S2 in A.ADJ_SETS:
            assert A.model_dbeta_units(S1, S2) <= A.DBETA_BOUND / 4.0, (S1, S2)


def _torch_act(act, beta):
    return {"softplus": Fn.softplus, "tanh": torch.tanh, "elu": Fn.elu, "swish": lambda x: x * torch.sigmoid(beta * x),
            "relu": Fn.relu, "leakyrelu": Fn.leaky_relu}[act]


@pytest.mark.parametrize("act", A.ACTS)
def test_oracle_matches_three_nested_autograd_sweeps_of_torch(act):
    """act_derivs against torch.autograd.grad applied three times to torch's own activation, fp64, on the sweep.  Both are fp64
    evaluations of the same functions, so they may differ by fp64 rounding amplified by cancellation only: 1e-11 of the natural
    scale of each derivative is 1/6000 of the unit the fp32 kernels are judged in."""
    beta = torch.tensor(float(A.BETA), dtype=torch.float64)
    x = torch.from_numpy(np.array(A.sweep())).double().requires_grad_(True)
    ref = [_torch_act(act, beta)(x)]
    for _ in range(3):
        y = ref[-1]
        g = torch.autograd.grad(y.sum(), x, create_graph=True, allow_unused=True)[0] if y.requires_grad else None
        ref.append(torch.zeros_like(x) if g is None else g)
    got = act_derivs(act, x.detach(), beta)
    a = x.detach()
    b = float(A.BETA) if act == "swish" else 1.0
    scales = [1 + a.abs(), torch.ones_like(a), b * torch.ones_like(a), b * b * torch.ones_like(a)]
    for k in range(4):
        keep = torch.ones_like(a, dtype=torch.bool)
        if k >= 2 and act in ("relu", "leakyrelu", "elu"):
            keep = a != 0
        err = (got[k] - ref[k].detach()).abs() / scales[k]
        if k >= 2 and act == "softplus":
            # torch's softplus switches to the identity for x > 20, its double backward keeps s (1 - s) only for x < 20: at
            # exactly 20 torch's slope is still the sigmoid and its derivative is already 0.  The oracle (and the kernels) are
            # consistent there, s (1 - s) = e^-20 = 2.1e-9, 1/29 of a unit; every other point is held to the 1e-11
            assert int((a == 20).sum()) == 1 and err[a == 20].max().item() <= 2.1e-9, (act, k)
            keep = a != 20
        assert err[keep].max().item() <= 1e-11, (act, k, err[keep].max().item())
    if act in ("relu", "leakyrelu", "elu"):           # torch's conventions at +-0, which the kernels follow
        slope = {"relu": 0.0, "leakyrelu": 0.01, "elu": 1.0}[act]
        assert (ref[1].detach()[a == 0] == slope).all() and (got[1][a == 0] == slope).all()


def _violates(act, mx):
    return any(mx[d][o] > A.BOUNDS[act][d][o] for d in ("fwd", "adj") for o in range(3))


@pytest.mark.parametrize("act", A.ACTS)
def test_bounds_see_a_2_pow_minus_14_change_of_any_single_derivative(act):
    s = A.model_fp32(act, A.sweep())
    for k in range(4):
        if not np.any(s[k]):
            assert act in ("relu", "leakyrelu") and k >= 2       # identically zero: nothing to scale
            continue
        scale = [1.0] * 4
        scale[k] = 1.0 + 2.0 ** -14
        assert _violates(act, A.model_maxima(act, scale=tuple(scale))), (act, k)
    assert not _violates(act, A.model_maxima(act))


def test_bounds_see_a_halved_softplus_threshold_and_a_halved_log1p_seam():
    """Down is the direction that can be wrong (see tests/act_jet_model.py): threshold 10 returns slope 1 where sigmoid is
    1 - 4.5e-5; seam 2^-11 takes log(fl(1 + e)) where it has lost half of its bits."""
    assert _violates("softplus", A.model_maxima("softplus", threshold=10.0))
    mx = A.model_maxima("softplus", seam=2.0 ** -11)
    assert mx["fwd"][0] > A.BOUNDS["softplus"]["fwd"][0], mx
