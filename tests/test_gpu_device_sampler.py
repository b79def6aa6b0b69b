"""dataloader_spacetime.DeviceBatchSampler on the GPU (csrc/sampler.hip): explicit batches are bit-identical to
RB2DeviceLoader.get(), drawn batches equal the host model of the generator, the draw is capturable, and GraphedStep(sampler=...)
trains every replay on the batch the host model predicts.

Geometry: dataset [4, 12, 20, 24] (all extents distinct, so a swapped axis shows), crop (nt, nz, nx) = (8, 16, 16), downsamp_t = 2,
downsamp_xz = 4 -> low-res (4, 4, 4), ranges (5, 5, 9), len = 225; B = 3, N = 67, so B * N * 3 = 603 coordinates leave a ragged
last Philox call.  The second geometry has downsamp_t = 1 (the last low-res t tap is i0 = n - 2, w = 1) and nz = Z (range 1)."""
import numpy as np
import pytest
import torch

from space_time_pde_amd import dataloader_spacetime as dl

B, N = 3, 67
GEOMS = {"base": dict(nt=8, nz=16, nx=16, downsamp_t=2, downsamp_xz=4), "edge": dict(nt=8, nz=20, nx=16, downsamp_t=1, downsamp_xz=4)}
IDS = {"base": [0, 224, 113], "edge": [0, 44, 22]}       # first, last (= the far corner of the dataset), middle


@pytest.fixture(scope="module")
def dataset():
    return torch.randn(4, 12, 20, 24, generator=torch.Generator().manual_seed(5))


_loaders = {}


def _loader(dataset, geom="base", interp="linear", normalize=False):
    key = (geom, interp, normalize)
    if key not in _loaders:
        _loaders[key] = dl.RB2DeviceLoader(dataset, n_samp_pts_per_crop=N, normalize_output=normalize, device="cuda:0",
                                           lres_interp=interp, **GEOMS[geom])
    return _loaders[key]


def _points(geom):
    """[B, N, 3] in [0, 1): random, with the first 40 rows of every crop replaced by the cases that matter -- exactly 0, the two
    largest fp32 values below 1, and every multiple of 0.5 / (n - 1) (the nodes, and the mid-points where nearest mode ties)."""
    g = GEOMS[geom]
    pc = torch.rand(B, N, 3, generator=torch.Generator().manual_seed(6))
    for k, n in enumerate((g["nt"], g["nz"], g["nx"])):
        special = [0.0, float(np.float32(1.0) - np.float32(2.0 ** -24)), float(np.float32(1.0 - 1e-7))]
        special += [float(np.float32(j * 0.5 / (n - 1))) for j in range(2 * (n - 1))]
        for b in range(B):
            for r in range(40):
                pc[b, r, k] = special[(r + 5 * b + 3 * k) % len(special)]
    assert float(pc.min()) == 0.0 and 1.0 - 1e-7 <= float(pc.max()) < 1.0
    return pc


def _same(got, want):
    for name, a, b in zip(("lres", "point_coord", "point_value"), got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, name
        assert torch.equal(a, b), "%s: %d of %d elements differ, max |diff| %.3e" % (
            name, int((a != b).sum()), a.numel(), float((a - b).abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("geom", ["base", "edge"])
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("interp", ["linear", "nearest"])
def test_explicit_batches_equal_the_loader_bit_for_bit(hiplib, dataset, geom, interp, normalize):
    ld = _loader(dataset, geom, interp, normalize)
    assert len(ld) == {"base": 225, "edge": 45}[geom]
    s = dl.DeviceBatchSampler(ld, B, seed=1)
    pc = _points(geom).cuda()
    want = ld.get(IDS[geom], point_coord=pc)
    assert all(bool(torch.isfinite(t).all()) for t in want)
    got = s.produce(IDS[geom], pc)
    torch.cuda.synchronize()
    assert got[0].data_ptr() == s.lres.data_ptr() and got[2].data_ptr() == s.point_value.data_ptr()
    _same(got, want)
    s.check()                                                        # nothing was clamped
    assert s.offset() == 0                                           # explicit mode does not move the generator
    with pytest.raises(IndexError):
        s.produce([0, len(ld), 1], pc)                               # a host list is range-checked before any launch
    with pytest.raises(ValueError):
        s.produce(IDS[geom][:2], pc)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,offset", [(0, 0), (0x9E3779B97F4A7C15, 12345), (3, 2 ** 32 - 1)])
def test_drawn_batches_equal_the_host_model(hiplib, dataset, seed, offset):
    ld = _loader(dataset, "base", "linear", True)
    s = dl.DeviceBatchSampler(ld, B, seed=0)
    s.seed(seed, offset)
    for k in range(2):                                               # (the second draw from 2^32 - 1 carries into offset_hi)
        assert s.offset() == offset + k
        out = [t.clone() for t in s.draw()]
        ids, pc = s.expected(offset + k)
        assert torch.equal(s.crop_idx.cpu(), ids), (s.crop_idx.tolist(), ids.tolist())
        assert torch.equal(out[1].cpu(), pc)
        assert 0 <= int(ids.min()) and int(ids.max()) < 225 and 0.0 <= float(pc.min()) and float(pc.max()) < 1.0
        _same(out, ld.get(ids.tolist(), point_coord=pc.cuda()))
    assert s.offset() == offset + 2
    s.check()


@pytest.mark.gpu
def test_out_of_range_device_ids_are_clamped_and_counted(hiplib, dataset):
    ld = _loader(dataset, "base", "linear", False)
    s = dl.DeviceBatchSampler(ld, B)
    pc = _points("base").cuda()
    got = s.produce(torch.tensor([-1, 225, 7], device="cuda:0"), pc)
    _same(got, ld.get([0, 224, 7], point_coord=pc))
    assert s.oob_count() == 2
    with pytest.raises(IndexError) as e:
        s.check()
    assert "2 crop id" in str(e.value)
    s.seed(0)                                                        # a restart clears the count
    s.check()


@pytest.mark.gpu
def test_state_dict_resumes_and_seed_restarts_the_sequence(hiplib, dataset):
    ld = _loader(dataset, "base", "linear", True)
    s = dl.DeviceBatchSampler(ld, B, seed=99)
    s.draw()
    s.draw()
    sd = s.state_dict()
    assert sd == {"seed": 99, "offset": 2}
    t = dl.DeviceBatchSampler(ld, B, seed=0)
    t.load_state_dict(sd)
    for k in (2, 3):
        a, b = [x.clone() for x in s.draw()], [x.clone() for x in t.draw()]
        _same(a, b)
        assert torch.equal(s.crop_idx, t.crop_idx) and torch.equal(a[1].cpu(), s.expected(k)[1])
    s.seed(99)
    s.draw()
    assert s.offset() == 1 and torch.equal(s.point_coord.cpu(), t.expected(0)[1]) and torch.equal(s.crop_idx.cpu(), t.expected(0)[0])


@pytest.mark.gpu
def test_a_captured_draw_advances_with_every_replay(hiplib, dataset):
    ld = _loader(dataset, "base", "linear", True)
    s, twin = dl.DeviceBatchSampler(ld, B, seed=21), dl.DeviceBatchSampler(ld, B, seed=21)
    s.draw()                                                         # eager warm-up: kernels loaded before the capture
    twin.draw()
    torch.cuda.synchronize()
    o = s.offset()
    assert o == 1
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.draw()
    assert s.offset() == o                                           # a capture executes nothing
    seen = []
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        ids, pc = s.expected(o + k)
        assert torch.equal(s.crop_idx.cpu(), ids) and torch.equal(s.point_coord.cpu(), pc)
        _same((s.lres, s.point_coord, s.point_value), [x.clone() for x in twin.draw()])
        assert torch.equal(s.crop_idx, twin.crop_idx)
        seen.append(s.point_coord.clone())
    assert s.offset() == o + 3
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2]) and not torch.equal(seen[0], seen[2])


@pytest.mark.gpu
def test_graphed_step_draws_its_own_batches(hiplib):
    """The small regime of test_graphed_step_replays_the_eager_step (U-Net to a (4, 16, 16) latent grid, IM-NET nf = 32, RB2 +
    continuity, no optimizer) over a loader whose crops down-sample to that size: every replay trains on the batch the host model
    predicts for offset0 + k (the warm-up consumed nothing), and its losses are the eager step's on that batch to 1e-5."""
    from space_time_pde_amd import implicit_net, local_implicit_grid as lig, physics, unet3d
    from space_time_pde_amd.train_step import GraphedStep, sharded_step
    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    nb, npts = 4, 512
    data = torch.randn(4, 10, 36, 40, generator=torch.Generator().manual_seed(13))
    ld = dl.RB2DeviceLoader(data, nx=32, nz=32, nt=8, n_samp_pts_per_crop=npts, downsamp_xz=2, downsamp_t=2,
                            normalize_output=True, device=dev)
    s = dl.DeviceBatchSampler(ld, nb, seed=5)
    s.seed(5, offset=7)
    assert tuple(s.lres.shape) == (nb, 4, 4, 16, 16)
    unet = unet3d.UNet3d(in_features=4, out_features=32, igres=(4, 16, 16), nf=16, mf=256).to(dev).train()
    net = implicit_net.ImNet(dim=3, in_features=32, out_features=4, nf=32, activation=torch.nn.Softplus).to(dev)
    layer = physics.get_rb2_pde_layer(mean=(0.01, 0, 0.02, -0.01), std=(0.05, 0.3, 0.15, 0.12), t_crop=2., z_crop=1.,
                                      x_crop=1., use_continuity=True)
    params = list(unet.parameters()) + list(net.parameters())
    with pytest.raises(ValueError):
        GraphedStep(unet, net, layer, s.lres, None, None, npts, 1.0, 0.0125, "l1", sampler=s)
    n0 = lig.stats["hip_jet_calls"]
    gstep = GraphedStep(unet, net, layer, None, None, None, npts, 1.0, 0.0125, "l1", sampler=s)
    assert lig.stats["hip_jet_calls"] > n0                           # the HIP jet path is what was captured
    assert s.offset() == 7                                           # construction consumed no draw
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(gstep.static, (s.lres, s.point_coord, s.point_value)))
    with pytest.raises(ValueError):
        gstep(s.lres)
    for k in range(3):
        out = gstep()
        torch.cuda.synchronize()
        got = [float(v) for v in out]
        crop, pts, tgt = [t.clone() for t in gstep.static]
        ids, pc = s.expected(7 + k)
        assert torch.equal(s.crop_idx.cpu(), ids) and torch.equal(pts.cpu(), pc)
        _same((crop, pts, tgt), ld.get(ids.tolist(), point_coord=pc.to(dev)))
        for p in params:
            p.grad = None
        want = [float(v) for v in sharded_step(unet, net, layer, crop, pts, tgt, npts, 1.0, 0.0125, "l1", distributed=False)]
        print("replay %d: graphed %s eager %s" % (k, got, want))
        for x, y in zip(got, want):
            assert abs(x - y) <= 1e-5 * abs(y), (got, want)
    assert gstep.replays == 3 and s.offset() == 10
