"""The Euler-Maruyama sampler on the GPU: the device generator against its host model (bit-exact words, normals
within the measured fp32 error), pdm_em_step against a torch model over consecutive steps, the fused ODE / SDE
samplers against the reference's results (tests/golden/em_golden.npz) and the CPU port, the invariances the noise
keying promises (lanes, batch composition, sample_offset, replay, capture block) and the stale-graph rule."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import uvit_ref
from panopticdiffusionmodels_amd import configs as C
from panopticdiffusionmodels_amd import philox, sde
from panopticdiffusionmodels_amd import weights as W
from panopticdiffusionmodels_amd.sampler import EulerMaruyamaSampler
from panopticdiffusionmodels_amd.utils import get_nnet

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, STEPS = "tiny_uvit_cond", 12
TOL_FINAL = 1e-2        # bf16 net vs the reference's final latent (test_gpu_sample.py)
# fp32 Box-Muller on the device vs the float64 host model of the same words: the largest difference measured on an
# MI355X over the two blocks below was 6.522e-07; 4x for logf / sincospif differences between ROCm versions
NORMAL_MAX_ABS = 4 * 6.522e-07
SEED = (0x9abcdef1 << 32) | 0x12345678   # both halves non-zero


def rel(a, b):
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from panopticdiffusionmodels_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope="module")
def dev(lib):
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def em_golden():
    return np.load(os.path.join(REPO, "tests", "golden", "em_golden.npz"))


def _net(dev, seed=11):
    cfg = C.nnet_kwargs(NAME)
    net = get_nnet(**cfg)
    net.load_state_dict(W.nnet_state_dict(cfg, seed=seed, init="random"))
    return net.to(dev).eval(), cfg


@pytest.fixture(scope="module")
def net(dev):
    return _net(dev)[0]


def _sampler(net, **kw):
    full = C.get_config(NAME)
    kw.setdefault("steps", STEPS)
    return EulerMaruyamaSampler(net, cfg_scale=full["cfg_scale"], **kw)


def _inputs(B, dev, seed=1234):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 4, 16, 16, generator=g).to(dev), torch.randint(0, 10, (B,), generator=g).to(dev)


# ---- generator ---------------------------------------------------------------------------------------------

def _words(lib, *a, **k):
    return lib.philox_normal(*a, raw=True, **k).cpu().numpy().view(np.uint32)


def test_philox_words_bit_exact(lib):
    """per_sample = 105 = 3 * 5 * 7 (not a multiple of 4), sample indices crossing 2^32, both seed halves set."""
    B, per, off, step = 5, 105, 2 ** 32 - 2, 7
    got = _words(lib, B, per, SEED, off, step)
    np.testing.assert_array_equal(got, philox.philox_words(B, per, SEED, off, step))
    big = _words(lib, 8, 3072, SEED, 3, 999)
    np.testing.assert_array_equal(big, philox.philox_words(8, 3072, SEED, 3, 999))


def test_philox_normals_vs_host_model(lib):
    worst = 0.0
    for B, per, off, step in [(5, 105, 2 ** 32 - 2, 7), (8, 3072, 3, 999)]:
        got = lib.philox_normal(B, per, SEED, off, step).cpu().numpy().astype(np.float64)
        want = philox.philox_normal(B, per, SEED, off, step)
        assert np.isfinite(got).all()
        worst = max(worst, float(np.abs(got - want).max()))
    print(f"philox normals: max |device fp32 - host fp64| = {worst:.3e}")
    assert worst <= NORMAL_MAX_ABS


def test_philox_streams_differ_and_repeat(lib):
    B, per = 4, 105
    a = _words(lib, B, per, SEED, 10, 3)
    assert np.array_equal(a, _words(lib, B, per, SEED, 10, 3))               # same arguments, same output
    assert torch.equal(lib.philox_normal(B, per, SEED, 10, 3), lib.philox_normal(B, per, SEED, 10, 3))
    assert not np.array_equal(a, _words(lib, B, per, SEED, 10, 4))           # another step
    assert not np.array_equal(a[0], a[1])                                    # another sample
    assert np.array_equal(a[1:], _words(lib, B - 1, per, SEED, 11, 3))       # keyed on the global sample index
    assert not np.array_equal(a, _words(lib, B, per, SEED + 1, 10, 3))       # another seed


# ---- step kernel -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B, Cc, H, Wd, conv_cfg", [(3, 4, 6, 10, True), (2, 3, 5, 7, False)])
def test_em_step_vs_torch_model(lib, B, Cc, H, Wd, conv_cfg):
    """Three consecutive pdm_em_step calls on a 3-row table (last row c == 0) against x' = a x + b e + c z in torch
    fp32 with the dumped noise: the counter, the table indexing and the next-t write; bound of test_stage_epilogue."""
    g = torch.Generator(device="cuda").manual_seed(5)
    rows = 2 * B if conv_cfg else B
    w = torch.randn(Cc, Cc, 3, 3, device="cuda", generator=g) * 0.2 if conv_cfg else None
    bias = torch.randn(Cc, device="cuda", generator=g) if conv_cfg else None
    scale = 0.4 if conv_cfg else None
    table = torch.tensor([[999.0, 1.7, -0.9, 1.3], [500.5, 1.2, -0.5, 0.6], [0.999, 1.01, -0.01, 0.0]], device="cuda")
    x = torch.randn(B, Cc, H, Wd, device="cuda", generator=g)
    xin = torch.zeros(rows, Cc, H, Wd, device="cuda")
    t = torch.full((rows,), -1.0, device="cuda")
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    off_dev = torch.tensor([2], dtype=torch.int64, device="cuda")
    ref = x.clone()
    for k in range(3):
        pre = torch.randn(rows, Cc, H, Wd, device="cuda", generator=g)
        lib.em_step(pre, B, x, xin, table, counter, t, conv_w=w, conv_b=bias, cfg_scale=scale, seed=SEED,
                    sample_offset=5, sample_offset_dev=off_dev)
        e = F.conv2d(pre, w, bias, padding=1) if conv_cfg else pre
        if conv_cfg:
            e = e[:B] + scale * (e[:B] - e[B:])
        z = lib.philox_normal(B, Cc * H * Wd, SEED, 7, k).view(B, Cc, H, Wd)
        a, b, c = (float(v) for v in table[k, 1:])
        ref = a * ref + b * e + c * z
        assert rel(x, ref) < 1e-5, k
        assert torch.equal(xin[:B], x) and (not conv_cfg or torch.equal(xin[B:], x))
        assert int(counter) == k + 1
        assert torch.equal(t, table[min(k + 1, 2), 0].expand(rows))   # the next step's t_net; kept after the last
        ref = x.clone()   # compare step by step
    # the last row has c == 0: that step added no noise (checked above with z scaled by 0); a call past the end of
    # the table changes nothing
    before = (x.clone(), xin.clone(), t.clone())
    lib.em_step(pre, B, x, xin, table, counter, t, conv_w=w, conv_b=bias, cfg_scale=scale, seed=SEED)
    assert int(counter) == 3 and all(torch.equal(p, q) for p, q in zip(before, (x, xin, t)))


# ---- fused samplers ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("graph", [False, True])
def test_fused_ode_vs_reference(em_golden, dev, net, graph):
    s = _sampler(net, kind="ode", use_graph=graph)
    z0, y = torch.from_numpy(em_golden["z_init"]).to(dev), torch.from_numpy(em_golden["y"]).to(dev)
    z = s.sample(z0, y)
    r = rel(z, em_golden["ode/z"])
    print(f"fused ode (graph={graph}) vs reference: rel-L2 {r:.3e}; per sample "
          f"{[round(rel(z[i], em_golden['ode/z'][i]), 5) for i in range(z.shape[0])]}")
    assert r < TOL_FINAL


def _oracle_score(em_golden):
    cfg = C.nnet_kwargs(NAME)
    sd = W.nnet_state_dict(cfg, seed=11, init="random")
    kw = dict(cfg)
    kw.pop("name")
    null, scale = cfg["num_classes"] - 1, float(em_golden["cfg_scale"])

    def cfg_nnet(x, timesteps, y):
        c = uvit_ref.uvit_forward(sd, kw, x, timesteps, y)
        u = uvit_ref.uvit_forward(sd, kw, x, timesteps, torch.tensor([null] * x.size(0)))
        return c + scale * (c - u)
    return sde.ScoreModel(cfg_nnet, pred="noise_pred", sde=sde.VPSDE())


def test_fused_sde_vs_cpu_port(em_golden, dev, net, monkeypatch):
    """The fused SDE sampler against sde.euler_maruyama on the CPU oracle net drawing the sampler's own noise:
    torch.randn_like is replaced by the dumps of noise(step, ...) in call order (one call per step with s != 0)."""
    s = _sampler(net, kind="sde", seed=SEED, capture_block=5)   # 12 = 2 replays of 5 + 2 uncaptured
    z0, y = torch.from_numpy(em_golden["z_init"]), torch.from_numpy(em_golden["y"])
    z = s.sample(z0.to(dev), y.to(dev), sample_offset=40)
    dumps = [s.noise(k, z0.shape[0], sample_offset=40).cpu() for k in range(STEPS - 1)]
    it = iter(dumps)
    monkeypatch.setattr(torch, "randn_like", lambda x: next(it))
    want = sde.euler_maruyama(sde.ReverseSDE(_oracle_score(em_golden)), z0, STEPS, y=y)
    assert next(it, None) is None   # every dump was drawn
    r = rel(z, want)
    print(f"fused sde vs cpu port with the same noise: rel-L2 {r:.3e}")
    assert r < TOL_FINAL
    assert rel(z, em_golden["ode/z"]) > 1e-2   # noise was added


def test_invariances(dev, net):
    """A sample's result does not depend on lanes, batch composition, batch position, replay or the capture block."""
    z, y = _inputs(9, dev)
    kw = dict(kind="sde", seed=SEED)
    one = _sampler(net, **kw)
    full9 = one.sample(z, y)
    assert torch.isfinite(full9).all()
    a5 = one.sample(z[:5], y[:5])
    assert torch.equal(a5, one.sample(z[:5], y[:5]))                        # replay: counter and time buffer reset
    assert rel(_sampler(net, lanes=2, **kw).sample(z[:5], y[:5]), a5) < 1e-6   # lanes
    assert rel(a5[:3], one.sample(z[:3], y[:3])) < 1e-6                     # batch composition
    assert rel(a5, full9[:5]) < 1e-6
    assert rel(one.sample(z[7:9], y[7:9], sample_offset=7), full9[7:9]) < 1e-6   # batch position
    assert rel(one.sample(z[7:9], y[7:9]), full9[7:9]) > 1e-2               # ... and the offset is what does it
    s13 = _sampler(net, steps=13, capture_block=5, **kw)                    # 13 = 2 * 5 + 3
    assert rel(s13.sample(z[:3], y[:3]), s13.sample(z[:3], y[:3], eager=True)) < 1e-6
    assert rel(one.sample(z[:3], y[:3], eager=True), a5[:3]) < 1e-6


def test_stale_graph_recaptured(dev):
    """load_state_dict rebuilds the native handle: the next sample recaptures instead of replaying on freed memory."""
    net, cfg = _net(dev)
    z, y = _inputs(3, dev, seed=7)
    s = _sampler(net, kind="ode")
    first = s.sample(z, y)
    st = s._state[(3, z.device, None)]
    g1 = st["graph"]
    assert g1 is not None and torch.equal(s.sample(z, y), first) and st["graph"] is g1
    net.load_state_dict(W.nnet_state_dict(cfg, seed=12, init="random"))
    again = s.sample(z, y)
    assert st["graph"] is not None and st["graph"] is not g1
    fresh, _ = _net(dev, seed=12)
    assert torch.equal(again, _sampler(fresh, kind="ode", use_graph=False).sample(z, y))
    assert rel(again, first) > 1e-3
