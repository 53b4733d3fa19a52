"""CPU checks of the Euler-Maruyama sampler's host side: the Philox host model against the Random123 known answers,
solver_core.em_plan against the coefficients the reference computed (tests/golden/em_golden.npz, made by
make_em_golden.py from the reference's own sde.euler_maruyama), the torch port sde.euler_maruyama on the oracle net
against the reference's ODE and SDE results, and the native boundary's argument checks (no GPU)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import uvit_ref
from panopticdiffusionmodels_amd import _lib, philox, sde
from panopticdiffusionmodels_amd import configs as C
from panopticdiffusionmodels_amd import solver_core as sc
from panopticdiffusionmodels_amd import weights as W

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, STEPS = "tiny_uvit_cond", 12


@pytest.fixture(scope="module")
def em_golden():
    return np.load(os.path.join(REPO, "tests", "golden", "em_golden.npz"))


def rel(a, b):
    a = torch.as_tensor(a).double()
    b = torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# ---- Philox ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ctr, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, want):
    """Random123's kat_vectors for philox4x32 with 10 rounds."""
    got = philox.philox4x32(ctr, key)
    assert " ".join("%08x" % int(v) for v in got) == want


def test_philox_layout_and_normals():
    """Element o = word o & 3 of quad o >> 2 with counter (quad, step, sample lo, sample hi) and key (seed lo, hi);
    the sample index carries into the high counter word; the normals are the spec's Box-Muller of those words."""
    seed, off, step, per = (0x9abcdef1 << 32) | 0x12345678, 2 ** 32 - 2, 7, 105
    w = philox.philox_words(5, per, seed, off, step)
    assert w.shape == (5, per) and w.dtype == np.uint32
    for b, o in [(0, 0), (1, 5), (2, 104), (4, 63)]:
        s = off + b
        q = philox.philox4x32((o >> 2, step, s & 0xffffffff, s >> 32), (seed & 0xffffffff, seed >> 32))
        assert int(w[b, o]) == int(q[o & 3])
    n = philox.philox_normal(5, per, seed, off, step)
    u = ((w >> 8).astype(np.float64) + 0.5) * 2.0 ** -24
    assert n[3, 8] == np.sqrt(-2 * np.log(u[3, 8])) * np.cos(2 * np.pi * u[3, 9])
    assert n[3, 11] == np.sqrt(-2 * np.log(u[3, 10])) * np.sin(2 * np.pi * u[3, 11])
    # a prefix of a sample and a shifted batch see the same stream
    np.testing.assert_array_equal(philox.philox_words(2, 64, seed, off + 1, step), w[1:3, :64])
    big = philox.philox_normal(64, 4096, seed=3)
    assert abs(big.mean()) < 0.01 and abs(big.std() - 1) < 0.01


# ---- plan --------------------------------------------------------------------------------------------------

def test_em_plan_vs_reference_coefficients(em_golden):
    """em_plan rows against what the reference computed per step (fp64 host vs the reference's fp32: 1e-5 relative,
    the bound of test_solver_plan).  b against the reference's own fp32 score scale cum_beta(t).rsqrt() carries that
    value's cancellation error: cum_beta = 1 - exp(-x) loses up to 2^-24 absolutely (exp's rounding below 1 plus the
    subtraction's), and rsqrt halves the relative error 2^-24 / cum_beta, which is 1.4e-4 at t = eps = 1e-3; so b
    is checked at 1e-5 against the exact sigma_t of the fixture's t, and at 1e-5 + 2^-24 / cum_beta against the
    reference's fp32 rsqrt."""
    g = em_golden
    s, t = g["steps/s"].astype(np.float64), g["steps/t"].astype(np.float64)
    dt = s - t
    hs = sc.HostLinear(0.1, 20.0)
    for kind in ("sde", "ode"):
        half = 1.0 if kind == "sde" else 0.5
        p = sc.em_plan(hs, STEPS, 1e-3, 1.0, kind)
        assert p.shape == (STEPS, 4) and p.dtype == np.float64
        np.testing.assert_allclose(p[:, 0], 999.0 * t, rtol=1e-5)
        np.testing.assert_allclose(p[:, 1], 1.0 - 0.5 * g["steps/beta"] * dt, rtol=1e-5)
        cum_beta = -np.expm1(-(0.1 * t + 19.9 * t * t * 0.5))
        np.testing.assert_allclose(p[:, 2], half * g["steps/g2"] * dt / np.sqrt(cum_beta), rtol=1e-5)
        b_ref = half * g["steps/g2"].astype(np.float64) * dt * g["steps/rsqrt_cum_beta"]
        assert np.all(np.abs(p[:, 2] - b_ref) <= (1e-5 + 2.0 ** -24 / cum_beta) * np.abs(b_ref))
        if kind == "sde":
            np.testing.assert_allclose(p[:-1, 3], g["steps/sigma"][:-1], rtol=1e-5)
            assert np.all(p[:-1, 3] > 0)
        else:
            assert np.all(p[:, 3] == 0)
        assert p[-1, 3] == 0.0   # no noise on the last step (s == 0)
    # grid endpoints: the first step starts at T, the last net call is at eps and lands on 0
    p = sc.em_plan(hs, STEPS, 1e-3, 1.0, "sde")
    assert p[0, 0] == 999.0 and p[-1, 0] == 999.0 * float(np.float32(1e-3))
    ts = sc.em_grid(STEPS, 1e-3, 1.0)
    assert ts[0] == 0.0 and ts[1] == float(np.float32(1e-3)) and ts[-1] == 1.0 and len(ts) == STEPS + 1
    assert s[-1] == 0.0 and t[0] == 1.0


def test_em_plan_rejects():
    hs = sc.HostLinear(0.1, 20.0)
    with pytest.raises(ValueError):
        sc.em_plan(hs, 10, 1e-3, 1.0, "heun")
    with pytest.raises(NotImplementedError, match="noise"):
        sc.em_plan(hs, 10, 1e-3, 1.0, "sde", pred="x0_pred")
    with pytest.raises(NotImplementedError):
        sc.em_plan(sc.HostCosine(), 10, 1e-3, 1.0, "sde")
    with pytest.raises(ValueError):
        sc.em_plan(hs, 0, 1e-3, 1.0, "sde")


# ---- torch port --------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def oracle_score(em_golden):
    cfg = C.nnet_kwargs(NAME)
    sd = W.nnet_state_dict(cfg, seed=11, init="random")
    chk = np.array([float(v.double().sum()) for v in sd.values()] +
                   [float(v.double().abs().sum()) for v in sd.values()])
    np.testing.assert_allclose(chk, em_golden["sd_checksum"], rtol=1e-12)   # the fixture's weights
    kw = dict(cfg)
    kw.pop("name")
    null, scale = cfg["num_classes"] - 1, float(em_golden["cfg_scale"])

    def cfg_nnet(x, timesteps, y):   # eval_ldm.py:66-74
        _cond = uvit_ref.uvit_forward(sd, kw, x, timesteps, y)
        _uncond = uvit_ref.uvit_forward(sd, kw, x, timesteps, torch.tensor([null] * x.size(0)))
        return _cond + scale * (_cond - _uncond)
    return sde.ScoreModel(cfg_nnet, pred="noise_pred", sde=sde.VPSDE())


def test_euler_maruyama_ode_vs_reference(em_golden, oracle_score):
    """1e-5 rel-L2: the oracle-vs-reference bound (DESIGN §9 row c)."""
    z0, y = torch.from_numpy(em_golden["z_init"]), torch.from_numpy(em_golden["y"])
    trace = []
    z = sde.euler_maruyama(sde.ODE(oracle_score), z0, STEPS, trace=trace, y=y)
    assert len(trace) == STEPS + 1 and trace[0] is z0 and trace[-1] is z
    r = rel(z, em_golden["ode/z"])
    print(f"ode port vs reference: rel-L2 {r:.3e}")
    assert r < 1e-5


def test_euler_maruyama_sde_vs_reference(em_golden, oracle_score):
    """Same torch seed, same torch.randn_like calls in the same order -> the reference's noise."""
    z0, y = torch.from_numpy(em_golden["z_init"]), torch.from_numpy(em_golden["y"])
    torch.manual_seed(int(em_golden["sde/seed"]))
    z = sde.euler_maruyama(sde.ReverseSDE(oracle_score), z0, STEPS, y=y)
    r = rel(z, em_golden["sde/z"])
    print(f"sde port vs reference: rel-L2 {r:.3e}")
    assert r < 1e-5
    assert rel(z, em_golden["ode/z"]) > 1e-2   # and it is not the ODE's result


def test_euler_maruyama_randn_calls(monkeypatch):
    """One torch.randn_like per step with s != 0 (steps - 1 calls), none on the last; kwargs reach the net."""
    calls, seen = [], []
    real = torch.randn_like
    monkeypatch.setattr(torch, "randn_like", lambda x: calls.append(1) or real(x))

    def net(x, t, **kw):
        seen.append((float(t[0]), kw))
        return torch.zeros_like(x)
    sm = sde.ScoreModel(net, pred="noise_pred", sde=sde.VPSDE())
    x = torch.ones(2, 3, 4, 4, dtype=torch.float64)
    out = sde.euler_maruyama(sde.ReverseSDE(sm), x, 5, tag="k")
    assert len(calls) == 4 and out.dtype == torch.float64
    assert all(kw == dict(tag="k") for _, kw in seen)
    assert seen[0][0] == 999.0 and abs(seen[-1][0] - 0.999) < 1e-9 and len(seen) == 5


# ---- native boundary ---------------------------------------------------------------------------------------

def test_lib_declares_em_symbols():
    lib = _lib.load()
    for name in ("pdm_em_step", "pdm_philox_normal", "pdm_philox_raw"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)


def _good_args():
    a = _lib.PdmEmStepArgs()
    a.pre = a.x = a.xin = a.table = a.counter = a.t_next = 16   # never dereferenced: every case fails the checks
    a.B, a.C, a.H, a.W, a.steps = 2, 3, 5, 7, 4
    return a


@pytest.mark.parametrize("field, value", [("pre", None), ("x", None), ("xin", None), ("table", None),
                                          ("counter", None), ("t_next", None), ("B", 0), ("C", -1), ("H", 0),
                                          ("W", 0), ("steps", 0), ("conv_w", 16)])
def test_em_step_rejects_bad_arguments_without_gpu(field, value):
    """pdm_em_step checks its arguments before any GPU call (status 1 = PDM_ERR_ARG, as pdm_stage_epilogue)."""
    lib = _lib.load()
    a = _good_args()
    setattr(a, field, value)   # conv_w without conv_b: the bias is missing
    assert lib.pdm_em_step(ctypes.byref(a), None) == 1
    assert b"em_step" in lib.pdm_last_error()
    assert lib.pdm_em_step(None, None) == 1


def test_philox_rejects_bad_arguments_without_gpu():
    lib = _lib.load()
    for fn in (lib.pdm_philox_normal, lib.pdm_philox_raw):
        for args in [(None, 1, 4, 0, 0, 0), (ctypes.c_void_p(16), 0, 4, 0, 0, 0), (ctypes.c_void_p(16), 1, 0, 0, 0, 0),
                     (ctypes.c_void_p(16), 1, 4, 0, 0, -1)]:
            assert fn(*args, None) == 1
            assert b"philox" in lib.pdm_last_error()


def test_wrappers_reject_bad_arguments_without_gpu():
    """The Python wrappers validate shapes and dtypes on the host before anything touches the GPU."""
    f = torch.zeros
    pre, x, xin = f(4, 3, 5, 7), f(2, 3, 5, 7), f(4, 3, 5, 7)
    table, counter, t = f(6, 4), f(1, dtype=torch.int32), f(4)
    ok = _lib.em_step_args(pre, 2, x, xin, table, counter, t, cfg_scale=0.4, seed=2 ** 64 - 1, sample_offset=2 ** 63)
    assert (ok.B, ok.C, ok.H, ok.W, ok.steps, ok.has_uncond) == (2, 3, 5, 7, 6, 1)
    assert ok.seed == 2 ** 64 - 1 and ok.sample_offset == 2 ** 63
    with pytest.raises(ValueError):
        _lib.em_step_args(pre, 2, x, xin, table, counter, t)                       # rows do not match no-CFG
    with pytest.raises(ValueError):
        _lib.em_step_args(pre, 2, x, xin, f(6, 3), counter, t, cfg_scale=0.4)      # table not [steps, 4]
    with pytest.raises(ValueError):
        _lib.em_step_args(pre, 2, x, xin, table, f(1), t, cfg_scale=0.4)           # counter not int32
    with pytest.raises(ValueError):
        _lib.em_step_args(pre, 2, x, xin, table, counter, f(2), cfg_scale=0.4)     # time buffer not [rows]
    with pytest.raises(ValueError):
        _lib.em_step_args(pre, 2, x, xin, table, counter, t, cfg_scale=0.4, conv_w=f(3, 3, 3, 3))
    with pytest.raises(ValueError):
        _lib.em_step_args(pre, 2, x, xin, table, counter, t, cfg_scale=0.4, seed=2 ** 64)
    with pytest.raises(ValueError):
        _lib.philox_normal(0, 4)
    with pytest.raises(ValueError):
        _lib.philox_normal(1, 4, sample_offset=-1)


def test_sampler_and_configs_declare_the_feature():
    from panopticdiffusionmodels_amd import sampler
    assert hasattr(sampler, "EulerMaruyamaSampler")
    assert C.get_config("cifar10_uvit_small")["reference_sample"] == dict(algorithm="euler_maruyama_sde",
                                                                          sample_steps=1000)
    for name in C.CONFIGS:
        if name != "cifar10_uvit_small":
            assert C.get_config(name)["reference_sample"] == dict(algorithm="dpm_solver", sample_steps=50)
