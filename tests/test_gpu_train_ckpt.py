"""GPU checks of HipTrainState's checkpoints (save / load / resume, interchangeable with the reference's
utils.TrainState directory) and of the global gradient norm / clipping kernels (pdm_grad_norm_clip,
pdm_train_grad_norm).

The reference-written checkpoint comes from tests/golden/ckpt_golden*.npz (tests/golden/make_ckpt_golden.py ran the
reference's own loop and TrainState.save); the .pth files are rebuilt from it in a temporary directory.  Error measure
of the norm kernel, u = 2^-24 as in tests/test_gpu_train_kernels.py: derived below from the reduction's shape."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ckpt_fixture import NAME, Fixture  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
CONFIGS = ["tiny_uvit_train", "tiny_uvit_train_uncond", "tiny_t2i_train"]


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.fixture(scope="module")
def fx():
    return Fixture.get()


def _trainer(name, lanes=1, seed=11):
    from panopticdiffusionmodels_amd import configs, weights
    from panopticdiffusionmodels_amd.train import HipTrainState
    full = configs.get_config(name)
    st = HipTrainState(full["nnet"], DEV, optimizer=full.get("optimizer"), lr_scheduler=full.get("lr_scheduler"),
                       ema_rate=full["train"]["ema_rate"], lanes=lanes)
    st.load_state_dict(weights.nnet_state_dict(full["nnet"], seed=seed, init="random"))
    return full, st


def _inputs(name, i, B=4):
    """Seeded inputs of real step i (distinct labels: the label_emb gradient adds with float atomics, which is
    order-dependent only where a label repeats)."""
    from panopticdiffusionmodels_amd import configs
    full = configs.get_config(name)
    n = full["nnet"]
    g = torch.Generator().manual_seed(1000 + i)
    shape = (B,) + tuple(full["z_shape"])
    xt, eps = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    t = torch.randint(1, 1001, (B,), generator=g).float()
    if n["name"] == "uvit_t2i":
        ctx = torch.randn(B, n["num_clip_token"], n["clip_dim"], generator=g)
        scaled = torch.randint(0, 2, (B, n["num_panoptic_class"]) + shape[2:], generator=g).float() * 2 - 1
        mask_n = 0.7 * scaled + 0.7 * 2 * torch.randn(scaled.shape, generator=g)
        return xt, t, ctx, mask_n, eps, scaled
    y = (torch.arange(B) * 3 + i) % n["num_classes"] if n.get("num_classes", -1) > 0 else None
    return xt, t, y, eps


def _step(st, name, i):
    args = _inputs(name, i, B=2 if st.t2i else 4)
    if st.t2i:
        st.forward_backward_t2i(*args)
    else:
        st.forward_backward(*args)
    return st.optimizer_step()


def _flat(st):
    return {k: getattr(st, k).detach().cpu().clone() for k in ("P", "E", "M", "V", "WB", "WT")}


# ---- 1. restored state ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [(1, 2), (2, 1)])
@pytest.mark.parametrize("name", CONFIGS)
def test_load_restores_every_buffer(name, lanes, tmp_path):
    """Two real steps, save, load into a fresh trainer of the other lane count (holding other weights, non-zero
    moments and gradients): P, E, M, V and the bf16 copies bit-equal, step and LR equal, gradients zero."""
    full, a = _trainer(name, lanes=lanes[0])
    for i in range(2):
        _step(a, name, i)
    path = str(tmp_path / "2.ckpt")
    a.save(path)
    assert sorted(os.listdir(path)) == ["lr_scheduler.pth", "nnet.pth", "nnet_ema.pth", "optimizer.pth", "step.pth"]
    _, b = _trainer(name, lanes=lanes[1], seed=5)
    _step(b, name, 7)                         # moments, a step count and gradients of its own
    b.optimizer.update(lr=1.0, betas=(0.5, 0.5), weight_decay=0.5)
    b.load(path)
    fa, fb = _flat(a), _flat(b)
    for k in fa:
        assert same_bits(fa[k], fb[k]), k
    assert b.step == a.step == 2 and b.current_lr() == a.current_lr()
    assert b.optimizer["betas"] == tuple(full["optimizer"]["betas"]) and b.optimizer["lr"] == full["optimizer"]["lr"]
    assert b.optimizer["weight_decay"] == full["optimizer"]["weight_decay"]
    assert float(b.G.abs().max()) == 0.0 and (b.G2 is None or float(b.G2.abs().max()) == 0.0)
    # every file loads with plain torch.load under the default weights_only; t2i: no state for the unused parameters
    osd = torch.load(os.path.join(path, "optimizer.pth"), map_location="cpu")
    names = [k for k, _ in a.param_order()]
    assert {names[i] for i in osd["state"]} == set(names) - a.stateless_params()
    assert (len(a.stateless_params()) > 0) == a.t2i
    assert torch.load(os.path.join(path, "step.pth")) == 2
    nsd = torch.load(os.path.join(path, "nnet.pth"), map_location="cpu")
    assert list(nsd) == names and all(v.dtype == torch.float32 and tuple(v.shape) == s
                                      for v, (_, s) in zip(nsd.values(), a.param_order()))


def test_load_rejects_disagreeing_steps_and_strict_keys(fx, tmp_path):
    path = fx.write_dir(str(tmp_path / "3.ckpt"))
    _, st = _trainer(NAME)
    before = _flat(st)
    torch.save(4, os.path.join(path, "step.pth"))
    with pytest.raises(ValueError, match=r"step\.pth = 4.*step = 3.*last_epoch = 3"):
        st.load(path)
    torch.save(3, os.path.join(path, "step.pth"))
    sd = fx.nnet_sd()
    sd["extra.weight"] = torch.zeros(3)
    del sd["norm.bias"]
    torch.save(sd, os.path.join(path, "nnet.pth"))
    with pytest.raises(KeyError):
        st.load(path)
    after = _flat(st)
    assert all(same_bits(before[k], after[k]) for k in before) and st.step == 0     # nothing changed by a failed load
    st.load(path, strict=False)                                                      # the reference's strict=False
    p = st.state_dict()
    assert same_bits(p["norm.weight"], fx.nnet_sd()["norm.weight"]) and st.step == 3
    off, n = st.index["norm.bias"]
    assert same_bits(st.P[off:off + n], before["P"][off:off + n])                    # the missing key keeps its value


# ---- 2. resume equals not stopping ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CONFIGS)
def test_resume_equals_not_stopping(name, tmp_path):
    """Five steps uninterrupted (twice) against three steps + save + a fresh trainer + resume + two steps, same inputs.
    Per tensor the resumed run may differ from an uninterrupted one by at most 4x what the two uninterrupted runs
    differ by: bit-equal wherever those are."""
    runs = []
    for _ in range(2):
        _, st = _trainer(name)
        for i in range(5):
            _step(st, name, i)
        runs.append(st)
    _, a = _trainer(name)
    for i in range(3):
        _step(a, name, i)
    root = str(tmp_path / "ckpts")
    a.save(os.path.join(root, "1.ckpt"))      # an older one: resume must take the largest step
    a.save(os.path.join(root, "3.ckpt"))
    torch.save(1, os.path.join(root, "1.ckpt", "step.pth"))
    del a
    _, b = _trainer(name, seed=5)
    assert b.resume(os.path.join(root, "missing")) is False
    assert b.resume(root) is True and b.step == 3
    for i in range(3, 5):
        _step(b, name, i)
    assert b.step == runs[0].step == 5 and b.current_lr() == runs[0].current_lr()
    worst = 0.0
    for buf in ("P", "E", "M", "V"):
        r0, r1, rb = (getattr(s, buf).detach().cpu().double() for s in (runs[0], runs[1], b))
        for k, (off, n) in b.index.items():
            spread = float((r0[off:off + n] - r1[off:off + n]).norm())
            diff = float((rb[off:off + n] - r0[off:off + n]).norm())
            worst = max(worst, spread / max(float(r0[off:off + n].norm()), 1e-30))
            assert diff <= 4 * spread, (buf, k, diff, spread)
    print(f"resume {name}: worst run-to-run spread of the uninterrupted runs, relative per tensor = {worst:.3e}")


# ---- 3. a reference-written checkpoint ------------------------------------------------------------------------------
def test_reference_checkpoint_next_optimizer_step(fx, tmp_path):
    """Load the reference's step-3 directory, give AdamW the reference's iteration-3 gradients: the applied LR is the
    reference's (an off-by-one step fails here: the LR and both bias corrections move), and parameters, EMA and
    moments follow torch.optim.AdamW / utils.ema within the bounds of test_adamw_ema_vs_reference."""
    from oracle import train_ref
    path = fx.write_dir(str(tmp_path / "3.ckpt"))
    full, st = _trainer(NAME, seed=5)
    st.load(path)
    assert st.step == 3 and st.current_lr() == float(fx["it3_lr"])
    p0, e0 = st.state_dict(), st.ema_state_dict()
    for k in fx.names:
        assert same_bits(p0[k], fx.nnet_sd()[k]) and same_bits(e0[k], fx.ema_sd()[k]), k
    g = {k: fx.t(f"grad/{k}") for k in fx.names}
    with torch.no_grad():
        for k, v in g.items():
            st._view(st.G, k).copy_(v.to(DEV).view(st._view(st.G, k).shape))
    lr = st.optimizer_step()
    assert abs(lr - float(fx["it3_lr"])) < 1e-12 and st.step == 4
    opt = full["optimizer"]
    p, e = st.state_dict(), st.ema_state_dict()
    m, v = st._host_dict(st.M), st._host_dict(st.V)
    m3, v3 = fx.exp_avg(), fx.exp_avg_sq()
    worst = {}
    for k in fx.names:
        pr, mr, vr = train_ref.adamw_step(fx.nnet_sd()[k], g[k], m3[k], v3[k], 4, float(fx["it3_lr"]), opt["betas"],
                                          1e-8, opt["weight_decay"])
        er = train_ref.ema(fx.ema_sd()[k], pr, full["train"]["ema_rate"])
        for what, got, ref in (("p", p[k].cpu(), pr), ("ema", e[k].cpu(), er), ("m", m[k], mr), ("v", v[k], vr)):
            frac = float(((got - ref).abs() / (2.5e-7 * ref.abs() + 1e-9)).max())
            worst[what] = max(worst.get(what, 0.0), frac)
    print("reference checkpoint, one AdamW step: worst fraction of 2.5e-7 |ref| + 1e-9:", worst)
    assert max(worst.values()) <= 1.0, worst


def _sketch(key, v, S=8):
    """tests/golden/make_train_h_golden.sketch without the norm: inner products with N(0, 1) vectors seeded crc32(key) + i"""
    import zlib
    v = v.detach().double().flatten().cpu()
    return np.array([float(torch.randn(v.numel(), generator=torch.Generator().manual_seed(zlib.crc32(key.encode()) + i),
                                       dtype=torch.float64) @ v) for i in range(S)])


def test_reference_checkpoint_continues_the_references_loop(fx, tmp_path):
    """From the reference's step-3 directory, iterations 3 and 4 on the reference's draws: losses <= 1e-2, and the
    displacement from the step-3 parameters against the reference's (sketches of its step-5 parameters) < 0.25, the
    EMA <= 1e-3 -- the measures and bounds of test_three_iterations_vs_reference."""
    path = fx.write_dir(str(tmp_path / "3.ckpt"))
    _, st = _trainer(NAME, seed=5)
    st.load(path)
    y = torch.from_numpy(fx.tg[f"{NAME}/y"])
    for i in (3, 4):
        loss = st.forward_backward(fx.t(f"it{i}_xt"), fx.t(f"it{i}_t"), y, fx.t(f"it{i}_eps"))
        print(f"iteration {i}: loss rel {rel(loss, fx[f'it{i}_loss']):.3e}")
        assert rel(loss, fx[f"it{i}_loss"]) < 1e-2, i
        lr = st.optimizer_step()
        assert abs(lr - float(fx[f"it{i}_lr"])) < 1e-12
    p, e = st.state_dict(), st.ema_state_dict()
    p3 = fx.nnet_sd()
    num = den = 0.0
    for k in fx.names:
        d_ref = fx[f"psk5/{k}"][1:] - _sketch(k, p3[k])
        d = _sketch(k, p[k].cpu().double() - p3[k].double())
        num += float(np.linalg.norm(d - d_ref) ** 2)
        den += float(np.linalg.norm(d_ref) ** 2)
        e_ref = fx[f"esk5/{k}"][1:]
        assert np.linalg.norm(_sketch(k, e[k]) - e_ref) / max(np.linalg.norm(e_ref), 1e-30) < 1e-3, k
    print(f"displacement over iterations 3, 4 vs the reference: {(num / den) ** 0.5:.3e}")
    assert (num / den) ** 0.5 < 0.25, (num / den) ** 0.5


# ---- 4. the other direction -----------------------------------------------------------------------------------------
def test_torch_optimizer_and_scheduler_load_the_written_files(tmp_path):
    """After three real steps the written optimizer.pth / lr_scheduler.pth load into torch.optim.AdamW + LambdaLR over
    the net's parameters, and torch's next step on a fixed gradient is AdamW from the trainer's own moments."""
    from oracle import train_ref
    full, st = _trainer(NAME)
    for i in range(3):
        _step(st, NAME, i)
    path = str(tmp_path / "3.ckpt")
    st.save(path)
    nsd = torch.load(os.path.join(path, "nnet.pth"), map_location="cpu")
    order = st.param_order()
    assert list(nsd) == [k for k, _ in order]
    params = [torch.nn.Parameter(nsd[k].clone()) for k, _ in order]        # the oracle net's parameters, in order
    opt = torch.optim.AdamW(params, lr=1.0, betas=(0.5, 0.5), weight_decay=0.9)
    warm = full["lr_scheduler"]["warmup_steps"]
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: min(s / warm, 1))
    opt.load_state_dict(torch.load(os.path.join(path, "optimizer.pth"), map_location="cpu"))
    sched.load_state_dict(torch.load(os.path.join(path, "lr_scheduler.pth"), map_location="cpu"))
    assert sched.last_epoch == 3 and opt.param_groups[0]["lr"] == st.current_lr() == sched.get_last_lr()[0]
    assert opt.param_groups[0]["betas"] == tuple(full["optimizer"]["betas"])
    m, v = st._host_dict(st.M), st._host_dict(st.V)
    g = torch.Generator().manual_seed(3)
    grads = [torch.randn(p.shape, generator=g) * 0.01 for p in params]
    for p, gr in zip(params, grads):
        p.grad = gr.clone()
    opt.step()
    sched.step()
    assert opt.param_groups[0]["lr"] == full["optimizer"]["lr"] * min(4 / warm, 1)
    o = full["optimizer"]
    for (k, _), p, gr in zip(order, params, grads):
        assert float(opt.state[p]["step"]) == 4.0
        pr, mr, vr = train_ref.adamw_step(nsd[k].double(), gr.double(), m[k].double(), v[k].double(), 4, st.current_lr(),
                                          o["betas"], 1e-8, o["weight_decay"])
        # two fp32 evaluations of one formula: a rounding of p and a few of the (1e-3 |p|) update
        assert bool(((p.detach().double() - pr).abs() <= 2.5e-7 * pr.abs() + 1e-9).all()), k
        assert bool(((opt.state[p]["exp_avg"].double() - mr).abs() <= 2.5e-7 * mr.abs() + 1e-9).all()), k


# ---- 5. the gradient norm and clip kernels, alone -------------------------------------------------------------------
MAX_BLOCKS = 1024       # GRAD_NORM_MAX_BLOCKS (csrc/pdm_train.h)


def _grid(n):
    """grad_norm_launch: one block of 256 threads per 256 float4, at most MAX_BLOCKS; (blocks, float4 per thread)."""
    n4 = n // 4
    blocks = max(1, min(MAX_BLOCKS, (n4 + 255) // 256))
    return blocks, (n4 + blocks * 256 - 1) // (blocks * 256)


# the largest size: 2 * 1024 * 256 float4 + 300 more, so the grid is capped (1024 blocks: each thread of the second
# kernel sums four partials), every thread of the first kernel loops twice and the first 300 three times; + 3 tail floats
BIG = 4 * (2 * MAX_BLOCKS * 256 + 300) + 3
SIZES = [1, 3, 4, 1023, 1025, 165120, BIG]


def _norm_bound(n):
    """Relative bound of the kernel's norm against float64 on the same fp32 inputs.  All summands are >= 0, so a sum
    tree of depth d is within about d u of exact, relatively.  Depth of a term's path: its square (1), the thread's
    chain (iters float4 adds into one accumulator lane), the four lanes' tree (2), the tail element (1), the wave
    butterfly (6), the four waves' chain (3); the second kernel: its thread's chain (ceil(blocks / 256)), 6, 3.  The
    norm is the square root: half the sum's relative error plus the root's own rounding (1 ulp = 2 u allowed)."""
    blocks, iters = _grid(n)
    d = 1 + iters + 2 + 1 + 6 + 3 + (blocks + 255) // 256 + 6 + 3
    return (d / 2 + 2) * U * 1.001, d


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_grad_norm_clip_kernels(n, two):
    from panopticdiffusionmodels_amd import _lib
    assert _grid(BIG) == (MAX_BLOCKS, 3) and _grid(BIG - 4 * 300 - 3)[1] == 2 and _grid(165120)[0] == 162
    gen = torch.Generator().manual_seed(n + int(two))
    PAD, SENT = 64, 1234.5
    blocks, _ = _grid(n)

    def buf(scale):
        t = torch.full((n + PAD,), SENT)
        t[:n] = torch.randn(n, generator=gen) * scale
        return t
    g0, g20 = buf(0.3), (buf(0.2) if two else None)
    v = (g0[:n] + g20[:n]) if two else g0[:n]                 # fp32: the element the kernel squares
    ref = math.sqrt(float((v.double() ** 2).sum()))
    bound, depth = _norm_bound(n)

    def run(max_norm):
        g, g2 = g0.to(DEV), (g20.to(DEV) if two else None)
        out = torch.full((2 + PAD,), SENT, device=DEV)
        scratch = torch.full((blocks + PAD,), SENT, device=DEV)
        _lib.check(_lib.load().pdm_grad_norm_clip(_lib.ptr(g), _lib.ptr(g2), n, float(max_norm), _lib.ptr(out),
                                                  _lib.ptr(scratch), blocks * 4, _lib.stream_ptr(g.device)),
                   "pdm_grad_norm_clip")
        torch.cuda.synchronize()
        for t, used in ((g, n), (g2, n), (out, 2), (scratch, blocks)):
            if t is not None:
                assert same_bits(t[used:], torch.full((PAD,), SENT)), "sentinel behind a buffer overwritten"
        return g.cpu(), (g2.cpu() if two else None), out[:2].cpu()

    worst = 0.0
    # the norm only (max_norm <= 0) and a threshold above the norm: nothing is written, coef = 1
    norms = []
    for max_norm in (0.0, -1.0, ref * 2 + 1.0):
        g, g2, out = run(max_norm)
        assert same_bits(g, g0) and (not two or same_bits(g2, g20)), max_norm
        err = abs(float(out[0].double()) - ref) / ref
        worst = max(worst, err / bound)
        assert err <= bound, (n, two, max_norm, err, bound)
        assert float(out[1]) == 1.0
        norms.append(out[0])
    assert same_bits(norms[0], norms[1]) and same_bits(norms[0], norms[2])      # run to run: the same bits
    # a threshold below the norm: every element is one fp32 multiply by the kernel's own coef
    max_norm = ref * 0.37
    g, g2, out = run(max_norm)
    assert same_bits(out[0], norms[0])
    coef = torch.minimum(torch.tensor(max_norm, dtype=torch.float32) / (out[0] + torch.tensor(1e-6)), torch.tensor(1.0))
    assert same_bits(out[1], coef), (float(out[1]), float(coef))
    assert 0.36 < float(coef) < 0.38
    exp = g0.clone()
    exp[:n] = g0[:n] * out[1]
    assert same_bits(g, exp)
    if two:
        exp2 = g20.clone()
        exp2[:n] = g20[:n] * out[1]
        assert same_bits(g2, exp2)
    ga, g2a, outa = run(max_norm)
    assert same_bits(ga, g) and same_bits(outa, out) and (not two or same_bits(g2a, g2))
    print(f"grad norm n {n} two {int(two)}: depth {depth}, worst / bound = {worst:.3f}")


def test_grad_norm_nan_and_zero():
    """A NaN gradient gives a NaN norm, which fails the coef >= 1 test and scales by NaN, as torch does; all-zero
    gradients give norm 0, coef 1 and stay zero."""
    from panopticdiffusionmodels_amd import _lib
    n = 1025
    scratch = torch.zeros(_lib.GRAD_NORM_SCRATCH_BYTES // 4, device=DEV)
    out = torch.zeros(2, device=DEV)
    g = torch.ones(n, device=DEV)
    g[77] = float("nan")
    _lib.grad_norm_clip(g, None, n, 1.0, out, scratch)
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(g).all())
    z = torch.zeros(n, device=DEV)
    _lib.grad_norm_clip(z, None, n, 1.0, out, scratch)
    assert out.tolist() == [0.0, 1.0] and float(z.abs().max()) == 0.0


# ---- 6. clip_grad_norm_ on a trainer after a real backward ----------------------------------------------------------
@pytest.mark.parametrize("lanes", [1, 2])
def test_clip_grad_norm_on_a_trainer(lanes):
    """The norm against torch.nn.utils.clip_grad_norm_ over the per-parameter gradients on the host (rel 1e-5: one
    flat sum against per-parameter norms; worst case (n + 2) u ~ 1e-2 for n = 165120, measured orders below), the
    gradients afterwards coef x the gradients before."""
    _, st = _trainer(NAME, lanes=lanes)
    st.forward_backward(*_inputs(NAME, 0))
    before = {k: v.cpu() for k, v in st.grads().items()}
    G0, G20 = st.G.clone(), (st.G2.clone() if lanes == 2 else None)
    host = [torch.nn.Parameter(torch.zeros_like(v)) for v in before.values()]
    for p, v in zip(host, before.values()):
        p.grad = v.clone()
    ref_norm = float(torch.nn.utils.clip_grad_norm_(host, 1e30))
    n0 = st.grad_norm()
    assert n0.dim() == 0 and n0.device.type == "cuda"
    print(f"clip lanes {lanes}: norm {float(n0):.9g} vs torch {ref_norm:.9g}, rel {abs(float(n0) - ref_norm) / ref_norm:.3e}")
    assert abs(float(n0) - ref_norm) / ref_norm < 1e-5
    assert same_bits(st.G, G0)                                              # the norm alone writes nothing
    max_norm = 0.5 * ref_norm
    torch.nn.utils.clip_grad_norm_(host, max_norm)
    ret = st.clip_grad_norm_(max_norm)
    assert same_bits(ret, n0)                                               # the norm from before clipping
    coef = st._gn[1].clone()
    assert 0.49 < float(coef) < 0.51
    assert same_bits(st.G, G0 * coef) and (lanes == 1 or same_bits(st.G2, G20 * coef))
    after = st.grads()
    for p, k in zip(host, before):
        # torch's coefficient comes from its own norm (within 1e-5 of the kernel's), one rounding per element on top
        assert rel(after[k], p.grad) < 1.1e-5 or float(p.grad.norm()) == 0.0, k
    # the clipped norm is max_norm up to the 1e-6 in the coefficient's denominator and the roundings above
    assert abs(float(st.grad_norm()) - max_norm) / max_norm < 1e-6 / ref_norm + 1e-5
    with pytest.raises(ValueError):
        st.clip_grad_norm_(0.0)


def test_train_step_grad_clip():
    """train_step(grad_clip=huge) leaves the parameters bit-equal to train_step() without it; a small threshold moves
    them differently (the clipped step is the one AdamW sees)."""
    outs = []
    for clip in (None, 1e30, 1e-3):
        _, st = _trainer(NAME)
        x0 = torch.randn(4, 4, 16, 16, generator=torch.Generator().manual_seed(9))
        for i in range(2):
            torch.manual_seed(50 + i)
            out = st.train_step(x0, torch.tensor([1, 4, 10, 0]), rng=np.random.RandomState(60 + i), grad_clip=clip)
        assert st.step == 2 and math.isfinite(float(out["loss"]))
        outs.append((st.P.cpu(), st.M.cpu()))
    assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1])
    assert not same_bits(outs[0][1], outs[2][1])
