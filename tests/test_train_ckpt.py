"""Checkpoint formats of HipTrainState (panopticdiffusionmodels_amd/checkpoint.py) against the files the reference's
utils.TrainState.save wrote (tests/golden/ckpt_golden*.npz, made by tests/golden/make_ckpt_golden.py), the directory
choice of resume, and the argument checks of the gradient-norm entries.  No GPU."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ckpt_fixture import NAME, Fixture, jsonable  # noqa: E402

from panopticdiffusionmodels_amd import checkpoint, configs, weights  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return Fixture.get()


def _hyper(full):
    o = full["optimizer"]
    return dict(lr=o["lr"], betas=tuple(o["betas"]), eps=o.get("eps", 1e-8), weight_decay=o["weight_decay"])


def test_parameter_order_is_the_references(fx):
    for name, key in ((NAME, "names"), ("tiny_uvit_train_uncond", "uncond_names"), ("tiny_t2i_train", "t2i_names")):
        cfg = configs.get_config(name)["nnet"]
        order = checkpoint.param_order(cfg)
        assert [k for k, _ in order] == [str(k) for k in fx[key]], name
        sd = weights.nnet_state_dict(cfg, seed=0)
        assert all(tuple(sd[k].shape) == shape for k, shape in order)


def test_t2i_stateless_set_is_the_references(fx):
    from panopticdiffusionmodels_amd.train import stateless_params
    got = stateless_params(configs.get_config("tiny_t2i_train")["nnet"])
    assert got == {str(k) for k in fx["t2i_stateless"]} and len(got) > 0
    assert stateless_params(configs.get_config(NAME)["nnet"]) == set()


def test_optimizer_file_equals_the_reference_written_one(fx, tmp_path):
    full = configs.get_config(NAME)
    order = checkpoint.param_order(full["nnet"])
    ours = checkpoint.optimizer_state_dict(order, fx.exp_avg(), fx.exp_avg_sq(), fx.step, _hyper(full),
                                           full["lr_scheduler"]["warmup_steps"])
    ref = fx.optimizer_sd()
    assert list(ours) == list(ref) and len(ours["param_groups"]) == 1
    assert sorted(ours["state"]) == sorted(ref["state"])
    for i in ref["state"]:
        assert set(ours["state"][i]) == set(ref["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
        for key in ("step", "exp_avg", "exp_avg_sq"):
            a, b = ours["state"][i][key], ref["state"][i][key]
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (i, key)
    go, gr = ours["param_groups"][0], ref["param_groups"][0]
    assert set(go) == set(gr)
    for key in gr:
        assert go[key] == gr[key] and type(go[key]) is type(gr[key]), (key, go[key], gr[key])
    # through a file, read with the default torch.load, into torch.optim.AdamW over the oracle net's parameters
    torch.save(ours, tmp_path / "optimizer.pth")
    loaded = torch.load(tmp_path / "optimizer.pth", map_location="cpu")
    sd = weights.nnet_state_dict(full["nnet"], seed=11, init="random")
    params = [torch.nn.Parameter(sd[k].clone()) for k, _ in order]   # the oracle's net: uvit_ref.uvit_forward(sd, ...)
    opt = torch.optim.AdamW(params, lr=1.0)
    opt.load_state_dict(loaded)
    assert opt.param_groups[0]["betas"] == tuple(full["optimizer"]["betas"])
    assert opt.param_groups[0]["lr"] == float(fx["it3_lr"])
    assert torch.equal(opt.state[params[3]]["exp_avg"], fx.exp_avg()[order[3][0]])


def test_lr_scheduler_file_equals_the_reference_written_one(fx, tmp_path):
    full = configs.get_config(NAME)
    ours = checkpoint.lr_scheduler_state_dict(fx.step, _hyper(full), full["lr_scheduler"]["warmup_steps"])
    assert jsonable(ours) == fx.sched and ours["lr_lambdas"] == [None]
    torch.save(ours, tmp_path / "lr_scheduler.pth")
    loaded = torch.load(tmp_path / "lr_scheduler.pth", map_location="cpu")
    opt = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=full["optimizer"]["lr"])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: min(s / 5, 1))
    sched.load_state_dict(loaded)
    assert sched.last_epoch == 3 and sched.get_last_lr() == [float(fx["it3_lr"])]


def test_the_way_back_restores_every_bit(fx, tmp_path):
    full = configs.get_config(NAME)
    order = checkpoint.param_order(full["nnet"])
    path = fx.write_dir(str(tmp_path / "3.ckpt"))
    step, nnet_sd, ema_sd, opt_sd, sched_sd = checkpoint.read_dir(path)   # plain torch.load, default weights_only
    m, v, pstep, hyper = checkpoint.read_optimizer_state_dict(opt_sd, order)
    last_epoch, base_lr = checkpoint.read_lr_scheduler_state_dict(sched_sd)
    assert checkpoint.check_steps(step, pstep, last_epoch) == 3
    assert hyper == _hyper(full) and base_lr == full["optimizer"]["lr"]
    rm, rv = fx.exp_avg(), fx.exp_avg_sq()
    for k, shape in order:
        assert m[k].dtype == torch.float32 and tuple(m[k].shape) == shape
        assert torch.equal(m[k], rm[k]) and torch.equal(v[k], rv[k]), k
        assert torch.equal(nnet_sd[k], fx.nnet_sd()[k]) and torch.equal(ema_sd[k], fx.ema_sd()[k])
    # and the round trip through the product's writer
    out = str(tmp_path / "again.ckpt")
    checkpoint.write_dir(out, step, nnet_sd, ema_sd,
                         checkpoint.optimizer_state_dict(order, m, v, pstep, hyper, 5),
                         checkpoint.lr_scheduler_state_dict(last_epoch, hyper, 5))
    assert sorted(os.listdir(out)) == sorted(checkpoint.FILES)
    m2, v2, pstep2, hyper2 = checkpoint.read_optimizer_state_dict(checkpoint.read_dir(out)[3], order)
    assert pstep2 == 3 and hyper2 == hyper and all(torch.equal(m2[k], rm[k]) and torch.equal(v2[k], rv[k]) for k in rm)


def test_no_step_taken_is_an_empty_state():
    full = configs.get_config(NAME)
    order = checkpoint.param_order(full["nnet"])
    sd = checkpoint.optimizer_state_dict(order, {}, {}, 0, _hyper(full), 5)
    assert sd["state"] == {} and sd["param_groups"][0]["lr"] == 0.0
    m, v, pstep, _ = checkpoint.read_optimizer_state_dict(sd, order)
    assert m == {} and v == {} and pstep is None and checkpoint.check_steps(0, pstep, 0) == 0


def test_disagreeing_steps_raise(fx):
    with pytest.raises(ValueError, match=r"step\.pth = 4.*step = 3.*last_epoch = 3"):
        checkpoint.check_steps(4, 3, 3)
    with pytest.raises(ValueError, match=r"step\.pth = 3.*step = 2.*last_epoch = 3"):
        checkpoint.check_steps(3, 2, 3)
    with pytest.raises(ValueError, match=r"step\.pth = 3.*step = 3.*last_epoch = 7"):
        checkpoint.check_steps(3, 3, 7)
    with pytest.raises(ValueError):
        checkpoint.check_steps(3, None, 3)
    order = checkpoint.param_order(configs.get_config(NAME)["nnet"])
    sd = fx.optimizer_sd()
    sd["state"][5] = dict(sd["state"][5], step=torch.tensor(2.0))
    with pytest.raises(ValueError, match="steps differ"):
        checkpoint.read_optimizer_state_dict(sd, order)


def test_state_for_a_stateless_t2i_parameter_raises(fx):
    from panopticdiffusionmodels_amd.train import stateless_params
    full = configs.get_config("tiny_t2i_train")
    order = checkpoint.param_order(full["nnet"])
    stateless = stateless_params(full["nnet"])
    zeros = {k: torch.zeros(shape) for k, shape in order}
    sd = checkpoint.optimizer_state_dict(order, zeros, zeros, 2, _hyper(full), -1, stateless)
    names = [k for k, _ in order]
    assert {names[i] for i in sd["state"]} == set(names) - stateless
    checkpoint.read_optimizer_state_dict(sd, order, stateless)
    i = names.index("mask_embed_0.proj.weight")
    sd["state"][i] = {"step": torch.tensor(2.0), "exp_avg": zeros[names[i]], "exp_avg_sq": zeros[names[i]]}
    with pytest.raises(ValueError, match="mask_embed_0.proj.weight"):
        checkpoint.read_optimizer_state_dict(sd, order, stateless)


def test_resume_chooses_the_references_directory(tmp_path, monkeypatch):
    from panopticdiffusionmodels_amd.train import HipTrainState
    st = object.__new__(HipTrainState)   # resume is host logic; load is recorded, not run
    seen = []
    monkeypatch.setattr(HipTrainState, "load", lambda self, path, strict=True: seen.append(path))
    root = tmp_path / "ckpts"
    assert st.resume(str(root)) is False                       # missing root
    root.mkdir()
    assert st.resume(str(root)) is False                       # empty root
    (root / "notes.txt").write_text("x")
    assert st.resume(str(root)) is False and seen == []        # nothing named *.ckpt
    (root / "3.ckpt").mkdir()
    (root / "10.ckpt").mkdir()
    assert st.resume(str(root)) is True and seen[-1] == str(root / "10.ckpt")
    assert st.resume(str(root), step=3) is True and seen[-1] == str(root / "3.ckpt")
    best = tmp_path / "best_only"
    (best / "best.ckpt").mkdir(parents=True)
    assert st.resume(str(best)) is True and seen[-1] == str(best / "best.ckpt")
    assert checkpoint.resume_path(str(best)) == str(best / "best.ckpt")


# ---- the gradient-norm entries' argument checks: PDM_ERR_ARG before any launch, so no GPU is needed ---------------

def test_grad_norm_entries_reject_bad_arguments_before_launching():
    from panopticdiffusionmodels_amd import _lib
    from panopticdiffusionmodels_amd.native import cfg_struct
    lib = _lib.load()
    P = ctypes.c_void_p
    a, ARG, STATE = 4096, 1, 3          # an aligned, never dereferenced address
    big = _lib.GRAD_NORM_SCRATCH_BYTES
    gn = lib.pdm_grad_norm_clip
    assert gn(P(a + 4), None, 64, 1.0, P(a), P(a), big, None) == ARG        # misaligned gradients
    assert gn(P(a), P(a + 8), 64, 1.0, P(a), P(a), big, None) == ARG        # misaligned second lane
    assert gn(P(a), None, 0, 1.0, P(a), P(a), big, None) == ARG             # n <= 0
    assert gn(P(a), None, -5, 1.0, P(a), P(a), big, None) == ARG
    assert gn(None, None, 64, 1.0, P(a), P(a), big, None) == ARG            # null pointers
    assert gn(P(a), None, 64, 1.0, None, P(a), big, None) == ARG
    assert gn(P(a), None, 64, 1.0, P(a), None, 0, None) == ARG
    assert gn(P(a), None, 64, 1.0, P(a + 2), P(a), big, None) == ARG        # misaligned output
    assert gn(P(a), None, 4096, 1.0, P(a), P(a), 12, None) == ARG           # 4 blocks need 16 bytes of scratch
    assert b"scratch" in lib.pdm_last_error()
    assert gn(P(a), None, 1 << 40, 0.0, P(a), P(a), big - 4, None) == ARG   # the largest grid: 1024 partials
    # the trainer entry: a state error before the buffers are set, the same argument checks after
    kw = dict(configs.get_config(NAME)["nnet"])
    kw.pop("name")
    h = ctypes.c_void_p()
    _lib.check(lib.pdm_train_create(ctypes.byref(cfg_struct(kw, False)), ctypes.byref(h)))
    try:
        tn = lib.pdm_train_grad_norm
        assert tn(h, None, 1.0, P(a), P(a), big, None) == STATE
        _lib.check(lib.pdm_train_set_buffers(h, P(a), P(a), P(a), P(a)))
        assert tn(h, P(a + 4), 1.0, P(a), P(a), big, None) == ARG
        assert tn(h, None, 1.0, None, P(a), big, None) == ARG
        assert tn(h, None, 1.0, P(a), P(a), 16, None) == ARG                # 165120 floats: 162 blocks
        assert tn(h, None, 1.0, P(a), None, big, None) == ARG
        active = ctypes.c_longlong()
        _lib.check(lib.pdm_train_active(h, ctypes.byref(active)))
        n = ctypes.c_longlong()
        _lib.check(lib.pdm_train_sizes(h, ctypes.byref(n), None))
        assert active.value == n.value == 165120
        assert lib.pdm_train_active(h, None) == ARG
    finally:
        lib.pdm_train_destroy(h)
