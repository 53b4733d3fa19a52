"""The joint image+mask sequence of the panoptic t2i U-ViT (`enable_panoptic=True, separate=False`: one block stack
over [time, context, N image patches, N mask patches], libs/uvit_t2i.py:397-399, 419-520 of the reference), no GPU:
the fp32 oracle against the reference's own outputs (tests/golden/joint_golden.npz, made by
tests/golden/make_joint_golden.py), the native handle's parameter table and workspace sizes, and the Python module.

Tolerance: oracle vs reference rel-L2 <= 1e-5, forwards and 50-NFE samples alike."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import joint_fixture as J  # noqa: E402

from oracle import solver_ref, uvit_ref  # noqa: E402
from panopticdiffusionmodels_amd import _lib, configs, native, weights  # noqa: E402
from panopticdiffusionmodels_amd.utils import get_nnet  # noqa: E402

JOINT = J.TINY + J.FULL


@pytest.fixture(scope="module")
def jg():
    return J.load()


@pytest.mark.parametrize("name", JOINT)
def test_oracle_forward_vs_reference(jg, name):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    kw, sd = J.state_dict(jg, name)
    i = J.forward_inputs(jg, name)
    with torch.no_grad():
        eps, pm = uvit_ref.uvit_t2i_forward(sd, kw, i["x"], i["t"], i["context"], mask_token=i["mask_token"])
        assert J.rel_l2(eps, jg[f"{name}/eps_mask"]) < 1e-5
        assert J.rel_l2(pm, jg[f"{name}/pred_mask"]) < 1e-5
        if name in J.TINY:
            eps = uvit_ref.uvit_t2i_forward(sd, kw, i["x"], i["t"], i["context"])
            assert J.rel_l2(eps, jg[f"{name}/eps_nomask"]) < 1e-5
            eps, y = uvit_ref.uvit_t2i_forward(sd, kw, i["x"], i["t"], i["context"], mask_token=i["mask_token"],
                                               use_ground_truth=True)
            assert J.rel_l2(eps, jg[f"{name}/eps_gt"]) < 1e-5
            assert y is i["mask_token"]


@pytest.mark.parametrize("name", ["tiny_t2i_joint", "mscoco_uvit_small_joint"])
def test_oracle_sample_vs_reference(jg, name):
    """50 NFE, CFG on eps and on the mask, through the project's host solver driving the oracle."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    kw, sd = J.state_dict(jg, name)
    i = J.sample_inputs(jg, name)

    def net(x, t, c, m=None):
        return uvit_ref.uvit_t2i_forward(sd, kw, x, t, c, mask_token=m)
    fn = solver_ref.cfg_t2i_closure(net, i["context"], i["empty"], configs.get_config(name)["cfg_scale"])
    with torch.no_grad():
        z, pm = solver_ref.pp_sample(fn, solver_ref.sd_betas(), i["x"].clone(), steps=50,
                                     mask_token=i["mask_token"].clone(), enable_mask_opt=True)
    assert J.rel_l2(z, jg[f"sample/{name}/z"]) < 1e-5
    assert J.rel_l2(pm, jg[f"sample/{name}/pred_mask"]) < 1e-5


def _create(kw, t2i=True):
    h = ctypes.c_void_p()
    _lib.check(_lib.load().pdm_uvit_create(ctypes.byref(native.cfg_struct(kw, t2i)), ctypes.byref(h)), "pdm_uvit_create")
    return h


def _ws(h, rows):
    ws = ctypes.c_size_t()
    _lib.check(_lib.load().pdm_uvit_workspace_size(h, rows, ctypes.byref(ws)), "pdm_uvit_workspace_size")
    return ws.value


@pytest.mark.parametrize("name", JOINT)
def test_create_and_param_table(name):
    """pdm_uvit_create takes the joint layout; its table is the joint parameter set of weights.uvit_t2i_spec."""
    lib = _lib.load()
    kw = configs.nnet_kwargs(name)
    assert kw.pop("name") == "uvit_t2i"
    h = _create(kw)
    shapes = {k: int(np.prod(s)) for k, s, _ in weights.uvit_t2i_spec(**kw)}
    D = kw["embed_dim"]
    N = (kw["img_size"] // kw["patch_size"]) ** 2
    Lm = 1 + kw["num_clip_token"] + 2 * N
    buf = ctypes.create_string_buffer(256)
    table = {}
    for i in range(lib.pdm_uvit_param_count(h)):
        dt, ne = ctypes.c_int(), ctypes.c_longlong()
        _lib.check(lib.pdm_uvit_param_info(h, i, buf, 256, ctypes.byref(dt), ctypes.byref(ne)))
        key = buf.value.decode()
        table[key] = ne.value
        # no separate-stream entry: no zero conv, no pos_embed_mask, no *_mask block stack (decoder_pred_mask, the
        # mask head both layouts have, is the one key with "_mask." in its name that belongs here)
        assert not key.startswith(("zero_convs", "pos_embed_mask")), key
        assert "_mask." not in key or key.startswith("decoder_pred_mask."), key
        if key.endswith((".ln_colsum", ".ln_bias")):   # fused-LayerNorm terms: one per output feature
            assert ne.value == shapes[key.rsplit(".", 1)[0] + ".weight"] // D
            continue
        assert key in shapes, key
        if key.startswith("decoder_pred"):
            assert ne.value >= shapes[key]
        else:
            assert ne.value == shapes[key], key
    assert table["pos_embed"] == Lm * D
    for key in ("mask_embed.proj.weight", "mask_embed.proj.bias", "decoder_pred_mask.weight", "decoder_pred_mask.bias"):
        assert key in table, key
    assert "mask_embed_0.proj.weight" not in table   # never used by the reference's forward either
    # a forward on a handle without registered weights: the state error, before any GPU call
    p16 = ctypes.c_void_p(16)
    for mt in (p16, None):
        st = lib.pdm_uvit_t2i_forward(h, p16, p16, p16, mt, 0, p16, p16, 1, p16, 1 << 40, None)
        assert st == 3 and b"not registered" in lib.pdm_last_error()
    lib.pdm_uvit_destroy(h)


def test_fp8_t2i_stays_rejected():
    kw = configs.nnet_kwargs("mscoco_uvit_small_joint")
    kw.pop("name")
    kw["fp8"] = True
    with pytest.raises(ValueError):
        _create(kw)


def test_mask_patch_width_check_kept():
    """patch_size^2 * num_panoptic_class <= 64 (the head / assembly tiles) holds for the joint layout too."""
    kw = configs.nnet_kwargs("tiny_t2i_joint")
    kw.pop("name")
    kw["num_panoptic_class"] = 17   # 68 > 64
    with pytest.raises(ValueError):
        _create(kw)


# pdm_uvit_workspace_size at rows (2, 100) of the library built from commit fed3cc2 (the parent of the joint layout)
PARENT_WS = {
    ("imagenet256_uvit_large", "bf16"): (24330752, 1216524800),
    ("imagenet256_uvit_large", "fp32"): (24330752, 1216524800),
    ("imagenet256_uvit_huge", "bf16"): (32131584, 1606569984),
    ("imagenet256_uvit_huge", "fp32"): (32131584, 1606569984),
    ("imagenet512_uvit_huge", "bf16"): (32131584, 1606569984),
    ("imagenet512_uvit_huge", "fp32"): (32131584, 1606569984),
    ("cifar10_uvit_small", "bf16"): (10015232, 500739584),
    ("cifar10_uvit_small", "fp32"): (10015232, 500739584),
    ("mscoco_uvit_small", "bf16"): (37622784, 1881126912),
    ("mscoco_uvit_small", "fp32"): (30247424, 1512361984),
    ("tiny_uvit_cond", "bf16"): (255488, 12752384),
    ("tiny_uvit_cond", "fp32"): (255488, 12752384),
    ("tiny_t2i", "bf16"): (775936, 38765056),
    ("tiny_t2i", "fp32"): (579072, 28929792),
    ("mscoco_uvit_small_512", "bf16"): (130593792, 6529677312),
    ("mscoco_uvit_small_512", "fp32"): (105892352, 5294608384),
}


@pytest.mark.parametrize("name,residual", sorted(PARENT_WS))
def test_existing_workspace_sizes_unchanged(name, residual):
    kw = configs.nnet_kwargs(name)
    t2i = kw.pop("name") == "uvit_t2i"
    kw["residual"] = residual
    h = _create(kw, t2i)
    assert (_ws(h, 2), _ws(h, 100)) == PARENT_WS[(name, residual)]
    _lib.load().pdm_uvit_destroy(h)


def _joint_ws(kw, r):
    """The layout rule: every buffer of the single stream holds r * Lm rows (the fp32 residual stream X, its bf16
    copy XB, the block-internal copy XT, the LayerNorm partials of both (T = ceil(D / 256) (sum, M2) pairs per row),
    QKV, the attention output, the MLP hidden, depth // 2 long skips), the head input r * 2N rows, then the embedded
    (fp32) and the bf16 context; no mask-stream buffer.  Each buffer starts on a 256-byte boundary."""
    D, Hid = kw["embed_dim"], int(kw["embed_dim"] * kw["mlp_ratio"])
    N = (kw["img_size"] // kw["patch_size"]) ** 2
    nctx, clip = kw["num_clip_token"], kw["clip_dim"]
    Lm = 1 + nctx + 2 * N
    M, T = r * Lm, (D + 255) // 256
    sizes = [M * D * 4, M * D * 2, M * D * 2, M * T * 8, M * T * 8, M * 3 * D * 2, M * D * 2, M * Hid * 2,
             (kw["depth"] // 2) * M * D * 2, r * 2 * N * D * 2, r * nctx * D * 4, r * nctx * clip * 2]
    return sum((s + 255) // 256 * 256 for s in sizes)


@pytest.mark.parametrize("name", JOINT)
@pytest.mark.parametrize("residual", ["bf16", "fp32"])
def test_joint_workspace_size(name, residual):
    lib = _lib.load()
    kw = configs.nnet_kwargs(name)
    kw.pop("name")
    kw["residual"] = residual
    h = _create(kw)
    hs = _create(dict(kw, separate=True))   # the same shape with separate streams
    for r in (1, 2, 100):
        assert _ws(h, r) == _joint_ws(kw, r)
        assert _ws(h, r) < _ws(hs, r)
    lib.pdm_uvit_destroy(h)
    lib.pdm_uvit_destroy(hs)


@pytest.mark.parametrize("name", JOINT)
def test_module_builds_and_loads_strictly(name):
    kw = configs.nnet_kwargs(name)
    net = get_nnet(**kw)
    assert net.enable_panoptic and not net.separate
    sd = weights.nnet_state_dict(kw, seed=0)
    assert set(net.state_dict()) == set(sd)
    net.load_state_dict(sd, strict=True)
    N = (kw["img_size"] // kw["patch_size"]) ** 2
    assert net.pos_embed.shape == (1, 1 + kw["num_clip_token"] + 2 * N, kw["embed_dim"])
    assert "reference_sample" in configs.get_config(name)


def test_new_config_shapes():
    """The token counts the issue names: Lx / Lm and the head dim of each new entry."""
    want = {"tiny_t2i_joint": (70, 134, 32), "tiny_t2i_joint64": (334, 590, 64),
            "mscoco_uvit_small_joint": (334, 590, 64), "mscoco_uvit_small_512_joint": (1102, 2126, 64),
            "mscoco_uvit_large": (334, 590, 64)}
    for name, (Lx, Lm, Dh) in want.items():
        kw = configs.nnet_kwargs(name)
        N = (kw["img_size"] // kw["patch_size"]) ** 2
        assert (1 + kw["num_clip_token"] + N, 1 + kw["num_clip_token"] + 2 * N, kw["embed_dim"] // kw["num_heads"]) == \
            (Lx, Lm, Dh)
    sep = configs.get_config("mscoco_uvit_small")
    jnt = configs.get_config("mscoco_uvit_small_joint")
    assert {k: v for k, v in jnt.items() if k != "nnet"} == {k: v for k, v in sep.items() if k != "nnet"}
    assert dict(jnt["nnet"], separate=True) == sep["nnet"]
    assert configs.get_config("mscoco_uvit_small_512_joint")["mini_batch_size"] == 10
    assert configs.get_config("mscoco_uvit_large")["mini_batch_size"] == 32
