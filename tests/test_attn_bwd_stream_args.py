"""The streaming attention backward's entry points and the trainer's lifted token limit, without a GPU: the
declarations, the scratch size, the argument checks (PDM_ERR_ARG before any launch, with never-dereferenced pointers
as in tests/test_train_kernel_refs.py), and pdm_train_create / pdm_train_workspace_size on the long-sequence configs.
"""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p
A = 4096          # an aligned, never dereferenced address
OK, ARG = 0, 1


@pytest.fixture(scope="module")
def lib():
    from panopticdiffusionmodels_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpdm.so not built")
    return _lib.load()


def _scratch_size(lib, B, L, H, Dh):
    n = ctypes.c_size_t(0)
    assert lib.pdm_attention_backward_scratch_size(B, L, H, Dh, ctypes.byref(n)) == OK
    return n.value


def test_symbols_declared_and_exported(lib):
    with open(os.path.join(REPO, "include", "pdm.h")) as f:
        header = f.read()
    for name in ("pdm_attention_backward_scratch_size", "pdm_attention_backward_ex"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name


def test_scratch_size_covers_two_floats_per_query_and_grows_with_L(lib):
    prev = 0
    for L in (1, 17, 127, 128, 129, 608, 609, 1102, 2126, 100000):
        for B, H, Dh in ((1, 1, 64), (2, 8, 64), (3, 16, 72)):
            assert _scratch_size(lib, B, L, H, Dh) >= 2 * B * H * L * 4, (B, L, H, Dh)
        n = _scratch_size(lib, 2, L, 8, 64)
        assert n >= prev, L
        prev = n
    n = ctypes.c_size_t(0)
    assert lib.pdm_attention_backward_scratch_size(1, 0, 1, 64, ctypes.byref(n)) == ARG
    assert lib.pdm_attention_backward_scratch_size(1, 16, 1, 48, ctypes.byref(n)) == ARG
    assert lib.pdm_attention_backward_scratch_size(1, 16, 1, 64, None) == ARG


def _ex(lib, B, L, H, Dh, algo, scratch=A, scratch_bytes=1 << 40):
    return lib.pdm_attention_backward_ex(P(A), P(A), P(A), P(A), B, L, H, Dh, algo, P(scratch), scratch_bytes, None)


def test_ex_rejects_bad_arguments_before_launching(lib):
    # the head-in-LDS kernels only, one past their limits
    assert _ex(lib, 1, 609, 1, 64, 1) == ARG
    assert b"608" in lib.pdm_last_error()
    assert _ex(lib, 1, 416, 1, 72, 1) == ARG
    # a scratch one byte short (automatic past the limit, and forced streaming below it); none at all; misaligned
    for B, L, H, Dh, algo in ((2, 1102, 2, 64, 0), (1, 416, 1, 72, 0), (2, 66, 1, 64, 2)):
        need = _scratch_size(lib, B, L, H, Dh)
        assert _ex(lib, B, L, H, Dh, algo, scratch_bytes=need - 1) == ARG, (B, L, H, Dh, algo)
        assert b"scratch" in lib.pdm_last_error()
        assert _ex(lib, B, L, H, Dh, algo, scratch=0, scratch_bytes=0) == ARG
        assert _ex(lib, B, L, H, Dh, algo, scratch=A + 4) == ARG
    # an unknown algo, a head dim without a kernel, empty shapes, a null tensor
    assert _ex(lib, 1, 66, 1, 64, 3) == ARG and _ex(lib, 1, 66, 1, 64, -1) == ARG
    assert b"algo" in lib.pdm_last_error()
    assert _ex(lib, 1, 66, 1, 32, 2) == ARG
    assert _ex(lib, 0, 66, 1, 64, 2) == ARG and _ex(lib, 1, 0, 1, 64, 2) == ARG
    assert lib.pdm_attention_backward_ex(None, P(A), P(A), P(A), 1, 66, 1, 64, 2, P(A), 1 << 40, None) == ARG


def test_old_entry_still_rejects_past_its_limits(lib):
    assert lib.pdm_attention_backward(P(A), P(A), P(A), P(A), 1, 609, 1, 64, None) == ARG
    assert b"pdm_attention_backward_ex" in lib.pdm_last_error()
    assert lib.pdm_attention_backward(P(A), P(A), P(A), P(A), 1, 416, 1, 72, None) == ARG


def _trainer(lib, name):
    from panopticdiffusionmodels_amd import configs
    from panopticdiffusionmodels_amd.native import cfg_struct
    kw = dict(configs.nnet_kwargs(name))
    t2i = kw.pop("name") == "uvit_t2i"
    h = ctypes.c_void_p()
    rc = lib.pdm_train_create(ctypes.byref(cfg_struct(kw, t2i)), ctypes.byref(h))
    assert rc == OK, (name, lib.pdm_last_error())
    return h


def _params(lib, h):
    out = {}
    buf = ctypes.create_string_buffer(256)
    for i in range(lib.pdm_train_param_count(h)):
        off, numel = ctypes.c_longlong(), ctypes.c_longlong()
        assert lib.pdm_train_param_info(h, i, buf, 256, ctypes.byref(off), ctypes.byref(numel)) == OK
        out[buf.value.decode()] = (off.value, numel.value)
    return out


def _workspace(lib, h, rows):
    n = ctypes.c_size_t(0)
    assert lib.pdm_train_workspace_size(h, rows, ctypes.byref(n)) == OK
    return n.value


def test_trainer_takes_the_long_sequence_configs(lib):
    h = _trainer(lib, "tiny_t2i_train_512")
    prm = _params(lib, h)
    assert prm["pos_embed"][1] == 1102 * 64 and prm["pos_embed_mask"][1] == 1024 * 64
    w1, w2 = _workspace(lib, h, 1), _workspace(lib, h, 2)
    # the streaming attention backward's scratch (the mask stream's, the larger) is part of the workspace
    assert w2 - w1 >= _scratch_size(lib, 2, 2126, 1, 64) - _scratch_size(lib, 1, 2126, 1, 64) > 0
    lib.pdm_train_destroy(h)
    h = _trainer(lib, "tiny_uvit_train_h_long")
    assert _params(lib, h)["pos_embed"][1] == 1026 * 576
    assert _workspace(lib, h, 2) > 0
    lib.pdm_train_destroy(h)
    h = _trainer(lib, "mscoco_uvit_small_512")
    assert _params(lib, h)["pos_embed"][1] == 1102 * 512
    lib.pdm_train_destroy(h)


def test_existing_configs_keep_their_workspace(lib):
    """Bytes of the commit before the streaming kernels: streams the head-in-LDS kernels take reserve no scratch."""
    want = {"tiny_t2i_train": {1: 76539648, 2: 85970176, 3: 95400960},
            "tiny_uvit_train_uncond": {2: 68472064},
            "tiny_uvit_train_h": {2: 77172224}}
    for name, rows in want.items():
        h = _trainer(lib, name)
        for r, nbytes in rows.items():
            assert _workspace(lib, h, r) == nbytes, (name, r)
        lib.pdm_train_destroy(h)


def test_trainer_states_the_bound_it_keeps(lib):
    """tokens * embed_dim must stay below 2^31 (32-bit row-group strides); the message and pdm.h say so."""
    from panopticdiffusionmodels_amd import configs
    from panopticdiffusionmodels_amd.native import cfg_struct
    kw = dict(configs.nnet_kwargs("tiny_uvit_train"))
    kw.pop("name")
    kw.update(img_size=2 * 5800, patch_size=2, embed_dim=64)      # 5800^2 tokens * 64 > 2^31
    h = ctypes.c_void_p()
    assert lib.pdm_train_create(ctypes.byref(cfg_struct(kw, False)), ctypes.byref(h)) == ARG
    assert b"2^31" in lib.pdm_last_error()
    with open(os.path.join(REPO, "include", "pdm.h")) as f:
        assert "tokens * embed_dim < 2^31" in f.read()


def test_configs_declare_the_512_entries():
    from panopticdiffusionmodels_amd import configs as C
    c = C.get_config("mscoco_uvit_small_512")
    assert c["z_shape"] == (4, 64, 64) and c["nnet"]["img_size"] == 64 and c["nnet"]["patch_size"] == 2
    assert c["mini_batch_size"] == 10 and c["train"]["batch_size"] == 8 and c["train"]["p_uncond"] == 0.1
    assert c["optimizer"]["betas"] == (0.9, 0.9) and c["scale_factor"] == 0.23010
    small = C.get_config("mscoco_uvit_small")["nnet"]
    for k in ("enable_panoptic", "separate", "num_panoptic_class", "use_ground_truth"):
        assert c["nnet"][k] == small[k], k
    assert {k: v for k, v in c["nnet"].items() if k != "img_size"} == {k: v for k, v in small.items() if k != "img_size"}
    t, t512 = C.get_config("tiny_t2i_train"), C.get_config("tiny_t2i_train_512")
    assert t512["nnet"] == dict(t["nnet"], img_size=64) and t512["z_shape"] == (4, 64, 64)
    h, hl = C.get_config("tiny_uvit_train_h"), C.get_config("tiny_uvit_train_h_long")
    assert hl["nnet"] == dict(h["nnet"], img_size=64) and hl["z_shape"] == (4, 64, 64)
