"""Time the global gradient norm / clip launch (pdm_grad_norm_clip) on a flat buffer the size of a config's trainer.

    python tools/grad_norm_bench.py [--config imagenet256_uvit_large] [--reps 200]

Prints one JSON line: microseconds per call (device events over `reps` back-to-back calls after a warm-up) and the
bytes the algorithm needs over that time, for the norm alone, a step that does not clip (the norm pass plus the
scale kernel's early return) and a step that clips (one more read and a write), with one and with two lanes."""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from panopticdiffusionmodels_amd import _lib, configs  # noqa: E402
from panopticdiffusionmodels_amd.native import cfg_struct  # noqa: E402


def trainer_elements(name):
    kw = dict(configs.get_config(name)["nnet"])
    t2i = kw.pop("name") == "uvit_t2i"
    lib = _lib.load()
    h, n = ctypes.c_void_p(), ctypes.c_longlong()
    _lib.check(lib.pdm_train_create(ctypes.byref(cfg_struct(kw, t2i)), ctypes.byref(h)), "pdm_train_create")
    _lib.check(lib.pdm_train_active(h, ctypes.byref(n)), "pdm_train_active")
    lib.pdm_train_destroy(h)
    return n.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="imagenet256_uvit_large")
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    n = trainer_elements(a.config)
    _lib.require_gpu()
    dev = torch.device("cuda")
    out = torch.zeros(2, device=dev)
    scratch = torch.empty(_lib.GRAD_NORM_SCRATCH_BYTES // 4, device=dev)
    res = dict(config=a.config, elements=n, reps=a.reps)
    for lanes in (1, 2):
        g = torch.randn(n, device=dev)
        g2 = torch.randn(n, device=dev) if lanes == 2 else None
        # clip: a threshold that shrinks by 0.1 % per call, so every call finds coef ~ 0.999 < 1 and the scale kernel
        # runs (a fixed threshold clips once and never again)
        for what, max_norm, decay, passes in (("norm", 0.0, 1.0, 1), ("no_clip", 1e30, 1.0, 1), ("clip", 1.0, 0.999, 3)):
            for _ in range(5):
                max_norm *= decay
                _lib.grad_norm_clip(g, g2, n, max_norm, out, scratch)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.reps):
                max_norm *= decay
                _lib.grad_norm_clip(g, g2, n, max_norm, out, scratch)
            t1.record()
            torch.cuda.synchronize()
            us = t0.elapsed_time(t1) * 1e3 / a.reps
            res[f"{what}_lanes{lanes}_coef"] = round(float(out[1]), 6)   # the last call's: < 1 iff it clipped
            res[f"{what}_lanes{lanes}_us"] = round(us, 1)
            res[f"{what}_lanes{lanes}_TBps"] = round(passes * lanes * n * 4 / (us * 1e-6) / 1e12, 2)
        del g, g2
    print(json.dumps(res))


if __name__ == "__main__":
    main()
