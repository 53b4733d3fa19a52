"""Time the fused Euler-Maruyama sampler (dev tool):

    python tools/em_bench.py                          both cases below, each in a child process with its own time limit
    python tools/em_bench.py cifar [B [S ...]]        cifar10_uvit_small, 1000-step SDE, batch B (default: the config's
                                                      mini_batch_size), capture blocks S ... (default: the sampler's)
    python tools/em_bench.py imagenet [B [S ...]]     imagenet256_uvit_large, 50-step ODE with CFG 0.4

Per capture block it prints the first sample (warm-up + capture + run), the replayed sample and ms per step, then
the yardstick: ClassCondSampler's ms per model evaluation at the same config and batch (the same forward with an
epilogue of similar weight).
"""
import subprocess
import sys
import time

import torch

sys.path.insert(0, ".")
from panopticdiffusionmodels_amd import configs as C  # noqa: E402
from panopticdiffusionmodels_amd import weights as W  # noqa: E402
from panopticdiffusionmodels_amd.sampler import ClassCondSampler, EulerMaruyamaSampler  # noqa: E402
from panopticdiffusionmodels_amd.utils import get_nnet  # noqa: E402

CASES = {"cifar": ("cifar10_uvit_small", "sde", 1000, 600), "imagenet": ("imagenet256_uvit_large", "ode", 50, 300)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def run(case, B=None, blocks=()):
    name, kind, steps, _ = CASES[case]
    full = C.get_config(name)
    cfg = full["nnet"]
    dev = torch.device("cuda")
    net = get_nnet(**cfg)
    net.load_state_dict(W.nnet_state_dict(cfg, seed=0, init="reference"))
    net = net.to(dev).eval()
    B = B or full["mini_batch_size"]
    g = torch.Generator().manual_seed(1)
    z = torch.randn(B, *full["z_shape"], generator=g).to(dev)
    cond = cfg.get("num_classes", -1) > 0
    y = torch.randint(0, cfg["num_classes"] - 1, (B,), generator=g).to(dev) if cond else None
    kw = dict(cfg_scale=full["cfg_scale"], null_label=cfg["num_classes"] - 1 if cond else None)
    for S in blocks or (None,):
        s = EulerMaruyamaSampler(net, kind=kind, steps=steps, capture_block=S, **kw)
        first, _ = timed(lambda: s.sample(z, y))
        again, out = min((timed(lambda: s.sample(z, y)) for _ in range(2)), key=lambda r: r[0])
        print(f"{name} B={B} {kind} {steps} steps, capture block {s.capture_block}: first sample {first*1e3:.0f} ms, "
              f"replayed {again*1e3:.1f} ms = {again/steps*1e3:.4f} ms/step, finite={bool(torch.isfinite(out).all())}",
              flush=True)
    d = ClassCondSampler(net, front_end=full["front_end"], steps=50, eps=full.get("eps"), **kw)
    d.sample(z, y)
    t, _ = min((timed(lambda: d.sample(z, y)) for _ in range(3)), key=lambda r: r[0])
    print(f"{name} B={B} yardstick ClassCondSampler: {t*1e3:.1f} ms / {d.nfe} NFE = {t/d.nfe*1e3:.4f} ms/NFE", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1:
        a = sys.argv[2:]
        run(sys.argv[1], int(a[0]) if a else None, tuple(int(v) for v in a[1:]))
    else:
        for case, (_, _, _, limit) in CASES.items():   # a fresh process per case; stop at the first failure
            subprocess.run([sys.executable, __file__, case], timeout=limit, check=True)
