"""Forward time of mscoco_uvit_small_joint beside mscoco_uvit_small (separate streams) at 32 rows (the t2i bench's rows
per lane): HIP events around forward_pre after warm-up, the two nets alternated; then the per-GEMM split of one joint
forward (pdm_uvit_profile).

    python tools/t2i_joint_time.py
"""
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from panopticdiffusionmodels_amd import _lib, configs as C, weights as W
from panopticdiffusionmodels_amd.utils import get_nnet
dev = torch.device("cuda:0")
ROWS, REPS, INNER = 32, 7, 20
def net(name):
    cfg = C.nnet_kwargs(name)
    n = get_nnet(**cfg); n.load_state_dict(W.nnet_state_dict(cfg, seed=0, init="reference"))
    return n.to(dev).eval()
g = torch.Generator().manual_seed(1)
x = torch.randn(ROWS, 4, 32, 32, generator=g).to(dev); t = (torch.rand(ROWS, generator=g) * 999 + 1).to(dev)
ctx = torch.randn(ROWS, 77, 768, generator=g).to(dev); mt = torch.randn(ROWS, 8, 32, 32, generator=g).to(dev)
nets = {"joint": net("mscoco_uvit_small_joint"), "separate": net("mscoco_uvit_small")}
out = torch.empty(ROWS, 4, 32, 32, device=dev); mout = torch.empty(ROWS, 8, 32, 32, device=dev)
def run(n, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        n.forward_pre(x, t, ctx, mt, out=out, mask_out=mout)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / k
with torch.no_grad():
    for n in nets.values():
        run(n, 10)
    res = {k: [] for k in nets}
    for r in range(REPS):
        for k in (("joint", "separate") if r % 2 == 0 else ("separate", "joint")):
            res[k].append(run(nets[k], INNER))
    for k, v in res.items():
        print(f"forward_pre {k:9s} rows {ROWS} with mask: mean {statistics.mean(v):.4f} ms, min {min(v):.4f}, max {max(v):.4f}, "
              f"stdev {statistics.stdev(v):.4f} ({REPS} repeats of {INNER} forwards, alternated) :: " + " ".join(f"{a:.4f}" for a in v))
    # the plain (no mask token) forward of both nets: the same kernels at Lx
    for k, n in nets.items():
        n.forward_pre(x, t, ctx, out=out)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            n.forward_pre(x, t, ctx, out=out)
        e1.record(); torch.cuda.synchronize()
        print(f"forward_pre {k:9s} rows {ROWS} without mask: {e0.elapsed_time(e1) / INNER:.4f} ms")
    # per-GEMM split of one joint forward (pdm_uvit_profile: HIP events around every GEMM launch)
    n = nets["joint"]
    prof = _lib.GemmProfiler(n.native(), max_launches=512)
    prof.enable()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); n.forward_pre(x, t, ctx, mt, out=out, mask_out=mout); e1.record(); torch.cuda.synchronize()
    ms, fl = prof.read(); prof.disable()
    D, Hid, M = 512, 2048, ROWS * 590
    kinds = {2.0 * M * 3 * D * D: "qkv", 2.0 * M * D * D: "proj", 2.0 * M * Hid * D: "fc1/fc2", 2.0 * M * D * 2 * D: "skip_linear",
             2.0 * ROWS * 77 * D * 768: "context_embed"}
    agg = {}
    for a, f in zip(ms, fl):
        k = kinds.get(f, f"other({f:.3g})")
        c = agg.setdefault(k, [0, 0.0, 0.0]); c[0] += 1; c[1] += a; c[2] += f
    tot = e0.elapsed_time(e1)
    print(f"profiled joint forward (events on): {tot:.4f} ms wall, {len(ms)} GEMM launches, {sum(ms):.4f} ms in GEMMs")
    for k, (cnt, a, f) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        print(f"  {k:14s} {cnt:3d} launches {a:8.4f} ms  {f / a / 1e9:8.1f} TFLOP/s")
    print(f"  attention (13 launches), assembly, row stats, final norm, heads, gaps: {tot - sum(ms):.4f} ms")
