"""One family of eager (uncaptured) B = 2 forwards, for two measurements of the forward drivers' host code:

    python tools/forward_eager.py <class|fp8|two_stream|joint> <bf16|fp32>     # ONE forward: run it under
        rocprofv3 --kernel-trace and turn the trace into the ordered launch list with --list (below)
    python tools/forward_eager.py class bf16 --time 200     # median wall time of 200 forwards after warm-up,
        launches only (host-bound) and with a device sync after each; one line per repetition (3)
    python tools/forward_eager.py --list <kernel_trace.csv>  # (kernel name, grid, workgroup) per dispatch, in order

PDM_LIB_PATH names another build of the library; equal lists from two builds mean that neither reordered nor
regrouped a launch."""
import csv
import os
import statistics
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if sys.argv[1] == "--list":
    rows = sorted(csv.DictReader(open(sys.argv[2])), key=lambda r: int(r["Dispatch_Id"]))
    for r in rows:
        if "pdm::" in r["Kernel_Name"]:   # the library's kernels (not torch's copies and fills)
            print(r["Kernel_Name"], "grid", r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"], "wg",
                  r["Workgroup_Size_X"], r["Workgroup_Size_Y"], r["Workgroup_Size_Z"])
    sys.exit(0)

import torch
from panopticdiffusionmodels_amd import configs as C, weights as W
from panopticdiffusionmodels_amd.utils import get_nnet
family, residual = sys.argv[1], sys.argv[2]
cfg = {"class": C.nnet_kwargs("tiny_uvit_cond"),
       "fp8": dict(name="uvit", img_size=16, patch_size=2, in_chans=4, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4,
                   qkv_bias=False, mlp_time_embed=False, num_classes=11),
       "two_stream": C.nnet_kwargs("tiny_t2i"), "joint": C.nnet_kwargs("tiny_t2i_joint")}[family]
dev = torch.device("cuda:0")
net = get_nnet(**cfg)
net.load_state_dict(W.nnet_state_dict(cfg, seed=3, init="random"))
net = net.to(dev).eval().set_residual(residual)
if family == "fp8":
    net.set_precision("fp8")
g = torch.Generator().manual_seed(1)
x = torch.randn(2, 4, 16, 16, generator=g).to(dev)
t = (torch.rand(2, generator=g) * 999 + 1).to(dev)
if cfg["name"] == "uvit":
    args, kw = (x, t, torch.tensor([3, 10]).to(dev)), {}
else:
    args = (x, t, torch.randn(2, 5, 64, generator=g).to(dev))
    kw = dict(mask_token=torch.randn(2, 8, 16, 16, generator=g).to(dev))
with torch.no_grad():
    if "--time" not in sys.argv:
        net.forward_pre(*args, **kw)
        torch.cuda.synchronize()
        sys.exit(0)
    n = int(sys.argv[sys.argv.index("--time") + 1])
    for rep in range(3):
        med = []
        for sync in (False, True):
            for _ in range(20):
                net.forward_pre(*args, **kw)
            torch.cuda.synchronize()
            ts = []
            for _ in range(n):
                t0 = time.perf_counter()
                net.forward_pre(*args, **kw)
                if sync:
                    torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            med.append(statistics.median(ts) * 1e6)
        print(f"{family} residual={residual} rep {rep}: median of {n} eager forwards {med[0]:.1f} us launches only, "
              f"{med[1]:.1f} us with a sync after each")
