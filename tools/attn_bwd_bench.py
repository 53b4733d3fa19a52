"""The attention backward's two paths against each other (dev tool).

    python tools/attn_bwd_bench.py [--repeats 5] [--iters 20] [--warmup 5]

algo 1 = the head-in-LDS kernels (one workgroup per (sequence, head); Dh 64: L <= 608, Dh 72: L <= 415), algo 2 = the
streaming kernels (one workgroup per (sequence, head, 128 rows), three launches).  At the shapes both take, each
repeat times `iters` back-to-back calls of one, then of the other, between device events, the order alternating from
repeat to repeat; the streaming kernels alone at the 512^2 t2i lengths (L 1102 / 2126, B * H = 64).  Prints one JSON
line per shape: microseconds per call, mean and min .. max over the repeats, so the spread is visible.
"""
import argparse
import ctypes
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from panopticdiffusionmodels_amd import _lib  # noqa: E402

BOTH = [(64, 64, 258, 16), (64, 32, 334, 8), (64, 32, 590, 8), (72, 64, 258, 16)]   # Dh, B, L, H
STREAM_ONLY = [(64, 8, 1102, 8), (64, 8, 2126, 8), (72, 8, 1026, 8)]


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def stats(v):
    return dict(mean=round(sum(v) / len(v), 1), min=round(min(v), 1), max=round(max(v), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda")
    for Dh, B, L, H in BOTH + STREAM_ONLY:
        g = torch.Generator().manual_seed(L)
        qkv = (torch.randn(B * L, 3 * H * Dh, generator=g) * 1.5).bfloat16().to(dev)
        dout = torch.randn(B * L, H * Dh, generator=g).bfloat16().to(dev)
        o = _lib.attention(qkv, B, L, H, Dh)
        out = torch.empty_like(qkv)
        nbytes = ctypes.c_size_t(0)
        _lib.check(_lib.load().pdm_attention_backward_scratch_size(B, L, H, Dh, ctypes.byref(nbytes)))
        scratch = torch.empty(nbytes.value // 4, dtype=torch.float32, device=dev)
        algos = [1, 2] if (Dh, B, L, H) in BOTH else [2]
        fns = {a: (lambda a=a: _lib.attention_backward(qkv, o, dout, B, L, H, Dh, algo=a, out=out, scratch=scratch))
               for a in algos}
        for fn in fns.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        us = {a: [] for a in algos}
        for r in range(args.repeats):
            for a in (algos if r % 2 == 0 else algos[::-1]):
                us[a].append(timed(fns[a], args.iters))
        # S, dP, dV, dK, dQ: 5 products of 2 L^2 Dh (the streaming kernels recompute S twice more: 7 executed)
        flop = 5 * 2.0 * B * H * L * L * Dh
        line = dict(Dh=Dh, B=B, L=L, H=H, repeats=args.repeats, iters=args.iters)
        for a in algos:
            line["head_in_lds_us" if a == 1 else "streaming_us"] = stats(us[a])
            line["head_in_lds_tflops" if a == 1 else "streaming_tflops"] = round(flop / (sum(us[a]) / len(us[a])) / 1e6, 1)
        if len(algos) == 2:
            line["streaming_over_head_in_lds"] = round(sum(us[2]) / sum(us[1]), 3)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
