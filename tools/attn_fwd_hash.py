"""sha256 of the forward attention's output bits at the lengths the shipped configs use (Dh 64 and 72, with and without
q_log2, a small and a many-heads batch).  Run from the repository root, once per build, and compare the BITS lines:
    python tools/attn_fwd_hash.py > new.log; PDM_LIB_PATH=path/to/other/libpdm.so python tools/attn_fwd_hash.py > old.log
(profiles/attn_fwd_bed/shipped_shape_hashes_*.log: the dispatcher refactoring against its parent)."""
import hashlib
import sys

import torch

sys.path.insert(0, ".")
from panopticdiffusionmodels_amd import _lib

for Dh in (64, 72):
    for L in (66, 257, 258, 334, 590, 1025, 1026, 1102):
        for B, H in ((2, 3), (40, 16)):
            for q_log2 in (True, False):
                g = torch.Generator().manual_seed(L * 100 + Dh + B)
                qkv = torch.randn(B * L, 3 * H * Dh, generator=g) * 1.5
                pos = torch.arange(B * L) % L
                qkv[:, H * Dh:2 * H * Dh] *= (1 + 3 * pos / L)[:, None]
                if q_log2:
                    qkv[:, :H * Dh] *= Dh ** -0.5 * 1.4426950408889634
                out = _lib.attention(qkv.bfloat16().cuda(), B, L, H, Dh, q_log2=q_log2)
                torch.cuda.synchronize()
                h = hashlib.sha256(out.cpu().view(torch.int16).numpy().tobytes()).hexdigest()[:24]
                print("BITS Dh %d L %d B %d H %d q_log2 %d %s" % (Dh, L, B, H, q_log2, h), flush=True)
