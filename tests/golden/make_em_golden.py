"""Generate tests/golden/em_golden.npz by running the REFERENCE's own sde.euler_maruyama (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_em_golden.py REFERENCE_CHECKOUT

The reference is imported read-only exactly as make_golden.py imports it.  The net is the reference's libs.uvit.UViT
at the tiny_uvit_cond shape with this repo's seeded weights, wrapped in the CFG closure of eval_ldm.py:66-74; the
sampler is sde.euler_maruyama on the CPU (sde.py:243-267), 12 steps, B = 3:

  ode/z          the ODE result                      (eval_ldm.py:91-92)
  sde/z          the ReverseSDE result under torch.manual_seed(SDE_SEED) with the CPU generator (eval_ldm.py:89-90)
  z_init, y      the inputs;  sd_checksum the weights checksum (make_golden._sd_checksum)
  steps/s, t     the grid values of each step, in the order the steps run (fp32, as the reference holds them)
  steps/beta     the drift coefficient squared_diffusion(t) the reference multiplied x by (f = -beta x / 2)
  steps/g2       diffusion(t) ** 2, what it multiplied the score by (beta up to an fp32 rounding)
  steps/rsqrt_cum_beta   cum_beta(t).rsqrt(), the score's scale (fp32; cancellation near t = eps included)
  steps/sigma    the noise scale diffusion * sqrt(-dt) of each step of the ReverseSDE run

These are recorded from the reference's own scalar-tensor products (sde.stp is wrapped to note its scalar
argument: per step it is called with beta, -rsqrt(cum_beta), g2 and, when s != 0, sigma).  The
last step's sigma is computed but not used by the reference (s == 0); it is stored as the same fp32 expression.
The .npz holds data only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402

C, W = MG.C, MG.W
NAME, B, STEPS, INPUT_SEED, SDE_SEED = "tiny_uvit_cond", 3, 12, 31, 1234


def gen_em(mods, out):
    uvit, sde = mods[0], mods[5]
    cfg = C.nnet_kwargs(NAME)
    sd = W.nnet_state_dict(cfg, seed=11, init="random")
    kw = dict(cfg)
    kw.pop("name")
    net = uvit.UViT(**kw)
    net.load_state_dict(sd)
    net.eval()
    inp = MG._inputs(NAME, B, seed=INPUT_SEED)
    null = cfg["num_classes"] - 1
    scale = C.get_config(NAME)["cfg_scale"]

    def cfg_nnet(x, timesteps, y):
        _cond = net(x, timesteps, y=y)
        _uncond = net(x, timesteps, y=torch.tensor([null] * x.size(0)))
        return _cond + scale * (_cond - _uncond)
    score_model = sde.ScoreModel(cfg_nnet, pred="noise_pred", sde=sde.VPSDE())

    z_ode = sde.euler_maruyama(sde.ODE(score_model), inp["x"].clone(), STEPS, y=inp["y"])

    scalars = []
    ref_stp = sde.stp

    def noting_stp(s, ts):
        scalars.append(float(s) if not isinstance(s, np.ndarray) else float(s.reshape(-1)[0]))
        return ref_stp(s, ts)
    sde.stp = noting_stp
    try:
        torch.manual_seed(SDE_SEED)
        trace = []
        z_sde = sde.euler_maruyama(sde.ReverseSDE(score_model), inp["x"].clone(), STEPS, trace=trace, y=inp["y"])
    finally:
        sde.stp = ref_stp
    assert len(scalars) == 4 * STEPS - 1 and len(trace) == STEPS + 1, (len(scalars), len(trace))

    ts = torch.tensor(np.append(0., np.linspace(1e-3, 1, STEPS))).to(inp["x"])   # sde.py:251-252
    pairs = list(zip(ts, ts[1:]))[::-1]
    rec = {k: [] for k in ("s", "t", "beta", "g2", "rsqrt_cum_beta", "sigma")}
    for k, (s, t) in enumerate(pairs):
        beta, nrs, g2 = scalars[4 * k: 4 * k + 3]
        rec["s"].append(float(s))
        rec["t"].append(float(t))
        rec["beta"].append(beta)
        rec["g2"].append(g2)
        rec["rsqrt_cum_beta"].append(-nrs)
        if k < STEPS - 1:
            rec["sigma"].append(scalars[4 * k + 3])
        else:
            rec["sigma"].append(float(sde.VPSDE().diffusion(t) * (-(s - t)).sqrt()))
    out["z_init"] = MG._np(inp["x"])
    out["y"] = MG._np(inp["y"])
    out["sd_checksum"] = MG._sd_checksum(sd)
    out["ode/z"] = MG._np(z_ode)
    out["sde/z"] = MG._np(z_sde)
    out["sde/seed"] = np.array(SDE_SEED)
    out["cfg_scale"] = np.array(scale)
    for k, v in rec.items():
        out[f"steps/{k}"] = np.array(v, dtype=np.float32)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    mods = MG._import_reference(ref)
    out = {}
    with torch.no_grad():
        gen_em(mods, out)
    path = os.path.join(HERE, "em_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
