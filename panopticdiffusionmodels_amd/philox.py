"""Host model (numpy) of the device noise generator of the Euler-Maruyama sampler (csrc/sampler_em.hip).

Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants),
keyed and counted so that a sample's noise depends on nothing but (seed, global sample index, step, element):

  key     = (seed & 0xffffffff, seed >> 32)
  counter = (quad index within the sample, step index, global sample index low, global sample index high)
  element o of a sample = output word o & 3 of quad o >> 2
  u       = ((r >> 8) + 0.5) * 2^-24                          (0 < u <= 1)
  normals = Box-Muller on the word pairs (0, 1) and (2, 3):
            n_a = sqrt(-2 ln u_a) cos(2 pi u_b),  n_b = sqrt(-2 ln u_a) sin(2 pi u_b)

The device evaluates u and the Box-Muller transform in fp32; this model evaluates them in float64 from the same
words, so `philox_words` is bit-exact against the device and `philox_normal` is its exact-arithmetic reference.
"""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32(counter, key, rounds=10):
    """counter: 4 uint32 arrays (broadcastable), key: 2 uint32 values / arrays -> 4 uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & _LO for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (int(key[0]) & 0xFFFFFFFF), (int(key[1]) & 0xFFFFFFFF)
    for _ in range(rounds):
        p0 = _M0 * c[0]
        p1 = _M1 * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ np.uint64(k0), p1 & _LO, (p0 >> _S32) ^ c[3] ^ np.uint64(k1), p0 & _LO]
        k0 = (k0 + _W0) & 0xFFFFFFFF
        k1 = (k1 + _W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def _quads(B, per_sample, seed, sample_offset, step):
    """The Philox outputs of every quad of B samples: uint32 [B, ceil(per_sample / 4), 4]."""
    nq = (per_sample + 3) // 4
    q = np.arange(nq, dtype=np.uint64)[None, :]
    sample = [(int(sample_offset) + b) & 0xFFFFFFFFFFFFFFFF for b in range(B)]
    lo = np.array([s & 0xFFFFFFFF for s in sample], dtype=np.uint64)[:, None]
    hi = np.array([s >> 32 for s in sample], dtype=np.uint64)[:, None]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    out = philox4x32((q, np.uint64(int(step) & 0xFFFFFFFF), lo, hi), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(out, axis=-1)


def philox_words(B, per_sample, seed=0, sample_offset=0, step=0):
    """The raw 32-bit word of every element: uint32 [B, per_sample]."""
    return _quads(B, per_sample, seed, sample_offset, step).reshape(B, -1)[:, :per_sample].copy()


def philox_normal(B, per_sample, seed=0, sample_offset=0, step=0, dtype=np.float64):
    """The standard normals the device draws for step `step` of samples sample_offset .. sample_offset + B - 1:
    [B, per_sample], evaluated in float64 (module docstring) and returned as `dtype`."""
    r = _quads(B, per_sample, seed, sample_offset, step)
    u = ((r >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    n = np.empty(u.shape, dtype=np.float64)
    for a in (0, 2):
        rad = np.sqrt(-2.0 * np.log(u[..., a]))
        ang = 2.0 * np.pi * u[..., a + 1]
        n[..., a] = rad * np.cos(ang)
        n[..., a + 1] = rad * np.sin(ang)
    return n.reshape(B, -1)[:, :per_sample].astype(dtype)
