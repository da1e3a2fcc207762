"""numpy replay of the library's in-kernel standard-normal stream (social_stgcnn_amd/csrc/philox.hpp): Philox4x32-10
keyed by the 64-bit seed, counter (lane, draw, 0, 'STGN'), Box-Muller on the top 24 bits of the first two words.  The
kernels use lane = scene * V + ped (V the padded width) and draw = k * P + t.  Shared by test_sampling_cpu.py and
test_gpu_sampling.py."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(lane, draw, seed):
    """The four output words for counters (lane, draw) (broadcast uint64 / uint32 arrays) under `seed`."""
    lane = np.asarray(lane, dtype=np.uint64)
    draw = np.asarray(draw, dtype=np.uint64)
    lane, draw = np.broadcast_arrays(lane, draw)
    c0 = (lane & MASK).astype(np.uint32)
    c1 = (lane >> np.uint64(32)).astype(np.uint32)
    c2 = draw.astype(np.uint32)
    c3 = np.full(c0.shape, 0x5354474E, dtype=np.uint32)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32)
    with np.errstate(over="ignore"):
        for _ in range(10):
            p0 = M0 * c0.astype(np.uint64)
            p1 = M1 * c2.astype(np.uint64)
            hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), (p0 & MASK).astype(np.uint32)
            hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), (p1 & MASK).astype(np.uint32)
            c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
            k0 = np.uint32(k0 + W0)
            k1 = np.uint32(k1 + W1)
    return c0, c1, c2, c3


def normal2(lane, draw, seed):
    """(z0, z1) float64 arrays: the two standard normals the kernel draws for (lane, draw).  The uniforms and the
    angle are the kernel's float32 values; log / sqrt / sin / cos in float64 (the device's differ by an ulp or so)."""
    c0, c1, _, _ = philox4x32_10(lane, draw, seed)
    u0 = ((c0 >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    u1 = ((c1 >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    r = np.sqrt(-2.0 * np.log(u0.astype(np.float64)))
    a = (np.float32(6.28318530717958647692) * u1).astype(np.float64)
    return r * np.cos(a), r * np.sin(a)


def noise_tensor(seed, k, n, p, v, scenes=None):
    """The (K,N,P,V,2) standard normals the kernels draw in place of a caller-provided noise tensor (`scenes`: only
    these scene indices of the batch, in that order)."""
    scenes = np.arange(n) if scenes is None else np.asarray(scenes)
    kk, nn, tt, vv = np.meshgrid(np.arange(k), scenes, np.arange(p), np.arange(v), indexing="ij")
    z0, z1 = normal2(nn.astype(np.uint64) * np.uint64(v) + vv.astype(np.uint64), kk * p + tt, seed)
    return np.stack([z0, z1], axis=-1)
