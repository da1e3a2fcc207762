// risk: what a caller acts on, reduced from the K sampled trajectories without writing them out.  Per scene, over the
// K samples stg_sample_trajectories would write for the same arguments: in how many of them a pedestrian comes within
// `radius` of another one (per step, at any step, and with whom), and in how many a rectangle is occupied.  Integer
// counts only, so the result is bitwise repeatable.
//
// The work is not a stream: K * P * vi^2 / 2 distance tests per scene (1.95 M at vi = 128) on top of the sampler's
// draws.  One workgroup per scene, the K samples in passes of kb:
//   draw    lane = (kk, pedestrian): all P steps of one sample into the LDS image img[kk][t][v] (sample_draw.hpp's
//           draw, as in sample_traj_kernel).  The image is carved for kb samples of V pedestrians and laid out with
//           the scene's own width vi, so a scene of few pedestrians takes more samples per pass (kb * V / vi, up to
//           K): the draw is the long serial part, and it needs lanes
//   pairs   lane = unordered pair, enumerated by offset: item -> (d, i), j = (i + d) mod vi, d = 1 .. (vi-1)/2 for
//           every i, and d = vi/2 for i < vi/2 when vi is even -- every pair once, no idle half, and the lanes of a wave
//           read consecutive i and consecutive j (conflict-free 8-byte LDS reads).  A lane owns the same items in every
//           pass, so its pair counts are plain byte read-modify-writes in LDS; per-step hits are byte stores of 1 into
//           flags[kk][t][i], summed after the barrier
//   zones   lane = (kk, t, z) over the pedestrians and lane = (kk, v, z) over the steps, LDS integer atomics
// and at the end the accumulators go out with plain vector stores; partner is a row scan of the pair counts.
#include "common.hpp"
#include "sample_draw.hpp"

namespace stg {

namespace {

struct RiskPlan {
    int threads, kb;
    // byte offsets into the dynamic LDS block
    size_t o_img, o_zone, o_zcnt, o_zany, o_pedz, o_pc, o_conf, o_cany, o_flag, o_fany, total;
};

inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

// the LDS carve for one scene of width V; kb samples per pass
RiskPlan risk_plan(int P, int V, int K, int Z, bool pairs) {
    RiskPlan p;
    p.threads = V <= 32 ? 256 : (V <= 64 ? 512 : 1024);
    const size_t n_pair = pairs ? (size_t)V * (V - 1) / 2 : 0;
    size_t fixed = 0;
    p.o_zone = fixed, fixed += up16((size_t)Z * 16);
    p.o_zcnt = fixed, fixed += up16((size_t)P * Z * 4);
    p.o_zany = fixed, fixed += up16((size_t)P * Z * 4);
    p.o_pedz = fixed, fixed += up16((size_t)V * Z * 4);
    p.o_pc = fixed, fixed += up16(n_pair);
    p.o_conf = fixed, fixed += up16(pairs ? (size_t)P * V : 0);
    p.o_cany = fixed, fixed += up16(pairs ? (size_t)V : 0);
    const size_t img_k = (size_t)P * V * 8, flag_k = pairs ? (size_t)P * V : 0, fany_k = pairs ? up16(V) : 0;
    const size_t per_k = img_k + flag_k + fany_k;
    // as many samples per pass as fill the draw phase's lanes, inside a budget that keeps three of the smaller
    // workgroups on a CU (their 6 waves per SIMD are what the kernel's registers allow); a workgroup of 1,024 threads
    // has a CU to itself by registers, and half of its LDS
    const size_t budget = (p.threads == 1024 ? 76 : 53) * 1024;
    int kb = (int)((budget > fixed ? budget - fixed : 0) / per_k);
    const int fill = p.threads / V > 1 ? p.threads / V : 1;
    kb = kb < 1 ? 1 : kb;
    kb = kb > fill ? fill : kb;
    kb = kb > K ? K : kb;
    const int passes = (K + kb - 1) / kb;
    p.kb = (K + passes - 1) / passes;
    p.o_img = fixed, fixed += (size_t)p.kb * img_k;
    p.o_flag = fixed, fixed += up16((size_t)p.kb * flag_k);
    p.o_fany = fixed, fixed += (size_t)p.kb * fany_k;
    p.total = fixed;
    return p;
}

}  // namespace

struct RiskArgs {
    const float *pred;
    int64_t p_sn, p_sf, p_sp, p_sv;
    const float *obs_last;
    const int32_t *num_peds;
    const float *noise;
    uint64_t seed;
    const uint64_t *seed_dev;
    int N, P, V, K;
    float radius;
    const float *zones;
    int64_t z_sn;
    int Z;
    int32_t *conflict, *conflict_any, *partner, *pair, *zone_any, *zone_count, *ped_zone;
    int kb;
    uint32_t o_img, o_zone, o_zcnt, o_zany, o_pedz, o_pc, o_conf, o_cany, o_flag, o_fany, total;
};

// the pair item `it` of a scene of n pedestrians -> (i, j)
__device__ __forceinline__ void pair_of_item(int it, int n, int &i, int &j) {
    const int full = n * ((n - 1) >> 1);
    int d;
    if (it < full) {
        d = it / n;
        i = it - d * n;
        d += 1;
    } else {
        d = n >> 1;
        i = it - full;
    }
    j = i + d;
    j = j >= n ? j - n : j;
}
// the item that holds the unordered pair {i, j}, i != j
__device__ __forceinline__ int item_of_pair(int i, int j, int n) {
    int d = j - i;
    d = d < 0 ? d + n : d;
    const int h = (n - 1) >> 1;
    if (d <= h) return (d - 1) * n + i;
    if (d > n - 1 - h) return (n - d - 1) * n + j;          // the pair is listed from j with offset n - d
    return n * h + (i < j ? i : j);                          // n even, d == n / 2
}

__global__ __launch_bounds__(1024) void sample_risk_kernel(const RiskArgs a) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int n = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int P = a.P, V = a.V, K = a.K, Z = a.Z;
    const bool pairs = a.radius > 0.f;
    float2 *img = reinterpret_cast<float2 *>(lds + a.o_img);
    float4 *zone = reinterpret_cast<float4 *>(lds + a.o_zone);
    int *zcnt = reinterpret_cast<int *>(lds + a.o_zcnt), *zany = reinterpret_cast<int *>(lds + a.o_zany);
    int *pedz = reinterpret_cast<int *>(lds + a.o_pedz);
    unsigned char *pc = lds + a.o_pc, *conf = lds + a.o_conf, *cany = lds + a.o_cany;
    unsigned char *flag = lds + a.o_flag, *fany = lds + a.o_fany;

    uint64_t seed = a.seed;
    if (a.seed_dev) seed = *a.seed_dev;
    int vi = a.num_peds ? a.num_peds[n] : V;
    vi = vi < 0 ? 0 : (vi > V ? V : vi);
    const int n_item = pairs ? vi * (vi - 1) / 2 : 0;
    // the image and the flags are carved for a.kb samples of V pedestrians and laid out with the scene's own width, so
    // a small scene takes more samples per pass (the draw phase then has lanes to fill): kb * vi <= a.kb * V
    const int vs = vi > 0 ? vi : 1;
    const int kb = a.kb * V / vs < K ? a.kb * V / vs : K;
    const float r2 = a.radius * a.radius;

    // zero every accumulator and flag (everything but the image), then the scene's rectangles
    {
        uint32_t *w = reinterpret_cast<uint32_t *>(lds);
        const uint32_t lo = a.o_img / 4, hi = (a.o_img + (uint32_t)a.kb * P * V * 8) / 4, end = a.total / 4;
        for (uint32_t x = tid; x < end; x += nt)
            if (x < lo || x >= hi) w[x] = 0u;
    }
    __syncthreads();
    for (int z = tid; z < Z; z += nt) {
        const float *r = a.zones + n * a.z_sn + 4 * z;
        zone[z] = make_float4(r[0], r[1], r[2], r[3]);
    }

    for (int k0 = 0; k0 < K; k0 += kb) {
        const int kc = K - k0 < kb ? K - k0 : kb;
        // ---- draw: lane = (kk, v), the P steps of one sampled trajectory
        for (int it = tid; it < kc * vi; it += nt) {
            const int kk = it / vi, v = it - kk * vi, k = k0 + kk;
            const int64_t o = ((int64_t)n * V + v) * 2;
            const float ox = a.obs_last ? a.obs_last[o] : 0.f, oy = a.obs_last ? a.obs_last[o + 1] : 0.f;
            const float *nrow = a.noise ? a.noise + (((int64_t)k * a.N + n) * P * V + v) * 2 : nullptr;
            float cx = 0.f, cy = 0.f;
            for (int t = 0; t < P; ++t) {
                const float *q = a.pred + n * a.p_sn + v * a.p_sv + t * a.p_sp;
                const float mx = q[0], my = q[a.p_sf];
                const Chol2 l = draw_chol(q, a.p_sf);
                float2 e;
                if (nrow)
                    e = *reinterpret_cast<const float2 *>(nrow + (int64_t)t * V * 2);
                else
                    e = draw_normal2(seed, n, V, v, k, P, t);
                draw_step(cx, cy, mx, my, l, e);
                img[(kk * P + t) * vs + v] = make_float2(cx + ox, cy + oy);
            }
        }
        __syncthreads();
        // ---- pairs: lane = unordered pair, over the pass's samples and steps
        for (int it = tid; it < n_item; it += nt) {
            int i, j;
            pair_of_item(it, vi, i, j);
            int cnt = 0;
            for (int kk = 0; kk < kc; ++kk) {
                const float2 *row = img + kk * P * vs;
                unsigned char *frow = flag + kk * P * vs;
                bool any = false;
#pragma unroll 4
                for (int t = 0; t < P; ++t) {
                    const float2 pi = row[t * vs + i], pj = row[t * vs + j];
                    const float dx = pi.x - pj.x, dy = pi.y - pj.y;
                    if (dx * dx + dy * dy < r2) {
                        any = true;
                        frow[t * vs + i] = 1;
                        frow[t * vs + j] = 1;
                    }
                }
                if (any) {
                    ++cnt;
                    fany[kk * vs + i] = 1;
                    fany[kk * vs + j] = 1;
                }
            }
            pc[it] = (unsigned char)(pc[it] + cnt);
        }
        // ---- zones: lane = (kk, t, z) over the pedestrians; lane = (kk, v, z) over the steps
        if (Z > 0) {
            for (int it = tid; it < kc * P * Z; it += nt) {
                const int z = it % Z, kt = it / Z;                                   // kt = kk * P + t
                const float4 r = zone[z];
                const float2 *row = img + kt * vs;
                int c = 0;
                for (int v = 0; v < vi; ++v) {
                    const float2 s = row[v];
                    c += (r.x <= s.x && s.x < r.z && r.y <= s.y && s.y < r.w) ? 1 : 0;
                }
                if (c) {
                    const int t = kt % P;
                    atomicAdd(&zcnt[t * Z + z], c);
                    atomicAdd(&zany[t * Z + z], 1);
                }
            }
            for (int it = tid; it < kc * vi * Z; it += nt) {
                const int z = it % Z, kv = it / Z, kk = kv / vi, v = kv - kk * vi;
                const float4 r = zone[z];
                const float2 *col = img + kk * P * vs + v;
                bool any = false;
                for (int t = 0; t < P; ++t) {
                    const float2 s = col[t * vs];
                    any = any || (r.x <= s.x && s.x < r.z && r.y <= s.y && s.y < r.w);
                }
                if (any) atomicAdd(&pedz[v * Z + z], 1);
            }
        }
        __syncthreads();
        // ---- the pass's hit flags into the counts
        if (pairs) {
            for (int it = tid; it < P * vi; it += nt) {
                const int t = it / vi, x = t * V + (it - t * vi);             // `it` is the flag's own index
                int s = 0;
                for (int kk = 0; kk < kc; ++kk) {
                    s += flag[kk * P * vs + it];
                    flag[kk * P * vs + it] = 0;
                }
                conf[x] = (unsigned char)(conf[x] + s);
            }
            for (int v = tid; v < vi; v += nt) {
                int s = 0;
                for (int kk = 0; kk < kc; ++kk) {
                    s += fany[kk * vs + v];
                    fany[kk * vs + v] = 0;
                }
                cany[v] = (unsigned char)(cany[v] + s);
            }
        }
        // (the next pass's draw writes only the image, which nobody reads any more; its barrier orders the rest)
    }
    __syncthreads();

    // ---- results
    if (pairs) {
        for (int x = tid; x < P * V; x += nt) a.conflict[(int64_t)n * P * V + x] = conf[x];
        for (int i = tid; i < V; i += nt) {
            a.conflict_any[(int64_t)n * V + i] = cany[i];
            int best = 0, arg = -1;
            if (i < vi)
                for (int j = 0; j < vi; ++j) {
                    if (j == i) continue;
                    const int c = pc[item_of_pair(i, j, vi)];
                    if (c > best) best = c, arg = j;
                }
            a.partner[(int64_t)n * V + i] = arg;
        }
        if (a.pair)
            for (int x = tid; x < V * V; x += nt) {
                const int i = x / V, j = x - i * V;
                a.pair[(int64_t)n * V * V + x] = (i < vi && j < vi && i != j) ? pc[item_of_pair(i, j, vi)] : 0;
            }
    }
    if (Z > 0) {
        for (int x = tid; x < P * Z; x += nt) {
            a.zone_any[(int64_t)n * P * Z + x] = zany[x];
            a.zone_count[(int64_t)n * P * Z + x] = zcnt[x];
        }
        for (int x = tid; x < V * Z; x += nt) a.ped_zone[(int64_t)n * V * Z + x] = pedz[x];
    }
}

}  // namespace stg

extern "C" {

int stg_sample_risk(const float *pred, int64_t p_sn, int64_t p_sf, int64_t p_sp, int64_t p_sv, const float *obs_last,
                    const int32_t *num_peds, const float *noise, uint64_t seed, const uint64_t *seed_dev, int N, int P,
                    int V, int K, float radius, const float *zones, int64_t z_sn, int Z, int32_t *conflict,
                    int32_t *conflict_any, int32_t *partner, int32_t *pair, int32_t *zone_any, int32_t *zone_count,
                    int32_t *ped_zone, void *stream) {
    STG_REQUIRE(N >= 0 && P >= 1 && V >= 1 && K >= 1 && Z >= 0, STG_EINVAL,
                "stg_sample_risk: bad sizes N=%d P=%d V=%d K=%d Z=%d", N, P, V, K, Z);
    if (N == 0) return STG_OK;
    const bool pairs = radius > 0.f;                          // (a NaN radius asks for nothing)
    STG_REQUIRE(pairs || Z > 0, STG_EINVAL, "stg_sample_risk: nothing to compute (radius <= 0 and Z == 0)");
    STG_REQUIRE(pred, STG_EINVAL, "stg_sample_risk: null pointer (pred)");
    STG_REQUIRE(!pairs || (conflict && conflict_any && partner), STG_EINVAL,
                "stg_sample_risk: null pointer (conflict / conflict_any / partner with radius > 0)");
    STG_REQUIRE(Z == 0 || (zones && zone_any && zone_count && ped_zone), STG_EINVAL,
                "stg_sample_risk: null pointer (zones / zone_any / zone_count / ped_zone with Z=%d)", Z);
    STG_REQUIRE(stg::aligned(noise, 8) && stg::aligned(obs_last, 8), STG_EINVAL,
                "stg_sample_risk: noise / obs_last must be 8-byte aligned");
    STG_REQUIRE(V <= STG_RISK_MAX_V, STG_EUNSUPPORTED, "stg_sample_risk: V=%d above STG_RISK_MAX_V=%d", V,
                STG_RISK_MAX_V);
    STG_REQUIRE(K <= STG_RISK_MAX_K, STG_EUNSUPPORTED, "stg_sample_risk: K=%d above STG_RISK_MAX_K=%d", K,
                STG_RISK_MAX_K);
    STG_REQUIRE(Z <= STG_RISK_MAX_Z, STG_EUNSUPPORTED, "stg_sample_risk: Z=%d above STG_RISK_MAX_Z=%d", Z,
                STG_RISK_MAX_Z);
    STG_REQUIRE(P <= STG_RISK_MAX_P, STG_EUNSUPPORTED, "stg_sample_risk: P=%d above STG_RISK_MAX_P=%d", P,
                STG_RISK_MAX_P);
    const stg::RiskPlan pl = stg::risk_plan(P, V, K, Z, pairs);
    STG_REQUIRE(pl.total <= (size_t)stg::kLdsBytes, STG_ELDS, "stg_sample_risk: %zu bytes of LDS for P=%d V=%d Z=%d",
                pl.total, P, V, Z);
    stg::RiskArgs a{pred, p_sn, p_sf, p_sp, p_sv, obs_last, num_peds, noise, seed, seed_dev, N, P, V, K, radius, zones,
                    z_sn, Z, conflict, conflict_any, partner, pair, zone_any, zone_count, ped_zone, pl.kb,
                    (uint32_t)pl.o_img, (uint32_t)pl.o_zone, (uint32_t)pl.o_zcnt, (uint32_t)pl.o_zany,
                    (uint32_t)pl.o_pedz, (uint32_t)pl.o_pc, (uint32_t)pl.o_conf, (uint32_t)pl.o_cany,
                    (uint32_t)pl.o_flag, (uint32_t)pl.o_fany, (uint32_t)pl.total};
    return stg::launch({"stg_sample_risk", dim3((unsigned)N), dim3((unsigned)pl.threads), pl.total,
                        stg::as_stream(stream), 64 * 1024},
                       stg::sample_risk_kernel, a);
}

}  // extern "C"
