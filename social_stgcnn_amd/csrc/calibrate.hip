// calibrate: one positive factor g_t on the covariance of every predicted step, fitted on held-out predictions on the
// device, and the launch that applies it to V_pred in front of its consumers.
//
// The sampler draws the steps independently and sums them (sample_draw.hpp), so factors g_t on the steps' covariances
// change the absolute covariance at horizon h to C'_h = sum_{t<=h} g_t sig_t, sig_t = [sx^2, rho sx sy, sy^2]_t -- the
// term score_cov_add sums (score_sig, shared) -- and that is a shift of 0.5 log g_t on V_pred's two log-sigma channels at
// step t.  The fit is sequential over the horizons: g_h is the smallest candidate of a fixed search at which the truths
// at horizon h are calibrated under base_h + g sig_h, base_h = sum_{t<h} g_t sig_t from the factors already fitted.
// d2 is score_gauss's, float32 as written, so a fitted factor is judged by the arithmetic the scores and dist_metrics use.
//
//   scan      one workgroup: first[n] = the number of live elements (n', v < num_peds[n']) of the scenes n' < n
//   prologue  a thread per (n, v): sig (N,P,V,3), and the element's flat index n V + v into elem[first[n] + v]
//   eval      a thread per LIVE element in 256-thread workgroups (not a workgroup per scene: nothing is reduced per
//             scene, and padded slots would idle whole lanes -- DESIGN.md 5.31 on V = 32): off_h, base_h and sig_h in
//             registers, then the round's 32 candidates; per candidate the wave's sum of d2 (float64) and its number of
//             d2 <= thr, the four waves added in ascending order through LDS into row blockIdx of the partials
//   pick      one wave: lane c adds candidate c's partials over the workgroups in ascending order, forms ok, a ballot
//             finds the first ok candidate, whose lane writes the next bracket -- device memory the next eval reads --
//             and on the horizon's last round g, bracket, flags and stats
//   apply     a workgroup per scene, one launch: the two log-sigma fields in place, or all five fields into `out`
// 2 + 8 P launches, every size they depend on read from device memory: no atomics, no cooperative launch, no host
// synchronisation, capturable, and the sums have ONE order (a wave by the xor butterfly of wave_sum(double), waves
// ascending, workgroups ascending), so two runs give the same bits.  LDS: 1.5 KB static.
#include <cmath>

#include "score_fn.hpp"

namespace stg {

constexpr int kCalibThreads = 256;
constexpr int kCalibWaves = kCalibThreads / kWave;
constexpr int kCalibCand = 32;                 // candidates per round
constexpr int kCalibRounds = 4;                // the powers of two, then three refinements
constexpr int kCalibExpLo = -10;               // round 0: 2^-10 .. 2^21
constexpr int64_t kCalibMaxElems = (int64_t)1 << 30;

// the search's state between the launches of one horizon
struct CalibState {
    float lo, hi;
    int32_t done;                              // round 0 decided the horizon (LOW, HIGH or EMPTY)
    int32_t pad;
};

// the scratch buffer, carved
struct CalibWs {
    double *pd;                                // (G,32) sums of d2
    int32_t *pi, *pc;                          // (G,32) numbers of d2 <= thr; (G) live elements
    int32_t *first, *elem;                     // (N+1); (N V)
    CalibState *st;
};

static inline int64_t up8(int64_t x) { return (x + 7) & ~(int64_t)7; }
static inline int64_t calib_groups(int N, int V) { return ((int64_t)N * V + kCalibThreads - 1) / kCalibThreads; }

static inline int64_t calib_carve(void *ws, int N, int V, CalibWs *w) {
    const int64_t G = calib_groups(N, V), E = (int64_t)N * V;
    unsigned char *p = static_cast<unsigned char *>(ws);
    int64_t at = 0;
    const auto take = [&](int64_t bytes) {
        unsigned char *q = p + at;
        at += up8(bytes);
        return q;
    };
    w->pd = reinterpret_cast<double *>(take(G * kCalibCand * 8));
    w->pi = reinterpret_cast<int32_t *>(take(G * kCalibCand * 4));
    w->pc = reinterpret_cast<int32_t *>(take(G * 4));
    w->first = reinterpret_cast<int32_t *>(take(((int64_t)N + 1) * 4));
    w->elem = reinterpret_cast<int32_t *>(take(E * 4));
    w->st = reinterpret_cast<CalibState *>(take(sizeof(CalibState)));
    return at;
}

struct CalibArgs {
    const float *v_pred;
    int64_t p_sn, p_sf, p_sp, p_sv;
    const float *mean, *truth;
    const int32_t *num_peds;
    int N, P, V, mode;
    float level, thr;
    float *g, *bracket;
    int32_t *flags;
    double *stats;
    float *sig;
    CalibWs w;
};

__device__ __forceinline__ int calib_peds(const CalibArgs &a, int n) {
    const int c = a.num_peds ? a.num_peds[n] : a.V;
    return c < 0 ? 0 : (c > a.V ? a.V : c);
}

// first[n] = sum_{n' < n} peds(n'), n = 0 .. N: a thread sums a contiguous chunk of scenes, thread 0 adds the chunks
__global__ __launch_bounds__(kCalibThreads) void calib_scan_kernel(const CalibArgs a) {
    __shared__ int32_t chunk[kCalibThreads];
    const int tid = threadIdx.x, per = (a.N + kCalibThreads - 1) / kCalibThreads;
    const int lo = tid * per < a.N ? tid * per : a.N, hi = lo + per < a.N ? lo + per : a.N;
    int32_t s = 0;
    for (int n = lo; n < hi; ++n) s += calib_peds(a, n);
    chunk[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int32_t run = 0;
        for (int i = 0; i < kCalibThreads; ++i) {
            const int32_t c = chunk[i];
            chunk[i] = run;
            run += c;
        }
        a.w.first[a.N] = run;
    }
    __syncthreads();
    s = chunk[tid];
    for (int n = lo; n < hi; ++n) {
        a.w.first[n] = s;
        s += calib_peds(a, n);
    }
}

__global__ __launch_bounds__(kCalibThreads) void calib_prologue_kernel(const CalibArgs a) {
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * kCalibThreads + threadIdx.x;
    if (e >= (int64_t)a.N * a.V) return;
    const int n = (int)(e / a.V), v = (int)(e - (int64_t)n * a.V);
    const bool live = v < calib_peds(a, n);
    if (live) a.w.elem[a.w.first[n] + v] = (int32_t)e;
    for (int t = 0; t < a.P; ++t) {
        float sxx = 0.f, sxy = 0.f, syy = 0.f;
        if (live) score_sig(a.v_pred + n * a.p_sn + v * a.p_sv + t * a.p_sp, a.p_sf, sxx, sxy, syy);
        float *s = a.sig + (((int64_t)n * a.P + t) * a.V + v) * 3;
        s[0] = sxx;
        s[1] = sxy;
        s[2] = syy;
    }
}

// candidate c (0 .. 31) of a round: the powers of two, or the 32 steps from lo to hi with hi itself as the last
__device__ __forceinline__ float calib_candidate(int round, int c, float lo, float hi) {
#pragma clang fp contract(off)
    if (round == 0) return ldexpf(1.f, c + kCalibExpLo);
    return c == kCalibCand - 1 ? hi : lo + (hi - lo) * ((float)(c + 1) * 0x1p-5f);
}

// horizon h (0-based), one round: the workgroup's row of the partials
__global__ __launch_bounds__(kCalibThreads) void calib_eval_kernel(const CalibArgs a, int h, int round) {
#pragma clang fp contract(off)
    __shared__ double sd[kCalibWaves][kCalibCand];
    __shared__ int32_t si[kCalibWaves][kCalibCand];
    __shared__ int32_t sc[kCalibWaves];
    const CalibState st = *a.w.st;
    if (round > 0 && st.done) return;                                  // (uniform over the grid)
    const int64_t L = a.w.first[a.N], i = (int64_t)blockIdx.x * kCalibThreads + threadIdx.x;
    if ((int64_t)blockIdx.x * kCalibThreads >= L) return;              // (uniform over the workgroup)
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const bool live = i < L;
    float dx = 0.f, dy = 0.f, bxx = 0.f, bxy = 0.f, byy = 0.f, sxx = 0.f, sxy = 0.f, syy = 0.f;
    if (live) {
        const int64_t e = a.w.elem[i];
        const int64_t n = e / a.V, v = e - n * a.V;
        const int64_t e0 = n * a.P * a.V + v;                           // the element (n, 0, v)
        for (int t = 0; t < h; ++t) {
            const float *s = a.sig + (e0 + (int64_t)t * a.V) * 3;
            const float gt = a.g[t];
            bxx += gt * s[0];
            bxy += gt * s[1];
            byy += gt * s[2];
        }
        const int64_t eh = e0 + (int64_t)h * a.V;
        sxx = a.sig[eh * 3], sxy = a.sig[eh * 3 + 1], syy = a.sig[eh * 3 + 2];
        const float2 mu = *reinterpret_cast<const float2 *>(a.mean + eh * 2);
        const float2 tr = *reinterpret_cast<const float2 *>(a.truth + eh * 2);
        dx = mu.x - tr.x, dy = mu.y - tr.y;
    }
    const int cnt = __popcll(__ballot(live));
    if (lane == 0) sc[wave] = cnt;
    for (int c = 0; c < kCalibCand; ++c) {
        const float gc = calib_candidate(round, c, st.lo, st.hi);
        float d2 = 0.f, nll;
        if (live) score_gauss(dx, dy, bxx + gc * sxx, bxy + gc * sxy, byy + gc * syy, d2, nll);
        const double s = wave_sum(live ? (double)d2 : 0.0);
        const int in = __popcll(__ballot(live && d2 <= a.thr));
        if (lane == 0) {
            sd[wave][c] = s;
            si[wave][c] = in;
        }
    }
    __syncthreads();
    if (threadIdx.x < kCalibCand) {
        const int c = threadIdx.x;
        double s = sd[0][c];
        int32_t in = si[0][c];
        for (int w = 1; w < kCalibWaves; ++w) {
            s += sd[w][c];
            in += si[w][c];
        }
        a.w.pd[(int64_t)blockIdx.x * kCalibCand + c] = s;
        a.w.pi[(int64_t)blockIdx.x * kCalibCand + c] = in;
    }
    if (threadIdx.x == 0) a.w.pc[blockIdx.x] = sc[0] + sc[1] + sc[2] + sc[3];
}

__device__ __forceinline__ void calib_result(const CalibArgs &a, int h, float g, float lo, float hi, int32_t flag,
                                             double count, double sum, double inside) {
    a.g[h] = g;
    a.bracket[2 * h] = lo;
    a.bracket[2 * h + 1] = hi;
    a.flags[h] = flag;
    a.stats[3 * h] = count;
    a.stats[3 * h + 1] = sum;
    a.stats[3 * h + 2] = inside;
}

// one wave: lane c holds candidate c
__global__ __launch_bounds__(kWave) void calib_pick_kernel(const CalibArgs a, int h, int round) {
#pragma clang fp contract(off)
    const CalibState st = *a.w.st;
    if (round > 0 && st.done) return;
    const int c = threadIdx.x;
    const int64_t L = a.w.first[a.N], G = (L + kCalibThreads - 1) / kCalibThreads;
    if (L == 0) {
        if (c == 0) {
            calib_result(a, h, 1.f, 1.f, 1.f, STG_CALIB_EMPTY, 0.0, 0.0, 0.0);
            *a.w.st = {1.f, 1.f, 1, 0};
        }
        return;
    }
    double sum = 0.0;
    int64_t inside = 0, count = 0;
    if (c < kCalibCand) {
        sum = a.w.pd[c];
        inside = a.w.pi[c];
        for (int64_t b = 1; b < G; ++b) {
            sum += a.w.pd[b * kCalibCand + c];
            inside += a.w.pi[b * kCalibCand + c];
        }
        for (int64_t b = 0; b < G; ++b) count += a.w.pc[b];
    }
    bool ok = false;
    if (c < kCalibCand)
        ok = a.mode == STG_CALIB_MOMENT ? sum <= 2.0 * (double)count
                                        : (double)inside >= (double)a.level * (double)count;
    const unsigned long long mask = __ballot(ok);
    const float mine = calib_candidate(round, c < kCalibCand ? c : 0, st.lo, st.hi);
    float lo, hi;
    int32_t flag = 0;
    int first;
    if (round == 0) {
        if (mask & 1ull) first = 0, flag = STG_CALIB_LOW;
        else if (mask == 0ull) first = kCalibCand - 1, flag = STG_CALIB_HIGH;
        else first = __ffsll((long long)mask) - 1;
        hi = __shfl(mine, first, kWave);
        lo = flag ? hi : __shfl(mine, first > 0 ? first - 1 : 0, kWave);
    } else {
        first = mask ? __ffsll((long long)mask) - 1 : kCalibCand - 1;   // (candidate 32 is the old hi, which was ok)
        hi = __shfl(mine, first, kWave);
        const float below = __shfl(mine, first > 0 ? first - 1 : 0, kWave);
        lo = first > 0 ? below : st.lo;
    }
    if (c == first) {
        *a.w.st = {lo, hi, flag != 0, 0};
        if (flag || round == kCalibRounds - 1) calib_result(a, h, hi, lo, hi, flag, (double)count, sum, (double)inside);
    }
}

struct ApplyArgs {
    const float *in;
    int64_t i_sn, i_sf, i_sp, i_sv;
    const float *shift;
    float *out;
    int64_t o_sn, o_sf, o_sp, o_sv;
    int P, V, f0, nf;                          // the fields f0 .. f0 + nf - 1 are written
};

// a workgroup per scene: its nf P V elements (at most 5 x 32 x 256) in 32-bit index arithmetic
__global__ __launch_bounds__(kCalibThreads) void calib_apply_kernel(const ApplyArgs a) {
    const float *in = a.in + (int64_t)blockIdx.x * a.i_sn;
    float *out = a.out + (int64_t)blockIdx.x * a.o_sn;
    const int pv = a.P * a.V, total = a.nf * pv;
    for (int i = threadIdx.x; i < total; i += kCalibThreads) {
        const int fi = i / pv, r = i - fi * pv, t = r / a.V, v = r - t * a.V, f = a.f0 + fi;
        float x = in[f * a.i_sf + t * a.i_sp + v * a.i_sv];
        if (f == 2 || f == 3) x += a.shift[t];
        out[f * a.o_sf + t * a.o_sp + v * a.o_sv] = x;
    }
}

static int calib_sizes(const char *what, int N, int P, int V) {
    STG_REQUIRE(N >= 0 && P >= 1 && V >= 1, STG_EINVAL, "%s: bad sizes N=%d P=%d V=%d", what, N, P, V);
    STG_REQUIRE(V <= STG_SCORE_MAX_V, STG_EUNSUPPORTED, "%s: V=%d above STG_SCORE_MAX_V=%d", what, V, STG_SCORE_MAX_V);
    STG_REQUIRE(P <= STG_SCORE_MAX_P, STG_EUNSUPPORTED, "%s: P=%d above STG_SCORE_MAX_P=%d", what, P, STG_SCORE_MAX_P);
    STG_REQUIRE((int64_t)N * V <= kCalibMaxElems, STG_EUNSUPPORTED, "%s: N V = %lld above 2^30", what,
                (long long)N * V);
    return STG_OK;
}

}  // namespace stg

extern "C" {

int64_t stg_calib_fit_ws_bytes(int N, int P, int V) {
    const int rc = stg::calib_sizes("stg_calib_fit_ws_bytes", N, P, V);
    if (rc != STG_OK) return rc;
    stg::CalibWs w;
    return stg::calib_carve(nullptr, N, V, &w);
}

int stg_calib_fit(const float *v_pred, int64_t p_sn, int64_t p_sf, int64_t p_sp, int64_t p_sv, const float *mean,
                  const float *truth, const int32_t *num_peds, int N, int P, int V, int mode, float level, float *g,
                  float *bracket, int32_t *flags, double *stats, float *sig, void *ws, int64_t ws_bytes, void *stream) {
    using stg::aligned;
    const int rc = stg::calib_sizes("stg_calib_fit", N, P, V);
    if (rc != STG_OK) return rc;
    STG_REQUIRE(mode == STG_CALIB_MOMENT || mode == STG_CALIB_COVERAGE, STG_EINVAL,
                "stg_calib_fit: unknown mode %d (STG_CALIB_MOMENT or STG_CALIB_COVERAGE)", mode);
    STG_REQUIRE(level > 0.f && level < 1.f, STG_EINVAL, "stg_calib_fit: level %g outside (0, 1)", (double)level);
    if (N == 0) return STG_OK;
    STG_REQUIRE(v_pred && mean && truth, STG_EINVAL, "stg_calib_fit: null pointer (v_pred / mean / truth)");
    STG_REQUIRE(g && bracket && flags && stats && sig, STG_EINVAL,
                "stg_calib_fit: null pointer among the outputs (g / bracket / flags / stats / sig)");
    STG_REQUIRE(ws, STG_EINVAL, "stg_calib_fit: null pointer (ws)");
    STG_REQUIRE(aligned(mean, 8) && aligned(truth, 8) && aligned(ws, 8) && aligned(stats, 8), STG_EINVAL,
                "stg_calib_fit: mean / truth / ws / stats must be 8-byte aligned");
    stg::CalibArgs a{};
    const int64_t need = stg::calib_carve(ws, N, V, &a.w);
    STG_REQUIRE(ws_bytes >= need, STG_EINVAL, "stg_calib_fit: ws_bytes=%lld below stg_calib_fit_ws_bytes=%lld",
                (long long)ws_bytes, (long long)need);
    a.v_pred = v_pred, a.p_sn = p_sn, a.p_sf = p_sf, a.p_sp = p_sp, a.p_sv = p_sv;
    a.mean = mean, a.truth = truth, a.num_peds = num_peds;
    a.N = N, a.P = P, a.V = V, a.mode = mode;
    a.level = level, a.thr = (float)(-2.0 * log1p(-(double)level));
    a.g = g, a.bracket = bracket, a.flags = flags, a.stats = stats, a.sig = sig;
    hipStream_t st = stg::as_stream(stream);
    const dim3 block(stg::kCalibThreads), grid((unsigned)stg::calib_groups(N, V));
    hipLaunchKernelGGL(stg::calib_scan_kernel, dim3(1), block, 0, st, a);
    STG_LAUNCH_CHECK("stg_calib_fit (scan)");
    hipLaunchKernelGGL(stg::calib_prologue_kernel, grid, block, 0, st, a);
    STG_LAUNCH_CHECK("stg_calib_fit (prologue)");
    for (int h = 0; h < P; ++h) {
        for (int r = 0; r < stg::kCalibRounds; ++r) {
            hipLaunchKernelGGL(stg::calib_eval_kernel, grid, block, 0, st, a, h, r);
            STG_LAUNCH_CHECK("stg_calib_fit (eval)");
            hipLaunchKernelGGL(stg::calib_pick_kernel, dim3(1), dim3(stg::kWave), 0, st, a, h, r);
            STG_LAUNCH_CHECK("stg_calib_fit (pick)");
        }
    }
    return STG_OK;
}

int stg_calib_apply(const float *v_pred, int64_t p_sn, int64_t p_sf, int64_t p_sp, int64_t p_sv, const float *shift,
                    int N, int P, int V, float *out, int64_t o_sn, int64_t o_sf, int64_t o_sp, int64_t o_sv,
                    void *stream) {
    const int rc = stg::calib_sizes("stg_calib_apply", N, P, V);
    if (rc != STG_OK) return rc;
    if (N == 0) return STG_OK;
    STG_REQUIRE(v_pred && shift, STG_EINVAL, "stg_calib_apply: null pointer (v_pred / shift)");
    const bool in_place = out == nullptr || out == v_pred;
    STG_REQUIRE(out != v_pred || (o_sn == p_sn && o_sf == p_sf && o_sp == p_sp && o_sv == p_sv), STG_EINVAL,
                "stg_calib_apply: out is v_pred with other strides");
    stg::ApplyArgs a{};
    a.in = v_pred, a.i_sn = p_sn, a.i_sf = p_sf, a.i_sp = p_sp, a.i_sv = p_sv;
    a.shift = shift;
    a.out = in_place ? const_cast<float *>(v_pred) : out;
    if (in_place) a.o_sn = p_sn, a.o_sf = p_sf, a.o_sp = p_sp, a.o_sv = p_sv;
    else a.o_sn = o_sn, a.o_sf = o_sf, a.o_sp = o_sp, a.o_sv = o_sv;
    a.P = P, a.V = V;
    a.f0 = in_place ? 2 : 0, a.nf = in_place ? 2 : 5;
    hipLaunchKernelGGL(stg::calib_apply_kernel, dim3((unsigned)N), dim3(stg::kCalibThreads), 0, stg::as_stream(stream),
                       a);
    STG_LAUNCH_CHECK("stg_calib_apply");
    return STG_OK;
}

}  // extern "C"
