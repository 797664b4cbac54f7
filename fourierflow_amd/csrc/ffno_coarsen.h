// Reduced-grid correlation of the Markov routine's validation (the torus_kochkov configs validate on `corr_data` at 32 x 32
// while the model runs at 64, 128 or 256): the velocity image of a prediction -> coarse staggered velocity -> coarse
// vorticity -> the three sums of its correlation with corr_data, one launch per rollout step.  Reference
// fourierflow/utils/array.py:18-80 (downsample_vorticity: jax-cfd on the CPU, a Python loop over batch and time) called at
// routines/grid_2d_markov.py:353-370.  With f = X / m = Y / m, dx = len_x / m, dy = len_y / m:
//     u_c[i][j] = (sum_{b<f} u[f i + f-1][f j + b]) / f          every f-th line along x, the LAST of its block, mean across it
//     v_c[i][j] = (sum_{a<f} v[f i + a][f j + f-1]) / f          the same for v along y
//     w_c[i][j] = (v_c[(i+1) % m][j] - v_c[i][j]) / dx - (u_c[i][(j+1) % m] - u_c[i][j]) / dy
// Workgroup (slice, sample) owns R consecutive coarse rows.  It first fills LDS with u_c of its R rows and v_c of its R + 1 rows
// (the halo row below, wrapped), every mean a sequential sum in index order; the lanes of a wave walk one fine row of `vel`
// together, 12 f bytes apart, so each line of the row is fetched once and used by the following trips.  The halo column of
// u_c is in LDS already (a row is whole).  Then one thread per coarse cell differences, writes preds2 and adds its three
// products; wave butterfly, four waves, one store per sum.  fp32, no atomics, every output written once.
#pragma once

#include "ffno_device.h"
#include "ffno.h"

namespace ffno {
namespace coarsen {

static constexpr int kSums = 3;
static constexpr int kMaxM = 4096;      // (2 R + 1) m + 12 floats of LDS with R = 1: 48 KB

// slices of coarse rows per sample: about 1024 cells each, at least one row; rows() rows per slice, slices() of them
static inline int rows(int m) {
    const long want = ((long)m * m + 1023) / 1024;
    const int S = want < m ? (int)want : m;
    return (m + S - 1) / S;
}
static inline int slices(int m) { return (m + rows(m) - 1) / rows(m); }

__global__ __launch_bounds__(256) void vorticity_coarsen_kernel(const float* __restrict__ vel, const float* __restrict__ corr,
                                                                float* __restrict__ preds2, float* __restrict__ sums, int X,
                                                                int Y, int m, int f, int R, int Tc, int n_steps, int t,
                                                                float dx, float dy) {
    FFNO_DYN_SMEM(smem);
    float* uc = reinterpret_cast<float*>(smem);      // [R][m]
    float* vc = uc + (size_t)R * m;                  // [R + 1][m]
    float(*red)[kSums] = reinterpret_cast<float(*)[kSums]>(vc + (size_t)(R + 1) * m);      // [4][kSums]: no static LDS in front
    const int bidx = blockIdx.y, S = gridDim.x, B = gridDim.y;
    const int i0 = blockIdx.x * R, nr = min(R, m - i0);      // this slice's coarse rows [i0, i0 + nr)
    const float* img = vel + (size_t)bidx * X * Y * 3;
    const float ff = (float)f;
    for (int c = threadIdx.x; c < nr * m; c += 256) {
        const int r = c / m, j = c - r * m;
        const float* row = img + ((size_t)(f * (i0 + r) + f - 1) * Y + (size_t)f * j) * 3 + 1;
        float a = 0.f;
        for (int b = 0; b < f; ++b) a += row[3 * b];
        uc[c] = a / ff;
    }
    for (int c = threadIdx.x; c < (nr + 1) * m; c += 256) {
        const int r = c / m, j = c - r * m;
        const int i = (i0 + r) % m;                          // r = nr on the last slice: coarse row 0
        const float* col = img + ((size_t)f * i * Y + (size_t)f * j + f - 1) * 3 + 2;
        float a = 0.f;
        for (int k = 0; k < f; ++k) a += col[(size_t)3 * Y * k];
        vc[c] = a / ff;
    }
    __syncthreads();
    const int tc = Tc - n_steps + t;
    float s[kSums] = {0.f, 0.f, 0.f};
    for (int c = threadIdx.x; c < nr * m; c += 256) {
        const int r = c / m, j = c - r * m;
        const int jn = j + 1 < m ? j + 1 : 0;
        const float w = (vc[c + m] - vc[c]) / dx - (uc[r * m + jn] - uc[c]) / dy;
        const size_t e = ((size_t)bidx * m + (i0 + r)) * m + j;
        const float y = corr[e * Tc + tc];
        if (preds2) preds2[e * n_steps + t] = w;
        s[0] = fmaf(w, w, s[0]);
        s[1] = fmaf(y, y, s[1]);
        s[2] = fmaf(w, y, s[2]);
    }
    FFNO_UNROLL
    for (int k = 0; k < kSums; ++k) {
        s[k] = wave_sum(s[k]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x < kSums) {
        const int k = threadIdx.x;
        sums[(((size_t)t * B + bidx) * S + blockIdx.x) * kSums + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    }
}

// metrics = { diverged_t, mean_t p_2, p_2[n_steps] }; one workgroup, every sum in index order
__global__ __launch_bounds__(256) void markov_corr_metrics_kernel(const float* __restrict__ sums, float* metrics, int B, int S,
                                                                  int n_steps, float threshold) {
    auto slice_sum = [&](int t, int b, int k) {
        float a = 0.f;
        for (int sl = 0; sl < S; ++sl) a += sums[(((size_t)t * B + b) * S + sl) * kSums + k];
        return a;
    };
    for (int t = threadIdx.x; t < n_steps; t += 256) {
        float p = 0.f;
        for (int b = 0; b < B; ++b) p += slice_sum(t, b, 2) / (sqrtf(slice_sum(t, b, 0)) * sqrtf(slice_sum(t, b, 1)));
        metrics[2 + t] = p / (float)B;
    }
    __syncthreads();      // orders this workgroup's metrics[2..] stores before thread 0 reads them back
    if (threadIdx.x == 0) {
        float pm = 0.f;
        int diverged = n_steps;
        for (int t = n_steps - 1; t >= 0; --t)
            if (metrics[2 + t] < threshold) diverged = t;
        for (int t = 0; t < n_steps; ++t) pm += metrics[2 + t];
        metrics[0] = (float)diverged;
        metrics[1] = pm / (float)n_steps;
    }
}

static inline int status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? FFNO_OK : (int)e;
}

}  // namespace coarsen
}  // namespace ffno

extern "C" size_t ffno_vorticity_coarsen_ws_floats(int B, int m, int n_steps) {
    if (B <= 0 || m <= 0 || m > ffno::coarsen::kMaxM || n_steps <= 0) return 0;
    return (size_t)n_steps * (size_t)B * (size_t)ffno::coarsen::slices(m) * (size_t)ffno::coarsen::kSums;
}

extern "C" int ffno_vorticity_coarsen_step(const float* vel, const float* corr, float* preds2, float* sums, int B, int X, int Y,
                                           int m, int Tc, int n_steps, int t, float len_x, float len_y, void* stream) {
    using namespace ffno::coarsen;
    if (!vel || !corr || !sums || B <= 0 || X <= 0 || Y <= 0 || m < 1 || !(len_x > 0.f) || !(len_y > 0.f)) return FFNO_EINVAL;
    if (X % m || Y % m || X / m != Y / m) return FFNO_EINVAL;
    if (n_steps <= 0 || Tc < n_steps || t < 0 || t >= n_steps) return FFNO_EINVAL;
    if (m > kMaxM || B > 65535) return FFNO_EUNSUPPORTED;
    const int R = rows(m);
    FFNO_LAUNCH(vorticity_coarsen_kernel, dim3(slices(m), B), dim3(256), sizeof(float) * ((size_t)(2 * R + 1) * m + 4 * kSums),
                (hipStream_t)stream, vel, corr, preds2, sums, X, Y, m, X / m, R, Tc, n_steps, t, len_x / (float)m,
                len_y / (float)m);
    return status();
}

extern "C" int ffno_markov_corr_metrics(const float* sums, float* metrics, int B, int m, int n_steps, float threshold,
                                        void* stream) {
    using namespace ffno::coarsen;
    if (!sums || !metrics || B <= 0 || m < 1 || n_steps <= 0) return FFNO_EINVAL;
    if (m > kMaxM) return FFNO_EUNSUPPORTED;
    FFNO_LAUNCH(markov_corr_metrics_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, sums, metrics, B, slices(m), n_steps,
                threshold);
    return status();
}
