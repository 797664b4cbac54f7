// The time step of the Kolmogorov-flow data generator behind `generate kolmogorov` (reference builders/kolmogorov.py:328-428 with
// jax-cfd's spectral NavierStokes2D and crank_nicolson_rk4; written from the formulas), on torch.fft.rfft2
// HALF spectra [B][N][N/2+1][2] of the vorticity on the periodic square [0, len)^2, len = 2 pi / k0 (k0 = 1: integer wavenumbers):
//     ffno_kf2d_derivs      w_h -> the spectra of v_x = psi_y, v_y = -psi_x, w_x, w_y, psi_h = w_h / |k|^2   (one read of w_h)
//     (one batched irfft2 of the four, ffno_ns2d_advect for v_x w_x + v_y w_y, one rfft2)
//     ffno_kf2d_stage       one stage of the low-storage Carpenter-Kennedy RK4(5) with Crank-Nicolson for the linear part:
//                               h <- E(w_h) + beta h,   w_h <- (w_h + gamma dt h + mu L w_h) / (1 - mu L)        in place
//                               E = -filt adv_scale adv_h + c w_h + f_h,   L = -nu |k|^2 - drag,   filt: 9 (kx^2 + ky^2) <= N^2 in indices
//     ffno_kf2d_downsample  the velocity fields [2][B][N][N] -> the coarse vorticity [B][m][m] by the staggered-velocity formulas
//                           at the top of ffno_coarsen.h (the last line of each block of f = N / m, averaged across the block;
//                           periodic forward differences), with that file's LDS row scheme and sequential sums in index order
// Row r is k_x = k0 r (r < N/2) or k0 (r - N), column c is k_y = k0 c; derivatives along an axis are zero at that axis' Nyquist
// bin, as in ffno_ns2d.h and for the same reason.  The Kolmogorov forcing has ONE non-zero bin in a half spectrum, (0, kf), so the
// stage gets it as three scalars and reads no force image.  derivs and stage stream: 16 bytes (two bins) per thread and tensor and
// trip of a grid-stride loop, indices from shifts and masks after one division by N/2+1, no LDS, no atomics.
#pragma once

#include "ffno_ns2d.h"

namespace ffno {
namespace kf2d {

using ns2d::aligned16;
using ns2d::Bin;
using ns2d::bins_of;
using ns2d::blocks_for;
using ns2d::status;

__device__ __forceinline__ int k2_of(const Bin& b, int N) {
    const int k = b.kx(N);
    return k * k + b.c * b.c;      // at most 2 (N/2)^2 = 2^23 for N = 4096
}

// (v_x, v_y, w_x, w_y) of one bin w = (re, im)
__device__ __forceinline__ void derivs_bin(float re, float im, const Bin& b, int N, float k0, float2& vx, float2& vy, float2& wx,
                                           float2& wy) {
    const int k2 = k2_of(b, N);
    const float lap = k2 ? k0 * k0 * (float)k2 : 1.f;      // bin (0, 0): both factors below are zero, psi_h(0, 0) = 0
    const float pr = re / lap, pi = im / lap;
    const float sx = b.r == N / 2 ? 0.f : k0 * (float)b.kx(N);
    const float sy = b.c == N / 2 ? 0.f : k0 * (float)b.c;
    vx = make_float2(-sy * pi, sy * pr);       //  i k_y psi
    vy = make_float2(sx * pi, -sx * pr);       // -i k_x psi
    wx = make_float2(-sx * im, sx * re);
    wy = make_float2(-sy * im, sy * re);
}

__global__ __launch_bounds__(256) void kf2d_derivs_kernel(const float4* __restrict__ w, float4* __restrict__ out, unsigned pairs,
                                                          int N, float k0) {
    const int Nh = N / 2 + 1;
    for (unsigned p = blockIdx.x * 256u + threadIdx.x; p < pairs; p += gridDim.x * 256u) {
        const float4 a = w[p];
        Bin b(2u * p, N, Nh);
        float2 u0, v0, x0, y0, u1, v1, x1, y1;
        derivs_bin(a.x, a.y, b, N, k0, u0, v0, x0, y0);
        b.next(N, Nh);
        derivs_bin(a.z, a.w, b, N, k0, u1, v1, x1, y1);
        out[p] = make_float4(u0.x, u0.y, u1.x, u1.y);
        out[(size_t)pairs + p] = make_float4(v0.x, v0.y, v1.x, v1.y);
        out[2 * (size_t)pairs + p] = make_float4(x0.x, x0.y, x1.x, x1.y);
        out[3 * (size_t)pairs + p] = make_float4(y0.x, y0.y, y1.x, y1.y);
    }
}

struct StageArgs {
    float nu_k0sq, drag, c, gdt, beta, mu, f_re, f_im, adv_scale;      // nu k0^2; gamma dt
    int kf;                                                  // column of the forced bin (0, kf); 0: no forcing
};

// one bin of a stage: h' = E + beta h, w' = (w + gamma dt h' + mu L w) / (1 - mu L)
template <bool FIRST>
__device__ __forceinline__ void stage_bin(float2& w, float2& h, float2 A, const Bin& b, int N, const StageArgs& s) {
    const int k2 = k2_of(b, N);
    const float keep = 9 * k2 <= N * N ? s.adv_scale : 0.f;       // the circular 2/3 rule |k| <= N/3 in indices; 9 k2 < 2^27
    const bool forced = s.kf && b.r == 0 && b.c == s.kf;
    float ex = fmaf(s.c, w.x, -(keep * A.x)) + (forced ? s.f_re : 0.f);
    float ey = fmaf(s.c, w.y, -(keep * A.y)) + (forced ? s.f_im : 0.f);
    if (!FIRST) ex = fmaf(s.beta, h.x, ex), ey = fmaf(s.beta, h.y, ey);
    h = make_float2(ex, ey);
    const float mL = s.mu * -fmaf(s.nu_k0sq, (float)k2, s.drag);      // mu L, L = -(nu |k|^2 + drag)
    const float d = 1.f - mL;
    w = make_float2(fmaf(mL, w.x, fmaf(s.gdt, ex, w.x)) / d, fmaf(mL, w.y, fmaf(s.gdt, ey, w.y)) / d);
}

template <bool FIRST>
__global__ __launch_bounds__(256) void kf2d_stage_kernel(float4* __restrict__ w, float4* __restrict__ h, const float4* __restrict__ adv,
                                                         unsigned pairs, int N, StageArgs s) {
    const int Nh = N / 2 + 1;
    for (unsigned p = blockIdx.x * 256u + threadIdx.x; p < pairs; p += gridDim.x * 256u) {
        const float4 a = w[p], g = adv[p];
        float4 hh = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!FIRST) hh = h[p];
        Bin b(2u * p, N, Nh);
        float2 w0 = make_float2(a.x, a.y), h0 = make_float2(hh.x, hh.y), w1 = make_float2(a.z, a.w), h1 = make_float2(hh.z, hh.w);
        stage_bin<FIRST>(w0, h0, make_float2(g.x, g.y), b, N, s);
        b.next(N, Nh);
        stage_bin<FIRST>(w1, h1, make_float2(g.z, g.w), b, N, s);
        w[p] = make_float4(w0.x, w0.y, w1.x, w1.y);
        h[p] = make_float4(h0.x, h0.y, h1.x, h1.y);
    }
}

// Workgroup (slice, sample) owns R consecutive coarse rows: u_c of its R rows and v_c of its R + 1 rows (the halo row below,
// wrapped) go to LDS, every mean a sequential sum in index order; then one thread per coarse cell differences and stores.
__global__ __launch_bounds__(256) void kf2d_downsample_kernel(const float* __restrict__ vel, float* __restrict__ out, int N, int m,
                                                              int f, int R, float dx) {
    FFNO_DYN_SMEM(smem);
    float* uc = reinterpret_cast<float*>(smem);      // [R][m]
    float* vc = uc + (size_t)R * m;                  // [R + 1][m]
    const int bidx = blockIdx.y, B = gridDim.y;
    const int i0 = blockIdx.x * R, nr = min(R, m - i0);      // this slice's coarse rows [i0, i0 + nr)
    const float* u = vel + (size_t)bidx * N * N;
    const float* v = vel + ((size_t)B + bidx) * N * N;
    const float ff = (float)f;
    for (int c = threadIdx.x; c < nr * m; c += 256) {
        const int r = c / m, j = c - r * m;
        const float* row = u + (size_t)(f * (i0 + r) + f - 1) * N + (size_t)f * j;
        float a = 0.f;
        for (int b = 0; b < f; ++b) a += row[b];
        uc[c] = a / ff;
    }
    for (int c = threadIdx.x; c < (nr + 1) * m; c += 256) {
        const int r = c / m, j = c - r * m;
        const int i = (i0 + r) % m;                          // r = nr on the last slice: coarse row 0
        const float* col = v + (size_t)f * i * N + (size_t)f * j + f - 1;
        float a = 0.f;
        for (int k = 0; k < f; ++k) a += col[(size_t)N * k];
        vc[c] = a / ff;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < nr * m; c += 256) {
        const int r = c / m, j = c - r * m;
        const int jn = j + 1 < m ? j + 1 : 0;
        out[((size_t)bidx * m + (i0 + r)) * m + j] = (vc[c + m] - vc[c]) / dx - (uc[r * m + jn] - uc[c]) / dx;
    }
}

// the slicing rule of ffno_coarsen.h (that header defines entry points of another translation unit, so the rule is restated):
// about 1024 coarse cells per workgroup, at least one row; rows() rows per slice, slices() of them
static inline int rows(int m) {
    const long want = ((long)m * m + 1023) / 1024;
    const int S = want < m ? (int)want : m;
    return (m + S - 1) / S;
}
static inline int slices(int m) { return (m + rows(m) - 1) / rows(m); }
static inline bool valid_k0(float k0) { return k0 > 0.f && k0 < 1e6f; }      // also refuses NaN

}  // namespace kf2d
}  // namespace ffno

extern "C" int ffno_kf2d_supported(int N) { return N >= 16 && N <= 4096 && (N & (N - 1)) == 0; }

extern "C" int ffno_kf2d_derivs(const float* w_h, float* out4, float k0, int B, int N, void* stream) {
    using namespace ffno::kf2d;
    if (!w_h || !out4 || B <= 0 || N <= 0 || !valid_k0(k0) || !aligned16(w_h) || !aligned16(out4)) return FFNO_EINVAL;
    const size_t bins = ffno_kf2d_supported(N) ? bins_of(B, N) : 0;
    if (!bins) return FFNO_EUNSUPPORTED;
    FFNO_LAUNCH(kf2d_derivs_kernel, dim3(blocks_for(bins / 2)), dim3(256), 0, (hipStream_t)stream,
                reinterpret_cast<const float4*>(w_h), reinterpret_cast<float4*>(out4), (unsigned)(bins / 2), N, k0);
    return status();
}

extern "C" int ffno_kf2d_stage(float* w_h, float* h, const float* adv_h, float viscosity, float drag, float linear_coefficient,
                               float dt, float beta, float gamma, float mu, int kf, float f_re, float f_im, float k0, float adv_scale,
                               int first, int B, int N, void* stream) {
    using namespace ffno::kf2d;
    if (!w_h || !h || !adv_h || B <= 0 || N <= 0 || !valid_k0(k0) || !(adv_scale > 0.f) || !aligned16(w_h) || !aligned16(h) || !aligned16(adv_h))
        return FFNO_EINVAL;
    const size_t bins = ffno_kf2d_supported(N) ? bins_of(B, N) : 0;
    if (!bins) return FFNO_EUNSUPPORTED;
    if (kf < 0 || (kf == 0 && (f_re != 0.f || f_im != 0.f)) || kf > N / 2 - 1) return FFNO_EINVAL;      // kf = 0: no forcing
    const unsigned pairs = (unsigned)(bins / 2);
    const StageArgs s = {viscosity * k0 * k0, drag, linear_coefficient, gamma * dt, beta, mu, f_re, f_im, adv_scale, kf};
    float4 *w = reinterpret_cast<float4*>(w_h), *hh = reinterpret_cast<float4*>(h);
    const float4* a = reinterpret_cast<const float4*>(adv_h);
    if (first) FFNO_LAUNCH(kf2d_stage_kernel<true>, dim3(blocks_for(pairs)), dim3(256), 0, (hipStream_t)stream, w, hh, a, pairs, N, s);
    else FFNO_LAUNCH(kf2d_stage_kernel<false>, dim3(blocks_for(pairs)), dim3(256), 0, (hipStream_t)stream, w, hh, a, pairs, N, s);
    return status();
}

extern "C" int ffno_kf2d_downsample(const float* vel2, float* out, int B, int N, int m, float length, void* stream) {
    using namespace ffno::kf2d;
    if (!vel2 || !out || B <= 0 || N <= 0 || m < 1 || !(length > 0.f)) return FFNO_EINVAL;
    if (!ffno_kf2d_supported(N) || B > 65535) return FFNO_EUNSUPPORTED;
    if (N % m) return FFNO_EINVAL;
    const int R = rows(m);
    FFNO_LAUNCH(kf2d_downsample_kernel, dim3(slices(m), B), dim3(256), sizeof(float) * (size_t)(2 * R + 1) * m,
                (hipStream_t)stream, vel2, out, N, m, N / m, R, length / (float)m);
    return status();
}
