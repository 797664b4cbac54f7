// Non-uniform DFT of the point-cloud F-FNO: features on arbitrary points <-> a 2 m1 x m2 block of Fourier modes.
//
// Replaces SpectralConv2d.fft2d / .ifft2d of the reference (fourierflow/modules/factorized_fno/point_cloud_2d.py:95-131 and
// :133-159) together with the corner slicing that follows them (:54-62, :66-67).  Mode r of the 2 m1 rows has
// k1(r) = r for r < m1 and r - 2 m1 otherwise (the kept rows [0, m1) and [-m1, 0) of the reference's m1 = 2 modes1 basis);
// column j has k2 = j, 0 <= j < m2 (the reference also forms m2 - 1 negative columns and drops them before use).
//
//   E(n, r, j) = exp(2 pi i (k1 xi_n1 + j xi_n2)) * q_j(n),    q_j = 1 when quirk = 0 or j = 0, else 1 + exp(2 pi i xi_n1)
//
// q is what ifft2d's `u_ft[..., 1:].flip(-1, -2).conj()` amounts to (:153-154): the flipped rows pair k1 with -1 - k1, not
// with -k1, so the "negative-k2 half" adds Re(V exp(2 pi i ((k1 + 1) xi_1 + j xi_2))) per column j >= 1 instead of the
// Hermitian partner.
//
//   points -> modes (nudft_modes_kernel):   spec[b][c][r][j] = sum_n u[b][c][n] conj(E(n, r, j))
//       quirk = 0: fft2d (no normalisation); quirk = 1: the adjoint of ifft2d with respect to its modes (dV from dout)
//   modes -> points (nudft_points_kernel):  out[b][c][n] = Re sum_{r,j} spec[b][c][r][j] E(n, r, j)
//       dxi[b][n][d] (+)= sum_c w[b][c][n] d out[b][c][n] / d xi_{n,d}
//       quirk = 1: ifft2d and its xi gradient (w = dout); quirk = 0: the adjoint of fft2d (out = du, w = u gives its dxi)
//
// Twiddles are per point and per axis, exp(2 pi i k x) for k in [-m1, m1] and [0, m2): one sincos per (point, k), never one per
// (point, mode).  The argument k x is reduced modulo 1 exactly (two-product + rint) before sincospi, so xi far outside the unit
// square loses no phase accuracy.  Plain fp32 FMAs, fixed summation order, no atomics: every result is deterministic.
#pragma once

#include "ffno_device.h"
#include "ffno.h"

namespace ffno {
namespace nudft {

static constexpr int kPts = 64;        // points per tile (one wave across the points)
static constexpr int kChunk = 8;       // channels staged per pass
static constexpr int kMaxModes = 16;   // m1, m2 <= 16: 2 m1 m2 <= 512 modes per channel

__device__ __forceinline__ float2 cis_2pi(int k, float x) {   // exp(2 pi i k x)
#pragma clang fp contract(off)   // p must stay the rounded product: a contracted p - rint(p) would count e twice
    const float fk = (float)k;
    const float p = fk * x;
    const float e = fmaf(fk, x, -p);          // k x = p + e exactly
    const float t = (p - rintf(p)) + e;       // k x mod 1 in [-1/2, 1/2] (p - rint(p) is exact)
    float s, c;
    plat::sincos_pi(2.f * t, s, c);
    return make_float2(c, s);
}

__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
    return make_float2(fmaf(a.x, b.x, -a.y * b.y), fmaf(a.x, b.y, a.y * b.x));
}

// One workgroup per (256-mode tile, 8-channel chunk, sample); the points stream through LDS 64 at a time with their twiddles.
// LDS: e1[64][2 m1 + 1], e2[64][m2] (one row per point: the lanes of a wave read one row, distinct words), us[8][64].
__global__ __launch_bounds__(256) void nudft_modes_kernel(const float* __restrict__ u, const float2* __restrict__ xi,
                                                          float2* __restrict__ spec, int C, int N, int m1, int m2, int quirk) {
    FFNO_DYN_SMEM(smem);
    const int R = 2 * m1, K1 = 2 * m1 + 1, RM = R * m2;
    float2* e1 = reinterpret_cast<float2*>(smem);
    float2* e2 = e1 + kPts * K1;
    float* us = reinterpret_cast<float*>(e2 + kPts * m2);
    const int tid = threadIdx.x;
    const int t = blockIdx.x * 256 + tid;
    const int c0 = blockIdx.y * kChunk;
    const long b = blockIdx.z;
    const bool live = t < RM;
    const int r = live ? t / m2 : 0, j = live ? t - r * m2 : 0;
    const int ki = (r < m1 ? r : r - R) + m1;          // row of k1 in e1
    const bool shifted = quirk && j >= 1;              // conj(q_j) adds the k1 + 1 row
    float2 acc[kChunk];
    for (int c = 0; c < kChunk; ++c) acc[c] = make_float2(0.f, 0.f);
    const int KT = K1 + m2;
    for (int n0 = 0; n0 < N; n0 += kPts) {
        __syncthreads();   // the previous tile is consumed
        for (int i = tid; i < kPts * KT; i += 256) {
            const int q = i / KT, k = i - q * KT, n = n0 + q;
            const float2 x = n < N ? xi[b * N + n] : make_float2(0.f, 0.f);
            if (k < K1) e1[q * K1 + k] = cis_2pi(k - m1, x.x);
            else e2[q * m2 + (k - K1)] = cis_2pi(k - K1, x.y);
        }
        for (int i = tid; i < kChunk * kPts; i += 256) {
            const int cl = i / kPts, q = i - cl * kPts, n = n0 + q, c = c0 + cl;
            us[i] = (n < N && c < C) ? u[(b * C + c) * N + n] : 0.f;
        }
        __syncthreads();
        const int nq = min(kPts, N - n0);
        for (int q = 0; q < nq; ++q) {
            float2 a = e1[q * K1 + ki];
            if (shifted) {
                const float2 a1 = e1[q * K1 + ki + 1];
                a.x += a1.x, a.y += a1.y;
            }
            float2 bas = cmul(a, e2[q * m2 + j]);
            bas.y = -bas.y;                               // conj(E)
            FFNO_UNROLL
            for (int c = 0; c < kChunk; ++c) {
                const float v = us[c * kPts + q];
                acc[c].x = fmaf(v, bas.x, acc[c].x);
                acc[c].y = fmaf(v, bas.y, acc[c].y);
            }
        }
    }
    if (!live) return;
    for (int c = 0; c < kChunk; ++c)
        if (c0 + c < C) spec[(b * C + c0 + c) * RM + t] = acc[c];
}

// One workgroup per (64-point tile, sample, channel group): lane = point, threadIdx.y = a pair of the 8 channels staged per pass.
// With dxi the grid has one channel group, the workgroup walks every channel and reduces their dxi sum in LDS without atomics;
// without it, each 8-channel chunk is a workgroup of its own (20 x 972 points are only 320 tiles for 256 CUs).
// LDS: e1[2 m1 + 1][64], e2[m2][64] (one row per k: the lanes of a wave read consecutive words), vs[8][2 m1 m2], red[4][64][2].
template <bool GRAD>
__global__ __launch_bounds__(256) void nudft_points_kernel(const float2* __restrict__ spec, const float2* __restrict__ xi,
                                                           const float* __restrict__ w, float* __restrict__ out,
                                                           float2* __restrict__ dxi, int C, int N, int m1, int m2, int quirk,
                                                           int accumulate) {
    FFNO_DYN_SMEM(smem);
    const int R = 2 * m1, K1 = 2 * m1 + 1, RM = R * m2;
    float2* e1 = reinterpret_cast<float2*>(smem);
    float2* e2 = e1 + K1 * kPts;
    float2* vs = e2 + m2 * kPts;
    float* red = reinterpret_cast<float*>(vs + kChunk * RM);
    const int p = threadIdx.x, ty = threadIdx.y, tid = ty * kPts + p;
    const long b = blockIdx.y;
    const int n = blockIdx.x * kPts + p;
    const bool live = n < N;
    for (int i = tid; i < (K1 + m2) * kPts; i += 256) {
        const int k = i / kPts, q = i - k * kPts, nn = blockIdx.x * kPts + q;
        const float2 x = nn < N ? xi[b * N + nn] : make_float2(0.f, 0.f);
        if (k < K1) e1[i] = cis_2pi(k - m1, x.x);
        else e2[i - K1 * kPts] = cis_2pi(k - K1, x.y);
    }
    float g1 = 0.f, g2 = 0.f;
    for (int cc0 = blockIdx.z * kChunk; cc0 < C; cc0 += gridDim.z * kChunk) {
        __syncthreads();   // twiddles written / the previous chunk consumed
        for (int i = tid; i < kChunk * RM; i += 256) {
            const int cl = i / RM, tt = i - cl * RM, c = cc0 + cl;
            vs[i] = c < C ? spec[(b * C + c) * RM + tt] : make_float2(0.f, 0.f);
        }
        __syncthreads();
        const float2* v0 = vs + (2 * ty) * RM;
        const float2* v1 = v0 + RM;
        // column j = 0 (z: sum, z1: k1-weighted sum) and columns j >= 1 (s: sum, s1: k1-weighted, s2: j-weighted)
        float2 z[2] = {}, z1[2] = {}, s[2] = {}, s1[2] = {}, s2[2] = {};
        for (int j = 0; j < m2; ++j) {
            const float2 ej = e2[j * kPts + p];
            float2 a[2] = {}, a1[2] = {};
            for (int r = 0; r < R; ++r) {
                const int k1 = r < m1 ? r : r - R;
                const float2 bas = cmul(e1[(k1 + m1) * kPts + p], ej);
                const float2 t0 = cmul(v0[r * m2 + j], bas), t1 = cmul(v1[r * m2 + j], bas);
                a[0].x += t0.x, a[0].y += t0.y, a[1].x += t1.x, a[1].y += t1.y;
                if (GRAD) {
                    const float fk = (float)k1;
                    a1[0].x = fmaf(fk, t0.x, a1[0].x), a1[0].y = fmaf(fk, t0.y, a1[0].y);
                    a1[1].x = fmaf(fk, t1.x, a1[1].x), a1[1].y = fmaf(fk, t1.y, a1[1].y);
                }
            }
            for (int h = 0; h < 2; ++h) {
                if (j == 0) {
                    z[h] = a[h], z1[h] = a1[h];
                } else {
                    s[h].x += a[h].x, s[h].y += a[h].y;
                    if (GRAD) {
                        s1[h].x += a1[h].x, s1[h].y += a1[h].y;
                        s2[h].x = fmaf((float)j, a[h].x, s2[h].x), s2[h].y = fmaf((float)j, a[h].y, s2[h].y);
                    }
                }
            }
        }
        const float2 Q = e1[(m1 + 1) * kPts + p];                          // exp(2 pi i xi_1)
        const float2 q1 = quirk ? make_float2(1.f + Q.x, Q.y) : make_float2(1.f, 0.f);
        for (int h = 0; h < 2; ++h) {
            const int c = cc0 + 2 * ty + h;
            if (!live || c >= C) continue;
            const float2 full = cmul(s[h], q1);
            if (out) out[(b * C + c) * N + n] = z[h].x + full.x;
            if (GRAD) {
                // d/dxi_1: sum k1 V E + [quirk] Q sum_{j>=1} V e (the k1 + 1 row);  d/dxi_2: sum j V E;  times 2 pi i, real part
                float2 d1 = cmul(s1[h], q1);
                d1.x += z1[h].x, d1.y += z1[h].y;
                if (quirk) {
                    const float2 qs = cmul(Q, s[h]);
                    d1.x += qs.x, d1.y += qs.y;
                }
                const float2 d2 = cmul(s2[h], q1);
                const float wv = w[(b * C + c) * N + n];
                g1 = fmaf(wv, d1.y, g1);
                g2 = fmaf(wv, d2.y, g2);
            }
        }
    }
    if (!GRAD) return;
    red[(ty * kPts + p) * 2] = g1;
    red[(ty * kPts + p) * 2 + 1] = g2;
    __syncthreads();
    if (ty != 0 || !live) return;
    float t1 = 0.f, t2 = 0.f;
    for (int y = 0; y < 4; ++y) t1 += red[(y * kPts + p) * 2], t2 += red[(y * kPts + p) * 2 + 1];
    const float m2pi = -6.28318530717958647692f;                          // Re(2 pi i z) = -2 pi Im z
    float2 g = make_float2(m2pi * t1, m2pi * t2);
    if (accumulate) {
        const float2 o = dxi[b * N + n];
        g.x += o.x, g.y += o.y;
    }
    dxi[b * N + n] = g;
}

static inline size_t modes_lds(int m1, int m2) { return sizeof(float2) * kPts * (2 * m1 + 1 + m2) + sizeof(float) * kChunk * kPts; }
static inline size_t points_lds(int m1, int m2) {
    return sizeof(float2) * ((size_t)kPts * (2 * m1 + 1 + m2) + (size_t)kChunk * 2 * m1 * m2) + sizeof(float) * 4 * kPts * 2;
}

static inline int status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? FFNO_OK : (int)e;
}

}  // namespace nudft
}  // namespace ffno

extern "C" int ffno_nudft_supported(int C, int m1, int m2) {
    using namespace ffno::nudft;
    return C > 0 && m1 >= 1 && m2 >= 1 && m1 <= kMaxModes && m2 <= kMaxModes;
}

extern "C" int ffno_nudft_modes(const float* u, const float* xi, float* spec, int B, int C, int N, int m1, int m2, int quirk,
                                void* stream) {
    using namespace ffno::nudft;
    if (!u || !xi || !spec || B <= 0 || C <= 0 || N <= 0 || m1 <= 0 || m2 <= 0) return FFNO_EINVAL;
    if (!ffno_nudft_supported(C, m1, m2) || B > 65535) return FFNO_EUNSUPPORTED;
    const int RM = 2 * m1 * m2;
    const dim3 grid((unsigned)((RM + 255) / 256), (unsigned)((C + kChunk - 1) / kChunk), (unsigned)B);
    FFNO_LAUNCH(nudft_modes_kernel, grid, dim3(256), modes_lds(m1, m2), (hipStream_t)stream, u,
                reinterpret_cast<const float2*>(xi), reinterpret_cast<float2*>(spec), C, N, m1, m2, quirk ? 1 : 0);
    return status();
}

extern "C" int ffno_nudft_points(const float* spec, const float* xi, const float* w, float* out, float* dxi, int B, int C, int N,
                                 int m1, int m2, int quirk, int accumulate, void* stream) {
    using namespace ffno::nudft;
    if (!spec || !xi || (!out && !dxi) || (dxi && !w) || B <= 0 || C <= 0 || N <= 0 || m1 <= 0 || m2 <= 0) return FFNO_EINVAL;
    if (!ffno_nudft_supported(C, m1, m2) || B > 65535) return FFNO_EUNSUPPORTED;
    const unsigned tiles = (unsigned)((N + kPts - 1) / kPts), chunks = (unsigned)((C + kChunk - 1) / kChunk);
    const dim3 grid(tiles, (unsigned)B, dxi ? 1u : chunks), block(kPts, 4);
    const size_t lds = points_lds(m1, m2);
    hipStream_t s = (hipStream_t)stream;
    const float2* sp = reinterpret_cast<const float2*>(spec);
    const float2* x = reinterpret_cast<const float2*>(xi);
    if (dxi)
        FFNO_LAUNCH(nudft_points_kernel<true>, grid, block, lds, s, sp, x, w, out, reinterpret_cast<float2*>(dxi), C, N, m1, m2,
                    quirk ? 1 : 0, accumulate ? 1 : 0);
    else
        FFNO_LAUNCH(nudft_points_kernel<false>, grid, block, lds, s, sp, x, w, out, reinterpret_cast<float2*>(dxi), C, N, m1,
                    m2, quirk ? 1 : 0, accumulate ? 1 : 0);
    return status();
}
