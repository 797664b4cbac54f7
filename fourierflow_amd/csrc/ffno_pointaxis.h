// Per-axis non-uniform DFT of the fully factorised point-cloud F-FNO: features on arbitrary points <-> m2 + m1 one-dimensional
// Fourier modes, one set per coordinate, and those modes <-> the separable latent grid h(x) + g(y).
//
// Replaces SpectralConv2d.get_fft_bases / .get_ifft_bases of the reference (fourierflow/modules/factorized_fno/mesh_plus_2d.py
// :118-168) with the einsums over them (:65, :83-84, :93, :109-110), and the rfft / irfft of the repeated bases (:61, :78, :89,
// :106).  Mode t of the m2 + m1 is
//     t <  m2:  j = t,       coordinate 0 of xi   (the y set: modes2, fourier_weight[0], the last grid axis)
//     t >= m2:  k = t - m2,  coordinate 1 of xi   (the x set: modes1, fourier_weight[1], the first grid axis)
// and E(n, t) = exp(2 pi i j xi_n0) or exp(2 pi i k xi_n1).
//
//   points -> modes (axis_modes_kernel):    spec[b][c][t] = sum_n u[b][c][n] conj(E(n, t))
//   modes -> points (axis_points_kernel):   out[b][c][n]  = Re sum_t spec[b][c][t] E(n, t)
//       dxi[b][n][d] (+)= sum_c w[b][c][n] d out[b][c][n] / d xi_{n,d}
//   modes -> grid (axis_to_grid_kernel):    grid[b][x][y][c] = sum_k a_k Re(spec[b][c][m2 + k] e(k x)) + sum_j a_j Re(spec[b][c][j] e(j y))
//   grid -> modes (grid_to_axis_kernel):    spec[b][c][j] = a_j sum_y (sum_x grid[b][x][y][c]) conj(e(j y)),  [m2 + k] likewise in x
//       e(j s) = exp(2 pi i j s / S);  a = 1 (plain), or the c2r weights of irfft(n = S): 1 / S at DC and Nyquist, 2 / S between,
//       where the imaginary parts of DC and Nyquist do not count (they are written as zero by grid -> modes).
//
// The two point kernels follow ffno_pointcloud.h: one sincos per (point, k) on the exactly reduced k x mod 1, the points stream
// through LDS 64 at a time with their twiddles, plain fp32 FMAs, fixed summation order, no atomics.
#pragma once

#include "ffno_device.h"
#include "ffno.h"
#include "ffno_pointcloud.h"

namespace ffno {
namespace nudft_axis {

using nudft::cis_2pi;
using nudft::cmul;
using nudft::kChunk;
using nudft::kPts;

static constexpr int kMaxModes = 32;   // m1, m2 <= 32: at most 64 modes per channel
static constexpr int kSlab = 8;        // modes per workgroup of axis_modes_kernel
static constexpr int kSub = 256 / kSlab;   // ... and its interleaved point subsets
static constexpr int kRows = 4;        // grid rows written per workgroup of axis_to_grid_kernel
static constexpr int kLine = 16;       // channels per workgroup of grid_to_axis_kernel
static constexpr int kMaxGrid = 256;   // S
static constexpr int kMaxPlane = 8192; // S C: the g(y) table of one sample in LDS

// One workgroup per (8-channel chunk, sample, slab of 8 modes): thread = (mode of the slab, one of 32 interleaved point subsets), so
// every thread works whatever m2 + m1 is and the twiddles of a mode are computed by the one workgroup that uses them; the 32
// partial sums are added in LDS in a fixed order at the end.  LDS: e[64][8] (one row per point), us[8][64], red[32][8][8].
__global__ __launch_bounds__(256) void axis_modes_kernel(const float* __restrict__ u, const float2* __restrict__ xi,
                                                         float2* __restrict__ spec, int C, int N, int m1, int m2) {
    FFNO_DYN_SMEM(smem);
    const int K = m1 + m2;
    float2* e = reinterpret_cast<float2*>(smem);
    float* us = reinterpret_cast<float*>(e + kPts * kSlab);
    float2* red = reinterpret_cast<float2*>(us + kChunk * kPts);
    const int tid = threadIdx.x, tx = tid % kSlab, ty = tid / kSlab;
    const int c0 = blockIdx.x * kChunk, t0 = blockIdx.z * kSlab;
    const long b = blockIdx.y;
    float2 acc[kChunk];
    for (int c = 0; c < kChunk; ++c) acc[c] = make_float2(0.f, 0.f);
    for (int n0 = 0; n0 < N; n0 += kPts) {
        __syncthreads();   // the previous tile is consumed
        for (int i = tid; i < kPts * kSlab; i += 256) {
            const int q = i / kSlab, t = t0 + (i - q * kSlab), n = n0 + q;
            float2 v = make_float2(0.f, 0.f);      // a mode past m2 + m1 adds nothing and is not written
            if (t < K) {
                const float2 x = n < N ? xi[b * N + n] : make_float2(0.f, 0.f);
                v = t < m2 ? cis_2pi(t, x.x) : cis_2pi(t - m2, x.y);
            }
            e[i] = v;
        }
        for (int i = tid; i < kChunk * kPts; i += 256) {
            const int cl = i / kPts, q = i - cl * kPts, n = n0 + q, c = c0 + cl;
            us[i] = (n < N && c < C) ? u[(b * C + c) * N + n] : 0.f;
        }
        __syncthreads();
        const int nq = min(kPts, N - n0);
        for (int q = ty; q < nq; q += kSub) {
            const float2 bas = e[q * kSlab + tx];
            FFNO_UNROLL
            for (int c = 0; c < kChunk; ++c) {
                const float v = us[c * kPts + q];
                acc[c].x = fmaf(v, bas.x, acc[c].x);
                acc[c].y = fmaf(-v, bas.y, acc[c].y);     // conj(E)
            }
        }
    }
    for (int c = 0; c < kChunk; ++c) red[(ty * kChunk + c) * kSlab + tx] = acc[c];
    __syncthreads();
    if (tid >= kChunk * kSlab) return;
    const int c = tid / kSlab, t = t0 + tx;      // the first 64 threads: one (channel, mode) each
    if (c0 + c >= C || t >= K) return;
    float2 s = red[c * kSlab + tx];
    for (int y = 1; y < kSub; ++y) {
        const float2 r = red[(y * kChunk + c) * kSlab + tx];
        s.x += r.x, s.y += r.y;
    }
    spec[(b * C + c0 + c) * K + t] = s;
}

// One workgroup per (64-point tile, sample, channel group): lane = point, threadIdx.y = a pair of the 8 channels staged per pass.
// With dxi the grid has one channel group and the workgroup walks every channel (the dxi sum over channels is reduced in LDS
// without atomics); without it each 8-channel chunk is a workgroup of its own.  LDS: e[K][64] (one row per mode), vs[8][K],
// red[4][64][2].
template <bool GRAD>
__global__ __launch_bounds__(256) void axis_points_kernel(const float2* __restrict__ spec, const float2* __restrict__ xi,
                                                          const float* __restrict__ w, float* __restrict__ out,
                                                          float2* __restrict__ dxi, int C, int N, int m1, int m2, int accumulate) {
    FFNO_DYN_SMEM(smem);
    const int K = m1 + m2;
    float2* e = reinterpret_cast<float2*>(smem);
    float2* vs = e + K * kPts;
    float* red = reinterpret_cast<float*>(vs + kChunk * K);
    const int p = threadIdx.x, ty = threadIdx.y, tid = ty * kPts + p;
    const long b = blockIdx.y;
    const int n = blockIdx.x * kPts + p;
    const bool live = n < N;
    for (int i = tid; i < K * kPts; i += 256) {
        const int k = i / kPts, q = i - k * kPts, nn = blockIdx.x * kPts + q;
        const float2 x = nn < N ? xi[b * N + nn] : make_float2(0.f, 0.f);
        e[i] = k < m2 ? cis_2pi(k, x.x) : cis_2pi(k - m2, x.y);
    }
    float g0 = 0.f, g1 = 0.f;
    for (int cc0 = blockIdx.z * kChunk; cc0 < C; cc0 += gridDim.z * kChunk) {
        __syncthreads();   // twiddles written / the previous chunk consumed
        for (int i = tid; i < kChunk * K; i += 256) {
            const int cl = i / K, tt = i - cl * K, c = cc0 + cl;
            vs[i] = c < C ? spec[(b * C + c) * K + tt] : make_float2(0.f, 0.f);
        }
        __syncthreads();
        for (int h = 0; h < 2; ++h) {
            const float2* v = vs + (2 * ty + h) * K;
            float s = 0.f, d0 = 0.f, d1 = 0.f;      // Re sum, and the j- / k-weighted Im sums of the two coordinates
            for (int j = 0; j < m2; ++j) {
                const float2 t = cmul(v[j], e[j * kPts + p]);
                s += t.x;
                if (GRAD) d0 = fmaf((float)j, t.y, d0);
            }
            for (int k = 0; k < m1; ++k) {
                const float2 t = cmul(v[m2 + k], e[(m2 + k) * kPts + p]);
                s += t.x;
                if (GRAD) d1 = fmaf((float)k, t.y, d1);
            }
            const int c = cc0 + 2 * ty + h;
            if (!live || c >= C) continue;
            if (out) out[(b * C + c) * N + n] = s;
            if (GRAD) {
                const float wv = w[(b * C + c) * N + n];
                g0 = fmaf(wv, d0, g0);
                g1 = fmaf(wv, d1, g1);
            }
        }
    }
    if (!GRAD) return;
    red[(ty * kPts + p) * 2] = g0;
    red[(ty * kPts + p) * 2 + 1] = g1;
    __syncthreads();
    if (ty != 0 || !live) return;
    float t0 = 0.f, t1 = 0.f;
    for (int y = 0; y < 4; ++y) t0 += red[(y * kPts + p) * 2], t1 += red[(y * kPts + p) * 2 + 1];
    const float m2pi = -6.28318530717958647692f;                          // Re(2 pi i z) = -2 pi Im z
    float2 g = make_float2(m2pi * t0, m2pi * t1);
    if (accumulate) {
        const float2 o = dxi[b * N + n];
        g.x += o.x, g.y += o.y;
    }
    dxi[b * N + n] = g;
}

__device__ __forceinline__ void grid_twiddles(float2* tw, int S, int tid) {   // tw[r] = exp(2 pi i r / S)
    for (int r = tid; r < S; r += 256) {
        float s, c;
        plat::sincos_pi(2.f * ((float)r / (float)S), s, c);
        tw[r] = make_float2(c, s);
    }
}

__device__ __forceinline__ float axis_weight(int j, int S, int c2r) {
    if (!c2r) return 1.f;
    return (j == 0 || 2 * j == S ? 1.f : 2.f) / (float)S;
}

// One workgroup per (4 grid rows, sample): g(y) for every y and h(x) for its rows into LDS, then channel-last rows written with
// consecutive lanes on consecutive floats.  LDS: tw[S], g[S][C], h[4][C].
__global__ __launch_bounds__(256) void axis_to_grid_kernel(const float2* __restrict__ spec, float* __restrict__ grid, int C, int S,
                                                           int m1, int m2, int c2r) {
    FFNO_DYN_SMEM(smem);
    const int K = m1 + m2;
    float2* tw = reinterpret_cast<float2*>(smem);
    float* g = reinterpret_cast<float*>(tw + S);
    float* h = g + S * C;
    const int tid = threadIdx.x;
    const long b = blockIdx.y;
    const int x0 = blockIdx.x * kRows;
    const int rows = min(kRows, S - x0);
    grid_twiddles(tw, S, tid);
    __syncthreads();
    for (int i = tid; i < (S + rows) * C; i += 256) {
        const int row = i / C, c = i - row * C;
        const bool is_y = row < S;
        const int s = is_y ? row : x0 + (row - S);
        const int m = is_y ? m2 : m1;
        const float2* v = spec + (b * C + c) * K + (is_y ? 0 : m2);
        float acc = 0.f;
        for (int j = 0; j < m; ++j) {
            const float2 t = tw[(j * s) % S], z = v[j];
            acc = fmaf(axis_weight(j, S, c2r), fmaf(z.x, t.x, -z.y * t.y), acc);
        }
        g[i] = acc;      // (h follows g: row S + r is h[r])
    }
    __syncthreads();
    const int plane = S * C;
    float* dst = grid + (b * S + x0) * (long)plane;
    for (int i = tid; i < rows * plane; i += 256) {
        const int r = i / plane, rem = i - r * plane, c = rem % C;
        dst[i] = h[r * C + c] + g[rem];
    }
}

// One workgroup per (16-channel chunk, sample, axis): the sums over the other grid axis into LDS, then the truncated forward DFT
// of that line.  LDS: tw[S], line[S][16].
__global__ __launch_bounds__(256) void grid_to_axis_kernel(const float* __restrict__ grid, float2* __restrict__ spec, int C, int S,
                                                           int m1, int m2, int c2r) {
    FFNO_DYN_SMEM(smem);
    const int K = m1 + m2;
    float2* tw = reinterpret_cast<float2*>(smem);
    float* line = reinterpret_cast<float*>(tw + S);
    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * kLine;
    const long b = blockIdx.y;
    const int axis = blockIdx.z;      // 0: the y modes (sum over x), 1: the x modes (sum over y)
    grid_twiddles(tw, S, tid);
    const float* src = grid + b * S * (long)S * C;
    const long step = axis == 0 ? (long)S * C : (long)C;       // along the summed axis
    const long keep = axis == 0 ? (long)C : (long)S * C;       // along the kept one
    for (int i = tid; i < S * kLine; i += 256) {
        const int s = i / kLine, c = c0 + (i - s * kLine);
        float acc = 0.f;
        if (c < C) {
            const float* px = src + s * keep + c;
            for (int o = 0; o < S; ++o) acc += px[o * step];
        }
        line[i] = acc;
    }
    __syncthreads();
    const int m = axis == 0 ? m2 : m1, off = axis == 0 ? 0 : m2;
    for (int i = tid; i < kLine * m; i += 256) {
        const int cl = i / m, j = i - cl * m, c = c0 + cl;
        if (c >= C) continue;
        float re = 0.f, im = 0.f;
        for (int s = 0; s < S; ++s) {
            const float2 t = tw[(j * s) % S];
            const float v = line[s * kLine + cl];
            re = fmaf(v, t.x, re);
            im = fmaf(-v, t.y, im);
        }
        const float a = axis_weight(j, S, c2r);
        if (c2r && (j == 0 || 2 * j == S)) im = 0.f;
        spec[(b * C + c) * K + off + j] = make_float2(a * re, a * im);
    }
}

static inline size_t modes_lds() { return sizeof(float2) * kPts * kSlab + sizeof(float) * kChunk * kPts + sizeof(float2) * kSub * kChunk * kSlab; }
static inline size_t points_lds(int K) { return sizeof(float2) * ((size_t)kPts * K + (size_t)kChunk * K) + sizeof(float) * 4 * kPts * 2; }

static inline int grid_args(const void* a, const void* b, int B, int C, int S, int m1, int m2) {
    if (!a || !b || B <= 0 || C <= 0 || S <= 0 || m1 <= 0 || m2 <= 0) return FFNO_EINVAL;
    if (!ffno_nudft_axis_supported(C, m1, m2) || B > 65535 || S > kMaxGrid || C > 256 || (long)S * C > kMaxPlane)
        return FFNO_EUNSUPPORTED;
    if (m1 > S / 2 + 1 || m2 > S / 2 + 1) return FFNO_EMODES;
    return FFNO_OK;
}

}  // namespace nudft_axis
}  // namespace ffno

extern "C" int ffno_nudft_axis_supported(int C, int m1, int m2) {
    using namespace ffno::nudft_axis;
    return C > 0 && m1 >= 1 && m2 >= 1 && m1 <= kMaxModes && m2 <= kMaxModes;
}

extern "C" int ffno_nudft_axis_modes(const float* u, const float* xi, float* spec, int B, int C, int N, int m1, int m2,
                                     void* stream) {
    using namespace ffno::nudft_axis;
    if (!u || !xi || !spec || B <= 0 || C <= 0 || N <= 0 || m1 <= 0 || m2 <= 0) return FFNO_EINVAL;
    if (!ffno_nudft_axis_supported(C, m1, m2) || B > 65535) return FFNO_EUNSUPPORTED;
    const dim3 grid((unsigned)((C + kChunk - 1) / kChunk), (unsigned)B, (unsigned)((m1 + m2 + kSlab - 1) / kSlab));
    FFNO_LAUNCH(axis_modes_kernel, grid, dim3(256), modes_lds(), (hipStream_t)stream, u, reinterpret_cast<const float2*>(xi),
                reinterpret_cast<float2*>(spec), C, N, m1, m2);
    return ffno::nudft::status();
}

extern "C" int ffno_nudft_axis_points(const float* spec, const float* xi, const float* w, float* out, float* dxi, int B, int C,
                                      int N, int m1, int m2, int accumulate, void* stream) {
    using namespace ffno::nudft_axis;
    if (!spec || !xi || (!out && !dxi) || (dxi && !w) || B <= 0 || C <= 0 || N <= 0 || m1 <= 0 || m2 <= 0) return FFNO_EINVAL;
    if (!ffno_nudft_axis_supported(C, m1, m2) || B > 65535) return FFNO_EUNSUPPORTED;
    const unsigned tiles = (unsigned)((N + kPts - 1) / kPts), chunks = (unsigned)((C + kChunk - 1) / kChunk);
    const dim3 grid(tiles, (unsigned)B, dxi ? 1u : chunks), block(kPts, 4);
    const size_t lds = points_lds(m1 + m2);
    hipStream_t s = (hipStream_t)stream;
    const float2* sp = reinterpret_cast<const float2*>(spec);
    const float2* x = reinterpret_cast<const float2*>(xi);
    if (dxi)
        FFNO_LAUNCH(axis_points_kernel<true>, grid, block, lds, s, sp, x, w, out, reinterpret_cast<float2*>(dxi), C, N, m1, m2,
                    accumulate ? 1 : 0);
    else
        FFNO_LAUNCH(axis_points_kernel<false>, grid, block, lds, s, sp, x, w, out, reinterpret_cast<float2*>(dxi), C, N, m1, m2,
                    0);
    return ffno::nudft::status();
}

extern "C" int ffno_axis_modes_to_grid(const float* spec, float* grid, int B, int C, int S, int m1, int m2, int c2r,
                                       void* stream) {
    using namespace ffno::nudft_axis;
    const int rc = grid_args(spec, grid, B, C, S, m1, m2);
    if (rc != FFNO_OK) return rc;
    const dim3 g((unsigned)((S + kRows - 1) / kRows), (unsigned)B);
    const size_t lds = sizeof(float2) * S + sizeof(float) * ((size_t)S + kRows) * C;
    FFNO_LAUNCH(axis_to_grid_kernel, g, dim3(256), lds, (hipStream_t)stream, reinterpret_cast<const float2*>(spec), grid, C, S, m1,
                m2, c2r ? 1 : 0);
    return ffno::nudft::status();
}

extern "C" int ffno_grid_to_axis_modes(const float* grid, float* spec, int B, int C, int S, int m1, int m2, int c2r,
                                       void* stream) {
    using namespace ffno::nudft_axis;
    const int rc = grid_args(grid, spec, B, C, S, m1, m2);
    if (rc != FFNO_OK) return rc;
    const dim3 g((unsigned)((C + kLine - 1) / kLine), (unsigned)B, 2u);
    const size_t lds = sizeof(float2) * S + sizeof(float) * (size_t)S * kLine;
    FFNO_LAUNCH(grid_to_axis_kernel, g, dim3(256), lds, (hipStream_t)stream, grid, reinterpret_cast<float2*>(spec), C, S, m1, m2,
                c2r ? 1 : 0);
    return ffno::nudft::status();
}
