// Output head of the point-cloud F-FNO (reference fourierflow/modules/factorized_fno/point_cloud_2d.py:263-270) on the
// channel-major point features t[B][W][N] that ffno_nudft_points writes:
//     s[b, n, c] = t[b][c][n] + bs_w[c][0] x[b, n, 0] + bs_w[c][1] x[b, n, 1] + bs_b[c]       (bs[-1], a Conv1d(2 -> W, 1))
//     y[b, n, :] = fc2(gelu(fc1 s))                                                             (exact erf GELU, hidden 128)
// A workgroup owns 64 points of one sample: the [64][W] tile is transposed on its way into LDS (coalesced along n on the
// global side), fc1 runs on v_mfma_f32_32x32x2_f32, fc2 (128 -> out_channels, 1 in every shipped config) on the vector ALUs.
// Backward: a fixed number of workgroups walk the tiles; each produces dt for its tiles (again channel-major, no transposed
// copy in memory) and keeps its share of the six parameter gradients -- fc1's as MFMA accumulators -- which one reduction then
// sums in a fixed order: deterministic, no atomics.
#pragma once

#include "ffno_device.h"
#include "ffno.h"

namespace ffno {
namespace pchead {

static constexpr int kPts = 64, kHid = 128, kLH = kHid + 1;
static constexpr int kMaxSplit = 128;

typedef ffno_pchead_params Params;

__device__ __forceinline__ float gelu(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f)); }
__device__ __forceinline__ float dgelu(float v) {
    return 0.5f * (1.f + erff(v * 0.70710678118654752440f)) + v * 0.39894228040143267794f * expf(-0.5f * v * v);
}

// S[q][c] = s of point n0 + q (zero rows past N)
template <int W>
__device__ __forceinline__ void stage_points(const Params& p, const float* __restrict__ t, const float2* __restrict__ x, float* S,
                                             long b, int n0, int N) {
    for (int e = threadIdx.x; e < W * kPts; e += 256) {
        const int c = e / kPts, q = e - c * kPts, n = n0 + q;
        float v = 0.f;
        if (n < N) {
            const float2 xv = x[b * N + n];
            v = t[(b * W + c) * N + n] + (fmaf(p.bs_w[2 * c], xv.x, p.bs_w[2 * c + 1] * xv.y) + p.bs_b[c]);
        }
        S[q * (W + 1) + c] = v;
    }
}

template <int W>
__global__ __launch_bounds__(256) void pchead_fwd_kernel(Params p, const float* __restrict__ t, const float2* __restrict__ x,
                                                         float* __restrict__ y, float* __restrict__ pre, int N, int O) {
    FFNO_DYN_SMEM(smem);
    float* S = reinterpret_cast<float*>(smem);       // [64][W + 1]
    float* Wt = S + kPts * (W + 1);                  // [W][129]: fc1 transposed
    float* Hs = Wt + W * kLH;                        // [64][129]
    const int tid = threadIdx.x;
    const long b = blockIdx.y;
    const int n0 = blockIdx.x * kPts;
    stage_points<W>(p, t, x, S, b, n0, N);
    for (int e = tid; e < kHid * W; e += 256) {
        const int hid = e / W, c = e - hid * W;
        Wt[c * kLH + hid] = p.fc1_w[e];
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6, wr = wave & 1, wc = wave >> 1, j = lane & 31, half = lane >> 5;
    f32x16 acc[2] = {zero16(), zero16()};
    FFNO_UNROLL
    for (int kk = 0; kk < W; kk += 2) {
        const float a = S[(wr * 32 + j) * (W + 1) + kk + half];
        FFNO_UNROLL
        for (int u = 0; u < 2; ++u) acc[u] = mfma32(a, Wt[(kk + half) * kLH + (wc + 2 * u) * 32 + j], acc[u]);
    }
    FFNO_UNROLL
    for (int u = 0; u < 2; ++u) {
        const int col = (wc + 2 * u) * 32 + j;
        const float b1 = p.fc1_b[col];
        FFNO_UNROLL
        for (int r = 0; r < 16; ++r) {
            const int row = wr * 32 + drow(r, half);
            const float v = acc[u][r] + b1;
            if (pre && n0 + row < N) pre[(b * N + n0 + row) * kHid + col] = v;
            Hs[row * kLH + col] = gelu(v);
        }
    }
    __syncthreads();
    for (int e = tid; e < kPts * O; e += 256) {
        const int q = e / O, o = e - q * O;
        if (n0 + q >= N) continue;
        float s = p.fc2_b[o];
        for (int k = 0; k < kHid; ++k) s = fmaf(Hs[q * kLH + k], p.fc2_w[o * kHid + k], s);
        y[(b * N + n0 + q) * O + o] = s;
    }
}

__host__ __device__ static inline long part_floats(int W, int O) { return (long)kHid * W + kHid + (long)O * kHid + O + 3 * W; }

// partial[blockIdx.x] = { dfc1_w [128][W], dfc1_b [128], dfc2_w [O][128], dfc2_b [O], dbs_w [W][2], dbs_b [W] } over this workgroup's tiles
template <int W>
__global__ __launch_bounds__(256) void pchead_bwd_kernel(Params p, const float* __restrict__ t, const float2* __restrict__ x,
                                                         const float* __restrict__ dy, const float* __restrict__ pre,
                                                         float* __restrict__ dt, float* __restrict__ partial, int N, int O,
                                                         int tiles_n, int ntiles) {
    FFNO_DYN_SMEM(smem);
    constexpr int LS = W + 1, NC = W / 32;
    float* S = reinterpret_cast<float*>(smem);       // [64][W + 1]: s, then ds
    float* W1 = S + kPts * LS;                       // [128][W + 1]: fc1 as stored
    float* Hs = W1 + kHid * LS;                      // [64][129]: dpre
    float* Gs = Hs + kPts * kLH;                     // [64][129]: gelu(pre)
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6, wr = wave & 1, wc = wave >> 1, j = lane & 31, half = lane >> 5;
    float* part = partial + (long)blockIdx.x * part_floats(W, O);
    float* part_fc2 = part + (long)kHid * W + kHid;
    for (int e = tid; e < kHid * W; e += 256) W1[(e / W) * LS + e % W] = p.fc1_w[e];
    for (int e = tid; e < O * kHid + O; e += 256) part_fc2[e] = 0.f;       // (each element is only ever touched by thread e % 256)
    f32x16 accw[NC];
    FFNO_UNROLL
    for (int u = 0; u < NC; ++u) accw[u] = zero16();
    float db1 = 0.f, dbw0 = 0.f, dbw1 = 0.f, dbb = 0.f;
    for (int it = blockIdx.x; it < ntiles; it += gridDim.x) {
        const long b = it / tiles_n;
        const int n0 = (it - (int)b * tiles_n) * kPts;
        __syncthreads();   // the previous tile is consumed (first pass: W1 and the zeroed slice are written)
        stage_points<W>(p, t, x, S, b, n0, N);
        for (int e = tid; e < kPts * kHid; e += 256) {
            const int q = e / kHid, k = e - q * kHid, n = n0 + q;
            float v = 0.f, gl = 0.f;
            if (n < N) {
                const float pv = pre[(b * N + n) * kHid + k];
                const float* g = dy + (b * N + n) * O;
                float dh = 0.f;
                for (int o = 0; o < O; ++o) dh = fmaf(g[o], p.fc2_w[o * kHid + k], dh);
                v = dh * dgelu(pv);
                gl = gelu(pv);
            }
            Hs[q * kLH + k] = v;
            Gs[q * kLH + k] = gl;
        }
        __syncthreads();
        // fc2's gradients (VALU, in this workgroup's slice), fc1's bias
        for (int e = tid; e < O * kHid + O; e += 256) {
            float s = 0.f;
            if (e < O * kHid) {
                const int o = e / kHid, k = e - o * kHid;
                for (int q = 0; q < kPts && n0 + q < N; ++q) s = fmaf(dy[(b * N + n0 + q) * O + o], Gs[q * kLH + k], s);
            } else {
                const int o = e - O * kHid;
                for (int q = 0; q < kPts && n0 + q < N; ++q) s += dy[(b * N + n0 + q) * O + o];
            }
            part_fc2[e] += s;
        }
        if (tid < kHid)
            for (int q = 0; q < kPts; ++q) db1 += Hs[q * kLH + tid];
        // ds = dpre fc1 (rows 32 wr, column tile wc) and dfc1 += dpre^T s (row tile = wave, every column tile)
        f32x16 accd = zero16();
        if (wc < NC) {
            FFNO_UNROLL
            for (int kk = 0; kk < kHid; kk += 2)
                accd = mfma32(Hs[(wr * 32 + j) * kLH + kk + half], W1[(kk + half) * LS + wc * 32 + j], accd);
        }
        FFNO_UNROLL
        for (int kk = 0; kk < kPts; kk += 2) {
            const float a = Hs[(kk + half) * kLH + wave * 32 + j];
            FFNO_UNROLL
            for (int u = 0; u < NC; ++u) accw[u] = mfma32(a, S[(kk + half) * LS + u * 32 + j], accw[u]);
        }
        __syncthreads();   // s is consumed: the tile buffer takes ds
        if (wc < NC) {
            FFNO_UNROLL
            for (int r = 0; r < 16; ++r) S[(wr * 32 + drow(r, half)) * LS + wc * 32 + j] = accd[r];
        }
        __syncthreads();
        for (int e = tid; e < W * kPts; e += 256) {
            const int c = e / kPts, q = e - c * kPts;
            if (n0 + q < N) dt[(b * W + c) * N + n0 + q] = S[q * LS + c];
        }
        if (tid < W) {
            for (int q = 0; q < kPts && n0 + q < N; ++q) {
                const float2 xv = x[b * N + n0 + q];
                const float d = S[q * LS + tid];
                dbw0 = fmaf(d, xv.x, dbw0), dbw1 = fmaf(d, xv.y, dbw1), dbb += d;
            }
        }
    }
    FFNO_UNROLL
    for (int u = 0; u < NC; ++u) {
        FFNO_UNROLL
        for (int r = 0; r < 16; ++r) part[(long)(wave * 32 + drow(r, half)) * W + u * 32 + j] = accw[u][r];
    }
    if (tid < kHid) part[(long)kHid * W + tid] = db1;
    if (tid < W) {
        float* pb = part_fc2 + O * kHid + O;
        pb[2 * tid] = dbw0, pb[2 * tid + 1] = dbw1, pb[2 * W + tid] = dbb;
    }
}

__global__ __launch_bounds__(256) void pchead_reduce_kernel(Params g, const float* __restrict__ partial, int W, int O, int nsplit) {
    const long n1 = (long)kHid * W, n2 = n1 + kHid, n3 = n2 + (long)O * kHid, n4 = n3 + O, n5 = n4 + 2 * W, n6 = n5 + W;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n6) return;
    float s = 0.f;
    for (int sp = 0; sp < nsplit; ++sp) s += partial[(long)sp * n6 + e];
    if (e < n1) g.fc1_w[e] = s;
    else if (e < n2) g.fc1_b[e - n1] = s;
    else if (e < n3) g.fc2_w[e - n2] = s;
    else if (e < n4) g.fc2_b[e - n3] = s;
    else if (e < n5) g.bs_w[e - n4] = s;
    else g.bs_b[e - n5] = s;
}

static inline bool params_ok(const Params* p) {
    return p && p->bs_w && p->bs_b && p->fc1_w && p->fc1_b && p->fc2_w && p->fc2_b;
}
static inline int nsplit_of(int B, int N) {
    const long tiles = (long)B * ((N + kPts - 1) / kPts);
    return (int)(tiles < kMaxSplit ? tiles : kMaxSplit);
}
static inline int status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? FFNO_OK : (int)e;
}

template <int W>
static int launch_fwd(const Params& p, const float* t, const float* x, float* y, float* pre, int B, int N, int O, hipStream_t st) {
    const size_t lds = sizeof(float) * ((size_t)kPts * (W + 1) + (size_t)W * kLH + (size_t)kPts * kLH);
    const int e = allow_dynamic_lds(pchead_fwd_kernel<W>, lds);
    if (e) return e;
    FFNO_LAUNCH(pchead_fwd_kernel<W>, dim3((unsigned)((N + kPts - 1) / kPts), (unsigned)B), dim3(256), lds, st, p, t,
                reinterpret_cast<const float2*>(x), y, pre, N, O);
    return status();
}
template <int W>
static int launch_bwd(const Params& p, const float* t, const float* x, const float* dy, const float* pre, float* dt, float* partial,
                      int B, int N, int O, hipStream_t st) {
    const size_t lds = sizeof(float) * ((size_t)(kPts + kHid) * (W + 1) + 2 * (size_t)kPts * kLH);
    const int e = allow_dynamic_lds(pchead_bwd_kernel<W>, lds);
    if (e) return e;
    const int tiles_n = (N + kPts - 1) / kPts;
    FFNO_LAUNCH(pchead_bwd_kernel<W>, dim3((unsigned)nsplit_of(B, N)), dim3(256), lds, st, p, t, reinterpret_cast<const float2*>(x),
                dy, pre, dt, partial, N, O, tiles_n, B * tiles_n);
    return status();
}

}  // namespace pchead
}  // namespace ffno

extern "C" int ffno_pchead_supported(int W, int hidden, int out_channels) {
    return (W == 32 || W == 64) && hidden == ffno::pchead::kHid && out_channels >= 1 && out_channels <= 64;
}

extern "C" size_t ffno_pchead_partial_floats(int B, int N, int W, int out_channels) {
    using namespace ffno::pchead;
    if (B <= 0 || N <= 0 || !ffno_pchead_supported(W, kHid, out_channels)) return 0;
    return (size_t)nsplit_of(B, N) * (size_t)part_floats(W, out_channels);
}

extern "C" int ffno_pchead_fwd(const ffno_pchead_params* params, const float* t, const float* x, float* y, float* pre, int B, int N,
                               int W, int out_channels, void* stream) {
    using namespace ffno::pchead;
    if (!params_ok(params) || !t || !x || !y || B <= 0 || N <= 0) return FFNO_EINVAL;
    if (!ffno_pchead_supported(W, kHid, out_channels) || B > 65535 || (long)B * N * kHid >= (1L << 31)) return FFNO_EUNSUPPORTED;
    return W == 32 ? launch_fwd<32>(*params, t, x, y, pre, B, N, out_channels, (hipStream_t)stream)
                   : launch_fwd<64>(*params, t, x, y, pre, B, N, out_channels, (hipStream_t)stream);
}

extern "C" int ffno_pchead_bwd(const ffno_pchead_params* params, const ffno_pchead_params* grads, const float* t, const float* x,
                               const float* dy, const float* pre, float* dt, float* partial, int B, int N, int W, int out_channels,
                               void* stream) {
    using namespace ffno::pchead;
    if (!params_ok(params) || !params_ok(grads) || !t || !x || !dy || !pre || !dt || !partial || B <= 0 || N <= 0) return FFNO_EINVAL;
    if (!ffno_pchead_supported(W, kHid, out_channels) || (long)B * N * kHid >= (1L << 31)) return FFNO_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    int rc = W == 32 ? launch_bwd<32>(*params, t, x, dy, pre, dt, partial, B, N, out_channels, st)
                     : launch_bwd<64>(*params, t, x, dy, pre, dt, partial, B, N, out_channels, st);
    if (rc) return rc;
    const long total = part_floats(W, out_channels);
    FFNO_LAUNCH(pchead_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, *grads, partial, W, out_channels,
                nsplit_of(B, N));
    return status();
}
